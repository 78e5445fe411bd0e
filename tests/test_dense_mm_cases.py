"""CPU side of tests/test_gpu_dense_mul_mat.py: the case list itself. Every case is a legal ggml mat-mul, every kernel of the dense path has
cases, the exact inputs are exact in any order, and the bound on the random inputs is one a plain float32 evaluation keeps."""
import numpy as np
import pytest

import dense_mm_cases as dm
import ops_ref as ref
from dense_mm_cases import BF16, F16, F32


def test_cases_are_legal_and_distinct():
    ids = [dm.case_id(c) for c in dm.CASES]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:5]
    for c in dm.CASES:
        assert dm.shape_ok(c), dm.case_id(c)
        assert c.k <= 1057, "the exact-input argument is made for k <= 1057"
    ids = [dm.id_case_id(c) for c in dm.ID_CASES]
    assert len(set(ids)) == len(ids)
    for c in dm.ID_CASES:
        assert 1 <= c.n_used <= c.n_mats and c.m >= 1 and c.k >= 1 and c.n >= 1, dm.id_case_id(c)


def test_reference_grid_is_complete():
    """the counts of tests/test-backend-ops.cpp:5716-5763 (3 x 2 type pairs x (2 k x 27 + 3)) and :5791-5813 (8 + 2 x 4 x 2 x 2 x 2 x 3 x 2)"""
    assert sum(c.tag == "ref" for c in dm.CASES) == 3 * 2 * (2 * 27 + 3)
    assert sum(c.tag == "attn" for c in dm.CASES) == 8 + 384
    assert {c.k for c in dm.CASES if c.tag == "attn"} >= {129, 193, 67, 1057} and {c.m for c in dm.CASES if c.tag == "attn"} >= {83, 1057}


def test_every_path_has_cases_and_written_paths_agree():
    count = dict.fromkeys(dm.PATHS, 0)
    generic_pairs = set()
    for c in dm.CASES:
        p = dm.expected_path(c)
        assert c.want is None or c.want == p, (dm.case_id(c), c.want, p)
        count[p] += 1
        if p == "generic":
            generic_pairs.add((c.ta, c.tb))
    assert all(v >= 3 for v in count.values()), count
    assert generic_pairs == {(ta, tb) for ta in (F32, F16, BF16) for tb in (F32, F16)}
    rows = [c for c in dm.CASES if dm.expected_path(c) == "f32_rows"]
    assert sum(c.m >= 32 for c in rows) >= 3 and sum(c.m < 32 for c in rows) >= 3       # the two row kernels share a counter: the shape tells them apart


def _shuffled_f32_sums(A, B, rng):
    """sum_k a*b accumulated in float32, one element after the other, in a random order of k -> [.., n, m] float32"""
    perm = rng.permutation(A.shape[-1])
    A = A[..., perm].astype(np.float32); B = B[..., perm].astype(np.float32)
    r3, r2 = B.shape[0] // A.shape[0], B.shape[1] // A.shape[1]
    out = np.empty(B.shape[:3] + (A.shape[2],), np.float32)
    for i3 in range(B.shape[0]):
        for i2 in range(B.shape[1]):
            a, b = A[i3 // r3, i2 // r2], B[i3, i2]
            step = max(64, (1 << 22) // (a.shape[0] * a.shape[1]))       # (blocks of columns: bounded memory)
            for n0 in range(0, b.shape[0], step):
                prod = b[n0:n0 + step, None, :] * a[None, :, :]
                out[i3, i2, n0:n0 + step] = np.cumsum(prod, axis=-1, dtype=np.float32)[..., -1]
    return out


@pytest.mark.parametrize("chunk", range(8))
def test_exact_inputs_are_exact_in_any_order(chunk):
    rng = np.random.default_rng(chunk)
    for c in dm.CASES[chunk::8]:
        a_s, b_s = dm.inputs(c, "exact")
        A, B = dm.dec(c.ta, a_s), dm.dec(c.tb, b_s)
        assert (A != 0).all() and (B != 0).all() and np.array_equal(A * 8, np.round(A * 8)) and np.abs(A).max() <= 2 and np.abs(B).max() <= 2
        exp, _ = dm.expected(c, a_s, b_s)
        got = _shuffled_f32_sums(A, B, rng)
        dm.assert_exact(got, exp, dm.case_id(c))
        # the F16 rounding of src1 changes nothing either
        assert np.array_equal(ref.round_f16(B.astype(np.float32)).astype(np.float64), B)


def test_exact_id_inputs_are_exact():
    for c in dm.ID_CASES:
        a_s, b_s, ids = dm.id_inputs(c, "exact")
        exp, _ = dm.id_expected(c, a_s, b_s, ids)
        assert np.array_equal(exp.astype(np.float32).astype(np.float64), exp) and np.array_equal(exp * 64, np.round(exp * 64))
        assert (dm.dec(c.ta, a_s) != 0).all() and (b_s != 0).all()


def _round_src1(ta, tb, B):
    if (ta, tb) == (F16, F32):
        return ref.round_f16(B.astype(np.float32)).astype(np.float32)
    if (ta, tb) == (BF16, F32):
        return ref.bf16_to_f32(ref.round_bf16(B.astype(np.float32)))
    return B.astype(np.float32)


@pytest.mark.parametrize("chunk", range(4))
def test_random_bound_is_tenable(chunk):
    """ggml-cpu's evaluation (src1 rounded to the vec_dot_type, float32 dot products) stays inside the bound for every case"""
    worst = 0.0
    for c in dm.CASES[chunk::4]:
        a_s, b_s = dm.inputs(c, "random")
        exp, mag = dm.expected(c, a_s, b_s)
        A = dm.dec(c.ta, a_s).astype(np.float32); B = _round_src1(c.ta, c.tb, dm.dec(c.tb, b_s))
        r3, r2 = B.shape[0] // A.shape[0], B.shape[1] // A.shape[1]
        got = np.stack([np.stack([B[i3, i2] @ A[i3 // r3, i2 // r2].T for i2 in range(B.shape[1])]) for i3 in range(B.shape[0])])
        bound = dm.random_bound(c.ta, c.tb, c.k, mag)
        dm.assert_random(got, exp, bound, dm.case_id(c))
        worst = max(worst, float((np.abs(got - exp) / bound).max()))
        Bv = np.abs(dm.dec(c.tb, b_s))
        assert Bv.min() >= 2.0 ** -6 * (1 - 2.0 ** -8) and Bv.max() <= 2.0 and np.abs(A).max() <= 1.0
    assert worst <= 1.0
    for c in dm.ID_CASES[chunk::4]:
        a_s, b_s, ids = dm.id_inputs(c, "random")
        exp, mag = dm.id_expected(c, a_s, b_s, ids)
        A = dm.dec(c.ta, a_s)[0].astype(np.float32); B = _round_src1(c.ta, F32, b_s)[0]
        got = np.stack([np.stack([A[ids[t, u]] @ B[t, u % B.shape[1]] for u in range(c.n_used)]) for t in range(c.n)])
        dm.assert_random(got, exp, dm.random_bound(c.ta, F32, c.k, mag), dm.id_case_id(c))


def test_bound_rejects_a_dropped_element():
    """one k element of 4096 dropped (1.1 of an expected size around 10: NMSE 1e-2 per element at worst, 1e-5 typically) is outside the bound;
    mis-rounded operands are the exact and the conversion sets' business"""
    rng = np.random.default_rng(5)
    k = 4096
    a = ref.round_f16(rng.uniform(-1, 1, size=k)).astype(np.float64); b = dm._draw_b(rng, k).astype(np.float32).astype(np.float64)
    a[-1], b[-1] = 0.75, 1.5
    exp, mag = a @ b, np.abs(a) @ np.abs(b)
    assert abs(a[:-1] @ b[:-1] - exp) > dm.random_bound(F16, F32, k, mag)


@pytest.mark.parametrize("c", dm.CONV_CASES, ids=dm.conv_id)
def test_conversion_inputs(c):
    ta, tb, side, _ = c
    a, b, want = dm.conv_inputs(c)
    cc = dm.conv_case(c)
    exp, _ = dm.expected(cc, a, b)
    assert np.isfinite(exp).all()
    dm.assert_conversion(exp.astype(np.float32), want, dm.conv_id(c))       # every hard value is a float32, and the float64 sum is that value
    vt = dm.conv_value_type(c)
    assert set(dm.f32_bits(want).reshape(-1).tolist()) == set(dm.f32_bits(dm.dec(vt, dm.from_bits(vt, dm.HARD_BITS[vt])).astype(np.float32)).tolist())
    if side == "b" and (ta, tb) == (F16, F32):      # through the F16 rounding unchanged, subnormals included
        assert np.array_equal(dm.f32_bits(ref.round_f16(b).astype(np.float32)), dm.f32_bits(b))
