"""Cases, inputs, expected results and the expected kernel of every dense (F16 / BF16 / F32 src0) MUL_MAT and MUL_MAT_ID case, shared by
tests/test_gpu_dense_mul_mat.py (the kernels, on the GPU) and tests/test_dense_mm_cases.py (the list itself, on the CPU). No GPU and no
native library is touched here.

Arrays are in numpy order [ne3, ne2, ne1, ne0]; `ne` / `nb` tuples are in ggml order. Types are the ggml_type numbers.

Three input sets, all compared with oracle/ops_ref.mul_mat_dense (float64):
  exact       every element a non-zero multiple of 1/8 in [-2, 2]: exact in F32, F16 and BF16; a product is a multiple of 2^-6 of magnitude
              <= 4, a partial sum over k <= 1057 a multiple of 2^-6 below 2^13, 19 bits: exact in float32 in ANY summation order, with or
              without FMA, with or without the F16 rounding of src1, on the matrix cores or not. The comparison is bit equality. No
              element is 0, so a dropped, doubled or misplaced element changes the sum it belongs to (by a non-zero multiple of 2^-6).
  random      a uniform in [-1, 1], |b| in [2^-6, 2] (log-uniform, random sign), each stored in its type; every output element within
              ((k + 2) 2^-24 + r) sum_i |a_i| |b_i| of the float64 result, r the unit roundoff of the format ggml-cpu's vec_dot_type rounds
              src1 to: 2^-11 for F16 x F32, 2^-8 for BF16 x F32, 0 otherwise (the kernels round to F16 in the first case and not at all in
              the second: both are inside).
  conversion  one operand the identity, the other the type's hard values (CONV_CASES): the result is those values, bit for bit."""
from collections import namedtuple

import numpy as np

import ops_ref as ref

F32, F16, BF16 = 0, 1, 30
TNAME = {F32: "f32", F16: "f16", BF16: "bf16"}
ESIZE = {F32: 4, F16: 2, BF16: 2}
PATHS = ("mfma", "f16_pairs", "f32_vec", "f32_rows", "generic")      # + "id" for MUL_MAT_ID; the counter of path p is "dense_" + p
MMVQ_MAX_N = 8                                                       # more columns than this: the matrix-core kernel may take F16 x F32
GRID_YZ = 65535                                                      # the last index of grid dims y and z
JUNK = 7.0                                                           # what lies around a view's elements in its parent: not a value of any input set

# a layout: ("cont",) | ("perm", (p0, p1, p2, p3)) as ggml_permute | ("view", pad, off): rows of ne0 + pad elements in the parent, the view
# starts `off` elements in (ggml_view_4d) | ("transpose",): ggml_transpose of a [ne1, ne0, ne2, ne3] tensor
CONT = ("cont",)
Case = namedtuple("Case", "tag ta tb m n k bs nr lay_a lay_b want")           # want: the path the case was written for, or None = whatever the predicate says
IdCase = namedtuple("IdCase", "tag ta m k n_mats n_used bcast_b n lay_a")


# ---- layout ----------------------------------------------------------------------------------------------------------------------
def _contig_nb(t, ne):
    nb = [ESIZE[t]]
    for i in range(1, 4):
        nb.append(nb[-1] * ne[i - 1])
    return tuple(nb)


def operand(t, ne, lay):
    """-> dict(t, parent_ne, ne, nb, off): the view a kernel is handed (ne, nb in bytes, off = byte offset into the parent) and its parent"""
    if lay[0] == "cont":
        pne, nb, off = tuple(ne), _contig_nb(t, ne), 0
    elif lay[0] == "perm":
        per = lay[1]
        pne = tuple(ne[per[i]] for i in range(4))
        pnb = _contig_nb(t, pne)
        nb = [0] * 4
        for i in range(4):
            nb[per[i]] = pnb[i]
        nb, off = tuple(nb), 0
    elif lay[0] == "view":
        _, pad, o = lay
        assert 0 <= o <= pad
        pne = (ne[0] + pad,) + tuple(ne[1:])
        nb, off = _contig_nb(t, pne), o * ESIZE[t]
    elif lay[0] == "transpose":
        pne = (ne[1], ne[0], ne[2], ne[3])
        pnb = _contig_nb(t, pne)
        nb, off = (pnb[1], pnb[0], pnb[2], pnb[3]), 0
    else:
        raise ValueError(lay)
    return dict(t=t, parent_ne=pne, ne=tuple(ne), nb=nb, off=off)


def ne_a(c):
    return (c.k, c.m, c.bs[0], c.bs[1])


def ne_b(c):
    return (c.k, c.n, c.bs[0] * c.nr[0], c.bs[1] * c.nr[1])


def operands(c):
    return operand(c.ta, ne_a(c), c.lay_a), operand(c.tb, ne_b(c), c.lay_b)


def embed(op, data):
    """data [ne3, ne2, ne1, ne0] (storage of op's type) -> the parent's storage array with the view's elements set and JUNK elsewhere"""
    par = np.empty(op["parent_ne"][::-1], dtype=data.dtype)
    par[...] = enc(op["t"], np.float32(JUNK))
    v = np.ndarray(shape=op["ne"][::-1], dtype=data.dtype, buffer=par.reshape(-1).data, offset=op["off"], strides=op["nb"][::-1])
    v[...] = data
    return par


# ---- storage ---------------------------------------------------------------------------------------------------------------------
def enc(t, x):
    x = np.asarray(x, dtype=np.float32)
    return x if t == F32 else ref.round_f16(x) if t == F16 else ref.round_bf16(x)


def dec(t, s):
    return (ref.bf16_to_f32(s) if t == BF16 else np.asarray(s)).astype(np.float64)


def from_bits(t, bits):
    bits = np.asarray(bits)
    return bits.astype(np.uint32).view(np.float32) if t == F32 else bits.astype(np.uint16).view(np.float16) if t == F16 else bits.astype(np.uint16)


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- the dispatch predicate, restated (mm_dense.hip mul_mat_dense_path; parents are 16-byte aligned, the scratch is as large as the graph asks) ----
def expected_path(c):
    a, b = operands(c)
    k, m, n = c.k, c.m, c.n
    nz = b["ne"][2] * b["ne"][3]
    rows_k = a["nb"][0] == ESIZE[c.ta] and b["nb"][0] == ESIZE[c.tb]
    if c.ta == F16 and c.tb == F32 and rows_k:
        if n > MMVQ_MAX_N and k % 32 == 0 and nz <= GRID_YZ and m <= GRID_YZ * 128 and n <= GRID_YZ:
            return "mfma"
        if k % 2 == 0:
            return "f16_pairs"
    if c.ta == F32 and c.tb == F32 and rows_k and k % 4 == 0 and k < 2 ** 30 and a["off"] % 16 == 0 and b["off"] % 16 == 0 \
            and all(s % 16 == 0 for s in a["nb"][1:] + b["nb"][1:]):
        return "f32_rows" if n >= 64 and m >= 8 else "f32_vec"
    return "generic"


def shape_ok(c):
    """ggml_can_mul_mat (ggml.c): same k, src1's batch dims multiples of src0's; the views stay inside their parents"""
    a, b = operands(c)
    ok = a["ne"][0] == b["ne"][0] and b["ne"][2] % a["ne"][2] == 0 and b["ne"][3] % a["ne"][3] == 0 and min(a["ne"] + b["ne"]) >= 1
    for o in (a, b):
        last = o["off"] + sum((o["ne"][i] - 1) * o["nb"][i] for i in range(4)) + ESIZE[o["t"]]
        ok = ok and last <= int(np.prod(o["parent_ne"])) * ESIZE[o["t"]] and o["off"] % ESIZE[o["t"]] == 0
    return ok


# ---- the reference's grid (tests/test-backend-ops.cpp:5716-5763 and :5791-5813), as data ----------------------------------------
_BS_NR = [((1, 1), (1, 1)), ((1, 1), (2, 1)), ((1, 1), (1, 2)), ((3, 1), (1, 1)), ((3, 1), (2, 1)),
          ((3, 2), (1, 1)), ((3, 2), (2, 1)), ((3, 2), (1, 2)), ((3, 2), (2, 2))]
_PERMS = [(0, 2, 1, 3), (0, 1, 3, 2), (0, 3, 2, 1)]


def _mk(tag, ta, tb, m, n, k, bs=(1, 1), nr=(1, 1), per=None, v=False, lay_a=None, lay_b=None, want=None):
    if per is not None and per != (0, 1, 2, 3):
        la = lb = ("perm", per)
    elif v:
        la = lb = ("view", k, 0)
    else:
        la = lb = CONT
    return Case(tag, ta, tb, m, n, k, tuple(bs), tuple(nr), lay_a or la, lay_b or lb, want)


def _reference_grid():
    out = []
    for ta in (F32, F16, BF16):
        for tb in (F32, F16):
            for k in (256, 4):
                for n in (1, 16):
                    out += [_mk("ref", ta, tb, 16, n, k, bs, nr) for bs, nr in _BS_NR]
                for n in (1, 8, 16):
                    out += [_mk("ref", ta, tb, 16, n, k, (2, 3), (1, 1), per) for per in _PERMS]
            out += [_mk("ref", ta, tb, 16, n, 1024, (3, 2)) for n in (1, 8, 16)]
    # the attention shapes: F16 cache x F32, GQA broadcast 4
    for m, n, k, bs, nr, per in [(64, 2, 128, (8, 1), (1, 1), None), (83, 2, 128, (8, 1), (4, 1), None), (64, 2, 64, (8, 1), (4, 1), None),
                                 (83, 2, 64, (8, 1), (4, 1), None), (64, 45, 128, (8, 1), (4, 1), None), (128, 45, 64, (8, 1), (4, 1), None),
                                 (1056, 1, 193, (1, 1), (4, 1), (0, 2, 1, 3)), (1056, 1, 67, (1, 1), (4, 1), (0, 2, 1, 3))]:
        out.append(_mk("attn", F16, F32, m, n, k, bs, nr, per))
    for bs2 in (1, 3):
        for bs in (1, 2, 4, 8):
            for nr in (1, 4):
                for dm in (0, 1):
                    for dk in (0, 1):
                        for t in (F16, BF16, F32):
                            out.append(_mk("attn", t, F32, 1056 + dm, 1, 128 + dk, (bs, bs2), (nr, 1), (0, 2, 1, 3)))
                            out.append(_mk("attn", t, F32, 128 + dm, 1, 1056 + dk, (bs, bs2), (nr, 1), None, True))
    return out


# ---- the project's own edges: one small case per dispatch boundary, each naming the path it was written for ----------------------
def _own_edges():
    o = []
    # the matrix-core kernel: 64-wide k steps (k % 64 == 32 is the tail, k = 32 a single half step), 128 x 128 tiles
    o += [_mk("mfma-k", F16, F32, 16, 16, k, want="mfma") for k in (32, 96, 160)]
    o += [_mk("mfma-m", F16, F32, m, 16, 64, want="mfma") for m in (1, 3, 83, 129)]
    o += [_mk("mfma-n", F16, F32, 16, n, 64, want="mfma") for n in (9, 45, 129, 257)]
    o.append(_mk("mfma-r2", F16, F32, 16, 16, 64, (2, 1), (4, 1), want="mfma"))
    o.append(_mk("mfma-r3", F16, F32, 16, 16, 64, (1, 2), (1, 2), want="mfma"))
    o.append(_mk("mfma-a-rows-unaligned", F16, F32, 19, 16, 96, (2, 1), lay_a=("view", 1, 0), want="mfma"))      # nb01 = 194: the 128-bit row loads start unaligned
    o.append(_mk("mfma-a-offset-2", F16, F32, 19, 16, 96, (2, 1), lay_a=("view", 8, 1), want="mfma"))             # rows 16-byte multiples, the view 2 bytes in
    o.append(_mk("mfma-b-offset-4", F16, F32, 19, 16, 96, (2, 1), lay_b=("view", 1, 1), want="mfma"))             # k_act_to_16's 128-bit loads of b: rows of 388 bytes, the view 4 bytes in
    # F16 pairs
    o += [_mk("pairs-n", F16, F32, 5, n, 64, want="f16_pairs") for n in (1, 8)]
    o.append(_mk("pairs-k34", F16, F32, 5, 16, 34, want="f16_pairs"))          # n > 8 but k % 32 != 0: the matrix-core kernel refuses
    o.append(_mk("pairs-k33", F16, F32, 5, 16, 33, want="generic"))            # odd k: no pairs either
    o.append(_mk("pairs-a-offset-2", F16, F32, 5, 3, 130, (2, 1), lay_a=("view", 8, 1), want="f16_pairs"))      # k = 130: two lanes take a second step
    o.append(_mk("pairs-b-offset-4", F16, F32, 5, 3, 130, (2, 1), lay_b=("view", 1, 1), want="f16_pairs"))      # the 64-bit loads of b: rows of 524 bytes, the view 4 bytes in
    # F32 vectors / rows x4 (m >= 32) / rows x2 (8 <= m < 32)
    for n in (8, 63, 64, 71):
        for m in (7, 8, 31, 32, 33, 37):
            o.append(_mk("f32", F32, F32, m, n, 256, want="f32_rows" if n >= 64 and m >= 8 else "f32_vec"))
    for k in (4, 260):
        o += [_mk("f32-k", F32, F32, m, n, k, want=w) for m, n, w in ((5, 3, "f32_vec"), (37, 71, "f32_rows"), (9, 65, "f32_rows"))]
    o.append(_mk("f32-r2", F32, F32, 33, 65, 8, (2, 1), (2, 2), want="f32_rows"))
    o.append(_mk("f32-k-not-4", F32, F32, 37, 71, 258, want="generic"))
    o.append(_mk("f32-b-offset-4", F32, F32, 37, 71, 256, lay_b=("view", 4, 1), want="generic"))                 # b's rows 16-byte multiples, the view 4 bytes in
    o.append(_mk("f32-a-offset-4", F32, F32, 5, 3, 256, lay_a=("view", 4, 1), want="generic"))
    # generic
    for ta in (F32, F16, BF16):
        for tb in (F32, F16):
            o.append(_mk("generic-bT", ta, tb, 7, 9, 40, (2, 1), (2, 1), lay_b=("transpose",), want="generic"))  # nb10 is a row stride
            o.append(_mk("generic-k1", ta, tb, 7, 9, 1, want="generic"))
            o.append(_mk("generic-k65", ta, tb, 5, 17, 65, (1, 2), (1, 1), want="generic"))                       # a second step for lane 0 only
    o.append(_mk("generic-f16xf16", F16, F16, 33, 17, 256, want="generic"))
    o.append(_mk("generic-bf16xf16", BF16, F16, 33, 17, 256, want="generic"))
    o.append(_mk("generic-bf16xf32", BF16, F32, 33, 17, 256, want="generic"))
    # grid limits: a column per grid row in k_act_to_16 (n > 65535 leaves the matrix-core kernel), batches in grid dim z (more than 65535: several launches)
    o.append(_mk("grid-n65544", F16, F32, 4, 65544, 32, want="f16_pairs"))
    o.append(_mk("grid-z65792", F32, F32, 2, 1, 4, (1, 1), (256, 257), want="f32_vec"))
    o.append(_mk("grid-y65537", F32, F32, 1, 524296, 4, want="f32_vec"))                       # 65537 column tiles of 8: a second launch from y0 = 65535
    return o


CASES = _reference_grid() + _own_edges()


def case_id(c):
    lay = "-".join(f"{w}{'_'.join(map(str, l)).replace('(', '').replace(')', '').replace(', ', '')}" for w, l in (("a", c.lay_a), ("b", c.lay_b)) if l != CONT)
    return f"{c.tag}-{TNAME[c.ta]}x{TNAME[c.tb]}-m{c.m}n{c.n}k{c.k}-bs{c.bs[0]}x{c.bs[1]}-nr{c.nr[0]}x{c.nr[1]}" + ("-" + lay if lay else "")


# ---- MUL_MAT_ID over an unquantized expert stack -----------------------------------------------------------------------------------
ID_ROUTES = [(4, 1, False, 1), (4, 2, True, 1), (8, 4, False, 5), (8, 8, False, 3), (8, 2, True, 40)]      # (n_mats, n_used, bcast_b, n tokens)
ID_CASES = [IdCase("id", ta, m, k, nm, nu, bc, n, CONT) for ta in (F32, F16, BF16) for k in (1, 5, 160) for m in (1, 48) for nm, nu, bc, n in ID_ROUTES]
ID_CASES += [IdCase("id-v", ta, 48, 160, 8, 4, False, 5, ("view", 160, 0)) for ta in (F32, F16, BF16)]      # the stack as the first k of rows of 2k


def id_case_id(c):
    return f"{c.tag}-{TNAME[c.ta]}-m{c.m}k{c.k}-e{c.n_mats}u{c.n_used}{'b' if c.bcast_b else ''}n{c.n}"


def id_operand(c):
    return operand(c.ta, (c.k, c.m, c.n_mats, 1), c.lay_a)


def id_inputs(c, kind):
    """-> (as [1, n_mats, m, k] storage, b [1, n, n_b, k] float32, ids_full [n, n_mats] int32: the first n_used of each row are used)"""
    rng = np.random.default_rng(_seed(c, kind))
    nb = 1 if c.bcast_b else c.n_used
    if kind == "exact":
        a, b = _draw_exact(rng, (1, c.n_mats, c.m, c.k)), _draw_exact(rng, (1, c.n, nb, c.k))
    else:
        a, b = rng.uniform(-1, 1, size=(1, c.n_mats, c.m, c.k)), _draw_b(rng, (1, c.n, nb, c.k))
    ids = np.stack([rng.permutation(c.n_mats) for _ in range(c.n)]).astype(np.int32)
    return enc(c.ta, a), enc(F32, b), ids


def id_expected(c, a_s, b_s, ids):
    """-> (float64 result [n, n_used, m], sum |a||b| of every element)"""
    A, B = dec(c.ta, a_s)[0], dec(F32, b_s)[0]
    nb = B.shape[1]
    exp = np.empty((c.n, c.n_used, c.m)); mag = np.empty_like(exp)
    for t in range(c.n):
        for u in range(c.n_used):
            exp[t, u] = A[ids[t, u]] @ B[t, u % nb]
            mag[t, u] = np.abs(A[ids[t, u]]) @ np.abs(B[t, u % nb])
    return exp, mag


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _seed(c, kind):
    import zlib
    return zlib.crc32((repr(tuple(c)) + kind).encode())


def _draw_exact(rng, shape):
    return rng.integers(1, 17, size=shape) * rng.choice([-1.0, 1.0], size=shape) / 8.0


def _draw_b(rng, shape):
    return np.exp2(rng.uniform(-6, 1, size=shape)) * rng.choice([-1.0, 1.0], size=shape)


def inputs(c, kind):
    """kind 'exact' | 'random' -> (a [ne03, ne02, m, k], b [ne13, ne12, n, k]) as storage of their types"""
    rng = np.random.default_rng(_seed(c, kind))
    sa, sb = ne_a(c)[::-1], ne_b(c)[::-1]
    if kind == "exact":
        return enc(c.ta, _draw_exact(rng, sa)), enc(c.tb, _draw_exact(rng, sb))
    return enc(c.ta, rng.uniform(-1, 1, size=sa)), enc(c.tb, _draw_b(rng, sb))


def expected(c, a_s, b_s):
    """-> (the float64 result [ne13, ne12, n, m], sum_i |a_i||b_i| of every element: the scale of the random-input bound)"""
    A, B = dec(c.ta, a_s), dec(c.tb, b_s)
    return ref.mul_mat_dense(A, B), ref.mul_mat_dense(np.abs(A), np.abs(B))


def src1_roundoff(ta, tb):
    """unit roundoff of the format ggml-cpu rounds src1 to before the dot product (its vec_dot_type)"""
    return 2.0 ** -11 if (ta, tb) == (F16, F32) else 2.0 ** -8 if (ta, tb) == (BF16, F32) else 0.0


def random_bound(ta, tb, k, mag):
    return ((k + 2) * 2.0 ** -24 + src1_roundoff(ta, tb)) * mag


def assert_exact(got, exp64, what=""):
    want = exp64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), exp64), "the expected result is not a float32: the input set is not exact"
    bad = np.argwhere(f32_bits(got) != f32_bits(want))
    assert bad.size == 0, (what, f"{len(bad)} of {want.size} elements differ; first at [i3, i2, i1, i0] = {bad[0].tolist()}: "
                                 f"got {got[tuple(bad[0])]!r}, expected {want[tuple(bad[0])]!r}")


def assert_random(got, exp64, bound, what=""):
    err = np.abs(got.astype(np.float64) - exp64)
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))


# ---- conversion: the identity against a type's hard values, m = k = n = 64 --------------------------------------------------------
HARD_BITS = {      # +-0, the smallest and largest subnormal, the smallest normal, +-max finite, all low mantissa bits set, one low bit set
    F16: [0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x3FFF, 0xBFFF, 0x3C01, 0x8001, 0x83FF, 0x8400],
    BF16: [0x0000, 0x8000, 0x0001, 0x007F, 0x0080, 0x7F7F, 0xFF7F, 0x3FFF, 0xBFFF, 0x3F81, 0x8001, 0x807F, 0x8080],
    F32: [0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3FFFFFFF, 0xBFFFFFFF, 0x3F800001,
          0x80000001, 0x807FFFFF, 0x80800000],
}
CONV_N = 64
CONV_CASES = [(ta, tb, side, CONV_N) for ta in (F32, F16, BF16) for tb in (F32, F16) for side in ("a", "b")]      # side: which operand holds the hard values
# 64 columns take F32 x F32 to the rows kernel and F16 x F32 to the matrix cores: 8 columns reach the F32 vector and the F16 pair kernel
CONV_CASES += [(ta, F32, side, 8) for ta in (F32, F16) for side in ("a", "b")]


def conv_id(c):
    return f"{TNAME[c[0]]}x{TNAME[c[1]]}-hard_{c[2]}-n{c[3]}"


def conv_case(c):
    ta, tb, _, n = c
    return _mk("conv", ta, tb, CONV_N, n, CONV_N)


def conv_value_type(c):
    """the format whose hard values the hard operand holds. `a` holds its own type's. An F32 `b` against F16 or BF16 weights holds the
    weights' format's values (as float32): ggml-cpu rounds src1 to that format, the kernels round to F16 in the first case and not at all in
    the second, and a value of the format passes through either unchanged — F16 subnormals through the F16 rounding included."""
    ta, tb, side, _ = c
    return ta if side == "a" else (ta if tb == F32 else tb)


def conv_inputs(c):
    """-> (a, b) storage, and the float32 [n, m] the result must equal"""
    ta, tb, side, n = c
    vt = conv_value_type(c)
    bits = np.array(HARD_BITS[vt], dtype=np.uint32)
    vals = from_bits(vt, bits[np.arange(CONV_N * CONV_N) % len(bits)]).reshape(CONV_N, CONV_N)
    hard32 = dec(vt, vals).astype(np.float32)                  # (every value of F16 / BF16 is a float32)
    eye = np.eye(CONV_N, dtype=np.float32)
    if side == "a":
        a, b, want = vals, enc(tb, eye[:n]), hard32.T[:n]      # dst[n, m] = a[m, n]
    else:
        a, b, want = enc(ta, eye), enc(tb, hard32[:n]), hard32[:n]     # dst[n, m] = b[n, m]
    return a.reshape(1, 1, CONV_N, CONV_N), b.reshape(1, 1, n, CONV_N), want.reshape(1, 1, n, CONV_N)


def assert_conversion(got, want, what=""):
    """bit for bit, with one exception: where -0 is expected +0 is right too. A sum that starts at +0 and adds -0 (the value itself, or a
    negative value times the identity's 0) is +0 under round-to-nearest, in any order; ggml-cpu returns the same. -0 for an expected +0 fails."""
    g, w = f32_bits(got), f32_bits(want)
    bad = np.argwhere((g != w) & ~((w == 0x80000000) & (g == 0)))
    assert bad.size == 0, (what, f"{len(bad)} elements differ; first at {bad[0].tolist()}: got {int(g[tuple(bad[0])]):#010x}, expected {int(w[tuple(bad[0])]):#010x}")
