"""CPU side of tests/test_gpu_elem_ops.py: the rounding helpers of oracle/ops_ref.py against torch, bit for bit, and — for the inputs of
every half-precision case of the GPU suite — that the suite's tolerance is tenable: a float32 evaluation of the definition, rounded to
the output type, stays within 1 ulp of the float64 result rounded once, and under the cap on how many elements may differ."""
import numpy as np
import pytest
import torch

import elem_cases as ec
import ops_ref as ref
from elem_cases import F32


def _patterns():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 2 ** 32, size=10 ** 6, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.concatenate([ec.conversion_specials(), x])


def test_round_bf16_matches_torch():
    x = _patterns()
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = ref.round_bf16(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.isnan(ref.bf16_to_f32(got[nan])).all() and ((got[nan] & 64) == 64).all()       # NaN stays NaN, quiet bit set
    fin = np.isfinite(x)
    assert np.array_equal(ref.round_bf16_from_f64(x[fin].astype(np.float64)), got[fin])      # the float64 entry agrees on float32 values


def test_round_bf16_from_f64_rounds_once():
    """just above / below a bf16 tie by less than a float32 ulp: through float32 these would land ON the tie and go to even"""
    x = np.array([1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -8 - 2.0 ** -30, 1 + 3 * 2.0 ** -8 - 2.0 ** -30, 1 + 3 * 2.0 ** -8 + 2.0 ** -30])
    assert ref.round_bf16_from_f64(x).tolist() == [0x3F81, 0x3F80, 0x3F81, 0x3F82]


def test_round_f16_matches_torch():
    x = _patterns()
    want = torch.from_numpy(x.copy()).to(torch.float16).numpy()
    got = ref.round_f16(x)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan].view(np.uint16), want[~nan].view(np.uint16))
    assert np.isnan(got[nan]).all()


def test_reference_tables_agree_with_torch_float64():
    """the float64 definitions against torch's, where torch has the function"""
    x = np.linspace(-10, 10, 4001)
    t = torch.from_numpy(x)
    F = torch.nn.functional
    for op, fn in ((4, torch.tanh), (5, F.elu), (7, torch.sigmoid), (8, lambda v: F.gelu(v, approximate="tanh")), (10, F.silu), (11, F.hardswish),
                   (12, F.hardsigmoid), (13, torch.exp), (14, F.gelu)):
        want = fn(t).numpy(); got = ref.UNARY[op](x)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), ref.UNARY_NAMES[op]


def _tenable(t, r32, r64, what):
    assert r32.dtype == np.float32, what
    ulps, frac = ec.compare_rounded(t, ec.enc(t, r32), r64)
    assert ulps <= 1 and frac <= ec.HALF_DIFF_CAP, (what, ulps, frac)


@pytest.mark.parametrize("c", [c for c in ec.BIN_CASES if c[1][2] != F32], ids=ec.bin_id)
def test_bin_cases_tenable(c):
    x, y = ec.bin_inputs(c)
    _tenable(c[1][2], ec.bin_eval(c, x, y, np.float32), ec.bin_eval(c, x, y, np.float64), ec.bin_id(c))


@pytest.mark.parametrize("c", [c for c in ec.UNARY_CASES if c[1] != F32 and not c[3]], ids=ec.unary_id)      # (the view form has the same values)
def test_unary_cases_tenable(c):
    x = ec.unary_inputs(c)
    _tenable(c[1], ec.unary_eval(c, x, np.float32), ec.unary_eval(c, x, np.float64), ec.unary_id(c))


@pytest.mark.parametrize("c", [c for c in ec.GLU_CASES if c[1] != F32 and c[2] == "split"], ids=ec.glu_id)     # (the other forms have the same values)
def test_glu_cases_tenable(c):
    x, g = ec.glu_inputs(c)
    r64 = ec.glu_eval(c, x, g, np.float64)
    assert np.isfinite(ec.dec(c[1], ec.enc(c[1], r64))).all()
    _tenable(c[1], ec.glu_eval(c, x, g, np.float32), r64, ec.glu_id(c))


@pytest.mark.parametrize("c", [c for c in ec.ROPE_CASES if c[0] != F32 and c[4] == "cont"], ids=ec.rope_id)
def test_rope_half_cases_tenable(c):
    """float32 here means: the angles, their sines and cosines and the rotation in float32, as the kernel (and ggml) computes them"""
    t, mode, (hd, nd), (with_ff, ext, af), lay = c
    x, pos, ff = ec.rope_inputs(c)
    r64 = ec.rope_eval(c, x, pos, ff)
    assert np.abs(r64).min() >= ec.ROPE_F16_MIN
    _tenable(t, ec.rope_eval_f32(c, x, pos, ff), r64, ec.rope_id(c))


def test_permute_axes_is_ggml_permute():
    """ggml_permute(a, p): result dim p[i] = a's dim i — checked on shapes"""
    ne = (2, 3, 5, 7)
    for p in ((0, 2, 1, 3), (1, 0, 2, 3), (0, 3, 1, 2)):
        a = np.zeros(ne[::-1])
        assert np.transpose(a, ec.permute_axes(p)).shape[::-1] == ec.permuted_ne(ne, p)
