"""Cases, inputs and comparisons shared by tests/test_gpu_elem_ops.py (the kernels, on the GPU) and tests/test_elem_cases.py (the same
inputs on the CPU: is the half-precision tolerance tenable for them?). No GPU and no native library is touched here.

Arrays are in numpy order [ne3, ne2, ne1, ne0]; a tensor's `ne` tuples are in ggml order. Types are the ggml_type numbers."""
import numpy as np

import ops_ref as ref

F32, F16, I32, BF16 = 0, 1, 26, 30
TNAME = {F32: "f32", F16: "f16", BF16: "bf16", I32: "i32"}
ESIZE = {F32: 4, F16: 2, BF16: 2, I32: 4}

SHAPES = [(128, 2, 2, 2), (5, 7, 11, 13)]      # the reference's two (tests/test-backend-ops.cpp:5274-5303): one contiguous-friendly, one odd in every dim
HALF_DIFF_CAP = 0.01                            # at most 1 % of a case's elements may differ from the once-rounded float64 result


# ---- storage: values <-> what tensor_set / tensor_get move -----------------------------------------------------------------------
def enc(t, x):
    """float values (float32, or float64 for an expected result: ONE rounding) -> the type's storage array"""
    x = np.asarray(x)
    if t == F32:
        return x.astype(np.float32)
    if t == F16:
        return ref.round_f16(x)
    if t == BF16:
        return ref.round_bf16(x) if x.dtype == np.float32 else ref.round_bf16_from_f64(x)
    raise ValueError(t)


def dec(t, s):
    """storage array -> float64 values"""
    return (ref.bf16_to_f32(s) if t == BF16 else np.asarray(s)).astype(np.float64)


def quant(t, x):
    """the float64 values a kernel sees after x (float32) was stored as type t"""
    return dec(t, enc(t, np.asarray(x, dtype=np.float32)))


def key(t, s):
    """storage -> integers ordered like the values, one step per representable value, +0 and -0 both 0 (NaN: compare positions apart)"""
    if t == F32:
        u = np.ascontiguousarray(s, np.float32).view(np.uint32).astype(np.int64); sign = u >> 31; mag = u & 0x7FFFFFFF
    else:
        u = np.ascontiguousarray(s).view(np.uint16).astype(np.int64); sign = u >> 15; mag = u & 0x7FFF
    return np.where(sign == 1, -mag, mag)


def is_nan(t, s):
    return np.isnan(dec(t, s))


def compare_rounded(t, got, exp64):
    """got (storage of type t) against the float64 result rounded once to t -> (max distance in ulps of t, fraction of elements that differ).
    NaN positions must agree."""
    want = enc(t, exp64)
    gn, wn = is_nan(t, got), is_nan(t, want)
    assert np.array_equal(gn, wn), "NaN positions differ"
    d = np.abs(key(t, got) - key(t, want))[~gn]
    return (int(d.max()) if d.size else 0), (float((d != 0).mean()) if d.size else 0.0)


def assert_half(t, got, exp64, what=""):
    """F16 / BF16 output: every element within 1 ulp of the once-rounded float64 result (a flip at a rounding tie is the only legal
    difference: the float32 evaluation error is far below half an ulp), and at most 1 % of the elements differ at all"""
    ulps, frac = compare_rounded(t, got, exp64)
    assert ulps <= 1 and frac <= HALF_DIFF_CAP, (what, ulps, frac)


def assert_f32_1ulp(got, exp64, what=""):
    """one correctly rounded float32 operation: within 1 ulp of the float64 result rounded to float32"""
    ulps, _ = compare_rounded(F32, got, exp64)
    assert ulps <= 1, (what, ulps)


def nmse(exp, got):
    exp = np.asarray(exp, np.float64); got = np.asarray(got, np.float64)
    den = float((exp * exp).sum())
    return float(((exp - got) ** 2).sum()) / den if den > 0 else float(((exp - got) ** 2).sum())


def assert_out(t, got, exp64, gate, what=""):
    """the output rule of one case: F32 -> the NMSE gate; F16 / BF16 -> 1 ulp and the 1 % cap"""
    if t == F32:
        assert np.isfinite(got).all() and nmse(exp64, got) <= gate, (what, nmse(exp64, got))
    else:
        assert_half(t, got, exp64, what)


# ---- layout ----------------------------------------------------------------------------------------------------------------------
def permute_axes(p):
    """ggml_permute(a, p0, p1, p2, p3) puts a's dim i at dim p[i] -> the numpy `axes` of the same view"""
    axes = [0] * 4
    for i in range(4):
        axes[3 - p[i]] = 3 - i
    return axes


def permuted_ne(ne, p):
    out = [0] * 4
    for i in range(4):
        out[p[i]] = ne[i]
    return tuple(out)


def view_parent_ne(ne, extra_rows=True):
    """the parent of the view form: ne0 + 3 columns and (unless the op's constructor wants dims 1..3 contiguous) one extra row per dim"""
    return (ne[0] + 3,) + tuple(n + (1 if extra_rows else 0) for n in ne[1:])


def embed(t, data, extra_rows=True, seed=12345):
    """data [ne3, ne2, ne1, ne0] (storage) -> the parent array of the view form: data sits from column 1, everything else is a
    pattern of other values of the same type"""
    ne = data.shape[::-1]
    pne = view_parent_ne(ne, extra_rows)
    rng = np.random.default_rng(seed)
    if t == I32:
        par = rng.integers(-1000, 1000, size=pne[::-1]).astype(np.int32)
    else:
        par = enc(t, rng.uniform(50, 100, size=pne[::-1]).astype(np.float32))
    par[:ne[3], :ne[2], :ne[1], 1:1 + ne[0]] = data
    return par


# ---- bin ops ---------------------------------------------------------------------------------------------------------------------
BIN_OPS = ["add", "sub", "mul", "div"]
BIN_TYPES = [(F32, F32, F32), (F16, F16, F16), (BF16, BF16, BF16), (F16, F32, F16), (F32, F16, F32)]     # (a, b, dst); dst has a's type
BIN_SHAPES = [((4096, 1, 1, 1), (1, 1, 1, 1)), ((64, 5, 3, 2), (1, 1, 1, 1)), ((16, 5, 4, 3), (1, 2, 1, 1)), ((4096, 8, 1, 1), (1, 8, 1, 1)),
              ((1, 4, 7, 1), (32, 1, 1, 1)),
              ((10, 5, 4, 3), (2, 1, 1, 1)), ((10, 5, 4, 3), (1, 1, 2, 2)), ((10, 5, 4, 3), (2, 2, 2, 2)),
              ((16, 5, 4, 3), (2, 1, 1, 1)), ((16, 5, 4, 3), (1, 1, 2, 2)), ((16, 5, 4, 3), (2, 2, 2, 2))]
BIN_CASES = [(op, tt, ne, nr) for op in BIN_OPS for tt in BIN_TYPES for ne, nr in BIN_SHAPES]


def bin_id(c):
    op, tt, ne, nr = c
    return f"{op}-{TNAME[tt[0]]}_{TNAME[tt[1]]}-{'x'.join(map(str, ne))}-nr{''.join(map(str, nr))}"


def bin_inputs(c):
    """-> (x, y) float32, already values of their types; b in U(0.5, 1.5) so that DIV stays away from 0"""
    op, (ta, tb, _), ne, nr = c
    rng = np.random.default_rng(2)
    ne_a = tuple(n * r for n, r in zip(ne, nr))
    x = quant(ta, rng.uniform(-1, 1, size=ne_a[::-1])).astype(np.float32)
    y = quant(tb, rng.uniform(0.5, 1.5, size=ne[::-1])).astype(np.float32)
    return x, y


def bin_eval(c, x, y, dtype):
    x = x.astype(dtype); yb = ref.bcast(y.astype(dtype), x.shape)
    return {"add": x + yb, "sub": x - yb, "mul": x * yb, "div": x / yb}[c[0]]


# ---- UNARY -----------------------------------------------------------------------------------------------------------------------
UNARY_EXACT = (0, 1, 2, 3, 6)       # ABS, SGN, NEG, STEP, RELU: compared as integers
UNARY_CASES = [(op, t, ne, view) for op in range(15) for t in (F32, F16, BF16) for ne in SHAPES for view in (False, True)]


def unary_id(c):
    op, t, ne, view = c
    return f"{ref.UNARY_NAMES[op]}-{TNAME[t]}-{'x'.join(map(str, ne))}-{'view' if view else 'cont'}"


def unary_inputs(c):
    op, t, ne, _ = c
    rng = np.random.default_rng(3 + op)
    lim = 10.0 if op == 13 else 5.0
    x = rng.uniform(-lim, lim, size=ne[::-1]).astype(np.float32)
    x.reshape(-1)[:6] = [0.0, -0.0, 3.0, -3.0, 6.0, -6.0]
    return quant(t, x).astype(np.float32)


def unary_eval(c, x, dtype):
    return ref.UNARY[c[0]](x.astype(dtype))


# ---- GLU -------------------------------------------------------------------------------------------------------------------------
GLU_FORMS = ["split", "split_views", "single", "single_swapped"]
GLU_CASES = [(op, t, form, ne) for op in range(6) for t in (F32, F16, BF16) for form in GLU_FORMS for ne in SHAPES]


def glu_id(c):
    op, t, form, ne = c
    return f"{ref.GLU_NAMES[op]}-{TNAME[t]}-{form}-{'x'.join(map(str, ne))}"


def glu_inputs(c):
    """-> (x, g): the activated half and the gate half, float32 values of type t; +-150 where the reference uses it to catch overflow
    (tests/test-backend-ops.cpp:1882-1886), +-10 for the GELU family. BF16 has float32's exponent range, so a BF16 result can hold what a
    float32 evaluation has already lost: expf(-x) is infinite from x = -88.7 (alpha * x for swiglu_oai), and x / inf = -0 where the true
    silu(-100) = -3.7e-42 is a BF16 subnormal. The 1-ulp rule can be asked only where float32 holds the intermediate: +-50 for BF16."""
    op, t, _, ne = c
    rng = np.random.default_rng(40 + op)
    lim = (50.0 if t == BF16 else 150.0) if op in (0, 2, 3) else 10.0
    x = quant(t, rng.uniform(-lim, lim, size=ne[::-1])).astype(np.float32)
    g = quant(t, rng.uniform(-lim, lim, size=ne[::-1])).astype(np.float32)
    return x, g


def glu_eval(c, x, g, dtype):
    return ref.GLU[c[0]](x.astype(dtype), g.astype(dtype))


# ---- ROPE ------------------------------------------------------------------------------------------------------------------------
ROPE_HEADS = [(80, 20), (80, 32), (80, 80), (128, 128), (64, 64)]          # (head size, n_dims)
ROPE_FF = [(False, 0.0, 1.0), (True, 0.0, 1.0), (False, 1.0, 1.4245)]      # (freq factors, ext_factor, attn_factor); ext_factor != 0 pairs with freq_scale 0.5
ROPE_CASES = [(t, mode, hn, ff, lay) for t in (F32, F16, BF16) for mode in (0, 2) for hn in ROPE_HEADS for ff in ROPE_FF for lay in ("cont", "qkv")]
ROPE_NHEAD, ROPE_NTOK = 3, 5


def rope_id(c):
    t, mode, (hd, nd), (ff, ext, af), lay = c
    return f"{TNAME[t]}-{'neox' if mode else 'norm'}-h{hd}_{nd}-ff{int(ff)}-ext{ext:g}-{lay}"


ROPE_POS = {F32: [0, 1, 17, 300, 511], F16: [0, 1, 2, 3, 1], BF16: [0, 1, 2, 3, 1]}
ROPE_F16_MIN = 2.0 ** -9


def rope_inputs(c):
    """-> (x, pos, freq factors). F32 output is gated by NMSE and an absolute 1e-3, so its positions span the range. An F16 result is held to
    1 ulp of F16, and that can only be asked where float32 arithmetic is that good: the angle pos * theta_scale^i carries a relative error of
    about i * 2^-23 (theta_scale is a float32, raised to the i-th power), at most pos * 2.2e-7 absolute at the sizes used here, and x0*c - x1*s
    adds about 1e-7 of its own, whatever the size of the result. With pos <= 3 that is 7.6e-7, below the F16 ulp of 9.5e-7 at 2^-9: so the F16
    cases use positions 0..3 and the first seed whose every result is at least 2^-9 in magnitude (BF16, with its wider ulp, likewise)."""
    t, mode, (hd, nd), (with_ff, ext, af), lay = c
    pos = np.array(ROPE_POS[t], dtype=np.int32)
    for seed in range(5, 400):
        rng = np.random.default_rng(seed)
        x = quant(t, rng.uniform(-1, 1, size=(1, ROPE_NTOK, ROPE_NHEAD, hd))).astype(np.float32)
        ff = rng.uniform(0.9, 1.1, size=nd // 2).astype(np.float32) if with_ff else None
        if t == F32 or np.abs(rope_eval(c, x, pos, ff)).min() >= ROPE_F16_MIN:
            return x, pos, ff
    raise AssertionError("no seed keeps every F16 ROPE result above 2^-9")


def rope_eval(c, x, pos, ff):
    t, mode, (hd, nd), (with_ff, ext, af), lay = c
    return ref.rope(x, pos, nd, mode, 8192, 500000.0, 0.5 if ext else 1.0, ext, af, 32.0, 1.0, ff)


def rope_eval_f32(c, x, pos, ff):
    """the rotation with every step in float32, in the kernel's order (elem.hip k_rope, rope_yarn): theta_scale = powf(base, -2 / n_dims),
    theta = pos * powf(theta_scale, i) / ff, YaRN's ramp, cos / sin times mscale, x0*c - x1*s"""
    import math
    t, mode, (hd, nd), (with_ff, ext, af), lay = c
    f = np.float32
    fs = f(0.5 if ext else 1.0)
    theta_scale = np.power(f(500000.0), f(-2.0) / f(nd), dtype=np.float32)
    lo, hi = ref._rope_corr_dims(nd, 8192, 500000.0, 32.0, 1.0)
    ip = np.arange(nd // 2)
    out = x.astype(np.float32).copy()
    for tok in range(x.shape[1]):
        te = f(pos[tok]) * np.power(theta_scale, ip.astype(np.float32), dtype=np.float32)
        if ff is not None:
            te = te / ff[:nd // 2]
        theta = fs * te
        ms = f(af)
        if ext:
            y = (ip.astype(np.float32) - f(lo)) / f(max(0.001, hi - lo))
            mix = (f(1) - np.clip(y, f(0), f(1))) * f(ext)
            theta = theta * (f(1) - mix) + te * mix
            ms = ms * (f(1) + f(0.1) * f(math.log(1.0 / float(fs))))
        cs, sn = np.cos(theta).astype(np.float32) * ms, np.sin(theta).astype(np.float32) * ms
        sl = (slice(0, nd // 2), slice(nd // 2, nd)) if mode & 2 else (slice(0, nd, 2), slice(1, nd, 2))
        x0, x1 = x[:, tok, :, sl[0]].astype(np.float32), x[:, tok, :, sl[1]].astype(np.float32)
        out[:, tok, :, sl[0]] = x0 * cs - x1 * sn
        out[:, tok, :, sl[1]] = x0 * sn + x1 * cs
    return out


# ---- conversions -----------------------------------------------------------------------------------------------------------------
def conversion_specials():
    """the float32 values at which a float -> F16 / BF16 conversion goes wrong: signed zeros, infinities, NaN, the F16 overflow edge
    (65504 is the largest finite value, 65520 the first that rounds to infinity), the F16 subnormal edges, ties of both formats,
    and the BF16 overflow edge"""
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 65504.0, 65519.99, 65520.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10),
                     1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.3895e38, np.finfo(np.float32).max,
                     -65504.0, -65520.0, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -8), -3.3895e38, -np.finfo(np.float32).max], dtype=np.float32)


def convert(src_t, dst_t, s):
    """storage of src_t -> storage of dst_t, the way a copy converts: same type = the bits; else through float32, one rounding"""
    if src_t == dst_t:
        return s.copy()
    f = s if src_t == F32 else (ref.bf16_to_f32(s) if src_t == BF16 else s.astype(np.float32))
    return enc(dst_t, f)


def same_storage(t, a, b):
    """bit-exact comparison; NaN positions compared as 'is NaN'"""
    if t == I32:
        return np.array_equal(a, b)
    an, bn = is_nan(t, a), is_nan(t, b)
    ai = np.ascontiguousarray(a).view(np.uint32 if t == F32 else np.uint16); bi = np.ascontiguousarray(b).view(ai.dtype)
    return np.array_equal(an, bn) and np.array_equal(ai[~an], bi[~bn])
