"""ops_ref.py — numpy (float64) restatement of the element ops on the decode path.
TEST INFRASTRUCTURE ONLY (same rule as ggml_oracle.c).

The op definitions live in the reference's missing ggml.c, so the formulas are
[UPSTREAM-KNOWLEDGE]; what is citeable is how the reference calls and tests each op
 — cited per function. Arrays use numpy order [ne3, ne2, ne1, ne0]
(the reverse of ggml's ne[]).
"""
from __future__ import annotations

import math

import numpy as np


def rms_norm(x: np.ndarray, eps: float) -> np.ndarray:
    """src/llama-graph.cpp:605; tests/test-backend-ops.cpp:2773 — y = x / sqrt(mean(x^2) + eps) per row of ne0"""
    x = x.astype(np.float64)
    return x / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + eps)


def bcast(b: np.ndarray, shape) -> np.ndarray:
    """ggml repeat-broadcast of b to `shape` (tests/test-backend-ops.cpp:2469)"""
    reps = [s // bs for s, bs in zip(shape, b.shape)]
    return np.tile(b, reps)


def silu(x):
    x = x.astype(np.float64)
    return x / (1.0 + np.exp(-x))


def swiglu(a, b):
    """src/llama-graph.cpp:691; tests/test-backend-ops.cpp:1832-1888 — silu(a) * b"""
    return silu(a) * b.astype(np.float64)


def swiglu_oai(a, b, alpha=1.702, limit=7.0):
    """src/llama-graph.cpp:961-968; tests/test-backend-ops.cpp:1890-1949"""
    x = np.minimum(a.astype(np.float64), limit)
    y = np.clip(b.astype(np.float64), -limit, limit)
    return (x / (1.0 + np.exp(-x * alpha))) * (y + 1.0)


def gelu(x):
    x = x.astype(np.float64)
    return 0.5 * x * (1.0 + np.tanh(0.79788456080286535587989211986876 * x * (1.0 + 0.044715 * x * x)))


def soft_max(x, mask=None, scale=1.0, max_bias=0.0, sinks=None):
    """src/llama-graph.cpp:1312-1313; tests/test-backend-ops.cpp:3569-3626.
    x [ne3, ne2(heads), ne1, ne0]; mask [ne3', ne2', >=ne1, ne0] broadcast over heads; sinks [ne2]."""
    x = x.astype(np.float64) * scale
    n3, n_head, n1, n0 = x.shape
    if mask is not None:
        m = mask.astype(np.float64)[:, :, :n1, :]
        m = np.tile(m, (n3 // m.shape[0], n_head // m.shape[1], 1, 1))
        if max_bias > 0.0:
            n_head_log2 = 1 << int(math.floor(math.log2(n_head)))
            m0 = 2.0 ** (-max_bias / n_head_log2)
            m1 = 2.0 ** (-(max_bias / 2.0) / n_head_log2)
            slope = np.array([m0 ** (h + 1) if h < n_head_log2 else m1 ** (2 * (h - n_head_log2) + 1) for h in range(n_head)])
            m = m * slope[None, :, None, None]
        x = x + m
    mx = x.max(axis=-1, keepdims=True)
    if sinks is not None:
        s = sinks.astype(np.float64)[None, :, None, None]
        mx = np.maximum(mx, s)
    e = np.exp(x - mx)
    den = e.sum(axis=-1, keepdims=True)
    if sinks is not None:
        den = den + np.exp(s - mx)
    return e / den


def _rope_corr_dims(n_dims, n_ctx_orig, freq_base, beta_fast, beta_slow):
    def corr_dim(n_rot):
        return n_dims * math.log(n_ctx_orig / (n_rot * 2 * math.pi)) / (2 * math.log(freq_base))
    start = math.floor(corr_dim(beta_fast))
    end = math.ceil(corr_dim(beta_slow))
    return max(0, start), min(n_dims - 1, end)


def rope(x, pos, n_dims, mode, n_ctx_orig=0, freq_base=10000.0, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0,
         beta_fast=32.0, beta_slow=1.0, freq_factors=None):
    """src/llama-model.cpp:6030-6040; tests/test-backend-ops.cpp:3660-3782.
    x [ne3, ne2(tokens), ne1(heads), ne0(head dim)]; pos [ne2]; NORM rotates (2i, 2i+1), NEOX (i, i + n_dims/2)."""
    x = x.astype(np.float64)
    out = x.copy()
    neox = (mode & 2) != 0
    theta_scale = freq_base ** (-2.0 / n_dims)
    lo, hi = _rope_corr_dims(n_dims, n_ctx_orig, freq_base, beta_fast, beta_slow) if ext_factor != 0.0 else (0, 0)
    half = n_dims // 2
    ip = np.arange(half)
    for t in range(x.shape[1]):
        theta_extrap = float(pos[t]) * theta_scale ** ip
        if freq_factors is not None:
            theta_extrap = theta_extrap / freq_factors[:half].astype(np.float64)
        theta_interp = freq_scale * theta_extrap
        theta = theta_interp
        mscale = attn_factor
        if ext_factor != 0.0:
            y = (ip - lo) / max(0.001, hi - lo)
            ramp_mix = (1.0 - np.clip(y, 0.0, 1.0)) * ext_factor
            theta = theta_interp * (1 - ramp_mix) + theta_extrap * ramp_mix
            mscale = attn_factor * (1.0 + 0.1 * math.log(1.0 / freq_scale))
        c, s = np.cos(theta) * mscale, np.sin(theta) * mscale
        if neox:
            x0, x1 = x[:, t, :, :half], x[:, t, :, half:n_dims]
            out[:, t, :, :half] = x0 * c - x1 * s
            out[:, t, :, half:n_dims] = x0 * s + x1 * c
        else:
            x0, x1 = x[:, t, :, 0:n_dims:2], x[:, t, :, 1:n_dims:2]
            out[:, t, :, 0:n_dims:2] = x0 * c - x1 * s
            out[:, t, :, 1:n_dims:2] = x0 * s + x1 * c
    return out


def set_rows(dst, src, idx):
    """src/llama-kv-cache-unified.cpp:1123; tests/test-backend-ops.cpp:2060-2127.
    dst [ne3, ne2, nrows, ne0]; src [ne3, ne2, ne1, ne0]; idx i64 [ne12, ne11, ne1] broadcast over (ne2 % ne11, ne3 % ne12)"""
    out = dst.copy()
    n3, n2, n1, _ = src.shape
    for i3 in range(n3):
        for i2 in range(n2):
            for i1 in range(n1):
                r = int(idx[i3 % idx.shape[0], i2 % idx.shape[1], i1])
                out[i3, i2, r, :] = src[i3, i2, i1, :].astype(out.dtype)
    return out


def get_rows(src, idx):
    """tests/test-backend-ops.cpp:1951 — src [ne3?, ne2, nrows, ne0], idx i32 [ne12, ne11, ne10] -> [ne12, ne11, ne10, ne0]"""
    n12, n11, n10 = idx.shape
    out = np.empty((n12, n11, n10, src.shape[-1]), dtype=np.float64)
    for i12 in range(n12):
        for i11 in range(n11):
            for i10 in range(n10):
                out[i12, i11, i10] = src[i12 if src.shape[0] > 1 else 0, i11, int(idx[i12, i11, i10])]
    return out


def add_id(a, bias, ids):
    """src/llama-graph.cpp:927; tests/test-backend-ops.cpp:2548 — a [n_tok, n_used, ne0], bias [n_expert, ne0], ids [n_tok, n_used]"""
    return a.astype(np.float64) + bias.astype(np.float64)[ids]


def argsort_desc(x):
    """tests/test-backend-ops.cpp:4120 — indices sorting each row of ne0 in descending order"""
    return np.argsort(-x, axis=-1, kind="stable").astype(np.int32)


def mul_mat_dense(a, b):
    """tests/test-backend-ops.cpp:3127-3191 — a [ne03, ne02, m, k], b [ne13, ne12, n, k] -> [ne13, ne12, n, m], broadcast r2/r3"""
    a = a.astype(np.float64); b = b.astype(np.float64)
    r3, r2 = b.shape[0] // a.shape[0], b.shape[1] // a.shape[1]
    out = np.empty((b.shape[0], b.shape[1], b.shape[2], a.shape[2]))
    for i3 in range(b.shape[0]):
        for i2 in range(b.shape[1]):
            out[i3, i2] = b[i3, i2] @ a[i3 // r3, i2 // r2].T
    return out


def flash_attn_ext(q, K, V, mask, scale, max_bias=0.0, softcap=0.0, sinks=None):
    """FLASH_ATTN_EXT (ggml_compute_forward_flash_attn_ext_f16, ggml/src/ggml-cpu/ops.cpp) in float64: q [T, n_head, hd], K / V the dequantized cache
    [n_kv, n_head_kv, hd], mask [>= T, n_kv] (the f32 values of the f16 mask), sinks [n_head] or None -> [T, n_head, hd]. ALiBi: head h's mask
    times its slope; the soft-cap: scale / c, then c * tanh."""
    T, n_head, hd = q.shape
    n_head_kv = K.shape[1]
    n2 = 1 << int(np.floor(np.log2(n_head)))
    m0, m1 = 2.0 ** (-max_bias / n2), 2.0 ** (-(max_bias / 2.0) / n2)
    out = np.zeros((T, n_head, hd))
    for h in range(n_head):
        hk = h // (n_head // n_head_kv)
        slope = 1.0 if max_bias <= 0 else (m0 ** (h + 1) if h < n2 else m1 ** (2 * (h - n2) + 1))
        s = q[:, h, :].astype(np.float64) @ K[:, hk, :].T * scale
        if softcap:
            s = softcap * np.tanh(s / softcap)
        s = s + slope * mask[:T].astype(np.float64)
        mx = s.max(-1, keepdims=True)
        if sinks is not None:
            mx = np.maximum(mx, sinks[h])
        p = np.exp(s - mx); den = p.sum(-1, keepdims=True) + (np.exp(sinks[h] - mx) if sinks is not None else 0.0)
        out[:, h, :] = (p / den) @ V[:, hk, :]
    return out


# ---- element ops beyond the decode path: every variant supports_op accepts (tests/test_gpu_elem_ops.py) ----------------------------
def _f64(x):
    return np.asarray(x, dtype=np.float64)


# The tables keep the dtype they are given: float64 for the reference; float32 to ask, on the CPU, how far a float32 evaluation of the
# same formula lands from it. The GELU forms are written without the cancellation of 1 + tanh(u) and 1 + erf(z) in the negative tail:
# 0.5 * (1 + tanh(u)) = 1 / (1 + exp(-2u)) and 1 + erf(z) = erfc(-z), the same functions.
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _gelu_tanh(x):
    return x * _sigmoid(2.0 * (0.79788456080286535587989211986876 * x * (1.0 + 0.044715 * x * x)))


def _gelu_erf(x):
    return 0.5 * x * _erfc(-x * 0.70710678118654752440).astype(x.dtype)


def _hardsigmoid(x):
    return np.minimum(1.0, np.maximum(0.0, (x + 3.0) / 6.0))


def _swiglu_oai(x, g, alpha=1.702, limit=7.0):
    xc = np.minimum(x, limit)
    return (xc * _sigmoid(xc * alpha)) * (np.clip(g, -limit, limit) + 1.0)


# enum ggml_unary_op order (ABS ... GELU_ERF) -> f(x), from the mathematical definitions; GELU is the tanh form with elem.hip's constants
UNARY = {
    0: np.abs,
    1: lambda x: np.where(x > 0, 1.0, np.where(x < 0, -1.0, 0.0)).astype(x.dtype),
    2: lambda x: -x,
    3: lambda x: (x > 0).astype(x.dtype),
    4: np.tanh,
    5: lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0.0))),
    6: lambda x: np.where(x > 0, x, 0.0).astype(x.dtype),
    7: _sigmoid,
    8: _gelu_tanh,
    9: lambda x: x * _sigmoid(1.702 * x),
    10: lambda x: x * _sigmoid(x),
    11: lambda x: x * _hardsigmoid(x),
    12: _hardsigmoid,
    13: np.exp,
    14: _gelu_erf,
}
UNARY_NAMES = ["abs", "sgn", "neg", "step", "tanh", "elu", "relu", "sigmoid", "gelu", "gelu_quick", "silu", "hardswish", "hardsigmoid", "exp", "gelu_erf"]


# enum ggml_glu_op order (REGLU, GEGLU, SWIGLU, SWIGLU_OAI, GEGLU_ERF, GEGLU_QUICK) -> f(x, g): act(x) * g (SWIGLU_OAI: alpha 1.702, limit 7)
GLU = {
    0: lambda x, g: np.maximum(x, 0.0) * g,
    1: lambda x, g: _gelu_tanh(x) * g,
    2: lambda x, g: x * _sigmoid(x) * g,
    3: _swiglu_oai,
    4: lambda x, g: _gelu_erf(x) * g,
    5: lambda x, g: x * _sigmoid(1.702 * x) * g,
}
GLU_NAMES = ["reglu", "geglu", "swiglu", "swiglu_oai", "geglu_erf", "geglu_quick"]


def sub(a, b):
    """a - repeat(b) in float64 (tests/test-backend-ops.cpp:2469)"""
    return _f64(a) - bcast(_f64(b), a.shape)


def argsort(x, order):
    """tests/test-backend-ops.cpp:4120 — order 0 ascending, 1 descending"""
    return np.argsort(x if order == 0 else -x, axis=-1, kind="stable").astype(np.int32)


def get_rows_batched(src, idx):
    """tests/test-backend-ops.cpp:1951 — src [ne3, ne2, rows, ne0], idx [ne12, ne11, ne10] with ne11 = ne2, ne12 = ne3 -> [ne12, ne11, ne10, ne0];
    the values are moved, not computed: the result keeps src's dtype"""
    n12, n11, n10 = idx.shape
    out = np.empty((n12, n11, n10, src.shape[-1]), dtype=src.dtype)
    for i12 in range(n12):
        for i11 in range(n11):
            out[i12, i11] = src[i12, i11][idx[i12, i11]]
    return out


def set_rows_bcast(dst, src, idx, conv):
    """tests/test-backend-ops.cpp:2060-2127 — dst [ne3, ne2, rows, ne0] (storage dtype), src f32 [ne3, ne2, ne1, ne0], idx i64 [ne12, ne11, ne1]
    broadcast over (i2 % ne11, i3 % ne12); conv rounds a float32 row to dst's storage"""
    out = dst.copy()
    n3, n2, n1, _ = src.shape
    for i3 in range(n3):
        for i2 in range(n2):
            out[i3, i2, idx[i3 % idx.shape[0], i2 % idx.shape[1]]] = conv(src[i3, i2])
    return out


def cpy(src_view, dst_shape):
    """tests/test-backend-ops.cpp:2438 — element i of src (in src's logical order) becomes element i of dst (in dst's logical order)"""
    return np.ascontiguousarray(src_view).reshape(dst_shape)


def round_f16(x):
    """float -> IEEE binary16, round to nearest even (one rounding, also from float64)"""
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16)


def round_bf16(x):
    """float32 -> bf16 bits (uint16): round to nearest even on the upper 16 bits; NaN stays NaN with the quiet bit set
    (ggml_compute_fp32_to_bf16's rule, restated in elem.hip st_elem)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (u.astype(np.uint64) + np.uint64(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)).astype(np.uint64)) >> np.uint64(16)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(64), r).astype(np.uint16)


def bf16_to_f32(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_bf16_from_f64(x):
    """float64 -> bf16 bits with ONE rounding (through float32 would round twice): the two bf16 neighbours of the float32 image are
    compared with x in float64 (their differences are exact), ties to the even mantissa"""
    x = _f64(x)
    with np.errstate(over="ignore"):
        u = np.ascontiguousarray(x.astype(np.float32)).view(np.uint32)
    lo = u & np.uint32(0xFFFF0000)
    hi = lo + np.uint32(0x10000)
    with np.errstate(invalid="ignore"):
        flo, fhi = lo.view(np.float32).astype(np.float64), hi.view(np.float32).astype(np.float64)
    fhi = np.where(np.isinf(fhi), np.copysign(2.0 ** 128, fhi), fhi)       # the neighbour above the largest finite bf16 stands for infinity
    with np.errstate(invalid="ignore"):
        dlo, dhi = np.abs(x - flo), np.abs(fhi - x)
    up = (dhi < dlo) | ((dhi == dlo) & (((lo >> np.uint32(16)) & np.uint32(1)) == 1))
    out = np.where(up, hi, lo) >> np.uint32(16)
    special = ~np.isfinite(x)
    return np.where(special, round_bf16(x.astype(np.float32)), out).astype(np.uint16)
