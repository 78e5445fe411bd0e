"""The weight formats of MUL_MAT(_ID) for the tests and tools (a helper like gpu_util.py, not a test file): one name -> type id table and one
weights() for all of them, plus the float64 pieces the GPU suites share (nmse, probe, ffn_f64).

The oracle knows six formats (q4_0, q8_0, q4_K, q5_K, q6_K, mxfp4) and stays that way: their bytes and values come from orc.random_blocks /
orc.dequantize. The other three are restated here in numpy and pinned bit for bit against golden vectors of the reference's gguf-py by
tests/test_q5_formats.py and tests/test_q3_k_format.py (no GPU needed):

  Q5_0: 32 elements / 22 bytes: f16 d | u32 qh (little-endian) | 16 bytes qs.   x = d * (q - 16)
  Q5_1: 32 elements / 24 bytes: f16 d | f16 m | u32 qh | 16 bytes qs.           x = d * q + m
  element j < 16: q = (qs[j] & 15) | bit j of qh << 4;   element j >= 16: q = (qs[j - 16] >> 4) | bit j of qh << 4

  Q3_K: 256 elements / 110 bytes: hmask 32 B | qs 64 B | scales 12 B | f16 d
  element 128 n + 32 j + l:  q = ((qs[32 n + l] >> 2 j) & 3) - (bit 4 n + j of hmask[l] ? 0 : 4);  group g = element / 16
  scale g: low four bits = nibble g / 8 of scales[g % 8], top two = bits 2 (g / 4) of scales[8 + g % 4], value sc - 32
  x = (d * (sc_g - 32)) * q, in f32
  gguf-py has no Q3_K quantizer, so Q3_K weights are GENERATED blocks (random_q3_k): every byte random — which reaches every bit pattern,
  negative scales included — under a block scale of chosen magnitude.
"""
import numpy as np

import oracle as orc

# enum ggml_type
TYPES = {"q4_0": 2, "q5_0": 6, "q5_1": 7, "q8_0": 8, "q3_K": 11, "q4_K": 12, "q5_K": 13, "q6_K": 14, "mxfp4": 39}
Q5_0, Q5_1, Q3_K = TYPES["q5_0"], TYPES["q5_1"], TYPES["q3_K"]
BLOCK_BYTES = {Q5_0: 22, Q5_1: 24, Q3_K: 110}
NAMES = {"q5_0": Q5_0, "q5_1": Q5_1}      # the two formats with a numpy quantizer


def _unpack_q(qh_bytes, qs):
    """qh_bytes [nb, 4] u8, qs [nb, 16] u8 -> the 32 five-bit quants per block, [nb, 32] u8"""
    qh = qh_bytes.astype(np.uint32)
    word = qh[:, 0] | (qh[:, 1] << 8) | (qh[:, 2] << 16) | (qh[:, 3] << 24)
    hi = ((word[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(np.uint8)
    nib = np.concatenate([qs & 0x0F, qs >> 4], axis=1)
    return nib | (hi << 4)


def _pack_q(q):
    """q [nb, 32] u8 in 0..31 -> (qh [nb, 4] u8, qs [nb, 16] u8)"""
    qs = (q[:, :16] & 0x0F) | ((q[:, 16:] & 0x0F) << 4)
    bits = (q >> 4).astype(np.uint32)
    word = (bits << np.arange(32, dtype=np.uint32)[None, :]).sum(axis=1, dtype=np.uint32)
    qh = np.stack([(word >> (8*i)) & 0xFF for i in range(4)], axis=1).astype(np.uint8)
    return qh, qs.astype(np.uint8)


def _f16(col):
    return np.ascontiguousarray(col).view(np.float16).astype(np.float32)      # [nb, 1]


def dequant_q5_0(blocks):
    """blocks u8 [..., n*22] -> f32 [..., n*32]"""
    b = blocks.reshape(-1, 22)
    q = _unpack_q(b[:, 2:6], b[:, 6:22]).astype(np.int32) - 16
    return (_f16(b[:, 0:2]) * q.astype(np.float32)).reshape(*blocks.shape[:-1], -1)


def dequant_q5_1(blocks):
    """blocks u8 [..., n*24] -> f32 [..., n*32]"""
    b = blocks.reshape(-1, 24)
    q = _unpack_q(b[:, 4:8], b[:, 8:24]).astype(np.float32)
    return (_f16(b[:, 0:2]) * q + _f16(b[:, 2:4])).reshape(*blocks.shape[:-1], -1)


def _inverse(d):
    with np.errstate(divide="ignore"):
        return np.where(d == 0, np.float32(0), np.float32(1) / d).astype(np.float32)


def quant_q5_0(x):
    """x f32 [..., k] -> u8 [..., k/32*22]: d = (the first element of largest magnitude) / -16, q = trunc(x/d + 16.5) in 0..31"""
    v = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 32)
    first = np.abs(v).argmax(axis=1)
    d = (v[np.arange(v.shape[0]), first] / np.float32(-16)).astype(np.float32)[:, None]
    t = np.trunc(v * _inverse(d) + np.float32(16.5)).astype(np.float32)
    q = np.clip(t.astype(np.uint8), 0, 31)
    qh, qs = _pack_q(q)
    out = np.concatenate([d.astype(np.float16).view(np.uint8), qh, qs], axis=1)
    return out.reshape(*x.shape[:-1], -1)


def quant_q5_1(x):
    """x f32 [..., k] -> u8 [..., k/32*24]: m = min, d = (max - min) / 31, q = trunc((x - m)/d + 0.5) in 0..31"""
    v = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 32)
    lo = v.min(axis=1, keepdims=True); hi = v.max(axis=1, keepdims=True)
    d = ((hi - lo) / np.float32(31)).astype(np.float32)
    t = np.trunc((v - lo) * _inverse(d) + np.float32(0.5)).astype(np.float32)
    q = np.clip(t.astype(np.uint8), 0, 31)
    qh, qs = _pack_q(q)
    out = np.concatenate([d.astype(np.float16).view(np.uint8), lo.astype(np.float16).view(np.uint8), qh, qs], axis=1)
    return out.reshape(*x.shape[:-1], -1)


DEQUANT = {Q5_0: dequant_q5_0, Q5_1: dequant_q5_1}
QUANT = {Q5_0: quant_q5_0, Q5_1: quant_q5_1}


def unpack_q3_k(blocks):
    """blocks u8 [nb, 110] -> (q int32 [nb, 256] in -4..3, sc int32 [nb, 16] in -32..31, d f32 [nb, 1])"""
    b = np.ascontiguousarray(blocks).reshape(-1, BLOCK_BYTES[Q3_K])
    hmask, qs, scales = b[:, 0:32], b[:, 32:96], b[:, 96:108]
    d = np.ascontiguousarray(b[:, 108:110]).view(np.float16).astype(np.float32)
    q = np.empty((b.shape[0], 256), np.int32)
    for n in range(2):
        for j in range(4):
            low = (qs[:, 32*n:32*n + 32] >> (2*j)) & 3
            high = (hmask >> (4*n + j)) & 1
            q[:, 128*n + 32*j:128*n + 32*j + 32] = low.astype(np.int32) - 4*(1 - high.astype(np.int32))
    sc = np.empty((b.shape[0], 16), np.int32)
    for g in range(16):
        sc[:, g] = (((scales[:, g % 8] >> (4*(g // 8))) & 0xF) | (((scales[:, 8 + g % 4] >> (2*(g // 4))) & 3) << 4)).astype(np.int32) - 32
    return q, sc, d


def dequant_q3_k(blocks):
    """blocks u8 [..., n*110] -> f32 [..., n*256]"""
    q, sc, d = unpack_q3_k(blocks)
    dl = (d * sc.astype(np.float32)).astype(np.float32)                     # [nb, 16]
    x = (np.repeat(dl, 16, axis=1) * q.astype(np.float32)).astype(np.float32)
    return x.reshape(*blocks.shape[:-1], -1)


def random_q3_k(rng, shape, k, scale):
    """valid Q3_K rows u8 [*shape, k/256*110]: every byte random, d = +-U(0.5, 2) * scale in f16"""
    assert k % 256 == 0
    nb = int(np.prod(shape, dtype=np.int64))*(k//256)
    b = rng.integers(0, 256, size=(nb, BLOCK_BYTES[Q3_K]), dtype=np.uint8)
    d = (rng.uniform(0.5, 2.0, size=nb)*rng.choice([-1.0, 1.0], size=nb)*scale).astype(np.float16)
    b[:, 108:110] = d.view(np.uint8).reshape(-1, 2)
    return b.reshape(*shape, k//256*BLOCK_BYTES[Q3_K])


def weight_bytes(rng, name, shape, k, scale=None):
    """rows of format `name`, u8 [*shape, row_bytes]. scale None: the generator as it comes — quant(U(-1, 1)) for the 32-element formats, random
    K-quant blocks with values of order one, Q3_K blocks with d = +-U(0.5, 2)/128. A number: values of about that rms (a generated Q3_K block's
    values have rms ~58 d; the other generators spread theirs over +-3 scale)."""
    if name in NAMES:
        a = 1.0 if scale is None else 3.0*scale
        return QUANT[NAMES[name]](rng.uniform(-a, a, size=(*shape, k)).astype(np.float32))
    if name == "q3_K":
        return random_q3_k(rng, shape, k, 1/128 if scale is None else scale/58)
    return orc.random_blocks(rng, TYPES[name], shape, k, scale=1.0 if scale is None else 3.0*scale)


def dequant(name, w):
    """u8 [..., row_bytes] -> f32 [..., k]"""
    if name in NAMES:
        return DEQUANT[NAMES[name]](w)
    return dequant_q3_k(w) if name == "q3_K" else orc.dequantize(w, TYPES[name])


def weights(rng, name, shape, k, scale=None):
    """(bytes u8 [*shape, row_bytes], their values f64 [*shape, k]) — weight_bytes and its dequantization"""
    w = weight_bytes(rng, name, shape, k, scale)
    return w, dequant(name, w).astype(np.float64)


def nmse(expected, got):
    e = np.asarray(expected, np.float64); g = np.asarray(got, np.float64)
    return float(((e - g)**2).sum() / ((e**2).sum() + 1e-300))


def probe(type_id, k, m, n):
    """what llama.cpp asks at load time (and what fails without the format)"""
    from gpu_util import backend, gg
    with gg.Context() as ctx:
        out = gg.base().ggml_mul_mat(ctx.ctx, ctx.new_tensor(type_id, [k, m]), ctx.new_tensor(gg.F32, [k, n]))
        assert backend().supports_op(out), f"type {type_id}: MUL_MAT refused"


def ffn_f64(x, wn, wg, wu, wd, eps):
    """RMS_NORM * wn -> gate / up -> swiglu -> down -> + x, in float64"""
    x = x.astype(np.float64)
    h = x / np.sqrt((x*x).mean(axis=-1, keepdims=True) + eps) * wn.astype(np.float64)
    g = h @ wg.T; u = h @ wu.T
    return (g / (1.0 + np.exp(-g)) * u) @ wd.T + x
