"""Q5_0 / Q5_1: this file's own numpy restatement of the two block formats against the golden vectors
(tests/golden/make_golden_q5.py: the reference's gguf-py quantize / dequantize), bit for bit.

The oracle knows six formats and stays that way; tests/test_gpu_q5_weights.py builds its weights and its float64
expectations with the functions below, so they are pinned here first (no GPU needed).

  Q5_0: 32 elements / 22 bytes: f16 d | u32 qh (little-endian) | 16 bytes qs.   x = d * (q - 16)
  Q5_1: 32 elements / 24 bytes: f16 d | f16 m | u32 qh | 16 bytes qs.           x = d * q + m
  element j < 16: q = (qs[j] & 15) | bit j of qh << 4;   element j >= 16: q = (qs[j - 16] >> 4) | bit j of qh << 4
"""
import numpy as np
import pytest

Q5_0, Q5_1 = 6, 7                       # enum ggml_type
BLOCK_BYTES = {Q5_0: 22, Q5_1: 24}
NAMES = {"q5_0": Q5_0, "q5_1": Q5_1}


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


@pytest.mark.parametrize("name", list(NAMES))
def test_dequant_matches_golden_bit_for_bit(name, golden_dir):
    g = np.load(golden_dir / f"dequant_{name}.npz")
    blocks, expected = g["blocks"], g["expected"]
    assert blocks.shape[0] >= 200 and blocks.shape[1] == BLOCK_BYTES[NAMES[name]] and expected.shape == (blocks.shape[0], 32)
    got = DEQUANT[NAMES[name]](blocks)
    assert got.dtype == np.float32 and got.shape == expected.shape
    assert np.array_equal(got.view(np.uint32), expected.view(np.uint32))


@pytest.mark.parametrize("name", list(NAMES))
def test_dequant_golden_holds_the_edge_blocks(name, golden_dir):
    """the fixture is what the issue asks for: zero block, qh all ones, qh alternating, subnormal d, negative m"""
    blocks = np.load(golden_dir / f"dequant_{name}.npz")["blocks"]
    qh0 = 2 if name == "q5_0" else 4
    qh = blocks[:, qh0:qh0 + 4]
    assert (blocks == 0).all(axis=1).any()
    assert (qh == 0xFF).all(axis=1).any() and (qh == 0xAA).all(axis=1).any() and (qh == 0x55).all(axis=1).any()
    d = np.ascontiguousarray(blocks[:, 0:2]).view(np.float16)[:, 0]
    assert ((np.abs(d.astype(np.float32)) < 6.2e-5) & (d != 0)).any()          # below the smallest normal f16
    if name == "q5_1":
        assert (np.ascontiguousarray(blocks[:, 2:4]).view(np.float16)[:, 0] < 0).any()


@pytest.mark.parametrize("name", list(NAMES))
def test_quant_matches_golden_bit_for_bit(name, golden_dir):
    g = np.load(golden_dir / f"quant_{name}.npz")
    x, expected = g["x"], g["expected"]
    got = QUANT[NAMES[name]](x)
    assert got.dtype == np.uint8 and got.shape == expected.shape
    assert np.array_equal(got, expected)
    # ... and the round trip through this file's dequantizer is the reference's
    assert np.isfinite(DEQUANT[NAMES[name]](got)).all()


@pytest.mark.parametrize("name", list(NAMES))
def test_host_row_decoder_matches_golden_bit_for_bit(name, golden_dir):
    """the C++ decoder the GGUF model path reads token-embedding rows with (csrc/harness/gguf_tools.cpp)"""
    import graft_pkg
    H = graft_pkg.load().llama_synth.harness()
    g = np.load(golden_dir / f"dequant_{name}.npz")
    blocks = np.ascontiguousarray(g["blocks"]); expected = g["expected"]
    got = np.full(expected.size, np.nan, np.float32)
    assert H.mi_gguf_dequant_row(NAMES[name], blocks.ctypes.data, got.ctypes.data, expected.size) == 1
    assert np.array_equal(got.view(np.uint32), expected.reshape(-1).view(np.uint32))


def test_package_constants_name_both_formats():
    import graft_pkg
    gg = graft_pkg.load().ggml
    assert (gg.Q5_0, gg.Q5_1) == (Q5_0, Q5_1)
    assert gg.QUANT_SIZES[gg.Q5_0] == (32, 22) and gg.QUANT_SIZES[gg.Q5_1] == (32, 24)
