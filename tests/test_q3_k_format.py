"""Q3_K: this file's own numpy restatement of the block format against the golden vectors
(tests/golden/make_golden_q3_k.py: the reference's gguf-py dequantize), bit for bit, and the C++ row decoder against the same.

The oracle knows six formats and stays that way; tests/test_gpu_q3_k_weights.py builds its weights and its float64
expectations with the functions below, so they are pinned here first (no GPU needed). gguf-py has no Q3_K quantizer, so
weights are GENERATED blocks (random_q3_k): every byte random — which reaches every bit pattern, negative scales included —
under a block scale of chosen magnitude.

  Q3_K: 256 elements / 110 bytes: hmask 32 B | qs 64 B | scales 12 B | f16 d
  element 128 n + 32 j + l:  q = ((qs[32 n + l] >> 2 j) & 3) - (bit 4 n + j of hmask[l] ? 0 : 4);  group g = element / 16
  scale g: low four bits = nibble g / 8 of scales[g % 8], top two = bits 2 (g / 4) of scales[8 + g % 4], value sc - 32
  x = (d * (sc_g - 32)) * q, in f32
"""
import numpy as np

Q3_K = 11                               # enum ggml_type
BLOCK_BYTES = 110


def unpack_q3_k(blocks):
    """blocks u8 [nb, 110] -> (q int32 [nb, 256] in -4..3, sc int32 [nb, 16] in -32..31, d f32 [nb, 1])"""
    b = np.ascontiguousarray(blocks).reshape(-1, BLOCK_BYTES)
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
    b = rng.integers(0, 256, size=(nb, BLOCK_BYTES), dtype=np.uint8)
    d = (rng.uniform(0.5, 2.0, size=nb)*rng.choice([-1.0, 1.0], size=nb)*scale).astype(np.float16)
    b[:, 108:110] = d.view(np.uint8).reshape(-1, 2)
    return b.reshape(*shape, k//256*BLOCK_BYTES)


def _golden(golden_dir):
    g = np.load(golden_dir / "dequant_q3_K.npz")
    return np.ascontiguousarray(g["blocks"]), g["expected"]


def test_dequant_matches_golden_bit_for_bit(golden_dir):
    blocks, expected = _golden(golden_dir)
    assert blocks.shape[0] >= 90 and blocks.shape[1] == BLOCK_BYTES and expected.shape == (blocks.shape[0], 256)
    got = dequant_q3_k(blocks)
    assert got.dtype == np.float32 and got.shape == expected.shape
    assert np.array_equal(got.view(np.uint32), expected.view(np.uint32))


def test_dequant_golden_holds_the_edge_blocks(golden_dir):
    blocks, _ = _golden(golden_dir)
    hmask, qs, scales = blocks[:, 0:32], blocks[:, 32:96], blocks[:, 96:108]
    d = np.ascontiguousarray(blocks[:, 108:110]).view(np.float16)[:, 0]
    assert (blocks == 0).all(axis=1).any()
    for v in (0xFF, 0x00, 0xAA, 0x55):
        assert ((hmask == v).all(axis=1) & (d != 0)).any(), hex(v)
    assert (qs == 0xFF).all(axis=1).any()
    q, sc, _ = unpack_q3_k(blocks)
    assert ((scales == 0).all(axis=1) & (d != 0)).any() and ((sc == -32).all(axis=1) & (d != 0)).any()
    assert (sc == 31).all(axis=1).any()
    assert any(len(set(row)) == 16 for row in sc.tolist())
    assert ((np.abs(d.astype(np.float32)) < 6.2e-5) & (d != 0)).any()           # below the smallest normal f16
    assert (d < 0).any()
    assert ((q == -4).all(axis=1) & (sc == -32).all(axis=1) & (np.abs(d.astype(np.float32)) >= 1024)).any()
    # the random blocks: finite d of magnitude [0.5, 2] / 128
    a = np.abs(d[:80].astype(np.float32))*128
    assert ((a >= 0.49) & (a <= 2.01)).all()


def test_random_blocks_are_valid_and_cover_negative_scales():
    rng = np.random.default_rng(3)
    w = random_q3_k(rng, (5, 3), 768, 1/128)
    assert w.shape == (5, 3, 330) and w.dtype == np.uint8
    q, sc, d = unpack_q3_k(w)
    assert q.min() == -4 and q.max() == 3 and sc.min() == -32 and sc.max() == 31
    a = np.abs(d)*128
    assert np.isfinite(d).all() and ((a >= 0.49) & (a <= 2.01)).all() and (d < 0).any() and (d > 0).any()
    x = dequant_q3_k(w)
    assert x.shape == (5, 3, 768) and np.isfinite(x).all()


def test_host_row_decoder_matches_golden_bit_for_bit(golden_dir):
    """the C++ decoder the GGUF model path reads token-embedding rows with (csrc/harness/gguf_tools.cpp): Q3_K_S files keep token_embd in Q3_K"""
    import graft_pkg
    H = graft_pkg.load().llama_synth.harness()
    blocks, expected = _golden(golden_dir)
    got = np.full(expected.size, np.nan, np.float32)
    assert H.mi_gguf_dequant_row(Q3_K, blocks.ctypes.data, got.ctypes.data, expected.size) == 1
    assert np.array_equal(got.view(np.uint32), expected.reshape(-1).view(np.uint32))


def test_package_constants_name_the_format():
    import graft_pkg
    gg = graft_pkg.load().ggml
    assert gg.Q3_K == Q3_K
    assert gg.QUANT_SIZES[gg.Q3_K] == (256, 110)
