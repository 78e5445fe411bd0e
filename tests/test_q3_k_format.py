"""Q3_K: the numpy restatement of the block format (tests/weight_formats.py) against the golden vectors
(tests/golden/make_golden_q3_k.py: the reference's gguf-py dequantize), bit for bit, and the C++ row decoder against the same.

tests/gpu_weight_format_cases.py builds its Q3_K weights (generated blocks: random_q3_k) and its float64 expectations with those
functions, so they are pinned here first (no GPU needed).
"""
import numpy as np

from weight_formats import Q3_K, dequant_q3_k, random_q3_k, unpack_q3_k
from weight_formats import BLOCK_BYTES as _BYTES

BLOCK_BYTES = _BYTES[Q3_K]


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
