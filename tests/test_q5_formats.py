"""Q5_0 / Q5_1: the numpy restatement of the two block formats (tests/weight_formats.py) against the golden vectors
(tests/golden/make_golden_q5.py: the reference's gguf-py quantize / dequantize), bit for bit, and the C++ row decoder against the same.

tests/gpu_weight_format_cases.py builds its weights and its float64 expectations with those functions, so they are pinned here first
(no GPU needed).
"""
import numpy as np
import pytest

from weight_formats import BLOCK_BYTES, DEQUANT, NAMES, Q5_0, Q5_1, QUANT


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
