#!/usr/bin/env python3
"""Generate the Q3_K golden vectors under tests/golden/ from the reference's own Python definition of the block format
(gguf-py/gguf/quants.py:431-472), in the manner of make_golden_q5.py.

Run ONLY in the build container (the reference tree does not travel to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_q3_k.py

Writes dequant_q3_K.npz (blocks u8 [N, 110], expected f32 [N, 256]). The committed .npz is DATA (inputs + expected outputs);
nothing here copies reference source text. tests/test_q3_k_format.py checks its own numpy restatement of the format and the
C++ row decoder against it bit for bit.

gguf-py has no Q3_K quantizer (gguf.quants.quantize raises NotImplementedError for the type — asserted below), so there is no
quantizer golden.

Block layout (little-endian): hmask 32 B | qs 64 B | scales 12 B | f16 d.
Edge blocks: all zero; hmask all ones / all zero / 0xAA / 0x55; qs all 0xFF; every scale at its minimum (twelve zero bytes -> -32) and at
its maximum (-> +31); sixteen different scales; an f16-subnormal d; a negative d; the largest quants under a large d.
"""
import os
import sys
from pathlib import Path

import numpy as np

REF = Path(os.environ.get("GGUF_PY", "/root/reference/gguf-py"))
sys.dont_write_bytecode = True
sys.path.insert(0, str(REF))
import gguf  # noqa: E402
from gguf.constants import GGMLQuantizationType as T  # noqa: E402

OUT = Path(__file__).resolve().parent
HM, QS, SC, D = slice(0, 32), slice(32, 96), slice(96, 108), slice(108, 110)


def f16_bytes(v):
    return np.array([v], dtype=np.float16).view(np.uint8)


def pack_scales(sc):
    """sixteen values 0..63 -> the 12 scale bytes: low nibble of scale g in nibble g / 8 of byte g % 8, top two bits in bits 2 (g / 4) of byte 8 + g % 4"""
    out = np.zeros(12, dtype=np.uint8)
    for g, s in enumerate(sc):
        out[g % 8] |= (s & 0xF) << (4*(g // 8))
        out[8 + g % 4] |= ((s >> 4) & 3) << (2*(g // 4))
    return out


def edge_blocks(rng):
    e = rng.integers(0, 256, size=(12, 110), dtype=np.uint8)
    for i in range(12):
        e[i, D] = f16_bytes(0.0078125)
    e[0, :] = 0                                                           # the all-zero block
    e[1, HM] = 0xFF                                                       # no element carries the -4 offset
    e[2, HM] = 0x00                                                       # every element does
    e[3, HM] = 0xAA
    e[4, HM] = 0x55
    e[5, QS] = 0xFF                                                       # low bits all 3
    e[6, SC] = 0x00                                                       # every scale -32
    e[7, SC] = 0xFF                                                       # every scale +31
    e[8, SC] = pack_scales([0, 63, 31, 32, 1, 62, 16, 47, 5, 58, 33, 30, 12, 51, 20, 43])      # sixteen different scales
    e[9, D] = f16_bytes(6e-8)                                             # f16 subnormal d
    e[10, D] = f16_bytes(-0.0117)                                         # negative d
    e[11, HM] = 0x00; e[11, QS] = 0x00; e[11, SC] = 0x00; e[11, D] = f16_bytes(1024.0)      # q = -4, scale -32 everywhere, large d: the largest magnitude
    return e


def main():
    rng = np.random.default_rng(20260811)
    bs, ts = gguf.GGML_QUANT_SIZES[T.Q3_K]
    assert (bs, ts) == (256, 110)
    try:
        gguf.quants.quantize(np.zeros((1, 256), np.float32), T.Q3_K)
        raise SystemExit("gguf-py now has a Q3_K quantizer: add a quantizer golden")
    except NotImplementedError:
        pass
    n = 88
    blocks = rng.integers(0, 256, size=(n, ts), dtype=np.uint8)
    d = (rng.uniform(0.5, 2.0, size=n)*rng.choice([-1.0, 1.0], size=n)/128.0).astype(np.float16)
    blocks[:, D] = d.view(np.uint8).reshape(-1, 2)
    blocks = np.concatenate([blocks, edge_blocks(rng)], axis=0)
    expected = gguf.quants.dequantize(blocks, T.Q3_K).astype(np.float32)
    assert expected.shape == (blocks.shape[0], bs) and np.isfinite(expected).all()
    np.savez_compressed(OUT / "dequant_q3_K.npz", blocks=blocks, expected=expected)
    print("Q3_K golden vectors written to", OUT, "-", blocks.shape[0], "blocks")


if __name__ == "__main__":
    main()
