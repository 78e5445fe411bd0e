#!/usr/bin/env python3
"""Generate the Q5_0 / Q5_1 golden vectors under tests/golden/ from the reference's own Python definition of the
two block formats (gguf-py/gguf/quants.py:291-375), in the manner of make_golden.py.

Run ONLY in the build container (the reference tree does not travel to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_q5.py

Writes dequant_q5_0.npz, dequant_q5_1.npz (blocks, expected) and quant_q5_0.npz, quant_q5_1.npz (x, expected).
The committed .npz files are DATA (inputs + expected outputs); nothing here copies reference source text.
tests/test_q5_formats.py checks the numpy restatement of both formats (tests/weight_formats.py) against them bit for bit.

Block layouts (little-endian):  Q5_0 = f16 d | u32 qh | 16 B qs;   Q5_1 = f16 d | f16 m | u32 qh | 16 B qs.
Edge blocks of the dequant fixtures: all zero; qh all ones; qh alternating (0xAAAAAAAA, 0x55555555); an f16-subnormal d;
a negative m (Q5_1); the largest quants (all nibbles and all high bits set) under a large d.
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
TYPES = {"q5_0": T.Q5_0, "q5_1": T.Q5_1}
N_F16 = {"q5_0": 1, "q5_1": 2}            # f16 fields in front of qh


def f16_bytes(v):
    return np.array([v], dtype=np.float16).view(np.uint8)


def edge_blocks(name, ts, rng):
    nf = N_F16[name]
    qh0 = 2*nf
    e = np.zeros((8, ts), dtype=np.uint8)                                 # [0]: the all-zero block
    e[1:, qh0 + 4:] = rng.integers(0, 256, size=(7, 16), dtype=np.uint8)
    for i in range(1, 8):
        e[i, 0:2] = f16_bytes(0.5)
        if nf == 2:
            e[i, 2:4] = f16_bytes(0.25)
    e[1, qh0:qh0 + 4] = 0xFF                                              # qh all ones
    e[2, qh0:qh0 + 4] = 0xAA                                              # qh alternating, odd elements
    e[3, qh0:qh0 + 4] = 0x55                                              # qh alternating, even elements
    e[4, 0:2] = f16_bytes(6e-8)                                           # f16 subnormal d
    e[4, qh0:qh0 + 4] = rng.integers(0, 256, size=4, dtype=np.uint8)
    e[5, qh0:qh0 + 4] = rng.integers(0, 256, size=4, dtype=np.uint8)
    if nf == 2:
        e[5, 2:4] = f16_bytes(-3.75)                                      # negative m
    else:
        e[5, 0:2] = f16_bytes(-0.5)                                       # negative d
    e[6, 0:2] = f16_bytes(1024.0); e[6, qh0:] = 0xFF                      # q = 31 everywhere, large d
    e[7, qh0:qh0 + 4] = [0x01, 0x00, 0x00, 0x80]                          # only elements 0 and 31 carry the fifth bit
    return e


def main():
    rng = np.random.default_rng(20260607)
    for name, qt in TYPES.items():
        bs, ts = gguf.GGML_QUANT_SIZES[qt]
        assert (bs, ts) == {"q5_0": (32, 22), "q5_1": (32, 24)}[name]
        # --- dequant goldens: random bytes with finite f16 fields + the edge blocks ---
        n = 248
        blocks = rng.integers(0, 256, size=(n, ts), dtype=np.uint8)
        for f in range(N_F16[name]):
            d = rng.uniform(-2.0, 2.0, size=n).astype(np.float16)
            blocks[:, 2*f:2*f + 2] = d.view(np.uint8).reshape(-1, 2)
        blocks = np.concatenate([blocks, edge_blocks(name, ts, rng)], axis=0)
        expected = gguf.quants.dequantize(blocks, qt).astype(np.float32)
        assert expected.shape == (blocks.shape[0], bs) and np.isfinite(expected).all(), name
        np.savez_compressed(OUT / f"dequant_{name}.npz", blocks=blocks, expected=expected)

        # --- quantizer goldens (make_golden.py's rows, more of them) ---
        k = 256
        x = rng.standard_normal((32, k)).astype(np.float32)
        x[0, :] = 0                                                        # zero blocks
        x[1, :] = (0.1 + 2*np.cos(np.arange(k, dtype=np.float32) + 0.0)).astype(np.float32)
        x[2, :] = (0.1 + 2*np.cos(np.arange(k, dtype=np.float32) + 1.0)).astype(np.float32)
        x[3, :] *= 1e-6
        x[4, :] *= 1e4
        x[5, :32] = np.linspace(-1, 1, 32, dtype=np.float32)               # ties / symmetric extrema
        x[5, 32:64] = -x[5, :32]
        x[6, :] = 0.75                                                     # constant blocks: Q5_1's d = 0
        x[7, :] = rng.uniform(-1, 1, size=k).astype(np.float32)            # the GPU tests' weight distribution
        x[8, :] = np.abs(x[8, :])                                          # positive only: Q5_0's d < 0
        q = gguf.quants.quantize(x, qt)
        assert q.shape == (32, k//bs*ts)
        back = gguf.quants.dequantize(q, qt)
        assert back.shape == x.shape and np.isfinite(back).all()
        np.savez_compressed(OUT / f"quant_{name}.npz", x=x, expected=q)
    print("Q5_0 / Q5_1 golden vectors written to", OUT)


if __name__ == "__main__":
    main()
