#!/usr/bin/env python3
"""kv_shift_perf.py — time one K-shift graph of a quantized cache (build_graph_shift: per layer ggml_cast -> ggml_rope_ext -> ggml_cpy back into the view)
with hipEvents round graph_compute, fused (one in-place launch per layer) against node by node (three launches per layer) in the same process,
alternating. Default shape: Llama-3-8B with -ctk q8_0 — 32 layers, 8 KV heads of 128, 8192 cells.

    python tools/kv_shift_perf.py [--layers 32] [--heads 8] [--hd 128] [--cells 8192] [--type q8_0] [--reps 10] [--out FILE]

Prints one JSON line: the median and the spread of both times, the launches per graph and the bytes the fused launches must move (every block read
once and written once). Needs an MI355X: there is no other path."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "oracle"))
import graft_pkg      # noqa: E402
import oracle as orc  # noqa: E402

gg = graft_pkg.load().ggml


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32); ap.add_argument("--heads", type=int, default=8); ap.add_argument("--hd", type=int, default=128)
    ap.add_argument("--cells", type=int, default=8192); ap.add_argument("--type", default="q8_0", choices=["q8_0", "q4_0"])
    ap.add_argument("--mode", type=int, default=0, help="0 NORM, 2 NEOX"); ap.add_argument("--reps", type=int, default=10); ap.add_argument("--out")
    a = ap.parse_args()
    qt = {"q8_0": gg.Q8_0, "q4_0": gg.Q4_0}[a.type]
    L = gg.base()
    be = gg.Backend(0)
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p(be.stream())

    def check(rc):
        assert rc == 0, f"HIP error {rc}"
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        check(hip.hipEventCreate(C.byref(e)))

    n_embd = a.heads * a.hd
    rs_h, rs_row = orc.row_size(qt, a.hd), orc.row_size(qt, n_embd)
    rng = np.random.default_rng(0)
    ctx = gg.Context()
    k_shift = ctx.new_tensor(gg.I32, (a.cells,))
    caches, outs = [], []
    for _ in range(a.layers):
        cache = ctx.new_tensor(qt, (n_embd, a.cells)); caches.append(cache)
        view = L.ggml_view_3d(ctx.ctx, cache, a.hd, a.heads, a.cells, rs_h, rs_row, 0)
        tmp = L.ggml_rope_ext(ctx.ctx, L.ggml_cast(ctx.ctx, view, gg.F32), k_shift, None, a.hd, a.mode, 8192, 500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        outs.append(L.ggml_cpy(ctx.ctx, tmp, view))
    assert all(be.supports_op(o) for o in outs)
    assert ctx.alloc(be)
    graph = ctx.new_graph(size=8 * a.layers + 16)
    for o in outs:
        L.ggml_build_forward_expand(graph, o)
    gg.tensor_set(k_shift, np.full((1, 1, 1, a.cells), -256, np.int32))      # a discard of 256 cells in front of all of them
    one = orc.random_blocks(rng, qt, (1, 1, a.cells), n_embd)
    for t in caches:
        gg.tensor_set(t, one)

    be.set_option("graphs", 0)      # a shift graph runs once between decode steps: the eager pass is what a user waits for
    times, launches = {1: [], 0: []}, {}
    for rep in range(a.reps + 2):      # two warm-up rounds (code objects), then alternating
        for fusion in (1, 0):
            be.set_option("fusion", fusion); be.reset_counters()
            check(hip.hipEventRecord(ev[0], stream))
            assert be.compute_async(graph) == gg.GGML_STATUS_SUCCESS
            check(hip.hipEventRecord(ev[1], stream))
            check(hip.hipEventSynchronize(ev[1]))
            ms = C.c_float()
            check(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
            launches[fusion] = be.counters()["kernels_launched"]
            if rep >= 2:
                times[fusion].append(ms.value)
    be.set_option("fusion", 1); be.set_option("graphs", 1)
    moved = 2 * a.layers * a.cells * rs_row
    res = {"shape": {"layers": a.layers, "n_head_kv": a.heads, "hd": a.hd, "kv_size": a.cells, "type": a.type, "mode": a.mode}, "reps": a.reps,
           "fused_ms": {"median": statistics.median(times[1]), "min": min(times[1]), "max": max(times[1]), "launches": launches[1]},
           "nodes_ms": {"median": statistics.median(times[0]), "min": min(times[0]), "max": max(times[0]), "launches": launches[0]},
           "fused_bytes_moved": moved, "fused_gb_per_s": moved / (statistics.median(times[1]) * 1e-3) / 1e9}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")
    ctx.free(); be.free()


if __name__ == "__main__":
    main()
