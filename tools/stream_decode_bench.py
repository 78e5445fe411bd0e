"""stream_decode_bench.py — decode over per-sequence KV streams: one ubatch with a token of every sequence (SynthLlama.decode_batch, one graph, the weights read
once per step) against the same tokens as n_stream successive one-sequence steps (decode(seq=s), the weights read once per sequence).

Llama-3-8B-shaped Q4_K_M, n_stream sequences at depth `--depth`, one token per sequence and step. Protocol: every repetition re-prompts all sequences to the
depth (so both forms always run at the same depth), warms both forms' graphs up once, then times `--steps` steps of each, alternating the two forms between
repetitions; every step ends in a device synchronise (llama-bench's per-token llama_synchronize). Reported: aggregate tok/s = n_stream * steps / time, best
and median over the repetitions. On a tree without decode_batch only the sequential form is measured. One JSON line per n_stream."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graft_pkg

ap = argparse.ArgumentParser()
ap.add_argument("--streams", default="1,2,4,8")
ap.add_argument("--depth", type=int, default=512)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--fa", type=int, default=0)
ap.add_argument("--model", default="llama3-8b")
args = ap.parse_args()

pkg = graft_pkg.load(); gg, ls = pkg.ggml, pkg.llama_synth
be = gg.Backend(0)
be.set_option("graphs", 1); be.set_option("fusion", 1)
rng = np.random.default_rng(1)
for S in [int(x) for x in args.streams.split(",")]:
    m = ls.SynthLlama(be, args.model, "Q4_K_M", n_ctx=args.depth + 2 * args.steps + 64, seed=1, n_seq_max=S, flash_attn=bool(args.fa))
    n_vocab = m.cfg["n_vocab"]
    prompt = rng.integers(0, n_vocab, size=(S, args.depth)).astype(np.int32)
    toks = rng.integers(0, n_vocab, size=(args.steps + 1, S, 1)).astype(np.int32)
    forms = [f for f in ("batch", "seq") if (f != "batch" or hasattr(m, "decode_batch"))]
    rate = {f: [] for f in forms}

    def step(form, i):
        if form == "batch":
            m.decode_batch(toks[i], want_host=True, sync=True)
        else:
            for s in range(S):
                m.decode(toks[i, s], seq=s, want_host=True, sync=True, view=True)
    for rep in range(args.reps):
        for form in (forms if rep % 2 == 0 else forms[::-1]):
            m.kv_clear()
            for s in range(S):
                m.decode(prompt[s], seq=s, want_host=False, sync=True)
            step(form, args.steps)                              # warm-up: the form's graph at this n_kv bucket is built and captured outside the window
            step(form, args.steps)
            be.synchronize(); t0 = time.perf_counter()
            for i in range(args.steps):
                step(form, i)
            be.synchronize(); dt = time.perf_counter() - t0
            rate[form].append(S * args.steps / dt)
    out = {"model": args.model, "ftype": "Q4_K_M", "fa": args.fa, "n_stream": S, "depth": args.depth, "steps": args.steps, "reps": args.reps}
    for f in forms:
        out[f + "_tok_s_best"] = round(max(rate[f]), 1); out[f + "_tok_s_median"] = round(float(np.median(rate[f])), 1)
    print(json.dumps(out), flush=True)
    m.free()
be.free()
