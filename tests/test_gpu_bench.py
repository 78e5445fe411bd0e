"""bench.py's plain run (no --full): one JSON line with the headline only, and --dump-outputs writes the logits the timed path returned in
its last timed step — the same logits a single process gets from the same model and token ids."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle as orc
from gpu_util import backend, pkg

pytestmark = pytest.mark.gpu
ls = pkg.llama_synth
ROOT = Path(__file__).resolve().parent.parent


def test_plain_bench_dumps_the_last_timed_step(tmp_path):
    K, W = 12, 4
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--model", "tiny4",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == K and d["warmup"] == W and d["value"] > 0 and d["unit"] == "tok/s" and d["higher_is_better"] is True
    assert abs(d["ms_per_step"] - 1e3 / d["value"]) <= 1e-3 * d["ms_per_step"] + 1e-3
    assert d["roofline"] is None and d["cpu_baseline"] is None and "kernels_per_token" not in d
    got = np.load(out / "logits.npy")
    # bench.py's inputs: the synthetic weights of seed 1 and the token ids of default_rng(1); the timed steps start on an empty cache
    tokens = np.random.default_rng(1).integers(0, ls.MODELS["tiny4"]["n_vocab"], size=max(K, W) + 8).astype(np.int32)
    be = backend(); be.set_option("graphs", 1); be.set_option("fusion", 1)
    m = ls.SynthLlama(be, "tiny4", "Q4_K_M", n_ctx=128, seed=1)
    try:
        for t in tokens[:K]:
            want = m.decode([int(t)])
    finally:
        m.free()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert orc.nmse(want, got) <= 1e-9
