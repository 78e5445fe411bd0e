"""GPU parity for Q3_K weights — the default type of every Q3_K_S / _M / _L file (src/llama-quant.cpp:553-555: wq, wk, ffn_gate, ffn_up, Mixtral's
expert stacks) — in MUL_MAT and MUL_MAT_ID, through the backend's C-ABI.

The oracle knows six formats; this file carries its own reference: tests/test_q3_k_format.py's numpy dequantizer (pinned bit for bit against
the golden vectors there) and its block generator random_q3_k — gguf-py has no Q3_K quantizer, and generated blocks reach every bit pattern,
negative scales included, which a quantizer's output would not. Expected values = dequant(W) @ X in float64; gate for one mat-mul = the
reference's MUL_MAT gate NMSE <= 5e-4 (tests/test-backend-ops.cpp:3106-3108). On such blocks (scale 1/128, X ~ U(-1, 1)) the CPU arithmetic
alone sits at 2.3e-5 .. 3.6e-5 (Q8_K-rounded activations, worst column) and the bf16 tile arithmetic at <= 1.5e-5.
Every case first asserts supports_op.

Shapes (the smallest at which each path can go wrong):
  k = 256 (one block), 768 (three: an odd count, a wave's tail, row starts alternating between 4-byte aligned and 2 off), 1024 (four streamed
  units), 1280 (five);
  m = 1, 33, 130 (one row, a row tail, more than one 128-row prefill tile);
  n = 1 (streamed / simple decode kernel; fusion off: the simple kernel at every k), 2, 5, 8 (the column forms), 9, 33, 130 (prefill tiles
  with row and column tails).
"""
import numpy as np
import pytest

import oracle as orc
from gpu_util import backend, gg, run_mul_mat, run_mul_mat_bcast
from test_q3_k_format import dequant_q3_k, random_q3_k

pytestmark = pytest.mark.gpu
L = gg.base()

GATE = 5e-4
GRAPH_GATE = 2e-3       # the reference's whole-graph gate (tests/test-backend-ops.cpp:4991-4993), as tests/test_gpu_llama_graph.py uses it
Q3_K, Q2_K = 11, 10     # enum ggml_type (spelled out, so that without the format a case fails at its supports_op assertion, not at import)
OTHER = {"q4_K": 12, "q5_K": 13, "q6_K": 14}


def nmse(expected, got):
    e = np.asarray(expected, np.float64); g = np.asarray(got, np.float64)
    return float(((e - g)**2).sum() / ((e**2).sum() + 1e-300))


def weights(rng, shape, k, scale=1/128):
    """generated Q3_K rows [*shape, row_bytes] u8 and their dequantization [*shape, k] f64"""
    w = random_q3_k(rng, shape, k, scale)
    return w, dequant_q3_k(w).astype(np.float64)


def weights_of(rng, name, shape, k, scale):
    """(type id, bytes, f64 values) of a weight in Q3_K or — the oracle's generator and dequantizer — one of the other K-quants"""
    if name == "q3_K":
        w, wd = weights(rng, shape, k, scale/58)          # (a generated block's values have rms ~58 d)
        return Q3_K, w, wd
    w = orc.random_blocks(rng, OTHER[name], shape, k, scale=3.0*scale)
    return OTHER[name], w, orc.dequantize(w, OTHER[name]).astype(np.float64)


def probe(k, m, n):
    """what llama.cpp asks at load time (and what fails without the format)"""
    be = backend()
    with gg.Context() as ctx:
        out = L.ggml_mul_mat(ctx.ctx, ctx.new_tensor(Q3_K, [k, m]), ctx.new_tensor(gg.F32, [k, n]))
        assert be.supports_op(out), "q3_K: MUL_MAT refused"


@pytest.mark.parametrize("m", [1, 33, 130])
@pytest.mark.parametrize("k", [256, 768, 1024, 1280])
def test_mul_mat(k, m):
    probe(k, m, 512)
    rng = np.random.default_rng(1000*k + m)
    w, wd = weights(rng, (m,), k)
    xs = rng.uniform(-1, 1, size=(130, k)).astype(np.float32)
    be = backend()
    for n in (1, 2, 5, 8, 9, 33, 130):
        x = xs[:n]
        exp = x.astype(np.float64) @ wd.T
        for fusion in ((1, 0) if n == 1 else (1,)):
            be.set_option("fusion", fusion)
            try:
                got = run_mul_mat(Q3_K, w, x, m, k)
            finally:
                be.set_option("fusion", 1)
            e = nmse(exp, got)
            print(f"q3_K k={k} m={m} n={n} fusion={fusion}: NMSE {e:.3g}")
            assert np.isfinite(got).all() and e <= GATE, (k, m, n, fusion, e)


@pytest.mark.parametrize("k,m", [(4096, 300), (14336, 4096)])
def test_mul_mat_one_column_at_model_row_lengths(k, m):
    """the streamed kernel where its other branches run: k / 256 = 16 units per row (the 16-lane row reduction), and the ffn_down shape whose workgroups
    stream more slots than the LDS ring holds, so that slots are reused. (The 4096 rows are 256 generated rows tiled.)"""
    probe(k, m, 512)
    rng = np.random.default_rng(k + m)
    base, based = weights(rng, (min(m, 256),), k)
    reps = -(-m // base.shape[0])
    w = np.tile(base, (reps, 1))[:m]; wd = np.tile(based, (reps, 1))[:m]
    x = rng.uniform(-1, 1, size=(1, k)).astype(np.float32)
    got = run_mul_mat(Q3_K, w, x, m, k)
    e = nmse(x.astype(np.float64) @ wd.T, got)
    print(f"q3_K k={k} m={m} n=1: NMSE {e:.3g}")
    assert np.isfinite(got).all() and e <= GATE


def test_one_column_runs_on_the_streamed_kernel():
    """the decode launch is the streamed kernel's instantiation for the format (DESIGN.md §4 has the measurement behind that route)"""
    probe(1024, 130, 1)
    rng = np.random.default_rng(4)
    be = backend()
    m, k = 130, 1024
    be.set_option("graphs", 0); be.set_option("fusion", 1); be.set_option("profile", 1)
    try:
        w, wd = weights(rng, (m,), k)
        x = rng.uniform(-1, 1, size=(1, k)).astype(np.float32)
        got = run_mul_mat(Q3_K, w, x, m, k)
        assert nmse(x.astype(np.float64) @ wd.T, got) <= GATE
        prof = [e for e in be.profile(64) if e["type"] == Q3_K]
    finally:
        be.set_option("profile", 0); be.set_option("graphs", 1)
    grouped = {e["k"]: e["kernel"] for e in prof if e["m"] < 0}
    assert grouped.get(1024, "").startswith("k_mmvq_stream<11, 11,"), prof


@pytest.mark.parametrize("n", [1, 3, 40])
def test_mul_mat_f16_src1(n):
    """tests/test-backend-ops.cpp:5715-5716: F16 activations"""
    rng = np.random.default_rng(77 + n)
    m, k = 33, 768
    be = backend()
    w, wd = weights(rng, (m,), k)
    x16 = rng.uniform(-1, 1, size=(n, k)).astype(np.float16)
    with gg.Context() as ctx:
        a = ctx.new_tensor(Q3_K, [k, m]); b = ctx.new_tensor(gg.F16, [k, n])
        out = L.ggml_mul_mat(ctx.ctx, a, b)
        assert be.supports_op(out)
        assert ctx.alloc(be)
        gg.tensor_set(a, w); gg.tensor_set(b, x16)
        be.compute(gg.graph_of(ctx, out))
        got = gg.tensor_get(out)[0, 0].copy()
    e = nmse(x16.astype(np.float64) @ wd.T, got)
    print(f"q3_K f16 src1 n={n}: NMSE {e:.3g}")
    assert np.isfinite(got).all() and e <= GATE


@pytest.mark.parametrize("n", [1, 3])
def test_mul_mat_broadcast(n):
    """ne02 = 2, ne12 = 4: dst[.., i2] = a[.., i2 / 2] . b[.., i2] — the batched mat-vec launch"""
    rng = np.random.default_rng(5 + n)
    m, k, bs, nr = 33, 768, (2, 1), (2, 1)
    w, wd = weights(rng, (1, 2, m), k)
    x = rng.uniform(-1, 1, size=(1, 4, n, k)).astype(np.float32)
    with gg.Context() as ctx:
        assert backend().supports_op(L.ggml_mul_mat(ctx.ctx, ctx.new_tensor(Q3_K, [k, m, 2, 1]), ctx.new_tensor(gg.F32, [k, n, 4, 1])))
    got = run_mul_mat_bcast(Q3_K, w, x, m, k, bs, nr)
    assert got.shape == (1, 4, n, m)
    for i2 in range(4):
        e = nmse(x[0, i2].astype(np.float64) @ wd[0, i2 // 2].T, got[0, i2])
        print(f"q3_K broadcast n={n} batch {i2}: NMSE {e:.3g}")
        assert e <= GATE


@pytest.mark.parametrize("k,n", [(1024, 1), (768, 4), (768, 40)])
def test_mul_mat_twice_is_bitwise_equal(k, n):
    """the same graph computed twice with graph capture on: the second compute replays the captured launches"""
    rng = np.random.default_rng(k + n)
    m = 130
    be = backend()
    w, wd = weights(rng, (m,), k)
    x = rng.uniform(-1, 1, size=(n, k)).astype(np.float32)
    be.set_option("graphs", 1); be.set_option("fusion", 1)
    with gg.Context() as ctx:
        a = ctx.new_tensor(Q3_K, [k, m]); b = ctx.new_tensor(gg.F32, [k, n])
        out = L.ggml_mul_mat(ctx.ctx, a, b)
        assert be.supports_op(out)
        assert ctx.alloc(be)
        gg.tensor_set(a, w); gg.tensor_set(b, x)
        graph = gg.graph_of(ctx, out)
        be.compute(graph); first = gg.tensor_get(out)[0, 0].copy()
        L.ggml_backend_tensor_memset(out, 0xFF, 0, L.ggml_nbytes(out))
        be.compute(graph); second = gg.tensor_get(out)[0, 0].copy()
    assert nmse(x.astype(np.float64) @ wd.T, first) <= GATE
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))


@pytest.mark.parametrize("n_tokens", [1, 3, 35])
@pytest.mark.parametrize("k", [768, 1024])
def test_mul_mat_id(k, n_tokens):
    """4 experts, 2 used; ids = a strided view of a shuffled [n_expert, n_tokens] tensor (tests/test-backend-ops.cpp:3231-3236).
    One token: decode pairs (the grouped launch over the expert stack where the streamed kernel takes it); 3 tokens: the mat-vec _id form;
    35 tokens: 70 pairs sorted by expert through the prefill tiles."""
    rng = np.random.default_rng(31*k + n_tokens)
    n_expert, n_used, m = 4, 2, 33
    be = backend()
    w, wd = weights(rng, (n_expert, m), k)
    ids_full = np.stack([rng.permutation(n_expert) for _ in range(n_tokens)]).astype(np.int32)
    b_ = rng.uniform(-1, 1, size=(1, n_tokens, n_used, k)).astype(np.float32)
    exp = np.einsum("tumk,tuk->tum", wd[ids_full[:, :n_used]], b_[0].astype(np.float64))
    for fusion in (1, 0):
        be.set_option("fusion", fusion)
        try:
            with gg.Context() as ctx:
                as_ = ctx.new_tensor(Q3_K, (k, m, n_expert)); ids = ctx.new_tensor(gg.I32, (n_expert, n_tokens)); b = ctx.new_tensor(gg.F32, (k, n_used, n_tokens))
                idv = L.ggml_view_2d(ctx.ctx, ids, n_used, n_tokens, n_expert*4, 0)
                out = L.ggml_mul_mat_id(ctx.ctx, as_, b, idv)
                assert be.supports_op(out), "q3_K: MUL_MAT_ID refused"
                assert ctx.alloc(be)
                gg.tensor_set(as_, w); gg.tensor_set(ids, ids_full.reshape(1, 1, n_tokens, n_expert)); gg.tensor_set(b, b_)
                be.compute(gg.graph_of(ctx, out))
                got = gg.tensor_get(out)[0].copy()
        finally:
            be.set_option("fusion", 1)
        e = nmse(exp, got)
        print(f"q3_K MUL_MAT_ID k={k} tokens={n_tokens} fusion={fusion}: NMSE {e:.3g}")
        assert got.shape == exp.shape and np.isfinite(got).all() and e <= GATE


def _ffn_f64(x, wn, wg, wu, wd, eps):
    x = x.astype(np.float64)
    h = x / np.sqrt((x*x).mean(axis=-1, keepdims=True) + eps) * wn.astype(np.float64)
    g = h @ wg.T; u = h @ wu.T
    return (g / (1.0 + np.exp(-g)) * u) @ wd.T + x


@pytest.mark.parametrize("T", [1, 4, 40])
@pytest.mark.parametrize("down", ["q3_K", "q4_K"])
@pytest.mark.parametrize("n_embd,n_ff", [(256, 768), (1024, 2048)])
def test_ffn_subgraph_fused_and_unfused(n_embd, n_ff, down, T):
    """RMS_NORM -> MUL(weight) -> gate / up MUL_MAT (Q3_K) -> GLU(swiglu) -> down MUL_MAT (Q3_K, or Q4_K: the Q3_K_M mix) -> ADD(residual), with
    the fusion pass on and off: a matcher that routed the format into a launcher without it would abort or disagree. Weights of rms ~1/sqrt(k), so
    that the activations stay of order one. Both runs within the whole-graph gate 2e-3 against float64 (not 5e-4: the CPU arithmetic alone — Q8_K
    rounding of the normed input and of the heavy-tailed SwiGLU product — is 2.1e-4 .. 3.5e-4 on these shapes), and within 5e-4 of each other.
    (The Q4_K down weight comes from the oracle's block generator and dequantizer: the oracle has no Q4_K quantizer.)"""
    rng = np.random.default_rng(n_embd + T)
    be = backend()
    x = rng.standard_normal((T, n_embd)).astype(np.float32)
    wn = rng.uniform(0.5, 1.5, size=(n_embd,)).astype(np.float32)
    wg, wgd = weights(rng, (n_ff,), n_embd, 1/(48*np.sqrt(n_embd))); wu, wud = weights(rng, (n_ff,), n_embd, 1/(48*np.sqrt(n_embd)))
    if down == "q3_K":
        td = Q3_K; wd, wdd = weights(rng, (n_embd,), n_ff, 1/(48*np.sqrt(n_ff)))
    else:
        td, wd, wdd = weights_of(rng, down, (n_embd,), n_ff, 1/np.sqrt(n_ff))
    exp = _ffn_f64(x, wn, wgd, wud, wdd, 1e-5)
    res = {}
    for fusion in (1, 0):
        be.set_option("fusion", fusion)
        try:
            with gg.Context() as ctx:
                xt = ctx.new_tensor(gg.F32, (n_embd, T)); wt = ctx.new_tensor(gg.F32, (n_embd,))
                g_ = ctx.new_tensor(Q3_K, (n_embd, n_ff)); u_ = ctx.new_tensor(Q3_K, (n_embd, n_ff)); d_ = ctx.new_tensor(td, (n_ff, n_embd))
                nm = L.ggml_mul(ctx.ctx, L.ggml_rms_norm(ctx.ctx, xt, 1e-5), wt)
                gate = L.ggml_mul_mat(ctx.ctx, g_, nm); up = L.ggml_mul_mat(ctx.ctx, u_, nm)
                assert be.supports_op(gate) and be.supports_op(up)
                act = L.ggml_swiglu_split(ctx.ctx, gate, up)
                down_t = L.ggml_mul_mat(ctx.ctx, d_, act)
                assert be.supports_op(down_t)
                out = L.ggml_add(ctx.ctx, down_t, xt)
                assert ctx.alloc(be)
                gg.tensor_set(xt, x.reshape(1, 1, T, n_embd)); gg.tensor_set(wt, wn.reshape(1, 1, 1, n_embd))
                gg.tensor_set(g_, wg); gg.tensor_set(u_, wu); gg.tensor_set(d_, wd)
                be.compute(gg.graph_of(ctx, out))
                res[fusion] = gg.tensor_get(out)[0, 0].copy()
        finally:
            be.set_option("fusion", 1)
    e1, e0, e10 = nmse(exp, res[1]), nmse(exp, res[0]), nmse(res[0], res[1])
    print(f"FFN {n_embd}/{n_ff} down={down} T={T}: NMSE fused {e1:.3g}, unfused {e0:.3g}, fused vs unfused {e10:.3g}")
    assert np.isfinite(res[1]).all() and np.isfinite(res[0]).all()
    assert e1 <= GRAPH_GATE and e0 <= GRAPH_GATE
    assert e10 <= 5e-4


@pytest.mark.parametrize("k", [768, 1024])
@pytest.mark.parametrize("third", ["q3_K", "q4_K", "q5_K", "q6_K"])
def test_mat_vecs_on_one_normed_activation(third, k):
    """RMS_NORM -> MUL(weight) -> three mat-vecs that read the product (wq / wk / wv of a decode step), wq and wk in Q3_K: with the fusion pass on,
    wv in Q3_K, Q4_K or Q5_K (the Q3_K_M / _L mixes) shares ONE grouped streamed launch with them — asserted through the profile at k = 1024 for the
    two mixed pairs — and wv in Q6_K, a pair without a common kernel, splits it."""
    types = ("q3_K", "q3_K", third)
    rng = np.random.default_rng(k + sum(map(ord, third)))
    be = backend()
    ms = (130, 66, 34)
    x = rng.standard_normal((1, k)).astype(np.float32); wn = rng.uniform(0.5, 1.5, size=(k,)).astype(np.float32)
    ws = [weights_of(rng, t, (m,), k, 1/np.sqrt(k)) for t, m in zip(types, ms)]
    h = x.astype(np.float64) / np.sqrt((x.astype(np.float64)**2).mean() + 1e-5) * wn
    check_route = k == 1024 and third in ("q4_K", "q5_K")
    res = {}; prof = []
    for fusion in (1, 0):
        be.set_option("fusion", fusion)
        if fusion and check_route:
            be.set_option("graphs", 0); be.set_option("profile", 1)
        try:
            with gg.Context() as ctx:
                xt = ctx.new_tensor(gg.F32, (k, 1)); wt = ctx.new_tensor(gg.F32, (k,))
                wts = [ctx.new_tensor(t, (k, m)) for (t, _, _), m in zip(ws, ms)]
                nm = L.ggml_mul(ctx.ctx, L.ggml_rms_norm(ctx.ctx, xt, 1e-5), wt)
                outs = [L.ggml_mul_mat(ctx.ctx, w_, nm) for w_ in wts]
                assert all(be.supports_op(o) for o in outs)
                assert ctx.alloc(be)
                gg.tensor_set(xt, x); gg.tensor_set(wt, wn.reshape(1, k))
                for w_, (_, wb, _) in zip(wts, ws):
                    gg.tensor_set(w_, wb)
                be.compute(gg.graph_of(ctx, *outs))
                res[fusion] = [gg.tensor_get(o)[0, 0, 0].copy() for o in outs]
            if fusion and check_route:
                prof = be.profile(64)
        finally:
            be.set_option("fusion", 1)
            if fusion and check_route:
                be.set_option("profile", 0); be.set_option("graphs", 1)
    for i, (_, _, wd) in enumerate(ws):
        exp = (h @ wd.T)[0]
        e1, e0 = nmse(exp, res[1][i]), nmse(exp, res[0][i])
        print(f"{types} k={k} mat-vec {i}: NMSE fused {e1:.3g}, unfused {e0:.3g}")
        assert e1 <= GATE and e0 <= GATE and nmse(res[0][i], res[1][i]) <= 5e-4
    if check_route:
        grouped = [e["kernel"] for e in prof if e["m"] < 0 and e["k"] == k]
        assert len(grouped) == 1 and grouped[0].startswith(f"k_mmvq_stream<11, {OTHER[third]},"), prof


def test_refusals():
    """Q2_K has no kernel, and a Q3_K row that is not whole 256-element blocks cannot exist: supports_op says so and llama.cpp keeps those weights on the CPU"""
    be = backend()
    k, m, n_expert, n_used = 1024, 64, 4, 2
    with gg.Context() as ctx:
        assert be.supports_op(L.ggml_mul_mat(ctx.ctx, ctx.new_tensor(Q3_K, [k, m]), ctx.new_tensor(gg.F32, [k, 1]))), "q3_K: MUL_MAT refused"
        for n in (1, 512):
            assert not be.supports_op(L.ggml_mul_mat(ctx.ctx, ctx.new_tensor(Q2_K, [k, m]), ctx.new_tensor(gg.F32, [k, n])))
        op = L.ggml_mul_mat_id(ctx.ctx, ctx.new_tensor(Q2_K, [k, m, n_expert]), ctx.new_tensor(gg.F32, [k, n_used, 4]), ctx.new_tensor(gg.I32, [n_used, 4]))
        assert not be.supports_op(op)
        # ne[0] = 288 is no multiple of the block size: the tensor is described by hand (ggml_new_tensor asserts on such a row)
        a = ctx.new_tensor(Q3_K, [256, m])
        a.contents.ne[0] = 288
        for n in (1, 512):
            assert not be.supports_op(L.ggml_mul_mat(ctx.ctx, a, ctx.new_tensor(gg.F32, [288, n])))
