"""GPU parity for the weight formats the oracle does not know, in MUL_MAT and MUL_MAT_ID, through the backend's C-ABI — the case bodies, written once with
the format a parameter (a helper like gpu_util.py, not a test file). tests/test_gpu_q5_weights.py and tests/test_gpu_q3_k_weights.py hold the parameter lines — which
formats, row lengths, seeds and mixes — and nothing else:

  q5_0, q5_1  the 32-element formats llama_tensor_get_type writes in place of Q4_K / Q5_K when a row is not a multiple of 256 long
              (src/llama-quant.cpp:436-470)
  q3_K        the default type of every Q3_K_S / _M / _L file (src/llama-quant.cpp:553-555: wq, wk, ffn_gate, ffn_up, Mixtral's expert stacks)

The oracle knows six formats (tests/test_gpu_mul_mat.py checks those against its integer path); the reference here is tests/weight_formats.py: numpy
dequantizers pinned bit for bit against golden vectors (tests/test_q5_formats.py, tests/test_q3_k_format.py), weights = quant(U(-1, 1)) for q5_0 / q5_1 and
generated blocks for q3_K (gguf-py has no Q3_K quantizer, and generated blocks reach every bit pattern, negative scales included, which a quantizer's
output would not), fixed seeds. Expected values = dequant(W) @ X in float64; gate for one mat-mul = the reference's MUL_MAT gate NMSE <= 5e-4
(tests/test-backend-ops.cpp:3106-3108). On generated Q3_K blocks (scale 1/128, X ~ U(-1, 1)) the CPU arithmetic alone sits at 2.3e-5 .. 3.6e-5 (Q8_K-rounded
activations, worst column) and the bf16 tile arithmetic at <= 1.5e-5. Every case first asserts supports_op.

Shapes (the smallest at which each path can go wrong):
  k, 32-element formats: 32 (one block), 288 (nine blocks: k % 256 != 0, odd block count, a wave's tail), 1024 (four streamed units), 1280 (five: odd);
  k, q3_K: 256 (one block), 768 (three: an odd count, a wave's tail, row starts alternating between 4-byte aligned and 2 off), 1024, 1280;
  m = 1, 33, 130 (fewer rows than a workgroup's waves x 2, a row tail, more than one 128-row prefill tile);
  n = 1 (streamed / simple decode kernel; fusion off: the simple kernel at every k), 2, 5, 8 (the column forms), 9, 33, 130 (prefill tiles
  with row and column tails).

Adding a format: its id in QT here, and a file of parameter lines like the two above.
"""
import numpy as np
from gpu_util import backend, gg, run_mul_mat, run_mul_mat_bcast
from weight_formats import ffn_f64, nmse, probe, weights

L = gg.base()

GATE = 5e-4
GRAPH_GATE = 2e-3       # the reference's whole-graph gate (tests/test-backend-ops.cpp:4991-4993), as tests/test_gpu_llama_graph.py uses it
# enum ggml_type, spelled out, so that without a format a case fails at its supports_op assertion, not at import
QT = {"q5_0": 6, "q5_1": 7, "q3_K": 11, "q4_K": 12, "q5_K": 13, "q6_K": 14}
BLOCK32 = ("q5_0", "q5_1")      # blocks of 32 elements: rows need not be whole 256-weight units, and the weights are quant(U(-1, 1)) whatever the chain


def check_mul_mat(name, k, m):
    probe(QT[name], k, m, 512)
    rng = np.random.default_rng(1000*k + m)
    w, wd = weights(rng, name, (m,), k)
    xs = rng.uniform(-1, 1, size=(130, k)).astype(np.float32)
    be = backend()
    for n in (1, 2, 5, 8, 9, 33, 130):
        x = xs[:n]
        exp = x.astype(np.float64) @ wd.T
        for fusion in ((1, 0) if n == 1 else (1,)):
            be.set_option("fusion", fusion)
            try:
                got = run_mul_mat(QT[name], w, x, m, k)
            finally:
                be.set_option("fusion", 1)
            e = nmse(exp, got)
            print(f"{name} k={k} m={m} n={n} fusion={fusion}: NMSE {e:.3g}")
            assert np.isfinite(got).all() and e <= GATE, (name, k, m, n, fusion, e)


def check_mul_mat_one_column_at_model_row_lengths(name, k, m):
    """the streamed kernel where its other branches run: k / 256 = 16 units per row (the 16-lane row reduction), and the ffn_down shape whose workgroups
    stream more slots than the LDS ring holds, so that slots are reused. (The 4096 rows are 256 rows repeated: the numpy quantizer is the slow part.)"""
    probe(QT[name], k, m, 512)
    rng = np.random.default_rng(k + m)
    base, based = weights(rng, name, (min(m, 256),), k)
    reps = -(-m // base.shape[0])
    w = np.tile(base, (reps, 1))[:m]; wd = np.tile(based, (reps, 1))[:m]
    x = rng.uniform(-1, 1, size=(1, k)).astype(np.float32)
    got = run_mul_mat(QT[name], w, x, m, k)
    e = nmse(x.astype(np.float64) @ wd.T, got)
    print(f"{name} k={k} m={m} n=1: NMSE {e:.3g}")
    assert np.isfinite(got).all() and e <= GATE


def check_one_column_runs_on_the_streamed_kernel(name, ks):
    """k % 256 == 0: the decode launch is the streamed kernel's instantiation for the format (DESIGN.md §4 has the measurement behind that route);
    k % 256 != 0 (ks holds 288: a row length only the 32-element formats have): it declines and the generic kernel runs (no grouped-launch record)."""
    t, m = QT[name], 130
    probe(t, 1024, m, 1)
    rng = np.random.default_rng(4)
    be = backend()
    be.set_option("graphs", 0); be.set_option("fusion", 1); be.set_option("profile", 1)
    try:
        for k in ks:
            w, wd = weights(rng, name, (m,), k)
            x = rng.uniform(-1, 1, size=(1, k)).astype(np.float32)
            got = run_mul_mat(t, w, x, m, k)
            assert nmse(x.astype(np.float64) @ wd.T, got) <= GATE
        prof = [e for e in be.profile(64) if e["type"] == t]
    finally:
        be.set_option("profile", 0); be.set_option("graphs", 1)
    grouped = {e["k"]: e["kernel"] for e in prof if e["m"] < 0}
    assert grouped.get(1024, "").startswith(f"k_mmvq_stream<{t}, {t},"), prof
    if 288 in ks:
        assert 288 not in grouped and any(e["k"] == 288 and e["m"] == m for e in prof), prof


def check_mul_mat_f16_src1(name, k, n):
    """tests/test-backend-ops.cpp:5715-5716: F16 activations"""
    rng = np.random.default_rng(77 + n)
    m = 33
    be = backend()
    w, wd = weights(rng, name, (m,), k)
    x16 = rng.uniform(-1, 1, size=(n, k)).astype(np.float16)
    with gg.Context() as ctx:
        a = ctx.new_tensor(QT[name], [k, m]); b = ctx.new_tensor(gg.F16, [k, n])
        out = L.ggml_mul_mat(ctx.ctx, a, b)
        assert be.supports_op(out)
        assert ctx.alloc(be)
        gg.tensor_set(a, w); gg.tensor_set(b, x16)
        be.compute(gg.graph_of(ctx, out))
        got = gg.tensor_get(out)[0, 0].copy()
    e = nmse(x16.astype(np.float64) @ wd.T, got)
    print(f"{name} f16 src1 n={n}: NMSE {e:.3g}")
    assert np.isfinite(got).all() and e <= GATE


def check_mul_mat_broadcast(name, k, n):
    """ne02 = 2, ne12 = 4: dst[.., i2] = a[.., i2 / 2] . b[.., i2] — the batched mat-vec launch"""
    rng = np.random.default_rng(5 + n)
    m, bs, nr = 33, (2, 1), (2, 1)
    w, wd = weights(rng, name, (1, 2, m), k)
    x = rng.uniform(-1, 1, size=(1, 4, n, k)).astype(np.float32)
    with gg.Context() as ctx:
        assert backend().supports_op(L.ggml_mul_mat(ctx.ctx, ctx.new_tensor(QT[name], [k, m, 2, 1]), ctx.new_tensor(gg.F32, [k, n, 4, 1])))
    got = run_mul_mat_bcast(QT[name], w, x, m, k, bs, nr)
    assert got.shape == (1, 4, n, m)
    for i2 in range(4):
        e = nmse(x[0, i2].astype(np.float64) @ wd[0, i2 // 2].T, got[0, i2])
        print(f"{name} broadcast n={n} batch {i2}: NMSE {e:.3g}")
        assert e <= GATE


def check_mul_mat_twice_is_bitwise_equal(name, k, n):
    """the same graph computed twice with graph capture on: the second compute replays the captured launches"""
    rng = np.random.default_rng(k + n)
    m = 130
    be = backend()
    w, wd = weights(rng, name, (m,), k)
    x = rng.uniform(-1, 1, size=(n, k)).astype(np.float32)
    be.set_option("graphs", 1); be.set_option("fusion", 1)
    with gg.Context() as ctx:
        a = ctx.new_tensor(QT[name], [k, m]); b = ctx.new_tensor(gg.F32, [k, n])
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


def check_mul_mat_id(name, k, n_tokens):
    """4 experts, 2 used; ids = a strided view of a shuffled [n_expert, n_tokens] tensor (tests/test-backend-ops.cpp:3231-3236).
    One token: decode pairs (the grouped launch over the expert stack where the streamed kernel takes it); 3 tokens: the mat-vec _id form;
    35 tokens: 70 pairs sorted by expert through the prefill tiles."""
    rng = np.random.default_rng(31*k + n_tokens)
    n_expert, n_used, m = 4, 2, 33
    be = backend()
    w, wd = weights(rng, name, (n_expert, m), k)
    ids_full = np.stack([rng.permutation(n_expert) for _ in range(n_tokens)]).astype(np.int32)
    b_ = rng.uniform(-1, 1, size=(1, n_tokens, n_used, k)).astype(np.float32)
    exp = np.einsum("tumk,tuk->tum", wd[ids_full[:, :n_used]], b_[0].astype(np.float64))
    for fusion in (1, 0):
        be.set_option("fusion", fusion)
        try:
            with gg.Context() as ctx:
                as_ = ctx.new_tensor(QT[name], (k, m, n_expert)); ids = ctx.new_tensor(gg.I32, (n_expert, n_tokens)); b = ctx.new_tensor(gg.F32, (k, n_used, n_tokens))
                idv = L.ggml_view_2d(ctx.ctx, ids, n_used, n_tokens, n_expert*4, 0)
                out = L.ggml_mul_mat_id(ctx.ctx, as_, b, idv)
                assert be.supports_op(out), f"{name}: MUL_MAT_ID refused"
                assert ctx.alloc(be)
                gg.tensor_set(as_, w); gg.tensor_set(ids, ids_full.reshape(1, 1, n_tokens, n_expert)); gg.tensor_set(b, b_)
                be.compute(gg.graph_of(ctx, out))
                got = gg.tensor_get(out)[0].copy()
        finally:
            be.set_option("fusion", 1)
        e = nmse(exp, got)
        print(f"{name} MUL_MAT_ID k={k} tokens={n_tokens} fusion={fusion}: NMSE {e:.3g}")
        assert got.shape == exp.shape and np.isfinite(got).all() and e <= GATE


def rms_scale(name, k, c=1.0):
    """the scale that gives generated K-quant weights an rms of ~c/sqrt(k), so that a chain's activations stay of order one"""
    return None if name in BLOCK32 else c/np.sqrt(k)


def check_ffn_subgraph_fused_and_unfused(gate_up, down, n_embd, n_ff, gate, T):
    """RMS_NORM -> MUL(weight) -> gate / up MUL_MAT -> GLU(swiglu) -> down MUL_MAT -> ADD(residual), with the fusion pass on and off: a matcher that
    routed a format into a launcher without it would abort or disagree. Both runs within the gate against float64, and within 5e-4 (NMSE) of each other.
    Q5_0 gate / up with Q5_1 down: the one-mat-mul gate 5e-4.
    Q3_K gate / up with Q3_K or Q4_K down (the Q3_K_M mix; the Q4_K weight comes from the oracle's block generator and dequantizer): weights of rms
    ~1/sqrt(k), and the whole-graph gate 2e-3 — not 5e-4: the CPU arithmetic alone — Q8_K rounding of the normed input and of the heavy-tailed SwiGLU
    product — is 2.1e-4 .. 3.5e-4 on these shapes."""
    rng = np.random.default_rng(n_embd + T)
    be = backend()
    x = rng.standard_normal((T, n_embd)).astype(np.float32)
    wn = rng.uniform(0.5, 1.5, size=(n_embd,)).astype(np.float32)
    c = {"q3_K": 58/48}      # (block scales of 1/(48 sqrt(k)), as these cases have always had)
    wg, wgd = weights(rng, gate_up, (n_ff,), n_embd, rms_scale(gate_up, n_embd, c.get(gate_up, 1.0)))
    wu, wud = weights(rng, gate_up, (n_ff,), n_embd, rms_scale(gate_up, n_embd, c.get(gate_up, 1.0)))
    wd, wdd = weights(rng, down, (n_embd,), n_ff, rms_scale(down, n_ff, c.get(down, 1.0)))
    exp = ffn_f64(x, wn, wgd, wud, wdd, 1e-5)
    res = {}
    for fusion in (1, 0):
        be.set_option("fusion", fusion)
        try:
            with gg.Context() as ctx:
                xt = ctx.new_tensor(gg.F32, (n_embd, T)); wt = ctx.new_tensor(gg.F32, (n_embd,))
                g_ = ctx.new_tensor(QT[gate_up], (n_embd, n_ff)); u_ = ctx.new_tensor(QT[gate_up], (n_embd, n_ff)); d_ = ctx.new_tensor(QT[down], (n_ff, n_embd))
                nm = L.ggml_mul(ctx.ctx, L.ggml_rms_norm(ctx.ctx, xt, 1e-5), wt)
                gate_t = L.ggml_mul_mat(ctx.ctx, g_, nm); up = L.ggml_mul_mat(ctx.ctx, u_, nm)
                assert be.supports_op(gate_t) and be.supports_op(up)
                act = L.ggml_swiglu_split(ctx.ctx, gate_t, up)
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
    print(f"FFN {n_embd}/{n_ff} {gate_up} / {down} T={T}: NMSE fused {e1:.3g}, unfused {e0:.3g}, fused vs unfused {e10:.3g}")
    assert np.isfinite(res[1]).all() and np.isfinite(res[0]).all()
    assert e1 <= gate and e0 <= gate
    assert e10 <= 5e-4


def check_mat_vecs_on_one_normed_activation(types, k, seed, one_launch):
    """RMS_NORM -> MUL(weight) -> three mat-vecs that read the product (wq / wk / wv of a decode step). With the fusion pass on, same-format neighbours
    share one grouped launch (streamed at k % 256 == 0); a Q5_0 / Q5_1 neighbour pair, which has no common kernel, splits it. wq and wk in Q3_K: wv in
    Q3_K, Q4_K or Q5_K (the Q3_K_M / _L mixes) shares ONE grouped streamed launch with them — asserted through the profile at k = 1024 for the two mixed
    pairs — and wv in Q6_K, a pair without a common kernel, splits it."""
    rng = np.random.default_rng(seed)
    be = backend()
    ms = (130, 66, 34)
    x = rng.standard_normal((1, k)).astype(np.float32); wn = rng.uniform(0.5, 1.5, size=(k,)).astype(np.float32)
    ws = [weights(rng, t, (m,), k, rms_scale(t, k)) for t, m in zip(types, ms)]
    h = x.astype(np.float64) / np.sqrt((x.astype(np.float64)**2).mean() + 1e-5) * wn
    res = {}; prof = []
    for fusion in (1, 0):
        be.set_option("fusion", fusion)
        if fusion and one_launch:
            be.set_option("graphs", 0); be.set_option("profile", 1)
        try:
            with gg.Context() as ctx:
                xt = ctx.new_tensor(gg.F32, (k, 1)); wt = ctx.new_tensor(gg.F32, (k,))
                wts = [ctx.new_tensor(QT[t], (k, m)) for t, m in zip(types, ms)]
                nm = L.ggml_mul(ctx.ctx, L.ggml_rms_norm(ctx.ctx, xt, 1e-5), wt)
                outs = [L.ggml_mul_mat(ctx.ctx, w_, nm) for w_ in wts]
                assert all(be.supports_op(o) for o in outs)
                assert ctx.alloc(be)
                gg.tensor_set(xt, x); gg.tensor_set(wt, wn.reshape(1, k))
                for w_, (wb, _) in zip(wts, ws):
                    gg.tensor_set(w_, wb)
                be.compute(gg.graph_of(ctx, *outs))
                res[fusion] = [gg.tensor_get(o)[0, 0, 0].copy() for o in outs]
            if fusion and one_launch:
                prof = be.profile(64)
        finally:
            be.set_option("fusion", 1)
            if fusion and one_launch:
                be.set_option("profile", 0); be.set_option("graphs", 1)
    for i, (_, wd) in enumerate(ws):
        exp = (h @ wd.T)[0]
        e1, e0 = nmse(exp, res[1][i]), nmse(exp, res[0][i])
        print(f"{types} k={k} mat-vec {i}: NMSE fused {e1:.3g}, unfused {e0:.3g}")
        assert e1 <= GATE and e0 <= GATE and nmse(res[0][i], res[1][i]) <= 5e-4
    if one_launch:
        grouped = [e["kernel"] for e in prof if e["m"] < 0 and e["k"] == k]
        assert len(grouped) == 1 and grouped[0].startswith(f"k_mmvq_stream<{QT[one_launch[0]]}, {QT[one_launch[1]]},"), prof


def check_other_32_element_formats_are_still_refused(type_id, tname):
    """the backend has no kernel for them: supports_op says so and llama.cpp keeps those weights on the CPU"""
    be = backend()
    k, m, n_expert, n_used = 1024, 64, 4, 2
    with gg.Context() as ctx:
        for n in (1, 512):
            assert not be.supports_op(L.ggml_mul_mat(ctx.ctx, ctx.new_tensor(type_id, [k, m]), ctx.new_tensor(gg.F32, [k, n]))), tname
        op = L.ggml_mul_mat_id(ctx.ctx, ctx.new_tensor(type_id, [k, m, n_expert]), ctx.new_tensor(gg.F32, [k, n_used, 4]), ctx.new_tensor(gg.I32, [n_used, 4]))
        assert not be.supports_op(op), tname


def check_refusals():
    """Q2_K has no kernel, and a Q3_K row that is not whole 256-element blocks cannot exist: supports_op says so and llama.cpp keeps those weights on the CPU"""
    be = backend()
    Q3_K, Q2_K = 11, 10
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
