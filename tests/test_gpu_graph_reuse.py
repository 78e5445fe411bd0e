"""The backend driven the way llama.cpp drives it between submissions: the SAME graph and tensor objects re-submitted with shapes changed in place
(llama.cpp rebuilds a graph in one buf_compute_meta, src/llama-graph.cpp:424-428, so node pointers and topology stay put from one n_kv bucket to the
next), and a dead tensor's memory handed to the next tensor that fits (ggml-alloc). The backend keeps host-side state keyed on exactly those node
pointers and data addresses: the hipGraph cache and its segment-by-segment replay, the router -> combine hand-off. The other GPU tests give every
tensor memory of its own and build a fresh graph per case, so none of them reaches this state."""
import numpy as np
import pytest

import oracle as orc
import ops_ref as ref
from gpu_util import QTYPES, gg, pkg
import ref_llama
from ref_llama import RefLlama

ls = pkg.llama_synth

pytestmark = pytest.mark.gpu
L = gg.base()
TY = {"f16": gg.F16, "q8_0": gg.Q8_0}


def _set_shape(t, ne, nb):
    tt = t.contents
    for d in range(4):
        tt.ne[d] = ne[d]; tt.nb[d] = nb[d]


# fa_launches: FLASH_ATTN_EXT's own launches — the V conversion (kv_to_f16 at decode, the transpose for the prefill kernel) + the attention kernel
@pytest.mark.parametrize("tk,tv,T,fa_launches", [("f16", "q8_0", 1, 2), ("f16", "f16", 16, 2), ("q8_0", "q8_0", 1, 1)])
def test_attention_replay_with_n_kv_changed_in_place(tk, tv, T, fa_launches):
    """One graph, kept across submissions: six ADDs that do not depend on n_kv (segment 0 of a captured graph is six launches) and behind them
    FLASH_ATTN_EXT over views of a 1024-cell cache. Between submissions n_kv changes IN PLACE — ne / nb of the K / V views, their permutes and the
    mask, which is allocated for the largest n_kv as ggml-alloc's worst-case reservation would — as llama.cpp does when n_kv moves to the next
    256-cell bucket: 256 x3 (captured on the 2nd), 1024 x4, 512 x2. At the first 1024 step topology and segment 0 match the cached graph and the
    attention's segment does not: the prefix is replayed and the rest follows it. (f16, q8_0) at T = 1 reads V through kv_to_f16 and T = 16
    transposes V: both need a larger conversion buffer at 1024 cells than at 256; (q8_0, q8_0) at T = 1 needs none. At every step: the f64
    reference within FLASH_ATTN_EXT's gate, and the same bits as a backend with graphs off; within two more 1024 steps that graph is captured and
    replayed in full."""
    rng = np.random.default_rng(77 + T)
    hd, n_head, n_head_kv, kv_size = 128, 8, 2, 1024
    ne = hd * n_head_kv
    Tp = (T + 63) // 64 * 64
    scale = 1.0 / np.sqrt(hd)

    def make(t):
        x = rng.uniform(-1, 1, size=(kv_size, ne)).astype(np.float32)
        if t == "f16":
            b = x.astype(np.float16); return b.reshape(1, 1, kv_size, ne), b.astype(np.float64)
        b = orc.quantize(x, TY[t]); return b, orc.dequantize(b, TY[t]).astype(np.float64)
    kb, Kf = make(tk); vb, Vf = make(tv)
    q_ = rng.uniform(-1, 1, size=(1, T, n_head, hd)).astype(np.float32)
    be = gg.Backend(0); be.set_option("graphs", 1)          # (a backend of its own: no cached graph of another test, counters from zero)
    be_ref = gg.Backend(0); be_ref.set_option("graphs", 0)
    try:
        with gg.Context() as ctx:
            k_l = ctx.new_tensor(TY[tk], (ne, kv_size)); v_l = ctx.new_tensor(TY[tv], (ne, kv_size))
            q_cur = ctx.new_tensor(gg.F32, (hd, n_head, T)); zero = ctx.new_tensor(gg.F32, (hd, n_head, T))
            mask = ctx.new_tensor(gg.F16, (kv_size, Tp))        # room for the largest n_kv; ne / nb follow n_kv
            p = q_cur
            for _ in range(6):
                p = L.ggml_add(ctx.ctx, p, zero)                 # (x + 0 = x exactly: the reference attends with q_)
            rs_k = orc.row_size(TY[tk], hd); rs_v = orc.row_size(TY[tv], hd)
            kview = L.ggml_view_3d(ctx.ctx, k_l, hd, n_head_kv, kv_size, rs_k, rs_k * n_head_kv, 0)
            vview = L.ggml_view_3d(ctx.ctx, v_l, hd, n_head_kv, kv_size, rs_v, rs_v * n_head_kv, 0)
            q = L.ggml_permute(ctx.ctx, p, 0, 2, 1, 3); k = L.ggml_permute(ctx.ctx, kview, 0, 2, 1, 3); v = L.ggml_permute(ctx.ctx, vview, 0, 2, 1, 3)
            fa = L.ggml_flash_attn_ext(ctx.ctx, q, k, v, mask, float(scale), 0.0, 0.0)
            L.ggml_flash_attn_ext_set_prec(fa, 10)
            assert be.supports_op(fa) and ctx.alloc(be)
            gg.tensor_set(k_l, kb); gg.tensor_set(v_l, vb); gg.tensor_set(q_cur, q_); gg.tensor_set(zero, np.zeros_like(q_))
            graph = gg.graph_of(ctx, fa)

            def set_n_kv(n_kv):
                for view, perm, rs in ((kview, k, rs_k), (vview, v, rs_v)):
                    _set_shape(view, (hd, n_head_kv, n_kv, 1), (view.contents.nb[0], rs, rs * n_head_kv, rs * n_head_kv * n_kv))
                    _set_shape(perm, (hd, n_kv, n_head_kv, 1), (perm.contents.nb[0], rs * n_head_kv, rs, rs * n_head_kv * n_kv))
                _set_shape(mask, (n_kv, Tp, 1, 1), (2, n_kv * 2, n_kv * 2 * Tp, n_kv * 2 * Tp))
                mk = np.full((Tp, n_kv), -np.inf, np.float32)
                for t in range(T):
                    mk[t, :n_kv - T + t + 1] = 0.0
                gg.tensor_set(mask, mk.astype(np.float16).reshape(1, 1, Tp, n_kv))
                return mk

            # the prefix really is six launches of their own (no matcher takes the ADDs together): the attention is in segment 1
            set_n_kv(256)
            be_ref.reset_counters(); be_ref.compute(graph)
            assert be_ref.counters()["kernels_launched"] == 6 + fa_launches, be_ref.counters()

            be.reset_counters()
            seq = [256] * 3 + [1024] * 4 + [512] * 2
            hist = []
            for step, n_kv in enumerate(seq):
                mk = set_n_kv(n_kv)
                be.compute(graph)                                # raises unless graph_compute returned SUCCESS
                got = gg.tensor_get(fa).copy()
                hist.append(be.counters())
                be_ref.compute(graph)
                assert np.array_equal(got, gg.tensor_get(fa)), (step, n_kv, "the result differs from the one with graphs off")
                K = Kf[:n_kv].reshape(n_kv, n_head_kv, hd); V = Vf[:n_kv].reshape(n_kv, n_head_kv, hd)
                exp = ref.flash_attn_ext(q_[0], K, V, mk, scale)
                assert orc.nmse(exp, got[0]) <= 5e-4, (step, n_kv, orc.nmse(exp, got[0]))
    finally:
        be_ref.free(); be.free()
    c = lambda step, key: hist[step][key]
    assert c(1, "graph_captures") == 1 and c(2, "graph_replays") == 1, hist[:3]
    assert c(3, "graph_partial_replays") > c(2, "graph_partial_replays"), hist[3]      # the first 1024 step: prefix replayed, the rest behind it
    assert c(5, "graph_captures") == c(3, "graph_captures") + 1, hist[3:6]            # ... the 1024 graph is captured within two more steps
    assert c(5, "graph_replays") > c(3, "graph_replays") and c(6, "graph_replays") == c(5, "graph_replays") + 1, hist[3:7]   # ... and replayed in full
    assert c(7, "graph_partial_replays") > c(6, "graph_partial_replays"), hist[7]      # 512 behind the 1024 graph: a partial match again


def _moe_block(ctx, x, gate_w, down_w, n_expert, n_used, k):
    """build_moe_ffn for one token (src/llama-graph.cpp:838-1012), the experts reduced to the down product: router MUL_MAT -> SOFT_MAX -> ARGSORT
    -> top-k view; MUL_MAT_ID(down, x); GET_ROWS of the probabilities -> SUM_ROWS / DIV; MUL; the ADD chain over the expert slots"""
    probs = L.ggml_soft_max(ctx.ctx, L.ggml_mul_mat(ctx.ctx, gate_w, x))
    srt = L.ggml_argsort(ctx.ctx, probs, gg.GGML_SORT_ORDER_DESC)
    sel = L.ggml_view_2d(ctx.ctx, srt, n_used, 1, n_expert * 4, 0)
    ex = L.ggml_mul_mat_id(ctx.ctx, down_w, L.ggml_reshape_3d(ctx.ctx, x, k, 1, 1), sel)
    wts = L.ggml_get_rows(ctx.ctx, L.ggml_reshape_3d(ctx.ctx, probs, 1, n_expert, 1), sel)
    wts = L.ggml_reshape_2d(ctx.ctx, wts, n_used, 1)
    wts = L.ggml_div(ctx.ctx, wts, L.ggml_sum_rows(ctx.ctx, wts))
    ex = L.ggml_mul(ctx.ctx, ex, L.ggml_reshape_3d(ctx.ctx, wts, 1, n_used, 1))
    out = L.ggml_view_2d(ctx.ctx, ex, k, 1, ex.contents.nb[2], 0)
    for u in range(1, n_used):
        out = L.ggml_add(ctx.ctx, out, L.ggml_view_2d(ctx.ctx, ex, k, 1, ex.contents.nb[2], u * ex.contents.nb[1]))
    return probs, srt, out


def _moe_block_ref(x, gate, down, n_used):
    logits = gate.astype(np.float64) @ x.astype(np.float64)
    p = np.exp(logits - logits.max()); p /= p.sum()
    sel = np.argsort(-p, kind="stable")[:n_used]
    w = p[sel] / p[sel].sum()
    return sum(w[u] * (down[sel[u]] @ x.astype(np.float64)) for u in range(n_used)), p, sel


@pytest.mark.parametrize("n_expert,n_used", [(8, 2), (32, 4)])
def test_moe_router_hand_off_with_reused_memory(n_expert, n_used):
    """Two MoE blocks in one graph. Block 1's router (F32 gate) runs fused (k_moe_route) and leaves its ranked top values for the combine; block 2's
    gate is F16, so its router runs node by node — and, as ggml-alloc would place them once block 1's are dead, its probabilities and its ranking
    are written over block 1's. Block 2's combine must weight its experts with block 2's probabilities, not with the values block 1's router
    left behind (the hand-off is keyed on those addresses). Against float64 on the dequantized experts (NMSE 1e-3, the MoE layer tests' gate),
    with fusion on and off."""
    k = 256
    rng = np.random.default_rng(40 + n_expert)
    qt = QTYPES["q8_0"]
    # gate rows that rank the experts with clear gaps at the top-k boundary, and two blocks that weight their experts very differently
    x_ = rng.standard_normal((2, k)).astype(np.float32)
    gates = []
    for blk in (0, 1):
        while True:
            g = rng.standard_normal((n_expert, k)) / np.sqrt(k)
            if blk == 0:
                g[rng.integers(n_expert)] += 6.0 * x_[blk] / float(x_[blk] @ x_[blk])       # one expert's logit 6 above its draw
            g = g.astype(np.float32)
            if blk == 1:
                g = g.astype(np.float16).astype(np.float32)
            p = np.sort(_moe_block_ref(x_[blk], g, np.zeros((n_expert, 1, k)), n_used)[1])[::-1]
            lead = p[0] / p[:n_used].sum()      # block 1: one expert carries the token; block 2: spread out
            if p[n_used] < 0.8 * p[n_used - 1] and (lead > 0.85 if blk == 0 else lead < 0.6):
                break
        gates.append(g)
    downs = [orc.random_blocks(rng, qt, (n_expert, k), k, scale=1.0 / np.sqrt(k)) for _ in range(2)]
    dd = [orc.dequantize(d.reshape(n_expert * k, -1), qt).reshape(n_expert, k, k).astype(np.float64) for d in downs]
    exp = [_moe_block_ref(x_[b], gates[b], dd[b], n_used) for b in range(2)]
    w0 = exp[0][1][exp[0][2]] / exp[0][1][exp[0][2]].sum(); w1 = exp[1][1][exp[1][2]] / exp[1][1][exp[1][2]].sum()
    assert np.abs(w0 - w1).max() > 0.25         # (block 1's weights in block 2's combine would show far above the gate)
    be = gg.Backend(0)
    try:
        with gg.Context() as ctx:
            xs = [ctx.new_tensor(gg.F32, (k, 1)) for _ in range(2)]
            gw = [ctx.new_tensor(gg.F32, (k, n_expert)), ctx.new_tensor(gg.F16, (k, n_expert))]
            dw = [ctx.new_tensor(qt, (k, k, n_expert)) for _ in range(2)]
            blocks = [_moe_block(ctx, xs[b], gw[b], dw[b], n_expert, n_used, k) for b in range(2)]
            graph = gg.graph_of(ctx, blocks[0][2], blocks[1][2])
            assert ctx.alloc(be)
            # block 2's probabilities and ranking at block 1's addresses (and every view of them)
            (p0, s0, _), (p1, s1, _) = blocks
            for t0, t1 in ((p0, p1), (s0, s1)):
                old = t1.contents.data
                for i in range(L.ggml_graph_n_nodes(graph)):
                    nd = L.ggml_graph_node(graph, i)
                    if nd.contents.data == old:
                        nd.contents.data = t0.contents.data
                assert t1.contents.data == t0.contents.data
            gg.tensor_set(xs[0], x_[0:1]); gg.tensor_set(xs[1], x_[1:2])
            gg.tensor_set(gw[0], gates[0]); gg.tensor_set(gw[1], gates[1].astype(np.float16))
            gg.tensor_set(dw[0], downs[0]); gg.tensor_set(dw[1], downs[1])
            for fusion in (1, 0):
                be.set_option("fusion", fusion); be.reset_counters()
                be.compute(graph)
                # fused: block 1's combine takes the router's hand-off, block 2's (its router ran node by node over the same memory) must not
                assert be.counters()["moe_combine_direct"] == fusion, be.counters()
                for b in range(2):
                    got = gg.tensor_get(blocks[b][2])[0, 0, 0].astype(np.float64)
                    assert orc.nmse(exp[b][0], got) <= 1e-3, (fusion, b, orc.nmse(exp[b][0], got))
    finally:
        be.free()


@pytest.mark.parametrize("scenario", ["oai-fa0", "oai-fa1", "tiny-fa1-q8_0"])
def test_model_graph_reused_across_n_kv_buckets(scenario, monkeypatch):
    """MI_HARNESS_REUSE_GRAPH=1: one graph per (sequence, n_tokens), built for the largest n_kv and resized in place from one n_kv bucket to the next —
    the same node objects at the same addresses, as llama.cpp's rebuild in one buf_compute_meta leaves them.
    oai-fa0 / oai-fa1: tiny-oai (MXFP4 experts, iSWA: even layers attend through a 16-token window in a 32-cell ring, odd layers through the full cache),
    8-token steps (one prompt and single tokens without flash attention; 66 batches of 8, then single tokens with it) past the window, past the ring's
    wrap and across n_kv buckets (32 cells without flash attention, 256 with).
    Once the window cache is full, layer 0's n_kv is fixed while layer 1's grows, so a cached graph matches in its leading segments only.
    tiny-fa1-q8_0: flash attention over a q8_0 / q8_0 cache, the prompt fed as equal 16-token ubatches across 256-cell buckets (V is converted for the
    prefill kernel: the conversion buffer grows with n_kv), then single tokens.
    Every step against RefLlama (cpu16) at the model tests' 1e-3 gate and bit for bit against the same steps with graphs off."""
    monkeypatch.setenv("MI_HARNESS_REUSE_GRAPH", "1")
    rng = np.random.default_rng(13)
    if scenario.startswith("oai"):
        fa = scenario == "oai-fa1"
        n_ctx = 600 if fa else 96
        args = dict(model="tiny-oai", ftype="MXFP4_MOE", n_ctx=n_ctx, seed=10, flash_attn=fa)
        # (8-token batches: the ring holds n_swa + n_ubatch cells, n_ubatch = 8)
        # (the streams end one step before a routing near-tie among the 32 experts: the harness without MI_HARNESS_REUSE_GRAPH, graphs on or off, gives
        # the same bits there and misses the reference by ~1e-2 as well — a fourth-ranked expert decided by the order of f32 additions)
        steps = ([[int(t) for t in rng.integers(0, 512, size=8)] for _ in range(66)] + [[int(t)] for t in rng.integers(0, 512, size=13)] if fa else
                 [[int(t) for t in rng.integers(0, 512, size=8)]] + [[int(t)] for t in rng.integers(0, 512, size=34)])
    else:
        args = dict(model="tiny", ftype="Q4_K_M", n_ctx=1024, seed=3, flash_attn=True, type_k=gg.Q8_0, type_v=gg.Q8_0)
        steps = [[int(t) for t in rng.integers(0, 512, size=16)] for _ in range(40)] + [[int(t)] for t in rng.integers(0, 512, size=8)]
    be = gg.Backend(0)
    outs, cnts = {}, {}
    try:
        for graphs in (1, 0):
            be.set_option("graphs", graphs); be.reset_counters()
            m = ls.SynthLlama(be, args["model"], args["ftype"], n_ctx=args["n_ctx"], seed=args["seed"], flash_attn=args["flash_attn"],
                              type_k=args.get("type_k", 0), type_v=args.get("type_v", 0))
            try:
                if graphs:
                    rc = RefLlama(m.cfg, ref_llama.read_weights(m, gg), args["n_ctx"], "cpu16")
                res = []; tight = True
                for i, toks in enumerate(steps):
                    got = m.decode(toks)
                    assert np.isfinite(got).all()
                    if graphs:
                        exp_c = rc.decode(np.stack([m.embedding(t) for t in toks]))
                        tight = tight and len(toks) <= 8     # (after a > 8-token pass through the bf16 matrix-core kernels: 2e-3, as test_gpu_row_split)
                        assert orc.nmse(exp_c, got) <= (1e-3 if tight else 2e-3), (scenario, i, m.n_past, orc.nmse(exp_c, got))
                    res.append(got.copy())
                outs[graphs] = res
                cnts[graphs] = be.counters()
            finally:
                m.free()
    finally:
        be.free()
    for i, (a_, b_) in enumerate(zip(outs[1], outs[0])):
        assert np.array_equal(a_, b_), (scenario, i, "graph replay changed the logits")
    print(scenario, {k: cnts[1][k] for k in ("graph_replays", "graph_captures", "graph_partial_replays")})
    assert cnts[1]["graph_replays"] > 0 and cnts[1]["graph_partial_replays"] > 0, cnts[1]      # (4 in each scenario when this was written)
