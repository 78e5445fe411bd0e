"""Attention over per-sequence KV streams (kv_unified = false: q [hs, T, n_head, n_stream], K / V [hs, n_kv, n_head_kv, n_stream], the mask
[n_kv, PAD(T), 1, n_stream]; src/llama-graph.cpp:1231-1238, :1421): one node, one launch, every stream attending to its own cells.

Graphs are built through the C-ABI the way tests/test_gpu_flash_attn_head_sizes.py builds them; its fa_ref is the float64 reference, applied per stream
(test_stream_reference_agrees_with_oracle checks that without a GPU). Every stream has its own K / V / q content and its own live length through its
mask, and the cache has kv_size = n_kv + 64 cells per stream, so that nb[3] != n_kv*nb[1]: a kernel that took the streams for dense would read the
wrong cells. Gate: NMSE 5e-4 (tests/test-backend-ops.cpp:4559). Each case also runs as n_stream one-stream nodes over views of the same buffers.
The launch's plan (nsplit, kv_chunk, live_scan; the prefill form's tile split) does not read the stream count unless the decode split's partial results
of all streams outgrow the partial buffer (same_plan below, the plan's own formula) — so wherever same_plan holds the two results are the same bits; one case has
more partial results than the buffer holds and runs with fewer ranges than its one-stream nodes."""
import numpy as np
import pytest

import oracle as orc
import ops_ref as ref
from test_gpu_flash_attn_head_sizes import NMSE_GATE, _bf16_round, fa_ref

ATTN_PART_BYTES = 8 * 128 * 32 * (128 + 2) * 4      # csrc/kernels.h
LIVE = (40, 200, 130, 256, 77)                       # visible cells per stream, of 256 (scaled with n_kv)


def stream_masks(S, T, n_kv, max_bias=0.0, shared=False):
    """[S, PAD(T, 64), n_kv] f32: stream s's T tokens are the last T of its LIVE[s]/256 * n_kv live cells, causal among themselves; everything behind
    is -inf (the padding of the largest stream's n_kv). ALiBi: minus the distance / 16 (f16 values). shared: every stream gets stream 0's mask."""
    Tp = (T + 63) // 64 * 64
    m = np.full((S, Tp, n_kv), -np.inf, np.float32)
    for s in range(S):
        live = max(T, LIVE[0 if shared else s] * n_kv // 256)
        for t in range(T):
            n_vis = live - T + t + 1
            m[s, t, :n_vis] = (-np.arange(n_vis)[::-1] / 16.0).astype(np.float16) if max_bias > 0 else 0.0
    return m


def fa_ref_streams(q, K, V, masks, scale, max_bias=0.0, softcap=0.0, sinks=None):
    """q [S, T, n_head, hsk], K [S, n_kv, n_head_kv, hsk], V [S, n_kv, n_head_kv, hsv], masks [S, >= T, n_kv] -> [S, T, n_head, hsv]: fa_ref per stream;
    sinks and ALiBi slopes are per head, the same for every stream"""
    return np.stack([fa_ref(q[s], K[s], V[s], masks[s], scale, max_bias, softcap, sinks) for s in range(q.shape[0])])


def test_stream_reference_agrees_with_oracle():
    """the per-stream float64 reference == oracle.ops_ref.flash_attn_ext stream by stream (1e-12 relative) on a 2-stream case with different live lengths"""
    rng = np.random.default_rng(5)
    S, T, n_head, n_head_kv, n_kv, hs = 2, 5, 6, 2, 256, 64
    q = rng.uniform(-1, 1, size=(S, T, n_head, hs)).astype(np.float16).astype(np.float32)
    K = rng.uniform(-1, 1, size=(S, n_kv, n_head_kv, hs)); V = rng.uniform(-1, 1, size=(S, n_kv, n_head_kv, hs))
    sk = rng.uniform(-1, 1, size=(n_head,)).astype(np.float32)
    for max_bias, softcap, sinks in ((0.0, 0.0, None), (8.0, 0.0, sk), (0.0, 10.0, sk)):
        masks = stream_masks(S, T, n_kv, max_bias)
        assert not np.array_equal(masks[0], masks[1])
        a = fa_ref_streams(q, K, V, masks, 1.0 / np.sqrt(hs), max_bias, softcap, sinks)
        assert a.shape == (S, T, n_head, hs)
        for s in range(S):
            b = ref.flash_attn_ext(q[s], K[s], V[s], masks[s], 1.0 / np.sqrt(hs), max_bias, softcap, sinks)
            assert float(np.abs(a[s] - b).max()) <= 1e-12 * float(np.abs(b).max()), (s, max_bias, softcap)


def _gpu():
    from gpu_util import backend, gg, pkg
    return backend, gg, pkg


def same_plan(S, T, n_kv, n_head, hsv):
    """does the S-stream launch get the plan fields of a one-stream launch (attn_plan_decode: every range's slot for all streams fits the buffer)"""
    if T > 8 or n_kv < 256 or n_kv % 32:
        return True
    return T * S * n_head * min((n_kv + 127) // 128, 32) * (hsv + 2) * 4 <= ATTN_PART_BYTES


def make_cache(gg, rng, t, S, kv_size, ne):
    """-> (bytes for tensor_set of a [ne, kv_size, S] cache, its float64 values [S, kv_size, ne])"""
    TY = {"f16": gg.F16, "bf16": gg.BF16, "q8_0": gg.Q8_0, "q4_0": gg.Q4_0}
    x = rng.uniform(-1, 1, size=(S * kv_size, ne)).astype(np.float32)
    if t == "f16":
        b = x.astype(np.float16); return b, b.astype(np.float64).reshape(S, kv_size, ne)
    if t == "bf16":
        b = _bf16_round(x); return b, (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(S, kv_size, ne)
    b = orc.quantize(x, TY[t]); return b, orc.dequantize(b, TY[t]).astype(np.float64).reshape(S, kv_size, ne)


def build_fa_streams(ctx, gg, L, S_q, S_kv, hsk, hsv, n_head, n_head_kv, n_kv, T, tk, tv, kv_size, mask_ne2=1, mask_ne3=None, max_bias=0.0, softcap=0.0, sinks=False, prefix_adds=0):
    """the node of build_attn_mha with flash attention for a ubatch of S_q streams (S_kv cache streams), and the tensors it reads. prefix_adds: q goes through that
    many ADDs of a zero tensor first (x + 0 = x exactly) — the backend captures graphs of eight nodes and more"""
    TY = {"f16": gg.F16, "bf16": gg.BF16, "q8_0": gg.Q8_0, "q4_0": gg.Q4_0}
    Tp = (T + 63) // 64 * 64
    k_l = ctx.new_tensor(TY[tk], (hsk * n_head_kv, kv_size, S_kv)); v_l = ctx.new_tensor(TY[tv], (hsv * n_head_kv, kv_size, S_kv))
    q_cur = ctx.new_tensor(gg.F32, (hsk, n_head, T, S_q))
    m_ = ctx.new_tensor(gg.F16, (n_kv, Tp, mask_ne2, S_q if mask_ne3 is None else mask_ne3)); s_ = ctx.new_tensor(gg.F32, (n_head,))
    rs_k = orc.row_size(TY[tk], hsk); rs_v = orc.row_size(TY[tv], hsv)
    k = L.ggml_view_4d(ctx.ctx, k_l, hsk, n_head_kv, n_kv, S_kv, rs_k, rs_k * n_head_kv, rs_k * n_head_kv * kv_size, 0)      # get_k / get_v
    v = L.ggml_view_4d(ctx.ctx, v_l, hsv, n_head_kv, n_kv, S_kv, rs_v, rs_v * n_head_kv, rs_v * n_head_kv * kv_size, 0)
    zero = ctx.new_tensor(gg.F32, (hsk, n_head, T, S_q)) if prefix_adds else None
    qa = q_cur
    for _ in range(prefix_adds):
        qa = L.ggml_add(ctx.ctx, qa, zero)
    q = L.ggml_permute(ctx.ctx, qa, 0, 2, 1, 3); k = L.ggml_permute(ctx.ctx, k, 0, 2, 1, 3); v = L.ggml_permute(ctx.ctx, v, 0, 2, 1, 3)
    fa = L.ggml_flash_attn_ext(ctx.ctx, q, k, v, m_, float(1.0 / np.sqrt(hsk)), float(max_bias), float(softcap))
    if sinks:
        L.ggml_flash_attn_ext_add_sinks(fa, s_)
    L.ggml_flash_attn_ext_set_prec(fa, 10)
    return fa, k_l, v_l, q_cur, m_, s_, zero


def run_case(S, T, n_kv, n_head, n_head_kv, hs, tk="f16", tv="f16", max_bias=0.0, softcap=0.0, sinks=False, shared_mask=False, repeat=False):
    backend, gg, _ = _gpu()
    L = gg.base()
    TY = {"f16": gg.F16, "bf16": gg.BF16, "q8_0": gg.Q8_0, "q4_0": gg.Q4_0}
    rng = np.random.default_rng(9000 + 131 * S + 17 * T + n_kv + hs)
    kv_size = n_kv + 64
    Tp = (T + 63) // 64 * 64
    kb, Kf = make_cache(gg, rng, tk, S, kv_size, hs * n_head_kv); vb, Vf = make_cache(gg, rng, tv, S, kv_size, hs * n_head_kv)
    q_ = rng.uniform(-1, 1, size=(S, T, n_head, hs)).astype(np.float32)
    masks = stream_masks(S, T, n_kv, max_bias, shared_mask)
    sk = rng.uniform(-1, 1, size=(n_head,)).astype(np.float32)
    be = backend()
    with gg.Context() as ctx:
        fa, k_l, v_l, q_cur, m_, s_, zero = build_fa_streams(ctx, gg, L, S, S, hs, hs, n_head, n_head_kv, n_kv, T, tk, tv, kv_size, mask_ne3=1 if shared_mask else S,
                                                             max_bias=max_bias, softcap=softcap, sinks=sinks, prefix_adds=6 if repeat else 0)
        assert be.supports_op(fa), "a node with one KV stream per sequence is refused"
        # the same work as S one-stream nodes over views of the same buffers
        rs_k = orc.row_size(TY[tk], hs); rs_v = orc.row_size(TY[tv], hs)
        qc, mc = q_cur.contents, m_.contents
        singles = []
        for s in range(S):
            k1 = L.ggml_view_4d(ctx.ctx, k_l, hs, n_head_kv, n_kv, 1, rs_k, rs_k * n_head_kv, rs_k * n_head_kv * kv_size, s * rs_k * n_head_kv * kv_size)
            v1 = L.ggml_view_4d(ctx.ctx, v_l, hs, n_head_kv, n_kv, 1, rs_v, rs_v * n_head_kv, rs_v * n_head_kv * kv_size, s * rs_v * n_head_kv * kv_size)
            q1 = L.ggml_view_3d(ctx.ctx, q_cur, hs, n_head, T, qc.nb[1], qc.nb[2], s * qc.nb[3])
            m1 = L.ggml_view_2d(ctx.ctx, m_, n_kv, Tp, mc.nb[1], 0 if shared_mask else s * mc.nb[3])
            f1 = L.ggml_flash_attn_ext(ctx.ctx, L.ggml_permute(ctx.ctx, q1, 0, 2, 1, 3), L.ggml_permute(ctx.ctx, k1, 0, 2, 1, 3), L.ggml_permute(ctx.ctx, v1, 0, 2, 1, 3),
                                       m1, float(1.0 / np.sqrt(hs)), float(max_bias), float(softcap))
            if sinks:
                L.ggml_flash_attn_ext_add_sinks(f1, s_)
            L.ggml_flash_attn_ext_set_prec(f1, 10)
            assert be.supports_op(f1)
            singles.append(f1)
        assert ctx.alloc(be)
        gg.tensor_set(k_l, kb); gg.tensor_set(v_l, vb); gg.tensor_set(q_cur, q_)
        gg.tensor_set(m_, (masks[:1] if shared_mask else masks).astype(np.float16)); gg.tensor_set(s_, sk)
        if zero:
            gg.tensor_set(zero, np.zeros_like(q_))
        graph = gg.graph_of(ctx, fa)
        if repeat:
            be.set_option("graphs", 1)
        be.reset_counters()
        be.compute(graph)
        got = gg.tensor_get(fa).copy()                                             # [S, T, n_head, hs]
        if repeat:      # the conversion buffer and the captured graph are reused: the same bits every time
            for _ in range(3):
                be.compute(graph)
                assert np.array_equal(got, gg.tensor_get(fa))
            cnt = be.counters()
            assert cnt["graph_replays"] >= 1, cnt
        be.compute(gg.graph_of(ctx, *singles))
        one = np.stack([gg.tensor_get(f)[0] for f in singles])
    K = Kf[:, :n_kv].reshape(S, n_kv, n_head_kv, hs); V = Vf[:, :n_kv].reshape(S, n_kv, n_head_kv, hs)
    qr = q_.astype(np.float16).astype(np.float32)
    exp = fa_ref_streams(qr, K, V, masks, 1.0 / np.sqrt(hs), max_bias, softcap, sk if sinks else None)
    assert got.shape == exp.shape == one.shape == (S, T, n_head, hs)
    e = orc.nmse(exp, got); e1 = orc.nmse(exp, one); per = [orc.nmse(exp[s], got[s]) for s in range(S)]
    same = same_plan(S, T, n_kv, n_head, hs)
    print(f"streams {S} T {T} n_kv {n_kv} heads {n_head}/{n_head_kv} hs {hs} {tk}/{tv} bias {max_bias} cap {softcap} sinks {sinks} shared mask {shared_mask}: "
          f"nmse {e:.3e} (per stream {' '.join('%.2e' % x for x in per)}), one-stream nodes {e1:.3e}, batched vs one-stream {orc.nmse(one, got):.3e}, same plan {same}")
    assert e <= NMSE_GATE and max(per) <= NMSE_GATE, (e, per)
    assert e1 <= NMSE_GATE, e1
    if same:
        assert np.array_equal(got, one), "one launch for all streams and one launch per stream share a plan but not their bits"


# S, T, n_kv, n_head, n_head_kv, hs, tk, tv, max_bias, softcap, sinks, shared_mask, repeat
GRID = []
for _S in (2, 3):
    for _T in (1, 2, 8, 33):
        for _n_kv in (256, 2048):      # 256: one workgroup per (head, token) (T = 1: the live scan); 2048: split + merge; T = 33: the prompt kernel
            for _tk in ("f16", "q8_0"):
                _heads = (8, 2) if (_S + _T + _n_kv // 256) % 2 else (6, 2)
                _hs = 128 if (_T + (_tk == "f16")) % 2 else 64
                GRID.append((_S, _T, _n_kv, _heads[0], _heads[1], _hs, _tk, _tk, 0.0, 0.0, False, False, False))
GRID += [
    (5, 1, 256, 8, 2, 128, "f16", "f16", 0.0, 0.0, False, False, False),
    (2, 2, 16384, 8, 2, 128, "f16", "f16", 0.0, 0.0, False, False, False),        # only the split form runs
    (3, 2, 512, 6, 2, 96, "f16", "f16", 0.0, 0.0, True, False, False),
    (2, 33, 256, 8, 2, 128, "bf16", "bf16", 0.0, 0.0, False, False, False),        # kv_to_f16 for all streams
    (3, 33, 512, 8, 2, 64, "q4_0", "q4_0", 0.0, 0.0, True, False, False),
    (3, 8, 256, 8, 2, 128, "f16", "bf16", 0.0, 0.0, False, False, False),
    (2, 1, 2048, 6, 2, 128, "f16", "f16", 8.0, 0.0, True, False, False),
    (3, 33, 256, 6, 2, 64, "f16", "f16", 8.0, 10.0, False, False, False),
    (2, 2, 256, 8, 2, 64, "q8_0", "q8_0", 0.0, 10.0, True, False, False),
    (3, 1, 256, 8, 2, 128, "f16", "f16", 0.0, 0.0, False, True, False),            # one mask (ne[3] = 1) for all streams
    (3, 33, 512, 8, 2, 128, "q8_0", "q8_0", 0.0, 0.0, False, False, True),         # graphs on, computed again: conversion buffer + captured graph reused
    (2, 1, 2048, 8, 2, 128, "f16", "f16", 0.0, 0.0, False, False, True),
    # 3 streams x 8 tokens x 48 heads x 32 ranges do not fit the partial-result buffer: the batched launch splits into the 28 ranges it holds (the one-stream
    # nodes into 32), so the two runs have different plans — both against the reference, their distance printed
    (3, 8, 4096, 48, 4, 128, "f16", "f16", 0.0, 0.0, True, False, False),
]
assert not same_plan(*GRID[-1][:4], GRID[-1][5]) and all(same_plan(*g[:4], g[5]) for g in GRID[:-1])


@pytest.mark.gpu
@pytest.mark.parametrize("S,T,n_kv,n_head,n_head_kv,hs,tk,tv,max_bias,softcap,sinks,shared_mask,repeat", GRID)
def test_flash_attn_ext_streams(S, T, n_kv, n_head, n_head_kv, hs, tk, tv, max_bias, softcap, sinks, shared_mask, repeat):
    run_case(S, T, n_kv, n_head, n_head_kv, hs, tk, tv, max_bias, softcap, sinks, shared_mask, repeat)


@pytest.mark.gpu
def test_flash_attn_ext_stream_support_answers():
    """supports_op from shapes alone: nodes with a cache stream per sequence are accepted; ggml's broadcast of one cache over several q batches, a per-head mask
    and a mask whose stream count is neither 1 nor the node's are refused — and so is a stream count whose decode launch has no form that fits the
    partial-result buffer: 16384 cells are more than one workgroup's LDS holds (12288), so the launch must split into >= 2 ranges, i.e.
    2 * T * n_stream * n_head * (hsv + 2) * 4 bytes of partial results (csrc/decode_fused.hip: attn_plan_decode); one stream fewer fits and is accepted."""
    backend, gg, _ = _gpu()
    L = gg.base()
    be = backend()

    def answer(S_q, S_kv, T=1, n_kv=256, n_head=8, mask_ne2=1, mask_ne3=None):
        with gg.Context() as ctx:
            fa = build_fa_streams(ctx, gg, L, S_q, S_kv, 128, 128, n_head, 2, n_kv, T, "f16", "f16", n_kv + 64, mask_ne2, mask_ne3)[0]
            return be.supports_op(fa)
    for T in (1, 33):
        assert answer(2, 2, T) and answer(3, 3, T) and answer(2, 2, T, mask_ne3=1)
        assert not answer(2, 1, T), "one cache stream broadcast over two q batches"
        assert not answer(2, 2, T, mask_ne2=2), "a per-head mask"
        assert not answer(2, 2, T, mask_ne3=3), "three masks for two streams"
    T, n_head, hsv, n_kv = 8, 128, 128, 16384
    assert n_kv * 4 > 48 * 1024
    S_max = ATTN_PART_BYTES // (2 * T * n_head * (hsv + 2) * 4)      # the most streams whose two ranges fit
    assert S_max == 16
    assert answer(S_max, S_max, T, n_kv, n_head)
    assert not answer(S_max + 1, S_max + 1, T, n_kv, n_head), "no decode form fits the partial-result buffer"


def build_chain(ctx, gg, L, S, T, n_kv, n_head, n_head_kv, hd, tk, mask_type, sinks, kv_size):
    """build_attn_mha without flash attention for S streams (src/llama-graph.cpp:1283-1341): MUL_MAT(k, q) -> SOFT_MAX(mask, scale[, sinks]) -> MUL_MAT(v, kq) ->
    PERMUTE -> CONT to [hd*n_head, T*S]; K rows are cells, V is the transposed cache (a row over cells per dimension)"""
    TYK = gg.Q8_0 if tk == "q8_0" else gg.F16
    Tp = (T + 63) // 64 * 64
    ne = hd * n_head_kv
    k_l = ctx.new_tensor(TYK, (ne, kv_size, S)); v_l = ctx.new_tensor(gg.F16, (kv_size, ne, S))
    q_cur = ctx.new_tensor(gg.F32, (hd, n_head, T, S)); m_ = ctx.new_tensor(mask_type, (n_kv, Tp, 1, S)); s_ = ctx.new_tensor(gg.F32, (n_head,))
    rs = orc.row_size(TYK, hd)
    k = L.ggml_view_4d(ctx.ctx, k_l, hd, n_head_kv, n_kv, S, rs, rs * n_head_kv, rs * n_head_kv * kv_size, 0)
    v = L.ggml_view_4d(ctx.ctx, v_l, n_kv, n_head_kv, hd, S, 2 * kv_size * hd, 2 * kv_size, 2 * kv_size * ne, 0)
    q = L.ggml_permute(ctx.ctx, q_cur, 0, 2, 1, 3); k = L.ggml_permute(ctx.ctx, k, 0, 2, 1, 3); v = L.ggml_permute(ctx.ctx, v, 0, 2, 1, 3)
    kq = L.ggml_mul_mat(ctx.ctx, k, q)
    L.ggml_mul_mat_set_prec(kq, 10)
    kq = L.ggml_soft_max_ext(ctx.ctx, kq, m_, float(1.0 / np.sqrt(hd)), 0.0)
    if sinks:
        L.ggml_soft_max_add_sinks(kq, s_)
    kqv = L.ggml_mul_mat(ctx.ctx, v, kq)
    cur = L.ggml_permute(ctx.ctx, kqv, 0, 2, 1, 3)
    cur = L.ggml_cont_2d(ctx.ctx, cur, hd * n_head, T * S)
    return cur, k_l, v_l, q_cur, m_, s_


@pytest.mark.gpu
@pytest.mark.parametrize("S,T,tk,mask,sinks", [(2, 1, "f16", "f16", False), (3, 1, "q8_0", "f32", False), (3, 1, "f16", "f16", True), (2, 33, "f16", "f32", False),
                                               (3, 33, "f16", "f16", True), (2, 33, "q8_0", "f16", False), (2, 1, "q8_0", "f16", True), (3, 33, "f16", "f32", False)])
def test_attention_chain_streams(S, T, tk, mask, sinks):
    """the graph without flash attention, every tensor with ne[3] = n_stream: with fusion on one attention launch replaces the chain (kernels_launched, graphs
    off, as the fusion tests count); with fusion off the nodes run one by one; both within the gate of the float64 reference. (A prompt over a Q8_0 K
    cache keeps the generic nodes with fusion on as well, as it does for one stream.)"""
    backend, gg, _ = _gpu()
    L = gg.base()
    be = backend()
    n_kv, n_head, n_head_kv, hd = 256, 8, 2, 128
    kv_size = n_kv + 64
    ne = hd * n_head_kv
    rng = np.random.default_rng(4000 + 7 * S + T)
    kb, Kf = make_cache(gg, rng, tk, S, kv_size, ne)
    vt = rng.uniform(-1, 1, size=(S, ne, kv_size)).astype(np.float16)                      # [S][dim][cell]
    q_ = rng.uniform(-1, 1, size=(S, T, n_head, hd)).astype(np.float32)
    masks = stream_masks(S, T, n_kv)
    sk = rng.uniform(-1, 1, size=(n_head,)).astype(np.float32)
    K = Kf[:, :n_kv].reshape(S, n_kv, n_head_kv, hd)
    V = vt.astype(np.float64).transpose(0, 2, 1)[:, :n_kv].reshape(S, n_kv, n_head_kv, hd)
    qr = q_.astype(np.float16).astype(np.float32) if tk == "f16" else q_                    # (an F16 K: q goes through its vec_dot type)
    exp = fa_ref_streams(qr, K, V, masks, 1.0 / np.sqrt(hd), 0.0, 0.0, sk if sinks else None).reshape(S * T, n_head * hd)
    launches = {}
    try:
        with gg.Context() as ctx:
            cur, k_l, v_l, q_cur, m_, s_ = build_chain(ctx, gg, L, S, T, n_kv, n_head, n_head_kv, hd, tk, gg.F32 if mask == "f32" else gg.F16, sinks, kv_size)
            assert ctx.alloc(be)
            gg.tensor_set(k_l, kb); gg.tensor_set(v_l, vt); gg.tensor_set(q_cur, q_); gg.tensor_set(s_, sk)
            gg.tensor_set(m_, masks.astype(np.float32 if mask == "f32" else np.float16))
            graph = gg.graph_of(ctx, cur)
            be.set_option("graphs", 0)
            for fusion in (1, 0):
                be.set_option("fusion", fusion); be.reset_counters()
                be.compute(graph)
                launches[fusion] = be.counters()["kernels_launched"]
                got = gg.tensor_get(cur)[0, 0].copy()                                       # [S*T, hd*n_head]: token t of stream s is row s*T + t
                e = orc.nmse(exp, got)
                print(f"chain streams {S} T {T} K {tk} mask {mask} sinks {sinks} fusion {fusion}: nmse {e:.3e}, launches {launches[fusion]}")
                assert got.shape == exp.shape and e <= NMSE_GATE, (fusion, e)
    finally:
        be.set_option("graphs", 1); be.set_option("fusion", 1)
    assert launches[0] >= 4, launches
    if tk == "q8_0" and T > 8:
        assert launches[1] == launches[0], launches
    else:
        assert launches[1] == 1, launches
