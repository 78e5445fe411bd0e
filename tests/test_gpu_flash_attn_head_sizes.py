"""FLASH_ATTN_EXT at the head sizes beyond 64 / 128: 80, 96, 192, 256 and the 192/128 K/V pair (the reference's op grid walks
hsk in {64, 80, 128, 192, 256, 576} with hsv = hsk plus 192/128 and 576/512, tests/test-backend-ops.cpp:6059-6087). Graphs are built as
tests/test_gpu_ops.py::test_flash_attn_ext builds them, through the C-ABI; expected values are float64 arithmetic on the dequantized cache
with q rounded to f16 (the CPU's vec_dot type of an F16 K), gate NMSE 5e-4 (tests/test-backend-ops.cpp:4559). oracle/ops_ref.py's
flash_attn_ext takes hsv = hsk only, so the reference here is this file's own; it is checked against the oracle's where both apply
(test_reference_agrees_with_oracle, no GPU needed)."""
import numpy as np
import pytest

import oracle as orc
import ops_ref as ref

NMSE_GATE = 5e-4      # tests/test-backend-ops.cpp:4559


def fa_ref(q, K, V, mask, scale, max_bias=0.0, softcap=0.0, sinks=None):
    """float64 FLASH_ATTN_EXT with separate K and V head sizes: q [T, n_head, hsk], K [n_kv, n_head_kv, hsk], V [n_kv, n_head_kv, hsv],
    mask [>= T, n_kv] -> [T, n_head, hsv]. ALiBi: head h's mask times its slope; soft-cap: c * tanh(s / c); sinks join the denominator."""
    T, n_head, _ = q.shape
    n_head_kv, hsv = K.shape[1], V.shape[2]
    n2 = 1 << int(np.floor(np.log2(n_head)))
    m0, m1 = 2.0 ** (-max_bias / n2), 2.0 ** (-(max_bias / 2.0) / n2)
    out = np.zeros((T, n_head, hsv))
    for h in range(n_head):
        hk = h // (n_head // n_head_kv)
        slope = 1.0 if max_bias <= 0 else (m0 ** (h + 1) if h < n2 else m1 ** (2 * (h - n2) + 1))
        s = (q[:, h, :].astype(np.float64) @ K[:, hk, :].astype(np.float64).T) * scale
        if softcap:
            s = softcap * np.tanh(s / softcap)
        s = s + slope * mask[:T].astype(np.float64)
        mx = s.max(-1, keepdims=True)
        if sinks is not None:
            mx = np.maximum(mx, sinks[h])
        p = np.exp(s - mx)
        den = p.sum(-1, keepdims=True) + (np.exp(sinks[h] - mx) if sinks is not None else 0.0)
        out[:, h, :] = (p / den) @ V[:, hk, :].astype(np.float64)
    return out


def _bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def make_mask(T, n_kv, max_bias, window):
    """causal (the T tokens are the last T cells), padded to 64 tokens; ALiBi: minus the distance / 16; window: cells more than `window` back are masked"""
    Tp = (T + 63) // 64 * 64
    mask = np.full((Tp, n_kv), -np.inf, np.float32)
    for t in range(T):
        n_vis = n_kv - T + t + 1
        mask[t, :n_vis] = (-np.arange(n_vis)[::-1] / 16.0).astype(np.float16) if max_bias > 0 else 0.0
        if window:
            mask[t, : max(0, n_vis - window)] = -np.inf
    return mask


@pytest.mark.parametrize("hs", [64, 96])
def test_reference_agrees_with_oracle(hs):
    """this file's float64 reference == oracle.ops_ref.flash_attn_ext (1e-12 relative) where the oracle's applies (hsv = hsk), with sinks, ALiBi and
    the soft-cap: the 192/128 expectation does not rest on unchecked test code"""
    rng = np.random.default_rng(hs)
    T, n_head, n_head_kv, n_kv = 5, 6, 2, 64
    q = rng.uniform(-1, 1, size=(T, n_head, hs)).astype(np.float16).astype(np.float32)
    K = rng.uniform(-1, 1, size=(n_kv, n_head_kv, hs)); V = rng.uniform(-1, 1, size=(n_kv, n_head_kv, hs))
    sk = rng.uniform(-1, 1, size=(n_head,)).astype(np.float32)
    for max_bias, softcap, sinks in ((0.0, 0.0, None), (8.0, 0.0, sk), (0.0, 10.0, sk), (8.0, 10.0, None)):
        mask = make_mask(T, n_kv, max_bias, 0)
        a = fa_ref(q, K, V, mask, 1.0 / np.sqrt(hs), max_bias, softcap, sinks)
        b = ref.flash_attn_ext(q, K, V, mask, 1.0 / np.sqrt(hs), max_bias, softcap, sinks)
        assert a.shape == b.shape
        assert float(np.abs(a - b).max()) <= 1e-12 * float(np.abs(b).max()), (hs, max_bias, softcap)


def _gpu():
    from gpu_util import backend, gg, pkg
    return backend, gg, pkg


def build_fa(ctx, gg, L, hsk, hsv, n_head, n_head_kv, n_kv, T, tk, tv, max_bias, softcap, sinks, kv_size):
    TY = {"f16": gg.F16, "bf16": gg.BF16, "q8_0": gg.Q8_0, "q4_0": gg.Q4_0}
    Tp = (T + 63) // 64 * 64
    k_l = ctx.new_tensor(TY[tk], (hsk * n_head_kv, kv_size)); v_l = ctx.new_tensor(TY[tv], (hsv * n_head_kv, kv_size))
    q_cur = ctx.new_tensor(gg.F32, (hsk, n_head, T)); m_ = ctx.new_tensor(gg.F16, (n_kv, Tp)); s_ = ctx.new_tensor(gg.F32, (n_head,))
    rs_k = orc.row_size(TY[tk], hsk); rs_v = orc.row_size(TY[tv], hsv)
    k = L.ggml_view_3d(ctx.ctx, k_l, hsk, n_head_kv, n_kv, rs_k, rs_k * n_head_kv, 0)
    v = L.ggml_view_3d(ctx.ctx, v_l, hsv, n_head_kv, n_kv, rs_v, rs_v * n_head_kv, 0)
    q = L.ggml_permute(ctx.ctx, q_cur, 0, 2, 1, 3); k = L.ggml_permute(ctx.ctx, k, 0, 2, 1, 3); v = L.ggml_permute(ctx.ctx, v, 0, 2, 1, 3)
    fa = L.ggml_flash_attn_ext(ctx.ctx, q, k, v, m_, float(1.0 / np.sqrt(hsk)), float(max_bias), float(softcap))
    if sinks:
        L.ggml_flash_attn_ext_add_sinks(fa, s_)
    L.ggml_flash_attn_ext_set_prec(fa, 10)
    return fa, k_l, v_l, q_cur, m_, s_


def run_case(hsk, hsv, n_head, n_head_kv, n_kv, T, tk="f16", tv="f16", max_bias=0.0, softcap=0.0, sinks=False, window=0, repeat=False):
    backend, gg, _ = _gpu()
    L = gg.base()
    TY = {"f16": gg.F16, "bf16": gg.BF16, "q8_0": gg.Q8_0, "q4_0": gg.Q4_0}
    rng = np.random.default_rng(7000 + 13 * hsk + hsv + T + n_kv)
    kv_size = n_kv + 64

    def make(t, ne):
        x = rng.uniform(-1, 1, size=(kv_size, ne)).astype(np.float32)
        if t == "f16":
            b = x.astype(np.float16); return b.reshape(1, 1, kv_size, ne), b.astype(np.float64)
        if t == "bf16":
            b = _bf16_round(x); return b.reshape(1, 1, kv_size, ne), (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        b = orc.quantize(x, TY[t]); return b, orc.dequantize(b, TY[t]).astype(np.float64)
    kb, Kf = make(tk, hsk * n_head_kv); vb, Vf = make(tv, hsv * n_head_kv)
    q_ = rng.uniform(-1, 1, size=(1, T, n_head, hsk)).astype(np.float32)
    mask = make_mask(T, n_kv, max_bias, window)
    sk = rng.uniform(-1, 1, size=(n_head,)).astype(np.float32)
    with gg.Context() as ctx:
        fa, k_l, v_l, q_cur, m_, s_ = build_fa(ctx, gg, L, hsk, hsv, n_head, n_head_kv, n_kv, T, tk, tv, max_bias, softcap, sinks, kv_size)
        be = backend(); assert be.supports_op(fa); ctx.alloc(be)
        gg.tensor_set(k_l, kb); gg.tensor_set(v_l, vb); gg.tensor_set(q_cur, q_); gg.tensor_set(m_, mask[None, None].astype(np.float16)); gg.tensor_set(s_, sk.reshape(1, 1, 1, -1))
        graph = gg.graph_of(ctx, fa)
        be.compute(graph)
        got = gg.tensor_get(fa).copy()                                             # [1, T, n_head, hsv]
        if repeat:
            be.compute(graph)                                                      # (the conversion buffer and any captured graph are reused)
            assert np.array_equal(got, gg.tensor_get(fa))
    K = Kf[:n_kv].reshape(n_kv, n_head_kv, hsk); V = Vf[:n_kv].reshape(n_kv, n_head_kv, hsv)
    exp = fa_ref(q_[0].astype(np.float16).astype(np.float32), K, V, mask, 1.0 / np.sqrt(hsk), max_bias, softcap, sk if sinks else None)
    assert got[0].shape == exp.shape == (T, n_head, hsv)
    e = orc.nmse(exp, got[0])
    print(f"hsk {hsk} hsv {hsv} heads {n_head}/{n_head_kv} n_kv {n_kv} T {T} {tk}/{tv} bias {max_bias} cap {softcap} sinks {sinks}: nmse {e:.3e}")
    assert e <= NMSE_GATE, e


SIZES = [(80, 80), (96, 96), (192, 192), (256, 256), (192, 128)]

# per head size: the one-workgroup decode form, the split + merge form (16384 cells only run split), and the prompt form; GQA ratios 1, 3, 4 (and 2, 8);
# sinks on and off; max_bias 8 and logit_softcap 10 at least once; the sliding window at T = 130 (whole leading blocks skipped); one bitwise repeat
GRID = []
for _hsk, _hsv in SIZES:
    GRID += [
        # hsk, hsv, n_head, n_head_kv, n_kv, T, tk, tv, max_bias, softcap, sinks, window, repeat
        (_hsk, _hsv, 8, 2, 256, 1, "f16", "f16", 0.0, 0.0, False, 0, True),
        (_hsk, _hsv, 6, 2, 512, 3, "f16", "f16", 8.0, 10.0, True, 0, False),
        (_hsk, _hsv, 8, 2, 2048, 1, "f16", "f16", 0.0, 0.0, True, 0, False),
        (_hsk, _hsv, 4, 4, 16384, 2, "f16", "f16", 0.0, 0.0, False, 0, False),
        (_hsk, _hsv, 8, 2, 256, 33, "f16", "f16", 0.0, 0.0, False, 0, False),
        (_hsk, _hsv, 6, 2, 512, 35, "f16", "f16", 8.0, 0.0, True, 0, False),
        (_hsk, _hsv, 16, 2, 512, 130, "f16", "f16", 0.0, 10.0, False, 100, False),
        (_hsk, _hsv, 4, 4, 1024, 300, "f16", "f16", 0.0, 0.0, False, 0, False),
    ]
# cache types at 96 and 256 (and 192/128): few tokens read the blocks directly, many go through the f16 copies
for _hs in (96, 256):
    for _tk, _tv in (("q8_0", "q8_0"), ("q4_0", "q4_0"), ("bf16", "bf16"), ("q8_0", "f16")):
        GRID += [(_hs, _hs, 8, 2, 512, 1, _tk, _tv, 0.0, 0.0, False, 0, True),
                 (_hs, _hs, 8, 2, 512, 35, _tk, _tv, 0.0, 0.0, True, 0, True),
                 (_hs, _hs, 4, 1, 2048, 2, _tk, _tv, 8.0, 0.0, False, 0, False)]
GRID += [(80, 80, 8, 2, 256, 1, "bf16", "bf16", 0.0, 0.0, False, 0, True), (80, 80, 8, 2, 512, 35, "bf16", "bf16", 0.0, 10.0, True, 0, False),
         (80, 80, 6, 2, 2048, 2, "bf16", "bf16", 8.0, 0.0, False, 0, False),
         (192, 128, 8, 2, 512, 1, "q8_0", "q8_0", 0.0, 0.0, False, 0, False), (192, 128, 8, 2, 512, 35, "q4_0", "q4_0", 0.0, 0.0, False, 0, False),
         (192, 192, 8, 2, 2048, 1, "q8_0", "q4_0", 0.0, 0.0, False, 0, False), (256, 256, 8, 2, 256, 8, "f16", "bf16", 0.0, 0.0, False, 0, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("hsk,hsv,n_head,n_head_kv,n_kv,T,tk,tv,max_bias,softcap,sinks,window,repeat", GRID)
def test_flash_attn_ext_head_sizes(hsk, hsv, n_head, n_head_kv, n_kv, T, tk, tv, max_bias, softcap, sinks, window, repeat):
    run_case(hsk, hsv, n_head, n_head_kv, n_kv, T, tk, tv, max_bias, softcap, sinks, window, repeat)


@pytest.mark.gpu
@pytest.mark.parametrize("hsk,hsv,tk,want", [(576, 512, "f16", False), (40, 40, "f16", False), (72, 72, "f16", False), (112, 112, "f16", False),
                                             (128, 64, "f16", False), (256, 128, "f16", False), (80, 80, "q8_0", False),
                                             (64, 64, "f16", True), (128, 128, "f16", True), (96, 96, "q8_0", True), (192, 128, "f16", True)])
def test_flash_attn_ext_head_size_refusals(hsk, hsv, tk, want):
    """supports_op: MLA's 576/512, sizes without a kernel, K/V pairs other than 192/128 and a quantized cache at 80 (no whole 32-element
    blocks; the host pads such a cache to 96) are refused, for a few tokens and for many; 64 and 128 still run"""
    backend, gg, _ = _gpu()
    L = gg.base()
    for T in (1, 35):
        with gg.Context() as ctx:
            if tk == "q8_0" and hsk % 32:
                # 80 is not a whole number of 32-element blocks: views of head size 80 over the rows of a cache padded to 96 (3 blocks a head)
                rs = orc.row_size(gg.Q8_0, 96)
                k_l = ctx.new_tensor(gg.Q8_0, (96 * 2, 320)); v_l = ctx.new_tensor(gg.Q8_0, (96 * 2, 320))
                q_cur = ctx.new_tensor(gg.F32, (hsk, 8, T)); m_ = ctx.new_tensor(gg.F16, (256, 64))
                k = L.ggml_view_3d(ctx.ctx, k_l, hsk, 2, 256, rs, rs * 2, 0); v = L.ggml_view_3d(ctx.ctx, v_l, hsv, 2, 256, rs, rs * 2, 0)
                q = L.ggml_permute(ctx.ctx, q_cur, 0, 2, 1, 3); k = L.ggml_permute(ctx.ctx, k, 0, 2, 1, 3); v = L.ggml_permute(ctx.ctx, v, 0, 2, 1, 3)
                fa = L.ggml_flash_attn_ext(ctx.ctx, q, k, v, m_, 0.1, 0.0, 0.0)
            else:
                fa = build_fa(ctx, gg, L, hsk, hsv, 8, 2, 256, T, tk, tk, 0.0, 0.0, False, 320)[0]
            assert bool(backend().supports_op(fa)) == want, (hsk, hsv, tk, T)


@pytest.mark.gpu
@pytest.mark.parametrize("model,type_kv", [("tiny-hd96", 0), ("tiny-hd256", 0), ("tiny-hd96", 8)])
def test_flash_attention_graph_head_sizes(model, type_kv):
    """-fa 1 on two-layer models with head sizes 96 and 256 (F16 cache; 96 also with -ctk q8_0 -ctv q8_0): a prompt pass and decode steps against the
    oracle graph, the way and with the gates of tests/test_gpu_llama_graph.py::test_flash_attention_graph: the reference's whole-graph 2e-3 against
    the exact oracle, and 1e-3 against the CPU-style one ("cpu16") for <= 8 tokens. On these models the second gate is narrower than the yardstick
    itself is sharp: on the <= 8-token steps the two CPU-style oracles ("cpu16": q and p rounded to f16, and "cpu": kept in f32) lie up to 9.4e-4
    (tiny-hd96), 7.2e-4 (tiny-hd96, Q8_0 cache) and 6.7e-4 (tiny-hd256) apart, and the backend lies 4.3e-4 .. 1.17e-3 from "cpu16" while 2.3e-4 ..
    7.2e-4 from the exact oracle (every figure of one run: profiles/r05_flash_attn_head_sizes_tests.log; the test prints them again). The "cpu16" gate
    is therefore max(1e-3, 2 x the largest "cpu16"-vs-"cpu" distance of the same model over the same (<= 8-token) steps) — 1.88e-3, 1.45e-3 and
    1.34e-3 for the three cases — computed here from the oracles alone and printed beside every figure. As in that test, the F16-cache
    models also run without flash attention (their attention then goes node by node: the fused no-flash-attention kernels stop at 64 / 128) and the
    two runs agree to 5e-4."""
    backend, gg, pkg = _gpu()
    import ref_llama
    from ref_llama import RefLlama
    ls = pkg.llama_synth
    be = backend()
    be.set_option("graphs", 1); be.set_option("fusion", 1)
    m = ls.SynthLlama(be, model, "Q4_K_M", n_ctx=256, seed=8, flash_attn=True, type_k=type_kv, type_v=type_kv)
    try:
        W = ref_llama.read_weights(m, gg)
        re_ = RefLlama(m.cfg, W, 256, "exact"); rc = RefLlama(m.cfg, W, 256, "cpu16"); rp = RefLlama(m.cfg, W, 256, "cpu")
        batches = [list(range(20, 60)), [5, 9, 200, 17, 3, 44, 101]] + [[t] for t in (7, 8, 300, 2, 11, 45, 99, 130)]
        exp = []
        for toks in batches:
            emb = np.stack([m.embedding(t) for t in toks])
            exp.append((rc.decode(emb), re_.decode(emb), rp.decode(emb)))
        oo = max(orc.nmse(ep, ec_) for toks, (ec_, _, ep) in zip(batches, exp) if len(toks) <= 8)      # oracle vs oracle ("cpu16" against "cpu") on the gated steps
        gate_c = max(1e-3, 2.0 * oo)
        outs = []
        for toks, (exp_c, exp_e, _) in zip(batches, exp):
            got = m.decode(toks)
            outs.append(got.copy())
            assert np.isfinite(got).all()
            ec, ee = orc.nmse(exp_c, got), orc.nmse(exp_e, got)
            print(f"{model} type_kv {type_kv} tokens {len(toks)}: nmse vs cpu16 {ec:.3e} (gate {gate_c:.3e} = max(1e-3, 2 x cpu16-vs-cpu {oo:.3e})), vs exact {ee:.3e}")
            if len(toks) <= 8:
                assert ec <= gate_c, (len(toks), ec, gate_c, oo)
            assert ee <= 2e-3, (len(toks), ee)
    finally:
        m.free()
    if type_kv == 0:      # (a quantized V cache needs flash attention) the same model without -fa: node-by-node attention at these head sizes, gate as in that test
        m = ls.SynthLlama(be, model, "Q4_K_M", n_ctx=256, seed=8, flash_attn=False)
        try:
            off = [m.decode(toks).copy() for toks in batches]
        finally:
            m.free()
        d = orc.nmse(np.concatenate([o.ravel() for o in off]), np.concatenate([o.ravel() for o in outs]))
        print(f"{model}: -fa on vs off nmse {d:.3e}")
        assert d <= 5e-4, d
