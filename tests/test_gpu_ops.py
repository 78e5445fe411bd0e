"""GPU parity for the remaining ops of the decode graph, each driven as a one-op ggml graph through the
backend C-ABI (the way tests/test-backend-ops.cpp:1082-1240 does) and compared with oracle/ops_ref.py.
Gates are the reference's: default NMSE 1e-7 (tests/test-backend-ops.cpp:948-950), SOFT_MAX / CPY 1e-6,
MUL_MAT / MUL_MAT_ID 5e-4; ROPE within the reference's max asymmetry 1e-3 (:3775)."""
import numpy as np
import pytest

import oracle as orc
import ops_ref as ref
from gpu_util import QTYPES, backend, gg

pytestmark = pytest.mark.gpu
L = gg.base()


def run(ctx, out, inputs):
    be = backend()
    assert be.supports_op(out), "backend refused an op on the path"
    assert ctx.alloc(be)
    for t, arr in inputs:
        gg.tensor_set(t, arr)
    be.compute(gg.graph_of(ctx, out))
    return gg.tensor_get(out)


@pytest.mark.parametrize("ne", [(64, 5, 4, 3), (4096, 1, 1, 1), (4096, 7, 1, 1), (288, 3, 1, 1), (10, 2, 1, 1)])
def test_rms_norm(ne):
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, size=ne[::-1]).astype(np.float32)
    for eps in (0.0, 1e-6, 1e-1):
        with gg.Context() as ctx:
            a = ctx.new_tensor(gg.F32, ne)
            got = run(ctx, L.ggml_rms_norm(ctx.ctx, a, eps), [(a, x)])
        assert orc.nmse(ref.rms_norm(x, eps), got) <= 1e-7


def test_rms_norm_mul_add_fused_matches_unfused():
    """tests/test-backend-ops.cpp:2856 test_rms_norm_mul_add"""
    rng = np.random.default_rng(1)
    ne = (4096, 3, 1, 1)
    x = rng.uniform(-1, 1, size=ne[::-1]).astype(np.float32)
    w = rng.uniform(-1, 1, size=(1, 1, 1, 4096)).astype(np.float32)
    c = rng.uniform(-1, 1, size=ne[::-1]).astype(np.float32)
    outs = {}
    be = backend()
    for fusion in (1, 0):
        be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            a = ctx.new_tensor(gg.F32, ne); b = ctx.new_tensor(gg.F32, (4096,)); d = ctx.new_tensor(gg.F32, ne)
            o = L.ggml_add(ctx.ctx, L.ggml_mul(ctx.ctx, L.ggml_rms_norm(ctx.ctx, a, 1e-5), b), d)
            outs[fusion] = run(ctx, o, [(a, x), (b, w), (d, c)]).copy()
    be.set_option("fusion", 1)
    exp = ref.rms_norm(x, 1e-5) * w + c
    assert orc.nmse(exp, outs[1]) <= 1e-7 and orc.nmse(exp, outs[0]) <= 1e-7
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("op", ["add", "mul", "div"])
@pytest.mark.parametrize("ne,nr", [((4096, 1, 1, 1), (1, 1, 1, 1)), ((64, 5, 3, 2), (1, 1, 1, 1)), ((16, 5, 4, 3), (1, 2, 1, 1)),
                                   ((4096, 8, 1, 1), (1, 8, 1, 1)), ((1, 4, 7, 1), (32, 1, 1, 1))])
def test_bin_bcast(op, ne, nr):
    rng = np.random.default_rng(2)
    ne_a = tuple(n * r for n, r in zip(ne, nr))
    x = rng.uniform(-1, 1, size=ne_a[::-1]).astype(np.float32)
    y = rng.uniform(0.5, 1.5, size=ne[::-1]).astype(np.float32)
    with gg.Context() as ctx:
        a = ctx.new_tensor(gg.F32, ne_a); b = ctx.new_tensor(gg.F32, ne)
        got = run(ctx, getattr(L, f"ggml_{op}")(ctx.ctx, a, b), [(a, x), (b, y)])
    yb = ref.bcast(y.astype(np.float64), x.shape)
    exp = {"add": x + yb, "mul": x * yb, "div": x / yb}[op]
    assert orc.nmse(exp, got) <= 1e-7


def test_scale_and_sum_rows_and_unary():
    rng = np.random.default_rng(3)
    x = rng.uniform(-2, 2, size=(1, 3, 5, 70)).astype(np.float32)
    with gg.Context() as ctx:
        a = ctx.new_tensor(gg.F32, (70, 5, 3))
        got = run(ctx, L.ggml_scale_bias(ctx.ctx, a, 0.37, -1.5), [(a, x)])
    assert orc.nmse(x.astype(np.float64) * 0.37 - 1.5, got) <= 1e-7
    with gg.Context() as ctx:
        a = ctx.new_tensor(gg.F32, (70, 5, 3))
        got = run(ctx, L.ggml_sum_rows(ctx.ctx, a), [(a, x)])
    assert orc.nmse(x.astype(np.float64).sum(-1, keepdims=True), got) <= 1e-7
    for uop, fn in ((gg.UNARY_SILU, ref.silu), (gg.UNARY_SIGMOID, lambda v: 1 / (1 + np.exp(-v.astype(np.float64)))), (gg.UNARY_GELU, ref.gelu)):
        with gg.Context() as ctx:
            a = ctx.new_tensor(gg.F32, (70, 5, 3))
            got = run(ctx, L.ggml_unary(ctx.ctx, a, uop), [(a, x)])
        assert orc.nmse(fn(x), got) <= 1e-6


def test_glu_split_swiglu_and_oai():
    """inputs in +-150 to catch NaN (tests/test-backend-ops.cpp:1882-1886)"""
    rng = np.random.default_rng(4)
    a_ = rng.uniform(-150, 150, size=(1, 1, 7, 128)).astype(np.float32)
    b_ = rng.uniform(-150, 150, size=(1, 1, 7, 128)).astype(np.float32)
    with gg.Context() as ctx:
        a = ctx.new_tensor(gg.F32, (128, 7)); b = ctx.new_tensor(gg.F32, (128, 7))
        got = run(ctx, L.ggml_swiglu_split(ctx.ctx, a, b), [(a, a_), (b, b_)])
    assert np.isfinite(got).all() and orc.nmse(ref.swiglu(a_, b_), got) <= 1e-7
    with gg.Context() as ctx:
        a = ctx.new_tensor(gg.F32, (128, 7)); b = ctx.new_tensor(gg.F32, (128, 7))
        got = run(ctx, L.ggml_swiglu_oai(ctx.ctx, a, b, 1.702, 7.0), [(a, a_), (b, b_)])
    assert np.isfinite(got).all() and orc.nmse(ref.swiglu_oai(a_, b_), got) <= 1e-7
    # strided (non-contiguous rows) inputs: views of a wider tensor, as build_ffn's fused gate_up produces
    wide = rng.uniform(-5, 5, size=(1, 1, 7, 256)).astype(np.float32)
    with gg.Context() as ctx:
        t = ctx.new_tensor(gg.F32, (256, 7))
        va = L.ggml_view_2d(ctx.ctx, t, 128, 7, 256 * 4, 0)
        vb = L.ggml_view_2d(ctx.ctx, t, 128, 7, 256 * 4, 128 * 4)
        got = run(ctx, L.ggml_swiglu_split(ctx.ctx, va, vb), [(t, wide)])
    assert orc.nmse(ref.swiglu(wide[..., :128], wide[..., 128:]), got) <= 1e-7


@pytest.mark.parametrize("mode", [0, gg.GGML_ROPE_TYPE_NEOX])
@pytest.mark.parametrize("with_ff,ext", [(False, 0.0), (True, 0.0), (False, 1.0)])
def test_rope(mode, with_ff, ext):
    """model-shaped cases tests/test-backend-ops.cpp:5975-6005: head 128 x 32 heads, n_dims = 128 and partial 64"""
    rng = np.random.default_rng(5)
    for n_dims, heads, ntok in ((128, 32, 3), (64, 8, 2)):
        x = rng.uniform(-1, 1, size=(1, ntok, heads, 128)).astype(np.float32)
        pos = rng.integers(0, 500, size=ntok).astype(np.int32)
        ff = rng.uniform(0.9, 1.1, size=n_dims // 2).astype(np.float32)
        fs = 0.5 if ext else 1.0
        with gg.Context() as ctx:
            a = ctx.new_tensor(gg.F32, (128, heads, ntok)); p = ctx.new_tensor(gg.I32, (ntok,))
            f = ctx.new_tensor(gg.F32, (n_dims // 2,)) if with_ff else None
            o = L.ggml_rope_ext(ctx.ctx, a, p, f, n_dims, mode, 8192, 500000.0, fs, ext, 1.0, 32.0, 1.0)
            got = run(ctx, o, [(a, x), (p, pos)] + ([(f, ff)] if with_ff else []))
        exp = ref.rope(x, pos, n_dims, mode, 8192, 500000.0, fs, ext, 1.0, 32.0, 1.0, ff if with_ff else None)
        assert orc.nmse(exp, got) <= 1e-6
        assert np.abs(exp - got).max() <= 1e-3


@pytest.mark.parametrize("ne0,ne1,heads", [(32, 1, 32), (128, 1, 32), (96, 7, 8), (1000, 3, 4), (4100, 2, 2)])
@pytest.mark.parametrize("mask_t,max_bias,sinks", [(None, 0.0, False), (gg.F32, 0.0, False), (gg.F16, 0.0, True), (gg.F32, 8.0, False)])
def test_soft_max(ne0, ne1, heads, mask_t, max_bias, sinks):
    rng = np.random.default_rng(6)
    x = rng.uniform(-4, 4, size=(1, heads, ne1, ne0)).astype(np.float32)
    ne1p = (ne1 + 63) // 64 * 64            # GGML_KQ_MASK_PAD (src/llama-graph.cpp:1421)
    m = rng.uniform(-1, 0, size=(1, 1, ne1p, ne0)).astype(np.float32)
    m[..., ne0 // 2:] = -np.inf               # causal-style masking
    m[..., 0] = 0
    sk = rng.uniform(-1, 1, size=heads).astype(np.float32)
    with gg.Context() as ctx:
        a = ctx.new_tensor(gg.F32, (ne0, ne1, heads))
        mt = ctx.new_tensor(mask_t, (ne0, ne1p)) if mask_t is not None else None
        o = L.ggml_soft_max_ext(ctx.ctx, a, mt, 0.125, max_bias)
        ins = [(a, x)]
        if mt is not None:
            ins.append((mt, m if mask_t == gg.F32 else m.astype(np.float16)))
        if sinks:
            s = ctx.new_tensor(gg.F32, (heads,)); L.ggml_soft_max_add_sinks(o, s); ins.append((s, sk))
        got = run(ctx, o, ins)
    mm = None if mask_t is None else (m if mask_t == gg.F32 else m.astype(np.float16).astype(np.float32))
    exp = ref.soft_max(x, mm, 0.125, max_bias, sk if sinks else None)
    assert np.isfinite(got).all() and orc.nmse(exp, got) <= 1e-6


@pytest.mark.parametrize("dst_t", [gg.F16, gg.F32])
def test_set_rows_kv_write(dst_t):
    """K write: [1024, n_tok] f32 rows scattered into the f16 cache [1024, kv_size] by I64 indices
    (src/llama-kv-cache-unified.cpp:1123); V-transposed write: element scatter on a [1, N] view (:1157-1167)."""
    rng = np.random.default_rng(7)
    n_embd, kv, ntok = 1024, 64, 5
    cache0 = rng.uniform(-1, 1, size=(1, 1, kv, n_embd)).astype(np.float16 if dst_t == gg.F16 else np.float32)
    cur = rng.uniform(-1, 1, size=(1, 1, ntok, n_embd)).astype(np.float32)
    idx = rng.permutation(kv)[:ntok].astype(np.int64)
    with gg.Context() as ctx:
        c = ctx.new_tensor(dst_t, (n_embd, kv)); s = ctx.new_tensor(gg.F32, (n_embd, ntok)); i = ctx.new_tensor(gg.I64, (ntok,))
        o = L.ggml_set_rows(ctx.ctx, c, s, i)
        be = backend(); assert be.supports_op(o); ctx.alloc(be)
        gg.tensor_set(c, cache0); gg.tensor_set(s, cur); gg.tensor_set(i, idx)
        be.compute(gg.graph_of(ctx, o))
        got = gg.tensor_get(c)
    exp = ref.set_rows(cache0, cur, idx.reshape(1, 1, ntok))
    assert np.array_equal(got, exp)          # f32 -> f16 conversion is exact-rounding on both sides
    # element scatter (v_trans): dst viewed as [1, kv*n_embd], one I64 index per element
    n_el = ntok * 16
    flat0 = rng.uniform(-1, 1, size=(1, 1, 1, kv * 16)).astype(np.float16 if dst_t == gg.F16 else np.float32)
    vals = rng.uniform(-1, 1, size=(1, 1, n_el, 1)).astype(np.float32)
    eidx = rng.permutation(kv * 16)[:n_el].astype(np.int64)
    with gg.Context() as ctx:
        c = ctx.new_tensor(dst_t, (kv * 16,)); s = ctx.new_tensor(gg.F32, (1, n_el)); i = ctx.new_tensor(gg.I64, (n_el,))
        cv = L.ggml_reshape_2d(ctx.ctx, c, 1, kv * 16)
        o = L.ggml_set_rows(ctx.ctx, cv, s, i)
        be = backend(); assert be.supports_op(o); ctx.alloc(be)
        gg.tensor_set(c, flat0); gg.tensor_set(s, vals); gg.tensor_set(i, eidx)
        be.compute(gg.graph_of(ctx, o))
        got = gg.tensor_get(c)
    exp = flat0.copy(); exp[0, 0, 0, eidx] = vals[0, 0, :, 0].astype(exp.dtype)
    assert np.array_equal(got, exp)


def test_get_rows_and_cpy_cont():
    rng = np.random.default_rng(8)
    src = rng.uniform(-1, 1, size=(1, 1, 50, 96)).astype(np.float32)
    idx = rng.integers(0, 50, size=(1, 1, 9)).astype(np.int32)
    with gg.Context() as ctx:
        a = ctx.new_tensor(gg.F32, (96, 50)); i = ctx.new_tensor(gg.I32, (9,))
        got = run(ctx, L.ggml_get_rows(ctx.ctx, a, i), [(a, src), (i, idx)])
    assert np.array_equal(got[0, 0], src[0, 0][idx[0, 0]])
    # CONT of a permuted tensor (src/llama-graph.cpp:1327-1330: kqv permute(0,2,1,3) then cont_2d)
    x = rng.uniform(-1, 1, size=(1, 4, 6, 32)).astype(np.float32)      # ggml ne = (32, 6, 4)
    with gg.Context() as ctx:
        a = ctx.new_tensor(gg.F32, (32, 6, 4))
        p = L.ggml_permute(ctx.ctx, a, 0, 2, 1, 3)                       # -> ne (32, 4, 6)
        got = run(ctx, L.ggml_cont_2d(ctx.ctx, p, 32 * 4, 6), [(a, x)])
    assert np.array_equal(got[0, 0], x[0].transpose(1, 0, 2).reshape(6, 128))
    # CPY f32 -> f16 (legacy KV path, src/llama-kv-cache-unified.cpp:1135)
    with gg.Context() as ctx:
        a = ctx.new_tensor(gg.F32, (32, 6, 4)); d = ctx.new_tensor(gg.F16, (32, 6, 4))
        o = L.ggml_cpy(ctx.ctx, a, d)
        be = backend(); ctx.alloc(be); gg.tensor_set(a, x); be.compute(gg.graph_of(ctx, o))
        got = gg.tensor_get(d)
    assert np.array_equal(got, x.astype(np.float16))


def test_add_id_and_argsort_topk():
    rng = np.random.default_rng(9)
    n_expert, n_used, ntok, ne0 = 32, 4, 3, 2880
    a_ = rng.uniform(-1, 1, size=(1, ntok, n_used, ne0)).astype(np.float32)
    bias = rng.uniform(-1, 1, size=(1, 1, n_expert, ne0)).astype(np.float32)
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(ntok)]).astype(np.int32)
    with gg.Context() as ctx:
        a = ctx.new_tensor(gg.F32, (ne0, n_used, ntok)); b = ctx.new_tensor(gg.F32, (ne0, n_expert)); i = ctx.new_tensor(gg.I32, (n_used, ntok))
        got = run(ctx, L.ggml_add_id(ctx.ctx, a, b, i), [(a, a_), (b, bias), (i, ids.reshape(1, 1, ntok, n_used))])
    assert orc.nmse(ref.add_id(a_[0], bias[0, 0], ids), got[0]) <= 1e-7
    # argsort desc (+ top_k view) over router logits
    for ne0 in (8, 32, 100, 128):
        logits = rng.permutation(ne0 * 5).astype(np.float32).reshape(1, 1, 5, ne0)   # distinct values: order is unique
        with gg.Context() as ctx:
            a = ctx.new_tensor(gg.F32, (ne0, 5))
            got = run(ctx, L.ggml_argsort(ctx.ctx, a, gg.GGML_SORT_ORDER_DESC), [(a, logits)])
        assert np.array_equal(got, ref.argsort_desc(logits))


@pytest.mark.parametrize("n_expert,k,bias,softmax", [(8, 4096, False, True), (32, 2880, True, False), (32, 2880, False, True), (128, 2048, False, True),
                                                    (128, 4096, True, False), (256, 7168, False, True)])
def test_moe_router_at_model_widths(n_expert, k, bias, softmax):
    """build_moe_ffn's router for one token (src/llama-graph.cpp:838-883): logits = gate_inp . x (+ bias) [-> soft_max] -> argsort desc, at the
    widths of Mixtral (8 x 4096), gpt-oss (32 x 2880, bias, SOFTMAX_WEIGHT gating: the logits are ranked) and the 128 / 256-expert models the
    reference's perf cases name (tests/test-backend-ops.cpp:6226-6229). From 16 experts on this is k_moe_route_wide: one workgroup per 16
    experts, every logit handed to the ranking workgroup as an 8-byte {value, launch tag} granule that workgroup polls — run three times on
    the same buffers so that stale granules of the launch before would be caught."""
    rng = np.random.default_rng(n_expert + k)
    w_ = (rng.standard_normal((1, 1, n_expert, k))/np.sqrt(k)).astype(np.float32)
    b_ = rng.uniform(-0.5, 0.5, size=(1, 1, 1, n_expert)).astype(np.float32)
    be = backend(); be.set_option("fusion", 1)
    with gg.Context() as ctx:
        w = ctx.new_tensor(gg.F32, (k, n_expert)); x = ctx.new_tensor(gg.F32, (k, 1)); bt = ctx.new_tensor(gg.F32, (n_expert,))
        lg = L.ggml_mul_mat(ctx.ctx, w, x)
        if bias:
            lg = L.ggml_add(ctx.ctx, lg, bt)
        pr = L.ggml_soft_max(ctx.ctx, lg) if softmax else lg
        srt = L.ggml_argsort(ctx.ctx, pr, gg.GGML_SORT_ORDER_DESC)
        assert ctx.alloc(be)
        gg.tensor_set(w, w_); gg.tensor_set(bt, b_)
        graph = gg.graph_of(ctx, srt, pr)
        for rep in range(3):
            x_ = rng.standard_normal((1, 1, 1, k)).astype(np.float32)
            gg.tensor_set(x, x_)
            be.reset_counters()
            be.compute(graph)
            assert be.counters()["kernels_launched"] == 1, be.counters()      # the whole router is ONE launch
            got_p = gg.tensor_get(pr)[0, 0, 0].copy(); got_s = gg.tensor_get(srt)[0, 0, 0].copy()
            logits = w_[0, 0].astype(np.float64) @ x_[0, 0, 0].astype(np.float64) + (b_[0, 0, 0] if bias else 0.0)
            exp_p = np.exp(logits - logits.max())/np.exp(logits - logits.max()).sum() if softmax else logits
            assert np.abs(got_p - exp_p).max() <= 1e-5*max(1.0, np.abs(exp_p).max()), (rep, float(np.abs(got_p - exp_p).max()))
            # the ranking must be THE descending order of the values the kernel itself produced (index breaks ties, as ggml's argsort leaves them)
            assert sorted(got_s.tolist()) == list(range(n_expert))
            assert np.all(np.diff(got_p[got_s]) <= 0), rep
            top = np.argsort(-exp_p, kind="stable")[:4]
            if np.min(np.abs(np.diff(np.sort(exp_p)[::-1][:5]))) > 1e-4*np.abs(exp_p).max():      # no near-tie among the leaders: the choice is the oracle's
                assert np.array_equal(got_s[:4], top), (rep, got_s[:4], top)


@pytest.mark.parametrize("tname", ["f16", "f32"])
@pytest.mark.parametrize("n_mats,n_used,bcast_b,n", [(4, 2, True, 1), (8, 2, False, 5), (8, 4, False, 40)])
def test_mul_mat_id_unquantized_expert_stack(tname, n_mats, n_used, bcast_b, n):
    """MUL_MAT_ID over an F16 / F32 expert stack (tests/test-backend-ops.cpp:5821-5824 with base_types F32, F16 :5241-5249): the product against float64;
    F16 weights round src1 to F16 first, as ggml-cpu's vec_dot_f16 does (the oracle does the same)."""
    rng = np.random.default_rng(21 + n)
    m, k = 48, 160
    t = gg.F16 if tname == "f16" else gg.F32
    w = rng.uniform(-1, 1, size=(n_mats, m, k)).astype(np.float16 if tname == "f16" else np.float32)
    ids_full = np.stack([rng.permutation(n_mats) for _ in range(n)]).astype(np.int32)
    nb = 1 if bcast_b else n_used
    b_ = rng.uniform(-1, 1, size=(1, n, nb, k)).astype(np.float32)
    with gg.Context() as ctx:
        as_ = ctx.new_tensor(t, (k, m, n_mats)); ids = ctx.new_tensor(gg.I32, (n_mats, n)); b = ctx.new_tensor(gg.F32, (k, nb, n))
        idv = L.ggml_view_2d(ctx.ctx, ids, n_used, n, n_mats * 4, 0)
        got = run(ctx, L.ggml_mul_mat_id(ctx.ctx, as_, b, idv), [(as_, w.reshape(1, n_mats, m, k)), (ids, ids_full.reshape(1, 1, n, n_mats)), (b, b_)])
    bb = b_[0].astype(np.float16).astype(np.float64) if tname == "f16" else b_[0].astype(np.float64)
    exp = np.empty((n, n_used, m))
    for tk in range(n):
        for u in range(n_used):
            exp[tk, u] = w[ids_full[tk, u]].astype(np.float64) @ bb[tk, u % nb]
    assert orc.nmse(exp, got[0]) <= 1e-7


@pytest.mark.parametrize("name", list(QTYPES))
@pytest.mark.parametrize("n_mats,n_used,bcast_b,n", [(4, 1, False, 1), (4, 2, True, 1), (8, 2, False, 1), (8, 4, False, 5), (8, 2, True, 32), (8, 8, False, 3)])
def test_mul_mat_id(name, n_mats, n_used, bcast_b, n):
    """tests/test-backend-ops.cpp:5821-5856; ids = a strided view of a shuffled [n_mats, n] tensor (:3231-3236)"""
    rng = np.random.default_rng(10 + n)
    m, k = 64, 256
    qt = QTYPES[name]
    w = orc.random_blocks(rng, qt, (n_mats, m), k)
    ids_full = np.stack([rng.permutation(n_mats) for _ in range(n)]).astype(np.int32)
    nb = 1 if bcast_b else n_used
    b_ = rng.uniform(-1, 1, size=(1, n, nb, k)).astype(np.float32)
    with gg.Context() as ctx:
        as_ = ctx.new_tensor(qt, (k, m, n_mats)); ids = ctx.new_tensor(gg.I32, (n_mats, n)); b = ctx.new_tensor(gg.F32, (k, nb, n))
        idv = L.ggml_view_2d(ctx.ctx, ids, n_used, n, n_mats * 4, 0) if n_used != n_mats else ids
        got = run(ctx, L.ggml_mul_mat_id(ctx.ctx, as_, b, idv), [(as_, w), (ids, ids_full.reshape(1, 1, n, n_mats)), (b, b_)])
    exp = orc.mul_mat_id(w, qt, b_[0], ids_full[:, :n_used], "exact")
    cpu = orc.mul_mat_id(w, qt, b_[0], ids_full[:, :n_used], "cpu")
    assert orc.nmse(exp, got[0]) <= 5e-4
    if n_used * n <= 32:      # the int8-activation mat-vec path; more pairs go through bf16 tiles on the matrix cores (NMSE gate only)
        assert np.abs(got[0] - cpu).max() <= 2e-5 * (np.abs(cpu).max() + 1e-30)


@pytest.mark.parametrize("name", list(QTYPES))
@pytest.mark.parametrize("n_mats,n_used,bcast_b,n,m,k", [(8, 2, True, 512, 192, 512), (32, 4, False, 130, 64, 256), (8, 2, False, 300, 320, 1024)])
def test_mul_mat_id_prefill_grouped(name, n_mats, n_used, bcast_b, n, m, k):
    """MUL_MAT_ID with many tokens (Mixtral 8/2 and gpt-oss 32/4 routing at pp sizes, tests/test-backend-ops.cpp:5821-5856 perf cases
    :6226-6229): the (token, slot) pairs are sorted by expert on the device and run as MFMA tiles. Ragged on purpose: expert loads that
    are not multiples of the 128-pair tile, m not a multiple of 128, ids a strided view."""
    rng = np.random.default_rng(77 + n)
    qt = QTYPES[name]
    w = orc.random_blocks(rng, qt, (n_mats, m), k)
    ids_full = np.stack([rng.permutation(n_mats) for _ in range(n)]).astype(np.int32)
    ids_full[: n // 3, 0] = 1                       # an overloaded expert, so that one expert spans several tiles
    nb = 1 if bcast_b else n_used
    b_ = rng.uniform(-1, 1, size=(1, n, nb, k)).astype(np.float32)
    with gg.Context() as ctx:
        as_ = ctx.new_tensor(qt, (k, m, n_mats)); ids = ctx.new_tensor(gg.I32, (n_mats, n)); b = ctx.new_tensor(gg.F32, (k, nb, n))
        idv = L.ggml_view_2d(ctx.ctx, ids, n_used, n, n_mats * 4, 0)
        got = run(ctx, L.ggml_mul_mat_id(ctx.ctx, as_, b, idv), [(as_, w), (ids, ids_full.reshape(1, 1, n, n_mats)), (b, b_)])
    # dequantized weights in float64 (the exact oracle), vectorised per expert: the per-pair oracle loop is too slow at this size
    wd = orc.dequantize(w.reshape(n_mats * m, -1), qt).reshape(n_mats, m, k).astype(np.float64)
    exp = np.empty((n, n_used, m))
    for t in range(n):
        for u in range(n_used):
            exp[t, u] = wd[ids_full[t, u]] @ b_[0, t, u % nb].astype(np.float64)
    assert got[0].shape == exp.shape
    assert orc.nmse(exp, got[0]) <= 5e-4, orc.nmse(exp, got[0])


@pytest.mark.parametrize("gname,dname,n_mats,n_used,n,m,k,biased,oai,weighted", [
    ("q4_K", "q4_K", 8, 2, 512, 256, 512, False, False, True),      # Mixtral: swiglu, no biases, the routing-weight multiply; ~128 pairs per expert: gate and up as two launches
    ("mxfp4", "mxfp4", 4, 2, 300, 320, 320, True, True, True),      # ... the two-launch form with biases and swiglu_oai
    ("q4_K", "q4_K", 8, 2, 300, 256, 512, False, False, True),      # fewer pairs per expert: the dual launch
    ("q4_K", "q6_K", 8, 2, 150, 256, 256, False, False, True),      # ... its Q6_K down matrices
    ("mxfp4", "mxfp4", 32, 4, 130, 320, 320, True, True, True),     # gpt-oss: ADD_ID biases, swiglu_oai, 10-block rows
    ("q8_0", "q4_0", 8, 2, 70, 128, 256, True, False, False),       # the chain ends at the ADD_ID
    ("q5_K", "q5_K", 4, 2, 40, 256, 256, False, True, False),        # ... at the down product
])
def test_moe_expert_chain_many_tokens(gname, dname, n_mats, n_used, n, m, k, biased, oai, weighted):
    """The experts of build_moe_ffn for a prompt pass (src/llama-graph.cpp:914-990): MUL_MAT_ID(up) [ADD_ID]; MUL_MAT_ID(gate) [ADD_ID]; swiglu | swiglu_oai;
    MUL_MAT_ID(down) [ADD_ID] [MUL weights]. With fusions on this is one copy, one dual tile launch and one down launch (+ a sort each) (backend_nodes.cpp try_fused_prefill_moe);
    with fusions off, node by node. Both against the exact product of the dequantized weights (bf16 operands: the MUL_MAT_ID gate), and against each other:
    the fused chain rounds the same values to bf16 at the same places, so only the ragged last digits of expf differ."""
    rng = np.random.default_rng(500 + n)
    gt, dt = QTYPES[gname], QTYPES[dname]
    wu = orc.random_blocks(rng, gt, (n_mats, m), k); wg = orc.random_blocks(rng, gt, (n_mats, m), k); wd = orc.random_blocks(rng, dt, (n_mats, k), m)
    ids_full = np.stack([rng.permutation(n_mats) for _ in range(n)]).astype(np.int32)
    ids_full[: n // 3, 0] = 1                       # an overloaded expert
    x_ = rng.uniform(-1, 1, size=(1, n, 1, k)).astype(np.float32)
    bu_ = rng.uniform(-1, 1, size=(1, 1, n_mats, m)).astype(np.float32); bg_ = rng.uniform(-1, 1, size=(1, 1, n_mats, m)).astype(np.float32)
    bd_ = rng.uniform(-1, 1, size=(1, 1, n_mats, k)).astype(np.float32)
    wt_ = rng.uniform(0.1, 1, size=(1, n, n_used, 1)).astype(np.float32)
    be = backend(); outs = {}
    for fusion in (1, 0):
        be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            up_w = ctx.new_tensor(gt, (k, m, n_mats)); gate_w = ctx.new_tensor(gt, (k, m, n_mats)); down_w = ctx.new_tensor(dt, (m, k, n_mats))
            ids = ctx.new_tensor(gg.I32, (n_mats, n)); x = ctx.new_tensor(gg.F32, (k, 1, n)); wt = ctx.new_tensor(gg.F32, (1, n_used, n))
            bu = ctx.new_tensor(gg.F32, (m, n_mats)); bg = ctx.new_tensor(gg.F32, (m, n_mats)); bd = ctx.new_tensor(gg.F32, (k, n_mats))
            idv = L.ggml_view_2d(ctx.ctx, ids, n_used, n, n_mats * 4, 0)
            up = L.ggml_mul_mat_id(ctx.ctx, up_w, x, idv)
            if biased: up = L.ggml_add_id(ctx.ctx, up, bu, idv)
            gate = L.ggml_mul_mat_id(ctx.ctx, gate_w, x, idv)
            if biased: gate = L.ggml_add_id(ctx.ctx, gate, bg, idv)
            act = L.ggml_swiglu_oai(ctx.ctx, gate, up, 1.702, 7.0) if oai else L.ggml_swiglu_split(ctx.ctx, gate, up)
            o = L.ggml_mul_mat_id(ctx.ctx, down_w, act, idv)
            if biased: o = L.ggml_add_id(ctx.ctx, o, bd, idv)
            if weighted: o = L.ggml_mul(ctx.ctx, o, wt)
            be.reset_counters()
            outs[fusion] = run(ctx, o, [(up_w, wu), (gate_w, wg), (down_w, wd), (ids, ids_full.reshape(1, 1, n, n_mats)), (x, x_), (wt, wt_), (bu, bu_), (bg, bg_), (bd, bd_)])[0].copy()
            if fusion: assert be.counters()["kernels_launched"] in (4, 5), be.counters()       # copy, sort, dual launch, down launch | copy, sort, up launch, gate launch, down launch
    be.set_option("fusion", 1)
    du = orc.dequantize(wu.reshape(n_mats * m, -1), gt).reshape(n_mats, m, k).astype(np.float64)
    dg = orc.dequantize(wg.reshape(n_mats * m, -1), gt).reshape(n_mats, m, k).astype(np.float64)
    dd = orc.dequantize(wd.reshape(n_mats * k, -1), dt).reshape(n_mats, k, m).astype(np.float64)
    exp = np.empty((n, n_used, k))
    for t in range(n):
        for u in range(n_used):
            e = ids_full[t, u]
            a = du[e] @ x_[0, t, 0].astype(np.float64) + (bu_[0, 0, e] if biased else 0.0)
            g_ = dg[e] @ x_[0, t, 0].astype(np.float64) + (bg_[0, 0, e] if biased else 0.0)
            if oai:
                xc = np.minimum(g_, 7.0); gc = np.clip(a, -7.0, 7.0); h = xc / (1.0 + np.exp(-1.702 * xc)) * (gc + 1.0)
            else:
                h = g_ / (1.0 + np.exp(-g_)) * a
            y = dd[e] @ h + (bd_[0, 0, e] if biased else 0.0)
            exp[t, u] = y * (wt_[0, t, u, 0] if weighted else 1.0)
    assert outs[1].shape == exp.shape
    assert orc.nmse(exp, outs[1]) <= 5e-4 and orc.nmse(exp, outs[0]) <= 5e-4, (orc.nmse(exp, outs[1]), orc.nmse(exp, outs[0]))
    assert orc.nmse(outs[0], outs[1]) <= 1e-6, orc.nmse(outs[0], outs[1])


@pytest.mark.parametrize("name,k", [("q8_0", 320), ("q4_K", 512)])
def test_prompt_pass_qkv_with_bias_rows(name, k):
    """gpt-oss's attention projections in a prompt pass (src/llama-model.cpp:17636-17645): MUL_MAT(wq) + bq, MUL_MAT(wk) + bk, MUL_MAT(wv) + bv on the same 512
    tokens. Fused: ONE grouped launch (k = 2880 does not split, 80 tiles) with the bias rows added in its epilogue (backend_nodes.cpp try_fused_prefill_qkv); node by node:
    three launches and three ADDs. Same operands, same order of accumulation: the same bits; and the exact product within the MUL_MAT gate."""
    rng = np.random.default_rng(31)
    qt = QTYPES[name]; n = 512; ms = (4096, 512, 512)
    ws = [orc.random_blocks(rng, qt, (m,), k) for m in ms]
    bs = [rng.uniform(-1, 1, size=(1, 1, 1, m)).astype(np.float32) for m in ms]
    x_ = rng.uniform(-1, 1, size=(1, 1, n, k)).astype(np.float32)
    be = backend(); outs = {}
    for fusion in (1, 0):
        be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            x = ctx.new_tensor(gg.F32, (k, n))
            wt = [ctx.new_tensor(qt, (k, m)) for m in ms]; bt = [ctx.new_tensor(gg.F32, (m,)) for m in ms]
            o = [L.ggml_add(ctx.ctx, L.ggml_mul_mat(ctx.ctx, w, x), b) for w, b in zip(wt, bt)]
            gf = gg.graph_of(ctx, *o)
            assert ctx.alloc(be)
            for t, a in list(zip(wt, ws)) + list(zip(bt, bs)) + [(x, x_)]: gg.tensor_set(t, a)
            be.reset_counters(); be.compute(gf)
            outs[fusion] = [gg.tensor_get(t)[0, 0].copy() for t in o]
            if fusion: assert be.counters()["kernels_launched"] == 2, be.counters()      # the bf16 copy of x, the grouped launch
    be.set_option("fusion", 1)
    for q in range(3):
        exp = orc.dequantize(ws[q], qt).astype(np.float64) @ x_[0, 0].astype(np.float64).T + bs[q][0, 0, 0][:, None].astype(np.float64)
        assert orc.nmse(exp.T, outs[1][q]) <= 5e-4
        assert np.array_equal(outs[1][q], outs[0][q]), (q, orc.nmse(outs[0][q], outs[1][q]))


def test_prompt_pass_qkv_with_bias_rows_on_a_split_k():
    """The one fall-back of try_fused_prefill_qkv: bias rows on a grouped launch whose k splits. q4_K, k = 2048, rows (4096, 512, 512), 512 tokens: 40 m-tiles x 2 token
    tiles = 80 tiles, so k splits in two and the launcher does not take the bias rows (they ride on the epilogue only). The matcher then takes the plain grouped launch
    and runs the three ADDs behind it. Against the exact product: the bound of test_prefill_qkv_group, the same launch form. Against fusion off: the same bits (measured on
    the commit before the launchers took call records: the one-by-one launches split this k in two as well, and the planes and the bias are added in the same order)."""
    rng = np.random.default_rng(32)
    qt = QTYPES["q4_K"]; n = 512; k = 2048; ms = (4096, 512, 512)
    ws = [orc.random_blocks(rng, qt, (m,), k) for m in ms]
    bs = [rng.uniform(-1, 1, size=(1, 1, 1, m)).astype(np.float32) for m in ms]
    x_ = rng.uniform(-1, 1, size=(1, 1, n, k)).astype(np.float32)
    be = backend(); outs = {}
    for fusion in (1, 0):
        be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            x = ctx.new_tensor(gg.F32, (k, n))
            wt = [ctx.new_tensor(qt, (k, m)) for m in ms]; bt = [ctx.new_tensor(gg.F32, (m,)) for m in ms]
            o = [L.ggml_add(ctx.ctx, L.ggml_mul_mat(ctx.ctx, w, x), b) for w, b in zip(wt, bt)]
            gf = gg.graph_of(ctx, *o)
            assert ctx.alloc(be)
            for t, a in list(zip(wt, ws)) + list(zip(bt, bs)) + [(x, x_)]: gg.tensor_set(t, a)
            be.reset_counters(); be.compute(gf)
            outs[fusion] = [gg.tensor_get(t)[0, 0].copy() for t in o]
            if fusion:
                cnt = be.counters()
                assert cnt["mmq_launches"] == 1, cnt
                # the value the commit before the launchers took call records gives for this graph (run there once): the bf16 copy of x, the grouped launch, three ADDs
                # (the pass that combines the two planes is not counted: DESIGN.md §6)
                assert cnt["kernels_launched"] == 5, cnt
    be.set_option("fusion", 1)
    for q in range(3):
        exp = orc.dequantize(ws[q], qt).astype(np.float64) @ x_[0, 0].astype(np.float64).T + bs[q][0, 0, 0][:, None].astype(np.float64)
        assert orc.nmse(exp.T, outs[1][q]) <= 2e-5, (q, orc.nmse(exp.T, outs[1][q]))
        assert np.array_equal(outs[1][q], outs[0][q]), (q, orc.nmse(outs[0][q], outs[1][q]))


@pytest.mark.parametrize("n_used,with_res", [(2, True), (4, True), (4, False), (8, True)])
def test_moe_slot_sum_many_tokens(n_used, with_res):
    """The end of build_moe_ffn for a prompt pass (src/llama-graph.cpp:996-1012 + the residual ADD of src/llama-model.cpp:6096): the ADD chain over the slot views of
    the experts' outputs, fused into one pass (backend_nodes.cpp try_fused_slot_sum) — bit-identical to node-by-node execution, same order of additions."""
    rng = np.random.default_rng(900 + n_used)
    m, n = 320, 37
    ex_ = rng.uniform(-1, 1, size=(1, n, n_used, m)).astype(np.float32); res_ = rng.uniform(-1, 1, size=(1, 1, n, m)).astype(np.float32)
    be = backend(); outs = {}
    for fusion in (1, 0):
        be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            ex = ctx.new_tensor(gg.F32, (m, n_used, n)); res = ctx.new_tensor(gg.F32, (m, n))
            views = [L.ggml_view_2d(ctx.ctx, ex, m, n, n_used * m * 4, u * m * 4) for u in range(n_used)]
            o = views[0]
            for u in range(1, n_used): o = L.ggml_add(ctx.ctx, o, views[u])
            if with_res: o = L.ggml_add(ctx.ctx, o, res)
            be.reset_counters()
            outs[fusion] = run(ctx, o, [(ex, ex_), (res, res_)])[0, 0].copy()
            if fusion: assert be.counters()["kernels_launched"] == 1, be.counters()
    be.set_option("fusion", 1)
    exp = ex_[0, :, 0]
    for u in range(1, n_used): exp = exp + ex_[0, :, u]
    if with_res: exp = exp + res_[0, 0]
    assert np.array_equal(outs[1], outs[0]) and np.array_equal(outs[1], exp.astype(np.float32))


@pytest.mark.parametrize("name", list(QTYPES))
def test_mul_mat_id_golden(name, golden_dir):
    g = np.load(golden_dir / f"mulmatid_{name}.npz")
    n_mats, m, _ = g["w"].shape; n, n_used, k = g["b"].shape
    with gg.Context() as ctx:
        as_ = ctx.new_tensor(QTYPES[name], (k, m, n_mats)); ids = ctx.new_tensor(gg.I32, (n_used, n)); b = ctx.new_tensor(gg.F32, (k, n_used, n))
        got = run(ctx, L.ggml_mul_mat_id(ctx.ctx, as_, b, ids), [(as_, g["w"]), (ids, g["ids"]), (b, g["b"])])
    assert orc.nmse(g["expected"], got[0]) <= 5e-4


def test_attention_matmuls_f16_kv_views():
    """kq = mul_mat(k, q), kqv = mul_mat(v, kq) on F16 cache views with GQA broadcast 32/8
    (src/llama-graph.cpp:1285,1320; src/llama-kv-cache-unified.cpp:1056-1106; tests/test-backend-ops.cpp:5791-5813)."""
    rng = np.random.default_rng(11)
    hd, n_head, n_head_kv, kv_size, n_kv = 128, 32, 8, 256, 96
    for ntok in (1, 3, 17):
        kc = rng.uniform(-1, 1, size=(1, 1, kv_size, hd * n_head_kv)).astype(np.float16)       # cache [n_embd_k_gqa, kv_size]
        vc = rng.uniform(-1, 1, size=(1, 1, hd * n_head_kv, kv_size)).astype(np.float16)       # transposed V cache [kv_size, n_embd_v_gqa]
        q_ = rng.uniform(-1, 1, size=(1, ntok, n_head, hd)).astype(np.float32)                 # q_cur [hd, n_head, n_tok]
        with gg.Context() as ctx:
            k_l = ctx.new_tensor(gg.F16, (hd * n_head_kv, kv_size)); v_l = ctx.new_tensor(gg.F16, (kv_size, hd * n_head_kv))
            q_cur = ctx.new_tensor(gg.F32, (hd, n_head, ntok))
            k = L.ggml_view_3d(ctx.ctx, k_l, hd, n_kv, n_head_kv, hd * n_head_kv * 2, hd * 2, 0)    # get_k
            v = L.ggml_view_3d(ctx.ctx, v_l, n_kv, hd, n_head_kv, kv_size * 2, kv_size * hd * 2, 0)  # get_v (v_trans)
            q = L.ggml_permute(ctx.ctx, q_cur, 0, 2, 1, 3)
            kq = L.ggml_mul_mat(ctx.ctx, k, q)
            L.ggml_mul_mat_set_prec(kq, 10)
            kqv = L.ggml_mul_mat(ctx.ctx, v, kq)
            be = backend(); assert be.supports_op(kq) and be.supports_op(kqv); ctx.alloc(be)
            gg.tensor_set(k_l, kc); gg.tensor_set(v_l, vc); gg.tensor_set(q_cur, q_)
            be.compute(gg.graph_of(ctx, kqv))
            got_kq = gg.tensor_get(kq); got_kqv = gg.tensor_get(kqv)
        K = kc[0, 0, :n_kv].reshape(n_kv, n_head_kv, hd).transpose(1, 0, 2)[None].astype(np.float32)      # [1, hkv, n_kv, hd]
        Q = q_.transpose(0, 2, 1, 3)                                                                       # [1, n_head, ntok, hd]
        exp_kq = ref.mul_mat_dense(K, Q)
        assert orc.nmse(exp_kq, got_kq) <= 5e-4
        V = vc[0, 0].reshape(n_head_kv, hd, kv_size)[:, :, :n_kv][None].astype(np.float32)                # [1, hkv, hd, n_kv]
        exp_kqv = ref.mul_mat_dense(V, got_kq)
        assert orc.nmse(exp_kqv, got_kqv) <= 5e-4


def test_mul_mat_f32_f16_batched_broadcast():
    """contiguous F32 / F16 weights x F32, k = 40, n = 9, broadcast 2 in dim 2: the F32 vector kernel and (n > 8, k % 32 != 0) the F16 pair kernel;
    tests/test_gpu_dense_mul_mat.py holds the layouts, types and kernels this does not reach"""
    rng = np.random.default_rng(12)
    a_ = rng.uniform(-1, 1, size=(2, 3, 16, 40)).astype(np.float32)
    b_ = rng.uniform(-1, 1, size=(2, 6, 9, 40)).astype(np.float32)
    for ta in (gg.F32, gg.F16):
        with gg.Context() as ctx:
            a = ctx.new_tensor(ta, (40, 16, 3, 2)); b = ctx.new_tensor(gg.F32, (40, 9, 6, 2))
            got = run(ctx, L.ggml_mul_mat(ctx.ctx, a, b), [(a, a_ if ta == gg.F32 else a_.astype(np.float16)), (b, b_)])
        aa = a_ if ta == gg.F32 else a_.astype(np.float16).astype(np.float32)
        assert orc.nmse(ref.mul_mat_dense(aa, b_), got) <= 5e-4


@pytest.mark.parametrize("hd,n_head,n_head_kv,n_kv,T,sinks", [(128, 8, 2, 256, 1, False), (128, 8, 2, 512, 3, True), (64, 4, 4, 256, 8, False),
                                                            (128, 8, 2, 256, 33, False), (64, 8, 2, 512, 64, True), (128, 4, 1, 256, 40, False),
                                                            # the prefill kernel's workgroup shapes: 1 / 2 / 8 heads of a kv head per workgroup, a GQA
                                                            # ratio that is no power of two (3), idle waves in the last workgroup, a sliding window
                                                            # (T = 130: cells more than 100 back are masked, so whole blocks at the START are skipped)
                                                            (64, 4, 4, 256, 70, False), (128, 8, 4, 256, 100, True), (128, 16, 2, 512, 130, False),
                                                            (64, 6, 2, 256, 45, True), (128, 32, 8, 1024, 300, False),
                                                            # long contexts, few tokens: the cells are split into ranges over several workgroups and merged
                                                            # (16384 cells of scores do not fit one workgroup's LDS: only the split form can run it)
                                                            (128, 8, 2, 2048, 1, True), (64, 8, 2, 4096, 3, False), (128, 8, 8, 16384, 2, True)])
def test_flash_attn_ext(hd, n_head, n_head_kv, n_kv, T, sinks):
    """FLASH_ATTN_EXT as build_attn_mha emits it with -fa (src/llama-graph.cpp:1245-1265; tests/test-backend-ops.cpp:4559, NMSE 5e-4):
    q F32 permuted view, K and V F16 views of the cache with rows = cells (V NOT transposed), F16 mask padded in the token dimension,
    GQA broadcast, optional attention sinks; result [hd, n_head, T]. T <= 8 runs the decode kernel, more the matrix-core one."""
    rng = np.random.default_rng(100 + T)
    kv_size = n_kv + 64
    kc = rng.uniform(-1, 1, size=(1, 1, kv_size, hd * n_head_kv)).astype(np.float16)
    vc = rng.uniform(-1, 1, size=(1, 1, kv_size, hd * n_head_kv)).astype(np.float16)
    q_ = rng.uniform(-1, 1, size=(1, T, n_head, hd)).astype(np.float32)
    Tp = (T + 63) // 64 * 64
    mask = np.full((1, 1, Tp, n_kv), -np.inf, np.float32)
    for t in range(T):
        mask[0, 0, t, : n_kv - T + t + 1] = 0.0          # causal: the T tokens are the last T cells
        if T == 130:
            mask[0, 0, t, : max(0, n_kv - T + t + 1 - 100)] = -np.inf
    sk = rng.uniform(-1, 1, size=(n_head,)).astype(np.float32)
    scale = 1.0 / np.sqrt(hd)
    with gg.Context() as ctx:
        k_l = ctx.new_tensor(gg.F16, (hd * n_head_kv, kv_size)); v_l = ctx.new_tensor(gg.F16, (hd * n_head_kv, kv_size))
        q_cur = ctx.new_tensor(gg.F32, (hd, n_head, T)); m_ = ctx.new_tensor(gg.F16, (n_kv, Tp)); s_ = ctx.new_tensor(gg.F32, (n_head,))
        k = L.ggml_view_3d(ctx.ctx, k_l, hd, n_head_kv, n_kv, hd * 2, hd * n_head_kv * 2, 0)
        v = L.ggml_view_3d(ctx.ctx, v_l, hd, n_head_kv, n_kv, hd * 2, hd * n_head_kv * 2, 0)
        q = L.ggml_permute(ctx.ctx, q_cur, 0, 2, 1, 3); k = L.ggml_permute(ctx.ctx, k, 0, 2, 1, 3); v = L.ggml_permute(ctx.ctx, v, 0, 2, 1, 3)
        fa = L.ggml_flash_attn_ext(ctx.ctx, q, k, v, m_, float(scale), 0.0, 0.0)
        if sinks:
            L.ggml_flash_attn_ext_add_sinks(fa, s_)
        L.ggml_flash_attn_ext_set_prec(fa, 10)
        be = backend(); assert be.supports_op(fa); ctx.alloc(be)
        gg.tensor_set(k_l, kc); gg.tensor_set(v_l, vc); gg.tensor_set(q_cur, q_); gg.tensor_set(m_, mask.astype(np.float16)); gg.tensor_set(s_, sk.reshape(1, 1, 1, -1))
        be.compute(gg.graph_of(ctx, fa))
        got = gg.tensor_get(fa)                                                     # [1, T, n_head, hd]
    K = kc[0, 0, :n_kv].reshape(n_kv, n_head_kv, hd).astype(np.float64); V = vc[0, 0, :n_kv].reshape(n_kv, n_head_kv, hd).astype(np.float64)
    exp = np.zeros((T, n_head, hd))
    for h in range(n_head):
        hk = h // (n_head // n_head_kv)
        s = q_[0, :, h, :].astype(np.float16).astype(np.float64) @ K[:, hk, :].T * scale + mask[0, 0, :T].astype(np.float64)
        mx = s.max(-1, keepdims=True)
        if sinks:
            mx = np.maximum(mx, sk[h])
        p = np.exp(s - mx); den = p.sum(-1, keepdims=True) + (np.exp(sk[h] - mx) if sinks else 0.0)
        exp[:, h, :] = (p / den) @ V[:, hk, :]
    assert got[0].shape == exp.shape
    assert orc.nmse(exp, got[0]) <= 5e-4, orc.nmse(exp, got[0])


def _bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16))


@pytest.mark.parametrize("hd,n_head,n_head_kv,n_kv,T,tk,tv,max_bias,softcap,sinks", [
    # the reference's grid (tests/test-backend-ops.cpp:6081-6087): type_KV in {F16, BF16, Q8_0, Q4_0} x max_bias {0, 8} x logit_softcap {0, 10}, few and many tokens
    (128, 8, 2, 256, 1, "q8_0", "q8_0", 0.0, 0.0, False), (128, 8, 2, 256, 1, "q4_0", "q4_0", 0.0, 0.0, True), (64, 8, 4, 512, 3, "bf16", "bf16", 0.0, 0.0, False),
    (128, 32, 8, 256, 1, "q8_0", "f16", 0.0, 0.0, False), (128, 8, 2, 512, 2, "q8_0", "q4_0", 8.0, 0.0, False), (64, 4, 4, 256, 1, "q4_0", "q8_0", 0.0, 10.0, False),
    (128, 12, 4, 256, 1, "f16", "f16", 8.0, 0.0, False), (128, 8, 2, 256, 1, "f16", "f16", 0.0, 10.0, True), (64, 6, 2, 2048, 2, "q8_0", "q8_0", 8.0, 10.0, False),
    (128, 8, 8, 16384, 1, "q4_0", "q4_0", 0.0, 0.0, False), (64, 4, 1, 512, 1, "f16", "bf16", 0.0, 0.0, False),
    (128, 8, 2, 512, 35, "q8_0", "q8_0", 0.0, 0.0, False), (64, 4, 4, 256, 70, "q4_0", "q4_0", 8.0, 0.0, True), (128, 16, 2, 512, 130, "bf16", "bf16", 0.0, 10.0, False),
    (128, 8, 4, 1024, 300, "f16", "f16", 8.0, 10.0, False), (64, 6, 2, 256, 45, "q8_0", "q4_0", 0.0, 0.0, True), (128, 32, 8, 512, 512, "q8_0", "q8_0", 0.0, 0.0, False)])
def test_flash_attn_ext_cache_types_alibi_softcap(hd, n_head, n_head_kv, n_kv, T, tk, tv, max_bias, softcap, sinks):
    """FLASH_ATTN_EXT's other parameters (VERDICT r2 missing 2 / 3): the cache as -ctk / -ctv q8_0, q4_0 or bf16 keep it (rows of blocks; V is NOT
    transposed under flash attention), ALiBi (max_bias: head h's mask values times its slope) and the logit soft-cap (scale / c, then c * tanh)
    — ggml_compute_forward_flash_attn_ext_f16, ggml/src/ggml-cpu/ops.cpp. Few tokens: the decode kernel reads the blocks itself (kv_types.h) or, for
    the pairs it is not instantiated for, after kv_to_f16; many tokens: K is converted and V transposed once, then the matrix-core kernel.
    Expected: exact arithmetic on the dequantized cache, NMSE 5e-4 (tests/test-backend-ops.cpp:4559)."""
    rng = np.random.default_rng(1000 + T + n_kv)
    TY = {"f16": gg.F16, "bf16": gg.BF16, "q8_0": gg.Q8_0, "q4_0": gg.Q4_0}
    kv_size = n_kv + 64
    ne = hd * n_head_kv

    def make(t):
        x = rng.uniform(-1, 1, size=(kv_size, ne)).astype(np.float32)
        if t == "f16":
            b = x.astype(np.float16); return b.reshape(1, 1, kv_size, ne), b.astype(np.float64)
        if t == "bf16":
            b = _bf16_round(x); return b.reshape(1, 1, kv_size, ne), (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        b = orc.quantize(x, TY[t]); return b, orc.dequantize(b, TY[t]).astype(np.float64)
    kb, Kf = make(tk); vb, Vf = make(tv)
    q_ = rng.uniform(-1, 1, size=(1, T, n_head, hd)).astype(np.float32)
    Tp = (T + 63) // 64 * 64
    mask = np.full((1, 1, Tp, n_kv), -np.inf, np.float32)
    for t in range(T):
        n_vis = n_kv - T + t + 1
        mask[0, 0, t, :n_vis] = (-np.arange(n_vis)[::-1] / 16.0).astype(np.float16) if max_bias > 0 else 0.0      # ALiBi: minus the distance (here / 16), as f16
    sk = rng.uniform(-1, 1, size=(n_head,)).astype(np.float32)
    scale = 1.0 / np.sqrt(hd)
    with gg.Context() as ctx:
        k_l = ctx.new_tensor(TY[tk], (ne, kv_size)); v_l = ctx.new_tensor(TY[tv], (ne, kv_size))
        q_cur = ctx.new_tensor(gg.F32, (hd, n_head, T)); m_ = ctx.new_tensor(gg.F16, (n_kv, Tp)); s_ = ctx.new_tensor(gg.F32, (n_head,))
        rs_k = orc.row_size(TY[tk], hd); rs_v = orc.row_size(TY[tv], hd)
        k = L.ggml_view_3d(ctx.ctx, k_l, hd, n_head_kv, n_kv, rs_k, rs_k * n_head_kv, 0)
        v = L.ggml_view_3d(ctx.ctx, v_l, hd, n_head_kv, n_kv, rs_v, rs_v * n_head_kv, 0)
        q = L.ggml_permute(ctx.ctx, q_cur, 0, 2, 1, 3); k = L.ggml_permute(ctx.ctx, k, 0, 2, 1, 3); v = L.ggml_permute(ctx.ctx, v, 0, 2, 1, 3)
        fa = L.ggml_flash_attn_ext(ctx.ctx, q, k, v, m_, float(scale), float(max_bias), float(softcap))
        if sinks:
            L.ggml_flash_attn_ext_add_sinks(fa, s_)
        L.ggml_flash_attn_ext_set_prec(fa, 10)
        be = backend(); assert be.supports_op(fa); ctx.alloc(be)
        gg.tensor_set(k_l, kb); gg.tensor_set(v_l, vb); gg.tensor_set(q_cur, q_); gg.tensor_set(m_, mask.astype(np.float16)); gg.tensor_set(s_, sk.reshape(1, 1, 1, -1))
        graph = gg.graph_of(ctx, fa)
        be.compute(graph)
        got = gg.tensor_get(fa).copy()
        be.compute(graph)                                                          # (the conversion buffer and any captured graph are reused)
        assert np.array_equal(got, gg.tensor_get(fa))
    K = Kf[:n_kv].reshape(n_kv, n_head_kv, hd); V = Vf[:n_kv].reshape(n_kv, n_head_kv, hd)
    exp = ref.flash_attn_ext(q_[0], K, V, mask[0, 0], scale, max_bias, softcap, sk if sinks else None)
    assert got[0].shape == exp.shape
    assert orc.nmse(exp, got[0]) <= 5e-4, orc.nmse(exp, got[0])


@pytest.mark.parametrize("types", [("q4_K", "q4_K", "q6_K"), ("q4_K", "q4_K", "q4_K"), ("q8_0", "q8_0", "q8_0")])
def test_norm_qkv_group_at_model_size(types):
    """RMS_NORM -> MUL(w) -> three mat-vecs that all read the product, at Llama-3-8B's sizes (4096 -> 4096 / 1024 / 1024): with fusion on
    this is ONE grouped launch with the norm in its prologue and — 3072 row pairs on 256 CUs — the 16-wave workgroup variant;
    against the oracle evaluation of the separate ops, and bit-for-bit against the node-by-node path's quantized arithmetic."""
    rng = np.random.default_rng(21)
    k = 4096
    ms = (4096, 1024, 1024)
    x = rng.standard_normal((1, 1, 1, k)).astype(np.float32)
    wn = rng.uniform(0.5, 1.5, size=(1, 1, 1, k)).astype(np.float32)
    ws = [orc.random_blocks(rng, QTYPES[t], (m,), k, scale=1.0 / np.sqrt(k)) for t, m in zip(types, ms)]
    res = {}
    for fusion in (1, 0):
        be = backend(); be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            xt = ctx.new_tensor(gg.F32, (k, 1)); wt = ctx.new_tensor(gg.F32, (k,))
            mats = [ctx.new_tensor(QTYPES[t], (k, m)) for t, m in zip(types, ms)]
            nm = L.ggml_mul(ctx.ctx, L.ggml_rms_norm(ctx.ctx, xt, 1e-5), wt)
            outs = [L.ggml_mul_mat(ctx.ctx, a, nm) for a in mats]
            assert ctx.alloc(be)
            gg.tensor_set(xt, x); gg.tensor_set(wt, wn)
            for a, w in zip(mats, ws):
                gg.tensor_set(a, w)
            be.compute(gg.graph_of(ctx, *outs))
            res[fusion] = [gg.tensor_get(o)[0, 0, 0].copy() for o in outs]
        be.set_option("fusion", 1)
    h = (ref.rms_norm(x[0, 0], 1e-5) * wn[0, 0, 0]).astype(np.float32)
    for i, (t, m) in enumerate(zip(types, ms)):
        cpu = orc.mul_mat_2d(ws[i], QTYPES[t], h, "cpu")[0]; exact = orc.mul_mat_2d(ws[i], QTYPES[t], h, "exact")[0]
        assert orc.nmse(exact, res[1][i]) <= 5e-4 and orc.nmse(cpu, res[1][i]) <= 5e-4
        assert np.abs(res[1][i] - cpu).max() <= 2e-5 * (np.abs(cpu).max() + 1e-30)
        assert np.abs(res[1][i] - res[0][i]).max() <= 2e-5 * (np.abs(cpu).max() + 1e-30)


@pytest.mark.parametrize("t_ff,t_down", [("q4_K", "q6_K"), ("q4_K", "q4_K"), ("q8_0", "q8_0")])
def test_ffn_at_model_size(t_ff, t_down):
    """build_ffn at Llama-3-8B's sizes (src/llama-graph.cpp:632-774): norm -> gate / up (4096 -> 14336) -> swiglu -> down (14336 -> 4096)
    -> + residual. With fusion on: the dual-stream GLU launch (one-row units, 7 rows per wave) and the down launch with the f32 -> int8
    quantization of 14336 activations in its prologue and the residual in its epilogue."""
    rng = np.random.default_rng(22)
    k, ff = 4096, 14336
    x = rng.standard_normal((1, 1, 1, k)).astype(np.float32)
    wn = rng.uniform(0.5, 1.5, size=(1, 1, 1, k)).astype(np.float32)
    wg = orc.random_blocks(rng, QTYPES[t_ff], (ff,), k, scale=1.0 / np.sqrt(k)); wu = orc.random_blocks(rng, QTYPES[t_ff], (ff,), k, scale=1.0 / np.sqrt(k))
    wd = orc.random_blocks(rng, QTYPES[t_down], (k,), ff, scale=1.0 / np.sqrt(ff))
    res = {}
    for fusion in (1, 0):
        be = backend(); be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            xt = ctx.new_tensor(gg.F32, (k, 1)); wt = ctx.new_tensor(gg.F32, (k,))
            g_ = ctx.new_tensor(QTYPES[t_ff], (k, ff)); u_ = ctx.new_tensor(QTYPES[t_ff], (k, ff)); d_ = ctx.new_tensor(QTYPES[t_down], (ff, k))
            nm = L.ggml_mul(ctx.ctx, L.ggml_rms_norm(ctx.ctx, xt, 1e-5), wt)
            up = L.ggml_mul_mat(ctx.ctx, u_, nm); gate = L.ggml_mul_mat(ctx.ctx, g_, nm)
            act = L.ggml_swiglu_split(ctx.ctx, gate, up)
            out = L.ggml_add(ctx.ctx, L.ggml_mul_mat(ctx.ctx, d_, act), xt)
            assert ctx.alloc(be)
            gg.tensor_set(xt, x); gg.tensor_set(wt, wn); gg.tensor_set(g_, wg); gg.tensor_set(u_, wu); gg.tensor_set(d_, wd)
            be.compute(gg.graph_of(ctx, out))
            res[fusion] = gg.tensor_get(out)[0, 0, 0].copy()
        be.set_option("fusion", 1)
    h = (ref.rms_norm(x[0, 0], 1e-5) * wn[0, 0, 0]).astype(np.float32)
    outs = {}
    for mode in ("cpu", "exact"):
        a = ref.swiglu(orc.mul_mat_2d(wg, QTYPES[t_ff], h, mode), orc.mul_mat_2d(wu, QTYPES[t_ff], h, mode)).astype(np.float32)
        outs[mode] = orc.mul_mat_2d(wd, QTYPES[t_down], a, mode)[0] + x[0, 0, 0]
    assert orc.nmse(outs["exact"], res[1]) <= 5e-4 and orc.nmse(outs["cpu"], res[1]) <= 5e-4
    assert orc.nmse(res[0], res[1]) <= 1e-6


@pytest.mark.parametrize("name,ff,k,n,gate_first", [("q4_K", 10240, 512, 512, True), ("q6_K", 10300, 256, 300, False), ("q8_0", 20500, 288, 257, True),
                                                  ("mxfp4", 10240, 96, 300, True), ("q5_K", 5200, 512, 1000, False), ("q4_0", 10250, 64, 512, True)])
def test_prefill_gate_up_glu_fused(name, ff, k, n, gate_first):
    """build_ffn's gate / up / swiglu for many tokens (src/llama-graph.cpp:646-691): with fusion on, one matrix-core kernel computes both
    products and the SwiGLU (mmq.hip DUAL) — checked against node-by-node execution (same bf16 operands: only expf's argument rounding
    can differ) and against the oracle's exact product."""
    rng = np.random.default_rng(ff + k + n)
    x = rng.uniform(-1, 1, size=(1, 1, n, k)).astype(np.float32)
    wg = orc.random_blocks(rng, QTYPES[name], (ff,), k, scale=2.0 / np.sqrt(k)); wu = orc.random_blocks(rng, QTYPES[name], (ff,), k, scale=2.0 / np.sqrt(k))
    res = {}
    for fusion in (1, 0):
        be = backend(); be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            xt = ctx.new_tensor(gg.F32, (k, n)); g_ = ctx.new_tensor(QTYPES[name], (k, ff)); u_ = ctx.new_tensor(QTYPES[name], (k, ff))
            if gate_first:
                gate = L.ggml_mul_mat(ctx.ctx, g_, xt); up = L.ggml_mul_mat(ctx.ctx, u_, xt)
            else:
                up = L.ggml_mul_mat(ctx.ctx, u_, xt); gate = L.ggml_mul_mat(ctx.ctx, g_, xt)
            act = L.ggml_swiglu_split(ctx.ctx, gate, up)
            assert ctx.alloc(be)
            gg.tensor_set(xt, x); gg.tensor_set(g_, wg); gg.tensor_set(u_, wu)
            c0 = be.counters()
            be.compute(gg.graph_of(ctx, act))
            c1 = be.counters()
            res[fusion] = gg.tensor_get(act)[0, 0].copy()
        be.set_option("fusion", 1)
        if fusion:
            assert c1["mmq_launches"] - c0["mmq_launches"] == 1, "the gate / up / swiglu chain did not run as one kernel"
    exact = ref.swiglu(orc.mul_mat_2d(wg, QTYPES[name], x[0, 0], "exact"), orc.mul_mat_2d(wu, QTYPES[name], x[0, 0], "exact")).astype(np.float32)
    assert np.isfinite(res[1]).all()
    assert orc.nmse(exact, res[1]) <= 5e-4
    assert orc.nmse(exact, res[1]) <= 5e-5, orc.nmse(exact, res[1])
    assert orc.nmse(res[0], res[1]) <= 1e-9, orc.nmse(res[0], res[1])


@pytest.mark.parametrize("name,m,k,n", [("q4_K", 1024, 2048, 512), ("q4_K", 4096, 4096, 512), ("q6_K", 512, 8192, 300), ("q8_0", 1024, 288, 64)])
def test_prefill_residual_norm_chain(name, m, k, n):
    """wo (or ffn_down) -> + residual -> RMS_NORM * w -> the next mat-mul, many tokens (src/llama-model.cpp:6057-6070): when the first mat-mul
    splits k, ONE pass adds its planes and the residual, writes the sum (the residual stream, read again later) and the normalised rows plus
    their bf16 copy for the next mat-mul. Shapes: k split in 2 (128-token tiles), in 4 (256-token tiles), ragged n, and no split at all."""
    rng = np.random.default_rng(m + k + n)
    x = rng.uniform(-1, 1, size=(1, 1, n, k)).astype(np.float32)
    r = rng.uniform(-1, 1, size=(1, 1, n, m)).astype(np.float32)
    wn = rng.uniform(0.5, 1.5, size=(1, 1, 1, m)).astype(np.float32)
    w1 = orc.random_blocks(rng, QTYPES[name], (m,), k, scale=1.0 / np.sqrt(k))
    w2 = orc.random_blocks(rng, QTYPES["q8_0"], (256,), m, scale=1.0 / np.sqrt(m))
    res = {}
    for fusion in (1, 0):
        be = backend(); be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            xt = ctx.new_tensor(gg.F32, (k, n)); rt = ctx.new_tensor(gg.F32, (m, n)); wt = ctx.new_tensor(gg.F32, (m,))
            a1 = ctx.new_tensor(QTYPES[name], (k, m)); a2 = ctx.new_tensor(QTYPES["q8_0"], (m, 256))
            s_ = L.ggml_add(ctx.ctx, L.ggml_mul_mat(ctx.ctx, a1, xt), rt)
            y = L.ggml_mul(ctx.ctx, L.ggml_rms_norm(ctx.ctx, s_, 1e-5), wt)
            o2 = L.ggml_mul_mat(ctx.ctx, a2, y)
            o3 = L.ggml_scale(ctx.ctx, s_, 2.0)                         # a second reader of the residual stream
            assert ctx.alloc(be)
            gg.tensor_set(xt, x); gg.tensor_set(rt, r); gg.tensor_set(wt, wn); gg.tensor_set(a1, w1); gg.tensor_set(a2, w2)
            be.compute(gg.graph_of(ctx, o2, o3))
            res[fusion] = (gg.tensor_get(o2)[0, 0].copy(), gg.tensor_get(o3)[0, 0].copy())
        be.set_option("fusion", 1)
    s_ref = orc.mul_mat_2d(w1, QTYPES[name], x[0, 0], "exact") + r[0, 0]
    y_ref = (ref.rms_norm(s_ref.astype(np.float32), 1e-5) * wn[0, 0, 0]).astype(np.float32)
    o_ref = orc.mul_mat_2d(w2, QTYPES["q8_0"], y_ref, "exact")
    assert orc.nmse(2.0 * s_ref, res[1][1]) <= 2e-5 and orc.nmse(o_ref, res[1][0]) <= 1e-4, (orc.nmse(2.0 * s_ref, res[1][1]), orc.nmse(o_ref, res[1][0]))
    assert np.array_equal(res[0][1], res[1][1]), "the residual stream: same kernels, same summation order"
    assert orc.nmse(res[0][0], res[1][0]) <= 1e-9


@pytest.mark.parametrize("t_ff,t_down,k,ff,n", [("q4_K", "q6_K", 512, 10240, 512), ("q8_0", "q4_K", 256, 10496, 300), ("q4_0", "q4_0", 1024, 20480, 256)])
def test_prefill_ffn_chain(t_ff, t_down, k, ff, n):
    """build_ffn for many tokens (src/llama-graph.cpp:632-774): norm -> gate / up -> swiglu -> down -> + residual. With fusion on: the norm
    writes the bf16 copy gate / up read, ONE kernel does gate, up and SwiGLU and writes — instead of the f32 tensor — the bf16 copy that
    ffn_down reads, and down adds the residual in its epilogue / combine pass: 3 kernels for 7 nodes."""
    rng = np.random.default_rng(ff + n)
    x = rng.standard_normal((1, 1, n, k)).astype(np.float32)
    wn = rng.uniform(0.5, 1.5, size=(1, 1, 1, k)).astype(np.float32)
    wg = orc.random_blocks(rng, QTYPES[t_ff], (ff,), k, scale=1.0 / np.sqrt(k)); wu = orc.random_blocks(rng, QTYPES[t_ff], (ff,), k, scale=1.0 / np.sqrt(k))
    wd = orc.random_blocks(rng, QTYPES[t_down], (k,), ff, scale=1.0 / np.sqrt(ff))
    res = {}
    for fusion in (1, 0):
        be = backend(); be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            xt = ctx.new_tensor(gg.F32, (k, n)); wt = ctx.new_tensor(gg.F32, (k,))
            g_ = ctx.new_tensor(QTYPES[t_ff], (k, ff)); u_ = ctx.new_tensor(QTYPES[t_ff], (k, ff)); d_ = ctx.new_tensor(QTYPES[t_down], (ff, k))
            nm = L.ggml_mul(ctx.ctx, L.ggml_rms_norm(ctx.ctx, xt, 1e-5), wt)
            gate = L.ggml_mul_mat(ctx.ctx, g_, nm); up = L.ggml_mul_mat(ctx.ctx, u_, nm)
            act = L.ggml_swiglu_split(ctx.ctx, gate, up)
            out = L.ggml_add(ctx.ctx, L.ggml_mul_mat(ctx.ctx, d_, act), xt)
            assert ctx.alloc(be)
            gg.tensor_set(xt, x); gg.tensor_set(wt, wn); gg.tensor_set(g_, wg); gg.tensor_set(u_, wu); gg.tensor_set(d_, wd)
            c0 = be.counters(); be.compute(gg.graph_of(ctx, out)); c1 = be.counters()
            res[fusion] = gg.tensor_get(out)[0, 0].copy()
        be.set_option("fusion", 1)
        if fusion:
            assert c1["mmq_launches"] - c0["mmq_launches"] == 2, "norm | gate+up+swiglu | down+residual"
    h = (ref.rms_norm(x[0, 0], 1e-5) * wn[0, 0, 0]).astype(np.float32)
    a = ref.swiglu(orc.mul_mat_2d(wg, QTYPES[t_ff], h, "exact"), orc.mul_mat_2d(wu, QTYPES[t_ff], h, "exact")).astype(np.float32)
    exact = orc.mul_mat_2d(wd, QTYPES[t_down], a, "exact") + x[0, 0]
    assert np.isfinite(res[1]).all()
    assert orc.nmse(exact, res[1]) <= 5e-5, orc.nmse(exact, res[1])
    assert orc.nmse(res[0], res[1]) <= 1e-8, orc.nmse(res[0], res[1])


@pytest.mark.parametrize("types,ms,k,n,hd", [(("q4_K", "q4_K", "q6_K"), (4096, 1024, 1024), 4096, 512, 128), (("q4_K", "q4_K", "q4_K"), (2048, 512, 512), 4096, 300, 64),
                                            (("q6_K", "q5_K", "q5_K"), (7000, 7000, 7200), 256, 257, 8), (("q8_0", "q8_0"), (2048, 2048), 2048, 1000, 64),
                                            (("mxfp4", "mxfp4", "mxfp4"), (14336, 4096, 4096), 2880, 256, 64), (("q4_0", "q4_K", "q4_0"), (4096, 1024, 1024), 1024, 512, 64)])
def test_prefill_qkv_group(types, ms, k, n, hd):
    """wq / wk / wv of build_attn on many tokens (src/llama-model.cpp:6017-6040): mat-muls on the same activations, the first two followed by
    RESHAPE -> ROPE. With fusion on they run as one launch of 256-token tiles (two block formats at most), the ROPEs after it. Shapes:
    k split in two / in four / not at all, ragged tiles, a type mix without a kernel (falls back to one launch per mat-mul)."""
    rng = np.random.default_rng(sum(ms) + k + n)
    x = rng.uniform(-1, 1, size=(1, 1, n, k)).astype(np.float32)
    ws = [orc.random_blocks(rng, QTYPES[t], (m,), k) for t, m in zip(types, ms)]
    pos = np.arange(n, dtype=np.int32)
    res = {}
    for fusion in (1, 0):
        be = backend(); be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            xt = ctx.new_tensor(gg.F32, (k, n)); pt = ctx.new_tensor(gg.I32, (n,))
            wt = [ctx.new_tensor(QTYPES[t], (k, m)) for t, m in zip(types, ms)]
            outs = []
            for q, w_ in enumerate(wt):
                o = L.ggml_mul_mat(ctx.ctx, w_, xt)
                if q < 2 and ms[q] % hd == 0:
                    o = L.ggml_rope_ext(ctx.ctx, L.ggml_reshape_3d(ctx.ctx, o, hd, ms[q] // hd, n), pt, None, hd, 0, 8192, 10000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
                outs.append(o)
            assert ctx.alloc(be)
            g_ = gg.graph_of(ctx, *outs)
            gg.tensor_set(xt, x); gg.tensor_set(pt, pos)
            for t_, w_ in zip(wt, ws):
                gg.tensor_set(t_, w_)
            c0 = be.counters(); be.compute(g_); c1 = be.counters()
            res[fusion] = [gg.tensor_get(o).reshape(n, -1).copy() for o in outs]
        be.set_option("fusion", 1)
        tiles = sum((m + 127) // 128 for m in ms) * ((n + 255) // 256)       # the launcher's rule (mmq.hip mul_mat_q_multi)
        fills = tiles >= 160 or (tiles * 2 >= 160 and k % 512 == 0 and k >= 2048) or (tiles * 4 >= 160 and k % 1024 == 0 and k >= 4096)
        if fusion and fills and n >= 256 and len(set(types)) <= 2 and not ("q4_0" in types and "q4_K" in types):
            assert c1["mmq_launches"] - c0["mmq_launches"] == 1, "the mat-muls did not run as one launch"
    for q in range(len(types)):
        exact = orc.mul_mat_2d(ws[q], QTYPES[types[q]], x[0, 0], "exact")
        if q < 2 and ms[q] % hd == 0:
            exact = ref.rope(exact.reshape(1, n, ms[q] // hd, hd).astype(np.float32), pos, hd, 0, 8192, 10000.0, 1.0, 0.0, 1.0, 32.0, 1.0, None).reshape(n, -1)
        assert np.isfinite(res[1][q]).all()
        assert orc.nmse(exact, res[1][q]) <= 2e-5, (q, orc.nmse(exact, res[1][q]))
        assert orc.nmse(res[0][q], res[1][q]) <= 1e-10, (q, orc.nmse(res[0][q], res[1][q]))


@pytest.mark.parametrize("name,m,k,n", [("q4_K", 1024, 2048, 512), ("q6_K", 300, 512, 100), ("q8_0", 10240, 288, 512), ("q4_K", 5120, 8192, 300),
                                        ("mxfp4", 1026, 2880, 64), ("q5_K", 1028, 2048, 257)])
def test_prefill_mul_mat_residual_fused(name, m, k, n):
    """build_attn's wo / build_ffn's down followed by the residual ADD, many tokens (src/llama-model.cpp:6057,6096): with fusion on the
    residual is added in the mat-mul's epilogue (or by the pass that combines the split-k planes). The shapes walk through the launch
    variants: k split in two, no split with ragged tiles, 256-token tiles, k split in four; m not a multiple of 4 (no split)."""
    rng = np.random.default_rng(m + k + n)
    x = rng.uniform(-1, 1, size=(1, 1, n, k)).astype(np.float32)
    r = rng.uniform(-3, 3, size=(1, 1, n, m)).astype(np.float32)
    w = orc.random_blocks(rng, QTYPES[name], (m,), k)
    res = {}
    for fusion in (1, 0):
        be = backend(); be.set_option("fusion", fusion)
        with gg.Context() as ctx:
            xt = ctx.new_tensor(gg.F32, (k, n)); rt = ctx.new_tensor(gg.F32, (m, n)); wt = ctx.new_tensor(QTYPES[name], (k, m))
            out = L.ggml_add(ctx.ctx, L.ggml_mul_mat(ctx.ctx, wt, xt), rt) if m % 2 == 0 else L.ggml_add(ctx.ctx, rt, L.ggml_mul_mat(ctx.ctx, wt, xt))
            assert ctx.alloc(be)
            gg.tensor_set(xt, x); gg.tensor_set(rt, r); gg.tensor_set(wt, w)
            c0 = be.counters(); be.compute(gg.graph_of(ctx, out)); c1 = be.counters()
            res[fusion] = gg.tensor_get(out)[0, 0].copy()
        be.set_option("fusion", 1)
        if fusion:
            assert c1["nodes_computed"] - c0["nodes_computed"] == 2
    exact = orc.mul_mat_2d(w, QTYPES[name], x[0, 0], "exact") + r[0, 0]
    assert np.isfinite(res[1]).all()
    assert orc.nmse(exact, res[1]) <= 2e-5, orc.nmse(exact, res[1])
    assert np.array_equal(res[0], res[1]), "same kernels, same summation order: the fused result must be bit-identical"


@pytest.mark.parametrize("name", ["q8_0", "q4_0"])
@pytest.mark.parametrize("ne0,rows,r,b", [(256, 5, 1, 1), (256, 11, 7, 3), (96, 3, 2, 7), (1024, 64, 5, 1)])
def test_set_rows_quantized_dst(name, ne0, rows, r, b):
    """SET_ROWS into a quantized destination (a q8_0 / q4_0 KV cache; tests/test-backend-ops.cpp:5333-5343): the written rows must be
    byte-identical to the reference row quantizer's output (oracle quantize_row_*_ref, pinned by the golden vectors); rows that are
    not addressed keep their bytes."""
    rng = np.random.default_rng(ne0 + rows + r)
    qt = QTYPES[name]
    rb = orc.row_size(qt, ne0)
    dst0 = orc.random_blocks(rng, qt, (1, b, rows), ne0)                      # [1, b, rows, row_bytes]
    src = rng.uniform(-1, 1, size=(1, b, r, ne0)).astype(np.float32)
    src[0, 0, 0, :32] = 0.0                                                  # a zero block
    idx = np.stack([rng.permutation(rows)[:r] for _ in range(b)]).astype(np.int64).reshape(1, 1, b, r)
    with gg.Context() as ctx:
        d = ctx.new_tensor(qt, (ne0, rows, b)); s_ = ctx.new_tensor(gg.F32, (ne0, r, b)); i_ = ctx.new_tensor(gg.I64, (r, b))
        o = L.ggml_set_rows(ctx.ctx, d, s_, i_)
        be = backend(); assert be.supports_op(o); ctx.alloc(be)
        gg.tensor_set(d, dst0); gg.tensor_set(s_, src); gg.tensor_set(i_, idx)
        be.compute(gg.graph_of(ctx, o))
        got = gg.tensor_get(d)
    exp = dst0.copy().reshape(1, b, rows, rb)
    q = orc.quantize(src.reshape(-1, ne0), qt).reshape(b, r, rb)
    for ib in range(b):
        for ir in range(r):
            exp[0, ib, idx[0, 0, ib, ir]] = q[ib, ir]
    g2 = got.reshape(exp.shape)
    bad = np.argwhere(g2 != exp)
    assert bad.size == 0, (len(bad), bad[:6].tolist(), [int(g2[tuple(b)]) for b in bad[:6]], [int(exp[tuple(b)]) for b in bad[:6]], idx.tolist())
