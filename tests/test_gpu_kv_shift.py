"""The K-shift of a quantized KV cache (-ctk q8_0 / q4_0), built as llama_kv_cache_unified::build_graph_shift / build_rope_shift build it
(src/llama-kv-cache-unified.cpp:1416-1526): one I32 k_shift tensor of kv_size entries; per layer a cache tensor [n_embd_k_gqa, kv_size], its view
[hd, n_head_kv, kv_size] with nb1 = row_size(hd), nb2 = row_size(n_embd_k_gqa), then ggml_cast(F32) -> ggml_rope_ext -> ggml_cpy back into the view.
With fusion on the three nodes run as ONE in-place launch (elem.hip k_kv_shift); the gate is that it leaves the same BYTES as the three launches.

Per case: (1) fusion 1 and fusion 0 leave identical cache bytes; (2) kernels_launched = layers, and 3 x layers node by node; (3) against the oracle:
x = ops_ref.rope in float64 on the dequantized cache, e_ref = NMSE(dequant(quantize(f32(x))), x) is the reference's own requantization loss on these
rows and e_got the same for the bytes the GPU left: e_got <= 1.25 x e_ref. The only extra error is the f32 angle (|shift| <= 512: ~1e-4 rad, ~1e-8 in
NMSE, three orders below Q8_0's step loss of ~1.5e-5 on these inputs): the 1.25 is room for rounding flips at quantizer boundaries, not for precision;
(4) 8 cache cells behind the view keep their bytes; (5) the same graph computed three times with graphs on (eager, capture, replay) equals three
node-by-node applications. The chain is declined, and still right in three launches, when the final CPY targets another cache or the ROPE result is also a
graph output. The F16-cache form (ROPE written into its own source view) is the control: it passes before this feature as well.

Largest e_got / e_ref measured over the grid: 1.0003 (DESIGN.md §4 "K-shift and defrag of a quantized cache")."""
import itertools

import numpy as np
import pytest

import elem_cases as ec
import oracle as orc
import ops_ref as ref
from gpu_util import backend, gg

pytestmark = pytest.mark.gpu
L = gg.base()
F32, F16, I32 = gg.F32, gg.F16, gg.I32
QT = {"q8_0": gg.Q8_0, "q4_0": gg.Q4_0}
EXTRA_CELLS = 8
FREQ_BASE, BETA_FAST, BETA_SLOW = 10000.0, 32.0, 1.0


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
# case = (type, mode, (hd, n_rot), n_head_kv, kv_size, extra) with extra in "", "ff", "yarn", "layers3"
def _grid():
    cases = []
    prod = list(itertools.product((0, 2), ((64, 64), (128, 128), (128, 64)), (1, 3), (1, 33, 300)))
    for i, (mode, dims, nh, kv) in enumerate(prod):      # every combination with one type, every third with the other one as well: 48 of the 72
        names = ("q8_0", "q4_0") if i % 2 == 0 else ("q4_0", "q8_0")
        cases.append((names[0], mode, dims, nh, kv, ""))
        if i % 3 == 0:
            cases.append((names[1], mode, dims, nh, kv, ""))
    for name in QT:
        cases.append((name, 0, (128, 128), 3, 33, "ff"))
        cases.append((name, 2, (128, 64), 3, 33, "yarn"))
        cases.append((name, 2, (128, 128), 3, 33, "layers3"))
    return cases


CASES = _grid()
for _name in QT:      # every value of the grid occurs with both types
    _mine = [c for c in CASES if c[0] == _name]
    assert {c[1] for c in _mine} == {0, 2} and {c[2] for c in _mine} == {(64, 64), (128, 128), (128, 64)}
    assert {c[3] for c in _mine} == {1, 3} and {c[4] for c in _mine} == {1, 33, 300} and {c[5] for c in _mine} == {"", "ff", "yarn", "layers3"}


def case_id(c):
    name, mode, (hd, nr), nh, kv, extra = c
    return f"{name}-{'neox' if mode else 'norm'}-hd{hd}-rot{nr}-h{nh}-kv{kv}" + ("-" + extra if extra else "")


def shifts_of(kv, rng):
    """[-512, 512], with zeros (cells that stay) and a run of equal negative values (the cells behind a discarded range all move by its length)"""
    s = rng.integers(-512, 513, size=kv).astype(np.int32)
    if kv == 1:
        s[0] = -37
    else:
        s[0:3] = 0
        s[kv // 3:kv // 3 + max(2, kv // 4)] = -64
        s[-1] = 512; s[-2] = -512
    return s


def rope_args(extra):
    """(n_ctx_orig, freq_scale, ext_factor, attn_factor)"""
    return (256, 0.25, 1.0, 1.0) if extra == "yarn" else (8192, 1.0, 0.0, 1.0)


class ShiftGraph:
    """the graph of build_graph_shift over `layers` caches of type `t` (a block type, or F16 for the control), in a context of its own"""

    def __init__(self, t, mode, dims, nh, kv, extra, seed, target="same", rope_is_output=False, shifts=None, data=None, freq_base=FREQ_BASE):
        self.t, self.mode, (self.hd, self.n_rot), self.nh, self.kv, self.extra = t, mode, dims, nh, kv, extra
        self.layers = 3 if extra == "layers3" else 1
        self.n_embd = self.hd * nh
        self.cells = kv + EXTRA_CELLS
        rng = np.random.default_rng(seed)
        self.shifts = shifts_of(kv, rng) if shifts is None else shifts
        self.freq_base = freq_base
        self.ff = rng.uniform(1.0, 4.0, size=self.n_rot // 2).astype(np.float32) if extra == "ff" else None
        if data is not None:
            self.data = data
        else:
            self.data = [orc.random_blocks(rng, t, (1, 1, self.cells), self.n_embd) for _ in range(self.layers)]      # orc.quantize(U(-1, 1))
        self.ctx = gg.Context()
        c = self.ctx.ctx
        n_ctx_orig, fs, ext, af = rope_args(extra)
        rs = (lambda n: n * 2) if t == F16 else (lambda n: orc.row_size(t, n))
        self.k_shift = self.ctx.new_tensor(I32, (kv,))
        self.ff_t = self.ctx.new_tensor(F32, (self.n_rot // 2,)) if self.ff is not None else None
        self.caches, self.others, self.nodes, self.ropes, outs = [], [], [], [], []
        for _ in range(self.layers):
            cache = self.ctx.new_tensor(t, (self.n_embd, self.cells))
            view = L.ggml_view_3d(c, cache, self.hd, nh, kv, rs(self.hd), rs(self.n_embd), 0)
            rope = lambda a: L.ggml_rope_ext(c, a, self.k_shift, self.ff_t, self.n_rot, mode, n_ctx_orig, freq_base, fs, ext, af, BETA_FAST, BETA_SLOW)
            if t == F16:
                # ggml_rope_ext_inplace: the result is a view of its source (described by hand: the binding has no in-place constructor)
                r = rope(view)
                r.contents.view_src = cache; r.contents.view_offs = 0
                for d in range(4):
                    r.contents.nb[d] = view.contents.nb[d]
                self.nodes.append([r]); outs.append(r)
            else:
                tmp = L.ggml_cast(c, view, F32)
                r = rope(tmp)
                to = view
                if target == "other":
                    other = self.ctx.new_tensor(t, (self.n_embd, self.cells)); self.others.append(other)
                    to = L.ggml_view_3d(c, other, self.hd, nh, kv, rs(self.hd), rs(self.n_embd), 0)
                back = L.ggml_cpy(c, r, to)
                if rope_is_output:
                    r.contents.flags |= 2      # GGML_TENSOR_FLAG_OUTPUT
                self.nodes.append([tmp, r, back]); self.ropes.append(r); outs.append(back)
            self.caches.append(cache)
        self.graph = self.ctx.new_graph()
        for o in outs:      # build_forward_expand once per layer
            L.ggml_build_forward_expand(self.graph, o)

    def supported(self, be):
        return all(be.supports_op(n) for ns in self.nodes for n in ns)

    def upload(self, be):
        assert self.ctx.alloc(be)
        gg.tensor_set(self.k_shift, self.shifts.reshape(1, 1, 1, -1))
        if self.ff_t:
            gg.tensor_set(self.ff_t, self.ff.reshape(1, 1, 1, -1))
        for cache, d in zip(self.caches, self.data):
            gg.tensor_set(cache, d)
        for o in self.others:
            gg.tensor_set(o, np.full_like(self.data[0], 0x5A))

    def rows(self, cache_bytes):
        """the view's rows of one cache array -> [1, kv, nh, row bytes or hd]"""
        return cache_bytes.reshape(self.cells, self.nh, -1)[:self.kv][None]

    def rotated64(self, layer=0, times=1, data=None):
        """ops_ref.rope in float64 on the dequantized cache rows"""
        d = self.data[layer] if data is None else data
        x = self.rows(d).astype(np.float64) if self.t == F16 else orc.dequantize(self.rows(d), self.t).astype(np.float64)
        n_ctx_orig, fs, ext, af = rope_args(self.extra)
        for _ in range(times):
            x = ref.rope(x, self.shifts, self.n_rot, self.mode, n_ctx_orig, self.freq_base, fs, ext, af, BETA_FAST, BETA_SLOW, self.ff)
        return x

    def free(self):
        self.ctx.free()


def run(c, fusion, graphs, times=1, **kw):
    """-> (the caches' bytes after `times` computes of one graph, kernels_launched, counters, the graph object's extras)"""
    name, mode, dims, nh, kv, extra = c
    be = backend()
    be.set_option("graphs", graphs); be.set_option("fusion", fusion)      # (setting fusion drops every captured graph)
    sg = ShiftGraph(QT.get(name, F16), mode, dims, nh, kv, extra, seed=1000 + CASES.index(c) if c in CASES else 999, **kw)
    try:
        assert sg.supported(be), "supports_op refused a node of the K-shift graph"
        sg.upload(be)
        be.reset_counters()
        for _ in range(times):
            be.compute(sg.graph)
        cnt = be.counters()
        got = [gg.tensor_get(t).copy() for t in sg.caches]
        others = [gg.tensor_get(t).copy() for t in sg.others]
        ropes = [gg.tensor_get(r).copy() for r in sg.ropes] if kw.get("rope_is_output") else []
        return sg, got, cnt, others, ropes
    finally:
        sg.free()
        be.set_option("graphs", 1); be.set_option("fusion", 1)


def requant_errors(sg, x64, got_rows_bytes):
    qt = sg.t
    e_ref = orc.nmse(x64, orc.dequantize(orc.quantize(x64.astype(np.float32), qt), qt))
    e_got = orc.nmse(x64, orc.dequantize(got_rows_bytes, qt))
    return e_got, e_ref


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_kv_shift(c):
    sg, fused, cnt1, _, _ = run(c, fusion=1, graphs=0)
    _, plain, cnt0, _, _ = run(c, fusion=0, graphs=0)
    # 1. fused equals node by node, byte for byte
    for l in range(sg.layers):
        bad = np.argwhere(fused[l] != plain[l])
        assert bad.size == 0, ("fused != node by node", l, len(bad), bad[:6].tolist())
    # 2. launches
    assert cnt1["kernels_launched"] == sg.layers and cnt0["kernels_launched"] == 3 * sg.layers, (cnt1["kernels_launched"], cnt0["kernels_launched"])
    for l in range(sg.layers):
        # 3. against the reference's own requantization loss
        e_got, e_ref = requant_errors(sg, sg.rotated64(l), sg.rows(fused[l]))
        print(f"{case_id(c)} layer {l}: e_got {e_got:.4e} e_ref {e_ref:.4e} ratio {e_got / e_ref:.4f}")
        assert e_got <= 1.25 * e_ref, (e_got, e_ref)
        # 4. the cells behind the view
        assert np.array_equal(fused[l].reshape(sg.cells, -1)[sg.kv:], sg.data[l].reshape(sg.cells, -1)[sg.kv:]), "cells outside the view changed"
    # 5. eager, capture, replay: three applications
    _, thrice_g, cntg, _, _ = run(c, fusion=1, graphs=1, times=3)
    _, thrice_p, _, _, _ = run(c, fusion=0, graphs=0, times=3)
    if 4 * sg.layers >= 8:      # (graphs of fewer than 8 nodes are not captured)
        assert cntg["graph_captures"] == 1 and cntg["graph_replays"] >= 1, cntg
    for l in range(sg.layers):
        assert np.array_equal(thrice_g[l], thrice_p[l]), ("three computes with graphs on != three node-by-node applications", l)


@pytest.mark.parametrize("name", list(QT))
@pytest.mark.parametrize("mode", [0, 2], ids=["norm", "neox"])
def test_kv_shift_declined(name, mode):
    """the chain is left to the three kernels when it is not the in-place pattern"""
    c = (name, mode, (128, 64), 3, 33, "")
    # the ROPE result is also a graph output: three launches, the output holds the rotated f32 values, the cache their quantization
    sg, got, cnt, _, ropes = run(c, fusion=1, graphs=0, rope_is_output=True)
    assert cnt["kernels_launched"] == 3, cnt["kernels_launched"]
    x64 = sg.rotated64()
    r32 = ropes[0]
    assert r32.shape == x64.shape
    assert ec.nmse(x64, r32) <= 1e-6 and np.abs(x64 - r32).max() <= 1e-3, (ec.nmse(x64, r32), np.abs(x64 - r32).max())      # test_rope's gate
    assert np.array_equal(sg.rows(got[0]), orc.quantize(r32, sg.t)), "the cache does not hold the quantized ROPE output"
    assert np.array_equal(got[0].reshape(sg.cells, -1)[sg.kv:], sg.data[0].reshape(sg.cells, -1)[sg.kv:])
    # the final CPY targets another cache tensor: three launches, that cache holds the quantized rotated rows, the source cache keeps its bytes
    sg2, src_after, cnt2, others, _ = run(c, fusion=1, graphs=0, target="other")
    assert cnt2["kernels_launched"] == 3, cnt2["kernels_launched"]
    assert np.array_equal(src_after[0], sg2.data[0]), "the source cache changed"
    assert np.array_equal(sg2.rows(others[0]), orc.quantize(r32, sg2.t)), "the target cache does not hold the quantized rotated rows"
    assert (others[0].reshape(sg2.cells, -1)[sg2.kv:] == 0x5A).all(), "cells outside the target view changed"
    e_got, e_ref = requant_errors(sg2, x64, sg2.rows(others[0]))
    print(f"declined {name} mode {mode}: e_got {e_got:.4e} e_ref {e_ref:.4e} ratio {e_got / e_ref:.4f}")
    assert e_got <= 1.25 * e_ref, (e_got, e_ref)


def test_kv_shift_f16_cache_control():
    """the F16-cache form of the same graph (build_rope_shift's other branch: ggml_rope_ext_inplace on the view) stays accepted and stays within the
    tolerance tests/test_gpu_elem_ops.py::test_rope holds an F16 result to: 1 ulp of the once-rounded float64 result. That rule is only tenable where
    float32 arithmetic is that good (elem_cases.rope_inputs: positions of at most 3 in magnitude, every result at least 2^-9), so this case takes
    test_rope's sizes and frequency base, shifts of -3 .. 3 and the first seed that keeps the results that large; the float32 evaluation is checked
    against the rule first, as tests/test_elem_cases.py does for test_rope's cases"""
    mode, hd, n_rot, nh, kv = 2, 128, 64, ec.ROPE_NHEAD, ec.ROPE_NTOK
    shifts = np.array([0, -2, -2, 3, -1], dtype=np.int32)
    ec_case = (F16, mode, (hd, n_rot), (False, 0.0, 1.0), "cont")
    for seed in range(400):
        data = [np.random.default_rng(seed).uniform(-1, 1, size=(1, 1, kv + EXTRA_CELLS, hd * nh)).astype(np.float16)]
        x = data[0].reshape(kv + EXTRA_CELLS, nh, hd)[:kv][None].astype(np.float32)
        r64 = ec.rope_eval(ec_case, x, shifts, None)
        if np.abs(r64).min() >= ec.ROPE_F16_MIN:
            break
    else:
        raise AssertionError("no seed keeps every F16 ROPE result above 2^-9")
    ulps, frac = ec.compare_rounded(F16, ec.enc(F16, ec.rope_eval_f32(ec_case, x, shifts, None)), r64)
    assert ulps <= 1 and frac <= ec.HALF_DIFF_CAP, ("the float32 evaluation does not keep to the rule on these inputs", ulps, frac)
    c = ("f16", mode, (hd, n_rot), nh, kv, "")
    sg, got, cnt, _, _ = run(c, fusion=1, graphs=0, shifts=shifts, data=data, freq_base=500000.0)
    assert cnt["kernels_launched"] == 1
    assert np.array_equal(sg.rotated64(), r64)
    ec.assert_half(F16, sg.rows(got[0]), r64, "f16 cache shift")
    assert np.array_equal(got[0].reshape(sg.cells, -1)[sg.kv:], data[0].reshape(sg.cells, -1)[sg.kv:])
