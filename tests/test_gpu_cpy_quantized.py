"""CPY with a Q8_0 / Q4_0 side, the three forms a quantized KV cache's shift and defrag graphs hold (src/llama-kv-cache-unified.cpp:1416-1670): F32 -> q
(ggml_cpy back into the cache after the rotation), q -> F32 (ggml_cast) and q -> q between two views of one cache (a defrag move), each as one-op graphs
through the backend C-ABI. Expected bytes come from the oracle's row quantizers and dequantizers (pinned by tests/golden/quant_*.npz, dequant_*.npz): all
comparisons are bit for bit. The cache side is always a view into a larger cache tensor whose other bytes must keep their values. Every case asserts
supports_op first; what stays refused is asserted refused."""
import numpy as np
import pytest

import oracle as orc
from gpu_util import backend, gg

pytestmark = pytest.mark.gpu
L = gg.base()
F32, F16 = gg.F32, gg.F16
QT = {"q8_0": gg.Q8_0, "q4_0": gg.Q4_0}
SHAPES = [(64, 3), (128, 2, 33), (256, 4, 4, 4)]


def ne4(ne):
    return tuple(ne) + (1,) * (4 - len(ne))


def f32_rows(ne, seed):
    """[ne3, ne2, ne1, ne0] from U(-1, 1) with one all-zero block and two blocks whose largest magnitude occurs twice with opposite signs (Q4_0 takes
    the sign of the FIRST such element for its scale: one block has the negative one first, one the positive)"""
    hd, n1, n2, n3 = ne4(ne)
    x = np.random.default_rng(seed).uniform(-1, 1, size=(n3, n2, n1, hd)).astype(np.float32)
    x[0, 0, 0, 0:32] = 0.0
    x[-1, -1, -1, 32:64] *= 0.5
    x[-1, -1, -1, 32 + 3] = -0.9; x[-1, -1, -1, 32 + 17] = 0.9
    x[0, 0, 0, 32:64] *= 0.5
    x[0, 0, 0, 32 + 5] = 0.8; x[0, 0, 0, 32 + 30] = -0.8
    return x


class CacheView:
    """a cache tensor [hd*n1, rows] of type qt, pre-filled with valid blocks, and the view [hd, n1, n2, n3] into it that the K-shift takes (view_3d with
    nb1 = row_size(hd), nb2 = row_size(hd*n1); one more dim for ne3 > 1): the view starts one cell in, leaves one cell out between the ne3 slabs and one at the end"""

    def __init__(self, ctx, qt, ne, seed):
        self.hd, self.n1, self.n2, self.n3 = ne4(ne)
        self.qt = qt
        self.cells = (self.n2 + 1) * self.n3 + 1
        self.rs1, self.rs2 = orc.row_size(qt, self.hd), orc.row_size(qt, self.hd * self.n1)
        self.t = ctx.new_tensor(qt, (self.hd * self.n1, self.cells))
        self.bytes0 = orc.random_blocks(np.random.default_rng(seed), qt, (1, 1, self.cells), self.hd * self.n1)
        if self.n3 == 1:
            self.view = L.ggml_view_3d(ctx.ctx, self.t, self.hd, self.n1, self.n2, self.rs1, self.rs2, self.rs2)
        else:
            self.view = L.ggml_view_4d(ctx.ctx, self.t, self.hd, self.n1, self.n2, self.n3, self.rs1, self.rs2, self.rs2 * (self.n2 + 1), self.rs2)

    def cells_of_view(self):
        return np.array([1 + i3 * (self.n2 + 1) + i2 for i3 in range(self.n3) for i2 in range(self.n2)])

    def rows(self, cache_bytes):
        """the view's rows out of the whole cache's bytes -> [n3, n2, n1, row_size(hd)]"""
        return cache_bytes.reshape(self.cells, self.n1, self.rs1)[self.cells_of_view()].reshape(self.n3, self.n2, self.n1, self.rs1)

    def with_rows(self, rows):
        out = self.bytes0.copy().reshape(self.cells, self.n1, self.rs1)
        out[self.cells_of_view()] = rows.reshape(-1, self.n1, self.rs1)
        return out.reshape(self.bytes0.shape)


def strided_f32(ctx, ne, data=None):
    """an F32 tensor [hd, n1, n2, n3] as a permuted, strided view that starts off alignment: the parent is [n1 + 1, hd + 3, n2, n3], the view takes its
    box from element (1, 1) on and swaps the first two dims (nb0 = (n1 + 1)*4, nb1 = 4). -> (view, parent, parent array holding `data`)"""
    hd, n1, n2, n3 = ne4(ne)
    par = ctx.new_tensor(F32, (n1 + 1, hd + 3, n2, n3))
    arr = np.full((n3, n2, hd + 3, n1 + 1), 7.25, np.float32)
    if data is not None:
        arr[:, :, 1:hd + 1, 1:n1 + 1] = data.transpose(0, 1, 3, 2)
    nb1 = (n1 + 1) * 4; nb2 = nb1 * (hd + 3); nb3 = nb2 * n2
    box = L.ggml_view_4d(ctx.ctx, par, n1, hd, n2, n3, nb1, nb2, nb3, nb1 + 4)
    return L.ggml_permute(ctx.ctx, box, 1, 0, 2, 3), par, arr


def same_bytes(got, exp, what):
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, len(bad), bad[:6].tolist(), [int(got[tuple(b)]) for b in bad[:6]], [int(exp[tuple(b)]) for b in bad[:6]])


@pytest.mark.parametrize("src_layout", ["cont", "permuted"])
@pytest.mark.parametrize("ne", SHAPES, ids=str)
@pytest.mark.parametrize("name", list(QT))
def test_cpy_f32_to_quantized(name, ne, src_layout):
    """the written rows equal the reference quantizer's bytes (a zero block keeps Q4_0's -0.0 scale; a tie in magnitude takes the first element's sign),
    and every byte of the cache outside the view keeps its value"""
    qt = QT[name]
    x = f32_rows(ne, 11)
    be = backend()
    with gg.Context() as ctx:
        cv = CacheView(ctx, qt, ne, 12)
        if src_layout == "cont":
            src = ctx.new_tensor(F32, ne4(ne)); par, arr = src, x
        else:
            src, par, arr = strided_f32(ctx, ne, x)
        o = L.ggml_cpy(ctx.ctx, src, cv.view)
        assert be.supports_op(o), "CPY F32 -> %s refused" % name
        assert ctx.alloc(be)
        gg.tensor_set(cv.t, cv.bytes0); gg.tensor_set(par, arr)
        be.compute(gg.graph_of(ctx, o))
        got = gg.tensor_get(cv.t)
    same_bytes(got, cv.with_rows(orc.quantize(x, qt)), (name, ne, src_layout))


@pytest.mark.parametrize("dst_layout", ["cont", "permuted"])
@pytest.mark.parametrize("ne", SHAPES, ids=str)
@pytest.mark.parametrize("name", list(QT))
def test_cpy_quantized_to_f32(name, ne, dst_layout):
    """ggml_cast of the cache view (and ggml_cpy into a strided F32 view): bit-equal to the oracle's dequantization; the cache keeps its bytes and a
    strided destination's parent keeps everything outside the view"""
    qt = QT[name]
    be = backend()
    with gg.Context() as ctx:
        cv = CacheView(ctx, qt, ne, 13)
        if dst_layout == "cont":
            o = L.ggml_cast(ctx.ctx, cv.view, F32); par, arr = o, None
        else:
            dst, par, arr = strided_f32(ctx, ne)
            o = L.ggml_cpy(ctx.ctx, cv.view, dst)
        assert be.supports_op(o), "CPY %s -> F32 refused" % name
        assert ctx.alloc(be)
        gg.tensor_set(cv.t, cv.bytes0)
        if arr is not None:
            gg.tensor_set(par, arr)
        be.compute(gg.graph_of(ctx, o))
        got = gg.tensor_get(par); cache = gg.tensor_get(cv.t)
    exp = orc.dequantize(cv.rows(cv.bytes0), qt)
    hd, n1, n2, n3 = ne4(ne)
    if arr is not None:
        arr[:, :, 1:hd + 1, 1:n1 + 1] = exp.transpose(0, 1, 3, 2); exp = arr
    same_bytes(got.view(np.uint32), exp.view(np.uint32), (name, ne, dst_layout))
    same_bytes(cache, cv.bytes0, "the source cache changed")


@pytest.mark.parametrize("name", list(QT))
def test_cpy_quantized_moves(name):
    """build_graph_defrag (src/llama-kv-cache-unified.cpp:1528-1670): four disjoint view_2d -> view_2d moves of 1, 3, 7 and 16 cells inside a
    [n_embd_k_gqa = 256, 64 cells] cache in one graph, and the same for a second tensor standing for V under -fa 1"""
    qt = QT[name]
    n_embd, cells = 256, 64
    rs = orc.row_size(qt, n_embd)
    moves = [(16, 48, 0), (7, 40, 16), (3, 36, 24), (1, 34, 30)]      # (cells, from, to): cells from the tail into holes at the front, all ranges disjoint
    be = backend()
    rng = np.random.default_rng(14)
    with gg.Context() as ctx:
        caches = [ctx.new_tensor(qt, (n_embd, cells)) for _ in range(2)]
        data = [orc.random_blocks(rng, qt, (1, 1, cells), n_embd) for _ in caches]
        outs = []
        for t in caches:
            for n, a, b in moves:
                o = L.ggml_cpy(ctx.ctx, L.ggml_view_2d(ctx.ctx, t, n_embd, n, rs, rs * a), L.ggml_view_2d(ctx.ctx, t, n_embd, n, rs, rs * b))
                assert be.supports_op(o), "CPY %s -> %s refused" % (name, name)
                outs.append(o)
        assert ctx.alloc(be)
        for t, d in zip(caches, data):
            gg.tensor_set(t, d)
        be.compute(gg.graph_of(ctx, *outs))
        got = [gg.tensor_get(t) for t in caches]
    for g_, d in zip(got, data):
        exp = d.copy()
        for n, a, b in moves:
            exp[0, 0, b:b + n] = d[0, 0, a:a + n]
        same_bytes(g_, exp, name)


def test_cpy_quantized_refusals():
    """what stays with the CPU: F16 / BF16 on the other side, a change of block type, every other block type, rows that are not whole blocks or differ
    in length, and CONT / DUP of a quantized tensor"""
    be = backend()
    Q4_K = gg.Q4_K
    with gg.Context() as ctx:
        c = ctx.ctx
        new = ctx.new_tensor
        assert not be.supports_op(L.ggml_cpy(c, new(F16, (64, 3)), new(gg.Q8_0, (64, 3)))), "F16 -> Q8_0"
        assert not be.supports_op(L.ggml_cast(c, new(gg.Q8_0, (64, 3)), F16)), "Q8_0 -> F16"
        assert not be.supports_op(L.ggml_cpy(c, new(gg.BF16, (64, 3)), new(gg.Q4_0, (64, 3)))), "BF16 -> Q4_0"
        assert not be.supports_op(L.ggml_cpy(c, new(gg.Q8_0, (64, 3)), new(gg.Q4_0, (64, 3)))), "Q8_0 -> Q4_0"
        assert not be.supports_op(L.ggml_cpy(c, new(gg.Q4_0, (64, 3)), new(gg.Q8_0, (64, 3)))), "Q4_0 -> Q8_0"
        assert not be.supports_op(L.ggml_cast(c, new(Q4_K, (256, 3)), F32)), "Q4_K -> F32"
        assert not be.supports_op(L.ggml_cpy(c, new(F32, (256, 3)), new(Q4_K, (256, 3)))), "F32 -> Q4_K"
        assert not be.supports_op(L.ggml_cpy(c, new(F32, (64, 3)), new(gg.Q5_0, (64, 3)))), "F32 -> Q5_0"
        # ne[0] = 48 is no multiple of the block size: described by hand (ggml_new_tensor asserts on such a row)
        a, b = new(F32, (64, 3)), new(gg.Q8_0, (64, 3))
        o = L.ggml_cpy(c, a, b)
        a.contents.ne[0] = 48; b.contents.ne[0] = 48; o.contents.ne[0] = 48
        assert not be.supports_op(o), "F32 -> Q8_0, ne[0] = 48"
        # the same number of elements in rows of another length
        assert not be.supports_op(L.ggml_cpy(c, new(F32, (128, 3)), new(gg.Q8_0, (64, 6)))), "F32 [128, 3] -> Q8_0 [64, 6]"
        q = new(gg.Q8_0, (128, 8))
        v = L.ggml_view_2d(c, q, 64, 8, orc.row_size(gg.Q8_0, 128), 0)
        assert not be.supports_op(L.ggml_cont(c, v)), "CONT of a Q8_0 view"
        assert not be.supports_op(L.ggml_dup(c, q)), "DUP of a Q8_0 tensor"
        # and the accepted forms, so that this test fails where nothing quantized is accepted at all
        assert be.supports_op(L.ggml_cast(c, v, F32)) and be.supports_op(L.ggml_cpy(c, new(F32, (64, 8)), v))
