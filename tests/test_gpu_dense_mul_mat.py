"""Dense MUL_MAT and MUL_MAT_ID (F16 / BF16 / F32 src0) on the GPU, over tests/dense_mm_cases.py: the reference's whole grid for the op
(tests/test-backend-ops.cpp:5716-5763, :5791-5813) and one case per boundary of this backend's dispatch. Every case asserts supports_op, the
kernel that ran (the per-path counters of ggml_backend_mi355x_counters) and the result: bit equality with float64 on the exact inputs, the
element-wise rounding bound on the random ones (dense_mm_cases.py says why each holds). Sentinel tensors sit before and after dst."""
import numpy as np
import pytest

import dense_mm_cases as dm
from gpu_util import SENTINEL_ELEMS, backend, gg

pytestmark = pytest.mark.gpu
L = gg.base()
GG_T = {dm.F32: gg.F32, dm.F16: gg.F16, dm.BF16: gg.BF16}
SENT = np.full((1, SENTINEL_ELEMS), 3.25, np.float32)
COUNTERS = ["dense_" + p for p in dm.PATHS] + ["dense_id"]


def make_operand(ctx, op, lay, name):
    """-> (parent tensor, the view the op reads), built with the ggml constructor the layout names; the view must be what operand() describes"""
    par = ctx.new_tensor(GG_T[op["t"]], op["parent_ne"], name)
    ne, nb = op["ne"], op["nb"]
    if lay[0] == "cont":
        v = par
    elif lay[0] == "perm":
        v = L.ggml_permute(ctx.ctx, par, *lay[1])
    elif lay[0] == "view":
        v = L.ggml_view_4d(ctx.ctx, par, ne[0], ne[1], ne[2], ne[3], nb[1], nb[2], nb[3], op["off"])
    else:
        v = L.ggml_transpose(ctx.ctx, par)
    t = v.contents
    assert tuple(t.ne) == tuple(ne) and tuple(t.nb) == tuple(nb) and (t.view_offs if t.view_src else 0) == op["off"], (tuple(t.ne), tuple(t.nb), op)
    return par, v


class Launch:
    """one op whose result lies between two sentinels, allocated once; run() sets the inputs, computes and returns dst and the counters of
    that compute. The buffer holds the tensors in the order they are made: the operands' parents, a sentinel, dst, a sentinel (as
    gpu_util.run_mul_mat lays them out), so a store on either side of dst lands in a sentinel. operands() -> (parent tensors, views);
    make_op(views) -> the op node."""

    def __init__(self, ctx, operands, make_op):
        self.ctx, self.be = ctx, backend()
        self.parents, views = operands()
        self.s0 = ctx.new_tensor(gg.F32, [SENTINEL_ELEMS], "sent0")
        self.out = make_op(views)
        self.s1 = ctx.new_tensor(gg.F32, [SENTINEL_ELEMS], "sent1")

    def alloc(self):
        assert self.ctx.alloc(self.be)
        for p in self.parents:
            assert p.contents.data % 16 == 0      # the predicate's restatement takes the parents as 16-byte aligned
        addr = [t.contents.data for t in self.parents + [self.s0, self.out, self.s1]]
        assert addr == sorted(addr) and self.s0.contents.data + SENTINEL_ELEMS * 4 <= self.out.contents.data, "the sentinels do not enclose dst"
        gg.tensor_set(self.s0, SENT); gg.tensor_set(self.s1, SENT)
        self.graph = gg.graph_of(self.ctx, self.out)

    def run(self, arrays):
        for t, arr in zip(self.parents, arrays):
            gg.tensor_set(t, arr)
        L.ggml_backend_tensor_memset(self.out, 0xFF, 0, L.ggml_nbytes(self.out))      # (NaN: an element the kernel does not write shows)
        self.be.reset_counters()
        self.be.compute(self.graph)
        cnt = self.be.counters()
        got = gg.tensor_get(self.out).copy()
        for s in (self.s0, self.s1):
            assert np.array_equal(gg.tensor_get(s)[0, 0], SENT), "a sentinel next to dst was overwritten"
        for t, arr in zip(self.parents, arrays):      # the operands and the padding around their views come back as they were set
            back = gg.tensor_get(t)
            assert back.tobytes() == np.ascontiguousarray(arr).tobytes(), "an operand was written to"
        return got, cnt


def assert_path(cnt, path, what):
    got = {n: cnt[n] for n in COUNTERS if cnt[n]}
    assert got == {"dense_" + path: 1}, (what, "expected " + path, got)


def mm_launch(ctx, c):
    a_op, b_op = dm.operands(c)

    def operands():
        pa, a = make_operand(ctx, a_op, c.lay_a, "a")
        pb, b = make_operand(ctx, b_op, c.lay_b, "b")
        return [pa, pb], (a, b)
    ln = Launch(ctx, operands, lambda v: L.ggml_mul_mat(ctx.ctx, v[0], v[1]))
    assert ln.be.supports_op(ln.out), "supports_op refused a dense MUL_MAT"
    ln.alloc()
    return ln, a_op, b_op


@pytest.mark.parametrize("c", dm.CASES, ids=dm.case_id)
def test_mul_mat(c):
    what = dm.case_id(c)
    path = dm.expected_path(c)
    with gg.Context() as ctx:
        ln, a_op, b_op = mm_launch(ctx, c)
        for kind in ("exact", "random"):
            a_s, b_s = dm.inputs(c, kind)
            exp, mag = dm.expected(c, a_s, b_s)
            got, cnt = ln.run([dm.embed(a_op, a_s), dm.embed(b_op, b_s)])
            assert_path(cnt, path, what)
            if kind == "exact":
                dm.assert_exact(got, exp, what)
            else:
                dm.assert_random(got, exp, dm.random_bound(c.ta, c.tb, c.k, mag), what)


@pytest.mark.parametrize("c", dm.CONV_CASES, ids=dm.conv_id)
def test_conversion(c):
    """the identity against the hard values of a type: what the kernel's loads and conversions make of subnormals, the largest finite
    values and full mantissas comes back bit for bit. 64 columns: the matrix cores (F16 x F32), the F32 rows kernel and the generic kernel; 8 columns:
    the F16 pair kernel and the F32 vector kernel"""
    cc = dm.conv_case(c)
    a_s, b_s, want = dm.conv_inputs(c)
    with gg.Context() as ctx:
        ln, a_op, b_op = mm_launch(ctx, cc)
        got, cnt = ln.run([dm.embed(a_op, a_s), dm.embed(b_op, b_s)])
    assert_path(cnt, dm.expected_path(cc), dm.conv_id(c))
    dm.assert_conversion(got, want, dm.conv_id(c))


@pytest.mark.parametrize("c", dm.ID_CASES, ids=dm.id_case_id)
def test_mul_mat_id(c):
    """ids = a strided view (the first n_used of n_mats columns) of a shuffled [n_mats, n] tensor, as tests/test-backend-ops.cpp:3231-3236"""
    what = dm.id_case_id(c)
    a_op = dm.id_operand(c)
    nb = 1 if c.bcast_b else c.n_used
    with gg.Context() as ctx:
        def operands():
            pa, a = make_operand(ctx, a_op, c.lay_a, "as")
            b = ctx.new_tensor(gg.F32, (c.k, nb, c.n), "b")
            ids = ctx.new_tensor(gg.I32, (c.n_mats, c.n), "ids")
            idv = L.ggml_view_2d(ctx.ctx, ids, c.n_used, c.n, c.n_mats * 4, 0)
            return [pa, b, ids], (a, b, idv)
        ln = Launch(ctx, operands, lambda v: L.ggml_mul_mat_id(ctx.ctx, *v))
        assert ln.be.supports_op(ln.out)
        ln.alloc()
        for kind in ("exact", "random"):
            a_s, b_s, ids = dm.id_inputs(c, kind)
            exp, mag = dm.id_expected(c, a_s, b_s, ids)
            got, cnt = ln.run([dm.embed(a_op, a_s), b_s, ids.reshape(1, 1, c.n, c.n_mats)])
            assert_path(cnt, "id", what)
            if kind == "exact":
                dm.assert_exact(got[0], exp, what)
            else:
                dm.assert_random(got[0], exp, dm.random_bound(c.ta, dm.F32, c.k, mag), what)


def test_mul_mat_id_refuses_more_pairs_than_a_grid_dim():
    """k_mm_id_dense has the slots in grid dim y and the tokens in grid dim z: supports_op refuses what does not fit (no compute here)"""
    be = backend()
    for n_used, n_tok, ok in ((2, 65535, True), (2, 65536, False)):
        with gg.Context() as ctx:
            a = ctx.new_tensor(gg.F16, (4, 2, 2)); b = ctx.new_tensor(gg.F32, (4, 1, n_tok)); ids = ctx.new_tensor(gg.I32, (n_used, n_tok))
            assert be.supports_op(L.ggml_mul_mat_id(ctx.ctx, a, b, ids)) == ok, (n_used, n_tok)

