"""Every type, layout and variant of the element ops that `supports_op` accepts (csrc/backend.cpp mi_supports_op), each as a
one-op graph through the backend C-ABI and compared with the float64 definitions in oracle/ops_ref.py. The grid is the reference's own
(tests/test-backend-ops.cpp:5274-6030): its two shapes, (128, 2, 2, 2) and (5, 7, 11, 13) — odd ne0, a partial last workgroup, all four
coordinates live — each also as a view whose parent has 3 more columns and one more row per dim and which starts at element 1, so that
rows are strided and not 16-byte aligned (UNARY and GLU want dims 1..3 contiguous: their views have the wider rows only).

Every case asserts supports_op first (a refusal of something §7 lists is a failure), keeps sentinel tensors before and after the output and
checks them, pre-fills the parent wherever the destination is a view and compares the whole parent, and quantizes its inputs to the source
type before the reference is computed.

Tolerances (derived, none tuned):
  bit-exact, as integers: ABS, NEG, SGN, STEP, RELU; CPY, CONT, DUP; GET_ROWS, SET_ROWS (conversions against round_f16 / round_bf16); ARGSORT.
      NaN positions are compared as "is NaN".
  F32 output: ADD, SUB, MUL, DIV, SCALE within 1 ulp of the float64 result rounded to float32 (one correctly rounded operation each);
      the rest by the reference's gates, as tests/test_gpu_ops.py: NMSE <= 1e-7, <= 1e-6 for the transcendental UNARY ops and SOFT_MAX,
      ROPE <= 1e-6 and max |diff| <= 1e-3.
  F16 / BF16 output: within 1 ulp of the float64 result rounded once to the type, and at most 1 % of a case's elements different at all.
      tests/test_elem_cases.py checks on the CPU, for the inputs of every such case, that a float32 evaluation keeps to this.

Not covered: the 64-bit branches of `unravel` / `wrap` (elem.hip) need 2^31 elements."""
import numpy as np
import pytest

import elem_cases as ec
import ops_ref as ref
from elem_cases import BF16, F16, F32, I32
from gpu_util import SENTINEL_ELEMS, backend, gg

pytestmark = pytest.mark.gpu
L = gg.base()
I64 = gg.I64


class H:
    """one graph: tensors in creation order = buffer order, so `sent()` before and after the op's output brackets it"""

    def __init__(self):
        self.ctx = gg.Context(); self.c = self.ctx.ctx; self.sets = []; self.sents = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.free()

    def new(self, t, ne, data=None):
        x = self.ctx.new_tensor(t, ne)
        if data is not None:
            assert tuple(data.shape) == tuple(list(ne) + [1] * (4 - len(ne)))[::-1], (data.shape, ne)
            self.sets.append((x, data))
        return x

    def view(self, t, data, extra_rows=True):
        """the view form of `data` (storage, [ne3, ne2, ne1, ne0]) -> (view tensor, parent tensor, parent array)"""
        ne = data.shape[::-1]
        pne = ec.view_parent_ne(ne, extra_rows)
        par = ec.embed(t, data, extra_rows)
        p = self.new(t, pne, par)
        es = ec.ESIZE[t]
        nb1 = pne[0] * es; nb2 = nb1 * pne[1]; nb3 = nb2 * pne[2]
        return L.ggml_view_4d(self.c, p, *ne, nb1, nb2, nb3, es), p, par

    def src(self, t, data, view, extra_rows=True):
        return self.view(t, data, extra_rows)[0] if view else self.new(t, data.shape[::-1], data)

    def sent(self):
        self.sents.append(self.ctx.new_tensor(F32, [SENTINEL_ELEMS]))

    def go(self, *outs):
        be = backend()
        for o in outs:
            assert be.supports_op(o), "the backend refused an op INTEGRATION.md §7 lists"
        assert self.ctx.alloc(be)
        pat = (np.arange(SENTINEL_ELEMS, dtype=np.float32) * 0.5 + 7.25).reshape(1, 1, 1, -1)
        for s in self.sents:
            gg.tensor_set(s, pat)
        for x, a in self.sets:
            gg.tensor_set(x, a)
        be.compute(gg.graph_of(self.ctx, *outs))
        for s in self.sents:
            assert np.array_equal(gg.tensor_get(s), pat), "a sentinel next to the output was overwritten"


def bracket(h, make):
    h.sent(); o = make(); h.sent()
    return o


def refused(o):
    return not backend().supports_op(o)


def set_op_f32(o, i, v):
    o.contents.op_params[i] = int(np.array([v], np.float32).view(np.int32)[0])


# ---- ADD / SUB / MUL / DIV ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ec.BIN_CASES, ids=ec.bin_id)
def test_bin(c):
    op, (ta, tb, td), ne, nr = c
    x, y = ec.bin_inputs(c)
    with H() as h:
        a = h.new(ta, x.shape[::-1], ec.enc(ta, x)); b = h.new(tb, ne, ec.enc(tb, y))
        o = bracket(h, lambda: getattr(L, f"ggml_{op}")(h.c, a, b))
        assert o.contents.type == td
        h.go(o); got = gg.tensor_get(o)
    exp = ec.bin_eval(c, x, y, np.float64)
    if td == F32:
        ec.assert_f32_1ulp(got, exp, ec.bin_id(c))
    else:
        ec.assert_half(td, got, exp, ec.bin_id(c))


@pytest.mark.parametrize("op", ec.BIN_OPS)
@pytest.mark.parametrize("t", [F32, F16, BF16], ids=lambda t: ec.TNAME[t])
@pytest.mark.parametrize("ne", ec.SHAPES, ids=str)
def test_bin_views(op, t, ne):
    """both operands and nothing else: a and b as the view form (strided rows, 4 / 2 bytes off 16-byte alignment), b repeated over ne1"""
    c = (op, (t, t, t), (ne[0], 1, ne[2], ne[3]), (1, ne[1], 1, 1))
    x, y = ec.bin_inputs(c)
    with H() as h:
        a = h.src(t, ec.enc(t, x), True); b = h.src(t, ec.enc(t, y), True)
        o = bracket(h, lambda: getattr(L, f"ggml_{op}")(h.c, a, b))
        h.go(o); got = gg.tensor_get(o)
    exp = ec.bin_eval(c, x, y, np.float64)
    if t == F32:
        ec.assert_f32_1ulp(got, exp)
    else:
        ec.assert_half(t, got, exp)


# ---- UNARY -------------------------------------------------------------------------------------------------------------------------
UNARY_TRANSCENDENTAL = (4, 5, 7, 8, 9, 10, 13, 14)     # TANH, ELU, SIGMOID, GELU, GELU_QUICK, SILU, EXP, GELU_ERF: the 1e-6 gate


@pytest.mark.parametrize("c", ec.UNARY_CASES, ids=ec.unary_id)
def test_unary(c):
    op, t, ne, view = c
    x = ec.unary_inputs(c)
    with H() as h:
        a = h.src(t, ec.enc(t, x), view, extra_rows=False)
        o = bracket(h, lambda: L.ggml_unary(h.c, a, op))
        h.go(o); got = gg.tensor_get(o)
    exp = ec.unary_eval(c, x, np.float64)
    if op in ec.UNARY_EXACT:
        assert ec.same_storage(t, got, ec.enc(t, exp)), ec.unary_id(c)
    else:
        ec.assert_out(t, got, exp, 1e-6 if op in UNARY_TRANSCENDENTAL else 1e-7, ec.unary_id(c))


# ---- GLU ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ec.GLU_CASES, ids=ec.glu_id)
def test_glu(c):
    """split (two tensors, also as column views of one wide tensor: build_ffn's fused gate_up) and single-tensor ([x | g] along ne0,
    `swapped`: [g | x]); +-150 where the reference uses it to catch overflow: the result must be finite"""
    op, t, form, ne = c
    x, g = ec.glu_inputs(c)
    xs, gs = ec.enc(t, x), ec.enc(t, g)
    es = ec.ESIZE[t]
    with H() as h:
        if form == "split":
            a = h.new(t, ne, xs); b = h.new(t, ne, gs)
        elif form == "split_views":
            w = h.new(t, (2 * ne[0],) + ne[1:], np.concatenate([xs, gs], axis=-1))
            nb1 = 2 * ne[0] * es; nb2 = nb1 * ne[1]; nb3 = nb2 * ne[2]
            a = L.ggml_view_4d(h.c, w, *ne, nb1, nb2, nb3, 0); b = L.ggml_view_4d(h.c, w, *ne, nb1, nb2, nb3, ne[0] * es)
        else:
            a = h.new(t, (2 * ne[0],) + ne[1:], np.concatenate([gs, xs] if form == "single_swapped" else [xs, gs], axis=-1)); b = None

        def make():
            if b is None:
                o = L.ggml_glu(h.c, a, op, form == "single_swapped")
                if op == gg.GLU_SWIGLU_OAI:
                    set_op_f32(o, 2, 1.702); set_op_f32(o, 3, 7.0)
                return o
            return L.ggml_swiglu_oai(h.c, a, b, 1.702, 7.0) if op == gg.GLU_SWIGLU_OAI else L.ggml_glu_split(h.c, a, b, op)
        o = bracket(h, make)
        assert tuple(o.contents.ne) == ne and o.contents.type == t
        h.go(o); got = gg.tensor_get(o)
    exp = ec.glu_eval(c, x, g, np.float64)
    assert np.isfinite(ec.dec(t, got)).all()
    ec.assert_out(t, got, exp, 1e-7, ec.glu_id(c))


# ---- CPY / CONT / DUP --------------------------------------------------------------------------------------------------------------
CPY_PAIRS = [(s, d) for s in (F32, F16, BF16) for d in (F32, F16, BF16)] + [(I32, I32)]
PAIR_ID = lambda p: f"{ec.TNAME[p[0]]}_{ec.TNAME[p[1]]}"
I32_SPECIALS = np.array([0, 1, -1, 16777217, -16777217, 123456789, -123456789, np.iinfo(np.int32).max, np.iinfo(np.int32).min], dtype=np.int32)


def rand_storage(t, ne, seed, specials=True):
    """a source of type t; an F32 source carries the conversion specials, an I32 source the values a float cannot hold"""
    rng = np.random.default_rng(seed)
    if t == I32:
        s = rng.integers(-2 ** 31, 2 ** 31, size=ne[::-1], dtype=np.int64).astype(np.int32)
        s.reshape(-1)[:min(s.size, I32_SPECIALS.size)] = I32_SPECIALS[:s.size]
        return s
    x = rng.uniform(-1, 1, size=ne[::-1]).astype(np.float32)
    if t == F32 and specials:
        sp = ec.conversion_specials()
        if x.size >= sp.size:
            x.reshape(-1)[-sp.size:] = sp
    return ec.enc(t, x)


@pytest.mark.parametrize("pair", CPY_PAIRS, ids=PAIR_ID)
@pytest.mark.parametrize("perm", [(0, 2, 1, 3), (1, 0, 2, 3), (0, 3, 1, 2)], ids=str)
@pytest.mark.parametrize("ne", [(256, 2, 3, 4), (10, 8, 3, 1)], ids=str)
def test_cpy_permuted_src(pair, perm, ne):
    """tests/test-backend-ops.cpp:5565-5599; the F32 source holds the conversion specials (overflow edges, subnormals, ties, NaN, infinities)"""
    ts, td = pair
    s = rand_storage(ts, ne, 60)
    with H() as h:
        a = h.new(ts, ne, s)
        p = L.ggml_permute(h.c, a, *perm)
        h.sent(); d = h.new(td, ec.permuted_ne(ne, perm)); h.sent()
        o = L.ggml_cpy(h.c, p, d)
        h.go(o); got = gg.tensor_get(d)
    exp = ec.convert(ts, td, np.ascontiguousarray(np.transpose(s, ec.permute_axes(perm))))
    assert ec.same_storage(td, got, exp)


@pytest.mark.parametrize("pair", CPY_PAIRS, ids=PAIR_ID)
@pytest.mark.parametrize("ne", [(256, 2, 3, 4), (10, 8, 3, 1)], ids=str)
@pytest.mark.parametrize("dst", ["permuted", "view"])
def test_cpy_noncontiguous_dst(pair, ne, dst):
    """the destination permuted (1, 0, 2, 3) ("dst not contiguous", tests/test-backend-ops.cpp:5562 / :5599), or the view form of a
    pre-filled parent: the whole parent comes back, and every byte outside the view is the pattern"""
    ts, td = pair
    s = rand_storage(ts, ne, 61)
    with H() as h:
        a = h.new(ts, ne, s)
        h.sent()
        if dst == "permuted":
            par0 = rand_storage(td, ne, 62, specials=False)
            par = h.new(td, ne, par0)
            d = L.ggml_permute(h.c, par, 1, 0, 2, 3)
        else:
            d, par, par0 = h.view(td, rand_storage(td, ne, 62, specials=False))
        h.sent()
        o = L.ggml_cpy(h.c, a, d)
        h.go(o)
        got_view, got_par = gg.tensor_get_strided(d)
    exp = par0.copy()
    conv = ec.convert(ts, td, s)
    if dst == "permuted":
        v = np.transpose(exp, ec.permute_axes((1, 0, 2, 3)))
        v[...] = conv.reshape(v.shape)
        assert ec.same_storage(td, got_view, conv.reshape(v.shape))
    else:
        exp[:ne[3], :ne[2], :ne[1], 1:1 + ne[0]] = conv
        assert ec.same_storage(td, got_view, conv)
    assert ec.same_storage(td, got_par, exp), "bytes of the parent that the copy does not own were changed"


@pytest.mark.parametrize("pair", CPY_PAIRS, ids=PAIR_ID)
def test_cpy_between_shapes(pair):
    """equal element counts, different shapes: element i in the source's order becomes element i in the destination's"""
    ts, td = pair
    s = rand_storage(ts, (24, 5, 1, 1), 63)
    with H() as h:
        a = h.new(ts, (24, 5, 1, 1), s)
        h.sent(); d = h.new(td, (6, 4, 5, 1)); h.sent()
        o = L.ggml_cpy(h.c, a, d)
        h.go(o); got = gg.tensor_get(d)
    assert ec.same_storage(td, got, ec.convert(ts, td, ref.cpy(s, (1, 5, 4, 6))))


@pytest.mark.parametrize("t", [F32, F16, BF16], ids=lambda t: ec.TNAME[t])
@pytest.mark.parametrize("ne", [(2, 1, 1, 1), (2, 1, 3, 5), (2, 3, 5, 7)], ids=str)
def test_cont_of_transposed(t, ne):
    """tests/test-backend-ops.cpp:5604-5612 test_cont: CONT of the transposed tensor, and CONT_4D of it into another shape"""
    s = rand_storage(t, ne, 64, specials=False)
    tr = np.ascontiguousarray(np.swapaxes(s, -1, -2))
    with H() as h:
        a = h.new(t, ne, s)
        o = bracket(h, lambda: L.ggml_cont(h.c, L.ggml_transpose(h.c, a)))
        o4 = bracket(h, lambda: L.ggml_cont_4d(h.c, L.ggml_transpose(h.c, a), ne[1] * ne[0], ne[2], ne[3], 1))
        h.go(o, o4); got = gg.tensor_get(o); got4 = gg.tensor_get(o4)
    assert ec.same_storage(t, got, tr)
    assert ec.same_storage(t, got4, tr.reshape(got4.shape))


@pytest.mark.parametrize("t", [F32, F16, I32], ids=lambda t: ec.TNAME[t])
@pytest.mark.parametrize("perm", [None, (1, 0, 2, 3), (0, 2, 1, 3)], ids=str)
def test_dup(t, perm):
    """tests/test-backend-ops.cpp:5555-5562 test_dup"""
    ne = (10, 8, 3, 2)
    s = rand_storage(t, ne, 65)
    with H() as h:
        a = h.new(t, ne, s)
        p = L.ggml_permute(h.c, a, *perm) if perm else a
        o = bracket(h, lambda: L.ggml_dup(h.c, p))
        h.go(o); got = gg.tensor_get(o)
    assert ec.same_storage(t, got, np.ascontiguousarray(np.transpose(s, ec.permute_axes(perm))) if perm else s)


# ---- GET_ROWS ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [F32, F16, BF16, I32], ids=lambda t: ec.TNAME[t])
@pytest.mark.parametrize("n,m", [(256, 5), (33, 7)])
@pytest.mark.parametrize("b", [1, 7])
@pytest.mark.parametrize("view", [False, True], ids=["cont", "view"])
def test_get_rows(t, n, m, b, view):
    """tests/test-backend-ops.cpp:5308-5320: 4 indices per batch with repeats, batches over ne[2]; the rows are moved, not computed. An I32
    source gives an I32 result holding values no float can carry: 16777217 must not come back as 16777216 nor INT32_MAX through a
    float -> int conversion (before this test k_get_rows moved every element through a float)."""
    s = rand_storage(t, (n, m, b, 1), 70 + n)
    rng = np.random.default_rng(71 + b)
    idx = rng.integers(0, m, size=(1, b, 4)).astype(np.int32); idx[0, :, 3] = idx[0, :, 0]      # a repeat in every batch
    with H() as h:
        a = h.src(t, s, view); i = h.new(I32, (4, b, 1), idx.reshape(1, 1, b, 4))
        o = bracket(h, lambda: L.ggml_get_rows(h.c, a, i))
        assert o.contents.type == (I32 if t == I32 else F32)
        h.go(o); got = gg.tensor_get(o)
    moved = ref.get_rows_batched(s, idx)
    if t == I32:
        assert np.array_equal(got, moved)
    else:
        assert ec.same_storage(F32, got, ec.convert(t, F32, moved))


# ---- SET_ROWS into an unquantized destination ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("td", [F32, F16, BF16], ids=lambda t: ec.TNAME[t])
@pytest.mark.parametrize("shape", ["256x5xbx3-nr11-r1", "256x11x1xb-nr23-r7", "31x3xbx1-nr23-r2", "33x5x1xb-nr23-r1"])
@pytest.mark.parametrize("b", [1, 7])
def test_set_rows(td, shape, b):
    """tests/test-backend-ops.cpp:5332-5343 test_set_rows(type, ne, nr23, r): dst [ne0, ne1, ne2*nr2, ne3*nr3], r source rows per batch, the
    index tensor [r, ne2, ne3] broadcast over nr2 / nr3; distinct indices within a batch. The source rows hold the conversion specials;
    the destination is pre-filled and comes back whole: rows that are not addressed keep their bytes."""
    ne, nr, r = {"256x5xbx3-nr11-r1": ((256, 5, b, 3), (1, 1), 1), "256x11x1xb-nr23-r7": ((256, 11, 1, b), (2, 3), 7),
                 "31x3xbx1-nr23-r2": ((31, 3, b, 1), (2, 3), 2), "33x5x1xb-nr23-r1": ((33, 5, 1, b), (2, 3), 1)}[shape]
    n2, n3 = ne[2] * nr[0], ne[3] * nr[1]
    rng = np.random.default_rng(80 + b)
    dst0 = rand_storage(td, (ne[0], ne[1], n2, n3), 81, specials=False)
    src = rng.uniform(-1, 1, size=(n3, n2, r, ne[0])).astype(np.float32)
    sp = ec.conversion_specials()
    src.reshape(-1)[:sp.size] = sp
    idx = np.stack([np.stack([rng.permutation(ne[1])[:r] for _ in range(ne[2])]) for _ in range(ne[3])]).astype(np.int64)     # [ne3, ne2, r]
    with H() as h:
        h.sent(); d = h.new(td, (ne[0], ne[1], n2, n3), dst0); h.sent()
        s = h.new(F32, (ne[0], r, n2, n3), src); i = h.new(I64, (r, ne[2], ne[3]), idx.reshape(1, ne[3], ne[2], r))
        o = L.ggml_set_rows(h.c, d, s, i)
        h.go(o); got = gg.tensor_get(d)
    exp = ref.set_rows_bcast(dst0, src, idx, lambda rows: ec.enc(td, rows))
    assert ec.same_storage(td, got, exp)


# ---- ARGSORT -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [gg.GGML_SORT_ORDER_ASC, gg.GGML_SORT_ORDER_DESC], ids=["asc", "desc"])
@pytest.mark.parametrize("ne0,strided", [(n, False) for n in (1, 2, 3, 8, 16, 60, 100, 129, 1000, 1024)] + [(60, True)])
def test_argsort(order, ne0, strided):
    """rows (3, 2, 2) of distinct values (a permutation each: the order is unique); ne0 = 60 also with the columns strided (nb0 = 12)"""
    rng = np.random.default_rng(90 + ne0)
    x = np.stack([rng.permutation(ne0) for _ in range(12)]).astype(np.float32).reshape(2, 2, 3, ne0)
    with H() as h:
        if strided:
            par = h.new(F32, (3, ne0, 2, 2), np.ascontiguousarray(np.swapaxes(x, -1, -2)))
            a = L.ggml_permute(h.c, par, 1, 0, 2, 3)
            assert a.contents.nb[0] == 12 and tuple(a.contents.ne) == (ne0, 3, 2, 2)
        else:
            a = h.new(F32, (ne0, 3, 2, 2), x)
        o = bracket(h, lambda: L.ggml_argsort(h.c, a, order))
        h.go(o); got = gg.tensor_get(o)
    assert np.array_equal(got, ref.argsort(x, order))


# ---- SOFT_MAX ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [(1, 1, 3, 1), (1, 3, 1, 1), (2, 3, 2, 1), (1, 1, 2, 3)], ids=lambda b: "n%d_%d-r%d_%d" % b)
@pytest.mark.parametrize("ne0", [16, 31, 1031])
@pytest.mark.parametrize("ne1", [1, 5])
@pytest.mark.parametrize("mask_t", [F16, F32], ids=lambda t: ec.TNAME[t])
@pytest.mark.parametrize("sinks", [False, True], ids=["nosink", "sinks"])
@pytest.mark.parametrize("max_bias", [0.0, 8.0])
def test_soft_max_mask_broadcast(bc, ne0, ne1, mask_t, sinks, max_bias):
    """tests/test-backend-ops.cpp:5913-5953: x [ne0, ne1, n2*r2, n3*r3], the mask [ne0, pad64(ne1), n2, n3] repeated r2 / r3 times over ne[2] / ne[3]"""
    n2, n3, r2, r3 = bc
    rng = np.random.default_rng(100 + ne0 + ne1)
    x = rng.uniform(-4, 4, size=(n3 * r3, n2 * r2, ne1, ne0)).astype(np.float32)
    ne1p = (ne1 + 63) // 64 * 64
    m = rng.uniform(-1, 0, size=(n3, n2, ne1p, ne0)).astype(np.float32)
    m[..., ne0 // 2:] = -np.inf
    m[..., 0] = 0
    m = ec.quant(mask_t, m).astype(np.float32)
    sk = rng.uniform(-1, 1, size=n2 * r2).astype(np.float32)
    with H() as h:
        a = h.new(F32, (ne0, ne1, n2 * r2, n3 * r3), x); mt = h.new(mask_t, (ne0, ne1p, n2, n3), ec.enc(mask_t, m))
        s = h.new(F32, (n2 * r2,), sk.reshape(1, 1, 1, -1)) if sinks else None

        def make():
            o = L.ggml_soft_max_ext(h.c, a, mt, 0.1, max_bias)
            if sinks:
                L.ggml_soft_max_add_sinks(o, s)
            return o
        o = bracket(h, make)
        h.go(o); got = gg.tensor_get(o)
    exp = ref.soft_max(x, m, np.float32(0.1), max_bias, sk if sinks else None)
    assert np.isfinite(got).all() and ec.nmse(exp, got) <= 1e-6, ec.nmse(exp, got)


# ---- RMS_NORM (+ MUL (+ ADD)) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne0", [10, 64, 288, 1031])
@pytest.mark.parametrize("chain", ["norm", "mul-w_ne0", "mul-w_ne0xne1", "mul-w_1", "mul-w_ne0-add_ne0", "mul-w_ne0-add_full", "mul-w_ne0xne1-add_ne0",
                                   "mul-w_ne0xne1-add_full", "mul-w_1-add_ne0", "mul-w_1-add_full"])
def test_rms_norm_view_and_weight_shapes(ne0, chain):
    """x as the view form (strided rows that start 4 bytes off alignment: the scalar loops of k_rms_norm), the weight of every repeatable
    shape ([ne0], [ne0, ne1], [1]: the `wrap` path), the addend a row or full; against float64 and, fused against node by node, bit for bit
    (tests/test-backend-ops.cpp:2856 test_rms_norm_mul_add)"""
    ne = (ne0, 5, 3, 2)
    rng = np.random.default_rng(110 + ne0)
    x = rng.uniform(-1, 1, size=ne[::-1]).astype(np.float32)
    parts = chain.split("-")
    wne = {"w_ne0": (ne0,), "w_ne0xne1": (ne0, 5), "w_1": (1,)}.get(parts[1]) if len(parts) > 1 else None
    ane = {"add_ne0": (ne0,), "add_full": ne}.get(parts[2]) if len(parts) > 2 else None
    full = lambda n: tuple(list(n) + [1] * (4 - len(n)))[::-1]
    w = rng.uniform(0.5, 1.5, size=full(wne)).astype(np.float32) if wne else None
    ad = rng.uniform(-1, 1, size=full(ane)).astype(np.float32) if ane else None
    be = backend()
    try:
        for eps in (0.0, 1e-6, 0.1):
            outs = {}
            for fusion in (1, 0):
                be.set_option("fusion", fusion)
                with H() as h:
                    a = h.src(F32, x, True)
                    wt = h.new(F32, wne, w) if wne else None
                    at = h.new(F32, ane, ad) if ane else None

                    def make():
                        o = L.ggml_rms_norm(h.c, a, eps)
                        if wt:
                            o = L.ggml_mul(h.c, o, wt)
                        if at:
                            o = L.ggml_add(h.c, o, at)
                        return o
                    o = bracket(h, make)
                    h.go(o); outs[fusion] = gg.tensor_get(o).copy()
            exp = ref.rms_norm(x, np.float32(eps))
            if wne:
                exp = exp * ref.bcast(w.astype(np.float64), x.shape)
            if ane:
                exp = exp + ref.bcast(ad.astype(np.float64), x.shape)
            assert ec.nmse(exp, outs[1]) <= 1e-7 and ec.nmse(exp, outs[0]) <= 1e-7, (eps, ec.nmse(exp, outs[1]), ec.nmse(exp, outs[0]))
            assert np.array_equal(outs[0], outs[1]), eps
    finally:
        be.set_option("fusion", 1)


# ---- ROPE --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ec.ROPE_CASES, ids=ec.rope_id)
def test_rope(c):
    """tests/test-backend-ops.cpp:5975-6005: F16 and F32, NORM and NEOX, head 80 with n_dims 20 / 32 / 80 (a pass-through tail), 128 / 128, 64 / 64;
    frequency factors; YaRN (ext_factor 1, freq_scale 0.5, attn_factor 1.4245); contiguous, and as one slice of a fused QKV row
    (nb1 = head size, nb2 = three projections, a non-zero offset)"""
    t, mode, (hd, nd), (with_ff, ext, af), lay = c
    x, pos, ff = ec.rope_inputs(c)
    nh, ntok = ec.ROPE_NHEAD, ec.ROPE_NTOK
    es = ec.ESIZE[t]
    xs = ec.enc(t, x)
    with H() as h:
        if lay == "cont":
            a = h.new(t, (hd, nh, ntok), xs)
        else:
            row = ec.enc(t, np.random.default_rng(7).uniform(50, 100, size=(1, 1, ntok, 3 * hd * nh)).astype(np.float32))
            row[0, 0, :, hd * nh:2 * hd * nh] = xs.reshape(ntok, nh * hd)
            par = h.new(t, (3 * hd * nh, ntok), row)
            a = L.ggml_view_3d(h.c, par, hd, nh, ntok, hd * es, 3 * hd * nh * es, hd * nh * es)
        p = h.new(I32, (ntok,), pos.reshape(1, 1, 1, -1))
        f = h.new(F32, (nd // 2,), ff.reshape(1, 1, 1, -1)) if with_ff else None
        o = bracket(h, lambda: L.ggml_rope_ext(h.c, a, p, f, nd, mode, 8192, 500000.0, 0.5 if ext else 1.0, ext, af, 32.0, 1.0))
        h.go(o); got = gg.tensor_get(o)
    exp = ec.rope_eval(c, x, pos, ff)
    if t == F32:
        assert ec.nmse(exp, got) <= 1e-6 and np.abs(exp - got).max() <= 1e-3, (ec.nmse(exp, got), np.abs(exp - got).max())
    else:
        ec.assert_half(t, got, exp, ec.rope_id(c))


# ---- SCALE, SUM_ROWS, ADD_ID on strided sources ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ne", ec.SHAPES, ids=str)
@pytest.mark.parametrize("view", [False, True], ids=["cont", "view"])
def test_scale(ne, view):
    rng = np.random.default_rng(120)
    x = rng.uniform(-2, 2, size=ne[::-1]).astype(np.float32)
    with H() as h:
        a = h.src(F32, x, view)
        o = bracket(h, lambda: L.ggml_scale(h.c, a, 0.37))
        ob = bracket(h, lambda: L.ggml_scale_bias(h.c, a, 0.37, -1.5))
        h.go(o, ob); got = gg.tensor_get(o); gotb = gg.tensor_get(ob)
    s = np.float64(np.float32(0.37))
    ec.assert_f32_1ulp(got, x.astype(np.float64) * s)                 # one multiplication
    assert ec.nmse(x.astype(np.float64) * s - 1.5, gotb) <= 1e-7      # two roundings: the NMSE gate


@pytest.mark.parametrize("ne0", [1, 63, 64, 65, 1000])
def test_sum_rows_view(ne0):
    rng = np.random.default_rng(121 + ne0)
    x = rng.uniform(-2, 2, size=(2, 3, 5, ne0)).astype(np.float32)
    with H() as h:
        a = h.src(F32, x, True)
        o = bracket(h, lambda: L.ggml_sum_rows(h.c, a))
        h.go(o); got = gg.tensor_get(o)
    assert got.shape == (2, 3, 5, 1) and ec.nmse(x.astype(np.float64).sum(-1, keepdims=True), got) <= 1e-7


@pytest.mark.parametrize("ne0", [65, 128])
def test_add_id_view(ne0):
    """tests/test-backend-ops.cpp:2548 with `a` the view form"""
    rng = np.random.default_rng(122)
    n_expert, n_used, ntok = 8, 3, 5
    a_ = rng.uniform(-1, 1, size=(1, ntok, n_used, ne0)).astype(np.float32)
    bias = rng.uniform(-1, 1, size=(1, 1, n_expert, ne0)).astype(np.float32)
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(ntok)]).astype(np.int32)
    with H() as h:
        a = h.src(F32, a_, True); b = h.new(F32, (ne0, n_expert), bias); i = h.new(I32, (n_used, ntok), ids.reshape(1, 1, ntok, n_used))
        o = bracket(h, lambda: L.ggml_add_id(h.c, a, b, i))
        h.go(o); got = gg.tensor_get(o)
    ec.assert_f32_1ulp(got[0], ref.add_id(a_[0], bias[0, 0], ids))      # one addition per element


# ---- what supports_op must refuse --------------------------------------------------------------------------------------------------
def test_refusals():
    with H() as h:
        a = h.new(F32, (64, 2, 3)); p = h.new(I32, (3,))
        for mode in (gg.GGML_ROPE_TYPE_MROPE, gg.GGML_ROPE_TYPE_VISION):
            assert refused(L.ggml_rope_ext(h.c, a, p, None, 64, mode, 8192, 10000.0, 1.0, 0.0, 1.0, 32.0, 1.0)), "ROPE mrope / vision"
        assert refused(L.ggml_cpy(h.c, a, h.new(I32, (64, 2, 3)))), "CPY F32 -> I32"
        assert refused(L.ggml_argsort(h.c, h.new(F32, (1025, 2)), gg.GGML_SORT_ORDER_DESC)), "ARGSORT over 1025 columns"
        assert not refused(L.ggml_argsort(h.c, h.new(F32, (1024, 2)), gg.GGML_SORT_ORDER_DESC))
        q = L.ggml_set_rows(h.c, h.new(gg.Q8_0, (33, 4)), h.new(F32, (33, 2)), h.new(I64, (2,)))
        assert refused(q), "SET_ROWS into Q8_0 rows that are no whole blocks"
        g = L.ggml_get_rows(h.c, h.new(F32, (64, 5)), h.new(I32, (4,)))
        assert not refused(g)
        g.contents.src[1] = h.new(F16, (4,))          # (the constructor itself insists on I32 indices)
        assert refused(g), "GET_ROWS with F16 indices"
