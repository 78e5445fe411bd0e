"""No-GPU pin of the host code's answers about weight formats, read through the product library's diagnostic export
mi355x_weight_format_info (csrc/mmvq_fused.hip): which types MUL_MAT(_ID) takes, their activation format and block geometry, which have a
register-ring kernel, and which pairs may share a grouped mat-vec launch. The library loads without a device (as in tests/test_abi.py); no
compute call is made. The expected values are spelled out here, not derived from the package: they are what the list in csrc/blocks.h and
the two pair tables have to keep saying."""
import ctypes as C

import graft_pkg

gg = graft_pkg.load().ggml

SUPPORTED = {2, 6, 7, 8, 11, 12, 13, 14, 39}          # enum ggml_type: Q4_0, Q5_0, Q5_1, Q8_0, Q3_K, Q4_K, Q5_K, Q6_K, MXFP4
Q8_0, Q8_K = 8, 15
ACT = {2: Q8_0, 6: Q8_0, 7: Q8_0, 8: Q8_0, 39: Q8_0, 11: Q8_K, 12: Q8_K, 13: Q8_K, 14: Q8_K}
RING = {2, 8, 12, 13, 14, 39}
GROUP_PAIRS = {frozenset(p) for p in ((12, 13), (12, 14), (13, 14), (11, 12), (11, 13))}
MIXED_PAIRS = {frozenset((8, 12))}


def info(a, b=None):
    f = gg.backend_cdll().mi355x_weight_format_info
    f.restype = None; f.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int*7)(*([-99]*7))
    f(a, a if b is None else b, out)
    return dict(zip(("supported", "act", "elements", "bytes", "ring", "can_group", "can_group_mixed"), out))


def test_supported_types_and_their_activation_kind():
    for t in range(41):
        r = info(t)
        assert r["supported"] == (1 if t in SUPPORTED else 0), t
        assert r["act"] == ACT.get(t, -1), t


def test_block_geometry_matches_the_package_constants():
    for t in sorted(SUPPORTED):
        r = info(t)
        assert (r["elements"], r["bytes"]) == gg.QUANT_SIZES[t], t


def test_register_ring_formats():
    assert {t for t in range(41) if info(t)["ring"]} == RING


def test_pairs_that_may_share_a_grouped_launch():
    for a in sorted(SUPPORTED):
        for b in sorted(SUPPORTED):
            r = info(a, b)
            assert r["can_group"] == (1 if a == b or frozenset((a, b)) in GROUP_PAIRS else 0), (a, b)
            assert r["can_group_mixed"] == (1 if frozenset((a, b)) in MIXED_PAIRS else 0), (a, b)
