"""No-GPU pin of what the host code decides about the prompt pass's quantized mat-mul launches, read through the product library's diagnostic export
mi355x_prefill_plan_info (csrc/mmq.hip): tile size, k split, grid and kernel of a one-tensor launch; whether the grouped wq / wk / wv launch takes a call with bias
rows, rotations or KV-cache stores riding on it (mul_mat_q_multi_takes); whether gate / up / SwiGLU runs as one kernel; and the expert chain's dual launch, tile
sizes and scratch bytes (mul_mat_q_id_plan). The library loads without a device (as in tests/test_abi.py); no compute call is made. The rows are the shapes the GPU
tests of these launch forms use (tests/test_gpu_ops.py) and the model shapes the plan functions' comments name. The expected values were recorded from the commit
before the launchers took call records, through the same export on top of its plan functions and the old launcher's early returns, with no GGML_MI355X_* variable
set: they are the defaults (16-wave kernel on, no forced tile, no forced dual launch), and this file is what keeps a change of the host code from moving them."""
import ctypes as C
import os

import graft_pkg

gg = graft_pkg.load().ggml

Q4_0, Q8_0, Q4_K, Q5_K, Q6_K, MXFP4 = 2, 8, 12, 13, 14, 39          # enum ggml_type
BIG = 1 << 40
NO = (0, 0, 0, 0, 0, 0)


def info(form, args, nout):
    assert not [v for v in ("MMQ16", "WIDE4_MINK", "MOE_TILE", "MOE_DUAL") if "GGML_MI355X_" + v in os.environ], "the table pins the defaults of the switches the plans read"
    f = gg.backend_cdll().mi355x_prefill_plan_info
    f.restype = None; f.argtypes = [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    out = (C.c_int64*8)(*([-99]*8))
    f(form, (C.c_int64*16)(*args), out)
    return tuple(out[:nout])


# (m, k, n, vec_ok) -> (ok, tile, ksplit, grid.x, grid.y, 16-wave kernel)
ONE = [
    ((1024, 2048, 512, 1), (1, 128, 2, 4, 16, 0)),        # test_prefill_mul_mat_residual_fused: k split in two
    ((300, 512, 100, 1), (1, 128, 1, 1, 3, 0)),           # ... ragged tiles, no split
    ((10240, 288, 512, 1), (1, 256, 1, 2, 80, 1)),        # ... 256-token tiles
    ((5120, 8192, 300, 1), (1, 256, 4, 2, 160, 1)),       # ... k split in four
    ((1026, 2880, 64, 0), (1, 128, 1, 1, 9, 0)),          # ... m % 4 != 0
    ((1028, 2048, 257, 1), (1, 128, 2, 3, 18, 0)),
    ((4096, 4096, 512, 1), (1, 256, 4, 2, 128, 1)),       # wo at 512 tokens: 64 tiles, k in four parts
    ((14336, 4096, 512, 1), (1, 256, 1, 2, 112, 1)),      # ffn_up: 224 tiles fill the chip
    ((4096, 14336, 512, 1), (1, 256, 4, 2, 128, 1)),      # ffn_down
    ((4096, 2880, 512, 1), (1, 128, 1, 4, 32, 0)),        # gpt-oss's k = 2880 does not split
    ((4096, 4096, 512, 0), (1, 128, 1, 4, 32, 0)),        # rows that cannot be combined 16 bytes at a time: no split
]

# (types, ms, k, n, what rides) -> (takes, tile, ksplit, grid.x, grid.y, 16-wave kernel). hd: the rotation on segments 0 and 1; kv: a row and an element store on the
# last two segments; bias: a bias row on segment 0
QKV = (4096, 512, 512)
LLAMA = ((Q4_K, Q4_K, Q6_K), (4096, 1024, 1024), 4096, 512)
GPT_OSS = ((MXFP4, MXFP4, MXFP4), (14336, 4096, 4096), 2880, 256)
MULTI = [
    (*LLAMA, dict(hd=128), (1, 256, 2, 2, 96, 1)),                                              # test_prefill_qkv_group, with its ROPEs riding and plain
    (*LLAMA, {}, (1, 256, 2, 2, 96, 1)),
    ((Q4_K, Q4_K, Q4_K), (2048, 512, 512), 4096, 300, dict(hd=64), (1, 256, 4, 2, 96, 1)),
    ((Q4_K, Q4_K, Q4_K), (2048, 512, 512), 4096, 300, {}, (1, 256, 4, 2, 96, 1)),
    ((Q6_K, Q5_K, Q5_K), (7000, 7000, 7200), 256, 257, dict(hd=8), NO),                        # no k split: the rotation does not ride
    ((Q6_K, Q5_K, Q5_K), (7000, 7000, 7200), 256, 257, {}, (1, 256, 1, 2, 167, 1)),
    ((Q8_0, Q8_0), (2048, 2048), 2048, 1000, dict(hd=64), (1, 256, 2, 4, 64, 1)),
    ((Q8_0, Q8_0), (2048, 2048), 2048, 1000, {}, (1, 256, 2, 4, 64, 1)),
    (*GPT_OSS, dict(hd=64), NO),                                                                # rope flips takes
    (*GPT_OSS, {}, (1, 256, 1, 1, 176, 1)),
    ((Q4_0, Q4_K, Q4_0), (4096, 1024, 1024), 1024, 512, dict(hd=64), NO),                      # a type mix without a kernel
    ((Q4_0, Q4_K, Q4_0), (4096, 1024, 1024), 1024, 512, {}, NO),
    ((Q8_0, Q8_0, Q8_0), QKV, 320, 512, dict(bias=1), (1, 256, 1, 2, 40, 1)),                   # test_prompt_pass_qkv_with_bias_rows
    ((Q4_K, Q4_K, Q4_K), QKV, 512, 512, dict(bias=1), (1, 256, 1, 2, 40, 1)),
    ((Q4_K, Q4_K, Q4_K), QKV, 2048, 512, dict(bias=1), NO),                                     # ... on a k that splits: bias flips takes
    ((Q4_K, Q4_K, Q4_K), QKV, 2048, 512, {}, (1, 256, 2, 2, 80, 1)),
    (*LLAMA, dict(hd=128, kv=1), (1, 256, 2, 2, 96, 1)),                                        # the KV-cache stores ride on the combine pass
    (*LLAMA, dict(hd=128, kv=1, scratch=16 << 20), NO),                                         # ... the scratch too small for two planes
    (*LLAMA, dict(vec_ok=0), (1, 256, 1, 2, 48, 1)),
    (*LLAMA, dict(hd=96), NO),                                                                  # rows that are no whole heads
    (*GPT_OSS, dict(kv=1), NO),                                                                 # kv flips takes
    (*GPT_OSS, dict(bias=1), (1, 256, 1, 1, 176, 1)),
    ((Q4_K,), (4096,), 4096, 512, {}, NO),                                                      # one segment is no group
]

# (m, n) -> ok: test_prefill_gate_up_glu_fused's shapes, ffn_up of Llama-3-8B, wo's rows, a short batch
GLU = [((10240, 512), 1), ((10300, 300), 1), ((20500, 257), 1), ((10240, 300), 1), ((5200, 1000), 1), ((10250, 512), 1), ((14336, 512), 1), ((4096, 512), 0), ((14336, 128), 0)]

# (k, n_tokens, n_used, n_expert, m, option moe_dual) -> (dual, gate / up tile, down tile, scratch bytes)
MOE = [
    ((512, 512, 2, 8, 256, -1), (0, 128, 128, 1065728)),          # test_moe_expert_chain_many_tokens: ~128 pairs per expert, two launches
    ((320, 300, 2, 4, 320, -1), (0, 128, 128, 722176)),
    ((512, 300, 2, 8, 256, -1), (1, 256, 256, 845056)),           # ... fewer pairs per expert: the dual launch
    ((256, 150, 2, 8, 256, -1), (1, 256, 256, 292096)),
    ((320, 130, 4, 32, 320, -1), (1, 256, 256, 507136)),
    ((256, 70, 2, 8, 128, -1), (1, 256, 256, 172800)),
    ((256, 40, 2, 4, 256, -1), (1, 256, 256, 177408)),
    ((4096, 512, 2, 8, 14336, -1), (0, 128, 128, 33628928)),      # Mixtral at 512 tokens: 128 pairs per expert
    ((2880, 512, 4, 32, 2880, -1), (1, 256, 256, 14809856)),      # gpt-oss at 512 tokens: 64 pairs per expert
    ((4096, 512, 2, 8, 14336, 1), (1, 256, 128, 33628928)),       # the option forces the dual launch: the down launch sorts again for its own tiles
    ((2880, 512, 4, 32, 2880, 0), (0, 256, 256, 14809856)),       # ... and two launches
]


def multi(types, ms, k, n, vec_ok=1, hd=0, kv=0, bias=0, scratch=BIG):
    pad = lambda v: list(v) + [0]*(3 - len(v))
    return info(1, [len(types)] + pad(types) + pad(ms) + [k, n, vec_ok, hd, kv, bias, scratch], 6)


def test_one_tensor_launch_plan():
    for args, exp in ONE:
        assert info(0, args, 6) == exp, args


def test_grouped_launch_takes_and_plan():
    for types, ms, k, n, rides, exp in MULTI:
        assert multi(types, ms, k, n, **rides) == exp, (types, ms, k, n, rides)


def test_gate_up_glu_supported():
    for args, exp in GLU:
        assert info(2, args, 1) == (exp,), args


def test_expert_chain_plan():
    for args, exp in MOE:
        assert info(3, args, 5) == (1,) + exp, args
