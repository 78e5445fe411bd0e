"""GPU parity for Q5_0 / Q5_1 weights — the 32-element formats llama_tensor_get_type writes in place of Q4_K / Q5_K when a row is
not a multiple of 256 long (src/llama-quant.cpp:436-470) — in MUL_MAT and MUL_MAT_ID: the parameter lines. The case bodies, the reference
and the gates are tests/gpu_weight_format_cases.py's.

  k = 32 (one block), 288 (nine blocks: k % 256 != 0, odd block count, a wave's tail), 1024 (four streamed units), 1280 (five: odd)
"""
import pytest

import gpu_weight_format_cases as cases

pytestmark = pytest.mark.gpu
NAMES = ["q5_0", "q5_1"]


@pytest.mark.parametrize("m", [1, 33, 130])
@pytest.mark.parametrize("k", [32, 288, 1024, 1280])
@pytest.mark.parametrize("name", NAMES)
def test_mul_mat(name, k, m):
    cases.check_mul_mat(name, k, m)


@pytest.mark.parametrize("k,m", [(4096, 300), (14336, 4096)])
@pytest.mark.parametrize("name", NAMES)
def test_mul_mat_one_column_at_model_row_lengths(name, k, m):
    cases.check_mul_mat_one_column_at_model_row_lengths(name, k, m)


@pytest.mark.parametrize("name", NAMES)
def test_one_column_runs_on_the_streamed_kernel(name):
    cases.check_one_column_runs_on_the_streamed_kernel(name, (1024, 288))


@pytest.mark.parametrize("n", [1, 3, 40])
@pytest.mark.parametrize("name", NAMES)
def test_mul_mat_f16_src1(name, n):
    cases.check_mul_mat_f16_src1(name, 288, n)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_mul_mat_broadcast(name, n):
    cases.check_mul_mat_broadcast(name, 288, n)


@pytest.mark.parametrize("k,n", [(1024, 1), (288, 4), (288, 40)])
@pytest.mark.parametrize("name", NAMES)
def test_mul_mat_twice_is_bitwise_equal(name, k, n):
    cases.check_mul_mat_twice_is_bitwise_equal(name, k, n)


@pytest.mark.parametrize("n_tokens", [1, 3, 35])
@pytest.mark.parametrize("k", [288, 1024])
@pytest.mark.parametrize("name", NAMES)
def test_mul_mat_id(name, k, n_tokens):
    cases.check_mul_mat_id(name, k, n_tokens)


@pytest.mark.parametrize("T", [1, 4, 40])
@pytest.mark.parametrize("n_embd,n_ff", [(288, 768), (1024, 2048)])
def test_ffn_subgraph_fused_and_unfused(n_embd, n_ff, T):
    """gate / up Q5_0, down Q5_1, the one-mat-mul gate"""
    cases.check_ffn_subgraph_fused_and_unfused("q5_0", "q5_1", n_embd, n_ff, cases.GATE, T)


@pytest.mark.parametrize("k", [288, 1024])
@pytest.mark.parametrize("types", [("q5_0", "q5_0", "q5_0"), ("q5_1", "q5_1", "q5_1"), ("q5_0", "q5_1", "q5_0")])
def test_mat_vecs_on_one_normed_activation(types, k):
    """same-format neighbours share one grouped launch (streamed at k % 256 == 0); a Q5_0 / Q5_1 pair, which has no common kernel, splits it"""
    cases.check_mat_vecs_on_one_normed_activation(types, k, k + len(set(types)), None)


@pytest.mark.parametrize("type_id,tname", [(3, "Q4_1"), (20, "IQ4_NL")])
def test_other_32_element_formats_are_still_refused(type_id, tname):
    cases.check_other_32_element_formats_are_still_refused(type_id, tname)
