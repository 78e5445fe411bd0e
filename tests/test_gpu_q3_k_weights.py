"""GPU parity for Q3_K weights — the default type of every Q3_K_S / _M / _L file (src/llama-quant.cpp:553-555: wq, wk, ffn_gate, ffn_up, Mixtral's
expert stacks) — in MUL_MAT and MUL_MAT_ID: the parameter lines. The case bodies, the reference and the gates are tests/gpu_weight_format_cases.py's.

  k = 256 (one block), 768 (three: an odd count, a wave's tail, row starts alternating between 4-byte aligned and 2 off), 1024 (four streamed
  units), 1280 (five)
"""
import pytest

import gpu_weight_format_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("m", [1, 33, 130])
@pytest.mark.parametrize("k", [256, 768, 1024, 1280])
def test_mul_mat(k, m):
    cases.check_mul_mat("q3_K", k, m)


@pytest.mark.parametrize("k,m", [(4096, 300), (14336, 4096)])
def test_mul_mat_one_column_at_model_row_lengths(k, m):
    cases.check_mul_mat_one_column_at_model_row_lengths("q3_K", k, m)


def test_one_column_runs_on_the_streamed_kernel():
    cases.check_one_column_runs_on_the_streamed_kernel("q3_K", (1024,))


@pytest.mark.parametrize("n", [1, 3, 40])
def test_mul_mat_f16_src1(n):
    cases.check_mul_mat_f16_src1("q3_K", 768, n)


@pytest.mark.parametrize("n", [1, 3])
def test_mul_mat_broadcast(n):
    cases.check_mul_mat_broadcast("q3_K", 768, n)


@pytest.mark.parametrize("k,n", [(1024, 1), (768, 4), (768, 40)])
def test_mul_mat_twice_is_bitwise_equal(k, n):
    cases.check_mul_mat_twice_is_bitwise_equal("q3_K", k, n)


@pytest.mark.parametrize("n_tokens", [1, 3, 35])
@pytest.mark.parametrize("k", [768, 1024])
def test_mul_mat_id(k, n_tokens):
    cases.check_mul_mat_id("q3_K", k, n_tokens)


@pytest.mark.parametrize("T", [1, 4, 40])
@pytest.mark.parametrize("down", ["q3_K", "q4_K"])
@pytest.mark.parametrize("n_embd,n_ff", [(256, 768), (1024, 2048)])
def test_ffn_subgraph_fused_and_unfused(n_embd, n_ff, down, T):
    """gate / up Q3_K, down Q3_K or Q4_K (the Q3_K_M mix), the whole-graph gate: the case's docstring says why and has the measured values"""
    cases.check_ffn_subgraph_fused_and_unfused("q3_K", down, n_embd, n_ff, cases.GRAPH_GATE, T)


@pytest.mark.parametrize("k", [768, 1024])
@pytest.mark.parametrize("third", ["q3_K", "q4_K", "q5_K", "q6_K"])
def test_mat_vecs_on_one_normed_activation(third, k):
    """wq and wk in Q3_K; wv in Q4_K / Q5_K shares ONE grouped streamed launch with them, asserted through the profile at k = 1024"""
    one_launch = ("q3_K", third) if k == 1024 and third in ("q4_K", "q5_K") else None
    cases.check_mat_vecs_on_one_normed_activation(("q3_K", "q3_K", third), k, k + sum(map(ord, third)), one_launch)


def test_refusals():
    cases.check_refusals()
