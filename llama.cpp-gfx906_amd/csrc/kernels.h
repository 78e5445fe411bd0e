// kernels.h — host-callable launchers for the gfx950 kernels. Plain pointers,
// strides in BYTES (ggml nb[] convention) and a hipStream_t; no ggml types, so the
// kernels can be driven from backend*.cpp (ggml tensors) or from the flat C-ABI in
// include/ggml-mi355x.h. Every launcher is asynchronous on `stream` and performs
// no allocation or synchronisation (safe under hipGraph capture). A launcher has put
// all its kernels on the stream when it returns and keeps nothing from one call to
// the next: what a caller wants back (a kernel's name, its timing) goes through the
// call's arguments. Run-time switches are read through env_switch.h.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "blocks.h"
#include "env_switch.h"

namespace mi355x {

// ggml_type ids used on the path (gguf-py/gguf/constants.py:2698-2730); the weight formats' ids and T_Q8_K come from the list in blocks.h
enum : int { T_F32 = 0, T_F16 = 1, T_I32 = 26, T_I64 = 27, T_BF16 = 30 };

// ---- activation quantisation (the CPU path's vec_dot_type, the list's last column: Q8_0 for the 32-element formats, Q8_K for the K-quants)
// Device layout (SoA, internal): for a [k, n] activation
//   qs    : int8  [n][k]
//   d     : float [n][k/32]   (Q8_0: value of the f16-rounded scale)  | float [n][k/256] (Q8_K)
//   bsums : int16 [n][k/32]   (Q8_0: sum of the 32 quants)            | int16 [n][k/16]  (Q8_K)
struct act_q8 {
    int8_t  * qs;
    float   * d;
    int16_t * bsums;
    int       kind;   // T_Q8_0 or T_Q8_K
    int64_t   k;
    int64_t   n;
};

size_t act_q8_bytes(int kind, int64_t k, int64_t n);            // scratch bytes needed
act_q8 act_q8_carve(void * scratch, int kind, int64_t k, int64_t n);
int    act_kind_for(int type_a);                                   // T_Q8_0 / T_Q8_K / -1: the list's activation format

// x: f32, rows of k contiguous floats; row r (< q.n) lives at
//   x + (r % n_inner)*stride_inner + (r / n_inner)*stride_outer      (bytes)
// (n_inner = q.n, stride_outer = 0 for a plain 2-D activation; the two-level form serves MUL_MAT_ID's [k, n_b, n_tokens] src1)
void quantize_act(const float * x, int64_t n_inner, size_t stride_inner, size_t stride_outer, const act_q8 & q, hipStream_t stream);

// ---- quantized mat-vec (decode, n <= MMVQ_MAX_N): dst[col*dst_stride + row] = W[row,:] . x[col,:]
constexpr int MMVQ_MAX_N = 8;
bool mul_mat_vec_q_supported(int type_a);      // = the type is in the list (blocks.h)
void mul_mat_vec_q(int type_a, const void * W, size_t w_row_stride, int64_t m, int64_t k,
                   const act_q8 & act, int64_t n, float * dst, size_t dst_col_stride_bytes, hipStream_t stream);

void mul_mat_vec_q_batched(int type_a, const void * W, size_t w_row_stride, size_t w_batch_stride, int r2, int64_t m, int64_t k,
                           const act_q8 & act, int64_t n, int64_t n_batch, float * dst, size_t dst_col_stride_bytes, size_t dst_batch_stride_bytes, hipStream_t stream);

// 2 <= n <= 8 columns of Q4_K / Q5_K / Q6_K on the streamed weight path (mmvq_stream_cols.hip: LDS-DMA ring, every unit multiplied with all columns);
// false = not taken (k % 2048, the column images + two slots must fit LDS)
bool mul_mat_vec_q_stream_cols(int type_a, const void * W, size_t w_row_stride, int64_t m, int64_t k,
                               const act_q8 & act, int64_t n, float * dst, size_t dst_col_stride_bytes, hipStream_t stream);
// 2 <= n <= 8 columns of Q4_K / Q5_K / Q6_K on the int8 matrix cores; false = not taken (the caller runs its own kernel)
bool mul_mat_vec_q_cols_mfma(int type_a, const void * W, size_t w_row_stride, int64_t m, int64_t k,
                             const act_q8 & act, int64_t n, float * dst, size_t dst_col_stride_bytes, hipStream_t stream);

// MUL_MAT_ID decode form: for pair p (< n_pairs): dst[p*dst_stride + :] = W[expert[p]] . act row (p % act rows as given by act_row[p])
void mul_mat_vec_q_id(int type_a, const void * W, size_t w_row_stride, size_t w_expert_stride, int64_t m, int64_t k,
                      const act_q8 & act, const int32_t * ids, size_t ids_nb0, size_t ids_nb1,
                      int64_t n_used, int64_t n_tokens, int64_t n_b,
                      float * dst, size_t dst_nb1, size_t dst_nb2, hipStream_t stream);

// ---- the rotary embedding's descriptors: ROPE's op_params, and what a mat-mul launch that applies the rotation carries (the grouped mat-vec's EPI_ROPE, the grouped prefill launch) ----
struct rope_params {
    int n_dims, mode, n_ctx_orig;
    float freq_base, freq_scale, ext_factor, attn_factor, beta_fast, beta_slow;
};
// table (the grouped mat-vec only): n_dims/2 x (cos, sin) for the token at pos[0], filled by mul_mat_vec_q_fused_rope_table on the same stream before the launch
// (one tiny launch per token and rope configuration instead of powf / cosf / sinf per row pair inside every norm+QKV launch)
struct mmvq_rope { const int32_t * pos; const float * freq_factors; int head_dim; rope_params p; const float * table; };
// ---- quantized mat-mat (prefill, n > MMVQ_MAX_N): dequantize-to-bf16 tiles in LDS + v_mfma_f32_32x32x16_bf16 ----
// Every launcher takes ONE named record (value-initialise, fill by name, as attn_call), asks a pure plan function (mmq.hip: mmq_plan_one / _multi / _glu: tile size, k split, grid,
// 16-wave kernel or not) and mul_mat_q_layout for where things sit in the scratch, then only sets pointers and launches. The scratch of one launch: the bf16 copy of x in [0, x_end), n_planes split-k planes (dense [n][m] f32 each) from planes_off; total includes the slack
// behind them. A producer kernel that writes the next mat-mul's copy while this one's is still read puts it at x_end as well.
struct mmq_layout { size_t x_end, planes_off, planes_bytes, total; };
mmq_layout mul_mat_q_layout(int64_t k, int64_t n, int64_t m, int n_planes = 4);
size_t mul_mat_q_scratch_bytes(int64_t k, int64_t n, int64_t m);     // = layout(k, n, m).total
size_t mul_mat_q_x_bytes(int64_t k, int64_t n);      // size of the bf16 activation copy at the start of the scratch (= layout(k, n, 0).x_end)
// the activations of a prefill launch, shared by the three forms below. x: f32 rows of k floats at x + i*x_row_stride, n of them; scratch: scratch_size bytes, at least mul_mat_q_scratch_bytes(k, n, m)
// (only the grouped launch's question reads the size); scratch_ready: it already holds the copy of exactly this x — the caller's cache — so the conversion pass is skipped
struct mmq_act { const float * x; size_t x_row_stride; int64_t k, n; void * scratch; size_t scratch_size; bool scratch_ready; };
// defer != NULL: when the launch splits k, the pass that adds the planes (and res) is left to the caller (who fuses it with the norm that
// follows): np = number of planes (0: nothing deferred, dst is complete), planes = dense [np][n][m] f32 in the scratch, planes_off bytes behind `scratch`
struct mmq_deferred { int np; const float * planes; size_t planes_off; };
// mul_mat_q: dst[i*dst_stride + row] = W[row,:] . x[i,:], strides in bytes; res != NULL: dst = W.x + res (f32 rows of m floats at res + i*res_stride; may be dst itself) — the residual
// ADD of build_attn / build_ffn. mul_mat_q_glu (no res, no defer): gate / up + SwiGLU in one kernel, dst[n][m] = silu(W.x) * (W2.x), both weight tensors of one type and shape;
// y16 != NULL (m % 64 == 0): the result also (dst == NULL: only) as the bf16 activation copy of the mat-mul that follows (ffn_down), rows of m elements
struct mmq_call { int type; const void * W; size_t w_row_stride; int64_t m; mmq_act act; float * dst; size_t dst_stride; const float * res; size_t res_stride;
                  mmq_deferred * defer; hipStream_t stream; const void * W2; uint16_t * y16; };      // W2, y16: the GLU form only
void mul_mat_q(const mmq_call & c);
bool mul_mat_q_glu_supported(int64_t m, int64_t n);      // the 256-token tiles fill the chip
void mul_mat_q_glu(const mmq_call & c);

// 2 or 3 mat-muls on the same activations (wq / wk / wv) as one launch of 256-token tiles. Per segment: bias != NULL: m floats added to every row (only without a k
// split); rope: the NORM rotary embedding `rope` on the segment's rows of heads; st_*: the KV-cache write done by the pass that combines the launch's split-k planes:
// st_mode 0 none | 1 f16 rows st16[st_idx[token]*st_row_elems + col] | 2 element scatter st16[st_idx[token*m + col]] (the transposed V cache)
struct mmq_multi_seg { int type; const void * W; size_t w_row_stride; int64_t m; float * dst; size_t dst_stride; const float * bias; bool rope;
                       uint16_t * st16; const int64_t * st_idx; int64_t st_row_elems; int st_mode; };
struct mmq_multi_call { int nseg; mmq_multi_seg seg[3]; mmq_act act; mmvq_rope rope; hipStream_t stream; };
// does the grouped launch take this call? Pure: from shapes, types, flags, pointer alignment and the scratch size; no pointer's target is read, nothing is launched. false: too few
// tiles, an unsupported mix of types or rope shape, a rider that the k split (or its absence) rules out, scratch too small. mul_mat_q_multi only launches: a call it does not take aborts.
bool mul_mat_q_multi_takes(const mmq_multi_call & c);
void mul_mat_q_multi(const mmq_multi_call & c);

// ---- MUL_MAT_ID for many tokens (src/llama-graph.cpp:569-595): (token, slot) pairs sorted by expert on the device, then the tiled
// MFMA kernel per (expert, 128 pairs). b: f32 [k, n_b, n_tokens] (n_b = 1 or n_used); ids: i32 [n_used, n_tokens] (strided);
// dst: f32 [m, n_used, n_tokens]. No host round trip, so the launch sequence can be captured in a hipGraph.
bool   mul_mat_q_id_supported(int64_t n_expert, int64_t n_used, int64_t n_tokens);
size_t mul_mat_q_id_scratch_bytes(int64_t k, int64_t n_b, int64_t n_tokens, int64_t n_used, int64_t n_expert);
// a tile launch's epilogue: the ADD_ID biases, the (oai) SwiGLU of a dual launch, the routing weight (MUL(experts, weights), src/llama-graph.cpp:990)
struct mmq_moe_epi { const float * bias = nullptr; const float * bias2 = nullptr; size_t bias_stride = 0; const float * scale = nullptr; size_t scale_nb0 = 0, scale_nb1 = 0;
                     int oai = 0; float alpha = 0.0f, limit = 0.0f;
                     const float * glu_up = nullptr; size_t glu_up_nb1 = 0, glu_up_nb2 = 0; };     // (single-tensor launch as the gate half of a GLU: the finished up half, f32 [m, n_used, n_tokens])
// one launch over an expert stack. mul_mat_q_id (node by node: copy, sort, tiles) reads b / ids / scratch (mul_mat_q_id_scratch_bytes bytes) and sets xb / table / tile itself. mul_mat_q_id_tiles (the tiled
// kernel over a sorted pair table) reads xb: bf16 rows [token][n_b][kp(k)] (n_b == 1: a row per token, n_used: per pair); W2 != NULL: the dual kernel (tile 256): GLU(W.x + bias, W2.x + bias2) -> dst (f32, may be NULL) and / or y16 (bf16 rows of m per pair)
struct mmq_moe_call {
    int type; const void * W; const void * W2; size_t w_row_stride, w_expert_stride; int64_t m, k, n_expert; int64_t n_used, n_tokens, n_b;      // the expert stack; the pairs
    const float * b; size_t b_nb1, b_nb2; const int32_t * ids; size_t ids_nb0, ids_nb1; void * scratch;           // what the copy and the sort read and write
    const uint16_t * xb; const int * table; int tile; mmq_moe_epi epi;
    float * dst; size_t dst_nb1, dst_nb2; uint16_t * y16; hipStream_t stream;
};
void mul_mat_q_id(const mmq_moe_call & c);
void mul_mat_q_id_tiles(const mmq_moe_call & c);
// The fused expert chain of a prompt pass (backend_nodes.cpp try_fused_prefill_moe): one bf16 copy of the layer input and one sort serve gate, up and down. Planned once: the carve of
// the scratch (table2: the down launch's tiles, when their size differs) and the form — dual: gate / up as ONE launch of 256-pair tiles, biases and (oai) SwiGLU in its epilogue; else the up
// launch, then the gate launch, which reads the up product back (epi.glu_up). Both hand the down launch bf16 rows per pair (y16). dual_opt: option "moe_dual", or -1 (mmq.hip)
struct mmq_moe_plan { uint16_t * xb; int * table; int * table2; uint16_t * y16; size_t bytes; bool dual; int tile, tile_down; };
mmq_moe_plan mul_mat_q_id_plan(void * scratch, int64_t k, int64_t n_tokens, int64_t n_used, int64_t n_expert, int64_t m_glu, int dual_opt = -1);
// copy, sort and the gate / up launch(es): c as for the dual launch (W = gate, W2 = up, epi.bias / bias2, b, ids); !pl.dual: epi.glu_up is the tensor the up launch writes.
// Then (a second sort and) the down launch: reads pl.y16, adds its ADD_ID bias and multiplies with the routing weight; c: the down stack, ids, epi, dst
void mul_mat_q_id_gate_up(const mmq_moe_call & c, const mmq_moe_plan & pl);
void mul_mat_q_id_down(const mmq_moe_call & c, const mmq_moe_plan & pl);

// ---- dense f16/f32 x f32 mat-mul with ggml broadcast (attention K.Q and V.KQ; tests/test-backend-ops.cpp:5791-5813)
struct mm_dense_args {
    const void * a; int type_a; int64_t ne00, ne01, ne02, ne03; size_t nb00, nb01, nb02, nb03;
    const void * b; int type_b; int64_t ne10, ne11, ne12, ne13; size_t nb10, nb11, nb12, nb13;
    float * dst; size_t nb1, nb2, nb3;
};
// the kernel a dense MUL_MAT runs (mm_dense.hip: mul_mat_dense_path decides, from the arguments and the scratch size alone; mul_mat_dense launches it and says which)
enum mm_dense_path { MM_DENSE_MFMA, MM_DENSE_F16_PAIRS, MM_DENSE_F32_VEC, MM_DENSE_F32_ROWS, MM_DENSE_GENERIC };
mm_dense_path mul_mat_dense_path(const mm_dense_args & p, size_t scratch_bytes);
mm_dense_path mul_mat_dense(const mm_dense_args & p, void * scratch, size_t scratch_bytes, hipStream_t stream, int * n_launches);      // n_launches: how many kernels it started
// MUL_MAT_ID over an F16 / BF16 / F32 expert stack (correctness path: a wave per (row, pair))
void mul_mat_id_dense(int type_a, const void * as, size_t nb00, size_t nb01, size_t nb02, int64_t m, int64_t k, const void * b, size_t nb10, size_t nb11, size_t nb12, int64_t n_b,
                      const void * ids, size_t ids_nb0, size_t ids_nb1, int64_t n_used, int64_t n_tokens, int64_t n_expert, float * dst, size_t nb1, size_t nb2, hipStream_t stream);
// matrix-core form for more than 8 columns of f16 x f32 (prefill attention): f32 b is converted to f16 in `scratch`
bool   mul_mat_dense_mfma_supported(const mm_dense_args & p);
size_t mul_mat_dense_mfma_scratch_bytes(const mm_dense_args & p);
void   mul_mat_dense_mfma(const mm_dense_args & p, void * scratch, hipStream_t stream);

// ---- element kernels ---------------------------------------------
struct tensor_desc {           // a strided 4-D view, ggml convention (ne = elements, nb = bytes)
    void * data; int type; int64_t ne[4]; size_t nb[4];
};

void rms_norm(const tensor_desc & src, const tensor_desc & dst, float eps, hipStream_t stream);
// fused RMS_NORM * w (+ add) — tests/test-backend-ops.cpp:2856
// y16 != NULL (no add; rms_norm_mul_bf16_supported): also writes the bf16 copy of the result in the layout the prefill mat-mul reads
// (rows of ne0 rounded up to 64 elements, zero tail), so that its activation pre-pass is skipped
bool rms_norm_mul_bf16_supported(const tensor_desc & src, const tensor_desc & w, const tensor_desc & dst);
void rms_norm_mul(const tensor_desc & src, const tensor_desc & w, const tensor_desc * add, const tensor_desc & dst, float eps, hipStream_t stream, uint16_t * y16 = nullptr);
// the split-k planes of a prefill mat-mul (mul_mat_q with `defer`) + residual -> sum_out, and RMS_NORM(sum) * w -> y (+ its bf16 copy y16, or NULL);
// m % 4 == 0, all rows 16-byte aligned, np = 2 | 4 | 8
void combine_rms_norm(const float * planes, int np, int64_t m, int64_t n, const float * res, size_t res_nb1, float * sum_out, size_t sum_nb1,
                      const float * w, float * y, size_t y_nb1, uint16_t * y16, float eps, hipStream_t stream);
enum bin_op { BIN_ADD = 0, BIN_MUL = 1, BIN_DIV = 2, BIN_SUB = 3 };
void bin_bcast(int op, const tensor_desc & a, const tensor_desc & b, const tensor_desc & dst, hipStream_t stream);
void add_id(const tensor_desc & a, const tensor_desc & bias, const tensor_desc & ids, const tensor_desc & dst, hipStream_t stream);
void scale(const tensor_desc & src, const tensor_desc & dst, float s, float b, hipStream_t stream);
void cpy(const tensor_desc & src, const tensor_desc & dst, hipStream_t stream);      // f32<->f16/f32 strided copy/convert (CPY, CONT, DUP); CPY with a Q8_0 / Q4_0 side
// CPY with a quantized side: F32 -> Q8_0 / Q4_0, Q8_0 / Q4_0 -> F32, Q8_0 -> Q8_0, Q4_0 -> Q4_0; the same ne0 on both sides, whole blocks, quantized rows dense
bool cpy_quantized_supported(const tensor_desc & src, const tensor_desc & dst);
void set_rows(const tensor_desc & src, const tensor_desc & idx, const tensor_desc & dst, hipStream_t stream);
void get_rows(const tensor_desc & src, const tensor_desc & idx, const tensor_desc & dst, hipStream_t stream);
void sum_rows(const tensor_desc & src, const tensor_desc & dst, hipStream_t stream);
// one token: logits = w . x (+ bias) [-> soft_max -> probs] -> sorted = argsort descending (elem.hip: k_moe_route); n_expert <= 256,
// k % 4 == 0, 16-byte aligned rows; logits / probs may be NULL when the graph does not read them
bool moe_route_norm_supported(int64_t k, int64_t n_expert, const float * ws);
// norm_w != NULL: x is the raw residual stream; the router's input y = RMS_NORM(x) * norm_w is computed in the kernel and written to y_out
void moe_route(const float * w, size_t w_nb1, const float * x, const float * bias, int64_t k, int64_t n_expert, bool softmax,
               float * logits, float * probs, int32_t * sorted, hipStream_t stream, float * ws,
               const float * norm_w = nullptr, float eps = 0.0f, float * y_out = nullptr,    // ws: 257 zero-initialised words (>= 16 experts: several workgroups)
               unsigned * err = nullptr,    // host-mapped words: err[1] is set when the ranking workgroup's bounded wait for a logit gave up
               float * topv = nullptr);     // 8 floats: the best values in rank order (moe_combine / the grouped mat-vec's plane weights take them with ids == NULL)
// one token: dst[i] = sum_u experts[u][i] * w_u (+ res[i]); w from probs[ids[u]] (ids == NULL: probs[u]) normalised (mode 0) or soft_max'ed (mode 1);
// n_used <= 8, n_embd % 4 == 0, 16-byte aligned rows (elem.hip: k_moe_combine)
void moe_combine(const float * probs, const int32_t * ids, int n_used, int mode, const void * experts, size_t e_nb1, int64_t n_embd,
                 const float * res, float * dst, hipStream_t stream);
// many tokens: dst[t] = ((experts[t][0] + experts[t][1]) + ...) [+ res[t]] (m % 4 == 0, 16-byte aligned rows; elem.hip: k_slot_sum)
void moe_slot_sum(const void * experts, size_t nb1, size_t nb2, int n_used, int64_t m, int64_t n_tokens, const float * res, size_t res_nb1, float * dst, size_t dst_nb1, hipStream_t stream);
void argsort(const tensor_desc & src, const tensor_desc & dst, int order, hipStream_t stream);
void unary(int op, const tensor_desc & src, const tensor_desc & dst, hipStream_t stream);
void glu(int glu_op, bool swapped, const tensor_desc & a, const tensor_desc * b, const tensor_desc & dst, float alpha, float limit, hipStream_t stream);

void rope(const tensor_desc & src, const int32_t * pos, const float * freq_factors, const tensor_desc & dst, const rope_params & p, hipStream_t stream);
// CPY(kv -> F32) -> ROPE -> CPY(F32 -> kv) on a Q8_0 / Q4_0 cache view [head dim, kv heads, cells, ne3] in place, one launch (elem.hip: k_kv_shift);
// pos: one I32 per cell (ne2). The bytes are those the three launches leave.
bool kv_shift_supported(const tensor_desc & kv, const rope_params & p);
void kv_shift(const tensor_desc & kv, const int32_t * pos, const float * freq_factors, const rope_params & p, hipStream_t stream);

void soft_max(const tensor_desc & src, const tensor_desc * mask, const float * sinks, const tensor_desc & dst,
              float scale, float max_bias, hipStream_t stream);

// ---- fused decode kernels (decode_fused.hip): same arithmetic as the node-by-node kernels, fewer launches -----
// RMS_NORM * w -> f32 row y AND its quantized form q (rows of ne0 floats, ne0 % 256 == 0, ne0 <= 8192)
bool rms_norm_mul_quant_supported(int64_t ne0);
void rms_norm_mul_quant(const float * x, size_t x_stride, const float * w, float * y, size_t y_stride, const act_q8 & q,
                        int64_t ne0, int64_t nrows, float eps, hipStream_t stream);
// swiglu(g, u) = silu(g)*u -> f32 row y AND its quantized form q
void swiglu_quant(const float * g, size_t g_stride, const float * u, size_t u_stride, float * y, size_t y_stride, const act_q8 & q,
                  int64_t ne0, int64_t nrows, hipStream_t stream);
// SET_ROWS(k) + SET_ROWS(v, element scatter) into the f16 cache, one launch
void kv_store_f16(const float * k_src, size_t k_src_nb1, const int64_t * k_idx, void * k_dst, size_t k_dst_nb1, int64_t k_ne0, int64_t k_rows,
                  const float * v_src, const int64_t * v_idx, void * v_dst, int64_t v_n, hipStream_t stream);
// ---- attention: K.q -> soft_max(scale, mask, sinks) -> V.p -> [hsv*n_head, T]; a few tokens (T <= 8): decode_fused.hip, many: attn_prefill.hip ----
// FLASH_ATTN_EXT's (K, V) head sizes: 64/64, 80/80 (not a multiple of a 32-element block: F16 / BF16 caches only), 96/96, 128/128, 192/192, 256/256 and 192/128
constexpr bool attn_fa_head_sizes(int64_t hsk, int64_t hsv, int k_type, int v_type) {
    if (hsk == 192 && hsv == 128) return true;
    if (hsk != hsv) return false;
    if (hsk == 80) return (k_type == T_F16 || k_type == T_BF16) && (v_type == T_F16 || v_type == T_BF16);
    return hsk == 64 || hsk == 96 || hsk == 128 || hsk == 192 || hsk == 256;
}
// the (K, V) type pairs the row-major-V decode kernel reads directly; the others go through kv_to_f16 first
constexpr bool attn_decode_kv_types_fused(int k_type, int v_type) {
    return (k_type == v_type && (k_type == T_F16 || k_type == T_Q8_0 || k_type == T_Q4_0 || k_type == T_BF16)) || (k_type == T_Q8_0 && (v_type == T_F16 || v_type == T_Q4_0));
}
// the decode attention's partial-result buffer: 8 tokens x 128 heads x 32 ranges x (128 + 2) floats, i.e. 64 heads of 256 (+ 2); allocated once per backend
constexpr size_t ATTN_PART_BYTES = (size_t) 8*128*32*(128 + 2)*4;
constexpr int T_NONE = -1;
// one attention launch, as both launchers and every plan and support answer take it: value-initialise, fill by name (the plans read no pointer)
struct attn_call {
    const void * q; size_t q_nb1, q_nb2; int q_type;      // [hsk, T, n_head], T_F32: nb1 = token stride, nb2 = head stride
    const void * k; size_t k_nb1, k_nb2; int k_type;      // [hsk, n_kv, n_head_kv]: nb1 = cell stride, nb2 = head stride
    const void * v; size_t v_nb1, v_nb2; int v_type;      // row-major [hsv, n_kv, n_head_kv]: nb1 = cell stride; v_trans [n_kv, hsv, n_head_kv]: nb1 = dim stride (a row over cells)
    bool v_trans;                                         // the V cache of the graph without flash attention, and kv_to_f16's transposed copy
    const void * mask; size_t m_nb1; int mask_type = T_NONE;      // [n_kv, >= T] of T_F16 / T_F32, or T_NONE
    const float * sinks;
    float * dst; size_t dst_nb1;                          // [hsv*n_head, T]; NULL (prefill): only y16 is wanted
    uint16_t * y16;                                       // prefill: also the bf16 copy the following mat-mul reads, rows of hsv*n_head rounded up to a multiple of 64
    int64_t hsk, hsv, n_kv, n_head, n_head_kv, T;
    // per-sequence KV streams (kv_unified = false, src/llama-graph.cpp:1231-1238): n_stream sequences of T tokens each in one launch, every one over its own K / V
    // (and mask); 0 or 1: one stream, the strides below are not read. Byte strides along the stream dimension (ne[3]); m_nb3 = 0: one mask for all streams.
    // dst_nb3: stream s's rows start T rows behind stream s - 1's in a dense [hsv*n_head, T*n_stream] result. y16 rows likewise. Sinks are per head.
    int64_t n_stream; size_t q_nb3, k_nb3, v_nb3, m_nb3, dst_nb3;
    float scale, softcap, max_bias;                       // logit_softcap and ALiBi: FLASH_ATTN_EXT's other two parameters (0: none)
    float * part; size_t part_bytes;                      // decode: the partial-result buffer on offer (0 bytes: none)
    hipStream_t stream;
};
// Decode, planned once. Long contexts (a multiple of 32 cells): with the partial buffer the cells are split into nsplit ranges of kv_chunk (up to 32 workgroups per
// (head, token)) that a second small kernel merges; live_scan: one workgroup per head that stops at the last unmasked cell. ok: there is a kernel for the
// head sizes and types (v_trans: 64 / 128, F16 or Q8_0 K, F16 V; row-major V: attn_fa_head_sizes, attn_decode_kv_types_fused) and the score row fits the LDS
// (n_kv % 8 == 0 up to 12288 cells) or its ranges fit part_bytes. part_bytes_needed: 0 = no split for this shape. The buffer holds a slot per (stream, token, head,
// range): with several streams, when the full count of ranges does not fit, fewer are taken (at least 2, each within one LDS); when none fits and the row does not
// either, ok = false. (One stream keeps the rule it had: the full count or no split.)
struct attn_decode_plan { bool ok; int nsplit, kv_chunk; bool live_scan; size_t lds_bytes, part_bytes_needed; };
attn_decode_plan attn_plan_decode(const attn_call & c);
// Prefill: one wave per (head, 32 queries), nw waves per workgroup = hpw heads of one kv head x query tiles x ks-way split cell blocks; grid.z = the stream. ok: F16 K and V, n_kv % 32 == 0,
// head sizes: v_trans: attn_fa_head_sizes; row-major V: 64 / 128
struct attn_prefill_plan { bool ok; int nw, hpw, ks; dim3 grid; };
attn_prefill_plan attn_plan_prefill(const attn_call & c);
// the one support answer, for supports_op (part_bytes = ATTN_PART_BYTES) and the nodes themselves (the buffer they have): the plan's ok for the operands as
// the launcher gets them — FLASH_ATTN_EXT's after fa_kv16_plan's conversions (backend_nodes.cpp)
inline int64_t attn_n_stream(const attn_call & c) { return c.n_stream > 1 ? c.n_stream : 1; }
inline bool attn_supported(const attn_call & c) { return c.T > 8 ? attn_plan_prefill(c).ok : attn_plan_decode(c).ok; }
void attn_decode(const attn_call & c);       // T <= 8
void attn_prefill(const attn_call & c);      // T > 8
// K / V cache views [hd, n_kv, n_head_kv, n_stream] of type F16 / BF16 / Q8_0 / Q4_0 -> dense f16: rows of cells [n_stream][n_head_kv][n_kv][hd], or transposed
// (rows over cells, the layout the matrix-core prefill kernel stages with coalesced loads) [n_stream][n_head_kv][hd][n_kv]; n_kv % 8 == 0; hd (the size of the tensor
// converted, K's or V's): a multiple of 8 (of 32 for Q8_0 / Q4_0) up to 256. One launch for all streams, each stream's copy dense behind the previous one's.
void kv_to_f16(int type, const void * src, size_t nb1, size_t nb2, size_t nb3, int64_t hd, int64_t n_kv, int64_t n_head_kv, int64_t n_stream, uint16_t * dst, bool transpose, hipStream_t stream);
// the soft_max's constants as both kernels' argument structs carry them: the scale divided by logit_softcap, and ALiBi's slopes
// (ggml_compute_forward_flash_attn_ext_f16 / soft_max: m0 = 2^(-max_bias / n), m1 = 2^(-max_bias / 2 / n), n = 2^floor(log2 n_head))
template <typename A> static inline void attn_set_softmax(A & a, const attn_call & c) {
    a.scale = c.softcap != 0.0f ? c.scale/c.softcap : c.scale; a.softcap = c.softcap; a.max_bias = c.max_bias;
    a.n_head_log2 = 1; while (2*a.n_head_log2 <= (int) c.n_head) a.n_head_log2 *= 2;
    a.m0 = powf(2.0f, -c.max_bias/(float) a.n_head_log2); a.m1 = powf(2.0f, -(c.max_bias/2.0f)/(float) a.n_head_log2);
}
// the instantiations: f(K, V) with the matching pair as two std::integral_constant (as weight_format_dispatch, blocks.h); false: no such pair
template <int A, int B, typename F> static inline bool attn_pair_is(int64_t a, int64_t b, F & f) { return a == A && b == B && (f(std::integral_constant<int, A>{}, std::integral_constant<int, B>{}), true); }
template <typename F> static inline bool attn_dispatch_sizes(int64_t hsk, int64_t hsv, F && f) {      // the pairs of attn_fa_head_sizes
    return attn_pair_is<64, 64>(hsk, hsv, f) || attn_pair_is<80, 80>(hsk, hsv, f) || attn_pair_is<96, 96>(hsk, hsv, f) || attn_pair_is<128, 128>(hsk, hsv, f) ||
           attn_pair_is<192, 192>(hsk, hsv, f) || attn_pair_is<256, 256>(hsk, hsv, f) || attn_pair_is<192, 128>(hsk, hsv, f);
}
template <typename F> static inline bool attn_dispatch_types(int k_type, int v_type, F && f) {      // the pairs of attn_decode_kv_types_fused
    return attn_pair_is<T_F16, T_F16>(k_type, v_type, f) || attn_pair_is<T_Q8_0, T_Q8_0>(k_type, v_type, f) || attn_pair_is<T_Q4_0, T_Q4_0>(k_type, v_type, f) ||
           attn_pair_is<T_BF16, T_BF16>(k_type, v_type, f) || attn_pair_is<T_Q8_0, T_F16>(k_type, v_type, f) || attn_pair_is<T_Q8_0, T_Q4_0>(k_type, v_type, f);
}
// a run-time int as a compile-time tag: f(std::integral_constant<int, v>{}) when v is one of Vs; false: it is not
template <int... Vs, typename F> static inline bool dispatch_int(int v, F && f) { return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...); }

// the persistent kernels run one workgroup per CU: the current device's CU count, asked for once (mmvq_fused.hip)
int device_cu_count();
// the dynamic LDS a workgroup of the streamed kernels may use: a CU's 160 KiB
constexpr int MI_LDS_BUDGET = 160*1024;

// grouped mat-vec (n = 1): up to MMVQ_MAX_GROUPS weight tensors that share one activation vector, each with an epilogue
constexpr int MMVQ_MAX_GROUPS = 4;
enum mmvq_epilogue { EPI_NONE = 0, EPI_ADD = 1, EPI_ROPE = 2, EPI_GLU = 3 };
struct mmvq_group {
    const char * W; const char * W2;   // W2: the second weight tensor of EPI_GLU (dst = silu(W.x) * (W2.x))
    size_t row_stride; int m; int type;
    float * dst; int epi;
    const float * res;                 // EPI_ADD: dst[row] = W.x + res[row]
    // optional f16 store of the result (the KV-cache write that follows wk / wv in the graph):
    //   st_mode 1: row store     st16[st_idx[0]*st_row_elems + row]   (SET_ROWS of one K row)
    //   st_mode 2: element store st16[st_idx[row]]                    (SET_ROWS on the transposed-V [1, N] view)
    uint16_t * st16; const int64_t * st_idx; int64_t st_row_elems; int st_mode;
    // MUL_MAT_ID for one token (src/llama-graph.cpp:569-595): the group's matrices are expert eid[0] of a stack (W += eid[0]*estride,
    // W2 likewise); x_off: this group's activation vector starts x_off floats into the launch's x (the down projection reads one
    // activation per used expert). eid == NULL: a plain weight tensor.
    const int32_t * eid; size_t estride; int x_off;
    // EPI_GLU variants of gpt-oss's expert FFN (src/llama-graph.cpp:927-968): per-expert biases added to the two products (ADD_ID,
    // row `eid[0]` of [m, n_expert] f32 tensors) and swiglu_oai(alpha, limit) instead of swiglu when glu_alpha != 0
    const float * b_gate; const float * b_up; float glu_alpha, glu_limit;
    // EPI_ADD extras: res2 = a second addend, added after res (MUL_MAT -> ADD(bias) -> ADD(residual)); res_eid != 0: res is a [m, n_expert]
    // table and the group adds row eid[0] of it (MUL_MAT_ID -> ADD_ID)
    const float * res2; int res_eid;
};
// GLU launches only: the launch also writes its f32 output as the quantized image (act_q8 layout for n = 1) the next mat-vec reads;
// counters: >= m/256 words, zero between launches (the kernel re-arms them). m % 256 == 0, one group, no expert stack.
struct mmvq_fin { int kind; int pad; int8_t * qs; float * d; int16_t * bs; unsigned * counters; };
void mul_mat_vec_q_fused_rope_table(const mmvq_rope & rope, float * table, hipStream_t stream);

// where the activation vector comes from
enum mmvq_prologue { PRO_Q8 = 0, PRO_QUANT = 1, PRO_NORM = 2 };
struct mmvq_input {
    int mode;
    act_q8 act;            // PRO_Q8: one quantized column laid out by act_q8_carve(…, n = 1) (one contiguous image)
    const float * x;       // PRO_QUANT / PRO_NORM: the f32 vector (16-byte aligned, k % 256 == 0)
    const float * norm_w;  // PRO_NORM: y = (x * rsqrt(mean(x^2) + eps)) * norm_w, then quantized — RMS_NORM -> MUL folded in
    float eps;
    int act_kind;
    // PRO_NORM only, planes != NULL (then pl_probs != NULL too): the vector is not materialized yet and the launch also stores it to x_out (the graph's
    // ADD result)
    const float * planes; int n_planes; int plane_stride; float * x_out;
    // — the tail of build_moe_ffn (src/llama-graph.cpp:887-1012) left unevaluated: the planes are the used experts' outputs and the vector
    // is sum_u planes[u][i] * w_u (+ x[i], the residual, when x != NULL), w_u from pl_probs[pl_ids[u]] normalised (pl_mode 0) or soft_max'ed (1) — k_moe_combine's
    // arithmetic in k_moe_combine's order
    const float * pl_probs; const int32_t * pl_ids; int pl_mode;
};
bool mul_mat_vec_q_fused_supported(int64_t k, int act_kind);
bool mul_mat_vec_q_fused_prologue_supported(int64_t k, int act_kind);        // PRO_QUANT / PRO_NORM limits (k % 256, or k % 32 with Q8_0 activations)
bool mul_mat_vec_q_fused_can_group(int type_a, int type_b);         // may these two weight types share one grouped launch
bool mul_mat_vec_q_fused_can_group_mixed(int type_a, int type_b);   // pairs of different activation formats (only when the launch quantizes the activation itself)
// the optional timing record of ONE grouped launch, filled per call (NULL: not profiling; the module keeps no launch state of its own). e0 != NULL: the
// launch carries (e0, e1) as its dispatch's start / stop events (hipExtLaunchKernelGGL). kernel: the launcher stores the name of the instantiation it used,
// spelled as rocprofv3's kernel trace spells it
struct mmvq_launch_rec { hipEvent_t e0, e1; const char * kernel; };
// every kernel of the launch is on `stream` when this returns
void mul_mat_vec_q_fused(const mmvq_group * groups, int n_groups, int64_t k, const mmvq_input & in, const mmvq_rope * rope, hipStream_t stream,
                         const mmvq_fin * fin = nullptr, mmvq_launch_rec * rec = nullptr);
// the streamed form of the grouped launch (mmvq_stream.h: loader wave + LDS slot ring + one 256-weight unit per lane): K-quant weights in
// contiguous rows, no expert stacks; mul_mat_vec_q_fused routes to it when mul_mat_vec_q_stream_takes says so (it never writes an mmvq_fin image)
bool mul_mat_vec_q_stream_enabled(void);       // GGML_MI355X_STREAM (default 1)
bool mul_mat_vec_q_stream_takes(const mmvq_group * groups, int n_groups, int64_t k, const mmvq_input & in, const mmvq_rope * rope);     // = the launch's plan is ok (mmvq_stream.h: st_plan)
// may this grouped launch be handed to mul_mat_vec_q_fused at all: every group's format has a register-ring kernel (mmvq_fused_<format>.hip), or the streamed kernel
// takes the launch as it stands. Not every format of the list has a register-ring kernel (mmvq_fused.hip: fused_pairs): a matcher asks this before it emits and runs the nodes one by one on false
bool mul_mat_vec_q_fused_takes(const mmvq_group * groups, int n_groups, int64_t k, const mmvq_input & in, const mmvq_rope * rope);
bool mul_mat_vec_q_fused_fin_supported(int64_t m, int64_t k_in);   // may a GLU launch with m output rows carry an mmvq_fin

// ---- small uploads batched into one launch (backend.cpp: be_set_tensor_async / uploads_flush) ----
constexpr int UPLOAD_BATCH_MAX = 12;
struct upload_batch { int n; const void * src[UPLOAD_BATCH_MAX]; void * dst[UPLOAD_BATCH_MAX]; uint32_t bytes[UPLOAD_BATCH_MAX]; int blocks[UPLOAD_BATCH_MAX]; };   // blocks[i] = ceil(bytes[i] / 4096)
void upload_batch_launch(const upload_batch & b, hipStream_t stream);

// ---- test / bench support ------------------------------------------------------------------
// raw streaming read of `bytes` (16 B/lane, nontemporal) — measures the achievable HBM rate on the box
void hbm_read_probe(const void * p, size_t bytes, unsigned * sink, hipStream_t stream);

} // namespace mi355x
