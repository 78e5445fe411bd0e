// blocks.h — GGUF block formats as the backend sees them in HBM (raw GGUF bytes,
// unmodified: src/llama-model-loader.cpp:1060 uploads them as-is).
// Layouts: gguf-py/gguf/quants.py (class per type, cited below); sizes:
// gguf-py/gguf/constants.py:2839-2872 — and the list of weight formats built on them. Shared by host and device code.
#pragma once

#include <stdint.h>
#include <type_traits>

#define MI_QK_K 256
#define MI_K_SCALE_SIZE 12

#pragma pack(push, 1)
// Q4_0: 32 el / 18 B — quants.py:241-251. el j<16 = low nibble of qs[j], j>=16 = high nibble; x = d*(q-8)
struct block_q4_0 { uint16_t d; uint8_t qs[16]; };
// Q5_0: 32 el / 22 B — quants.py:291-330. nibbles as Q4_0; bit j of qh (little-endian u32) = 5th bit of el j; x = d*(q-16)
struct block_q5_0 { uint16_t d; uint8_t qh[4]; uint8_t qs[16]; };
// Q5_1: 32 el / 24 B — quants.py:333-375. as Q5_0 plus f16 m; x = d*q + m
struct block_q5_1 { uint16_t d; uint16_t m; uint8_t qh[4]; uint8_t qs[16]; };
// Q8_0: 32 el / 34 B — quants.py:396-401. x = d*q
struct block_q8_0 { uint16_t d; int8_t qs[32]; };
// Q3_K: 256 el / 110 B — quants.py:431-472. el 128n + 32j + l: low 2 bits = (qs[32n + l] >> 2j) & 3, bit 4n + j of hmask[l] SET = no -4 offset; sixteen 6-bit
// scales (16 elements each, value sc - 32) packed in 12 bytes, f16 d LAST; x = (d*(sc-32))*q
struct block_q3_K { uint8_t hmask[32]; uint8_t qs[64]; uint8_t scales[12]; uint16_t d; };
// Q4_K: 256 el / 144 B — quants.py:504-522. 8 sub-blocks of 32; qs in 4 groups of 32 B
// (low nibble = sub-block 2g, high = 2g+1); x = d*sc*q - dmin*m, sc/m 6-bit (quants.py:479-501)
struct block_q4_K { uint16_t d; uint16_t dmin; uint8_t scales[MI_K_SCALE_SIZE]; uint8_t qs[MI_QK_K/2]; };
// Q5_K: 256 el / 176 B — quants.py:527-549. as Q4_K plus qh: bit i of qh[j] = 5th bit of sub-block i, el j
struct block_q5_K { uint16_t d; uint16_t dmin; uint8_t scales[MI_K_SCALE_SIZE]; uint8_t qh[MI_QK_K/8]; uint8_t qs[MI_QK_K/2]; };
// Q6_K: 256 el / 210 B — quants.py:554-572. ql 128 B, qh 64 B, 16 int8 scales, f16 d LAST; x = d*sc*(q-32)
struct block_q6_K { uint8_t ql[MI_QK_K/2]; uint8_t qh[MI_QK_K/4]; int8_t scales[MI_QK_K/16]; uint16_t d; };
// MXFP4: 32 el / 17 B — quants.py:656-700. e8m0 scale byte, nibbles split like Q4_0; x = e8m0_half(e)*kvalues[q]
struct block_mxfp4 { uint8_t e; uint8_t qs[16]; };
#pragma pack(pop)

namespace mi355x {
// THE list of weight formats MUL_MAT(_ID) takes: X(name, ggml_type id, block struct, elements per block, bytes per block, activation format). Ids: constants.py:2698-2730;
// sizes: constants.py:2839-2872; activation format = the CPU path's vec_dot_type. Every plain fact about a format is generated from here — the T_<name> constants, the
// size asserts, weight_format_of(), weight_format_dispatch(); what stays per format is code shaped for one kernel (DESIGN.md "Adding a weight format").
#define MI_WEIGHT_FORMATS(X) \
    X(Q4_0,  2,  block_q4_0,  32,  18,  Q8_0) X(Q5_0,  6,  block_q5_0,  32,  22,  Q8_0) X(Q5_1,  7,  block_q5_1,  32,  24,  Q8_0) \
    X(Q8_0,  8,  block_q8_0,  32,  34,  Q8_0) X(Q3_K,  11, block_q3_K,  256, 110, Q8_K) X(Q4_K,  12, block_q4_K,  256, 144, Q8_K) \
    X(Q5_K,  13, block_q5_K,  256, 176, Q8_K) X(Q6_K,  14, block_q6_K,  256, 210, Q8_K) X(MXFP4, 39, block_mxfp4, 32,  17,  Q8_0)
#define MI_X(N_, ID_, B_, QK_, BYTES_, A_) T_##N_ = ID_,
enum : int { MI_WEIGHT_FORMATS(MI_X) T_Q8_K = 15 };      // (Q8_K: the K-quants' activation format, never a weight)
#undef MI_X
// a row of the list by run-time or compile-time type, in host and device code; qk == 0: the type is not in the list
struct weight_format { int qk, bytes, act; };
constexpr weight_format weight_format_of(int type) {
    switch (type) {
#define MI_X(N_, ID_, B_, QK_, BYTES_, A_) case ID_: static_assert(sizeof(B_) == BYTES_, #N_ " block size"); return { QK_, BYTES_, T_##A_ };
        MI_WEIGHT_FORMATS(MI_X)
#undef MI_X
        default: return { 0, 0, -1 };
    }
}
// a run-time weight type as a compile-time tag: calls f(std::integral_constant<int, type>{}); false: the type is not in the list (f was not called)
template <typename F> static inline bool weight_format_dispatch(int type, F && f) {
    switch (type) {
#define MI_X(N_, ID_, B_, QK_, BYTES_, A_) case ID_: f(std::integral_constant<int, ID_>{}); return true;
        MI_WEIGHT_FORMATS(MI_X)
#undef MI_X
        default: return false;
    }
}
} // namespace mi355x
