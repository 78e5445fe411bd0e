// kv_quant_dev.h — one 32-element block of a quantized KV cache (Q8_0 / Q4_0) on the device: the reference row quantizers restated operation for
// operation (gguf-py/gguf/quants.py:222-238 Q4_0, :381-393 Q8_0 — oracle/ggml_oracle.c quantize_row_q4_0_ref / quantize_row_q8_0_ref, pinned bit-exactly
// by tests/golden/quant_*.npz) and their inverse. Shared by every kernel that writes or reads such a block from f32 (elem.hip: k_set_rows_q, k_cpy_q,
// k_kv_shift), so that the same 32 floats give the same bytes whichever launch carries them.
#pragma once

#include "dev_common.h"
#include "blocks.h"

namespace mi355x {

template <int TYPE> constexpr int kv_block_bytes() { static_assert(TYPE == T_Q8_0 || TYPE == T_Q4_0, "a KV cache block type"); return TYPE == T_Q8_0 ? 34 : 18; }

// v[0..31] -> the block at out (2-byte aligned, as every Q8_0 / Q4_0 row is: 34- and 18-byte blocks), written as 16-bit words
template <int TYPE>
static __device__ __forceinline__ void quant_block(const float (&v)[32], void * out) {
    u16_u * o = (u16_u *) out;
    if (TYPE == T_Q8_0) {
        float amax = 0.0f;
#pragma unroll
        for (int j = 0; j < 32; j++) { const float a = fabsf(v[j]); if (a > amax) amax = a; }
        const float d = amax/127.0f;
        const float id = d != 0.0f ? 1.0f/d : 0.0f;
        o[0].v = f32_to_f16_bits(d);
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t q0 = (uint8_t)(int8_t) roundf(v[2*j]*id), q1 = (uint8_t)(int8_t) roundf(v[2*j + 1]*id);
            o[1 + j].v = (uint16_t)(q0 | (q1 << 8));
        }
    } else {
        // the first element of largest magnitude gives the scale its sign: strict <, a tie keeps the earlier element
        float amax = 0.0f, mx = 0.0f;
#pragma unroll
        for (int j = 0; j < 32; j++) { if (amax < fabsf(v[j])) { amax = fabsf(v[j]); mx = v[j]; } }
        float d = mx/-8.0f;
        // keep the product in a register of its own: fused into the f16 conversion (v_fma_mixlo_f16 with a +0 addend) a zero block's
        // d = 0 / -8 = -0.0 came out as +0.0, one bit off the reference's bytes
        asm volatile("" : "+v"(d));
        const float id = d != 0.0f ? 1.0f/d : 0.0f;
        o[0].v = f32_to_f16_bits(d);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            uint32_t w = 0;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int v0 = (int)(v[2*j + h]*id + 8.5f), v1 = (int)(v[16 + 2*j + h]*id + 8.5f);
                w |= (uint32_t)((v0 < 15 ? v0 : 15) | ((v1 < 15 ? v1 : 15) << 4)) << (8*h);
            }
            o[1 + j].v = (uint16_t) w;
        }
    }
}

// element i0 (< 32*blocks) of the row of blocks at `row`: x = f32(d)*q (Q8_0), f32(d)*(q - 8) (Q4_0) — an exact integer times one f32, one rounding
template <int TYPE>
static __device__ __forceinline__ float dequant_elem(const char * row, int64_t i0) {
    const uint8_t * b = (const uint8_t *) row + (i0 >> 5)*kv_block_bytes<TYPE>();
    const int j = (int)(i0 & 31);
    const float d = f16_bits_to_f32(((const u16_u *) b)->v);
    if (TYPE == T_Q8_0) return d*(float)(int8_t) b[2 + j];
    const int q = b[2 + (j & 15)];
    return d*(float)((j < 16 ? (q & 0xF) : (q >> 4)) - 8);
}

} // namespace mi355x
