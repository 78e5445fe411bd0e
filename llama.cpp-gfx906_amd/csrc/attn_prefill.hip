// attn_prefill.hip — K.q -> soft_max(scale, mask, sinks) -> V.kq -> [hd*n_head, T] for MANY tokens (T > 8) as one kernel on the matrix
// cores, with an online softmax: the n_kv x T score matrix never goes to memory.
//
// Replaces, for the node group build_attn_mha emits without flash attention (src/llama-graph.cpp:1283-1330):
//   MUL_MAT(k, q) [prec F32] -> SOFT_MAX(mask, scale) [+ sinks] -> MUL_MAT(v, kq) -> PERMUTE -> CONT
// with the unified KV cache's layouts (src/llama-kv-cache-unified.cpp:1056-1106): K rows [hd] per cell, V TRANSPOSED (v_trans: one
// row of cells per head dimension). Arithmetic as the node-by-node path: q and the probabilities rounded to f16 (the vec_dot type
// of an F16 matrix), f32 accumulation, soft_max in f32.
//
// One wave per (head, 32 queries); 8 waves (a GQA group x query tiles) share the K / V^T blocks through LDS (see the kernel). Everything is
// computed TRANSPOSED so that a lane owns ONE query column:
//   S^T[32 cells x 32 queries] = K[32 x hd] . Q^T      (v_mfma_f32_32x32x16_f16, A = K rows straight from the cache, B = Q^T)
//   per-lane online softmax over the 16 cells a lane holds (+ one exchange with lane ^ 32: the other 16 cells of the same query)
//   O^T[hd x 32 queries] += V^T[hd x 32 cells] . P^T   (A = rows of the transposed V cache, B = P^T straight from the registers of S^T)
// The C-layout of S^T (cell = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) IS a valid B-operand k-slot order as long as V^T's k-slots use
// the same cell permutation — a sum over cells does not care about their order — so the probabilities never leave the registers.
#include "dev_common.h"
#include "kv_types.h"
#include "kernels.h"

namespace mi355x {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float    f32x16 __attribute__((ext_vector_type(16)));

struct attn_pf_args {
    const char * q; size_t q_nb1, q_nb2;                // q [hd, T, n_head] f32 (permuted view): nb1 = token stride, nb2 = head stride
    const char * k; size_t k_nb1, k_nb2;                // k [hd, n_kv, n_head_kv] f16: nb1 = cell stride, nb2 = head stride
    const char * v; size_t v_nb1, v_nb2;                // v [n_kv, hd, n_head_kv] f16 (transposed): nb1 = dim stride, nb2 = head stride
    const char * mask; size_t m_nb1; int mask_f16;      // mask [n_kv, T_pad]
    const float * sinks;
    float * dst; size_t dst_nb1;                        // [hd*n_head, T] (NULL: only the bf16 copy is wanted)
    uint16_t * y16; int kp16;                           // != NULL: the result also as bf16 rows of kp16 elements — the activation copy the wo mat-mul reads (mmq.hip)
    int n_kv, n_head, n_head_kv, T;
    float scale;
    float softcap, max_bias, m0, m1; int n_head_log2;      // logit_softcap (scale already divided by it) and ALiBi, as in decode_fused.hip
    size_t q_nb3, k_nb3, v_nb3, m_nb3, dst_nb3;            // blockIdx.z = the KV stream (kernels.h: attn_call): its q, K, V, mask (m_nb3 = 0: shared) and T result rows
};

static __device__ __forceinline__ float xhalf(float v, int lane) {      // the value lane ^ 32 holds
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, __builtin_bit_cast(int, v)));
}

// VT: transposed V cache (rows over cells). !VT: V rows are cells (FLASH_ATTN_EXT): the 8 cells of a k-slot group are then 8 two-byte
// gathers per operand — correct, not fast; a transposing LDS read is the next step for that layout.
constexpr int APF_NW = 8;
constexpr int APF_KLD = 16;     // LDS row padding (bytes): K rows HD*2 + 16 (ds_read_b128 conflict-free), V^T rows 64 + 8 (ds_read_b64 conflict-free)
// One workgroup of 8 waves = hpw heads of ONE kv head (the GQA group, or a power-of-two part of it) x 8/hpw tiles of 32 queries. The waves
// walk the cell blocks together: a block's K rows and V^T rows are staged ONCE into LDS with coalesced loads (double-buffered, the next
// block's loads in flight during the arithmetic) and every wave takes its MFMA operands from there. Before this, every wave gathered its
// own K rows (2 KB apart) and V^T rows (n_ctx*2 bytes apart) 8-16 bytes at a time: 768 sector requests per block and wave, 42 us per
// layer at 512 tokens and 399 us at 2048 however the blocks were spread over waves.
// MASK: 0 = none, 1 = f32, 2 = f16 (a template parameter: the loads stay in one basic block). A wave skips the arithmetic of a block
// whose mask is -inf for all its 32 x 32 pairs (the causal future); staging and barriers go on.
// KS = 2 (few workgroups, i.e. short prompts: the cell loop is the critical path): an iteration stages TWO cell blocks, the waves of a
// (head, query tile) come in pairs — one per block — and the pair's states are merged through LDS at the end: half the iterations.
// HD / HDV: the sizes of a K and a V row (flash attention: every pair of attn_fa_head_sizes, with the transposed V copy). NC comes from HD, the NDT output
// tiles of 32 dims from HDV: 80 is computed as 96, rows 80..95 of V^T zero in LDS and never stored. Staging takes KTR / VTR trips of the workgroup per block.
// NW: waves per workgroup. 192 and 256 run with 4: their accumulators (NDT x 16) and Q (NC x 4 registers) need more than the 256 registers a lane has
// when two waves share a SIMD.
template <int HD, bool VT, int MASK, int KS, int HDV = HD, int NW = APF_NW>
__global__ void __launch_bounds__(64*NW) k_attn_prefill(const attn_pf_args pa, int hpw) {
    attn_pf_args p = pa;      // this workgroup's stream (all zero offsets in a one-stream launch)
    {
        const size_t sz = blockIdx.z;
        p.q += sz*pa.q_nb3; p.k += sz*pa.k_nb3; p.v += sz*pa.v_nb3;
        if (pa.mask) p.mask += sz*pa.m_nb3;
        if (pa.dst) p.dst = (float *) ((char *) pa.dst + sz*pa.dst_nb3);
        if (pa.y16) p.y16 += sz*(size_t) pa.T*pa.kp16;
    }
    constexpr int NC = HD/16, NDT = (HDV + 31)/32, CPR = HD/8, NT = 64*NW;      // CPR: 16-byte chunks per K row
    constexpr int HDVP = 32*NDT;                                        // V^T rows in LDS
    constexpr int KROW = HD*2 + APF_KLD, VROW = 64 + 8, KBLK = 32*KROW, VBLK = HDVP*VROW;
    constexpr int KTR = (32*CPR + NT - 1)/NT, VTR = VT ? (HDV*4 + NT - 1)/NT : KTR;
    static_assert(HD % 16 == 0 && HDV % 8 == 0, "S-product chunks of 16 dims; stores of 4 dims");
    static_assert(VT || (HDV == HD && KTR == 1 && NW == APF_NW), "row-major V: head size 64 / 128");
    extern __shared__ __attribute__((aligned(16))) char lds_all[];     // K: [2][KS][KBLK] | V^T: [2][KS][VBLK]
    char * const ldsk_base = lds_all, * const ldsv_base = lds_all + 2*KS*KBLK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ql = lane & 31, hf = lane >> 5;
    const int h = blockIdx.y*hpw + wave % hpw, hk = h/(p.n_head/p.n_head_kv);
    const int ks = KS > 1 ? (wave/hpw) & (KS - 1) : 0;                  // which of the iteration's blocks this wave multiplies
    const int q0 = (blockIdx.x*(NW/(hpw*KS)) + wave/(hpw*KS))*32;
    const bool active = q0 < p.T;                        // wave-uniform; an idle wave still stages and meets the barriers
    const int t = min(q0 + ql, p.T - 1);

    // Q^T as B operand: chunk c holds head dims 16c + 8 hf .. + 7 of query t, rounded to f16
    f16x8 qb[NC];
    {
        const char * qrow = p.q + (size_t) t*p.q_nb1 + (size_t) h*p.q_nb2;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const float4v a = *(const float4v *) (qrow + (size_t)(16*c + 8*hf)*4), b = *(const float4v *) (qrow + (size_t)(16*c + 8*hf + 4)*4);
            qb[c] = f16x8{ (_Float16) a.x, (_Float16) a.y, (_Float16) a.z, (_Float16) a.w, (_Float16) b.x, (_Float16) b.y, (_Float16) b.z, (_Float16) b.w };
        }
    }
    f32x16 o[NDT];
#pragma unroll
    for (int d = 0; d < NDT; d++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[d][r] = 0.0f;
    float m = -INFINITY, l = 0.0f;     // running maximum (common to both halves; base-2 domain) and this half's share of the denominator
    constexpr float LOG2E = 1.4426950408889634f;
    const float scale2 = p.scale*LOG2E;
    const float slope = p.max_bias > 0.0f ? (h < p.n_head_log2 ? powf(p.m0, (float)(h + 1)) : powf(p.m1, (float)(2*(h - p.n_head_log2) + 1))) : 1.0f;

    // staging roles, piece e = tid + trip*NT. K (and a row-major V): e -> (cell = e / CPR, 16-byte chunk); transposed V: e -> (dim row = e / 4, 8 cells)
    const char * kg[KTR]; const char * vg[VTR];
#pragma unroll
    for (int r = 0; r < KTR; r++) kg[r] = p.k + (size_t) hk*p.k_nb2 + (size_t)((tid + r*NT) % CPR)*16;
#pragma unroll
    for (int r = 0; r < VTR; r++) vg[r] = VT ? p.v + (size_t) hk*p.v_nb2 + (size_t) min((tid + r*NT) >> 2, HDV - 1)*p.v_nb1 + (size_t)(tid & 3)*16
                                             : p.v + (size_t) hk*p.v_nb2 + (size_t)(tid % CPR)*16;
    const char * mrow = MASK ? p.mask + (size_t) t*p.m_nb1 : nullptr;
    if constexpr (HDVP != HDV) {       // the output tiles' rows past V's size: zero, in every staging buffer, once
        constexpr int NZ = (HDVP - HDV)*VROW/8;
        for (int i = tid; i < 2*KS*NZ; i += NT) *(int2v *) (ldsv_base + (i / NZ)*VBLK + HDV*VROW + (i % NZ)*8) = int2v{ 0, 0 };
    }

    int4v kst[KS][KTR], vst[KS][VTR];  // the next iteration's K / V pieces
    int4v mst[4];                      // the next block's mask values of this lane (f16: .xy used)
    auto fetch = [&](int kv0) {        // kv0 = first cell of the iteration (KS blocks)
#pragma unroll
        for (int b = 0; b < KS; b++) {
            const int kvb = min(kv0 + 32*b, p.n_kv - 32);
#pragma unroll
            for (int r = 0; r < KTR; r++) {
                const int e = tid + r*NT, kcell = e / CPR;
                if (e < 32*CPR) kst[b][r] = *(const int4v *) (kg[r] + (size_t)(kvb + min(kcell, 31))*p.k_nb1);
            }
#pragma unroll
            for (int r = 0; r < VTR; r++) {
                const int e = tid + r*NT;
                if (VT ? e < HDV*4 : e < 32*CPR) vst[b][r] = VT ? *(const int4v *) (vg[r] + (size_t) kvb*2) : *(const int4v *) (vg[r] + (size_t)(kvb + min(e / CPR, 31))*p.v_nb1);
            }
        }
        const int kvc = min(kv0 + 32*ks, p.n_kv - 32);
        if (MASK == 2) {
#pragma unroll
            for (int j = 0; j < 4; j++) { const int2v raw = ld_b64(mrow + (size_t)(kvc + 8*j + 4*hf)*2); mst[j].x = raw.x; mst[j].y = raw.y; }
        } else if (MASK == 1) {
#pragma unroll
            for (int j = 0; j < 4; j++) mst[j] = ld_b128(mrow + (size_t)(kvc + 8*j + 4*hf)*4);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int b = 0; b < KS; b++) {
            char * lk = ldsk_base + (buf*KS + b)*KBLK, * lv = ldsv_base + (buf*KS + b)*VBLK;
#pragma unroll
            for (int r = 0; r < KTR; r++) {
                const int e = tid + r*NT, kcell = e / CPR, kch = e % CPR;
                if (e < 32*CPR) *(int4v *) (lk + kcell*KROW + kch*16) = kst[b][r];
            }
#pragma unroll
            for (int r = 0; r < VTR; r++) {
                const int e = tid + r*NT;
                if (VT) {
                    const int vrow = e >> 2, vch = e & 3;
                    if (e < HDV*4) {
                        *(int2v *) (lv + vrow*VROW + vch*16)     = int2v{ vst[b][r].x, vst[b][r].y };
                        *(int2v *) (lv + vrow*VROW + vch*16 + 8) = int2v{ vst[b][r].z, vst[b][r].w };
                    }
                } else if (e < 32*CPR) {        // transpose on the way in: 8 dims of one cell -> 8 rows of V^T
                    const int kcell = e / CPR, kch = e % CPR;
                    const uint32_t w[4] = { (uint32_t) vst[b][r].x, (uint32_t) vst[b][r].y, (uint32_t) vst[b][r].z, (uint32_t) vst[b][r].w };
#pragma unroll
                    for (int i = 0; i < 8; i++) *(uint16_t *) (lv + (kch*8 + i)*VROW + kcell*2) = (uint16_t)(w[i >> 1] >> (16*(i & 1)));
                }
            }
        }
    };

    fetch(0);
    stage(0);
    float mk[16];
    auto take_mask = [&]() {
        if (MASK == 2) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const f16x4 hv = __builtin_bit_cast(f16x4, int2v{ mst[j].x, mst[j].y });
                mk[4*j] = (float) hv[0]; mk[4*j + 1] = (float) hv[1]; mk[4*j + 2] = (float) hv[2]; mk[4*j + 3] = (float) hv[3];
            }
        } else if (MASK == 1) {
#pragma unroll
            for (int j = 0; j < 4; j++) { const float4v fv = __builtin_bit_cast(float4v, mst[j]); mk[4*j] = fv.x; mk[4*j + 1] = fv.y; mk[4*j + 2] = fv.z; mk[4*j + 3] = fv.w; }
        } else {
#pragma unroll
            for (int r = 0; r < 16; r++) mk[r] = 0.0f;
        }
    };
    take_mask();
    __syncthreads();

    for (int kv0 = 0, buf = 0; kv0 < p.n_kv; kv0 += 32*KS, buf ^= 1) {
        fetch(kv0 + 32*KS);            // clamped past the end: staged into a buffer nobody reads
        bool need = active && kv0 + 32*ks < p.n_kv;
        if (MASK && need) {
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; r++) mx = fmaxf(mx, mk[r]);
            need = __builtin_amdgcn_ballot_w64(mx != -INFINITY) != 0;       // wave-uniform
        }
        if (need) {
            // ---- S^T = K . Q^T ----
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; r++) s[r] = 0.0f;
            const char * kl = ldsk_base + (buf*KS + ks)*KBLK + ql*KROW + hf*16;
#pragma unroll
            for (int c = 0; c < NC; c++) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, *(const int4v *) (kl + c*32)), qb[c], s, 0, 0, 0);
            // ---- scale + mask; s[r] belongs to cell kv0 + (r & 3) + 8 (r >> 2) + 4 hf of query t. The softmax runs in the base-2 domain
            //      (scores times log2 e, v_exp_f32 is 2^x): one instruction per exponential instead of expf's six ----
            float bm = -INFINITY;
            if (p.softcap != 0.0f || p.max_bias > 0.0f) {
#pragma unroll
                for (int r = 0; r < 16; r++) { float x = s[r]*p.scale; if (p.softcap != 0.0f) x = p.softcap*tanhf(x); s[r] = (x + slope*mk[r])*LOG2E; bm = fmaxf(bm, s[r]); }
            } else
#pragma unroll
            for (int r = 0; r < 16; r++) { s[r] = s[r]*scale2 + mk[r]*LOG2E; bm = fmaxf(bm, s[r]); }
            bm = fmaxf(bm, xhalf(bm, lane));
            const float m_new = fmaxf(m, bm);
            const float alpha = m == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(m - m_new);     // m_new == -inf only while every cell so far was masked: p = 0
            float psum = 0.0f;
            float pr[16];
#pragma unroll
            for (int r = 0; r < 16; r++) { pr[r] = s[r] == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(s[r] - m_new); psum += pr[r]; }
            l = l*alpha + psum;
            m = m_new;
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {      // the running maximum settles early: most blocks rescale nothing
#pragma unroll
                for (int d = 0; d < NDT; d++)
#pragma unroll
                    for (int r = 0; r < 16; r++) o[d][r] *= alpha;
            }
            // ---- O^T += V^T . P^T: the k-slots of chunk c2 are the cells kv0 + 16 c2 + 8 (s >> 2) + 4 hf + (s & 3), s = 0..7 ----
#pragma unroll
            for (int c2 = 0; c2 < 2; c2++) {
                const f16x8 pb = { (_Float16) pr[8*c2 + 0], (_Float16) pr[8*c2 + 1], (_Float16) pr[8*c2 + 2], (_Float16) pr[8*c2 + 3],
                                   (_Float16) pr[8*c2 + 4], (_Float16) pr[8*c2 + 5], (_Float16) pr[8*c2 + 6], (_Float16) pr[8*c2 + 7] };
#pragma unroll
                for (int d = 0; d < NDT; d++) {
                    const char * vp = ldsv_base + (buf*KS + ks)*VBLK + (32*d + ql)*VROW + (16*c2 + 4*hf)*2;
                    const int2v lo = *(const int2v *) vp, hi = *(const int2v *) (vp + 16);
                    o[d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, int4v{ lo.x, lo.y, hi.x, hi.y }), pb, o[d], 0, 0, 0);
                }
            }
        }
        stage(buf ^ 1);                // last read before the previous barrier
        take_mask();
        __syncthreads();
    }
    if (KS > 1) {        // the waves of a (head, query tile) merge their states pairwise (KS = 4: 1 -> 0 and 3 -> 2, then 2 -> 0); the staging buffers are free: the loop's last barrier is behind us
        constexpr int PS = 16*NDT + 2;
        bool gone = false;
#pragma unroll
        for (int step = 1; step < KS; step <<= 1) {
            const bool give = !gone && (ks & (2*step - 1)) == step, take = !gone && (ks & (2*step - 1)) == 0;
            // the slot of the RECEIVING wave: (query tile of the workgroup, head, receiver's ks)
            const int rk = give ? ks - step : ks;
            float * part = (float *) lds_all + (size_t)((wave/(KS*hpw)*hpw + wave % hpw)*(KS/2) + rk/2)*PS*64 + lane;      // (receivers have even ks: KS/2 slots per (tile, head))
            if (give) {
#pragma unroll
                for (int d = 0; d < NDT; d++)
#pragma unroll
                    for (int r = 0; r < 16; r++) part[(16*d + r)*64] = o[d][r];
                part[(16*NDT)*64] = m; part[(16*NDT + 1)*64] = l;
                gone = true;
            }
            __syncthreads();
            if (take) {
                const float mw = part[(16*NDT)*64], lw = part[(16*NDT + 1)*64];
                const float m_new = fmaxf(m, mw);
                const float a = m == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(m - m_new), b = mw == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(mw - m_new);
                l = l*a + lw*b; m = m_new;
#pragma unroll
                for (int d = 0; d < NDT; d++)
#pragma unroll
                    for (int r = 0; r < 16; r++) o[d][r] = o[d][r]*a + part[(16*d + r)*64]*b;
            }
            if (step*2 < KS) __syncthreads();      // (the slots are written again in the next round)
        }
        if (gone) return;
    }
    if (!active) return;
    // ---- finish: both halves' denominators, the sink logit (src/llama-graph.cpp:1313), normalise, store ----
    float lt = l + xhalf(l, lane);
    float fin = 1.0f;
    if (p.sinks) {
        const float sk = p.sinks[h]*LOG2E;
        const float mf = fmaxf(m, sk);
        fin = m == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(m - mf);
        lt = lt*fin + __builtin_amdgcn_exp2f(sk - mf);
    }
    const float inv = fin/lt;
    if (q0 + ql < p.T) {
        float * orow = p.dst ? (float *) ((char *) p.dst + (size_t) t*p.dst_nb1) + (size_t) h*HDV : nullptr;
        uint16_t * yrow = p.y16 ? p.y16 + (size_t) t*p.kp16 + (size_t) h*HDV : nullptr;
#pragma unroll
        for (int d = 0; d < NDT; d++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (HDVP != HDV && 32*d + 8*j + 4*hf >= HDV) continue;      // a padded tile's dims
                const float4v ov = { o[d][4*j]*inv, o[d][4*j + 1]*inv, o[d][4*j + 2]*inv, o[d][4*j + 3]*inv };
                if (orow) *(float4v *) (orow + 32*d + 8*j + 4*hf) = ov;
                if (yrow) *(uint2 *) (yrow + 32*d + 8*j + 4*hf) = uint2{ pack_bf16(ov.x, ov.y), pack_bf16(ov.z, ov.w) };
            }
    }
}

// ---- the prefill launch, planned once (kernels.h: attn_call, attn_prefill_plan) ----
attn_prefill_plan attn_plan_prefill(const attn_call & c) {
    static const bool ks4_on = env_on("GGML_MI355X_ATTN_PF_KS4");
    attn_prefill_plan pl = {};
    pl.ok = c.q_type == T_F32 && c.k_type == T_F16 && c.v_type == T_F16 && c.n_kv % 32 == 0 && c.n_kv > 0 && c.n_head_kv > 0 && c.n_head % c.n_head_kv == 0 && attn_n_stream(c) <= 65535 &&
            (c.v_trans ? attn_fa_head_sizes(c.hsk, c.hsv, T_F16, T_F16) : c.hsv == c.hsk && (c.hsk == 64 || c.hsk == 128));
    if (!pl.ok) return pl;
    pl.nw = c.hsk > 128 ? 4 : APF_NW;                                       // waves per workgroup (the kernel's NW)
    const int64_t R = c.n_head/c.n_head_kv, T = c.T;
    pl.hpw = R % 8 == 0 && pl.nw >= 8 ? 8 : R % 4 == 0 ? 4 : R % 2 == 0 ? 2 : 1;          // heads of one kv head per workgroup
    // (the workgroup counts below are ONE stream's: a launch of several streams keeps the one-stream plan, and with it the one-stream launch's bits; whether the cell
    // split still pays once the streams fill the chip is not measured)
    // few workgroups (short prompts): the waves of a (head, query tile) split the cell blocks of an iteration two or four ways, shortening the loop that is the critical path
    const int64_t wgs1 = ((T + 32*(pl.nw/pl.hpw) - 1)/(32*(pl.nw/pl.hpw)))*(c.n_head/pl.hpw);
    pl.ks = (pl.hpw*2 <= pl.nw && pl.hpw <= 4 && wgs1 < 160 && c.n_kv >= 128) ? 2 : 1;
    if (ks4_on && pl.ks == 2 && R % 2 == 0 && c.n_kv >= 256 && c.hsk == 128 && c.v_trans) {
        // ... four ways with two heads per workgroup when even the pairs leave half the chip idle (pp512 of a 32-head model: 128 workgroups -> 256)
        const int64_t wgs2 = ((T + 32*(APF_NW/(pl.hpw*2)) - 1)/(32*(APF_NW/(pl.hpw*2))))*(c.n_head/pl.hpw);
        if (wgs2 < 200) { pl.hpw = 2; pl.ks = 4; }
    }
    const int qpw = pl.nw/(pl.hpw*pl.ks);                                            // query tiles per workgroup
    pl.grid = dim3((unsigned)((T + 32*qpw - 1)/(32*qpw)), (unsigned)(c.n_head/pl.hpw), (unsigned) attn_n_stream(c));
    return pl;
}

// One instantiation's launch. LDS: the staging buffers 2*KS*(32*(HDK*2 + 16) + HDVP*72), HDVP = HDV rounded up to 32 — 141 KB at 256 with KS = 2, of a CU's
// 160 KB; the wave pairs' merge at the end reuses them and is the larger of the two at 80 only: NW/2 receivers x (16*NDT + 2) floats x 64 lanes.
// KS = 4 exists for the transposed-V form at 128 only (the plan never asks for another).
template <int HD, bool VT, int MK, int KS, int HV, int NW>
static void apf_launch(const attn_pf_args & a, const attn_prefill_plan & pl, hipStream_t stream) {
    if constexpr (KS == 4 && !(HD == 128 && VT)) { fprintf(stderr, "attn_prefill: no four-way form at head size %d\n", HD); abort(); }
    else {
        constexpr size_t ndt = (HV + 31)/32, st = (size_t) 2*KS*(32*(HD*2 + APF_KLD) + ndt*32*(64 + 8)), mg = KS > 1 ? (size_t)(NW/2)*(16*ndt + 2)*256 : 0;
        constexpr size_t lds = st > mg ? st : mg;
        static_assert(lds <= (size_t) 160*1024, "a workgroup's LDS");
        MI_LDS_LIMIT_OR_DIE(lds, k_attn_prefill<HD, VT, MK, KS, HV, NW>);
        hipLaunchKernelGGL((k_attn_prefill<HD, VT, MK, KS, HV, NW>), pl.grid, dim3(64*NW), lds, stream, a, pl.hpw);
    }
}

void attn_prefill(const attn_call & c) {
    const attn_prefill_plan pl = attn_plan_prefill(c);
    if (!pl.ok) { fprintf(stderr, "attn_prefill: no kernel for head sizes (%lld, %lld), KV types (%d, %d), %lld cells\n", (long long) c.hsk, (long long) c.hsv, c.k_type, c.v_type, (long long) c.n_kv); abort(); }
    attn_pf_args a = {};
    a.q = (const char *) c.q; a.q_nb1 = c.q_nb1; a.q_nb2 = c.q_nb2;
    a.k = (const char *) c.k; a.k_nb1 = c.k_nb1; a.k_nb2 = c.k_nb2;
    a.v = (const char *) c.v; a.v_nb1 = c.v_nb1; a.v_nb2 = c.v_nb2;
    if (c.mask_type != T_NONE) { a.mask = (const char *) c.mask; a.m_nb1 = c.m_nb1; a.mask_f16 = c.mask_type == T_F16; }
    a.sinks = c.sinks; a.dst = c.dst; a.dst_nb1 = c.dst_nb1; a.y16 = c.y16; a.kp16 = (int)((c.hsv*c.n_head + 63) & ~(int64_t) 63);
    a.n_kv = (int) c.n_kv; a.n_head = (int) c.n_head; a.n_head_kv = (int) c.n_head_kv; a.T = (int) c.T;
    if (c.n_stream > 1) { a.q_nb3 = c.q_nb3; a.k_nb3 = c.k_nb3; a.v_nb3 = c.v_nb3; a.m_nb3 = c.m_nb3; a.dst_nb3 = c.dst_nb3; }
    attn_set_softmax(a, c);
    // the (hsk, hsv) pairs of attn_fa_head_sizes x the mask's kind (0 = none, 1 = f32, 2 = f16) x the plan's ks, one instantiation each
    attn_dispatch_sizes(c.hsk, c.hsv, [&](auto hk, auto hv) { dispatch_int<0, 1, 2>(c.mask_type == T_NONE ? 0 : c.mask_type == T_F16 ? 2 : 1, [&](auto mk) { dispatch_int<1, 2, 4>(pl.ks, [&](auto ks) {
        constexpr int HK = decltype(hk)::value, HV = decltype(hv)::value, MK = decltype(mk)::value, KS = decltype(ks)::value, NW = HK > 128 ? 4 : APF_NW;
        if (c.v_trans) apf_launch<HK, true, MK, KS, HV, NW>(a, pl, c.stream);
        else if constexpr (HK == HV && (HK == 64 || HK == 128)) apf_launch<HK, false, MK, KS, HV, NW>(a, pl, c.stream);
    }); }); });
}

// ---- the cache as the kernels above want it: f16, cells as rows or transposed (kv_types.h has the element types) ----
// n_heads = n_head_kv*n_stream rows of cells: head index hs = stream*n_head_kv + kv head, the order of the dense copy
struct kvc_args { const char * src; size_t nb1, nb2, nb3; int hd, n_kv, n_head_kv, n_heads; uint16_t * dst; };
static __device__ __forceinline__ const char * kvc_head(const kvc_args & p, int hs) { return p.src + (size_t)(hs % p.n_head_kv)*p.nb2 + (size_t)(hs / p.n_head_kv)*p.nb3; }
template <int TY>
__global__ void __launch_bounds__(256) k_kv_rows_f16(const kvc_args p) {
    const int c8 = p.hd >> 3;
    const long long e = (long long) blockIdx.x*256 + threadIdx.x, tot = (long long) p.n_heads*p.n_kv*c8;
    if (e >= tot) return;
    const int sub = (int)(e % c8); const long long cj = e / c8; const int j = (int)(cj % p.n_kv), hk = (int)(cj / p.n_kv);
    float f[8];
    kv_cvt8<TY>(kv_raw8<TY>(kvc_head(p, hk) + (size_t) j*p.nb1, sub), sub, f);
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = (uint32_t) f32_to_f16_bits(f[2*i]) | ((uint32_t) f32_to_f16_bits(f[2*i + 1]) << 16);
    *(int4v *) (p.dst + ((size_t) hk*p.n_kv + j)*p.hd + sub*8) = int4v{ (int) w[0], (int) w[1], (int) w[2], (int) w[3] };
}
// one workgroup = 64 cells of one kv head and a slab of up to 128 dims (blockIdx.z): cells are read as rows (coalesced), turned in LDS, written as 128-byte
// pieces of the rows over cells
template <int TY>
__global__ void __launch_bounds__(256) k_kv_trans_f16(const kvc_args p) {
    constexpr int LROW = 64 + 8;       // halves per LDS row (16-byte aligned rows)
    __shared__ __attribute__((aligned(16))) uint16_t tile[128*LROW];
    const int hk = blockIdx.y, j0 = blockIdx.x*64, d0 = blockIdx.z*128, c8 = min(p.hd - d0, 128) >> 3;      // c8: the slab's 8-dim chunks
    const char * src_h = kvc_head(p, hk);
    for (int e = threadIdx.x; e < 64*c8; e += 256) {
        const int cell = e / c8, sub = e % c8, j = min(j0 + cell, p.n_kv - 1);
        float f[8];
        kv_cvt8<TY>(kv_raw8<TY>(src_h + (size_t) j*p.nb1, (d0 >> 3) + sub), (d0 >> 3) + sub, f);
#pragma unroll
        for (int i = 0; i < 8; i++) tile[(sub*8 + i)*LROW + cell] = f32_to_f16_bits(f[i]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < c8*64; e += 256) {
        const int d = e >> 3, g8 = e & 7;
        if (j0 + g8*8 < p.n_kv) *(int4v *) (p.dst + ((size_t) hk*p.hd + d0 + d)*p.n_kv + j0 + g8*8) = *(const int4v *) (tile + d*LROW + g8*8);
    }
}
void kv_to_f16(int type, const void * src, size_t nb1, size_t nb2, size_t nb3, int64_t hd, int64_t n_kv, int64_t n_head_kv, int64_t n_stream, uint16_t * dst, bool transpose, hipStream_t stream) {
    const int64_t n_heads = n_head_kv*(n_stream > 1 ? n_stream : 1);
    if (hd % 8 || hd < 8 || hd > 256 || ((type == T_Q8_0 || type == T_Q4_0) && hd % 32) || n_kv % 8 || n_kv < 8 || n_heads > 65535) { fprintf(stderr, "kv_to_f16: unsupported shape (hd %lld, n_kv %lld)\n", (long long) hd, (long long) n_kv); abort(); }
    const kvc_args a = { (const char *) src, nb1, nb2, nb3, (int) hd, (int) n_kv, (int) n_head_kv, (int) n_heads, dst };
    const long long tot = (long long) n_heads*n_kv*(hd/8);
    if (!dispatch_int<T_F16, T_BF16, T_Q8_0, T_Q4_0>(type, [&](auto ty) {
            constexpr int TY = decltype(ty)::value;
            if (transpose) hipLaunchKernelGGL((k_kv_trans_f16<TY>), dim3((unsigned)((n_kv + 63)/64), (unsigned) n_heads, (unsigned)((hd + 127)/128)), dim3(256), 0, stream, a);
            else           hipLaunchKernelGGL((k_kv_rows_f16<TY>), dim3((unsigned)((tot + 255)/256)), dim3(256), 0, stream, a);
        })) { fprintf(stderr, "kv_to_f16: cache type %d is not supported\n", type); abort(); }
}

} // namespace mi355x
