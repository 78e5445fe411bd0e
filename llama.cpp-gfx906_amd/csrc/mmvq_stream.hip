// mmvq_stream.hip — host side of the streamed mat-vec (device code and the design: mmvq_stream.h): plans a grouped launch ONCE — may it take
// this path, how the workgroups (one per CU) are dealt to the groups in proportion to their weight bytes, the LDS carve and the slot ring —
// and launches a plan. Called by mul_mat_vec_q_fused (mmvq_fused.hip), which runs the register-ring kernels when the plan is not ok.
#include <hip/hip_ext.h>

#include "mmvq_stream.h"

#include <limits.h>
#include <string.h>
#include <algorithm>

namespace mi355x {

template <int TA, int TB, bool GLU> static void st_launch_t(const st_args & a, int blocks, size_t lds, hipStream_t stream, mmvq_launch_rec * rec) {
    static char name[64] = "";
    if (!name[0]) snprintf(name, sizeof(name), "k_mmvq_stream<%d, %d, true, %s>", TA, TB, GLU ? "true" : "false");
    if (rec) rec->kernel = name;
    MI_LDS_LIMIT_OR_DIE(MI_LDS_BUDGET, k_mmvq_stream<TA, TB, true, GLU>);
    if (rec && rec->e0) hipExtLaunchKernelGGL((k_mmvq_stream<TA, TB, true, GLU>), dim3((unsigned) blocks), dim3(ST_THREADS), lds, stream, rec->e0, rec->e1, 0, a);
    else hipLaunchKernelGGL((k_mmvq_stream<TA, TB, true, GLU>), dim3((unsigned) blocks), dim3(ST_THREADS), lds, stream, a);
}

// THE table of unit-type pairs (ta <= tb) that have a kernel — what is instantiated, what the planner admits and what the launcher calls. glu: the
// single-group gate/up instantiation (same-type rows only: a launch of one group has one type)
typedef void (*st_launch_fn)(const st_args &, int, size_t, hipStream_t, mmvq_launch_rec *);
struct st_pair { int ta, tb, ub_a, ub_b; st_launch_fn glu, plain; };
#define ST_SAME(T_)      { T_, T_, st_unit<T_>::UB, st_unit<T_>::UB, st_launch_t<T_, T_, true>, st_launch_t<T_, T_, false> }
#define ST_MIXED(A_, B_) { A_, B_, st_unit<A_>::UB, st_unit<B_>::UB, nullptr, st_launch_t<A_, B_, false> }
static const st_pair st_pairs[] = {
    ST_SAME(T_Q4_K), ST_SAME(T_Q5_K), ST_SAME(T_Q6_K), ST_SAME(ST_Q8_0_B10), ST_SAME(ST_MXFP4_B10), ST_SAME(T_Q4_0), ST_SAME(T_Q8_0), ST_SAME(T_Q5_0), ST_SAME(T_Q5_1), ST_SAME(T_Q3_K),
    ST_MIXED(T_Q8_0, T_Q4_K), ST_MIXED(T_Q8_0, T_Q6_K), ST_MIXED(T_Q4_K, T_Q5_K), ST_MIXED(T_Q4_K, T_Q6_K), ST_MIXED(T_Q5_K, T_Q6_K),
    ST_MIXED(T_Q3_K, T_Q4_K), ST_MIXED(T_Q3_K, T_Q5_K),      // (Q3_K_M / _L: wq and wk in Q3_K beside wv in Q4_K / Q5_K)
};
#undef ST_SAME
#undef ST_MIXED
static const st_pair * st_pair_of(int ta, int tb) {
    for (const st_pair & r : st_pairs) if (r.ta == ta && r.tb == tb) return &r;
    return nullptr;
}
bool mul_mat_vec_q_stream_has_pair(int type_a, int type_b) { return st_pair_of(std::min(type_a, type_b), std::max(type_a, type_b)) != nullptr; }
static int st_unit_bytes(int utype) { const st_pair * r = st_pair_of(utype, utype); return r ? r->ub_a : 0; }      // (every unit type has a same-type row)
// the unit a weight type is streamed in at row length k: 256 weights, or ten 32-blocks where k is not a multiple of 256 (gpt-oss: 2880); 0: none
static int st_utype(int type, int64_t k) {
    if (k % 256 == 0) return type == T_MXFP4 ? 0 : type;
    if (k % 320 == 0 && type == T_Q8_0) return ST_Q8_0_B10;
    if (k % 320 == 0 && type == T_MXFP4) return ST_MXFP4_B10;
    return 0;
}

#ifdef MI_STAMPS
static unsigned long long * g_st_stamps = nullptr; static int g_st_slots = 0, g_st_next = 0;
struct st_stamp_meta { int blocks, k, rows, type_a, type_b, mode, glu; long long bytes; };
static st_stamp_meta g_st_meta[4096];
extern "C" int mi355x_stream_stamps_enable(int n_slots) {
    if (g_st_stamps) { (void) hipFree(g_st_stamps); g_st_stamps = nullptr; }
    g_st_slots = n_slots > 4096 ? 4096 : n_slots; g_st_next = 0;
    if (g_st_slots <= 0) return 0;
    const size_t bytes = (size_t) g_st_slots*256*(ST_NC + 1)*ST_NSTAMP*8;
    if (hipMalloc(&g_st_stamps, bytes) != hipSuccess) return -1;
    (void) hipMemset(g_st_stamps, 0, bytes);
    return 0;
}
extern "C" int mi355x_stream_stamps_used(void) { return g_st_next; }
extern "C" int mi355x_stream_stamps_read(int slot, unsigned long long * out, int * meta, long long * bytes) {
    if (!g_st_stamps || slot < 0 || slot >= g_st_slots) return -1;
    const st_stamp_meta & m = g_st_meta[slot];
    (void) hipMemcpy(out, g_st_stamps + (size_t) slot*256*(ST_NC + 1)*ST_NSTAMP, (size_t) 256*(ST_NC + 1)*ST_NSTAMP*8, hipMemcpyDeviceToHost);
    meta[0] = m.blocks; meta[1] = m.k; meta[2] = m.rows; meta[3] = m.type_a; meta[4] = m.type_b; meta[5] = m.mode; meta[6] = m.glu;
    *bytes = m.bytes;
    return 0;
}
#endif

bool mul_mat_vec_q_stream_enabled(void) {
    static const bool on = env_on("GGML_MI355X_STREAM");
    return on;
}

bool mul_mat_vec_q_stream_takes(const mmvq_group * groups, int n_groups, int64_t k, const mmvq_input & in, const mmvq_rope * rope) {
    return mul_mat_vec_q_stream_plan(groups, n_groups, k, in, rope).ok;
}

// plans one grouped launch (mmvq_stream.h: st_plan). Not ok — a shape, alignment or epilogue the kernel does not do, two unit types without a kernel of
// their own, no room in the LDS for a ring of two slots — and the register-ring kernels (mmvq_fused.hip) take the launch
st_plan mul_mat_vec_q_stream_plan(const mmvq_group * groups, int n_groups, int64_t k, const mmvq_input & in, const mmvq_rope * rope) {
    st_plan P = {};
    // ---- may it? ----
    if (!mul_mat_vec_q_stream_enabled() || n_groups < 1 || n_groups > MMVQ_MAX_GROUPS) return P;
    if ((k % 256 != 0 && k % 320 != 0) || k > 16384 || k < 256) return P;
    const bool b10 = k % 256 != 0;         // ten-block units (Q8_0 / MXFP4 rows of 320 n weights)
    if (b10 && in.mode == PRO_Q8) return P;
    if (in.mode != PRO_Q8 && in.mode != PRO_QUANT && in.mode != PRO_NORM) return P;
    if (in.mode == PRO_Q8 && in.act_kind != T_Q8_K) return P;      // (a ready-made image: Q8_K only; the launch's own prologue quantizes per workgroup, in the format its group's weights ask for)
    if (in.mode == PRO_Q8) { if (((uintptr_t) in.act.qs % 16) || ((uintptr_t) in.act.bsums % 16) || !in.act.d) return P; }
    else { if ((!in.x && !(in.planes && in.pl_probs)) || ((uintptr_t) in.x % 16) || (in.mode == PRO_NORM && ((uintptr_t) in.norm_w % 16))) return P; }
    const int nb = (int)(b10 ? k/320 : k/256);
    if (in.planes && (in.mode != PRO_NORM || (k + 255)/256 > 16 || !in.pl_probs || in.n_planes < 1 || in.n_planes > 8 || !in.x_out || ((uintptr_t) in.planes % 16) || in.plane_stride % 4 || ((uintptr_t) in.x_out % 16))) return P;
    int ut[MMVQ_MAX_GROUPS], ub[MMVQ_MAX_GROUPS];      // the groups' unit types and unit bytes
    int ta = -1, tb = -1;
    for (int i = 0; i < n_groups; i++) {
        const mmvq_group & g = groups[i];
        ut[i] = st_utype(g.type, k); ub[i] = st_unit_bytes(ut[i]);
        if (!ub[i] || (act_kind_for(g.type) == T_Q8_0 && in.mode == PRO_Q8)) return P;      // (units of a Q8_0-activation format read the Q8_0 image only the launch's own prologue builds)
        if (ut[i] != ta && ut[i] != tb) { if (ta < 0) ta = ut[i]; else if (tb < 0) tb = ut[i]; else return P; }
        if (b10 && tb >= 0) return P;                              // (one kernel per ten-block format: no mixed launches)
        if ((g.b_gate != nullptr) != (g.b_up != nullptr) || (g.b_gate && (g.epi != EPI_GLU || !g.eid)) || (g.res_eid && (g.epi != EPI_ADD || !g.eid))) return P;
        if (g.eid && (g.estride % 16 || in.mode == PRO_NORM)) return P;
        if (g.x_off && (in.mode == PRO_Q8 || g.x_off % 4)) return P;
        if (g.row_stride != (size_t) nb*ub[i] || ((uintptr_t) g.W % 16) || (g.W2 && ((uintptr_t) g.W2 % 16))) return P;
        if (g.epi == EPI_GLU && !g.W2) return P;
        if (g.epi == EPI_ROPE) {
            if (!rope || !rope->table || (g.m & 1)) return P;
            if (rope->p.mode & 2) { const int hd = rope->head_dim; if (hd <= 0 || (hd & (hd - 1)) || rope->p.n_dims != hd || g.m % hd) return P; }
            else if (rope->p.mode != 0) return P;
        }
        if (g.epi == EPI_ADD && !g.res) return P;
        if (g.m < 1 || (int64_t) 256*g.m >= (1ll << 31)) return P;      // (the kernel deals rows with 32-bit arithmetic: workgroups x row units)
    }
    if (tb < 0) tb = ta;
    if (tb < ta) std::swap(ta, tb);
    P.glu = n_groups == 1 && groups[0].epi == EPI_GLU;
    const st_pair * pair = st_pair_of(ta, tb);
    if (!pair || !(P.glu ? pair->glu : pair->plain)) return P;
    P.ta = ta; P.tb = tb;

    // ---- the argument block ----
    st_args & a = P.a;
    a.n_groups = n_groups; a.k = (int) k; a.nb = nb; a.mode = in.mode; a.eps = in.eps;
    a.nchunk = (int)((k + 255)/256); a.act_stride = !b10 ? ST_ACT_STRIDE : ut[0] == ST_MXFP4_B10 ? ST_ACT_STRIDE_FP4 : ST_ACT_STRIDE_B10;
    a.magic = nb == 1 ? 0u : (uint32_t)((0x100000000ull + nb - 1)/nb);
    a.x = in.x; a.norm_w = in.norm_w;
    a.planes = in.planes; a.n_planes = in.n_planes; a.plane_stride = in.plane_stride; a.x_out = in.x_out;
    a.pl_probs = in.pl_probs; a.pl_ids = in.pl_ids; a.pl_mode = in.pl_mode;
    // (measured, tg128 on one box, `profiles/r04_stream_early_sweep.log`: 0 slots 588.4 tok/s, 1 slot 616.5, 2 slots 613.9, 4 slots 603.3)
    // (not kept: one batch of scalar loads over the whole 928-byte argument block at entry, so that the compiler's ~9 dependent s_loads before the first vector load
    // hit the scalar cache — same box, alternating: 604 / 600 tok/s with the batch, 617 / 617 without: the chain was not missing)
    { static const int early = (int) env_int("GGML_MI355X_STREAM_EARLY", 1);
      static const bool q16 = env_on("GGML_MI355X_STREAM_Q16"), touch = env_on("GGML_MI355X_STREAM_XTOUCH");
      a.early = (early & 0xFF) | (q16 ? 0 : 0x100) | (touch ? 0 : 0x200); }
    if (in.mode == PRO_Q8) { a.a_qs = in.act.qs; a.a_d = in.act.d; a.a_bs = in.act.bsums; }
    if (rope) a.rope = make_fused_rope(*rope);

    // workgroups per group: in proportion to the weight bytes, at least one each, never more than the group has row units
    const int budget = device_cu_count();
    double gbytes[MMVQ_MAX_GROUPS];
    for (int i = 0; i < n_groups; i++) {
        gbytes[i] = (double) groups[i].m*nb*ub[i]*(groups[i].epi == EPI_GLU ? 2 : 1);
        P.bytes_total += gbytes[i];
    }
    for (int i = 0; i < MMVQ_MAX_GROUPS; i++) a.block_end[i] = INT_MAX;
    int share[MMVQ_MAX_GROUPS], used = 0;
    for (int i = 0; i < n_groups; i++) {
        const mmvq_group & g = groups[i];
        st_group & s = a.g[i];
        s.W = g.W; s.W2 = g.W2; s.dst = g.dst; s.res = g.res; s.res2 = g.res2; s.st16 = g.st16; s.st_idx = g.st_idx; s.st_row_elems = g.st_row_elems;
        s.m = g.m; s.type = ut[i]; s.epi = g.epi; s.st_mode = g.st_mode; s.glu_alpha = g.glu_alpha; s.glu_limit = g.glu_limit;
        s.eid = g.eid; s.estride = (long long) g.estride; s.x_off = g.x_off;
        s.b_gate = g.b_gate; s.b_up = g.b_up; s.res_eid = g.res_eid;
        s.ralign = 1; s.neox2 = 0; s.neox_hh = 0;
        if (g.epi == EPI_ROPE) s.ralign = (rope->p.mode & 2) ? rope->head_dim : 2;
        while (((int64_t) s.ralign*nb*ub[i]) % 16 != 0) s.ralign *= 2;      // a workgroup's rows start on a 16-byte boundary (LDS-DMA source)
        const int nru = std::max(1, g.m/s.ralign);
        int sh = (int)((double) budget*gbytes[i]/P.bytes_total);
        sh = sh < 1 ? 1 : (sh > nru ? nru : sh);
        share[i] = sh; used += sh;
    }
    // NEOX groups as two row streams (mmvq_stream.h: st_group::neox2): the smallest number of pairs per workgroup c for which every such group gets EXACTLY m/2/c
    // workgroups and the launch still fits the chip; the other groups share what is left
    static const bool neox2_on = env_on("GGML_MI355X_NEOX2");
    if (neox2_on && rope && (rope->p.mode & 2) && rope->head_dim >= 16) {
        const int hh = rope->head_dim/2;
        for (int c = 4; c < hh; c *= 2) {
            int fixed = 0, others = 0; bool ok = hh % c == 0;
            for (int i = 0; i < n_groups && ok; i++) {
                if (groups[i].epi == EPI_ROPE) { ok = (groups[i].m/2) % c == 0 && ((int64_t) c*nb*ub[i]) % 16 == 0 && ((int64_t) hh*nb*ub[i]) % 16 == 0 && !groups[i].eid; fixed += groups[i].m/2/c; }
                else others++;
            }
            if (!ok || fixed + others > budget) continue;
            double obytes = 0; for (int i = 0; i < n_groups; i++) if (groups[i].epi != EPI_ROPE) obytes += gbytes[i];
            used = 0;
            for (int i = 0; i < n_groups; i++) {
                st_group & s = a.g[i];
                if (groups[i].epi == EPI_ROPE) { s.neox2 = c; s.neox_hh = hh; s.ralign = c; s.W2 = s.W + (size_t) hh*nb*ub[i]; share[i] = groups[i].m/2/c; }
                else { const int nru = std::max(1, groups[i].m/s.ralign); int sh = (int)((double)(budget - fixed)*gbytes[i]/obytes); share[i] = sh < 1 ? 1 : (sh > nru ? nru : sh); }
                used += share[i];
            }
            break;
        }
    }
    // hand the workgroups rounding left over to the groups with the most bytes per workgroup
    while (used < budget) {
        int best = -1; double bw = 0;
        for (int i = 0; i < n_groups; i++) { const int nru = std::max(1, groups[i].m/a.g[i].ralign); if (!a.g[i].neox2 && share[i] < nru && gbytes[i]/share[i] > bw) { bw = gbytes[i]/share[i]; best = i; } }
        if (best < 0) break;
        share[best]++; used++;
    }
    // ---- the LDS: what every workgroup carves besides the ring (fixed), a ring slot, the slots the busiest workgroup streams ----
    size_t fixed_max = 0; int slot_max = 0, nslots_max = 0;
    for (int i = 0; i < n_groups; i++) {
        const mmvq_group & g = groups[i];
        st_group & s = a.g[i];
        const int nru = std::max(1, g.m/s.ralign), sh = share[i];
        const int Rmax = s.neox2 ? s.neox2 : ((nru + sh - 1)/sh)*s.ralign + (g.m - (g.m/s.ralign)*s.ralign);
        const bool row16 = (nb & 15) == 0;
        const int streams = (g.epi == EPI_GLU || s.neox2) ? 2 : 1;
        s.npart_max = (row16 ? Rmax*(nb >> 4) : Rmax*nb)*streams;
        const size_t fixed = 2*ST_SYNC_WORDS*4 + (size_t) nb*a.act_stride + (size_t)((nb + 3) & ~3)*4 + 64 + (size_t) s.npart_max*4 + 16;
        fixed_max = std::max(fixed_max, fixed);
        slot_max = std::max(slot_max, ((64*ub[i] + 1023)/1024)*1024);
        nslots_max = std::max(nslots_max, (int)(((int64_t) Rmax*nb + 63)/64)*streams);
        P.blocks += sh;
        a.block_end[i] = P.blocks;
    }
    // the carve must leave room for a ring of at least two slots (rows whose block count is not a multiple of 16 keep one partial sum per unit: a
    // workgroup with many such rows can fill the LDS with them)
    const int need = std::min(nslots_max, 2);
    int64_t S = fixed_max < (size_t) MI_LDS_BUDGET ? (MI_LDS_BUDGET - (int64_t) fixed_max)/slot_max : 0;
    if (S < need) return P;
    static const int ring_env = (int) env_int("GGML_MI355X_STREAM_RING", 0);
    S = std::min<int64_t>(S, std::min(nslots_max, ST_MAX_RING));
    if (ring_env > 0) S = std::min<int64_t>(S, std::max(ring_env, need));
    P.S = a.S = (int) S;
    P.lds = fixed_max + (size_t) S*slot_max;
    // experiment knob: launches that stream fewer bytes than this go to the register-ring kernel (is the streamed kernel's envelope a loss on the small launches?)
    static const double min_bytes = env_double("GGML_MI355X_STREAM_MIN_MB", 0.0)*1e6;
    if (min_bytes > 0.0 && P.bytes_total < min_bytes && !in.planes && !b10) {
        for (int i = 0; i < n_groups; i++) if (groups[i].eid || groups[i].epi == EPI_GLU || (groups[i].epi == EPI_ROPE && rope && (rope->p.mode & 2))) P.ok = true;
        return P;
    }
    P.ok = true;
    return P;
}

void mul_mat_vec_q_stream(const st_plan & plan, hipStream_t stream, mmvq_launch_rec * rec) {
#ifdef MI_STAMPS
    st_args a = plan.a;
    a.stamps = nullptr;
    if (g_st_stamps && g_st_next < g_st_slots && plan.blocks <= 256) {
        st_stamp_meta & sm = g_st_meta[g_st_next];
        sm.blocks = plan.blocks; sm.k = a.k; sm.rows = 0; for (int i = 0; i < a.n_groups; i++) sm.rows += a.g[i].m*(a.g[i].epi == EPI_GLU ? 2 : 1);
        sm.type_a = plan.ta; sm.type_b = plan.tb; sm.mode = a.mode; sm.glu = a.g[0].epi == EPI_GLU; sm.bytes = (long long) plan.bytes_total;
        a.stamps = g_st_stamps + (size_t) g_st_next*256*(ST_NC + 1)*ST_NSTAMP;
        g_st_next++;
    }
#else
    const st_args & a = plan.a;
#endif
    const st_pair * pair = st_pair_of(plan.ta, plan.tb);
    (plan.glu ? pair->glu : pair->plain)(a, plan.blocks, plan.lds, stream, rec);
}

} // namespace mi355x
