// backend_nodes.cpp — running one graph node (or the group of nodes a fusion takes) during a pass: the pass state's operations, the op
// launchers, the fusion matchers and compute_node, which dispatches between them. The pass itself is run_nodes' (backend_graph.cpp).
#include "backend_impl.h"

// ---- the pass state (mi_pass, backend_impl.h) ----------------------------------------------------------------------
void mi_pass::begin(const struct ggml_cgraph * g, bool count_uses) {
    rope_valid = false;      // every pass over a graph (eager or under capture) fills the token's rotation table itself
    aq.valid = false;
    uses.clear();
    if (count_uses) {
        for (int i = 0; i < g->n_nodes; i++) {
            for (int s = 0; s < GGML_MAX_SRC; s++) if (g->nodes[i]->src[s]) uses[g->nodes[i]->src[s]]++;
        }
    }
    pp.active = false; rt.valid = false;
}

void mi_pass::note_writes(const struct ggml_cgraph * g, int i, int n) {
    for (int j = i; j < i + n; j++) {
        const struct ggml_tensor * w = g->nodes[j];
        // any write into the memory the cached activations were made from ends them, unless it is their producer's own
        if (aq.valid && (j < aq.lo || j > aq.hi) && w->data && ranges_overlap(w->data, ggml_nbytes(w), aq.data, aq.span)) aq.valid = false;
        // ... and into what the last fused router ranked, unless it is that router's own node
        if (rt.valid && (j < rt.lo || j > rt.hi) && w->data &&
            (ranges_overlap(w->data, ggml_nbytes(w), rt.vals, rt.bytes) || ranges_overlap(w->data, ggml_nbytes(w), rt.sorted, rt.bytes))) rt.valid = false;
    }
}

// the pending MoE combine is needed as a tensor after all (its reader is not the launch that would have evaluated it itself)
static void pp_flush(mi_backend_ctx * c) {
    auto & pp = c->pass.pp;
    if (!pp.active) return;
    moe_combine(pp.probs, pp.ids, pp.n_planes, pp.mode, pp.planes, (size_t) pp.stride*4, pp.m, pp.res, pp.x_out, c->stream);
    c->cnt.kernels_launched++;
    pp.active = false;
}

void pass_end(mi_backend_ctx * c) {
    pp_flush(c);
    c->pass.drop_act();
}

// FLASH_ATTN_EXT as its kernels get it: the dense f16 copies they need (kv_to_f16 into kv16, K first and V behind it) — the V cache transposed for the matrix-core
// prefill kernel (always: rows over cells are what it stages with coalesced loads), K when it is not f16; for a few tokens only what the decode kernel does not read
// directly (attn_decode_kv_types_fused) — and the launch's operands after them. ok: the cache's types have kernels at these head sizes and the launch has a plan
// with the partial buffer on offer. kv16 may be NULL (supports_op, sizing kv16: nothing is launched from the result). Per-sequence KV streams (ne[3] of q, K and V):
// one call for all of them; the copies hold every stream, each dense behind the previous one.
fa_operands fa_kv16_plan(const struct ggml_tensor * n, void * kv16, float * part, size_t part_bytes) {
    const struct ggml_tensor * q = n->src[0]; const struct ggml_tensor * k = n->src[1]; const struct ggml_tensor * v = n->src[2];
    const struct ggml_tensor * mask = n->src[3]; const struct ggml_tensor * sinks = n->src[4];
    fa_operands p = {};
    attn_call & a = p.call;
    a.hsk = k->ne[0]; a.hsv = v->ne[0]; a.n_kv = k->ne[1]; a.n_head = q->ne[2]; a.n_head_kv = k->ne[2]; a.T = q->ne[1];
    a.q = q->data; a.q_nb1 = q->nb[1]; a.q_nb2 = q->nb[2]; a.q_type = (int) q->type;
    a.k = k->data; a.k_nb1 = k->nb[1]; a.k_nb2 = k->nb[2]; a.k_type = (int) k->type;
    a.v = v->data; a.v_nb1 = v->nb[1]; a.v_nb2 = v->nb[2]; a.v_type = (int) v->type;
    if (mask) { a.mask = mask->data; a.m_nb1 = mask->nb[1]; a.mask_type = (int) mask->type; }
    a.sinks = sinks ? (const float *) sinks->data : nullptr; a.dst = (float *) n->data; a.dst_nb1 = n->nb[2];
    a.scale = op_f32(n, 0); a.max_bias = op_f32(n, 1); a.softcap = op_f32(n, 2);
    a.part = part; a.part_bytes = part_bytes;
    a.n_stream = q->ne[3]; a.q_nb3 = q->nb[3]; a.k_nb3 = k->nb[3]; a.v_nb3 = v->nb[3]; a.m_nb3 = mask && mask->ne[3] > 1 ? mask->nb[3] : 0; a.dst_nb3 = n->nb[3];
    const size_t S = (size_t) attn_n_stream(a);
    const bool prefill = a.T > 8, direct = !prefill && attn_decode_kv_types_fused(a.k_type, a.v_type);
    if (!direct && k->type != GGML_TYPE_F16) {
        p.k_bytes = (((size_t) a.hsk*a.n_kv*a.n_head_kv*2*S) + 255) & ~(size_t) 255;
        a.k = kv16; a.k_nb1 = (size_t) a.hsk*2; a.k_nb2 = (size_t) a.n_kv*a.hsk*2; a.k_nb3 = a.k_nb2*a.n_head_kv; a.k_type = T_F16;
    }
    if (!direct && (prefill || v->type != GGML_TYPE_F16)) {
        p.v_bytes = (((size_t) a.hsv*a.n_kv*a.n_head_kv*2*S) + 255) & ~(size_t) 255;
        a.v = kv16 ? (char *) kv16 + p.k_bytes : nullptr; a.v_type = T_F16; a.v_trans = prefill;
        a.v_nb1 = (size_t)(prefill ? a.n_kv : a.hsv)*2; a.v_nb2 = (size_t) a.hsv*a.n_kv*2; a.v_nb3 = a.v_nb2*a.n_head_kv;
    }
    p.ok = attn_fa_head_sizes(a.hsk, a.hsv, (int) k->type, (int) v->type) && attn_supported(a) && (size_t) a.n_head_kv*S <= 65535;      // (kv_to_f16: a grid row per (stream, kv head))
    return p;
}

// quantize (or reuse) the activations of a quantized mat-mul: rows r -> x + (r % n_inner)*s_inner + (r / n_inner)*s_outer
static act_q8 get_act(mi_backend_ctx * c, const void * x, int64_t k, int64_t n_inner, int64_t n_outer, size_t s_inner, size_t s_outer, int kind) {
    if (const act_q8 * have = c->pass.q8_of(x, k, n_inner, n_outer, s_inner, s_outer, kind)) {
        c->cnt.act_quant_reused++;
        return *have;
    }
    act_q8 q = act_q8_carve(c->scratch, kind, k, n_inner*n_outer);
    quantize_act((const float *) x, n_inner, s_inner, s_outer, q, c->stream);
    c->cnt.act_quant_launches++; c->cnt.kernels_launched++;
    c->pass.converted_q8(x, k, n_inner, n_outer, s_inner, s_outer, kind, q);
    return q;
}

// F16 activations of a quantized mat-mul (tests/test-backend-ops.cpp:5715-5716): a dense F32 copy in c->cvt first (the CPU backend converts src1 to the
// weights' vec_dot type row by row as well), then the F32 path reads `tmp`, the copy's descriptor
static const struct ggml_tensor * f16_src1_to_f32(mi_backend_ctx * c, const struct ggml_tensor * b, struct ggml_tensor & tmp) {
    tmp = *b; tmp.type = GGML_TYPE_F32; tmp.data = c->cvt;
    tmp.nb[0] = 4; tmp.nb[1] = (size_t) b->ne[0]*4; tmp.nb[2] = tmp.nb[1]*b->ne[1]; tmp.nb[3] = tmp.nb[2]*b->ne[2];
    cpy(desc(b), desc(&tmp), c->stream);
    c->cnt.kernels_launched++;
    c->pass.drop_act();
    return &tmp;
}

// out/res: the prefill residual fusion (try_fused_prefill_add) writes W.x + res into `out` instead of W.x into dst
static void op_mul_mat(mi_backend_ctx * c, struct ggml_tensor * dst, struct ggml_tensor * out = nullptr, const struct ggml_tensor * res = nullptr, mmq_deferred * defer = nullptr) {
    const struct ggml_tensor * a = dst->src[0];
    const struct ggml_tensor * b = dst->src[1];
    struct ggml_tensor b32;
    if (ggml_is_quantized(a->type) && b->type == GGML_TYPE_F16) b = f16_src1_to_f32(c, b, b32);
    if (ggml_is_quantized(a->type)) {
        const int kind = act_kind_for((int) a->type);
        const int64_t K = a->ne[0], M = a->ne[1], N = b->ne[1];
        const int64_t r2 = b->ne[2]/a->ne[2], r3 = b->ne[3]/a->ne[3];
        // few columns x several batches (the K.q product over a quantized K cache: one batch per head): ONE launch, blockIdx.y = batch
        if (N <= MMVQ_MAX_N && b->ne[2] > 1 && b->ne[3] == 1 && a->ne[3] == 1 && act_q8_bytes(kind, K, N*b->ne[2]) <= c->scratch_size) {
            const act_q8 q = get_act(c, b->data, K, N, b->ne[2], b->nb[1], b->nb[2], kind);
            prof_begin(c, (int) a->type, M, K, N, (uint64_t) a->ne[2]*M*ggml_row_size(a->type, K));
            mul_mat_vec_q_batched((int) a->type, a->data, a->nb[1], a->nb[2], (int) r2, M, K, q, N, b->ne[2], (float *) dst->data, dst->nb[1], dst->nb[2], c->stream);
            prof_end(c);
            c->cnt.mmvq_launches++; c->cnt.kernels_launched++;
            c->cnt.weight_bytes += (uint64_t) a->ne[2]*M*ggml_row_size(a->type, K);
            return;
        }
        for (int64_t i13 = 0; i13 < b->ne[3]; i13++) {
            for (int64_t i12 = 0; i12 < b->ne[2]; i12++) {
                const char * bp = (const char *) b->data + i12*b->nb[2] + i13*b->nb[3];
                const char * W = (const char *) a->data + (i12/r2)*a->nb[2] + (i13/r3)*a->nb[3];
                float * d = (float *) ((char *) dst->data + i12*dst->nb[2] + i13*dst->nb[3]);
                prof_begin(c, (int) a->type, M, K, N, (uint64_t) M*ggml_row_size(a->type, K));
                if (N <= MMVQ_MAX_N) {
                    const act_q8 q = get_act(c, bp, K, N, 1, b->nb[1], 0, kind);
                    mul_mat_vec_q((int) a->type, W, a->nb[1], M, K, q, N, d, dst->nb[1], c->stream);
                    c->cnt.mmvq_launches++;
                } else {
                    // the scratch holds the bf16 copy of the activations; wq/wk/wv and gate/up read the same ones: convert once
                    const size_t at = c->pass.bf16_at(bp, K, N, b->nb[1]);      // (at any offset: a producer may have left it above its own)
                    const bool ready = at != mi_pass::NO_ACT;
                    const size_t off = ready ? at : 0;
                    mmq_call mc = {};
                    mc.type = (int) a->type; mc.W = W; mc.w_row_stride = a->nb[1]; mc.m = M; mc.stream = c->stream;
                    mc.act = { (const float *) bp, b->nb[1], K, N, (char *) c->scratch + off, c->scratch_size - off, ready };
                    mc.dst = out ? (float *) out->data : d; mc.dst_stride = out ? out->nb[1] : dst->nb[1];
                    if (out) { mc.defer = defer; mc.res = (const float *) res->data; mc.res_stride = res->ne[1] == 1 && N > 1 ? 0 : res->nb[1]; }     // (a bias row: the same addend for every token)
                    mul_mat_q(mc);
                    if (ready) c->cnt.act_quant_reused++;
                    else c->pass.converted_bf16(bp, K, N, b->nb[1]);
                    if (defer) defer->planes_off += off;      // (mul_mat_q counted from `scr`; now from the start of the scratch)
                    c->cnt.mmq_launches++; c->cnt.kernels_launched += ready ? 0 : 1;
                }
                prof_end(c);
                c->cnt.kernels_launched++;
                c->cnt.weight_bytes += (uint64_t) M*ggml_row_size(a->type, K);
            }
        }
        return;
    }
    const mm_dense_args p = mm_dense_args_of(dst);
    int launches = 0;
    switch (mul_mat_dense(p, c->scratch, c->scratch_size, c->stream, &launches)) {
        case MM_DENSE_MFMA:      c->pass.drop_act(); c->cnt.dense_mfma++; break;      // (the scratch was reused)
        case MM_DENSE_F16_PAIRS: c->cnt.dense_f16_pairs++; break;
        case MM_DENSE_F32_VEC:   c->cnt.dense_f32_vec++; break;
        case MM_DENSE_F32_ROWS:  c->cnt.dense_f32_rows++; break;
        case MM_DENSE_GENERIC:   c->cnt.dense_generic++; break;
    }
    c->cnt.kernels_launched += (uint64_t) launches;
}

// MUL_MAT on a row-split weight: the main device quantizes the activations once (few tokens) and runs its own slice; every other device that holds
// rows runs the same kernel on its slice on its own stream, reading the activations from and writing its rows of dst into the main device's
// memory through the peer mapping. Order: peers start after everything the main stream has queued so far (split_ready), the main stream
// continues after every peer's launch has finished (peer.done) — so dst is complete, and the scratch the peers read is not reused early.
static void op_mul_mat_split(mi_backend_ctx * c, struct ggml_tensor * dst) {
    const struct ggml_tensor * a = dst->src[0];
    const struct ggml_tensor * b = dst->src[1];
    struct ggml_tensor b32;
    if (b->type == GGML_TYPE_F16) b = f16_src1_to_f32(c, b, b32);      // (converted on the main device: the peers read it from there, as they read F32 activations)
    const mi_split_tensor * e = (const mi_split_tensor *) a->extra;
    const int kind = act_kind_for((int) a->type);
    const int64_t K = a->ne[0], N = b->ne[1];
    const bool few = N <= MMVQ_MAX_N;
    act_q8 q = {};
    if (few) q = get_act(c, b->data, K, N, 1, b->nb[1], 0, kind);
    else c->pass.drop_act();
    if (!c->split_ready) MI_CHECK_G(hipEventCreateWithFlags(&c->split_ready, hipEventDisableTiming));
    MI_CHECK_G(hipEventRecord(c->split_ready, c->stream));
    const size_t need = c->scratch_size;
    bool waited[GGML_MI355X_MAX_DEVICES] = {};
    for (int i = 0; i < G().n_devices; i++) {
        const int64_t rows = e->row_lo[i + 1] - e->row_lo[i];
        if (rows == 0) continue;
        float * d = (float *) dst->data + e->row_lo[i];
        const bool local = i == c->dev_index;
        hipStream_t st = c->stream; void * scr = c->scratch;
        if (!local) {
            mi_backend_ctx::split_peer & pr = c->peers[i];
            set_device(G().devices[i].id);
            if (!pr.stream) { MI_CHECK_G(hipStreamCreateWithFlags(&pr.stream, hipStreamNonBlocking)); MI_CHECK_G(hipEventCreateWithFlags(&pr.done, hipEventDisableTiming)); }
            if (!few && pr.scratch_size < need) {
                MI_CHECK_G(hipStreamSynchronize(pr.stream));
                if (pr.scratch) MI_CHECK_G(hipFree(pr.scratch));
                pr.scratch = nullptr; pr.scratch_size = 0;
                MI_CHECK_G(hipMalloc(&pr.scratch, need)); pr.scratch_size = need;
            }
            MI_CHECK_G(hipStreamWaitEvent(pr.stream, c->split_ready, 0));
            st = pr.stream; scr = pr.scratch;
        }
        if (few) mul_mat_vec_q((int) a->type, e->data[i], a->nb[1], rows, K, q, N, d, dst->nb[1], st);
        else {
            mmq_call mc = {};
            mc.type = (int) a->type; mc.W = e->data[i]; mc.w_row_stride = a->nb[1]; mc.m = rows; mc.stream = st; mc.dst = d; mc.dst_stride = dst->nb[1];
            mc.act = { (const float *) b->data, b->nb[1], K, N, scr, need, false };
            mul_mat_q(mc);
        }
        c->cnt.kernels_launched++; c->cnt.weight_bytes += (uint64_t) rows*a->nb[1];
        if (few) c->cnt.mmvq_launches++; else c->cnt.mmq_launches++;
        if (!local) { MI_CHECK_G(hipEventRecord(c->peers[i].done, st)); waited[i] = true; }
    }
    set_device(c->device);
    for (int i = 0; i < G().n_devices; i++) if (waited[i]) MI_CHECK_G(hipStreamWaitEvent(c->stream, c->peers[i].done, 0));
    c->cnt.split_mul_mats++;
}

// a launch over the expert stack `as` ([k, m, n_expert]) for the pairs of `ids`: what the caller adds is the input, the epilogue and dst
static mmq_moe_call moe_call_of(mi_backend_ctx * c, const struct ggml_tensor * as, const struct ggml_tensor * ids) {
    mmq_moe_call mc = {};
    mc.type = (int) as->type; mc.W = as->data; mc.w_row_stride = as->nb[1]; mc.w_expert_stride = as->nb[2]; mc.m = as->ne[1]; mc.k = as->ne[0]; mc.n_expert = as->ne[2];
    mc.ids = (const int32_t *) ids->data; mc.ids_nb0 = ids->nb[0]; mc.ids_nb1 = ids->nb[1]; mc.n_used = ids->ne[0]; mc.n_tokens = ids->ne[1]; mc.stream = c->stream;
    return mc;
}
static void op_mul_mat_id(mi_backend_ctx * c, struct ggml_tensor * dst) {
    const struct ggml_tensor * as  = dst->src[0];
    const struct ggml_tensor * b   = dst->src[1];
    const struct ggml_tensor * ids = dst->src[2];
    const int64_t K = as->ne[0], M = as->ne[1];
    const int64_t n_used = ids->ne[0], n_tokens = ids->ne[1], n_b = b->ne[1];
    if (!ggml_is_quantized(as->type)) {      // F16 / BF16 / F32 expert stack
        mul_mat_id_dense((int) as->type, as->data, as->nb[0], as->nb[1], as->nb[2], M, K, b->data, b->nb[0], b->nb[1], b->nb[2], n_b,
                         ids->data, ids->nb[0], ids->nb[1], n_used, n_tokens, as->ne[2], (float *) dst->data, dst->nb[1], dst->nb[2], c->stream);
        c->cnt.kernels_launched++; c->cnt.dense_id++;
        return;
    }
    const int kind = act_kind_for((int) as->type);
    // many tokens: sort the (token, slot) pairs by expert on the device and run the MFMA tile kernel per expert; the mat-vec kernel
    // below would read every expert matrix once per pair
    if (n_used*n_tokens > 4*MMVQ_MAX_N && mul_mat_q_id_supported(as->ne[2], n_used, n_tokens) && dst->nb[0] == sizeof(float)) {
        c->pass.drop_act();   // the scratch is reused
        mmq_moe_call mc = moe_call_of(c, as, ids);
        mc.n_b = n_b; mc.b = (const float *) b->data; mc.b_nb1 = b->nb[1]; mc.b_nb2 = b->nb[2]; mc.scratch = c->scratch;
        mc.dst = (float *) dst->data; mc.dst_nb1 = dst->nb[1]; mc.dst_nb2 = dst->nb[2];
        mul_mat_q_id(mc);
        c->cnt.mmq_launches++; c->cnt.kernels_launched += 3;
        c->cnt.weight_bytes += (uint64_t) as->ne[2]*M*ggml_row_size(as->type, K);
        return;
    }
    const act_q8 q = get_act(c, b->data, K, n_b, n_tokens, b->nb[1], b->nb[2], kind);
    mul_mat_vec_q_id((int) as->type, as->data, as->nb[1], as->nb[2], M, K, q,
                     (const int32_t *) ids->data, ids->nb[0], ids->nb[1], n_used, n_tokens, n_b,
                     (float *) dst->data, dst->nb[1], dst->nb[2], c->stream);
    c->cnt.mmvq_launches++; c->cnt.kernels_launched++;
    c->cnt.weight_bytes += (uint64_t) n_used*n_tokens*M*ggml_row_size(as->type, K);
}

static void op_flash_attn_ext(mi_backend_ctx * c, struct ggml_tensor * node) {
    const struct ggml_tensor * q = node->src[0]; const struct ggml_tensor * k = node->src[1]; const struct ggml_tensor * v = node->src[2];
    const struct ggml_tensor * mask = node->src[3];
    const int64_t hd = k->ne[0], hsv = v->ne[0], n_kv = k->ne[1], T = q->ne[1];      // hd: K's head size
    // what supports_op cannot see (data alignment of the views handed in) fails the graph instead of the process
    MI_REQUIRE_G(node->nb[1] == (size_t) hsv*4 && ((uintptr_t) q->data % 16) == 0);
    MI_REQUIRE_G(((uintptr_t) k->data % (k->type == GGML_TYPE_F16 || k->type == GGML_TYPE_BF16 ? 16 : 2)) == 0 && ((uintptr_t) v->data % (v->type == GGML_TYPE_F16 || v->type == GGML_TYPE_BF16 ? 16 : 2)) == 0);
    MI_REQUIRE_G(!mask || (mask->ne[0] == n_kv && mask->ne[1] >= T && ((uintptr_t) mask->data % 16) == 0 && mask->nb[1] % 16 == 0 && mask->nb[3] % 16 == 0));
    fa_operands p = fa_kv16_plan(node, c->kv16, c->attn_part, c->attn_part_bytes);
    MI_REQUIRE_G(p.ok && p.k_bytes + p.v_bytes <= c->kv16_size);
    p.call.stream = c->stream;
    if (p.k_bytes) {
        kv_to_f16((int) k->type, k->data, k->nb[1], k->nb[2], k->nb[3], hd, n_kv, k->ne[2], k->ne[3], (uint16_t *) c->kv16, /* transpose */ false, c->stream);
        c->cnt.kernels_launched++;
    }
    if (p.v_bytes) {
        kv_to_f16((int) v->type, v->data, v->nb[1], v->nb[2], v->nb[3], hsv, n_kv, v->ne[2], v->ne[3], (uint16_t *) ((char *) c->kv16 + p.k_bytes), p.call.v_trans, c->stream);
        c->cnt.kernels_launched++;
    }
    if (T <= 8) attn_decode(p.call); else attn_prefill(p.call);
    c->cnt.kernels_launched++;
}

// the one place that launches a grouped mat-vec. wbytes: the weight bytes the launch streams, as its caller counts them. Profile record: m < 0 marks a
// grouped launch, |m| = KiB of weights; n = 1; type of the first group. Eager profiling: the event pair rides on the dispatch itself (kernel start ->
// kernel end, the interval rocprofv3's kernel trace reports); in-graph profiling: event-record nodes around the call, like every other mat-mul — so
// where the dispatcher first has to run a pending MoE combine as its own kernel (no streamed route), that kernel lies inside the pair.
// (The type is the first group's on both routes, deliberately: the register-ring route once reported the lower type of a mixed launch.)
static void emit_mmv(mi_backend_ctx * c, const mmvq_group * grp, int nc, int64_t K, const mmvq_input & in, const mmvq_rope * rope, const mmvq_fin * fin, uint64_t wbytes) {
    const bool prof = c->profiling && !c->prof_suspend;
    mmvq_launch_rec rec = { nullptr, nullptr, "" };
    prof_begin(c, grp[0].type, -(int64_t)(wbytes/1024), K, 1, wbytes, c->prof_in_graph);
    if (prof && !c->prof_in_graph) { rec.e0 = c->prof.back().e0; rec.e1 = c->prof.back().e1; }
    mul_mat_vec_q_fused(grp, nc, K, in, rope, c->stream, fin, prof ? &rec : nullptr);
    if (prof && c->prof_in_graph) prof_end(c);
    if (prof) c->prof.back().kernel = rec.kernel;
    c->cnt.mmvq_launches++; c->cnt.kernels_launched++; c->cnt.weight_bytes += wbytes;
}

// ---------------------------------------------------------------------------------------------------------------
// decode fusions (decode_fused.hip). Each matcher checks op, type, shape, layout AND that every skipped intermediate
// has exactly one consumer and is not a graph output; anything else falls back to node-by-node execution.
// ---------------------------------------------------------------------------------------------------------------
static int next_real(const struct ggml_cgraph * g, int i) {
    for (int j = i + 1; j < g->n_nodes; j++) {
        if (!is_view_op(g->nodes[j]->op) && !ggml_is_empty(g->nodes[j])) return j;
    }
    return -1;
}
static int n_uses(mi_backend_ctx * c, const struct ggml_tensor * t) {
    auto it = c->pass.uses.find(t);
    return it == c->pass.uses.end() ? 0 : it->second;
}
static bool is_internal(mi_backend_ctx * c, const struct ggml_tensor * t) {   // safe to leave unwritten
    return n_uses(c, t) == 1 && !(t->flags & GGML_TENSOR_FLAG_OUTPUT);
}
static bool is_row_vec_f32(const struct ggml_tensor * t) {   // [ne0, 1, 1, 1] contiguous f32, 16-byte aligned
    return t->type == GGML_TYPE_F32 && t->ne[1] == 1 && t->ne[2] == 1 && t->ne[3] == 1 && t->nb[0] == 4 && ((uintptr_t) t->data % 16) == 0;
}
static bool fusable_mmv(const struct ggml_tensor * n) {       // quantized weights x one f32 column
    if (n->op != GGML_OP_MUL_MAT) return false;
    const struct ggml_tensor * a = n->src[0]; const struct ggml_tensor * b = n->src[1];
    if (!ggml_is_quantized(a->type) || !mul_mat_vec_q_supported((int) a->type) || tensor_is_split(a)) return false;
    if (a->ne[2] != 1 || a->ne[3] != 1 || !is_row_vec_f32(b)) return false;
    if (a->nb[0] != ggml_type_size(a->type)) return false;
    return mul_mat_vec_q_fused_supported(a->ne[0], act_kind_for((int) a->type)) && a->ne[1] < (1 << 30);
}

struct mmv_chain { mmvq_group grp; int last; bool has_rope; mmvq_rope rope; const void * out_ptr; size_t out_bytes; };

// the chain of nodes that starts at mat-vec node i and can run as one group of the fused launch
static mmv_chain match_mmv_chain(mi_backend_ctx * c, const struct ggml_cgraph * g, int i) {
    struct ggml_tensor * n = g->nodes[i];
    const struct ggml_tensor * a = n->src[0];
    mmv_chain ch = {};
    ch.grp = { (const char *) a->data, nullptr, a->nb[1], (int) a->ne[1], (int) a->type, (float *) n->data, EPI_NONE, nullptr, nullptr, nullptr, 0, 0 };
    ch.last = i; ch.has_rope = false; ch.out_ptr = n->data; ch.out_bytes = ggml_nbytes(n);

    // MUL_MAT [-> ADD(bias)] -> RESHAPE -> ROPE: NORM pairs (src/llama-model.cpp:6017-6040), or NEOX pairs over a whole power-of-two head, with
    // gpt-oss's bias in between (src/llama-model.cpp:17636-17660)
    if (i + 2 < g->n_nodes && is_internal(c, n)) {
        int ir = i + 1;
        const struct ggml_tensor * bias = nullptr; const struct ggml_tensor * pre = n;
        if (g->nodes[ir]->op == GGML_OP_ADD && ir + 2 < g->n_nodes) {
            const struct ggml_tensor * ad = g->nodes[ir];
            const struct ggml_tensor * other = ad->src[0] == n ? ad->src[1] : (ad->src[1] == n ? ad->src[0] : nullptr);
            if (other && other != n && other->type == GGML_TYPE_F32 && ad->type == GGML_TYPE_F32 && ggml_are_same_shape(other, n) && ggml_are_same_shape(ad, n) &&
                ggml_is_contiguous(other) && ggml_is_contiguous(ad) && is_internal(c, ad)) { bias = other; pre = ad; ir++; }
        }
        struct ggml_tensor * rs = g->nodes[ir]; struct ggml_tensor * rp = g->nodes[ir + 1];
        const int rmode = rp->op == GGML_OP_ROPE ? rp->op_params[2] : -1;
        const bool neox_ok = rmode == 2 && rp->op_params[1] == rp->ne[0] && (rp->ne[0] & (rp->ne[0] - 1)) == 0 && rp->ne[0] >= 4 && a->ne[1] % rp->ne[0] == 0;
        if (rs->op == GGML_OP_RESHAPE && rs->src[0] == pre && is_internal(c, rs) && rp->op == GGML_OP_ROPE && rp->src[0] == rs &&
            rp->type == GGML_TYPE_F32 && ggml_is_contiguous(rp) && (rmode == 0 || neox_ok) && rp->ne[2] == 1 && rp->ne[3] == 1 &&
            rp->op_params[1] % 2 == 0 && rp->ne[0] % 2 == 0 && a->ne[1] % 2 == 0 && rp->src[1]->type == GGML_TYPE_I32) {
            ch.grp.dst = (float *) rp->data; ch.grp.epi = EPI_ROPE; ch.last = ir + 1; ch.has_rope = true;
            ch.grp.res = bias ? (const float *) bias->data : nullptr;
            ch.rope = mmvq_rope_of(rp);
            ch.out_ptr = rp->data; ch.out_bytes = ggml_nbytes(rp);
            return ch;
        }
    }
    const int j = next_real(g, i);
    if (j < 0) return ch;
    struct ggml_tensor * nx = g->nodes[j];
    // MUL_MAT -> ADD(residual): src/llama-model.cpp:6057,6096
    if (nx->op == GGML_OP_ADD && is_internal(c, n) && (nx->src[0] == n || nx->src[1] == n) && nx->type == GGML_TYPE_F32) {
        const struct ggml_tensor * other = nx->src[0] == n ? nx->src[1] : nx->src[0];
        if (other->type == GGML_TYPE_F32 && ggml_are_same_shape(other, n) && ggml_is_contiguous(other) && ggml_is_contiguous(nx) && ggml_are_same_shape(nx, n)) {
            ch.grp.dst = (float *) nx->data; ch.grp.epi = EPI_ADD; ch.grp.res = (const float *) other->data; ch.last = j;
            ch.out_ptr = nx->data; ch.out_bytes = ggml_nbytes(nx);
            // ... -> ADD again (gpt-oss: wo.x + bias, then + the residual stream, src/llama-graph.cpp:1479-1481 + llama-model.cpp:17676)
            const int j2 = next_real(g, j);
            if (j2 > 0 && is_internal(c, nx)) {
                struct ggml_tensor * n2 = g->nodes[j2];
                if (n2->op == GGML_OP_ADD && (n2->src[0] == nx || n2->src[1] == nx) && n2->src[0] != n2->src[1] && n2->type == GGML_TYPE_F32) {
                    const struct ggml_tensor * o2 = n2->src[0] == nx ? n2->src[1] : n2->src[0];
                    if (o2->type == GGML_TYPE_F32 && ggml_are_same_shape(o2, n) && ggml_is_contiguous(o2) && ggml_is_contiguous(n2) && ggml_are_same_shape(n2, n)) {
                        ch.grp.dst = (float *) n2->data; ch.grp.res2 = (const float *) o2->data; ch.last = j2;
                        ch.out_ptr = n2->data; ch.out_bytes = ggml_nbytes(n2);
                    }
                }
            }
            return ch;
        }
    }
    // MUL_MAT(gate) ; MUL_MAT(up) -> GLU(swiglu, gate, up), in either graph order (the DFS of ggml_build_forward_expand puts
    // GLU's src[0] = gate first): src/llama-graph.cpp:646-691
    if (fusable_mmv(nx) && nx->src[1] == n->src[1] && nx->src[0]->type == a->type && ggml_are_same_shape(nx->src[0], a) &&
        nx->src[0]->nb[1] == a->nb[1] && is_internal(c, n) && is_internal(c, nx)) {
        const int j2 = next_real(g, j);
        if (j2 > 0) {
            struct ggml_tensor * gl = g->nodes[j2];
            if (gl->op == GGML_OP_GLU && ggml_get_glu_op(gl) == GGML_GLU_OP_SWIGLU && gl->op_params[1] == 0 && gl->src[1] != NULL &&
                ((gl->src[0] == nx && gl->src[1] == n) || (gl->src[0] == n && gl->src[1] == nx)) && gl->type == GGML_TYPE_F32 && ggml_is_contiguous(gl)) {
                ch.grp.W  = (const char *) gl->src[0]->src[0]->data;   // gate weights (silu side)
                ch.grp.W2 = (const char *) gl->src[1]->src[0]->data;   // up weights
                ch.grp.dst = (float *) gl->data; ch.grp.epi = EPI_GLU; ch.last = j2;
                ch.out_ptr = gl->data; ch.out_bytes = ggml_nbytes(gl);
                return ch;
            }
        }
    }
    return ch;
}

static const struct ggml_tensor * base_of(const struct ggml_tensor * t) {   // strip view ops
    while (t && is_view_op(t->op) && t->op != GGML_OP_NONE && t->src[0]) t = t->src[0];
    return t;
}

// Run the mat-vec at node i together with the mat-vecs that directly follow it on the same activation.
//   norm/normw != NULL: the activation is MUL(RMS_NORM(norm->src[0]), normw) and the caller has checked that every consumer of
//   that product is a mat-vec; if they all fit into this launch the norm is computed in the prologue (PRO_NORM).
//   from: the first node of this step (the norm's, with a norm prologue).
// Returns the index of the last node consumed (-1 = not fused).
static int try_fused_mmv(mi_backend_ctx * c, struct ggml_cgraph * g, int i, int from, const struct ggml_tensor * norm, const struct ggml_tensor * normw) {
    struct ggml_tensor * n = g->nodes[i];
    if (!fusable_mmv(n)) return -1;
    int deferred[MMVQ_MAX_GROUPS]; int n_def = 0;      // ROPE nodes between the grouped mat-vecs that the epilogue cannot do (NEOX): run after the launch
    const struct ggml_tensor * b = n->src[1];
    const int kind = act_kind_for((int) n->src[0]->type);
    mmv_chain chains[MMVQ_MAX_GROUPS];
    int nc = 0, last = i, n_mm = 0;
    chains[nc++] = match_mmv_chain(c, g, i);
    last = chains[0].last;
    n_mm += chains[0].grp.epi == EPI_GLU ? 2 : 1;
    while (nc < MMVQ_MAX_GROUPS && chains[0].grp.epi != EPI_GLU) {
        int j = next_real(g, last);
        if (j < 0) break;
        struct ggml_tensor * m = g->nodes[j];
        int def_j = -1;
        if (m->op == GGML_OP_ROPE && !chains[nc - 1].has_rope && m->src[0] && base_of(m->src[0])->data == chains[nc - 1].out_ptr && n_def < MMVQ_MAX_GROUPS) {
            // gpt-oss: wq -> + bias -> RESHAPE -> ROPE(NEOX) ; wk -> ... ; wv (src/llama-model.cpp:17636-17660): the rotation of the chain just matched
            // only needs that chain — if the next mat-vec on the same activation follows it, it joins the launch and the ROPE runs afterwards
            const int j2 = next_real(g, j);
            if (j2 < 0 || !fusable_mmv(g->nodes[j2]) || g->nodes[j2]->src[1] != b) break;
            bool okr = !ranges_overlap(m->data, ggml_nbytes(m), b->data, ggml_nbytes(b));
            for (int q = 0; q < nc && okr; q++) okr = m->data == chains[q].out_ptr ? q == nc - 1 : !ranges_overlap(m->data, ggml_nbytes(m), chains[q].out_ptr, chains[q].out_bytes);
            if (!okr) break;
            def_j = j; j = j2; m = g->nodes[j];
        }
        if (!fusable_mmv(m) || m->src[1] != b) break;
        if (act_kind_for((int) m->src[0]->type) != kind) {
            // another activation format (Mixtral: wq Q4_K, wk / wv Q8_0) joins only a launch in which every workgroup quantizes the activation
            // itself: the norm prologue, or the plain quantizing one when no image of b is cached
            const bool cached_b = c->pass.holds_image_of(b->data);
            if (!(norm || !cached_b) || !mul_mat_vec_q_fused_can_group_mixed(chains[0].grp.type, (int) m->src[0]->type) ||
                !mul_mat_vec_q_fused_prologue_supported(n->src[0]->ne[0], kind) || !mul_mat_vec_q_fused_prologue_supported(n->src[0]->ne[0], act_kind_for((int) m->src[0]->type))) break;
        }
        mmv_chain ch = match_mmv_chain(c, g, j);
        if (ch.grp.epi == EPI_GLU) break;   // the dual (GLU) kernel runs alone
        {   // at most two distinct weight types per launch, and only pairs that have a kernel
            int t2 = -1; bool ok_t = true;
            for (int q = 0; q < nc; q++) if (chains[q].grp.type != chains[0].grp.type) t2 = chains[q].grp.type;
            if (ch.grp.type != chains[0].grp.type) { if (t2 >= 0 && t2 != ch.grp.type) ok_t = false; else ok_t = mul_mat_vec_q_fused_can_group(chains[0].grp.type, ch.grp.type) || mul_mat_vec_q_fused_can_group_mixed(chains[0].grp.type, ch.grp.type); }
            if (!ok_t) break;
        }
        if (ch.has_rope && chains[0].has_rope && memcmp(&ch.rope, &chains[0].rope, sizeof(ch.rope)) != 0) break;   // one rope descriptor per launch
        // groups run concurrently: no output may alias another group's output, residual, or the shared activation
        bool ok = !ranges_overlap(ch.out_ptr, ch.out_bytes, b->data, ggml_nbytes(b));
        for (int q = 0; q < nc && ok; q++) {
            ok = !ranges_overlap(ch.out_ptr, ch.out_bytes, chains[q].out_ptr, chains[q].out_bytes);
            if (ok && chains[q].grp.res) ok = !ranges_overlap(ch.out_ptr, ch.out_bytes, chains[q].grp.res, (size_t) chains[q].grp.m*4);
            if (ok && ch.grp.res)       ok = !ranges_overlap(chains[q].out_ptr, chains[q].out_bytes, ch.grp.res, (size_t) ch.grp.m*4);
            if (ok && chains[q].grp.res2) ok = !ranges_overlap(ch.out_ptr, ch.out_bytes, chains[q].grp.res2, (size_t) chains[q].grp.m*4);
            if (ok && ch.grp.res2)        ok = !ranges_overlap(chains[q].out_ptr, chains[q].out_bytes, ch.grp.res2, (size_t) ch.grp.m*4);
        }
        // ... nor what a ROPE that now runs after the launch still has to write (its own chain's buffer excepted: in-place rotation)
        for (int r = 0; r < n_def + (def_j >= 0 ? 1 : 0) && ok; r++) {
            const struct ggml_tensor * rp = g->nodes[r < n_def ? deferred[r] : def_j];
            ok = !ranges_overlap(ch.out_ptr, ch.out_bytes, rp->data, ggml_nbytes(rp));
        }
        if (!ok) break;
        if (def_j >= 0) deferred[n_def++] = def_j;
        chains[nc++] = ch;
        last = ch.last;
        n_mm++;
    }

    // the KV-cache writes that follow wk / wv: SET_ROWS(k_cache, rope(k)) ; SET_ROWS(v_view[1,N], v[1,N]) — src/llama-kv-cache-unified.cpp:1123,1157-1167
    {
        const int j1 = next_real(g, last);
        const int j2 = j1 > 0 ? next_real(g, j1) : -1;
        if (j2 > 0 && g->nodes[j1]->op == GGML_OP_SET_ROWS && g->nodes[j2]->op == GGML_OP_SET_ROWS) {
            struct ggml_tensor * sk = g->nodes[j1]; struct ggml_tensor * sv = g->nodes[j2];
            const struct ggml_tensor * ks = sk->src[0]; const struct ggml_tensor * ki = sk->src[1];
            const struct ggml_tensor * vs = sv->src[0]; const struct ggml_tensor * vi = sv->src[1];
            int qk = -1, qv = -1;
            for (int q = 0; q < nc; q++) {
                if (base_of(ks)->data == chains[q].out_ptr && ks->data == chains[q].out_ptr) qk = q;
                if (base_of(vs)->data == chains[q].out_ptr && vs->data == chains[q].out_ptr) qv = q;
            }
            // a quantized K cache (-ctk q8_0 / q4_0): the row quantizer needs whole 32-element blocks, which no wave of this launch holds — K's SET_ROWS runs as
            // its own launch right after this one (deferred), V's store is still taken into the launch
            const bool k_quant = sk->type == GGML_TYPE_Q8_0 || sk->type == GGML_TYPE_Q4_0;
            const bool ok = qk >= 0 && qv >= 0 && qk != qv && (sk->type == GGML_TYPE_F16 || (k_quant && n_def < MMVQ_MAX_GROUPS)) && sv->type == GGML_TYPE_F16 &&
                ks->type == GGML_TYPE_F32 && vs->type == GGML_TYPE_F32 && ki->type == GGML_TYPE_I64 && vi->type == GGML_TYPE_I64 &&
                ggml_is_contiguous(ki) && ggml_is_contiguous(vi) && ggml_is_contiguous(ks) && ggml_is_contiguous(vs) &&
                ks->ne[1] == 1 && ks->ne[2] == 1 && ks->ne[3] == 1 && ks->ne[0] == chains[qk].grp.m && (k_quant || (sk->nb[0] == 2 && sk->nb[1] % 2 == 0)) &&
                vs->ne[2] == 1 && vs->ne[3] == 1 && qv >= 0 && (chains[qv].grp.epi == EPI_NONE || chains[qv].grp.epi == EPI_ADD) &&
                // V: element scatter on the transposed cache's [1, N] view (v_trans), or — with flash attention — a row like K (:1154)
                ((vs->ne[0] == 1 && vs->ne[1] == chains[qv].grp.m && sv->ne[0] == 1 && sv->nb[1] == 2 && ggml_nelements(vi) == chains[qv].grp.m) ||
                 (vs->ne[0] == chains[qv].grp.m && vs->ne[1] == 1 && sv->nb[0] == 2 && sv->nb[1] % 2 == 0 && ggml_nelements(vi) == 1)) &&
                // the cache rows written must not be read by anything inside the launch (they are not: only weights and the activation are)
                !ranges_overlap(sk->data, ggml_nbytes(sk), b->data, ggml_nbytes(b)) && !ranges_overlap(sv->data, ggml_nbytes(sv), b->data, ggml_nbytes(b));
            if (ok) {
                if (k_quant) deferred[n_def++] = j1;
                else {
                    chains[qk].grp.st16 = (uint16_t *) sk->data; chains[qk].grp.st_idx = (const int64_t *) ki->data;
                    chains[qk].grp.st_row_elems = (int64_t)(sk->nb[1]/2); chains[qk].grp.st_mode = 1;
                }
                chains[qv].grp.st16 = (uint16_t *) sv->data; chains[qv].grp.st_idx = (const int64_t *) vi->data;
                if (vs->ne[0] == 1) { chains[qv].grp.st_row_elems = 0; chains[qv].grp.st_mode = 2; }
                else                { chains[qv].grp.st_row_elems = (int64_t)(sv->nb[1]/2); chains[qv].grp.st_mode = 1; }
                last = j2;
            }
        }
    }

    mmvq_group grp[MMVQ_MAX_GROUPS];
    const mmvq_rope * rope = nullptr;
    uint64_t wbytes = 0;
    for (int q = 0; q < nc; q++) {
        grp[q] = chains[q].grp;
        if (chains[q].has_rope) rope = &chains[q].rope;
        wbytes += (uint64_t) grp[q].m*grp[q].row_stride*(grp[q].epi == EPI_GLU ? 2 : 1);
    }
    const int64_t K = n->src[0]->ne[0];
    mmvq_input in = {};
    in.act_kind = kind;
    const act_q8 * cached = c->pass.q8_of_row(b->data, K, kind);
    // The norm's product is left unwritten only where nobody else can look at it: not when the view handed to graph_compute ENDS at one of
    // its consumers (the scheduler's eval-callback cuts the graph there and the callback — tools/imatrix/imatrix.cpp:223-247 — reads the mat-mul's
    // src1), and not for result_norm, which llama_context reads back as the embeddings without an OUTPUT flag (src/llama-context.cpp:1137-1151)
    bool view_ends_here = false;
    for (int q = 0; q < g->n_nodes; q++) if (g->nodes[q]->op == GGML_OP_MUL_MAT && g->nodes[q]->src[1] == b && q == g->n_nodes - 1) view_ends_here = true;
    const bool keep_norm = norm && (view_ends_here || strncmp(b->name, "result_norm", 11) == 0 || strncmp(b->name, "result_embd", 11) == 0);
    if (norm && !keep_norm && n_mm == n_uses(c, b) && mul_mat_vec_q_fused_prologue_supported(K, kind) && ((uintptr_t) normw->data % 16) == 0) {
        in.mode = PRO_NORM; in.x = (const float *) norm->src[0]->data; in.norm_w = (const float *) normw->data; in.eps = op_f32(norm, 0);
    } else if (norm) {
        return -1;      // the caller runs the norm (+ quantization) as its own kernel, then comes back without `norm`
    } else if (cached) {
        in.mode = PRO_Q8; in.act = *cached; c->cnt.act_quant_reused++;
    } else if (mul_mat_vec_q_fused_prologue_supported(K, kind)) {
        in.mode = PRO_QUANT; in.x = (const float *) b->data;
    } else {
        in.mode = PRO_Q8; in.act = get_act(c, b->data, K, 1, 1, b->nb[1], 0, kind);
    }
    // gate/up/SwiGLU whose output the down projection reads next (build_ffn, src/llama-graph.cpp:691-748): the launch also writes the quantized
    // image of its output (mmvq_fin) — the f32 tensor is written as always, so any other reader still finds it
    mmvq_fin fin = {}; act_q8 fin_q = {}; const struct ggml_tensor * fin_t = nullptr;
    static const bool fin_env = env_on("GGML_MI355X_FIN");
    if (fin_env && nc == 1 && grp[0].epi == EPI_GLU && !grp[0].eid && c->fin_img && !mul_mat_vec_q_stream_takes(grp, nc, K, in, rope)) {
        const int jn = next_real(g, last);
        const struct ggml_tensor * gl = g->nodes[last];
        const struct ggml_tensor * mm = jn > 0 ? g->nodes[jn] : nullptr;
        if (mm && fusable_mmv(mm) && mm->src[1] == gl && (void *) grp[0].dst == gl->data) {
            const int kind2 = act_kind_for((int) mm->src[0]->type);
            const int64_t M = grp[0].m;
            if (kind2 > 0 && mul_mat_vec_q_fused_fin_supported(M, K) && mul_mat_vec_q_fused_supported(M, kind2) && M/256 <= mi_backend_ctx::FIN_COUNTERS &&
                act_q8_bytes(kind2, M, 1) <= mi_backend_ctx::FIN_IMG_BYTES) {
                fin_q = act_q8_carve(c->fin_img, kind2, M, 1);
                fin = { kind2, 0, fin_q.qs, fin_q.d, fin_q.bsums, c->fin_cnt };
                fin_t = gl;
            }
        }
    }
    mmvq_rope rope_l;
    if (rope) {
        if (!c->rope_tab || rope->p.n_dims/2 > 512) return -1;
        if (!c->pass.rope_valid || memcmp(&c->pass.rope_key, rope, sizeof(*rope)) != 0) {
            mul_mat_vec_q_fused_rope_table(*rope, c->rope_tab, c->stream);
            c->cnt.kernels_launched++;
            c->pass.rope_key = *rope; c->pass.rope_valid = true;
        }
        rope_l = *rope; rope_l.table = c->rope_tab; rope = &rope_l;
    }
    if (!mul_mat_vec_q_fused_takes(grp, nc, K, in, rope)) return -1;      // (a format without a register-ring kernel — mmvq_fused.hip: fused_pairs — in a launch the streamed kernel declines: node by node)
    if (c->pass.pp.active && in.mode == PRO_NORM && (const void *) in.x == (const void *) c->pass.pp.x_out && K == c->pass.pp.m) {
        // the norm's input is the MoE combine left pending: this launch evaluates it in its prologue (and stores the sum). EVERY workgroup's prologue reads the
        // residual, the experts' outputs, the router's probabilities and the ids while other workgroups already store their rows — and by graph order all four are
        // dead after the combine, so an allocator that reuses memory (ggml-alloc) may have put this launch's outputs there: then the combine runs as
        // its own kernel first
        bool clash = false;
        const size_t planes_bytes = ((size_t)(c->pass.pp.n_planes - 1)*c->pass.pp.stride + (size_t) c->pass.pp.m)*4;
        for (int q = 0; q < nc && !clash; q++) {
            const void * d = chains[q].out_ptr; const size_t nb = chains[q].out_bytes;
            clash = (c->pass.pp.res && ranges_overlap(d, nb, c->pass.pp.res, (size_t) c->pass.pp.m*4)) || ranges_overlap(d, nb, c->pass.pp.planes, planes_bytes) ||
                    ranges_overlap(d, nb, c->pass.pp.probs, c->pass.pp.probs_bytes) || (c->pass.pp.ids && ranges_overlap(d, nb, c->pass.pp.ids, (size_t) c->pass.pp.n_planes*4));
        }
        if (clash) pp_flush(c);
        else {
            in.x = c->pass.pp.res; in.planes = c->pass.pp.planes; in.n_planes = c->pass.pp.n_planes; in.plane_stride = c->pass.pp.stride; in.x_out = c->pass.pp.x_out;
            in.pl_probs = c->pass.pp.probs; in.pl_ids = c->pass.pp.ids; in.pl_mode = c->pass.pp.mode;
            c->pass.pp.active = false;
        }
    }
    emit_mmv(c, grp, nc, K, in, rope, fin_t ? &fin : nullptr, wbytes);
    if (fin_t) c->pass.produced_q8(from, last, fin_t->data, grp[0].m, 1, fin_t->nb[1], fin.kind, fin_q);
    for (int r = 0; r < n_def; r++) compute_node(c, g, deferred[r]);
    return last;
}

// the quantized many-token mat-mul that is the ONLY reader of t and directly follows node `last`, or NULL: its producer may then emit the
// bf16 activation copy itself (and skip the f32 tensor)
static const struct ggml_tensor * prefill_mm_consumer(mi_backend_ctx * c, const struct ggml_cgraph * g, int last, const struct ggml_tensor * t) {
    static const bool on = env_on("GGML_MI355X_PREFILL_BF16_OUT");
    const int j = next_real(g, last);
    if (!on || j < 0 || j == g->n_nodes - 1) return nullptr;      // (a view that ends at the consumer: the eval-callback case — its src1 must exist as f32)
    const struct ggml_tensor * n = g->nodes[j];
    if (n->op != GGML_OP_MUL_MAT || n->src[1] != t || !ggml_is_quantized(n->src[0]->type) || tensor_is_split(n->src[0]) || t->type != GGML_TYPE_F32 || t->ne[1] <= MMVQ_MAX_N || t->ne[2] != 1 || t->ne[3] != 1 ||
        n->src[0]->ne[2] != 1 || n->src[0]->ne[3] != 1 || t->nb[0] != 4 || t->ne[0] % 64 != 0 || !is_internal(c, t)) return nullptr;
    return n;
}

// SET_ROWS(k) immediately followed by SET_ROWS(v as [1, N] element scatter), f32 -> f16 (src/llama-kv-cache-unified.cpp:1123,1157-1167)
static int try_fused_kv_store(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    struct ggml_tensor * sk = g->nodes[i];
    const int j = next_real(g, i);
    if (j < 0) return 0;
    struct ggml_tensor * sv = g->nodes[j];
    if (sv->op != GGML_OP_SET_ROWS) return 0;
    const struct ggml_tensor * ks = sk->src[0]; const struct ggml_tensor * ki = sk->src[1];
    const struct ggml_tensor * vs = sv->src[0]; const struct ggml_tensor * vi = sv->src[1];
    if (sk->type != GGML_TYPE_F16 || sv->type != GGML_TYPE_F16 || ks->type != GGML_TYPE_F32 || vs->type != GGML_TYPE_F32) return 0;
    if (ki->type != GGML_TYPE_I64 || vi->type != GGML_TYPE_I64 || !ggml_is_contiguous(ki) || !ggml_is_contiguous(vi)) return 0;
    if (ks->ne[2] != 1 || ks->ne[3] != 1 || vs->ne[2] != 1 || vs->ne[3] != 1 || ks->nb[0] != 4 || sk->nb[0] != 2) return 0;
    if (vs->ne[0] != 1 || vs->nb[1] != 4 || sv->ne[0] != 1 || sv->nb[1] != 2) return 0;
    if (ks->ne[0]*ks->ne[1] + vs->ne[1] >= (1ll << 31)) return 0;
    kv_store_f16((const float *) ks->data, ks->nb[1], (const int64_t *) ki->data, sk->data, sk->nb[1], ks->ne[0], ks->ne[1],
                 (const float *) vs->data, (const int64_t *) vi->data, sv->data, vs->ne[1], c->stream);
    c->cnt.kernels_launched++;
    return j - i + 1;
}

// CPY(kv -> F32) -> ROPE -> CPY(F32 -> kv): the K-shift of a Q8_0 / Q4_0 cache (build_rope_shift, src/llama-kv-cache-unified.cpp:1416-1452: ggml_cast,
// ggml_rope_ext, ggml_cpy back into the same view) as one in-place launch. The last node must write exactly what the first read (placement, type, shape,
// strides) and nobody else may read the two F32 tensors; anything else runs node by node. ggml_cast names its result as its own src[1]: that use is not a reader.
static int try_fused_kv_shift(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    const struct ggml_tensor * cast = g->nodes[i];
    const struct ggml_tensor * kv = cast->src[0];
    const int j1 = next_real(g, i), j2 = j1 > 0 ? next_real(g, j1) : -1;
    if (j2 < 0) return 0;
    const struct ggml_tensor * rp = g->nodes[j1]; const struct ggml_tensor * back = g->nodes[j2];
    if (rp->op != GGML_OP_ROPE || rp->src[0] != cast || rp->type != GGML_TYPE_F32 || !ggml_are_same_shape(rp, cast) || rp->src[1]->type != GGML_TYPE_I32) return 0;
    if (back->op != GGML_OP_CPY || back->src[0] != rp) return 0;
    const struct ggml_tensor * to = back->src[1];
    if (to->data != kv->data || to->type != kv->type || !ggml_are_same_shape(to, kv) || !ggml_are_same_shape(kv, cast) ||
        to->nb[0] != kv->nb[0] || to->nb[1] != kv->nb[1] || to->nb[2] != kv->nb[2] || to->nb[3] != kv->nb[3]) return 0;
    if (cast->src[1] != cast || n_uses(c, cast) != 2 || (cast->flags & GGML_TENSOR_FLAG_OUTPUT) || !is_internal(c, rp)) return 0;      // (2: itself and the ROPE)
    const rope_params p = rope_params_of(rp);
    if (!kv_shift_supported(desc(kv), p) || ggml_nelements(rp->src[1]) < kv->ne[2]) return 0;
    kv_shift(desc(kv), (const int32_t *) rp->src[1]->data, rp->src[2] ? (const float *) rp->src[2]->data : nullptr, p, c->stream);
    c->cnt.kernels_launched++;
    return j2 - i + 1;
}

// MUL_MAT(k, q) -> SOFT_MAX -> MUL_MAT(v, kq) -> PERMUTE -> CONT (src/llama-graph.cpp:1283-1330). With per-sequence KV streams every tensor of the chain has
// ne[3] = n_stream (q [hd, T, n_head, n_stream], :1231-1238; the mask [n_kv, T_pad, 1, n_stream]) and the CONT's rows are stream-major: token t of stream s is
// row s*T + t. One launch either way; a chain in which only some of the tensors carry streams is left to the single nodes.
static int try_fused_attn(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    struct ggml_tensor * kq = g->nodes[i];
    const struct ggml_tensor * k = kq->src[0]; const struct ggml_tensor * q = kq->src[1];
    const bool kq8 = k->type == GGML_TYPE_Q8_0;       // -ctk q8_0: the decode kernel reads the blocks itself (<= 8 tokens); prompts keep the generic ops
    if ((k->type != GGML_TYPE_F16 && !kq8) || q->type != GGML_TYPE_F32 || k->ne[3] != q->ne[3]) return 0;
    const int64_t hd = k->ne[0], n_kv = k->ne[1], n_head_kv = k->ne[2], T = q->ne[1], n_head = q->ne[2], S = q->ne[3];
    const bool prefill = T > 8;      // many tokens: the matrix-core kernel with online softmax (attn_prefill.hip)
    if (kq8 && (k->nb[0] != 34 || k->nb[2] != (size_t) hd/32*34 || k->nb[1] % 2 || k->nb[3] % 2 || (uintptr_t) k->data % 2)) return 0;
    if ((!kq8 && (k->nb[0] != 2 || k->nb[1] % 16 || k->nb[2] % 16 || k->nb[3] % 16 || (uintptr_t) k->data % 16)) || q->nb[0] != 4 || q->nb[1] % 16 || q->nb[2] % 16 || q->nb[3] % 16 || (uintptr_t) q->data % 16) return 0;
    const int j1 = next_real(g, i); if (j1 < 0) return 0;
    struct ggml_tensor * sm = g->nodes[j1];
    if (sm->op != GGML_OP_SOFT_MAX || sm->src[0] != kq || op_f32(sm, 1) != 0.0f || !is_internal(c, kq)) return 0;
    const struct ggml_tensor * mask = sm->src[1];
    if (mask && (mask->ne[0] != n_kv || mask->ne[2] != 1 || (mask->ne[3] != 1 && mask->ne[3] != S) || mask->nb[3] % 4 || !(mask->type == GGML_TYPE_F32 || mask->type == GGML_TYPE_F16))) return 0;
    const int j2 = next_real(g, j1); if (j2 < 0) return 0;
    struct ggml_tensor * kqv = g->nodes[j2];
    if (kqv->op != GGML_OP_MUL_MAT || kqv->src[1] != sm || !is_internal(c, sm)) return 0;
    const struct ggml_tensor * v = kqv->src[0];
    if (v->type != GGML_TYPE_F16 || v->nb[0] != 2 || v->ne[0] != n_kv || v->ne[1] != hd || v->ne[2] != n_head_kv || v->ne[3] != S || v->nb[3] % 16) return 0;
    // PERMUTE(0,2,1,3) view then CONT into [hd*n_head, T]
    const int j3 = next_real(g, j2); if (j3 < 0) return 0;
    struct ggml_tensor * ct = g->nodes[j3];
    if (ct->op != GGML_OP_CONT || !is_internal(c, kqv)) return 0;
    const struct ggml_tensor * pm = ct->src[0];
    if (pm->op != GGML_OP_PERMUTE || pm->src[0] != kqv || !is_internal(c, pm)) return 0;
    if (pm->ne[0] != hd || pm->ne[1] != n_head || pm->ne[2] != T || pm->ne[3] != S) return 0;
    if (ct->type != GGML_TYPE_F32 || !ggml_is_contiguous(ct) || ggml_nelements(ct) != hd*n_head*T*S) return 0;
    attn_call a = {};
    a.hsk = a.hsv = hd; a.n_kv = n_kv; a.n_head = n_head; a.n_head_kv = n_head_kv; a.T = T;
    a.q = q->data; a.q_nb1 = q->nb[1]; a.q_nb2 = q->nb[2]; a.q_type = (int) q->type;
    a.k = k->data; a.k_nb1 = k->nb[1]; a.k_nb2 = k->nb[2]; a.k_type = (int) k->type;
    a.v = v->data; a.v_nb1 = v->nb[1]; a.v_nb2 = v->nb[2]; a.v_type = (int) v->type; a.v_trans = true;
    if (mask) { a.mask = mask->data; a.m_nb1 = mask->nb[1]; a.mask_type = (int) mask->type; }
    a.sinks = sm->src[2] ? (const float *) sm->src[2]->data : nullptr; a.dst = (float *) ct->data; a.dst_nb1 = (size_t) hd*n_head*4;
    a.scale = op_f32(sm, 0); a.part = c->attn_part; a.part_bytes = c->attn_part_bytes; a.stream = c->stream;
    a.n_stream = S; a.q_nb3 = q->nb[3]; a.k_nb3 = k->nb[3]; a.v_nb3 = v->nb[3]; a.m_nb3 = mask && mask->ne[3] > 1 ? mask->nb[3] : 0; a.dst_nb3 = (size_t) T*a.dst_nb1;
    // the chain is taken at head sizes 64 / 128 only, as it always was (the prefill kernel's transposed-V form has FLASH_ATTN_EXT's other sizes too); prompts over a Q8_0 K cache keep the generic ops
    if ((hd != 64 && hd != 128) || !attn_supported(a)) return 0;
    if (prefill) {
        if (mask && (mask->ne[1] < T || ((uintptr_t) mask->data % 16) || mask->nb[1] % 16 || mask->nb[3] % 16)) return 0;
        if (v->nb[1] % 8 || v->nb[2] % 8 || ((uintptr_t) v->data % 8)) return 0;
        // wo reads the result next: hand it the bf16 copy directly (nothing reads the scratch's offset 0 during this kernel)
        const struct ggml_tensor * wo = prefill_mm_consumer(c, g, j3, ct);
        if (wo && mul_mat_q_scratch_bytes(hd*n_head, T*S, wo->src[0]->ne[1]) <= c->scratch_size) { a.y16 = (uint16_t *) c->scratch; a.dst = nullptr; }
        attn_prefill(a);
        if (a.y16) c->pass.produced_bf16(i, j3, ct->data, hd*n_head, T*S, ct->nb[1], 0);
    } else attn_decode(a);
    c->cnt.kernels_launched++;
    return j3 - i + 1;
}

// GET_ROWS(probs, selected) -> [SUM_ROWS -> DIV | SOFT_MAX] -> MUL(experts, weights) -> ADD ... ADD (sum over the used experts)
// [-> ADD residual], one token: the tail of build_moe_ffn (src/llama-graph.cpp:887-1012) as one kernel
static int try_fused_moe_combine(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    struct ggml_tensor * gr = g->nodes[i];
    const struct ggml_tensor * pr = gr->src[0]; const struct ggml_tensor * ids = gr->src[1];
    if (gr->type != GGML_TYPE_F32 || pr->type != GGML_TYPE_F32 || ids->type != GGML_TYPE_I32) return 0;
    const int64_t n_used = ids->ne[0];
    if (gr->ne[0] != 1 || gr->ne[1] != n_used || gr->ne[2] != 1 || gr->ne[3] != 1 || n_used < 2 || n_used > 8) return 0;
    if (pr->ne[0] != 1 || pr->ne[2] != 1 || pr->ne[3] != 1 || pr->nb[1] != 4 || ids->ne[1] != 1 || ids->nb[0] != 4) return 0;
    if (!is_internal(c, gr)) return 0;
    int j = next_real(g, i); if (j < 0) return 0;
    int mode; const struct ggml_tensor * wsrc;      // wsrc: the tensor whose reshape is the MUL's weight operand
    struct ggml_tensor * n1 = g->nodes[j];
    if (n1->op == GGML_OP_SUM_ROWS && base_of(n1->src[0]) == gr && n1->src[0]->ne[0] == n_used && is_internal(c, n1)) {
        const int j2 = next_real(g, j); if (j2 < 0) return 0;
        struct ggml_tensor * dv = g->nodes[j2];
        if (dv->op != GGML_OP_DIV || base_of(dv->src[0]) != gr || dv->src[1] != n1 || dv->ne[0] != n_used || ggml_nelements(dv) != n_used) return 0;
        mode = 0; wsrc = dv; j = j2;
    } else if (n1->op == GGML_OP_SOFT_MAX && base_of(n1->src[0]) == gr && !n1->src[1] && !n1->src[2] && op_f32(n1, 0) == 1.0f && op_f32(n1, 1) == 0.0f &&
               n1->ne[0] == n_used && ggml_nelements(n1) == n_used) {
        mode = 1; wsrc = n1;
    } else return 0;
    if (n_uses(c, wsrc) != 1 || (wsrc->flags & GGML_TENSOR_FLAG_OUTPUT)) return 0;
    const int jm = next_real(g, j); if (jm < 0) return 0;
    struct ggml_tensor * mul = g->nodes[jm];
    if (mul->op != GGML_OP_MUL || mul->type != GGML_TYPE_F32) return 0;
    const struct ggml_tensor * ex = base_of(mul->src[1]) == wsrc ? mul->src[0] : (base_of(mul->src[0]) == wsrc ? mul->src[1] : nullptr);
    if (!ex || ex->type != GGML_TYPE_F32 || ex->ne[1] != n_used || ex->ne[2] != 1 || ex->ne[3] != 1 || ex->nb[0] != 4 || ex->ne[0] % 4 || ex->nb[1] % 16 ||
        ((uintptr_t) ex->data % 16) || !ggml_are_same_shape(ex, mul) || (mul->flags & GGML_TENSOR_FLAG_OUTPUT) || n_uses(c, mul) != (int) n_used) return 0;
    const int64_t n_embd = ex->ne[0];
    // the adds: ((view0 + view1) + view2) + ...
    int jl = jm; const struct ggml_tensor * prev = nullptr;
    for (int64_t u = 1; u < n_used; u++) {
        const int ja = next_real(g, jl); if (ja < 0) return 0;
        struct ggml_tensor * ad = g->nodes[ja];
        if (ad->op != GGML_OP_ADD || ad->type != GGML_TYPE_F32 || ad->ne[0] != n_embd || ggml_nelements(ad) != n_embd) return 0;
        const struct ggml_tensor * a0 = ad->src[0]; const struct ggml_tensor * a1 = ad->src[1];
        if (u == 1) { if (base_of(a0) != mul || a0->data != mul->data) return 0; }
        else if (a0 != prev) return 0;
        if (base_of(a1) != mul || (const char *) a1->data != (const char *) mul->data + u*mul->nb[1]) return 0;
        if (u + 1 < n_used && !is_internal(c, ad)) return 0;
        prev = ad; jl = ja;
    }
    struct ggml_tensor * out = g->nodes[jl];
    const float * res = nullptr;
    // + residual (src/llama-model.cpp:6096)
    if (is_internal(c, out)) {
        const int jr = next_real(g, jl);
        if (jr > 0) {
            struct ggml_tensor * ra = g->nodes[jr];
            if (ra->op == GGML_OP_ADD && ra->type == GGML_TYPE_F32 && ggml_nelements(ra) == n_embd && ggml_is_contiguous(ra) && (ra->src[0] == out || ra->src[1] == out)) {
                const struct ggml_tensor * r = ra->src[0] == out ? ra->src[1] : ra->src[0];
                if (r->type == GGML_TYPE_F32 && ggml_nelements(r) == n_embd && ggml_is_contiguous(r) && ((uintptr_t) r->data % 16) == 0 && ((uintptr_t) ra->data % 16) == 0) {
                    res = (const float *) r->data; out = ra; jl = jr;
                }
            }
        }
    }
    if (!ggml_is_contiguous(out) || ((uintptr_t) out->data % 16)) return 0;
    // the sum's first reader is the norm of a grouped mat-vec launch (the next layer's norm + QKV, or the final norm + lm_head): that launch's prologue
    // evaluates the combine itself (weighted planes, mmvq_stream.h) — this kernel and its boundary go. Anything else: pp_flush runs it after all.
    static const bool defer_on = env_on("GGML_MI355X_MOE_COMBINE_DEFER");
    // the values this combine gathers are the ones the router just ranked (same tensors): its top-8 list is probs[ids[u]] already
    const bool direct = c->pass.rt.valid && c->moe_ws && pr->data == c->pass.rt.vals && ids->data == c->pass.rt.sorted && ids->nb[0] == 4;
    if (direct) c->cnt.moe_combine_direct++;
    {
        const int jn = next_real(g, jl);
        const int jm2 = jn > 0 ? next_real(g, jn) : -1;
        const int jq = jm2 > 0 ? next_real(g, jm2) : -1;
        // (every workgroup of that launch reads the residual and the experts' outputs while one of them stores the sum: the sum's tensor must not share memory
        // with either — an allocator that made the ADD in place, as ggml-alloc does when the residual has no later reader, keeps the stand-alone kernel)
        const bool aliased = (res && ranges_overlap(out->data, ggml_nbytes(out), res, (size_t) n_embd*4)) || ranges_overlap(out->data, ggml_nbytes(out), ex->data, ggml_nbytes(ex)) ||
                             ranges_overlap(out->data, ggml_nbytes(out), pr->data, ggml_nbytes(pr)) || ranges_overlap(out->data, ggml_nbytes(out), ids->data, ggml_nbytes(ids));
        if (defer_on && !aliased && jq > 0 && c->use_fusion && mul_mat_vec_q_stream_enabled() && n_embd <= 4096 && ex->nb[1] % 16 == 0 &&
            g->nodes[jn]->op == GGML_OP_RMS_NORM && g->nodes[jn]->src[0] == out && is_row_vec_f32(out) &&
            g->nodes[jm2]->op == GGML_OP_MUL && (g->nodes[jm2]->src[0] == g->nodes[jn] || g->nodes[jm2]->src[1] == g->nodes[jn]) &&
            fusable_mmv(g->nodes[jq]) && g->nodes[jq]->src[1] == g->nodes[jm2] && g->nodes[jq]->src[0]->ne[0] == n_embd &&
            (n_embd % 256 == 0 ? (g->nodes[jq]->src[0]->type == GGML_TYPE_Q4_K || g->nodes[jq]->src[0]->type == GGML_TYPE_Q5_K || g->nodes[jq]->src[0]->type == GGML_TYPE_Q6_K ||
                                  g->nodes[jq]->src[0]->type == GGML_TYPE_Q8_0 || g->nodes[jq]->src[0]->type == GGML_TYPE_Q4_0)
                               : (n_embd % 320 == 0 && (g->nodes[jq]->src[0]->type == GGML_TYPE_Q8_0 || g->nodes[jq]->src[0]->type == GGML_TYPE_MXFP4)))) {
            pp_flush(c);
            c->pass.pp.active = true; c->pass.pp.res = res; c->pass.pp.x_out = (float *) out->data; c->pass.pp.n_planes = (int) n_used; c->pass.pp.m = n_embd;
            c->pass.pp.planes = (const float *) ex->data; c->pass.pp.stride = (int)(ex->nb[1]/4);
            c->pass.pp.probs = direct ? c->moe_ws + 64 : (const float *) pr->data; c->pass.pp.probs_bytes = direct ? 32 : ggml_nbytes(pr); c->pass.pp.ids = direct ? nullptr : (const int32_t *) ids->data; c->pass.pp.mode = mode;
            return jl - i + 1;
        }
    }
    moe_combine(direct ? c->moe_ws + 64 : (const float *) pr->data, direct ? nullptr : (const int32_t *) ids->data, (int) n_used, mode, ex->data, ex->nb[1], n_embd, res, (float *) out->data, c->stream);
    c->cnt.kernels_launched++;
    return jl - i + 1;
}

// MUL_MAT_ID for ONE token as grouped launches of the persistent mat-vec kernel, one group per used expert (the expert index is read
// on the device): up + gate + SwiGLU of build_moe_ffn in one launch (src/llama-graph.cpp:923-947), any other one-token MUL_MAT_ID
// (the down projection: one activation vector per expert, :981) in one launch with the f32 -> int8 quantization in its prologue
static bool moe_mmv_ok(const struct ggml_tensor * n) {
    if (n->op != GGML_OP_MUL_MAT_ID) return false;
    const struct ggml_tensor * as = n->src[0]; const struct ggml_tensor * b = n->src[1]; const struct ggml_tensor * ids = n->src[2];
    if (!ggml_is_quantized(as->type) || !mul_mat_vec_q_supported((int) as->type) || as->nb[0] != ggml_type_size(as->type) || as->ne[3] != 1) return false;
    if (ids->type != GGML_TYPE_I32 || ids->ne[1] != 1 || ids->ne[2] != 1 || ids->nb[0] != 4 || ids->ne[0] < 1 || ids->ne[0] > MMVQ_MAX_GROUPS) return false;
    if (b->type != GGML_TYPE_F32 || b->ne[2] != 1 || b->ne[3] != 1 || b->nb[0] != 4 || !(b->ne[1] == 1 || b->ne[1] == ids->ne[0])) return false;
    if (((uintptr_t) b->data % 16) || (b->ne[1] > 1 && b->nb[1] % 16) || n->type != GGML_TYPE_F32 || n->nb[0] != 4) return false;
    const int64_t K = as->ne[0];
    return mul_mat_vec_q_fused_supported(K, act_kind_for((int) as->type)) && mul_mat_vec_q_fused_prologue_supported(K, act_kind_for((int) as->type)) && as->ne[1] < (1 << 30);
}
static int try_fused_moe_experts(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    struct ggml_tensor * up = g->nodes[i];
    if (!moe_mmv_ok(up)) return 0;
    const struct ggml_tensor * as = up->src[0]; const struct ggml_tensor * b = up->src[1]; const struct ggml_tensor * ids = up->src[2];
    const int n_used = (int) ids->ne[0];
    const int64_t K = as->ne[0], M = as->ne[1];
    mmvq_input in = {};
    in.act_kind = act_kind_for((int) as->type); in.mode = PRO_QUANT; in.x = (const float *) b->data;
    mmvq_group grp[MMVQ_MAX_GROUPS];
    // up, gate (in either order: the graph lists a node's sources depth-first), each optionally followed by its ADD_ID bias, then
    // swiglu_split(gate, up) or swiglu_oai(gate, up) (src/llama-graph.cpp:923-968)
    if (b->ne[1] == 1 && is_internal(c, up)) {
        auto bias_of = [&](struct ggml_tensor * mm, int & j) -> struct ggml_tensor * {      // the ADD_ID that consumes mm, if it is next
            const int jn = next_real(g, j);
            if (jn < 0) return nullptr;
            struct ggml_tensor * ad = g->nodes[jn];
            if (ad->op != GGML_OP_ADD_ID || ad->src[0] != mm || ad->src[2] != ids || ad->type != GGML_TYPE_F32 || !is_internal(c, ad)) return nullptr;
            const struct ggml_tensor * bt = ad->src[1];
            if (bt->type != GGML_TYPE_F32 || bt->ne[0] != M || bt->nb[0] != 4 || bt->nb[1] != (size_t) M*4 || bt->ne[1] != as->ne[2]) return nullptr;
            j = jn;
            return ad;
        };
        int j = i;
        struct ggml_tensor * a_b = bias_of(up, j);
        const int jo = next_real(g, j);
        struct ggml_tensor * other = jo > 0 ? g->nodes[jo] : nullptr;
        if (other && moe_mmv_ok(other) && other->src[1] == b && other->src[2] == ids && other->src[0]->type == as->type && other->src[0]->ne[0] == K &&
            other->src[0]->ne[1] == M && other->src[0]->nb[1] == as->nb[1] && other->src[0]->nb[2] == as->nb[2] && is_internal(c, other)) {
            j = jo;
            struct ggml_tensor * o_b = bias_of(other, j);
            const int jg = next_real(g, j);
            struct ggml_tensor * gl = jg > 0 ? g->nodes[jg] : nullptr;
            struct ggml_tensor * a_out = a_b ? a_b : up; struct ggml_tensor * o_out = o_b ? o_b : other;
            if (gl && gl->op == GGML_OP_GLU && gl->op_params[1] == 0 && (!a_b) == (!o_b) &&
                (ggml_get_glu_op(gl) == GGML_GLU_OP_SWIGLU || ggml_get_glu_op(gl) == GGML_GLU_OP_SWIGLU_OAI) &&
                ((gl->src[0] == o_out && gl->src[1] == a_out) || (gl->src[0] == a_out && gl->src[1] == o_out)) &&
                gl->type == GGML_TYPE_F32 && gl->nb[0] == 4 && gl->ne[0] == M && gl->ne[1] == n_used && ggml_nelements(gl) == M*n_used &&
                !ranges_overlap(gl->data, ggml_nbytes(gl), b->data, ggml_nbytes(b))) {
                // out = act(src0) * src1: src0 is the gate side
                const bool a_is_gate = gl->src[0] == a_out;
                const struct ggml_tensor * mm_gate = a_is_gate ? up : other; const struct ggml_tensor * mm_up = a_is_gate ? other : up;
                const struct ggml_tensor * bg = a_is_gate ? a_b : o_b; const struct ggml_tensor * bu = a_is_gate ? o_b : a_b;
                const bool oai = ggml_get_glu_op(gl) == GGML_GLU_OP_SWIGLU_OAI;
                for (int u = 0; u < n_used; u++) {
                    grp[u] = { (const char *) mm_gate->src[0]->data, (const char *) mm_up->src[0]->data, as->nb[1], (int) M, (int) as->type,
                               (float *) ((char *) gl->data + (size_t) u*gl->nb[1]), EPI_GLU, nullptr, nullptr, nullptr, 0, 0,
                               (const int32_t *) ids->data + u, as->nb[2], 0,
                               bg ? (const float *) bg->src[1]->data : nullptr, bu ? (const float *) bu->src[1]->data : nullptr,
                               oai ? op_f32(gl, 2) : 0.0f, oai ? op_f32(gl, 3) : 0.0f };
                }
                if (!mul_mat_vec_q_fused_takes(grp, n_used, K, in, nullptr)) return 0;
                emit_mmv(c, grp, n_used, K, in, nullptr, nullptr, (uint64_t) 2*n_used*M*ggml_row_size(as->type, K));
                return jg - i + 1;
            }
        }
    }
    // a single one-token MUL_MAT_ID, optionally followed by its ADD_ID bias (gpt-oss's ffn_down_exps.bias, src/llama-graph.cpp:979-983)
    if (ranges_overlap(up->data, ggml_nbytes(up), b->data, ggml_nbytes(b))) return 0;
    struct ggml_tensor * out = up; const struct ggml_tensor * bias = nullptr; int consumed = 1;
    {
        const int jn = next_real(g, i);
        struct ggml_tensor * ad = jn > 0 ? g->nodes[jn] : nullptr;
        if (ad && ad->op == GGML_OP_ADD_ID && ad->src[0] == up && ad->src[2] == ids && ad->type == GGML_TYPE_F32 && is_internal(c, up) && ggml_are_same_shape(ad, up) &&
            ad->nb[0] == 4 && ad->nb[1] == up->nb[1] && ad->src[1]->type == GGML_TYPE_F32 && ad->src[1]->ne[0] == M && ad->src[1]->nb[0] == 4 &&
            ad->src[1]->nb[1] == (size_t) M*4 && ad->src[1]->ne[1] == as->ne[2] && !ranges_overlap(ad->data, ggml_nbytes(ad), b->data, ggml_nbytes(b))) {
            out = ad; bias = ad->src[1]; consumed = jn - i + 1;
        }
    }
    for (int u = 0; u < n_used; u++) {
        grp[u] = { (const char *) as->data, nullptr, as->nb[1], (int) M, (int) as->type, (float *) ((char *) out->data + (size_t) u*out->nb[1]), bias ? EPI_ADD : EPI_NONE,
                   bias ? (const float *) bias->data : nullptr, nullptr, nullptr, 0, 0, (const int32_t *) ids->data + u, as->nb[2], b->ne[1] > 1 ? (int)((size_t) u*b->nb[1]/4) : 0 };
        grp[u].res_eid = bias ? 1 : 0;
    }
    if (!mul_mat_vec_q_fused_takes(grp, n_used, K, in, nullptr)) return 0;
    emit_mmv(c, grp, n_used, K, in, nullptr, nullptr, (uint64_t) n_used*M*ggml_row_size(as->type, K));
    return consumed;
}

// Prompt pass: the slot sum that ends build_moe_ffn (src/llama-graph.cpp:996-1012) — ADD(view 0, view 1), ADD(., view 2), ... over the n_used slot views of the
// weighted experts' outputs — and the residual ADD behind it (src/llama-model.cpp:6096) as one pass instead of n_used launches
static int try_fused_slot_sum(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    struct ggml_tensor * ad = g->nodes[i];
    const struct ggml_tensor * v0 = ad->src[0]; const struct ggml_tensor * v1 = ad->src[1];
    if (ad->type != GGML_TYPE_F32 || !v0 || !v1 || !v0->view_src || v0->view_src != v1->view_src) return 0;
    const struct ggml_tensor * ex = v0->view_src;
    const int64_t M = ex->ne[0], n_used = ex->ne[1], T = ex->ne[2];
    if (ex->type != GGML_TYPE_F32 || ex->ne[3] != 1 || n_used < 2 || n_used > 8 || T < 2 || M % 4 || ex->nb[0] != 4 || ex->nb[1] % 16 || ex->nb[2] % 16 || ((uintptr_t) ex->data % 16)) return 0;
    auto is_slot = [&](const struct ggml_tensor * v, int64_t u) {
        return v->view_src == ex && v->type == GGML_TYPE_F32 && v->ne[0] == M && v->ne[1] == T && v->ne[2] == 1 && v->ne[3] == 1 && v->nb[0] == 4 && v->nb[1] == ex->nb[2] &&
               (const char *) v->data == (const char *) ex->data + u*ex->nb[1];
    };
    if (!is_slot(v0, 0) || !is_slot(v1, 1)) return 0;
    int jl = i; const struct ggml_tensor * prev = ad;
    for (int64_t u = 2; u < n_used; u++) {
        if (!is_internal(c, prev)) return 0;
        const int ja = next_real(g, jl); if (ja < 0) return 0;
        const struct ggml_tensor * a2 = g->nodes[ja];
        if (a2->op != GGML_OP_ADD || a2->type != GGML_TYPE_F32 || a2->src[0] != prev || !is_slot(a2->src[1], u)) return 0;
        prev = a2; jl = ja;
    }
    struct ggml_tensor * out = g->nodes[jl];
    const struct ggml_tensor * res = nullptr;
    if (is_internal(c, out)) {
        const int jr = next_real(g, jl);
        struct ggml_tensor * ra = jr > 0 ? g->nodes[jr] : nullptr;
        if (ra && ra->op == GGML_OP_ADD && ra->type == GGML_TYPE_F32 && (ra->src[0] == out || ra->src[1] == out)) {
            const struct ggml_tensor * r = ra->src[0] == out ? ra->src[1] : ra->src[0];
            if (r != out && r->type == GGML_TYPE_F32 && ggml_are_same_shape(r, out) && ggml_are_same_shape(ra, out) && r->nb[0] == 4 && r->nb[1] % 16 == 0 && ((uintptr_t) r->data % 16) == 0) {
                res = r; out = ra; jl = jr;
            }
        }
    }
    if (out->ne[0] != M || out->ne[1] != T || out->ne[2] != 1 || out->ne[3] != 1 || out->nb[0] != 4 || out->nb[1] % 16 || ((uintptr_t) out->data % 16)) return 0;
    // every element is read and written by the same lane, so `out` may be the residual's or slot 0's own memory (an in-place ADD) — but not a shifted overlap
    if ((out->data != ex->data || out->nb[1] != ex->nb[2]) && ranges_overlap(out->data, ggml_nbytes(out), ex->data, ggml_nbytes(ex))) return 0;
    if (res && (out->data != res->data || out->nb[1] != res->nb[1]) && ranges_overlap(out->data, ggml_nbytes(out), res->data, ggml_nbytes(res))) return 0;
    moe_slot_sum(ex->data, ex->nb[1], ex->nb[2], (int) n_used, M, T, res ? (const float *) res->data : nullptr, res ? res->nb[1] : 0, (float *) out->data, out->nb[1], c->stream);
    c->cnt.kernels_launched++;
    return jl - i + 1;
}

// Prompt pass (many tokens) through the experts of build_moe_ffn (src/llama-graph.cpp:914-990):
//   MUL_MAT_ID(up) [ADD_ID] ; MUL_MAT_ID(gate) [ADD_ID] ; GLU (swiglu | swiglu_oai) ; MUL_MAT_ID(down) [ADD_ID] [MUL weights]
// as: ONE bf16 copy of the layer input, ONE sort of the (token, slot) pairs by expert, ONE dual tile launch (both products of an expert's pairs against one
// activation tile, biases and the GLU in its epilogue, result as bf16 rows per pair) and ONE tile launch for the down projection reading those rows (bias and routing
// weight in its epilogue). Node by node the same work is 3 copies + 3 sorts + 3 tile launches + up to 5 element kernels, and every expert's gate and up tiles stage the same
// activation rows twice. The down half is taken only if it follows directly; intermediates are skipped only if nobody else reads them.
static bool moe_mmq_ok(const struct ggml_tensor * n) {
    if (n->op != GGML_OP_MUL_MAT_ID) return false;
    const struct ggml_tensor * as = n->src[0]; const struct ggml_tensor * b = n->src[1]; const struct ggml_tensor * ids = n->src[2];
    if (!ggml_is_quantized(as->type) || act_kind_for((int) as->type) < 0 || as->nb[0] != ggml_type_size(as->type) || as->ne[3] != 1) return false;
    if (ids->type != GGML_TYPE_I32 || ids->ne[2] != 1 || ids->ne[3] != 1) return false;
    const int64_t n_used = ids->ne[0], n_tokens = ids->ne[1];
    if (n_used*n_tokens <= 4*MMVQ_MAX_N || !mul_mat_q_id_supported(as->ne[2], n_used, n_tokens)) return false;
    if (b->type != GGML_TYPE_F32 || b->nb[0] != 4 || b->ne[2] != n_tokens || b->ne[3] != 1 || !(b->ne[1] == 1 || b->ne[1] == n_used)) return false;
    return n->type == GGML_TYPE_F32 && n->nb[0] == 4 && n->ne[0] == as->ne[1] && n->ne[1] == n_used && n->ne[2] == n_tokens && n->ne[3] == 1;
}
static int try_fused_prefill_moe(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    static const bool on = env_on("GGML_MI355X_PREFILL_MOE");
    if (!on) return 0;
    struct ggml_tensor * up = g->nodes[i];
    if (!moe_mmq_ok(up) || up->src[1]->ne[1] != 1 || !is_internal(c, up)) return 0;
    const struct ggml_tensor * as = up->src[0]; const struct ggml_tensor * b = up->src[1]; const struct ggml_tensor * ids = up->src[2];
    const int64_t K = as->ne[0], M = as->ne[1], E = as->ne[2], n_used = ids->ne[0], n_tokens = ids->ne[1];
    if (M % 64 != 0) return 0;                  // the GLU rows are the down projection's bf16 activation rows: no padding between them
    auto bias_of = [&](struct ggml_tensor * mm, const struct ggml_tensor * w, int & j) -> struct ggml_tensor * {      // the ADD_ID that consumes mm, if it is next
        const int jn = next_real(g, j);
        if (jn < 0) return nullptr;
        struct ggml_tensor * ad = g->nodes[jn];
        if (ad->op != GGML_OP_ADD_ID || ad->src[0] != mm || ad->src[2] != ids || ad->type != GGML_TYPE_F32 || !ggml_are_same_shape(ad, mm) || ad->nb[0] != 4) return nullptr;
        const struct ggml_tensor * bt = ad->src[1];
        if (bt->type != GGML_TYPE_F32 || bt->ne[0] != w->ne[1] || bt->nb[0] != 4 || bt->nb[1] % 4 || bt->ne[1] != w->ne[2] || !is_internal(c, mm)) return nullptr;
        j = jn;
        return ad;
    };
    int j = i;
    struct ggml_tensor * a_b = bias_of(up, as, j);
    if (a_b && !is_internal(c, a_b)) return 0;
    const int jo = next_real(g, j);
    struct ggml_tensor * other = jo > 0 ? g->nodes[jo] : nullptr;
    if (!other || !moe_mmq_ok(other) || other->src[1] != b || other->src[2] != ids || other->src[0]->type != as->type || other->src[0]->ne[0] != K || other->src[0]->ne[1] != M ||
        other->src[0]->ne[2] != E || other->src[0]->nb[1] != as->nb[1] || other->src[0]->nb[2] != as->nb[2] || !is_internal(c, other)) return 0;
    j = jo;
    struct ggml_tensor * o_b = bias_of(other, other->src[0], j);
    if ((o_b && !is_internal(c, o_b)) || (!a_b) != (!o_b)) return 0;
    if (a_b && a_b->src[1]->nb[1] != o_b->src[1]->nb[1]) return 0;
    const int jg = next_real(g, j);
    struct ggml_tensor * gl = jg > 0 ? g->nodes[jg] : nullptr;
    struct ggml_tensor * a_out = a_b ? a_b : up; struct ggml_tensor * o_out = o_b ? o_b : other;
    if (!gl || gl->op != GGML_OP_GLU || gl->op_params[1] != 0 || (ggml_get_glu_op(gl) != GGML_GLU_OP_SWIGLU && ggml_get_glu_op(gl) != GGML_GLU_OP_SWIGLU_OAI) ||
        !((gl->src[0] == o_out && gl->src[1] == a_out) || (gl->src[0] == a_out && gl->src[1] == o_out)) || gl->type != GGML_TYPE_F32 || gl->nb[0] != 4 ||
        gl->ne[0] != M || gl->ne[1] != n_used || gl->ne[2] != n_tokens || gl->ne[3] != 1) return 0;
    const bool a_is_gate = gl->src[0] == a_out;           // out = act(src0) * src1: src0 is the gate side
    const struct ggml_tensor * w_gate = (a_is_gate ? up : other)->src[0]; const struct ggml_tensor * w_up = (a_is_gate ? other : up)->src[0];
    const struct ggml_tensor * bg = a_is_gate ? a_b : o_b; const struct ggml_tensor * bu = a_is_gate ? o_b : a_b;
    const bool oai = ggml_get_glu_op(gl) == GGML_GLU_OP_SWIGLU_OAI;

    // the down half: MUL_MAT_ID(down, gl, ids) [ADD_ID] [MUL weights], directly behind the GLU
    int consumed_to = jg, between_from = 0, between_to = 0;       // [between_from, between_to): the routing weights' nodes between the down product and its MUL
    struct ggml_tensor * down = nullptr; struct ggml_tensor * d_out = nullptr; const struct ggml_tensor * d_bias = nullptr; const struct ggml_tensor * d_scale = nullptr;
    {
        const int jd = next_real(g, jg);
        struct ggml_tensor * dn = jd > 0 ? g->nodes[jd] : nullptr;
        if (dn && moe_mmq_ok(dn) && dn->src[1] == gl && dn->src[2] == ids && dn->src[0]->ne[0] == M && dn->src[0]->ne[2] == E && dn->nb[0] == 4) {
            down = dn; d_out = dn; consumed_to = jd;
            int jj = jd;
            struct ggml_tensor * ad = bias_of(dn, dn->src[0], jj);
            if (ad) { d_out = ad; d_bias = ad->src[1]; consumed_to = jj; }
            // MUL(experts, weights): the graph lists a node's sources depth-first, so the routing weights' own nodes (GET_ROWS of the probabilities, their
            // normalisation: src/llama-graph.cpp:887-908) sit BETWEEN the down product and the MUL. They do not depend on anything of this chain: they are
            // computed first (node by node), then the down launch applies the weight in its epilogue.
            int jm = jj; bool between_ok = true;
            for (int hop = 0; hop < 12; hop++) {
                jm = next_real(g, jm);
                if (jm < 0) break;
                const struct ggml_tensor * t = g->nodes[jm];
                if (t->op == GGML_OP_MUL && t->src[0] == d_out) break;
                const bool light = t->op == GGML_OP_GET_ROWS || t->op == GGML_OP_SOFT_MAX || t->op == GGML_OP_SUM_ROWS || t->op == GGML_OP_DIV || t->op == GGML_OP_SCALE;
                bool reads_chain = false;
                for (int q = 0; q < GGML_MAX_SRC; q++) {
                    const struct ggml_tensor * sq = t->src[q];
                    while (sq) { if (sq == up || sq == other || sq == a_out || sq == o_out || sq == gl || sq == dn || sq == d_out) reads_chain = true; sq = sq->view_src; }
                }
                if (!light || reads_chain) { between_ok = false; break; }
            }
            struct ggml_tensor * ml = jm > 0 && between_ok ? g->nodes[jm] : nullptr;
            if (ml && ml->op == GGML_OP_MUL && ml->src[0] == d_out && is_internal(c, d_out) && ml->type == GGML_TYPE_F32 && ggml_are_same_shape(ml, d_out) && ml->nb[0] == 4) {
                const struct ggml_tensor * wt = ml->src[1];
                if (wt->type == GGML_TYPE_F32 && wt->ne[0] == 1 && wt->ne[1] == n_used && wt->ne[2] == n_tokens && wt->ne[3] == 1 &&
                    !ranges_overlap(ml->data, ggml_nbytes(ml), wt->data, ggml_nbytes(wt))) { d_scale = wt; d_out = ml; between_from = jj + 1; between_to = jm; consumed_to = jm; }
            }
        }
    }
    const mmq_moe_plan pl = mul_mat_q_id_plan(c->scratch, K, n_tokens, n_used, E, M, c->moe_dual);
    if (pl.bytes > c->scratch_size) return 0;
    const bool gl_f32 = !down || !is_internal(c, gl);      // somebody else reads the GLU result as a tensor
    c->pass.drop_act();     // the scratch is reused
    // the up side's last tensor: in the two-launch form its memory holds the up product (+ bias) between the two launches, and the gate launch reads it while it writes the
    // GLU tensor: the same element by the same lane if they are one buffer, a race if they overlap otherwise
    struct ggml_tensor * u_out = a_is_gate ? o_out : a_out;
    if (!pl.dual && gl_f32 && gl->data != u_out->data && ranges_overlap(gl->data, ggml_nbytes(gl), u_out->data, ggml_nbytes(u_out))) return 0;
    mmq_moe_call gu = moe_call_of(c, w_gate, ids);
    gu.W2 = w_up->data; gu.b = (const float *) b->data; gu.b_nb1 = b->nb[1]; gu.b_nb2 = b->nb[2];
    gu.epi.oai = oai ? 1 : 0; gu.epi.alpha = oai ? op_f32(gl, 2) : 0.0f; gu.epi.limit = oai ? op_f32(gl, 3) : 0.0f;
    if (bg) { gu.epi.bias = (const float *) bg->src[1]->data; gu.epi.bias2 = (const float *) bu->src[1]->data; gu.epi.bias_stride = bg->src[1]->nb[1]/4; }
    if (!pl.dual) { gu.epi.glu_up = (const float *) u_out->data; gu.epi.glu_up_nb1 = u_out->nb[1]; gu.epi.glu_up_nb2 = u_out->nb[2]; }
    gu.dst = gl_f32 ? (float *) gl->data : nullptr; gu.dst_nb1 = gl->nb[1]; gu.dst_nb2 = gl->nb[2]; gu.y16 = down ? pl.y16 : nullptr;
    mul_mat_q_id_gate_up(gu, pl);
    c->cnt.mmq_launches += pl.dual ? 1 : 2; c->cnt.kernels_launched += pl.dual ? 3 : 4;      // copy, sort, the dual launch | the up and the gate launch
    c->cnt.weight_bytes += (uint64_t) 2*E*M*ggml_row_size(as->type, K);
    if (down) {
        if (between_to > between_from) {      // (not earlier: an allocator may have given these nodes the up tensor's memory, dead in graph order, which the gate launch reads)
            const bool uf = c->use_fusion; c->use_fusion = false;
            for (int q = between_from; q < between_to; ) q += compute_node(c, g, q);
            c->use_fusion = uf;
        }
        const struct ggml_tensor * ad = down->src[0];
        mmq_moe_call dc = moe_call_of(c, ad, ids);
        if (d_bias) { dc.epi.bias = (const float *) d_bias->data; dc.epi.bias_stride = d_bias->nb[1]/4; }
        if (d_scale) { dc.epi.scale = (const float *) d_scale->data; dc.epi.scale_nb0 = d_scale->nb[1]; dc.epi.scale_nb1 = d_scale->nb[2]; }
        dc.dst = (float *) d_out->data; dc.dst_nb1 = d_out->nb[1]; dc.dst_nb2 = d_out->nb[2];
        mul_mat_q_id_down(dc, pl);
        c->cnt.mmq_launches++; c->cnt.kernels_launched += pl.tile_down != pl.tile ? 2 : 1;      // (a second sort when the down launch's tiles differ)
        c->cnt.weight_bytes += (uint64_t) E*ad->ne[1]*ggml_row_size(ad->type, M);
    }
    return consumed_to - i + 1;
}

// MUL_MAT(F32 router weights, x) [-> ADD bias] [-> SOFT_MAX] -> ARGSORT desc, one token (src/llama-graph.cpp:838-883)
// norm / normw != NULL: x (= lg->src[1]) is MUL(RMS_NORM(norm->src[0]), normw), not computed yet: the router kernel computes it and writes it
static int try_fused_moe_route(mi_backend_ctx * c, struct ggml_cgraph * g, int i, const struct ggml_tensor * norm = nullptr, const struct ggml_tensor * normw = nullptr) {
    struct ggml_tensor * lg = g->nodes[i];
    const struct ggml_tensor * w = lg->src[0]; const struct ggml_tensor * x = lg->src[1];
    if (w->type != GGML_TYPE_F32 || x->type != GGML_TYPE_F32 || lg->type != GGML_TYPE_F32) return 0;
    const int64_t K = w->ne[0], E = w->ne[1];
    if (E < 2 || E > 256 || K % 4 || K >= (1ll << 30) || w->ne[2] != 1 || w->ne[3] != 1 || w->nb[0] != 4 || w->nb[1] % 16 || ((uintptr_t) w->data % 16)) return 0;
    if (!is_row_vec_f32(x) || x->ne[0] != K || !ggml_is_contiguous(lg) || ggml_nelements(lg) != E) return 0;
    int j = next_real(g, i); if (j < 0) return 0;
    const struct ggml_tensor * cur = lg; const float * bias = nullptr; float * logits_out = nullptr;
    struct ggml_tensor * nd = g->nodes[j];
    if (nd->op == GGML_OP_ADD && (nd->src[0] == cur || nd->src[1] == cur) && ggml_is_contiguous(nd) && ggml_nelements(nd) == E && is_internal(c, cur)) {
        const struct ggml_tensor * bt = nd->src[0] == cur ? nd->src[1] : nd->src[0];
        if (bt->type != GGML_TYPE_F32 || !ggml_is_contiguous(bt) || ggml_nelements(bt) != E) return 0;
        bias = (const float *) bt->data; cur = nd;
        j = next_real(g, j); if (j < 0) return 0;
        nd = g->nodes[j];
    }
    float * probs_out = nullptr; bool softmax = false;
    if (nd->op == GGML_OP_SOFT_MAX && nd->src[0] == cur && !nd->src[1] && !nd->src[2] && op_f32(nd, 0) == 1.0f && op_f32(nd, 1) == 0.0f &&
        ggml_is_contiguous(nd) && ggml_nelements(nd) == E && is_internal(c, cur)) {
        softmax = true; probs_out = (float *) nd->data; cur = nd;
        j = next_real(g, j); if (j < 0) return 0;
        nd = g->nodes[j];
    } else {
        logits_out = (float *) cur->data;      // the logits themselves are gathered later (SOFTMAX_WEIGHT gating)
    }
    if (nd->op != GGML_OP_ARGSORT || nd->src[0] != cur || nd->op_params[0] != GGML_SORT_ORDER_DESC || nd->type != GGML_TYPE_I32 ||
        !ggml_is_contiguous(nd) || ggml_nelements(nd) != E) return 0;
    static const bool topv_on = env_on("GGML_MI355X_MOE_TOPV");
    float * topv = topv_on && c->moe_ws ? c->moe_ws + 64 : nullptr;
    if (norm) {
        if (!moe_route_norm_supported(K, E, c->moe_ws) || ((uintptr_t) normw->data % 16) || ((uintptr_t) norm->src[0]->data % 16) || ((uintptr_t) x->data % 16)) return 0;
        moe_route((const float *) w->data, w->nb[1], (const float *) norm->src[0]->data, bias, K, E, softmax, logits_out, probs_out, (int32_t *) nd->data, c->stream, c->moe_ws,
                  (const float *) normw->data, op_f32(norm, 0), (float *) x->data, c->err_dev, topv);
    } else {
        moe_route((const float *) w->data, w->nb[1], (const float *) x->data, bias, K, E, softmax, logits_out, probs_out, (int32_t *) nd->data, c->stream, c->moe_ws, nullptr, 0.0f, nullptr, c->err_dev, topv);
    }
    c->pass.rt.valid = topv != nullptr; c->pass.rt.vals = softmax ? (const void *) probs_out : (const void *) logits_out; c->pass.rt.sorted = nd->data;
    c->pass.rt.bytes = (size_t) E*4; c->pass.rt.lo = i; c->pass.rt.hi = j;
    c->cnt.kernels_launched++;
    return j - i + 1;
}

// Prefill: MUL_MAT(gate) ; MUL_MAT(up) -> GLU(swiglu) on the same many-token activations (build_ffn, src/llama-graph.cpp:646-691) as one
// matrix-core kernel (mmq.hip DUAL): neither product is written, the GLU kernel is gone and the activation tile is staged once.
static int try_fused_prefill_glu(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    static const bool on = env_on("GGML_MI355X_PREFILL_GLU");
    if (!on) return 0;
    struct ggml_tensor * n = g->nodes[i];
    const struct ggml_tensor * a = n->src[0]; const struct ggml_tensor * b = n->src[1];
    if (!ggml_is_quantized(a->type) || b->type != GGML_TYPE_F32 || b->ne[1] <= MMVQ_MAX_N || b->ne[2] != 1 || b->ne[3] != 1 || a->ne[2] != 1 || a->ne[3] != 1 ||
        b->nb[0] != 4 || !mul_mat_q_glu_supported(a->ne[1], b->ne[1]) || !is_internal(c, n)) return 0;
    const int j = next_real(g, i); if (j < 0) return 0;
    struct ggml_tensor * nx = g->nodes[j];
    if (nx->op != GGML_OP_MUL_MAT || nx->src[1] != b || tensor_is_split(nx->src[0]) || nx->src[0]->type != a->type || !ggml_are_same_shape(nx->src[0], a) || nx->src[0]->nb[1] != a->nb[1] ||
        !is_internal(c, nx)) return 0;
    const int j2 = next_real(g, j); if (j2 < 0) return 0;
    struct ggml_tensor * gl = g->nodes[j2];
    if (gl->op != GGML_OP_GLU || ggml_get_glu_op(gl) != GGML_GLU_OP_SWIGLU || gl->op_params[1] != 0 || gl->src[1] == NULL || gl->type != GGML_TYPE_F32 ||
        !ggml_is_contiguous(gl) || !((gl->src[0] == nx && gl->src[1] == n) || (gl->src[0] == n && gl->src[1] == nx))) return 0;
    const int64_t K = a->ne[0], M = a->ne[1], N = b->ne[1];
    if (mul_mat_q_scratch_bytes(K, N, M) > c->scratch_size) return 0;
    const bool ready = c->pass.bf16_at(b->data, K, N, b->nb[1]) == 0;      // (at the start only: this launch reads its activations there)
    // ffn_down reads the result next: the kernel writes its bf16 copy (above this kernel's own activation copy) instead of the f32 tensor
    const struct ggml_tensor * down = prefill_mm_consumer(c, g, j2, gl);
    const size_t off2 = mul_mat_q_x_bytes(K, N);
    const bool y16 = down && off2 + mul_mat_q_scratch_bytes(M, N, down->src[0]->ne[1]) <= c->scratch_size;
    prof_begin(c, (int) a->type, 2*M, K, N, (uint64_t) 2*M*ggml_row_size(a->type, K));
    mmq_call mc = {};
    mc.type = (int) a->type; mc.W = gl->src[0]->src[0]->data; mc.W2 = gl->src[1]->src[0]->data; mc.w_row_stride = a->nb[1]; mc.m = M; mc.stream = c->stream;
    mc.act = { (const float *) b->data, b->nb[1], K, N, c->scratch, c->scratch_size, ready };
    mc.dst = y16 ? nullptr : (float *) gl->data; mc.dst_stride = gl->nb[1]; mc.y16 = y16 ? (uint16_t *) ((char *) c->scratch + off2) : nullptr;
    mul_mat_q_glu(mc);
    prof_end(c);
    if (ready) c->cnt.act_quant_reused++;
    if (y16) c->pass.produced_bf16(i, j2, gl->data, M, N, gl->nb[1], off2);
    else if (!ready) c->pass.converted_bf16(b->data, K, N, b->nb[1]);
    c->cnt.mmq_launches++; c->cnt.kernels_launched += ready ? 1 : 2;
    c->cnt.weight_bytes += (uint64_t) 2*M*ggml_row_size(a->type, K);
    return j2 - i + 1;
}


// Prefill: the mat-muls that directly follow each other on the same many-token activations — wq / wk / wv of build_attn
// (src/llama-model.cpp:6017-6040), each optionally followed by its (RESHAPE ->) ROPE — as ONE launch of 256-token tiles: alone, wk / wv
// (1024 rows) are 32 tiles on 256 CUs. The ROPEs run after the launch, i.e. later than in graph order relative to the following
// mat-muls: allowed only if no output of one chain overlaps an output of another (the allocator may have recycled a dead buffer).
static int try_fused_prefill_qkv(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    static const bool on = env_on("GGML_MI355X_PREFILL_QKV");
    if (!on) return 0;
    const struct ggml_tensor * b = g->nodes[i]->src[1];
    // a chain: MUL_MAT [-> ADD bias (gpt-oss's bq / bk / bv, src/llama-model.cpp:17636-17645)] [-> (RESHAPE ->) ROPE]; the ADDs run as their own launches behind the
    // grouped mat-mul, like ROPEs that cannot ride on it
    struct chain { int mm, add, rope, end; } ch[3];
    int nc = 0, at = i; bool any_add = false;
    while (nc < 3 && at >= 0) {
        struct ggml_tensor * n = g->nodes[at];
        if (n->op != GGML_OP_MUL_MAT) break;
        const struct ggml_tensor * a = n->src[0];
        if (n->src[1] != b || !ggml_is_quantized(a->type) || tensor_is_split(a) || b->type != GGML_TYPE_F32 || b->ne[1] <= MMVQ_MAX_N || b->ne[2] != 1 || b->ne[3] != 1 ||
            a->ne[2] != 1 || a->ne[3] != 1 || b->nb[0] != 4 || a->ne[0] != g->nodes[i]->src[0]->ne[0] || n->nb[0] != 4) break;
        ch[nc] = { at, -1, -1, at };
        const struct ggml_tensor * last = n;
        int j = next_real(g, at);
        if (j > 0 && g->nodes[j]->op == GGML_OP_ADD && (g->nodes[j]->src[0] == n || g->nodes[j]->src[1] == n) && g->nodes[j]->src[0] != b && g->nodes[j]->src[1] != b) {
            ch[nc].add = j; ch[nc].end = j; last = g->nodes[j]; any_add = true;
            j = next_real(g, j);
        }
        if (j > 0 && g->nodes[j]->op == GGML_OP_ROPE && base_of(g->nodes[j]->src[0]) == last) { ch[nc].rope = j; ch[nc].end = j; }
        nc++;
        at = next_real(g, ch[nc - 1].end);
    }
    if (nc < 2) return 0;
    for (int q = 0; q < nc; q++) {
        const struct ggml_tensor * oq[3] = { g->nodes[ch[q].mm], ch[q].rope >= 0 ? g->nodes[ch[q].rope] : nullptr, ch[q].add >= 0 ? g->nodes[ch[q].add] : nullptr };
        for (int u = 0; u < 3; u++) {
            if (!oq[u]) continue;
            if (ranges_overlap(oq[u]->data, ggml_nbytes(oq[u]), b->data, ggml_nbytes(b))) return 0;
            for (int r = q + 1; r < nc; r++) {
                const struct ggml_tensor * orr[3] = { g->nodes[ch[r].mm], ch[r].rope >= 0 ? g->nodes[ch[r].rope] : nullptr, ch[r].add >= 0 ? g->nodes[ch[r].add] : nullptr };
                for (int v = 0; v < 3; v++) if (orr[v] && ranges_overlap(oq[u]->data, ggml_nbytes(oq[u]), orr[v]->data, ggml_nbytes(orr[v]))) return 0;
            }
        }
    }
    const int64_t K = b->ne[0], N = b->ne[1];
    const bool ready = c->pass.bf16_at(b->data, K, N, b->nb[1]) == 0;      // (at the start only: this launch reads its activations there)
    mmq_multi_call plain = {};      // the plain grouped launch: every mat-mul writes its own tensor, the ADDs and ROPEs run behind it
    plain.nseg = nc; plain.stream = c->stream; plain.act = { (const float *) b->data, b->nb[1], K, N, c->scratch, c->scratch_size, ready };
    uint64_t wbytes = 0; int64_t m_tot = 0;
    for (int q = 0; q < nc; q++) {
        const struct ggml_tensor * n = g->nodes[ch[q].mm]; const struct ggml_tensor * a = n->src[0]; mmq_multi_seg & sg = plain.seg[q];
        sg.type = (int) a->type; sg.W = a->data; sg.w_row_stride = a->nb[1]; sg.m = a->ne[1]; sg.dst = (float *) n->data; sg.dst_stride = n->nb[1];
        wbytes += (uint64_t) a->ne[1]*ggml_row_size(a->type, a->ne[0]); m_tot += a->ne[1];
    }
    // the ROPEs go into the launch (epilogue, or the pass that combines split-k planes) when they are NORM-mode, share one descriptor and
    // are the only readers of their mat-muls: the mat-mul then writes the ROPE node's tensor directly
    mmq_multi_call roped = plain; bool have_rd = false, rope_ok = !any_add;
    for (int q = 0; q < nc && rope_ok; q++) {
        if (ch[q].rope < 0) continue;
        const struct ggml_tensor * mm = g->nodes[ch[q].mm]; const struct ggml_tensor * rp = g->nodes[ch[q].rope];
        const mmvq_rope r1 = mmvq_rope_of(rp);
        rope_ok = rp->op_params[2] == 0 && rp->type == GGML_TYPE_F32 && ggml_is_contiguous(rp) && rp->src[1]->type == GGML_TYPE_I32 && rp->ne[3] == 1 &&
                  rp->ne[2] == b->ne[1] && rp->ne[0]*rp->ne[1] == mm->ne[0] && rp->op_params[1] % 2 == 0 && rp->op_params[1] <= rp->ne[0] && rp->ne[0] % 4 == 0 &&
                  ggml_nelements(rp->src[1]) == b->ne[1] && is_internal(c, mm) && (rp->src[0] == mm || is_internal(c, rp->src[0])) &&
                  (!have_rd || memcmp(&roped.rope, &r1, sizeof(r1)) == 0);
        roped.rope = r1; have_rd = true; roped.seg[q].rope = true; roped.seg[q].dst = (float *) rp->data; roped.seg[q].dst_stride = rp->nb[2];
    }
    const bool fuse_rope = have_rd && rope_ok;
    prof_begin(c, plain.seg[0].type, m_tot, K, N, wbytes);
    // the KV-cache writes that follow (SET_ROWS of rope(k) as f16 rows, SET_ROWS of v as an element scatter into the transposed cache — the pair
    // try_fused_kv_store takes) ride on the same combine pass
    int kv_last = -1;
    if (fuse_rope) {
        const int j1 = next_real(g, ch[nc - 1].end), j2 = j1 > 0 ? next_real(g, j1) : -1;
        if (j2 > 0 && g->nodes[j1]->op == GGML_OP_SET_ROWS && g->nodes[j2]->op == GGML_OP_SET_ROWS) {
            struct ggml_tensor * sk = g->nodes[j1]; struct ggml_tensor * sv = g->nodes[j2];
            const struct ggml_tensor * ks = sk->src[0]; const struct ggml_tensor * ki = sk->src[1];
            const struct ggml_tensor * vs = sv->src[0]; const struct ggml_tensor * vi = sv->src[1];
            int qk = -1, qv = -1;
            for (int q = 0; q < nc; q++) { if (ks->data == (void *) roped.seg[q].dst) qk = q; if (vs->data == (void *) roped.seg[q].dst) qv = q; }
            const int64_t mk = qk >= 0 ? roped.seg[qk].m : 0, mv = qv >= 0 ? roped.seg[qv].m : 0;
            const bool ok = qk >= 0 && qv >= 0 && qk != qv && sk->type == GGML_TYPE_F16 && sv->type == GGML_TYPE_F16 && ks->type == GGML_TYPE_F32 && vs->type == GGML_TYPE_F32 &&
                ki->type == GGML_TYPE_I64 && vi->type == GGML_TYPE_I64 && ggml_is_contiguous(ki) && ggml_is_contiguous(vi) &&
                ks->ne[0] == mk && ks->ne[1] == N && ks->ne[2] == 1 && ks->ne[3] == 1 && ks->nb[0] == 4 && ks->nb[1] == (size_t) mk*4 && roped.seg[qk].dst_stride == (size_t) mk*4 &&
                sk->nb[0] == 2 && sk->nb[1] % 8 == 0 && ((uintptr_t) sk->data % 8) == 0 && ggml_nelements(ki) == N && mk % 4 == 0 &&
                vs->ne[0] == 1 && vs->ne[1] == mv*N && vs->ne[2] == 1 && vs->ne[3] == 1 && vs->nb[1] == 4 && roped.seg[qv].dst_stride == (size_t) mv*4 &&
                sv->ne[0] == 1 && sv->nb[1] == 2 && ggml_nelements(vi) == mv*N &&
                !ranges_overlap(sk->data, ggml_nbytes(sk), b->data, ggml_nbytes(b)) && !ranges_overlap(sv->data, ggml_nbytes(sv), b->data, ggml_nbytes(b));
            if (ok) {
                mmq_multi_seg & gk = roped.seg[qk]; mmq_multi_seg & gv = roped.seg[qv];
                gk.st16 = (uint16_t *) sk->data; gk.st_idx = (const int64_t *) ki->data; gk.st_row_elems = (int64_t)(sk->nb[1]/2); gk.st_mode = 1;
                gv.st16 = (uint16_t *) sv->data; gv.st_idx = (const int64_t *) vi->data; gv.st_row_elems = 0; gv.st_mode = 2;
                kv_last = j2;
            }
        }
    }
    // bias rows (ADD behind a mat-mul, the mat-mul read by nobody else): the launch's epilogue adds them and writes the ADD's tensor
    mmq_multi_call biased = plain; bool bias_ok = any_add;
    for (int q = 0; q < nc && bias_ok; q++) {
        if (ch[q].add < 0) continue;
        const struct ggml_tensor * mm = g->nodes[ch[q].mm]; const struct ggml_tensor * ad = g->nodes[ch[q].add];
        const struct ggml_tensor * bt = ad->src[0] == mm ? ad->src[1] : ad->src[0];
        bias_ok = is_internal(c, mm) && ad->type == GGML_TYPE_F32 && ggml_are_same_shape(ad, mm) && ad->nb[0] == 4 && bt->type == GGML_TYPE_F32 && bt->ne[0] == mm->ne[0] &&
                  ggml_nelements(bt) == mm->ne[0] && bt->nb[0] == 4;
        biased.seg[q].bias = (const float *) bt->data; biased.seg[q].dst = (float *) ad->data; biased.seg[q].dst_stride = ad->nb[1];
    }
    // what the launcher takes: with the bias rows (no k split), else with the rotations and cache writes (a k split), else plain; none: the mat-muls run one by one
    const mmq_multi_call * take = bias_ok && mul_mat_q_multi_takes(biased) ? &biased : fuse_rope && mul_mat_q_multi_takes(roped) ? &roped :
                                  mul_mat_q_multi_takes(plain) ? &plain : nullptr;
    if (take) mul_mat_q_multi(*take);
    prof_end(c);
    if (!take) { if (c->profiling && !c->prof_suspend) c->prof.pop_back(); return 0; }
    if (ready) c->cnt.act_quant_reused++;
    else c->pass.converted_bf16(b->data, K, N, b->nb[1]);
    c->cnt.mmq_launches++; c->cnt.kernels_launched += ready ? 1 : 2; c->cnt.weight_bytes += wbytes;
    for (int q = 0; q < nc; q++) {      // what did not ride
        if (take != &biased && ch[q].add >= 0) compute_node(c, g, ch[q].add);
        if (take != &roped && ch[q].rope >= 0) compute_node(c, g, ch[q].rope);
    }
    return (take == &roped && kv_last >= 0 ? kv_last : ch[nc - 1].end) - i + 1;
}

// Prefill: MUL_MAT -> ADD(residual) (build_attn's wo, build_ffn's down: src/llama-model.cpp:6057,6096) — the residual is added in the
// mat-mul's epilogue, or by the pass that combines its split-k planes
static int try_fused_prefill_add(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    struct ggml_tensor * n = g->nodes[i];
    const struct ggml_tensor * a = n->src[0]; const struct ggml_tensor * b = n->src[1];
    if (!ggml_is_quantized(a->type) || b->type != GGML_TYPE_F32 || b->ne[1] <= MMVQ_MAX_N || b->ne[2] != 1 || b->ne[3] != 1 || a->ne[2] != 1 || a->ne[3] != 1 ||
        b->nb[0] != 4 || !is_internal(c, n)) return 0;
    const int j = next_real(g, i); if (j < 0) return 0;
    struct ggml_tensor * nx = g->nodes[j];
    if (nx->op != GGML_OP_ADD || (nx->src[0] != n && nx->src[1] != n) || nx->type != GGML_TYPE_F32 || !ggml_is_contiguous(nx) || !ggml_are_same_shape(nx, n)) return 0;
    const struct ggml_tensor * other = nx->src[0] == n ? nx->src[1] : nx->src[0];
    // the addend: the residual stream (same shape), or a bias row (gpt-oss's bo, src/llama-graph.cpp:1479-1481) — then a row stride of 0
    const bool bias_row = other->ne[0] == n->ne[0] && ggml_nelements(other) == n->ne[0] && n->ne[1] > 1;
    if (other == n || other->type != GGML_TYPE_F32 || (!ggml_are_same_shape(other, n) && !bias_row) || other->nb[0] != 4) return 0;
    // the sum is the residual stream; if RMS_NORM -> MUL(w) reads it next (ffn_norm, the next layer's attn_norm: build_norm, src/llama-graph.cpp:597-630)
    // and the mat-mul splits k, ONE pass adds the planes and the residual, writes the sum and normalises it
    static const bool norm_on = env_on("GGML_MI355X_PREFILL_COMBINE_NORM");
    struct ggml_tensor * nrm = nullptr; struct ggml_tensor * mul = nullptr; const struct ggml_tensor * w = nullptr;
    const int jn = next_real(g, j);
    if (norm_on && !bias_row && jn > 0 && jn + 1 < g->n_nodes && g->nodes[jn]->op == GGML_OP_RMS_NORM && g->nodes[jn]->src[0] == nx && g->nodes[jn + 1]->op == GGML_OP_MUL) {
        nrm = g->nodes[jn]; mul = g->nodes[jn + 1];
        w = mul->src[0] == nrm ? mul->src[1] : (mul->src[1] == nrm ? mul->src[0] : nullptr);
        const int64_t M = n->ne[0];
        const bool ok = w && is_internal(c, nrm) && w->type == GGML_TYPE_F32 && ggml_nelements(w) == M && w->ne[0] == M && w->nb[0] == 4 && ((uintptr_t) w->data % 16) == 0 &&
                        mul->type == GGML_TYPE_F32 && ggml_are_same_shape(mul, nx) && mul->nb[0] == 4 && mul->nb[1] % 16 == 0 && ((uintptr_t) mul->data % 16) == 0 &&
                        M % 4 == 0 && other->nb[1] % 16 == 0 && ((uintptr_t) other->data % 16) == 0 && nx->nb[1] % 16 == 0 && ((uintptr_t) nx->data % 16) == 0 &&
                        nrm->ne[2] == 1 && nrm->ne[3] == 1;
        if (!ok) { nrm = nullptr; mul = nullptr; }
    }
    mmq_deferred df = {};
    op_mul_mat(c, n, nx, other, nrm ? &df : nullptr);
    if (!nrm || df.np == 0) return j - i + 1;          // no k split: the epilogue has added the residual; the norm runs as usual
    const int64_t M = n->ne[0], N = n->ne[1];
    // the mat-mul after the norm reads bf16: written here too (the planes sit above the activation copy's slot only if that slot is this launch's own x:
    // the copy goes to offset 0, which the finished mat-mul no longer needs — but the PLANES live right after its x region, so the new copy must not reach them)
    const int jm = next_real(g, jn + 1);
    const struct ggml_tensor * mm = jm > 0 ? g->nodes[jm] : nullptr;
    uint16_t * y16 = nullptr;
    if (mm && mm->op == GGML_OP_MUL_MAT && mm->src[1] == mul && ggml_is_quantized(mm->src[0]->type) && N > MMVQ_MAX_N && mul->ne[2] == 1 && mul->ne[3] == 1 &&
        c->pass.act_off() + mul_mat_q_x_bytes(M, N) <= df.planes_off) {
        y16 = (uint16_t *) c->scratch;
    }
    combine_rms_norm(df.planes, df.np, M, N, (const float *) other->data, other->nb[1], (float *) nx->data, nx->nb[1], (const float *) w->data,
                     (float *) mul->data, mul->nb[1], y16, op_f32(nrm, 0), c->stream);
    c->cnt.kernels_launched++;
    if (y16) c->pass.produced_bf16(i, jn + 1, mul->data, M, N, mul->nb[1], 0);
    else c->pass.drop_act();
    return jn + 1 - i + 1;
}

// RMS_NORM -> MUL(by weight), when the intermediate has no other reader (the pattern build_norm emits, src/llama-graph.cpp:597-630; pinned by
// tests/test-backend-ops.cpp:2856): the norm in the prologue of the grouped mat-vec launch that reads the product, in the router kernel, or as one
// kernel that also writes the product's quantized image / bf16 copy for the mat-mul that reads it next. 0: not fused (a pending combine is still pending).
static int try_fused_norm(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    struct ggml_tensor * node = g->nodes[i];
    const struct ggml_tensor * s0 = node->src[0];
    if (i + 1 >= g->n_nodes) return 0;
    struct ggml_tensor * mul = g->nodes[i + 1];
    if (mul->op != GGML_OP_MUL || (mul->src[0] != node && mul->src[1] != node) || mul->type != GGML_TYPE_F32 || (node->flags & GGML_TENSOR_FLAG_OUTPUT)) return 0;
    const struct ggml_tensor * w = mul->src[0] == node ? mul->src[1] : mul->src[0];
    bool only_reader = true;
    for (int j = i + 2; j < g->n_nodes && only_reader; j++) {
        for (int s = 0; s < GGML_MAX_SRC; s++) if (g->nodes[j]->src[s] == node) { only_reader = false; break; }
    }
    if (!(only_reader && w->type == GGML_TYPE_F32 && w->nb[0] == sizeof(float) && ggml_are_same_shape(node, mul) &&
          ggml_can_repeat(w, node) && mul->nb[0] == sizeof(float))) return 0;
    // ... and when a quantized mat-mul reads the result next, quantize it in the same kernel
    const int jn = next_real(g, i + 1);
    const struct ggml_tensor * mm = jn > 0 ? g->nodes[jn] : nullptr;
    // best case: every reader of the product is a mat-vec of ONE grouped launch -> the norm runs in its prologue
    if (mm && fusable_mmv(mm) && mm->src[1] == mul && node->ne[1] == 1 && w->ne[0] == node->ne[0] && ggml_nelements(w) == w->ne[0] &&
        is_row_vec_f32(s0) && !(mul->flags & GGML_TENSOR_FLAG_OUTPUT)) {
        const int l = try_fused_mmv(c, g, jn, i, node, w);
        if (l >= 0) return l - i + 1;
    }
    pp_flush(c);       // (no grouped launch took the pending planes)
    // MoE: the router's F32 mat-mul reads the product first (build_moe_ffn, src/llama-graph.cpp:838): the norm runs inside the
    // router kernel, which also writes the product for the expert mat-vecs that follow
    if (mm && mm->op == GGML_OP_MUL_MAT && mm->src[1] == mul && mm->src[0]->type == GGML_TYPE_F32 && node->ne[1] == 1 && w->ne[0] == node->ne[0] &&
        ggml_nelements(w) == w->ne[0] && is_row_vec_f32(s0) && is_row_vec_f32(mul) && s0->data != mul->data) {
        const int f = try_fused_moe_route(c, g, jn, node, w);
        if (f) return jn + f - i;
    }
    if (mm && (mm->op == GGML_OP_MUL_MAT) && mm->src[1] == mul && ggml_is_quantized(mm->src[0]->type) &&
        act_kind_for((int) mm->src[0]->type) > 0 && rms_norm_mul_quant_supported(node->ne[0]) && node->ne[1] <= 8 && node->ne[2] == 1 && node->ne[3] == 1 &&
        w->ne[0] == node->ne[0] && ggml_nelements(w) == w->ne[0] && s0->nb[0] == 4 &&
        ((uintptr_t) s0->data % 16) == 0 && (s0->nb[1] % 16) == 0 && ((uintptr_t) mul->data % 16) == 0 && (mul->nb[1] % 16) == 0 &&
        ((uintptr_t) w->data % 16) == 0) {
        const int kind = act_kind_for((int) mm->src[0]->type);
        const act_q8 q = act_q8_carve(c->scratch, kind, node->ne[0], node->ne[1]);
        rms_norm_mul_quant((const float *) s0->data, s0->nb[1], (const float *) w->data, (float *) mul->data, mul->nb[1], q,
                           node->ne[0], node->ne[1], op_f32(node, 0), c->stream);
        c->pass.produced_q8(i, i + 1, mul->data, node->ne[0], node->ne[1], mul->nb[1], kind, q);
        c->cnt.kernels_launched++; c->cnt.act_quant_launches++;
        return 2;
    }
    // prefill: a quantized mat-mul on many tokens reads the product next — its bf16 copy comes out of this kernel too
    uint16_t * y16 = nullptr;
    if (mm && mm->op == GGML_OP_MUL_MAT && mm->src[1] == mul && ggml_is_quantized(mm->src[0]->type) && mul->ne[1] > MMVQ_MAX_N &&
        mul->ne[2] == 1 && mul->ne[3] == 1 && rms_norm_mul_bf16_supported(desc(s0), desc(w), desc(mul)) &&
        mul_mat_q_scratch_bytes(mul->ne[0], mul->ne[1], 0) <= c->scratch_size) {
        y16 = (uint16_t *) c->scratch;
    }
    rms_norm_mul(desc(s0), desc(w), nullptr, desc(mul), op_f32(node, 0), c->stream, y16);
    if (y16) c->pass.produced_bf16(i, i + 1, mul->data, mul->ne[0], mul->ne[1], mul->nb[1], 0);
    c->cnt.kernels_launched++;
    return 2;
}

int compute_node(mi_backend_ctx * c, struct ggml_cgraph * g, int i) {
    struct ggml_tensor * node = g->nodes[i];
    if (ggml_is_empty(node) || is_view_op(node->op)) return 1;
    const struct ggml_tensor * s0 = node->src[0];
    const struct ggml_tensor * s1 = node->src[1];

    // a MoE combine is pending: only the norm that reads its sum may go on without it (its grouped launch evaluates it) — and if no fusion takes
    // that norm, the combine runs in front of it after all
    if (c->pass.pp.active && !(node->op == GGML_OP_RMS_NORM && s0 && s0->data == (void *) c->pass.pp.x_out && c->use_fusion)) pp_flush(c);
    int consumed = 0;
    if (c->use_fusion) {
        if (node->op == GGML_OP_MUL_MAT && !tensor_is_split(s0)) {
            const int l = try_fused_mmv(c, g, i, i, nullptr, nullptr); consumed = l >= 0 ? l - i + 1 : 0;
            if (!consumed) consumed = try_fused_attn(c, g, i);       // (one token: recorded; many tokens: flushes, then launches)
            if (!consumed) consumed = try_fused_moe_route(c, g, i);
            if (!consumed) consumed = try_fused_prefill_glu(c, g, i);
            if (!consumed) consumed = try_fused_prefill_qkv(c, g, i);
            if (!consumed) consumed = try_fused_prefill_add(c, g, i);
        } else if (node->op == GGML_OP_SET_ROWS) consumed = try_fused_kv_store(c, g, i);
        else if (node->op == GGML_OP_GET_ROWS) consumed = try_fused_moe_combine(c, g, i);
        else if (node->op == GGML_OP_MUL_MAT_ID) { consumed = try_fused_moe_experts(c, g, i); if (!consumed) consumed = try_fused_prefill_moe(c, g, i); }
        else if (node->op == GGML_OP_ADD && s0 && s0->view_src) consumed = try_fused_slot_sum(c, g, i);
        else if (node->op == GGML_OP_RMS_NORM) { consumed = try_fused_norm(c, g, i); if (!consumed) pp_flush(c); }
        else if (node->op == GGML_OP_CPY && node->type == GGML_TYPE_F32 && (s0->type == GGML_TYPE_Q8_0 || s0->type == GGML_TYPE_Q4_0)) consumed = try_fused_kv_shift(c, g, i);
    }
    if (!consumed) {
        consumed = 1;
        switch (node->op) {
            case GGML_OP_MUL_MAT:    if (tensor_is_split(s0)) op_mul_mat_split(c, node); else op_mul_mat(c, node); break;
            case GGML_OP_MUL_MAT_ID: op_mul_mat_id(c, node); break;
            case GGML_OP_FLASH_ATTN_EXT: op_flash_attn_ext(c, node); break;
            case GGML_OP_RMS_NORM: rms_norm(desc(s0), desc(node), op_f32(node, 0), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_ADD: bin_bcast(BIN_ADD, desc(s0), desc(s1), desc(node), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_MUL: bin_bcast(BIN_MUL, desc(s0), desc(s1), desc(node), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_DIV: bin_bcast(BIN_DIV, desc(s0), desc(s1), desc(node), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_SUB: bin_bcast(BIN_SUB, desc(s0), desc(s1), desc(node), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_ADD_ID: add_id(desc(s0), desc(s1), desc(node->src[2]), desc(node), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_SCALE: scale(desc(s0), desc(node), op_f32(node, 0), op_f32(node, 1), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_CPY:  cpy(desc(s0), desc(s1), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_CONT: case GGML_OP_DUP: cpy(desc(s0), desc(node), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_SET_ROWS: set_rows(desc(s0), desc(s1), desc(node), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_GET_ROWS: get_rows(desc(s0), desc(s1), desc(node), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_SUM_ROWS: sum_rows(desc(s0), desc(node), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_ARGSORT: argsort(desc(s0), desc(node), node->op_params[0], c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_UNARY: unary((int) ggml_get_unary_op(node), desc(s0), desc(node), c->stream); c->cnt.kernels_launched++; break;
            case GGML_OP_GLU: {
                tensor_desc b;
                if (s1) b = desc(s1);
                glu((int) ggml_get_glu_op(node), node->op_params[1] != 0, desc(s0), s1 ? &b : nullptr, desc(node), op_f32(node, 2), op_f32(node, 3), c->stream);
                c->cnt.kernels_launched++;
            } break;
            case GGML_OP_ROPE:
                rope(desc(s0), (const int32_t *) s1->data, node->src[2] ? (const float *) node->src[2]->data : nullptr, desc(node), rope_params_of(node), c->stream);
                c->cnt.kernels_launched++;
                break;
            case GGML_OP_SOFT_MAX: {
                tensor_desc m;
                if (s1) m = desc(s1);
                soft_max(desc(s0), s1 ? &m : nullptr, node->src[2] ? (const float *) node->src[2]->data : nullptr, desc(node),
                         op_f32(node, 0), op_f32(node, 1), c->stream);
                c->cnt.kernels_launched++;
            } break;
            default:
                GGML_ABORT("MI355X backend: graph_compute met unsupported op %s (supports_op should have refused it)", ggml_op_name(node->op));
        }
    }
    c->pass.note_writes(g, i, consumed);
    c->cnt.nodes_computed += consumed;
    return consumed;
}
