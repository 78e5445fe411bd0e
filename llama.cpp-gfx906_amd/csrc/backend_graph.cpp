// backend_graph.cpp — running a whole graph: the scratch sizing pre-pass, the hipGraph cache keyed on node signatures, segmented capture and
// replay, and graph_compute (the backend vtable's entry, backend.cpp). One node at a time is compute_node's business (backend_nodes.cpp).
#include "backend_impl.h"

#include <chrono>

static constexpr int MI_MAX_GRAPHS = 24;

// scratch needed by the largest quantized mat-mul in the graph
static size_t graph_scratch_need(const struct ggml_cgraph * g) {
    size_t need = 0;
    for (int i = 0; i < g->n_nodes; i++) {
        const struct ggml_tensor * n = g->nodes[i];
        if ((n->op == GGML_OP_MUL_MAT || n->op == GGML_OP_MUL_MAT_ID) && ggml_is_quantized(n->src[0]->type)) {
            const int kind = act_kind_for((int) n->src[0]->type);
            if (kind < 0) continue;
            const struct ggml_tensor * b = n->src[1];
            const int64_t rows = n->op == GGML_OP_MUL_MAT ? b->ne[1] : b->ne[1]*b->ne[2];
            size_t s = act_q8_bytes(kind, b->ne[0], n->op == GGML_OP_MUL_MAT && rows <= MMVQ_MAX_N ? rows*b->ne[2] : rows);    // (few columns: all batches quantized at once)
            if (n->op == GGML_OP_MUL_MAT && rows > MMVQ_MAX_N) s = mul_mat_q_scratch_bytes(b->ne[0], rows, n->src[0]->ne[1]) + mul_mat_q_x_bytes(b->ne[0], rows);   // + room for a producer's copy above its own
            if (n->op == GGML_OP_MUL_MAT_ID) {
                const struct ggml_tensor * ids = n->src[2];
                size_t sg = mul_mat_q_id_scratch_bytes(b->ne[0], b->ne[1], ids->ne[1], ids->ne[0], n->src[0]->ne[2]);
                if (sg > s) s = sg;
                if (b->ne[1] == 1 && ids->ne[0]*ids->ne[1] > 4*MMVQ_MAX_N) {      // the fused expert chain of a prompt pass keeps the GLU result (rows of this tensor's m) beside the input copy
                    sg = mul_mat_q_id_plan(nullptr, b->ne[0], ids->ne[1], ids->ne[0], n->src[0]->ne[2], n->src[0]->ne[1]).bytes;
                    if (sg > s) s = sg;
                }
            }
            if (s > need) need = s;
        } else if (n->op == GGML_OP_MUL_MAT && !ggml_is_quantized(n->src[0]->type)) {
            // the matrix-core attention products: the f16 copy of src1, where and as large as mul_mat_dense_path asks for it — so that path is taken
            // from a backend's first graph on, whatever ran before, and nothing is requested for a product another kernel runs
            const mm_dense_args p = mm_dense_args_of(n);
            const size_t s = mul_mat_dense_mfma_supported(p) ? mul_mat_dense_mfma_scratch_bytes(p) : 0;
            if (s > need) need = s;
        }
    }
    return need;
}

// ---- the hipGraph cache ----------------------------------------------------------------------------------------
// A decode graph is captured the second time its signature is seen and replayed afterwards. The capture is cut into SEGMENTS (a few launches, then a few
// layers, then the rest), each its own executable graph: a replay checks and launches segment 0 first, so the GPU starts on the token while the host is
// still checking and launching the rest — one 166-node hipGraphLaunch took 62 us of host time during which the GPU sat idle, on top of 21 us for the
// 1125-node signature (llama-bench synchronizes after every token, so that gap is paid per token).
// What makes launching a prefix safe: (1) a TOPOLOGY pass over the whole graph first (every node and its source tensors are the cached graph's: who reads
// what decides which intermediates a fused group may leave unwritten); (2) a segment is launched only once its nodes' full signatures (op, type, shape,
// strides, placement, op_params, the sources' placement and layout) match and every segment before it has been launched. If a later segment does not
// match (same topology, another parameter), the rest follows the prefix already launched (graph_compute_suffix).
static void end_capture_segment(mi_backend_ctx * c, graph_entry & e, int begin, int end) {
    hipGraph_t graph = nullptr;
    MI_CHECK_G(hipStreamEndCapture(c->stream, &graph));
    c->capturing = false;
    graph_seg sg = { begin, end, nullptr };
    size_t n_nodes = 0;
    if (graph && hipGraphGetNodes(graph, nullptr, &n_nodes) == hipSuccess && n_nodes > 0) {
        const hipError_t err = hipGraphInstantiate(&sg.exec, graph, nullptr, nullptr, 0);
        if (err != hipSuccess) { (void) hipGraphDestroy(graph); throw mi_graph_error{ err, __FILE__, __LINE__ }; }
    } else (void) hipGetLastError();
    if (graph) MI_CHECK_G(hipGraphDestroy(graph));
    e.segs.push_back(sg);
}

// runs nodes [start, n_nodes). cap != NULL: under stream capture into cap's segments (the caller has begun the first capture; the last one is ended here)
static void run_nodes(mi_backend_ctx * c, struct ggml_cgraph * g, int start = 0, graph_entry * cap = nullptr) {
    c->pass.begin(g, c->use_fusion);
    // segment sizes in kernel launches: the first is small (the GPU starts early), the second covers the time the host needs to launch the rest
    static const int seg_kernels[2] = { (int) env_int("GGML_MI355X_GRAPH_SEG0", 6), (int) env_int("GGML_MI355X_GRAPH_SEG1", 24) };
    int seg_begin = start; uint64_t k0 = c->cnt.kernels_launched;
    for (int i = start; i < g->n_nodes; ) {
        i += compute_node(c, g, i);
        if (cap && i < g->n_nodes && cap->segs.size() < 2 && seg_kernels[cap->segs.size()] > 0 && !c->pass.pp.active &&
            c->cnt.kernels_launched - k0 >= (uint64_t) seg_kernels[cap->segs.size()]) {
            end_capture_segment(c, *cap, seg_begin, i);
            c->pass.cut();
            MI_CHECK_G(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            c->capturing = true;
            seg_begin = i; k0 = c->cnt.kernels_launched;
        }
    }
    pass_end(c);
    if (cap) end_capture_segment(c, *cap, seg_begin, g->n_nodes);
}

// records the whole graph into e's segments (recording runs nothing)
static void capture_graph(mi_backend_ctx * c, struct ggml_cgraph * g, graph_entry & e) {
    c->cap_entry = &e;
    MI_CHECK_G(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    c->prof_suspend = false;
    c->capturing = true;
    run_nodes(c, g, 0, &e);
    c->cap_entry = nullptr;
    c->prof_suspend = c->prof_in_graph;
    c->cnt.graph_captures++;
}
static void launch_segments(mi_backend_ctx * c, const graph_entry & e, size_t from = 0) {
    for (size_t si = from; si < e.segs.size(); si++) if (e.segs[si].exec) MI_CHECK_G(hipGraphLaunch(e.segs[si].exec, c->stream));
}

// (round 3: 64-bit lanes — one multiply per 8 bytes instead of one per 4, two independent chains for the op parameters — and only the sources that
// exist are walked)
static inline uint64_t sig_mix(uint64_t h, uint64_t v) { h = (h ^ v)*0x9E3779B97F4A7C15ull; return h ^ (h >> 32); }
static inline uint32_t hash_params(const int32_t * p) {
    uint64_t w[GGML_MAX_OP_PARAMS/8];
    memcpy(w, p, sizeof(w));
    uint64_t h0 = 0x243F6A8885A308D3ull, h1 = 0x13198A2E03707344ull;
    for (int i = 0; i < (int)(GGML_MAX_OP_PARAMS/8); i += 2) { h0 = sig_mix(h0, w[i]); h1 = sig_mix(h1, w[i + 1]); }
    const uint64_t h = sig_mix(h0, h1);
    return (uint32_t)(h ^ (h >> 32));
}

static inline void fill_sig(node_sig & s, const struct ggml_tensor * n) {
    s.node = n; s.data = n->data; s.op = (int32_t) n->op; s.type = (int32_t) n->type;
    for (int d = 0; d < 4; d++) s.ne[d] = n->ne[d];
    for (int d = 0; d < 3; d++) s.nb[d] = n->nb[d + 1];
    for (int j = 0; j < GGML_MAX_SRC; j++) {
        const struct ggml_tensor * t = n->src[j];
        s.src[j] = t;
        if (!t) { s.src_data[j] = NULL; s.src_hash[j] = 0u; continue; }
        s.src_data[j] = t->data;
        uint64_t h0 = sig_mix(0x452821E638D01377ull, (uint64_t) t->type), h1 = 0xBE5466CF34E90C6Cull;
        for (int d = 0; d < 4; d++) { h0 = sig_mix(h0, (uint64_t) t->ne[d]); h1 = sig_mix(h1, (uint64_t) t->nb[d]); }
        const uint64_t h = sig_mix(h0, h1);
        const uint32_t h32 = (uint32_t)(h ^ (h >> 32));
        s.src_hash[j] = h32 ? h32 : 1u;
    }
    s.params_hash = hash_params(n->op_params);
    s.flags = (uint32_t) n->flags;
}

static void free_entry(graph_entry & e) {
    for (auto & sg : e.segs) if (sg.exec) (void) hipGraphExecDestroy(sg.exec);
    e.segs.clear();
}
void drop_graphs(mi_backend_ctx * c) {
    for (auto & e : c->graphs) free_entry(e);
    c->graphs.clear();
}

// ---- replay, fast path: the cached graph this submission most likely is (same first node, same length, most recently used) ----
static graph_entry * replay_candidate(mi_backend_ctx * c, const struct ggml_cgraph * g) {
    graph_entry * best = nullptr;
    for (auto & e : c->graphs) {
        if (e.segs.empty() || (int) e.sig.size() != g->n_nodes || e.sig[0].node != g->nodes[0]) continue;
        if (!best || e.last_use > best->last_use) best = &e;
    }
    return best;
}
static bool topology_matches(const graph_entry & e, const struct ggml_cgraph * g) {
    static_assert(sizeof(((struct ggml_tensor *) 0)->src) == sizeof(((node_sig *) 0)->src), "node_sig::src mirrors ggml_tensor::src");
    for (int i = 0; i < g->n_nodes; i++) {
        const struct ggml_tensor * n = g->nodes[i];
        if (n != e.sig[i].node || memcmp(n->src, e.sig[i].src, sizeof(n->src)) != 0) return false;
    }
    return true;
}
static bool signature_matches(const graph_entry & e, const struct ggml_cgraph * g, int begin, int end) {
    node_sig ns;
    for (int i = begin; i < end; i++) {
        fill_sig(ns, g->nodes[i]);
        if (memcmp(&ns, &e.sig[i], sizeof(ns)) != 0) return false;
    }
    return true;
}

// find (or create) the cache entry whose signature equals this graph's
static graph_entry & graph_lookup(mi_backend_ctx * c, const struct ggml_cgraph * g) {
    c->cur_sig.resize(g->n_nodes);
    uint64_t d0 = 0x9E3779B97F4A7C15ull, d1 = 0xC2B2AE3D27D4EB4Full;
    for (int i = 0; i < g->n_nodes; i++) {
        node_sig & ns = c->cur_sig[i];
        fill_sig(ns, g->nodes[i]);
        d0 = sig_mix(d0, (uint64_t)(uintptr_t) ns.data ^ ((uint64_t) ns.ne[1] << 20) ^ ((uint64_t) ns.ne[0] << 44) ^ ns.params_hash);
        d1 = sig_mix(d1, (uint64_t)(uintptr_t) ns.src_data[0] ^ ((uint64_t)(uintptr_t) ns.src_data[1] << 1) ^ ((uint64_t) ns.src_hash[0] << 32) ^ ns.src_hash[1] ^ ((uint64_t) ns.nb[0] << 13));
    }
    const uint64_t digest = sig_mix(d0, d1);
    c->cur_digest = digest;
    graph_entry * lru = nullptr;
    // most recently used first: consecutive decode steps re-submit the same graph (src/llama-context.cpp:728)
    graph_entry * best = nullptr;
    for (auto & e : c->graphs) {
        if (!lru || e.last_use < lru->last_use) lru = &e;
        if (e.digest == digest && (int) e.sig.size() == g->n_nodes && (!best || e.last_use > best->last_use) &&
            memcmp(e.sig.data(), c->cur_sig.data(), sizeof(node_sig)*g->n_nodes) == 0) best = &e;
    }
    if (best) { best->last_use = ++c->graph_tick; best->seen++; return *best; }
    if ((int) c->graphs.size() >= MI_MAX_GRAPHS) {
        if (!lru->segs.empty()) MI_CHECK_G(hipStreamSynchronize(c->stream));
        free_entry(*lru);
        *lru = graph_entry();
        lru->sig = c->cur_sig; lru->digest = c->cur_digest; lru->last_use = ++c->graph_tick; lru->seen = 1;
        return *lru;
    }
    c->graphs.emplace_back();
    graph_entry & e = c->graphs.back();
    e.sig = c->cur_sig; e.digest = c->cur_digest; e.last_use = ++c->graph_tick; e.seen = 1;
    return e;
}

// the buffers a graph needs: allocated outside any capture (a captured graph holds their addresses). Growing one synchronizes the stream first (work
// already queued, a replayed prefix included, may still read the old allocation) and drops every captured graph.
static enum ggml_status prepare_buffers(mi_backend_ctx * c, const struct ggml_cgraph * g) {
    if (!c->rope_tab) { if (hipMalloc((void **) &c->rope_tab, 4096) != hipSuccess) { (void) hipGetLastError(); c->rope_tab = nullptr; } }
    if (!c->moe_ws) {
        if (hipMalloc((void **) &c->moe_ws, 4096) == hipSuccess) { MI_CHECK_G(hipMemsetAsync(c->moe_ws, 0, 4096, c->stream)); MI_CHECK_G(hipStreamSynchronize(c->stream)); }
        else { (void) hipGetLastError(); c->moe_ws = nullptr; }
    }
    if (!c->err_host) {      // the error words of the kernels with bounded waits (host-mapped)
        if (hipHostMalloc((void **) &c->err_host, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer((void **) &c->err_dev, c->err_host, 0) == hipSuccess) memset(c->err_host, 0, 64);
        else { (void) hipGetLastError(); c->err_host = nullptr; c->err_dev = nullptr; }
    }
    if (!c->fin_img) {       // allocated once, outside any capture; the counters are zero between launches (the kernels re-arm them)
        if (hipMalloc(&c->fin_img, mi_backend_ctx::FIN_IMG_BYTES) != hipSuccess) { (void) hipGetLastError(); c->fin_img = nullptr; }
        if (c->fin_img && hipMalloc((void **) &c->fin_cnt, (mi_backend_ctx::FIN_COUNTERS + 8)*4) == hipSuccess) {
            MI_CHECK_G(hipMemsetAsync(c->fin_cnt, 0, (mi_backend_ctx::FIN_COUNTERS + 8)*4, c->stream)); MI_CHECK_G(hipStreamSynchronize(c->stream));
        } else if (c->fin_img) { (void) hipGetLastError(); (void) hipFree(c->fin_img); c->fin_img = nullptr; c->fin_cnt = nullptr; }
    }
    if (!c->attn_part) {     // allocated once, outside any capture
        const size_t pb = ATTN_PART_BYTES;
        if (hipMalloc((void **) &c->attn_part, pb) == hipSuccess) c->attn_part_bytes = pb; else (void) hipGetLastError();
    }
    const size_t need = graph_scratch_need(g);
    if (need > c->scratch_size) {
        MI_CHECK_G(hipStreamSynchronize(c->stream));
        if (c->scratch) MI_CHECK_G(hipFree(c->scratch));
        c->scratch = nullptr; c->scratch_size = 0;
        drop_graphs(c);   // captured graphs hold the old scratch pointer
        const size_t sz = need + (need >> 2);
        if (hipMalloc(&c->scratch, sz) != hipSuccess) { (void) hipGetLastError(); return GGML_STATUS_ALLOC_FAILED; }
        c->scratch_size = sz;
    }
    {
        size_t kv_need = 0;
        for (int i = 0; i < g->n_nodes; i++) if (g->nodes[i]->op == GGML_OP_FLASH_ATTN_EXT) { const fa_operands p = fa_kv16_plan(g->nodes[i], nullptr, nullptr, 0); kv_need = std::max(kv_need, p.k_bytes + p.v_bytes); }
        if (kv_need > c->kv16_size) {
            MI_CHECK_G(hipStreamSynchronize(c->stream));
            if (c->kv16) MI_CHECK_G(hipFree(c->kv16));
            c->kv16 = nullptr; c->kv16_size = 0;
            drop_graphs(c);   // captured graphs hold the old pointer
            const size_t sz = kv_need + (kv_need >> 1);      // (the cache view grows with the context: fewer re-allocations)
            if (hipMalloc(&c->kv16, sz) != hipSuccess) { (void) hipGetLastError(); return GGML_STATUS_ALLOC_FAILED; }
            c->kv16_size = sz;
        }
    }

    {
        size_t cv_need = 0;
        for (int i = 0; i < g->n_nodes; i++) {
            const struct ggml_tensor * nd = g->nodes[i];
            if (nd->op == GGML_OP_MUL_MAT && ggml_is_quantized(nd->src[0]->type) && nd->src[1]->type == GGML_TYPE_F16) cv_need = std::max(cv_need, (size_t) ggml_nelements(nd->src[1])*4 + 256);
        }
        if (cv_need > c->cvt_size) {
            MI_CHECK_G(hipStreamSynchronize(c->stream));
            if (c->cvt) MI_CHECK_G(hipFree(c->cvt));
            c->cvt = nullptr; c->cvt_size = 0;
            drop_graphs(c);
            if (hipMalloc(&c->cvt, cv_need) != hipSuccess) { (void) hipGetLastError(); return GGML_STATUS_ALLOC_FAILED; }
            c->cvt_size = cv_need;
        }
    }

    return GGML_STATUS_SUCCESS;
}

// ---- replay, partial match: a cached graph's segments before node `resume` are on the stream; this graph differs from it behind them ----
// (llama.cpp rebuilds a graph in the same memory when n_kv moves to the next bucket: same nodes, the attention's shapes changed). The rest still needs
// buffers sized for THIS graph, before any of its nodes runs (a larger K / V conversion, more scratch), and its signature counts like any other: on
// its second sighting the whole graph is captured — recording runs nothing — and only the segments behind the prefix are launched; from then on the
// fast path replays it in full. Growing a buffer behind the prefix loses nothing the suffix reads: what prepare_buffers may replace (scratch, kv16,
// cvt) holds nothing across a cut — the cached activations are dropped at every cut and the deferred combine never spans one — and what does cross a
// cut (the rotation table, the router's top values at moe_ws + 64, the producer images in fin_img, attn_part) lives in buffers allocated once and never
// replaced; the prefix launched is the one this graph's own capture would hold, so it leaves the same values there.
static enum ggml_status graph_compute_suffix(mi_backend_ctx * c, struct ggml_cgraph * g, int resume) {
    const enum ggml_status st = prepare_buffers(c, g);
    if (st != GGML_STATUS_SUCCESS) return st;
    graph_entry & e = graph_lookup(c, g);
    if (e.segs.empty() && e.seen >= 2) capture_graph(c, g, e);
    size_t si = 0;
    while (si < e.segs.size() && e.segs[si].begin < resume) si++;
    if (si < e.segs.size() && e.segs[si].begin == resume) {
        launch_segments(c, e, si);
        return GGML_STATUS_SUCCESS;
    }
    c->prof_suspend = false;
    run_nodes(c, g, resume);
    return GGML_STATUS_SUCCESS;
}

static enum ggml_status be_graph_compute_impl(ggml_backend_t backend, struct ggml_cgraph * g);
static double g_host_ns = 0.0; static long g_host_calls = 0;     // GGML_MI355X_HOST_TIMING=1: host time spent inside graph_compute
static bool host_timing() { static const bool on = env_is_set("GGML_MI355X_HOST_TIMING"); return on; }
enum ggml_status be_graph_compute(ggml_backend_t backend, struct ggml_cgraph * g) {
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    (void) hipGetLastError();      // a stale thread-level error (another library's probe, a failed allocation elsewhere) is not this graph's: only what this call raises counts
    try {
        const bool timing = host_timing();
        const auto t0 = std::chrono::steady_clock::now();
        const enum ggml_status st = be_graph_compute_impl(backend, g);
        if (timing) {
            g_host_ns += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
            if (++g_host_calls % 256 == 0) fprintf(stderr, "ggml-mi355x: graph_compute host time %.1f us per call over %ld calls\n", g_host_ns/g_host_calls/1e3, g_host_calls);
        }
        // a kernel launch that failed (bad configuration, out of resources) shows up as the runtime's last error
        const hipError_t le = hipGetLastError();
        if (st == GGML_STATUS_SUCCESS && le != hipSuccess) { MI_LOG("graph_compute: %s (%s)\n", hipGetErrorName(le), hipGetErrorString(le)); return GGML_STATUS_FAILED; }
        return st;
    } catch (const mi_graph_error & e) {
        MI_LOG("graph_compute failed: HIP error %s (%s) at %s:%d\n", hipGetErrorName(e.err), hipGetErrorString(e.err), e.file, e.line);
        if (c->capturing) {       // leave the stream usable: end the capture, drop what was recorded
            hipGraph_t graph = nullptr;
            (void) hipStreamEndCapture(c->stream, &graph);
            if (graph) (void) hipGraphDestroy(graph);
            c->capturing = false;
        }
        if (c->cap_entry) { free_entry(*c->cap_entry); c->cap_entry = nullptr; }      // a partly captured graph is not replayable
        c->pass.abandon(); c->up.n = 0;
        // a throw inside the row-split fork leaves the current device on a peer, and peer streams that were already launched may still write dst:
        // back to this backend's device, and nothing is returned before they have finished
        set_device(c->device);
        for (int i = 0; i < G().n_devices; i++) if (c->peers[i].stream) { set_device(G().devices[i].id); (void) hipStreamSynchronize(c->peers[i].stream); }
        set_device(c->device);
        (void) hipStreamSynchronize(c->stream);
        (void) hipGetLastError();
        return GGML_STATUS_FAILED;
    }
}
static enum ggml_status be_graph_compute_impl(ggml_backend_t backend, struct ggml_cgraph * g) {
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    c->cnt.graphs_computed++;
    uploads_flush(c);       // the inputs the host has set (set_tensor_async) go out first, as one launch

    const bool timing2 = host_timing();
    static double t_first = 0, t_rest = 0; static long n_rep = 0;
    const bool try_graph = c->use_graphs && (!c->profiling || c->prof_in_graph) && g->n_nodes >= 8;

    // ---- fast path: replay segment by segment ----
    if (try_graph) {
        const auto ta = std::chrono::steady_clock::now();
        graph_entry * e = replay_candidate(c, g);
        if (e && topology_matches(*e, g)) {
            size_t si = 0; auto tb = ta;
            for (; si < e->segs.size(); si++) {
                const graph_seg & sg = e->segs[si];
                if (!signature_matches(*e, g, sg.begin, sg.end)) break;
                if (sg.exec) MI_CHECK_G(hipGraphLaunch(sg.exec, c->stream));
                if (si == 0 && timing2) tb = std::chrono::steady_clock::now();
            }
            if (si == e->segs.size()) {
                e->last_use = ++c->graph_tick; e->seen++;
                c->cnt.graph_replays++;
                if (timing2) {
                    const auto tc = std::chrono::steady_clock::now();
                    t_first += std::chrono::duration<double, std::micro>(tb - ta).count(); t_rest += std::chrono::duration<double, std::micro>(tc - tb).count();
                    if (++n_rep % 128 == 0) fprintf(stderr, "ggml-mi355x: replay host us: until segment 0 is launched %.1f, the other %zu segments %.1f (n_nodes %d, %zu cached)\n", t_first/n_rep, e->segs.size() - 1, t_rest/n_rep, g->n_nodes, c->graphs.size());
                }
                return GGML_STATUS_SUCCESS;
            }
            if (si > 0) {      // same topology, a parameter changed behind an identical prefix: the prefix is on the stream, the rest follows it
                c->cnt.graph_partial_replays++;
                return graph_compute_suffix(c, g, e->segs[si].begin);
            }
        }
    }

    {
        const enum ggml_status st = prepare_buffers(c, g);
        if (st != GGML_STATUS_SUCCESS) return st;
    }

    c->split_graph = false;
    for (int i = 0; i < g->n_nodes && !c->split_graph; i++) c->split_graph = g->nodes[i]->op == GGML_OP_MUL_MAT && tensor_is_split(g->nodes[i]->src[0]);
    if (c->split_graph) {     // several devices' streams take part: eager execution, no capture (the fusion matchers leave split weights to op_mul_mat_split)
        run_nodes(c, g);
        return GGML_STATUS_SUCCESS;
    }
    c->prof_suspend = try_graph && c->prof_in_graph;     // only what is captured gets recorded in that mode
    if (try_graph) {
        graph_entry & e = graph_lookup(c, g);
        if (!e.segs.empty()) {      // (a cached graph the fast path did not pick: e.g. several sequences' graphs taking turns)
            launch_segments(c, e);
            c->cnt.graph_replays++;
            return GGML_STATUS_SUCCESS;
        }
        if (e.seen >= 2) {
            capture_graph(c, g, e);
            launch_segments(c, e);
            return GGML_STATUS_SUCCESS;
        }
    }
    run_nodes(c, g);
    return GGML_STATUS_SUCCESS;
}
