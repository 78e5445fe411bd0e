// backend_impl.h — internal to the backend*.cpp translation units (the only ones that see ggml struct layouts): error macros, the backend
// context, the per-pass state, the graph cache entry, small shared helpers and the few functions that cross files.
//   backend.cpp        registry, device, buffer types, the backend vtable, uploads, copies, events, supports_op, options, profile, C exports
//   backend_nodes.cpp  the pass state's operations, op launchers, fusion matchers, compute_node
//   backend_graph.cpp  node signatures, the hipGraph cache, segmented capture and replay, prepare_buffers, graph_compute
#pragma once

#include "ggml-mi355x.h"
#include "ggml-backend-impl.h"
#include "ggml-impl.h"

#include "kernels.h"

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

using namespace mi355x;

#define MI_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    GGML_ABORT("MI355X backend: HIP error %s (%s) at %s:%d", hipGetErrorName(e_), hipGetErrorString(e_), __FILE__, __LINE__); } } while (0)

#define MI_LOG(...) do { fprintf(stderr, "ggml-mi355x: " __VA_ARGS__); } while (0)

// On the graph path (be_graph_compute and what it calls) a HIP error is not fatal: it unwinds to be_graph_compute, which ends a capture in
// progress and returns GGML_STATUS_FAILED — llama_context::decode maps that and rolls the KV cells of the batch back
// (src/llama-context.cpp:1078-1107). Everywhere else (buffer and device entry points, which have no status to return) MI_CHECK aborts.
struct mi_graph_error { hipError_t err; const char * file; int line; };
#define MI_CHECK_G(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw mi_graph_error{ e_, __FILE__, __LINE__ }; } while (0)
#define MI_REQUIRE_G(cond) do { if (!(cond)) throw mi_graph_error{ hipErrorInvalidValue, __FILE__, __LINE__ }; } while (0)

// ---- device table ----
struct mi_device {
    int id;
    std::string name;         // "MI355X0"
    std::string description;
    size_t total_mem;
    struct ggml_backend_device dev;
    struct ggml_backend_buffer_type buft;
};

struct mi_globals {
    int n_devices = 0;
    mi_device devices[GGML_MI355X_MAX_DEVICES];
    struct ggml_backend_reg reg;
    struct ggml_backend_buffer_type host_buft;
    bool initialised = false;
};

mi_globals & G();

static inline void set_device(int id) { MI_CHECK(hipSetDevice(id)); }

struct mi_split_tensor {                                   // tensor->extra of a tensor in a split buffer
    void *  data[GGML_MI355X_MAX_DEVICES] = {};            // the slice in device i's memory (NULL: no rows there)
    int64_t row_lo[GGML_MI355X_MAX_DEVICES + 1] = {};      // device i holds rows [row_lo[i], row_lo[i+1])
};

// ---- the hipGraph cache entry ----
// What must be unchanged for a captured hipGraph to be replayed, per node (the checks the reference's GPU
// backends make before reusing a captured graph): the node itself, its op/type/shape/strides/data pointer,
// a hash of op_params, and the data pointers + leading shape of its sources (leaf tensors are not nodes and
// split graphs carry no leaf list, so their placement is pinned through the nodes that read them).
struct node_sig {
    const void * node; const void * data;
    const void * src[GGML_MAX_SRC];                                            // the source TENSORS: the graph's topology (checked for the whole graph before any segment is launched)
    int32_t op, type;
    int64_t ne[4]; size_t nb[3];
    const void * src_data[GGML_MAX_SRC]; uint32_t src_hash[GGML_MAX_SRC];      // every source: placement + a hash of its type, shape and strides
    uint32_t params_hash; uint32_t flags;
};

static_assert(sizeof(node_sig) == 16 + 8*GGML_MAX_SRC + 8 + 32 + 24 + 8*GGML_MAX_SRC + 4*GGML_MAX_SRC + 8, "node_sig has no padding bytes: signatures are compared with memcmp");
struct graph_seg { int begin, end; hipGraphExec_t exec; };      // nodes [begin, end) as one executable graph (exec == NULL: view ops only, nothing to launch)
struct graph_entry {
    std::vector<node_sig> sig; uint64_t digest = 0;      // digest: a cheap hash of the signature — only the entry that shares it is compared in full
    std::vector<graph_seg> segs;                          // empty: not captured (yet)
    uint64_t last_use = 0;
    int seen = 0;              // identical submissions observed (capture on the 2nd)
};

// ---- per-pass state ----
// What one node of a pass over a graph (run_nodes, eager or under capture) leaves for a later node of the same pass. The buffers it points into
// (scratch, moe_ws, rope_tab) belong to mi_backend_ctx; this only says what they hold. Every reset or invalidation goes through the operations below.
struct mi_pass {
    std::unordered_map<const struct ggml_tensor *, int> uses;   // consumers per tensor in the graph being run (fusion legality)
    // the activations of a quantized mat-mul as the scratch holds them (quantized, or the bf16 copy the MFMA prefill kernel reads); off: where in the
    // scratch the bf16 copy sits (a producer kernel that still reads offset 0 writes its result's copy higher up). Nodes lo..hi are the launch that
    // produced it (empty when a node quantized its own input): their writes over `data` do not end it, anybody else's do.
    // Rows r of the input: data + (r % n_inner)*s_inner + (r / n_inner)*s_outer. Written and looked up through the operations below only.
    struct { const void * data; int64_t k, n_inner, n_outer; size_t s_inner, s_outer; int kind; act_q8 q; bool valid; size_t span;
             size_t off; int lo = 0, hi = -1; } aq = {};
    static constexpr int ACT_KIND_BF16 = -16;          // aq.kind of the dense bf16 copy the MFMA prefill kernel reads
    static constexpr size_t NO_ACT = ~(size_t) 0;
    // the last router launch: it ranked `vals` (probabilities, or logits) into `sorted` and left the eight best values in rank order at moe_ws + 64
    // (floats the kernel does not use otherwise): a combine that gathers vals[sorted[u]] takes them from there — one load instead of two dependent cold ones.
    // Keyed on addresses, so any later node that writes over vals or sorted (an allocator reuses a dead router's memory for the next layer's, whose router
    // may run unfused) ends it; nodes lo..hi are the router launch's own.
    struct { bool valid = false; const void * vals = nullptr; const void * sorted = nullptr; size_t bytes = 0; int lo = 0, hi = -1; } rt;
    // a MoE combine left pending (try_fused_moe_combine): the vector x_out = res + sum_u w_u * plane u does not exist until the launch that reads it (the next
    // norm + mat-vec launch, streamed kernel) has evaluated it in its prologue, or pp_flush has
    struct { bool active = false; const float * res = nullptr; float * x_out = nullptr; int n_planes = 0; int64_t m = 0;
             const float * planes = nullptr; int stride = 0;                                     // where the planes are (floats between them)
             const float * probs = nullptr; size_t probs_bytes = 0; const int32_t * ids = nullptr; int mode = 0; } pp;      // planes = the used experts' outputs, weights from probs[ids[u]]
    // rope_tab holds the rotation table for these parameters ((cos, sin) per pair index; mmvq_rope::table): filled by one small launch when a pass's
    // first rotated mat-vec launch comes up (and again if a launch asks for other rope parameters), read by every such launch after it
    mmvq_rope rope_key = {}; bool rope_valid = false;

    void begin(const struct ggml_cgraph * g, bool count_uses);         // a pass starts: nothing is carried over from the last one
    // a capture segment ends. aq does not cross a cut: the scratch it describes may be replaced (prepare_buffers) before a partial replay runs the
    // rest of a graph behind a launched prefix. rt and the rope table do: they describe moe_ws and rope_tab, allocated once and never replaced, and
    // the prefix launched in front of a cut is the one this graph's own capture holds, so it has left the same values there.
    void cut() { aq.valid = false; }
    void abandon() { aq.valid = false; pp.active = false; }            // a pass unwound by an error
    void drop_act() { aq.valid = false; }                              // a launch reuses the scratch
    void note_writes(const struct ggml_cgraph * g, int i, int n);      // nodes [i, i+n) have run: what they wrote over ends aq / rt

    // look-ups: does the scratch hold the image of exactly this input? Each asks for what its caller relies on, no more.
    // the bf16 copy of n rows of k floats, row_stride bytes apart: its offset in the scratch, or NO_ACT (a caller that needs it at the start asks `== 0`)
    size_t bf16_at(const void * x, int64_t k, int64_t n, size_t row_stride) const {
        return aq.valid && aq.kind == ACT_KIND_BF16 && aq.data == x && aq.k == k && aq.n_inner == n && aq.s_inner == row_stride ? aq.off : NO_ACT;
    }
    // the quantized image of these rows in this format, or NULL
    const act_q8 * q8_of(const void * x, int64_t k, int64_t n_inner, int64_t n_outer, size_t s_inner, size_t s_outer, int kind) const {
        return aq.valid && aq.data == x && aq.k == k && aq.n_inner == n_inner && aq.n_outer == n_outer && aq.s_inner == s_inner && aq.s_outer == s_outer &&
               aq.kind == kind ? &aq.q : nullptr;
    }
    // ... of one row (no stride to compare)
    const act_q8 * q8_of_row(const void * x, int64_t k, int kind) const {
        return aq.valid && aq.data == x && aq.k == k && aq.n_inner == 1 && aq.n_outer == 1 && aq.kind == kind ? &aq.q : nullptr;
    }
    bool holds_image_of(const void * x) const { return aq.valid && aq.data == x; }      // any image, any format
    size_t act_off() const { return aq.valid ? aq.off : 0; }                             // where the live image starts (0 when there is none)

    // writes. converted_*: a node made the image of its own input (at the start of the scratch); produced_*: the launch that covers nodes lo..hi
    // left the image of its result (bf16: at offset off)
    void converted_q8(const void * x, int64_t k, int64_t n_inner, int64_t n_outer, size_t s_inner, size_t s_outer, int kind, const act_q8 & q) {
        aq = { x, k, n_inner, n_outer, s_inner, s_outer, kind, q, true, (size_t)(n_outer - 1)*s_outer + (size_t)(n_inner - 1)*s_inner + (size_t) k*4, 0, 0, -1 };
    }
    void produced_q8(int lo, int hi, const void * x, int64_t k, int64_t n, size_t row_stride, int kind, const act_q8 & q) {
        converted_q8(x, k, n, 1, row_stride, 0, kind, q); aq.lo = lo; aq.hi = hi;
    }
    void converted_bf16(const void * x, int64_t k, int64_t n, size_t row_stride) { converted_q8(x, k, n, 1, row_stride, 0, ACT_KIND_BF16, act_q8{}); }
    void produced_bf16(int lo, int hi, const void * x, int64_t k, int64_t n, size_t row_stride, size_t off) {
        converted_bf16(x, k, n, row_stride); aq.off = off; aq.lo = lo; aq.hi = hi;
    }
};

struct mi_backend_ctx {
    int device;                    // HIP device id
    int dev_index = 0;             // index into G().devices
    std::string name;
    hipStream_t stream = nullptr;

    void * scratch = nullptr;      // quantized activations
    size_t scratch_size = 0;
    int moe_dual = -1;                  // option "moe_dual"
    float * moe_ws = nullptr;                                   // logits + arrival counter of the multi-workgroup router kernel (moe_route); the router hand-off at + 64
    // producer-side activation quantization (mmvq_fin): the image a GLU launch writes for the mat-vec that follows + its arrival counters
    void * fin_img = nullptr; unsigned * fin_cnt = nullptr;
    float * rope_tab = nullptr;                                 // the rotation table of the token being decoded (mi_pass::rope_valid)
    static constexpr size_t FIN_IMG_BYTES = 64*1024; static constexpr int FIN_COUNTERS = 256;
    void * cvt = nullptr; size_t cvt_size = 0;                  // the F32 copy of an F16 src1 of a quantized MUL_MAT
    void * kv16 = nullptr; size_t kv16_size = 0;                // FLASH_ATTN_EXT: dense f16 copies of a quantized / bf16 cache view, and the transposed V of the prefill kernel (kv_to_f16)
    float * attn_part = nullptr; size_t attn_part_bytes = 0;   // partial results of the decode attention's cell ranges at long contexts (attn_decode)

    mi_pass pass;

    // hipGraph cache (one entry: llama.cpp re-submits the same decode graph, src/llama-context.cpp:728)
    bool use_graphs = true;
    bool use_fusion = true;
    std::vector<graph_entry> graphs;     // small LRU: decode graphs differ only in n_kv (one per 32 tokens of context)
    std::vector<node_sig> cur_sig; uint64_t cur_digest = 0;
    uint64_t graph_tick = 0;

    struct ggml_backend_mi355x_counters cnt = {};

    bool capturing = false;
    graph_entry * cap_entry = nullptr;               // the cache entry a capture in progress fills (dropped if the capture fails)
    // small uploads (set_tensor_async of <= UP_SMALL_MAX bytes: a decode step's inputs) are staged in a pinned, device-mapped ring and go out as ONE
    // launch in front of whatever the stream is asked to do next (uploads_flush), instead of one copy each
    struct { char * host = nullptr; char * dev = nullptr; int cur = 0; size_t off = 0; hipEvent_t ev[2] = { nullptr, nullptr }; bool ev_pending[2] = { false, false };
             int n = 0; upload_batch b = {}; bool failed = false; } up;
    static constexpr size_t UP_HALF = 1u << 20, UP_SMALL_MAX = 64u << 10;
    unsigned * err_host = nullptr;                   // host-mapped words: a bounded wait inside a kernel gave up ([1] the MoE router)
    unsigned * err_dev = nullptr;                    // ... their device address

    // "profile" option: every quantized mat-mul launch is bracketed by a hipEvent pair on this stream (eager mode)
    struct prof_rec { int type; int64_t m, k, n; uint64_t bytes; hipEvent_t e0, e1; const char * kernel = nullptr; };
    bool profiling = false;
    bool prof_in_graph = false;      // option "profile" = 2: the event pairs are captured into the hipGraphs as event-record nodes
    bool prof_suspend = false;       //   ... and eager passes (before a graph's capture) are not recorded
    std::vector<prof_rec> prof;
    std::vector<hipEvent_t> ev_pool;

    // row-split mat-muls: a stream, a completion event and (for the many-token kernel) a scratch area per peer device, made on first use
    struct split_peer { hipStream_t stream = nullptr; hipEvent_t done = nullptr; void * scratch = nullptr; size_t scratch_size = 0; };
    split_peer peers[GGML_MI355X_MAX_DEVICES];
    hipEvent_t split_ready = nullptr;
    hipEvent_t cpy_ev = nullptr;     // cpy_tensor_async to another backend: the destination stream waits on it
    bool split_graph = false;        // the graph being run reads row-split weights: eager execution (several devices' streams take part)
};

// ---- small shared helpers ----
static inline bool is_view_op(enum ggml_op op) {
    return op == GGML_OP_NONE || op == GGML_OP_RESHAPE || op == GGML_OP_VIEW || op == GGML_OP_PERMUTE || op == GGML_OP_TRANSPOSE;
}
static inline float op_f32(const struct ggml_tensor * t, int i) { float f; memcpy(&f, &t->op_params[i], 4); return f; }
static inline tensor_desc desc(const struct ggml_tensor * t) {
    tensor_desc d;
    d.data = t->data; d.type = (int) t->type;
    for (int i = 0; i < 4; i++) { d.ne[i] = t->ne[i]; d.nb[i] = t->nb[i]; }
    return d;
}
// a ROPE node's op_params, and the node as the descriptor a mat-mul launch that applies its rotation carries (no table)
static inline rope_params rope_params_of(const struct ggml_tensor * rope_node) {
    rope_params p;
    p.n_dims = rope_node->op_params[1]; p.mode = rope_node->op_params[2]; p.n_ctx_orig = rope_node->op_params[4];
    p.freq_base = op_f32(rope_node, 5); p.freq_scale = op_f32(rope_node, 6); p.ext_factor = op_f32(rope_node, 7);
    p.attn_factor = op_f32(rope_node, 8); p.beta_fast = op_f32(rope_node, 9); p.beta_slow = op_f32(rope_node, 10);
    return p;
}
static inline mmvq_rope mmvq_rope_of(const struct ggml_tensor * rope_node) {
    mmvq_rope r = {};
    r.pos = (const int32_t *) rope_node->src[1]->data; r.freq_factors = rope_node->src[2] ? (const float *) rope_node->src[2]->data : nullptr;
    r.head_dim = (int) rope_node->ne[0]; r.p = rope_params_of(rope_node);
    return r;
}
// the arguments of a dense (F16 / BF16 / F32 src0) MUL_MAT node: what mul_mat_dense_path decides from, for the launch and for the graph's scratch request alike
static inline mm_dense_args mm_dense_args_of(const struct ggml_tensor * dst) {
    const struct ggml_tensor * a = dst->src[0]; const struct ggml_tensor * b = dst->src[1];
    mm_dense_args p;
    p.a = a->data; p.type_a = (int) a->type;
    p.ne00 = a->ne[0]; p.ne01 = a->ne[1]; p.ne02 = a->ne[2]; p.ne03 = a->ne[3];
    p.nb00 = a->nb[0]; p.nb01 = a->nb[1]; p.nb02 = a->nb[2]; p.nb03 = a->nb[3];
    p.b = b->data; p.type_b = (int) b->type;
    p.ne10 = b->ne[0]; p.ne11 = b->ne[1]; p.ne12 = b->ne[2]; p.ne13 = b->ne[3];
    p.nb10 = b->nb[0]; p.nb11 = b->nb[1]; p.nb12 = b->nb[2]; p.nb13 = b->nb[3];
    p.dst = (float *) dst->data; p.nb1 = dst->nb[1]; p.nb2 = dst->nb[2]; p.nb3 = dst->nb[3];
    return p;
}
static inline bool ranges_overlap(const void * a, size_t na, const void * b, size_t nb) {
    const char * pa = (const char *) a; const char * pb = (const char *) b;
    return pa < pb + nb && pb < pa + na;
}

// ---- across files ----
// backend.cpp
bool tensor_is_split(const struct ggml_tensor * t);
void uploads_flush(mi_backend_ctx * c);
// option "profile": open / close the record of one quantized mat-mul launch (no-ops when the option is off). In a record, m < 0 marks a grouped
// mat-vec launch: |m| = KiB of weights (emit_mmv, backend_nodes.cpp)
void prof_begin(mi_backend_ctx * c, int type, int64_t m, int64_t k, int64_t n, uint64_t bytes, bool record_start = true);
void prof_end(mi_backend_ctx * c);
// backend_nodes.cpp
int  compute_node(mi_backend_ctx * c, struct ggml_cgraph * g, int i);     // returns the number of graph nodes consumed (>= 1)
void pass_end(mi_backend_ctx * c);                                         // the last node of a pass has run: the pending combine runs, aq ends
struct fa_operands { bool ok; size_t k_bytes, v_bytes; attn_call call; };
fa_operands fa_kv16_plan(const struct ggml_tensor * n, void * kv16, float * part, size_t part_bytes);
// backend_graph.cpp
enum ggml_status be_graph_compute(ggml_backend_t backend, struct ggml_cgraph * g);
void drop_graphs(mi_backend_ctx * c);
