// backend.cpp — the ggml-facing half of the MI355X backend: registry, device, buffer types (device, pinned host, row split),
// buffers, the stream backend's vtable, uploads, copies, events, supports_op, options, profile and the C exports.
// The backend*.cpp files are the ONLY translation units that depend on the ggml struct layouts (include/ggml-compat/*.h, or a
// real ggml's headers): backend_nodes.cpp runs one graph node (op launchers, fusion matchers), backend_graph.cpp runs a graph
// (the hipGraph cache, segmented capture and replay); backend_impl.h is what they share. Everything below the op switch is
// plain-pointer HIP code in kernels.h.
//
// Conventions kept from the reference's call sites:
//  * alloc failure -> NULL (src/llama-model.cpp:5602,5611); compute -> enum ggml_status
//    (src/llama-context.cpp:1101-1106); unsupported op -> supports_op says no, graph_compute never
//    meets one; supports_op never dereferences tensor->data (dummy tensors, src/llama-model.cpp:278-283).
//  * one ggml_backend_t = one ordered HIP stream driven by one host thread at a time
//    (tests/test-thread-safety.cpp:1-4); graph_compute is asynchronous (src/llama-context.cpp:1449).
//  * device type GPU so that it is auto-selected for offload (src/llama.cpp:183-190);
//    caps.async && caps.events so that pipeline parallelism can turn on (src/llama-context.cpp:262-279).
#include "backend_impl.h"

#include <mutex>

static constexpr size_t MI_BUFFER_ALIGN = 128;
static constexpr size_t MI_TENSOR_PAD   = 256;   // readable slack after quantized tensors (wave-wide 16 B loads may run past the last block)

extern "C" {
int    ggml_backend_mi355x_test_quantize(ggml_backend_t backend, const float * x, int64_t k, int64_t n, int kind, int8_t * qs, float * d, int16_t * bsums);
double ggml_backend_mi355x_test_hbm_read_gbps(ggml_backend_t backend, size_t bytes, int iters);
}

// ---------------------------------------------------------------------------------------------
// device buffer
// ---------------------------------------------------------------------------------------------
struct mi_buffer_ctx {
    int device;
    void * base;
};

static void buf_free(ggml_backend_buffer_t buffer) {
    mi_buffer_ctx * c = (mi_buffer_ctx *) buffer->context;
    set_device(c->device);
    MI_CHECK(hipFree(c->base));
    delete c;
}
static void * buf_get_base(ggml_backend_buffer_t buffer) { return ((mi_buffer_ctx *) buffer->context)->base; }

static enum ggml_status buf_init_tensor(ggml_backend_buffer_t buffer, struct ggml_tensor * tensor) {
    mi_buffer_ctx * c = (mi_buffer_ctx *) buffer->context;
    if (tensor->view_src != NULL) return GGML_STATUS_SUCCESS;
    if (ggml_is_quantized(tensor->type) && tensor->view_src == NULL) {
        // zero the padding after the last block so over-reads see defined bytes
        const size_t size = ggml_nbytes(tensor);
        const size_t alloc = ggml_backend_buft_get_alloc_size(buffer->buft, tensor);
        if (alloc > size) {
            set_device(c->device);
            MI_CHECK(hipMemset((char *) tensor->data + size, 0, alloc - size));
        }
    }
    return GGML_STATUS_SUCCESS;
}
static void buf_memset_tensor(ggml_backend_buffer_t buffer, struct ggml_tensor * tensor, uint8_t value, size_t offset, size_t size) {
    mi_buffer_ctx * c = (mi_buffer_ctx *) buffer->context;
    set_device(c->device);
    MI_CHECK(hipMemsetAsync((char *) tensor->data + offset, value, size, hipStreamPerThread));
    MI_CHECK(hipStreamSynchronize(hipStreamPerThread));
}
static void buf_set_tensor(ggml_backend_buffer_t buffer, struct ggml_tensor * tensor, const void * data, size_t offset, size_t size) {
    mi_buffer_ctx * c = (mi_buffer_ctx *) buffer->context;
    set_device(c->device);
    MI_CHECK(hipMemcpyAsync((char *) tensor->data + offset, data, size, hipMemcpyHostToDevice, hipStreamPerThread));
    MI_CHECK(hipStreamSynchronize(hipStreamPerThread));
}
static void buf_get_tensor(ggml_backend_buffer_t buffer, const struct ggml_tensor * tensor, void * data, size_t offset, size_t size) {
    mi_buffer_ctx * c = (mi_buffer_ctx *) buffer->context;
    set_device(c->device);
    MI_CHECK(hipMemcpyAsync(data, (const char *) tensor->data + offset, size, hipMemcpyDeviceToHost, hipStreamPerThread));
    MI_CHECK(hipStreamSynchronize(hipStreamPerThread));
}

static bool buffer_is_mi355x(ggml_backend_buffer_t buffer);

static bool buf_cpy_tensor(ggml_backend_buffer_t buffer, const struct ggml_tensor * src, struct ggml_tensor * dst) {
    ggml_backend_buffer_t sbuf = src->view_src ? src->view_src->buffer : src->buffer;
    if (!sbuf || !buffer_is_mi355x(sbuf)) return false;
    mi_buffer_ctx * sc = (mi_buffer_ctx *) sbuf->context;
    mi_buffer_ctx * dc = (mi_buffer_ctx *) buffer->context;
    set_device(dc->device);
    if (sc->device == dc->device) {
        MI_CHECK(hipMemcpyAsync(dst->data, src->data, ggml_nbytes(src), hipMemcpyDeviceToDevice, hipStreamPerThread));
    } else {
        MI_CHECK(hipMemcpyPeerAsync(dst->data, dc->device, src->data, sc->device, ggml_nbytes(src), hipStreamPerThread));   // xGMI hop
    }
    MI_CHECK(hipStreamSynchronize(hipStreamPerThread));
    return true;
}
static void buf_clear(ggml_backend_buffer_t buffer, uint8_t value) {
    mi_buffer_ctx * c = (mi_buffer_ctx *) buffer->context;
    set_device(c->device);
    MI_CHECK(hipMemsetAsync(c->base, value, buffer->size, hipStreamPerThread));
    MI_CHECK(hipStreamSynchronize(hipStreamPerThread));
}

static const struct ggml_backend_buffer_i mi_buffer_iface = {
    /* .free_buffer   = */ buf_free,
    /* .get_base      = */ buf_get_base,
    /* .init_tensor   = */ buf_init_tensor,
    /* .memset_tensor = */ buf_memset_tensor,
    /* .set_tensor    = */ buf_set_tensor,
    /* .get_tensor    = */ buf_get_tensor,
    /* .cpy_tensor    = */ buf_cpy_tensor,
    /* .clear         = */ buf_clear,
    /* .reset         = */ NULL,
};

static bool buffer_is_mi355x(ggml_backend_buffer_t buffer) { return buffer->iface.free_buffer == buf_free; }

// ---------------------------------------------------------------------------------------------
// device buffer type
// ---------------------------------------------------------------------------------------------
static const char * buft_get_name(ggml_backend_buffer_type_t buft) { return ((mi_device *) buft->context)->name.c_str(); }

static ggml_backend_buffer_t buft_alloc_buffer(ggml_backend_buffer_type_t buft, size_t size) {
    mi_device * d = (mi_device *) buft->context;
    set_device(d->id);
    void * p = NULL;
    hipError_t err = hipMalloc(&p, size + MI_TENSOR_PAD);
    if (err != hipSuccess) {
        (void) hipGetLastError();
        MI_LOG("allocating %.2f MiB on device %d failed: %s\n", size/1024.0/1024.0, d->id, hipGetErrorString(err));
        return NULL;
    }
    mi_buffer_ctx * c = new mi_buffer_ctx{ d->id, p };
    return ggml_backend_buffer_init(buft, mi_buffer_iface, c, size);
}
static size_t buft_get_alignment(ggml_backend_buffer_type_t) { return MI_BUFFER_ALIGN; }
static size_t buft_get_alloc_size(ggml_backend_buffer_type_t, const struct ggml_tensor * tensor) {
    size_t size = ggml_nbytes(tensor);
    if (ggml_is_quantized(tensor->type)) size += MI_TENSOR_PAD;
    return size;
}
static bool buft_is_host_no(ggml_backend_buffer_type_t) { return false; }

static const struct ggml_backend_buffer_type_i mi_buft_iface = {
    /* .get_name       = */ buft_get_name,
    /* .alloc_buffer   = */ buft_alloc_buffer,
    /* .get_alignment  = */ buft_get_alignment,
    /* .get_max_size   = */ NULL,
    /* .get_alloc_size = */ buft_get_alloc_size,
    /* .is_host        = */ buft_is_host_no,
};

// ---------------------------------------------------------------------------------------------
// row-split buffer type (-sm row; the host binds it through the "ggml_backend_split_buffer_type" proc, src/llama-model.cpp:368-387).
// EXPERIMENTAL until it has run on two real GPUs: so far only under GGML_MI355X_VIRTUAL_DEVICES (both "devices" the same HIP device, no peer traffic).
// Peer kernels store their row ranges straight into the main device's compute buffer through the peer mapping, ordered by events only; that the main device
// sees those stores without stale L2 lines is unproven here (the reference computes into a per-device dst and copies: ggml-cuda.cu ggml_cuda_op_mul_mat).
// a weight matrix's ROWS are spread over the devices in the proportions of tensor_split; every device holds its slice in its own HBM.
// A MUL_MAT on such a weight runs one launch per device, each on its own stream: the devices read the (small) activations straight from the
// main device's memory and write their rows of the result straight into the main device's dst — both through the peer mappings over xGMI, no
// staging copies and no collective (the result is a concatenation of row ranges, not a sum). Only 2-D quantized weights of MUL_MAT can live here
// (supports_op refuses everything else, so the host's weight_buft_supported probe, src/llama-model.cpp:152-286, sends norms, biases and
// expert stacks to the device's ordinary buffer type).
// ---------------------------------------------------------------------------------------------
struct mi_split_buft_ctx {
    int main_device = 0;                                   // index into G().devices
    float cum[GGML_MI355X_MAX_DEVICES + 1] = {};           // cum[i] = fraction of the rows before device i; cum[n_devices] = 1
    std::string name;
    struct ggml_backend_buffer_type buft;
};
struct mi_split_buffer_ctx {
    mi_split_buft_ctx * bt;
    std::vector<mi_split_tensor *> tensors;
};
static const int64_t MI_SPLIT_ROW_ROUND = 64;              // slice boundaries at multiples of this many rows (the MFMA tile height of the prefill kernel)

static void split_rows(const mi_split_buft_ctx * bt, int64_t nrows, int64_t * row_lo) {
    const int n = G().n_devices;
    for (int i = 0; i <= n; i++) {
        int64_t r = i == n ? nrows : (int64_t)(nrows*(double) bt->cum[i]);
        if (i > 0 && i < n) r -= r % MI_SPLIT_ROW_ROUND;
        row_lo[i] = i == 0 ? 0 : std::max(r, row_lo[i - 1]);
    }
}
static void split_buf_free(ggml_backend_buffer_t buffer) {
    mi_split_buffer_ctx * c = (mi_split_buffer_ctx *) buffer->context;
    for (mi_split_tensor * e : c->tensors) {
        for (int i = 0; i < G().n_devices; i++) if (e->data[i]) { set_device(G().devices[i].id); MI_CHECK(hipFree(e->data[i])); }
        delete e;
    }
    delete c;
}
static void * split_buf_get_base(ggml_backend_buffer_t) { return (void *) 0x1000; }     // never dereferenced: the slices hang off tensor->extra
static enum ggml_status split_buf_init_tensor(ggml_backend_buffer_t buffer, struct ggml_tensor * tensor) {
    mi_split_buffer_ctx * c = (mi_split_buffer_ctx *) buffer->context;
    if (tensor->view_src != NULL || !ggml_is_contiguous(tensor) || tensor->ne[2] != 1 || tensor->ne[3] != 1) return GGML_STATUS_FAILED;   // whole 2-D matrices only
    mi_split_tensor * e = new mi_split_tensor;
    split_rows(c->bt, tensor->ne[1], e->row_lo);
    for (int i = 0; i < G().n_devices; i++) {
        const int64_t rows = e->row_lo[i + 1] - e->row_lo[i];
        if (rows == 0) continue;
        const size_t bytes = (size_t) rows*tensor->nb[1];
        set_device(G().devices[i].id);
        if (hipMalloc(&e->data[i], bytes + MI_TENSOR_PAD) != hipSuccess) {
            (void) hipGetLastError();
            for (int j = 0; j < i; j++) if (e->data[j]) { set_device(G().devices[j].id); (void) hipFree(e->data[j]); }
            delete e;
            return GGML_STATUS_ALLOC_FAILED;
        }
        MI_CHECK(hipMemset((char *) e->data[i] + bytes, 0, MI_TENSOR_PAD));       // wave-wide loads may run past the last block
    }
    c->tensors.push_back(e);
    tensor->extra = e;
    return GGML_STATUS_SUCCESS;
}
static void split_buf_set_tensor(ggml_backend_buffer_t, struct ggml_tensor * tensor, const void * data, size_t offset, size_t size) {
    GGML_ASSERT(offset == 0 && size == ggml_nbytes(tensor) && "split tensors are written whole");
    const mi_split_tensor * e = (const mi_split_tensor *) tensor->extra;
    for (int i = 0; i < G().n_devices; i++) {
        if (!e->data[i]) continue;
        set_device(G().devices[i].id);
        MI_CHECK(hipMemcpyAsync(e->data[i], (const char *) data + e->row_lo[i]*tensor->nb[1], (size_t)(e->row_lo[i + 1] - e->row_lo[i])*tensor->nb[1], hipMemcpyHostToDevice, hipStreamPerThread));
    }
    for (int i = 0; i < G().n_devices; i++) if (e->data[i]) { set_device(G().devices[i].id); MI_CHECK(hipStreamSynchronize(hipStreamPerThread)); }
}
static void split_buf_get_tensor(ggml_backend_buffer_t, const struct ggml_tensor * tensor, void * data, size_t offset, size_t size) {
    GGML_ASSERT(offset == 0 && size == ggml_nbytes(tensor) && "split tensors are read whole");
    const mi_split_tensor * e = (const mi_split_tensor *) tensor->extra;
    for (int i = 0; i < G().n_devices; i++) {
        if (!e->data[i]) continue;
        set_device(G().devices[i].id);
        MI_CHECK(hipMemcpyAsync((char *) data + e->row_lo[i]*tensor->nb[1], e->data[i], (size_t)(e->row_lo[i + 1] - e->row_lo[i])*tensor->nb[1], hipMemcpyDeviceToHost, hipStreamPerThread));
    }
    for (int i = 0; i < G().n_devices; i++) if (e->data[i]) { set_device(G().devices[i].id); MI_CHECK(hipStreamSynchronize(hipStreamPerThread)); }
}
static void split_buf_clear(ggml_backend_buffer_t, uint8_t) {}
static const struct ggml_backend_buffer_i mi_split_buffer_iface = {
    /* .free_buffer   = */ split_buf_free,
    /* .get_base      = */ split_buf_get_base,
    /* .init_tensor   = */ split_buf_init_tensor,
    /* .memset_tensor = */ NULL,
    /* .set_tensor    = */ split_buf_set_tensor,
    /* .get_tensor    = */ split_buf_get_tensor,
    /* .cpy_tensor    = */ NULL,
    /* .clear         = */ split_buf_clear,
    /* .reset         = */ NULL,
};
static const char * split_buft_get_name(ggml_backend_buffer_type_t buft) { return ((mi_split_buft_ctx *) buft->context)->name.c_str(); }
static ggml_backend_buffer_t split_buft_alloc_buffer(ggml_backend_buffer_type_t buft, size_t size) {
    // the slices are allocated per tensor in init_tensor: the address range handed to the host's allocator is only bookkeeping
    return ggml_backend_buffer_init(buft, mi_split_buffer_iface, new mi_split_buffer_ctx{ (mi_split_buft_ctx *) buft->context, {} }, size);
}
static size_t split_buft_get_alloc_size(ggml_backend_buffer_type_t buft, const struct ggml_tensor * tensor) {
    int64_t row_lo[GGML_MI355X_MAX_DEVICES + 1];
    split_rows((const mi_split_buft_ctx *) buft->context, tensor->ne[1], row_lo);
    size_t total = 0;
    for (int i = 0; i < G().n_devices; i++) if (row_lo[i + 1] > row_lo[i]) total += (size_t)(row_lo[i + 1] - row_lo[i])*tensor->nb[1] + MI_TENSOR_PAD;
    return total;
}
static const struct ggml_backend_buffer_type_i mi_split_buft_iface = {
    /* .get_name       = */ split_buft_get_name,
    /* .alloc_buffer   = */ split_buft_alloc_buffer,
    /* .get_alignment  = */ buft_get_alignment,
    /* .get_max_size   = */ NULL,
    /* .get_alloc_size = */ split_buft_get_alloc_size,
    /* .is_host        = */ buft_is_host_no,
};
static bool buft_is_split(ggml_backend_buffer_type_t buft) { return buft && buft->iface.get_name == split_buft_get_name; }
bool tensor_is_split(const struct ggml_tensor * t) { return t && t->buffer && buft_is_split(t->buffer->buft); }

// ---------------------------------------------------------------------------------------------
// pinned host buffer type (src/llama-model-loader.cpp:951-959 uses it for the 4 x 1 MiB upload ring)
// ---------------------------------------------------------------------------------------------
static void host_buf_free(ggml_backend_buffer_t buffer) { MI_CHECK(hipHostFree(buffer->context)); }
static void * host_buf_get_base(ggml_backend_buffer_t buffer) { return buffer->context; }
static void host_buf_memset_tensor(ggml_backend_buffer_t, struct ggml_tensor * t, uint8_t v, size_t off, size_t size) { memset((char *) t->data + off, v, size); }
static void host_buf_set_tensor(ggml_backend_buffer_t, struct ggml_tensor * t, const void * data, size_t off, size_t size) { memcpy((char *) t->data + off, data, size); }
static void host_buf_get_tensor(ggml_backend_buffer_t, const struct ggml_tensor * t, void * data, size_t off, size_t size) { memcpy(data, (const char *) t->data + off, size); }
static void host_buf_clear(ggml_backend_buffer_t buffer, uint8_t value) { memset(buffer->context, value, buffer->size); }

static const struct ggml_backend_buffer_i mi_host_buffer_iface = {
    host_buf_free, host_buf_get_base, NULL, host_buf_memset_tensor, host_buf_set_tensor, host_buf_get_tensor, NULL, host_buf_clear, NULL,
};

static const char * host_buft_get_name(ggml_backend_buffer_type_t) { return GGML_MI355X_NAME "_Host"; }
static ggml_backend_buffer_t host_buft_alloc_buffer(ggml_backend_buffer_type_t buft, size_t size) {
    void * p = NULL;
    hipError_t err = hipHostMalloc(&p, size, hipHostMallocDefault);
    if (err != hipSuccess) {
        (void) hipGetLastError();
        MI_LOG("failed to allocate %.2f MiB of pinned memory: %s\n", size/1024.0/1024.0, hipGetErrorString(err));
        return NULL;
    }
    return ggml_backend_buffer_init(buft, mi_host_buffer_iface, p, size);
}
static size_t host_buft_get_alignment(ggml_backend_buffer_type_t) { return 64; }
static bool host_buft_is_host(ggml_backend_buffer_type_t) { return true; }

static const struct ggml_backend_buffer_type_i mi_host_buft_iface = {
    host_buft_get_name, host_buft_alloc_buffer, host_buft_get_alignment, NULL, NULL, host_buft_is_host,
};

static hipEvent_t prof_event(mi_backend_ctx * c) {
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e; MI_CHECK(hipEventCreate(&e)); return e;
}
// record_start = false: the pair is only made — the caller hands it to a launch that carries it as its dispatch's own start / stop events
void prof_begin(mi_backend_ctx * c, int type, int64_t m, int64_t k, int64_t n, uint64_t bytes, bool record_start) {
    if (!c->profiling || c->prof_suspend) return;
    mi_backend_ctx::prof_rec r = { type, m, k, n, bytes, prof_event(c), prof_event(c) };
    if (record_start) MI_CHECK(hipEventRecord(r.e0, c->stream));
    c->prof.push_back(r);
}
void prof_end(mi_backend_ctx * c) {
    if (!c->profiling || c->prof_suspend) return;
    MI_CHECK(hipEventRecord(c->prof.back().e1, c->stream));
}

static ggml_guid_t mi_guid(void) {
    static ggml_guid guid = { 0x4d, 0x49, 0x33, 0x35, 0x35, 0x58, 0x67, 0x66, 0x78, 0x39, 0x35, 0x30, 0x63, 0x64, 0x6e, 0x34 };
    return &guid;
}

static const char * be_get_name(ggml_backend_t backend) { return ((mi_backend_ctx *) backend->context)->name.c_str(); }

static void be_free(ggml_backend_t backend) {
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    if (c->stream) (void) hipStreamSynchronize(c->stream);
    drop_graphs(c);
    if (c->scratch) (void) hipFree(c->scratch);
    if (c->attn_part) (void) hipFree(c->attn_part);
    if (c->moe_ws) (void) hipFree(c->moe_ws);
    if (c->kv16) (void) hipFree(c->kv16);
    if (c->cvt) (void) hipFree(c->cvt);
    if (c->err_host) (void) hipHostFree(c->err_host);
    if (c->up.host) { (void) hipHostFree(c->up.host); (void) hipEventDestroy(c->up.ev[0]); (void) hipEventDestroy(c->up.ev[1]); }
    if (c->fin_img) (void) hipFree(c->fin_img);
    if (c->fin_cnt) (void) hipFree(c->fin_cnt);
    if (c->rope_tab) (void) hipFree(c->rope_tab);
    for (int i = 0; i < G().n_devices; i++) {
        mi_backend_ctx::split_peer & pr = c->peers[i];
        if (!pr.stream) continue;
        set_device(G().devices[i].id);
        (void) hipStreamSynchronize(pr.stream);
        if (pr.scratch) (void) hipFree(pr.scratch);
        (void) hipEventDestroy(pr.done); (void) hipStreamDestroy(pr.stream);
    }
    set_device(c->device);
    if (c->split_ready) (void) hipEventDestroy(c->split_ready);
    if (c->cpy_ev) (void) hipEventDestroy(c->cpy_ev);
    if (c->stream) (void) hipStreamDestroy(c->stream);
    delete c;
    delete backend;
}

// ---- small uploads, batched -------------------------------------------------------------------------------------
void uploads_flush(mi_backend_ctx * c) {
    if (c->up.n == 0) return;
    upload_batch_launch(c->up.b, c->stream);
    c->cnt.kernels_launched++;
    c->up.n = 0;
}
static bool uploads_stage(mi_backend_ctx * c, void * dst, const void * data, size_t size) {
    auto & u = c->up;
    if (u.failed) return false;
    if (!u.host) {
        if (hipHostMalloc((void **) &u.host, 2*mi_backend_ctx::UP_HALF, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer((void **) &u.dev, u.host, 0) != hipSuccess ||
            hipEventCreateWithFlags(&u.ev[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&u.ev[1], hipEventDisableTiming) != hipSuccess) {
            (void) hipGetLastError(); u.failed = true; return false;
        }
    }
    const size_t need = (size + 255) & ~(size_t) 255;
    if (u.off + need > mi_backend_ctx::UP_HALF) {
        // this half is full: everything that reads it is on the stream once the pending batch is; the other half may be reused when ITS event has passed
        uploads_flush(c);
        MI_CHECK(hipEventRecord(u.ev[u.cur], c->stream)); u.ev_pending[u.cur] = true;
        u.cur ^= 1; u.off = 0;
        if (u.ev_pending[u.cur]) { MI_CHECK(hipEventSynchronize(u.ev[u.cur])); u.ev_pending[u.cur] = false; }
    }
    if (u.n == UPLOAD_BATCH_MAX) uploads_flush(c);
    const size_t o = (size_t) u.cur*mi_backend_ctx::UP_HALF + u.off;
    memcpy(u.host + o, data, size);
    u.b.src[u.n] = u.dev + o; u.b.dst[u.n] = dst; u.b.bytes[u.n] = (uint32_t) size; u.b.blocks[u.n] = (int)((size + 4095)/4096);
    u.n++; u.b.n = u.n;
    u.off += need;
    return true;
}

// `data` is HOST memory (pageable or pinned), as the interface says; device-to-device copies have entry points of their own below
static void be_set_tensor_async(ggml_backend_t backend, struct ggml_tensor * tensor, const void * data, size_t offset, size_t size) {
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    if (size == 0) return;
    static const bool batch = env_on("GGML_MI355X_UPLOAD_BATCH");
    if (batch && size <= mi_backend_ctx::UP_SMALL_MAX && uploads_stage(c, (char *) tensor->data + offset, data, size)) return;
    uploads_flush(c);       // stream order: what was set before this goes first
    MI_CHECK(hipMemcpyAsync((char *) tensor->data + offset, data, size, hipMemcpyHostToDevice, c->stream));
}
static void be_get_tensor_async(ggml_backend_t backend, const struct ggml_tensor * tensor, void * data, size_t offset, size_t size) {
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    uploads_flush(c);
    MI_CHECK(hipMemcpyAsync(data, (const char *) tensor->data + offset, size, hipMemcpyDeviceToHost, c->stream));
}

// layer-split hand-off: a point-to-point copy of [n_embd, n_tokens] F32 over one xGMI link,
// ordered after the producer stream's work and before the consumer stream's next op, no host sync.
static bool be_cpy_tensor_async(ggml_backend_t backend_src, ggml_backend_t backend_dst, const struct ggml_tensor * src, struct ggml_tensor * dst) {
    if (!ggml_backend_is_mi355x(backend_src) || !ggml_backend_is_mi355x(backend_dst)) return false;
    ggml_backend_buffer_t sbuf = src->view_src ? src->view_src->buffer : src->buffer;
    ggml_backend_buffer_t dbuf = dst->view_src ? dst->view_src->buffer : dst->buffer;
    if (!buffer_is_mi355x(sbuf) || !buffer_is_mi355x(dbuf)) return false;
    mi_backend_ctx * cs = (mi_backend_ctx *) backend_src->context;
    mi_backend_ctx * cd = (mi_backend_ctx *) backend_dst->context;
    mi_buffer_ctx * bs = (mi_buffer_ctx *) sbuf->context;
    mi_buffer_ctx * bd = (mi_buffer_ctx *) dbuf->context;
    if (cs->device != bs->device || cd->device != bd->device) return false;
    set_device(cs->device); uploads_flush(cs);
    if (backend_src != backend_dst) { set_device(cd->device); uploads_flush(cd); }
    if (backend_src != backend_dst) {
        set_device(cs->device);
        if (cs->device == cd->device) {
            MI_CHECK(hipMemcpyAsync(dst->data, src->data, ggml_nbytes(dst), hipMemcpyDeviceToDevice, cs->stream));
        } else {
            MI_CHECK(hipMemcpyPeerAsync(dst->data, cd->device, src->data, cs->device, ggml_nbytes(dst), cs->stream));
        }
        // make the destination stream wait for the copy: one event per source backend, re-recorded per copy (a wait captures the record that precedes it,
        // so re-recording for the next copy does not disturb a wait already queued)
        if (!cs->cpy_ev) MI_CHECK(hipEventCreateWithFlags(&cs->cpy_ev, hipEventDisableTiming));
        MI_CHECK(hipEventRecord(cs->cpy_ev, cs->stream));
        set_device(cd->device);
        MI_CHECK(hipStreamWaitEvent(cd->stream, cs->cpy_ev, 0));
    } else {
        set_device(cs->device);
        MI_CHECK(hipMemcpyAsync(dst->data, src->data, ggml_nbytes(dst), hipMemcpyDeviceToDevice, cs->stream));
    }
    return true;
}

static void be_synchronize(ggml_backend_t backend) {
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    uploads_flush(c);
    MI_CHECK(hipStreamSynchronize(c->stream));
    if (c->err_host && c->err_host[1] != 0) {
        GGML_ABORT("MI355X backend: the MoE router kernel timed out waiting for an expert's logit (GGML_MI355X_MOE_ROUTE_WIDE=0 selects the one-workgroup router)");
    }
}

// ---- op support -----------------------------------------------------------------------------------
static bool float_type(enum ggml_type t) { return t == GGML_TYPE_F32 || t == GGML_TYPE_F16 || t == GGML_TYPE_BF16; }
static bool fa_kv_type(enum ggml_type t) { return t == GGML_TYPE_F16 || t == GGML_TYPE_BF16 || t == GGML_TYPE_Q8_0 || t == GGML_TYPE_Q4_0; }

static bool mi_supports_op(const struct ggml_tensor * op) {
    const struct ggml_tensor * s0 = op->src[0];
    const struct ggml_tensor * s1 = op->src[1];
    // row-split weights: MUL_MAT's 2-D quantized src0 only
    for (int j = 0; j < GGML_MAX_SRC; j++) {
        if (!tensor_is_split(op->src[j])) continue;
        if (op->op != GGML_OP_MUL_MAT || j != 0 || !ggml_is_quantized(s0->type) || s0->ne[2] != 1 || s0->ne[3] != 1 || s1->ne[2] != 1 || s1->ne[3] != 1) return false;
    }
    switch (op->op) {
        case GGML_OP_NONE: case GGML_OP_RESHAPE: case GGML_OP_VIEW: case GGML_OP_PERMUTE: case GGML_OP_TRANSPOSE:
            return true;
        case GGML_OP_MUL_MAT: {
            if (op->type != GGML_TYPE_F32) return false;
            if (ggml_is_quantized(s0->type)) {
                // quantized weights x F32 activations: the hot path
                if (!mul_mat_vec_q_supported((int) s0->type)) return false;
                if (s1->type != GGML_TYPE_F32 && s1->type != GGML_TYPE_F16) return false;      // (F16 activations: converted to F32 first — tests/test-backend-ops.cpp:5715-5716)
                if (s0->ne[0] % ggml_blck_size(s0->type) != 0) return false;
                if (s1->nb[0] != ggml_type_size(s1->type)) return false;
                if (s0->nb[0] != ggml_type_size(s0->type)) return false;
                return true;
            }
            if (s0->type == GGML_TYPE_F16 || s0->type == GGML_TYPE_F32 || s0->type == GGML_TYPE_BF16) {
                return s1->type == GGML_TYPE_F32 || s1->type == GGML_TYPE_F16;
            }
            return false;
        }
        case GGML_OP_MUL_MAT_ID: {
            if (op->type != GGML_TYPE_F32 || s1->type != GGML_TYPE_F32) return false;
            if (s0->type == GGML_TYPE_F16 || s0->type == GGML_TYPE_F32 || s0->type == GGML_TYPE_BF16)      // an unquantized expert stack (tests/test-backend-ops.cpp:5821-5824)
                return op->src[2]->type == GGML_TYPE_I32 && op->nb[0] == 4 && op->src[2]->ne[0] <= 65535 && op->src[2]->ne[1] <= 65535;      // (k_mm_id_dense: slots and tokens are grid dims y and z)
            if (!ggml_is_quantized(s0->type) || !mul_mat_vec_q_supported((int) s0->type)) return false;
            if (s0->ne[0] % ggml_blck_size(s0->type) != 0) return false;
            if (s1->nb[0] != sizeof(float)) return false;
            return op->src[2]->type == GGML_TYPE_I32;
        }
        case GGML_OP_FLASH_ATTN_EXT: {     // head sizes 64, 80, 96, 128, 192, 256 and 192/128 (attn_fa_head_sizes); K / V cache types F16, BF16, Q8_0, Q4_0; ALiBi and logit soft-cap (src/llama-graph.cpp:1245-1265)
            const struct ggml_tensor * k = op->src[1]; const struct ggml_tensor * v = op->src[2]; const struct ggml_tensor * mask = op->src[3];
            if (s0->type != GGML_TYPE_F32 || !fa_kv_type(k->type) || !fa_kv_type(v->type) || op->type != GGML_TYPE_F32) return false;
            // per-sequence KV streams: q, K and V carry the same ne[3] (one cache stream per q batch; ggml's broadcast of one cache over several is refused)
            if (s0->ne[3] != k->ne[3] || v->ne[3] != k->ne[3] || s0->ne[0] != k->ne[0] || v->ne[1] != k->ne[1] || v->ne[2] != k->ne[2] || s0->ne[2] % k->ne[2] != 0) return false;
            if (op_f32(op, 1) < 0.0f) return false;
            if (mask && (mask->type != GGML_TYPE_F16 || mask->ne[2] != 1 || (mask->ne[3] != 1 && mask->ne[3] != s0->ne[3]) || mask->ne[0] != k->ne[1] || mask->ne[1] < s0->ne[1] || mask->nb[1] % 16 || mask->nb[3] % 16)) return false;
            if (op->nb[1] != (size_t) v->ne[0]*4) return false;
            if (s0->nb[0] != 4 || k->nb[0] != ggml_type_size(k->type) || v->nb[0] != ggml_type_size(v->type) || s0->nb[1] % 16 || s0->nb[2] % 16 || s0->nb[3] % 16 || op->nb[3] % 16) return false;
            // (f16 rows are read 16 bytes at a time; block rows 2-byte aligned)
            if (k->nb[1] % (k->type == GGML_TYPE_F16 || k->type == GGML_TYPE_BF16 ? 16 : 2) || k->nb[2] % (k->type == GGML_TYPE_F16 || k->type == GGML_TYPE_BF16 ? 16 : 2) ||
                k->nb[3] % (k->type == GGML_TYPE_F16 || k->type == GGML_TYPE_BF16 ? 16 : 2)) return false;
            if (v->nb[1] % (v->type == GGML_TYPE_F16 || v->type == GGML_TYPE_BF16 ? 16 : 2) || v->nb[2] % (v->type == GGML_TYPE_F16 || v->type == GGML_TYPE_BF16 ? 16 : 2) ||
                v->nb[3] % (v->type == GGML_TYPE_F16 || v->type == GGML_TYPE_BF16 ? 16 : 2)) return false;
            // the head sizes, and the shapes: a few tokens' score row in LDS or their cell ranges through the fixed partial-result buffer; many tokens: 32-cell blocks
            return fa_kv16_plan(op, nullptr, nullptr, ATTN_PART_BYTES).ok;
        }
        case GGML_OP_RMS_NORM:
            return s0->type == GGML_TYPE_F32 && op->type == GGML_TYPE_F32 && s0->nb[0] == sizeof(float);
        case GGML_OP_ADD: case GGML_OP_MUL: case GGML_OP_DIV: case GGML_OP_SUB:
            return float_type(s0->type) && float_type(s1->type) && float_type(op->type);
        case GGML_OP_ADD_ID:
            return s0->type == GGML_TYPE_F32 && s1->type == GGML_TYPE_F32 && op->src[2]->type == GGML_TYPE_I32;
        case GGML_OP_SCALE:
            return s0->type == GGML_TYPE_F32;
        case GGML_OP_CPY: case GGML_OP_CONT: case GGML_OP_DUP: {
            const enum ggml_type st = s0->type, dt = op->op == GGML_OP_CPY ? s1->type : op->type;
            // a quantized KV cache's shift and defrag (src/llama-kv-cache-unified.cpp:1416-1670): CPY only, F32 <-> Q8_0 / Q4_0 and a move within one of the two types
            if (ggml_is_quantized(st) || ggml_is_quantized(dt)) return op->op == GGML_OP_CPY && cpy_quantized_supported(desc(s0), desc(s1));
            return (float_type(st) && float_type(dt)) || (st == GGML_TYPE_I32 && dt == GGML_TYPE_I32);
        }
        case GGML_OP_SET_ROWS:
            if (s0->type != GGML_TYPE_F32 || s1->type != GGML_TYPE_I64) return false;
            if (op->type == GGML_TYPE_Q8_0 || op->type == GGML_TYPE_Q4_0) return s0->ne[0] % 32 == 0 && op->nb[0] == ggml_type_size(op->type);   // quantized KV cache rows
            return float_type(op->type);
        case GGML_OP_GET_ROWS:
            return (float_type(s0->type) || s0->type == GGML_TYPE_I32) && s1->type == GGML_TYPE_I32 && s0->nb[0] == ggml_type_size(s0->type);
        case GGML_OP_SUM_ROWS:
            return s0->type == GGML_TYPE_F32;
        case GGML_OP_ARGSORT:
            return s0->type == GGML_TYPE_F32 && s0->ne[0] <= 1024;
        case GGML_OP_UNARY:
            return float_type(s0->type) && (int) ggml_get_unary_op(op) <= (int) GGML_UNARY_OP_GELU_ERF;
        case GGML_OP_GLU:
            return float_type(s0->type) && (int) ggml_get_glu_op(op) < (int) GGML_GLU_OP_COUNT;
        case GGML_OP_ROPE: {
            const int mode = op->op_params[2];
            if (mode & (GGML_ROPE_TYPE_MROPE | 16)) return false;    // mrope / vision: not on the path
            return float_type(s0->type) && s0->type == op->type;
        }
        case GGML_OP_SOFT_MAX:
            return s0->type == GGML_TYPE_F32 && s0->nb[0] == sizeof(float) && (s1 == NULL || s1->type == GGML_TYPE_F32 || s1->type == GGML_TYPE_F16);
        default:
            return false;
    }
}

static void be_event_record(ggml_backend_t backend, ggml_backend_event_t event) {
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    uploads_flush(c);
    MI_CHECK(hipEventRecord((hipEvent_t) event->context, c->stream));
}
static void be_event_wait(ggml_backend_t backend, ggml_backend_event_t event) {
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    uploads_flush(c);
    MI_CHECK(hipStreamWaitEvent(c->stream, (hipEvent_t) event->context, 0));
}

static const struct ggml_backend_i mi_backend_iface = {
    /* .get_name           = */ be_get_name,
    /* .free               = */ be_free,
    /* .set_tensor_async   = */ be_set_tensor_async,
    /* .get_tensor_async   = */ be_get_tensor_async,
    /* .cpy_tensor_async   = */ be_cpy_tensor_async,
    /* .synchronize        = */ be_synchronize,
    /* .graph_plan_create  = */ NULL,
    /* .graph_plan_free    = */ NULL,
    /* .graph_plan_update  = */ NULL,
    /* .graph_plan_compute = */ NULL,
    /* .graph_compute      = */ be_graph_compute,
    /* .event_record       = */ be_event_record,
    /* .event_wait         = */ be_event_wait,
};

// ---------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------
static const char * dev_get_name(ggml_backend_dev_t dev) { return ((mi_device *) dev->context)->name.c_str(); }
static const char * dev_get_description(ggml_backend_dev_t dev) { return ((mi_device *) dev->context)->description.c_str(); }
static void dev_get_memory(ggml_backend_dev_t dev, size_t * free, size_t * total) {
    mi_device * d = (mi_device *) dev->context;
    set_device(d->id);
    MI_CHECK(hipMemGetInfo(free, total));
}
static enum ggml_backend_dev_type dev_get_type(ggml_backend_dev_t) { return GGML_BACKEND_DEVICE_TYPE_GPU; }
static void dev_get_props(ggml_backend_dev_t dev, struct ggml_backend_dev_props * props) {
    props->name = dev_get_name(dev);
    props->description = dev_get_description(dev);
    props->type = GGML_BACKEND_DEVICE_TYPE_GPU;
    dev_get_memory(dev, &props->memory_free, &props->memory_total);
    props->caps.async = true;
    props->caps.host_buffer = true;
    props->caps.buffer_from_host_ptr = false;
    props->caps.events = true;
}
static ggml_backend_t dev_init_backend(ggml_backend_dev_t dev, const char *) {
    return ggml_backend_mi355x_init((int)((mi_device *) dev->context - G().devices));
}
static ggml_backend_buffer_type_t dev_get_buffer_type(ggml_backend_dev_t dev) { return &((mi_device *) dev->context)->buft; }
static ggml_backend_buffer_type_t dev_get_host_buffer_type(ggml_backend_dev_t) { return ggml_backend_mi355x_host_buffer_type(); }
static bool dev_supports_op(ggml_backend_dev_t, const struct ggml_tensor * op) { return mi_supports_op(op); }
static bool dev_supports_buft(ggml_backend_dev_t dev, ggml_backend_buffer_type_t buft) {
    if (buft->iface.get_name == host_buft_get_name) return false;   // kernels read device memory only
    if (buft_is_split(buft)) return ((mi_split_buft_ctx *) buft->context)->main_device == (int)((mi_device *) dev->context - G().devices);
    if (buft->iface.get_name != buft_get_name) return false;
    return ((mi_device *) buft->context)->id == ((mi_device *) dev->context)->id;
}
static bool dev_offload_op(ggml_backend_dev_t, const struct ggml_tensor * op) {
    // worth uploading host-resident weights for large batches only (same rule of thumb as the reference's GPU backends)
    const int min_batch = 32;
    if (op->op == GGML_OP_GET_ROWS) return false;
    if (op->op == GGML_OP_MUL_MAT_ID) return op->ne[2] >= min_batch;
    return op->ne[1] >= min_batch;
}
static ggml_backend_event_t dev_event_new(ggml_backend_dev_t dev) {
    mi_device * d = (mi_device *) dev->context;
    set_device(d->id);
    hipEvent_t ev;
    MI_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return new ggml_backend_event{ dev, ev };
}
static void dev_event_free(ggml_backend_dev_t, ggml_backend_event_t event) {
    MI_CHECK(hipEventDestroy((hipEvent_t) event->context));
    delete event;
}
static void dev_event_synchronize(ggml_backend_dev_t, ggml_backend_event_t event) { MI_CHECK(hipEventSynchronize((hipEvent_t) event->context)); }

static const struct ggml_backend_device_i mi_device_iface = {
    dev_get_name, dev_get_description, dev_get_memory, dev_get_type, dev_get_props, dev_init_backend,
    dev_get_buffer_type, dev_get_host_buffer_type, NULL /* buffer_from_host_ptr */,
    dev_supports_op, dev_supports_buft, dev_offload_op, dev_event_new, dev_event_free, dev_event_synchronize,
};

// ---------------------------------------------------------------------------------------------
// registry
// ---------------------------------------------------------------------------------------------
static const char * reg_get_name(ggml_backend_reg_t) { return GGML_MI355X_NAME; }
static size_t reg_get_device_count(ggml_backend_reg_t) { return (size_t) G().n_devices; }
static ggml_backend_dev_t reg_get_device(ggml_backend_reg_t, size_t index) {
    GGML_ASSERT(index < (size_t) G().n_devices);
    return &G().devices[index].dev;
}

static struct ggml_backend_feature * mi_get_features(ggml_backend_reg_t) {
    static struct ggml_backend_feature features[] = {
        { "ARCH", "gfx950" }, { "WAVE", "64" }, { "MMVQ", "sdot4+dpp" }, { "MMQ", "dequant_bf16+mfma_f32_32x32x16_bf16" }, { "GRAPHS", "1" }, { NULL, NULL },
    };
    return features;
}

static void * reg_get_proc_address(ggml_backend_reg_t, const char * name) {
    if (strcmp(name, "ggml_backend_get_features") == 0)        return (void *) mi_get_features;
    if (strcmp(name, "ggml_backend_split_buffer_type") == 0)   return (void *) ggml_backend_mi355x_split_buffer_type;
    if (strcmp(name, "ggml_backend_mi355x_get_stream") == 0)   return (void *) ggml_backend_mi355x_get_stream;
    if (strcmp(name, "ggml_backend_mi355x_get_counters") == 0) return (void *) ggml_backend_mi355x_get_counters;
    if (strcmp(name, "ggml_backend_mi355x_reset_counters") == 0) return (void *) ggml_backend_mi355x_reset_counters;
    if (strcmp(name, "ggml_backend_mi355x_set_option") == 0)   return (void *) ggml_backend_mi355x_set_option;
    if (strcmp(name, "ggml_backend_mi355x_get_profile") == 0)  return (void *) ggml_backend_mi355x_get_profile;
    if (strcmp(name, "ggml_backend_mi355x_tensor_set_from_device_async") == 0) return (void *) ggml_backend_mi355x_tensor_set_from_device_async;
    if (strcmp(name, "ggml_backend_mi355x_tensor_get_to_device_async") == 0)   return (void *) ggml_backend_mi355x_tensor_get_to_device_async;
    if (strcmp(name, "ggml_backend_mi355x_test_quantize") == 0) return (void *) ggml_backend_mi355x_test_quantize;
    if (strcmp(name, "ggml_backend_mi355x_test_hbm_read_gbps") == 0) return (void *) ggml_backend_mi355x_test_hbm_read_gbps;
    return NULL;
}

static const struct ggml_backend_reg_i mi_reg_iface = { reg_get_name, reg_get_device_count, reg_get_device, reg_get_proc_address };

static bool arch_is_gfx950(const hipDeviceProp_t & prop) { return strncmp(prop.gcnArchName, "gfx950", 6) == 0; }

mi_globals & G() {
    static mi_globals g;
    static std::once_flag once;
    std::call_once(once, [] {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) { (void) hipGetLastError(); n = 0; }
        g.reg = { GGML_BACKEND_API_VERSION, mi_reg_iface, NULL };
        g.host_buft = { mi_host_buft_iface, NULL, NULL };
        // GGML_MI355X_VIRTUAL_DEVICES=v lists every GPU v times (same HIP device, separate backend / stream / buffer type each): lets the
        // multi-device paths (layer split in one process, row split) be exercised on a one-GPU box
        const int virt = std::max(1, (int) env_int("GGML_MI355X_VIRTUAL_DEVICES", 1));
        for (int iv = 0; iv < n*virt && g.n_devices < GGML_MI355X_MAX_DEVICES; iv++) {
            const int i = iv/virt;
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, i) != hipSuccess) { (void) hipGetLastError(); continue; }
            if (!arch_is_gfx950(prop)) {
                MI_LOG("skipping device %d (%s, %s): this backend carries gfx950 code objects only\n", i, prop.name, prop.gcnArchName);
                continue;
            }
            mi_device & d = g.devices[g.n_devices];
            d.id = i;
            d.name = std::string(GGML_MI355X_NAME) + std::to_string(g.n_devices);
            d.description = prop.name;
            d.total_mem = prop.totalGlobalMem;
            d.dev = { mi_device_iface, &g.reg, &d };
            d.buft = { mi_buft_iface, &d.dev, &d };
            g.n_devices++;
        }
        if (g.n_devices > 0) g.host_buft.device = &g.devices[0].dev;
        // peer access for the layer-split hand-off over xGMI
        for (int i = 0; i < g.n_devices; i++) {
            for (int j = 0; j < g.n_devices; j++) {
                if (g.devices[i].id == g.devices[j].id) continue;
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, g.devices[i].id, g.devices[j].id) == hipSuccess && can) {
                    (void) hipSetDevice(g.devices[i].id);
                    hipError_t e = hipDeviceEnablePeerAccess(g.devices[j].id, 0);
                    if (e != hipSuccess) (void) hipGetLastError();
                }
            }
        }
        g.initialised = true;
    });
    return g;
}

// ---------------------------------------------------------------------------------------------
// exported C-ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

ggml_backend_reg_t ggml_backend_mi355x_reg(void) { return &G().reg; }

ggml_backend_reg_t ggml_backend_init(void) { return ggml_backend_mi355x_reg(); }

int ggml_backend_score(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void) hipGetLastError(); return 0; }
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, i) == hipSuccess && arch_is_gfx950(prop)) return 100;
    }
    return 0;
}

int ggml_backend_mi355x_get_device_count(void) { return G().n_devices; }

void ggml_backend_mi355x_get_device_description(int device, char * description, size_t description_size) {
    GGML_ASSERT(device >= 0 && device < G().n_devices);
    snprintf(description, description_size, "%s", G().devices[device].description.c_str());
}
void ggml_backend_mi355x_get_device_memory(int device, size_t * free, size_t * total) {
    GGML_ASSERT(device >= 0 && device < G().n_devices);
    dev_get_memory(&G().devices[device].dev, free, total);
}

ggml_backend_buffer_type_t ggml_backend_mi355x_buffer_type(int device) {
    if (device < 0 || device >= G().n_devices) return NULL;
    return &G().devices[device].buft;
}
ggml_backend_buffer_type_t ggml_backend_mi355x_host_buffer_type(void) {
    G();
    return &G().host_buft;
}

ggml_backend_t ggml_backend_mi355x_init(int device) {
    if (device < 0 || device >= G().n_devices) {
        MI_LOG("invalid device %d (have %d gfx950 device(s))\n", device, G().n_devices);
        return NULL;
    }
    mi_device & d = G().devices[device];
    set_device(d.id);
    mi_backend_ctx * c = new mi_backend_ctx;
    c->device = d.id;
    c->dev_index = device;
    c->name = d.name;
    MI_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->use_graphs = env_on("GGML_MI355X_GRAPHS", c->use_graphs);
    c->use_fusion = env_on("GGML_MI355X_FUSION", c->use_fusion);
    ggml_backend_t backend = new ggml_backend{ mi_guid(), mi_backend_iface, &d.dev, c };
    return backend;
}

ggml_backend_buffer_type_t ggml_backend_mi355x_split_buffer_type(int main_device, const float * tensor_split) {
    static std::mutex mu;
    static std::vector<mi_split_buft_ctx *> made;          // buffer types live as long as the process (the host keeps the pointer in its buft lists)
    const int n = G().n_devices;
    if (main_device < 0 || main_device >= n) return NULL;
    float share[GGML_MI355X_MAX_DEVICES]; double sum = 0;
    for (int i = 0; i < n; i++) { share[i] = tensor_split && tensor_split[i] > 0 ? tensor_split[i] : 0.0f; sum += share[i]; }
    if (sum == 0) { for (int i = 0; i < n; i++) share[i] = 1.0f; sum = n; }       // all zero: equal shares
    mi_split_buft_ctx want; want.main_device = main_device;
    double acc = 0;
    for (int i = 0; i < n; i++) { want.cum[i] = (float)(acc/sum); acc += share[i]; }
    want.cum[n] = 1.0f;
    // every device that CAN receive rows must be mapped into the main device's address space and back: not only those with a share — the rounding of
    // split_rows hands remainder rows to the devices behind the last share too (shares [1, 0], 300 rows: 44 rows on device 1)
    // From split_rows' rounding: device i < n - 1 holds rows [round64(nrows*cum[i]), round64(nrows*cum[i + 1])) — empty exactly when its share is zero — and the LAST
    // device holds everything behind round64(nrows*cum[n - 1]), which is non-empty for some row count whatever its share (a fixed list of probe counts
    // missed row counts like 2880)
    bool gets_rows[GGML_MI355X_MAX_DEVICES] = {};
    for (int i = 0; i < n; i++) gets_rows[i] = share[i] > 0 || i == n - 1;
    for (int i = 0; i < n; i++) {
        if ((share[i] == 0 && !gets_rows[i]) || G().devices[i].id == G().devices[main_device].id) continue;
        int ab = 0, ba = 0;
        if (hipDeviceCanAccessPeer(&ab, G().devices[i].id, G().devices[main_device].id) != hipSuccess || hipDeviceCanAccessPeer(&ba, G().devices[main_device].id, G().devices[i].id) != hipSuccess || !ab || !ba) {
            (void) hipGetLastError();
            MI_LOG("row split: no peer mapping between %s and %s\n", G().devices[i].name.c_str(), G().devices[main_device].name.c_str());
            return NULL;
        }
    }
    std::lock_guard<std::mutex> lock(mu);
    for (mi_split_buft_ctx * m : made) if (m->main_device == main_device && memcmp(m->cum, want.cum, sizeof(want.cum)) == 0) return &m->buft;
    mi_split_buft_ctx * m = new mi_split_buft_ctx(want);
    if (made.empty()) MI_LOG("row split (-sm row) is EXPERIMENTAL on this backend: functional, not tuned, and so far exercised on virtual devices only\n");
    m->name = std::string(GGML_MI355X_NAME) + "_Split";
    m->buft = { mi_split_buft_iface, &G().devices[main_device].dev, m };
    made.push_back(m);
    return &m->buft;
}

bool ggml_backend_is_mi355x(ggml_backend_t backend) { return backend != NULL && ggml_guid_matches(backend->guid, mi_guid()); }

void ggml_backend_mi355x_tensor_set_from_device_async(ggml_backend_t backend, struct ggml_tensor * tensor, const void * dev_src, size_t offset, size_t size) {
    GGML_ASSERT(ggml_backend_is_mi355x(backend));
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    uploads_flush(c);
    MI_CHECK(hipMemcpyAsync((char *) tensor->data + offset, dev_src, size, hipMemcpyDeviceToDevice, c->stream));
}
void ggml_backend_mi355x_tensor_get_to_device_async(ggml_backend_t backend, const struct ggml_tensor * tensor, void * dev_dst, size_t offset, size_t size) {
    GGML_ASSERT(ggml_backend_is_mi355x(backend));
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    uploads_flush(c);
    MI_CHECK(hipMemcpyAsync(dev_dst, (const char *) tensor->data + offset, size, hipMemcpyDeviceToDevice, c->stream));
}
void * ggml_backend_mi355x_get_stream(ggml_backend_t backend) {
    GGML_ASSERT(ggml_backend_is_mi355x(backend));
    return (void *) ((mi_backend_ctx *) backend->context)->stream;
}
void ggml_backend_mi355x_get_counters(ggml_backend_t backend, struct ggml_backend_mi355x_counters * out) {
    GGML_ASSERT(ggml_backend_is_mi355x(backend));
    *out = ((mi_backend_ctx *) backend->context)->cnt;
}
void ggml_backend_mi355x_reset_counters(ggml_backend_t backend) {
    GGML_ASSERT(ggml_backend_is_mi355x(backend));
    ((mi_backend_ctx *) backend->context)->cnt = {};
}
int ggml_backend_mi355x_set_option(ggml_backend_t backend, const char * key, int value) {
    GGML_ASSERT(ggml_backend_is_mi355x(backend));
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    if (strcmp(key, "graphs") == 0) { c->use_graphs = value != 0; return 0; }
    if (strcmp(key, "profile") == 0) {
        // 1: eager, an event pair around every quantized mat-mul launch; 2: the same pairs captured into the hipGraphs (what the
        // replayed token really costs per launch, without the eager launch gaps); either way the graphs are rebuilt
        MI_CHECK(hipStreamSynchronize(c->stream));
        drop_graphs(c);
        for (auto & r : c->prof) { c->ev_pool.push_back(r.e0); c->ev_pool.push_back(r.e1); }
        c->prof.clear();
        c->profiling = value != 0; c->prof_in_graph = value == 2; c->prof_suspend = false;
        return 0;
    }
    if (strcmp(key, "fusion") == 0) {
        c->use_fusion = value != 0;
        MI_CHECK(hipStreamSynchronize(c->stream));
        drop_graphs(c);
        return 0;
    }
    if (strcmp(key, "moe_dual") == 0) {       // the prompt pass's expert chain: -1 = by pairs per expert (default), 0 = gate / up as two launches, 1 = the dual launch
        c->moe_dual = value;
        MI_CHECK(hipStreamSynchronize(c->stream));
        drop_graphs(c);
        return 0;
    }
    return -1;
}

// per-kernel timing of the quantized mat-mul launches recorded while option "profile" was on (SURVEY.md §5:
// "expose per-kernel bytes/time counters"). Synchronises the stream, aggregates by (type, m, k, n), clears the log.
int ggml_backend_mi355x_get_profile(ggml_backend_t backend, struct ggml_backend_mi355x_prof_entry * out, int cap) {
    GGML_ASSERT(ggml_backend_is_mi355x(backend));
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    MI_CHECK(hipStreamSynchronize(c->stream));
    int n = 0;
    for (auto & r : c->prof) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) { (void) hipGetLastError(); continue; }     // a captured pair whose graph never ran
        if (!c->prof_in_graph) { c->ev_pool.push_back(r.e0); c->ev_pool.push_back(r.e1); }
        int j = 0;
        for (; j < n; j++) if (out[j].type == r.type && out[j].m == r.m && out[j].k == r.k && out[j].n == r.n) break;
        if (j == n) {
            if (n == cap) continue;
            out[n] = { r.type, (int32_t) r.n, r.m, r.k, 0, 0.0, r.bytes, {0} };
            if (r.kernel) snprintf(out[n].kernel, sizeof(out[n].kernel), "%s", r.kernel);
            n++;
        }
        out[j].launches++; out[j].total_ms += ms;
    }
    if (!c->prof_in_graph) c->prof.clear();      // captured pairs stay with their graphs until the option changes
    return n;
}

// ---- test hooks (reached by name through get_proc_address; not part of the ggml contract) --------------
// quantize host activations on the device and return the int8 blocks: lets tests/ compare the device
// quantizer with the oracle bit for bit.
int ggml_backend_mi355x_test_quantize(ggml_backend_t backend, const float * x, int64_t k, int64_t n, int kind,
                                      int8_t * qs, float * d, int16_t * bsums) {
    GGML_ASSERT(ggml_backend_is_mi355x(backend));
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    if (kind != T_Q8_0 && kind != T_Q8_K) return -1;
    if (k % (kind == T_Q8_0 ? 32 : 256) != 0) return -2;
    float * dx = nullptr; void * scratch = nullptr;
    const size_t sb = act_q8_bytes(kind, k, n);
    MI_CHECK(hipMalloc(&dx, (size_t) k*n*4));
    MI_CHECK(hipMalloc(&scratch, sb));
    MI_CHECK(hipMemcpy(dx, x, (size_t) k*n*4, hipMemcpyHostToDevice));
    const act_q8 q = act_q8_carve(scratch, kind, k, n);
    quantize_act(dx, n, (size_t) k*4, 0, q, c->stream);
    MI_CHECK(hipStreamSynchronize(c->stream));
    const int64_t nd = kind == T_Q8_0 ? k/32 : k/256, nbs = kind == T_Q8_0 ? k/32 : k/16;
    MI_CHECK(hipMemcpy(qs, q.qs, (size_t) k*n, hipMemcpyDeviceToHost));
    MI_CHECK(hipMemcpy(d, q.d, (size_t) nd*n*4, hipMemcpyDeviceToHost));
    MI_CHECK(hipMemcpy(bsums, q.bsums, (size_t) nbs*n*2, hipMemcpyDeviceToHost));
    MI_CHECK(hipFree(dx)); MI_CHECK(hipFree(scratch));
    return 0;
}

// achievable HBM read rate on this box (GB/s) with the same 16 B/lane nontemporal loads the mat-vec kernels use
double ggml_backend_mi355x_test_hbm_read_gbps(ggml_backend_t backend, size_t bytes, int iters) {
    GGML_ASSERT(ggml_backend_is_mi355x(backend));
    mi_backend_ctx * c = (mi_backend_ctx *) backend->context;
    set_device(c->device);
    void * p = nullptr; unsigned * sink = nullptr;
    MI_CHECK(hipMalloc(&p, bytes)); MI_CHECK(hipMalloc(&sink, 256));
    MI_CHECK(hipMemset(p, 1, bytes));
    hipEvent_t e0, e1;
    MI_CHECK(hipEventCreate(&e0)); MI_CHECK(hipEventCreate(&e1));
    hbm_read_probe(p, bytes, sink, c->stream);
    MI_CHECK(hipEventRecord(e0, c->stream));
    for (int i = 0; i < iters; i++) hbm_read_probe(p, bytes, sink, c->stream);
    MI_CHECK(hipEventRecord(e1, c->stream));
    MI_CHECK(hipEventSynchronize(e1));
    float ms = 0; MI_CHECK(hipEventElapsedTime(&ms, e0, e1));
    MI_CHECK(hipEventDestroy(e0)); MI_CHECK(hipEventDestroy(e1));
    MI_CHECK(hipFree(p)); MI_CHECK(hipFree(sink));
    return (double) bytes*iters/(ms*1e-3)/1e9;
}

} // extern "C"
