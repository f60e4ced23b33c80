// engine.cpp — the C-ABI of include/hypermerge_amd.h (host side of the engine).
//
// Owns the HIP device, stream, events and staging buffers; sizes and launches
// the merge kernels.  No C++ exception crosses the ABI: every entry point
// catches and returns an hm_status.  There is no CPU fallback: if the HIP
// library cannot run, calls fail with HM_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>
#include <algorithm>
#include <new>
#include "../../include/hypermerge_amd.h"
#include "merge_kernels.h"
#include "engine_internal.h"
#include "waiting_kernels.h"
#include "changes_kernels.h"
#include "field_kernels.h"
#include "past_kernels.h"
#include "op_diff_kernels.h"
#include "state_kernels.h"

struct hm_engine {
    int device = 0;
    int flags = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {};
    float last_ms[2] = {0, 0};
    int n_last = 0;
    int num_cus = 256;
    std::string err;
    void *dbuf = nullptr;
    size_t dbuf_size = 0;
    void *pool = nullptr;        // merge_large_kernel cursor + scratch pool
    size_t pool_size = 0;
    hipStream_t h2d = nullptr, d2h = nullptr;   // copy streams of the chunked hm_merge_host pipeline
    const char *last_scratch = nullptr;         // scratch of the last launch (hm_last_deferred)
};

namespace {

int fail(hm_engine *e, int status, const std::string &msg) {
    if (e) e->err = msg;
    return status;
}

int hip_fail(hm_engine *e, hipError_t r, const char *what) {
    return fail(e, HM_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(r));
}

#define HIPCHK(e, call)                                   \
    do {                                                  \
        hipError_t _r = (call);                           \
        if (_r != hipSuccess) return hip_fail(e, _r, #call); \
    } while (0)

struct Caps { uint32_t opl, cls; bool lists, counters; };

Caps launch_caps(const hm_batch *b) {
    Caps c;
    uint32_t mo = b->max_ops;
    c.opl = mo <= 64 ? 1 : (mo <= 128 ? 2 : (mo <= 192 ? 3 : 4));
    // 0 = unknown hint -> the larger class (documents outside it are deferred)
    c.cls = (b->max_regs && b->max_objs && b->max_deps) ? hm_small_class(b->max_regs, b->max_objs, b->max_deps) : 1u;
    c.lists = (b->doc_flags & HM_DOC_HAS_LISTS) != 0;
    c.counters = (b->doc_flags & HM_DOC_HAS_COUNTERS) != 0;
    return c;
}

// The launch's scratch: [counters 256 B: large-kernel cursor, pool bump pointer, deferred
// count][deferred document list, n_docs u32][large-kernel pool].  `scratch` = caller memory of
// hm_launch_scratch_bytes(b) bytes, or NULL for the engine's own pool (calls on the engine pool
// must be serialised: one stream at a time, which the engine enforces by synchronising the
// device before the pool is resized).
int launch_merge(hm_engine *e, const hm_batch *b, const hm_results *o, hipStream_t s, const uint32_t *doc_slot,
                 const hm_extents *ext, void *scratch, uint32_t *epos = nullptr) {
    Caps c = launch_caps(b);
    SmallParams p;
    p.res_epos = epos;
    p.docs = b->docs; p.changes = b->changes; p.deps = b->deps; p.ops = b->ops; p.min_clock = b->min_clock;
    p.res_docs = o->docs; p.res_clock = o->clock; p.res_back_clock = o->back_clock; p.res_heads = o->heads;
    p.res_hist = o->hist; p.res_all_deps = o->all_deps; p.res_regs = o->regs; p.res_surv = o->surv;
    p.n_docs = b->n_docs; p.a_stride = b->a_stride; p.cap_regs = 0; p.cap_objs = 0; p.cap_deps = 0;
    p.counters = c.counters ? 1u : 0u;
    p.general_only = (e->flags & HM_CFG_GENERAL_ONLY) ? 1u : 0u;
    {
        static const int remap = [] { const char *v = getenv("HM_XCD_REMAP"); return v ? atoi(v) : 1; }();
        p.xcd_remap = remap ? 1u : 0u;
    }
    p.doc_slot = doc_slot;
    p.lim_changes = ext ? ext->n_changes : b->n_changes; p.lim_deps = ext ? ext->n_deps : b->n_deps;
    p.lim_ops = ext ? ext->n_ops : b->n_ops; p.lim_regs = ext ? ext->n_regs : b->n_regs;
    if (b->n_docs == 0) { e->n_last = 0; return HM_OK; }
    const size_t list_bytes = ((size_t)b->n_docs * 4 + 255) & ~(size_t)255;
    const size_t need = hm_launch_scratch_bytes(b);
    const size_t pool_bytes = need - 256 - list_bytes;
    char *pb = (char *)scratch;
    if (!pb) {
        if (need > e->pool_size) {
            if (e->pool) { HIPCHK(e, hipDeviceSynchronize()); HIPCHK(e, hipFree(e->pool)); }
            e->pool = nullptr; e->pool_size = 0;
            if (hipMalloc(&e->pool, need) != hipSuccess) return fail(e, HM_ERR_NOMEM, "hipMalloc scratch pool");
            e->pool_size = need;
        }
        pb = (char *)e->pool;
    }
    p.large_cursor = (uint32_t *)pb;
    unsigned long long *pool_used = (unsigned long long *)(pb + 8);
    p.n_deferred = (uint32_t *)(pb + 16);
    p.deferred = (uint32_t *)(pb + 256);
    HIPCHK(e, hipMemsetAsync(pb, 0, 32, s));
    // persistent grid: exactly the resident 1-wave workgroups (VGPR/LDS occupancy of the
    // instantiation), so every wave starts at once and the documents split evenly — a
    // larger grid would leave a partial second round of waves as a tail
    const uint32_t per_cu = hm_small_occupancy(c.opl, c.cls, c.lists, c.counters);
    uint32_t grid = std::min<uint32_t>(b->n_docs, (uint32_t)e->num_cus * per_cu);
    HIPCHK(e, hipEventRecord(e->ev[0], s));
    hipError_t r = hm_launch_small(p, c.opl, c.cls, c.lists, grid, s);
    if (r != hipSuccess) return hip_fail(e, r, "merge_small_kernel launch");
    HIPCHK(e, hipEventRecord(e->ev[1], s));
    HIPCHK(e, hipEventRecord(e->ev[2], s));
    r = hm_launch_large(p, pb + 256 + list_bytes, pool_bytes, pool_used, (uint32_t)e->num_cus * 4, s);
    if (r != hipSuccess) return hip_fail(e, r, "merge_large_kernel launch");
    HIPCHK(e, hipEventRecord(e->ev[3], s));
    e->n_last = 2;
    // the deferred list lives in the scratch: only the engine's own pool outlives this call
    // (caller scratch may be freed or reused before hm_last_deferred)
    e->last_scratch = scratch ? nullptr : pb;
    return HM_OK;
}

}  // namespace

size_t hm_launch_scratch_bytes(const hm_batch *b) {
    const size_t list_bytes = ((size_t)b->n_docs * 4 + 255) & ~(size_t)255;
    return 256 + list_bytes + hm_large_scratch_bound(b);
}

namespace {

// hm_merge_host splits a batch into document ranges when its tables are laid out in document
// order (each doc's changes, deps, ops and registers directly follow the previous doc's, as
// every encoder here writes them); other layouts, and small batches, go in one piece.
uint32_t host_chunks(const hm_batch *b) {
    const uint32_t per = 1u << 16;                 // >= 64k documents per chunk
    if (b->n_docs < 2 * per || !b->docs || !b->changes || !b->ops) return 1;
    uint64_t c = 0, p = 0, o = 0, r = 0;
    for (uint32_t i = 0; i < b->n_docs; i++) {
        const hm_doc_row &d = b->docs[i];
        if (d.change_off != c || d.dep_off != p || d.op_off != o || d.reg_off != r) return 1;
        c += d.n_changes; p += d.n_deps; o += d.n_ops; r += d.n_regs;
    }
    if (c != b->n_changes || p != b->n_deps || o != b->n_ops) return 1;
    return std::min<uint32_t>(16, b->n_docs / per);
}

int check_batch(hm_engine *e, const hm_batch *b) {
    if (!b || b->a_stride == 0 || b->a_stride > HM_MAX_STRIDE) return fail(e, HM_ERR_INVALID, "a_stride must be in [1,256]");
    if (b->n_docs && !b->docs) return fail(e, HM_ERR_INVALID, "docs table missing");
    if ((b->n_changes && !b->changes) || (b->n_deps && !b->deps) || (b->n_ops && !b->ops))
        return fail(e, HM_ERR_INVALID, "row table missing");
    return HM_OK;
}

}  // namespace

// ---- internal interface for store.cpp (engine_internal.h) ----
int hm_engine_launch_merge(hm_engine *e, const hm_batch *b, const hm_results *o, const uint32_t *doc_slot,
                           const hm_extents *ext, uint32_t *epos) {
    return launch_merge(e, b, o, e->stream, doc_slot, ext, nullptr, epos);
}
hipStream_t hm_engine_stream(hm_engine *e) { return e->stream; }
int hm_engine_device(hm_engine *e) { return e->device; }
int hm_engine_fail(hm_engine *e, int status, const char *msg) { return fail(e, status, msg); }

extern "C" {

uint32_t hm_abi_version(void) { return HM_ABI_VERSION; }

const char *hm_status_message(int status) {
    switch (status) {
    case HM_OK: return "ok";
    case HM_ERR_INCONSISTENT_SEQ: return "Inconsistent reuse of sequence number";
    case HM_ERR_UNKNOWN_OBJECT: return "Modification of unknown object";
    case HM_ERR_DUPLICATE_OBJECT: return "Duplicate creation of object";
    case HM_ERR_DUPLICATE_ELEM: return "Duplicate list element ID";
    case HM_ERR_MISSING_ELEM: return "Missing index entry for list element";
    case HM_ERR_UNSUPPORTED: return "document outside the engine envelope";
    case HM_ERR_INVALID: return "invalid batch";
    case HM_ERR_DEVICE: return "HIP device error";
    case HM_ERR_NOMEM: return "out of memory";
    default: return "unknown status";
    }
}

int hm_engine_create(const hm_config *cfg, hm_engine **out) {
    if (!out) return HM_ERR_INVALID;
    *out = nullptr;
    hm_engine *e = new (std::nothrow) hm_engine();
    if (!e) return HM_ERR_NOMEM;
    e->device = cfg ? cfg->device : 0;
    e->flags = cfg ? cfg->flags : 0;
    int n = 0;
    // a failing step is named on stderr (there is no engine to hold the message)
    auto fail = [&](const char *what, hipError_t r) {
        fprintf(stderr, "hm_engine_create: %s failed: %s (device %d, %d devices)\n", what, hipGetErrorString(r), e->device, n);
        delete e;
        return HM_ERR_DEVICE;
    };
    hipError_t r = hipGetDeviceCount(&n);
    if (r != hipSuccess) return fail("hipGetDeviceCount", r);
    if (n <= e->device) return fail("device ordinal", hipErrorInvalidDevice);
    if ((r = hipSetDevice(e->device)) != hipSuccess) return fail("hipSetDevice", r);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, e->device) == hipSuccess) e->num_cus = prop.multiProcessorCount;
    {
        size_t lim = 0, need = hm_large_stack_bytes();
        if (hipDeviceGetLimit(&lim, hipLimitStackSize) == hipSuccess && need > lim &&
            (r = hipDeviceSetLimit(hipLimitStackSize, need)) != hipSuccess) return fail("hipDeviceSetLimit(stack)", r);
    }
    if ((r = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", r);
    for (auto &ev : e->ev)
        if ((r = hipEventCreate(&ev)) != hipSuccess) return fail("hipEventCreate", r);
    *out = e;
    return HM_OK;
}

void hm_engine_destroy(hm_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->dbuf) (void)hipFree(e->dbuf);
    if (e->pool) (void)hipFree(e->pool);
    for (auto &ev : e->ev) if (ev) (void)hipEventDestroy(ev);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    if (e->h2d) (void)hipStreamDestroy(e->h2d);
    if (e->d2h) (void)hipStreamDestroy(e->d2h);
    delete e;
}

const char *hm_engine_last_error(const hm_engine *e) { return e ? e->err.c_str() : "no engine"; }

size_t hm_scratch_bytes(const hm_batch *b) { return b ? hm_launch_scratch_bytes(b) : 0; }

int hm_merge_device(hm_engine *e, const hm_batch *b, const hm_results *o, void *scratch, void *stream) {
    try {
        if (!e || !o) return HM_ERR_INVALID;
        int st = check_batch(e, b);
        if (st) return st;
        if (b->n_docs && (!b->max_changes && !b->max_ops && !b->max_regs && !b->max_objs))
            return fail(e, HM_ERR_INVALID, "device batches must carry max_* launch hints");
        HIPCHK(e, hipSetDevice(e->device));
        return launch_merge(e, b, o, stream ? (hipStream_t)stream : e->stream, nullptr, nullptr, scratch);
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_merge_device");
    }
}

int hm_debug_small_occupancy(hm_engine *e, const hm_batch *hb, uint32_t *out6) {
    if (!e || !hb || !out6) return HM_ERR_INVALID;
    if (hipSetDevice(e->device) != hipSuccess) return fail(e, HM_ERR_DEVICE, "hipSetDevice");
    hm_batch b = *hb;
    if (!b.max_changes && !b.max_ops && !b.max_regs && !b.max_objs && hb->docs) {
        for (uint32_t d = 0; d < b.n_docs; d++) {          // (the hints hm_merge_host computes)
            b.max_ops = std::max(b.max_ops, hb->docs[d].n_ops);
            b.max_regs = std::max(b.max_regs, hb->docs[d].n_regs);
            b.max_objs = std::max(b.max_objs, hb->docs[d].n_objs);
            b.max_deps = std::max(b.max_deps, hb->docs[d].n_deps);
            b.doc_flags |= hb->docs[d].flags;
        }
    }
    const Caps c = launch_caps(&b);
    out6[0] = hm_small_occupancy(c.opl, c.cls, c.lists, c.counters);
    out6[1] = (uint32_t)e->num_cus;
    out6[2] = c.opl; out6[3] = c.cls; out6[4] = c.lists ? 1u : 0u; out6[5] = c.counters ? 1u : 0u;
    return HM_OK;
}

int hm_merge_host(hm_engine *e, const hm_batch *hb, const hm_results *ho) {
    try {
        if (!e || !hb || !ho) return HM_ERR_INVALID;
        int st = check_batch(e, hb);
        if (st) return st;
        HIPCHK(e, hipSetDevice(e->device));
        hm_batch b = *hb;
        if (!b.max_changes && !b.max_ops && !b.max_regs && !b.max_objs) {
            for (uint32_t d = 0; d < b.n_docs; d++) {
                b.max_changes = std::max(b.max_changes, hb->docs[d].n_changes);
                b.max_ops = std::max(b.max_ops, hb->docs[d].n_ops);
                b.max_regs = std::max(b.max_regs, hb->docs[d].n_regs);
                b.max_objs = std::max(b.max_objs, hb->docs[d].n_objs);
                b.max_deps = std::max(b.max_deps, hb->docs[d].n_deps);
                b.doc_flags |= hb->docs[d].flags;
            }
        }
        const size_t S = b.a_stride;
        struct Seg { size_t bytes; size_t off; };
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        size_t sz[13] = {
            b.n_docs * sizeof(hm_doc_row), b.n_changes * sizeof(hm_change_row), b.n_deps * sizeof(hm_dep_row),
            b.n_ops * sizeof(hm_op_row), hb->min_clock ? b.n_docs * S * 4 : 0,
            b.n_docs * sizeof(hm_doc_result), b.n_docs * S * 4, b.n_docs * S * 4, b.n_docs * S * 4,
            b.n_changes * 4, b.n_changes * S * 4, b.n_regs * sizeof(hm_reg_result), b.n_ops * sizeof(hm_surv_result)};
        size_t off[13], total = 0;
        for (int i = 0; i < 13; i++) { off[i] = total; total += al(sz[i] ? sz[i] : 1); }
        if (total > e->dbuf_size) {
            if (e->dbuf) (void)hipFree(e->dbuf);
            e->dbuf = nullptr; e->dbuf_size = 0;
            if (hipMalloc(&e->dbuf, total) != hipSuccess) return fail(e, HM_ERR_NOMEM, "hipMalloc staging");
            e->dbuf_size = total;
        }
        char *base = (char *)e->dbuf;
        auto P = [&](int i) { return (void *)(base + off[i]); };
        hipStream_t s = e->stream;
        b.docs = (const hm_doc_row *)P(0); b.changes = (const hm_change_row *)P(1);
        b.deps = (const hm_dep_row *)P(2); b.ops = (const hm_op_row *)P(3);
        b.min_clock = hb->min_clock ? (const uint32_t *)P(4) : nullptr;
        hm_results d;
        d.docs = (hm_doc_result *)P(5); d.clock = (uint32_t *)P(6); d.back_clock = (uint32_t *)P(7);
        d.heads = (uint32_t *)P(8); d.hist = (int32_t *)P(9); d.all_deps = (uint32_t *)P(10);
        d.regs = (hm_reg_result *)P(11); d.surv = (hm_surv_result *)P(12);
        const void *src[5] = {hb->docs, hb->changes, hb->deps, hb->ops, hb->min_clock};
        void *dst[8] = {ho->docs, ho->clock, ho->back_clock, ho->heads, ho->hist, ho->all_deps, ho->regs, ho->surv};
        const uint32_t nchunk = host_chunks(hb);
        if (nchunk <= 1) {
            for (int i = 0; i < 5; i++)
                if (sz[i]) HIPCHK(e, hipMemcpyAsync(P(i), src[i], sz[i], hipMemcpyHostToDevice, s));
            // the survivor table is only defined on [0, n_surv) per doc: zero it for stable host views
            if (sz[12]) HIPCHK(e, hipMemsetAsync(P(12), 0, sz[12], s));
            st = launch_merge(e, &b, &d, s, nullptr, nullptr, nullptr);
            if (st) return st;
            for (int i = 0; i < 8; i++)
                if (sz[5 + i] && dst[i]) HIPCHK(e, hipMemcpyAsync(dst[i], P(5 + i), sz[5 + i], hipMemcpyDeviceToHost, s));
            HIPCHK(e, hipStreamSynchronize(s));
            return HM_OK;
        }
        // Chunked pipeline over document ranges (documents laid out in order, host_chunks):
        // chunk k's upload (h2d stream) overlaps chunk k-1's merge (engine stream) and chunk
        // k-2's download (d2h stream), so both PCIe directions run at once.  Each chunk is a
        // sub-batch whose doc-indexed pointers start at its first document; row offsets inside
        // the doc rows stay absolute into the full-size device tables.
        if (!e->h2d) HIPCHK(e, hipStreamCreateWithFlags(&e->h2d, hipStreamNonBlocking));
        if (!e->d2h) HIPCHK(e, hipStreamCreateWithFlags(&e->d2h, hipStreamNonBlocking));
        std::vector<hipEvent_t> evs(2 * nchunk, nullptr);
        int rc = HM_OK;
        auto cleanup = [&]() {
            (void)hipStreamSynchronize(e->h2d); (void)hipStreamSynchronize(s); (void)hipStreamSynchronize(e->d2h);
            for (auto ev : evs) if (ev) (void)hipEventDestroy(ev);
        };
        for (auto &ev : evs)
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { cleanup(); return fail(e, HM_ERR_DEVICE, "hipEventCreate"); }
        const hm_doc_row *hd = hb->docs;
        const uint32_t nd = b.n_docs;
        auto H2D = [&](void *dp, const void *hp, size_t bytes) {
            return bytes ? hipMemcpyAsync(dp, hp, bytes, hipMemcpyHostToDevice, e->h2d) : hipSuccess; };
        auto D2H = [&](void *hp, const void *dp, size_t bytes) {
            return (bytes && hp) ? hipMemcpyAsync(hp, dp, bytes, hipMemcpyDeviceToHost, e->d2h) : hipSuccess; };
#define HM_CK(x) do { hipError_t _r = (x); if (_r != hipSuccess) { rc = hip_fail(e, _r, #x); goto done; } } while (0)
        for (uint32_t k = 0; k < nchunk; k++) {
            const uint32_t d0 = (uint32_t)((uint64_t)nd * k / nchunk), d1 = (uint32_t)((uint64_t)nd * (k + 1) / nchunk);
            const uint32_t l = d1 - 1;
            const size_t c0 = hd[d0].change_off, c1 = (size_t)hd[l].change_off + hd[l].n_changes;
            const size_t p0 = hd[d0].dep_off, p1 = (size_t)hd[l].dep_off + hd[l].n_deps;
            const size_t o0 = hd[d0].op_off, o1 = (size_t)hd[l].op_off + hd[l].n_ops;
            const size_t r0 = hd[d0].reg_off, r1 = (size_t)hd[l].reg_off + hd[l].n_regs;
            char *dc = (char *)P(1), *dp = (char *)P(2), *dop = (char *)P(3);
            HM_CK(H2D((char *)P(0) + d0 * sizeof(hm_doc_row), hd + d0, (size_t)(d1 - d0) * sizeof(hm_doc_row)));
            HM_CK(H2D(dc + c0 * sizeof(hm_change_row), hb->changes + c0, (c1 - c0) * sizeof(hm_change_row)));
            HM_CK(H2D(dp + p0 * sizeof(hm_dep_row), hb->deps + p0, (p1 - p0) * sizeof(hm_dep_row)));
            HM_CK(H2D(dop + o0 * sizeof(hm_op_row), hb->ops + o0, (o1 - o0) * sizeof(hm_op_row)));
            if (hb->min_clock) HM_CK(H2D((char *)P(4) + d0 * S * 4, hb->min_clock + d0 * S, (d1 - d0) * S * 4));
            HM_CK(hipEventRecord(evs[2 * k], e->h2d));
            HM_CK(hipStreamWaitEvent(s, evs[2 * k], 0));
            HM_CK(hipMemsetAsync((char *)P(12) + o0 * sizeof(hm_surv_result), 0, (o1 - o0) * sizeof(hm_surv_result), s));
            {
                hm_batch cb = b;
                cb.n_docs = d1 - d0;
                cb.docs = b.docs + d0;
                cb.min_clock = b.min_clock ? b.min_clock + d0 * S : nullptr;
                hm_results co = d;
                co.docs = d.docs + d0; co.clock = d.clock + d0 * S; co.back_clock = d.back_clock + d0 * S;
                co.heads = d.heads + d0 * S;
                rc = launch_merge(e, &cb, &co, s, nullptr, nullptr, nullptr);
                if (rc) goto done;
            }
            HM_CK(hipEventRecord(evs[2 * k + 1], s));
            HM_CK(hipStreamWaitEvent(e->d2h, evs[2 * k + 1], 0));
            HM_CK(D2H(ho->docs ? ho->docs + d0 : nullptr, d.docs + d0, (size_t)(d1 - d0) * sizeof(hm_doc_result)));
            HM_CK(D2H(ho->clock ? ho->clock + d0 * S : nullptr, d.clock + d0 * S, (d1 - d0) * S * 4));
            HM_CK(D2H(ho->back_clock ? ho->back_clock + d0 * S : nullptr, d.back_clock + d0 * S, (d1 - d0) * S * 4));
            HM_CK(D2H(ho->heads ? ho->heads + d0 * S : nullptr, d.heads + d0 * S, (d1 - d0) * S * 4));
            HM_CK(D2H(ho->hist ? ho->hist + c0 : nullptr, d.hist + c0, (c1 - c0) * 4));
            HM_CK(D2H(ho->all_deps ? ho->all_deps + c0 * S : nullptr, d.all_deps + c0 * S, (c1 - c0) * S * 4));
            HM_CK(D2H(ho->regs ? ho->regs + r0 : nullptr, d.regs + r0, (r1 - r0) * sizeof(hm_reg_result)));
            HM_CK(D2H(ho->surv ? ho->surv + o0 : nullptr, d.surv + o0, (o1 - o0) * sizeof(hm_surv_result)));
        }
#undef HM_CK
    done:
        cleanup();
        return rc;
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_merge_host");
    }
}

// (the missing-deps calls read the docs, changes and deps tables only: no op table is asked for)
static int check_waiting_batch(hm_engine *e, const hm_batch *b) {
    if (!b || b->a_stride == 0 || b->a_stride > HM_MAX_STRIDE) return fail(e, HM_ERR_INVALID, "a_stride must be in [1,256]");
    if ((b->n_docs && !b->docs) || (b->n_changes && !b->changes) || (b->n_deps && !b->deps))
        return fail(e, HM_ERR_INVALID, "row table missing");
    return HM_OK;
}

// a merged cold batch (device tables of b, device results r) as the device queries' document
// source; request i is document i unless the caller sets handles
static DocSource batch_source(const hm_batch *b, const hm_results *r) {
    DocSource D = {};
    D.docs = b->docs; D.res = r->docs; D.n_docs = b->n_docs; D.S = b->a_stride;
    D.changes = b->changes; D.hist = r->hist; D.all_deps = r->all_deps; D.deps = b->deps; D.ops = b->ops;
    D.clock = r->clock; D.back_clock = r->back_clock;
    D.lim_c = b->n_changes; D.lim_d = b->n_deps; D.lim_o = b->n_ops;
    return D;
}

// the missing row of every document of the batch ([n_docs * a_stride])
static hipError_t launch_waiting_batch(const hm_batch *b, const hm_results *r, uint32_t *out_missing, hipStream_t s) {
    WaitingArgs A = {};
    A.n = b->n_docs; A.src = batch_source(b, r); A.out_missing = out_missing;
    return hm_launch_waiting(A, s);
}

int hm_missing_deps_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t *out_missing, void *stream) {
    try {
        if (!e || !r) return HM_ERR_INVALID;
        int st = check_waiting_batch(e, b);
        if (st) return st;
        if (!b->n_docs) return HM_OK;
        if (!out_missing || !r->docs || !r->clock || (b->n_changes && !r->hist))
            return fail(e, HM_ERR_INVALID, "hm_missing_deps needs the results' docs, clock and hist tables");
        HIPCHK(e, hipSetDevice(e->device));
        hipError_t hr = launch_waiting_batch(b, r, out_missing, stream ? (hipStream_t)stream : e->stream);
        return hr == hipSuccess ? HM_OK : hip_fail(e, hr, "waiting_kernel launch");
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_missing_deps_device");
    }
}

int hm_missing_deps_host(hm_engine *e, const hm_batch *hb, const hm_results *hr, uint32_t *out_missing) {
    try {
        if (!e || !hr) return HM_ERR_INVALID;
        int st = check_waiting_batch(e, hb);
        if (st) return st;
        if (!hb->n_docs) return HM_OK;
        if (!out_missing || !hr->docs || !hr->clock || (hb->n_changes && !hr->hist))
            return fail(e, HM_ERR_INVALID, "hm_missing_deps needs the results' docs, clock and hist tables");
        HIPCHK(e, hipSetDevice(e->device));
        const size_t S = hb->a_stride, n = hb->n_docs;
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t sz[7] = {n * sizeof(hm_doc_row), hb->n_changes * sizeof(hm_change_row), hb->n_deps * sizeof(hm_dep_row),
                              n * sizeof(hm_doc_result), n * S * 4, (size_t)hb->n_changes * 4, n * S * 4};
        const void *src[6] = {hb->docs, hb->changes, hb->deps, hr->docs, hr->clock, hr->hist};
        size_t off[7], total = 0;
        for (int i = 0; i < 7; i++) { off[i] = total; total += al(sz[i] ? sz[i] : 1); }
        char *base = nullptr;
        if (hipMalloc((void **)&base, total) != hipSuccess) return fail(e, HM_ERR_NOMEM, "hipMalloc missing-deps staging");
        hipStream_t s = e->stream;
        hm_batch b = *hb;
        b.docs = (const hm_doc_row *)(base + off[0]); b.changes = (const hm_change_row *)(base + off[1]);
        b.deps = (const hm_dep_row *)(base + off[2]);
        hm_results d = {};
        d.docs = (hm_doc_result *)(base + off[3]); d.clock = (uint32_t *)(base + off[4]); d.hist = (int32_t *)(base + off[5]);
        hipError_t r = hipSuccess;
        for (int i = 0; i < 6 && r == hipSuccess; i++)
            if (sz[i]) r = hipMemcpyAsync(base + off[i], src[i], sz[i], hipMemcpyHostToDevice, s);
        if (r == hipSuccess) r = launch_waiting_batch(&b, &d, (uint32_t *)(base + off[6]), s);
        if (r == hipSuccess) r = hipMemcpyAsync(out_missing, base + off[6], sz[6], hipMemcpyDeviceToHost, s);
        if (r == hipSuccess) r = hipStreamSynchronize(s);
        (void)hipFree(base);
        return r == hipSuccess ? HM_OK : hip_fail(e, r, "hm_missing_deps_host");
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_missing_deps_host");
    }
}

static ChangesArgs changes_batch_args(const hm_batch *b, const hm_results *r, const uint32_t *entry_off,
                                      const uint16_t *entry_actor, const uint32_t *entry_seq, uint32_t n_entries,
                                      uint32_t flags, uint32_t *out_closure, uint32_t *out_range, uint32_t *out_log,
                                      uint32_t cap, uint32_t *total, uint32_t *bad) {
    ChangesArgs A = {};
    A.n = b->n_docs; A.src = batch_source(b, r);
    A.entry_off = entry_off; A.entry_actor = entry_actor; A.entry_seq = entry_seq; A.n_entries = n_entries; A.flags = flags;
    A.out_closure = out_closure; A.out_range = out_range; A.out_log = out_log; A.cap = cap; A.total = total; A.bad = bad;
    return A;
}

int hm_missing_changes_device(hm_engine *e, const hm_batch *b, const hm_results *r, const uint32_t *entry_off,
                              const uint16_t *entry_actor, const uint32_t *entry_seq, uint32_t n_entries, uint32_t flags,
                              uint32_t *out_closure, uint32_t *out_range, uint32_t *out_log_index, uint32_t cap,
                              uint32_t *out_total, uint32_t *out_bad, void *stream) {
    try {
        if (!e || !r) return HM_ERR_INVALID;
        int st = check_waiting_batch(e, b);
        if (st) return st;
        if (!b->n_docs) return HM_OK;
        if (flags & ~(HM_MC_RAW | HM_MC_ONLY_LISTED)) return fail(e, HM_ERR_INVALID, "unknown HM_MC_* flag");
        if (!entry_off || !out_range || !out_total || !out_bad || (cap && !out_log_index) || (n_entries && (!entry_actor || !entry_seq)))
            return fail(e, HM_ERR_INVALID, "hm_missing_changes: entry table or output missing");
        if (!r->docs || (b->n_changes && (!r->hist || !r->all_deps)))
            return fail(e, HM_ERR_INVALID, "hm_missing_changes needs the results' docs, hist and all_deps tables");
        HIPCHK(e, hipSetDevice(e->device));
        const ChangesArgs A = changes_batch_args(b, r, entry_off, entry_actor, entry_seq, n_entries, flags, out_closure, out_range,
                                                 out_log_index, cap, out_total, out_bad);
        hipError_t hr = hm_launch_missing_changes(A, stream ? (hipStream_t)stream : e->stream);
        return hr == hipSuccess ? HM_OK : hip_fail(e, hr, "changes_kernel launch");
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_missing_changes_device");
    }
}

size_t hm_materialize_work_bytes(uint32_t n) {
    // [counts 4n][offsets 4n][objects and flags 2n] u32, then the scan's per-chunk words
    return ((((size_t)n * 40) + 255) & ~(size_t)255) + (size_t)hm_past_scan_chunks(n) * HM_PAST_PART * 8;
}

int hm_materialize_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                          const uint32_t *hist_len, const uint32_t *clock_rows, const hm_past_out *out,
                          hm_past_summary *out_summary, void *work, void *stream) {
    try {
        if (!e || !r || !out || !out_summary) return HM_ERR_INVALID;
        int st = check_batch(e, b);
        if (st) return st;
        if ((hist_len != nullptr) == (clock_rows != nullptr))
            return fail(e, HM_ERR_INVALID, "hm_materialize: exactly one of hist_len and clock_rows");
        if (n && (!work || !out->docs)) return fail(e, HM_ERR_INVALID, "hm_materialize: work or out->docs missing");
        if (((uintptr_t)work | (uintptr_t)out->ops) & 15u)     // (the counts and the op rows move as 16-byte words)
            return fail(e, HM_ERR_INVALID, "hm_materialize: work and out->ops must be 16-byte aligned");
        if ((out->cap_changes && (!out->changes || !out->change_log)) || (out->cap_deps && !out->deps) ||
            (out->cap_ops && (!out->ops || !out->op_log)))
            return fail(e, HM_ERR_INVALID, "hm_materialize: an output table with a capacity is missing");
        if (!r->docs || (b->n_changes && !r->hist)) return fail(e, HM_ERR_INVALID, "hm_materialize needs the results' docs and hist tables");
        HIPCHK(e, hipSetDevice(e->device));
        hipStream_t s = stream ? (hipStream_t)stream : e->stream;
        PastArgs A = {};
        A.n = n; A.src = batch_source(b, r); A.src.handles = doc_index;
        A.hist_len = hist_len; A.clock_rows = clock_rows;
        A.cnt = (uint32_t *)work; A.off = A.cnt + 4 * (size_t)n; A.aux = A.off + 4 * (size_t)n;
        A.part = (unsigned long long *)((char *)work + ((((size_t)n * 40) + 255) & ~(size_t)255));
        A.sum = out_summary;
        A.cap[0] = out->cap_changes; A.cap[1] = out->cap_deps; A.cap[2] = out->cap_ops; A.cap[3] = out->cap_regs;
        A.out_docs = out->docs; A.out_changes = out->changes; A.out_deps = out->deps; A.out_ops = out->ops;
        A.out_change_log = out->change_log; A.out_op_log = out->op_log;
        hipError_t hr = hm_launch_past_count(A, s);
        if (hr == hipSuccess) hr = hm_launch_past_fill(A, s);
        return hr == hipSuccess ? HM_OK : hip_fail(e, hr, "past kernels launch");
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_materialize_device");
    }
}

// the words of a wave's slice for any document of b: its launch hints, or the batch totals without them
// (HM_ODF_LISTS: by the list formula when a document of b may carry HM_DOC_HAS_LISTS; doc_flags 0 = unknown)
// (at_clock: the clock forms, whose select phase keeps a bit per log change after the other words)
static unsigned long long od_batch_slice(const hm_batch *b, uint32_t opts, bool at_clock = false) {
    const bool hints = b->max_ops || b->max_regs || b->max_objs;
    const bool lists = (opts & HM_ODF_LISTS) && (!b->doc_flags || (b->doc_flags & HM_DOC_HAS_LISTS));
    const unsigned long long ops = hints ? b->max_ops : b->n_ops, regs = hints ? b->max_regs : b->n_regs,
                             objs = hints ? (b->max_objs ? b->max_objs : 1u) : (unsigned long long)b->n_ops + b->n_docs;
    const unsigned long long w = (lists ? hm_od_slice_words_lists(ops, regs, objs) : hm_od_slice_words(ops, regs, objs)) +
                                 (at_clock ? hm_od_slice_words_clock(hints && b->max_changes ? b->max_changes : b->n_changes) : 0ull);
    return w ? w : 1ull;
}
// [counts 4n][offsets 4n][zero and flags 2n] u32, the scan's per-chunk words, then the waves' slices
static size_t od_fixed_bytes(uint32_t n) {
    return ((((size_t)n * 40) + 255) & ~(size_t)255) + ((((size_t)hm_past_scan_chunks(n) * HM_PAST_PART * 8) + 255) & ~(size_t)255);
}

size_t hm_op_diffs_work_bytes(const hm_batch *b, uint32_t n) { return hm_op_diffs_work_bytes_ex(b, n, 0u); }

size_t hm_op_diffs_work_bytes_ex(const hm_batch *b, uint32_t n, uint32_t opts) {
    if (!b || !n || (opts & ~HM_ODF_LISTS)) return 0;         // (HM_ODF_ONCE is the resident store's alone)
    const unsigned long long sw = od_batch_slice(b, opts);
    return od_fixed_bytes(n) + (size_t)hm_od_waves(n, sw) * (size_t)sw * 4;
}

size_t hm_op_diffs_at_work_bytes(const hm_batch *b, uint32_t n, uint32_t opts) {
    if (!b || !n || (opts & ~HM_ODF_LISTS)) return 0;
    const unsigned long long sw = od_batch_slice(b, opts, true);
    return od_fixed_bytes(n) + (size_t)hm_od_waves(n, sw) * (size_t)sw * 4;
}

static int op_diffs_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                           const uint32_t *from, const uint32_t *to, const uint32_t *clock_rows, const hm_op_diff_out *out,
                           uint32_t *out_index, hm_op_diff_summary *out_summary, void *work, void *stream, uint32_t opts);
static int op_diffs_host(hm_engine *e, const hm_batch *hb, const hm_results *hr, uint32_t n, const uint32_t *doc_index,
                         const uint32_t *from, const uint32_t *to, const uint32_t *clock_rows, const hm_op_diff_out *out,
                         uint32_t *out_index, uint64_t *out_totals, uint32_t opts);

int hm_op_diffs_at_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                          const uint32_t *clock_rows, const hm_op_diff_out *out, uint32_t *out_index,
                          hm_op_diff_summary *out_summary, void *work, void *stream, uint32_t opts) {
    if (n && !clock_rows) return HM_ERR_INVALID;
    return op_diffs_device(e, b, r, n, doc_index, nullptr, nullptr, clock_rows, out, out_index, out_summary, work, stream, opts);
}

int hm_op_diffs_at_host(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                        const uint32_t *clock_rows, const hm_op_diff_out *out, uint32_t *out_index,
                        uint64_t *out_totals, uint32_t opts) {
    if (n && !clock_rows) return HM_ERR_INVALID;
    return op_diffs_host(e, b, r, n, doc_index, nullptr, nullptr, clock_rows, out, out_index, out_totals, opts);
}

int hm_op_diffs_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                       const uint32_t *from, const uint32_t *to, const hm_op_diff_out *out,
                       hm_op_diff_summary *out_summary, void *work, void *stream) {
    return hm_op_diffs_device_ex(e, b, r, n, doc_index, from, to, out, nullptr, out_summary, work, stream, 0u);
}

int hm_op_diffs_device_ex(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                          const uint32_t *from, const uint32_t *to, const hm_op_diff_out *out, uint32_t *out_index,
                          hm_op_diff_summary *out_summary, void *work, void *stream, uint32_t opts) {
    if (n && (!from || !to)) return e ? fail(e, HM_ERR_INVALID, "hm_op_diffs: work, a range array or a per-request output missing") : HM_ERR_INVALID;
    return op_diffs_device(e, b, r, n, doc_index, from, to, nullptr, out, out_index, out_summary, work, stream, opts);
}

// hm_op_diffs_device_ex (clock_rows NULL) and hm_op_diffs_at_device (from / to NULL)
static int op_diffs_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                           const uint32_t *from, const uint32_t *to, const uint32_t *clock_rows, const hm_op_diff_out *out,
                           uint32_t *out_index, hm_op_diff_summary *out_summary, void *work, void *stream, uint32_t opts) {
    try {
        if (!e || !r || !out || !out_summary || (opts & ~HM_ODF_LISTS)) return HM_ERR_INVALID;
        int st = check_batch(e, b);
        if (st) return st;
        if (n && (!work || !out->range || !out->flags))
            return fail(e, HM_ERR_INVALID, "hm_op_diffs: work, a range array or a per-request output missing");
        if (((uintptr_t)work | (uintptr_t)b->ops) & 15u)       // (the counts and the op rows are read as 16-byte words)
            return fail(e, HM_ERR_INVALID, "hm_op_diffs: work and b->ops must be 16-byte aligned");
        if ((out->cap_rows && !out->rows) || (out->cap_surv && !out->surv) || ((opts & HM_ODF_LISTS) && out->cap_rows && !out_index))
            return fail(e, HM_ERR_INVALID, "hm_op_diffs: an output table with a capacity is missing");
        if (!r->docs || (b->n_changes && (!r->hist || !r->all_deps)))
            return fail(e, HM_ERR_INVALID, "hm_op_diffs needs the results' docs, hist and all_deps tables");
        HIPCHK(e, hipSetDevice(e->device));
        hipStream_t s = stream ? (hipStream_t)stream : e->stream;
        OpDiffArgs A = {};
        A.n = n; A.src = batch_source(b, r); A.src.handles = doc_index;
        A.from = from; A.to = to; A.clock = clock_rows;
        A.cnt = (uint32_t *)work; A.off = A.cnt + 4 * (size_t)n; A.aux = A.off + 4 * (size_t)n;
        A.part = (unsigned long long *)((char *)work + ((((size_t)n * 40) + 255) & ~(size_t)255));
        A.sum = out_summary;
        A.opts = opts; A.out_index = (opts & HM_ODF_LISTS) ? out_index : nullptr;
        A.slice_words = od_batch_slice(b, opts, clock_rows != nullptr); A.waves = hm_od_waves(n, A.slice_words);
        A.work = (uint32_t *)((char *)work + od_fixed_bytes(n));
        A.cap_rows = out->cap_rows; A.cap_surv = out->cap_surv;
        A.out_rows = out->rows; A.out_surv = out->surv; A.out_range = out->range; A.out_flags = out->flags;
        hipError_t hr = hm_launch_op_diff_count(A, s);
        if (hr == hipSuccess) hr = hm_launch_op_diff_fill(A, s);
        return hr == hipSuccess ? HM_OK : hip_fail(e, hr, "op-diff kernels launch");
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_op_diffs_device");
    }
}

int hm_op_diffs_host(hm_engine *e, const hm_batch *hb, const hm_results *hr, uint32_t n, const uint32_t *doc_index,
                     const uint32_t *from, const uint32_t *to, const hm_op_diff_out *out, uint64_t *out_totals) {
    return hm_op_diffs_host_ex(e, hb, hr, n, doc_index, from, to, out, nullptr, out_totals, 0u);
}

int hm_op_diffs_host_ex(hm_engine *e, const hm_batch *hb, const hm_results *hr, uint32_t n, const uint32_t *doc_index,
                        const uint32_t *from, const uint32_t *to, const hm_op_diff_out *out, uint32_t *out_index,
                        uint64_t *out_totals, uint32_t opts) {
    if (n && (!from || !to)) return e ? fail(e, HM_ERR_INVALID, "hm_op_diffs: a range array or an output missing") : HM_ERR_INVALID;
    return op_diffs_host(e, hb, hr, n, doc_index, from, to, nullptr, out, out_index, out_totals, opts);
}

// hm_op_diffs_host_ex (clock_rows NULL) and hm_op_diffs_at_host (from / to NULL)
static int op_diffs_host(hm_engine *e, const hm_batch *hb, const hm_results *hr, uint32_t n, const uint32_t *doc_index,
                         const uint32_t *from, const uint32_t *to, const uint32_t *clock_rows, const hm_op_diff_out *out,
                         uint32_t *out_index, uint64_t *out_totals, uint32_t opts) {
    try {
        if (!e || !hr || !out || (opts & ~HM_ODF_LISTS)) return HM_ERR_INVALID;
        const bool want_index = (opts & HM_ODF_LISTS) != 0u;
        int st = check_batch(e, hb);
        if (st) return st;
        if (out_totals) out_totals[0] = out_totals[1] = 0;
        if (!n) return HM_OK;
        if (!out->range || !out->flags || (out->cap_rows && !out->rows) || (out->cap_surv && !out->surv) ||
            (want_index && out->cap_rows && !out_index))
            return fail(e, HM_ERR_INVALID, "hm_op_diffs: a range array or an output missing");
        if (!hr->docs || (hb->n_changes && (!hr->hist || !hr->all_deps)))
            return fail(e, HM_ERR_INVALID, "hm_op_diffs needs the results' docs, hist and all_deps tables");
        if (doc_index)
            for (uint32_t i = 0; i < n; i++)
                if (doc_index[i] >= hb->n_docs) return fail(e, HM_ERR_INVALID, "hm_op_diffs: a document outside the batch");
        if (!doc_index && n > hb->n_docs) return fail(e, HM_ERR_INVALID, "hm_op_diffs: a document outside the batch");
        HIPCHK(e, hipSetDevice(e->device));
        const size_t S = hb->a_stride, nd = hb->n_docs;
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        // inputs 0..8, then the summary, the work memory, the four outputs and the index table
        const size_t sz[16] = {nd * sizeof(hm_doc_row), hb->n_changes * sizeof(hm_change_row), hb->n_ops * sizeof(hm_op_row),
                               nd * sizeof(hm_doc_result), (size_t)hb->n_changes * 4, (size_t)hb->n_changes * S * 4,
                               doc_index ? (size_t)n * 4 : 0, clock_rows ? (size_t)n * S * 4 : (size_t)n * 4, clock_rows ? 0 : (size_t)n * 4,
                               sizeof(hm_op_diff_summary), clock_rows ? hm_op_diffs_at_work_bytes(hb, n, opts) : hm_op_diffs_work_bytes_ex(hb, n, opts),
                               (size_t)out->cap_rows * sizeof(hm_op_diff), (size_t)out->cap_surv * sizeof(hm_surv_result),
                               (size_t)n * 8, (size_t)n * 4, want_index ? (size_t)out->cap_rows * 4 : 0};
        const void *src[9] = {hb->docs, hb->changes, hb->ops, hr->docs, hr->hist, hr->all_deps, doc_index, clock_rows ? clock_rows : from, to};
        size_t off[16], total = 0;
        for (int i = 0; i < 16; i++) { off[i] = total; total += al(sz[i] ? sz[i] : 1); }
        char *base = nullptr;
        if (hipMalloc((void **)&base, total) != hipSuccess) return fail(e, HM_ERR_NOMEM, "hipMalloc op-diff staging");
        hipStream_t s = e->stream;
        hm_batch b = *hb;
        b.docs = (const hm_doc_row *)(base + off[0]); b.changes = (const hm_change_row *)(base + off[1]);
        b.deps = nullptr; b.n_deps = 0; b.ops = (const hm_op_row *)(base + off[2]);
        hm_results d = {};
        d.docs = (hm_doc_result *)(base + off[3]); d.hist = (int32_t *)(base + off[4]); d.all_deps = (uint32_t *)(base + off[5]);
        hm_op_diff_out o = *out;
        o.rows = (hm_op_diff *)(base + off[11]); o.surv = (hm_surv_result *)(base + off[12]);
        o.range = (uint32_t *)(base + off[13]); o.flags = (uint32_t *)(base + off[14]);
        hm_op_diff_summary sum;
        memset(&sum, 0, sizeof sum);
        hipError_t rr = hipSuccess;
        for (int i = 0; i < 9 && rr == hipSuccess; i++)
            if (sz[i]) rr = hipMemcpyAsync(base + off[i], src[i], sz[i], hipMemcpyHostToDevice, s);
        int rc = HM_OK;
        if (rr == hipSuccess)
            rc = op_diffs_device(e, &b, &d, n, doc_index ? (const uint32_t *)(base + off[6]) : nullptr,
                                 clock_rows ? nullptr : (const uint32_t *)(base + off[7]), clock_rows ? nullptr : (const uint32_t *)(base + off[8]),
                                 clock_rows ? (const uint32_t *)(base + off[7]) : nullptr, &o,
                                       (uint32_t *)(base + off[15]), (hm_op_diff_summary *)(base + off[9]), base + off[10], s, opts);
        if (rc == HM_OK && rr == hipSuccess) rr = hipMemcpyAsync(&sum, base + off[9], sizeof sum, hipMemcpyDeviceToHost, s);
        if (rc == HM_OK && rr == hipSuccess) rr = hipStreamSynchronize(s);
        const bool fits = sum.totals[0] <= out->cap_rows && sum.totals[1] <= out->cap_surv;
        if (rc == HM_OK && rr == hipSuccess && !sum.bad && fits) {
            if (sum.totals[0]) rr = hipMemcpy(out->rows, o.rows, (size_t)sum.totals[0] * sizeof(hm_op_diff), hipMemcpyDeviceToHost);
            if (rr == hipSuccess && sum.totals[1]) rr = hipMemcpy(out->surv, o.surv, (size_t)sum.totals[1] * sizeof(hm_surv_result), hipMemcpyDeviceToHost);
            if (rr == hipSuccess) rr = hipMemcpy(out->range, o.range, sz[13], hipMemcpyDeviceToHost);
            if (rr == hipSuccess) rr = hipMemcpy(out->flags, o.flags, sz[14], hipMemcpyDeviceToHost);
            if (rr == hipSuccess && want_index && sum.totals[0])
                rr = hipMemcpy(out_index, base + off[15], (size_t)sum.totals[0] * 4, hipMemcpyDeviceToHost);
        }
        (void)hipFree(base);
        if (rc != HM_OK) return rc;
        if (rr != hipSuccess) return hip_fail(e, rr, "hm_op_diffs_host");
        if (sum.bad & HM_OD_BAD_HANDLE) return fail(e, HM_ERR_INVALID, "hm_op_diffs: a document outside the batch");
        if (sum.bad & HM_OD_BAD_ROWS) return fail(e, HM_ERR_INVALID, "a change row outside its document's segments");
        if (sum.bad) return fail(e, HM_ERR_NOMEM, "a document outgrows the op-diff work memory");
        if (out_totals) { out_totals[0] = sum.totals[0]; out_totals[1] = sum.totals[1]; }
        if (!fits) return fail(e, HM_ERR_NOMEM, "a capacity below the rows of the op diffs");
        return HM_OK;
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_op_diffs_host");
    }
}

// (the state calls read the document table and the results alone: no change, dep or op table is asked for)
static int check_state_batch(hm_engine *e, const hm_batch *b, const hm_results *r, bool clock, bool heads) {
    if (!b || b->a_stride == 0 || b->a_stride > HM_MAX_STRIDE) return fail(e, HM_ERR_INVALID, "a_stride must be in [1,256]");
    if (b->n_docs && !b->docs) return fail(e, HM_ERR_INVALID, "docs table missing");
    if ((b->n_docs && !r->docs) || (b->n_regs && !r->regs) || (b->n_ops && !r->surv) || (clock && !r->clock) || (heads && !r->heads))
        return fail(e, HM_ERR_INVALID, "hm_state needs the results' docs, regs and surv tables (and clock / heads when asked for)");
    return HM_OK;
}

size_t hm_state_work_bytes(uint32_t n) {
    // [counts 4n][offsets 4n][zero and flags 2n] u32, then the scan's per-chunk words
    return ((((size_t)n * 40) + 255) & ~(size_t)255) + (size_t)hm_past_scan_chunks(n) * HM_PAST_PART * 8;
}

int hm_state_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                    const hm_state_out *out, uint32_t *out_clock, uint32_t *out_heads, hm_state_summary *out_summary,
                    void *work, void *stream) {
    try {
        if (!e || !r || !out || !out_summary) return HM_ERR_INVALID;
        int st = check_state_batch(e, b, r, out_clock != nullptr, out_heads != nullptr);
        if (st) return st;
        if (n && (!work || !out->range || !out->flags))
            return fail(e, HM_ERR_INVALID, "hm_state: work, the range array or the flags missing");
        if (((uintptr_t)work | (uintptr_t)r->regs | (uintptr_t)r->surv | (uintptr_t)out->surv | (uintptr_t)out->range) & 15u)
            return fail(e, HM_ERR_INVALID, "hm_state: work, the register and survivor tables and out->range must be 16-byte aligned");
        if ((out->cap_rows && !out->rows) || (out->cap_surv && !out->surv))
            return fail(e, HM_ERR_INVALID, "hm_state: an output table with a capacity is missing");
        HIPCHK(e, hipSetDevice(e->device));
        hipStream_t s = stream ? (hipStream_t)stream : e->stream;
        StateArgs A = {};
        A.n = n;
        A.src.docs = b->docs; A.src.res = r->docs; A.src.n_docs = b->n_docs; A.src.S = b->a_stride; A.src.handles = doc_index;
        A.src.clock = r->clock;
        A.regs = r->regs; A.surv = r->surv; A.lim_r = b->n_regs; A.lim_s = b->n_ops; A.heads = r->heads;
        A.cnt = (uint32_t *)work; A.off = A.cnt + 4 * (size_t)n; A.aux = A.off + 4 * (size_t)n;
        A.part = (unsigned long long *)((char *)work + ((((size_t)n * 40) + 255) & ~(size_t)255));
        A.sum = out_summary;
        A.cap_rows = out->cap_rows; A.cap_surv = out->cap_surv;
        A.out_rows = out->rows; A.out_surv = out->surv; A.out_range = out->range; A.out_flags = out->flags;
        A.out_clock = out_clock; A.out_heads = out_heads;
        hipError_t hr = hm_launch_state_count(A, s);
        if (hr == hipSuccess) hr = hm_launch_state_fill(A, s);
        return hr == hipSuccess ? HM_OK : hip_fail(e, hr, "state kernels launch");
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_state_device");
    }
}

int hm_state_host(hm_engine *e, const hm_batch *hb, const hm_results *hr, uint32_t n, const uint32_t *doc_index,
                  const hm_state_out *out, uint32_t *out_clock, uint32_t *out_heads, uint64_t *out_totals) {
    try {
        if (!e || !hr || !out) return HM_ERR_INVALID;
        int st = check_state_batch(e, hb, hr, out_clock != nullptr, out_heads != nullptr);
        if (st) return st;
        if (out_totals) out_totals[0] = out_totals[1] = 0;
        if (!n) return HM_OK;
        if (!out->range || !out->flags || (out->cap_rows && !out->rows) || (out->cap_surv && !out->surv))
            return fail(e, HM_ERR_INVALID, "hm_state: the range array, the flags or an output table missing");
        if (doc_index)
            for (uint32_t i = 0; i < n; i++)
                if (doc_index[i] >= hb->n_docs) return fail(e, HM_ERR_INVALID, "hm_state: a document outside the batch");
        if (!doc_index && n > hb->n_docs) return fail(e, HM_ERR_INVALID, "hm_state: a document outside the batch");
        HIPCHK(e, hipSetDevice(e->device));
        const size_t S = hb->a_stride, nd = hb->n_docs;
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        // inputs 0..6, then the summary, the work memory and the six outputs
        const size_t sz[15] = {nd * sizeof(hm_doc_row), nd * sizeof(hm_doc_result), hb->n_regs * sizeof(hm_reg_result),
                               hb->n_ops * sizeof(hm_surv_result), out_clock ? nd * S * 4 : 0, out_heads ? nd * S * 4 : 0,
                               doc_index ? (size_t)n * 4 : 0, sizeof(hm_state_summary), hm_state_work_bytes(n),
                               (size_t)out->cap_rows * sizeof(hm_state_row), (size_t)out->cap_surv * sizeof(hm_surv_result),
                               (size_t)n * 16, (size_t)n * 4, out_clock ? (size_t)n * S * 4 : 0, out_heads ? (size_t)n * S * 4 : 0};
        const void *src[7] = {hb->docs, hr->docs, hr->regs, hr->surv, hr->clock, hr->heads, doc_index};
        size_t off[15], total = 0;
        for (int i = 0; i < 15; i++) { off[i] = total; total += al(sz[i] ? sz[i] : 1); }
        char *base = nullptr;
        if (hipMalloc((void **)&base, total) != hipSuccess) return fail(e, HM_ERR_NOMEM, "hipMalloc state staging");
        hipStream_t s = e->stream;
        hm_batch b = *hb;
        b.docs = (const hm_doc_row *)(base + off[0]);
        b.changes = nullptr; b.deps = nullptr; b.ops = nullptr; b.min_clock = nullptr;
        hm_results d = {};
        d.docs = (hm_doc_result *)(base + off[1]); d.regs = (hm_reg_result *)(base + off[2]); d.surv = (hm_surv_result *)(base + off[3]);
        d.clock = (uint32_t *)(base + off[4]); d.heads = (uint32_t *)(base + off[5]);
        hm_state_out o = *out;
        o.rows = (hm_state_row *)(base + off[9]); o.surv = (hm_surv_result *)(base + off[10]);
        o.range = (uint32_t *)(base + off[11]); o.flags = (uint32_t *)(base + off[12]);
        hm_state_summary sum;
        memset(&sum, 0, sizeof sum);
        hipError_t rr = hipSuccess;
        for (int i = 0; i < 7 && rr == hipSuccess; i++)
            if (sz[i]) rr = hipMemcpyAsync(base + off[i], src[i], sz[i], hipMemcpyHostToDevice, s);
        int rc = HM_OK;
        if (rr == hipSuccess)
            rc = hm_state_device(e, &b, &d, n, doc_index ? (const uint32_t *)(base + off[6]) : nullptr, &o,
                                 out_clock ? (uint32_t *)(base + off[13]) : nullptr, out_heads ? (uint32_t *)(base + off[14]) : nullptr,
                                 (hm_state_summary *)(base + off[7]), base + off[8], s);
        if (rc == HM_OK && rr == hipSuccess) rr = hipMemcpyAsync(&sum, base + off[7], sizeof sum, hipMemcpyDeviceToHost, s);
        if (rc == HM_OK && rr == hipSuccess) rr = hipStreamSynchronize(s);
        const bool fits = sum.totals[0] <= out->cap_rows && sum.totals[1] <= out->cap_surv;
        if (rc == HM_OK && rr == hipSuccess && !sum.bad && fits) {
            if (sum.totals[0]) rr = hipMemcpy(out->rows, o.rows, (size_t)sum.totals[0] * sizeof(hm_state_row), hipMemcpyDeviceToHost);
            if (rr == hipSuccess && sum.totals[1]) rr = hipMemcpy(out->surv, o.surv, (size_t)sum.totals[1] * sizeof(hm_surv_result), hipMemcpyDeviceToHost);
            if (rr == hipSuccess) rr = hipMemcpy(out->range, o.range, sz[11], hipMemcpyDeviceToHost);
            if (rr == hipSuccess) rr = hipMemcpy(out->flags, o.flags, sz[12], hipMemcpyDeviceToHost);
            if (rr == hipSuccess && out_clock) rr = hipMemcpy(out_clock, base + off[13], sz[13], hipMemcpyDeviceToHost);
            if (rr == hipSuccess && out_heads) rr = hipMemcpy(out_heads, base + off[14], sz[14], hipMemcpyDeviceToHost);
        }
        (void)hipFree(base);
        if (rc != HM_OK) return rc;
        if (rr != hipSuccess) return hip_fail(e, rr, "hm_state_host");
        if (sum.bad & HM_ST_BAD_HANDLE) return fail(e, HM_ERR_INVALID, "hm_state: a document outside the batch");
        if (out_totals) { out_totals[0] = sum.totals[0]; out_totals[1] = sum.totals[1]; }
        if (!fits) return fail(e, HM_ERR_NOMEM, "a capacity below the rows of the state");
        return HM_OK;
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_state_host");
    }
}

int hm_missing_changes_host(hm_engine *e, const hm_batch *hb, const hm_results *hr, const uint32_t *entry_off,
                            const uint16_t *entry_actor, const uint32_t *entry_seq, uint32_t flags, uint32_t *out_closure,
                            uint32_t *out_range, uint32_t *out_log_index, uint32_t cap, uint32_t *out_total) {
    try {
        if (!e || !hr || !out_total) return HM_ERR_INVALID;
        int st = check_waiting_batch(e, hb);
        if (st) return st;
        *out_total = 0;
        if (!hb->n_docs) return HM_OK;
        if (flags & ~(HM_MC_RAW | HM_MC_ONLY_LISTED)) return fail(e, HM_ERR_INVALID, "unknown HM_MC_* flag");
        if (!entry_off || !out_range || (cap && !out_log_index))
            return fail(e, HM_ERR_INVALID, "hm_missing_changes: entry table or output missing");
        if (!hr->docs || (hb->n_changes && (!hr->hist || !hr->all_deps)))
            return fail(e, HM_ERR_INVALID, "hm_missing_changes needs the results' docs, hist and all_deps tables");
        const size_t S = hb->a_stride, n = hb->n_docs;
        if (entry_off[0]) return fail(e, HM_ERR_INVALID, "entry_off must start at 0");
        for (size_t i = 0; i < n; i++)
            if (entry_off[i + 1] < entry_off[i]) return fail(e, HM_ERR_INVALID, "entry_off must not decrease");
        const size_t ne = entry_off[n];
        if (ne && (!entry_actor || !entry_seq)) return fail(e, HM_ERR_INVALID, "hm_missing_changes: entry table or output missing");
        HIPCHK(e, hipSetDevice(e->device));
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        // inputs 0..7, then counters (total, bad), ranges, closure rows, log indices
        const size_t sz[12] = {n * sizeof(hm_doc_row), hb->n_changes * sizeof(hm_change_row), n * sizeof(hm_doc_result),
                               (size_t)hb->n_changes * 4, (size_t)hb->n_changes * S * 4, (n + 1) * 4, ne * 2, ne * 4,
                               8, n * 8, out_closure ? n * S * 4 : 0, (size_t)cap * 4};
        const void *src[8] = {hb->docs, hb->changes, hr->docs, hr->hist, hr->all_deps, entry_off, entry_actor, entry_seq};
        size_t off[12], total = 0;
        for (int i = 0; i < 12; i++) { off[i] = total; total += al(sz[i] ? sz[i] : 1); }
        char *base = nullptr;
        if (hipMalloc((void **)&base, total) != hipSuccess) return fail(e, HM_ERR_NOMEM, "hipMalloc missing-changes staging");
        hipStream_t s = e->stream;
        hm_batch b = *hb;
        b.docs = (const hm_doc_row *)(base + off[0]); b.changes = (const hm_change_row *)(base + off[1]);
        hm_results d = {};
        d.docs = (hm_doc_result *)(base + off[2]); d.hist = (int32_t *)(base + off[3]); d.all_deps = (uint32_t *)(base + off[4]);
        uint32_t cnt[2] = {0, 0};
        hipError_t r = hipMemsetAsync(base + off[8], 0, 8, s);
        for (int i = 0; i < 8 && r == hipSuccess; i++)
            if (sz[i]) r = hipMemcpyAsync(base + off[i], src[i], sz[i], hipMemcpyHostToDevice, s);
        if (r == hipSuccess) {
            const ChangesArgs A = changes_batch_args(&b, &d, (const uint32_t *)(base + off[5]), (const uint16_t *)(base + off[6]),
                                                     (const uint32_t *)(base + off[7]), (uint32_t)ne, flags,
                                                     out_closure ? (uint32_t *)(base + off[10]) : nullptr, (uint32_t *)(base + off[9]),
                                                     (uint32_t *)(base + off[11]), cap, (uint32_t *)(base + off[8]),
                                                     (uint32_t *)(base + off[8] + 4));
            r = hm_launch_missing_changes(A, s);
        }
        if (r == hipSuccess) r = hipMemcpyAsync(cnt, base + off[8], 8, hipMemcpyDeviceToHost, s);
        if (r == hipSuccess) r = hipMemcpyAsync(out_range, base + off[9], sz[9], hipMemcpyDeviceToHost, s);
        if (r == hipSuccess && out_closure) r = hipMemcpyAsync(out_closure, base + off[10], sz[10], hipMemcpyDeviceToHost, s);
        if (r == hipSuccess) r = hipStreamSynchronize(s);
        if (r == hipSuccess && !cnt[1] && cnt[0] && cnt[0] <= cap)
            r = hipMemcpy(out_log_index, base + off[11], (size_t)cnt[0] * 4, hipMemcpyDeviceToHost);
        (void)hipFree(base);
        if (r != hipSuccess) return hip_fail(e, r, "hm_missing_changes_host");
        if (cnt[1] & HM_MC_BAD_RANK) return fail(e, HM_ERR_INVALID, "entry actor rank outside a_stride");
        if (cnt[1] & HM_MC_BAD_REPEAT) return fail(e, HM_ERR_INVALID, "actor rank repeated within a request");
        if (cnt[1]) return fail(e, HM_ERR_INVALID, "bad entry_off");
        *out_total = cnt[0];
        if (cnt[0] > cap) return fail(e, HM_ERR_NOMEM, "cap below the rows of the missing changes");
        return HM_OK;
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_missing_changes_host");
    }
}

static int check_fields_tables(hm_engine *e, const hm_batch *b, const hm_results *r) {
    if (b->n_ops && !b->ops) return fail(e, HM_ERR_INVALID, "row table missing");
    if (!r->docs || !r->clock || (b->n_changes && (!r->hist || !r->all_deps)) || (b->n_regs && !r->regs) || (b->n_ops && !r->surv))
        return fail(e, HM_ERR_INVALID, "hm_fields needs the results' docs, clock, hist, all_deps, regs and surv tables");
    return HM_OK;
}

int hm_fields_device(hm_engine *e, const hm_batch *b, const hm_results *r, const uint32_t *entry_off,
                     const uint16_t *entry_actor, const uint32_t *entry_seq, uint32_t n_entries,
                     const uint32_t *field_off, const uint32_t *field_reg, uint32_t n_fields,
                     uint32_t *out_flags, uint32_t *out_closure, uint32_t *out_range, hm_field_op *out_rows,
                     uint32_t cap, uint32_t *out_total, uint32_t *out_bad, void *stream) {
    try {
        if (!e || !r) return HM_ERR_INVALID;
        int st = check_waiting_batch(e, b);
        if (st) return st;
        if (!b->n_docs) return HM_OK;
        if (!entry_off || !field_off || !out_flags || !out_total || !out_bad || (cap && !out_rows) ||
            (n_entries && (!entry_actor || !entry_seq)) || (n_fields && (!field_reg || !out_range)))
            return fail(e, HM_ERR_INVALID, "hm_fields: a request table or an output missing");
        if ((st = check_fields_tables(e, b, r))) return st;
        HIPCHK(e, hipSetDevice(e->device));
        FieldArgs A = {};
        A.n = b->n_docs; A.src = batch_source(b, r);
        A.regs = r->regs; A.surv = r->surv; A.lim_r = b->n_regs;
        A.entry_off = entry_off; A.entry_actor = entry_actor; A.entry_seq = entry_seq; A.n_entries = n_entries;
        A.field_off = field_off; A.field_reg = field_reg; A.n_fields = n_fields;
        A.out_flags = out_flags; A.out_closure = out_closure; A.out_range = out_range; A.out_rows = out_rows; A.cap = cap;
        A.total = out_total; A.bad = out_bad;
        hipError_t hr = hm_launch_fields(A, stream ? (hipStream_t)stream : e->stream);
        return hr == hipSuccess ? HM_OK : hip_fail(e, hr, "fields_kernel launch");
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_fields_device");
    }
}

int hm_fields_host(hm_engine *e, const hm_batch *hb, const hm_results *hr, const uint32_t *entry_off,
                   const uint16_t *entry_actor, const uint32_t *entry_seq, const uint32_t *field_off,
                   const uint32_t *field_reg, uint32_t *out_flags, uint32_t *out_closure, uint32_t *out_range,
                   hm_field_op *out_rows, uint32_t cap, uint32_t *out_total) {
    try {
        if (!e || !hr || !out_total) return HM_ERR_INVALID;
        int st = check_waiting_batch(e, hb);
        if (st) return st;
        *out_total = 0;
        if (!hb->n_docs) return HM_OK;
        if (!entry_off || !field_off || !out_flags || (cap && !out_rows))
            return fail(e, HM_ERR_INVALID, "hm_fields: a request table or an output missing");
        if ((st = check_fields_tables(e, hb, hr))) return st;
        const size_t S = hb->a_stride, n = hb->n_docs;
        if (entry_off[0] || field_off[0]) return fail(e, HM_ERR_INVALID, "entry_off and field_off must start at 0");
        for (size_t i = 0; i < n; i++) {
            if (entry_off[i + 1] < entry_off[i]) return fail(e, HM_ERR_INVALID, "entry_off must not decrease");
            if (field_off[i + 1] < field_off[i]) return fail(e, HM_ERR_INVALID, "field_off must not decrease");
        }
        const size_t ne = entry_off[n], nf = field_off[n];
        if ((ne && (!entry_actor || !entry_seq)) || (nf && (!field_reg || !out_range)))
            return fail(e, HM_ERR_INVALID, "hm_fields: a request table or an output missing");
        HIPCHK(e, hipSetDevice(e->device));
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        // inputs 0..13, then counters (total, bad), flags, ranges, closure rows, rows
        const size_t sz[19] = {n * sizeof(hm_doc_row), hb->n_changes * sizeof(hm_change_row), hb->n_ops * sizeof(hm_op_row),
                               n * sizeof(hm_doc_result), n * S * 4, (size_t)hb->n_changes * 4, (size_t)hb->n_changes * S * 4,
                               hb->n_regs * sizeof(hm_reg_result), hb->n_ops * sizeof(hm_surv_result),
                               (n + 1) * 4, ne * 2, ne * 4, (n + 1) * 4, nf * 4,
                               8, n * 4, nf * 8, out_closure ? n * S * 4 : 0, (size_t)cap * sizeof(hm_field_op)};
        const void *src[14] = {hb->docs, hb->changes, hb->ops, hr->docs, hr->clock, hr->hist, hr->all_deps, hr->regs, hr->surv,
                               entry_off, entry_actor, entry_seq, field_off, field_reg};
        size_t off[19], total = 0;
        for (int i = 0; i < 19; i++) { off[i] = total; total += al(sz[i] ? sz[i] : 1); }
        char *base = nullptr;
        if (hipMalloc((void **)&base, total) != hipSuccess) return fail(e, HM_ERR_NOMEM, "hipMalloc fields staging");
        hipStream_t s = e->stream;
        hm_batch b = *hb;
        b.docs = (const hm_doc_row *)(base + off[0]); b.changes = (const hm_change_row *)(base + off[1]);
        b.deps = nullptr; b.n_deps = 0; b.ops = (const hm_op_row *)(base + off[2]);
        hm_results d = {};
        d.docs = (hm_doc_result *)(base + off[3]); d.clock = (uint32_t *)(base + off[4]); d.hist = (int32_t *)(base + off[5]);
        d.all_deps = (uint32_t *)(base + off[6]); d.regs = (hm_reg_result *)(base + off[7]); d.surv = (hm_surv_result *)(base + off[8]);
        uint32_t cnt[2] = {0, 0};
        hipError_t r = hipMemsetAsync(base + off[14], 0, 8, s);
        for (int i = 0; i < 14 && r == hipSuccess; i++)
            if (sz[i]) r = hipMemcpyAsync(base + off[i], src[i], sz[i], hipMemcpyHostToDevice, s);
        int rc = HM_OK;
        if (r == hipSuccess)
            rc = hm_fields_device(e, &b, &d, (const uint32_t *)(base + off[9]), (const uint16_t *)(base + off[10]),
                                  (const uint32_t *)(base + off[11]), (uint32_t)ne, (const uint32_t *)(base + off[12]),
                                  (const uint32_t *)(base + off[13]), (uint32_t)nf, (uint32_t *)(base + off[15]),
                                  out_closure ? (uint32_t *)(base + off[17]) : nullptr, (uint32_t *)(base + off[16]),
                                  (hm_field_op *)(base + off[18]), cap, (uint32_t *)(base + off[14]),
                                  (uint32_t *)(base + off[14] + 4), s);
        if (rc == HM_OK && r == hipSuccess) r = hipMemcpyAsync(cnt, base + off[14], 8, hipMemcpyDeviceToHost, s);
        if (rc == HM_OK && r == hipSuccess) r = hipStreamSynchronize(s);
        if (rc == HM_OK && r == hipSuccess && !cnt[1]) {
            r = hipMemcpy(out_flags, base + off[15], sz[15], hipMemcpyDeviceToHost);
            if (r == hipSuccess && nf) r = hipMemcpy(out_range, base + off[16], sz[16], hipMemcpyDeviceToHost);
            if (r == hipSuccess && out_closure) r = hipMemcpy(out_closure, base + off[17], sz[17], hipMemcpyDeviceToHost);
            if (r == hipSuccess && cnt[0] && cnt[0] <= cap)
                r = hipMemcpy(out_rows, base + off[18], (size_t)cnt[0] * sizeof(hm_field_op), hipMemcpyDeviceToHost);
        }
        (void)hipFree(base);
        if (rc != HM_OK) return rc;
        if (r != hipSuccess) return hip_fail(e, r, "hm_fields_host");
        if (cnt[1] & HM_FD_BAD_RANK) return fail(e, HM_ERR_INVALID, "entry actor rank outside a_stride");
        if (cnt[1] & HM_FD_BAD_REPEAT) return fail(e, HM_ERR_INVALID, "actor rank repeated within a request");
        if (cnt[1]) return fail(e, HM_ERR_INVALID, "bad entry_off or field_off");
        *out_total = cnt[0];
        if (cnt[0] > cap) return fail(e, HM_ERR_NOMEM, "cap below the rows of the fields");
        return HM_OK;
    } catch (...) {
        return fail(e, HM_ERR_DEVICE, "exception in hm_fields_host");
    }
}

int hm_last_kernel_ms(hm_engine *e, float *ms, int max_kernels) {
    if (!e || !ms) return 0;
    int n = std::min(max_kernels, e->n_last);
    for (int i = 0; i < n; i++) {
        if (hipEventSynchronize(e->ev[2 * i + 1]) != hipSuccess) return 0;
        if (hipEventElapsedTime(&ms[i], e->ev[2 * i], e->ev[2 * i + 1]) != hipSuccess) return 0;
    }
    return n;
}

int hm_last_deferred(hm_engine *e, uint32_t *out_docs, uint32_t cap) {
    if (!e) return -HM_ERR_INVALID;
    if (e->n_last < 2) return 0;
    if (!e->last_scratch) return -fail(e, HM_ERR_INVALID, "the last launch used caller scratch: its deferred list is the caller's");
    if (hipEventSynchronize(e->ev[3]) != hipSuccess) return -HM_ERR_DEVICE;
    uint32_t n = 0;
    if (hipMemcpy(&n, e->last_scratch + 16, 4, hipMemcpyDeviceToHost) != hipSuccess) return -HM_ERR_DEVICE;
    const uint32_t k = std::min(n, cap);
    if (k && out_docs && hipMemcpy(out_docs, e->last_scratch + 256, (size_t)k * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return -HM_ERR_DEVICE;
    return (int)n;
}

int hm_clock_cmp_device(hm_engine *e, const uint32_t *a, const uint32_t *b, uint8_t *out, uint32_t n_docs,
                        uint32_t a_stride, void *stream) {
    if (!e) return HM_ERR_INVALID;
    hipError_t r = hm_launch_clock(0, a, b, out, n_docs, a_stride, stream ? (hipStream_t)stream : e->stream);
    return r == hipSuccess ? HM_OK : hip_fail(e, r, "clock_cmp");
}

int hm_clock_union_device(hm_engine *e, const uint32_t *a, const uint32_t *b, uint32_t *c, uint32_t n_docs,
                          uint32_t a_stride, void *stream) {
    if (!e) return HM_ERR_INVALID;
    hipError_t r = hm_launch_clock(1, a, b, c, n_docs, a_stride, stream ? (hipStream_t)stream : e->stream);
    return r == hipSuccess ? HM_OK : hip_fail(e, r, "clock_union");
}

int hm_clock_intersection_device(hm_engine *e, const uint32_t *a, const uint32_t *b, uint32_t *c,
                                 uint32_t n_docs, uint32_t a_stride, void *stream) {
    if (!e) return HM_ERR_INVALID;
    hipError_t r = hm_launch_clock(2, a, b, c, n_docs, a_stride, stream ? (hipStream_t)stream : e->stream);
    return r == hipSuccess ? HM_OK : hip_fail(e, r, "clock_intersection");
}

}  // extern "C"
