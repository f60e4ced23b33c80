// store.cpp — the resident document store of include/hypermerge_amd.h (hm_store_*,
// hm_doc_*, hm_batch_submit/wait, hm_store_clock_update, hm_sync_ranges_device).
//
// Replaces the per-document Automerge BackendState that DocBackend keeps in
// `this.back` (src/DocBackend.ts:50) for every open document of a repo, plus the
// DocBackend / ClockStore bookkeeping around it.  Layout in HBM:
//
//   change space  changes[]  hist[]  all_deps[][S]      (one segment per document)
//   dep space     deps[]
//   op space      ops[]      surv[]
//   reg space     regs[]
//   per handle    res_docs[] clock[][S] back_clock[][S] heads[][S] min_clock[][S] stored_clock[][S]
//
// A document's segments have power-of-two capacities; an append that overflows one
// moves the document to a fresh segment at the arena's end (append_kernel copies and
// rebases the old rows once).  When an arena is full every document is compacted into
// a new, larger arena and re-merged.  A submit appends the new rows; a document whose new
// changes apply in arrival order on its resident state (nothing queued, map ops) is
// advanced in place by inc_apply_kernel, touching only the registers the new ops hit;
// any other document re-merges its whole log with the batch merge kernels (applyChanges
// is a left fold of addChange, so the state after A then B is the state after A ++ B).
//
// The documents' segments and totals live on the device (DevDoc, 64 B per handle) and a
// submit is planned there: plan_kernel checks every row and routes it, alloc_kernel takes
// the new segments from device bump pointers and writes the append descriptors, the
// rollback of failed documents is a kernel too.  The host moves only the batch tables, a
// few 64-byte plan summaries, and the per-document results.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>
#include "../../include/hypermerge_amd.h"
#include "engine_internal.h"
#include "store_kernels.h"
#include "waiting_kernels.h"
#include "changes_kernels.h"
#include "field_kernels.h"
#include "past_kernels.h"
#include "op_diff_kernels.h"
#include "state_kernels.h"

namespace {

template <typename T>
struct DBuf {                            // device buffer of T with capacity
    T *p = nullptr;
    size_t cap = 0;
};

uint32_t pow2ceil(uint32_t x) {
    uint32_t c = 1;
    while (c < x) c <<= 1;
    return c;
}
// a compacted segment: its rows and a quarter as many again, to a power of two (the plan grows
// segments the same way, store_kernels.hip grow_rows)
uint32_t seg_cap(uint32_t n) {
    const uint64_t x = (uint64_t)n + (n >> 2);
    return pow2ceil((uint32_t)std::max<uint64_t>(std::min<uint64_t>(x, 0x80000000ull), 16));
}

}  // namespace

struct hm_store {
    hm_engine *e = nullptr;
    uint32_t S = 8;
    uint32_t n_handles = 0;
    // arenas (capacity in rows); the bump pointers live in the device PlanStats
    size_t cap_c = 0, cap_d = 0, cap_o = 0, cap_r = 0;
    hm_change_row *changes = nullptr; int32_t *hist = nullptr; uint32_t *all_deps = nullptr; uint32_t *ckey = nullptr;
    hm_dep_row *deps = nullptr;
    hm_op_row *ops = nullptr; hm_surv_result *surv = nullptr; uint2 *smeta = nullptr;
    hm_reg_result *regs = nullptr;
    uint32_t *epos = nullptr, *epar = nullptr, *ekey = nullptr, *lorder = nullptr;   // reg space: resident list order
    // per handle
    size_t cap_h = 0;
    DevDoc *dm = nullptr;                         // segments and totals
    IncState *ist = nullptr;                      // survivor slots / metadata state of the incremental path
    uint2 *ldir = nullptr;                        // list directory (HM_INC_LISTS per handle)
    uint32_t *seen = nullptr;                     // submit stamps (repeated-handle check)
    hm_doc_result *res_docs = nullptr;
    uint32_t *clock = nullptr, *back_clock = nullptr, *heads = nullptr, *min_clock = nullptr, *stored = nullptr;
    // per submit (device): plan rows, descriptors, lists, stats
    DBuf<PlanRow> plan;
    DBuf<AppendDesc> descs, bdescs;
    DBuf<uint32_t> list;                          // re-merge list (cold, then handed back)
    DBuf<uint32_t> blist;                         // rollback list
    DBuf<uint32_t> klist;                         // a re-merge's documents that may keep incremental state
    DBuf<int> mpart;                              // inc_meta_kernel's per-workgroup n_valid changes
    DBuf<uint32_t> alist;                         // append list (batch rows with append work)
    DBuf<uint8_t> remap, inv;
    DBuf<hm_doc_row> rows;
    PlanStats *st = nullptr;
    uint32_t stamp = 0;
    // staging (device)
    DBuf<uint8_t> stage;
    DBuf<uint8_t> past;                           // hm_store_materialize: the gathered batch and its merge
    // the fork batch in flight: its gathered tables in `past` (hm_store_fork_rows reads them until the wait)
    uint64_t fork_id = 0;
    uint32_t fork_n = 0;
    size_t fork_rows[3] = {0, 0, 0}, fork_off[6] = {0, 0, 0, 0, 0, 0};
    // in-flight batch
    std::atomic<bool> pending{false};             // a submitted batch not yet waited for (other threads may read it)
    uint64_t next_id = 1, pending_id = 0;
    uint32_t p_n = 0;                             // batch rows
    uint32_t *p_handles_dev = nullptr;            // batch rows -> handles (staged, or the caller's device array)
    bool p_remap = false;
    uint8_t *p_gather_dev = nullptr;
    uint32_t *p_fail_dev = nullptr;               // rows whose status is not OK (gather_kernel)
    // the last waited batch, for hm_batch_undo (until the next submit)
    uint64_t undo_id = 0;
    uint32_t undo_n = 0;
    DBuf<uint32_t> undo_handles;
    // incremental applyRemoteChanges (inc_apply_kernel) and the last submit's routing
    bool incremental = true;
    // some document holds incremental state a submit can use (PlanStats.n_valid > 0, read back after
    // every re-merge): without one no document can route to the incremental kernels and a submit
    // does not launch them
    bool any_state = false;
    uint32_t inc_mode = 1;                        // 1: small list documents re-merge (cost policy); 2: every one
    uint32_t st_inc = 0, st_cold = 0, st_bail = 0;
    // HIP events around the last submit's incremental kernels and its re-merge (engine stream)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // page-locked host words the submit's small read-backs land in (a pageable destination makes
    // each copy a staged, synchronous one): the plan stats, then the re-merge counts
    PlanStats *h_st = nullptr;
    uint32_t *h_cnt = nullptr;
    bool ev_live = false;                    // ev[] recorded by the pending submit, not read yet
    float last_ms[2] = {0.f, 0.f};
};

namespace {

#define SCHK(s, call)                                                              \
    do {                                                                           \
        hipError_t _r = (call);                                                    \
        if (_r != hipSuccess)                                                      \
            return hm_engine_fail((s)->e, HM_ERR_DEVICE, (std::string(#call) + ": " + hipGetErrorString(_r)).c_str()); \
    } while (0)

template <typename T>
int dev_alloc(hm_store *s, T **p, size_t n) {
    *p = nullptr;
    if (!n) n = 1;
    if (hipMalloc((void **)p, n * sizeof(T)) != hipSuccess) return hm_engine_fail(s->e, HM_ERR_NOMEM, "hipMalloc store arena");
    return HM_OK;
}

// a per-submit device buffer of at least n elements (contents not kept)
template <typename T>
int ensure_buf(hm_store *s, DBuf<T> &b, size_t n) {
    if (n <= b.cap && b.p) return HM_OK;
    SCHK(s, hipStreamSynchronize(hm_engine_stream(s->e)));
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    const size_t cap = std::max<size_t>(n, 1024) * 3 / 2;
    if (hipMalloc((void **)&b.p, cap * sizeof(T)) != hipSuccess) return hm_engine_fail(s->e, HM_ERR_NOMEM, "hipMalloc store buffer");
    b.cap = cap;
    return HM_OK;
}

int ensure_stage(hm_store *s, size_t bytes) { return ensure_buf(s, s->stage, bytes); }

PlanStats read_stats(hm_store *s, int *rc) {
    PlanStats st;
    memset(&st, 0, sizeof st);
    hipStream_t q = hm_engine_stream(s->e);
    if (hipMemcpyAsync(s->h_st, s->st, sizeof st, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        *rc = hm_engine_fail(s->e, HM_ERR_DEVICE, "reading the submit plan");
    else
        st = *s->h_st;
    return st;
}

// zero the per-phase fields of the device stats, keeping the bump pointers
int reset_stats(hm_store *s) {
    SCHK(s, hipMemsetAsync(s->st, 0, offsetof(PlanStats, bump), hm_engine_stream(s->e)));
    return HM_OK;
}

DevDoc read_doc(hm_store *s, uint32_t h, int *rc) {
    DevDoc m;
    memset(&m, 0, sizeof m);
    hipStream_t q = hm_engine_stream(s->e);
    if (hipMemcpyAsync(&m, s->dm + h, sizeof m, hipMemcpyDeviceToHost, q) != hipSuccess || hipStreamSynchronize(q) != hipSuccess)
        *rc = hm_engine_fail(s->e, HM_ERR_DEVICE, "reading a document's meta");
    return m;
}

// grow the per-handle tables to hold `need` documents (contents preserved)
int ensure_handles(hm_store *s, size_t need) {
    if (need <= s->cap_h) return HM_OK;
    const size_t cap = std::max<size_t>(need, std::max<size_t>(1024, s->cap_h * 2));
    hipStream_t st = hm_engine_stream(s->e);
    const uint32_t S = s->S;
    hm_doc_result *rd; DevDoc *dm; uint32_t *seen; IncState *ist; uint2 *ldir; int r;
    if ((r = dev_alloc(s, &rd, cap)) || (r = dev_alloc(s, &dm, cap)) || (r = dev_alloc(s, &seen, cap)) ||
        (r = dev_alloc(s, &ist, cap)) || (r = dev_alloc(s, &ldir, cap * HM_INC_LISTS)))
        return r;
    SCHK(s, hipMemsetAsync(rd, 0, cap * sizeof(hm_doc_result), st));
    SCHK(s, hipMemsetAsync(dm, 0, cap * sizeof(DevDoc), st));
    SCHK(s, hipMemsetAsync(seen, 0, cap * 4, st));
    SCHK(s, hipMemsetAsync(ist, 0, cap * sizeof(IncState), st));
    SCHK(s, hipMemsetAsync(ldir, 0, cap * HM_INC_LISTS * sizeof(uint2), st));
    if (s->cap_h) {
        SCHK(s, hipMemcpyAsync(rd, s->res_docs, s->cap_h * sizeof(hm_doc_result), hipMemcpyDeviceToDevice, st));
        SCHK(s, hipMemcpyAsync(dm, s->dm, s->cap_h * sizeof(DevDoc), hipMemcpyDeviceToDevice, st));
        SCHK(s, hipMemcpyAsync(seen, s->seen, s->cap_h * 4, hipMemcpyDeviceToDevice, st));
        SCHK(s, hipMemcpyAsync(ist, s->ist, s->cap_h * sizeof(IncState), hipMemcpyDeviceToDevice, st));
        SCHK(s, hipMemcpyAsync(ldir, s->ldir, s->cap_h * HM_INC_LISTS * sizeof(uint2), hipMemcpyDeviceToDevice, st));
    }
    uint32_t **tabs[5] = {&s->clock, &s->back_clock, &s->heads, &s->min_clock, &s->stored};
    uint32_t *nt[5];
    for (int i = 0; i < 5; i++) {
        if ((r = dev_alloc(s, &nt[i], cap * S))) return r;
        SCHK(s, hipMemsetAsync(nt[i], 0, cap * S * 4, st));
        if (s->cap_h) SCHK(s, hipMemcpyAsync(nt[i], *tabs[i], s->cap_h * S * 4, hipMemcpyDeviceToDevice, st));
    }
    SCHK(s, hipStreamSynchronize(st));
    if (s->res_docs) (void)hipFree(s->res_docs);
    if (s->dm) (void)hipFree(s->dm);
    if (s->seen) (void)hipFree(s->seen);
    if (s->ist) (void)hipFree(s->ist);
    if (s->ldir) (void)hipFree(s->ldir);
    s->res_docs = rd; s->dm = dm; s->seen = seen; s->ist = ist; s->ldir = ldir;
    for (int i = 0; i < 5; i++) { if (*tabs[i]) (void)hipFree(*tabs[i]); *tabs[i] = nt[i]; }
    s->cap_h = cap;
    return HM_OK;
}

// HM_STORE_PROFILE=1: per-phase wall times of hm_batch_submit / hm_batch_wait on stderr (the
// stream is synchronised at each mark, so device work is attributed to its phase)
struct PhaseTimer {
    bool on;
    hipStream_t st;
    std::chrono::steady_clock::time_point t;
    explicit PhaseTimer(hipStream_t s) : on(getenv("HM_STORE_PROFILE") != nullptr), st(s), t(std::chrono::steady_clock::now()) {}
    void mark(const char *what) {
        if (!on) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[hm_store] %-18s %9.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// Staged batch layout on the device: [changes][deps][ops][docs][handles][remap][gather][bail]
struct StageLayout {
    size_t o_ch, o_dp, o_op, o_docs, o_hand, o_remap, o_gather, o_bail, o_defer, o_gdone, o_fail, total;
};
StageLayout layout(size_t nc, size_t nd, size_t no, size_t n, size_t nremap, uint32_t S) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    StageLayout L;
    size_t o = 0;
    L.o_ch = o; o += al(nc * sizeof(hm_change_row) + 1);
    L.o_dp = o; o += al(nd * sizeof(hm_dep_row) + 1);
    L.o_op = o; o += al(no * sizeof(hm_op_row) + 1);
    L.o_docs = o; o += al(n * sizeof(hm_doc_row) + 1);
    L.o_hand = o; o += al(n * 4 + 1);
    L.o_remap = o; o += al(nremap + 1);
    L.o_gather = o; o += al(n * (sizeof(hm_doc_result) + 3 * 4 * (size_t)S) + 1);
    L.o_bail = o; o += al(4 * (n + 1));
    L.o_defer = o; o += al(4 * (n + 1));
    L.o_gdone = o; o += al(n);
    L.o_fail = o; o += 256;
    L.total = o;
    return L;
}

// HM_INC_DEBUG_HANDLE=h (dev diagnostics): the incremental list state of handle h on stderr
void dbg_list_state(hm_store *s, const char *when) {
    const char *e = getenv("HM_INC_DEBUG_HANDLE");
    if (!e) return;
    const uint32_t h = (uint32_t)atoi(e);
    if (h >= s->n_handles) return;
    hipStream_t st = hm_engine_stream(s->e);
    DevDoc m; IncState I; uint2 dir[HM_INC_LISTS];
    (void)hipMemcpyAsync(&m, s->dm + h, sizeof m, hipMemcpyDeviceToHost, st);
    (void)hipMemcpyAsync(&I, s->ist + h, sizeof I, hipMemcpyDeviceToHost, st);
    (void)hipMemcpyAsync(dir, s->ldir + (size_t)h * HM_INC_LISTS, sizeof dir, hipMemcpyDeviceToHost, st);
    (void)hipStreamSynchronize(st);
    std::vector<uint32_t> lo(m.n_r + 1), ep(m.n_r + 1), pa(m.n_r + 1), ek(m.n_r + 1);
    if (m.n_r) {
        (void)hipMemcpyAsync(lo.data(), s->lorder + m.r_off, m.n_r * 4, hipMemcpyDeviceToHost, st);
        (void)hipMemcpyAsync(ep.data(), s->epos + m.r_off, m.n_r * 4, hipMemcpyDeviceToHost, st);
        (void)hipMemcpyAsync(pa.data(), s->epar + m.r_off, m.n_r * 4, hipMemcpyDeviceToHost, st);
        (void)hipMemcpyAsync(ek.data(), s->ekey + m.r_off, m.n_r * 4, hipMemcpyDeviceToHost, st);
        (void)hipStreamSynchronize(st);
    }
    fprintf(stderr, "[inc dbg %s] h=%u n_r=%u r_off=%u flags=%u n_el=%u nl=%u dir=", when, h, m.n_r, m.r_off, I.flags, I.pad[0], I.pad[1]);
    for (uint32_t k = 0; k < HM_INC_LISTS && k < I.pad[1]; k++) fprintf(stderr, "(%u,%u)", dir[k].x, dir[k].y);
    fprintf(stderr, "\n  lorder:");
    for (uint32_t i = 0; i < I.pad[0] && i < m.n_r; i++) fprintf(stderr, " %u", lo[i]);
    fprintf(stderr, "\n  epos/epar/ekey:");
    for (uint32_t r = 0; r < m.n_r; r++) fprintf(stderr, " %u:%d/%d/%x", r, (int)ep[r], (int)pa[r], ek[r]);
    fprintf(stderr, "\n");
}

// Re-merge the `n` documents listed (handles, device) on the engine stream: their launch rows
// built on the device from their metas, the launch hints read back.
int launch_list_merge(hm_store *s, const uint32_t *dev_list, uint32_t n) {
    if (!n) return HM_OK;
    hipStream_t st = hm_engine_stream(s->e);
    int rc;
    if ((rc = ensure_buf(s, s->rows, n)) || (rc = ensure_buf(s, s->klist, n))) return rc;
    if ((rc = reset_stats(s))) return rc;
    const uint32_t small_lists = hm_small_list_ops(s->S, s->inc_mode);
    // (the states of the documents that keep none are cleared — unless no document holds one)
    SCHK(s, hm_launch_doc_rows(dev_list, n, s->dm, s->rows.p, s->st, small_lists, s->incremental && s->any_state ? s->ist : nullptr,
                               s->klist.p, st));
    rc = HM_OK;
    const PlanStats P = read_stats(s, &rc);
    if (rc) return rc;
    hm_batch b = {};
    b.a_stride = s->S;
    b.n_docs = n;
    b.n_changes = (uint32_t)std::min<unsigned long long>(P.tot_c, 0xFFFFFFFFull);
    b.n_deps = (uint32_t)std::min<unsigned long long>(P.tot_d, 0xFFFFFFFFull);
    b.n_ops = (uint32_t)std::min<unsigned long long>(P.tot_o, 0xFFFFFFFFull);
    b.n_regs = (uint32_t)std::min<unsigned long long>(P.tot_r, 0xFFFFFFFFull);
    b.max_changes = P.max_c; b.max_ops = P.max_o; b.max_regs = P.max_r; b.max_objs = P.max_objs; b.max_deps = P.max_d;
    b.doc_flags = P.flags;
    if (!b.max_changes && !b.max_ops && !b.max_regs && !b.max_objs) b.max_objs = 1;   // device hints present
    b.docs = s->rows.p;
    b.changes = s->changes; b.deps = s->deps; b.ops = s->ops; b.min_clock = s->min_clock;
    hm_results o;
    o.docs = s->res_docs; o.clock = s->clock; o.back_clock = s->back_clock; o.heads = s->heads;
    o.hist = s->hist; o.all_deps = s->all_deps; o.regs = s->regs; o.surv = s->surv;
    const hm_extents ext = {(uint32_t)s->cap_c, (uint32_t)s->cap_d, (uint32_t)s->cap_o, (uint32_t)s->cap_r};
    // the incremental path keeps list documents' element order: positions written by the merge
    // (mode 1: when every listed document holds <= HM_INC_SMALL_LIST_OPS ops, none with lists keeps
    // incremental state — inc_meta skips them — so no positions are needed)
    // (P.mx[3]: listed list documents that may keep incremental state)
    const bool positions = s->incremental && (P.flags & HM_DOC_HAS_LISTS) && P.mx[3] != 0;
    if (positions) SCHK(s, hm_launch_epos_clear(s->klist.p, P.mx[2], s->dm, s->epos, st));     // (the keep list)
    rc = hm_engine_launch_merge(s->e, &b, &o, dev_list, &ext, positions ? s->epos : nullptr);
    // the incremental path's survivor metadata of the re-merged documents that may keep state (the
    // keep list doc_rows_kernel built; it cleared the others' IncState)
    if (rc == HM_OK && s->incremental && P.mx[2]) {
        MetaArgs M;
        M.list = s->klist.p; M.n = P.mx[2]; M.dm = s->dm; M.res_docs = s->res_docs; M.changes = s->changes; M.hist = s->hist;
        M.ckey = s->ckey; M.ops = s->ops; M.surv = s->surv; M.smeta = s->smeta; M.ist = s->ist;
        M.epos = s->epos; M.epar = s->epar; M.ekey = s->ekey; M.lorder = s->lorder; M.ldir = s->ldir;
        M.small_lists = small_lists;
        M.n_valid = &s->st->n_valid;
        if ((rc = ensure_buf(s, s->mpart, HM_META_GRID))) return rc;
        M.part = s->mpart.p;
        SCHK(s, hm_launch_inc_meta(M, st));
    }
    // documents whose state can route them to the incremental kernels, after this re-merge (the
    // only step that adds or drops states): none (e.g. mode 1 with only small list documents, or
    // every document with queued changes) = the next submits launch no incremental kernel
    const bool count = s->incremental && (s->any_state || P.mx[2]);
    if (count) SCHK(s, hipMemcpyAsync(&s->h_cnt[4], &s->st->n_valid, 4, hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));
    if (count) s->any_state = s->h_cnt[4] != 0;
    return rc;
}

// Rebuild every arena larger and compact all documents into it; every document is
// re-merged (its outputs live in the arenas too).  `extra` = rows the caller is about
// to append per space, so the new arenas fit them.  The metas come to the host for it.
int compact(hm_store *s, size_t extra_c, size_t extra_d, size_t extra_o, size_t extra_r) {
    hipStream_t st = hm_engine_stream(s->e);
    const uint32_t S = s->S, n = s->n_handles;
    std::vector<DevDoc> old(n);
    if (n) {
        SCHK(s, hipMemcpyAsync(old.data(), s->dm, (size_t)n * sizeof(DevDoc), hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
    }
    size_t live_c = extra_c, live_d = extra_d, live_o = extra_o, live_r = extra_r;
    for (auto &m : old) {
        live_c += seg_cap(m.n_c); live_d += seg_cap(m.n_d); live_o += seg_cap(m.n_o); live_r += seg_cap(m.n_r);
    }
    const size_t nc = std::max<size_t>(2 * live_c, 1 << 16), nd = std::max<size_t>(2 * live_d, 1 << 16);
    const size_t no = std::max<size_t>(2 * live_o, 1 << 16), nr = std::max<size_t>(2 * live_r, 1 << 16);
    hm_change_row *ch; int32_t *hi; uint32_t *ad; hm_dep_row *dp; hm_op_row *op; hm_surv_result *sv; hm_reg_result *rg;
    uint2 *sm;
    uint32_t *ck, *ep, *epr, *ek, *lo;
    int r;
    if ((r = dev_alloc(s, &ch, nc)) || (r = dev_alloc(s, &hi, nc)) || (r = dev_alloc(s, &ck, nc)) || (r = dev_alloc(s, &ad, nc * S)) ||
        (r = dev_alloc(s, &dp, nd)) || (r = dev_alloc(s, &op, no)) || (r = dev_alloc(s, &sv, no)) ||
        (r = dev_alloc(s, &sm, no)) || (r = dev_alloc(s, &rg, nr)) || (r = dev_alloc(s, &ep, nr)) ||
        (r = dev_alloc(s, &epr, nr)) || (r = dev_alloc(s, &ek, nr)) || (r = dev_alloc(s, &lo, nr)))
        return r;
    // relocate every document (old rows only; no new rows, no remap)
    std::vector<AppendDesc> descs(n);
    std::vector<DevDoc> nm = old;
    std::vector<uint32_t> all(n);
    uint64_t uc = 0, ud = 0, uo = 0, ur = 0;
    auto seg = [](uint64_t &used, uint32_t need, uint32_t &off, uint32_t &cap) {
        cap = seg_cap(need);
        off = (uint32_t)used;
        used += cap;
    };
    for (uint32_t h = 0; h < n; h++) {
        DevDoc &m = nm[h];
        const DevDoc &o = old[h];
        seg(uc, m.n_c, m.c_off, m.c_cap); seg(ud, m.n_d, m.d_off, m.d_cap);
        seg(uo, m.n_o, m.o_off, m.o_cap); seg(ur, m.n_r, m.r_off, m.r_cap);
        AppendDesc D = {};
        D.handle = h;
        D.src_c = o.c_off; D.dst_c = m.c_off; D.n_old_c = o.n_c;
        D.src_d = o.d_off; D.dst_d = m.d_off; D.n_old_d = o.n_d;
        D.src_o = o.o_off; D.dst_o = m.o_off; D.n_old_o = o.n_o;
        D.remap_row = 0xFFFFFFFFu;
        descs[h] = D;
        all[h] = h;
    }
    StoreArenas src = {s->changes, s->deps, s->ops, s->min_clock, s->stored};
    StoreArenas dst = {ch, dp, op, s->min_clock, s->stored};
    if (n) {
        if ((r = ensure_buf(s, s->descs, n))) return r;
        SCHK(s, hipMemcpyAsync(s->descs.p, descs.data(), (size_t)n * sizeof(AppendDesc), hipMemcpyHostToDevice, st));
        SCHK(s, hm_launch_append(s->descs.p, n, src, dst, nullptr, nullptr, nullptr, nullptr, S, st));
        SCHK(s, hipMemcpyAsync(s->dm, nm.data(), (size_t)n * sizeof(DevDoc), hipMemcpyHostToDevice, st));
        SCHK(s, hipStreamSynchronize(st));
    }
    (void)hipFree(s->changes); (void)hipFree(s->hist); (void)hipFree(s->ckey); (void)hipFree(s->all_deps); (void)hipFree(s->deps);
    (void)hipFree(s->ops); (void)hipFree(s->surv); (void)hipFree(s->smeta); (void)hipFree(s->regs);
    (void)hipFree(s->epos); (void)hipFree(s->epar); (void)hipFree(s->ekey); (void)hipFree(s->lorder);
    s->epos = ep; s->epar = epr; s->ekey = ek; s->lorder = lo;
    s->changes = ch; s->hist = hi; s->ckey = ck; s->all_deps = ad; s->deps = dp; s->ops = op; s->surv = sv; s->smeta = sm; s->regs = rg;
    s->cap_c = nc; s->cap_d = nd; s->cap_o = no; s->cap_r = nr;
    const unsigned long long bump[4] = {uc, ud, uo, ur};
    SCHK(s, hipMemcpyAsync(s->st->bump, bump, sizeof bump, hipMemcpyHostToDevice, st));
    if (!n) { SCHK(s, hipStreamSynchronize(st)); return HM_OK; }
    if ((r = ensure_buf(s, s->list, n))) return r;
    SCHK(s, hipMemcpyAsync(s->list.p, all.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    return launch_list_merge(s, s->list.p, n);
}

}  // namespace

extern "C" {

int hm_store_create(hm_engine *e, const hm_store_config *cfg, hm_store **out) {
    if (!e || !out) return HM_ERR_INVALID;
    *out = nullptr;
    const uint32_t S = cfg ? cfg->a_stride : 8;
    if (S == 0 || S > HM_MAX_STRIDE) return hm_engine_fail(e, HM_ERR_INVALID, "store a_stride must be in [1,256]");
    hm_store *s = new (std::nothrow) hm_store();
    if (!s) return HM_ERR_NOMEM;
    s->e = e; s->S = S;
    if (hipSetDevice(hm_engine_device(e)) != hipSuccess) { delete s; return HM_ERR_DEVICE; }
    int r = dev_alloc(s, &s->st, 1);
    if (r == HM_OK && hipMemset(s->st, 0, sizeof(PlanStats)) != hipSuccess) r = HM_ERR_DEVICE;
    if (r == HM_OK && (hipHostMalloc((void **)&s->h_st, sizeof(PlanStats), hipHostMallocDefault) != hipSuccess ||
                       hipHostMalloc((void **)&s->h_cnt, 64, hipHostMallocDefault) != hipSuccess))
        r = HM_ERR_NOMEM;
    if (r == HM_OK) r = compact(s, 0, 0, 0, 0);
    if (r == HM_OK) r = ensure_handles(s, 1024);
    if (r != HM_OK) { hm_store_destroy(s); return r; }
    *out = s;
    return HM_OK;
}

void hm_store_destroy(hm_store *s) {
    if (!s) return;
    (void)hipStreamSynchronize(hm_engine_stream(s->e));
    void *bufs[] = {s->changes, s->hist, s->ckey, s->all_deps, s->deps, s->ops, s->surv, s->smeta, s->ist, s->ldir, s->regs, s->epos,
                    s->epar, s->ekey, s->lorder, s->res_docs, s->clock,
                    s->back_clock, s->heads, s->min_clock, s->stored, s->stage.p, s->dm, s->seen, s->plan.p, s->descs.p,
                    s->bdescs.p, s->list.p, s->blist.p, s->alist.p, s->remap.p, s->inv.p, s->rows.p, s->undo_handles.p, s->klist.p, s->mpart.p, s->past.p, s->st};
    for (void *b : bufs) if (b) (void)hipFree(b);
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    if (s->h_st) (void)hipHostFree(s->h_st);
    if (s->h_cnt) (void)hipHostFree(s->h_cnt);
    delete s;
}

int hm_doc_open(hm_store *s, uint32_t *out_doc) { return hm_doc_open_n(s, 1, out_doc); }

int hm_doc_open_n(hm_store *s, uint32_t n, uint32_t *out_first) {
    if (!s || !out_first) return HM_ERR_INVALID;
    try {
        if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "hm_doc_open while a batch is in flight");
        const uint32_t h0 = s->n_handles;
        int r = ensure_handles(s, (size_t)h0 + n);
        if (r) return r;
        // Backend.init(): an empty log (ROOT only) and its result row, written on the engine
        // stream (ordered before any submit; the reads below synchronise the stream)
        hipStream_t st = hm_engine_stream(s->e);
        SCHK(s, hm_launch_init_docs(s->dm, h0, n, st));
        if (n) {
            SCHK(s, hipMemsetAsync(s->res_docs + h0, 0, (size_t)n * sizeof(hm_doc_result), st));
            std::vector<hm_doc_result> rows(n);
            for (auto &x : rows) { x = hm_doc_result{}; x.err_change = HM_NONE; x.err_op = HM_NONE; }
            SCHK(s, hipMemcpyAsync(s->res_docs + h0, rows.data(), (size_t)n * sizeof(hm_doc_result), hipMemcpyHostToDevice, st));
            SCHK(s, hipStreamSynchronize(st));
        }
        s->n_handles = h0 + n;
        *out_first = h0;
        return HM_OK;
    } catch (...) {
        return HM_ERR_NOMEM;
    }
}

int hm_doc_reset(hm_store *s, const uint32_t *doc_handles, uint32_t n) {
    if (!s || (n && !doc_handles)) return HM_ERR_INVALID;
    try {
        if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "hm_doc_reset while a batch is in flight");
        if (!n) return HM_OK;
        std::vector<uint32_t> hs(doc_handles, doc_handles + n);
        std::sort(hs.begin(), hs.end());
        if (hs.back() >= s->n_handles) return hm_engine_fail(s->e, HM_ERR_INVALID, "hm_doc_reset: bad handle");
        if (std::adjacent_find(hs.begin(), hs.end()) != hs.end())
            return hm_engine_fail(s->e, HM_ERR_INVALID, "hm_doc_reset: repeated handle");
        int r;
        if ((r = ensure_buf(s, s->blist, n))) return r;
        hipStream_t st = hm_engine_stream(s->e);
        SCHK(s, hipMemcpyAsync(s->blist.p, hs.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        SCHK(s, hm_launch_reset_docs(s->blist.p, n, s->dm, s->res_docs, s->ist, s->clock, s->back_clock, s->heads, s->min_clock,
                                     s->stored, s->S, &s->st->n_valid, st));
        SCHK(s, hipStreamSynchronize(st));
        s->undo_id = 0;                               // the last batch's undo no longer applies
        return HM_OK;
    } catch (...) {
        return HM_ERR_NOMEM;
    }
}

// hm_batch_submit / hm_batch_submit_device: `dev` = the batch's tables, handles and remap are
// device pointers (no host staging of the rows)
static int submit_impl(hm_store *s, const hm_batch *b, const uint32_t *doc_handles, const uint8_t *actor_remap,
                       uint64_t *out_batch_id, bool dev) {
    if (!s || !b || (b->n_docs && (!doc_handles || !b->docs))) return HM_ERR_INVALID;
    try {
        if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "a batch is already in flight (call hm_batch_wait)");
        const uint32_t S = s->S, n = b->n_docs;
        s->undo_id = 0;                                  // the plan rows hm_batch_undo reads are replaced
        if (b->a_stride != S) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch a_stride must equal the store's");
        SCHK(s, hipSetDevice(hm_engine_device(s->e)));
        hipStream_t st = hm_engine_stream(s->e);
        PhaseTimer T(st);
        int rc;
        // stage the batch (its tables, rows, handles and remap) on the device
        const size_t nremap = actor_remap ? (size_t)n * S : 0;
        const StageLayout L = dev ? layout(0, 0, 0, n, 0, S) : layout(b->n_changes, b->n_deps, b->n_ops, n, nremap, S);
        if ((rc = ensure_stage(s, L.total)) || (rc = ensure_buf(s, s->plan, n)) || (rc = ensure_buf(s, s->descs, n)) ||
            (rc = ensure_buf(s, s->list, n)))
            return rc;
        uint8_t *sp = s->stage.p;
        const hm_doc_row *t_docs = b->docs;
        const hm_change_row *t_ch = b->changes;
        const hm_dep_row *t_dp = b->deps;
        const hm_op_row *t_op = b->ops;
        const uint32_t *t_hand = doc_handles;
        const uint8_t *t_remap = actor_remap;
        if (!dev) {
            if (b->n_changes) SCHK(s, hipMemcpyAsync(sp + L.o_ch, b->changes, b->n_changes * sizeof(hm_change_row), hipMemcpyHostToDevice, st));
            if (b->n_deps) SCHK(s, hipMemcpyAsync(sp + L.o_dp, b->deps, b->n_deps * sizeof(hm_dep_row), hipMemcpyHostToDevice, st));
            if (b->n_ops) SCHK(s, hipMemcpyAsync(sp + L.o_op, b->ops, b->n_ops * sizeof(hm_op_row), hipMemcpyHostToDevice, st));
            if (n) {
                SCHK(s, hipMemcpyAsync(sp + L.o_docs, b->docs, (size_t)n * sizeof(hm_doc_row), hipMemcpyHostToDevice, st));
                SCHK(s, hipMemcpyAsync(sp + L.o_hand, doc_handles, (size_t)n * 4, hipMemcpyHostToDevice, st));
            }
            if (nremap) SCHK(s, hipMemcpyAsync(sp + L.o_remap, actor_remap, nremap, hipMemcpyHostToDevice, st));
            t_docs = (const hm_doc_row *)(sp + L.o_docs); t_ch = (const hm_change_row *)(sp + L.o_ch);
            t_dp = (const hm_dep_row *)(sp + L.o_dp); t_op = (const hm_op_row *)(sp + L.o_op);
            t_hand = (const uint32_t *)(sp + L.o_hand); t_remap = nremap ? sp + L.o_remap : nullptr;
        }
        T.mark("stage: h2d");
        PlanArgs A;
        A.docs = t_docs; A.changes = t_ch;
        A.handles = t_hand; A.remap = nremap ? t_remap : nullptr;
        A.n = n; A.n_changes = b->n_changes; A.n_deps = b->n_deps; A.n_ops = b->n_ops; A.n_handles = s->n_handles;
        A.S = S; A.stamp = ++s->stamp ? s->stamp : ++s->stamp; A.incremental = s->incremental && S <= 64 && s->any_state ? s->inc_mode : 0u;
        // (no document holds a usable state: the plan routes every document to the re-merge and no
        // incremental kernel is launched)
        A.dm = s->dm; A.res_docs = s->res_docs; A.seen = s->seen; A.plan = s->plan.p; A.descs = s->descs.p;
        A.list = s->list.p; A.st = s->st;
        A.ist = A.incremental ? s->ist : nullptr; A.ops = t_op; A.deps = t_dp; A.clock = s->clock;
        A.defer = (uint32_t *)(sp + L.o_defer);
        // the submit's work-list counts and gathered-row flags, zeroed by plan_kernel (no memsets)
        A.bail = (uint32_t *)(sp + L.o_bail); A.fail = (uint32_t *)(sp + L.o_fail); A.gdone = sp + L.o_gdone;
        if ((rc = ensure_buf(s, s->alist, n))) return rc;
        A.alist = s->alist.p;
        A.cap[0] = s->cap_c; A.cap[1] = s->cap_d; A.cap[2] = s->cap_o; A.cap[3] = s->cap_r;
        uint32_t *bail = (uint32_t *)(sp + L.o_bail);            // (count zeroed by the plan)
        if (!s->ev[0])
            for (auto &e : s->ev) SCHK(s, hipEventCreate(&e));
        // plan (checks, growth, routes), alloc, append and the incremental kernels go out back to
        // back: alloc_kernel itself does nothing when the plan failed a check or the arenas cannot
        // take the growth (every later kernel then finds no work), and the host reads the plan's
        // stats once, with the re-merge counts.  A failed check fails the submit with the store
        // as it was; no room compacts the store (every document re-merged) and runs the plan again.
        PlanStats P;
        uint32_t counts[2] = {0, 0};
        for (int attempt = 0;; attempt++) {
            if ((rc = reset_stats(s))) return rc;
            SCHK(s, hm_launch_plan(A, st));
            T.mark("plan");
            SCHK(s, hm_launch_alloc(A, st));
            StoreArenas ar = {s->changes, s->deps, s->ops, s->min_clock, s->stored};
            if (T.on) {
                // what the append has to move: documents whose segments moved, re-ranked ones, old rows
                std::vector<AppendDesc> dd(n);
                SCHK(s, hipMemcpyAsync(dd.data(), s->descs.p, (size_t)n * sizeof(AppendDesc), hipMemcpyDeviceToHost, st));
                SCHK(s, hipStreamSynchronize(st));
                size_t mv = 0, rmp = 0, inc = 0, old_o = 0, new_o = 0;
                for (const AppendDesc &D : dd) {
                    const bool m = D.src_c != D.dst_c || D.src_d != D.dst_d || D.src_o != D.dst_o;
                    mv += m; rmp += D.remap_row != 0xFFFFFFFFu; inc += (D.inc & HM_DINC_ROUTE) != 0; new_o += D.n_new_o;
                    if (m) old_o += D.n_old_o;
                }
                fprintf(stderr, "[hm_store] append: %zu docs, %zu moved (%zu old op rows), %zu re-ranked, %zu incremental, %zu new op rows\n",
                        (size_t)n, mv, old_o, rmp, inc, new_o);
                T.mark("(append census)");
            }
            SCHK(s, hm_launch_append(s->descs.p, n, ar, ar, A.changes, t_dp, t_op, A.remap, S, st, s->alist.p, &s->st->n_app));
            T.mark("alloc+append");
            SCHK(s, hipEventRecord(s->ev[0], st));
            if (A.incremental) {
                IncArgs IA;
                IA.descs = s->descs.p; IA.n = n; IA.list = nullptr; IA.S = S;
                IA.st_changes = A.changes; IA.st_deps = t_dp; IA.st_ops = t_op;
                IA.changes = s->changes; IA.deps = s->deps; IA.ops = s->ops; IA.hist = s->hist; IA.ckey = s->ckey; IA.all_deps = s->all_deps;
                IA.regs = s->regs; IA.surv = s->surv; IA.smeta = s->smeta; IA.res_docs = s->res_docs;
                IA.epos = s->epos; IA.epar = s->epar; IA.ekey = s->ekey; IA.lorder = s->lorder; IA.ldir = s->ldir;
                IA.clock = s->clock; IA.back_clock = s->back_clock; IA.heads = s->heads; IA.min_clock = s->min_clock;
                IA.ist = s->ist; IA.bail = bail; IA.defer = (uint32_t *)(sp + L.o_defer);
                IA.n_lane = S == 8 || S == 16 ? 1u : 0u;                 // (the lane pass reads its count on the device)
                IA.pst = s->st;
                // the documents the incremental kernels finish write their gathered rows themselves
                IA.gout = sp + L.o_gather; IA.gdone = sp + L.o_gdone;      // (gdone zeroed by the plan)
                dbg_list_state(s, "before");
                SCHK(s, hm_launch_inc_apply(IA, st));
                dbg_list_state(s, "after");
            }
            SCHK(s, hipEventRecord(s->ev[1], st));
            T.mark("incremental");
            // the plan's stats and the re-merge counts (cold documents, then those the incremental
            // kernels handed back), one read
            SCHK(s, hipMemcpyAsync(s->h_st, s->st, sizeof(PlanStats), hipMemcpyDeviceToHost, st));
            SCHK(s, hipMemcpyAsync(&s->h_cnt[1], bail, 4, hipMemcpyDeviceToHost, st));
            SCHK(s, hipStreamSynchronize(st));
            P = *s->h_st;
            counts[0] = P.n_cold; counts[1] = s->h_cnt[1];
            if (P.err) {
                const char *why = (P.err & HM_PLAN_BAD_HANDLE) || (P.err & HM_PLAN_REPEATED) ? "bad or repeated document handle"
                                : (P.err & HM_PLAN_ROWS) ? "document rows outside the batch tables"
                                : (P.err & HM_PLAN_TOTALS) ? "document totals must cover the existing log (and n_actors <= a_stride)"
                                : (P.err & HM_PLAN_CHANGE_ROWS) ? "change rows outside their document's deps/ops"
                                : "actor remap is not a permutation into the new ranks";
                if (attempt) return hm_engine_fail(s->e, HM_ERR_INVALID, "submit plan failed after compaction");
                return hm_engine_fail(s->e, HM_ERR_INVALID, why);
            }
            // (P.bump already counts this submit's segments when alloc_kernel ran: its own verdict decides)
            if (!P.mx[1]) break;
            // the arenas cannot take the growth (alloc_kernel did nothing): compact, then plan again
            if (attempt) return hm_engine_fail(s->e, HM_ERR_NOMEM, "the store's arenas cannot take the submit after compaction");
            if ((rc = compact(s, P.need[0], P.need[1], P.need[2], P.need[3]))) return rc;
            A.stamp = ++s->stamp ? s->stamp : ++s->stamp;
            A.dm = s->dm; A.descs = s->descs.p; A.list = s->list.p;     // (compaction may have regrown them)
            A.cap[0] = s->cap_c; A.cap[1] = s->cap_d; A.cap[2] = s->cap_o; A.cap[3] = s->cap_r;
            T.mark("compact");
        }
        if (counts[1]) SCHK(s, hipMemcpyAsync(s->list.p + counts[0], bail + 1, (size_t)counts[1] * 4, hipMemcpyDeviceToDevice, st));
        SCHK(s, hipEventRecord(s->ev[2], st));
        if ((rc = launch_list_merge(s, s->list.p, counts[0] + counts[1]))) return rc;
        SCHK(s, hipEventRecord(s->ev[3], st));
        s->ev_live = true;           // (read by hm_batch_wait after its stream sync: submit stays asynchronous)
        dbg_list_state(s, "after merge");
        T.mark("remerge");
        s->st_inc = P.n_inc - counts[1]; s->st_cold = counts[0]; s->st_bail = counts[1];
        uint32_t *fail = (uint32_t *)(sp + L.o_fail);            // (count zeroed by the plan)
        SCHK(s, hm_launch_gather(A.handles, n, S, s->res_docs, s->clock, s->back_clock, s->heads, sp + L.o_gather, fail, st,
                                 P.n_inc ? sp + L.o_gdone : nullptr));
        s->p_gather_dev = sp + L.o_gather;
        s->p_fail_dev = fail;
        s->p_handles_dev = const_cast<uint32_t *>(A.handles);
        s->p_n = n;
        s->p_remap = nremap != 0;
        if (nremap) {
            // the rollback needs the remap rows after the staging area is reused
            if ((rc = ensure_buf(s, s->remap, nremap))) return rc;
            SCHK(s, hipMemcpyAsync(s->remap.p, A.remap, nremap, hipMemcpyDeviceToDevice, st));
        }
        T.mark("gather");
        s->pending = true;
        s->pending_id = s->next_id++;
        if (out_batch_id) *out_batch_id = s->pending_id;
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_batch_submit");
    }
}

int hm_batch_submit(hm_store *s, const hm_batch *b, const uint32_t *doc_handles, const uint8_t *actor_remap,
                    uint64_t *out_batch_id) {
    return submit_impl(s, b, doc_handles, actor_remap, out_batch_id, false);
}

int hm_batch_submit_device(hm_store *s, const hm_batch *b, const uint32_t *doc_handles, const uint8_t *actor_remap,
                           uint64_t *out_batch_id) {
    return submit_impl(s, b, doc_handles, actor_remap, out_batch_id, true);
}

// Roll documents of the last submit back to their logs before it (every = false: those whose merge
// failed; true: all of them not rolled back yet): totals restored, ranks re-mapped back, the log
// truncated, the previous state re-merged.
static int roll_back(hm_store *s, const uint32_t *handles_dev, uint32_t n, bool every) {
    hipStream_t st = hm_engine_stream(s->e);
    const uint32_t S = s->S;
    int rc;
    if ((rc = ensure_buf(s, s->bdescs, n)) || (rc = ensure_buf(s, s->blist, n)) ||
        (s->p_remap && (rc = ensure_buf(s, s->inv, (size_t)n * S))))
        return rc;
    if ((rc = reset_stats(s))) return rc;
    SCHK(s, hm_launch_rollback(handles_dev, n, s->res_docs, s->plan.p, s->p_remap ? s->remap.p : nullptr, S, s->dm,
                               s->bdescs.p, s->p_remap ? s->inv.p : nullptr, s->blist.p, s->st, every ? 1u : 0u, st));
    uint32_t nb = 0;
    SCHK(s, hipMemcpyAsync(&nb, &s->st->n_back, 4, hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));
    StoreArenas ar = {s->changes, s->deps, s->ops, s->min_clock, s->stored};
    SCHK(s, hm_launch_append(s->bdescs.p, nb, ar, ar, nullptr, nullptr, nullptr, s->p_remap ? s->inv.p : nullptr, S, st));
    return launch_list_merge(s, s->blist.p, nb);
}

// hm_batch_wait / hm_batch_wait_device: the gathered rows to the host arrays, or (out_dev) as one
// device-to-device copy with only the failure count read back
static int wait_impl(hm_store *s, uint64_t batch_id, hm_doc_result *out_docs, uint32_t *out_clock,
                     uint32_t *out_back_clock, uint32_t *out_heads, void *out_dev, uint32_t *out_n_failed) {
    if (!s) return HM_ERR_INVALID;
    try {
        if (!s->pending || batch_id != s->pending_id) return hm_engine_fail(s->e, HM_ERR_INVALID, "no such batch in flight");
        SCHK(s, hipSetDevice(hm_engine_device(s->e)));        // the caller may be a host thread of its own
        hipStream_t st = hm_engine_stream(s->e);
        PhaseTimer T(st);
        // the batch stays in flight (pending) until this returns: copy-out and rollback below
        // still read and re-merge the store's documents
        struct Clear { std::atomic<bool> &p; ~Clear() { p.store(false); } } clear_pending{s->pending};
        const uint32_t n = s->p_n, S = s->S;
        // results straight from the gathered device rows into the caller's arrays
        std::vector<hm_doc_result> tmp;
        hm_doc_result *res = out_docs;
        if (!res && !out_dev) { tmp.resize(n); res = tmp.data(); }
        uint32_t n_fail = 0;
        if (n && out_dev) {
            const size_t bytes = (size_t)n * (sizeof(hm_doc_result) + 3 * 4 * (size_t)S);
            SCHK(s, hipMemcpyAsync(out_dev, s->p_gather_dev, bytes, hipMemcpyDeviceToDevice, st));
            SCHK(s, hipMemcpyAsync(&n_fail, s->p_fail_dev, 4, hipMemcpyDeviceToHost, st));
            SCHK(s, hipStreamSynchronize(st));
        } else if (n) {
            const uint8_t *g = s->p_gather_dev;
            const size_t rb = (size_t)n * S * 4;
            SCHK(s, hipMemcpyAsync(res, g, (size_t)n * sizeof(hm_doc_result), hipMemcpyDeviceToHost, st));
            g += (size_t)n * sizeof(hm_doc_result);
            if (out_clock) SCHK(s, hipMemcpyAsync(out_clock, g, rb, hipMemcpyDeviceToHost, st));
            if (out_back_clock) SCHK(s, hipMemcpyAsync(out_back_clock, g + rb, rb, hipMemcpyDeviceToHost, st));
            if (out_heads) SCHK(s, hipMemcpyAsync(out_heads, g + 2 * rb, rb, hipMemcpyDeviceToHost, st));
            SCHK(s, hipStreamSynchronize(st));
        }
        T.mark("wait copy-out");
        if (s->ev_live) {
            // the submit's kernel intervals (hm_store_last_kernel_ms), complete after the sync above
            SCHK(s, hipEventSynchronize(s->ev[3]));
            SCHK(s, hipEventElapsedTime(&s->last_ms[0], s->ev[0], s->ev[1]));
            SCHK(s, hipEventElapsedTime(&s->last_ms[1], s->ev[2], s->ev[3]));
            s->ev_live = false;
        }
        // roll back documents whose merge threw (or left the envelope): the log returns to its
        // previous length (rows stay where they are), ranks are re-ranked back, and the previous
        // state is re-merged
        bool any = n_fail != 0;
        for (uint32_t i = 0; res && i < n && !any; i++) any = res[i].status != HM_OK;
        if (out_n_failed) {
            uint32_t k = n_fail;
            if (!out_dev) for (uint32_t i = 0; i < n; i++) k += res[i].status != HM_OK;
            *out_n_failed = k;
        }
        if (any) {
            const int rc = roll_back(s, s->p_handles_dev, n, false);
            if (rc) return rc;
            T.mark("rollback");
        }
        // hm_batch_undo keeps the batch's handles (the staging area is reused by other calls)
        if (n) {
            int rc = ensure_buf(s, s->undo_handles, n);
            if (rc) return rc;
            SCHK(s, hipMemcpyAsync(s->undo_handles.p, s->p_handles_dev, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        }
        s->undo_id = batch_id;
        s->undo_n = n;
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_batch_wait");
    }
}

int hm_batch_wait(hm_store *s, uint64_t batch_id, hm_doc_result *out_docs, uint32_t *out_clock,
                  uint32_t *out_back_clock, uint32_t *out_heads) {
    return wait_impl(s, batch_id, out_docs, out_clock, out_back_clock, out_heads, nullptr, nullptr);
}

int hm_batch_wait_device(hm_store *s, uint64_t batch_id, void *out_dev, uint32_t *out_n_failed) {
    if (!out_dev) return HM_ERR_INVALID;
    return wait_impl(s, batch_id, nullptr, nullptr, nullptr, nullptr, out_dev, out_n_failed);
}

int hm_batch_undo(hm_store *s, uint64_t batch_id) {
    if (!s) return HM_ERR_INVALID;
    try {
        if (s->pending || !batch_id || batch_id != s->undo_id)
            return hm_engine_fail(s->e, HM_ERR_INVALID, "hm_batch_undo: not the last waited batch (or a submit since)");
        SCHK(s, hipSetDevice(hm_engine_device(s->e)));
        const int rc = roll_back(s, s->undo_handles.p, s->undo_n, true);
        s->undo_id = 0;
        return rc;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_batch_undo");
    }
}

int hm_store_set_incremental(hm_store *s, int on) {
    if (!s) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    // re-merges while the path was off kept no survivor metadata: every document's next submit
    // re-merges (and rebuilds it)
    if (on && !s->incremental && s->cap_h) {
        SCHK(s, hipMemsetAsync(s->ist, 0, s->cap_h * sizeof(IncState), hm_engine_stream(s->e)));
        SCHK(s, hipMemsetAsync(&s->st->n_valid, 0, 4, hm_engine_stream(s->e)));
        s->any_state = false;
    }
    s->incremental = on != 0;
    s->inc_mode = on == 2 ? 2u : 1u;
    return HM_OK;
}

int hm_store_last_routing(const hm_store *s, uint32_t *out3) {
    if (!s || !out3) return HM_ERR_INVALID;
    out3[0] = s->st_inc; out3[1] = s->st_cold; out3[2] = s->st_bail;
    return HM_OK;
}

int hm_store_inc_states(hm_store *s, uint32_t *out) {
    if (!s || !out) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    hipStream_t st = hm_engine_stream(s->e);
    SCHK(s, hipMemcpyAsync(&s->h_cnt[5], &s->st->n_valid, 4, hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));
    *out = s->h_cnt[5];
    return HM_OK;
}

int hm_store_arena_info(hm_store *s, uint64_t out_cap[4], uint64_t out_used[4]) {
    if (!s || !out_cap || !out_used) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    SCHK(s, hipSetDevice(hm_engine_device(s->e)));
    hipStream_t st = hm_engine_stream(s->e);
    // (the bump pointers through the page-locked stats block: no submit is using it here)
    SCHK(s, hipMemcpyAsync(s->h_st->bump, s->st->bump, sizeof s->h_st->bump, hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));
    out_cap[0] = s->cap_c; out_cap[1] = s->cap_d; out_cap[2] = s->cap_o; out_cap[3] = s->cap_r;
    for (int k = 0; k < 4; k++) out_used[k] = s->h_st->bump[k];
    return HM_OK;
}

int hm_store_last_kernel_ms(const hm_store *s, float *out2) {
    if (!s || !out2) return HM_ERR_INVALID;
    out2[0] = s->last_ms[0]; out2[1] = s->last_ms[1];
    return HM_OK;
}

int hm_doc_info(hm_store *s, uint32_t doc, hm_doc_info_t *out) {
    if (!s || !out || doc >= s->n_handles) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    int rc = HM_OK;
    const DevDoc m = read_doc(s, doc, &rc);
    if (rc) return rc;
    hm_doc_result r;
    SCHK(s, hipMemcpy(&r, s->res_docs + doc, sizeof(r), hipMemcpyDeviceToHost));
    out->n_changes = m.n_c; out->n_deps = m.n_d; out->n_ops = m.n_o; out->n_regs = m.n_r;
    out->n_objs = m.n_objs; out->n_actors = m.n_actors;
    out->hist_len = r.hist_len; out->n_queued = r.n_queued; out->n_surv = r.n_surv; out->status = r.status;
    return HM_OK;
}

int hm_doc_read(hm_store *s, uint32_t doc, int32_t *hist, uint32_t *all_deps, hm_reg_result *regs,
                hm_surv_result *surv, uint32_t *clock, uint32_t *back_clock, uint32_t *heads) {
    if (!s || doc >= s->n_handles) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    int rc = HM_OK;
    const DevDoc m = read_doc(s, doc, &rc);
    if (rc) return rc;
    const uint32_t S = s->S;
    if (hist && m.n_c) SCHK(s, hipMemcpy(hist, s->hist + m.c_off, m.n_c * 4, hipMemcpyDeviceToHost));
    if (all_deps && m.n_c) SCHK(s, hipMemcpy(all_deps, s->all_deps + (size_t)m.c_off * S, (size_t)m.n_c * S * 4, hipMemcpyDeviceToHost));
    if ((regs || surv) && m.n_r) {
        // survivor lists may sit anywhere in the op segment's slots (the incremental path moves a
        // list that grows to the end): handed out packed in register order, as a merge writes them
        std::vector<hm_reg_result> rg(m.n_r);
        std::vector<hm_surv_result> sv(m.o_cap ? m.o_cap : 1);
        SCHK(s, hipMemcpy(rg.data(), s->regs + m.r_off, m.n_r * sizeof(hm_reg_result), hipMemcpyDeviceToHost));
        if (m.o_cap) SCHK(s, hipMemcpy(sv.data(), s->surv + m.o_off, m.o_cap * sizeof(hm_surv_result), hipMemcpyDeviceToHost));
        uint32_t off = 0;
        for (uint32_t g = 0; g < m.n_r; g++) {
            hm_reg_result &r = rg[g];
            if ((uint64_t)r.surv_off + r.n_surv > m.o_cap || (uint64_t)off + r.n_surv > m.n_o)
                return hm_engine_fail(s->e, HM_ERR_DEVICE, "register survivors outside the document's slots");
            if (surv) for (uint32_t i = 0; i < r.n_surv; i++) surv[off + i] = sv[r.surv_off + i];
            r.surv_off = off;
            off += r.n_surv;
        }
        if (regs) memcpy(regs, rg.data(), m.n_r * sizeof(hm_reg_result));
    }
    if (clock) SCHK(s, hipMemcpy(clock, s->clock + (size_t)doc * S, S * 4, hipMemcpyDeviceToHost));
    if (back_clock) SCHK(s, hipMemcpy(back_clock, s->back_clock + (size_t)doc * S, S * 4, hipMemcpyDeviceToHost));
    if (heads) SCHK(s, hipMemcpy(heads, s->heads + (size_t)doc * S, S * 4, hipMemcpyDeviceToHost));
    return HM_OK;
}

int hm_doc_log(hm_store *s, uint32_t doc, hm_change_row *changes, hm_dep_row *deps, hm_op_row *ops) {
    if (!s || doc >= s->n_handles) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    int rc = HM_OK;
    const DevDoc m = read_doc(s, doc, &rc);
    if (rc) return rc;
    if (changes && m.n_c) {
        SCHK(s, hipMemcpy(changes, s->changes + m.c_off, m.n_c * sizeof(hm_change_row), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < m.n_c; i++) { changes[i].dep_off -= m.d_off; changes[i].op_first -= m.o_off; }
    }
    if (deps && m.n_d) SCHK(s, hipMemcpy(deps, s->deps + m.d_off, m.n_d * sizeof(hm_dep_row), hipMemcpyDeviceToHost));
    if (ops && m.n_o) SCHK(s, hipMemcpy(ops, s->ops + m.o_off, m.n_o * sizeof(hm_op_row), hipMemcpyDeviceToHost));
    return HM_OK;
}

int hm_store_read_regs(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *regs,
                       hm_reg_result *out_regs, hm_surv_result *out_surv, uint32_t surv_cap, uint32_t *out_n_surv) {
    if (!s || (n && (!doc_handles || !regs || !out_regs || (surv_cap && !out_surv)))) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        if (out_n_surv) *out_n_surv = 0;
        if (!n) return HM_OK;
        hipStream_t st = hm_engine_stream(s->e);
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_h = 0, o_r = al(4 * (size_t)n), o_cnt = o_r + al(4 * (size_t)n), o_regs = o_cnt + 256,
                     o_surv = o_regs + al((size_t)n * sizeof(hm_reg_result)), total = o_surv + al((size_t)surv_cap * sizeof(hm_surv_result) + 1);
        int rc = ensure_stage(s, total);
        if (rc) return rc;
        uint8_t *sp = s->stage.p;
        SCHK(s, hipMemcpyAsync(sp + o_h, doc_handles, (size_t)n * 4, hipMemcpyHostToDevice, st));
        SCHK(s, hipMemcpyAsync(sp + o_r, regs, (size_t)n * 4, hipMemcpyHostToDevice, st));
        SCHK(s, hipMemsetAsync(sp + o_cnt, 0, 8, st));
        SCHK(s, hm_launch_read_regs_h(n, (const uint32_t *)(sp + o_h), (const uint32_t *)(sp + o_r), s->dm, s->n_handles, s->regs,
                                      s->surv, (hm_reg_result *)(sp + o_regs), (hm_surv_result *)(sp + o_surv), surv_cap,
                                      (uint32_t *)(sp + o_cnt), (uint32_t *)(sp + o_cnt) + 1, st));
        uint32_t cb[2] = {0, 0};
        SCHK(s, hipMemcpyAsync(cb, sp + o_cnt, 8, hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        if (cb[1] & 1) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad handle");
        if (cb[1] & 2) return hm_engine_fail(s->e, HM_ERR_INVALID, "register outside its document");
        SCHK(s, hipMemcpy(out_regs, sp + o_regs, (size_t)n * sizeof(hm_reg_result), hipMemcpyDeviceToHost));
        if (out_n_surv) *out_n_surv = cb[0];
        if (cb[0] > surv_cap) return hm_engine_fail(s->e, HM_ERR_NOMEM, "surv_cap below the survivors of the registers");
        if (cb[0]) SCHK(s, hipMemcpy(out_surv, sp + o_surv, (size_t)cb[0] * sizeof(hm_surv_result), hipMemcpyDeviceToHost));
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_read_regs");
    }
}

int hm_store_read_history(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                          const uint32_t *out_off, uint32_t *out_log_index, uint32_t *out_all_deps) {
    if (!s || (n && (!doc_handles || !from || !to || !out_off || !out_log_index))) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        if (!n) return HM_OK;
        for (uint32_t i = 0; i < n; i++)
            if (to[i] < from[i] || out_off[i + 1] - out_off[i] != to[i] - from[i] || out_off[i + 1] < out_off[i])
                return hm_engine_fail(s->e, HM_ERR_INVALID, "history slice rows do not match out_off");
        const uint32_t rows = out_off[n], S = s->S;
        hipStream_t st = hm_engine_stream(s->e);
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_h = 0, o_f = al(4 * (size_t)n), o_t = o_f + al(4 * (size_t)n), o_o = o_t + al(4 * (size_t)n),
                     o_bad = o_o + al(4 * ((size_t)n + 1)), o_log = o_bad + 256, o_ad = o_log + al(4 * (size_t)rows + 4),
                     total = o_ad + (out_all_deps ? al(4 * (size_t)rows * S + 4) : 0);
        int rc = ensure_stage(s, total);
        if (rc) return rc;
        uint8_t *sp = s->stage.p;
        SCHK(s, hipMemcpyAsync(sp + o_h, doc_handles, (size_t)n * 4, hipMemcpyHostToDevice, st));
        SCHK(s, hipMemcpyAsync(sp + o_f, from, (size_t)n * 4, hipMemcpyHostToDevice, st));
        SCHK(s, hipMemcpyAsync(sp + o_t, to, (size_t)n * 4, hipMemcpyHostToDevice, st));
        SCHK(s, hipMemcpyAsync(sp + o_o, out_off, (size_t)n * 4, hipMemcpyHostToDevice, st));
        SCHK(s, hipMemsetAsync(sp + o_bad, 0, 4, st));
        SCHK(s, hipMemsetAsync(sp + o_log, 0xFF, 4 * (size_t)rows + 4, st));
        SCHK(s, hm_launch_read_hist(n, (const uint32_t *)(sp + o_h), (const uint32_t *)(sp + o_f), (const uint32_t *)(sp + o_t),
                                    (const uint32_t *)(sp + o_o), s->dm, s->n_handles, s->hist, s->all_deps, S,
                                    (uint32_t *)(sp + o_log), out_all_deps ? (uint32_t *)(sp + o_ad) : nullptr,
                                    (uint32_t *)(sp + o_bad), st));
        uint32_t bad = 0;
        SCHK(s, hipMemcpyAsync(&bad, sp + o_bad, 4, hipMemcpyDeviceToHost, st));
        if (rows) SCHK(s, hipMemcpyAsync(out_log_index, sp + o_log, 4 * (size_t)rows, hipMemcpyDeviceToHost, st));
        if (rows && out_all_deps) SCHK(s, hipMemcpyAsync(out_all_deps, sp + o_ad, 4 * (size_t)rows * S, hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        if (bad) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad handle");
        for (uint32_t r = 0; r < rows; r++)
            if (out_log_index[r] == HM_NONE) return hm_engine_fail(s->e, HM_ERR_INVALID, "history slice past the history");
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_read_history");
    }
}

int hm_store_blocked(hm_store *s, uint32_t *out_handles, uint32_t cap, uint32_t *out_n) {
    if (!s || !out_n || (cap && !out_handles)) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        *out_n = 0;
        if (!s->n_handles) return HM_OK;
        hipStream_t st = hm_engine_stream(s->e);
        const uint32_t rows = std::min(cap, s->n_handles);
        int rc = ensure_stage(s, 256 + 4 * (size_t)rows + 4);
        if (rc) return rc;
        uint8_t *sp = s->stage.p;
        SCHK(s, hipMemsetAsync(sp, 0, 4, st));
        SCHK(s, hm_launch_blocked(s->res_docs, s->n_handles, (uint32_t *)(sp + 256), rows, (uint32_t *)sp, st));
        SCHK(s, hipMemcpyAsync(&s->h_cnt[6], sp, 4, hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        const uint32_t k = s->h_cnt[6];
        *out_n = k;
        if (k > cap) return hm_engine_fail(s->e, HM_ERR_NOMEM, "cap below the number of blocked documents");
        if (k) {
            SCHK(s, hipMemcpy(out_handles, sp + 256, 4 * (size_t)k, hipMemcpyDeviceToHost));
            std::sort(out_handles, out_handles + k);       // (the waves' blocks land in any order)
        }
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_blocked");
    }
}

// the store as the device queries' document source; the caller sets handles (staged, device)
static DocSource store_source(const hm_store *s) {
    DocSource D = {};
    D.dm = s->dm; D.n_handles = s->n_handles; D.S = s->S;
    D.changes = s->changes; D.hist = s->hist; D.all_deps = s->all_deps; D.deps = s->deps; D.ops = s->ops;
    D.clock = s->clock; D.back_clock = s->back_clock; D.min_clock = s->min_clock;
    D.lim_c = s->cap_c; D.lim_d = s->cap_d; D.lim_o = s->cap_o;
    return D;
}

// hm_store_waiting / hm_store_read_queue: one launch of the waiting pass over the staged requests
static int waiting_impl(hm_store *s, uint32_t n, const uint32_t *doc_handles, uint32_t *out_missing, uint32_t *out_unmet,
                        uint32_t *out_nq, const uint32_t *q_off, uint32_t *out_queue) {
    const uint32_t S = s->S;
    const uint32_t q_rows = q_off ? q_off[n] : 0;
    hipStream_t st = hm_engine_stream(s->e);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t row_b = al(4 * (size_t)n * S);
    const size_t o_h = 0, o_bad = al(4 * (size_t)n), o_off = o_bad + 256, o_nq = o_off + al(4 * ((size_t)n + 1)),
                 o_miss = o_nq + al(4 * (size_t)n), o_unmet = o_miss + (out_missing ? row_b : 0),
                 o_q = o_unmet + (out_unmet ? row_b : 0), total = o_q + al(4 * (size_t)q_rows + 4);
    int rc = ensure_stage(s, total);
    if (rc) return rc;
    uint8_t *sp = s->stage.p;
    SCHK(s, hipMemcpyAsync(sp + o_h, doc_handles, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    if (q_off) SCHK(s, hipMemcpyAsync(sp + o_off, q_off, 4 * ((size_t)n + 1), hipMemcpyHostToDevice, st));
    SCHK(s, hipMemsetAsync(sp + o_bad, 0, 4, st));
    WaitingArgs A;
    A.n = n; A.src = store_source(s); A.src.handles = (const uint32_t *)(sp + o_h);
    A.out_missing = out_missing ? (uint32_t *)(sp + o_miss) : nullptr;
    A.out_unmet = out_unmet ? (uint32_t *)(sp + o_unmet) : nullptr;
    A.out_nq = out_nq ? (uint32_t *)(sp + o_nq) : nullptr;
    A.q_off = q_off ? (const uint32_t *)(sp + o_off) : nullptr;
    A.out_queue = q_off ? (uint32_t *)(sp + o_q) : nullptr;
    A.bad = (uint32_t *)(sp + o_bad);
    SCHK(s, hm_launch_waiting(A, st));
    SCHK(s, hipMemcpyAsync(&s->h_cnt[7], sp + o_bad, 4, hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));
    const uint32_t bad = s->h_cnt[7];
    if (bad & HM_WAIT_BAD_HANDLE) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad handle");
    if (bad & HM_WAIT_BAD_QUEUE) return hm_engine_fail(s->e, HM_ERR_INVALID, "out_off does not match the documents' queue lengths");
    if (out_missing) SCHK(s, hipMemcpyAsync(out_missing, sp + o_miss, 4 * (size_t)n * S, hipMemcpyDeviceToHost, st));
    if (out_unmet) SCHK(s, hipMemcpyAsync(out_unmet, sp + o_unmet, 4 * (size_t)n * S, hipMemcpyDeviceToHost, st));
    if (out_nq) SCHK(s, hipMemcpyAsync(out_nq, sp + o_nq, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    if (q_rows) SCHK(s, hipMemcpyAsync(out_queue, sp + o_q, 4 * (size_t)q_rows, hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));
    return HM_OK;
}

int hm_store_waiting(hm_store *s, uint32_t n, const uint32_t *doc_handles, uint32_t *out_missing, uint32_t *out_unmet_min,
                     uint32_t *out_n_queued) {
    if (!s || (n && !doc_handles)) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        if (!n) return HM_OK;
        return waiting_impl(s, n, doc_handles, out_missing, out_unmet_min, out_n_queued, nullptr, nullptr);
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_waiting");
    }
}

int hm_store_read_queue(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *out_off, uint32_t *out_log_index) {
    if (!s || (n && (!doc_handles || !out_off))) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        if (!n) return HM_OK;
        for (uint32_t i = 0; i < n; i++)
            if (out_off[i + 1] < out_off[i]) return hm_engine_fail(s->e, HM_ERR_INVALID, "out_off must not decrease");
        if (out_off[n] - out_off[0] && !out_log_index) return HM_ERR_INVALID;
        if (out_off[0]) {
            // (rows before out_off[0] are the caller's: stage the offsets from zero)
            std::vector<uint32_t> off(out_off, out_off + n + 1);
            for (auto &x : off) x -= out_off[0];
            return waiting_impl(s, n, doc_handles, nullptr, nullptr, nullptr, off.data(), out_log_index + out_off[0]);
        }
        return waiting_impl(s, n, doc_handles, nullptr, nullptr, nullptr, out_off, out_log_index);
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_read_queue");
    }
}

int hm_store_missing_changes(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *entry_off,
                             const uint16_t *entry_actor, const uint32_t *entry_seq, uint32_t flags, uint32_t *out_closure,
                             uint32_t *out_range, uint32_t *out_log_index, uint32_t cap, uint32_t *out_total) {
    if (!s || !out_total || (n && (!doc_handles || !entry_off || !out_range)) || (cap && !out_log_index)) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        *out_total = 0;
        if (!n) return HM_OK;
        if (flags & ~(HM_MC_RAW | HM_MC_ONLY_LISTED)) return hm_engine_fail(s->e, HM_ERR_INVALID, "unknown HM_MC_* flag");
        if (entry_off[0]) return hm_engine_fail(s->e, HM_ERR_INVALID, "entry_off must start at 0");
        for (uint32_t i = 0; i < n; i++)
            if (entry_off[i + 1] < entry_off[i]) return hm_engine_fail(s->e, HM_ERR_INVALID, "entry_off must not decrease");
        const uint32_t ne = entry_off[n];
        if (ne && (!entry_actor || !entry_seq)) return HM_ERR_INVALID;
        const uint32_t S = s->S;
        hipStream_t st = hm_engine_stream(s->e);
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_cnt = 0, o_h = 256, o_off = o_h + al(4 * (size_t)n), o_ea = o_off + al(4 * ((size_t)n + 1)),
                     o_es = o_ea + al(2 * (size_t)ne + 2), o_rng = o_es + al(4 * (size_t)ne + 4), o_cl = o_rng + al(8 * (size_t)n),
                     o_log = o_cl + (out_closure ? al(4 * (size_t)n * S) : 0), total = o_log + al(4 * (size_t)cap + 4);
        int rc = ensure_stage(s, total);
        if (rc) return rc;
        uint8_t *sp = s->stage.p;
        SCHK(s, hipMemsetAsync(sp + o_cnt, 0, 8, st));        // (total, bad)
        SCHK(s, hipMemcpyAsync(sp + o_h, doc_handles, 4 * (size_t)n, hipMemcpyHostToDevice, st));
        SCHK(s, hipMemcpyAsync(sp + o_off, entry_off, 4 * ((size_t)n + 1), hipMemcpyHostToDevice, st));
        if (ne) {
            SCHK(s, hipMemcpyAsync(sp + o_ea, entry_actor, 2 * (size_t)ne, hipMemcpyHostToDevice, st));
            SCHK(s, hipMemcpyAsync(sp + o_es, entry_seq, 4 * (size_t)ne, hipMemcpyHostToDevice, st));
        }
        ChangesArgs A = {};
        A.n = n; A.src = store_source(s); A.src.handles = (const uint32_t *)(sp + o_h);
        A.entry_off = (const uint32_t *)(sp + o_off); A.entry_actor = (const uint16_t *)(sp + o_ea);
        A.entry_seq = (const uint32_t *)(sp + o_es); A.n_entries = ne; A.flags = flags;
        A.out_closure = out_closure ? (uint32_t *)(sp + o_cl) : nullptr;
        A.out_range = (uint32_t *)(sp + o_rng); A.out_log = (uint32_t *)(sp + o_log); A.cap = cap;
        A.total = (uint32_t *)(sp + o_cnt); A.bad = (uint32_t *)(sp + o_cnt + 4);
        SCHK(s, hm_launch_missing_changes(A, st));
        SCHK(s, hipMemcpyAsync(&s->h_cnt[8], sp + o_cnt, 8, hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        const uint32_t tot = s->h_cnt[8], bad = s->h_cnt[9];
        if (bad & HM_MC_BAD_HANDLE) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad handle");
        if (bad & HM_MC_BAD_RANK) return hm_engine_fail(s->e, HM_ERR_INVALID, "entry actor rank outside the store's a_stride");
        if (bad & HM_MC_BAD_REPEAT) return hm_engine_fail(s->e, HM_ERR_INVALID, "actor rank repeated within a request");
        if (bad) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad entry_off");
        *out_total = tot;
        SCHK(s, hipMemcpyAsync(out_range, sp + o_rng, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
        if (out_closure) SCHK(s, hipMemcpyAsync(out_closure, sp + o_cl, 4 * (size_t)n * S, hipMemcpyDeviceToHost, st));
        if (tot && tot <= cap) SCHK(s, hipMemcpyAsync(out_log_index, sp + o_log, 4 * (size_t)tot, hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        if (tot > cap) return hm_engine_fail(s->e, HM_ERR_NOMEM, "cap below the rows of the missing changes");
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_missing_changes");
    }
}

int hm_store_fields(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *entry_off,
                    const uint16_t *entry_actor, const uint32_t *entry_seq, const uint32_t *field_off,
                    const uint32_t *field_reg, uint32_t *out_flags, uint32_t *out_closure, uint32_t *out_range,
                    hm_field_op *out_rows, uint32_t cap, uint32_t *out_total) {
    if (!s || !out_total || (n && (!doc_handles || !entry_off || !field_off || !out_flags)) || (cap && !out_rows)) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        *out_total = 0;
        if (!n) return HM_OK;
        if (entry_off[0]) return hm_engine_fail(s->e, HM_ERR_INVALID, "entry_off must start at 0");
        if (field_off[0]) return hm_engine_fail(s->e, HM_ERR_INVALID, "field_off must start at 0");
        for (uint32_t i = 0; i < n; i++) {
            if (entry_off[i + 1] < entry_off[i]) return hm_engine_fail(s->e, HM_ERR_INVALID, "entry_off must not decrease");
            if (field_off[i + 1] < field_off[i]) return hm_engine_fail(s->e, HM_ERR_INVALID, "field_off must not decrease");
        }
        const uint32_t ne = entry_off[n], nf = field_off[n];
        if ((ne && (!entry_actor || !entry_seq)) || (nf && (!field_reg || !out_range))) return HM_ERR_INVALID;
        const uint32_t S = s->S;
        hipStream_t st = hm_engine_stream(s->e);
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_cnt = 0, o_h = 256, o_eo = o_h + al(4 * (size_t)n), o_ea = o_eo + al(4 * ((size_t)n + 1)),
                     o_es = o_ea + al(2 * (size_t)ne + 2), o_fo = o_es + al(4 * (size_t)ne + 4), o_fr = o_fo + al(4 * ((size_t)n + 1)),
                     o_fl = o_fr + al(4 * (size_t)nf + 4), o_rng = o_fl + al(4 * (size_t)n), o_cl = o_rng + al(8 * (size_t)nf + 8),
                     o_rows = o_cl + (out_closure ? al(4 * (size_t)n * S) : 0), total = o_rows + al(sizeof(hm_field_op) * (size_t)cap + 8);
        int rc = ensure_stage(s, total);
        if (rc) return rc;
        uint8_t *sp = s->stage.p;
        SCHK(s, hipMemsetAsync(sp + o_cnt, 0, 8, st));        // (total, bad)
        SCHK(s, hipMemcpyAsync(sp + o_h, doc_handles, 4 * (size_t)n, hipMemcpyHostToDevice, st));
        SCHK(s, hipMemcpyAsync(sp + o_eo, entry_off, 4 * ((size_t)n + 1), hipMemcpyHostToDevice, st));
        SCHK(s, hipMemcpyAsync(sp + o_fo, field_off, 4 * ((size_t)n + 1), hipMemcpyHostToDevice, st));
        if (ne) {
            SCHK(s, hipMemcpyAsync(sp + o_ea, entry_actor, 2 * (size_t)ne, hipMemcpyHostToDevice, st));
            SCHK(s, hipMemcpyAsync(sp + o_es, entry_seq, 4 * (size_t)ne, hipMemcpyHostToDevice, st));
        }
        if (nf) SCHK(s, hipMemcpyAsync(sp + o_fr, field_reg, 4 * (size_t)nf, hipMemcpyHostToDevice, st));
        FieldArgs A = {};
        A.n = n; A.src = store_source(s); A.src.handles = (const uint32_t *)(sp + o_h);
        A.regs = s->regs; A.surv = s->surv; A.lim_r = s->cap_r;
        A.entry_off = (const uint32_t *)(sp + o_eo); A.entry_actor = (const uint16_t *)(sp + o_ea);
        A.entry_seq = (const uint32_t *)(sp + o_es); A.n_entries = ne;
        A.field_off = (const uint32_t *)(sp + o_fo); A.field_reg = (const uint32_t *)(sp + o_fr); A.n_fields = nf;
        A.out_flags = (uint32_t *)(sp + o_fl); A.out_closure = out_closure ? (uint32_t *)(sp + o_cl) : nullptr;
        A.out_range = (uint32_t *)(sp + o_rng); A.out_rows = (hm_field_op *)(sp + o_rows); A.cap = cap;
        A.total = (uint32_t *)(sp + o_cnt); A.bad = (uint32_t *)(sp + o_cnt + 4);
        SCHK(s, hm_launch_fields(A, st));
        // the per-request outputs travel with the counters; a small row table too, whole, so that the
        // latency path (one request, a guessed table) waits for the device once
        const bool whole = cap && sizeof(hm_field_op) * (size_t)cap <= 65536;
        SCHK(s, hipMemcpyAsync(&s->h_cnt[8], sp + o_cnt, 8, hipMemcpyDeviceToHost, st));
        SCHK(s, hipMemcpyAsync(out_flags, sp + o_fl, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        if (nf) SCHK(s, hipMemcpyAsync(out_range, sp + o_rng, 8 * (size_t)nf, hipMemcpyDeviceToHost, st));
        if (out_closure) SCHK(s, hipMemcpyAsync(out_closure, sp + o_cl, 4 * (size_t)n * S, hipMemcpyDeviceToHost, st));
        if (whole) SCHK(s, hipMemcpyAsync(out_rows, sp + o_rows, sizeof(hm_field_op) * (size_t)cap, hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        const uint32_t tot = s->h_cnt[8], bad = s->h_cnt[9];
        if (bad & HM_FD_BAD_HANDLE) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad handle");
        if (bad & HM_FD_BAD_RANK) return hm_engine_fail(s->e, HM_ERR_INVALID, "entry actor rank outside the store's a_stride");
        if (bad & HM_FD_BAD_REPEAT) return hm_engine_fail(s->e, HM_ERR_INVALID, "actor rank repeated within a request");
        if (bad) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad entry_off or field_off");
        *out_total = tot;
        if (tot > cap) return hm_engine_fail(s->e, HM_ERR_NOMEM, "cap below the rows of the fields");
        if (tot && !whole) {
            SCHK(s, hipMemcpyAsync(out_rows, sp + o_rows, sizeof(hm_field_op) * (size_t)tot, hipMemcpyDeviceToHost, st));
            SCHK(s, hipStreamSynchronize(st));
        }
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_fields");
    }
}

static_assert(sizeof(PlanStats) >= sizeof(hm_past_summary), "the summary is read back through h_st");

// The count pass of n staged requests: handles and the selector go to the stage buffer, the counts,
// offsets and summary stay there (P.cnt / P.off / P.sum); *sum = the summary, read back.
// order: the actor-major order rows (staged too); dst: a fork's destination handles, staged
// (*dst_dev) and checked on the device before the one read-back.  have: the clock selector's lower
// bound rows (staged); merge_totals: the destinations are a merge's, checked against their stated
// totals ([4n], staged, *tot_dev) instead of for emptiness.
static int past_count(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *hist_len,
                      const uint32_t *clock_rows, PastArgs &P, hm_past_summary *sum, const uint32_t *order = nullptr,
                      const uint32_t *dst = nullptr, const uint32_t **dst_dev = nullptr, const uint32_t *have = nullptr,
                      const uint32_t *merge_totals = nullptr, const uint32_t **tot_dev = nullptr) {
    const uint32_t S = s->S;
    hipStream_t st = hm_engine_stream(s->e);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t sel_b = hist_len ? 4 * (size_t)n : 4 * (size_t)n * S;
    const size_t o_sum = 0, o_h = 256, o_sel = o_h + al(4 * (size_t)n), o_cnt = o_sel + al(sel_b), o_off = o_cnt + al(16 * (size_t)n),
                 o_aux = o_off + al(16 * (size_t)n), o_part = o_aux + al(8 * (size_t)n),
                 o_ord = o_part + al((size_t)hm_past_scan_chunks(n) * HM_PAST_PART * 8),
                 o_dst = o_ord + (order ? al(4 * (size_t)n * S) : 0), o_have = o_dst + (dst ? al(4 * (size_t)n) : 0),
                 o_tot = o_have + (have ? al(4 * (size_t)n * S) : 0), total = o_tot + (merge_totals ? al(16 * (size_t)n) : 0);
    int rc = ensure_stage(s, total);
    if (rc) return rc;
    uint8_t *sp = s->stage.p;
    SCHK(s, hipMemcpyAsync(sp + o_h, doc_handles, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    SCHK(s, hipMemcpyAsync(sp + o_sel, hist_len ? hist_len : clock_rows, sel_b, hipMemcpyHostToDevice, st));
    if (order) SCHK(s, hipMemcpyAsync(sp + o_ord, order, 4 * (size_t)n * S, hipMemcpyHostToDevice, st));
    if (dst) SCHK(s, hipMemcpyAsync(sp + o_dst, dst, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    if (have) SCHK(s, hipMemcpyAsync(sp + o_have, have, 4 * (size_t)n * S, hipMemcpyHostToDevice, st));
    if (merge_totals) SCHK(s, hipMemcpyAsync(sp + o_tot, merge_totals, 16 * (size_t)n, hipMemcpyHostToDevice, st));
    P = PastArgs{};
    P.n = n; P.src = store_source(s); P.src.handles = (const uint32_t *)(sp + o_h);
    if (hist_len) P.hist_len = (const uint32_t *)(sp + o_sel); else P.clock_rows = (const uint32_t *)(sp + o_sel);
    if (order) P.order = (const uint32_t *)(sp + o_ord);
    if (have) P.have_rows = (const uint32_t *)(sp + o_have);
    P.cnt = (uint32_t *)(sp + o_cnt); P.off = (uint32_t *)(sp + o_off); P.aux = (uint32_t *)(sp + o_aux);
    P.part = (unsigned long long *)(sp + o_part);
    P.sum = (hm_past_summary *)(sp + o_sum);
    SCHK(s, hm_launch_past_count(P, st));
    if (dst) {
        const uint32_t stamp_src = ++s->stamp ? s->stamp : ++s->stamp, stamp_dst = ++s->stamp ? s->stamp : ++s->stamp;
        if (merge_totals) {
            SCHK(s, hm_launch_merge_check(P.src.handles, (const uint32_t *)(sp + o_dst), (const uint32_t *)(sp + o_tot), n,
                                          s->n_handles, S, s->dm, s->seen, stamp_src, stamp_dst, &P.sum->bad, st));
            *tot_dev = (const uint32_t *)(sp + o_tot);
        } else {
            SCHK(s, hm_launch_fork_check(P.src.handles, (const uint32_t *)(sp + o_dst), n, s->n_handles, s->dm, s->seen, stamp_src,
                                         stamp_dst, &P.sum->bad, st));
        }
        *dst_dev = (const uint32_t *)(sp + o_dst);
    }
    SCHK(s, hipMemcpyAsync(s->h_st, P.sum, sizeof(hm_past_summary), hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));
    memcpy(sum, s->h_st, sizeof *sum);
    if (sum->bad & HM_PAST_BAD_HANDLE) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad handle");
    if ((sum->bad & HM_FORK_BAD_DST) && merge_totals)
        return hm_engine_fail(s->e, HM_ERR_INVALID, "a merge's destination is outside the store, repeated, a source, or its stated totals are below its current ones or above a_stride");
    if (sum->bad & HM_FORK_BAD_DST)
        return hm_engine_fail(s->e, HM_ERR_INVALID, "a fork's destination is outside the store, repeated, a source or not empty");
    if (sum->bad & HM_PAST_BAD_ORDER)
        return hm_engine_fail(s->e, HM_ERR_INVALID, "actor order row: a rank outside the document, repeated, or an actor of the clock not listed");
    if (sum->bad) return hm_engine_fail(s->e, HM_ERR_INVALID, "a change row outside its document's segments");
    return HM_OK;
}

int hm_store_past_sizes(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *hist_len,
                        const uint32_t *clock_rows, uint32_t *out_counts, uint64_t *out_totals) {
    if (!s || (n && !doc_handles)) return HM_ERR_INVALID;
    if ((hist_len != nullptr) == (clock_rows != nullptr))
        return hm_engine_fail(s->e, HM_ERR_INVALID, "exactly one of hist_len and clock_rows");
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        if (!n) { if (out_totals) memset(out_totals, 0, 4 * sizeof(uint64_t)); return HM_OK; }
        PastArgs P;
        hm_past_summary sum;
        int rc = past_count(s, n, doc_handles, hist_len, clock_rows, P, &sum);
        if (rc) return rc;
        if (out_totals) memcpy(out_totals, sum.totals, sizeof sum.totals);
        if (out_counts) {
            hipStream_t st = hm_engine_stream(s->e);
            SCHK(s, hipMemcpyAsync(out_counts, P.cnt, 16 * (size_t)n, hipMemcpyDeviceToHost, st));
            SCHK(s, hipStreamSynchronize(st));
        }
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_past_sizes");
    }
}

int hm_store_materialize(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *hist_len,
                         const uint32_t *clock_rows, const hm_past_out *out, uint64_t *out_totals) {
    if (!out) return HM_ERR_INVALID;
    return hm_store_materialize_sized(s, n, doc_handles, hist_len, clock_rows,
                                      [](void *ctx, const uint64_t *) { return (const hm_past_out *)ctx; }, (void *)out, out_totals);
}

// The gathered batch of a count pass, placed in the store's own buffer: the slots [docs][changes][deps]
// [ops][change_log][op_log], the caller's n_extra slots behind them (one with a host source is copied up
// first), the fill.  sz / o: every slot's bytes and place in s->past; b: tables, counts and a_stride.
struct Gathered {
    size_t sz[17], o[17];
    hm_batch b;
};

static int place_gathered(hm_store *s, PastArgs &P, uint32_t n, const uint64_t *tot, int n_extra, const size_t *extra_sz,
                          const void *const *extra_host, Gathered &G) {
    const uint64_t tc = tot[0], td = tot[1], to = tot[2], tr = tot[3];
    if (std::max(std::max(tc, td), std::max(to, tr)) > 0xFFFFFFFFull)
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "a call's rows stay below 2^32");
    hipStream_t st = hm_engine_stream(s->e);
    const size_t head[6] = {n * sizeof(hm_doc_row), tc * sizeof(hm_change_row), td * sizeof(hm_dep_row), to * sizeof(hm_op_row), tc * 4, to * 4};
    size_t total = 0;
    for (int i = 0; i < 6 + n_extra; i++) { G.sz[i] = i < 6 ? head[i] : extra_sz[i - 6]; G.o[i] = total; total += (G.sz[i] + 1 + 255) & ~(size_t)255; }
    const int rc = ensure_buf(s, s->past, total);
    if (rc) return rc;
    uint8_t *bp = s->past.p;
    for (int i = 6; extra_host && i < 6 + n_extra; i++)
        if (extra_host[i - 6] && G.sz[i]) SCHK(s, hipMemcpyAsync(bp + G.o[i], extra_host[i - 6], G.sz[i], hipMemcpyHostToDevice, st));
    P.cap[0] = (uint32_t)tc; P.cap[1] = (uint32_t)td; P.cap[2] = (uint32_t)to; P.cap[3] = (uint32_t)tr;
    P.out_docs = (hm_doc_row *)(bp + G.o[0]); P.out_changes = (hm_change_row *)(bp + G.o[1]); P.out_deps = (hm_dep_row *)(bp + G.o[2]);
    P.out_ops = (hm_op_row *)(bp + G.o[3]); P.out_change_log = (uint32_t *)(bp + G.o[4]); P.out_op_log = (uint32_t *)(bp + G.o[5]);
    SCHK(s, hm_launch_past_fill(P, st));
    G.b = hm_batch{};
    G.b.a_stride = s->S; G.b.n_docs = n; G.b.n_changes = (uint32_t)tc; G.b.n_deps = (uint32_t)td; G.b.n_ops = (uint32_t)to;
    G.b.docs = P.out_docs; G.b.changes = P.out_changes; G.b.deps = P.out_deps; G.b.ops = P.out_ops;
    return HM_OK;
}

// the fork (or merge) batch now in flight: what hm_store_fork_rows reads until the wait
static void note_fork(hm_store *s, uint64_t id, uint32_t n, const uint64_t *tot, const Gathered &G) {
    s->fork_id = id; s->fork_n = n;
    for (int i = 0; i < 3; i++) s->fork_rows[i] = (size_t)tot[i];
    for (int i = 0; i < 6; i++) s->fork_off[i] = G.o[i];
}

// Fork: count, scan and fill into the store's own buffer, then the device-table submit of those
// tables to the destinations.  The gathered rows (and the staged destination handles, copied behind
// them) stay untouched until the wait: every call that would reuse the buffer is refused while the
// batch is in flight.
int hm_store_fork_submit(hm_store *s, uint32_t n, const uint32_t *src_handles, const uint32_t *hist_len,
                         const uint32_t *clock_rows, const uint32_t *actor_order, const uint32_t *dst_handles, uint32_t flags,
                         uint64_t *out_batch_id) {
    if (!s || !n || !src_handles || !dst_handles) return HM_ERR_INVALID;
    if ((hist_len != nullptr) == (clock_rows != nullptr))
        return hm_engine_fail(s->e, HM_ERR_INVALID, "exactly one of hist_len and clock_rows");
    if (actor_order && !clock_rows) return hm_engine_fail(s->e, HM_ERR_INVALID, "an actor order goes with a clock, not a history length");
    if (flags & ~HM_FORK_MIN_CLOCK) return hm_engine_fail(s->e, HM_ERR_INVALID, "unknown fork flags");
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "a batch is already in flight (call hm_batch_wait)");
    try {
        const uint32_t S = s->S;
        SCHK(s, hipSetDevice(hm_engine_device(s->e)));
        hipStream_t st = hm_engine_stream(s->e);
        PastArgs P;
        hm_past_summary sum;
        const uint32_t *dst_staged = nullptr;
        int rc = past_count(s, n, src_handles, hist_len, clock_rows, P, &sum, actor_order, dst_handles, &dst_staged);
        if (rc) return rc;
        // [the gathered batch][destination handles]
        // (the fill, the copy and the min-clock kernel below still read the stage buffer — handles, counts,
        // offsets, order rows — when the submit stages its own rows there: they are enqueued first on the
        // same stream, and a stage buffer that has to grow is freed only after ensure_buf has synchronised
        // that stream)
        const size_t extra[1] = {(size_t)n * 4};
        Gathered G;
        if ((rc = place_gathered(s, P, n, sum.totals, 1, extra, nullptr, G))) return rc;
        uint32_t *dst_dev = (uint32_t *)(s->past.p + G.o[6]);
        SCHK(s, hipMemcpyAsync(dst_dev, dst_staged, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        // (the destinations passed the check: empty documents, whose minimumClock row no result shows)
        SCHK(s, hm_launch_fork_min_clock(P.src.handles, dst_dev, n, S, s->dm, s->min_clock, flags & HM_FORK_MIN_CLOCK ? 1u : 0u, st));
        G.b.n_regs = (uint32_t)sum.totals[3];
        uint64_t id = 0;
        if ((rc = hm_batch_submit_device(s, &G.b, dst_dev, nullptr, &id))) return rc;
        note_fork(s, id, n, sum.totals, G);
        if (out_batch_id) *out_batch_id = id;
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_fork_submit");
    }
}

// Merge into documents that hold changes: count, scan and the destination check, fill into the
// store's buffer, the rename pass over the filled tables (the maps staged behind them), then the
// device-table submit to the destinations with their remap rows.  Two read-backs: the totals with
// the count's verdicts, the rename's verdict.
int hm_store_merge_from_submit(hm_store *s, uint32_t n, const uint32_t *src_handles, const uint32_t *have_rows,
                               const uint32_t *clock_rows, const uint32_t *actor_order, const uint32_t *dst_handles,
                               const hm_merge_maps *maps, const uint8_t *dst_actor_remap, uint64_t *out_batch_id) {
    if (!s || !n || !src_handles || !dst_handles || !maps) return HM_ERR_INVALID;
    if (!clock_rows) return hm_engine_fail(s->e, HM_ERR_INVALID, "a merge selects by a clock (clock_rows)");
    if (!maps->totals || !maps->rank || !maps->obj_off || !maps->reg_off || (maps->str_map && !maps->str_off) ||
        (maps->content_map && !maps->content_off))
        return hm_engine_fail(s->e, HM_ERR_INVALID, "hm_merge_maps: totals, rank and the object and register maps are required");
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "a batch is already in flight (call hm_batch_wait)");
    try {
        const uint32_t S = s->S;
        // the CSR offsets start at 0 and do not decrease; a map with entries has its table
        const uint32_t *offs[4] = {maps->obj_off, maps->reg_off, maps->str_map ? maps->str_off : nullptr,
                                   maps->content_map ? maps->content_off : nullptr};
        const uint32_t *tabs[4] = {maps->obj_map, maps->reg_map, maps->str_map, maps->content_map};
        for (int k = 0; k < 4; k++) {
            if (!offs[k]) continue;
            if (offs[k][0]) return hm_engine_fail(s->e, HM_ERR_INVALID, "hm_merge_maps: an offset table must start at 0");
            for (uint32_t i = 0; i < n; i++)
                if (offs[k][i + 1] < offs[k][i]) return hm_engine_fail(s->e, HM_ERR_INVALID, "hm_merge_maps: an offset table must not decrease");
            if (offs[k][n] && !tabs[k]) return hm_engine_fail(s->e, HM_ERR_INVALID, "hm_merge_maps: a map table is missing");
        }
        SCHK(s, hipSetDevice(hm_engine_device(s->e)));
        hipStream_t st = hm_engine_stream(s->e);
        PastArgs P;
        hm_past_summary sum;
        const uint32_t *dst_staged = nullptr, *tot_staged = nullptr;
        int rc = past_count(s, n, src_handles, nullptr, clock_rows, P, &sum, actor_order, dst_handles, &dst_staged, have_rows,
                            maps->totals, &tot_staged);
        if (rc) return rc;
        // [the gathered batch][destination handles][remap rows][rank rows]
        // [obj_off][obj_map][reg_off][reg_map][str_off][str_map][content_off][content_map]
        const size_t offb = ((size_t)n + 1) * 4;
        const size_t extra[11] = {(size_t)n * 4, dst_actor_remap ? (size_t)n * S : 0, (size_t)n * S * 4,
                                  offb, (size_t)offs[0][n] * 4, offb, (size_t)offs[1][n] * 4,
                                  offs[2] ? offb : 0, offs[2] ? (size_t)offs[2][n] * 4 : 0,
                                  offs[3] ? offb : 0, offs[3] ? (size_t)offs[3][n] * 4 : 0};
        const void *host[11] = {nullptr, dst_actor_remap, maps->rank, offs[0], tabs[0], offs[1], tabs[1], offs[2], tabs[2],
                                offs[3], tabs[3]};
        Gathered G;
        if ((rc = place_gathered(s, P, n, sum.totals, 11, extra, host, G))) return rc;
        const size_t *o = G.o;
        uint8_t *bp = s->past.p;
        uint32_t *dst_dev = (uint32_t *)(bp + o[6]);
        SCHK(s, hipMemcpyAsync(dst_dev, dst_staged, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        RenameArgs R = {};
        R.n = n; R.S = S; R.cnt = P.cnt; R.off = P.off;
        R.docs = P.out_docs; R.changes = P.out_changes; R.deps = P.out_deps; R.ops = P.out_ops;
        R.totals = tot_staged; R.rank = (const uint32_t *)(bp + o[8]);
        R.obj_off = (const uint32_t *)(bp + o[9]); R.obj_map = (const uint32_t *)(bp + o[10]);
        R.reg_off = (const uint32_t *)(bp + o[11]); R.reg_map = (const uint32_t *)(bp + o[12]);
        if (offs[2]) { R.str_off = (const uint32_t *)(bp + o[13]); R.str_map = (const uint32_t *)(bp + o[14]); }
        if (offs[3]) { R.cid_off = (const uint32_t *)(bp + o[15]); R.cid_map = (const uint32_t *)(bp + o[16]); }
        R.bad = &P.sum->bad;
        SCHK(s, hm_launch_past_rename(R, st));
        // the rename's verdict: the second read-back (the stage buffer is free for the submit afterwards)
        SCHK(s, hipMemcpyAsync(s->h_st, P.sum, sizeof(hm_past_summary), hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        memcpy(&sum, s->h_st, sizeof sum);
        if (sum.bad & HM_PAST_BAD_MAP)
            return hm_engine_fail(s->e, HM_ERR_INVALID, "a merge map: an id beyond its slice, an entry of HM_NONE, or an image beyond the stated totals");
        uint64_t id = 0;
        if ((rc = hm_batch_submit_device(s, &G.b, dst_dev, dst_actor_remap ? bp + o[7] : nullptr, &id))) return rc;
        note_fork(s, id, n, sum.totals, G);
        if (out_batch_id) *out_batch_id = id;
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_merge_from_submit");
    }
}

}  // extern "C"

// (engine_internal.h) the tables a fork batch in flight gathered, for a host that mirrors the forks'
// logs (the docset): request i's rows are out_docs[i]'s ranges, op_log[k] = the parent's log op index
// of gathered op k.  ops may be NULL (a host that holds the parents' op rows takes them through
// op_log).  Only between the fork's submit and its wait.
int hm_store_fork_rows(hm_store *s, uint64_t batch_id, std::vector<hm_doc_row> &docs, std::vector<hm_change_row> &changes,
                       std::vector<hm_op_row> *ops, std::vector<uint32_t> &op_log) {
    if (!s) return HM_ERR_INVALID;
    if (!s->pending || !batch_id || batch_id != s->pending_id || batch_id != s->fork_id)
        return hm_engine_fail(s->e, HM_ERR_INVALID, "hm_store_fork_rows: not the fork batch in flight");
    try {
        hipStream_t st = hm_engine_stream(s->e);
        docs.resize(s->fork_n); changes.resize(s->fork_rows[0]); op_log.resize(s->fork_rows[2]);
        if (ops) ops->resize(s->fork_rows[2]);
        const uint8_t *bp = s->past.p;
        void *dst[4] = {docs.data(), changes.data(), ops ? ops->data() : nullptr, op_log.data()};
        const size_t sz[4] = {docs.size() * sizeof(hm_doc_row), changes.size() * sizeof(hm_change_row),
                              ops ? ops->size() * sizeof(hm_op_row) : 0, op_log.size() * 4};
        const size_t at[4] = {s->fork_off[0], s->fork_off[1], s->fork_off[3], s->fork_off[5]};
        for (int i = 0; i < 4; i++)
            if (sz[i]) SCHK(s, hipMemcpyAsync(dst[i], bp + at[i], sz[i], hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_fork_rows");
    }
}

// (engine_internal.h) the DocBackend.clock rows of n documents, out[i * S ..], with one synchronise
int hm_store_back_clocks(hm_store *s, uint32_t n, const uint32_t *doc_handles, uint32_t *out) {
    if (!s || (n && (!doc_handles || !out))) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        const uint32_t S = s->S;
        hipStream_t st = hm_engine_stream(s->e);
        for (uint32_t i = 0; i < n; i++) {
            if (doc_handles[i] >= s->n_handles) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad handle");
            SCHK(s, hipMemcpyAsync(out + (size_t)i * S, s->back_clock + (size_t)doc_handles[i] * S, (size_t)S * 4, hipMemcpyDeviceToHost, st));
        }
        SCHK(s, hipStreamSynchronize(st));
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_back_clocks");
    }
}

// (engine_internal.h) the outputs are asked for once the count pass has sized them: one count pass
// for a caller that allocates by the totals
int hm_store_materialize_sized(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *hist_len,
                               const uint32_t *clock_rows, hm_past_alloc alloc, void *ctx, uint64_t *out_totals) {
    if (!s || !alloc || (n && !doc_handles)) return HM_ERR_INVALID;
    if ((hist_len != nullptr) == (clock_rows != nullptr))
        return hm_engine_fail(s->e, HM_ERR_INVALID, "exactly one of hist_len and clock_rows");
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        if (!n) { if (out_totals) memset(out_totals, 0, 4 * sizeof(uint64_t)); return HM_OK; }
        const uint32_t S = s->S;
        hipStream_t st = hm_engine_stream(s->e);
        PastArgs P;
        hm_past_summary sum;
        int rc = past_count(s, n, doc_handles, hist_len, clock_rows, P, &sum);
        if (rc) return rc;
        if (out_totals) memcpy(out_totals, sum.totals, sizeof sum.totals);
        const uint64_t tc = sum.totals[0], td = sum.totals[1], to = sum.totals[2], tr = sum.totals[3];
        const hm_past_out *out = alloc(ctx, sum.totals);
        if (!out) return hm_engine_fail(s->e, HM_ERR_NOMEM, "no outputs for the materialized documents");
        const hm_results &R = out->res;
        // a table nobody asked for needs no capacity
        const bool want_c = out->changes || out->change_log || R.hist || R.all_deps, want_d = out->deps != nullptr,
                   want_o = out->ops || out->op_log || R.surv, want_r = R.regs != nullptr;
        if ((want_c && tc > out->cap_changes) || (want_d && td > out->cap_deps) || (want_o && to > out->cap_ops) ||
            (want_r && tr > out->cap_regs))
            return hm_engine_fail(s->e, HM_ERR_NOMEM, "a capacity below the rows of the materialized documents");
        // [the gathered batch], then its merge's tables
        const size_t extra[8] = {n * sizeof(hm_doc_result), (size_t)n * S * 4, (size_t)n * S * 4, (size_t)n * S * 4,
                                 (size_t)tc * 4, (size_t)tc * S * 4, (size_t)tr * sizeof(hm_reg_result), (size_t)to * sizeof(hm_surv_result)};
        Gathered G;
        if ((rc = place_gathered(s, P, n, sum.totals, 8, extra, nullptr, G))) return rc;
        const size_t *sz = G.sz, *o = G.o;
        uint8_t *bp = s->past.p;
        hm_batch &b = G.b;
        b.n_regs = (uint32_t)tr;
        b.max_changes = sum.max_changes; b.max_ops = sum.max_ops; b.max_regs = sum.max_regs; b.max_objs = sum.max_objs;
        b.max_deps = sum.max_deps; b.doc_flags = sum.doc_flags;
        if (!b.max_changes && !b.max_ops && !b.max_regs && !b.max_objs) b.max_objs = 1;   // device hints present
        hm_results d;
        d.docs = (hm_doc_result *)(bp + o[6]); d.clock = (uint32_t *)(bp + o[7]); d.back_clock = (uint32_t *)(bp + o[8]);
        d.heads = (uint32_t *)(bp + o[9]); d.hist = (int32_t *)(bp + o[10]); d.all_deps = (uint32_t *)(bp + o[11]);
        d.regs = (hm_reg_result *)(bp + o[12]); d.surv = (hm_surv_result *)(bp + o[13]);
        if ((rc = hm_engine_launch_merge(s->e, &b, &d, nullptr, nullptr))) return rc;
        void *dst[14] = {out->docs, out->changes, out->deps, out->ops, out->change_log, out->op_log, R.docs, R.clock, R.back_clock,
                         R.heads, R.hist, R.all_deps, R.regs, R.surv};
        for (int i = 0; i < 14; i++)
            if (dst[i] && sz[i]) SCHK(s, hipMemcpyAsync(dst[i], bp + o[i], sz[i], hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_materialize");
    }
}

// n op-diff requests staged: handles and ranges (clock_rows != NULL: the clock table [n * a_stride]
// instead, from / to unused) go to the stage buffer, where the counts, offsets and
// summary will stay (A.cnt / A.off / A.aux / A.sum); the largest requested document sizes a wave's
// slice of the chains' work memory (A.slice_words, A.waves; A.work is the caller's to place).
static int op_diff_stage(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                         const uint32_t *clock_rows, uint32_t opts, OpDiffArgs &A) {
    hipStream_t st = hm_engine_stream(s->e);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t sel_b = clock_rows ? 4 * (size_t)n * s->S : 4 * (size_t)n;
    const size_t o_sum = 0, o_need = 128, o_h = 256, o_from = o_h + al(4 * (size_t)n), o_to = o_from + al(sel_b),
                 o_cnt = o_to + al(4 * (size_t)n), o_off = o_cnt + al(16 * (size_t)n), o_aux = o_off + al(16 * (size_t)n),
                 o_part = o_aux + al(8 * (size_t)n), total = o_part + al((size_t)hm_past_scan_chunks(n) * HM_PAST_PART * 8);
    int rc = ensure_stage(s, total);
    if (rc) return rc;
    uint8_t *sp = s->stage.p;
    SCHK(s, hipMemcpyAsync(sp + o_h, doc_handles, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    SCHK(s, hipMemcpyAsync(sp + o_from, clock_rows ? clock_rows : from, sel_b, hipMemcpyHostToDevice, st));
    if (!clock_rows) SCHK(s, hipMemcpyAsync(sp + o_to, to, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    SCHK(s, hipMemsetAsync(sp + o_need, 0, 16, st));
    A = OpDiffArgs{};
    A.n = n; A.src = store_source(s); A.src.handles = (const uint32_t *)(sp + o_h);
    A.opts = opts;
    if (clock_rows) A.clock = (const uint32_t *)(sp + o_from);
    else { A.from = (const uint32_t *)(sp + o_from); A.to = (const uint32_t *)(sp + o_to); }
    A.cnt = (uint32_t *)(sp + o_cnt); A.off = (uint32_t *)(sp + o_off); A.aux = (uint32_t *)(sp + o_aux);
    A.part = (unsigned long long *)(sp + o_part);
    A.sum = (hm_op_diff_summary *)(sp + o_sum);
    // the largest document of the call sizes a wave's slice of the work memory (HM_ODF_LISTS: a
    // document with lists by hm_od_slice_words_lists)
    SCHK(s, hm_launch_op_diff_need(A, (unsigned long long *)(sp + o_need), st));
    SCHK(s, hipMemcpyAsync(&s->h_cnt[10], sp + o_need, 16, hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));
    unsigned long long need, any_lists;
    memcpy(&need, &s->h_cnt[10], 8);
    memcpy(&any_lists, &s->h_cnt[12], 8);
    if (!any_lists) A.opts &= ~HM_ODF_LISTS;                   // (no requested document has lists: the walk without them)
    A.slice_words = need ? need : 1;
    A.waves = hm_od_waves(n, A.slice_words);
    return HM_OK;
}

// the summary a launch left, read back: *sum, and the status of its bad bits
static int op_diff_summary(hm_store *s, const OpDiffArgs &A, hm_op_diff_summary *sum) {
    hipStream_t st = hm_engine_stream(s->e);
    SCHK(s, hipMemcpyAsync(s->h_st, A.sum, sizeof(hm_op_diff_summary), hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));
    memcpy(sum, s->h_st, sizeof *sum);
    if (sum->bad & HM_OD_BAD_HANDLE) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad handle");
    if (sum->bad & HM_OD_BAD_ROWS) return hm_engine_fail(s->e, HM_ERR_INVALID, "a change row outside its document's segments");
    if (sum->bad) return hm_engine_fail(s->e, HM_ERR_NOMEM, "a document outgrows the op-diff work memory");
    return HM_OK;
}

// The count pass of n op-diff requests; the chains' work memory is the head of s->past.
static int op_diff_count(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                         const uint32_t *clock_rows, uint32_t opts, OpDiffArgs &A, hm_op_diff_summary *sum) {
    int rc = op_diff_stage(s, n, doc_handles, from, to, clock_rows, opts, A);
    if (rc) return rc;
    if ((rc = ensure_buf(s, s->past, ((size_t)A.waves * A.slice_words * 4 + 255) & ~(size_t)255))) return rc;
    A.work = (uint32_t *)s->past.p;
    SCHK(s, hm_launch_op_diff_count(A, hm_engine_stream(s->e)));
    return op_diff_summary(s, A, sum);
}

// hm_store_op_diff_sizes_ex (clock_rows NULL) and hm_store_op_diff_sizes_at (from / to NULL)
static int op_diff_sizes(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                         const uint32_t *clock_rows, uint32_t *out_counts, uint32_t *out_flags, uint64_t *out_totals, uint32_t opts) {
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        if (out_totals) out_totals[0] = out_totals[1] = 0;
        if (!n) return HM_OK;
        OpDiffArgs A;
        hm_op_diff_summary sum;
        int rc = op_diff_count(s, n, doc_handles, from, to, clock_rows, opts, A, &sum);
        if (rc) return rc;
        if (out_totals) { out_totals[0] = sum.totals[0]; out_totals[1] = sum.totals[1]; }
        if (out_counts || out_flags) {
            hipStream_t st = hm_engine_stream(s->e);
            std::vector<uint32_t> cnt(4 * (size_t)n), aux(2 * (size_t)n);
            SCHK(s, hipMemcpyAsync(cnt.data(), A.cnt, 16 * (size_t)n, hipMemcpyDeviceToHost, st));
            SCHK(s, hipMemcpyAsync(aux.data(), A.aux, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
            SCHK(s, hipStreamSynchronize(st));
            for (size_t i = 0; i < n; i++) {
                if (out_counts) { out_counts[2 * i] = cnt[4 * i]; out_counts[2 * i + 1] = cnt[4 * i + 1]; }
                if (out_flags) out_flags[i] = aux[2 * i + 1];
            }
        }
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_op_diff_sizes");
    }
}

// the count, scan and fill form of hm_store_op_diffs_ex (clock_rows NULL) and hm_store_op_diffs_at (from / to NULL)
static int op_diffs_filled(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                           const uint32_t *clock_rows, const hm_op_diff_out *out, uint32_t *out_index, uint64_t *out_totals, uint32_t opts) {
    const bool want_index = (opts & HM_ODF_LISTS) != 0u;
    hipStream_t st = hm_engine_stream(s->e);
    OpDiffArgs A;
    hm_op_diff_summary sum;
    int rc = op_diff_count(s, n, doc_handles, from, to, clock_rows, opts, A, &sum);
    if (rc) return rc;
    const uint64_t tr = sum.totals[0], ts = sum.totals[1];
    if (out_totals) { out_totals[0] = tr; out_totals[1] = ts; }
    if (tr > out->cap_rows || ts > out->cap_surv)
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "a capacity below the rows of the op diffs");
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // [work][rows][survivors][ranges][flags][index]
    const size_t sz[5] = {tr * sizeof(hm_op_diff), ts * sizeof(hm_surv_result), 8 * (size_t)n, 4 * (size_t)n, want_index ? 4 * (size_t)tr : 0};
    size_t o[5], total = al((size_t)A.waves * A.slice_words * 4);
    for (int i = 0; i < 5; i++) { o[i] = total; total += al(sz[i] + 1); }
    if ((rc = ensure_buf(s, s->past, total))) return rc;
    uint8_t *bp = s->past.p;
    A.work = (uint32_t *)bp;
    A.cap_rows = (uint32_t)tr; A.cap_surv = (uint32_t)ts;
    A.out_rows = (hm_op_diff *)(bp + o[0]); A.out_surv = (hm_surv_result *)(bp + o[1]);
    A.out_range = (uint32_t *)(bp + o[2]); A.out_flags = (uint32_t *)(bp + o[3]); A.out_index = want_index ? (uint32_t *)(bp + o[4]) : nullptr;
    SCHK(s, hm_launch_op_diff_fill(A, st));
    void *dst[5] = {out->rows, out->surv, out->range, out->flags, out_index};
    for (int i = 0; i < 5; i++)
        if (sz[i]) SCHK(s, hipMemcpyAsync(dst[i], bp + o[i], sz[i], hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));
    return HM_OK;
}

extern "C" {

int hm_store_op_diff_sizes(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                           uint32_t *out_counts, uint32_t *out_flags, uint64_t *out_totals) {
    return hm_store_op_diff_sizes_ex(s, n, doc_handles, from, to, out_counts, out_flags, out_totals, 0u);
}

int hm_store_op_diff_sizes_ex(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                              uint32_t *out_counts, uint32_t *out_flags, uint64_t *out_totals, uint32_t opts) {
    if (!s || (n && (!doc_handles || !from || !to)) || (opts & ~HM_ODF_LISTS)) return HM_ERR_INVALID;
    return op_diff_sizes(s, n, doc_handles, from, to, nullptr, out_counts, out_flags, out_totals, opts);
}

int hm_store_op_diff_sizes_at(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *clock_rows,
                              uint32_t *out_counts, uint32_t *out_flags, uint64_t *out_totals, uint32_t opts) {
    if (!s || (n && (!doc_handles || !clock_rows)) || (opts & ~HM_ODF_LISTS)) return HM_ERR_INVALID;
    return op_diff_sizes(s, n, doc_handles, nullptr, nullptr, clock_rows, out_counts, out_flags, out_totals, opts);
}

int hm_store_op_diffs_at(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *clock_rows,
                         const hm_op_diff_out *out, uint32_t *out_index, uint64_t *out_totals, uint32_t opts) {
    // (HM_ODF_ONCE is the docset round's form: not offered with a clock)
    if (!s || !out || (n && (!doc_handles || !clock_rows || !out->range || !out->flags)) || (opts & ~HM_ODF_LISTS)) return HM_ERR_INVALID;
    if ((out->cap_rows && !out->rows) || (out->cap_surv && !out->surv)) return HM_ERR_INVALID;
    if ((opts & HM_ODF_LISTS) && out->cap_rows && !out_index) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        if (out_totals) out_totals[0] = out_totals[1] = 0;
        if (!n) return HM_OK;
        return op_diffs_filled(s, n, doc_handles, nullptr, nullptr, clock_rows, out, out_index, out_totals, opts);
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_op_diffs_at");
    }
}

int hm_store_op_diffs(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                      const hm_op_diff_out *out, uint64_t *out_totals) {
    return hm_store_op_diffs_ex(s, n, doc_handles, from, to, out, nullptr, out_totals, 0u);
}

int hm_store_op_diffs_ex(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                         const hm_op_diff_out *out, uint32_t *out_index, uint64_t *out_totals, uint32_t opts) {
    if (!s || !out || (n && (!doc_handles || !from || !to || !out->range || !out->flags)) || (opts & ~(HM_ODF_LISTS | HM_ODF_ONCE))) return HM_ERR_INVALID;
    if ((out->cap_rows && !out->rows) || (out->cap_surv && !out->surv)) return HM_ERR_INVALID;
    const bool once = (opts & HM_ODF_ONCE) != 0u;
    if (once && !out_totals) return HM_ERR_INVALID;           // (a caller that guesses the sizes takes the ones to repeat with)
    const bool want_index = (opts & HM_ODF_LISTS) != 0u;
    if (want_index && out->cap_rows && !out_index) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        if (out_totals) out_totals[0] = out_totals[1] = 0;
        if (!n) return HM_OK;
        hipStream_t st = hm_engine_stream(s->e);
        OpDiffArgs A;
        hm_op_diff_summary sum;
        if (once) {
            // one launch into tables of the caller's capacities: [work][rows][survivors][ranges][flags][index]
            int rc = op_diff_stage(s, n, doc_handles, from, to, nullptr, opts & ~HM_ODF_ONCE, A);
            if (rc) return rc;
            auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
            const size_t cr = out->cap_rows, cs = out->cap_surv;
            const size_t sz[5] = {cr * sizeof(hm_op_diff), cs * sizeof(hm_surv_result), 8 * (size_t)n, 4 * (size_t)n, want_index ? 4 * cr : 0};
            size_t o[5], total = al((size_t)A.waves * A.slice_words * 4);
            for (int i = 0; i < 5; i++) { o[i] = total; total += al(sz[i] + 1); }
            if ((rc = ensure_buf(s, s->past, total))) return rc;
            uint8_t *bp = s->past.p;
            A.work = (uint32_t *)bp;
            A.cap_rows = out->cap_rows; A.cap_surv = out->cap_surv;
            A.out_rows = (hm_op_diff *)(bp + o[0]); A.out_surv = (hm_surv_result *)(bp + o[1]);
            A.out_range = (uint32_t *)(bp + o[2]); A.out_flags = (uint32_t *)(bp + o[3]); A.out_index = want_index ? (uint32_t *)(bp + o[4]) : nullptr;
            SCHK(s, hm_launch_op_diff_once(A, st));
            if ((rc = op_diff_summary(s, A, &sum))) return rc;
            out_totals[0] = sum.totals[0]; out_totals[1] = sum.totals[1];
            if (sum.totals[0] > cr || sum.totals[1] > cs)
                return hm_engine_fail(s->e, HM_ERR_NOMEM, "a capacity below the rows of the op diffs");
            // (the blocks lie anywhere below the totals)
            const size_t used[5] = {(size_t)sum.totals[0] * sizeof(hm_op_diff), (size_t)sum.totals[1] * sizeof(hm_surv_result), sz[2], sz[3],
                                    want_index ? 4 * (size_t)sum.totals[0] : 0};
            void *dst[5] = {out->rows, out->surv, out->range, out->flags, out_index};
            for (int i = 0; i < 5; i++)
                if (used[i]) SCHK(s, hipMemcpyAsync(dst[i], bp + o[i], used[i], hipMemcpyDeviceToHost, st));
            SCHK(s, hipStreamSynchronize(st));
            return HM_OK;
        }
        return op_diffs_filled(s, n, doc_handles, from, to, nullptr, out, out_index, out_totals, opts);
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_op_diffs");
    }
}

}  // extern "C"

// The count pass of n state requests: the handles go to the stage buffer, where the counts, offsets
// and summary stay (A.cnt / A.off / A.aux / A.sum); *sum = the summary read back.
static int state_count(hm_store *s, uint32_t n, const uint32_t *doc_handles, StateArgs &A, hm_state_summary *sum) {
    hipStream_t st = hm_engine_stream(s->e);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_sum = 0, o_h = 256, o_cnt = o_h + al(4 * (size_t)n), o_off = o_cnt + al(16 * (size_t)n),
                 o_aux = o_off + al(16 * (size_t)n), o_part = o_aux + al(8 * (size_t)n),
                 total = o_part + al((size_t)hm_past_scan_chunks(n) * HM_PAST_PART * 8);
    int rc = ensure_stage(s, total);
    if (rc) return rc;
    uint8_t *sp = s->stage.p;
    SCHK(s, hipMemcpyAsync(sp + o_h, doc_handles, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    A = StateArgs{};
    A.n = n; A.src = store_source(s); A.src.handles = (const uint32_t *)(sp + o_h);
    A.regs = s->regs; A.surv = s->surv; A.lim_r = s->cap_r; A.lim_s = s->cap_o; A.heads = s->heads;
    A.cnt = (uint32_t *)(sp + o_cnt); A.off = (uint32_t *)(sp + o_off); A.aux = (uint32_t *)(sp + o_aux);
    A.part = (unsigned long long *)(sp + o_part);
    A.sum = (hm_state_summary *)(sp + o_sum);
    SCHK(s, hm_launch_state_count(A, st));
    SCHK(s, hipMemcpyAsync(s->h_st, A.sum, sizeof(hm_state_summary), hipMemcpyDeviceToHost, st));
    SCHK(s, hipStreamSynchronize(st));
    memcpy(sum, s->h_st, sizeof *sum);
    if (sum->bad & HM_ST_BAD_HANDLE) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad handle");
    return HM_OK;
}

extern "C" {

int hm_store_state_sizes(hm_store *s, uint32_t n, const uint32_t *doc_handles, uint32_t *out_counts, uint32_t *out_flags,
                         uint64_t *out_totals) {
    if (!s || (n && !doc_handles)) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        if (out_totals) out_totals[0] = out_totals[1] = 0;
        if (!n) return HM_OK;
        StateArgs A;
        hm_state_summary sum;
        int rc = state_count(s, n, doc_handles, A, &sum);
        if (rc) return rc;
        if (out_totals) { out_totals[0] = sum.totals[0]; out_totals[1] = sum.totals[1]; }
        if (out_counts || out_flags) {
            hipStream_t st = hm_engine_stream(s->e);
            std::vector<uint32_t> cnt(4 * (size_t)n), aux(2 * (size_t)n);
            SCHK(s, hipMemcpyAsync(cnt.data(), A.cnt, 16 * (size_t)n, hipMemcpyDeviceToHost, st));
            SCHK(s, hipMemcpyAsync(aux.data(), A.aux, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
            SCHK(s, hipStreamSynchronize(st));
            for (size_t i = 0; i < n; i++) {
                if (out_counts) { out_counts[2 * i] = cnt[4 * i]; out_counts[2 * i + 1] = cnt[4 * i + 1]; }
                if (out_flags) out_flags[i] = aux[2 * i + 1];
            }
        }
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_state_sizes");
    }
}

int hm_store_state(hm_store *s, uint32_t n, const uint32_t *doc_handles, const hm_state_out *out, uint32_t *out_clock,
                   uint32_t *out_heads, uint64_t *out_totals) {
    if (!s || !out || (n && (!doc_handles || !out->range || !out->flags)) || (out->cap_rows && !out->rows) ||
        (out->cap_surv && !out->surv))
        return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        if (out_totals) out_totals[0] = out_totals[1] = 0;
        if (!n) return HM_OK;
        hipStream_t st = hm_engine_stream(s->e);
        StateArgs A;
        hm_state_summary sum;
        int rc = state_count(s, n, doc_handles, A, &sum);
        if (rc) return rc;
        const uint64_t tr = sum.totals[0], ts = sum.totals[1];
        if (out_totals) { out_totals[0] = tr; out_totals[1] = ts; }
        if (tr > out->cap_rows || ts > out->cap_surv)
            return hm_engine_fail(s->e, HM_ERR_NOMEM, "a capacity below the rows of the state");
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        // [rows][survivors][ranges][flags][clock][heads]
        const size_t row_b = 4 * (size_t)n * s->S;
        const size_t sz[6] = {tr * sizeof(hm_state_row), ts * sizeof(hm_surv_result), 16 * (size_t)n, 4 * (size_t)n,
                              out_clock ? row_b : 0, out_heads ? row_b : 0};
        size_t o[6], total = 0;
        for (int i = 0; i < 6; i++) { o[i] = total; total += al(sz[i] + 1); }
        if ((rc = ensure_buf(s, s->past, total))) return rc;
        uint8_t *bp = s->past.p;
        A.cap_rows = (uint32_t)tr; A.cap_surv = (uint32_t)ts;
        A.out_rows = (hm_state_row *)(bp + o[0]); A.out_surv = (hm_surv_result *)(bp + o[1]);
        A.out_range = (uint32_t *)(bp + o[2]); A.out_flags = (uint32_t *)(bp + o[3]);
        A.out_clock = out_clock ? (uint32_t *)(bp + o[4]) : nullptr; A.out_heads = out_heads ? (uint32_t *)(bp + o[5]) : nullptr;
        SCHK(s, hm_launch_state_fill(A, st));
        void *dst[6] = {out->rows, out->surv, out->range, out->flags, out_clock, out_heads};
        for (int i = 0; i < 6; i++)
            if (sz[i]) SCHK(s, hipMemcpyAsync(dst[i], bp + o[i], sz[i], hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_state");
    }
}

// (the selection of one prefix request of the past kernels: out_change_log, nothing else gathered)
int hm_doc_history_prefix(hm_store *s, uint32_t doc, uint32_t n, uint32_t *out) {
    if (!s || doc >= s->n_handles || (n && !out)) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        hipStream_t st = hm_engine_stream(s->e);
        PastArgs P;
        hm_past_summary sum;
        int rc = past_count(s, 1, &doc, &n, nullptr, P, &sum);
        if (rc) return -rc;
        const uint32_t k = (uint32_t)sum.totals[0];
        if (!k) return 0;
        if ((rc = ensure_buf(s, s->past, sizeof(hm_doc_row) + 256 + 4 * (size_t)k))) return -rc;
        P.log_only = 1u;
        P.cap[0] = k;
        P.out_docs = (hm_doc_row *)s->past.p;
        P.out_change_log = (uint32_t *)(s->past.p + 256);
        SCHK(s, hm_launch_past_fill(P, st));
        SCHK(s, hipMemcpyAsync(out, P.out_change_log, 4 * (size_t)k, hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        return (int)k;
    } catch (...) {
        return -hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_doc_history_prefix");
    }
}

int hm_doc_set_min_clock(hm_store *s, uint32_t doc, const uint32_t *clock) {
    if (!s || doc >= s->n_handles || !clock) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    SCHK(s, hipMemcpy(s->min_clock + (size_t)doc * s->S, clock, s->S * 4, hipMemcpyHostToDevice));
    // the incremental kernels read the row only for documents that have one
    DevDoc m;
    SCHK(s, hipMemcpy(&m, s->dm + doc, sizeof m, hipMemcpyDeviceToHost));
    m.pad[0] |= HM_DDOC_MINC;
    SCHK(s, hipMemcpy(s->dm + doc, &m, sizeof m, hipMemcpyHostToDevice));
    return HM_OK;
}

int hm_store_clock_update(hm_store *s, uint32_t n, const uint32_t *docs, uint8_t *out_written, uint8_t *out_differs,
                          uint32_t *out_stored) {
    if (!s || (n && !docs)) return HM_ERR_INVALID;
    if (s->pending) return hm_engine_fail(s->e, HM_ERR_INVALID, "batch in flight");
    try {
        for (uint32_t i = 0; i < n; i++) if (docs[i] >= s->n_handles) return hm_engine_fail(s->e, HM_ERR_INVALID, "bad handle");
        if (!n) return HM_OK;
        const uint32_t S = s->S;
        hipStream_t st = hm_engine_stream(s->e);
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_h = 0, o_w = al(n * 4), o_d = o_w + al(n + 4), o_s = o_d + al(n + 4), total = o_s + al((size_t)n * S * 4);
        int rc = ensure_stage(s, total);
        if (rc) return rc;
        uint8_t *sp = s->stage.p;
        SCHK(s, hipMemcpyAsync(sp + o_h, docs, n * 4, hipMemcpyHostToDevice, st));
        SCHK(s, hipMemsetAsync(sp + o_w, 0, o_s - o_w, st));
        SCHK(s, hm_launch_clock_update((const uint32_t *)(sp + o_h), n, S, s->back_clock, s->stored, sp + o_w, sp + o_d,
                                       (uint32_t *)(sp + o_s), st));
        if (out_written) SCHK(s, hipMemcpyAsync(out_written, sp + o_w, n, hipMemcpyDeviceToHost, st));
        if (out_differs) SCHK(s, hipMemcpyAsync(out_differs, sp + o_d, n, hipMemcpyDeviceToHost, st));
        if (out_stored) SCHK(s, hipMemcpyAsync(out_stored, sp + o_s, (size_t)n * S * 4, hipMemcpyDeviceToHost, st));
        SCHK(s, hipStreamSynchronize(st));
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(s->e, HM_ERR_NOMEM, "exception in hm_store_clock_update");
    }
}

int hm_sync_ranges_device(hm_engine *e, const uint64_t *present, const uint64_t *word_off, const uint32_t *lo,
                          const uint32_t *hi, uint32_t *out_end, uint32_t n, void *stream) {
    if (!e) return HM_ERR_INVALID;
    hipError_t r = hm_launch_sync_ranges(present, word_off, lo, hi, out_end, n,
                                         stream ? (hipStream_t)stream : hm_engine_stream(e));
    return r == hipSuccess ? HM_OK : hm_engine_fail(e, HM_ERR_DEVICE, "sync_ranges launch");
}

int hm_sync_ranges_host(hm_engine *e, const uint64_t *present, const uint64_t *word_off, const uint32_t *lo,
                        const uint32_t *hi, uint32_t *out_end, uint32_t n, uint32_t n_words) {
    if (!e || (n && (!present || !word_off || !lo || !hi || !out_end))) return HM_ERR_INVALID;
    if (!n) return HM_OK;
    for (uint32_t i = 0; i < n; i++)
        if (word_off[i] > n_words || hi[i] < lo[i] || word_off[i] + ((uint64_t)hi[i] + 63) / 64 > n_words)
            return hm_engine_fail(e, HM_ERR_INVALID, "sync range outside the present bitmap");
    hipStream_t st = hm_engine_stream(e);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_p = 0, o_w = al(8 * (size_t)n_words + 8), o_lo = o_w + al(8 * (size_t)n), o_hi = o_lo + al(4 * (size_t)n),
                 o_out = o_hi + al(4 * (size_t)n), total = o_out + al(4 * (size_t)n);
    uint8_t *sp = nullptr;
    if (hipMalloc((void **)&sp, total) != hipSuccess) return hm_engine_fail(e, HM_ERR_NOMEM, "hipMalloc sync staging");
    int rc = HM_OK;
    if (hipMemcpyAsync(sp + o_p, present, 8 * (size_t)n_words, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(sp + o_w, word_off, 8 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(sp + o_lo, lo, 4 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(sp + o_hi, hi, 4 * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hm_launch_sync_ranges((const uint64_t *)(sp + o_p), (const uint64_t *)(sp + o_w), (const uint32_t *)(sp + o_lo),
                              (const uint32_t *)(sp + o_hi), (uint32_t *)(sp + o_out), n, st) != hipSuccess ||
        hipMemcpyAsync(out_end, sp + o_out, 4 * (size_t)n, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        rc = hm_engine_fail(e, HM_ERR_DEVICE, "hm_sync_ranges_host");
    (void)hipFree(sp);
    return rc;
}

}  // extern "C"
