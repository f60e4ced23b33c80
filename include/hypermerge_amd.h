/*
 * hypermerge_amd.h — C-ABI boundary of the MI355X batched CRDT merge engine.
 *
 * The engine replaces the L5 -> L0 edge of hypermerge: everything that
 * Automerge 0.12's `Backend.applyChanges(state, changes)` computes when
 * `DocBackend.applyRemoteChanges` / `DocBackend.init` hand it a batch of
 * decoded `Change` objects, plus the vector-clock bookkeeping around it.
 *
 *   reference call sites replaced (paths relative to the reference repo):
 *     src/DocBackend.ts:115-117  applyRemoteChanges(changes)  -> remoteChangesQ
 *     src/DocBackend.ts:169-185  Backend.applyChanges(back, changes) + updateClock
 *     src/DocBackend.ts:144-167  init(changes): Backend.applyChanges(Backend.init(), changes)
 *     src/DocBackend.ts:135-142  updateClock (clock includes queued changes)
 *     src/DocBackend.ts:90-100   testMinimumClockSatisfied -> Clock.cmp
 *     src/Clock.ts:13-38,87-113  gte / cmp / union / intersection
 *     src/RepoBackend.ts:570-579 MaterializeMsg (history-prefix replay)
 *   Automerge 0.12.2-beta.0 (yarn.lock:178-185; NOT vendored) backend/op_set.js:
 *     addChange/applyQueuedOps/causallyReady, applyChange/transitiveDeps,
 *     applyAssign (map registers, counters, conflicts), applyInsert +
 *     updateListElement (RGA lists/text).  Restated in SURVEY.md Appendix A.
 *
 * A batch is columnar: plain little-endian tables, no strings.  Strings
 * (actor ids, object UUIDs, keys, string values) are interned by the host
 * encoder; the engine only needs their identity, except actor ids, whose
 * JS UTF-16 string order is encoded as the per-document actor *rank*.
 *
 * No C++ exception crosses this boundary.  Every call returns an hm_status;
 * per-document failures are reported per document (hm_doc_result.status),
 * never as a whole-batch failure (the reference aborts only the throwing
 * document's applyChanges; SURVEY.md §5, §8b "Errors").
 */
#ifndef HYPERMERGE_AMD_H
#define HYPERMERGE_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HM_ABI_VERSION 4u

/* ------------------------------------------------------------------ */
/* Status codes                                                        */
/* ------------------------------------------------------------------ */
typedef enum {
    HM_OK = 0,
    /* per-document Automerge errors (the message each maps to is what the
     * reference would throw; see hm_status_message) */
    HM_ERR_INCONSISTENT_SEQ = 1,   /* 'Inconsistent reuse of sequence number <seq> by <actor>' */
    HM_ERR_UNKNOWN_OBJECT = 2,     /* 'Modification of unknown object <obj>' */
    HM_ERR_DUPLICATE_OBJECT = 3,   /* 'Duplicate creation of object <obj>' */
    HM_ERR_DUPLICATE_ELEM = 4,     /* 'Duplicate list element ID <elemId>' */
    HM_ERR_MISSING_ELEM = 5,       /* 'Missing index entry for list element <elemId>' */
    /* engine-side limits / preconditions (not reference errors) */
    HM_ERR_UNSUPPORTED = 16,       /* document outside the engine's supported envelope */
    /* call-level errors */
    HM_ERR_INVALID = 32,           /* malformed batch (bad offsets, sizes) */
    HM_ERR_DEVICE = 33,            /* HIP runtime failure */
    HM_ERR_NOMEM = 34
} hm_status;

/* ------------------------------------------------------------------ */
/* Op actions / datatypes / value tags (Automerge 0.12 op vocabulary)   */
/* ------------------------------------------------------------------ */
enum {
    HM_MAKE_MAP = 0, HM_MAKE_TABLE = 1, HM_MAKE_LIST = 2, HM_MAKE_TEXT = 3,
    HM_INS = 4, HM_SET = 5, HM_DEL = 6, HM_LINK = 7, HM_INC = 8
};
enum { HM_DT_NONE = 0, HM_DT_COUNTER = 1, HM_DT_TIMESTAMP = 2 };
enum {
    HM_V_NULL = 0, HM_V_FALSE = 1, HM_V_TRUE = 2,
    HM_V_INT = 3,    /* integral JS number, |v| < 2^53, stored as int64 */
    HM_V_FLOAT = 4,  /* any other JS number, stored as IEEE-754 f64 bits */
    HM_V_STR = 5,    /* string-pool id */
    HM_V_OBJ = 6     /* doc-local object id (link target) */
};
#define HM_HEAD 0xFFFFFFFFu      /* ins parent '_head' */
#define HM_NONE 0xFFFFFFFFu

/* ------------------------------------------------------------------ */
/* Columnar batch tables                                               */
/* ------------------------------------------------------------------ */

/* One row per document (48 B).  Every input range of a document is in its row,
 * so all of a document's loads can be issued as soon as the row is read. */
typedef struct {
    uint32_t change_off;  /* first row of this doc in changes[] */
    uint32_t n_changes;   /* changes handed to applyChanges, in array (arrival) order */
    uint32_t dep_off;     /* first row of this doc in deps[] (= changes[change_off].dep_off) */
    uint32_t n_deps;      /* dep rows of all its changes (contiguous) */
    uint32_t op_off;      /* first row of this doc in ops[]; ops are grouped by change, in op order */
    uint32_t n_ops;
    uint32_t reg_off;     /* first row of this doc in the per-register output table */
    uint32_t n_regs;      /* registers = interned (obj, key) pairs; for lists key = elemId */
    uint32_t n_objs;      /* interned object ids, 0 = ROOT '00000000-0000-0000-0000-000000000000' */
    uint16_t n_actors;    /* actor ranks 0..n_actors-1 (rank = order of the actor id strings) */
    uint16_t flags;       /* HM_DOC_* bits set by the encoder */
    uint32_t reserved[2]; /* not read by the engine (the synthetic feeds keep the doc's global index here) */
} hm_doc_row;
#define HM_DOC_HAS_LISTS 1u     /* the doc creates a list/text object (launch sizing hint only) */
#define HM_DOC_HAS_COUNTERS 2u  /* the doc has counter sets or incs (launch sizing hint only) */

/* One row per change (24 B), in the order the changes are handed over. */
typedef struct {
    uint16_t actor;       /* actor rank within the doc */
    uint16_t n_deps;
    uint32_t seq;         /* 1-based */
    uint32_t dep_off;     /* first row in deps[] (global) */
    uint32_t n_ops;       /* ops of this change: rows [op_first, op_first+n_ops) */
    uint32_t op_first;    /* global op row */
    uint32_t content_id;  /* equal <=> the two changes are deep-equal (host-interned) */
} hm_change_row;

/* One row per dependency entry (8 B), in the change's `deps` key order. */
typedef struct {
    uint16_t actor;
    uint16_t pad;
    uint32_t seq;
} hm_dep_row;

/* One row per op (32 B). */
typedef struct {
    uint32_t obj;         /* doc-local object id the op modifies (make*: the created object) */
    uint32_t reg;         /* set/del/link/inc: register of (obj,key); ins: register of the new element */
    uint32_t parent;      /* ins: register of the predecessor element, or HM_HEAD */
    uint32_t elem;        /* ins: element counter */
    uint8_t  action;      /* HM_MAKE_* / HM_INS / HM_SET / HM_DEL / HM_LINK / HM_INC */
    uint8_t  datatype;    /* HM_DT_* */
    uint8_t  vtag;        /* HM_V_* */
    uint8_t  pad;
    uint32_t key;         /* string-pool id of the map key (rendering only) */
    uint64_t value;       /* int64 / f64 bits / string id / object id, by vtag */
} hm_op_row;

/* Widest per-actor row (actors per document): the reference mints one actor per writer
 * (src/RepoBackend.ts:286-293), so a shared document can have many.  Documents of more than
 * 8 actors merge in the general kernel; rows wider than 64 are the "wide" strides. */
#define HM_MAX_STRIDE 256u

typedef struct {
    uint32_t n_docs, n_changes, n_deps, n_ops, n_regs;
    uint32_t a_stride;    /* >= max n_actors; stride of every per-actor output row (1..HM_MAX_STRIDE) */
    /* per-document maxima over the batch (launch sizing hints); 0 = unknown,
     * computed by the engine from the doc table */
    uint32_t max_changes, max_ops, max_regs, max_objs;
    uint32_t doc_flags;   /* OR of every docs[d].flags (launch hint; 0 when unknown -> computed) */
    uint32_t max_deps;    /* max docs[d].n_deps (launch hint, sizes the LDS dep table) */
    const hm_doc_row    *docs;
    const hm_change_row *changes;
    const hm_dep_row    *deps;
    const hm_op_row     *ops;
    const uint32_t      *min_clock;  /* optional [n_docs*a_stride] minimumClock (0 = absent) or NULL */
} hm_batch;

/* ------------------------------------------------------------------ */
/* Results                                                             */
/* ------------------------------------------------------------------ */
typedef struct {          /* 32 B */
    int32_t  status;      /* hm_status for this document */
    uint32_t err_change;  /* doc-local change index where the first error fired (HM_NONE if ok) */
    uint32_t err_op;      /* op index within that change, HM_NONE for change-level errors */
    uint32_t hist_len;    /* opSet.history.size after the merge */
    uint32_t n_queued;    /* changes left in opSet.queue (causally blocked) */
    uint32_t n_surv;      /* survivors written for this doc */
    uint32_t min_cmp;     /* Clock.cmp(DocBackend.clock, minimumClock): 0 EQ 1 GT 2 LT 3 CONCUR */
    uint32_t pad;
} hm_doc_result;

typedef struct {          /* 16 B per register */
    uint32_t n_surv;      /* surviving ops (winner + conflicts) */
    uint32_t surv_off;    /* doc-local offset into the survivor table (doc base = docs[d].op_off) */
    int32_t  list_index;  /* list/text element: index among visible elements, else -1 */
    uint32_t obj;         /* object the register belongs to (HM_NONE if never touched) */
} hm_reg_result;

typedef struct {          /* 16 B per survivor, winner first then conflicts */
    uint32_t op;          /* doc-local op index (ops[docs[d].op_off + op]) */
    uint32_t vtag;        /* value tag of the resolved value (counters may turn INT -> FLOAT) */
    uint64_t value;       /* resolved value (counter: base + causally-later incs) */
} hm_surv_result;

typedef struct {
    hm_doc_result  *docs;       /* [n_docs] */
    uint32_t       *clock;      /* [n_docs*a_stride] opSet.clock (applied changes only) */
    uint32_t       *back_clock; /* [n_docs*a_stride] DocBackend.clock (max over handed changes, quirk) */
    uint32_t       *heads;      /* [n_docs*a_stride] opSet.deps (0 = no entry) */
    int32_t        *hist;       /* [n_changes] history position, -1 queued, -2 duplicate (no-op) */
    uint32_t       *all_deps;   /* [n_changes*a_stride] opSet.states[actor][seq-1].allDeps (0 if not applied) */
    hm_reg_result  *regs;       /* [n_regs] */
    hm_surv_result *surv;       /* [n_ops] */
} hm_results;

/* ------------------------------------------------------------------ */
/* Engine                                                              */
/* ------------------------------------------------------------------ */
typedef struct hm_engine hm_engine;

typedef struct {
    int device;           /* HIP device ordinal */
    int flags;            /* HM_CFG_* */
} hm_config;
#define HM_CFG_GENERAL_ONLY 1   /* route every document through the general (workgroup) kernel */

/* Version of the ABI compiled into the library. */
uint32_t hm_abi_version(void);
const char *hm_status_message(int status);

int  hm_engine_create(const hm_config *cfg, hm_engine **out);
void hm_engine_destroy(hm_engine *e);
const char *hm_engine_last_error(const hm_engine *e);

/* Host batch -> device -> merge -> host results (synchronous).  All host
 * buffers are owned by the caller; the engine stages copies.  A batch of
 * >= 128k documents whose tables are in document order is processed in up to
 * 16 document ranges with upload, merge and download overlapped on three
 * streams; page-locked caller buffers (hipHostMalloc / torch pin_memory) let
 * those copies run at PCIe DMA rate.  Results are identical either way. */
int hm_merge_host(hm_engine *e, const hm_batch *batch, const hm_results *out);

/* Device-resident merge: every pointer in `batch` and `out` is a device
 * pointer on the engine's device; work is enqueued on `stream` (hipStream_t,
 * NULL = the engine's stream) and the call returns without synchronising.
 * `scratch` is device memory of at least hm_scratch_bytes(batch) bytes. */
size_t hm_scratch_bytes(const hm_batch *batch);
int hm_merge_device(hm_engine *e, const hm_batch *batch, const hm_results *out,
                    void *scratch, void *stream);

/* Per-kernel launch timing of the last hm_merge_* call on `stream`,
 * measured with HIP events on that stream (ms).  Returns number filled. */
int hm_last_kernel_ms(hm_engine *e, float *ms, int max_kernels);
/* Documents the last hm_merge_* launch routed to the general (workgroup) kernel: waits
 * for that launch, copies up to `cap` of their launch-row indices (in hand-over order)
 * and returns their count (negative hm_status on failure; -HM_ERR_INVALID after a
 * hm_merge_device with caller scratch, whose list the engine cannot know is still valid).
 * Diagnostics / roofline attribution: the two kernels' algorithmic bytes are split by it. */
int hm_last_deferred(hm_engine *e, uint32_t *out_docs, uint32_t cap);

/* ------------------------------------------------------------------ */
/* Clock algebra (src/Clock.ts) over dense per-doc rows (a_stride wide) */
/* ------------------------------------------------------------------ */
/* out[d] = Clock.cmp(a[d], b[d]) coded 0 EQ, 1 GT, 2 LT, 3 CONCUR  (src/Clock.ts:27-38) */
int hm_clock_cmp_device(hm_engine *e, const uint32_t *a, const uint32_t *b, uint8_t *out,
                        uint32_t n_docs, uint32_t a_stride, void *stream);
/* c[d] = Clock.union(a[d], b[d]) elementwise max (src/Clock.ts:87-95) */
int hm_clock_union_device(hm_engine *e, const uint32_t *a, const uint32_t *b, uint32_t *c,
                          uint32_t n_docs, uint32_t a_stride, void *stream);
/* c[d] = Clock.intersection(a[d], b[d]) elementwise min, zeros dropped (src/Clock.ts:103-113) */
int hm_clock_intersection_device(hm_engine *e, const uint32_t *a, const uint32_t *b, uint32_t *c,
                                 uint32_t n_docs, uint32_t a_stride, void *stream);

/* ------------------------------------------------------------------ */
/* Resident document store: the per-document Automerge BackendState    */
/* (`DocBackend.back`, src/DocBackend.ts:50) kept on the device.       */
/* ------------------------------------------------------------------ */
/*
 * Every open document owns device segments holding its change log (the
 * change/dep/op rows of every change handed to applyChanges so far, in
 * arrival order) and its merged state (history, allDeps, registers,
 * survivors, clocks).  `Backend.applyChanges(back, changes)` is a left fold of
 * addChange over `changes`, so applyChanges(applyChanges(s, A), B) is
 * applyChanges(s, A ++ B): a submit appends each document's new rows to its
 * log and either applies them on the resident state (hm_store_set_incremental)
 * or re-merges the log with the batch kernels.  A document whose merge
 * throws is rolled back to its previous log, exactly as a throwing
 * applyChanges leaves `DocBackend.back` (and `DocBackend.clock`) unchanged
 * (src/DocBackend.ts:170-184).
 *
 *   replaces: src/DocBackend.ts:144-167 init(changes)  (hm_doc_open + submit)
 *             src/DocBackend.ts:115-117,169-185 applyRemoteChanges
 *             src/DocBackend.ts:90-113 testMinimumClockSatisfied / updateMinimumClock
 *             src/DocBackend.ts:135-142 updateClock (hm_batch_wait back_clock)
 *             src/RepoBackend.ts:572-576 history.slice(0, n) (hm_doc_history_prefix)
 *             src/ClockStore.ts:78-91 update (hm_store_clock_update)
 *             src/RepoBackend.ts:506-531 syncChanges contiguity (hm_sync_ranges_device)
 */
typedef struct hm_store hm_store;

typedef struct {
    uint32_t a_stride;      /* per-actor row width of every document (1..64) */
    uint32_t reserved;
} hm_store_config;

int  hm_store_create(hm_engine *e, const hm_store_config *cfg, hm_store **out);
void hm_store_destroy(hm_store *s);

/* A new, empty document (Backend.init()).  Handles are dense from 0. */
int hm_doc_open(hm_store *s, uint32_t *out_doc);

/* n new, empty documents with consecutive handles starting at *out_first. */
int hm_doc_open_n(hm_store *s, uint32_t n, uint32_t *out_first);

/* Release n documents: each handle becomes an empty document again (as hm_doc_open made it,
 * ready for reuse) and its old rows are dead space that the next compaction reclaims.
 * Not while a batch is in flight; the handles must be distinct.  (No reference counterpart:
 * the docset's restride (a document moving to a wider actor class) releases its old handle
 * with it instead of leaking its rows.) */
int hm_doc_reset(hm_store *s, const uint32_t *doc_handles, uint32_t n);

/* Append new changes to documents and re-merge them.  `b` is a batch in the
 * hm_batch layout whose rows are only the NEW changes (offsets local to `b`);
 * for each row i, docs[i].n_actors / n_regs / n_objs are document totals
 * after the append and doc_handles[i] names the document (each at most once
 * per batch).  actor_remap (optional, [n_docs * a_stride]) gives, for each row,
 * the new rank of every previously used actor rank (identity rows allowed;
 * NULL = no document's ranks moved) — ranks are actor-id string order, so a
 * new actor can shift the ranks of the document's existing rows.
 * Asynchronous: results are collected by hm_batch_wait.  One batch in flight. */
int hm_batch_submit(hm_store *s, const hm_batch *b, const uint32_t *doc_handles,
                    const uint8_t *actor_remap, uint64_t *out_batch_id);

/* Wait for a submitted batch (from any one host thread; the store is not otherwise
 * thread-safe: no other call on it until the wait returns); per batch row: the merge result of the
 * document's whole log, and (each optional) its opSet.clock, DocBackend.clock
 * and opSet.deps rows ([n_docs * a_stride]).  Documents whose merge threw are
 * reported with their error status and rolled back before this returns. */
int hm_batch_wait(hm_store *s, uint64_t batch_id, hm_doc_result *out_docs,
                  uint32_t *out_clock, uint32_t *out_back_clock, uint32_t *out_heads);

/* hm_batch_submit with the batch already in HBM: b->docs / changes / deps / ops, doc_handles
 * and actor_remap are device pointers on the store's device (counts in b as usual), read
 * in place — they must stay unchanged until the batch's wait returns.  (A host that decodes
 * blocks into device buffers on a copy stream, or a GPU producer, hands rows over without a
 * host round trip.) */
int hm_batch_submit_device(hm_store *s, const hm_batch *b, const uint32_t *doc_handles,
                           const uint8_t *actor_remap, uint64_t *out_batch_id);

/* Wait for a batch and leave its results on the device: out_dev (device memory) receives
 * [n_docs hm_doc_result][n_docs*a_stride clock][n_docs*a_stride back_clock][n_docs*a_stride heads]
 * by one device-to-device copy; out_n_failed (optional, host) = rows whose status is not OK
 * (those documents are rolled back before this returns, as in hm_batch_wait). */
int hm_batch_wait_device(hm_store *s, uint64_t batch_id, void *out_dev, uint32_t *out_n_failed);

/* Undo the last waited batch: every document of it back to its log and state before the
 * submit (its new rows dropped, actor ranks mapped back, the previous state re-merged), as if
 * the batch had thrown for all of them.  Only the last batch waited for, and only until the
 * store's next submit.  (The docset undoes the batches of a call whose later step failed, so a
 * call is applied to every store or to none.) */
int hm_batch_undo(hm_store *s, uint64_t batch_id);

/* Incremental applyRemoteChanges (on by default): a document whose new changes are each
 * causally ready in arrival order on its resident state (nothing queued, no actor re-rank,
 * map set/del/link/inc ops, small submits) is advanced in place — history, allDeps, heads and
 * clock appended, only the registers its new ops hit read and rewritten — instead of
 * re-merging its whole log.  Results are identical either way; off = always re-merge.
 * on = 1: a document with list / text objects whose log fits the small merge kernel (<= 256
 * ops) re-merges: it is one wave either way, and such a document then keeps no incremental
 * state to maintain; on = 2: every eligible document takes the incremental path (tests).
 * (A register's survivors may then sit anywhere in its document's op segment; hm_doc_read
 * hands them out packed, as a merge writes them.) */
int hm_store_set_incremental(hm_store *s, int on);
/* Routing of the last submit: out3 = {incremental, re-merged, incremental handed back to
 * the re-merge}. */
int hm_store_last_routing(const hm_store *s, uint32_t *out3);
/* Device time of the last submit, from HIP events on the engine stream: out2[0] = the
 * incremental kernels (lane / group / wave passes), out2[1] = the re-merge of the documents
 * they did not take (row build, merge kernels, metadata), in ms; read once hm_batch_wait(_device)
 * has returned for that submit (the submit itself does not wait for its kernels). */
int hm_store_last_kernel_ms(const hm_store *s, float *out2);
/* Documents whose resident incremental state a submit can use (kept on the device by every step
 * that builds or drops a state; a store with none plans its submits as whole re-merges and
 * launches no incremental kernel).  Synchronous; no batch may be in flight. */
int hm_store_inc_states(hm_store *s, uint32_t *out);
/* The store's four row arenas, in the order changes, deps, ops, registers: out_cap = their
 * capacities, out_used = their bump pointers (rows handed out to segments, dead ones included),
 * both in rows.  A submit whose growing segments fit the free rows of every arena allocates in
 * place; one that does not compacts the store into larger arenas first.  Read-only (diagnostics,
 * tests); synchronous; no batch may be in flight. */
int hm_store_arena_info(hm_store *s, uint64_t out_cap[4], uint64_t out_used[4]);

/* Diagnostics of check builds (libhmgpu_check.so, built beside libhmgpu.so): out2[0] = documents
 * whose next rows merge_small_kernel loaded asynchronously and re-read with counted loads,
 * out2[1] = those whose two reads differed (the asynchronous wait was too short); reset zeroes
 * both.  Returns 1 in a check build, 0 in the product build (out2 untouched), < 0 on a HIP error. */
int hm_debug_async_check(unsigned long long *out2, int reset);
/* The exit census of the incremental apply passes (check builds): out[pass * slots + slot] =
 * documents (or events) counted since the last reset, for the passes and slots of hm_inc_pass /
 * hm_inc_slot (csrc/store_kernels.h); at most n slots are copied; reset zeroes the table.  Returns the
 * slots copied in a check build, 0 in the product build (out untouched), < 0 on a HIP error. */
int hm_debug_inc_paths(unsigned long long *out, int n, int reset);
/* The persistent grid of merge_small_kernel for a host batch (its max_* hints, or its document
 * table when they are all 0): out6[0] = resident one-wave workgroups per CU of the instantiation
 * the launch uses (the smaller of the register and the LDS bound), out6[1] = the device's CUs
 * (the grid is their product, at most n_docs), out6[2..5] = the instantiation itself: op rows per
 * lane, size class, lists, counters.  Launches nothing.  Returns HM_OK or an hm_status. */
int hm_debug_small_occupancy(hm_engine *e, const hm_batch *host_batch, uint32_t *out6);

/* Sizes of a document's log and merged state. */
typedef struct {
    uint32_t n_changes, n_deps, n_ops, n_regs, n_objs, n_actors;
    uint32_t hist_len, n_queued, n_surv;
    int32_t  status;
} hm_doc_info_t;
int hm_doc_info(hm_store *s, uint32_t doc, hm_doc_info_t *out);

/* Read a document's merged state (any pointer may be NULL):
 * hist [n_changes], all_deps [n_changes*a_stride], regs [n_regs],
 * surv [n_ops] (first n_surv valid), clock/back_clock/heads [a_stride]. */
int hm_doc_read(hm_store *s, uint32_t doc, int32_t *hist, uint32_t *all_deps, hm_reg_result *regs,
                hm_surv_result *surv, uint32_t *clock, uint32_t *back_clock, uint32_t *heads);

/* Chosen registers of resident documents (incremental patches: only the registers a submit's
 * ops hit are read).  Request i = (doc_handles[i], regs[i]); out_regs[i] is that register's row
 * with surv_off rewritten to an offset into out_surv, where its n_surv survivors are copied
 * (request order of the survivor blocks is unspecified).  surv_cap = rows of out_surv; the
 * survivors of a document's registers never exceed its hm_doc_result.n_surv.  *out_n_surv =
 * rows needed; HM_ERR_NOMEM (nothing copied to out_surv) when that exceeds surv_cap. */
int hm_store_read_regs(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *regs,
                       hm_reg_result *out_regs, hm_surv_result *out_surv, uint32_t surv_cap, uint32_t *out_n_surv);

/* The log rows of a document (debug / materialize): changes [n_changes]
 * with dep_off/op_first local to the document, deps [n_deps], ops [n_ops]. */
int hm_doc_log(hm_store *s, uint32_t doc, hm_change_row *changes, hm_dep_row *deps, hm_op_row *ops);

/* history.slice(0, n): log indices of the first n applied changes, in history
 * order (src/RepoBackend.ts:572-576).  Returns the count written (<= n): the applied changes at
 * history positions below n (on a consistent document min(n, history.size)).  One prefix request of
 * the past kernels (hm_store_materialize's selection, the change map alone): per call two small
 * host-to-device copies, a memset, four kernel launches and two stream synchronisations, so a caller
 * with many documents asks hm_store_materialize / hm_store_past_sizes once instead. */
int hm_doc_history_prefix(hm_store *s, uint32_t doc, uint32_t n, uint32_t *out_log_index);

/* history.slice(from[i], to[i]) of many documents at once (the changes one applyChanges round
 * applied, in application order; patch rendering): request i writes
 * rows out_off[i] .. out_off[i+1]-1 (out_off[i+1] - out_off[i] = to[i] - from[i]): the log index
 * of each change and (out_all_deps optional, [rows * a_stride]) its allDeps row.
 * HM_ERR_INVALID if a slice runs past the document's history. */
int hm_store_read_history(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                          const uint32_t *out_off, uint32_t *out_log_index, uint32_t *out_all_deps);

/* What blocked documents wait for (Automerge 0.12 getMissingDeps; no reference call site: the
 * reference leaves opSet.queue alone until the dependency arrives).  A queued change (hist -1)
 * needs every (actor, seq) of deps.set(actor, seq - 1) (causallyReady's rule: the change's own actor
 * at seq - 1, whatever its deps say of that actor); the missing row holds, per actor rank, the
 * largest needed seq that opSet.clock has not reached (0 = no entry).  n_queued > 0 exactly when
 * the row is not zero.  All of these read the rounds already waited for (no batch in flight).
 *
 * hm_store_blocked: handles of the store's documents that hold queued changes, ascending;
 * HM_ERR_NOMEM (with *out_n = the count needed) when cap is too small. */
int hm_store_blocked(hm_store *s, uint32_t *out_handles, uint32_t cap, uint32_t *out_n);
/* Per requested document (a handle may repeat): the missing row, the unmet minimumClock row
 * (min_clock[a] where DocBackend.clock[a] < min_clock[a], else 0; all zero without
 * hm_doc_set_min_clock) and the queue length (each output may be NULL). */
int hm_store_waiting(hm_store *s, uint32_t n, const uint32_t *doc_handles,
                     uint32_t *out_missing /* [n*S] */, uint32_t *out_unmet_min /* [n*S] */, uint32_t *out_n_queued /* [n] */);
/* opSet.queue of each requested document as log indices in queue order: request i writes rows
 * out_off[i] .. out_off[i+1]-1, out_off[i+1] - out_off[i] = its queue length (from
 * hm_store_waiting's out_n_queued); a mismatch is HM_ERR_INVALID. */
int hm_store_read_queue(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *out_off, uint32_t *out_log_index);
/* The missing rows of a merged cold batch, [n_docs * a_stride]; a document whose status is not HM_OK
 * gets a zero row.  _device: b's docs / changes / deps, r's docs / clock / hist and out_missing are
 * device memory, enqueued on `stream` (NULL = the engine's) without synchronising; _host: host
 * tables in, host rows out (staged, synchronous). */
int hm_missing_deps_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t *out_missing, void *stream);
int hm_missing_deps_host(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t *out_missing);

/* Which of a document's changes a peer lacks, given the peer's clock (Automerge 0.12
 * Backend.getMissingChanges(state, have); getChanges(old, new) is the same with old's opSet.clock;
 * the reference's sync loop asks it when a peer's clock arrives, src/RepoBackend.ts:394-428).
 *   transitiveDeps(have): deps = {}; for (actor, seq) of have IN ITS KEY ORDER, seq > 0:
 *       deps = max-merge(deps, states[actor][seq-1].allDeps)   -- no such state: nothing merged
 *       deps[actor] = seq                                      -- set after the merge: it can lower the entry
 *   missing = history.filter(c => c.seq > (deps[c.actor] || 0))
 * so the answer is in history (application) order, never holds a queued (hist -1) or duplicate
 * (hist -2) change, and depends on the entries' order when `have` is not causally closed.
 *
 * Requests i = 0..n-1: document doc_handles[i] (a handle may repeat), entries entry_off[i] ..
 * entry_off[i+1]-1 of (entry_actor rank, entry_seq) in the have-clock's key order (entry_off[0] = 0,
 * not decreasing; a rank at most once per request).  out_closure (optional, [n*S]) = the
 * transitiveDeps row; out_range [2n] = (offset into out_log_index, count) per request; the blocks
 * lie in unspecified order, each block holds log indices in history order.  *out_total = rows
 * needed; HM_ERR_NOMEM when that exceeds cap (the ranges' counts, out_closure and *out_total are still
 * valid, out_log_index is not; out_log_index may be NULL when cap is 0).  HM_ERR_INVALID: a handle
 * outside the store, a rank >= a_stride, a rank repeated within a request, bad entry_off.  No batch
 * in flight.  A call's rows stay below 2^32.
 * flags: HM_MC_RAW: the entries are the threshold row itself (no fold; ranks not listed read 0);
 * HM_MC_ONLY_LISTED: changes of actors without an entry are left out.  getChangesForActor(a, n) is
 * HM_MC_RAW | HM_MC_ONLY_LISTED with the one entry (a, n). */
#define HM_MC_RAW 1u
#define HM_MC_ONLY_LISTED 2u
int hm_store_missing_changes(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *entry_off,
                             const uint16_t *entry_actor, const uint32_t *entry_seq, uint32_t flags,
                             uint32_t *out_closure, uint32_t *out_range, uint32_t *out_log_index,
                             uint32_t cap, uint32_t *out_total);
/* The same for the documents of a merged cold batch: request i = document i of b (n = b->n_docs), read
 * from b's docs / changes and r's docs / hist / all_deps; a document whose status is not HM_OK offers
 * nothing.  n_entries = rows of entry_actor / entry_seq (= entry_off[n_docs]).
 * _device: every table, the entry arrays and the outputs are device memory, enqueued on `stream`
 * (NULL = the engine's) without synchronising; *out_total and *out_bad are device words the caller
 * zeroes first (*out_bad != 0 afterwards: 2 a rank >= a_stride, 4 a repeated rank, 8 bad entry_off;
 * such a request has the range (0, 0)); blocks are written only while offset + count <= cap.
 * _host: host tables in, host rows out (staged, synchronous), errors as hm_store_missing_changes. */
int hm_missing_changes_device(hm_engine *e, const hm_batch *b, const hm_results *r, const uint32_t *entry_off,
                              const uint16_t *entry_actor, const uint32_t *entry_seq, uint32_t n_entries, uint32_t flags,
                              uint32_t *out_closure, uint32_t *out_range, uint32_t *out_log_index, uint32_t cap,
                              uint32_t *out_total, uint32_t *out_bad, void *stream);
int hm_missing_changes_host(hm_engine *e, const hm_batch *b, const hm_results *r, const uint32_t *entry_off,
                            const uint16_t *entry_actor, const uint32_t *entry_seq, uint32_t flags,
                            uint32_t *out_closure, uint32_t *out_range, uint32_t *out_log_index, uint32_t cap,
                            uint32_t *out_total);

/* A document as it was: resident documents materialized at a past history point, many per call
 * (src/RepoBackend.ts:570-579 MaterializeMsg: Backend.applyChanges(Backend.init(), history.slice(0, n));
 * src/RepoBackend.ts:238-257 loadDocument: each actor's changes.slice(0, cursor[actor])).
 * Request i = document doc_handles[i] (a handle may repeat) with one selector; exactly one of the
 * two arrays is not NULL:
 *   hist_len[i]                   the applied changes at history positions < min(hist_len[i], history.size)
 *   clock_rows[i*a_stride ..]     the applied changes with seq <= clock[actor rank] (0 = none of that actor)
 * Queued (hist -1) and duplicate (hist -2) changes are never selected.  The selected changes are
 * compacted on the device in history order, whatever order the log arrived in, into a cold batch
 * (request i = document i, tables in request order, dep_off / op_first rewritten; register, object
 * and rank ids are the document's own, so n_regs / n_objs / n_actors / flags are the document's
 * totals) and that batch is merged from Backend.init() with the batch kernels.  The resident state
 * is only read.  A clock that is not causally closed leaves queued changes in the result
 * (n_queued > 0), as applyChanges would. */
typedef struct {          /* 64 B */
    uint64_t totals[4];   /* changes, deps, ops, registers of all requests */
    uint32_t max_changes, max_ops, max_regs, max_objs, max_deps, doc_flags;  /* hm_batch launch hints */
    uint32_t bad;         /* _device form: 1 a handle outside the source, 2 a change row outside its document
                           * (store forms also: 4 a bad actor order row, 8 a bad fork / merge destination,
                           * 16 a bad merge map) */
    uint32_t pad;
} hm_past_summary;
typedef struct {
    uint32_t cap_changes, cap_deps, cap_ops, cap_regs;   /* rows the per-change / dep / op / register tables hold */
    /* the gathered batch (each may be NULL) */
    hm_doc_row    *docs;        /* [n] every range of request i */
    hm_change_row *changes;     /* [cap_changes] */
    hm_dep_row    *deps;        /* [cap_deps] */
    hm_op_row     *ops;         /* [cap_ops] */
    uint32_t      *change_log;  /* [cap_changes] log index of gathered change j (hm_doc_log's rows) */
    uint32_t      *op_log;      /* [cap_ops] the document's log op index of gathered op k */
    /* its merge (each may be NULL): docs / clock / back_clock / heads per request, hist / all_deps per
     * gathered change, regs [cap_regs], surv [cap_ops]; a survivor's `op` indexes the gathered ops */
    hm_results res;
} hm_past_out;
/* The count pass alone: out_counts [4n] = n_changes, n_deps, n_ops, n_regs per request, out_totals [4]
 * their sums (either may be NULL).  HM_ERR_INVALID: a handle outside the store, both or neither
 * selector.  No batch in flight. */
int hm_store_past_sizes(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *hist_len,
                        const uint32_t *clock_rows, uint32_t *out_counts, uint64_t *out_totals);
/* Gather + merge on the engine stream, results as host tables.  out_totals [4] (optional) = rows
 * needed per table; HM_ERR_NOMEM with out_totals filled and no other output written when one
 * exceeds its capacity.  HM_ERR_INVALID (outputs untouched): a handle outside the store, both or
 * neither selector; a call between submit and wait is refused.  The totals are read back once
 * between the count and the fill pass (the merge launch is sized by them); the call synchronises
 * once more at its end. */
int hm_store_materialize(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *hist_len,
                         const uint32_t *clock_rows, const hm_past_out *out, uint64_t *out_totals);
/* Fork: resident documents as they were, kept as new resident documents (src/RepoFrontend.ts:95-99
 * Repo.fork = create() + merge(fork, parent); src/RepoBackend.ts:213-217 the merge = cursors.update +
 * syncReadyActors, which hands the new document each listed actor's changes 1 .. clock[actor], actor
 * after actor).  Request i = document src_handles[i] (only read; a handle may repeat) with
 * hm_store_materialize's selectors, into the empty document dst_handles[i]: afterwards that document
 * is indistinguishable from a fresh one that received the selected changes, in the stated order, in
 * one applyChanges round.  It keeps the parent's id spaces (ranks, object and register ids; n_actors /
 * n_regs / n_objs / flags are the parent's totals).
 *   actor_order == NULL   history order (the parent's own), the only order a history length allows
 *   actor_order           with clock_rows only: row i ([a_stride], HM_NONE ends it) lists actor ranks in
 *                         hand-over order (the clock's key order); each contributes its seqs
 *                         1 .. min(clock[a], opSet.clock[a]) ascending.  Every rank whose clock entry
 *                         selects a change must be listed, none twice, all below the document's n_actors.
 *   HM_FORK_MIN_CLOCK     the fork gets the parent's minimumClock row (hm_doc_set_min_clock); without it
 *                         the fork has none (a row an earlier, undone fork left is cleared)
 * The selection is gathered on the device into a buffer of the store and handed to the device-table
 * submit: no row passes through the host, the one read-back is the count pass's totals.  The call is
 * the store's batch in flight: hm_batch_wait / hm_batch_wait_device return one row per request, a
 * merge that throws rolls its destination back, hm_batch_undo empties every destination again.  A
 * selection of no changes leaves the destination an empty document (with the parent's totals).
 * HM_ERR_INVALID, nothing changed: n == 0, both or neither selector, an order with hist_len, a bad
 * order row, a source outside the store, a destination that is outside the store, repeated, also a
 * source, or holds changes (or totals above its parent's), a batch in flight.  A call's rows stay below
 * 2^32 (HM_ERR_NOMEM).  The destinations' minimumClock rows are written once the checks have passed,
 * before the submit: a call that fails later (HM_ERR_NOMEM / HM_ERR_DEVICE from the submit) leaves them
 * replaced — the parent's row, or none — on otherwise unchanged, empty destinations; a row the caller
 * had set on an empty destination with hm_doc_set_min_clock does not survive a fork into it either way. */
#define HM_FORK_MIN_CLOCK 1u
int hm_store_fork_submit(hm_store *s, uint32_t n, const uint32_t *src_handles, const uint32_t *hist_len,
                         const uint32_t *clock_rows, const uint32_t *actor_order, const uint32_t *dst_handles, uint32_t flags,
                         uint64_t *out_batch_id);
/* Merge into a live document: resident documents' changes handed to other resident documents that may
 * already hold changes (src/RepoBackend.ts:213-217 RepoBackend.merge = cursors.update + syncReadyActors,
 * which hands the target each listed actor's changes above what it was handed before, up to
 * clock[actor], actor after actor).  Request i = the changes of document src_handles[i] (only read; a
 * handle may repeat) that are applied there with have[a] < seq <= clock[a], into document
 * dst_handles[i]:
 *   clock_rows   [n * a_stride], required; have_rows [n * a_stride] or NULL (no lower bound); both in
 *                the SOURCE's rank space
 *   actor_order  as hm_store_fork_submit's (source ranks; NULL = the source's history order); with it
 *                actor a contributes max(0, min(clock[a], opSet.clock[a]) - have[a]) changes
 * The two documents' id spaces differ, so the selected rows are renamed on the device through maps the
 * caller builds (it holds both documents' interners):
 *   totals       [4n] the destination's n_actors, n_regs, n_objs after the merge and flags to OR in
 *   rank         [n * a_stride] source rank -> destination rank (after the merge)
 *   obj / reg    CSR per request (off [n + 1], starting at 0): source object / register id ->
 *                destination id; str / content: the same for string-pool and content ids, optional
 *                (NULL map: identity, its off is not read)
 * A change row's actor goes through rank, its content_id through content; a dep row's actor through
 * rank; an op row's obj through obj, reg (unless HM_NONE) and parent (unless HM_HEAD) through reg, key
 * (set / del / link / inc ops) through str, value through str (HM_V_STR) or obj (HM_V_OBJ); elem and
 * everything else stay.  An id at or beyond its slice, a map entry of HM_NONE, or an image at or beyond
 * the stated totals is never read through and refuses the call.
 * dst_actor_remap is hm_batch_submit's actor_remap for the destinations ([n * a_stride] bytes, old rank
 * -> new rank; NULL = no destination's ranks moved).
 * No row passes through the host.  The call reads back twice before the submit: the totals with the
 * verdicts on handles, order rows and destinations after the count pass, and the maps' verdict after
 * the rename pass.  It is then the store's batch in flight: hm_batch_wait returns one row per request,
 * the result of the destination's WHOLE log; a merge that throws rolls only that destination back;
 * hm_batch_undo restores every destination (ranks mapped back).  An empty selection leaves the
 * destination's log as it was (it takes the stated totals) and returns its current result row.  The
 * destinations' minimumClock rows are not touched.
 * HM_ERR_INVALID, nothing changed: n == 0, no clock_rows, a bad order row, a handle outside the store, a
 * destination outside the store, named twice, also a source of the call, with stated totals below its
 * current ones or n_actors > a_stride, a bad map, offsets that decrease, a batch in flight. */
typedef struct {
    const uint32_t *totals;                    /* [4n] n_actors, n_regs, n_objs, flags */
    const uint32_t *rank;                      /* [n * a_stride] */
    const uint32_t *obj_off, *obj_map;         /* [n + 1], [obj_off[n]] */
    const uint32_t *reg_off, *reg_map;
    const uint32_t *str_off, *str_map;         /* str_map NULL: identity */
    const uint32_t *content_off, *content_map; /* content_map NULL: identity */
} hm_merge_maps;
int hm_store_merge_from_submit(hm_store *s, uint32_t n, const uint32_t *src_handles, const uint32_t *have_rows,
                               const uint32_t *clock_rows, const uint32_t *actor_order, const uint32_t *dst_handles,
                               const hm_merge_maps *maps, const uint8_t *dst_actor_remap, uint64_t *out_batch_id);
/* The gather alone over the tables of a merged cold batch (b's docs / changes / deps / ops, r's docs /
 * hist), everything in device memory, enqueued on `stream` (NULL = the engine's) without
 * synchronising.  Request i = document doc_index[i] of b (NULL: document i); hist_len / clock_rows
 * as above (device).  out's docs / changes / deps / ops / change_log / op_log are required device
 * tables of the given capacities (out->res is not read): the gathered batch is left there for the
 * caller's own hm_merge_device, sized by *out_summary (device; read it after synchronising).  `work`
 * and out->ops must be 16-byte aligned (the counts and the op rows move as 16-byte words; hipMalloc
 * memory is; HM_ERR_INVALID otherwise).  n == 0: *out_summary is zeroed and nothing else is touched
 * (work may be NULL).  When
 * a total exceeds its capacity nothing is gathered.  `work` = device memory of
 * hm_materialize_work_bytes(n) bytes; afterwards its first 4n words are the per-request counts and
 * the next 4n their offsets.  A document of b whose status is not HM_OK offers nothing. */
size_t hm_materialize_work_bytes(uint32_t n);
int hm_materialize_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                          const uint32_t *hist_len, const uint32_t *clock_rows, const hm_past_out *out,
                          hm_past_summary *out_summary, void *work, void *stream);

/* What each applied op of a history slice did to the document: the per-op diffs of Automerge's
 * makePatch (the patch of src/RepoBackend.ts:570-579 MaterializeMsg and of every applyChanges), read
 * off the resident tables without replaying anything.  Request i = document doc_handles[i] (a handle
 * may repeat) with the applied changes at history positions from[i] <= p < min(to[i], history.size).
 * In application order (history position of the change, op index in the change) the ops emit
 *   make op                                   one HM_OD_CREATE row
 *   ins                                       nothing
 *   set / del / link / inc with a register    one row: the register as it stands after that op,
 *   (reg < n_regs) on a map or table object   HM_OD_SET with its survivors (winner first, then the
 *                                             conflicts), or HM_OD_REMOVE when none is left
 * The survivors of an assign k on a register are taken over A(k), the applied assigns on it up to and
 * including k in the whole history: a set / link x survives when no later set / del / link y of A(k)
 * has all_deps[change(y)][actor(x)] >= seq(x); a numeric counter set adds the later incs of A(k) that
 * cover it the same way, in application order (INT + INT stays INT, else an f64 sum tagged FLOAT);
 * the order is actor rank descending, and of two survivors x before y of one change y comes first
 * exactly when A(k) holds an odd number of ops at or after y (applyAssign's sortBy(actor).reverse()).
 * Queued (hist -1) and duplicate (hist -2) changes contribute nothing.  A range that holds an assign
 * on an object made by makeList / makeText is flagged HM_OD_LISTS and gets no rows (a list element's
 * diff needs its index at that moment: the caller replays such a range on the host); a range that
 * only creates or inserts into a list is answered. */
#define HM_OD_CREATE 0u
#define HM_OD_SET 1u
#define HM_OD_REMOVE 2u
#define HM_OD_LISTS 1u      /* request flag: no rows, replay the range on the host */
typedef struct {          /* 16 B */
    uint32_t op;          /* document-local op index, as hm_doc_log orders them */
    uint32_t kind;        /* HM_OD_CREATE | HM_OD_SET | HM_OD_REMOVE; with HM_ODF_LISTS also HM_OD_ELEM_* */
    uint32_t n_surv;
    uint32_t surv_off;    /* into the call's table of hm_surv_result: winner first, then conflicts
                             (a survivor's `op` is a document-local op index too) */
} hm_op_diff;
typedef struct {          /* 64 B */
    uint64_t totals[4];   /* diff rows and survivor rows of all requests, 0, 0 */
    uint32_t max_rows, reserved[3], max_surv;   /* the largest request */
    uint32_t flags;       /* OR of the requests' flags */
    uint32_t bad;         /* _device form: 1 a handle outside the source, 2 a change row outside its document,
                             4 a document that outgrows the work memory */
    uint32_t pad;
} hm_op_diff_summary;
typedef struct {
    uint32_t cap_rows, cap_surv;   /* rows the two tables hold */
    hm_op_diff     *rows;          /* [cap_rows] request order, application order within a request */
    hm_surv_result *surv;          /* [cap_surv] */
    uint32_t       *range;         /* [2n] (first row, rows) per request */
    uint32_t       *flags;         /* [n] HM_OD_* per request */
} hm_op_diff_out;
/* The count pass alone: out_counts [2n] = diff rows, survivor rows per request, out_flags [n],
 * out_totals [2] the sums (each may be NULL).  HM_ERR_INVALID: a handle outside the store.  No batch
 * in flight. */
int hm_store_op_diff_sizes(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                           uint32_t *out_counts, uint32_t *out_flags, uint64_t *out_totals);
/* The rows as host tables (out->range and out->flags are required, the two tables when their
 * capacity is not 0).  out_totals [2] (optional) = rows needed per table; HM_ERR_NOMEM with out_totals
 * filled and no other output written when one exceeds its capacity; HM_ERR_INVALID (outputs
 * untouched) for a handle outside the store; a call between submit and wait is refused.  n == 0
 * launches nothing. */
int hm_store_op_diffs(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                      const hm_op_diff_out *out, uint64_t *out_totals);
/* The same over the tables of a merged cold batch (b's docs / changes / ops, r's docs / hist /
 * all_deps), everything in device memory, enqueued on `stream` (NULL = the engine's) without
 * synchronising.  Request i = document doc_index[i] of b (NULL: document i).  *out_summary (device)
 * is valid after synchronising; when a total exceeds its capacity nothing is written to out.
 * `work` = device memory of hm_op_diffs_work_bytes(b, n) bytes (b's counts and launch hints are
 * read, not its tables; without max_ops / max_regs / max_objs hints the batch totals size it),
 * 16-byte aligned as b->ops must be (HM_ERR_INVALID otherwise); afterwards its first 4n words are
 * the per-request counts (rows, survivors, 0, 0) and the next 4n their offsets.  n == 0:
 * *out_summary is zeroed and nothing else is touched.  A document whose status is not HM_OK offers
 * nothing. */
size_t hm_op_diffs_work_bytes(const hm_batch *b, uint32_t n);
int hm_op_diffs_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                       const uint32_t *from, const uint32_t *to, const hm_op_diff_out *out,
                       hm_op_diff_summary *out_summary, void *work, void *stream);
/* _host: host tables in, host rows out (staged, synchronous), errors as hm_store_op_diffs. */
int hm_op_diffs_host(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                     const uint32_t *from, const uint32_t *to, const hm_op_diff_out *out, uint64_t *out_totals);

/* The same calls with an option word; opts = 0 is the call above, bit for bit.
 *
 * HM_ODF_LISTS: list / text element assigns are answered too.  For an applied set / del / link / inc k
 * on the register of element e of list L, with `after` = the register holds survivors after k and
 * `before` = it did after the previous applied assign on e (false without one):
 *   before  after   row
 *   yes     yes     HM_OD_ELEM_SET     survivors as HM_OD_SET
 *   yes     no      HM_OD_ELEM_REMOVE
 *   no      yes     HM_OD_ELEM_INSERT  survivors as HM_OD_SET; the element id is regs[ops[op].reg]
 *   no      no      no row (a del or an inc on an element that is not visible)
 * The row's index = the elements of L before e in L's RGA order whose register held survivors just
 * before k: it travels in out_index [out->cap_rows], parallel to out->rows (HM_NONE for create and
 * map / table rows; required when cap_rows != 0; not read with opts = 0).  RGA order: the pre-order of
 * the tree of the applied ins ops below `to` from _head, siblings by (elem, actor rank) descending.
 * Nothing is replayed for it: the order comes from a sort and a ranked Euler tour of those ins rows,
 * the visibility from the same survivor rule.
 * Only a document whose HM_DOC_HAS_LISTS hint is set is answered this way.  Every encoder of this
 * project sets the hint and a store ORs it over a document's batches, so its own paths always are; a
 * foreign table that assigns list elements without the hint gets HM_OD_LISTS and no rows, as with
 * opts = 0 (the safe answer: replay it on the host).  An element assign on a register that no applied
 * ins of the prefix made (not a merge's tables) emits no row and fails the call like a change row
 * outside its document (HM_ERR_INVALID; _device: bad & 2).
 * The work memory of hm_op_diffs_device_ex is hm_op_diffs_work_bytes_ex(b, n, opts) bytes: with
 * HM_ODF_LISTS and HM_DOC_HAS_LISTS in b->doc_flags (0 = unknown counts as set) a wave's slice is
 * sized for the order phase as well.
 *
 * HM_ODF_ONCE (hm_store_op_diffs_ex only; every other call of this group answers HM_ERR_INVALID,
 * hm_op_diffs_work_bytes_ex 0): one walk instead of count, scan and fill, for a caller that guesses the
 * table sizes and grows them.  out_totals is required.  A request's rows take a block of the row
 * table sized by the ops of its slice's applied changes (an upper bound: an ins emits no row, every
 * other op at most one), a 64-op step's survivors a block of the survivor table; each block is
 * reserved with one atomic add on the call's totals, so
 *   out->range[2i ..] = (block, rows emitted): the blocks of different requests lie in whatever order
 *                        the waves finished, a block's unused tail is a gap (rows nobody refers to);
 *                        within a request the rows are in application order
 *   surv_off             anywhere in the survivor table (absolute, as always)
 *   out_totals           {sum of the row bounds, survivors}: at least hm_store_op_diff_sizes_ex's
 *                        rows and at most the ops of the slices; exactly its survivors unless a
 *                        request is flagged
 * A block that does not fit under cap_rows / cap_surv is not written and the walk goes on: the totals
 * are exact whatever the capacities, the call answers HM_ERR_NOMEM with them and no other output
 * written, and the same call with tables of those sizes succeeds.  A request that turns out flagged
 * (HM_OD_LISTS: without HM_ODF_LISTS, or without the hint) gets (block, 0); what its walk wrote is
 * unreferenced and stays counted in the totals.  Rows, survivors, indices, counts and flags are
 * otherwise those of the call without the bit. */
#define HM_ODF_LISTS 1u
#define HM_ODF_ONCE 2u
#define HM_OD_ELEM_INSERT 3u
#define HM_OD_ELEM_SET 4u
#define HM_OD_ELEM_REMOVE 5u
int hm_store_op_diff_sizes_ex(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                              uint32_t *out_counts, uint32_t *out_flags, uint64_t *out_totals, uint32_t opts);
int hm_store_op_diffs_ex(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *from, const uint32_t *to,
                         const hm_op_diff_out *out, uint32_t *out_index, uint64_t *out_totals, uint32_t opts);
size_t hm_op_diffs_work_bytes_ex(const hm_batch *b, uint32_t n, uint32_t opts);
int hm_op_diffs_device_ex(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                          const uint32_t *from, const uint32_t *to, const hm_op_diff_out *out, uint32_t *out_index,
                          hm_op_diff_summary *out_summary, void *work, void *stream, uint32_t opts);
int hm_op_diffs_host_ex(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                        const uint32_t *from, const uint32_t *to, const hm_op_diff_out *out, uint32_t *out_index,
                        uint64_t *out_totals, uint32_t opts);

/* The same rows for a document as it stood at a clock (RepoBackend's loadDocument at a cursor: each
 * actor's changes.slice(0, cursor[actor])) instead of a history slice.  Request i = (doc_handles[i],
 * clock_rows[i * a_stride ..]): per actor rank the largest seq selected, as hm_store_materialize's
 * clock selector takes it.  A change is applied at clock K when it is applied in the resident
 * document, its seq <= K[its actor] and every entry of its causal past (its all_deps row) is <= K:
 * exactly what applyChanges(Backend.init(), the selected changes) applies; the other selected
 * changes are hm_store_materialize's n_queued and contribute nothing.  The rows are the whole patch
 * from the empty document: every applied-at-K op is in range, and a register's survivors, a counter's
 * value and an element's index count the applied-at-K ops alone.  Row order is the resident history
 * order restricted to those changes (as for hm_store_materialize's clock selector), not loadDocument's
 * actor-major hand-over order; both lead a frontend to the same document.  The all-zero clock gives
 * no rows; a clock at or above every seq gives the call over [0, history size).  A handle may repeat
 * with different clocks.
 * Outputs, request-order layout, out_index, flags, HM_ERR_NOMEM with exact totals, HM_ERR_INVALID and
 * the refusal between submit and wait are those of the _ex calls; opts takes HM_ODF_LISTS only
 * (HM_ODF_ONCE: HM_ERR_INVALID, hm_op_diffs_at_work_bytes 0).  Nothing is re-merged: a select phase
 * per request leaves a bit per log change in the wave's work memory and the walk reads it. */
int hm_store_op_diff_sizes_at(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *clock_rows,
                              uint32_t *out_counts, uint32_t *out_flags, uint64_t *out_totals, uint32_t opts);
int hm_store_op_diffs_at(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *clock_rows,
                         const hm_op_diff_out *out, uint32_t *out_index, uint64_t *out_totals, uint32_t opts);
/* Over a merged cold batch, as hm_op_diffs_device_ex / _host_ex: clock_rows [n * b->a_stride] in
 * device (_device) or host (_host) memory; `work` of hm_op_diffs_at_work_bytes(b, n, opts) bytes. */
size_t hm_op_diffs_at_work_bytes(const hm_batch *b, uint32_t n, uint32_t opts);
int hm_op_diffs_at_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                          const uint32_t *clock_rows, const hm_op_diff_out *out, uint32_t *out_index,
                          hm_op_diff_summary *out_summary, void *work, void *stream, uint32_t opts);
int hm_op_diffs_at_host(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                        const uint32_t *clock_rows, const hm_op_diff_out *out, uint32_t *out_index,
                        uint64_t *out_totals, uint32_t opts);

/* The current state of many documents in one call: a stream compaction of each request's live
 * registers (what hm_doc_read hands out one document at a time, without the dead registers and the
 * survivor slack).  Request i = document doc_handles[i] (a handle may repeat).  A register is live
 * when n_surv > 0, obj != HM_NONE and obj < n_objs; one hm_state_row per live register, in ascending
 * register id, request after request; the survivors are copied in row order (op, vtag and value
 * unchanged), wherever the incremental path left them inside the document's slots.  Nothing is
 * re-merged and the device needs no object types: placing list elements by `index` is the
 * consumer's part. */
typedef struct {          /* 20 B, five 32-bit words */
    uint32_t reg;         /* document-local register id */
    uint32_t obj;         /* as hm_reg_result.obj */
    int32_t  index;       /* as hm_reg_result.list_index (-1: not a visible list element) */
    uint32_t n_surv;
    uint32_t surv_off;    /* into the call's hm_surv_result table: winner first, then conflicts */
} hm_state_row;
#define HM_ST_BAD_ROWS 1u   /* request flag: a live register's survivors (or the document's register
                               segment) lie outside the document's slots; the request gets no rows */
typedef struct {          /* 64 B */
    uint64_t totals[2];   /* state rows and survivor rows of all requests */
    uint64_t reserved64[2];
    uint32_t max_rows, reserved[3], max_surv;   /* the largest request */
    uint32_t flags;       /* OR of the requests' flags */
    uint32_t bad;         /* _device form: 1 a handle outside the source */
    uint32_t pad;
} hm_state_summary;
typedef struct {
    uint32_t cap_rows, cap_surv;   /* rows the two tables hold */
    hm_state_row   *rows;          /* [cap_rows] request order, ascending register id within a request */
    hm_surv_result *surv;          /* [cap_surv] row order */
    uint32_t       *range;         /* [4n] (first row, rows, first survivor, survivors) per request */
    uint32_t       *flags;         /* [n] HM_ST_* per request */
} hm_state_out;
/* The count pass alone: out_counts [2n] = state rows, survivor rows per request, out_flags [n],
 * out_totals [2] the sums (each may be NULL).  HM_ERR_INVALID: a handle outside the store.  No batch
 * in flight. */
int hm_store_state_sizes(hm_store *s, uint32_t n, const uint32_t *doc_handles, uint32_t *out_counts, uint32_t *out_flags,
                         uint64_t *out_totals);
/* The rows as host tables (out->range and out->flags are required, the two tables when their
 * capacity is not 0).  out_clock / out_heads (optional, [n * a_stride]): the requests' opSet.clock and
 * opSet.deps rows, gathered by the same launches.  out_totals [2] (optional) = rows needed per table;
 * HM_ERR_NOMEM with out_totals filled and no other output written when one exceeds its capacity (or
 * the call's rows reach 2^32); HM_ERR_INVALID (outputs untouched) for a handle outside the store; a
 * call between submit and wait is refused.  n == 0 launches nothing. */
int hm_store_state(hm_store *s, uint32_t n, const uint32_t *doc_handles, const hm_state_out *out, uint32_t *out_clock,
                   uint32_t *out_heads, uint64_t *out_totals);
/* The same over a merged cold batch (b's docs, r's docs / regs / surv and, when asked for, clock /
 * heads), everything in device memory, enqueued on `stream` (NULL = the engine's) without
 * synchronising.  Request i = document doc_index[i] of b (NULL: document i); a document whose status
 * is not HM_OK offers nothing.  *out_summary (device) is valid after synchronising; when a total
 * exceeds its capacity nothing is written to out, out_clock or out_heads.  `work` = device memory of
 * hm_state_work_bytes(n) bytes, 16-byte aligned as r->regs and r->surv must be (HM_ERR_INVALID
 * otherwise); afterwards its first 4n words are the per-request counts (rows, survivors, 0, 0) and
 * the next 4n their offsets.  n == 0: *out_summary is zeroed and nothing else is touched. */
size_t hm_state_work_bytes(uint32_t n);
int hm_state_device(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                    const hm_state_out *out, uint32_t *out_clock, uint32_t *out_heads, hm_state_summary *out_summary,
                    void *work, void *stream);
/* _host: host tables in, host rows out (staged, synchronous), errors as hm_store_state. */
int hm_state_host(hm_engine *e, const hm_batch *b, const hm_results *r, uint32_t n, const uint32_t *doc_index,
                  const hm_state_out *out, uint32_t *out_clock, uint32_t *out_heads, uint64_t *out_totals);

/* The fields a proposed local change touches (the undo bookkeeping of Automerge 0.12
 * applyLocalChange, src/DocBackend.ts:187-205: applyAssign's recordUndo reads fieldOps of every
 * (obj, key) the request assigns and tests isConcurrent against the request), read off the resident
 * tables without touching the document.
 *   request   = a document, the would-be change's base clock as ordered (actor rank, seq) entries
 *               — its deps in key order with its own actor at seq - 1: base = {...deps};
 *               base[actor] = seq - 1, so the own actor keeps its place if deps names it and goes
 *               last otherwise — and a list of registers
 *   ready     = every entry has seq <= opSet.clock[actor] (causallyReady).  A request that is not
 *               ready gets HM_FLD_NOT_READY and no rows (Automerge queues it: an empty undo list)
 *   closure   = transitiveDeps(entries), exactly hm_store_missing_changes's fold (order dependent
 *               when the entries are not causally closed): applyChange's allDeps of the request
 *   per register, in request order: its current survivors, winner first then the conflicts
 *               (fieldOps, the order of hm_reg_result / hm_surv_result); per survivor one hm_field_op:
 *               the document-local op index, the op row's action (HM_SET | HM_LINK) and datatype, the
 *               resolved vtag / value, its change's (actor rank, seq) and
 *               covered = closure[actor] >= seq: the request is not concurrent with it, so a set /
 *               del / link of the request removes it and an inc adds to it when it is a counter set
 *   a register at or past the document's n_regs, or one never touched, answers zero rows.
 *
 * Requests i = 0..n-1: document doc_handles[i] (a handle may repeat), entries entry_off[i] ..
 * entry_off[i+1]-1 (entry_off[0] = 0, not decreasing; a rank at most once per request), registers
 * field_reg[field_off[i] .. field_off[i+1]-1] (field_off[0] = 0, not decreasing; a register may
 * repeat).  out_flags [n] = HM_FLD_* per request (HM_FLD_BAD_ROWS: a survivor whose op lies in no
 * change of the document, or a register row outside the tables — not a merge's tables; its row has
 * actor 0xFFFF); out_closure (optional, [n*S]) = the closure row (zeros when not ready); out_range
 * [2 * n_fields] = (first row, rows) per field, n_fields = field_off[n]; the requests' blocks lie in
 * unspecified order, inside a block the rows are in field order, then survivor order.  *out_total =
 * rows needed; HM_ERR_NOMEM when that exceeds cap (flags, closure rows, the ranges' counts and
 * *out_total are still valid, out_rows is not; out_rows may be NULL when cap is 0).  HM_ERR_INVALID
 * (the outputs' content is then unspecified, *out_total 0): a handle outside the store, a rank >=
 * a_stride, a rank repeated within a request, bad entry_off / field_off.  No batch in flight.  n == 0
 * launches nothing.  A call's rows stay below 2^32.  One kernel launch per call; the per-request
 * outputs and a row table of at most 64 KiB come back with the counters (one wait for the device),
 * a larger table's rows in a second copy. */
typedef struct {          /* 24 B */
    uint32_t op;          /* document-local op index, as hm_doc_log orders them */
    uint32_t seq;         /* of the op's change */
    uint16_t actor;       /* rank of the op's change */
    uint8_t  action;      /* HM_SET | HM_LINK */
    uint8_t  datatype;    /* HM_DT_* of the op row */
    uint8_t  vtag;        /* HM_V_* of the resolved value (counters may turn INT -> FLOAT) */
    uint8_t  covered;     /* 1: closure[actor] >= seq */
    uint16_t pad;
    uint64_t value;       /* resolved value (counter: base + causally-later incs) */
} hm_field_op;
#define HM_FLD_NOT_READY 1u
#define HM_FLD_BAD_ROWS 2u
int hm_store_fields(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *entry_off,
                    const uint16_t *entry_actor, const uint32_t *entry_seq, const uint32_t *field_off,
                    const uint32_t *field_reg, uint32_t *out_flags, uint32_t *out_closure, uint32_t *out_range,
                    hm_field_op *out_rows, uint32_t cap, uint32_t *out_total);
/* The same for the documents of a merged cold batch: request i = document i of b (n = b->n_docs), read
 * from b's docs / changes / ops and r's docs / clock / hist / all_deps / regs / surv; a document whose
 * status is not HM_OK offers nothing (no rows; ready exactly when every entry's seq is 0).  n_entries /
 * n_fields = rows of the entry / field tables (= entry_off[n_docs] / field_off[n_docs]).
 * _device: every table, the request arrays and the outputs are device memory, enqueued on `stream`
 * (NULL = the engine's) without synchronising; *out_total and *out_bad are device words the caller
 * zeroes first (*out_bad != 0 afterwards: 2 a rank >= a_stride, 4 a repeated rank, 8 bad entry_off,
 * 16 bad field_off: the offsets are checked on the device; such a request has empty ranges); blocks
 * are written only while first row + rows <= cap.
 * _host: host tables in, host rows out (staged, synchronous), errors as hm_store_fields. */
int hm_fields_device(hm_engine *e, const hm_batch *b, const hm_results *r, const uint32_t *entry_off,
                     const uint16_t *entry_actor, const uint32_t *entry_seq, uint32_t n_entries,
                     const uint32_t *field_off, const uint32_t *field_reg, uint32_t n_fields,
                     uint32_t *out_flags, uint32_t *out_closure, uint32_t *out_range, hm_field_op *out_rows,
                     uint32_t cap, uint32_t *out_total, uint32_t *out_bad, void *stream);
int hm_fields_host(hm_engine *e, const hm_batch *b, const hm_results *r, const uint32_t *entry_off,
                   const uint16_t *entry_actor, const uint32_t *entry_seq, const uint32_t *field_off,
                   const uint32_t *field_reg, uint32_t *out_flags, uint32_t *out_closure, uint32_t *out_range,
                   hm_field_op *out_rows, uint32_t cap, uint32_t *out_total);

/* minimumClock row of a document (rank-indexed, 0 = absent); used for the
 * min_cmp of the next merges (Clock.cmp(DocBackend.clock, minimumClock)). */
int hm_doc_set_min_clock(hm_store *s, uint32_t doc, const uint32_t *clock);

/* ClockStore.update(repoId=self, docId, doc.clock) for n documents
 * (src/ClockStore.ts:78-91, called at src/RepoBackend.ts:343-345): the stored
 * row becomes max(stored, DocBackend.clock) per entry.  out_written[i] = 1 if any
 * stored entry changed (the rows SQLite must persist); out_differs[i] = 1 if
 * !Clock.equal(input, stored) (ClockStore pushes updateQ).  out_stored
 * (optional, [n*a_stride]) receives the stored rows. */
int hm_store_clock_update(hm_store *s, uint32_t n, const uint32_t *docs, uint8_t *out_written,
                          uint8_t *out_differs, uint32_t *out_stored);

/* ------------------------------------------------------------------ */
/* CursorStore (src/CursorStore.ts:19-79) on the device                 */
/* ------------------------------------------------------------------ */
/* One repo's Cursors table (schema src/migrations/0001_initial_schema.sql:15-21): per
 * document row (dense indices the caller assigns), up to max_actors_per_doc entries of
 * (actor key, seq); actor key = FNV-1a64 of the actor id (as hm_clock_rec), seq stored
 * boundedSeq-clamped to [0, INFINITY_SEQ = 2^53 - 1].  Entries keep insertion order.
 * It gates syncChanges (src/RepoBackend.ts:506-531): docsWithActor picks the documents of
 * a synced actor and entry bounds each one's range; every call here is a batch. */
typedef struct hm_cursors hm_cursors;
int  hm_cursors_create(hm_engine *e, uint32_t max_actors_per_doc, hm_cursors **out);
void hm_cursors_destroy(hm_cursors *c);
/* rows 0 .. n_rows-1 exist (new rows empty) */
int  hm_cursors_reserve(hm_cursors *c, uint32_t n_rows);
/* CursorStore.update(repoId, docId, cursor) for n_docs documents (src/CursorStore.ts:51-64):
 * document d's entries are [entry_off[d], entry_off[d+1]) of actor_keys / seqs (distinct
 * actors per document; seqs as JS numbers, Infinity allowed); each is an upsert-max
 * (ON CONFLICT DO UPDATE ... WHERE excluded.seq > seq).  out_differs[d] (optional) = 1 if
 * !Clock.equal(cursor, stored cursor after the update), i.e. updateQ is pushed.
 * All or nothing: HM_ERR_INVALID with nothing written if a row would outgrow
 * max_actors_per_doc, a row appears twice in the call, or an actor twice in one row's entries. */
int  hm_cursors_update(hm_cursors *c, uint32_t n_docs, const uint32_t *rows, const uint32_t *entry_off,
                       const uint64_t *actor_keys, const double *seqs, uint8_t *out_differs);
/* CursorStore.get for n rows: out_count[i] entries in out_actor/out_seq [i * max_actors_per_doc ...] */
int  hm_cursors_get(hm_cursors *c, uint32_t n, const uint32_t *rows, uint32_t *out_count, uint64_t *out_actor,
                    uint64_t *out_seq);
/* CursorStore.entry (src/CursorStore.ts:68-70) for n (row, actor) pairs: stored seq or 0 */
int  hm_cursors_entry(hm_cursors *c, uint32_t n, const uint32_t *rows, const uint64_t *actor_keys, uint64_t *out_seq);
/* CursorStore.docsWithActor(repoId, actor, seq) (src/CursorStore.ts:73-75) for n_actors
 * actors at once: every stored entry of one of the actors with seq >= boundedSeq(min_seqs[q])
 * (min_seqs may be NULL = 0) -> (row, query index q, stored seq); order unspecified.
 * *out_n = matches; HM_ERR_NOMEM (nothing copied) when that exceeds cap. */
int  hm_cursors_docs_with_actors(hm_cursors *c, uint32_t n_actors, const uint64_t *actor_keys, const double *min_seqs,
                                 uint32_t cap, uint32_t *out_row, uint32_t *out_actor, uint64_t *out_seq,
                                 uint32_t *out_n);

/* syncChanges contiguity (src/RepoBackend.ts:513-522) over many (doc, actor)
 * pairs on the device: for pair i, walk seq indices j = lo[i] .. hi[i]-1 while
 * bit j of the actor feed's present bitmap (words from present + word_off[i])
 * is set; out_end[i] = first missing index (or hi[i]).  Device pointers. */
int hm_sync_ranges_device(hm_engine *e, const uint64_t *present, const uint64_t *word_off,
                          const uint32_t *lo, const uint32_t *hi, uint32_t *out_end, uint32_t n,
                          void *stream);
/* The same from host arrays (present: n_words u64 bitmap words; staged through the device,
 * synchronous): the syncChanges plan of a batch of (doc, actor) pairs. */
int hm_sync_ranges_host(hm_engine *e, const uint64_t *present, const uint64_t *word_off, const uint32_t *lo,
                        const uint32_t *hi, uint32_t *out_end, uint32_t n, uint32_t n_words);

/* ------------------------------------------------------------------ */
/* Blocks -> columnar rows (host, multi-threaded)                      */
/* ------------------------------------------------------------------ */
/*
 * The host front of the path: hypercore blocks -> Change objects -> the rows above.
 *   replaces: src/Block.ts:18-29 Block.unpack ('{"' raw JSON | 'BR' + brotli(JSON), else throw)
 *             src/JsonBuffer.ts:1-4 JsonBuffer.parse, src/Actor.ts:137-141 Actor.parseBlock
 *             + the host encoder (hypermerge_amd/js/columnar.js), row for row.
 * Blocks of all documents lie back to back in `data`: block i is data[block_off[i] ..
 * block_off[i+1]); document d's blocks (one Change each, in arrival order) are blocks
 * doc_block[d] .. doc_block[d+1]-1.  Documents decode on `threads` threads; the rows do not
 * depend on the thread count.  A document with an undecodable block (the reference's
 * Block.unpack / JSON.parse throw) is reported HM_ERR_INVALID in hm_decoded_status with no
 * rows.  a_stride 0 = the batch's widest document.  Brotli uses the system libbrotlidec.
 */
typedef struct hm_decoded hm_decoded;
int hm_decode_blocks(const uint8_t *data, const uint64_t *block_off, const uint32_t *doc_block, uint32_t n_docs,
                     uint32_t a_stride, int threads, hm_decoded **out);
/* The decoded tables as a host hm_batch (pointers valid until hm_decoded_free). */
int hm_decoded_batch(const hm_decoded *d, hm_batch *out);
const int32_t *hm_decoded_status(const hm_decoded *d);            /* [n_docs] HM_OK / HM_ERR_INVALID */
uint32_t hm_decoded_n_strings(const hm_decoded *d);               /* the string pool (keys, string values) */
const char *hm_decoded_string(const hm_decoded *d, uint32_t i, size_t *len);
const char *hm_decoded_actor(const hm_decoded *d, uint32_t doc, uint32_t rank, size_t *len);
const char *hm_decoded_obj(const hm_decoded *d, uint32_t doc, uint32_t obj, size_t *len);       /* object uuid */
const char *hm_decoded_reg(const hm_decoded *d, uint32_t doc, uint32_t reg, uint32_t *obj, size_t *len); /* key | elemId */
void hm_decoded_free(hm_decoded *d);

/* ------------------------------------------------------------------ */
/* Docset: the Node drop-in's host engine (raw blocks in, patches out)  */
/* ------------------------------------------------------------------ */
/*
 * The documents of one device with everything the JS host used to keep per document: their
 * interners (actor ids ranked in JS string order, object UUIDs, registers, string values,
 * change content identity), their placement in resident stores (one hm_store per actor-stride
 * class 8/16/32/64; a document moves to a wider class when a new actor outgrows its rows) and
 * their patch base.  One hm_docset_apply = one applyChanges round of every listed document:
 *
 *   replaces: src/Actor.ts:137-141 parseBlock, src/Block.ts:18-29 unpack, src/JsonBuffer.ts:1-4
 *             src/DocBackend.ts:169-185 applyRemoteChanges -> Backend.applyChanges -> updateClock
 *             src/DocBackend.ts:144-167 init(changes) (the first call on a document)
 *             Automerge makePatch: {clock, deps, canUndo, canRedo, diffs}
 *
 * Input: the blocks of each document (one Change per block, '{"' JSON or 'BR' + brotli JSON),
 * laid out as in hm_decode_blocks; docs[i] is the docset document of doc_block[i]..[i+1]-1
 * (each at most once per call).  Output (hm_text): per document an hm_doc_result (status:
 * HM_ERR_INVALID with err_change = the block index in this call when a block does not decode
 * (the reference's Block.unpack / JSON.parse throw); an Automerge error status with err_change
 * = the log index (blocks of all successful calls, in order) when applyChanges throws; the
 * document is rolled back either way) and one JSON text
 *   {"p": [patch | null, ...], "b": [clock of the whole log | null, ...], "c": [clock of this call's changes | null, ...]}
 * patch.clock / deps are opSet.clock / opSet.deps; diffs take the document from the previous
 * successful call's patch to this one (objects created, map keys set / removed, list elements
 * removed / inserted / set) in the Automerge 0.12 diff vocabulary; "b" is the max seq per actor
 * over every change of the document's log and "c" over this call's changes (queued ones
 * included: DocBackend.updateClock(changes), src/DocBackend.ts:135-142).
 * Calls on one docset are serialised (a second concurrent call fails); hm_docset_open may run
 * while a call is in flight (it allocates host state only).
 */
typedef struct hm_docset hm_docset;
typedef struct hm_text hm_text;
typedef struct {
    uint32_t threads;     /* host threads for decode / render (0 = min(16, hardware)) */
    uint32_t flags;       /* HM_DOCSET_* */
} hm_docset_config;
#define HM_DOCSET_NO_PATCHES 1u   /* patches carry clock / deps only (no diffs, no register reads) */
#define HM_DOCSET_BINARY 2u       /* hm_docset_apply's text is the binary form below instead of JSON */
#define HM_DOCSET_NET_DIFFS 4u    /* diffs take the previous patch's document to the new one (one per changed
                                     register) instead of Automerge's per-op sequence (the default) */
#define HM_DOCSET_DEVICE_DIFFS 8u /* the per-op sequence of hm_docset_apply's rounds is rendered from the
                                     device's op-diff rows (hm_store_op_diffs_ex with HM_ODF_LISTS |
                                     HM_ODF_ONCE over each round's history slice, one call per stride
                                     class, repeated once with the reported sizes when the guessed tables
                                     are too small) instead of replayed on the host: the docset then
                                     keeps no replay state (per-register survivors, list orders) and does
                                     not read the registers back to check it.  Same patches, byte for
                                     byte.  HM_ERR_INVALID together with HM_DOCSET_NET_DIFFS or
                                     HM_DOCSET_NO_PATCHES. */
/* Binary results ('HMP1', for a host that builds the patch objects itself instead of parsing
 * JSON; a call whose strings hold a lone surrogate falls back to the JSON form, first byte '{'):
 *   u32 header[8] = {0x31504D48, n_docs, n_strings, n_words, n_nums, blob_bytes, ascii, 0}
 *   u32 doc_word_off[n_docs + 1], doc_str_base[n_docs + 1], doc_num_base[n_docs + 1]
 *   u32 str_off[n_strings + 1] (byte offsets into blob), u32 words[n_words], pad to 8,
 *   f64 nums[n_nums], u8 blob[blob_bytes]
 * A document's words (string and number indices local to the document): opSet.clock, opSet.deps,
 * the log's clock, this call's clock, each as n then n x (actor string, seq); then n_diffs and
 * per diff a head word (action 0 create | 1 set | 2 remove | 3 insert, type << 3 with type 0 map
 * | 1 table | 2 list | 3 text) followed by: create: obj; map set: obj, key, entry; map remove:
 * obj, key; list remove: obj, index; list insert: obj, index, elemId, entry; list set: obj,
 * index, entry.  entry = n_surv, the winner's value word, then per conflict (actor string, value
 * word); value word = vtag | datatype << 3 | payload << 5 (STR / OBJ: string index, INT / FLOAT:
 * number index). */

int  hm_docset_create(hm_engine *e, const hm_docset_config *cfg, hm_docset **out);
void hm_docset_destroy(hm_docset *ds);
hm_engine *hm_docset_engine(hm_docset *ds);
/* n new, empty documents (Backend.init()) with consecutive ids from *out_first */
int  hm_docset_open(hm_docset *ds, uint32_t n, uint32_t *out_first);
int  hm_docset_apply(hm_docset *ds, const uint8_t *data, const uint64_t *block_off, const uint32_t *doc_block,
                     const uint32_t *docs, uint32_t n_docs, hm_text **out);
const char *hm_text_data(const hm_text *t, size_t *len);
const hm_doc_result *hm_text_results(const hm_text *t, uint32_t *n);
void hm_text_free(hm_text *t);

typedef struct {
    uint32_t a_stride;    /* class of the store the document lives in (0 = not placed yet) */
    uint32_t n_changes, n_ops, n_actors, n_objs, n_regs, hist_len, n_queued;
} hm_docset_doc_info_t;
int hm_docset_doc_info(hm_docset *ds, uint32_t doc, hm_docset_doc_info_t *out);
/* history.slice(0, n) (src/RepoBackend.ts:572-576): log indices in history order; returns the count */
int hm_docset_history_prefix(hm_docset *ds, uint32_t doc, uint32_t n, uint32_t *out_log_index);
/* ClockStore.update(self, docId, doc.clock) for n documents (hm_store_clock_update per class);
 * *out_stored (optional) = JSON array of the stored clocks, in call order */
int hm_docset_clock_update(hm_docset *ds, uint32_t n, const uint32_t *docs, uint8_t *out_written, uint8_t *out_differs,
                           hm_text **out_stored);
/* documents that hold queued changes (hm_store_blocked over every stride class), ids ascending;
 * HM_ERR_NOMEM (with *out_n = the count needed) when cap is too small */
int hm_docset_blocked(hm_docset *ds, uint32_t *out_docs, uint32_t cap, uint32_t *out_n);
/* what n documents wait for: JSON array, per document {"queued":[log indices in queue order],
 * "missing":{"<actorId>":seq}} (Automerge getMissingDeps; hm_store_waiting + hm_store_read_queue
 * per class, ranks mapped back to actor ids) */
int hm_docset_waiting(hm_docset *ds, uint32_t n, const uint32_t *docs, hm_text **out);
/* the changes a peer lacks (hm_store_missing_changes per stride class): request i = document docs[i]
 * (may repeat) with the have-clock entries entry_off[i] .. entry_off[i+1]-1 in the clock's key order;
 * entry k = the actor id string actor_ids[actor_off[k] .. actor_off[k+1]) with seqs[k] (a JS number:
 * NaN and negatives read 0, clamped to 2^32-1, fractions truncated).  An id the document has never
 * seen is dropped (it names none of its changes); an id listed twice in a request is
 * HM_ERR_INVALID.  Result text = JSON [[log indices in history order], ...], one array per request
 * (a document not placed yet: []).  flags: HM_MC_*. */
int hm_docset_missing_changes(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *entry_off,
                              const char *actor_ids, const uint32_t *actor_off, const double *seqs,
                              uint32_t flags, hm_text **out);
/* the fields a proposed change touches (hm_store_fields per stride class, repeated once with the
 * reported size when the guessed row table was too small): request i = document docs[i] (may repeat),
 * the would-be change's base clock given as hm_docset_missing_changes takes a clock (base = {...deps};
 * base[actor] = seq - 1, in key order) — an id the document has never seen is dropped when its seq is
 * 0 and makes the request not ready otherwise — and the fields field_off[i] .. field_off[i+1]-1.
 * Field f = two strings: the object uuid names[name_off[2f] .. name_off[2f+1]) and the key (an elemId
 * for list / text) names[name_off[2f+1] .. name_off[2f+2]); they are looked up in the document's
 * interners, nothing is interned: an unknown object or key is an empty field.  Result text = JSON
 * array, per request {"ready": bool, "fields": [[op, ...], ...]}, a field's ops winner first, op =
 * {"action": "set"|"link", "value": v[, "datatype": "counter"|"timestamp"], "actor": id, "seq": n,
 * "covered": bool} (a link's value is the object uuid).  A request that is not ready has every field
 * empty; a document not placed yet is ready exactly when every seq is 0.  Works whatever the
 * docset's flags. */
int hm_docset_fields(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *entry_off,
                     const char *actor_ids, const uint32_t *actor_off, const double *seqs,
                     const uint32_t *field_off, const char *names, const uint32_t *name_off, hm_text **out);
/* documents as they were (hm_store_materialize per stride class): request i = document docs[i] (may
 * repeat) at history length hist_len[i], or at the clock given as hm_docset_missing_changes takes one
 * (entries entry_off[i] .. entry_off[i+1]-1 of actor id strings and seqs; an id the document has
 * never seen is dropped); exactly one of hist_len and entry_off is not NULL.  Result text = JSON array,
 * per request {"doc": id, "clock": {actorId: seq}, "deps": {actorId: seq}, "history": history.size,
 * "view": the document as hm_docset_view renders it} (a document not placed yet: Backend.init()). */
int hm_docset_materialize(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *hist_len,
                          const uint32_t *entry_off, const char *actor_ids, const uint32_t *actor_off,
                          const double *seqs, hm_text **out);
/* the patch of a document as it was (the reply of src/RepoBackend.ts:570-579 MaterializeMsg:
 * Backend.applyChanges(Backend.init(), history.slice(0, n))[1]): request i = document docs[i] (may
 * repeat) at history length hist_len[i].  Result text = JSON array, per request {"doc": id, "history":
 * history.size of the prefix, "patch": {"clock", "deps", "canUndo": false, "canRedo": false, "diffs"}}:
 * clock and deps are the prefix's (hm_store_materialize), the diffs are Automerge's per-op sequence
 * (create, map set, map remove) rendered from hm_store_op_diffs' rows, nothing replayed on the host.
 * A prefix that assigns list / text elements gets "patch": null and "host": true: the caller replays
 * it.  A document not placed yet: the empty patch.  HM_ERR_UNSUPPORTED on a docset created with
 * HM_DOCSET_NO_PATCHES or HM_DOCSET_NET_DIFFS (it keeps no per-op view of the log). */
int hm_docset_materialize_patch(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *hist_len, hm_text **out);
/* The same with hm_store_op_diffs_ex's option word; opts = 0 is the call above.  HM_ODF_LISTS: the
 * element rows are rendered too (insert with index and elemId, set and remove with index), so text and
 * list documents get their patch from the device; "patch": null with "host": true is then left to a
 * document that assigns list elements without the HM_DOC_HAS_LISTS hint, which no path of this
 * project produces. */
int hm_docset_materialize_patch_ex(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *hist_len, uint32_t opts,
                                   hm_text **out);
/* The patch of a document as it stood at a clock (the patch loadDocument sends when it opens a document
 * at a cursor, src/RepoBackend.ts:238-257): the clocks are given as hm_docset_materialize takes them
 * (entries entry_off[i] .. entry_off[i+1] of request i, actor id strings, an id the document has never
 * seen is dropped).  Per request {"doc", "history": changes applied at the clock, "queued": selected
 * but not applied, "patch": {clock, deps, canUndo: false, canRedo: false, diffs}}: clock and deps from
 * hm_store_materialize at that clock, the diffs rendered from hm_store_op_diffs_at's rows, in the
 * resident history order (not loadDocument's actor-major hand-over order; both lead a frontend to
 * the same document).  opts, "host": true, the empty patch of a document not placed yet and the
 * refusals are those of hm_docset_materialize_patch_ex. */
int hm_docset_materialize_patch_at(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *entry_off, const char *actor_ids,
                                   const uint32_t *actor_off, const double *seqs, uint32_t opts, hm_text **out);
/* Fork (Repo.fork / Repo.merge into a fresh document; hm_store_fork_submit per stride class): n new
 * documents are opened (*out_first = the first one's id, request i gets *out_first + i); request i is
 * parent docs[i] (may repeat) at history length hist_len[i], in the parent's history order, or at the
 * clock given as hm_docset_materialize takes one, handed over actor after actor in entry order (an id
 * the parent never saw is dropped, a repeated id counts once with its last seq); exactly one of
 * hist_len and entry_off is not NULL.  The fork lives in its parent's stride class with the parent's
 * interners and rank tables, the content table of the selected (actor, seq) and the per-op tables of
 * the gathered ops.  *out = what a first hm_docset_apply round handing the fork those changes returns
 * (result rows, the one combined patch, DocBackend.clock), in the docset's format, whatever its flags;
 * actors the fork does not hold appear nowhere in it.  A parent not placed yet gives an empty fork.
 * All-or-nothing as hm_docset_apply is (a failed call leaves the new documents empty). */
int hm_docset_fork(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *hist_len, const uint32_t *entry_off,
                   const char *actor_ids, const uint32_t *actor_off, const double *seqs, uint32_t *out_first, hm_text **out);
/* Merge into live documents (RepoBackend.merge, src/RepoBackend.ts:213-217; hm_store_merge_from_submit
 * per stride class): destination dst_docs[i] (each at most once, none a source of the call) is handed
 * source src_docs[i]'s (may repeat) applied changes above what it was handed before — its
 * DocBackend.clock — up to the clock given as hm_docset_materialize takes one, actor after actor in
 * entry order (an id the source never saw is dropped, a repeated id counts once with its last seq,
 * Infinity clamps).  Every actor, object, register and string of the source is interned into the
 * destination (deps and links may name any); its content table grows by the (actor, seq) entries the
 * selector covers.  *out = what a hm_docset_apply round handing the destinations those changes returns
 * (result rows, one combined patch per destination, DocBackend.clock), whatever the docset's flags.
 * Routes: a request whose two documents live in one stride class, the destination staying in it,
 * moves its rows on the device (renamed there; the change and op rows are read back for the host
 * mirror); every other request — classes that differ, a destination that must move to a wider class
 * or is not placed yet, a source not placed yet (nothing to hand) — reads the source's log back,
 * selects and renames on the host and goes through the apply round's placement.  A class that takes
 * a host-route round in a call takes all its rounds of that call that way (a store has one batch in
 * flight and undoes only its last).  A performance caveat: one such request in a class — a destination
 * or a source not placed yet among them — moves every request of that class in the call to the host
 * route; a caller that cares sends those requests in a call of their own (hm_docset_merge_stats shows
 * what happened).  Both routes give the same patches and state.  The destination's
 * DocBackend.clock rows are read once per stride class; the device route reads back the renamed change
 * rows and the op map, and the renamed op rows only where the docset keeps no host copy of its logs
 * (HM_DOCSET_NET_DIFFS, HM_DOCSET_NO_PATCHES).  All-or-nothing as hm_docset_apply is.
 * hm_docset_merge_stats: out2 = requests that took the device route, the host route. */
int hm_docset_merge_from(hm_docset *ds, uint32_t n, const uint32_t *dst_docs, const uint32_t *src_docs, const uint32_t *entry_off,
                         const char *actor_ids, const uint32_t *actor_off, const double *seqs, hm_text **out);
int hm_docset_merge_stats(const hm_docset *ds, uint64_t *out2);
/* the merged document: {uuid: {"type", "keys": [[key, entry]], "elems": [[elemId, entry]]}} */
int hm_docset_view(hm_docset *ds, uint32_t doc, hm_text **out);
/* the merged documents docs[0..n) (a document may repeat) as a JSON array: element i is byte for byte
 * hm_docset_view(docs[i]).  One hm_store_state call per stride class instead of a read per
 * document; the documents render on the docset's host threads.  A document not placed yet renders
 * as Backend.init().  HM_ERR_DEVICE: state rows that are not a merge's (a list element's index at
 * or past its object's elements, two elements at one index, survivors outside a document's slots). */
int hm_docset_views(hm_docset *ds, uint32_t n, const uint32_t *docs, hm_text **out);
/* Backend.getPatch for many documents, from the same call: a JSON array of {"doc": id, "history":
 * history.size, "patch": {"clock", "deps", "canUndo": false, "canRedo": false, "diffs"}}.  clock /
 * deps are the documents' opSet.clock / opSet.deps rows; diffs build the document from an empty one:
 * a create for every object of the view but ROOT, in view order, then per object its `set` diffs in
 * key order and its `insert` diffs (index, elemId) in element order.  No per-op row is read: the
 * call is the same whatever the docset's patch flags are. */
int hm_docset_get_patch(hm_docset *ds, uint32_t n, const uint32_t *docs, hm_text **out);
/* counters: calls, documents, class moves, net patches from the hit registers, net patches from every
 * register, per-op patches, per-op replays whose registers differ from the device's merged state
 * (always 0 unless the renderer and the kernels disagree) */
int hm_docset_stats(const hm_docset *ds, uint64_t *out8);
/* HM_DOCSET_DEVICE_DIFFS: out4 = {document rounds rendered from device rows, hm_store_op_diffs_ex calls,
 * calls repeated with larger tables, 0}; all 0 on a docset without the flag (whose per-op patches and
 * replay checks hm_docset_stats counts; with the flag those two stay 0). */
int hm_docset_diff_stats(const hm_docset *ds, uint64_t *out4);
/* How the docset's stores merged its document rounds so far (hm_store_last_routing summed over
 * every submit): out3 = {incremental, re-merged, incremental handed back to the re-merge}. */
int hm_docset_routing(const hm_docset *ds, uint64_t *out3);
/* The store of class a_stride (8, 16, 32, 64, 128, 256): handles opened in it and handles
 * released (a document moved to a wider class; empty, reused before new ones are opened) */
int hm_docset_handles(const hm_docset *ds, uint32_t a_stride, uint32_t *out_opened, uint32_t *out_free);

/* ------------------------------------------------------------------ */
/* Clock exchange across the node's GPUs (RCCL over xGMI)              */
/* ------------------------------------------------------------------ */
/*
 * Documents shard by FNV-1a64(docId) % G; each GPU (engine) owns its documents' state and the
 * merge never communicates.  What crosses GPUs is the ClockStore feed: per-document clock
 * entries as repo-global records, the analogue of the `clocks` a CursorMessage carries
 * ({docId, clock: {actorId: seq}}, src/PeerMsg.ts:12-16, assembled from ClockStore at
 * src/RepoBackend.ts:374-392 and applied at :397-418).  Actor ranks are per-document and
 * encoder-local, so records name documents and actors by 64-bit keys (FNV-1a64 of the docId /
 * actorId strings; 0 = no actor); the host keeps the key -> string tables.
 *
 *   replaces: src/RepoBackend.ts:374-392 onDiscovery clocks = ClockStore.get per doc
 *             src/RepoBackend.ts:402,412-418 ClockStore.update(sender, doc, clock) + minimumClock
 *             src/Clock.ts:103-113 intersection (the min-clock across replicas)
 *
 * One process per GPU: rank 0 makes a unique id (hm_comm_unique_id), the host distributes it
 * (any channel), every rank calls hm_comm_create.  One thread driving several GPUs: create
 * (and later issue each collective on) every communicator between hm_comm_group_start/_end.
 */
#define HM_COMM_ID_BYTES 128
#define HM_CLOCK_NOT_HELD 0xFFFFFFFFu   /* min-allreduce identity: "this rank does not hold the doc" */

typedef struct {          /* 24 B */
    uint64_t doc_key;     /* FNV-1a64(docId) */
    uint64_t actor_key;   /* FNV-1a64(actorId) */
    uint32_t seq;         /* the clock entry (DocBackend.clock / ClockStore row) */
    uint32_t flags;       /* 0 (reserved) */
} hm_clock_rec;

typedef struct hm_comm hm_comm;
int  hm_comm_unique_id(uint8_t *out /* HM_COMM_ID_BYTES */);
int  hm_comm_create(hm_engine *e, int world, int rank, const uint8_t *unique_id, hm_comm **out);
void hm_comm_destroy(hm_comm *c);
int  hm_comm_group_start(void);
int  hm_comm_group_end(void);

/* Dense per-document clock rows (device: doc_keys[n_docs], actor_keys / clock / base
 * [n_docs*a_stride], base optional) -> records of every entry with actor_key != 0 and
 * clock > base (base NULL: > 0), document-major, rank order within a document.
 * *out_count (device u32) receives the count; `scratch` = hm_clock_records_scratch_bytes. */
size_t hm_clock_records_scratch_bytes(uint32_t n_docs, uint32_t a_stride);
int hm_clock_records_device(hm_engine *e, const uint64_t *doc_keys, const uint64_t *actor_keys,
                            const uint32_t *clock, const uint32_t *base, uint32_t n_docs, uint32_t a_stride,
                            hm_clock_rec *out, uint32_t *out_count, void *scratch, void *stream);

/* d_counts[world] (device u64) <- every rank's record count (all-gather; returns after it). */
int hm_clock_count_allgather(hm_comm *c, uint64_t n_local, uint64_t *d_counts, void *stream);
/* d_out <- every rank's records back to back in rank order; counts (host, [world]) from
 * hm_clock_count_allgather; d_out holds sum(counts) records.  Enqueued on `stream`. */
int hm_clock_allgather(hm_comm *c, const hm_clock_rec *d_recs, const uint64_t *counts, hm_clock_rec *d_out,
                       void *stream);
/* In place, elementwise MIN over every rank of rank-aligned seq rows (row = a (doc, actor) key
 * of the gathered key universe): a rank that holds the document contributes its entry (0 =
 * absent), one that does not HM_CLOCK_NOT_HELD.  After it, 0 and HM_CLOCK_NOT_HELD are absent
 * entries and the rest is Clock.intersection over the replicas holding the document. */
int hm_clock_min_allreduce(hm_comm *c, uint32_t *d_seq, uint64_t n, void *stream);

/* One process driving n GPUs (the Node host's GpuEngine, one engine per device): an n-rank
 * communicator over the engines, and host-buffer forms of the two collectives (staged
 * through each device; every engine's records / seq row is one rank's contribution).
 * hm_clock_exchange_host: out <- all records in rank order (*out_total of them, <= out_cap).
 * hm_clock_min_host: every seq[i] row (len entries) <- the MIN over the n rows. */
int hm_comm_create_local(hm_engine *const *engines, int n, hm_comm **out);
int hm_clock_exchange_host(hm_comm *const *comms, int n, const hm_clock_rec *const *recs, const uint64_t *n_recs,
                           hm_clock_rec *out, uint64_t out_cap, uint64_t *out_total);
int hm_clock_min_host(hm_comm *const *comms, int n, uint32_t *const *seq, uint64_t len);

#ifdef __cplusplus
}
#endif
#endif /* HYPERMERGE_AMD_H */
