// past_kernels.h — launch interface of past_kernels.hip (store.cpp, engine.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hypermerge_amd.h"
#include "doc_source.h"

// history positions per bitmap tile of the fill pass (a longer selection takes several tiles, each
// a pass over the document's hist rows); the wave strides the rows 64 at a time
#define HM_PAST_TILE 512u
// the scan's chunks: requests per lane of a 1024-lane workgroup, and the u64 words a chunk leaves in
// `part` (4 sums, 5 maxima, the flags)
#define HM_PAST_SCAN_ITEMS 4u
#define HM_PAST_PART 10u
inline uint32_t hm_past_scan_chunks(uint32_t n) { return (uint32_t)(((unsigned long long)n + 4095ull) / 4096ull); }

// A document as it was: request i = (handles[i], selector), a handle may repeat.  The selector is
// hist_len[i] (the applied changes at history positions below it) or the clock row
// clock_rows[i * S ..] (the applied changes with seq <= clock[actor]); exactly one is not NULL.
// Queued (hist -1) and duplicate (hist -2) changes are never selected.
//
//   count  one wave per request: cnt[4i ..] = changes, deps, ops of the selection and the
//          document's registers; aux[2i ..] = its objects and flags
//   scan   off[4i ..] = exclusive prefix sums of cnt in request order (the requests' output blocks are
//          reserved by this scan over the counts, no atomics: the gathered tables lie in request
//          order, as every encoder here lays a batch out), sum = totals + launch hints; two launches
//          over chunks of 4096 requests, part = hm_past_scan_chunks(n) * HM_PAST_PART words between them
//   fill   one wave per request, nothing written when a total exceeds its cap: the hm_doc_row, the
//          change rows in history order with dep_off / op_first rewritten to the gathered tables,
//          the dep and op rows, out_change_log[j] = document-local log index of gathered change j,
//          out_op_log[k] = document-local log op index of gathered op k
//
// The documents come from src (doc_source.h; it reads changes, hist, deps and ops).  A handle
// outside the source sets HM_PAST_BAD_HANDLE in sum->bad and gets empty ranges; a change row whose
// dep / op range leaves its document's segment sets HM_PAST_BAD_ROWS and is gathered without those
// rows.
//
// order (optional, with clock_rows only): request i's row order[i * S ..] lists actor ranks in
// hand-over order, HM_NONE ends it.  The selection is then laid out actor after actor, each actor's
// changes by ascending seq (loadDocument's / syncReadyActors' order) instead of history order: a
// change's output position is base[actor] + seq - 1, base = the running sum over the row of
// min(clock[actor], opSet.clock[actor]) (src.clock is read; an actor's applied changes are exactly
// its seqs 1 .. opSet.clock[actor], so the positions are dense as history positions are).  The count
// pass checks the row — ranks below n_actors, none twice, every rank with a selected change listed —
// and sets HM_PAST_BAD_ORDER; the caller does not launch the fill then.  NULL: history order, the
// kernels' output as without the table, byte for byte.
#define HM_PAST_BAD_HANDLE 1u
#define HM_PAST_BAD_ROWS 2u
//
// have_rows (optional, with clock_rows only): request i's row have_rows[i * S ..], in the source's rank
// space, is a lower bound: a change is selected when it is applied and have[a] < seq <= clock[a] (what
// syncReadyActors hands a document that was handed each actor's first have[a] changes before).  With an
// order table actor a then contributes max(0, min(clock[a], opSet.clock[a]) - have[a]) changes and a
// change's position is base[a] + seq - have[a] - 1, dense again; history order ranks the selection as
// before.  The count pass's order check sees the narrowed selection.  NULL: as without the table.
// With a history-length selector (clock_rows == NULL) the table is not read: the kernels ignore it,
// and the store's calls refuse it before any launch.
#define HM_PAST_BAD_ORDER 4u
// (8: HM_FORK_BAD_DST, store_kernels.h)
#define HM_PAST_BAD_MAP 16u

struct PastArgs {
    uint32_t n;
    DocSource src;
    const uint32_t *hist_len;                  // [n] or NULL
    const uint32_t *clock_rows;                // [n * S] or NULL
    const uint32_t *order;                     // [n * S] or NULL: actor-major order (clock_rows only)
    const uint32_t *have_rows;                 // [n * S] or NULL: the clock selector's lower bound (clock_rows only)
    uint32_t *cnt, *aux, *off;                 // [4n], [2n], [4n]
    unsigned long long *part;                  // [hm_past_scan_chunks(n) * HM_PAST_PART]
    hm_past_summary *sum;
    // fill pass
    uint32_t cap[4];                           // rows of out_changes (and the logs), out_deps, out_ops; regs
    hm_doc_row *out_docs;
    hm_change_row *out_changes;
    hm_dep_row *out_deps;
    hm_op_row *out_ops;
    uint32_t *out_change_log, *out_op_log;
    uint32_t log_only;                         // 1: only out_docs and out_change_log are written (cap[0] alone counts)
};
// count + scan (sum need not be zeroed; n == 0: sum is zeroed and nothing else is read or written)
hipError_t hm_launch_past_count(const PastArgs &a, hipStream_t s);
hipError_t hm_launch_past_fill(const PastArgs &a, hipStream_t s);
// the scan alone over cnt / aux already written (n, cnt, aux, off, part and sum are read): the op-diff
// kernels reserve their requests' row and survivor blocks with it (op_diff_kernels.hip)
hipError_t hm_launch_past_scan(const PastArgs &a, hipStream_t s);

// The rename pass over a filled batch (cnt / off: the count pass's; one wave per request): the rows of
// request i enter another document's id spaces through the caller's maps.
//   change rows  actor through the rank row, content_id through the content map
//   dep rows     actor through the rank row
//   op rows      obj through the object map; reg (unless HM_NONE: make*) and parent (unless HM_HEAD)
//                through the register map; key (set / del / link / inc only: the others carry none)
//                through the string map; value through the string map (HM_V_STR) or the object map
//                (HM_V_OBJ); everything else, elem included, stays
//   doc row      n_actors / n_regs / n_objs = totals[4i ..], flags |= totals[4i + 3]
// rank is an [n * S] table; the other maps are CSR slices per request (off [n + 1]), the string and the
// content map optional (NULL: identity).  An id at or beyond its slice, an entry of HM_NONE, a source
// rank >= S, or an image at or beyond the stated totals sets HM_PAST_BAD_MAP in *bad (nothing is read
// through such an id; the request's rows are then garbage and the caller drops the batch).
struct RenameArgs {
    uint32_t n, S;
    const uint32_t *cnt, *off;                 // [4n] each
    hm_doc_row *docs;
    hm_change_row *changes;
    hm_dep_row *deps;
    hm_op_row *ops;
    const uint32_t *totals;                    // [4n] n_actors, n_regs, n_objs, flags after the merge
    const uint32_t *rank;                      // [n * S] source rank -> destination rank
    const uint32_t *obj_off, *obj_map, *reg_off, *reg_map;
    const uint32_t *str_off, *str_map, *cid_off, *cid_map;   // (maps may be NULL: identity)
    uint32_t *bad;
};
hipError_t hm_launch_past_rename(const RenameArgs &a, hipStream_t s);
