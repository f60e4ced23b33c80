// changes_kernels.h — launch interface of changes_kernels.hip (store.cpp, engine.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hypermerge_amd.h"
#include "store_kernels.h"

// bits of *bad
#define HM_MC_BAD_HANDLE 1u     // a handle outside the store
#define HM_MC_BAD_RANK 2u       // an entry's actor rank >= S
#define HM_MC_BAD_REPEAT 4u     // a rank listed twice in one request
#define HM_MC_BAD_ENTRIES 8u    // entry_off decreases or runs past n_entries

// getMissingChanges of n requests.  Request i asks document handles[i] (handles NULL: document i of
// the batch tables docs / res) with the have-clock entries entry_off[i] .. entry_off[i + 1] - 1 of
// (entry_actor, entry_seq), in the clock's key order.  Per request the transitiveDeps row goes to
// out_closure (optional, [n * S]), (offset, count) to out_range [2 * n], and — when offset + count
// <= cap — the log indices of the missing changes, in history order, to out_log[offset ..]; the
// offsets come from one atomicAdd per request on *total (zeroed by the caller), so the blocks lie
// in any order and *total ends as the rows needed.  A request that sets a bit of *bad (zeroed by the
// caller) gets the range (0, 0).  lim_c: rows of the change arena (hist and all_deps have as many,
// all_deps * S words); no row past it is read.
struct ChangesArgs {
    uint32_t n;
    const uint32_t *handles;                   // resident store ...
    const DevDoc *dm;
    uint32_t n_handles;
    const hm_doc_row *docs;                    // ... or a merged cold batch
    const hm_doc_result *res;
    uint32_t n_docs;
    uint32_t S;
    const hm_change_row *changes;
    const int32_t *hist;
    const uint32_t *all_deps;
    unsigned long long lim_c;
    const uint32_t *entry_off;
    const uint16_t *entry_actor;
    const uint32_t *entry_seq;
    uint32_t n_entries;
    uint32_t flags;                            // HM_MC_*
    uint32_t *out_closure, *out_range, *out_log;
    uint32_t cap;
    uint32_t *total, *bad;
};
hipError_t hm_launch_missing_changes(const ChangesArgs &a, hipStream_t s);
