// changes_kernels.h — launch interface of changes_kernels.hip (store.cpp, engine.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hypermerge_amd.h"
#include "doc_source.h"

// bits of *bad
#define HM_MC_BAD_HANDLE 1u     // a request's handle / document index outside the source
#define HM_MC_BAD_RANK 2u       // an entry's actor rank >= S
#define HM_MC_BAD_REPEAT 4u     // a rank listed twice in one request
#define HM_MC_BAD_ENTRIES 8u    // entry_off decreases or runs past n_entries

// getMissingChanges of n requests.  Request i asks its document of src (doc_source.h; it reads
// changes, hist and all_deps) with the have-clock entries entry_off[i] .. entry_off[i + 1] - 1 of
// (entry_actor, entry_seq), in the clock's key order.  Per request the transitiveDeps row goes to
// out_closure (optional, [n * S]), (offset, count) to out_range [2 * n], and — when offset + count
// <= cap — the log indices of the missing changes, in history order, to out_log[offset ..]; the
// offsets come from one atomicAdd per request on *total (zeroed by the caller), so the blocks lie
// in any order and *total ends as the rows needed.  A request that sets a bit of *bad (zeroed by the
// caller) gets the range (0, 0).
struct ChangesArgs {
    uint32_t n;
    DocSource src;
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
