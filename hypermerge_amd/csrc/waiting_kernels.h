// waiting_kernels.h — launch interface of waiting_kernels.hip (store.cpp, engine.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hypermerge_amd.h"
#include "doc_source.h"

// handles h < n_handles with res_docs[h].n_queued != 0 into out[0 .. cap) (any order; *count = how
// many there are, also when that exceeds cap); *count zeroed by the caller
hipError_t hm_launch_blocked(const hm_doc_result *res_docs, uint32_t n_handles, uint32_t *out, uint32_t cap,
                             uint32_t *count, hipStream_t s);

// bits of *bad
#define HM_WAIT_BAD_HANDLE 1u   // a request's handle / document index outside the source
#define HM_WAIT_BAD_QUEUE 2u    // q_off[i + 1] - q_off[i] is not the document's queue length

// getMissingDeps of n requests against src (doc_source.h; it reads changes, hist, deps and clock, and
// back_clock / min_clock for out_unmet).  Any output may be NULL: per request the missing row and
// the unmet minimumClock row ([n * S]), the queue length, and — q_off / out_queue given — the
// queue's log indices at out_queue[q_off[i] ..].  A document whose merge threw gets a zero row.
// *bad (zeroed by the caller) collects the bits above; it may be NULL where no index can lie
// outside the source (src.handles NULL and n == src.n_docs).
struct WaitingArgs {
    uint32_t n;
    DocSource src;
    uint32_t *out_missing, *out_unmet, *out_nq;
    const uint32_t *q_off;
    uint32_t *out_queue;
    uint32_t *bad;
};
hipError_t hm_launch_waiting(const WaitingArgs &a, hipStream_t s);
