// waiting_kernels.h — launch interface of waiting_kernels.hip (store.cpp, engine.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hypermerge_amd.h"
#include "store_kernels.h"

// handles h < n_handles with res_docs[h].n_queued != 0 into out[0 .. cap) (any order; *count = how
// many there are, also when that exceeds cap); *count zeroed by the caller
hipError_t hm_launch_blocked(const hm_doc_result *res_docs, uint32_t n_handles, uint32_t *out, uint32_t cap,
                             uint32_t *count, hipStream_t s);

// getMissingDeps of resident documents by handle (any output may be NULL): per request the missing
// row and the unmet minimumClock row ([n * S]), the queue length, and — q_off / out_queue given —
// the queue's log indices at out_queue[q_off[i] ..]; *bad |= 1: a handle outside the store,
// |= 2: q_off[i + 1] - q_off[i] is not the document's queue length.  lim_c / lim_d: rows of the
// change / dep arenas (no row past them is read).
struct WaitingArgs {
    uint32_t n;
    const uint32_t *handles;
    const DevDoc *dm;
    uint32_t n_handles, S;
    const hm_change_row *changes;
    const hm_dep_row *deps;
    unsigned long long lim_c, lim_d;
    const int32_t *hist;
    const uint32_t *clock, *back_clock, *min_clock;
    uint32_t *out_missing, *out_unmet, *out_nq;
    const uint32_t *q_off;
    uint32_t *out_queue;
    uint32_t *bad;
};
hipError_t hm_launch_waiting(const WaitingArgs &a, hipStream_t s);

// the same rows for the documents of a merged batch (device tables of b, device results r):
// out_missing [n_docs * a_stride], zero rows for documents whose status is not HM_OK
hipError_t hm_launch_waiting_batch(const hm_batch *b, const hm_results *r, uint32_t *out_missing, hipStream_t s);
