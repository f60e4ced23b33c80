// field_kernels.h — launch interface of field_kernels.hip (store.cpp, engine.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hypermerge_amd.h"
#include "doc_source.h"

// bits of *bad
#define HM_FD_BAD_HANDLE 1u     // a request's handle / document index outside the source
#define HM_FD_BAD_RANK 2u       // an entry's actor rank >= S
#define HM_FD_BAD_REPEAT 4u     // a rank listed twice in one request
#define HM_FD_BAD_ENTRIES 8u    // entry_off decreases or runs past n_entries
#define HM_FD_BAD_FIELDS 16u    // field_off decreases or runs past n_fields

// The fields of n proposed changes.  Request i asks its document of src (doc_source.h; it reads
// changes, hist, all_deps, ops and the clock rows) with the ordered entries entry_off[i] ..
// entry_off[i + 1] - 1 and the registers field_reg[field_off[i] .. field_off[i + 1] - 1].  regs /
// surv are the source's register and survivor tables (lim_r rows of regs; surv is as long as the
// op table, src.lim_o).  Per request: out_flags (HM_FLD_*), the transitiveDeps row to out_closure
// (optional, [n * S]; zero when the request is not ready); per field (first row, rows) to
// out_range [2 * n_fields]; and — when the request's block fits under cap — one row per survivor
// to out_rows, fields in request order, winner first.  The blocks come from one atomicAdd per
// request on *total (zeroed by the caller): they lie in any order and *total ends as the rows
// needed.  A request that sets a bit of *bad (zeroed by the caller) gets empty ranges.
struct FieldArgs {
    uint32_t n;
    DocSource src;
    const hm_reg_result *regs;
    const hm_surv_result *surv;
    unsigned long long lim_r;
    const uint32_t *entry_off;
    const uint16_t *entry_actor;
    const uint32_t *entry_seq;
    uint32_t n_entries;
    const uint32_t *field_off;
    const uint32_t *field_reg;
    uint32_t n_fields;
    uint32_t *out_flags, *out_closure, *out_range;
    hm_field_op *out_rows;
    uint32_t cap;
    uint32_t *total, *bad;
};
hipError_t hm_launch_fields(const FieldArgs &a, hipStream_t s);
