// state_kernels.h — launch interface of state_kernels.hip (store.cpp, engine.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hypermerge_amd.h"
#include "doc_source.h"
#include "past_kernels.h"

// What many documents hold now: request i = handles[i] of the source (a handle may repeat), answered
// with a compaction of the document's live registers (n_surv > 0, obj != HM_NONE, obj < n_objs) in
// ascending register id and their survivors in row order, copied from wherever they sit inside the
// document's survivor slots.
//
//   count  one workgroup per request (grid-stride): cnt[4i ..] = rows, survivors, 0, 0;
//          aux[2i ..] = 0, flags
//   scan   past_scan_kernel (hm_launch_past_scan): off[4i ..] = exclusive prefix sums of cnt in
//          request order, sum = totals, the largest request and the OR of the flags
//   fill   one workgroup per request, nothing written when a total exceeds its cap: the rows, their
//          survivors, out_range[4i ..] = (first row, rows, first survivor, survivors), out_flags[i],
//          and the request's clock / heads rows when asked for
//
// The document comes from src (doc_source.h: its totals and index); its register rows and survivor
// slots from the two tables here:
//   a resident store   registers at DevDoc.r_off, survivors anywhere inside [o_off, o_off + o_cap)
//   a merged batch     registers at docs[d].reg_off, survivors inside the document's n_ops rows
//                      (a document whose status is not HM_OK offers nothing)
// A handle outside the source sets HM_ST_BAD_HANDLE in sum->bad and gets empty ranges.  A register
// segment or slot range that leaves its table (lim_r / lim_s), or a live register whose surv_off +
// n_surv runs outside the document's slots, flags the request HM_ST_BAD_ROWS: it gets no rows and
// nothing is read outside the tables.
#define HM_ST_BAD_HANDLE 1u
#define HM_ST_WG 256u                          // lanes of a workgroup = registers of a chunk
#define HM_ST_MAX_GRID 65535u

struct StateArgs {
    uint32_t n;
    DocSource src;
    const hm_reg_result *regs;                 // [lim_r]
    const hm_surv_result *surv;                // [lim_s]
    unsigned long long lim_r, lim_s;
    const uint32_t *heads;                     // rank rows [index * S ..], or NULL (src.clock: the clock rows)
    uint32_t *cnt, *aux, *off;                 // [4n], [2n], [4n]
    unsigned long long *part;                  // [hm_past_scan_chunks(n) * HM_PAST_PART]
    hm_state_summary *sum;
    // fill pass
    uint32_t cap_rows, cap_surv;
    hm_state_row *out_rows;
    hm_surv_result *out_surv;
    uint32_t *out_range, *out_flags;           // [4n], [n]
    uint32_t *out_clock, *out_heads;           // [n * S] each, or NULL
};
// count + scan (sum need not be zeroed; n == 0: sum is zeroed and nothing else is read or written)
hipError_t hm_launch_state_count(const StateArgs &a, hipStream_t s);
hipError_t hm_launch_state_fill(const StateArgs &a, hipStream_t s);
