// merge_kernels.h — launch parameters shared by engine.cpp and merge_kernels.hip
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hypermerge_amd.h"

struct SmallParams {
    const hm_doc_row *docs;
    const hm_change_row *changes;
    const hm_dep_row *deps;
    const hm_op_row *ops;
    const uint32_t *min_clock;
    hm_doc_result *res_docs;
    uint32_t *res_clock, *res_back_clock, *res_heads;
    int32_t *res_hist;
    uint32_t *res_all_deps;
    hm_reg_result *res_regs;
    hm_surv_result *res_surv;
    uint32_t n_docs, a_stride;
    uint32_t cap_regs, cap_objs;     // LDS carve of this launch (set by the kernel's size class)
    uint32_t cap_deps;               // dep rows per document the carve holds
    uint32_t counters;               // the carve has the counter sums (HM_DOC_HAS_COUNTERS)
    uint32_t *large_cursor;          // merge_large_kernel's document cursor (zeroed before the launch)
    uint32_t *n_deferred;            // documents merge_small_kernel handed over (zeroed before the launch)
    uint32_t *deferred;              // [n_docs] their launch rows, in hand-over order
    uint32_t general_only;           // HM_CFG_GENERAL_ONLY: defer every document
    uint32_t xcd_remap;              // 1: neighbouring documents go to workgroups on one XCD
    const uint32_t *doc_slot;        // optional: launch row d -> row of the per-document outputs
                                     // (res_docs, clocks, heads, min_clock); NULL = identity
    // extents of the row tables: a document row whose ranges leave them (or whose n_actors
    // exceeds a_stride) is reported HM_ERR_INVALID and never read through
    uint32_t lim_changes, lim_deps, lim_ops, lim_regs;
    // optional (the resident store): per list element register, its position in its list's
    // document order (every inserted element, visible or not) — the order the incremental path
    // keeps resident; rows of other registers are not written
    uint32_t *res_epos;
};
#ifdef __HIPCC__
__device__ __forceinline__ bool hm_doc_row_ok(const SmallParams &p, const hm_doc_row &d) {
    // (no short-circuit: the four limits are one scalar load, not four dependent ones)
    return ((unsigned long long)d.change_off + d.n_changes <= p.lim_changes) &
           ((unsigned long long)d.dep_off + d.n_deps <= p.lim_deps) &
           ((unsigned long long)d.op_off + d.n_ops <= p.lim_ops) &
           ((unsigned long long)d.reg_off + d.n_regs <= p.lim_regs) & (d.n_actors <= p.a_stride);
}
#endif
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t hm_slot(const SmallParams &p, uint32_t d) { return p.doc_slot ? p.doc_slot[d] : d; }
#endif

// internal: the small kernel hands a document to merge_large_kernel (never returned to callers)
#define HM_DEFERRED 0x7FFFFFFF

// bytes of device scratch a launch over `b` uses: [256 B counters][deferred list][large-kernel pool]
size_t hm_launch_scratch_bytes(const hm_batch *b);

size_t hm_large_scratch_bound(const hm_batch *b);
size_t hm_large_stack_bytes();
hipError_t hm_launch_large(const SmallParams &p, void *pool, size_t pool_bytes, unsigned long long *pool_used,
                           uint32_t grid, hipStream_t s);
// Path census of merge_large_kernel (check builds, -DHM_PATH_CENSUS=1): one counter per outcome
// of each run-time layout decision in merge_large.hip.  Every slot counts documents, except the
// two REG slots (registers).  A yes / no pair is (slot, slot + 1).  tests/general_edges.py
// restates the order; keep the two in step.
enum hm_large_path {
    HM_LP_GATE_PASSED = 0,      // the dispatcher tried the all-LDS path (merge_doc_res)
    HM_LP_GATE_REFUSED,         // ... or went straight to the pool path (merge_doc_large)
    // the all-LDS path's exits to the pool path (RES_FALLBACK), one per document at most
    HM_LP_RES_OUT_ROWS,         // malformed change rows
    HM_LP_RES_OUT_TABLE,        // sparse first-arrival table, or table + closure rows over stage_base
    HM_LP_RES_OUT_NOT_READY,    // a change not ready on arrival, or a mismatched duplicate
    HM_LP_RES_OUT_FOLD,         // the literal fold differs from the closure
    HM_LP_RES_OUT_TAIL,         // l34_res: the layout's tail over the limit (or its id widths)
    HM_LP_RES_OUT_COUNTERS,     // counter ops
    HM_LP_RES_OUT_LONG_LIST,    // a register with more than RES_SEG_MAX assigns (and no counters)
    HM_LP_RES_OUT_TOUR,         // the Euler tour does not fit over the dead region (neither of the above)
    HM_LP_RES_OUT_LATE,         // an insert after an element that arrives later
    HM_LP_RES_DONE,             // the all-LDS path merged the document
    // the pool path: (yes, no) pairs
    HM_LP_STAGED, HM_LP_STAGED_NO,
    HM_LP_LTAB, HM_LP_LTAB_NO,
    HM_LP_CLOSURE_LDS, HM_LP_CLOSURE_LDS_NO,
    HM_LP_L3, HM_LP_L3_NO,
    HM_LP_LOP, HM_LP_LOP_NO,
    HM_LP_OBJ_LDS, HM_LP_OBJ_LDS_NO,
    HM_LP_TOUR_LDS, HM_LP_TOUR_LDS_NO,          // (documents with lists only)
    HM_LP_SCRATCH_REUSED, HM_LP_SCRATCH_CARVED,
    HM_LP_HIST_FAST, HM_LP_HIST_PARALLEL, HM_LP_HIST_SERIAL,     // the pool path's history
    HM_LP_REG_SHORT, HM_LP_REG_LONG,            // registers with 1..SEG_SHORT / more assigns
    HM_LP_POOL_DONE,            // the pool path merged the document
    HM_LP_N
};
// (check builds only) out[0 .. n) = the counters since the last reset; returns the slots copied
extern "C" int hm_debug_large_paths(unsigned long long *out, int n, int reset);

// small-kernel size class (LDS carve) for a batch's per-document maxima
uint32_t hm_small_class(uint32_t max_regs, uint32_t max_objs, uint32_t max_deps);
size_t hm_small_lds_bytes(uint32_t opl, uint32_t cls, bool lists, bool counters);
uint32_t hm_small_occupancy(uint32_t opl, uint32_t cls, bool lists, bool counters);
hipError_t hm_launch_small(const SmallParams &p, uint32_t opl, uint32_t cls, bool lists, uint32_t grid, hipStream_t s);
// which: 0 cmp (out uint8_t*), 1 union, 2 intersection (out uint32_t*)
hipError_t hm_launch_clock(int which, const uint32_t *a, const uint32_t *b, void *out, uint32_t n_docs,
                           uint32_t S, hipStream_t s);
