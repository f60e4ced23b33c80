// op_diff_kernels.h — launch interface of op_diff_kernels.hip (store.cpp, engine.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hypermerge_amd.h"
#include "doc_source.h"
#include "past_kernels.h"

// history positions per bitmap tile of the walk (a longer history takes several tiles, each a pass
// over the document's hist rows); a tile's ops are taken 64 at a time in application order
#define HM_OD_TILE 512u

// What each applied op of a history slice did to its document: request i = (handles[i], from[i],
// to[i]) covers the applied changes at history positions from <= p < to, a handle may repeat.  In
// application order (history position of the change, op index in the change) a make op emits a
// `create` row, an assign on a map / table register the register as it stands after that op (the
// survivors, winner first), `ins` nothing.  A range that holds an assign on a list / text object is
// flagged HM_OD_LISTS and gets no rows.  Queued (hist -1) and duplicate (hist -2) changes contribute
// nothing.
//
//   count  one wave per request: cnt[4i ..] = diff rows, survivor rows, 0, 0; aux[2i ..] = 0, flags
//   scan   past_scan_kernel (hm_launch_past_scan): off[4i ..] = exclusive prefix sums of cnt in request
//          order, sum = totals (rows, survivors), the maxima and the OR of the flags
//   fill   one wave per request, nothing written when a total exceeds its cap: the rows, their
//          survivors, out_range[2i ..] = (first row, rows), out_flags[i]
//
// Count and fill are one walk: the wave takes the document's applied ops in application order, tile
// by tile, 64 ops a step, and threads every map register's assigns into a chain (previous / next
// assign on the register, the op's change) in its slice of `work`; an op of the range then walks
// its register's chain backwards, and from each set / link forwards again to itself, to know
// whether a later assign covers it and which incs it collects.  A wave's slice holds
// hm_od_slice_words(ops, registers, objects) words of the largest document it meets; a document
// that needs more sets HM_OD_BAD_WORK and gets empty ranges.
//
// opts & HM_ODF_LISTS: a document whose HM_DOC_HAS_LISTS hint is set has its element assigns answered
// (HM_OD_ELEM_* rows, their index in out_index) instead of flagged; its slice is
// hm_od_slice_words_lists.  The walk is a second pair of instantiations: with opts = 0 the kernels
// are the ones they were.
//
// OpDiffArgs.clock: the clock forms, a third and fourth pair of instantiations.  Request i = (handles[i],
// clock[i * S ..]) covers the changes applied at that clock (hist >= 0, seq <= K[actor], all_deps row
// <= K), from the empty document: a select phase per request leaves a bit per log change behind the
// slice's other words (hm_od_slice_words_clock) and the walk reads it where it otherwise tests the
// history position.  Count, scan, fill, outputs and flags are the same; there is no one-walk form.
#define HM_OD_BAD_HANDLE 1u
#define HM_OD_BAD_ROWS 2u
#define HM_OD_BAD_WORK 4u

__host__ __device__ inline unsigned long long hm_od_slice_words(unsigned long long n_ops, unsigned long long n_regs, unsigned long long n_objs) {
    return 3ull * n_ops + n_regs + n_objs;
}

// The slice of a document that carries HM_DOC_HAS_LISTS, in a call that answers element assigns
// (HM_ODF_LISTS); term by term:
//   3 ops + regs + objs   the chains, last[] and the object types, as above
//   regs                  pos[]: an element register's place in the document's RGA order
//   regs                  vis[]: is the element visible (does its register hold survivors) so far
//   regs + 1              the Fenwick tree over pos (1-based): +1 per visible element; during the
//                         order phase the same words map a register to its node
//   regs                  a node's first child (order phase)
//   objs                  per list / text object: the pos of its first element
//   4 regs                the nodes being sorted: parent identity, ~elem, ~actor rank, register
//   8 regs                the Euler tour's successor and weight per edge (2 per node), ping and pong
// (a document has at most one applied ins per element register, so nodes <= regs)
__host__ __device__ inline unsigned long long hm_od_slice_words_lists(unsigned long long n_ops, unsigned long long n_regs, unsigned long long n_objs) {
    return 3ull * n_ops + 17ull * n_regs + 2ull * n_objs + 1ull;
}

// The clock forms (OpDiffArgs.clock) add the select phase's bitmap to a document's slice, after its other
// words: a bit per log change of the document, set when the change is applied at the request's clock
__host__ __device__ inline unsigned long long hm_od_slice_words_clock(unsigned long long n_changes) {
    return (n_changes + 31ull) / 32ull;
}

// workgroups (one wave each) of a call whose largest document needs slice_words: as many as the
// requests, the waves a 256-CU device keeps resident (8,704 B of LDS each: 16 to a CU) and a
// 256 MiB work budget allow, at least one
inline uint32_t hm_od_waves(uint32_t n, unsigned long long slice_words) {
    const unsigned long long budget = (256ull << 20) / 4ull, by_mem = budget / (slice_words ? slice_words : 1ull);
    unsigned long long w = n < 4096u ? n : 4096u;
    if (by_mem < w) w = by_mem;
    return (uint32_t)(w ? w : 1ull);
}

struct OpDiffArgs {
    uint32_t n;
    DocSource src;
    const uint32_t *from, *to;                 // [n] (not read when clock is given)
    uint32_t *cnt, *aux, *off;                 // [4n], [2n], [4n]
    unsigned long long *part;                  // [hm_past_scan_chunks(n) * HM_PAST_PART]
    hm_op_diff_summary *sum;
    uint32_t *work;                            // [waves * slice_words]
    unsigned long long slice_words;
    uint32_t waves;                            // workgroups of the count and fill launches
    // fill pass
    uint32_t cap_rows, cap_surv;
    hm_op_diff *out_rows;
    hm_surv_result *out_surv;
    uint32_t *out_range, *out_flags;           // [2n], [n]
    // HM_ODF_* of the call; with HM_ODF_LISTS the fill writes out_index [cap_rows] beside out_rows
    uint32_t opts;
    uint32_t *out_index;
    // != NULL: the clock forms.  Request i takes the changes applied at clock[i * S ..] (per rank the
    // largest seq selected): hist >= 0, seq <= K[actor] and all_deps row <= K; every row is in range,
    // the patch from the empty document.  The slice grows by hm_od_slice_words_clock(changes).
    const uint32_t *clock;                     // [n * S]
};
// the largest slice a request of the call needs, left in out_words[0]; out_words[1] = 1 when opts has
// HM_ODF_LISTS and a requested document carries HM_DOC_HAS_LISTS (device, two words zeroed by the
// caller).  A caller that finds it 0 may clear HM_ODF_LISTS in opts: no document would be answered
// differently, the walk is then the instantiation without lists, and the fill launch sets out_index
// (when given) to HM_NONE throughout, whatever the totals: only for a caller that launches the fill
// once the totals fit, as the store does.
hipError_t hm_launch_op_diff_need(const OpDiffArgs &a, unsigned long long *out_words, hipStream_t s);
// count + scan (sum need not be zeroed; n == 0: sum is zeroed and nothing else is read or written)
hipError_t hm_launch_op_diff_count(const OpDiffArgs &a, hipStream_t s);
hipError_t hm_launch_op_diff_fill(const OpDiffArgs &a, hipStream_t s);
// HM_ODF_ONCE: one launch instead of count + scan + fill.  A request reserves its row block (the ops
// of its slice: an upper bound of its rows) and, per 64-op step, the step's survivor block, each with
// one atomicAdd on sum->totals; a block that does not fit under cap_rows / cap_surv is not written and
// the walk goes on, so sum->totals = (the row bounds, the survivors) of the whole call whatever the
// caps.  out_range[2i ..] = (block, rows emitted): the blocks lie in the order the waves finished, a
// block's unused tail is a gap; a flagged request gets (block, 0).  surv_off is absolute.  sum: totals,
// flags and bad are written, the maxima stay 0; cnt / off / aux / part are not used.  out_index as in
// the fill launch (HM_NONE throughout when opts has no HM_ODF_LISTS).
hipError_t hm_launch_op_diff_once(const OpDiffArgs &a, hipStream_t s);
