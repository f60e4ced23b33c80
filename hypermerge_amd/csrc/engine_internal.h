// engine_internal.h — what store.cpp needs from the engine (not part of the C-ABI)
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hypermerge_amd.h"

// row extents of the tables a launch's document rows index (the store's arenas)
struct hm_extents { uint32_t n_changes, n_deps, n_ops, n_regs; };

// launch the merge kernels on the engine stream; doc_slot maps launch rows to the rows of
// the per-document outputs (NULL = identity); ext = table extents (NULL = the batch's counts);
// epos (optional, indexed like o->regs) receives every list element's document-order position
int hm_engine_launch_merge(hm_engine *e, const hm_batch *b, const hm_results *o, const uint32_t *doc_slot,
                           const hm_extents *ext, uint32_t *epos = nullptr);
hipStream_t hm_engine_stream(hm_engine *e);
int hm_engine_device(hm_engine *e);
int hm_engine_fail(hm_engine *e, int status, const char *msg);

// hm_store_materialize for a caller that allocates by the totals: after the count pass alloc(ctx,
// totals[4]) returns the outputs (NULL: HM_ERR_NOMEM), then fill and merge run; one count pass
typedef const hm_past_out *(*hm_past_alloc)(void *ctx, const uint64_t *totals);
struct hm_store;
int hm_store_materialize_sized(hm_store *s, uint32_t n, const uint32_t *doc_handles, const uint32_t *hist_len,
                               const uint32_t *clock_rows, hm_past_alloc alloc, void *ctx, uint64_t *out_totals);

// the tables a fork batch in flight (hm_store_fork_submit) gathered, read back for a host that
// mirrors the forks' logs: request i's rows are docs[i]'s ranges, op_log[k] = the parent's log op
// index of gathered op k; ops may be NULL (the caller holds the parents' op rows and takes the forks'
// through op_log).  Only between the fork's submit and its wait.  A merge batch in flight
// (hm_store_merge_from_submit) answers the same way: its change and op rows are the renamed ones, the
// destinations' ids; op_log still indexes the source's log.
#include <vector>
// the DocBackend.clock rows of n resident documents (out[i * a_stride ..]) with one synchronise: the
// docset's merge reads its destinations' rows per stride class, not per request
int hm_store_back_clocks(hm_store *s, uint32_t n, const uint32_t *doc_handles, uint32_t *out);
int hm_store_fork_rows(hm_store *s, uint64_t batch_id, std::vector<hm_doc_row> &docs, std::vector<hm_change_row> &changes,
                       std::vector<hm_op_row> *ops, std::vector<uint32_t> &op_log);
