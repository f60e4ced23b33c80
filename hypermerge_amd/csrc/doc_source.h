// doc_source.h — where the device queries (waiting / changes / past kernels) find a request's
// document: the one place that knows the two forms a source takes and clamps a segment to its table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/hypermerge_amd.h"
#include "store_kernels.h"

// A resident store (dm != NULL: request i names handles[i], checked against n_handles) or a merged
// cold batch (docs / res: request i names document handles[i], handles NULL = document i, checked
// against n_docs; a document whose merge threw offers no rows).  A table a query does not read may
// be NULL.  lim_*: rows of the change (hist, all_deps), dep and op tables; no row past them is read.
struct DocSource {
    const uint32_t *handles;
    const DevDoc *dm;
    uint32_t n_handles;
    const hm_doc_row *docs;
    const hm_doc_result *res;
    uint32_t n_docs;
    uint32_t S;
    const hm_change_row *changes;
    const int32_t *hist;                       // [lim_c]
    const uint32_t *all_deps;                  // [lim_c * S]
    const hm_dep_row *deps;
    const hm_op_row *ops;
    const uint32_t *clock, *back_clock, *min_clock;   // rank rows, [index * S ..]
    unsigned long long lim_c, lim_d, lim_o;
};

// A request's document: its segments (a segment that runs past its table is empty: offset and
// count 0), its totals, and index = the handle or document, which is also its rank rows' index.
// bad: the index lies outside the source (everything else is then zero but n_objs, ROOT's 1).
struct DocRef {
    uint32_t c_off, n_c, d_off, n_d, o_off, n_o, n_r, n_objs, n_actors, flags;
    uint32_t bits;                             // HM_DDOC_* (store form)
    uint32_t index;
    bool bad;
};

__device__ __forceinline__ DocRef doc_of(const DocSource &D, unsigned long long q) {
    DocRef s = {};
    s.n_objs = 1u;                             // (ROOT: an empty document)
    const uint32_t h = D.handles ? D.handles[q] : (uint32_t)q;
    if (D.dm) {
        if (h >= D.n_handles) { s.bad = true; return s; }
        const DevDoc m = D.dm[h];
        s.c_off = m.c_off; s.n_c = m.n_c; s.d_off = m.d_off; s.n_d = m.n_d; s.o_off = m.o_off; s.n_o = m.n_o;
        s.n_r = m.n_r; s.n_objs = m.n_objs; s.n_actors = m.n_actors; s.flags = m.flags; s.bits = m.pad[0];
    } else {
        if (h >= D.n_docs) { s.bad = true; return s; }
        const hm_doc_row r = D.docs[h];
        s.n_r = r.n_regs; s.n_objs = r.n_objs; s.n_actors = r.n_actors; s.flags = r.flags;
        if (D.res[h].status == HM_OK) {        // (a document whose merge threw has no history)
            s.c_off = r.change_off; s.n_c = r.n_changes; s.d_off = r.dep_off; s.n_d = r.n_deps;
            s.o_off = r.op_off; s.n_o = r.n_ops;
        }
    }
    s.index = h;
    if ((unsigned long long)s.c_off + s.n_c > D.lim_c) { s.c_off = 0; s.n_c = 0; }
    if ((unsigned long long)s.d_off + s.n_d > D.lim_d) { s.d_off = 0; s.n_d = 0; }
    if ((unsigned long long)s.o_off + s.n_o > D.lim_o) { s.o_off = 0; s.n_o = 0; }
    return s;
}
