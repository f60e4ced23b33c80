// changes_kernels.hip — which of a document's changes a peer lacks (Automerge 0.12 getMissingChanges /
// getChanges / getChangesForActor), read from the resident state; no merge path is touched.
//
//  changes_kernel  one wavefront (a 64-lane workgroup) per request: a document — of a resident store
//                  or of a merged batch: doc_source.h finds its rows — and the peer's clock as
//                  ordered (actor rank, seq) entries.
//    locate   the lanes stride the document's change rows; an applied change (hist >= 0) that an
//             entry names leaves its log slot in a per-rank LDS row
//    fold     transitiveDeps: the entries in order, the lanes stride the S columns of the closure
//             row (in registers, then left in LDS) with max over the located change's allDeps
//             row, then the entry's own column is SET (it can lower what an earlier entry merged
//             in: the result depends on the entries' order when the clock is not causally closed)
//    mark     the rows stride again: an applied change with seq > closure[actor] sets the bit of its
//             history position in an LDS bitmap tile (wave.h HistTile, CTILE positions; longer
//             histories take several tiles, each a pass over the rows)
//    rank     popcount prefix over the tile's words, on a running base across tiles
//    write    one atomicAdd reserves the request's block; a marked row's log index lands at
//             block + base + prefix + bits below its own, i.e. in history order
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/hypermerge_amd.h"
#include "changes_kernels.h"
#include "wave.h"

namespace hmc {

#define CWG 64
#define CTILE 2048u                    // history positions per bitmap tile: one 32-bit word per lane
#define CCOLS (HM_MAX_STRIDE / 64u)    // closure columns a lane holds during the fold

struct Lds {
    uint32_t closure[HM_MAX_STRIDE];   // the threshold row (transitiveDeps, or the entries themselves)
    uint32_t slot[HM_MAX_STRIDE];      // per rank: log slot of the applied change its entry names
    uint32_t want[HM_MAX_STRIDE];      // per rank: its entry's seq
    uint32_t listed[HM_MAX_STRIDE];    // per rank: entries that name it
    HistTile<CTILE> tile;
    uint32_t err;
};

// One request on one single-wave workgroup (the barriers are the wave's own).  ch / hist / ad: the
// document's first change row / history position / allDeps row, n_c of each; ea / es: the request's
// n_e entries; closure_out (or NULL) / range_out: the request's output rows.
__device__ __forceinline__ void changes_core(uint32_t lane, const hm_change_row *__restrict__ ch,
                                             const int32_t *__restrict__ hist, const uint32_t *__restrict__ ad,
                                             uint32_t n_c, uint32_t S, const uint16_t *__restrict__ ea,
                                             const uint32_t *__restrict__ es, uint32_t n_e, uint32_t flags, Lds &L,
                                             uint32_t *closure_out, uint32_t *range_out, uint32_t *out_log, uint32_t cap,
                                             uint32_t *total, uint32_t *bad) {
    const bool raw = (flags & HM_MC_RAW) != 0, only = (flags & HM_MC_ONLY_LISTED) != 0;
    for (uint32_t a = lane; a < S; a += 64u) { L.closure[a] = 0u; L.slot[a] = HM_NONE; L.want[a] = 0u; L.listed[a] = 0u; }
    if (lane == 0) L.err = 0u;
    __syncthreads();
    for (uint32_t e = lane; e < n_e; e += 64u) {
        const uint32_t r = ea[e];
        if (r >= S) atomicOr(&L.err, HM_MC_BAD_RANK);
        else if (atomicAdd(&L.listed[r], 1u) != 0u) atomicOr(&L.err, HM_MC_BAD_REPEAT);
        else if (raw) L.closure[r] = es[e];
        else L.want[r] = es[e];
    }
    __syncthreads();
    if (L.err) {                                               // (the same word in every lane)
        if (lane == 0) { atomicOr(bad, L.err); range_out[0] = 0u; range_out[1] = 0u; }
        if (closure_out) for (uint32_t a = lane; a < S; a += 64u) closure_out[a] = 0u;
        __syncthreads();
        return;
    }
    if (!raw) {
        for (uint32_t i = lane; i < n_c; i += 64u) {
            if (hist[i] < 0) continue;
            const hm_change_row c = ch[i];
            if (c.actor < S && c.seq != 0u && L.want[c.actor] == c.seq) L.slot[c.actor] = i;
        }
        __syncthreads();
        // the fold keeps the closure row in registers, lane l the columns l, l + 64, ...: a step
        // needs no barrier, and the steps' row loads (their addresses are known) can overlap
        uint32_t cl[CCOLS] = {};
        for (uint32_t e = 0; e < n_e; e++) {
            const uint32_t r = ea[e], q = es[e];
            if (q == 0u) continue;
            const uint32_t sl = L.slot[r];
            if (sl != HM_NONE) {                               // (no such state: the merge is a no-op)
                const uint32_t *row = ad + (size_t)sl * S;
#pragma unroll
                for (uint32_t k = 0; k < CCOLS; k++) {
                    const uint32_t a = lane + 64u * k;
                    if (a < S) { const uint32_t v = row[a]; if (v > cl[k]) cl[k] = v; }
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < CCOLS; k++) if (lane + 64u * k == r) cl[k] = q;      // set after the merge
        }
#pragma unroll
        for (uint32_t k = 0; k < CCOLS; k++) { const uint32_t a = lane + 64u * k; if (a < S) L.closure[a] = cl[k]; }
        __syncthreads();
    }
    if (closure_out) for (uint32_t a = lane; a < S; a += 64u) closure_out[a] = L.closure[a];

    const uint32_t n_tiles = (n_c + CTILE - 1u) / CTILE;
    uint32_t count = 0, off = 0, base = 0;
    bool wr = false;
    if (!n_tiles && lane == 0) { range_out[0] = 0u; range_out[1] = 0u; }
    for (uint32_t t = 0; t < n_tiles; t++) {
        L.tile.clear(lane);
        __syncthreads();
        for (uint32_t i0 = 0; i0 < n_c; i0 += 64u) {
            const uint32_t i = i0 + lane;
            bool miss = false;
            uint32_t p = 0;
            if (i < n_c) {
                const int32_t hp = hist[i];
                if (hp >= 0 && (uint32_t)hp < n_c) {
                    p = (uint32_t)hp;
                    const hm_change_row c = ch[i];
                    miss = c.actor < S && c.seq > L.closure[c.actor] && (!only || L.listed[c.actor] != 0u);
                }
            }
            if (t == 0) count += (uint32_t)__popcll(__ballot(miss));
            if (miss && p / CTILE == t) L.tile.mark(p);
        }
        __syncthreads();
        const uint32_t tile_n = L.tile.rank(lane);
        if (t == 0) {
            if (lane == 0) {
                if (count) off = atomicAdd(total, count);
                range_out[0] = off; range_out[1] = count;
            }
            off = __shfl(off, 0);
            wr = out_log != nullptr && count != 0u && (unsigned long long)off + count <= cap;
        }
        __syncthreads();
        if (wr && tile_n) {
            for (uint32_t i = lane; i < n_c; i += 64u) {
                const int32_t hp = hist[i];
                if (hp < 0 || (uint32_t)hp >= n_c || (uint32_t)hp / CTILE != t) continue;
                uint32_t k;
                if (!L.tile.slot((uint32_t)hp, k)) continue;
                if (base + k < count) out_log[off + base + k] = i;
            }
        }
        base += tile_n;
        __syncthreads();
    }
}

__global__ __launch_bounds__(CWG) void changes_kernel(ChangesArgs A) {
    __shared__ Lds L;
    const uint32_t lane = threadIdx.x;
    const DocSource &D = A.src;
    const uint32_t S = D.S;
    for (unsigned long long q = blockIdx.x; q < A.n; q += gridDim.x) {
        const DocRef m = doc_of(D, q);
        // the request's entries, checked against the entry tables' length
        const uint32_t e0 = A.entry_off[q], e1 = A.entry_off[q + 1];
        const uint32_t b = m.bad ? HM_MC_BAD_HANDLE : e1 < e0 || e1 > A.n_entries ? HM_MC_BAD_ENTRIES : 0u;
        if (b) {
            if (lane == 0) { atomicOr(A.bad, b); A.out_range[2 * q] = 0u; A.out_range[2 * q + 1] = 0u; }
            continue;
        }
        changes_core(lane, D.changes + m.c_off, D.hist + m.c_off, D.all_deps + (size_t)m.c_off * S, m.n_c, S, A.entry_actor + e0,
                     A.entry_seq + e0, e1 - e0, A.flags, L, A.out_closure ? A.out_closure + q * S : nullptr, A.out_range + 2 * q,
                     A.out_log, A.cap, A.total, A.bad);
    }
}

}  // namespace hmc

hipError_t hm_launch_missing_changes(const ChangesArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    hipLaunchKernelGGL(hmc::changes_kernel, dim3(a.n < 65535u ? a.n : 65535u), dim3(CWG), 0, s, a);
    return hipGetLastError();
}
