// waiting_kernels.hip — what blocked documents wait for (Automerge 0.12 getMissingDeps), read from
// the resident state; no merge path is touched.
//
//  blocked_kernel        grid-stride sweep over every handle's result row: the handles whose
//                        opSet.queue is not empty (n_queued != 0), compacted with a wave ballot and
//                        one atomicAdd per wave that found any.
//  waiting_kernel        one wavefront per requested document (of a resident store or of a merged
//                        batch: doc_source.h finds its rows): the lanes stride the document's
//                        history positions; a queued change (hist == -1) walks its dep rows
//                        and raises, per actor, the largest seq opSet.clock has not reached — the
//                        deps.set(actor, seq - 1) rule of causallyReady — in a per-wave LDS row; the
//                        queue's log indices come out ascending (ballot prefix counts on a running base).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/hypermerge_amd.h"
#include "waiting_kernels.h"

namespace hmw {

#define WWG 256
#define WWAVES (WWG / 64)

__global__ __launch_bounds__(WWG) void blocked_kernel(const hm_doc_result *res_docs, uint32_t n_handles, uint32_t *out,
                                                       uint32_t cap, uint32_t *count) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * WWG;
    // (the loop bound is per wave, so every lane of a wave reaches the ballot)
    for (unsigned long long base = (unsigned long long)blockIdx.x * WWG + (threadIdx.x & ~63u); base < n_handles; base += stride) {
        const unsigned long long h = base + lane;
        const bool q = h < n_handles && res_docs[h].n_queued != 0;
        const unsigned long long m = __ballot(q);
        if (!m) continue;
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(count, (uint32_t)__popcll(m));
        at = __shfl(at, 0);
        if (q) {
            const uint32_t k = at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (k < cap) out[k] = (uint32_t)h;
        }
    }
}

// One document on one wave; every wave of the workgroup calls it the same number of times (the
// barriers), a wave without a document with n_c = 0 and no outputs.  ch / hist: the document's
// first change row / history position; clock, back, minc: its rank-indexed rows (back / minc NULL:
// no unmet row); row: the wave's LDS row.  Returns the queue length.
__device__ __forceinline__ uint32_t waiting_core(uint32_t lane, const hm_change_row *__restrict__ ch,
                                                 const int32_t *__restrict__ hist, uint32_t n_c,
                                                 const hm_dep_row *__restrict__ deps, unsigned long long lim_d,
                                                 const uint32_t *__restrict__ clock, uint32_t S, uint32_t *row, bool rows,
                                                 uint32_t *queue, uint32_t q_cap) {
    for (uint32_t a = lane; a < S; a += 64u) row[a] = 0u;
    __syncthreads();
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < n_c; i0 += 64u) {
        const uint32_t i = i0 + lane;
        const bool q = i < n_c && hist[i] == -1;
        const unsigned long long m = __ballot(q);
        if (q) {
            if (queue) {
                const uint32_t k = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (k < q_cap) queue[k] = i;
            }
            if (rows) {
                const hm_change_row c = ch[i];
                if (c.actor < S) {
                    for (uint32_t j = 0; j < c.n_deps; j++) {
                        const unsigned long long r = (unsigned long long)c.dep_off + j;
                        if (r >= lim_d) break;
                        const hm_dep_row d = deps[r];
                        if (d.actor == c.actor || d.actor >= S) continue;       // (own actor: seq - 1 below)
                        if (clock[d.actor] < d.seq) atomicMax(&row[d.actor], d.seq);
                    }
                    const uint32_t own = c.seq - 1u;
                    if (clock[c.actor] < own) atomicMax(&row[c.actor], own);
                }
            }
        }
        base += (uint32_t)__popcll(m);
    }
    __syncthreads();
    return base;
}

__global__ __launch_bounds__(WWG) void waiting_kernel(WaitingArgs A) {
    __shared__ uint32_t lds[WWAVES][HM_MAX_STRIDE];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const DocSource &D = A.src;
    const uint32_t S = D.S;
    for (unsigned long long q0 = (unsigned long long)blockIdx.x * WWAVES; q0 < A.n; q0 += (unsigned long long)gridDim.x * WWAVES) {
        const unsigned long long q = q0 + wave;
        bool live = q < A.n;
        DocRef m = {};
        if (live) {
            m = doc_of(D, q);
            if (m.bad) { if (lane == 0 && A.bad) atomicOr(A.bad, HM_WAIT_BAD_HANDLE); live = false; }
        }
        uint32_t q_at = 0, q_cap = 0;
        if (live && A.q_off) { q_at = A.q_off[q]; q_cap = A.q_off[q + 1] - q_at; }
        const bool rows = A.out_missing != nullptr;
        const uint32_t nq = waiting_core(lane, D.changes + m.c_off, D.hist + m.c_off, m.n_c, D.deps, D.lim_d,
                                         D.clock + (size_t)m.index * S, S, lds[wave], rows,
                                         live && A.q_off ? A.out_queue + q_at : nullptr, q_cap);
        if (!live) continue;
        if (A.q_off && nq != q_cap && lane == 0) atomicOr(A.bad, HM_WAIT_BAD_QUEUE);
        if (A.out_nq && lane == 0) A.out_nq[q] = nq;
        const bool minc = (m.bits & HM_DDOC_MINC) != 0;
        for (uint32_t a = lane; a < S; a += 64u) {
            if (rows) A.out_missing[q * S + a] = lds[wave][a];
            if (A.out_unmet) {
                uint32_t u = 0;
                if (minc) {
                    const uint32_t want = D.min_clock[(size_t)m.index * S + a];
                    if (D.back_clock[(size_t)m.index * S + a] < want) u = want;
                }
                A.out_unmet[q * S + a] = u;
            }
        }
    }
}

}  // namespace hmw

hipError_t hm_launch_blocked(const hm_doc_result *res_docs, uint32_t n_handles, uint32_t *out, uint32_t cap,
                             uint32_t *count, hipStream_t s) {
    if (!n_handles) return hipSuccess;
    const uint32_t need = (n_handles + WWG - 1) / WWG;
    hipLaunchKernelGGL(hmw::blocked_kernel, dim3(need < 2048u ? need : 2048u), dim3(WWG), 0, s, res_docs, n_handles, out, cap,
                       count);
    return hipGetLastError();
}

hipError_t hm_launch_waiting(const WaitingArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    const uint32_t need = (a.n + WWAVES - 1) / WWAVES;
    hipLaunchKernelGGL(hmw::waiting_kernel, dim3(need < 4096u ? need : 4096u), dim3(WWG), 0, s, a);
    return hipGetLastError();
}
