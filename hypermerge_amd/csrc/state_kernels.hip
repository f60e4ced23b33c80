// state_kernels.hip — what many documents hold now (DocSet.views / Backend.getPatch): a stream
// compaction of each requested document's live registers and of their survivors, read off the
// tables the merge and the incremental path keep resident.  Nothing is replayed or re-merged, and
// no object type is needed: a row carries the register's list index as the merge left it, placing
// the elements is the consumer's part.
//
//  state_count_kernel   a workgroup of HM_ST_WG lanes per request (grid-stride): the register rows
//                       are read 16 bytes a lane, lane = register, HM_ST_WG registers a chunk; per
//                       lane the live rows and their survivors are summed over the chunks, then
//                       over the wave (shuffles) and the workgroup's waves (LDS)
//  past_scan_kernel     (hm_launch_past_scan) the requests' row and survivor blocks, the totals, the
//                       largest request, the OR of the flags
//  state_fill_kernel    the same walk: a live register's rank within its chunk is the popcount of
//                       the wave's ballot below its lane plus the earlier waves' counts (LDS), its
//                       survivor offset a wave scan plus the earlier waves' sums; the running row
//                       and survivor totals are carried across chunks in registers.  The lane then
//                       writes its row and copies its survivors, 16 bytes each.
//
// Every read is bounded before it is made: the register segment against lim_r, the slot range
// against lim_s, a live register's survivor list against the document's slots (state_kernels.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/hypermerge_amd.h"
#include "state_kernels.h"
#include "wave.h"

namespace hms {

#define SWG HM_ST_WG
#define SWAVES (SWG / 64u)
static_assert(sizeof(hm_reg_result) == 16 && sizeof(hm_surv_result) == 16 && sizeof(hm_state_row) == 20, "row sizes");
static_assert(sizeof(hm_state_summary) == sizeof(hm_past_summary), "the scan writes the summary as hm_past_summary");
static_assert(offsetof(hm_state_summary, max_rows) == offsetof(hm_past_summary, max_changes) &&
              offsetof(hm_state_summary, max_surv) == offsetof(hm_past_summary, max_deps) &&
              offsetof(hm_state_summary, flags) == offsetof(hm_past_summary, doc_flags) &&
              offsetof(hm_state_summary, bad) == offsetof(hm_past_summary, bad), "summary layout");
static_assert(offsetof(hm_reg_result, n_surv) == 0 && offsetof(hm_reg_result, surv_off) == 4 &&
              offsetof(hm_reg_result, list_index) == 8 && offsetof(hm_reg_result, obj) == 12, "a register row as a uint4");

// a request's register rows and survivor slots (n_r = 0: nothing to read)
struct Seg {
    unsigned long long r0, s0;                 // first register row, first survivor slot
    uint32_t n_r, slots, n_objs, index;
    bool bad_handle, bad_rows;
};

__device__ __forceinline__ Seg seg_of(const StateArgs &A, unsigned long long q) {
    const DocSource &D = A.src;
    const DocRef s = doc_of(D, q);
    Seg g = {};
    g.index = s.index; g.bad_handle = s.bad; g.n_objs = s.n_objs;
    if (s.bad) return g;
    if (D.dm) {
        const DevDoc m = D.dm[s.index];
        g.r0 = m.r_off; g.s0 = m.o_off; g.n_r = m.n_r; g.slots = m.o_cap;
    } else {
        if (D.res[s.index].status != HM_OK) return g;          // (a document whose merge threw offers nothing)
        const hm_doc_row r = D.docs[s.index];
        g.r0 = r.reg_off; g.s0 = r.op_off; g.n_r = r.n_regs; g.slots = r.n_ops;
    }
    if (g.n_r && (g.r0 + g.n_r > A.lim_r || g.s0 + g.slots > A.lim_s)) { g.bad_rows = true; g.n_r = 0; }
    return g;
}

// a register row (n_surv, surv_off, list_index, obj): does it belong to the document's state?
__device__ __forceinline__ bool live_reg(const uint4 &w, uint32_t n_objs) { return w.x != 0u && w.w != HM_NONE && w.w < n_objs; }

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(SWG) void state_count_kernel(StateArgs A) {
    __shared__ unsigned long long s_surv[SWAVES];
    __shared__ uint32_t s_rows[SWAVES], s_bad[SWAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (unsigned long long q = blockIdx.x; q < A.n; q += gridDim.x) {
        const Seg g = seg_of(A, q);
        uint32_t rows = 0;
        unsigned long long surv = 0;
        bool bad = false;
        for (uint32_t c0 = 0; c0 < g.n_r; c0 += SWG) {
            const uint32_t r = c0 + tid;
            if (r >= g.n_r) continue;
            const uint4 w = *(const uint4 *)(A.regs + g.r0 + r);
            if (!live_reg(w, g.n_objs)) continue;
            if ((unsigned long long)w.y + w.x > g.slots) bad = true;
            else { rows++; surv += w.x; }
        }
        rows = wave_sum(rows); surv = wave_sum64(surv);
        const bool wbad = __ballot(bad) != 0ull;
        if (lane == 0) { s_rows[wv] = rows; s_surv[wv] = surv; s_bad[wv] = wbad ? 1u : 0u; }
        __syncthreads();
        if (tid == 0) {
            uint32_t tr = 0, tb = g.bad_rows ? 1u : 0u;
            unsigned long long ts = 0;
            for (uint32_t k = 0; k < SWAVES; k++) { tr += s_rows[k]; ts += s_surv[k]; tb |= s_bad[k]; }
            if (ts > g.slots) tb = 1u;                         // (more survivors than the document has slots: lists that overlap)
            *(uint4 *)(A.cnt + 4 * q) = tb ? make_uint4(0, 0, 0, 0) : make_uint4(tr, (uint32_t)ts, 0, 0);
            *(uint2 *)(A.aux + 2 * q) = make_uint2(0u, tb ? HM_ST_BAD_ROWS : 0u);
            if (g.bad_handle) atomicOr(&A.sum->bad, HM_ST_BAD_HANDLE);
        }
        __syncthreads();                                       // (the waves' words are read before the next request writes them)
    }
}

__global__ __launch_bounds__(SWG) void state_fill_kernel(StateArgs A) {
    __shared__ uint32_t s_w[2][2][SWAVES];                     // [chunk parity][rows | survivors][wave]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    {
        const hm_state_summary *t = A.sum;                    // (one decision for the whole grid)
        if (t->totals[0] > A.cap_rows || t->totals[1] > A.cap_surv) return;
    }
    const uint32_t S = A.src.S;
    uint32_t par = 0;
    for (unsigned long long q = blockIdx.x; q < A.n; q += gridDim.x) {
        const uint4 cn = *(const uint4 *)(A.cnt + 4 * q), of = *(const uint4 *)(A.off + 4 * q);
        const Seg g = seg_of(A, q);
        if (tid == 0) {
            *(uint4 *)(A.out_range + 4 * q) = make_uint4(of.x, cn.x, of.y, cn.y);
            A.out_flags[q] = A.aux[2 * q + 1];
        }
        if (A.out_clock)
            for (uint32_t k = tid; k < S; k += SWG) A.out_clock[q * S + k] = g.bad_handle ? 0u : A.src.clock[(size_t)g.index * S + k];
        if (A.out_heads)
            for (uint32_t k = tid; k < S; k += SWG) A.out_heads[q * S + k] = g.bad_handle ? 0u : A.heads[(size_t)g.index * S + k];
        if (!cn.x) continue;                                   // (nothing live, or flagged: uniform)
        uint32_t run_r = 0, run_s = 0;                         // rows and survivors of the earlier chunks
        for (uint32_t c0 = 0; c0 < g.n_r; c0 += SWG, par ^= 1u) {
            const uint32_t r = c0 + tid;
            uint4 w = make_uint4(0, 0, 0, 0);
            bool live = false;
            if (r < g.n_r) {
                w = *(const uint4 *)(A.regs + g.r0 + r);
                live = live_reg(w, g.n_objs) && (unsigned long long)w.y + w.x <= g.slots;
            }
            const unsigned long long m = __ballot(live);
            const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            const uint32_t ns = live ? w.x : 0u;
            const uint32_t is = wave_incl_scan(ns, lane);
            if (lane == 63u) { s_w[par][0][wv] = (uint32_t)__popcll(m); s_w[par][1][wv] = is; }
            __syncthreads();
            uint32_t pr = run_r, ps = run_s;
#pragma unroll
            for (uint32_t k = 0; k < SWAVES; k++) {
                const uint32_t a = s_w[par][0][k], b = s_w[par][1][k];
                if (k < wv) { pr += a; ps += b; }
                run_r += a; run_s += b;
            }
            if (!live) continue;
            const uint32_t row = pr + rank, so = ps + is - ns;
            if (row >= cn.x || (unsigned long long)so + ns > cn.y) continue;   // (the tables changed since the count: stay inside the block)
            hm_state_row o;
            o.reg = r; o.obj = w.w; o.index = (int32_t)w.z; o.n_surv = ns; o.surv_off = of.y + so;
            A.out_rows[(size_t)of.x + row] = o;
            const uint4 *src = (const uint4 *)(A.surv + g.s0 + w.y);
            uint4 *dst = (uint4 *)(A.out_surv + (size_t)of.y + so);
            for (uint32_t i = 0; i < ns; i++) dst[i] = src[i];
        }
    }
}

}  // namespace hms

static uint32_t state_grid(uint32_t n) { return n < HM_ST_MAX_GRID ? n : HM_ST_MAX_GRID; }

hipError_t hm_launch_state_count(const StateArgs &a, hipStream_t s) {
    hipError_t r = hipMemsetAsync(a.sum, 0, sizeof(hm_state_summary), s);
    if (r != hipSuccess || !a.n) return r;                     // (no request: the zero summary is the answer)
    hipLaunchKernelGGL(hms::state_count_kernel, dim3(state_grid(a.n)), dim3(SWG), 0, s, a);
    if ((r = hipGetLastError()) != hipSuccess) return r;
    PastArgs P = {};
    P.n = a.n; P.cnt = a.cnt; P.aux = a.aux; P.off = a.off; P.part = a.part; P.sum = (hm_past_summary *)a.sum;
    return hm_launch_past_scan(P, s);
}

hipError_t hm_launch_state_fill(const StateArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    hipLaunchKernelGGL(hms::state_fill_kernel, dim3(state_grid(a.n)), dim3(SWG), 0, s, a);
    return hipGetLastError();
}
