// field_kernels.hip — the fields a proposed local change touches: for each register the request
// names, its current survivors (fieldOps) and, per survivor, whether the request covers it (not
// isConcurrent), read from the resident state; no merge path is touched.
//
//  fields_kernel  one wavefront (a 64-lane workgroup) per request: a document — of a resident store
//                 or of a merged batch: doc_source.h finds its rows —, the would-be change's base
//                 clock as ordered (actor rank, seq) entries, and a list of registers.
//    ready    causallyReady: a ballot over the entries against the document's opSet.clock row
//    locate   } transitiveDeps of the entries: the two steps of changes_kernel (a copy: that kernel's
//    fold     } code and resources stay as they are); the closure row is left in LDS
//    size     the lanes stride the request's registers; each reads its register row, a wave scan
//             turns n_surv into the field's offset in the request's block (kept in out_range)
//    reserve  one atomicAdd on the call's row total
//    write    a lane per output row: its field by binary search over the offsets, the survivor
//             row, the op row, the op's change by binary search over the change rows' op_first
//             (the last change with op_first <= op), covered = closure[actor] >= seq
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/hypermerge_amd.h"
#include "field_kernels.h"
#include "wave.h"

namespace hmf {

#define FWG 64
#define FCOLS (HM_MAX_STRIDE / 64u)    // closure columns a lane holds during the fold

struct Lds {
    uint32_t closure[HM_MAX_STRIDE];   // the transitiveDeps row
    uint32_t slot[HM_MAX_STRIDE];      // per rank: log slot of the applied change its entry names
    uint32_t want[HM_MAX_STRIDE];      // per rank: its entry's seq
    uint32_t listed[HM_MAX_STRIDE];    // per rank: entries that name it
    uint32_t err, rowbad;
};

__global__ __launch_bounds__(FWG) void fields_kernel(FieldArgs A) {
    __shared__ Lds L;
    const uint32_t lane = threadIdx.x;
    const DocSource &D = A.src;
    const uint32_t S = D.S;
    for (unsigned long long q = blockIdx.x; q < A.n; q += gridDim.x) {
        const DocRef m = doc_of(D, q);
        // the request's entries and fields, checked against their tables' lengths
        const uint32_t e0 = A.entry_off[q], e1 = A.entry_off[q + 1], f0 = A.field_off[q], f1 = A.field_off[q + 1];
        const bool f_ok = f1 >= f0 && f1 <= A.n_fields;
        const uint32_t n_e = e1 - e0, n_f = f_ok ? f1 - f0 : 0u;
        const uint32_t b = m.bad ? HM_FD_BAD_HANDLE : e1 < e0 || e1 > A.n_entries ? HM_FD_BAD_ENTRIES : f_ok ? 0u : HM_FD_BAD_FIELDS;
        const uint16_t *ea = A.entry_actor + e0;
        const uint32_t *es = A.entry_seq + e0;
        const uint32_t *fr = A.field_reg + f0;
        uint32_t *rng = A.out_range + 2ull * f0;
        uint32_t *closure_out = A.out_closure ? A.out_closure + q * S : nullptr;

        for (uint32_t a = lane; a < S; a += 64u) { L.closure[a] = 0u; L.slot[a] = HM_NONE; L.want[a] = 0u; L.listed[a] = 0u; }
        if (lane == 0) { L.err = b; L.rowbad = 0u; }
        __syncthreads();
        if (!b)
            for (uint32_t e = lane; e < n_e; e += 64u) {
                const uint32_t r = ea[e];
                if (r >= S) atomicOr(&L.err, HM_FD_BAD_RANK);
                else if (atomicAdd(&L.listed[r], 1u) != 0u) atomicOr(&L.err, HM_FD_BAD_REPEAT);
                else L.want[r] = es[e];
            }
        __syncthreads();
        if (L.err) {                                               // (the same word in every lane)
            if (lane == 0) { atomicOr(A.bad, L.err); A.out_flags[q] = 0u; }
            if (closure_out) for (uint32_t a = lane; a < S; a += 64u) closure_out[a] = 0u;
            for (uint32_t k = lane; k < n_f; k += 64u) { rng[2 * k] = 0u; rng[2 * k + 1] = 0u; }
            __syncthreads();
            continue;
        }
        // a batch document whose merge threw offers nothing: no rows, and a clock of zeros
        const bool dead = !D.dm && D.res[m.index].status != HM_OK;
        const uint32_t *clk = D.clock + (size_t)m.index * S;
        bool late = false;
        for (uint32_t i0 = 0; i0 < n_e; i0 += 64u) {
            const uint32_t e = i0 + lane;
            const bool l = e < n_e && es[e] > (dead ? 0u : clk[ea[e]]);
            late = late || __ballot(l) != 0ull;
        }
        const bool ready = !late;

        const hm_change_row *ch = D.changes + m.c_off;
        if (ready) {
            const int32_t *hist = D.hist + m.c_off;
            const uint32_t *ad = D.all_deps + (size_t)m.c_off * S;
            for (uint32_t i = lane; i < m.n_c; i += 64u) {
                if (hist[i] < 0) continue;
                const hm_change_row c = ch[i];
                if (c.actor < S && c.seq != 0u && L.want[c.actor] == c.seq) L.slot[c.actor] = i;
            }
            __syncthreads();
            // the fold keeps the closure row in registers, lane l the columns l, l + 64, ...
            uint32_t cl[FCOLS] = {};
            for (uint32_t e = 0; e < n_e; e++) {
                const uint32_t r = ea[e], sq = es[e];
                if (sq == 0u) continue;
                const uint32_t sl = L.slot[r];
                if (sl != HM_NONE) {                               // (no such state: the merge is a no-op)
                    const uint32_t *row = ad + (size_t)sl * S;
#pragma unroll
                    for (uint32_t k = 0; k < FCOLS; k++) {
                        const uint32_t a = lane + 64u * k;
                        if (a < S) { const uint32_t v = row[a]; if (v > cl[k]) cl[k] = v; }
                    }
                }
#pragma unroll
                for (uint32_t k = 0; k < FCOLS; k++) if (lane + 64u * k == r) cl[k] = sq;     // set after the merge
            }
#pragma unroll
            for (uint32_t k = 0; k < FCOLS; k++) { const uint32_t a = lane + 64u * k; if (a < S) L.closure[a] = cl[k]; }
            __syncthreads();
        }
        if (closure_out) for (uint32_t a = lane; a < S; a += 64u) closure_out[a] = L.closure[a];

        // size: the request's block, field by field; out_range holds the offsets inside the block
        const uint32_t r_off = D.dm ? D.dm[m.index].r_off : D.docs[m.index].reg_off;
        uint32_t total = 0;
        for (uint32_t k0 = 0; k0 < n_f; k0 += 64u) {
            const uint32_t k = k0 + lane;
            uint32_t c = 0;
            if (k < n_f && ready && !dead) {
                const uint32_t reg = fr[k];
                if (reg < m.n_r && (unsigned long long)r_off + reg < A.lim_r) {
                    const hm_reg_result r = A.regs[(size_t)r_off + reg];
                    if (r.obj != HM_NONE && r.n_surv) {
                        if ((unsigned long long)m.o_off + r.surv_off + r.n_surv <= D.lim_o && r.n_surv <= 0xFFFFFFFFu - total) c = r.n_surv;
                        else atomicOr(&L.rowbad, 1u);
                    }
                }
            }
            const uint32_t incl = wave_incl_scan(c, lane);
            if (k < n_f) { rng[2 * k] = total + incl - c; rng[2 * k + 1] = c; }
            total += __shfl(incl, 63);
        }
        uint32_t off = 0;
        if (lane == 0 && total) off = atomicAdd(A.total, total);
        off = __shfl(off, 0);
        const bool wr = A.out_rows != nullptr && total != 0u && (unsigned long long)off + total <= A.cap;
        __syncthreads();                                           // (the offsets, for every lane)

        if (wr) {
            for (uint32_t j = lane; j < total; j += 64u) {
                uint32_t lo = 0, hi = n_f - 1u;                    // the last field that starts at or before row j
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo + 1u) / 2u;
                    if (rng[2 * mid] <= j) lo = mid; else hi = mid - 1u;
                }
                const uint32_t i = j - rng[2 * lo];
                hm_field_op o = {};
                o.op = HM_NONE; o.actor = 0xFFFFu;
                bool ok = i < rng[2 * lo + 1];
                if (ok) {
                    const hm_reg_result r = A.regs[(size_t)r_off + fr[lo]];
                    const hm_surv_result sv = A.surv[(size_t)m.o_off + r.surv_off + i];
                    o.op = sv.op; o.vtag = (uint8_t)sv.vtag; o.value = sv.value;
                    ok = sv.op < m.n_o && m.n_c != 0u;
                    if (ok) {
                        const hm_op_row p = D.ops[(size_t)m.o_off + sv.op];
                        o.action = p.action; o.datatype = p.datatype;
                        const uint32_t g = m.o_off + sv.op;
                        uint32_t a = 0, z = m.n_c - 1u;            // the last change with op_first <= g
                        while (a < z) {
                            const uint32_t mid = a + (z - a + 1u) / 2u;
                            if (ch[mid].op_first <= g) a = mid; else z = mid - 1u;
                        }
                        const hm_change_row c = ch[a];
                        ok = c.op_first <= g && g - c.op_first < c.n_ops && c.actor < S;
                        if (ok) { o.actor = c.actor; o.seq = c.seq; o.covered = L.closure[c.actor] >= c.seq ? 1u : 0u; }
                    }
                }
                if (!ok) atomicOr(&L.rowbad, 1u);
                A.out_rows[(size_t)off + j] = o;
            }
        }
        __syncthreads();
        for (uint32_t k = lane; k < n_f; k += 64u) rng[2 * k] += off;
        if (lane == 0) A.out_flags[q] = (ready ? 0u : HM_FLD_NOT_READY) | (L.rowbad ? HM_FLD_BAD_ROWS : 0u);
        __syncthreads();
    }
}

}  // namespace hmf

hipError_t hm_launch_fields(const FieldArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    hipLaunchKernelGGL(hmf::fields_kernel, dim3(a.n < 65535u ? a.n : 65535u), dim3(FWG), 0, s, a);
    return hipGetLastError();
}
