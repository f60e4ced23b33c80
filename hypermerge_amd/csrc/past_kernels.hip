// past_kernels.hip — a document as it was: the applied changes below a history position, or at or
// below a clock, selected and compacted on the device, in history order, into a cold batch the merge
// kernels take unchanged (RepoBackend's MaterializeMsg: history.slice(0, n) replayed from
// Backend.init(); loadDocument's changes.slice(0, cursor[actor])).  No merge path is touched.
//
//  past_count_kernel  one wavefront per request (four to a workgroup, no LDS): the lanes stride the
//                     document's hist rows coalesced; a selected change adds its dep / op rows
//  past_scan_kernel   exclusive prefix sums of the four count columns in request order, in two launches
//                     of one 1024-lane workgroup per chunk of 4096 requests (a lane four requests, a
//                     shuffle scan per wave, the waves' sums through LDS): the chunks' sums and maxima,
//                     then each chunk's offsets on the sum of the chunks before it; the last chunk
//                     leaves the totals and the launch hints of the gathered batch
//  past_fill_kernel   one wavefront per request, a 64-lane workgroup of its own; per tile of
//                     HM_PAST_TILE history positions:
//    mark     the lanes stride hist; a selected change sets the bit of its history position
//    rank     popcount prefix over the tile's words, on a running base across tiles
//    scatter  the rows stride again: a marked change leaves its log index, its dep / op counts and
//             its first source op row in LDS at its slot (= its rank within the tile)
//    scan     the slots' dep / op counts become offsets (a shuffle scan, 64 slots a step)
//    write    a lane per slot: the change row with dep_off / op_first rewritten, its dep rows, its log
//             index; then the tile's op rows with the whole wave: a lane per OUTPUT op row finds its
//             change by binary search over the slots' op offsets and moves the 32-byte row as two
//             16-byte words, so the stores are contiguous and the loads contiguous within a change
//
// Nothing inside a row is remapped by these passes: register, object and rank ids are the document's
// own.  The request's document comes from doc_source.h; the bitmap tile and the wave scans are wave.h's.
//
//  past_rename_kernel a pass of its own over the gathered tables (a merge into a document that already
//                     holds changes: the rows enter another document's id spaces): one wavefront per
//                     request strides its change, dep and op rows, every id through the caller's maps
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/hypermerge_amd.h"
#include "past_kernels.h"
#include "wave.h"

namespace hmp {

#define PWG 64
#define PTILE HM_PAST_TILE
static_assert(sizeof(hm_op_row) == 32 && sizeof(hm_change_row) == 24 && sizeof(hm_doc_row) == 48, "row sizes");

// the request's source document and its selector
struct Src : DocRef {
    uint32_t npre;                             // prefix selector (clock selector: unused)
    const uint32_t *clk;                       // clock selector's row, or NULL
    const uint32_t *ord;                       // actor-major order row, or NULL (history order)
    const uint32_t *hav;                       // clock selector's lower bound row (source ranks), or NULL
};

__device__ __forceinline__ Src source_of(const PastArgs &A, unsigned long long q) {
    Src s;
    static_cast<DocRef &>(s) = doc_of(A.src, q);
    s.npre = A.hist_len ? A.hist_len[q] : 0u;
    s.clk = A.clock_rows ? A.clock_rows + q * A.src.S : nullptr;
    s.ord = A.order ? A.order + q * A.src.S : nullptr;
    s.hav = A.have_rows && s.clk ? A.have_rows + q * A.src.S : nullptr;
    return s;
}

// is log row i selected?  p = its output position: its history position, or with ab (the request's
// per-rank bases of the actor-major order, in LDS) ab[actor] + seq - 1, or with a lower bound row
// ab[actor] + seq - have[actor] - 1
__device__ __forceinline__ bool selected(const Src &s, const PastArgs &A, uint32_t i, uint32_t &p, const uint32_t *ab = nullptr) {
    const int32_t hp = A.src.hist[s.c_off + i];
    if (hp < 0 || (uint32_t)hp >= s.n_c) return false;
    p = (uint32_t)hp;
    if (!s.clk) return p < s.npre;
    const hm_change_row *c = A.src.changes + s.c_off + i;
    const uint32_t a = c->actor, q = c->seq;
    if (a >= A.src.S || q > s.clk[a]) return false;
    const uint32_t lo = s.hav ? s.hav[a] : 0u;
    if (q <= lo && s.hav) return false;                      // (the destination was handed it already)
    if (!ab) return true;
    if (ab[a] == HM_NONE || !q) return false;                // (an unlisted rank: the count pass refused the row)
    p = ab[a] + q - lo - 1u;
    return p < s.n_c;
}

// The request's actor-major order row, checked by the whole wave: HM_NONE ends it, every rank lies
// below n_actors and appears once.  m[k] = the listed ranks 64 k .. 64 k + 63 as a bitmap.
__device__ __forceinline__ bool order_row(const Src &s, const PastArgs &A, uint32_t lane, unsigned long long m[4]) {
    const uint32_t S = A.src.S;
    uint32_t len = S;
    for (uint32_t j = lane; j < S; j += 64u)
        if (s.ord[j] == HM_NONE) { len = j; break; }
    for (uint32_t d = 32; d; d >>= 1) len = min(len, (uint32_t)__shfl_xor(len, d));
    bool ok = s.clk != nullptr && A.src.clock != nullptr && !s.bad;
    uint32_t mine = 0;
    m[0] = m[1] = m[2] = m[3] = 0ull;
    for (uint32_t j = lane; j < len; j += 64u) {
        const uint32_t r = s.ord[j];
        if (r >= s.n_actors || r >= S || r >= 256u) { ok = false; continue; }
        const unsigned long long b = 1ull << (r & 63u);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (k == (r >> 6)) { ok &= !(m[k] & b); m[k] |= b; }
        mine++;
    }
    mine = wave_sum(mine);
    uint32_t listed = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        for (uint32_t d = 32; d; d >>= 1) m[k] |= (unsigned long long)__shfl_xor((long long)m[k], d);
        listed += (uint32_t)__popcll(m[k]);
    }
    return __ballot(!ok) == 0ull && listed == mine;           // (a rank on two lanes: fewer bits than entries)
}

// the change's dep / op rows, none where the range leaves the document's segment
__device__ __forceinline__ bool rows_of(const Src &s, const hm_change_row &c, uint32_t &nd, uint32_t &no) {
    bool ok = true;
    nd = c.n_deps; no = c.n_ops;
    if (nd && (c.dep_off < s.d_off || (unsigned long long)c.dep_off + nd > (unsigned long long)s.d_off + s.n_d)) { nd = 0; ok = false; }
    if (no && (c.op_first < s.o_off || (unsigned long long)c.op_first + no > (unsigned long long)s.o_off + s.n_o)) { no = 0; ok = false; }
    return ok;
}

#define PCWG 256
__global__ __launch_bounds__(PCWG) void past_count_kernel(PastArgs A) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long step = (unsigned long long)gridDim.x * (PCWG / 64);
    for (unsigned long long q = (unsigned long long)blockIdx.x * (PCWG / 64) + wv; q < A.n; q += step) {
        const Src s = source_of(A, q);
        uint32_t nc = 0, nd = 0, no = 0;
        bool ok = true, listed = true;
        unsigned long long m[4] = {0ull, 0ull, 0ull, 0ull};
        const bool row_ok = s.ord ? order_row(s, A, lane, m) : true;
        for (uint32_t i = lane; i < s.n_c; i += 64u) {
            uint32_t p;
            if (!selected(s, A, i, p)) continue;
            if (s.ord) {                                       // every rank with a selected change is listed
                const uint32_t a = A.src.changes[s.c_off + i].actor, k = a >> 6;
                const unsigned long long w = k == 0 ? m[0] : (k == 1 ? m[1] : (k == 2 ? m[2] : m[3]));
                listed &= ((w >> (a & 63u)) & 1ull) != 0ull;
            }
            uint32_t d, o;
            ok &= rows_of(s, A.src.changes[s.c_off + i], d, o);
            nc++; nd += d; no += o;
        }
        nc = wave_sum(nc); nd = wave_sum(nd); no = wave_sum(no);
        const bool any_bad = __ballot(!ok) != 0ull;
        const bool bad_order = !row_ok || __ballot(!listed) != 0ull;
        if (lane == 0) {
            *(uint4 *)(A.cnt + 4 * q) = make_uint4(nc, nd, no, s.n_r);
            *(uint2 *)(A.aux + 2 * q) = make_uint2(s.n_objs, s.flags);
            const uint32_t b = (s.bad ? HM_PAST_BAD_HANDLE : 0u) | (any_bad ? HM_PAST_BAD_ROWS : 0u) |
                               (bad_order ? HM_PAST_BAD_ORDER : 0u);
            if (b) atomicOr(&A.sum->bad, b);
        }
    }
}

#define PSWG 1024
#define PSITEMS HM_PAST_SCAN_ITEMS
// One chunk of PSWG * PSITEMS requests per workgroup, a lane PSITEMS consecutive requests (64 contiguous
// bytes of counts).  FINAL = false: the chunk's sums and maxima go to part[chunk]; FINAL = true: the
// chunk's base is the sum of the earlier chunks' parts, the offsets are written, and the last chunk
// leaves the totals and the launch hints in the summary.
template <bool FINAL>
__global__ __launch_bounds__(PSWG) void past_scan_kernel(PastArgs A) {
    __shared__ unsigned long long s_w[PSWG / 64][4];
    __shared__ unsigned long long s_carry[4];
    __shared__ uint32_t s_mx[6];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6, j = blockIdx.x;
    const bool last = j == gridDim.x - 1u;
    if (tid < 4) s_carry[tid] = 0ull;
    if (tid < 6) s_mx[tid] = 0u;
    __syncthreads();
    if (FINAL) {
        unsigned long long acc[4] = {0, 0, 0, 0};
        for (uint32_t jj = tid; jj < j; jj += PSWG)
            for (int k = 0; k < 4; k++) acc[k] += A.part[(size_t)jj * HM_PAST_PART + k];
        for (int k = 0; k < 4; k++) if (acc[k]) atomicAdd(&s_carry[k], acc[k]);
    }
    const unsigned long long i0 = (unsigned long long)j * (PSWG * PSITEMS) + (unsigned long long)tid * PSITEMS;
    uint4 v[PSITEMS];
    unsigned long long in[4] = {0, 0, 0, 0};
    uint32_t mx[5] = {0, 0, 0, 0, 0}, fl = 0;
#pragma unroll
    for (uint32_t x = 0; x < PSITEMS; x++) {
        v[x] = make_uint4(0, 0, 0, 0);
        if (i0 + x < A.n) {
            v[x] = *(const uint4 *)(A.cnt + 4 * (i0 + x));
            if (!FINAL) {
                const uint2 o = *(const uint2 *)(A.aux + 2 * (i0 + x));
                mx[0] = max(mx[0], v[x].x); mx[1] = max(mx[1], v[x].z); mx[2] = max(mx[2], v[x].w); mx[3] = max(mx[3], o.x);
                mx[4] = max(mx[4], v[x].y); fl |= o.y;
            }
        }
        in[0] += v[x].x; in[1] += v[x].y; in[2] += v[x].z; in[3] += v[x].w;
    }
    const unsigned long long own[4] = {in[0], in[1], in[2], in[3]};
#pragma unroll
    for (int k = 0; k < 4; k++) in[k] = wave_incl_scan(in[k], lane);
    if (lane == 63u)
        for (int k = 0; k < 4; k++) s_w[wv][k] = in[k];
    __syncthreads();                                           // (s_w, and the chunk's base in s_carry)
    if (tid < 4) {                                             // the waves' sums -> their bases, on the chunk's base
        unsigned long long run = s_carry[tid];
        for (uint32_t w = 0; w < PSWG / 64; w++) { const unsigned long long t = s_w[w][tid]; s_w[w][tid] = run; run += t; }
        s_carry[tid] = run;
    }
    __syncthreads();
    if (!FINAL) {
        if (tid < 4) A.part[(size_t)j * HM_PAST_PART + tid] = s_carry[tid];
        for (int k = 0; k < 5; k++) if (mx[k]) atomicMax(&s_mx[k], mx[k]);
        if (fl) atomicOr(&s_mx[5], fl);
        __syncthreads();
        if (tid < 6) A.part[(size_t)j * HM_PAST_PART + 4 + tid] = s_mx[tid];
        return;
    }
    unsigned long long run[4];
#pragma unroll
    for (int k = 0; k < 4; k++) run[k] = s_w[wv][k] + in[k] - own[k];
#pragma unroll
    for (uint32_t x = 0; x < PSITEMS; x++) {
        if (i0 + x < A.n)
            *(uint4 *)(A.off + 4 * (i0 + x)) = make_uint4((uint32_t)run[0], (uint32_t)run[1], (uint32_t)run[2], (uint32_t)run[3]);
        run[0] += v[x].x; run[1] += v[x].y; run[2] += v[x].z; run[3] += v[x].w;
    }
    if (!last) return;
    for (uint32_t jj = tid; jj < gridDim.x; jj += PSWG) {
        for (int k = 0; k < 5; k++) mx[k] = max(mx[k], (uint32_t)A.part[(size_t)jj * HM_PAST_PART + 4 + k]);
        fl |= (uint32_t)A.part[(size_t)jj * HM_PAST_PART + 9];
    }
    for (int k = 0; k < 5; k++) if (mx[k]) atomicMax(&s_mx[k], mx[k]);
    if (fl) atomicOr(&s_mx[5], fl);
    __syncthreads();
    if (tid == 0) {
        hm_past_summary *o = A.sum;
        for (int k = 0; k < 4; k++) o->totals[k] = s_carry[k];
        o->max_changes = s_mx[0]; o->max_ops = s_mx[1]; o->max_regs = s_mx[2]; o->max_objs = s_mx[3]; o->max_deps = s_mx[4];
        o->doc_flags = s_mx[5];
    }
}

struct Lds {
    HistTile<PTILE> tile;
    uint32_t src[PTILE];                      // per slot: the change's log row (document-local)
    uint32_t dp[PTILE], op[PTILE];             // per slot: dep / op rows, then their offsets within the tile
    uint32_t of[PTILE];                        // per slot: the change's first source op row
    uint32_t ab[HM_MAX_STRIDE];                // actor-major order: per rank the position of its seq 1 (HM_NONE: unlisted)
};

__global__ __launch_bounds__(PWG) void past_fill_kernel(PastArgs A) {
    __shared__ Lds L;
    const uint32_t lane = threadIdx.x;
    const DocSource &D = A.src;
    {
        const hm_past_summary *t = A.sum;                     // (one decision for the whole grid)
        if (t->totals[0] > A.cap[0]) return;
        if (!A.log_only && (t->totals[1] > A.cap[1] || t->totals[2] > A.cap[2] || t->totals[3] > A.cap[3])) return;
    }
    for (unsigned long long q = blockIdx.x; q < A.n; q += gridDim.x) {
        const Src s = source_of(A, q);
        const uint4 cn = *(const uint4 *)(A.cnt + 4 * q), of = *(const uint4 *)(A.off + 4 * q);
        if (lane == 0) {
            hm_doc_row r;
            r.change_off = of.x; r.n_changes = cn.x; r.dep_off = of.y; r.n_deps = cn.y; r.op_off = of.z; r.n_ops = cn.z;
            r.reg_off = of.w; r.n_regs = cn.w; r.n_objs = s.n_objs; r.n_actors = (uint16_t)s.n_actors; r.flags = (uint16_t)s.flags;
            r.reserved[0] = r.reserved[1] = 0;
            A.out_docs[q] = r;
        }
        if (!cn.x) continue;
        const uint32_t *ab = nullptr;
        if (s.ord) {
            // the ranks' bases: the running sum, over the order row, of min(clock row, opSet.clock) —
            // an actor's applied changes are exactly its seqs 1 .. opSet.clock[actor] — less the lower
            // bound row where there is one
            __syncthreads();                                   // (the previous request's reads of L.ab)
            for (uint32_t a = lane; a < HM_MAX_STRIDE; a += 64u) L.ab[a] = HM_NONE;
            __syncthreads();
            const uint32_t *have = D.clock + (unsigned long long)s.index * D.S;
            uint32_t run = 0;
            bool open = true;                                  // (HM_NONE not met yet)
            for (uint32_t j0 = 0; j0 < D.S && open; j0 += 64u) {
                const uint32_t j = j0 + lane;
                const uint32_t r = j < D.S ? s.ord[j] : HM_NONE;
                const unsigned long long ends = __ballot(r == HM_NONE || r >= D.S);
                const bool live = ends == 0ull || lane < (uint32_t)__ffsll((long long)ends) - 1u;
                uint32_t k = live ? min(s.clk[r], have[r]) : 0u;
                if (s.hav && live) k -= min(k, s.hav[r]);
                const uint32_t incl = wave_incl_scan(k, lane);
                if (live) L.ab[r] = run + incl - k;
                run += __shfl(incl, 63);
                open = ends == 0ull;
            }
            __syncthreads();
            ab = L.ab;
        }
        const uint32_t n_tiles = (s.n_c + PTILE - 1u) / PTILE;
        uint32_t base = 0, dbase = 0, obase = 0;               // changes / deps / ops gathered by the earlier tiles
        for (uint32_t t = 0; t < n_tiles && base < cn.x; t++) {
            L.tile.clear(lane);
            __syncthreads();
            for (uint32_t i = lane; i < s.n_c; i += 64u) {     // mark
                uint32_t p;
                if (selected(s, A, i, p, ab) && p / PTILE == t) L.tile.mark(p);
            }
            __syncthreads();
            const uint32_t tile_n = L.tile.rank(lane);         // rank
            __syncthreads();
            if (!tile_n) continue;
            for (uint32_t i = lane; i < s.n_c; i += 64u) {     // scatter
                uint32_t p, k;
                if (ab) {                                      // (another rank's unselected change may name a marked position)
                    if (!selected(s, A, i, p, ab)) continue;
                } else {
                    const int32_t hp = D.hist[s.c_off + i];
                    if (hp < 0 || (uint32_t)hp >= s.n_c) continue;
                    p = (uint32_t)hp;
                }
                if (p / PTILE != t || !L.tile.slot(p, k)) continue;
                const hm_change_row c = D.changes[s.c_off + i];
                uint32_t nd, no;
                rows_of(s, c, nd, no);
                L.src[k] = i; L.dp[k] = nd; L.op[k] = no; L.of[k] = c.op_first;
            }
            __syncthreads();
            uint32_t dsum = 0, osum = 0;                        // scan
            for (uint32_t k0 = 0; k0 < tile_n; k0 += 64u) {
                const uint32_t k = k0 + lane;
                const uint32_t vd = k < tile_n ? L.dp[k] : 0u, vo = k < tile_n ? L.op[k] : 0u;
                const uint32_t id = wave_incl_scan(vd, lane), io = wave_incl_scan(vo, lane);
                if (k < tile_n) { L.dp[k] = dsum + id - vd; L.op[k] = osum + io - vo; }
                dsum += __shfl(id, 63); osum += __shfl(io, 63);
            }
            __syncthreads();
            for (uint32_t k = lane; k < tile_n; k += 64u) {    // write: change rows, dep rows, the change log
                const uint32_t j = base + k;
                if (j >= cn.x) continue;
                const uint32_t i = L.src[k];
                A.out_change_log[of.x + j] = i;
                if (A.log_only) continue;
                hm_change_row c = D.changes[s.c_off + i];
                uint32_t nd, no;
                rows_of(s, c, nd, no);
                const uint32_t d0 = dbase + L.dp[k], src_d = c.dep_off;
                if ((unsigned long long)d0 + nd > cn.y) nd = 0;
                c.n_deps = (uint16_t)nd; c.n_ops = no;
                c.dep_off = of.y + d0; c.op_first = of.z + obase + L.op[k];
                A.out_changes[of.x + j] = c;
                for (uint32_t x = 0; x < nd; x++) A.out_deps[of.y + d0 + x] = D.deps[src_d + x];
            }
            for (uint32_t k = lane; k < (A.log_only ? 0u : osum); k += 64u) {   // write: the tile's op rows, a lane per output row
                uint32_t lo = 0, hi = tile_n;                  // the last slot whose op offset is <= k
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (L.op[mid] <= k) lo = mid; else hi = mid;
                }
                const uint32_t o = obase + k;
                if (o >= cn.z) continue;
                const uint32_t srow = L.of[lo] + (k - L.op[lo]);
                const uint4 *sp = (const uint4 *)(D.ops + srow);
                uint4 *dp = (uint4 *)(A.out_ops + of.z + o);
                const uint4 x0 = sp[0], x1 = sp[1];
                dp[0] = x0; dp[1] = x1;
                A.out_op_log[of.z + o] = srow - s.o_off;
            }
            base += tile_n; dbase += dsum; obase += osum;
            __syncthreads();
        }
    }
}

// id through request q's slice of a CSR map (map == NULL: identity); an id at or beyond the slice, or
// an entry of HM_NONE, is not read through and marks the request bad
__device__ __forceinline__ uint32_t mapped(const uint32_t *off, const uint32_t *map, unsigned long long q, uint32_t id, bool &bad) {
    if (!map) return id;
    const uint32_t lo = off[q], hi = off[q + 1];
    if (hi < lo || id >= hi - lo) { bad = true; return id; }
    const uint32_t v = map[lo + id];
    bad |= v == HM_NONE;
    return v;
}

#define PRWG 256
__global__ __launch_bounds__(PRWG) void past_rename_kernel(RenameArgs R) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long step = (unsigned long long)gridDim.x * (PRWG / 64);
    for (unsigned long long q = (unsigned long long)blockIdx.x * (PRWG / 64) + wv; q < R.n; q += step) {
        const uint4 cn = *(const uint4 *)(R.cnt + 4 * q), of = *(const uint4 *)(R.off + 4 * q);
        const uint4 tot = *(const uint4 *)(R.totals + 4 * q);       // n_actors, n_regs, n_objs, flags
        const uint32_t *rk = R.rank + q * R.S;
        bool bad = false;
        auto ranked = [&](uint32_t a) -> uint32_t {
            if (a >= R.S) { bad = true; return a; }
            const uint32_t v = rk[a];
            bad |= v >= tot.x;                                 // (HM_NONE too)
            return v;
        };
        auto obj_of = [&](uint32_t o) -> uint32_t {
            const uint32_t v = mapped(R.obj_off, R.obj_map, q, o, bad);
            bad |= v >= tot.z;
            return v;
        };
        auto reg_of = [&](uint32_t r) -> uint32_t {
            const uint32_t v = mapped(R.reg_off, R.reg_map, q, r, bad);
            bad |= v >= tot.y;
            return v;
        };
        for (uint32_t i = lane; i < cn.x; i += 64u) {
            hm_change_row *c = R.changes + of.x + i;
            c->actor = (uint16_t)ranked(c->actor);
            c->content_id = mapped(R.cid_off, R.cid_map, q, c->content_id, bad);
        }
        for (uint32_t i = lane; i < cn.y; i += 64u) {
            hm_dep_row *d = R.deps + of.y + i;
            d->actor = (uint16_t)ranked(d->actor);
        }
        for (uint32_t i = lane; i < cn.z; i += 64u) {
            hm_op_row *p = R.ops + of.z + i;
            hm_op_row o = *p;
            o.obj = obj_of(o.obj);
            if (o.reg != HM_NONE) o.reg = reg_of(o.reg);       // (make*: no register)
            if (o.parent != HM_HEAD) o.parent = reg_of(o.parent);
            if (o.action >= HM_SET) o.key = mapped(R.str_off, R.str_map, q, o.key, bad);   // (the keyed actions)
            if (o.vtag == HM_V_STR) o.value = mapped(R.str_off, R.str_map, q, (uint32_t)o.value, bad);
            else if (o.vtag == HM_V_OBJ) o.value = obj_of((uint32_t)o.value);
            *p = o;
        }
        if (lane == 0) {
            hm_doc_row *r = R.docs + q;
            r->n_actors = (uint16_t)tot.x; r->n_regs = tot.y; r->n_objs = tot.z; r->flags |= (uint16_t)tot.w;
        }
        if (__ballot(bad) != 0ull && lane == 0) atomicOr(R.bad, HM_PAST_BAD_MAP);
    }
}

}  // namespace hmp

hipError_t hm_launch_past_rename(const RenameArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    const unsigned long long wgs = ((unsigned long long)a.n + PRWG / 64 - 1) / (PRWG / 64);
    hipLaunchKernelGGL(hmp::past_rename_kernel, dim3((uint32_t)(wgs < 65535ull ? wgs : 65535ull)), dim3(PRWG), 0, s, a);
    return hipGetLastError();
}

hipError_t hm_launch_past_count(const PastArgs &a, hipStream_t s) {
    hipError_t r = hipMemsetAsync(a.sum, 0, sizeof(hm_past_summary), s);
    if (r != hipSuccess || !a.n) return r;                     // (no request: the zero summary is the answer, nothing else is touched)
    {
        const unsigned long long wgs = ((unsigned long long)a.n + PCWG / 64 - 1) / (PCWG / 64);
        hipLaunchKernelGGL(hmp::past_count_kernel, dim3((uint32_t)(wgs < 65535ull ? wgs : 65535ull)), dim3(PCWG), 0, s, a);
        if ((r = hipGetLastError()) != hipSuccess) return r;
    }
    return hm_launch_past_scan(a, s);
}

hipError_t hm_launch_past_scan(const PastArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    const dim3 chunks(hm_past_scan_chunks(a.n));
    hipLaunchKernelGGL(hmp::past_scan_kernel<false>, chunks, dim3(PSWG), 0, s, a);
    const hipError_t r = hipGetLastError();
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(hmp::past_scan_kernel<true>, chunks, dim3(PSWG), 0, s, a);
    return hipGetLastError();
}

hipError_t hm_launch_past_fill(const PastArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    hipLaunchKernelGGL(hmp::past_fill_kernel, dim3(a.n < 65535u ? a.n : 65535u), dim3(PWG), 0, s, a);
    return hipGetLastError();
}
