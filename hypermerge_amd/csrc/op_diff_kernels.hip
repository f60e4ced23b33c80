// op_diff_kernels.hip — what each applied op of a history slice did to its document (Automerge
// makePatch's per-op diffs; RepoBackend's MaterializeMsg reply and every applyChanges return them
// with the merge): per make op a `create` row, per assign on a map / table register the register
// as it stands after that op.  Everything is read from tables the merge left resident (hist,
// all_deps, the change and op rows); no state is replayed.
//
// The rule (oracle/js/backend.js applyAssign; docset.cpp Replay::assign is the same in C++).  The
// application key of an op is (history position of its change, op index in the change).  For an
// assign k on register r, A(k) = the applied assigns on r with key <= key(k), over the whole history:
//   survivors  x in A(k), set or link, such that no set / del / link y in A(k) after x has
//              all_deps[change(y)][actor(x)] >= seq(x)  (a change's own column holds seq - 1: the ops
//              of one change are concurrent)
//   value      x's own; a counter set with a numeric value adds every inc y in A(k) after x with
//              all_deps[change(y)][actor(x)] >= seq(x), in application order (INT + INT stays INT,
//              anything else is an f64 sum tagged FLOAT)
//   order      actor rank descending; two survivors of one actor are ops of one change, and of
//              x before y, y comes first exactly when A(k) holds an odd number of ops with key >=
//              key(y) (every assign reverses the list once after appending)
//
//  od_need_kernel    a lane per request: the largest work slice a request's document needs
//  od_walk_kernel    <FILL, LISTS>: FILL false = count, true = fill; LISTS = the call answers list / text
//                    element assigns (HM_ODF_LISTS, further down); one wavefront per request, a 64-lane
//                    workgroup of its own; per tile of HM_OD_TILE history positions below `to`:
//    mark / rank / scatter / scan   as past_fill_kernel: the tile's applied changes in history order
//             with their op rows' offsets (wave.h HistTile, wave_incl_scan)
//    then 64 ops a step in application order, a lane per op:
//      types  a make op leaves its object's type in the slice
//      link   an assign on a map / table register joins the register's chain: matches inside the
//             step are found in the wave (64 lane reads), last[reg] carries the chain across steps
//      emit   the ops of the range: rows are numbered by ballot, survivors by a wave scan of the
//             counts a first walk of the chain returns; the fill pass walks again to write them
//  The scan between count and fill is past_scan_kernel (hm_launch_past_scan).
//  od_walk_kernel    <false, LISTS, true>: the one-walk form (HM_ODF_ONCE): no count pass and no scan; a
//                    request takes a row block sized by the ops of its slice and, per step, a survivor
//                    block sized by the step's first walks, each with one atomicAdd on the call's
//                    totals (changes_kernel's pattern), and writes as it goes
//  od_walk_kernel    <FILL, LISTS, false, true>: the clock forms (OpDiffArgs.clock): a request names a clock
//                    instead of a slice and gets the whole patch of the changes applied at it.  A select
//                    phase (select_at) leaves a bit per log change in the slice; collect, mark and
//                    scatter read it where the slice forms test the history position, and every
//                    marked op is in range
//
// Every loop over a chain is bounded by the document's op rows, so tables that are not a merge's
// (overlapping op ranges) cannot hang a wave; no row past a lim_* of the source is read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/hypermerge_amd.h"
#include "op_diff_kernels.h"
#include "wave.h"

namespace hmo {

#define OWG 64
#define OTILE HM_OD_TILE
static_assert(sizeof(hm_op_row) == 32 && sizeof(hm_change_row) == 24 && sizeof(hm_op_diff) == 16 && sizeof(hm_surv_result) == 16, "row sizes");
static_assert(sizeof(hm_op_diff_summary) == sizeof(hm_past_summary), "the scan writes the summary as hm_past_summary");
static_assert(offsetof(hm_op_diff_summary, flags) == offsetof(hm_past_summary, doc_flags) &&
              offsetof(hm_op_diff_summary, bad) == offsetof(hm_past_summary, bad) &&
              offsetof(hm_op_diff_summary, max_surv) == offsetof(hm_past_summary, max_deps), "summary layout");

__global__ __launch_bounds__(256) void od_need_kernel(OpDiffArgs A, unsigned long long *out_words) {
    const unsigned long long q = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (q >= A.n) return;
    const DocRef s = doc_of(A.src, q);
    if (s.bad) return;
    const bool lm = (A.opts & HM_ODF_LISTS) && (s.flags & HM_DOC_HAS_LISTS);
    atomicMax(out_words, (lm ? hm_od_slice_words_lists(s.n_o, s.n_r, s.n_objs) : hm_od_slice_words(s.n_o, s.n_r, s.n_objs)) +
                             (A.clock ? hm_od_slice_words_clock(s.n_c) : 0ull));
    if (lm) atomicOr(out_words + 1, 1ull);                     // (a document of the call has lists)
}

struct Lds {
    HistTile<OTILE> tile;
    uint32_t src[OTILE];                       // per slot: the change's log row (document-local)
    uint32_t hp[OTILE];                        // per slot: its history position
    uint32_t op[OTILE];                        // per slot: op rows, then their offset within the tile
    uint32_t of[OTILE];                        // per slot: the change's first source op row
};

// a wave's slice of the work memory, laid out for one document
struct Slice {
    uint32_t *prev, *next, *chg;               // per document-local op: the chain and the op's change (log row)
    uint32_t *last;                            // per register: the last op of its chain so far
    uint32_t *otype;                           // per object: 0, or 1 + the make action that created it
};

__device__ __forceinline__ bool numeric(uint32_t vt) { return vt == HM_V_INT || vt == HM_V_FLOAT; }
__device__ __forceinline__ double num(uint32_t vt, uint64_t v) {
    return vt == HM_V_INT ? (double)(int64_t)v : __longlong_as_double((long long)v);
}

// survivor order: does a come before b?  (key = vtag word while a row is being built: the tag in
// bits 0-7, the actor rank in bits 8-23, bit 31 = the parity of the ops of A(k) at or after the op)
__device__ __forceinline__ bool before(uint32_t a_op, uint32_t a_key, uint32_t b_op, uint32_t b_key) {
    const uint32_t ra = (a_key >> 8) & 0xFFFFu, rb = (b_key >> 8) & 0xFFFFu;
    if (ra != rb) return ra > rb;
    const bool a_later = a_op > b_op;          // (one change: op order is application order)
    const bool odd = ((a_later ? a_key : b_key) >> 31) != 0u;
    return a_later == odd;
}

// The register of op k as it stands after k: returns its survivors; out != NULL: written to
// out[0 .. n) in their order, at most room of them.
__device__ uint32_t walk(const DocSource &D, const DocRef &s, const Slice &W, uint32_t k, hm_surv_result *out, uint32_t room) {
    uint32_t n = 0, step = 0;
    for (uint32_t x = k; x != HM_NONE && step < s.n_o; x = W.prev[x]) {
        step++;                                // ops of A(k) with key >= key(x)
        const hm_op_row xo = D.ops[s.o_off + x];
        if (xo.action != HM_SET && xo.action != HM_LINK) continue;
        const hm_change_row cx = D.changes[s.c_off + W.chg[x]];
        const uint32_t ax = cx.actor, sx = cx.seq;
        const bool counter = xo.datatype == HM_DT_COUNTER;
        uint32_t vt = xo.vtag;
        uint64_t val = xo.value;
        bool alive = true;
        if (x != k) {
            uint32_t guard = 0;
            for (uint32_t y = W.next[x]; y != HM_NONE && guard < s.n_o; y = W.next[y], guard++) {
                const hm_op_row yo = D.ops[s.o_off + y];
                const bool covers = ax < D.S && D.all_deps[(size_t)(s.c_off + W.chg[y]) * D.S + ax] >= sx;
                if (yo.action == HM_INC) {
                    if (covers && counter && numeric(vt)) {
                        if (vt == HM_V_INT && yo.vtag == HM_V_INT) val = (uint64_t)((int64_t)val + (int64_t)yo.value);
                        else {
                            val = (uint64_t)__double_as_longlong(num(vt, val) + num(yo.vtag, yo.value));
                            vt = HM_V_FLOAT;
                        }
                    }
                } else if (covers) { alive = false; break; }
                if (y == k) break;
            }
        }
        if (!alive) continue;
        if (out && n < room) {
            const uint32_t key = (vt & 0xFFu) | (ax << 8) | ((step & 1u) << 31);
            uint32_t j = n;                    // insertion by `before` (a register holds a handful of survivors)
            for (; j > 0; j--) {
                const hm_surv_result p = out[j - 1];
                if (!before(x, key, p.op, p.vtag)) break;
                out[j] = p;
            }
            hm_surv_result r;
            r.op = x; r.vtag = key; r.value = val;
            out[j] = r;
        }
        n++;
    }
    if (out) for (uint32_t j = 0; j < n && j < room; j++) out[j].vtag &= 0xFFu;
    return n;
}

// ---- list / text elements (HM_ODF_LISTS) -------------------------------------------------------------
// An element assign's diff carries the element's index at that moment: the visible elements of its
// list that precede it in RGA order.  The order of the whole prefix serves every moment inside it
// (two elements never change places), so per request the order phase ranks every element once:
//   collect  the applied ins ops below `to` as nodes (parent identity, ~elem, ~actor rank, register);
//            every _head child of every list hangs under one virtual root, keyed by its object, so
//            the lists lie end to end in object order
//   sort     a bitonic network over the slice, ascending: a run of one parent is its sibling list in
//            (elem, actor rank) descending order
//   tour     down / up edge per node over first child / next sibling / parent; ranked by pointer
//            jumping (weight 1 on down edges, ping-pong arrays, ceil(log2(2 nodes)) rounds)
//   pos[reg] = nodes - (down edges from the node's own to the end of the tour); a node whose tour
//            does not end at the root (its chain does not reach _head) keeps HM_NONE
// The walk then keeps a Fenwick tree over pos with +1 per visible element.
#define OD_END_GOOD 0xFFFFFFFFu
#define OD_END_BAD 0xFFFFFFFEu

struct ListSlice {
    uint32_t *pos, *vis;                       // per register
    uint32_t *fen;                             // [regs + 1] the Fenwick tree; order phase: register -> node
    uint32_t *fc;                              // per node: its first child (order phase)
    uint32_t *ofirst;                          // per object: the pos of the list's first element
    uint32_t *key;                             // [4 nodes]
    uint32_t *nxt, *sum;                       // [2][2 nodes] each
    uint32_t n;                                // nodes of the request
};

__device__ __forceinline__ uint32_t fen_prefix(const uint32_t *fen, uint32_t p) {   // visible elements at pos < p
    uint32_t v = 0;
    for (uint32_t i = p; i > 0u; i -= i & (0u - i)) v += fen[i];
    return v;
}
__device__ __forceinline__ void fen_add(uint32_t *fen, uint32_t n, uint32_t p, uint32_t delta) {
    for (uint32_t i = p + 1u; i <= n; i += i & (0u - i)) atomicAdd(&fen[i], delta);
}

__device__ __forceinline__ bool key_less(const uint32_t *a, const uint32_t *b) {
    for (uint32_t w = 0; w < 3u; w++)
        if (a[w] != b[w]) return a[w] < b[w];
    return a[3] < b[3];
}
// the parent a node hangs under: every _head child (top bit clear) under the one virtual root
__device__ __forceinline__ uint32_t parent_id(uint32_t w0) { return (w0 & 0x80000000u) ? w0 : 0u; }

// is log change i of the document applied at the request's clock (the select phase's bitmap)
__device__ __forceinline__ bool selected(const uint32_t *sel, uint32_t i) { return (sel[i >> 5] >> (i & 31u)) & 1u; }

// returns the nodes; ok = false: an ins row that cannot be a merge's (a register, object or parent
// outside the document, more applied ins ops than registers)
template <bool CLOCK>
__device__ uint32_t list_order(const DocSource &D, const DocRef &s, uint32_t lim, const uint32_t *sel, const ListSlice &X, uint32_t lane,
                               uint32_t *ctr, bool &ok) {
    if (lane == 0) *ctr = 0u;
    for (uint32_t i = lane; i < s.n_r; i += 64u) { X.pos[i] = HM_NONE; X.vis[i] = 0u; X.fen[i] = HM_NONE; X.fc[i] = HM_NONE; }
    for (uint32_t i = lane; i < s.n_objs; i += 64u) X.ofirst[i] = HM_NONE;
    __syncthreads();
    for (uint32_t i = lane; i < s.n_c; i += 64u) {             // collect
        if (CLOCK) {
            if (!selected(sel, i)) continue;
        } else {
            const int32_t hp = D.hist[s.c_off + i];
            if (hp < 0 || (uint32_t)hp >= lim) continue;
        }
        const hm_change_row c = D.changes[s.c_off + i];
        if (!c.n_ops) continue;
        if (c.op_first < s.o_off || (unsigned long long)c.op_first + c.n_ops > (unsigned long long)s.o_off + s.n_o) continue;   // (the walk reports it)
        for (uint32_t j = 0; j < c.n_ops; j++) {
            const uint32_t *row = (const uint32_t *)(D.ops + c.op_first + j);
            if ((row[4] & 0xFFu) != HM_INS) continue;
            const uint32_t obj = row[0], reg = row[1], parent = row[2], elem = row[3];
            if (reg >= s.n_r || obj >= s.n_objs || (parent != HM_HEAD && parent >= s.n_r)) { ok = false; continue; }
            const uint32_t k = atomicAdd(ctr, 1u);
            if (k >= s.n_r) { ok = false; continue; }
            uint32_t *e = X.key + 4u * k;
            e[0] = parent == HM_HEAD ? obj : (0x80000000u | parent); e[1] = ~elem; e[2] = 0xFFFFu - c.actor; e[3] = reg;
        }
    }
    __syncthreads();
    const uint32_t n = *ctr < s.n_r ? *ctr : s.n_r;
    __syncthreads();
    if (!n) return 0u;
    for (uint32_t k = 2; (k >> 1) < n; k <<= 1)                // sort: every comparator ascending, rows past n count as +inf
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            const uint32_t m = j == (k >> 1) ? k - 1u : j;
            for (uint32_t i = lane; i < n; i += 64u) {
                const uint32_t l = i ^ m;
                if (l <= i || l >= n) continue;
                uint32_t a[4], b[4];
                for (uint32_t w = 0; w < 4u; w++) { a[w] = X.key[4u * i + w]; b[w] = X.key[4u * l + w]; }
                if (key_less(b, a))
                    for (uint32_t w = 0; w < 4u; w++) { X.key[4u * i + w] = b[w]; X.key[4u * l + w] = a[w]; }
            }
            __syncthreads();
        }
    for (uint32_t i = lane; i < n; i += 64u) X.fen[X.key[4u * i + 3u]] = i;          // register -> node
    __syncthreads();
    for (uint32_t i = lane; i < n; i += 64u) {                 // a run's head is its parent's first child
        const uint32_t w0 = X.key[4u * i];
        if (!(w0 & 0x80000000u) || (i && X.key[4u * (i - 1u)] == w0)) continue;
        const uint32_t pn = X.fen[w0 & 0x7FFFFFFFu];
        if (pn != HM_NONE) X.fc[pn] = i;
    }
    __syncthreads();
    const uint32_t e2 = 2u * n;
    for (uint32_t i = lane; i < n; i += 64u) {                 // the tour
        const uint32_t w0 = X.key[4u * i], c = X.fc[i];
        const bool sib = i + 1u < n && parent_id(X.key[4u * (i + 1u)]) == parent_id(w0);
        uint32_t up;
        if (sib) up = 2u * (i + 1u);
        else if (!(w0 & 0x80000000u)) up = OD_END_GOOD;
        else {
            const uint32_t pn = X.fen[w0 & 0x7FFFFFFFu];
            up = pn != HM_NONE ? 2u * pn + 1u : OD_END_BAD;
        }
        X.nxt[2u * i] = c != HM_NONE ? 2u * c : 2u * i + 1u; X.sum[2u * i] = 1u;
        X.nxt[2u * i + 1u] = up; X.sum[2u * i + 1u] = 0u;
    }
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t span = 1; span < e2; span <<= 1) {           // pointer jumping
        const uint32_t *sn = X.nxt + cur * e2, *ss = X.sum + cur * e2;
        uint32_t *dn = X.nxt + (cur ^ 1u) * e2, *dsum = X.sum + (cur ^ 1u) * e2;
        for (uint32_t e = lane; e < e2; e += 64u) {
            uint32_t t = sn[e], v = ss[e];
            if (t < e2) { v += ss[t]; t = sn[t]; }
            dn[e] = t; dsum[e] = v;
        }
        cur ^= 1u;
        __syncthreads();
    }
    const uint32_t *fn = X.nxt + cur * e2, *fs = X.sum + cur * e2;
    for (uint32_t i = lane; i < n; i += 64u) {
        const uint32_t v = fs[2u * i];
        if (fn[2u * i] != OD_END_GOOD || v == 0u || v > n) continue;
        const uint32_t w0 = X.key[4u * i];
        X.pos[X.key[4u * i + 3u]] = n - v;
        if (!(w0 & 0x80000000u) && (i == 0u || X.key[4u * (i - 1u)] != w0)) X.ofirst[w0] = n - v;
    }
    __syncthreads();
    for (uint32_t i = lane; i <= n; i += 64u) X.fen[i] = 0u;
    __syncthreads();
    return n;
}

// a 64-bit sum over the wave, in every lane
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// The select phase of the clock forms: which log changes of the document are applied at clock K, a bit
// per log change in sel[] (hm_od_slice_words_clock words): hist >= 0, seq <= K[actor] and the all_deps
// row <= K in every column.  64 changes a step, a lane per change for the cheap part; the row is then
// read by the change's own lane at strides up to 16 (at most 64 B a lane), and above that by the whole
// wave, a lane per column, 256 B a read, for the changes the cheap part left (a uniform loop over the
// step's ballot).  Returns 1 + the largest selected history position (0: nothing selected), in every lane.
__device__ uint32_t select_at(const DocSource &D, const DocRef &s, const uint32_t *K, uint32_t *sel, uint32_t lane) {
    const uint32_t S = D.S;
    uint32_t top = 0;
    for (uint32_t base = 0; base < s.n_c; base += 64u) {
        const uint32_t i = base + lane;
        bool c = false;
        if (i < s.n_c) {
            const int32_t hp = D.hist[s.c_off + i];
            const hm_change_row r = D.changes[s.c_off + i];
            c = hp >= 0 && (uint32_t)hp < s.n_c && r.actor < S && r.seq <= K[r.actor];
            if (c && S <= 16u) {
                const uint32_t *row = D.all_deps + (size_t)(s.c_off + i) * S;
                for (uint32_t a = 0; a < S; a++) c &= row[a] <= K[a];
            }
            if (c && S <= 16u) top = max(top, (uint32_t)hp + 1u);
        }
        unsigned long long m = __ballot(c);
        if (S > 16u) {
            for (uint32_t j = 0; j < 64u; j++) {               // (uniform: m is the wave's)
                if (!((m >> j) & 1ull)) continue;
                const uint32_t *row = D.all_deps + (size_t)(s.c_off + base + j) * S;
                bool ok = true;
                for (uint32_t a = lane; a < S; a += 64u) ok &= row[a] <= K[a];
                if (__ballot(!ok)) m &= ~(1ull << j);
            }
            if (i < s.n_c && ((m >> lane) & 1ull)) top = max(top, (uint32_t)D.hist[s.c_off + i] + 1u);
        }
        if (lane == 0) {
            sel[base >> 5] = (uint32_t)m;
            if (base + 32u < s.n_c) sel[(base >> 5) + 1u] = (uint32_t)(m >> 32);
        }
    }
    for (uint32_t d = 32; d; d >>= 1) top = max(top, __shfl_xor(top, d));
    __syncthreads();
    return top;
}

template <bool FILL, bool LISTS, bool ONCE = false, bool CLOCK = false>
__global__ __launch_bounds__(OWG) void od_walk_kernel(OpDiffArgs A) {
    static_assert(!(FILL && ONCE), "the one-walk form has no fill pass");
    static_assert(!(CLOCK && ONCE), "the one-walk form takes no clock");
    __shared__ Lds L;
    const uint32_t lane = threadIdx.x;
    const DocSource &D = A.src;
    if (FILL) {
        const hm_op_diff_summary *t = A.sum;                  // (one decision for the whole grid)
        if (t->totals[0] > A.cap_rows || t->totals[1] > A.cap_surv) return;
    }
    uint32_t *const wbase = A.work + (size_t)blockIdx.x * A.slice_words;
    for (unsigned long long q = blockIdx.x; q < A.n; q += gridDim.x) {
        DocRef s = doc_of(D, q);
        const uint32_t from = CLOCK ? 0u : A.from[q], to = CLOCK ? 0u : A.to[q];
        uint4 cn = make_uint4(0, 0, 0, 0), of = make_uint4(0, 0, 0, 0);
        uint32_t fl = 0;
        if (FILL) {
            cn = *(const uint4 *)(A.cnt + 4 * q); of = *(const uint4 *)(A.off + 4 * q);
            fl = A.aux[2 * q + 1];
            if (lane == 0) {
                *(uint2 *)(A.out_range + 2 * q) = make_uint2(of.x, cn.x);
                A.out_flags[q] = fl;
            }
            if (!cn.x) continue;
        }
        uint32_t bad = s.bad ? HM_OD_BAD_HANDLE : 0u;
        // element assigns are answered for a document that says it has lists; without the hint they are flagged
        const bool lm = LISTS && (s.flags & HM_DOC_HAS_LISTS);
        unsigned long long sel_at = 0;                         // CLOCK: the bitmap follows the document's other words
        if (CLOCK) {
            sel_at = lm ? hm_od_slice_words_lists(s.n_o, s.n_r, s.n_objs) : hm_od_slice_words(s.n_o, s.n_r, s.n_objs);
            if (sel_at + hm_od_slice_words_clock(s.n_c) > A.slice_words) { bad |= HM_OD_BAD_WORK; s.n_c = 0; }
        } else if ((lm ? hm_od_slice_words_lists(s.n_o, s.n_r, s.n_objs) : hm_od_slice_words(s.n_o, s.n_r, s.n_objs)) > A.slice_words) { bad |= HM_OD_BAD_WORK; s.n_c = 0; }
        Slice W;
        W.prev = wbase; W.next = W.prev + s.n_o; W.chg = W.next + s.n_o; W.last = W.chg + s.n_o; W.otype = W.last + s.n_r;
        ListSlice X = {};
        if (LISTS) {
            X.pos = W.otype + s.n_objs; X.vis = X.pos + s.n_r; X.fen = X.vis + s.n_r; X.fc = X.fen + s.n_r + 1u;
            X.ofirst = X.fc + s.n_r; X.key = X.ofirst + s.n_objs; X.nxt = X.key + 4u * (size_t)s.n_r; X.sum = X.nxt + 4u * (size_t)s.n_r;
        }
        // CLOCK: history positions of interest are the selected ones, all of them in range (the patch
        // from the empty document)
        uint32_t *const sel = CLOCK ? wbase + sel_at : nullptr;
        const uint32_t lim = CLOCK ? select_at(D, s, A.clock + (size_t)q * D.S, sel, lane)
                                   : (to < s.n_c ? to : s.n_c);   // history positions of interest lie below it
        uint32_t rows = 0, surv = 0;                           // emitted so far
        bool lists = false, rows_ok = true;
        // ONCE: the request's row block (the ops of its slice bound its rows: an ins emits none, every
        // other op at most one), reserved on the call's row total; written only when it fits
        unsigned long long blk = 0, bound = 0;
        bool fits = false;
        if (ONCE) {
            if (from < lim)
                for (uint32_t i = lane; i < s.n_c; i += 64u) {
                    const int32_t hp = D.hist[s.c_off + i];
                    if (hp < 0 || (uint32_t)hp < from || (uint32_t)hp >= lim) continue;
                    const hm_change_row c = D.changes[s.c_off + i];
                    if (c.n_ops && c.op_first >= s.o_off && (unsigned long long)c.op_first + c.n_ops <= (unsigned long long)s.o_off + s.n_o)
                        bound += c.n_ops;
                }
            bound = wave_sum64(bound);
            if (bound) {                                       // (uniform branch)
                if (lane == 0) blk = atomicAdd((unsigned long long *)&A.sum->totals[0], bound);
                blk = __shfl(blk, 0);
                fits = blk + bound <= (unsigned long long)A.cap_rows;
            }
        }
        if (from < lim) {
            for (uint32_t i = lane; i < s.n_r; i += 64u) W.last[i] = HM_NONE;
            for (uint32_t i = lane; i < s.n_objs; i += 64u) W.otype[i] = 0u;
            if (LISTS && lm) X.n = list_order<CLOCK>(D, s, lim, sel, X, lane, &L.src[0], rows_ok);
        }
        const uint32_t n_tiles = from < lim ? (lim + OTILE - 1u) / OTILE : 0u;
        for (uint32_t t = 0; t < n_tiles; t++) {
            L.tile.clear(lane);
            __syncthreads();
            for (uint32_t i = lane; i < s.n_c; i += 64u) {     // mark
                const int32_t hp = D.hist[s.c_off + i];
                if (CLOCK ? selected(sel, i) && (uint32_t)hp / OTILE == t
                          : hp >= 0 && (uint32_t)hp < lim && (uint32_t)hp / OTILE == t) L.tile.mark((uint32_t)hp);
            }
            __syncthreads();
            const uint32_t tile_n = L.tile.rank(lane);         // rank
            __syncthreads();
            if (!tile_n) continue;
            for (uint32_t i = lane; i < s.n_c; i += 64u) {     // scatter
                const int32_t hp = D.hist[s.c_off + i];
                if (CLOCK ? !selected(sel, i) || (uint32_t)hp / OTILE != t
                          : hp < 0 || (uint32_t)hp >= lim || (uint32_t)hp / OTILE != t) continue;
                uint32_t k;
                if (!L.tile.slot((uint32_t)hp, k)) continue;
                const hm_change_row c = D.changes[s.c_off + i];
                uint32_t no = c.n_ops;
                if (no && (c.op_first < s.o_off || (unsigned long long)c.op_first + no > (unsigned long long)s.o_off + s.n_o)) { no = 0; rows_ok = false; }
                L.src[k] = i; L.hp[k] = (uint32_t)hp; L.op[k] = no; L.of[k] = c.op_first;
            }
            __syncthreads();
            uint32_t osum = 0;                                  // scan
            for (uint32_t k0 = 0; k0 < tile_n; k0 += 64u) {
                const uint32_t k = k0 + lane;
                const uint32_t vo = k < tile_n ? L.op[k] : 0u;
                const uint32_t io = wave_incl_scan(vo, lane);
                if (k < tile_n) L.op[k] = osum + io - vo;
                osum += __shfl(io, 63);
            }
            __syncthreads();
            for (uint32_t k0 = 0; k0 < osum; k0 += 64u) {      // the tile's ops, 64 a step in application order
                const uint32_t k = k0 + lane;
                const bool valid = k < osum;
                uint32_t dop = HM_NONE, ci = 0, p = 0, obj = HM_NONE, reg = HM_NONE, action = HM_INS;
                if (valid) {
                    uint32_t lo = 0, hi = tile_n;              // the last slot whose op offset is <= k
                    while (hi - lo > 1u) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (L.op[mid] <= k) lo = mid; else hi = mid;
                    }
                    const uint32_t srow = L.of[lo] + (k - L.op[lo]);
                    const uint4 w0 = *(const uint4 *)(D.ops + srow);          // obj, reg, parent, elem
                    const uint32_t w1 = ((const uint32_t *)(D.ops + srow))[4]; // action, datatype, vtag, pad
                    dop = srow - s.o_off; ci = L.src[lo]; p = L.hp[lo];
                    obj = w0.x; reg = w0.y; action = w1 & 0xFFu;
                }
                const bool make = valid && action <= HM_MAKE_TEXT, assign = valid && action >= HM_SET && action <= HM_INC;
                if (make && obj < s.n_objs) W.otype[obj] = 1u + action;          // types
                __syncthreads();
                const uint32_t ot = assign && obj < s.n_objs ? W.otype[obj] : 0u;
                const bool list = ot == 1u + HM_MAKE_LIST || ot == 1u + HM_MAKE_TEXT;
                const bool in_range = valid && (CLOCK || p >= from);
                lists |= in_range && list && !(LISTS && lm);
                const bool chain = assign && (!list || (LISTS && lm)) && reg != HM_NONE && reg < s.n_r;
                const bool el = LISTS && chain && list;         // an element assign that is answered
                const unsigned long long cm = __ballot(chain);
                uint32_t pl = HM_NONE, nl = HM_NONE;           // nearest lanes below / above with the same register
                if (cm) {                                       // link (uniform branch)
                    for (uint32_t j = 0; j < 64u; j++) {
                        if (!((cm >> j) & 1ull)) continue;
                        const uint32_t rj = __shfl(reg, j);
                        if (chain && rj == reg) {
                            if (j < lane) pl = j;
                            else if (j > lane && nl == HM_NONE) nl = j;
                        }
                    }
                    const uint32_t dpl = __shfl(dop, pl == HM_NONE ? lane : pl), dnl = __shfl(dop, nl == HM_NONE ? lane : nl);
                    if (chain) {
                        const uint32_t pv = pl != HM_NONE ? dpl : W.last[reg];
                        W.prev[dop] = pv; W.next[dop] = nl != HM_NONE ? dnl : HM_NONE; W.chg[dop] = ci;
                        if (pl == HM_NONE && pv != HM_NONE && pv < s.n_o) W.next[pv] = dop;
                    }
                    __syncthreads();                            // (last[reg] read by the first lanes before the last lanes write it)
                    if (chain && nl == HM_NONE) W.last[reg] = dop;
                    __syncthreads();
                }
                uint32_t ns = 0, idx = HM_NONE;
                bool was = false, now = false;                   // the element's visibility before and after the op
                if (LISTS) {                                    // index
                    uint32_t pe = HM_NONE, lo = 0;
                    if (el) { pe = X.pos[reg]; lo = X.ofirst[obj]; }
                    const bool elv = el && pe != HM_NONE && lo != HM_NONE;
                    if (el && !elv) rows_ok = false;            // (no applied ins made this element: not a merge's tables)
                    if (__ballot(elv)) {                        // (uniform branch)
                        if (elv) { ns = walk(D, s, W, dop, nullptr, 0u); now = ns != 0u; }
                        const uint32_t now_pl = __shfl((uint32_t)now, pl == HM_NONE ? lane : pl);
                        if (elv) was = pl != HM_NONE ? now_pl != 0u : X.vis[reg] != 0u;
                        const uint32_t delta = (uint32_t)now - (uint32_t)was;
                        if (elv) idx = fen_prefix(X.fen, pe) - fen_prefix(X.fen, lo);   // as of the step's start
                        const unsigned long long tm = __ballot(elv && delta != 0u);
                        for (uint32_t j = 0; j < 64u; j++) {    // the earlier lanes of the step
                            if (!((tm >> j) & 1ull)) continue;
                            const uint32_t pj = __shfl(pe, j), dj = __shfl(delta, j);
                            if (elv && j < lane && pj >= lo && pj < pe) idx += dj;
                        }
                        __syncthreads();                        // (the tree is read before it is updated)
                        if (elv && delta != 0u) fen_add(X.fen, X.n, pe, delta);
                        if (elv && nl == HM_NONE) X.vis[reg] = (uint32_t)now;
                        __syncthreads();
                    }
                }
                const bool emit = in_range && (make || (chain && (!el || was || now)));  // emit
                const unsigned long long em = __ballot(emit);
                if (!em) continue;
                const uint32_t row = rows + (uint32_t)__popcll(em & ((1ull << lane) - 1ull));
                if (emit && chain && !el && !(FILL && fl)) ns = walk(D, s, W, dop, nullptr, 0u);
                if (LISTS && !emit) ns = 0u;                    // (an element assign outside the range was walked for its visibility)
                const uint32_t is = wave_incl_scan(ns, lane);
                if (FILL && emit && !fl) {
                    const uint32_t so = surv + is - ns;
                    if (row < cn.x && (unsigned long long)so + ns <= cn.y) {
                        if (ns) walk(D, s, W, dop, A.out_surv + of.y + so, ns);
                        hm_op_diff r;
                        r.op = dop; r.kind = make ? HM_OD_CREATE : (ns ? HM_OD_SET : HM_OD_REMOVE); r.n_surv = ns; r.surv_off = of.y + so;
                        if (LISTS && el) r.kind = was ? (now ? HM_OD_ELEM_SET : HM_OD_ELEM_REMOVE) : HM_OD_ELEM_INSERT;
                        A.out_rows[of.x + row] = r;
                        if (LISTS) A.out_index[of.x + row] = idx;
                    }
                }
                if (ONCE) {
                    // the step's survivor block, reserved on the call's survivor total by the sizes the
                    // first walks returned; the second walk writes into it
                    const uint32_t ssum = __shfl(is, 63);
                    unsigned long long sblk = 0;
                    if (ssum) {                                 // (uniform branch)
                        if (lane == 0) sblk = atomicAdd((unsigned long long *)&A.sum->totals[1], (unsigned long long)ssum);
                        sblk = __shfl(sblk, 0);
                    }
                    if (emit && fits && row < bound && sblk + ssum <= (unsigned long long)A.cap_surv) {
                        const unsigned long long so = sblk + is - ns;
                        if (ns) walk(D, s, W, dop, A.out_surv + so, ns);
                        hm_op_diff r;
                        r.op = dop; r.kind = make ? HM_OD_CREATE : (ns ? HM_OD_SET : HM_OD_REMOVE); r.n_surv = ns; r.surv_off = (uint32_t)so;
                        if (LISTS && el) r.kind = was ? (now ? HM_OD_ELEM_SET : HM_OD_ELEM_REMOVE) : HM_OD_ELEM_INSERT;
                        A.out_rows[blk + row] = r;
                        if (LISTS) A.out_index[blk + row] = idx;
                    }
                }
                rows += (uint32_t)__popcll(em); surv += __shfl(is, 63);
            }
            __syncthreads();
        }
        if (ONCE) {
            // (a flagged request keeps its block and refers to none of it)
            const bool any_lists = __ballot(lists) != 0ull, any_rows_bad = __ballot(!rows_ok) != 0ull;
            if (any_rows_bad) bad |= HM_OD_BAD_ROWS;
            if (lane == 0) {
                *(uint2 *)(A.out_range + 2 * q) = make_uint2((uint32_t)blk, any_lists || !fits ? 0u : rows);
                A.out_flags[q] = any_lists ? HM_OD_LISTS : 0u;
                if (any_lists) atomicOr(&A.sum->flags, HM_OD_LISTS);
                if (bad) atomicOr(&A.sum->bad, bad);
            }
        } else if (!FILL) {
            const bool any_lists = __ballot(lists) != 0ull, any_rows_bad = __ballot(!rows_ok) != 0ull;
            if (any_rows_bad) bad |= HM_OD_BAD_ROWS;
            if (lane == 0) {
                *(uint4 *)(A.cnt + 4 * q) = any_lists ? make_uint4(0, 0, 0, 0) : make_uint4(rows, surv, 0, 0);
                *(uint2 *)(A.aux + 2 * q) = make_uint2(0u, any_lists ? HM_OD_LISTS : 0u);
                if (bad) atomicOr(&A.sum->bad, bad);
            }
        }
    }
}

}  // namespace hmo

static PastArgs scan_args(const OpDiffArgs &a) {
    PastArgs P = {};
    P.n = a.n; P.cnt = a.cnt; P.aux = a.aux; P.off = a.off; P.part = a.part; P.sum = (hm_past_summary *)a.sum;
    return P;
}

hipError_t hm_launch_op_diff_need(const OpDiffArgs &a, unsigned long long *out_words, hipStream_t s) {
    if (!a.n) return hipSuccess;
    hipLaunchKernelGGL(hmo::od_need_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a, out_words);
    return hipGetLastError();
}

hipError_t hm_launch_op_diff_count(const OpDiffArgs &a, hipStream_t s) {
    hipError_t r = hipMemsetAsync(a.sum, 0, sizeof(hm_op_diff_summary), s);
    if (r != hipSuccess || !a.n) return r;                     // (no request: the zero summary is the answer)
    if (a.clock) {
        if (a.opts & HM_ODF_LISTS) hipLaunchKernelGGL((hmo::od_walk_kernel<false, true, false, true>), dim3(a.waves ? a.waves : 1u), dim3(OWG), 0, s, a);
        else hipLaunchKernelGGL((hmo::od_walk_kernel<false, false, false, true>), dim3(a.waves ? a.waves : 1u), dim3(OWG), 0, s, a);
    } else if (a.opts & HM_ODF_LISTS) hipLaunchKernelGGL((hmo::od_walk_kernel<false, true>), dim3(a.waves ? a.waves : 1u), dim3(OWG), 0, s, a);
    else hipLaunchKernelGGL((hmo::od_walk_kernel<false, false>), dim3(a.waves ? a.waves : 1u), dim3(OWG), 0, s, a);
    if ((r = hipGetLastError()) != hipSuccess) return r;
    return hm_launch_past_scan(scan_args(a), s);
}

hipError_t hm_launch_op_diff_once(const OpDiffArgs &a, hipStream_t s) {
    hipError_t r = hipMemsetAsync(a.sum, 0, sizeof(hm_op_diff_summary), s);
    if (r != hipSuccess || !a.n) return r;
    if (a.clock) return hipErrorInvalidValue;                  // (the one-walk form takes no clock)
    if (a.opts & HM_ODF_LISTS) hipLaunchKernelGGL((hmo::od_walk_kernel<false, true, true>), dim3(a.waves ? a.waves : 1u), dim3(OWG), 0, s, a);
    else {                                                     // (no document of the call has lists: no row has an index)
        if (a.out_index && a.cap_rows && (r = hipMemsetAsync(a.out_index, 0xFF, (size_t)a.cap_rows * 4, s)) != hipSuccess) return r;
        hipLaunchKernelGGL((hmo::od_walk_kernel<false, false, true>), dim3(a.waves ? a.waves : 1u), dim3(OWG), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t hm_launch_op_diff_fill(const OpDiffArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    const dim3 grid(a.waves ? a.waves : 1u);
    if (a.opts & HM_ODF_LISTS) {
        if (a.clock) hipLaunchKernelGGL((hmo::od_walk_kernel<true, true, false, true>), grid, dim3(OWG), 0, s, a);
        else hipLaunchKernelGGL((hmo::od_walk_kernel<true, true>), grid, dim3(OWG), 0, s, a);
        return hipGetLastError();
    }
    if (a.out_index && a.cap_rows) {                           // (no document of the call has lists: no row has an index)
        const hipError_t r = hipMemsetAsync(a.out_index, 0xFF, (size_t)a.cap_rows * 4, s);
        if (r != hipSuccess) return r;
    }
    if (a.clock) hipLaunchKernelGGL((hmo::od_walk_kernel<true, false, false, true>), grid, dim3(OWG), 0, s, a);
    else hipLaunchKernelGGL((hmo::od_walk_kernel<true, false>), grid, dim3(OWG), 0, s, a);
    return hipGetLastError();
}
