// docset.cpp — the host engine of the Node drop-in (include/hypermerge_amd.h, hm_docset_*).
//
// What the reference runs on the JS main thread for every arriving block, per document,
// natively and over many documents per call:
//   Actor.parseBlock / Block.unpack / JsonBuffer.parse   (src/Actor.ts:137-141, src/Block.ts:18-29,
//                                                         src/JsonBuffer.ts:1-4)
//   DocBackend.applyRemoteChanges -> Backend.applyChanges (src/DocBackend.ts:169-185)
//   DocBackend.updateClock, the patch of RemotePatchMsg   (src/DocBackend.ts:135-142, :173-183)
// A docset owns the documents of one device: their interners (actor ids ranked in JS string
// order, object UUIDs, (object, key|elemId) registers, string values, content identity of
// changes — columnar.js DocEncoder, kept across rounds), their placement in the resident
// stores (one hm_store per actor-stride class 8/16/32/64/128/256: a document moves to a wider class
// when a new actor outgrows its rows, its log rows re-submitted from the old store), and the
// patch base (the document as the last patch left it).  One call = one applyChanges round
// for every document of the call, the phases of `struct Call` in apply()'s order: validate,
// decode (on host threads), place (stride classes), merge_class (per class: handles, one batch
// built, submitted, waited for), settle (a document whose merge failed rolls back — a throwing
// applyChanges leaves DocBackend.back unchanged — and the others' reads are listed), read_regs
// (net diffs: the registers the round's ops hit, every register when changes were queued),
// read_history (op diffs: the applied changes in order; HM_DOCSET_DEVICE_DIFFS: read_diffs instead, the
// device's per-op rows of every round's slice), commit, release, render (each document's
// patch, opSet clock / deps and DocBackend.clock, binary or JSON), verify, assemble; fail() from
// any phase before commit applies the call to no store and rolls every document back.
//
// Content identity (Automerge's `Inconsistent reuse of sequence number` check, Immutable
// `equals` of two changes with one (actor, seq)) is a 128-bit hash of each change's
// canonical form (maps order-insensitive, last duplicate key wins, numbers by value), kept
// per (actor, seq): the blocks themselves stay with the caller.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>
#include "../../include/hypermerge_amd.h"
#include "engine_internal.h"
#include "scan.h"

namespace {

using namespace hmscan;

constexpr uint32_t N_CLASS = 6;
constexpr uint32_t STRIDES[N_CLASS] = {8, 16, 32, 64, 128, 256};
// a document's actors: rank 255 stays free for the stores' 0xFF "no rank" entries
constexpr uint32_t MAX_ACTORS = HM_MAX_STRIDE - 1;
constexpr uint8_t NO_CLASS = 0xFF;
constexpr uint8_t NO_TYPE = 0xFF;

inline uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

// (tag, bytes) -> dense id in first-insertion order, owning its bytes
struct Names {
    std::string arena;
    struct K { uint32_t off, len, tag, h; };
    std::vector<K> keys;
    std::vector<uint32_t> slot;                              // id + 1, 0 = empty
    uint32_t mask = 0;
    uint32_t size() const { return (uint32_t)keys.size(); }
    const char *ptr(uint32_t id) const { return arena.data() + keys[id].off; }
    uint32_t len(uint32_t id) const { return keys[id].len; }
    uint32_t tag(uint32_t id) const { return keys[id].tag; }
    void rehash(size_t cap) {
        slot.assign(cap, 0);
        mask = (uint32_t)cap - 1;
        for (uint32_t id = 0; id < keys.size(); id++) {
            uint32_t i = keys[id].h & mask;
            while (slot[i]) i = (i + 1) & mask;
            slot[i] = id + 1;
        }
    }
    uint32_t get(const char *p, uint32_t n, uint32_t tg, bool &fresh) {
        if ((keys.size() + 1) * 2 > slot.size()) rehash(std::max<size_t>(16, slot.size() * 2));
        const uint32_t h = (uint32_t)hash_bytes(p, n, tg);
        for (uint32_t i = h & mask;; i = (i + 1) & mask) {
            const uint32_t v = slot[i];
            if (!v) {
                slot[i] = size() + 1;
                keys.push_back({(uint32_t)arena.size(), n, tg, h});
                arena.append(p, n);
                fresh = true;
                return size() - 1;
            }
            const K &k = keys[v - 1];
            if (k.h == h && k.tag == tg && k.len == n && !memcmp(arena.data() + k.off, p, n)) { fresh = false; return v - 1; }
        }
    }
    // the id of a name already interned, or HM_NONE (nothing is added)
    uint32_t find(const char *p, uint32_t n, uint32_t tg) const {
        if (slot.empty()) return HM_NONE;
        const uint32_t h = (uint32_t)hash_bytes(p, n, tg);
        for (uint32_t i = h & mask;; i = (i + 1) & mask) {
            const uint32_t v = slot[i];
            if (!v) return HM_NONE;
            const K &k = keys[v - 1];
            if (k.h == h && k.tag == tg && k.len == n && !memcmp(arena.data() + k.off, p, n)) return v - 1;
        }
    }
    void truncate(uint32_t n) {
        if (n >= keys.size()) return;
        arena.resize(keys[n].off);
        keys.resize(n);
        rehash(std::max<size_t>(16, slot.size()));
    }
};

// ---------------- content identity: a 128-bit hash of a change's canonical form ----------------
struct H2 { uint64_t a, b; bool operator==(const H2 &o) const { return a == o.a && b == o.b; } };

H2 leaf(uint64_t tag, const char *p, size_t n) {
    return {mix64(hash_bytes(p, (uint32_t)n, 0x51ED270B27A1F00Dull ^ tag)), mix64(hash_bytes(p, (uint32_t)n, 0x2545F4914F6CDD1Dull + tag))};
}

struct CHash {
    const char *p, *e;
    std::vector<std::pair<H2, H2>> &stk;                     // (key, value) of the open objects' fields
    std::string &tmp;
    void ws() { while (p < e && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) p++; }
    bool str(H2 &h) {
        if (p >= e || *p != '"') return false;
        const char *s = p + 1, *q = s;
        while (q < e && *q != '"' && *q != '\\') q++;
        if (q < e && *q == '"') { h = leaf(5, s, (size_t)(q - s)); p = q + 1; return true; }
        Parser P{p, e};
        if (!P.string(tmp)) return false;
        p = P.p;
        h = leaf(5, tmp.data(), tmp.size());
        return true;
    }
    bool val(H2 &h, int depth) {
        if (depth > 256) return false;
        ws();
        if (p >= e) return false;
        const char c = *p;
        if (c == '"') return str(h);
        if (c == '{') {
            p++;
            const size_t base = stk.size();
            ws();
            if (p < e && *p == '}') p++;
            else for (;;) {
                ws();
                H2 k, v;
                if (!str(k)) return false;
                ws();
                if (p >= e || *p != ':') return false;
                p++;
                if (!val(v, depth + 1)) return false;
                bool dup = false;                             // JSON.parse: the last duplicate key wins
                for (size_t i = base; i < stk.size(); i++) if (stk[i].first == k) { stk[i].second = v; dup = true; }
                if (!dup) stk.push_back({k, v});
                ws();
                if (p < e && *p == ',') { p++; continue; }
                if (p < e && *p == '}') { p++; break; }
                return false;
            }
            uint64_t A = 0, B = 0;                            // order-insensitive over the fields
            for (size_t i = base; i < stk.size(); i++) {
                A += mix64(stk[i].first.a * 0x9E3779B97F4A7C15ull ^ stk[i].second.a);
                B += mix64(stk[i].first.b + 0xD6E8FEB86659FD93ull * stk[i].second.b);
            }
            const uint64_t n = stk.size() - base;
            stk.resize(base);
            h = {mix64(A ^ (0x7A11ull << 48) ^ n), mix64(B + 0x0B1Eull + n)};
            return true;
        }
        if (c == '[') {
            p++;
            uint64_t A = 0x1234567ull, B = 0x89ABCDEFull, n = 0;
            ws();
            if (p < e && *p == ']') p++;
            else for (;;) {
                H2 v;
                if (!val(v, depth + 1)) return false;
                A = mix64(A * 31 + v.a); B = mix64(B ^ (v.b + n));
                n++;
                ws();
                if (p < e && *p == ',') { p++; continue; }
                if (p < e && *p == ']') { p++; break; }
                return false;
            }
            h = {A ^ n, B + n};
            return true;
        }
        if (e - p >= 4 && !memcmp(p, "null", 4)) { p += 4; h = leaf(0, "", 0); return true; }
        if (e - p >= 4 && !memcmp(p, "true", 4)) { p += 4; h = leaf(2, "", 0); return true; }
        if (e - p >= 5 && !memcmp(p, "false", 5)) { p += 5; h = leaf(1, "", 0); return true; }
        Parser P{p, e};                                       // a number, compared by value (0 == -0)
        JV j;
        if (!P.value(j, 0) || j.t != J_NUM) return false;
        p = P.p;
        double v = j.num == 0 ? 0.0 : j.num;
        h = leaf(3, (const char *)&v, 8);
        return true;
    }
};

// A list's placed elements in document order, in blocks: a position, an insertion or a visible
// index costs O(blocks + block size) instead of O(elements) (a text document holds thousands of
// elements, and the per-op replay asks for one of these per list op).  Blocks have stable ids;
// `where` (per register, the document's) names each placed element's block; a block keeps its
// count of visible elements (a non-empty survivor set).
struct ListOrder {
    static constexpr uint32_t SPLIT = 256;
    struct Blk { std::vector<uint32_t> el; uint32_t vis = 0; };
    std::vector<Blk> pool;                                   // by block id
    std::vector<uint32_t> seq;                               // block ids in document order
    uint32_t n = 0;
    uint32_t size() const { return n; }
    uint32_t pos_of(uint32_t e, const std::vector<uint32_t> &where) const {
        const uint32_t b = where[e];
        uint32_t at = 0;
        for (uint32_t id : seq) {
            if (id == b) break;
            at += (uint32_t)pool[id].el.size();
        }
        const auto &v = pool[b].el;
        return at + (uint32_t)(std::find(v.begin(), v.end(), e) - v.begin());
    }
    template <typename Vis>
    uint32_t vis_before(uint32_t e, const std::vector<uint32_t> &where, Vis &&vis) const {
        if (e >= where.size() || where[e] == HM_NONE) return 0;
        const uint32_t b = where[e];
        uint32_t c = 0;
        for (uint32_t id : seq) {
            if (id == b) break;
            c += pool[id].vis;
        }
        for (uint32_t x : pool[b].el) {
            if (x == e) break;
            c += vis(x) ? 1u : 0u;
        }
        return c;
    }
    // the elements `sub` (in order) at position pos
    template <typename Vis>
    void insert_at(uint32_t pos, const std::vector<uint32_t> &sub, std::vector<uint32_t> &where, Vis &&vis) {
        if (sub.empty()) return;
        if (seq.empty()) { pool.emplace_back(); seq.push_back(0); }
        uint32_t k = 0, at = 0;
        while (k + 1 < seq.size() && at + pool[seq[k]].el.size() < pos) at += (uint32_t)pool[seq[k++]].el.size();
        const uint32_t b = seq[k];
        Blk &B = pool[b];
        B.el.insert(B.el.begin() + (pos - at), sub.begin(), sub.end());
        for (uint32_t x : sub) { where[x] = b; B.vis += vis(x) ? 1u : 0u; }
        n += (uint32_t)sub.size();
        if (pool[b].el.size() > SPLIT) {                     // split off the second half
            const uint32_t nb = (uint32_t)pool.size();
            pool.emplace_back();
            Blk &L = pool[b], &R = pool[nb];
            const size_t half = L.el.size() / 2;
            R.el.assign(L.el.begin() + half, L.el.end());
            L.el.resize(half);
            R.vis = 0;
            for (uint32_t x : R.el) { where[x] = nb; R.vis += vis(x) ? 1u : 0u; }
            L.vis -= R.vis;
            seq.insert(seq.begin() + k + 1, nb);
        }
    }
    void vis_change(uint32_t e, const std::vector<uint32_t> &where, bool now) {
        if (e < where.size() && where[e] != HM_NONE) { Blk &B = pool[where[e]]; B.vis = now ? B.vis + 1 : B.vis - 1; }
    }
};

// ---------------- one document ----------------
struct DocSt {
    bool ready = false;
    Names actors, objs, regs, strs;                          // actors: ids in first-appearance order
    std::vector<uint16_t> rank_of, by_rank;                  // actor id -> rank (JS string order) and back
    // content identity: (actor id, seq) -> chain of (canonical hash, content id)
    std::vector<uint64_t> ckey;                              // key + 1, 0 = empty slot
    std::vector<uint32_t> chead;
    struct CE { uint64_t key; H2 h; uint32_t cid, next; };
    std::vector<CE> cents;
    uint32_t n_content = 0;
    // the log (what the stores hold), per op: its change's actor id and datatype (rendering)
    std::vector<uint16_t> op_actor;
    std::vector<uint8_t> op_dt;
    uint32_t n_changes = 0, n_ops = 0;
    uint16_t flags = 0;
    uint8_t cls = NO_CLASS;
    uint32_t handle = 0;
    uint32_t hist_len = 0, n_queued = 0;
    // the patch base: the document as the last patch left it
    std::vector<uint8_t> obj_type, obj_emitted;
    std::vector<uint64_t> sig;                               // per register: rendered entry hash, 0 = absent
    std::vector<std::pair<uint32_t, std::vector<uint32_t>>> lists;   // list object -> visible element registers
    // the per-op patch base (op_diffs): the log's op rows, and the document as the last
    // applied op left it — per register its survivors (winner first), per list element its
    // insertion and place in the insertion tree, per list object its reachable elements in
    // document order
    std::vector<hm_op_row> oplog;
    std::vector<uint32_t> op_seq;                            // per op: its change's seq
    std::vector<uint32_t> ch_op0;                            // per change: its first op
    std::vector<std::vector<hm_surv_result>> rs;             // per register
    std::vector<uint32_t> el_op;                             // per register: its ins op, or HM_NONE
    std::vector<uint8_t> el_in;                              // per register: placed in its list's order
    std::vector<uint32_t> el_blk;                            // per register: its ListOrder block (HM_NONE = not placed)
    std::unordered_map<uint32_t, std::vector<uint32_t>> kids;      // parent key -> children, (elem, actor) descending
    std::vector<std::pair<uint32_t, ListOrder>> ord;         // list object -> placed elements in document order
    void setup() {
        bool f;
        objs.get(ROOT_ID, 36, 0, f);
        obj_type.assign(1, HM_MAKE_MAP);
        obj_emitted.assign(1, 1);
        ready = true;
    }
    void crehash(size_t cap) {
        ckey.assign(cap, 0);
        chead.assign(cap, 0);
        const uint64_t m = cap - 1;
        for (uint32_t i = 0; i < cents.size(); i++) {
            uint64_t s = mix64(cents[i].key) & m;
            while (ckey[s] && ckey[s] != cents[i].key + 1) s = (s + 1) & m;
            cents[i].next = ckey[s] ? chead[s] : HM_NONE;
            ckey[s] = cents[i].key + 1;
            chead[s] = i;
        }
    }
    uint32_t content_id(uint64_t key, const H2 &h) {
        if ((cents.size() + 1) * 2 > ckey.size()) crehash(std::max<size_t>(64, ckey.size() * 2));
        const uint64_t m = ckey.size() - 1;
        uint64_t s = mix64(key) & m;
        while (ckey[s] && ckey[s] != key + 1) s = (s + 1) & m;
        uint32_t nx = HM_NONE;
        if (ckey[s]) {
            for (uint32_t i = chead[s]; i != HM_NONE; i = cents[i].next)
                if (cents[i].h == h) return cents[i].cid;
            nx = chead[s];
        }
        cents.push_back({key, h, n_content, nx});
        ckey[s] = key + 1;
        chead[s] = (uint32_t)cents.size() - 1;
        return n_content++;
    }
    std::vector<uint32_t> *list_of(uint32_t obj, bool make) {
        for (auto &l : lists) if (l.first == obj) return &l.second;
        if (!make) return nullptr;
        lists.emplace_back(obj, std::vector<uint32_t>());
        return &lists.back().second;
    }
    ListOrder &order_of(uint32_t obj) {
        for (auto &x : ord) if (x.first == obj) return x.second;
        ord.emplace_back(obj, ListOrder());
        return ord.back().second;
    }
};

// JS string order (UTF-16 code units) of two UTF-8 names
bool js_less(const char *a, uint32_t na, const char *b, uint32_t nb) {
    bool ascii = true;
    for (uint32_t i = 0; i < na && ascii; i++) ascii = (unsigned char)a[i] < 0x80;
    for (uint32_t i = 0; i < nb && ascii; i++) ascii = (unsigned char)b[i] < 0x80;
    if (ascii) {
        const int r = memcmp(a, b, std::min(na, nb));
        return r ? r < 0 : na < nb;
    }
    return u16(std::string(a, na)) < u16(std::string(b, nb));
}

// One document's binary patch: u32 words, f64 numbers, and the strings it names (pointers into
// the document's name tables, local indices).  Words:
//   clock, deps, DocBackend.clock of the log, of this call: each n, then n x (actor string, seq)
//   n_diffs, then per diff a head word (action 0 create | 1 set | 2 remove | 3 insert, type << 3)
//   and: create: obj | set (map): obj key entry | remove (map): obj key | remove (list): obj index
//        insert: obj index elemId entry | set (list): obj index entry
//   entry: n_surv, the winner's value word, then per conflict: actor string, value word
//   value word: vtag | datatype << 3 | payload << 5 (payload: string index for STR / OBJ, number
//   index for INT / FLOAT)
struct BinDoc {
    std::vector<uint32_t> w;
    std::vector<double> nums;
    std::vector<std::pair<const char *, uint32_t>> strs;
    bool exotic = false;                                      // a lone surrogate: the call falls back to JSON
};

// One document's part of a call.
struct Round {
    uint32_t doc = 0, b0 = 0, b1 = 0;
    int32_t status = HM_OK;
    uint32_t err_block = HM_NONE;
    std::vector<hm_change_row> ch;
    std::vector<hm_dep_row> dp;
    std::vector<hm_op_row> op;
    uint16_t n_actors = 0, flags = 0;
    uint32_t n_regs = 0, n_objs = 0;
    std::vector<uint8_t> remap;                              // old rank -> new rank (empty = identity)
    // snapshot for the rollback
    uint32_t s_actors = 0, s_objs = 0, s_regs = 0, s_strs = 0, s_cents = 0, s_content = 0, s_ops = 0;
    std::vector<uint16_t> s_rank_of, s_by_rank;
    bool started = false;                                    // its decode took the snapshot above
    // placement in this call
    uint8_t cls = NO_CLASS;
    uint32_t handle = 0, row = 0;
    bool moved = false, placed = false, fresh = false;       // fresh: handle taken for it in this call
    hm_doc_result res = {};
    const uint32_t *clock = nullptr, *back = nullptr, *heads = nullptr;
    bool full = false;                                       // patch from every register (else the hit ones)
    uint32_t q0 = 0, q1 = 0;                                 // its register requests
    std::string patch, bclock, cclock;
    BinDoc bin;
    uint32_t h0 = 0, h1 = 0, prev_hist = 0;                  // op diffs: its rows of the class's history slices
    std::vector<uint32_t> touched;                           // op diffs: the registers its applied ops hit
};

struct Scratch {
    Ctx cx;
    std::vector<H2> hs;
    std::vector<std::pair<H2, H2>> stk;
    std::string tmp;
    std::vector<uint32_t> t2n;
};

// f(lo, hi, t) over T ranges of [0, n) on host threads.  A worker's exception (out of memory: block
// data comes from peers, brotli output is unbounded) is caught in the worker, every started
// thread is joined, a range whose thread cannot be created runs on this one, and the failure is
// rethrown here as std::bad_alloc (the call returns HM_ERR_NOMEM instead of terminating the process).
template <typename F> void par_for(uint32_t n, uint32_t T, F &&f) {
    T = std::max(1u, std::min(T, n));
    if (T <= 1) { f(0u, n, 0u); return; }
    std::atomic<bool> failed{false};
    auto run = [&f, &failed, n, T](uint32_t t) {
        try { f((uint32_t)((uint64_t)n * t / T), (uint32_t)((uint64_t)n * (t + 1) / T), t); } catch (...) { failed = true; }
    };
    std::vector<std::thread> th;
    try { th.reserve(T); } catch (...) {}
    for (uint32_t t = 0; t < T; t++) {
        try { th.emplace_back(run, t); } catch (...) { run(t); }
    }
    for (auto &x : th) x.join();
    if (failed) throw std::bad_alloc();
}

void rollback(DocSt &d, Round &R) {
    d.actors.truncate(R.s_actors);
    if (!R.s_rank_of.empty() || R.s_actors == 0) { d.rank_of = R.s_rank_of; d.by_rank = R.s_by_rank; }
    d.objs.truncate(R.s_objs);
    d.regs.truncate(R.s_regs);
    d.strs.truncate(R.s_strs);
    if (d.cents.size() > R.s_cents) {
        d.cents.resize(R.s_cents);
        d.crehash(std::max<size_t>(64, d.ckey.size()));
    }
    d.n_content = R.s_content;
    d.op_actor.resize(R.s_ops);
    d.op_dt.resize(R.s_ops);
}

bool unpack(const uint8_t *data, const uint64_t *bo, uint32_t b, Ctx &cx, const char *&s, size_t &len) {
    s = (const char *)data + bo[b];
    len = (size_t)(bo[b + 1] - bo[b]);
    if (len >= 2 && s[0] == 'B' && s[1] == 'R') {
        cx.arena.emplace_back();
        if (!brotli_decompress((const uint8_t *)s + 2, len - 2, cx.arena.back())) return false;
        s = cx.arena.back().data(); len = cx.arena.back().size();
        return true;
    }
    return len >= 2 && s[0] == '{' && s[1] == '"';            // else 'fail to unpack blocks - head is ...'
}

// decode one document's blocks of the call into rows against its interners
void decode_round(DocSt &d, Round &R, const uint8_t *data, const uint64_t *bo, Scratch &X) {
    if (!d.ready) d.setup();
    R.s_actors = d.actors.size(); R.s_objs = d.objs.size(); R.s_regs = d.regs.size(); R.s_strs = d.strs.size();
    R.s_cents = (uint32_t)d.cents.size(); R.s_content = d.n_content; R.s_ops = (uint32_t)d.op_actor.size();
    R.started = true;
    Ctx &cx = X.cx;
    const uint32_t n = R.b1 - R.b0;
    cx.arena.clear();
    cx.cs.assign(n, ScanChange());
    cx.ops.clear();
    cx.deps.clear();
    cx.actors.reset(16);
    X.hs.resize(n);
    auto fail = [&](int32_t st, uint32_t b) { R.status = st; R.err_block = b; };
    for (uint32_t i = 0; i < n; i++) {
        const char *s; size_t len;
        if (!unpack(data, bo, R.b0 + i, cx, s, len)) return fail(HM_ERR_INVALID, i);
        Scan S{s, s + len, &cx};
        cx.cs[i].text = s; cx.cs[i].len = (uint32_t)len;
        if (!S.change(cx.cs[i])) return fail(HM_ERR_INVALID, i);
        CHash C{s, s + len, X.stk, X.tmp};
        if (!C.val(X.hs[i], 0)) return fail(HM_ERR_INVALID, i);
    }
    // actors: the call's names -> the document's actor ids; a new actor re-ranks (JS string order)
    const auto &tk = cx.actors.keys;
    X.t2n.resize(tk.size());
    bool fresh_any = false;
    for (size_t k = 0; k < tk.size(); k++) {
        bool f;
        X.t2n[k] = d.actors.get(tk[k].s.p, tk[k].s.n, 0, f);
        fresh_any |= f;
    }
    const uint32_t na = d.actors.size();
    if (na > MAX_ACTORS) return fail(HM_ERR_UNSUPPORTED, HM_NONE);
    if (fresh_any) {
        R.s_rank_of = d.rank_of; R.s_by_rank = d.by_rank;
        std::vector<uint16_t> order(na);
        for (uint32_t i = 0; i < na; i++) order[i] = (uint16_t)i;
        std::sort(order.begin(), order.end(), [&](uint16_t x, uint16_t y) {
            return js_less(d.actors.ptr(x), d.actors.len(x), d.actors.ptr(y), d.actors.len(y)); });
        std::vector<uint16_t> rank_of(na);
        for (uint32_t r = 0; r < na; r++) rank_of[order[r]] = (uint16_t)r;
        bool ident = true;
        std::vector<uint8_t> remap(R.s_actors);
        for (uint32_t r = 0; r < R.s_actors; r++) {
            remap[r] = (uint8_t)rank_of[d.by_rank[r]];
            ident &= remap[r] == r;
        }
        if (!ident) R.remap = std::move(remap);
        d.rank_of = std::move(rank_of);
        d.by_rank = std::move(order);
    }
    R.n_actors = (uint16_t)na;
    bool f;
    uint32_t last_obj_id = 0;
    SV last_obj{ROOT_ID, 36};
    auto obj = [&](const SV &u) {
        if (u == last_obj) return last_obj_id;
        last_obj_id = d.objs.get(u.p, u.n, 0, f);
        last_obj = u;
        return last_obj_id;
    };
    R.ch.reserve(n); R.dp.reserve(cx.deps.size()); R.op.reserve(cx.ops.size());
    std::string el;
    for (uint32_t i = 0; i < n; i++) {
        const ScanChange &c = cx.cs[i];
        const uint32_t aid = X.t2n[c.actor];
        hm_change_row row = {};
        row.actor = d.rank_of[aid];
        row.seq = (uint32_t)(int64_t)c.seq;
        row.content_id = d.content_id(((uint64_t)aid << 32) | row.seq, X.hs[i]);
        row.dep_off = (uint32_t)R.dp.size();
        for (uint32_t k = 0; k < c.ndeps; k++) {
            const ScanDep &dd = cx.deps[c.dep0 + k];
            hm_dep_row r = {};
            r.actor = d.rank_of[X.t2n[dd.actor]];
            r.seq = (uint32_t)(int64_t)dd.seq;
            R.dp.push_back(r);
        }
        row.n_deps = (uint16_t)c.ndeps;
        row.op_first = (uint32_t)R.op.size();
        for (uint32_t k = 0; k < c.nops; k++) {
            const ScanOp &o = cx.ops[c.op0 + k];
            const int a = o.action;
            if (a < 0 || !o.obj.p) return fail(HM_ERR_INVALID, i);
            hm_op_row r = {};
            r.obj = obj(o.obj);
            r.reg = HM_NONE; r.parent = HM_NONE;
            if (a == HM_INS) {
                if (!o.has_key || !o.has_elem) return fail(HM_ERR_INVALID, i);
                r.elem = (uint32_t)(int64_t)o.elem;
                el.assign(d.actors.ptr(aid), d.actors.len(aid));
                el += ':';
                char nb[40];
                el.append(nb, js_num_text(o.elem, nb));
                r.reg = d.regs.get(el.data(), (uint32_t)el.size(), r.obj, f);
                r.parent = Scan::is(o.key, "_head") ? HM_HEAD : d.regs.get(o.key.p, o.key.n, r.obj, f);
            } else if (a >= HM_SET) {
                if (!o.has_key) return fail(HM_ERR_INVALID, i);
                r.reg = d.regs.get(o.key.p, o.key.n, r.obj, f);
                r.key = d.strs.get(o.key.p, o.key.n, 0, f);
                if (a == HM_LINK) {
                    if (o.vt != J_STR) return fail(HM_ERR_INVALID, i);
                    r.vtag = HM_V_OBJ; r.value = obj(o.sval);
                } else if (a != HM_DEL) {
                    if (!o.has_value || o.vt == J_NULL) r.vtag = HM_V_NULL;
                    else if (o.vt == J_TRUE) r.vtag = HM_V_TRUE;
                    else if (o.vt == J_FALSE) r.vtag = HM_V_FALSE;
                    else if (o.vt == J_NUM) {
                        if (js_int(o.num)) { r.vtag = HM_V_INT; r.value = (uint64_t)(int64_t)o.num; }
                        else { r.vtag = HM_V_FLOAT; memcpy(&r.value, &o.num, 8); }
                    } else if (o.vt == J_STR) { r.vtag = HM_V_STR; r.value = d.strs.get(o.sval.p, o.sval.n, 0, f); }
                    else return fail(HM_ERR_INVALID, i);            // 'unsupported op value'
                }
            }
            r.datatype = o.datatype;
            r.action = (uint8_t)a;
            if (a == HM_MAKE_LIST || a == HM_MAKE_TEXT) R.flags |= HM_DOC_HAS_LISTS;
            if (a == HM_INC || r.datatype == HM_DT_COUNTER) R.flags |= HM_DOC_HAS_COUNTERS;
            R.op.push_back(r);
            d.op_actor.push_back((uint16_t)aid);
            d.op_dt.push_back(r.datatype);
        }
        row.n_ops = c.nops;
        R.ch.push_back(row);
    }
    R.n_regs = d.regs.size();
    R.n_objs = d.objs.size();
}

// ---------------- JSON rendering (what JSON.parse turns back into the JS values) ----------------
void jstr(std::string &o, const char *p, size_t n) {
    static const char *hex = "0123456789abcdef";
    o += '"';
    for (size_t i = 0; i < n; i++) {
        const unsigned char c = (unsigned char)p[i];
        if (c == '"' || c == '\\') { o += '\\'; o += (char)c; }
        else if (c < 0x20) {
            switch (c) {
            case '\b': o += "\\b"; break; case '\f': o += "\\f"; break; case '\n': o += "\\n"; break;
            case '\r': o += "\\r"; break; case '\t': o += "\\t"; break;
            default: o += "\\u00"; o += hex[c >> 4]; o += hex[c & 15];
            }
        } else if (c == 0xED && i + 2 < n && ((unsigned char)p[i + 1] & 0xE0) == 0xA0) {
            // a lone surrogate (kept as its 3-byte form by the decoder): back to \uD8xx / \uDCxx
            const uint32_t u = 0xD000 | (((unsigned char)p[i + 1] & 0x3F) << 6) | ((unsigned char)p[i + 2] & 0x3F);
            o += "\\u";
            for (int s = 12; s >= 0; s -= 4) o += hex[(u >> s) & 15];
            i += 2;
        } else o += (char)c;
    }
    o += '"';
}

void jnum(std::string &o, uint32_t vtag, uint64_t value) {
    char b[48];
    if (vtag == HM_V_INT) { snprintf(b, sizeof b, "%lld", (long long)(int64_t)value); o += b; return; }
    double v;
    memcpy(&v, &value, 8);
    if (v != v) { o += "null"; return; }                       // JSON.stringify(NaN)
    if (v == 1.0 / 0.0) { o += "1e999"; return; }              // JSON.parse -> Infinity
    if (v == -1.0 / 0.0) { o += "-1e999"; return; }
    snprintf(b, sizeof b, "%.17g", v);                         // round-trips to the same double
    o += b;
}

void jvalue(std::string &o, const DocSt &d, const hm_surv_result &s) {
    o += "\"value\":";
    switch (s.vtag) {
    case HM_V_NULL: o += "null"; break;
    case HM_V_FALSE: o += "false"; break;
    case HM_V_TRUE: o += "true"; break;
    case HM_V_INT: case HM_V_FLOAT: jnum(o, s.vtag, s.value); break;
    case HM_V_STR: {
        const uint32_t id = (uint32_t)s.value;
        if (id < d.strs.size()) jstr(o, d.strs.ptr(id), d.strs.len(id)); else o += "null";
        break;
    }
    case HM_V_OBJ: {
        const uint32_t id = (uint32_t)s.value;
        if (id < d.objs.size()) jstr(o, d.objs.ptr(id), d.objs.len(id)); else o += "null";
        o += ",\"link\":true";
        break;
    }
    default: o += "null";
    }
    const uint8_t dt = s.op < d.op_dt.size() ? d.op_dt[s.op] : 0;
    if (dt == HM_DT_COUNTER) o += ",\"datatype\":\"counter\"";
    else if (dt == HM_DT_TIMESTAMP) o += ",\"datatype\":\"timestamp\"";
}

// a register's survivors (winner first) -> the fields of its diff entry:
// value[, link][, datatype][, conflicts: [{actor, value[, link][, datatype]}]]
void jentry(std::string &o, const DocSt &d, const hm_surv_result *sv, uint32_t n) {
    jvalue(o, d, sv[0]);
    if (n <= 1) return;
    o += ",\"conflicts\":[";
    for (uint32_t i = 1; i < n; i++) {
        if (i > 1) o += ',';
        o += "{\"actor\":";
        const uint32_t a = sv[i].op < d.op_actor.size() ? d.op_actor[sv[i].op] : 0;
        jstr(o, d.actors.ptr(a), d.actors.len(a));
        o += ',';
        jvalue(o, d, sv[i]);
        o += '}';
    }
    o += ']';
}

void jclock(std::string &o, const DocSt &d, const uint32_t *row, uint32_t n_actors) {
    o += '{';
    bool first = true;
    for (uint32_t r = 0; r < n_actors; r++) {
        if (!row[r]) continue;
        if (!first) o += ',';
        first = false;
        const uint32_t a = d.by_rank[r];
        jstr(o, d.actors.ptr(a), d.actors.len(a));
        o += ':';
        o += std::to_string(row[r]);
    }
    o += '}';
}

const char *TYPE_NAME[4] = {"map", "table", "list", "text"};

// What the frontend sees of a register's survivors (the winner's value / link / datatype, each
// conflict's actor, value, link, datatype): equal signatures render equal diff entries.
uint64_t entry_sig(const DocSt &d, const hm_surv_result *sv, uint32_t n) {
    if (!n) return 0;
    uint64_t h = 0x9E3779B97F4A7C15ull ^ n;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t op = sv[i].op;
        const uint64_t dt = op < d.op_dt.size() ? d.op_dt[op] : 0;
        const uint64_t act = i && op < d.op_actor.size() ? (uint64_t)d.op_actor[op] + 1 : 0;
        h = mix64(h ^ ((uint64_t)sv[i].vtag | dt << 8 | act << 16));
        h = mix64(h + sv[i].value);
    }
    return h | 1;
}

// Patch writers: JSON text (what JSON.parse turns back into the patch) and a compact binary
// form the Node host turns into the same objects without a JSON parse (HM_DOCSET_BINARY).
struct JsonW {
    std::string &o;
    const DocSt &d;
    bool any = false;
    void sep() { if (any) o += ','; any = true; }
    void clock(const uint32_t *row, uint32_t n_actors) { jclock(o, d, row, n_actors); }
    void head(const char *action, uint8_t t, uint32_t obj) {
        sep();
        o += "{\"action\":\""; o += action; o += "\",\"type\":\""; o += TYPE_NAME[t & 3]; o += "\",\"obj\":";
        jstr(o, d.objs.ptr(obj), d.objs.len(obj));
    }
    void create(uint32_t obj, uint8_t t) {
        sep();
        o += "{\"action\":\"create\",\"obj\":";
        jstr(o, d.objs.ptr(obj), d.objs.len(obj));
        o += ",\"type\":\""; o += TYPE_NAME[t & 3]; o += "\"}";
    }
    void map_set(uint8_t t, uint32_t obj, uint32_t g, const hm_surv_result *sv, uint32_t n) {
        head("set", t, obj);
        o += ",\"key\":"; jstr(o, d.regs.ptr(g), d.regs.len(g)); o += ','; jentry(o, d, sv, n); o += '}';
    }
    void map_remove(uint8_t t, uint32_t obj, uint32_t g) {
        head("remove", t, obj);
        o += ",\"key\":"; jstr(o, d.regs.ptr(g), d.regs.len(g)); o += '}';
    }
    void list_remove(uint8_t t, uint32_t obj, uint32_t i) { head("remove", t, obj); o += ",\"index\":" + std::to_string(i) + '}'; }
    void list_insert(uint8_t t, uint32_t obj, uint32_t i, uint32_t g, const hm_surv_result *sv, uint32_t n) {
        head("insert", t, obj);
        o += ",\"index\":" + std::to_string(i) + ",\"elemId\":";
        jstr(o, d.regs.ptr(g), d.regs.len(g));
        o += ','; jentry(o, d, sv, n); o += '}';
    }
    void list_set(uint8_t t, uint32_t obj, uint32_t i, const hm_surv_result *sv, uint32_t n) {
        head("set", t, obj);
        o += ",\"index\":" + std::to_string(i) + ','; jentry(o, d, sv, n); o += '}';
    }
};

struct StrMap {                                              // (kind, id) -> local string index, per document
    std::vector<uint64_t> key;
    std::vector<uint32_t> val, gen;
    uint32_t g = 0, mask = 0;
    void reset() {
        if (key.empty()) { key.assign(256, 0); val.assign(256, 0); gen.assign(256, 0); mask = 255; }
        if (++g == 0) { std::fill(gen.begin(), gen.end(), 0u); g = 1; }
    }
    void grow() {
        std::vector<uint64_t> k2 = key; std::vector<uint32_t> v2 = val, g2 = gen;
        const size_t cap = key.size() * 2;
        key.assign(cap, 0); val.assign(cap, 0); gen.assign(cap, 0); mask = (uint32_t)cap - 1;
        for (size_t i = 0; i < k2.size(); i++) if (g2[i] == g) {
            uint32_t s = (uint32_t)mix64(k2[i]) & mask;
            while (gen[s] == g) s = (s + 1) & mask;
            key[s] = k2[i]; val[s] = v2[i]; gen[s] = g;
        }
    }
};

struct BinW {
    BinDoc &b;
    const DocSt &d;
    StrMap &m;
    uint32_t n_diffs = 0;
    size_t diffs_at = 0;
    uint32_t str(uint32_t kind, uint32_t id) {
        const uint64_t k = ((uint64_t)kind << 32) | id;
        if ((b.strs.size() + 1) * 2 > m.key.size()) m.grow();
        uint32_t s = (uint32_t)mix64(k) & m.mask;
        while (m.gen[s] == m.g) { if (m.key[s] == k) return m.val[s]; s = (s + 1) & m.mask; }
        const Names &nm = kind == 0 ? d.actors : kind == 1 ? d.objs : kind == 2 ? d.regs : d.strs;
        const char *p = nm.ptr(id);
        const uint32_t n = nm.len(id);
        for (uint32_t i = 0; i + 2 < n; i++) if ((unsigned char)p[i] == 0xED && ((unsigned char)p[i + 1] & 0xE0) == 0xA0) b.exotic = true;
        m.key[s] = k; m.val[s] = (uint32_t)b.strs.size(); m.gen[s] = m.g;
        b.strs.emplace_back(p, n);
        return (uint32_t)b.strs.size() - 1;
    }
    void clock(const uint32_t *row, uint32_t n_actors) {
        const size_t at = b.w.size();
        b.w.push_back(0);
        for (uint32_t r = 0; r < n_actors; r++) {
            if (!row[r]) continue;
            b.w.push_back(str(0, d.by_rank[r]));
            b.w.push_back(row[r]);
            b.w[at]++;
        }
    }
    void begin() { diffs_at = b.w.size(); b.w.push_back(0); }
    void end() { b.w[diffs_at] = n_diffs; }
    void head(uint32_t action, uint8_t t, uint32_t obj) { n_diffs++; b.w.push_back(action | (uint32_t)(t & 3) << 3); b.w.push_back(str(1, obj)); }
    void value(const hm_surv_result &s) {
        const uint8_t dt = s.op < d.op_dt.size() ? d.op_dt[s.op] : 0;
        uint32_t payload = 0;
        switch (s.vtag) {
        case HM_V_INT: payload = (uint32_t)b.nums.size(); b.nums.push_back((double)(int64_t)s.value); break;
        case HM_V_FLOAT: { double v; memcpy(&v, &s.value, 8); payload = (uint32_t)b.nums.size(); b.nums.push_back(v); break; }
        case HM_V_STR: payload = str(3, (uint32_t)s.value); break;
        case HM_V_OBJ: payload = str(1, (uint32_t)s.value); break;
        default: break;
        }
        b.w.push_back((s.vtag & 7) | (uint32_t)(dt & 3) << 3 | payload << 5);
    }
    void entry(const hm_surv_result *sv, uint32_t n) {
        b.w.push_back(n);
        value(sv[0]);
        for (uint32_t i = 1; i < n; i++) {
            b.w.push_back(str(0, sv[i].op < d.op_actor.size() ? d.op_actor[sv[i].op] : 0));
            value(sv[i]);
        }
    }
    void create(uint32_t obj, uint8_t t) { head(0, t, obj); }
    void map_set(uint8_t t, uint32_t obj, uint32_t g, const hm_surv_result *sv, uint32_t n) { head(1, t, obj); b.w.push_back(str(2, g)); entry(sv, n); }
    void map_remove(uint8_t t, uint32_t obj, uint32_t g) { head(2, t, obj); b.w.push_back(str(2, g)); }
    void list_remove(uint8_t t, uint32_t obj, uint32_t i) { head(2, t, obj); b.w.push_back(i); }
    void list_insert(uint8_t t, uint32_t obj, uint32_t i, uint32_t g, const hm_surv_result *sv, uint32_t n) {
        head(3, t, obj); b.w.push_back(i); b.w.push_back(str(2, g)); entry(sv, n);
    }
    void list_set(uint8_t t, uint32_t obj, uint32_t i, const hm_surv_result *sv, uint32_t n) { head(1, t, obj); b.w.push_back(i); entry(sv, n); }
};

// A document's binary patch as the JSON form (the exotic-string fallback: JSON escapes lone
// surrogates, the binary blob cannot carry them through Buffer.toString)
void bin_to_json(const BinDoc &b, std::string &patch, std::string &bclock, std::string &cclock) {
    size_t p = 0;
    const auto &w = b.w;
    auto S = [&](uint32_t i, std::string &o) { jstr(o, b.strs[i].first, b.strs[i].second); };
    auto clock = [&](std::string &o) {
        const uint32_t n = w[p++];
        o += '{';
        for (uint32_t i = 0; i < n; i++) {
            if (i) o += ',';
            S(w[p], o);
            o += ':' + std::to_string(w[p + 1]);
            p += 2;
        }
        o += '}';
    };
    auto value = [&](std::string &o) {
        const uint32_t v = w[p++], tag = v & 7, dt = (v >> 3) & 3, pay = v >> 5;
        o += "\"value\":";
        switch (tag) {
        case HM_V_NULL: o += "null"; break;
        case HM_V_FALSE: o += "false"; break;
        case HM_V_TRUE: o += "true"; break;
        case HM_V_INT: case HM_V_FLOAT: { uint64_t bits; memcpy(&bits, &b.nums[pay], 8); jnum(o, HM_V_FLOAT, bits); break; }
        case HM_V_STR: S(pay, o); break;
        case HM_V_OBJ: S(pay, o); o += ",\"link\":true"; break;
        default: o += "null";
        }
        if (dt == HM_DT_COUNTER) o += ",\"datatype\":\"counter\"";
        else if (dt == HM_DT_TIMESTAMP) o += ",\"datatype\":\"timestamp\"";
    };
    auto entry = [&](std::string &o) {
        const uint32_t n = w[p++];
        value(o);
        if (n <= 1) return;
        o += ",\"conflicts\":[";
        for (uint32_t i = 1; i < n; i++) {
            if (i > 1) o += ',';
            o += "{\"actor\":";
            S(w[p++], o);
            o += ',';
            value(o);
            o += '}';
        }
        o += ']';
    };
    std::string &o = patch;
    o += "{\"clock\":"; clock(o);
    o += ",\"deps\":"; clock(o);
    clock(bclock);
    clock(cclock);
    o += ",\"canUndo\":false,\"canRedo\":false,\"diffs\":[";
    const uint32_t nd = w[p++];
    for (uint32_t k = 0; k < nd; k++) {
        if (k) o += ',';
        const uint32_t hd = w[p++], action = hd & 7, t = (hd >> 3) & 3;
        const bool list = t >= 2;
        static const char *ACT[4] = {"create", "set", "remove", "insert"};
        if (action == 0) {
            o += "{\"action\":\"create\",\"obj\":"; S(w[p++], o);
            o += ",\"type\":\""; o += TYPE_NAME[t]; o += "\"}";
            continue;
        }
        o += "{\"action\":\""; o += ACT[action]; o += "\",\"type\":\""; o += TYPE_NAME[t]; o += "\",\"obj\":";
        S(w[p++], o);
        if (!list) {
            o += ",\"key\":"; S(w[p++], o);
            if (action == 1) { o += ','; entry(o); }
        } else {
            o += ",\"index\":" + std::to_string(w[p++]);
            if (action == 3) { o += ",\"elemId\":"; S(w[p++], o); }
            if (action != 2) { o += ','; entry(o); }
        }
        o += '}';
    }
    o += "]}";
}

// The diffs that take the patch base to the registers' new state (hm_reg_result rows of the
// requested registers, survivors at `surv`): objects created first, then map keys in
// request order, then per list removals (descending old index), insertions (ascending new
// index) and value changes.  The base is advanced to the new state.
template <typename W>
void render_diffs(W &w, DocSt &d, const uint32_t *req, const hm_reg_result *rows, const hm_surv_result *surv, uint32_t n) {
    for (uint32_t ob = 1; ob < d.obj_type.size(); ob++) {
        if (d.obj_type[ob] == NO_TYPE || d.obj_emitted[ob]) continue;
        d.obj_emitted[ob] = 1;
        w.create(ob, d.obj_type[ob]);
    }
    struct LOp { uint32_t g, idx, q; };
    struct LD { uint32_t obj; std::vector<uint32_t> rem; std::vector<LOp> ins, set; };
    std::vector<LD> lds;
    for (uint32_t q = 0; q < n; q++) {
        const uint32_t g = req[q];
        const hm_reg_result &r = rows[q];
        if (r.obj == HM_NONE || r.obj >= d.obj_type.size()) continue;
        const uint8_t t = d.obj_type[r.obj] == NO_TYPE ? HM_MAKE_MAP : d.obj_type[r.obj];
        const bool list = t == HM_MAKE_LIST || t == HM_MAKE_TEXT;
        const uint64_t sg = entry_sig(d, surv + r.surv_off, r.n_surv);
        const uint64_t old = d.sig[g];
        if (!list) {
            if (sg == old) continue;
            d.sig[g] = sg;
            if (sg) w.map_set(t, r.obj, g, surv + r.surv_off, r.n_surv);
            else w.map_remove(t, r.obj, g);
            continue;
        }
        const bool vis = r.n_surv > 0 && r.list_index >= 0;
        const uint64_t ns = vis ? sg : 0;
        if (ns == old) continue;
        LD *L = nullptr;
        for (auto &x : lds) if (x.obj == r.obj) L = &x;
        if (!L) { lds.push_back(LD{r.obj, {}, {}, {}}); L = &lds.back(); }
        std::vector<uint32_t> &el = *d.list_of(r.obj, true);
        if (old && !vis) L->rem.push_back((uint32_t)(std::find(el.begin(), el.end(), g) - el.begin()));
        else (old ? L->set : L->ins).push_back(LOp{g, (uint32_t)r.list_index, q});
        d.sig[g] = ns;
    }
    for (auto &L : lds) {
        std::vector<uint32_t> &el = *d.list_of(L.obj, true);
        const uint8_t t = d.obj_type[L.obj];
        std::sort(L.rem.begin(), L.rem.end(), std::greater<uint32_t>());
        for (uint32_t i : L.rem) {
            if (i >= el.size()) continue;
            el.erase(el.begin() + i);
            w.list_remove(t, L.obj, i);
        }
        std::stable_sort(L.ins.begin(), L.ins.end(), [](const LOp &a, const LOp &b) { return a.idx < b.idx; });
        for (auto &x : L.ins) {
            const uint32_t i = std::min<uint32_t>(x.idx, (uint32_t)el.size());
            el.insert(el.begin() + i, x.g);
            w.list_insert(t, L.obj, i, x.g, surv + rows[x.q].surv_off, rows[x.q].n_surv);
        }
        for (auto &x : L.set) {
            const uint32_t i = (uint32_t)(std::find(el.begin(), el.end(), x.g) - el.begin());
            w.list_set(t, L.obj, i, surv + rows[x.q].surv_off, rows[x.q].n_surv);
        }
    }
}

// ---------------- per-op diffs (Automerge makePatch) ----------------
// Automerge collects one diff per applied op, in application order: `create` per make op,
// per map assign the key's state after it (`set` with the winner and its conflicts, or
// `remove`), per list-element assign `insert` / `set` / `remove` at the element's index at
// that moment, nothing for `ins` (oracle/js/backend.js:92-170 restates the same sequence).
// The GPU fixes what was applied and in which order (the round's history slice, with every
// applied change's allDeps row: hm_store_read_history); the renderer walks those changes' ops
// over the patch base — per register the survivors the previous op left, per list the
// insertion tree and document order of the placed elements — applying exactly
// applyAssign's filter (isConcurrent reduces to allDeps(new)[x.actor] < x.seq: nothing
// resident depends on the new op), inc's counter sums and the sortBy(actor).reverse(), and
// RGA placement ((elem, actor) descending siblings, pre-order), to know each op's diff.  The
// registers it ends on are compared with the device's merged registers afterwards.
// (For map / table registers and counters the same rows come from the device without a replay:
// hm_store_op_diffs, which hm_docset_materialize_patch renders, with HM_ODF_LISTS the list / text
// element diffs too; the rounds of hm_docset_apply go through this replay unless the docset was
// created with HM_DOCSET_DEVICE_DIFFS, which renders them from those rows: Call::read_diffs.)
struct Replay {
    DocSt &d;
    uint32_t S;
    static uint32_t pkey(const hm_op_row &o) { return o.parent == HM_HEAD ? (0x80000000u | o.obj) : o.parent; }
    static uint32_t find(const std::vector<uint32_t> &v, uint32_t x) {
        return (uint32_t)(std::find(v.begin(), v.end(), x) - v.begin());
    }
    uint32_t rank(uint32_t op) const { return d.rank_of[d.op_actor[op]]; }
    // lamportCompare (elem, actor) of two element registers: a after b in sibling order?
    bool sib_before(uint32_t a, uint32_t b) const {
        const uint32_t oa = d.el_op[a], ob = d.el_op[b];
        if (d.oplog[oa].elem != d.oplog[ob].elem) return d.oplog[oa].elem > d.oplog[ob].elem;
        return rank(oa) > rank(ob);
    }
    // applyInsert: the element joins its parent's children; once its chain reaches _head it
    // (and any subtree inserted under it earlier) takes its pre-order place
    void insert(uint32_t k) {
        const hm_op_row &o = d.oplog[k];
        const uint32_t e = o.reg;
        d.el_op[e] = k;
        std::vector<uint32_t> &sib = d.kids[pkey(o)];
        uint32_t i = 0;
        while (i < sib.size() && sib_before(sib[i], e)) i++;
        sib.insert(sib.begin() + i, e);
        if (o.parent != HM_HEAD && !(o.parent < d.el_in.size() && d.el_in[o.parent])) return;
        ListOrder &ov = d.order_of(o.obj);
        uint32_t pos;
        if (i == 0) pos = o.parent == HM_HEAD ? 0u : ov.pos_of(o.parent, d.el_blk) + 1;
        else if (i + 1 < sib.size()) pos = ov.pos_of(sib[i + 1], d.el_blk);
        else {                                               // after the parent's subtree
            pos = ov.size();
            for (uint32_t x = o.parent; x != HM_HEAD;) {
                const hm_op_row &xo = d.oplog[d.el_op[x]];
                const std::vector<uint32_t> &xs = d.kids[pkey(xo)];
                const uint32_t j = find(xs, x);
                if (j + 1 < xs.size()) { pos = ov.pos_of(xs[j + 1], d.el_blk); break; }
                x = xo.parent;
            }
        }
        std::vector<uint32_t> sub, stk{e};
        while (!stk.empty()) {
            const uint32_t x = stk.back();
            stk.pop_back();
            sub.push_back(x);
            d.el_in[x] = 1;
            auto it = d.kids.find(x);
            if (it != d.kids.end())
                for (size_t c = it->second.size(); c-- > 0;) stk.push_back(it->second[c]);
        }
        ov.insert_at(pos, sub, d.el_blk, [&](uint32_t x) { return !d.rs[x].empty(); });
    }
    uint32_t visible_before(uint32_t obj, uint32_t e) {
        return d.order_of(obj).vis_before(e, d.el_blk, [&](uint32_t x) { return !d.rs[x].empty(); });
    }
    static bool numeric(uint32_t vt) { return vt == HM_V_INT || vt == HM_V_FLOAT; }
    static double num(uint32_t vt, uint64_t v) {
        if (vt == HM_V_INT) return (double)(int64_t)v;
        double x;
        memcpy(&x, &v, 8);
        return x;
    }
    // applyAssign (A.2) of op k of a change whose allDeps row is ad
    template <typename W>
    void assign(W &w, uint32_t k, const uint32_t *ad) {
        const hm_op_row &o = d.oplog[k];
        std::vector<hm_surv_result> &sv = d.rs[o.reg];
        const bool was = !sv.empty();
        auto concurrent = [&](const hm_surv_result &x) {
            const uint32_t r = rank(x.op);
            return (r < S ? ad[r] : 0u) < d.op_seq[x.op];
        };
        if (o.action == HM_INC) {
            for (hm_surv_result &x : sv) {
                if (d.oplog[x.op].datatype != HM_DT_COUNTER || !numeric(x.vtag) || concurrent(x)) continue;
                if (x.vtag == HM_V_INT && o.vtag == HM_V_INT) x.value = (uint64_t)((int64_t)x.value + (int64_t)o.value);
                else {
                    const double r = num(x.vtag, x.value) + num(o.vtag, o.value);
                    memcpy(&x.value, &r, 8);
                    x.vtag = HM_V_FLOAT;
                }
            }
        } else {
            sv.erase(std::remove_if(sv.begin(), sv.end(), [&](const hm_surv_result &x) { return !concurrent(x); }), sv.end());
        }
        if (o.action == HM_SET || o.action == HM_LINK) {
            hm_surv_result y;
            y.op = k; y.vtag = o.vtag; y.value = o.value;
            sv.push_back(y);
        }
        // sortBy(actor).reverse() = reversed, then a stable sort by actor descending (insertion
        // sort: a register holds a handful of survivors)
        std::reverse(sv.begin(), sv.end());
        for (size_t i = 1; i < sv.size(); i++) {
            const hm_surv_result x = sv[i];
            const uint32_t rx = rank(x.op);
            size_t j = i;
            for (; j > 0 && rank(sv[j - 1].op) < rx; j--) sv[j] = sv[j - 1];
            sv[j] = x;
        }
        const uint8_t t = o.obj < d.obj_type.size() && d.obj_type[o.obj] != NO_TYPE ? d.obj_type[o.obj] : (uint8_t)HM_MAKE_MAP;
        if (was != !sv.empty() && o.reg < d.el_in.size() && d.el_in[o.reg])   // a placed element's visibility
            d.order_of(o.obj).vis_change(o.reg, d.el_blk, !sv.empty());
        if (t != HM_MAKE_LIST && t != HM_MAKE_TEXT) {
            if (sv.empty()) w.map_remove(t, o.obj, o.reg);
            else w.map_set(t, o.obj, o.reg, sv.data(), (uint32_t)sv.size());
            return;
        }
        // updateListElement
        if (was) {
            const uint32_t i = visible_before(o.obj, o.reg);
            if (sv.empty()) w.list_remove(t, o.obj, i);
            else w.list_set(t, o.obj, i, sv.data(), (uint32_t)sv.size());
        } else if (!sv.empty() && o.reg < d.el_in.size() && d.el_in[o.reg]) {
            w.list_insert(t, o.obj, visible_before(o.obj, o.reg), o.reg, sv.data(), (uint32_t)sv.size());
        }
    }
    // the round: n applied changes (log indices, application order) with their allDeps rows
    template <typename W>
    void round(W &w, const uint32_t *log, const uint32_t *ads, uint32_t n, std::vector<uint32_t> &touched) {
        for (uint32_t r = 0; r < n; r++) {
            const uint32_t ci = log[r];
            const uint32_t k0 = d.ch_op0[ci], k1 = ci + 1 < d.ch_op0.size() ? d.ch_op0[ci + 1] : (uint32_t)d.oplog.size();
            for (uint32_t k = k0; k < k1; k++) {
                const hm_op_row &o = d.oplog[k];
                if (o.action <= HM_MAKE_TEXT) { w.create(o.obj, o.action); continue; }
                if (o.action == HM_INS) { insert(k); continue; }
                if (o.reg == HM_NONE || o.reg >= d.rs.size()) continue;
                assign(w, k, ads + (size_t)r * S);
                touched.push_back(o.reg);
            }
        }
        std::sort(touched.begin(), touched.end());
        touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
    }
};

// a replayed register against the device's merged register (numbers compared by value)
bool same_register(const DocSt &d, uint32_t g, const hm_reg_result &r, const hm_surv_result *sv) {
    const std::vector<hm_surv_result> &h = d.rs[g];
    if (h.size() != r.n_surv) return false;
    for (uint32_t i = 0; i < r.n_surv; i++) {
        const hm_surv_result &a = h[i], &b = sv[r.surv_off + i];
        if (a.op != b.op) return false;
        if (Replay::numeric(a.vtag) && Replay::numeric(b.vtag)) {
            if (Replay::num(a.vtag, a.value) != Replay::num(b.vtag, b.value)) return false;
        } else if (a.vtag != b.vtag || a.value != b.value) return false;
    }
    return true;
}

// One request's op-diff rows (hm_store_op_diffs_ex: rows[first .. first + n), their index table and
// the call's survivors) into a patch writer, in the rows' order: what hm_docset_materialize_patch and
// the rounds of a HM_DOCSET_DEVICE_DIFFS docset render.  Reads the document's log rows, object types
// and names; returns NULL, or what is wrong with a row (nothing is written for that row or after it).
template <typename W>
const char *render_op_rows(W &w, const DocSt &d, const hm_op_diff *rows, const uint32_t *index, const hm_surv_result *surv,
                           uint32_t first, uint32_t n) {
    for (uint32_t x = first; x < first + n; x++) {
        const hm_op_diff &r = rows[x];
        if (r.op >= d.oplog.size()) return "an op diff outside the document's log";
        const hm_op_row &op = d.oplog[r.op];
        if (op.obj >= d.obj_type.size()) return "an op diff on an unknown object";
        if (r.kind == HM_OD_CREATE) { w.create(op.obj, op.action); continue; }
        if (op.reg >= d.regs.size()) return "an op diff on an unknown register";
        const uint8_t t = d.obj_type[op.obj] != NO_TYPE ? d.obj_type[op.obj] : (uint8_t)HM_MAKE_MAP;
        if (r.kind == HM_OD_SET) w.map_set(t, op.obj, op.reg, surv + r.surv_off, r.n_surv);
        else if (r.kind == HM_OD_REMOVE) w.map_remove(t, op.obj, op.reg);
        else if (r.kind == HM_OD_ELEM_INSERT) w.list_insert(t, op.obj, index[x], op.reg, surv + r.surv_off, r.n_surv);
        else if (r.kind == HM_OD_ELEM_SET) w.list_set(t, op.obj, index[x], surv + r.surv_off, r.n_surv);
        else if (r.kind == HM_OD_ELEM_REMOVE) w.list_remove(t, op.obj, index[x]);
        else return "an op diff of an unknown kind";
    }
    return nullptr;
}

// the document as the patch base holds it: {uuid: {type, keys: [[key, entry]], elems: [[elemId, entry]]}}
// (created: per object, 1 = it exists in the rendered state; NULL = every object the document knows)
void render_view(std::string &o, const DocSt &d, const hm_reg_result *rows, const hm_surv_result *surv, uint32_t n_regs,
                 const uint8_t *created = nullptr) {
    std::vector<std::string> keys(d.obj_type.size()), elems(d.obj_type.size());
    std::vector<std::vector<std::pair<int32_t, uint32_t>>> order(d.obj_type.size());
    std::string tmp;
    for (uint32_t g = 0; g < n_regs; g++) {
        const hm_reg_result &r = rows[g];
        if (!r.n_surv || r.obj == HM_NONE || r.obj >= d.obj_type.size()) continue;
        const uint8_t t = d.obj_type[r.obj] == NO_TYPE ? HM_MAKE_MAP : d.obj_type[r.obj];
        if (t == HM_MAKE_LIST || t == HM_MAKE_TEXT) { if (r.list_index >= 0) order[r.obj].push_back({r.list_index, g}); continue; }
        std::string &k = keys[r.obj];
        if (!k.empty()) k += ',';
        k += '[';
        jstr(k, d.regs.ptr(g), d.regs.len(g));
        k += ",{";
        jentry(k, d, surv + r.surv_off, r.n_surv);
        k += "}]";
    }
    o += '{';
    const size_t start = o.size();
    for (uint32_t ob = 0; ob < d.obj_type.size(); ob++) {
        if (d.obj_type[ob] == NO_TYPE && keys[ob].empty() && order[ob].empty()) continue;
        if (created && !created[ob]) continue;
        if (o.size() > start) o += ',';
        jstr(o, d.objs.ptr(ob), d.objs.len(ob));
        const uint8_t t = d.obj_type[ob] == NO_TYPE ? HM_MAKE_MAP : d.obj_type[ob];
        o += ":{\"type\":\""; o += TYPE_NAME[t & 3]; o += "\",\"keys\":[";
        o += keys[ob];
        o += "],\"elems\":[";
        std::sort(order[ob].begin(), order[ob].end());
        for (size_t i = 0; i < order[ob].size(); i++) {
            const uint32_t g = order[ob][i].second;
            if (i) o += ',';
            o += '[';
            jstr(o, d.regs.ptr(g), d.regs.len(g));
            o += ",{";
            jentry(o, d, surv + rows[g].surv_off, rows[g].n_surv);
            o += "}]";
        }
        o += "]}";
    }
    o += '}';
}

}  // namespace

struct hm_docset {
    hm_engine *e = nullptr;
    uint32_t threads = 16;
    bool patches = true;
    bool binary = false;                                     // HM_DOCSET_BINARY results
    bool op_diffs = true;                                    // Automerge's per-op diff sequence (else HM_DOCSET_NET_DIFFS)
    bool device_diffs = false;                               // HM_DOCSET_DEVICE_DIFFS: the sequence from the device's op-diff rows
    uint64_t dstat[4] = {0, 0, 0, 0};                        // device diffs: rounds rendered, store calls, calls repeated, 0
    double surv_per_row = 2.0;                               // device diffs: survivors guessed per row (grows with what the calls report)
    hm_store *stores[N_CLASS] = {};
    std::vector<uint32_t> free_h[N_CLASS];                   // released handles (empty documents), reused first
    uint32_t opened[N_CLASS] = {};                           // handles opened per store
    // documents: fixed chunks, so hm_docset_open may run while a call works on earlier documents
    static constexpr uint32_t CHUNK = 4096;
    std::vector<std::unique_ptr<DocSt[]>> chunks;
    std::atomic<uint32_t> n_docs{0};
    std::mutex open_mu;
    std::atomic<bool> busy{false};
    bool broken = false;                                     // a failed call could not be undone on a store
    uint64_t routing[3] = {0, 0, 0};                         // document rounds: incremental, re-merged, handed back
    uint64_t stat[8] = {0, 0, 0, 0, 0, 0, 0, 0};           // rounds, docs, restrides, hit-register patches, full patches,
                                                             // per-op patches, replay mismatches, replay checks skipped
    uint64_t mstat[2] = {0, 0};                              // merge requests: device route, host route
    DocSt &doc(uint32_t i) { return chunks[i / CHUNK][i % CHUNK]; }
};

struct hm_text {
    std::string s;
    std::vector<hm_doc_result> res;
};

namespace {

int store_of(hm_docset *ds, uint32_t c, hm_store **out) {
    if (!ds->stores[c]) {
        hm_store_config sc = {STRIDES[c], 0};
        const int r = hm_store_create(ds->e, &sc, &ds->stores[c]);
        if (r) return r;
    }
    *out = ds->stores[c];
    return HM_OK;
}

uint8_t class_for(uint32_t n_actors) {
    for (uint32_t c = 0; c < N_CLASS; c++) if (n_actors <= STRIDES[c]) return (uint8_t)c;
    return NO_CLASS;
}

struct Busy {
    hm_docset *ds;
    bool ok;
    explicit Busy(hm_docset *d) : ds(d) { bool f = false; ok = ds->busy.compare_exchange_strong(f, true); }
    ~Busy() { if (ok) ds->busy.store(false); }
};

// what one class's batch of a call left behind
struct ClsOut {
    std::vector<hm_doc_result> res;
    std::vector<uint32_t> clock, back, heads;
    uint64_t id = 0;
    bool sub = false, done = false;                          // submitted / waited (applied on the device)
};

// this call's changes alone (updateClock(changes))
void round_clock(const Round &x, uint32_t *rc) {
    for (uint32_t a = 0; a < HM_MAX_STRIDE; a++) rc[a] = 0;
    for (const hm_change_row &c : x.ch) if (c.actor < HM_MAX_STRIDE && c.seq > rc[c.actor]) rc[c.actor] = c.seq;
}

// One hm_docset_apply call: what the call holds, and one member function per phase.  apply()
// below runs the phases in order.  All-or-nothing: until commit() a document's host state has
// changed only in what rollback() (past the round's snapshot, Round::s_*) and fail() take back,
// and every applied batch can be undone; from commit() on nothing fails the call.
struct Call {
    hm_docset *ds;
    const uint8_t *data;
    const uint64_t *bo;
    const uint32_t *doc_block, *docs;
    const uint32_t n;
    std::vector<Round> R;
    uint32_t T = 1;                                          // host threads of the decode and the commit
    std::vector<uint32_t> by_cls[N_CLASS];                   // per class: its rounds of the call (indices into R)
    ClsOut co[N_CLASS];
    uint64_t call_routing[3] = {0, 0, 0};                    // this call's routing (ds->routing once it commits)
    // released handles (a moved document's old one, a fresh one its document does not keep) go
    // back to their store as empty documents (hm_doc_reset) and are reused by later calls; their
    // rows are reclaimed when the store compacts
    std::vector<uint32_t> rel[N_CLASS];
    // net diffs: the register requests per class (document handle, register), their rows and survivors
    std::vector<uint32_t> qdocs[N_CLASS], qregs[N_CLASS];
    uint32_t cap[N_CLASS] = {};
    std::vector<hm_reg_result> rrows[N_CLASS];
    std::vector<hm_surv_result> rsurv[N_CLASS];
    // op diffs: the rounds that read their history slice, per class, and the slices (applied
    // changes in application order, their allDeps rows)
    std::vector<uint32_t> hreq[N_CLASS], hlog[N_CLASS], had[N_CLASS];
    // device diffs (HM_DOCSET_DEVICE_DIFFS): per class the op-diff rows of its rounds' slices, their
    // survivors, index table and (block, rows) per request; Round::h0 = the round's request
    std::vector<hm_op_diff> drows[N_CLASS];
    std::vector<hm_surv_result> dsurv[N_CLASS];
    std::vector<uint32_t> dindex[N_CLASS], drange[N_CLASS];
    uint64_t call_dstat[3] = {0, 0, 0};                      // (ds->dstat once the call commits)
    bool exotic = false;                                     // a binary call that falls back to JSON
    // fault injection for the tests (HM_DOCSET_INJECT_FAIL=wait:<k> fails the call after the k-th
    // class's batch is applied, =read after every class's; the call must then be undone everywhere)
    const char *inj = getenv("HM_DOCSET_INJECT_FAIL");
    const int inj_wait = inj && !strncmp(inj, "wait:", 5) ? atoi(inj + 5) : -1;
    const bool inj_read = inj && !strcmp(inj, "read");
    int n_waited = 0;
    const bool prof = getenv("HM_DOCSET_PROFILE") != nullptr;    // a line per mark()
    std::chrono::steady_clock::time_point t0;
    void mark(const char *what) {
        if (!prof) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[hm_docset] %-14s %9.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t0).count());
        t0 = t;
    }
    int validate() {
        const uint32_t nd = ds->n_docs.load();
        std::vector<uint8_t> seen(nd, 0);
        for (uint32_t i = 0; i < n; i++) {
            if (docs[i] >= nd || seen[docs[i]]) return hm_engine_fail(ds->e, HM_ERR_INVALID, "bad or repeated docset document");
            seen[docs[i]] = 1;
            if (doc_block[i] > doc_block[i + 1]) return hm_engine_fail(ds->e, HM_ERR_INVALID, "doc_block not ascending");
        }
        t0 = std::chrono::steady_clock::now();               // (the profile clock starts at the decode)
        return HM_OK;
    }
    // every document's blocks -> rows, on host threads; a document whose blocks do not decode goes
    // back at once (its round keeps the status)
    void decode() {
        R.resize(n);
        for (uint32_t i = 0; i < n; i++) { R[i].doc = docs[i]; R[i].b0 = doc_block[i]; R[i].b1 = doc_block[i + 1]; }
        T = std::min<uint32_t>(ds->threads, std::max<uint32_t>(1, n / 64));
        try {
            par_for(n, T, [&](uint32_t lo, uint32_t hi, uint32_t) {
                Scratch X;
                for (uint32_t i = lo; i < hi; i++) {
                    DocSt &d = ds->doc(R[i].doc);
                    decode_round(d, R[i], data, bo, X);
                    if (R[i].status != HM_OK) { rollback(d, R[i]); R[i].started = false; }
                }
            });
        } catch (...) {
            // a decode ran out of memory: every document whose decode started goes back
            for (uint32_t i = 0; i < n; i++) if (R[i].started) rollback(ds->doc(R[i].doc), R[i]);
            throw;
        }
    }
    // placement: a document lives in the narrowest class that holds its actors
    void place() {
        for (uint32_t i = 0; i < n; i++) if (R[i].status == HM_OK) place_round(i);
    }
    void place_round(uint32_t i) {
        Round &x = R[i];
        DocSt &d = ds->doc(x.doc);
        uint8_t c = class_for(x.n_actors);
        if (d.cls != NO_CLASS && d.cls > c) c = d.cls;
        x.cls = c;
        x.placed = d.cls == NO_CLASS;
        x.moved = !x.placed && c != d.cls;
        x.handle = d.handle;
        by_cls[c].push_back(i);
    }
    // `fresh` handles of class c for its placed and moved documents: released ones first, then new ones
    int take_handles(uint32_t c, hm_store *st, uint32_t fresh, std::vector<uint32_t> &fh) {
        std::vector<uint32_t> &fl = ds->free_h[c];
        const size_t k = std::min<size_t>(fresh, fl.size());
        fh.assign(fl.end() - k, fl.end());
        fl.resize(fl.size() - k);
        uint32_t h0 = 0;
        int rc;
        if (fresh > k && (rc = hm_doc_open_n(st, fresh - (uint32_t)k, &h0))) { fl.insert(fl.end(), fh.begin(), fh.end()); return rc; }
        ds->opened[c] += fresh - (uint32_t)k;
        for (uint32_t j = 0; j < fresh - k; j++) fh.push_back(h0 + j);
        return HM_OK;
    }
    // a moved document's whole log: its rows from the old store, ranks re-mapped to this round's,
    // appended to the new class's batch
    int moved_log(const Round &x, const DocSt &d, std::vector<hm_change_row> &ch, std::vector<hm_dep_row> &dp,
                  std::vector<hm_op_row> &op) {
        const uint32_t d0 = (uint32_t)dp.size(), o0 = (uint32_t)op.size();
        ds->stat[2]++;
        hm_doc_info_t inf;
        hm_store *old = ds->stores[d.cls];
        int rc = hm_doc_info(old, d.handle, &inf);
        if (rc) return rc;
        std::vector<hm_change_row> lc(inf.n_changes);
        std::vector<hm_dep_row> ld(inf.n_deps);
        std::vector<hm_op_row> lo(inf.n_ops);
        if ((rc = hm_doc_log(old, d.handle, lc.data(), ld.data(), lo.data()))) return rc;
        for (auto &cr : lc) {
            if (!x.remap.empty() && cr.actor < x.remap.size()) cr.actor = x.remap[cr.actor];
            cr.dep_off += d0; cr.op_first += o0;
            ch.push_back(cr);
        }
        for (auto &dr : ld) { if (!x.remap.empty() && dr.actor < x.remap.size()) dr.actor = x.remap[dr.actor]; dp.push_back(dr); }
        op.insert(op.end(), lo.begin(), lo.end());
        return HM_OK;
    }
    // class c's documents of the call as one batch: handles, build, submit, wait.  A status other
    // than HM_OK fails the call (fail()): co[c].sub / .done say how far the batch got.
    int merge_class(uint32_t c) {
        auto &rows = by_cls[c];
        hm_store *st;
        int rc = store_of(ds, c, &st);
        if (rc) return rc;
        const uint32_t S = STRIDES[c];
        uint32_t fresh = 0;
        for (uint32_t i : rows) fresh += R[i].placed || R[i].moved;
        std::vector<uint32_t> fh;
        size_t next_fh = 0;
        if ((rc = take_handles(c, st, fresh, fh))) return rc;
        std::vector<hm_doc_row> drows(rows.size());
        std::vector<hm_change_row> ch;
        std::vector<hm_dep_row> dp;
        std::vector<hm_op_row> op;
        std::vector<uint32_t> hand(rows.size());
        std::vector<uint8_t> remap;
        bool any_remap = false;
        for (uint32_t k = 0; k < rows.size(); k++) if (!R[rows[k]].moved && !R[rows[k]].placed && !R[rows[k]].remap.empty()) any_remap = true;
        if (any_remap) {
            remap.resize(rows.size() * (size_t)S);
            for (uint32_t k = 0; k < rows.size(); k++) for (uint32_t a = 0; a < S; a++) remap[(size_t)k * S + a] = (uint8_t)a;
        }
        size_t tc = 0, td = 0, to = 0;
        for (uint32_t i : rows) { tc += R[i].ch.size(); td += R[i].dp.size(); to += R[i].op.size(); }
        ch.reserve(tc); dp.reserve(td); op.reserve(to);
        for (uint32_t k = 0; k < rows.size(); k++) {
            Round &x = R[rows[k]];
            DocSt &d = ds->doc(x.doc);
            x.row = k;
            hm_doc_row &r = drows[k];
            r = hm_doc_row{};
            r.change_off = (uint32_t)ch.size(); r.dep_off = (uint32_t)dp.size(); r.op_off = (uint32_t)op.size();
            const uint32_t c0 = (uint32_t)ch.size(), d0 = (uint32_t)dp.size(), o0 = (uint32_t)op.size();
            if (x.placed || x.moved) { x.handle = fh[next_fh++]; x.fresh = true; }
            hand[k] = x.handle;
            if (x.moved) {
                if ((rc = moved_log(x, d, ch, dp, op))) break;
            } else if (!x.placed && !x.remap.empty()) {
                for (size_t a = 0; a < x.remap.size(); a++) remap[(size_t)k * S + a] = x.remap[a];
            }
            const uint32_t d1 = (uint32_t)dp.size(), o1 = (uint32_t)op.size();
            for (auto cr : x.ch) { cr.dep_off += d1; cr.op_first += o1; ch.push_back(cr); }
            dp.insert(dp.end(), x.dp.begin(), x.dp.end());
            op.insert(op.end(), x.op.begin(), x.op.end());
            r.n_changes = (uint32_t)ch.size() - c0; r.n_deps = (uint32_t)dp.size() - d0; r.n_ops = (uint32_t)op.size() - o0;
            r.n_regs = x.n_regs; r.n_objs = x.n_objs; r.n_actors = x.n_actors;
            r.flags = (uint16_t)(x.flags | (x.moved ? d.flags : 0));
        }
        // handles taken but not handed to a document (a failed log read) are still empty
        ds->free_h[c].insert(ds->free_h[c].end(), fh.begin() + next_fh, fh.end());
        if (rc) return rc;
        hm_batch b = {};
        b.n_docs = (uint32_t)rows.size(); b.n_changes = (uint32_t)ch.size(); b.n_deps = (uint32_t)dp.size(); b.n_ops = (uint32_t)op.size();
        b.a_stride = S;
        b.docs = drows.data(); b.changes = ch.data(); b.deps = dp.data(); b.ops = op.data();
        ClsOut &O = co[c];
        if ((rc = hm_batch_submit(st, &b, hand.data(), any_remap ? remap.data() : nullptr, &O.id))) return rc;
        O.sub = true;
        if ((rc = wait_class(c, (uint32_t)rows.size()))) return rc;
        if (n_waited++ == inj_wait) return hm_engine_fail(ds->e, HM_ERR_DEVICE, "injected failure (HM_DOCSET_INJECT_FAIL)");
        for (uint32_t k = 0; k < rows.size(); k++) point_round(R[rows[k]], c, k);
        return HM_OK;
    }
    // class c's submitted batch of m rounds, waited for: its result rows, the call's routing
    int wait_class(uint32_t c, uint32_t m) {
        ClsOut &O = co[c];
        hm_store *st = ds->stores[c];
        const size_t S = STRIDES[c];
        O.res.resize(m); O.clock.resize(m * S); O.back.resize(m * S); O.heads.resize(m * S);
        const int rc = hm_batch_wait(st, O.id, O.res.data(), O.clock.data(), O.back.data(), O.heads.data());
        if (rc) return rc;
        O.sub = false; O.done = true;
        uint32_t r3[3] = {0, 0, 0};
        if (hm_store_last_routing(st, r3) == HM_OK)
            for (int k = 0; k < 3; k++) call_routing[k] += r3[k];         // (counted once the call commits)
        return HM_OK;
    }
    // round x reads row j of class c's results
    void point_round(Round &x, uint32_t c, uint32_t j) {
        const ClsOut &O = co[c];
        const size_t at = (size_t)j * STRIDES[c];
        x.res = O.res[j];
        x.clock = O.clock.data() + at; x.back = O.back.data() + at; x.heads = O.heads.data() + at;
    }
    // Class c's gathered batch in flight (a fork's, a merge's) as its rounds' rows, then the wait.  What a
    // decode would have handed each round: the gathered change rows and the op map come back; the op rows
    // through the map from the source's own host copy of its log where the docset keeps one (the per-op
    // patch modes), from the device otherwise; the per-op tables through the map.  Dep rows are not needed.
    // The hook says what differs: source(i), the document request i gathered from; rename / actor, host op
    // rows and an op's actor id into the round's id spaces (false / HM_NONE: outside them); rest, what else
    // the round's document takes over; PARALLEL, rows on host threads (else in row order, ending at the
    // first bad one); the error texts.
    template <typename H> int take_gathered(uint32_t c, const H &h) {
        const std::vector<uint32_t> &rows = by_cls[c];
        const bool host_ops = ds->patches && ds->op_diffs;
        std::vector<hm_doc_row> gd;
        std::vector<hm_change_row> gc;
        std::vector<hm_op_row> go;
        std::vector<uint32_t> gl;
        int rc = hm_store_fork_rows(ds->stores[c], co[c].id, gd, gc, host_ops ? nullptr : &go, gl);
        if (rc || (rc = wait_class(c, (uint32_t)rows.size()))) return rc;
        auto row = [&](uint32_t j) -> const char * {             // (what is wrong with row j, or nullptr)
            const uint32_t i = rows[j];
            Round &x = R[i];
            DocSt &d = ds->doc(x.doc);
            const DocSt &p = h.source(i);
            const hm_doc_row &r = gd[j];
            if ((uint64_t)r.change_off + r.n_changes > gc.size() || (uint64_t)r.op_off + r.n_ops > gl.size() ||
                (!host_ops && (uint64_t)r.op_off + r.n_ops > go.size()))
                return H::BAD_ROWS;
            x.ch.assign(gc.begin() + r.change_off, gc.begin() + r.change_off + r.n_changes);
            for (hm_change_row &cr : x.ch) { cr.dep_off -= r.dep_off; cr.op_first -= r.op_off; }
            const uint32_t *log = gl.data() + r.op_off;
            if (!host_ops) x.op.assign(go.begin() + r.op_off, go.begin() + r.op_off + r.n_ops);
            else {
                x.op.resize(r.n_ops);
                for (uint32_t q = 0; q < r.n_ops; q++) { if (log[q] >= p.oplog.size()) return H::BAD_OPS; x.op[q] = p.oplog[log[q]]; }
                if (!h.rename(i, x.op)) return H::BAD_IDS;
            }
            if (d.op_actor.empty()) { d.op_actor.reserve(r.n_ops); d.op_dt.reserve(r.n_ops); }
            for (uint32_t q = 0; q < r.n_ops; q++) {
                const uint32_t a = log[q] < p.op_actor.size() && log[q] < p.op_dt.size() ? h.actor(i, p.op_actor[log[q]]) : HM_NONE;
                if (a == HM_NONE) return H::BAD_OPS;
                d.op_actor.push_back((uint16_t)a); d.op_dt.push_back(p.op_dt[log[q]]);
            }
            h.rest(i, x, d);
            point_round(x, c, j);
            return nullptr;
        };
        std::atomic<const char *> bad{nullptr};
        try {
            par_for((uint32_t)rows.size(), H::PARALLEL ? T : 1u, [&](uint32_t lo, uint32_t hi, uint32_t) {
                for (uint32_t j = lo; j < hi && !bad; j++)
                    if (const char *w = row(j)) bad = w;
            });
        } catch (...) { return hm_engine_fail(ds->e, HM_ERR_NOMEM, H::NOMEM); }
        return bad ? hm_engine_fail(ds->e, HM_ERR_DEVICE, bad) : HM_OK;
    }
    void release() {
        for (uint32_t c = 0; c < N_CLASS; c++) {
            if (rel[c].empty()) continue;
            if (hm_doc_reset(ds->stores[c], rel[c].data(), (uint32_t)rel[c].size()) == HM_OK)
                ds->free_h[c].insert(ds->free_h[c].end(), rel[c].begin(), rel[c].end());
            rel[c].clear();
        }
    }
    // a call-level failure: the call is applied to no store — a store whose batch is in flight is
    // waited for, the batches already applied are undone (hm_batch_undo) — and every document of
    // the call rolls back on the host
    int fail(int why) {
        for (auto &v : rel) v.clear();                       // (every fresh handle is listed below)
        // a store whose batch cannot be waited for or undone keeps rows the host no longer
        // describes: the docset refuses every later call rather than diverge silently
        bool lost = false;
        for (uint32_t c = 0; c < N_CLASS; c++) {
            if (co[c].sub) {
                std::vector<hm_doc_result> tmp(by_cls[c].size());
                if (hm_batch_wait(ds->stores[c], co[c].id, tmp.data(), nullptr, nullptr, nullptr) == HM_OK) co[c].done = true;
                else lost = true;                              // submitted, neither waited for nor undoable
                co[c].sub = false;
            }
            if (co[c].done) {
                if (hm_batch_undo(ds->stores[c], co[c].id) != HM_OK) lost = true;
                co[c].done = false;
            }
        }
        for (uint32_t i = 0; i < n; i++) {
            Round &x = R[i];
            DocSt &d = ds->doc(x.doc);
            if (x.status == HM_OK) rollback(d, x);
            if (!x.fresh) continue;
            // a new document whose own merge failed was given its fresh handle above (an empty
            // document in its store); the handle goes back to the free list, so the document
            // must not keep it
            if (x.placed && d.cls == x.cls && d.handle == x.handle) { d.cls = NO_CLASS; d.handle = 0; }
            rel[x.cls].push_back(x.handle);
        }
        release();
        if (lost) ds->broken = true;
        return why;
    }
    // failed documents roll back; the registers and history slices each patch reads are requested
    // before any document's host state advances (a failed read then fails the call on every store)
    void settle() {
        for (uint32_t i = 0; i < n; i++) {
            Round &x = R[i];
            DocSt &d = ds->doc(x.doc);
            if (x.status == HM_OK && x.res.status != HM_OK) x.status = x.res.status;
            if (x.status != HM_OK) {
                if (x.cls != NO_CLASS) rollback(d, x);
                if (x.placed) { d.cls = x.cls; d.handle = x.handle; }          // an empty document in its store
                else if (x.moved) rel[x.cls].push_back(x.handle);               // it stays where it was
                continue;
            }
            x.prev_hist = d.hist_len;
            if (!ds->patches) continue;
            if (ds->op_diffs) { hreq[x.cls].push_back(i); continue; }
            x.full = !(d.n_queued == 0 && x.res.n_queued == 0 && x.res.hist_len - d.hist_len == x.ch.size());
            x.q0 = (uint32_t)qregs[x.cls].size();
            if (x.full) {
                for (uint32_t g = 0; g < x.n_regs; g++) { qdocs[x.cls].push_back(x.handle); qregs[x.cls].push_back(g); }
                ds->stat[4]++;
            } else {
                // the registers the round's set/del/link/inc ops hit, first hit first
                std::vector<uint32_t> &q = qregs[x.cls];
                for (const hm_op_row &o : x.op) {
                    if (o.action < HM_SET || o.reg == HM_NONE) continue;
                    bool dup = false;
                    for (uint32_t j = x.q0; j < q.size() && !dup; j++) dup = q[j] == o.reg;
                    if (dup) continue;
                    q.push_back(o.reg);
                    qdocs[x.cls].push_back(x.handle);
                }
                ds->stat[3]++;
            }
            x.q1 = (uint32_t)qregs[x.cls].size();
            cap[x.cls] += x.res.n_surv;
        }
    }
    int read_regs() {
        for (uint32_t c = 0; c < N_CLASS; c++) {
            if (qregs[c].empty()) continue;
            rrows[c].resize(qregs[c].size());
            rsurv[c].resize(std::max<uint32_t>(cap[c], 1));
            uint32_t got = 0;
            const int rc = hm_store_read_regs(ds->stores[c], (uint32_t)qregs[c].size(), qdocs[c].data(), qregs[c].data(),
                                              rrows[c].data(), rsurv[c].data(), (uint32_t)rsurv[c].size(), &got);
            if (rc) return rc;
        }
        return HM_OK;
    }
    // op diffs: each document's history slice of this round (the changes the GPU applied, in
    // application order) with their allDeps rows
    int read_history() {
        for (uint32_t c = 0; c < N_CLASS; c++) {
            if (hreq[c].empty()) continue;
            const uint32_t m = (uint32_t)hreq[c].size();
            std::vector<uint32_t> hh(m), from(m), to(m), off(m + 1, 0);
            for (uint32_t k = 0; k < m; k++) {
                Round &x = R[hreq[c][k]];
                hh[k] = x.handle;
                to[k] = x.res.hist_len;
                from[k] = x.prev_hist;
                off[k + 1] = off[k] + (to[k] - from[k]);
                x.h0 = off[k]; x.h1 = off[k + 1];
            }
            hlog[c].resize(std::max(1u, off[m]));                 // (rounds that applied nothing: no rows)
            had[c].resize(std::max<size_t>(1, (size_t)off[m] * STRIDES[c]));
            const int rc = hm_store_read_history(ds->stores[c], m, hh.data(), from.data(), to.data(), off.data(), hlog[c].data(),
                                                 had[c].data());
            if (rc) return rc;
        }
        return HM_OK;
    }
    // device diffs: what each applied op of every round's history slice did, from the stores (one
    // one-walk call per class).  The tables are guessed: rows = the ops the rounds handed in, plus the
    // log's ops of a document that held queued changes (they may apply now), survivors = rows times the
    // largest survivors-per-row ratio the docset's calls have reported so far; a call that reports
    // larger totals is repeated once with them.
    int read_diffs() {
        for (uint32_t c = 0; c < N_CLASS; c++) {
            call_dstat[0] += hreq[c].size();
            std::vector<uint32_t> hh, from, to, who;
            size_t ops = 0;
            for (uint32_t i : hreq[c]) {
                Round &x = R[i];
                x.h0 = HM_NONE;
                if (x.prev_hist >= x.res.hist_len) continue;     // (the round applied nothing: no diffs)
                x.h0 = (uint32_t)hh.size();
                hh.push_back(x.handle); from.push_back(x.prev_hist); to.push_back(x.res.hist_len); who.push_back(i);
                ops += x.op.size();
                const DocSt &d = ds->doc(x.doc);
                if (d.n_queued) ops += d.n_ops;
            }
            if (hh.empty()) continue;
            const uint32_t m = (uint32_t)hh.size();
            std::vector<uint32_t> flags(m);
            drange[c].resize(2 * (size_t)m);
            uint64_t cap[2] = {ops + 64, (uint64_t)((double)ops * ds->surv_per_row) + 64}, tot[2] = {0, 0};
            const std::string before = hm_engine_last_error(ds->e);
            for (int attempt = 0;; attempt++) {
                if (cap[0] > 0xFFFFFFFFull || cap[1] > 0xFFFFFFFFull) return hm_engine_fail(ds->e, HM_ERR_NOMEM, "a call's rows stay below 2^32");
                drows[c].resize(cap[0] + 1); dsurv[c].resize(cap[1] + 1); dindex[c].resize(cap[0] + 1);
                hm_op_diff_out po = {(uint32_t)cap[0], (uint32_t)cap[1], drows[c].data(), dsurv[c].data(), drange[c].data(), flags.data()};
                call_dstat[1]++;
                const int rc = hm_store_op_diffs_ex(ds->stores[c], m, hh.data(), from.data(), to.data(), &po, dindex[c].data(), tot,
                                                    HM_ODF_LISTS | HM_ODF_ONCE);
                if (rc == HM_OK) break;
                if (rc != HM_ERR_NOMEM || attempt || (tot[0] <= cap[0] && tot[1] <= cap[1])) return rc;
                hm_engine_fail(ds->e, HM_OK, before.c_str());     // (too small a guess is no failure: the sizes are known now)
                call_dstat[2]++;
                cap[0] = tot[0]; cap[1] = tot[1];
            }
            if (tot[0]) ds->surv_per_row = std::min(16.0, std::max(ds->surv_per_row, 1.25 * (double)tot[1] / (double)tot[0]));
            for (uint32_t k = 0; k < m; k++) {
                const Round &x = R[who[k]];
                if (flags[k]) return hm_engine_fail(ds->e, HM_ERR_INVALID, "a round's op diffs were flagged: list elements assigned without the document's hint");
                const uint64_t r0 = drange[c][2 * (size_t)k], rn = drange[c][2 * (size_t)k + 1];
                if (r0 + rn > cap[0]) return hm_engine_fail(ds->e, HM_ERR_INVALID, "a round's op diffs outside the call's rows");
                const uint64_t n_ops = (uint64_t)ds->doc(x.doc).n_ops + x.op.size();      // (the log once the round commits)
                for (uint64_t r = r0; r < r0 + rn; r++) {
                    const hm_op_diff &dr = drows[c][r];
                    if (dr.op >= n_ops || (uint64_t)dr.surv_off + dr.n_surv > cap[1])
                        return hm_engine_fail(ds->e, HM_ERR_INVALID, "an op diff outside the document's log");
                }
            }
        }
        return HM_OK;
    }
    // commit: every successful document's host state advances with the device's (a call lists a
    // document once, so the documents advance in parallel; the released handles of moved documents
    // go to the shared lists first)
    void commit() {
        for (uint32_t i = 0; i < n; i++)
            if (R[i].status == HM_OK && R[i].moved) { const DocSt &d = ds->doc(R[i].doc); rel[d.cls].push_back(d.handle); }
        par_for(n, T, [&](uint32_t lo, uint32_t hi, uint32_t) {
            for (uint32_t i = lo; i < hi; i++) {
                Round &x = R[i];
                if (x.status != HM_OK) continue;
                DocSt &d = ds->doc(x.doc);
                const uint32_t old_n_ops = d.n_ops;
                d.cls = x.cls; d.handle = x.handle;
                d.flags |= x.flags;
                d.n_changes += (uint32_t)x.ch.size();
                d.n_ops += (uint32_t)x.op.size();
                d.hist_len = x.res.hist_len; d.n_queued = x.res.n_queued;
                d.obj_type.resize(x.n_objs, NO_TYPE);
                d.obj_emitted.resize(x.n_objs, 0);
                d.sig.resize(x.n_regs, 0);
                for (const hm_op_row &o : x.op)
                    if (o.action <= HM_MAKE_TEXT && o.obj < d.obj_type.size() && d.obj_type[o.obj] == NO_TYPE) d.obj_type[o.obj] = o.action;
                if (!(ds->patches && ds->op_diffs)) continue;
                if (ds->device_diffs) {                          // (the renderer reads the log's op rows; nothing is replayed)
                    d.oplog.insert(d.oplog.end(), x.op.begin(), x.op.end());
                    continue;
                }
                // the replay's view of the log (op indices are the store's: appended in order)
                for (const hm_change_row &c : x.ch) {
                    d.ch_op0.push_back(old_n_ops + c.op_first);
                    d.op_seq.insert(d.op_seq.end(), c.n_ops, c.seq);
                }
                d.oplog.insert(d.oplog.end(), x.op.begin(), x.op.end());
                d.rs.resize(x.n_regs);
                d.el_op.resize(x.n_regs, HM_NONE);
                d.el_in.resize(x.n_regs, 0);
                d.el_blk.resize(x.n_regs, HM_NONE);
            }
        });
        for (int k = 0; k < 3; k++) ds->routing[k] += call_routing[k];
        for (int k = 0; k < 3; k++) ds->dstat[k] += call_dstat[k];
    }
    // a round's diffs into either writer: the replay of its history slice (op diffs), or the net
    // diffs of the registers it requested
    template <typename W> void diffs(W &w, Round &x, DocSt &d) {
        if (!ds->patches) return;
        if (ds->device_diffs) {
            // (read_diffs checked every row against the log before the commit)
            if (x.h0 != HM_NONE)
                render_op_rows(w, d, drows[x.cls].data(), dindex[x.cls].data(), dsurv[x.cls].data(), drange[x.cls][2 * (size_t)x.h0],
                               drange[x.cls][2 * (size_t)x.h0 + 1]);
        } else if (ds->op_diffs) {
            Replay rp{d, STRIDES[x.cls]};
            rp.round(w, hlog[x.cls].data() + x.h0, had[x.cls].data() + (size_t)x.h0 * STRIDES[x.cls], x.h1 - x.h0, x.touched);
        } else if (x.q1 > x.q0) {
            render_diffs(w, d, qregs[x.cls].data() + x.q0, rrows[x.cls].data() + x.q0, rsurv[x.cls].data(), x.q1 - x.q0);
        } else render_diffs(w, d, nullptr, nullptr, nullptr, 0);
    }
    // every successful document's patch and DocBackend.clock: the binary pass, then the JSON pass
    // (a JSON docset, or a binary call that met a lone surrogate: the binary pass already advanced
    // the patch base, so the JSON is rebuilt from the binary documents — same diffs, same order)
    void render() {
        const uint32_t Tr = std::min<uint32_t>(ds->threads, std::max<uint32_t>(1, n / 128));
        if (ds->binary) par_for(n, Tr, [&](uint32_t lo, uint32_t hi, uint32_t) {
            StrMap m;
            for (uint32_t i = lo; i < hi; i++) {
                Round &x = R[i];
                if (x.status != HM_OK) continue;
                DocSt &d = ds->doc(x.doc);
                m.reset();
                BinW w{x.bin, d, m};
                x.bin.w.reserve(64);
                w.clock(x.clock, x.n_actors);
                w.clock(x.heads, x.n_actors);
                w.clock(x.back, x.n_actors);
                uint32_t rc[HM_MAX_STRIDE];
                round_clock(x, rc);
                w.clock(rc, x.n_actors);
                w.begin();
                diffs(w, x, d);
                w.end();
            }
        });
        if (ds->binary) for (auto &x : R) exotic |= x.bin.exotic;
        if (ds->binary && !exotic) return;
        par_for(n, Tr, [&](uint32_t lo, uint32_t hi, uint32_t) {
            for (uint32_t i = lo; i < hi; i++) {
                Round &x = R[i];
                if (x.status != HM_OK) continue;
                if (exotic) { bin_to_json(x.bin, x.patch, x.bclock, x.cclock); continue; }
                DocSt &d = ds->doc(x.doc);
                std::string &o = x.patch;
                o.reserve(256);
                JsonW w{o, d};
                o += "{\"clock\":";
                jclock(o, d, x.clock, x.n_actors);
                o += ",\"deps\":";
                jclock(o, d, x.heads, x.n_actors);
                o += ",\"canUndo\":false,\"canRedo\":false,\"diffs\":[";
                diffs(w, x, d);
                o += "]}";
                jclock(x.bclock, d, x.back, x.n_actors);
                uint32_t rc[HM_MAX_STRIDE];
                round_clock(x, rc);
                jclock(x.cclock, d, rc, x.n_actors);
            }
        });
    }
    // op diffs: the replay's registers against the device's merged registers
    void verify() {
        for (uint32_t c = 0; c < N_CLASS; c++) {
            std::vector<uint32_t> vd, vr, vx;
            uint32_t vcap = 0;
            for (uint32_t i : hreq[c]) {
                Round &x = R[i];
                for (uint32_t g : x.touched) { vd.push_back(x.handle); vr.push_back(g); vx.push_back(i); }
                vcap += x.res.n_surv;
            }
            if (vr.empty()) continue;
            std::vector<hm_reg_result> gr(vr.size());
            std::vector<hm_surv_result> gs(std::max<uint32_t>(vcap, 1));
            uint32_t got = 0;
            // (a self-check of the committed round: a read that fails skips it, stat[7])
            if (hm_store_read_regs(ds->stores[c], (uint32_t)vr.size(), vd.data(), vr.data(), gr.data(), gs.data(),
                                   (uint32_t)gs.size(), &got) != HM_OK) { ds->stat[7]++; continue; }
            std::atomic<uint64_t> bad{0};
            const uint32_t nq = (uint32_t)vr.size();
            par_for(nq, std::min<uint32_t>(ds->threads, std::max<uint32_t>(1, nq / 4096)), [&](uint32_t lo, uint32_t hi, uint32_t) {
                uint32_t bad_doc = HM_NONE;
                uint64_t nb = 0;
                for (uint32_t q = lo; q < hi; q++) {
                    DocSt &d = ds->doc(R[vx[q]].doc);
                    bool ok = same_register(d, vr[q], gr[q], gs.data());
                    const uint32_t ob = gr[q].obj;
                    if (ok && !d.rs[vr[q]].empty() && ob < d.obj_type.size() &&
                        (d.obj_type[ob] == HM_MAKE_LIST || d.obj_type[ob] == HM_MAKE_TEXT)) {
                        Replay rp{d, STRIDES[c]};
                        ok = gr[q].list_index == (int32_t)rp.visible_before(ob, vr[q]);
                    }
                    if (!ok && bad_doc != vx[q]) { nb++; bad_doc = vx[q]; }
                }
                bad += nb;
            });
            ds->stat[6] += bad.load();
        }
        for (uint32_t c = 0; c < N_CLASS; c++) ds->stat[5] += hreq[c].size();
    }
    // HMP1 layout: header u32[8] {magic, n_docs, n_strings, n_words, n_nums, blob_bytes, ascii, 0},
    // doc_word_off / doc_str_base / doc_num_base u32[n_docs + 1] each, str_off u32[n_strings + 1]
    // (byte offsets into the blob), words u32[n_words], (8-aligned) nums f64[n_nums], blob
    void assemble_hmp1(std::string &s) {
        std::vector<uint32_t> wo(n + 1, 0), sb(n + 1, 0), nb(n + 1, 0);
        std::vector<uint64_t> bb(n + 1, 0);                  // each document's first blob byte
        for (uint32_t i = 0; i < n; i++) {
            const BinDoc &x = R[i].bin;
            wo[i + 1] = wo[i] + (uint32_t)x.w.size(); sb[i + 1] = sb[i] + (uint32_t)x.strs.size(); nb[i + 1] = nb[i] + (uint32_t)x.nums.size();
            uint64_t b = 0;
            for (auto &t : x.strs) b += t.second;
            bb[i + 1] = bb[i] + b;
        }
        const uint64_t blob = bb[n];
        const uint32_t ns = sb[n], nw = wo[n], nn = nb[n];
        size_t head = 4 * (8 + 3 * ((size_t)n + 1) + (size_t)ns + 1 + nw);
        const size_t pad = (8 - head % 8) % 8;
        s.resize(head + pad + 8 * (size_t)nn + blob);
        uint32_t *h = (uint32_t *)&s[0];
        h[0] = 0x31504D48u; h[1] = n; h[2] = ns; h[3] = nw; h[4] = nn; h[5] = (uint32_t)blob; h[6] = 1; h[7] = 0;
        uint32_t *p = h + 8;
        memcpy(p, wo.data(), 4 * ((size_t)n + 1)); p += n + 1;
        memcpy(p, sb.data(), 4 * ((size_t)n + 1)); p += n + 1;
        memcpy(p, nb.data(), 4 * ((size_t)n + 1)); p += n + 1;
        uint32_t *so = p;
        p += ns + 1;
        uint32_t *words = p;
        double *nums = (double *)(&s[0] + head + pad);
        char *bl = &s[0] + head + pad + 8 * (size_t)nn;
        so[0] = 0;
        // documents copied in parallel: every one has its own word / number / string ranges
        std::atomic<bool> ascii{true};
        par_for(n, std::min<uint32_t>(ds->threads, std::max<uint32_t>(1, n / 256)), [&](uint32_t lo, uint32_t hi, uint32_t) {
            bool asc = true;
            for (uint32_t i = lo; i < hi; i++) {
                const BinDoc &x = R[i].bin;
                if (!x.w.empty()) memcpy(words + wo[i], x.w.data(), 4 * x.w.size());
                if (!x.nums.empty()) memcpy(nums + nb[i], x.nums.data(), 8 * x.nums.size());
                uint64_t at = bb[i];
                uint32_t k = sb[i];
                for (auto &t : x.strs) {
                    memcpy(bl + at, t.first, t.second);
                    if (asc)
                        for (uint32_t c = 0; c < t.second; c++) asc &= (unsigned char)t.first[c] < 0x80;
                    at += t.second;
                    so[++k] = (uint32_t)at;
                }
            }
            if (!asc) ascii = false;
        });
        h[6] = ascii ? 1 : 0;
    }
    // {"p": [patch | null per document], "b": [max over the whole log | null], "c": [max over this call's changes | null]}
    void assemble_json(std::string &s) {
        size_t tot = 16;
        for (auto &x : R) tot += x.patch.size() + x.bclock.size() + x.cclock.size() + 18;
        s.reserve(tot);
        s += "{\"p\":[";
        for (uint32_t i = 0; i < n; i++) { if (i) s += ','; if (R[i].status == HM_OK) s += R[i].patch; else s += "null"; }
        s += "],\"b\":[";
        for (uint32_t i = 0; i < n; i++) { if (i) s += ','; if (R[i].status == HM_OK) s += R[i].bclock; else s += "null"; }
        s += "],\"c\":[";
        for (uint32_t i = 0; i < n; i++) { if (i) s += ','; if (R[i].status == HM_OK) s += R[i].cclock; else s += "null"; }
        s += "]}";
    }
    // the call's result: the text (HMP1, or JSON), every document's result row, the call counters
    void assemble(hm_text *out) {
        out->s.clear();
        if (ds->binary && !exotic) assemble_hmp1(out->s);
        else assemble_json(out->s);
        out->res.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            Round &x = R[i];
            hm_doc_result &r = out->res[i];
            if (x.cls == NO_CLASS && x.status != HM_OK) {                    // the call's blocks did not decode
                r = hm_doc_result{};
                r.status = x.status; r.err_change = x.err_block; r.err_op = HM_NONE;
                DocSt &d = ds->doc(x.doc);
                r.hist_len = d.hist_len; r.n_queued = d.n_queued;
            } else r = x.res;
        }
        ds->stat[0]++;
        ds->stat[1] += n;
    }
};

int finish(Call &c, hm_text *out);

// One call = one applyChanges round for every document of the call.  A phase that returns a
// status fails the call: fail() undoes it on every store and rolls every document back.
int apply(hm_docset *ds, const uint8_t *data, const uint64_t *bo, const uint32_t *doc_block, const uint32_t *docs, uint32_t n,
          hm_text *out) {
    Call c{ds, data, bo, doc_block, docs, n};
    int rc = c.validate();
    if (rc) return rc;
    c.decode();
    c.mark("decode");
    c.place();
    for (uint32_t k = 0; k < N_CLASS; k++)
        if (!c.by_cls[k].empty() && (rc = c.merge_class(k))) return c.fail(rc);
    c.mark("merge");
    return finish(c, out);
}

// the phases behind the merge: what every round's patch reads, the commit, the rendering
int finish(Call &c, hm_text *out) {
    hm_docset *ds = c.ds;
    int rc;
    c.settle();
    // (the injected read failure: after the requests are built, before any read)
    if (c.inj_read) return c.fail(hm_engine_fail(ds->e, HM_ERR_DEVICE, "injected failure (HM_DOCSET_INJECT_FAIL)"));
    if ((rc = c.read_regs())) return c.fail(rc);
    if (ds->device_diffs) {
        if ((rc = c.read_diffs())) return c.fail(rc);
        c.mark("read diffs");
    } else {
        if ((rc = c.read_history())) return c.fail(rc);
        c.mark("read history");
    }
    c.commit();
    c.mark("commit");
    c.release();
    c.mark("read regs");
    c.render();
    c.mark("diffs");
    if (ds->patches && ds->op_diffs && !ds->device_diffs) {
        c.verify();
        c.mark("verify");
    }
    c.assemble(out);
    c.mark("render");
    return HM_OK;
}

// ---------------- what the host queries over many documents share ----------------
// the request's documents exist (and, with entry_off, its entry ranges do not decrease)
int check_request(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *entry_off = nullptr) {
    const uint32_t nd = ds->n_docs.load();
    for (uint32_t i = 0; i < n; i++) {
        if (docs[i] >= nd) return hm_engine_fail(ds->e, HM_ERR_INVALID, "bad docset document");
        if (entry_off && entry_off[i + 1] < entry_off[i]) return hm_engine_fail(ds->e, HM_ERR_INVALID, "entry_off must not decrease");
    }
    return HM_OK;
}

// the request's documents that live in class c: their places in docs[0..n) and their store handles
void class_docs(hm_docset *ds, uint32_t c, uint32_t n, const uint32_t *docs, std::vector<uint32_t> &idx, std::vector<uint32_t> &hs) {
    for (uint32_t i = 0; i < n; i++) {
        const DocSt &d = ds->doc(docs[i]);
        if (d.cls == c) { idx.push_back(i); hs.push_back(d.handle); }
    }
}

// a clock entry's seq (a JS number) as the stores' u32
uint32_t seq_u32(double v) { return !(v > 0) ? 0u : v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v; }

// the per-document texts as one JSON array
hm_text *json_array(const std::vector<std::string> &js) {
    std::unique_ptr<hm_text> t(new hm_text());
    t->s = "[";
    for (size_t i = 0; i < js.size(); i++) { if (i) t->s += ','; t->s += js[i]; }
    t->s += ']';
    return t.release();
}

// what a request about a document's past selects by: a history length, or a clock row [a_stride], per request
struct Selector {
    std::vector<uint32_t> v;
    bool by_len = false;
    const uint32_t *lens() const { return by_len ? v.data() : nullptr; }
    const uint32_t *rows() const { return by_len ? nullptr : v.data(); }
};

// The clocks of a call's requests as the C ABI hands them over (request i's entries are entry_off[i] ..
// entry_off[i + 1]; entry e's actor id is actor_ids[actor_off[e] .. actor_off[e + 1]), its seq seqs[e]),
// and the one place that reads them against a document.
struct Clocks {
    hm_docset *ds;
    const uint32_t *entry_off;
    const char *actor_ids;
    const uint32_t *actor_off;
    const double *seqs;
    int check(uint32_t i) const { return each(i, nullptr, [](uint32_t, uint32_t) {}, [](uint32_t) {}); }
    // request i's entries in listed order: known(rank, seq) for an actor d has seen, unknown(seq) for any
    // other (without d: the entries' lengths are checked, nothing more)
    template <typename K, typename U> int each(uint32_t i, const DocSt *d, K &&known, U &&unknown) const {
        for (uint32_t e = entry_off[i]; e < entry_off[i + 1]; e++) {
            if (actor_off[e + 1] < actor_off[e]) return hm_engine_fail(ds->e, HM_ERR_INVALID, "actor_off must not decrease");
            if (!d) continue;
            const uint32_t a = d->actors.find(actor_ids + actor_off[e], actor_off[e + 1] - actor_off[e], 0);
            if (a == HM_NONE || a >= d->rank_of.size()) unknown(seq_u32(seqs[e]));
            else known(d->rank_of[a], seq_u32(seqs[e]));
        }
        return HM_OK;
    }
    // as a dense row[S] (zeroed by the caller): ranks from S on are dropped, a rank's later entry wins;
    // order[S] (HM_NONE by the caller, optional): the ranks in first-listed order
    int dense(uint32_t i, const DocSt &d, uint32_t S, uint32_t *row, uint32_t *order = nullptr) const {
        return each(i, &d, [&](uint32_t r, uint32_t q) {
            if (r >= S) return;
            row[r] = q;
            uint32_t *at = order ? std::find_if(order, order + S, [r](uint32_t o) { return o == r || o == HM_NONE; }) : nullptr;
            if (at && at != order + S) *at = r;
        }, [](uint32_t) {});
    }
    // as a sparse (rank, seq) list, appended.  With `ready`: an actor never seen with a seq above 0 is a
    // change d has not applied — the request is then not ready and appends nothing.
    int sparse(uint32_t i, const DocSt &d, std::vector<uint16_t> &act, std::vector<uint32_t> &seq, bool *ready = nullptr) const {
        const size_t keep = act.size();
        bool all = true;
        const int rc = each(i, &d, [&](uint32_t r, uint32_t q) { act.push_back((uint16_t)r); seq.push_back(q); },
                            [&](uint32_t q) { all = all && q == 0u; });
        if (ready && !(*ready = all)) { act.resize(keep); seq.resize(keep); }
        return rc;
    }
    // the selector of a class's requests idx[] (places in docs[] / hist_len[]) at stride S: the history
    // lengths, or each request's clock as a dense row (and, with `order`, its order row)
    int select(const uint32_t *docs, const uint32_t *hist_len, const std::vector<uint32_t> &idx, uint32_t S, Selector &sel,
               std::vector<uint32_t> *order = nullptr) const {
        sel.by_len = hist_len != nullptr;
        sel.v.assign(hist_len ? idx.size() : idx.size() * (size_t)S, 0u);
        if (order && !hist_len) order->assign(idx.size() * (size_t)S, HM_NONE);
        int rc = HM_OK;
        for (size_t j = 0; j < idx.size() && !rc; j++) {
            if (hist_len) sel.v[j] = hist_len[idx[j]];
            else rc = dense(idx[j], ds->doc(docs[idx[j]]), S, sel.v.data() + j * S, order ? order->data() + j * S : nullptr);
        }
        return rc;
    }
};

// ---------------- fork ----------------
// The new document d as its parent p names things: the interners and rank tables (the gathered rows
// keep the parent's ranks, object and register ids), an empty log.
void clone_names(DocSt &d, const DocSt &p) {
    if (!d.ready) d.setup();
    d.actors = p.actors; d.objs = p.objs; d.regs = p.regs; d.strs = p.strs;
    d.rank_of = p.rank_of; d.by_rank = p.by_rank;
}

// Call::take_gathered for a fork: the new document names things as its parent does (ids are copied) and
// takes over the content table of the selected (actor, seq)
struct ForkHook {
    hm_docset *ds;
    const uint32_t *parents;
    static constexpr bool PARALLEL = true;
    static constexpr const char *BAD_ROWS = "a fork's rows outside the gathered tables or its parent's log", *BAD_OPS = BAD_ROWS,
                                *BAD_IDS = BAD_ROWS, *NOMEM = "out of memory in hm_docset_fork";
    const DocSt &source(uint32_t i) const { return ds->doc(parents[i]); }
    bool rename(uint32_t, std::vector<hm_op_row> &) const { return true; }
    uint32_t actor(uint32_t, uint16_t a) const { return a; }
    void rest(uint32_t i, const Round &x, DocSt &d) const {
        const DocSt &p = source(i);
        std::unordered_set<uint64_t> keys;
        for (const hm_change_row &cr : x.ch)
            if (cr.actor < p.by_rank.size()) keys.insert(((uint64_t)p.by_rank[cr.actor] << 32) | cr.seq);
        for (const DocSt::CE &e : p.cents)
            if (keys.count(e.key)) d.cents.push_back({e.key, e.h, e.cid, HM_NONE});
        d.n_content = p.n_content;
        size_t cap = 64;
        while ((d.cents.size() + 1) * 2 > cap) cap *= 2;
        d.crehash(cap);
    }
};

// hm_docset_fork: the new documents first + i are rounds of one Call whose rows come from the stores'
// fork batches instead of a decode — a parent not placed yet gives a round without blocks — and whose
// later phases (what each patch reads, commit, rendering, the replay check) are hm_docset_apply's.
int fork_docs(hm_docset *ds, uint32_t n, const uint32_t *parents, const uint32_t *hist_len, const uint32_t *entry_off,
              const char *actor_ids, const uint32_t *actor_off, const double *seqs, uint32_t first, hm_text *out) {
    std::vector<uint32_t> nd(n), no_blocks(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) nd[i] = first + i;
    Call c{ds, nullptr, nullptr, no_blocks.data(), nd.data(), n};
    c.t0 = std::chrono::steady_clock::now();
    c.R.resize(n);
    const Clocks clocks{ds, entry_off, actor_ids, actor_off, seqs};
    std::vector<uint32_t> forks[N_CLASS];
    ClsOut plain;                                            // the batch of the rounds without blocks
    int rc;
    // the new documents' host state on host threads, as a decode's (a call lists a new document once;
    // parents are only read)
    c.T = std::min<uint32_t>(ds->threads, std::max<uint32_t>(1, n / 64));
    try {
    par_for(n, c.T, [&](uint32_t lo, uint32_t hi, uint32_t) {
        Scratch X;
        for (uint32_t i = lo; i < hi; i++) {
            Round &x = c.R[i];
            DocSt &d = ds->doc(nd[i]);
            const DocSt &p = ds->doc(parents[i]);
            x.doc = nd[i];
            if (p.cls == NO_CLASS) {                         // Backend.init(): an empty round of a fresh document
                decode_round(d, x, nullptr, nullptr, X);
                x.cls = class_for(0); x.placed = true;
                continue;
            }
            clone_names(d, p);
            x.started = true;
            x.s_objs = 1;                                    // (the rollback leaves Backend.init(): ROOT alone)
            x.n_actors = (uint16_t)p.actors.size(); x.n_regs = p.regs.size(); x.n_objs = p.objs.size(); x.flags = p.flags;
            x.cls = p.cls; x.placed = true;
        }
    });
    } catch (...) {
        return c.fail(hm_engine_fail(ds->e, HM_ERR_NOMEM, "out of memory in hm_docset_fork"));
    }
    for (uint32_t i = 0; i < n; i++) {
        if (ds->doc(parents[i]).cls == NO_CLASS) c.by_cls[c.R[i].cls].push_back(i);
        else forks[c.R[i].cls].push_back(i);
    }
    for (uint32_t k = 0; k < N_CLASS; k++) {
        if (c.by_cls[k].empty()) continue;
        if ((rc = c.merge_class(k))) return c.fail(rc);
        // (nothing of this batch needs an undo: its documents are fresh and empty, fail() releases their handles)
        plain = std::move(c.co[k]);
        c.co[k] = ClsOut();
        c.by_cls[k].clear();
    }
    for (uint32_t k = 0; k < N_CLASS; k++) {
        if (forks[k].empty()) continue;
        c.by_cls[k] = forks[k];
        const auto &rows = c.by_cls[k];
        const uint32_t S = STRIDES[k], m = (uint32_t)rows.size();
        hm_store *st = ds->stores[k];
        std::vector<uint32_t> fh, src(m), ord;
        Selector sel;
        if ((rc = c.take_handles(k, st, m, fh))) return c.fail(rc);
        for (uint32_t j = 0; j < m; j++) {
            Round &x = c.R[rows[j]];
            x.handle = fh[j]; x.fresh = true; x.row = j;
            src[j] = ds->doc(parents[rows[j]]).handle;
        }
        if ((rc = clocks.select(parents, hist_len, rows, S, sel, &ord))) return c.fail(rc);
        ClsOut &O = c.co[k];
        if ((rc = hm_store_fork_submit(st, m, src.data(), sel.lens(), sel.rows(), sel.by_len ? nullptr : ord.data(), fh.data(), 0u, &O.id)))
            return c.fail(rc);
        O.sub = true;
        if ((rc = c.take_gathered(k, ForkHook{ds, parents}))) return c.fail(rc);
    }
    c.mark("fork");
    return finish(c, out);
}

// ---------------- merge into a live document ----------------
// One request's maps from its source's id spaces into its destination's (hm_merge_maps' slices), the
// selector rows in the source's ranks, and what the destination's interners looked like before.
struct MergeReq {
    std::vector<uint32_t> amap;                              // source actor id -> destination actor id
    std::vector<uint32_t> rank, omap, rmap, smap, cmap;      // rank: [source ranks]
    std::vector<uint32_t> clock, have, order;                // [source ranks]; order: listed ranks, then HM_NONE
    bool device = false, empty = false;                      // route; empty: the source holds nothing
};

// a new actor re-ranks the document (JS string order): decode_round's step, for actors interned since
// `before`; the round keeps the old tables for the rollback and the remap for the store
void rerank(DocSt &d, Round &R, uint32_t before) {
    const uint32_t na = d.actors.size();
    R.s_rank_of = d.rank_of; R.s_by_rank = d.by_rank;
    std::vector<uint16_t> order(na);
    for (uint32_t i = 0; i < na; i++) order[i] = (uint16_t)i;
    std::sort(order.begin(), order.end(), [&](uint16_t x, uint16_t y) {
        return js_less(d.actors.ptr(x), d.actors.len(x), d.actors.ptr(y), d.actors.len(y)); });
    std::vector<uint16_t> rank_of(na);
    for (uint32_t r = 0; r < na; r++) rank_of[order[r]] = (uint16_t)r;
    bool ident = true;
    std::vector<uint8_t> remap(before);
    for (uint32_t r = 0; r < before; r++) {
        remap[r] = (uint8_t)rank_of[d.by_rank[r]];
        ident &= remap[r] == r;
    }
    if (!ident) R.remap = std::move(remap);
    d.rank_of = std::move(rank_of);
    d.by_rank = std::move(order);
}

// rows of the source's id spaces into the destination's, on the host (the host route; the device
// route's rename pass does the same through the same maps); false: an id outside its map
bool rename_rows(const MergeReq &q, std::vector<hm_change_row> &ch, std::vector<hm_dep_row> &dp, std::vector<hm_op_row> &op) {
    bool ok = true;
    auto thru = [&](const std::vector<uint32_t> &m, uint32_t id) -> uint32_t {
        if (id >= m.size() || m[id] == HM_NONE) { ok = false; return id; }
        return m[id];
    };
    for (hm_change_row &c : ch) { c.actor = (uint16_t)thru(q.rank, c.actor); c.content_id = thru(q.cmap, c.content_id); }
    for (hm_dep_row &d : dp) d.actor = (uint16_t)thru(q.rank, d.actor);
    for (hm_op_row &o : op) {
        o.obj = thru(q.omap, o.obj);
        if (o.reg != HM_NONE) o.reg = thru(q.rmap, o.reg);
        if (o.parent != HM_HEAD) o.parent = thru(q.rmap, o.parent);
        if (o.action >= HM_SET) o.key = thru(q.smap, o.key);
        if (o.vtag == HM_V_STR) o.value = thru(q.smap, (uint32_t)o.value);
        else if (o.vtag == HM_V_OBJ) o.value = thru(q.omap, (uint32_t)o.value);
    }
    return ok;
}

// Call::take_gathered for a merge: the source's ids go through the request's maps (the change rows were
// renamed on the device)
struct MergeHook {
    hm_docset *ds;
    const uint32_t *src;
    const MergeReq *Q;
    static constexpr bool PARALLEL = false;
    static constexpr const char *BAD_ROWS = "a merge's rows outside the gathered tables", *BAD_OPS = "a merge's ops outside its source's log",
                                *BAD_IDS = "a merge's ops name an id its source's tables do not hold", *NOMEM = "out of memory in hm_docset_merge_from";
    const DocSt &source(uint32_t i) const { return ds->doc(src[i]); }
    bool rename(uint32_t i, std::vector<hm_op_row> &op) const {
        std::vector<hm_change_row> no_ch;
        std::vector<hm_dep_row> no_dp;
        return rename_rows(Q[i], no_ch, no_dp, op);
    }
    uint32_t actor(uint32_t i, uint16_t a) const { return a < Q[i].amap.size() ? Q[i].amap[a] : HM_NONE; }
    void rest(uint32_t, const Round &, DocSt &) const {}
};

// hm_docset_merge_from: destination dst[i] is handed source src[i]'s applied changes above what it was
// handed before (its DocBackend.clock) up to the request's clock, actor after actor in the clock's key
// order.  The destinations are rounds of one Call whose rows come from the stores' merge batches (the
// device route: both documents in one stride class, the destination staying in it) or from the
// source's log read back and renamed here (the host route: every other request), and whose later phases
// are hm_docset_apply's.
int merge_docs(hm_docset *ds, uint32_t n, const uint32_t *dst, const uint32_t *src, const uint32_t *entry_off,
               const char *actor_ids, const uint32_t *actor_off, const double *seqs, hm_text *out) {
    std::vector<uint32_t> no_blocks(n + 1, 0);
    Call c{ds, nullptr, nullptr, no_blocks.data(), dst, n};
    const Clocks clocks{ds, entry_off, actor_ids, actor_off, seqs};
    int rc = c.validate();
    if (rc) return rc;
    {
        const uint32_t nd = ds->n_docs.load();
        std::vector<uint8_t> is_dst(nd, 0);
        for (uint32_t i = 0; i < n; i++) is_dst[dst[i]] = 1;
        for (uint32_t i = 0; i < n; i++)
            if (src[i] >= nd || is_dst[src[i]]) return hm_engine_fail(ds->e, HM_ERR_INVALID, "a merge's source is no document, or a destination of the same call");
    }
    c.R.resize(n);
    std::vector<MergeReq> Q(n);
    // the maps: every actor, object, register and string of the source is interned into the destination
    // (deps and links may name any); content ids of the (actor, seq) entries the selector covers
    for (uint32_t i = 0; i < n; i++) {                       // (every round's snapshot first: fail() rolls all of them back)
        Round &x = c.R[i];
        DocSt &d = ds->doc(dst[i]);
        x.doc = dst[i];
        if (!d.ready) d.setup();
        x.s_actors = d.actors.size(); x.s_objs = d.objs.size(); x.s_regs = d.regs.size(); x.s_strs = d.strs.size();
        x.s_cents = (uint32_t)d.cents.size(); x.s_content = d.n_content; x.s_ops = (uint32_t)d.op_actor.size();
        x.started = true;
    }
    try {
    // the destinations' DocBackend.clock rows, one read per stride class
    std::vector<std::vector<uint32_t>> backs(n);
    for (uint32_t k = 0; k < N_CLASS; k++) {
        std::vector<uint32_t> idx, hh;
        class_docs(ds, k, n, dst, idx, hh);
        if (idx.empty()) continue;
        const uint32_t Sd = STRIDES[k];
        std::vector<uint32_t> rows(idx.size() * (size_t)Sd);
        if ((rc = hm_store_back_clocks(ds->stores[k], (uint32_t)idx.size(), hh.data(), rows.data()))) return c.fail(rc);
        for (size_t j = 0; j < idx.size(); j++) backs[idx[j]].assign(rows.begin() + j * Sd, rows.begin() + (j + 1) * Sd);
    }
    for (uint32_t i = 0; i < n; i++) {
        Round &x = c.R[i];
        MergeReq &q = Q[i];
        DocSt &d = ds->doc(dst[i]);
        const DocSt &p = ds->doc(src[i]);
        q.empty = p.cls == NO_CLASS || !p.ready;
        bool f, fresh_any = false;
        if (!q.empty) {
            q.amap.resize(p.actors.size());
            for (uint32_t a = 0; a < p.actors.size(); a++) { q.amap[a] = d.actors.get(p.actors.ptr(a), p.actors.len(a), 0, f); fresh_any |= f; }
        }
        if (d.actors.size() > MAX_ACTORS) { x.status = HM_ERR_UNSUPPORTED; rollback(d, x); x.started = false; continue; }
        if (fresh_any) rerank(d, x, x.s_actors);
        x.n_actors = (uint16_t)d.actors.size();
        if (!q.empty) {
            const uint32_t ns = (uint32_t)p.by_rank.size();
            q.rank.resize(ns); q.clock.assign(ns, 0); q.have.assign(ns, 0);
            for (uint32_t r = 0; r < ns; r++) q.rank[r] = d.rank_of[q.amap[p.by_rank[r]]];
            q.omap.resize(p.objs.size());
            for (uint32_t o = 0; o < p.objs.size(); o++) q.omap[o] = d.objs.get(p.objs.ptr(o), p.objs.len(o), 0, f);
            q.rmap.resize(p.regs.size());
            for (uint32_t g = 0; g < p.regs.size(); g++) {
                const uint32_t o = p.regs.tag(g);
                q.rmap[g] = o < q.omap.size() ? d.regs.get(p.regs.ptr(g), p.regs.len(g), q.omap[o], f) : HM_NONE;
            }
            q.smap.resize(p.strs.size());
            for (uint32_t s = 0; s < p.strs.size(); s++) q.smap[s] = d.strs.get(p.strs.ptr(s), p.strs.len(s), 0, f);
            // the clock, by actor id in key order (the hand-over order); an id the source never saw is dropped
            q.order.assign(ns, HM_NONE);
            if ((rc = clocks.dense(i, p, ns, q.clock.data(), q.order.data()))) return c.fail(rc);
            // have: the destination's DocBackend.clock, in the source's ranks
            if (d.cls != NO_CLASS) {
                const std::vector<uint32_t> &back = backs[i];
                const uint32_t Sd = (uint32_t)back.size();
                for (uint32_t r = 0; r < ns; r++) {
                    const uint32_t da = q.amap[p.by_rank[r]];
                    if (da < x.s_actors) {
                        const uint32_t old = x.s_rank_of.empty() ? d.rank_of[da] : x.s_rank_of[da];
                        if (old < Sd) q.have[r] = back[old];
                    }
                }
            }
            q.cmap.assign(p.n_content, HM_NONE);
            for (const DocSt::CE &ce : p.cents) {
                const uint32_t a = (uint32_t)(ce.key >> 32), sq = (uint32_t)ce.key;
                if (a >= p.rank_of.size() || ce.cid >= q.cmap.size()) continue;
                const uint32_t r = p.rank_of[a];
                if (sq <= q.have[r] || sq > q.clock[r]) continue;
                q.cmap[ce.cid] = d.content_id(((uint64_t)q.amap[a] << 32) | sq, ce.h);
            }
        }
        x.n_regs = d.regs.size(); x.n_objs = d.objs.size(); x.flags = q.empty ? 0 : p.flags;
    }
    // routes: the device route where both documents live in one class and the destination stays in it —
    // unless the class also takes host-route rounds in this call (a store has one batch in flight, and
    // only its last batch can be undone: such a class's rounds all go through merge_class)
    bool host_cls[N_CLASS] = {};
    for (uint32_t i = 0; i < n; i++) {
        const DocSt &d = ds->doc(dst[i]), &p = ds->doc(src[i]);
        if (c.R[i].status != HM_OK) continue;
        const uint8_t want = std::max<uint8_t>(class_for(c.R[i].n_actors), d.cls == NO_CLASS ? 0 : d.cls);
        Q[i].device = !Q[i].empty && d.cls != NO_CLASS && p.cls == d.cls && want == d.cls;
        if (!Q[i].device) host_cls[want] = true;
    }
    for (uint32_t i = 0; i < n; i++)
        if (Q[i].device && host_cls[ds->doc(dst[i]).cls]) Q[i].device = false;
    // the host route: the source's log and hist read back, the selection laid out actor after actor,
    // renamed, then placed and merged as decoded rows are
    for (uint32_t i = 0; i < n; i++) {
        Round &x = c.R[i];
        MergeReq &q = Q[i];
        if (x.status != HM_OK || q.device) continue;
        ds->mstat[1]++;
        if (q.empty) continue;
        const DocSt &p = ds->doc(src[i]);
        hm_store *ps = ds->stores[p.cls];
        hm_doc_info_t inf;
        if ((rc = hm_doc_info(ps, p.handle, &inf))) return c.fail(rc);
        std::vector<hm_change_row> lc(inf.n_changes);
        std::vector<hm_dep_row> ld(inf.n_deps);
        std::vector<hm_op_row> lo(inf.n_ops);
        std::vector<int32_t> hist(inf.n_changes);
        if ((rc = hm_doc_log(ps, p.handle, lc.data(), ld.data(), lo.data())) ||
            (rc = hm_doc_read(ps, p.handle, hist.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)))
            return c.fail(rc);
        std::unordered_map<uint64_t, uint32_t> at;            // (rank, seq) of an applied change -> its log row
        for (uint32_t k = 0; k < lc.size(); k++)
            if (hist[k] >= 0) at[((uint64_t)lc[k].actor << 32) | lc[k].seq] = k;
        std::vector<uint32_t> oplog_at;                        // the gathered ops' source log indices
        for (uint32_t r : q.order) {
            if (r == HM_NONE) break;
            for (uint64_t sq = (uint64_t)q.have[r] + 1; sq <= q.clock[r]; sq++) {
                auto it = at.find(((uint64_t)r << 32) | sq);
                if (it == at.end()) break;                     // (an actor's applied changes are its seqs 1 .. opSet.clock)
                hm_change_row cr = lc[it->second];
                if ((uint64_t)cr.dep_off + cr.n_deps > ld.size() || (uint64_t)cr.op_first + cr.n_ops > lo.size())
                    return c.fail(hm_engine_fail(ds->e, HM_ERR_DEVICE, "a merge source's change rows outside its log"));
                const uint32_t d0 = cr.dep_off, o0 = cr.op_first;
                cr.dep_off = (uint32_t)x.dp.size(); cr.op_first = (uint32_t)x.op.size();
                x.ch.push_back(cr);
                x.dp.insert(x.dp.end(), ld.begin() + d0, ld.begin() + d0 + cr.n_deps);
                x.op.insert(x.op.end(), lo.begin() + o0, lo.begin() + o0 + cr.n_ops);
                for (uint32_t k = 0; k < cr.n_ops; k++) oplog_at.push_back(o0 + k);
            }
        }
        if (!rename_rows(q, x.ch, x.dp, x.op)) return c.fail(hm_engine_fail(ds->e, HM_ERR_DEVICE, "a merge's rows name an id its source's tables do not hold"));
        DocSt &d = ds->doc(dst[i]);
        for (uint32_t lo_i : oplog_at) {
            if (lo_i >= p.op_actor.size() || p.op_actor[lo_i] >= q.amap.size()) return c.fail(hm_engine_fail(ds->e, HM_ERR_DEVICE, "a merge's ops outside its source's log"));
            d.op_actor.push_back((uint16_t)q.amap[p.op_actor[lo_i]]);
            d.op_dt.push_back(p.op_dt[lo_i]);
        }
    }
    // place the host-route rounds, and merge them
    for (uint32_t i = 0; i < n; i++)
        if (c.R[i].status == HM_OK && !Q[i].device) c.place_round(i);
    for (uint32_t k = 0; k < N_CLASS; k++)
        if (!c.by_cls[k].empty() && (rc = c.merge_class(k))) return c.fail(rc);
    // the device route, a merge batch per class
    std::vector<uint32_t> dev[N_CLASS];
    for (uint32_t i = 0; i < n; i++)
        if (c.R[i].status == HM_OK && Q[i].device) dev[ds->doc(dst[i]).cls].push_back(i);
    for (uint32_t k = 0; k < N_CLASS; k++) {
        if (dev[k].empty()) continue;
        c.by_cls[k] = dev[k];
        const auto &rows = c.by_cls[k];
        const uint32_t S = STRIDES[k], m = (uint32_t)rows.size();
        hm_store *st = ds->stores[k];
        ds->mstat[0] += m;
        std::vector<uint32_t> sh(m), dh(m), clk((size_t)m * S, 0u), hav((size_t)m * S, 0u), ord((size_t)m * S, HM_NONE), tot((size_t)m * 4),
            rank((size_t)m * S, HM_NONE), off[4], tab[4];
        std::vector<uint8_t> remap;
        bool any_remap = false;
        for (uint32_t j = 0; j < m; j++) any_remap |= !c.R[rows[j]].remap.empty();
        if (any_remap) {
            remap.resize((size_t)m * S);
            for (uint32_t j = 0; j < m; j++) for (uint32_t a = 0; a < S; a++) remap[(size_t)j * S + a] = (uint8_t)a;
        }
        for (auto &o : off) o.assign(1, 0u);
        for (uint32_t j = 0; j < m; j++) {
            const uint32_t i = rows[j];
            Round &x = c.R[i];
            const MergeReq &q = Q[i];
            const DocSt &d = ds->doc(dst[i]), &p = ds->doc(src[i]);
            x.cls = (uint8_t)k; x.handle = d.handle; x.row = j;
            sh[j] = p.handle; dh[j] = d.handle;
            for (uint32_t r = 0; r < q.rank.size() && r < S; r++) { clk[(size_t)j * S + r] = q.clock[r]; hav[(size_t)j * S + r] = q.have[r]; rank[(size_t)j * S + r] = q.rank[r]; }
            for (uint32_t r = 0; r < q.order.size() && r < S; r++) ord[(size_t)j * S + r] = q.order[r];
            for (size_t a = 0; a < x.remap.size() && a < S; a++) remap[(size_t)j * S + a] = x.remap[a];
            tot[4 * (size_t)j] = x.n_actors; tot[4 * (size_t)j + 1] = x.n_regs; tot[4 * (size_t)j + 2] = x.n_objs; tot[4 * (size_t)j + 3] = x.flags;
            const std::vector<uint32_t> *mp[4] = {&q.omap, &q.rmap, &q.smap, &q.cmap};
            for (int t = 0; t < 4; t++) { tab[t].insert(tab[t].end(), mp[t]->begin(), mp[t]->end()); off[t].push_back((uint32_t)tab[t].size()); }
        }
        for (auto &t : tab) if (t.empty()) t.push_back(HM_NONE);
        hm_merge_maps mm = {tot.data(), rank.data(), off[0].data(), tab[0].data(), off[1].data(), tab[1].data(), off[2].data(), tab[2].data(),
                            off[3].data(), tab[3].data()};
        ClsOut &O = c.co[k];
        if ((rc = hm_store_merge_from_submit(st, m, sh.data(), hav.data(), clk.data(), ord.data(), dh.data(), &mm,
                                             any_remap ? remap.data() : nullptr, &O.id)))
            return c.fail(rc);
        O.sub = true;
        if ((rc = c.take_gathered(k, MergeHook{ds, src, Q.data()}))) return c.fail(rc);
    }
    } catch (...) {
        return c.fail(hm_engine_fail(ds->e, HM_ERR_NOMEM, "out of memory in hm_docset_merge_from"));
    }
    c.mark("merge_from");
    return finish(c, out);
}

// hm_docset_materialize: one class's result tables, sized by the store once its count pass has
// run (hm_past_alloc)
struct PastTables {
    uint32_t k, S;
    std::vector<hm_doc_row> rows_d;
    std::vector<hm_op_row> ops;
    std::vector<uint32_t> op_log, clock, heads;
    std::vector<hm_doc_result> res;
    std::vector<hm_reg_result> regs;
    std::vector<hm_surv_result> surv;
    hm_past_out po;
    static const hm_past_out *alloc(void *ctx, const uint64_t *tot) {
        PastTables &t = *(PastTables *)ctx;
        if (tot[2] > 0xFFFFFFFFull || tot[3] > 0xFFFFFFFFull) return nullptr;
        try {
            t.rows_d.resize(t.k); t.res.resize(t.k);
            t.clock.resize((size_t)t.k * t.S); t.heads.resize((size_t)t.k * t.S);
            t.ops.resize(tot[2] + 1); t.op_log.resize(tot[2] + 1); t.surv.resize(tot[2] + 1); t.regs.resize(tot[3] + 1);
        } catch (...) { return nullptr; }
        t.po = hm_past_out{};
        t.po.cap_ops = (uint32_t)tot[2]; t.po.cap_regs = (uint32_t)tot[3];
        t.po.docs = t.rows_d.data(); t.po.ops = t.ops.data(); t.po.op_log = t.op_log.data();
        t.po.res.docs = t.res.data(); t.po.res.clock = t.clock.data(); t.po.res.heads = t.heads.data();
        t.po.res.regs = t.regs.data(); t.po.res.surv = t.surv.data();
        return &t.po;
    }
    // hm_docset_materialize_patch: the prefix's clock, deps and history length alone
    static const hm_past_out *alloc_heads(void *ctx, const uint64_t *) {
        PastTables &t = *(PastTables *)ctx;
        try {
            t.rows_d.resize(t.k); t.res.resize(t.k);
            t.clock.resize((size_t)t.k * t.S); t.heads.resize((size_t)t.k * t.S);
        } catch (...) { return nullptr; }
        t.po = hm_past_out{};
        t.po.docs = t.rows_d.data();
        t.po.res.docs = t.res.data(); t.po.res.clock = t.clock.data(); t.po.res.heads = t.heads.data();
        return &t.po;
    }
};

}  // namespace

extern "C" {

int hm_docset_create(hm_engine *e, const hm_docset_config *cfg, hm_docset **out) {
    if (!e || !out) return HM_ERR_INVALID;
    *out = nullptr;
    hm_docset *ds = new (std::nothrow) hm_docset();
    if (!ds) return HM_ERR_NOMEM;
    ds->e = e;
    const uint32_t hw = std::max(1u, std::thread::hardware_concurrency());
    ds->threads = cfg && cfg->threads ? cfg->threads : std::min<uint32_t>(16, hw);
    ds->patches = !(cfg && (cfg->flags & HM_DOCSET_NO_PATCHES));
    ds->binary = cfg && (cfg->flags & HM_DOCSET_BINARY);
    ds->op_diffs = !(cfg && (cfg->flags & HM_DOCSET_NET_DIFFS));
    ds->device_diffs = cfg && (cfg->flags & HM_DOCSET_DEVICE_DIFFS);
    if (ds->device_diffs && !(ds->patches && ds->op_diffs)) {
        delete ds;
        return hm_engine_fail(e, HM_ERR_INVALID, "HM_DOCSET_DEVICE_DIFFS renders per-op diffs: not with HM_DOCSET_NO_PATCHES / HM_DOCSET_NET_DIFFS");
    }
    ds->chunks.reserve(1u << 16);
    *out = ds;
    return HM_OK;
}

void hm_docset_destroy(hm_docset *ds) {
    if (!ds) return;
    for (auto *s : ds->stores) if (s) hm_store_destroy(s);
    delete ds;
}

hm_engine *hm_docset_engine(hm_docset *ds) { return ds ? ds->e : nullptr; }

int hm_docset_open(hm_docset *ds, uint32_t n, uint32_t *out_first) {
    if (!ds || !out_first) return HM_ERR_INVALID;
    try {
        std::lock_guard<std::mutex> g(ds->open_mu);
        const uint32_t first = ds->n_docs.load();
        const uint64_t need = (uint64_t)first + n;
        if (need > (uint64_t)hm_docset::CHUNK * (1u << 16)) return HM_ERR_NOMEM;
        while ((uint64_t)ds->chunks.size() * hm_docset::CHUNK < need) ds->chunks.emplace_back(new DocSt[hm_docset::CHUNK]);
        ds->n_docs.store((uint32_t)need);
        *out_first = first;
        return HM_OK;
    } catch (...) {
        return HM_ERR_NOMEM;
    }
}

int hm_docset_apply(hm_docset *ds, const uint8_t *data, const uint64_t *block_off, const uint32_t *doc_block,
                    const uint32_t *docs, uint32_t n_docs, hm_text **out) {
    if (!ds || !out || (n_docs && (!block_off || !doc_block || !docs))) return HM_ERR_INVALID;
    *out = nullptr;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "hm_docset_apply: another call on this docset is running");
    if (ds->broken)
        return hm_engine_fail(ds->e, HM_ERR_DEVICE, "hm_docset_apply: an earlier failed call could not be undone on its store");
    try {
        std::unique_ptr<hm_text> t(new hm_text());
        const int rc = apply(ds, data, block_off, doc_block, docs, n_docs, t.get());
        if (rc) return rc;
        *out = t.release();
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_apply");
    }
}

const char *hm_text_data(const hm_text *t, size_t *len) {
    if (!t) return nullptr;
    if (len) *len = t->s.size();
    return t->s.data();
}

const hm_doc_result *hm_text_results(const hm_text *t, uint32_t *n) {
    if (!t) return nullptr;
    if (n) *n = (uint32_t)t->res.size();
    return t->res.data();
}

void hm_text_free(hm_text *t) { delete t; }

int hm_docset_doc_info(hm_docset *ds, uint32_t doc, hm_docset_doc_info_t *out) {
    if (!ds || !out || doc >= ds->n_docs.load()) return HM_ERR_INVALID;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    DocSt &d = ds->doc(doc);
    memset(out, 0, sizeof *out);
    out->a_stride = d.cls == NO_CLASS ? 0 : STRIDES[d.cls];
    out->n_changes = d.n_changes; out->n_ops = d.n_ops; out->n_actors = d.actors.size();
    out->n_objs = std::max<uint32_t>(1, d.objs.size()); out->n_regs = d.regs.size();
    out->hist_len = d.hist_len; out->n_queued = d.n_queued;
    return HM_OK;
}

int hm_docset_history_prefix(hm_docset *ds, uint32_t doc, uint32_t n, uint32_t *out) {
    if (!ds || doc >= ds->n_docs.load() || (n && !out)) return HM_ERR_INVALID;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    DocSt &d = ds->doc(doc);
    if (d.cls == NO_CLASS) return 0;
    return hm_doc_history_prefix(ds->stores[d.cls], d.handle, n, out);
}

int hm_docset_clock_update(hm_docset *ds, uint32_t n, const uint32_t *docs, uint8_t *out_written, uint8_t *out_differs,
                           hm_text **out_stored) {
    if (!ds || (n && !docs)) return HM_ERR_INVALID;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    try {
        int rc = check_request(ds, n, docs);
        if (rc) return rc;
        std::vector<std::string> js(n, "{}");
        for (uint32_t c = 0; c < N_CLASS; c++) {
            std::vector<uint32_t> idx, hs;
            class_docs(ds, c, n, docs, idx, hs);
            if (idx.empty()) continue;
            const uint32_t S = STRIDES[c], k = (uint32_t)idx.size();
            std::vector<uint8_t> w(k), df(k);
            std::vector<uint32_t> stv((size_t)k * S);
            if ((rc = hm_store_clock_update(ds->stores[c], k, hs.data(), w.data(), df.data(), stv.data()))) return rc;
            for (uint32_t j = 0; j < k; j++) {
                const uint32_t i = idx[j];
                if (out_written) out_written[i] = w[j];
                if (out_differs) out_differs[i] = df[j];
                js[i].clear();
                const DocSt &d = ds->doc(docs[i]);
                jclock(js[i], d, stv.data() + (size_t)j * S, d.actors.size());
            }
        }
        for (uint32_t i = 0; i < n; i++) if (ds->doc(docs[i]).cls == NO_CLASS) {
            if (out_written) out_written[i] = 0;
            if (out_differs) out_differs[i] = 0;
        }
        if (out_stored) *out_stored = json_array(js);
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_clock_update");
    }
}

int hm_docset_blocked(hm_docset *ds, uint32_t *out_docs, uint32_t cap, uint32_t *out_n) {
    if (!ds || !out_n || (cap && !out_docs)) return HM_ERR_INVALID;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    try {
        *out_n = 0;
        const uint32_t nd = ds->n_docs.load();
        std::vector<uint32_t> found;
        for (uint32_t c = 0; c < N_CLASS; c++) {
            if (!ds->stores[c] || !ds->opened[c]) continue;
            std::vector<uint32_t> hs(ds->opened[c]);
            uint32_t k = 0;
            const int rc = hm_store_blocked(ds->stores[c], hs.data(), (uint32_t)hs.size(), &k);
            if (rc) return rc;
            if (!k) continue;
            // (handle -> document of this class; a released handle is an empty document, never blocked)
            std::vector<uint32_t> doc_of(ds->opened[c], HM_NONE);
            for (uint32_t i = 0; i < nd; i++) {
                const DocSt &d = ds->doc(i);
                if (d.cls == c && d.handle < doc_of.size()) doc_of[d.handle] = i;
            }
            for (uint32_t j = 0; j < k; j++)
                if (hs[j] < doc_of.size() && doc_of[hs[j]] != HM_NONE) found.push_back(doc_of[hs[j]]);
        }
        std::sort(found.begin(), found.end());
        *out_n = (uint32_t)found.size();
        if (found.size() > cap) return hm_engine_fail(ds->e, HM_ERR_NOMEM, "cap below the number of blocked documents");
        if (!found.empty()) memcpy(out_docs, found.data(), found.size() * 4);
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_blocked");
    }
}

int hm_docset_waiting(hm_docset *ds, uint32_t n, const uint32_t *docs, hm_text **out) {
    if (!ds || !out || (n && !docs)) return HM_ERR_INVALID;
    *out = nullptr;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    try {
        int rc = check_request(ds, n, docs);
        if (rc) return rc;
        std::vector<std::string> js(n, "{\"queued\":[],\"missing\":{}}");      // (a document not placed yet)
        for (uint32_t c = 0; c < N_CLASS; c++) {
            std::vector<uint32_t> idx, hs;
            class_docs(ds, c, n, docs, idx, hs);
            if (idx.empty()) continue;
            const uint32_t S = STRIDES[c], k = (uint32_t)idx.size();
            std::vector<uint32_t> miss((size_t)k * S), nq(k), off(k + 1, 0);
            if ((rc = hm_store_waiting(ds->stores[c], k, hs.data(), miss.data(), nullptr, nq.data()))) return rc;
            for (uint32_t j = 0; j < k; j++) off[j + 1] = off[j] + nq[j];
            std::vector<uint32_t> q(off[k] + 1);
            if ((rc = hm_store_read_queue(ds->stores[c], k, hs.data(), off.data(), q.data()))) return rc;
            for (uint32_t j = 0; j < k; j++) {
                const DocSt &d = ds->doc(docs[idx[j]]);
                std::string &o = js[idx[j]];
                o = "{\"queued\":[";
                for (uint32_t r = off[j]; r < off[j + 1]; r++) { if (r > off[j]) o += ','; o += std::to_string(q[r]); }
                o += "],\"missing\":";
                jclock(o, d, miss.data() + (size_t)j * S, d.actors.size());
                o += '}';
            }
        }
        *out = json_array(js);
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_waiting");
    }
}

int hm_docset_missing_changes(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *entry_off,
                              const char *actor_ids, const uint32_t *actor_off, const double *seqs, uint32_t flags,
                              hm_text **out) {
    if (!ds || !out || (n && (!docs || !entry_off))) return HM_ERR_INVALID;
    *out = nullptr;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    try {
        int rc = check_request(ds, n, docs, entry_off);
        if (rc) return rc;
        if (n && entry_off[n] - entry_off[0] && (!actor_ids || !actor_off || !seqs)) return HM_ERR_INVALID;
        const Clocks clocks{ds, entry_off, actor_ids, actor_off, seqs};
        std::vector<std::string> js(n, "[]");                                    // (a document not placed yet)
        for (uint32_t c = 0; c < N_CLASS; c++) {
            std::vector<uint32_t> idx, hs, off(1, 0), eseq;
            std::vector<uint16_t> eact;
            class_docs(ds, c, n, docs, idx, hs);
            if (idx.empty()) continue;
            for (uint32_t i : idx) {                             // (an actor the document has never seen is dropped)
                if ((rc = clocks.sparse(i, ds->doc(docs[i]), eact, eseq))) return rc;
                off.push_back((uint32_t)eact.size());
            }
            const uint32_t k = (uint32_t)idx.size();
            std::vector<uint32_t> rng(2 * (size_t)k), log;
            uint32_t total = 0;
            rc = hm_store_missing_changes(ds->stores[c], k, hs.data(), off.data(), eact.data(), eseq.data(), flags, nullptr,
                                              rng.data(), nullptr, 0, &total);
            if (rc == HM_ERR_NOMEM && total) {                   // (the counts are known: now with room)
                log.resize(total);
                rc = hm_store_missing_changes(ds->stores[c], k, hs.data(), off.data(), eact.data(), eseq.data(), flags, nullptr,
                                              rng.data(), log.data(), total, &total);
            }
            if (rc) return rc;
            for (uint32_t j = 0; j < k; j++) {
                std::string &o = js[idx[j]];
                o = "[";
                for (uint32_t r = 0; r < rng[2 * j + 1]; r++) { if (r) o += ','; o += std::to_string(log[rng[2 * j] + r]); }
                o += ']';
            }
        }
        *out = json_array(js);
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_missing_changes");
    }
}

int hm_docset_fields(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *entry_off, const char *actor_ids,
                     const uint32_t *actor_off, const double *seqs, const uint32_t *field_off, const char *names,
                     const uint32_t *name_off, hm_text **out) {
    if (!ds || !out || (n && (!docs || !entry_off || !field_off))) return HM_ERR_INVALID;
    *out = nullptr;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    try {
        int rc = check_request(ds, n, docs, entry_off);
        if (rc) return rc;
        for (uint32_t i = 0; i < n; i++)
            if (field_off[i + 1] < field_off[i]) return hm_engine_fail(ds->e, HM_ERR_INVALID, "field_off must not decrease");
        if (n && entry_off[n] - entry_off[0] && (!actor_ids || !actor_off || !seqs)) return HM_ERR_INVALID;
        if (n && field_off[n] - field_off[0] && (!names || !name_off)) return HM_ERR_INVALID;
        const Clocks clocks{ds, entry_off, actor_ids, actor_off, seqs};
        for (uint32_t i = 0; i < n; i++) {
            if ((rc = clocks.check(i))) return rc;
            for (uint32_t f = 2 * field_off[i]; f < 2 * field_off[i + 1]; f++)
                if (name_off[f + 1] < name_off[f]) return hm_engine_fail(ds->e, HM_ERR_INVALID, "name_off must not decrease");
        }
        // a request with no device rows: every field empty
        auto plain = [&](uint32_t i, bool ready) {
            std::string o = ready ? "{\"ready\":true,\"fields\":[" : "{\"ready\":false,\"fields\":[";
            for (uint32_t f = field_off[i]; f < field_off[i + 1]; f++) { if (f > field_off[i]) o += ','; o += "[]"; }
            return o + "]}";
        };
        std::vector<std::string> js(n);
        for (uint32_t i = 0; i < n; i++) {                       // (a document not placed yet: nothing applied)
            if (ds->doc(docs[i]).cls != NO_CLASS) continue;
            bool ready = true;
            for (uint32_t k = entry_off[i]; k < entry_off[i + 1]; k++) ready = ready && seq_u32(seqs[k]) == 0u;
            js[i] = plain(i, ready);
        }
        for (uint32_t c = 0; c < N_CLASS; c++) {
            std::vector<uint32_t> idx, hs, eoff(1, 0), eseq, foff(1, 0), freg, fmap;
            std::vector<uint16_t> eact;
            for (uint32_t i = 0; i < n; i++) {
                const DocSt &d = ds->doc(docs[i]);
                if (d.cls != c) continue;
                bool ready = true;
                if ((rc = clocks.sparse(i, d, eact, eseq, &ready))) return rc;
                if (!ready) { js[i] = plain(i, false); continue; }
                idx.push_back(i); hs.push_back(d.handle);
                eoff.push_back((uint32_t)eact.size());
                for (uint32_t f = field_off[i]; f < field_off[i + 1]; f++) {
                    const uint32_t *no = name_off + 2 * (size_t)f;
                    const uint32_t obj = d.objs.find(names + no[0], no[1] - no[0], 0);
                    const uint32_t reg = obj == HM_NONE ? HM_NONE : d.regs.find(names + no[1], no[2] - no[1], obj);
                    fmap.push_back(reg == HM_NONE ? HM_NONE : (uint32_t)freg.size());     // (unknown: an empty field, not sent)
                    if (reg != HM_NONE) freg.push_back(reg);
                }
                foff.push_back((uint32_t)freg.size());
            }
            if (idx.empty()) continue;
            const uint32_t k = (uint32_t)idx.size();
            std::vector<uint32_t> flags(k), rng(2 * freg.size() + 2);
            std::vector<hm_field_op> rows(std::max<size_t>(64, 2 * freg.size()));
            uint32_t total = 0;
            eact.push_back(0); eseq.push_back(0); freg.push_back(0);             // (never empty tables)
            rc = hm_store_fields(ds->stores[c], k, hs.data(), eoff.data(), eact.data(), eseq.data(), foff.data(), freg.data(),
                                 flags.data(), nullptr, rng.data(), rows.data(), (uint32_t)rows.size(), &total);
            if (rc == HM_ERR_NOMEM && total > rows.size()) {      // (the guess was too small: now with the reported size)
                rows.resize(total);
                rc = hm_store_fields(ds->stores[c], k, hs.data(), eoff.data(), eact.data(), eseq.data(), foff.data(), freg.data(),
                                     flags.data(), nullptr, rng.data(), rows.data(), total, &total);
            }
            if (rc) return rc;
            size_t fm = 0;
            for (uint32_t j = 0; j < k; j++) {
                const uint32_t i = idx[j];
                const DocSt &d = ds->doc(docs[i]);
                if (flags[j] & HM_FLD_BAD_ROWS) return hm_engine_fail(ds->e, HM_ERR_INVALID, "a survivor outside its document's changes");
                std::string &o = js[i];
                o = (flags[j] & HM_FLD_NOT_READY) ? "{\"ready\":false,\"fields\":[" : "{\"ready\":true,\"fields\":[";
                for (uint32_t f = field_off[i]; f < field_off[i + 1]; f++, fm++) {
                    if (f > field_off[i]) o += ',';
                    o += '[';
                    const uint32_t g = fmap[fm];
                    for (uint32_t r = 0; g != HM_NONE && r < rng[2 * g + 1]; r++) {
                        const hm_field_op &p = rows[rng[2 * g] + r];
                        if (r) o += ',';
                        o += p.action == HM_LINK ? "{\"action\":\"link\",\"value\":" : "{\"action\":\"set\",\"value\":";
                        const uint32_t id = (uint32_t)p.value;
                        switch (p.vtag) {
                        case HM_V_FALSE: o += "false"; break;
                        case HM_V_TRUE: o += "true"; break;
                        case HM_V_INT: case HM_V_FLOAT: jnum(o, p.vtag, p.value); break;
                        case HM_V_STR: if (id < d.strs.size()) jstr(o, d.strs.ptr(id), d.strs.len(id)); else o += "null"; break;
                        case HM_V_OBJ: if (id < d.objs.size()) jstr(o, d.objs.ptr(id), d.objs.len(id)); else o += "null"; break;
                        default: o += "null";
                        }
                        if (p.datatype == HM_DT_COUNTER) o += ",\"datatype\":\"counter\"";
                        else if (p.datatype == HM_DT_TIMESTAMP) o += ",\"datatype\":\"timestamp\"";
                        o += ",\"actor\":";
                        if (p.actor < d.by_rank.size()) { const uint32_t a = d.by_rank[p.actor]; jstr(o, d.actors.ptr(a), d.actors.len(a)); }
                        else o += "null";
                        o += ",\"seq\":" + std::to_string(p.seq) + (p.covered ? ",\"covered\":true}" : ",\"covered\":false}");
                    }
                    o += ']';
                }
                o += "]}";
            }
        }
        *out = json_array(js);
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_fields");
    }
}

int hm_docset_materialize(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *hist_len, const uint32_t *entry_off,
                          const char *actor_ids, const uint32_t *actor_off, const double *seqs, hm_text **out) {
    if (!ds || !out || (n && !docs)) return HM_ERR_INVALID;
    *out = nullptr;
    if ((hist_len != nullptr) == (entry_off != nullptr))
        return hm_engine_fail(ds->e, HM_ERR_INVALID, "exactly one of hist_len and the clock entries");
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    try {
        int rc = check_request(ds, n, docs, entry_off);
        if (rc) return rc;
        if (entry_off && n && entry_off[n] - entry_off[0] && (!actor_ids || !actor_off || !seqs)) return HM_ERR_INVALID;
        const Clocks clocks{ds, entry_off, actor_ids, actor_off, seqs};
        std::vector<std::string> js(n);
        for (uint32_t i = 0; i < n; i++) {                       // (a document not placed yet: Backend.init())
            DocSt &d = ds->doc(docs[i]);
            if (d.cls != NO_CLASS) continue;
            if (!d.ready) d.setup();
            js[i] = "{\"doc\":" + std::to_string(docs[i]) + ",\"clock\":{},\"deps\":{},\"history\":0,\"view\":";
            render_view(js[i], d, nullptr, nullptr, 0);
            js[i] += '}';
        }
        for (uint32_t c = 0; c < N_CLASS; c++) {
            const uint32_t S = STRIDES[c];
            std::vector<uint32_t> idx, hs;
            Selector sel;
            class_docs(ds, c, n, docs, idx, hs);
            if (idx.empty()) continue;
            if ((rc = clocks.select(docs, hist_len, idx, S, sel))) return rc;
            const uint32_t k = (uint32_t)idx.size();
            PastTables T;                                        // (one count pass per class)
            T.k = k; T.S = S;
            if ((rc = hm_store_materialize_sized(ds->stores[c], k, hs.data(), sel.lens(), sel.rows(), PastTables::alloc, &T, nullptr))) return rc;
            std::vector<uint8_t> created;
            for (uint32_t j = 0; j < k; j++) {
                DocSt &d = ds->doc(docs[idx[j]]);
                if (!d.ready) d.setup();
                const hm_doc_row &r = T.rows_d[j];
                std::string &o = js[idx[j]];
                o = "{\"doc\":" + std::to_string(docs[idx[j]]) + ",\"clock\":";
                jclock(o, d, T.clock.data() + (size_t)j * S, std::min<size_t>(d.actors.size(), S));
                o += ",\"deps\":";
                jclock(o, d, T.heads.data() + (size_t)j * S, std::min<size_t>(d.actors.size(), S));
                o += ",\"history\":" + std::to_string(T.res[j].hist_len) + ",\"view\":";
                if (T.res[j].status != HM_OK) { o += "null}"; continue; }
                // the objects the gathered ops create, and the survivors' ops as the document's own log indices
                created.assign(std::max<size_t>(d.obj_type.size(), 1), 0);
                created[0] = 1;
                for (uint32_t x = r.op_off; x < r.op_off + r.n_ops; x++)
                    if (T.ops[x].action <= HM_MAKE_TEXT && T.ops[x].obj < created.size()) created[T.ops[x].obj] = 1;
                const uint32_t ns = std::min(T.res[j].n_surv, r.n_ops);
                for (uint32_t x = 0; x < ns; x++) {
                    hm_surv_result &sv = T.surv[r.op_off + x];
                    sv.op = sv.op < r.n_ops ? T.op_log[r.op_off + sv.op] : HM_NONE;
                }
                render_view(o, d, T.regs.data() + r.reg_off, T.surv.data() + r.op_off,
                            std::min<uint32_t>(r.n_regs, (uint32_t)d.regs.size()), created.data());
                o += '}';
            }
        }
        *out = json_array(js);
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_materialize");
    }
}

int hm_docset_fork(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *hist_len, const uint32_t *entry_off,
                   const char *actor_ids, const uint32_t *actor_off, const double *seqs, uint32_t *out_first, hm_text **out) {
    if (!ds || !out || !out_first || (n && !docs)) return HM_ERR_INVALID;
    *out = nullptr;
    if ((hist_len != nullptr) == (entry_off != nullptr))
        return hm_engine_fail(ds->e, HM_ERR_INVALID, "exactly one of hist_len and the clock entries");
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "hm_docset_fork: another call on this docset is running");
    if (ds->broken)
        return hm_engine_fail(ds->e, HM_ERR_DEVICE, "hm_docset_fork: an earlier failed call could not be undone on its store");
    try {
        int rc = check_request(ds, n, docs, entry_off);
        if (rc) return rc;
        if (entry_off && n && entry_off[n] - entry_off[0] && (!actor_ids || !actor_off || !seqs)) return HM_ERR_INVALID;
        uint32_t first = 0;
        if ((rc = hm_docset_open(ds, n, &first))) return rc;
        std::unique_ptr<hm_text> t(new hm_text());
        if ((rc = fork_docs(ds, n, docs, hist_len, entry_off, actor_ids, actor_off, seqs, first, t.get()))) return rc;
        *out_first = first;
        *out = t.release();
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_fork");
    }
}

int hm_docset_merge_from(hm_docset *ds, uint32_t n, const uint32_t *dst_docs, const uint32_t *src_docs, const uint32_t *entry_off,
                         const char *actor_ids, const uint32_t *actor_off, const double *seqs, hm_text **out) {
    if (!ds || !out || !n || !dst_docs || !src_docs || !entry_off) return HM_ERR_INVALID;
    *out = nullptr;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "hm_docset_merge_from: another call on this docset is running");
    if (ds->broken)
        return hm_engine_fail(ds->e, HM_ERR_DEVICE, "hm_docset_merge_from: an earlier failed call could not be undone on its store");
    try {
        int rc = check_request(ds, n, src_docs, entry_off);
        if (rc) return rc;
        if (entry_off[n] - entry_off[0] && (!actor_ids || !actor_off || !seqs)) return HM_ERR_INVALID;
        std::unique_ptr<hm_text> t(new hm_text());
        const uint64_t before[2] = {ds->mstat[0], ds->mstat[1]};
        if ((rc = merge_docs(ds, n, dst_docs, src_docs, entry_off, actor_ids, actor_off, seqs, t.get()))) {
            ds->mstat[0] = before[0]; ds->mstat[1] = before[1];
            return rc;
        }
        *out = t.release();
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_merge_from");
    }
}

int hm_docset_merge_stats(const hm_docset *ds, uint64_t *out2) {
    if (!ds || !out2) return HM_ERR_INVALID;
    out2[0] = ds->mstat[0]; out2[1] = ds->mstat[1];
    return HM_OK;
}

int hm_docset_materialize_patch(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *hist_len, hm_text **out) {
    return hm_docset_materialize_patch_ex(ds, n, docs, hist_len, 0u, out);
}

static int materialize_patch(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *hist_len, const uint32_t *entry_off,
                             const char *actor_ids, const uint32_t *actor_off, const double *seqs, uint32_t opts, hm_text **out);

int hm_docset_materialize_patch_ex(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *hist_len, uint32_t opts, hm_text **out) {
    if (!ds || !out || (n && (!docs || !hist_len)) || (opts & ~HM_ODF_LISTS)) return HM_ERR_INVALID;
    return materialize_patch(ds, n, docs, hist_len, nullptr, nullptr, nullptr, nullptr, opts, out);
}

int hm_docset_materialize_patch_at(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *entry_off, const char *actor_ids,
                                   const uint32_t *actor_off, const double *seqs, uint32_t opts, hm_text **out) {
    if (!ds || !out || !entry_off || (n && !docs) || (opts & ~HM_ODF_LISTS)) return HM_ERR_INVALID;
    return materialize_patch(ds, n, docs, nullptr, entry_off, actor_ids, actor_off, seqs, opts, out);
}

// hm_docset_materialize_patch_ex (a history length per request) and _at (entry_off != NULL: a clock per
// request, as hm_docset_materialize takes it; the reply then carries "queued" too)
static int materialize_patch(hm_docset *ds, uint32_t n, const uint32_t *docs, const uint32_t *hist_len, const uint32_t *entry_off,
                             const char *actor_ids, const uint32_t *actor_off, const double *seqs, uint32_t opts, hm_text **out) {
    *out = nullptr;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    try {
        int rc = check_request(ds, n, docs, entry_off);
        if (rc) return rc;
        if (entry_off && n && entry_off[n] - entry_off[0] && (!actor_ids || !actor_off || !seqs)) return HM_ERR_INVALID;
        if (n && !(ds->patches && ds->op_diffs))
            return hm_engine_fail(ds->e, HM_ERR_UNSUPPORTED, "hm_docset_materialize_patch renders per-op diffs: not with HM_DOCSET_NO_PATCHES / HM_DOCSET_NET_DIFFS");
        const Clocks clocks{ds, entry_off, actor_ids, actor_off, seqs};
        static const char TAIL[] = ",\"canUndo\":false,\"canRedo\":false,\"diffs\":[";
        std::vector<std::string> js(n);
        for (uint32_t i = 0; i < n; i++)                         // (a document not placed yet: Backend.init())
            if (ds->doc(docs[i]).cls == NO_CLASS)
                js[i] = "{\"doc\":" + std::to_string(docs[i]) + ",\"history\":0," + (entry_off ? "\"queued\":0," : "") +
                        "\"patch\":{\"clock\":{},\"deps\":{}" + TAIL + "]}}";
        for (uint32_t c = 0; c < N_CLASS; c++) {
            const uint32_t S = STRIDES[c];
            std::vector<uint32_t> idx, hs;
            Selector sel;
            class_docs(ds, c, n, docs, idx, hs);
            if (idx.empty()) continue;
            if ((rc = clocks.select(docs, hist_len, idx, S, sel))) return rc;
            const uint32_t k = (uint32_t)idx.size(), *hl = sel.v.data();       // (hl: the history lengths, or the clock rows)
            PastTables T;                                        // the selection's clock and deps: its merge from Backend.init()
            T.k = k; T.S = S;
            if ((rc = hm_store_materialize_sized(ds->stores[c], k, hs.data(), sel.lens(), sel.rows(),
                                                 PastTables::alloc_heads, &T, nullptr))) return rc;
            // the diffs: what each op of the selection did, from the resident tables
            const std::vector<uint32_t> from(hist_len ? k : 0u, 0u);
            uint64_t tot[2] = {0, 0};
            if ((rc = hist_len ? hm_store_op_diff_sizes_ex(ds->stores[c], k, hs.data(), from.data(), hl, nullptr, nullptr, tot, opts)
                               : hm_store_op_diff_sizes_at(ds->stores[c], k, hs.data(), hl, nullptr, nullptr, tot, opts))) return rc;
            if (tot[0] > 0xFFFFFFFFull || tot[1] > 0xFFFFFFFFull) return hm_engine_fail(ds->e, HM_ERR_NOMEM, "a call's rows stay below 2^32");
            std::vector<hm_op_diff> rows(tot[0] + 1);
            std::vector<hm_surv_result> surv(tot[1] + 1);
            std::vector<uint32_t> range(2 * (size_t)k), flags(k), index(tot[0] + 1);   // (index: element rows, HM_ODF_LISTS)
            hm_op_diff_out po = {(uint32_t)tot[0], (uint32_t)tot[1], rows.data(), surv.data(), range.data(), flags.data()};
            if ((rc = hist_len ? hm_store_op_diffs_ex(ds->stores[c], k, hs.data(), from.data(), hl, &po, index.data(), nullptr, opts)
                               : hm_store_op_diffs_at(ds->stores[c], k, hs.data(), hl, &po, index.data(), nullptr, opts))) return rc;
            for (uint32_t j = 0; j < k; j++) {
                DocSt &d = ds->doc(docs[idx[j]]);
                if (!d.ready) d.setup();
                std::string &o = js[idx[j]];
                o = "{\"doc\":" + std::to_string(docs[idx[j]]) + ",\"history\":" + std::to_string(T.res[j].hist_len);
                if (!hist_len) o += ",\"queued\":" + std::to_string(T.res[j].n_queued);
                o += ",\"patch\":";
                if (flags[j] & HM_OD_LISTS) { o += "null,\"host\":true}"; continue; }   // (list / text elements: the caller replays)
                if (T.res[j].status != HM_OK) { o += "null}"; continue; }
                o += "{\"clock\":";
                jclock(o, d, T.clock.data() + (size_t)j * S, std::min<size_t>(d.actors.size(), S));
                o += ",\"deps\":";
                jclock(o, d, T.heads.data() + (size_t)j * S, std::min<size_t>(d.actors.size(), S));
                o += TAIL;
                JsonW w{o, d};
                if (const char *err = render_op_rows(w, d, rows.data(), index.data(), surv.data(), range[2 * j], range[2 * j + 1]))
                    return hm_engine_fail(ds->e, HM_ERR_INVALID, err);
                o += "]}}";
            }
        }
        *out = json_array(js);
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_materialize_patch");
    }
}

namespace {

// The state rows of one document (hm_store_state) placed for rendering, by render_view's rules: a
// keyed row goes to its object's keys in register order (the rows' order); on a list / text object
// a row without an index (a detached element) is dropped and the others are placed at
// elems[index], no sort.  keys / elems hold row numbers.
struct StateView {
    std::vector<std::vector<uint32_t>> keys, elems;
    std::vector<uint32_t> n_el;
    // NULL, or why the rows are not a merge's: an index at or past its object's elements, a slot filled twice
    const char *place(const DocSt &d, const hm_state_row *rows, uint32_t n) {
        const size_t no = d.obj_type.size();
        keys.assign(no, {}); elems.assign(no, {}); n_el.assign(no, 0);
        auto usable = [&](const hm_state_row &r) { return r.obj < no && r.reg < d.regs.size(); };
        auto is_list = [&](uint32_t ob) { return d.obj_type[ob] == HM_MAKE_LIST || d.obj_type[ob] == HM_MAKE_TEXT; };
        for (uint32_t i = 0; i < n; i++)
            if (usable(rows[i]) && is_list(rows[i].obj) && rows[i].index >= 0) n_el[rows[i].obj]++;
        for (size_t ob = 0; ob < no; ob++) if (n_el[ob]) elems[ob].assign(n_el[ob], HM_NONE);
        for (uint32_t i = 0; i < n; i++) {
            const hm_state_row &r = rows[i];
            if (!usable(r)) continue;
            if (!is_list(r.obj)) { keys[r.obj].push_back(i); continue; }
            if (r.index < 0) continue;
            if ((uint32_t)r.index >= n_el[r.obj]) return "a list element's index at or past its object's elements";
            if (elems[r.obj][r.index] != HM_NONE) return "two list elements at one index";
            elems[r.obj][r.index] = i;
        }
        return nullptr;
    }
    bool shown(const DocSt &d, uint32_t ob) const { return d.obj_type[ob] != NO_TYPE || !keys[ob].empty() || !elems[ob].empty(); }
};

// render_view's text from placed state rows (surv: the call's survivor table)
void render_state_view(std::string &o, const DocSt &d, const StateView &V, const hm_state_row *rows, const hm_surv_result *surv) {
    o += '{';
    const size_t start = o.size();
    for (uint32_t ob = 0; ob < d.obj_type.size(); ob++) {
        if (!V.shown(d, ob)) continue;
        if (o.size() > start) o += ',';
        jstr(o, d.objs.ptr(ob), d.objs.len(ob));
        const uint8_t t = d.obj_type[ob] == NO_TYPE ? HM_MAKE_MAP : d.obj_type[ob];
        o += ":{\"type\":\""; o += TYPE_NAME[t & 3]; o += "\",\"keys\":[";
        for (size_t i = 0; i < V.keys[ob].size(); i++) {
            const hm_state_row &r = rows[V.keys[ob][i]];
            if (i) o += ',';
            o += '[';
            jstr(o, d.regs.ptr(r.reg), d.regs.len(r.reg));
            o += ",{";
            jentry(o, d, surv + r.surv_off, r.n_surv);
            o += "}]";
        }
        o += "],\"elems\":[";
        for (size_t i = 0; i < V.elems[ob].size(); i++) {
            const hm_state_row &r = rows[V.elems[ob][i]];
            if (i) o += ',';
            o += '[';
            jstr(o, d.regs.ptr(r.reg), d.regs.len(r.reg));
            o += ",{";
            jentry(o, d, surv + r.surv_off, r.n_surv);
            o += "}]";
        }
        o += "]}";
    }
    o += '}';
}

// Backend.getPatch's diffs from placed state rows: a create for every object of the view but ROOT, in
// view order, then per object its sets in key order and its inserts in element order
void render_state_diffs(std::string &o, const DocSt &d, const StateView &V, const hm_state_row *rows, const hm_surv_result *surv) {
    JsonW w{o, d};
    o += '[';
    for (uint32_t ob = 1; ob < d.obj_type.size(); ob++)
        if (V.shown(d, ob)) w.create(ob, d.obj_type[ob] == NO_TYPE ? HM_MAKE_MAP : d.obj_type[ob]);
    for (uint32_t ob = 0; ob < d.obj_type.size(); ob++) {
        if (!V.shown(d, ob)) continue;
        const uint8_t t = d.obj_type[ob] == NO_TYPE ? HM_MAKE_MAP : d.obj_type[ob];
        for (uint32_t i : V.keys[ob]) w.map_set(t, ob, rows[i].reg, surv + rows[i].surv_off, rows[i].n_surv);
        for (uint32_t x = 0; x < V.elems[ob].size(); x++) {
            const hm_state_row &r = rows[V.elems[ob][x]];
            w.list_insert(t, ob, x, r.reg, surv + r.surv_off, r.n_surv);
        }
    }
    o += ']';
}

// hm_docset_views (patch = false) and hm_docset_get_patch (patch = true): one hm_store_state call per
// stride class, the documents rendered on the docset's host threads
int docset_states(hm_docset *ds, uint32_t n, const uint32_t *docs, bool patch, hm_text **out) {
    int rc = check_request(ds, n, docs);
    if (rc) return rc;
    std::vector<std::string> js(n);
    auto head = [&](std::string &o, uint32_t doc, uint32_t hist) {
        o = "{\"doc\":" + std::to_string(doc) + ",\"history\":" + std::to_string(hist) + ",\"patch\":{\"clock\":";
    };
    const char *mid = ",\"canUndo\":false,\"canRedo\":false,\"diffs\":";
    for (uint32_t i = 0; i < n; i++) {                           // (a document not placed yet: Backend.init())
        DocSt &d = ds->doc(docs[i]);
        if (!d.ready) d.setup();
        if (d.cls != NO_CLASS) continue;
        StateView V;
        V.place(d, nullptr, 0);
        if (patch) {
            head(js[i], docs[i], 0);
            js[i] += "{},\"deps\":{}"; js[i] += mid;
            render_state_diffs(js[i], d, V, nullptr, nullptr);
            js[i] += "}}";
        } else render_state_view(js[i], d, V, nullptr, nullptr);
    }
    for (uint32_t c = 0; c < N_CLASS; c++) {
        const uint32_t S = STRIDES[c];
        std::vector<uint32_t> idx, hs;
        class_docs(ds, c, n, docs, idx, hs);
        if (idx.empty()) continue;
        const uint32_t k = (uint32_t)idx.size();
        // the tables sized by what the host knows of the documents: a live register is one of the
        // document's, a survivor one of its ops (the call's totals, should they be larger)
        uint64_t cap[2] = {0, 0};
        for (uint32_t j = 0; j < k; j++) { const DocSt &d = ds->doc(docs[idx[j]]); cap[0] += d.regs.size(); cap[1] += d.n_ops; }
        std::vector<hm_state_row> rows;
        std::vector<hm_surv_result> surv;
        std::vector<uint32_t> range(4 * (size_t)k), flags(k), clock, heads;
        if (patch) { clock.resize((size_t)k * S); heads.resize((size_t)k * S); }
        for (int attempt = 0;; attempt++) {
            if (cap[0] > 0xFFFFFFFFull || cap[1] > 0xFFFFFFFFull) return hm_engine_fail(ds->e, HM_ERR_NOMEM, "the state of the request's documents exceeds 2^32 rows");
            rows.resize(cap[0] + 1); surv.resize(cap[1] + 1);
            const hm_state_out so = {(uint32_t)cap[0], (uint32_t)cap[1], rows.data(), surv.data(), range.data(), flags.data()};
            uint64_t tot[2] = {0, 0};
            rc = hm_store_state(ds->stores[c], k, hs.data(), &so, patch ? clock.data() : nullptr, patch ? heads.data() : nullptr, tot);
            if (rc == HM_ERR_NOMEM && attempt == 0 && (tot[0] > cap[0] || tot[1] > cap[1])) { cap[0] = tot[0]; cap[1] = tot[1]; continue; }
            if (rc) return rc;
            break;
        }
        std::atomic<const char *> bad{nullptr};
        par_for(k, std::min<uint32_t>(ds->threads, std::max<uint32_t>(1, k / 64)), [&](uint32_t lo, uint32_t hi, uint32_t) {
            StateView V;
            for (uint32_t j = lo; j < hi; j++) {
                const DocSt &d = ds->doc(docs[idx[j]]);
                if (flags[j] & HM_ST_BAD_ROWS) { bad = "register survivors outside the document's slots"; return; }
                const hm_state_row *r = rows.data() + range[4 * (size_t)j];
                const char *why = V.place(d, r, range[4 * (size_t)j + 1]);
                if (why) { bad = why; return; }
                std::string &o = js[idx[j]];
                if (patch) {
                    const uint32_t na = (uint32_t)std::min<size_t>(d.actors.size(), S);
                    head(o, docs[idx[j]], d.hist_len);
                    jclock(o, d, clock.data() + (size_t)j * S, na);
                    o += ",\"deps\":";
                    jclock(o, d, heads.data() + (size_t)j * S, na);
                    o += mid;
                    render_state_diffs(o, d, V, r, surv.data());
                    o += "}}";
                } else render_state_view(o, d, V, r, surv.data());
            }
        });
        if (bad.load()) return hm_engine_fail(ds->e, HM_ERR_DEVICE, bad.load());
    }
    *out = json_array(js);
    return HM_OK;
}

}  // namespace

int hm_docset_views(hm_docset *ds, uint32_t n, const uint32_t *docs, hm_text **out) {
    if (!ds || !out || (n && !docs)) return HM_ERR_INVALID;
    *out = nullptr;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    try {
        return docset_states(ds, n, docs, false, out);
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_views");
    }
}

int hm_docset_get_patch(hm_docset *ds, uint32_t n, const uint32_t *docs, hm_text **out) {
    if (!ds || !out || (n && !docs)) return HM_ERR_INVALID;
    *out = nullptr;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    try {
        return docset_states(ds, n, docs, true, out);
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_get_patch");
    }
}

int hm_docset_view(hm_docset *ds, uint32_t doc, hm_text **out) {
    if (!ds || !out || doc >= ds->n_docs.load()) return HM_ERR_INVALID;
    *out = nullptr;
    Busy b(ds);
    if (!b.ok) return hm_engine_fail(ds->e, HM_ERR_INVALID, "docset busy");
    try {
        DocSt &d = ds->doc(doc);
        if (!d.ready) d.setup();
        std::unique_ptr<hm_text> t(new hm_text());
        if (d.cls == NO_CLASS) {
            render_view(t->s, d, nullptr, nullptr, 0);
        } else {
            hm_doc_info_t inf;
            int rc = hm_doc_info(ds->stores[d.cls], d.handle, &inf);
            if (rc) return rc;
            std::vector<hm_reg_result> regs(inf.n_regs + 1);
            std::vector<hm_surv_result> surv(inf.n_ops + 1);
            rc = hm_doc_read(ds->stores[d.cls], d.handle, nullptr, nullptr, regs.data(), surv.data(), nullptr, nullptr, nullptr);
            if (rc) return rc;
            render_view(t->s, d, regs.data(), surv.data(), inf.n_regs);
        }
        *out = t.release();
        return HM_OK;
    } catch (...) {
        return hm_engine_fail(ds->e, HM_ERR_NOMEM, "exception in hm_docset_view");
    }
}

int hm_docset_handles(const hm_docset *ds, uint32_t a_stride, uint32_t *out_opened, uint32_t *out_free) {
    if (!ds || !out_opened || !out_free) return HM_ERR_INVALID;
    for (uint32_t c = 0; c < N_CLASS; c++)
        if (STRIDES[c] == a_stride) { *out_opened = ds->opened[c]; *out_free = (uint32_t)ds->free_h[c].size(); return HM_OK; }
    return HM_ERR_INVALID;
}

int hm_docset_routing(const hm_docset *ds, uint64_t *out3) {
    if (!ds || !out3) return HM_ERR_INVALID;
    for (int k = 0; k < 3; k++) out3[k] = ds->routing[k];
    return HM_OK;
}

int hm_docset_diff_stats(const hm_docset *ds, uint64_t *out4) {
    if (!ds || !out4) return HM_ERR_INVALID;
    for (int i = 0; i < 4; i++) out4[i] = ds->dstat[i];
    return HM_OK;
}

int hm_docset_stats(const hm_docset *ds, uint64_t *out8) {
    if (!ds || !out8) return HM_ERR_INVALID;
    for (int i = 0; i < 8; i++) out8[i] = ds->stat[i];
    return HM_OK;
}

}  // extern "C"
