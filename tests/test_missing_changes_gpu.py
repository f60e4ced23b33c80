"""Which changes a peer lacks, on the device (hm_store_missing_changes / hm_missing_changes_*)
against Automerge 0.12 getMissingChanges restated in tests/missing_changes_ref.py and applied to the
CPU oracle's merge of the same log, against answers written out by hand, and against
hm_store_read_history for a have-clock recorded at an earlier round."""
import ctypes

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import CBatch, CResults, decode_doc, encode
from hypermerge_amd.engine import EngineError, pack_entries
from hypermerge_amd.store import DocStore
import oracle.oracle as O

from kat_cases import ch, s
from missing_changes_ref import ONLY_LISTED, RAW, doc_ref
from test_missing_changes_host import A, B, Cc, FOR_ACTOR, HAND, ranked
from test_store_gpu import split

pytestmark = pytest.mark.gpu

NOMEM, INVALID = 34, 32
TILE = 2048          # csrc/changes_kernels.hip CTILE: history positions per bitmap tile


class Ref:
    """The restatement on the oracle's merge of a resident document's log (merged once per handle)."""

    def __init__(self, store):
        self.store, self.merged = store, {}

    def __call__(self, h, entries, flags=0):
        if h not in self.merged:
            b = self.store.enc[h].log_batch(self.store.S)
            self.merged[h] = (b, O.merge(b))
        b, o = self.merged[h]
        return doc_ref(b, o, 0, entries, flags)

    def clock(self, h):
        self(h, [])
        return self.merged[h][1].clock


def rand_have(rng, clock, n_actors):
    """entries over a random subset of the ranks, in random order, seqs from 0 to one past the clock"""
    k = int(rng.integers(0, n_actors + 1))
    ranks = rng.permutation(n_actors)[:k]
    return [(int(a), int(rng.integers(0, int(clock[a]) + 2))) for a in ranks]


def check(store, ref, hs, have, flags=0):
    """One call for all requests; each block and closure row equals the restatement."""
    got, clo = store.missing_changes_rows(hs, have, flags)
    n_rows = 0
    for j, h in enumerate(hs):
        want, deps = ref(h, have[j], flags)
        assert got[j] == want, (j, h, have[j], flags)
        assert [int(x) for x in clo[j]] == deps, (j, h, have[j], flags)
        n_rows += len(want)
    return n_rows


def raw_call(store, hs, have, flags, cap):
    hs = np.ascontiguousarray(hs, np.uint32)
    n = len(hs)
    off, ea, es = pack_entries(have, n)
    rng = np.zeros((n, 2), np.uint32)
    out = np.full(max(cap, 1), 0xFFFFFFFF, np.uint32)
    tot = ctypes.c_uint32(77)
    st = store._L.hm_store_missing_changes(store._h, n, hs.ctypes.data, off.ctypes.data, ea.ctypes.data, es.ctypes.data,
                                           flags, None, rng.ctypes.data, out.ctypes.data, cap, ctypes.byref(tot))
    return st, rng, out, tot.value


def read_history(store, hs, frm, to):
    """hm_store_read_history: history.slice(frm, to) of each handle as log indices."""
    hs = np.ascontiguousarray(hs, np.uint32)
    f, t = np.ascontiguousarray(frm, np.uint32), np.ascontiguousarray(to, np.uint32)
    off = np.zeros(len(hs) + 1, np.uint32)
    np.cumsum(t - f, out=off[1:])
    out = np.zeros(max(int(off[-1]), 1), np.uint32)
    store._check(store._L.hm_store_read_history(store._h, len(hs), hs.ctypes.data, f.ctypes.data, t.ctypes.data,
                                                off.ctypes.data, out.ctypes.data, None), "hm_store_read_history")
    return [[int(x) for x in out[off[j]:off[j + 1]]] for j in range(len(hs))]


# ---- hand cases ---------------------------------------------------------------------------------
def test_hand_cases_through_the_store(engine):
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in HAND]
    res = store.apply([(h, c[1]) for h, c in zip(hs, HAND)])
    assert (res.docs["status"] == 0).all()
    for h, (name, _, queries) in zip(hs, HAND):
        for clock, flags, want in queries:
            assert store.missing_changes([h], [clock], flags)[0] == want, (name, clock, flags)
            if flags == 0:
                assert store.changes_since(h, clock) == want, (name, clock)
            elif flags == FOR_ACTOR:
                (actor, after), = clock.items()
                assert store.changes_for_actor(h, actor, after) == want, (name, clock)
    # every query of every case in one call per flags value
    for flags in (0, FOR_ACTOR, RAW):
        req = [(h, clock, want) for h, c in zip(hs, HAND) for clock, f, want in c[2] if f == flags]
        got = store.missing_changes([r[0] for r in req], [r[1] for r in req], flags)
        assert got == [r[2] for r in req], flags
    # an actor id the document has never seen names none of its changes
    assert store.changes_since(hs[0], {"nobody": 9}) == [1, 0]
    assert store.changes_for_actor(hs[0], "nobody") == []


def test_hand_cases_through_a_cold_batch(engine):
    import torch
    bad = [ch(A, 1, {}, s("x", 1)), ch(A, 1, {}, s("x", 2)), ch(A, 3, {}, s("x", 3))]         # INCONSISTENT_SEQ
    docs = [c[1] for c in HAND[:2]] + [bad] + [c[1] for c in HAND[2:]]
    cases = HAND[:2] + [("threw", bad, [({A: 0}, 0, []), ({}, 0, []), ({A: 0}, FOR_ACTOR, [])])] + HAND[2:]
    b = encode(docs, 8)
    o = O.merge(b)
    assert int(o.docs["status"][2]) == 1
    r = engine.merge(b)
    n = b.n_docs
    c0 = [int(x) for x in b.docs["change_off"]]
    for k in range(max(len(c[2]) for c in cases)):
        for flags in (0, FOR_ACTOR, RAW):
            # the k-th query of each document that has one with these flags, an empty clock for the rest
            have, want = [], []
            for d, (name, _, queries) in enumerate(cases):
                q = queries[k] if k < len(queries) and queries[k][1] == flags else None
                have.append(ranked(b.doc_actors[d], q[0]) if q else [])
                want.append(q[2] if q else doc_ref(b, o, d, [], flags)[0])
            got, clo = engine.missing_changes(b, r, have, flags, closure=True)
            assert got == want, (k, flags)
            for d in range(n):
                assert [int(x) for x in clo[d]] == doc_ref(b, o, d, have[d], flags)[1], (k, flags, d)
    # dense have rows (entries in rank order): the clock of each document's first change
    rows = np.zeros((n, 8), np.uint32)
    for d in range(n):
        c = b.changes[c0[d]]
        rows[d, int(c["actor"])] = int(c["seq"])
    have = [[(a, int(q)) for a, q in enumerate(rows[d]) if q] for d in range(n)]
    want = [doc_ref(b, o, d, have[d])[0] for d in range(n)]
    assert engine.missing_changes(b, r, rows) == want
    # the same from device tensors
    dev = torch.device("cuda", 0)
    off, ea, es = pack_entries(rows, n)
    t = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)
         for x in (b.docs, b.changes, b.deps, r.docs, r.hist, r.all_deps, off, ea, es)]
    cap = len(b.changes)
    out = torch.zeros(cap, dtype=torch.int32, device=dev)
    rng_t = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    clo_t = torch.zeros(n * 8, dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    cb = CBatch(n, len(b.changes), len(b.deps), len(b.ops), 0, 8, 0, 0, 0, 0, 0, 0,
                t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), None, None)
    cr = CResults(t[3].data_ptr(), None, None, None, t[4].data_ptr(), t[5].data_ptr(), None, None)
    torch.cuda.synchronize()
    engine.missing_changes_device(cb, cr, t[6].data_ptr(), t[7].data_ptr(), t[8].data_ptr(), int(off[-1]), 0,
                                  clo_t.data_ptr(), rng_t.data_ptr(), out.data_ptr(), cap, cnt.data_ptr(),
                                  cnt.data_ptr() + 4, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rg = rng_t.cpu().numpy().view(np.uint32).reshape(n, 2)
    lg = out.cpu().numpy().view(np.uint32)
    assert [[int(x) for x in lg[int(a):int(a) + int(c)]] for a, c in rg] == want
    assert [int(x) for x in cnt.cpu().numpy()] == [sum(len(w) for w in want), 0]
    np.testing.assert_array_equal(clo_t.cpu().numpy().view(np.uint32).reshape(n, 8),
                                  np.array([doc_ref(b, o, d, have[d])[1] for d in range(n)], np.uint32))


# ---- a C5 store fed in 4 rounds (shared, read-only once built) ------------------------------------
@pytest.fixture(scope="module")
def c5(engine):
    b = synth.generate(synth.config("C5", n_docs=40))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    rng = np.random.default_rng(11)
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in docs]
    parts = [split(c, 4, rng) for c in docs]
    clocks = [[{} for _ in hs]]                       # per round: each document's opSet.clock by actor id
    hist_len = [[0] * len(hs)]
    for rd in range(4):
        items = [(h, parts[i][rd]) for i, h in enumerate(hs) if rd == 0 or parts[i][rd]]
        res = store.apply(items)
        assert (res.docs["status"] == 0).all()
        ck, hl = list(clocks[-1]), list(hist_len[-1])
        for j, (h, _) in enumerate(items):
            ck[h] = {store.enc[h].actors[a]: int(q) for a, q in enumerate(res.clock[j]) if q}
            hl[h] = int(res.docs["hist_len"][j])
        clocks.append(ck)
        hist_len.append(hl)
    return store, hs, clocks, hist_len, Ref(store)


def test_slice_property_against_read_history(c5):
    """have = opSet.clock as recorded after round r: the answer is history.slice(hist_len then, now),
    read back through hm_store_read_history (no restatement involved)."""
    store, hs, clocks, hist_len, _ = c5
    now = hist_len[-1]
    grew = 0
    for r in range(len(clocks)):
        got = store.missing_changes(hs, [clocks[r][h] for h in hs])
        want = read_history(store, hs, [hist_len[r][h] for h in hs], [now[h] for h in hs])
        assert got == want, r
        grew += sum(1 for w in want if w)
    assert grew >= 60                                  # most documents gained history in most rounds
    assert store.missing_changes(hs, [{} for _ in hs]) == read_history(store, hs, [0] * len(hs), now)


def test_many_requests_repeated_handles(c5):
    """300 requests over 40 documents in one call (more than one workgroup), handles repeated, a
    different have-clock each."""
    store, hs, _, _, ref = c5
    rng = np.random.default_rng(3)
    req = [hs[int(x)] for x in rng.integers(0, len(hs), size=300)]
    have = [rand_have(rng, ref.clock(h), len(store.enc[h].actors)) for h in req]
    assert check(store, ref, req, have) > 300
    assert check(store, ref, req, have, RAW) > 300
    assert check(store, ref, req, have, ONLY_LISTED) > 100
    assert check(store, ref, req, have, FOR_ACTOR) > 100


# ---- shapes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n_actors", [(5, 5), (12, 9), (128, 70)])
def test_strides(engine, S, n_actors):
    """Strides that are no power of two, and 70 actors at stride 128 (the column loops pass one wave).
    Every writer's first change, a change of the last writer that has heard all of them, then second
    changes of some; the last writer's change arrives first and waits."""
    actors = [f"w{i:03d}" for i in range(n_actors - 1)]
    last = "zzzz"
    changes = [ch(last, 1, {a: 1 for a in actors}, s("all", 1))]
    changes += [ch(a, 1, {}, s("k%d" % (i % 5), i)) for i, a in enumerate(actors)]
    changes += [ch(a, 2, {last: 1}, s("late", i)) for i, a in enumerate(actors[::3])]
    store = DocStore(engine, a_stride=S)
    h, h2 = store.open(), store.open()
    res = store.apply([(h, changes), (h2, changes[1:4])])
    assert (res.docs["status"] == 0).all()
    ref = Ref(store)
    rng = np.random.default_rng(S)
    hs = [h, h2] * 12
    have = [rand_have(rng, ref.clock(x), len(store.enc[x].actors)) for x in hs]
    z = n_actors - 1                                    # rank of "zzzz"
    have[0], have[2], have[4] = [(z, 1)], [(0, 2)], [(0, 2), (z, 1), (n_actors - 2, 1)]
    assert ref(h, have[0])[0] == ref(h, [])[0][n_actors:]     # zzzz:1 closes over every first change
    assert check(store, ref, hs, have) > 0
    check(store, ref, hs, have, FOR_ACTOR)
    assert store.changes_since(h, {last: 1}) == list(range(n_actors, len(changes)))


def test_long_chain_spans_bitmap_tiles(engine):
    """One actor, 3000 changes, each pair delivered in reverse (log [A2, A1, A4, A3, ...], history
    A1 .. A3000): the lanes stride 3000 change rows, and 3000 history positions need two bitmap
    tiles of TILE = 2048."""
    n = 3000
    assert n > TILE
    changes = []
    for k in range(1, n + 1, 2):
        changes += [ch(A, k + 1, {}, s("x", k + 1)), ch(A, k, {}, s("x", k))]
    store = DocStore(engine, a_stride=8)
    h = store.open()
    res = store.apply([(h, changes)])
    assert int(res.docs["status"][0]) == 0 and int(res.docs["hist_len"][0]) == n
    log_of = lambda q: q - 2 if q % 2 == 0 else q            # log index of seq q
    ref = Ref(store)
    for after in (0, 1, 1000, TILE - 1, TILE, TILE + 1, n - 1, n, n + 5):
        want = [log_of(q) for q in range(after + 1, n + 1)]
        assert store.changes_since(h, {A: after}) == want, after
        assert store.changes_for_actor(h, A, after) == want, after
    assert ref(h, [(0, 1000)])[0] == [log_of(q) for q in range(1001, n + 1)]
    assert check(store, ref, [h] * 3, [[], [(0, 2500)], [(0, 64)]]) == 3000 + 500 + 2936


def test_empty_document(engine):
    store = DocStore(engine, a_stride=8)
    h, e = store.open(), store.open()
    store.apply([(h, HAND[0][1])])
    got, clo = store.missing_changes_rows([e, h, e], [[], [], [(0, 3), (7, 1)]])
    assert got == [[], [1, 0], []]
    assert [int(x) for x in clo[2]] == [3, 0, 0, 0, 0, 0, 0, 1]      # nothing to fold: the entries themselves
    assert store.changes_since(e, {A: 1}) == [] and store.changes_for_actor(e, A) == []


def test_incremental_and_remerge_stores_agree(engine):
    """State written by the incremental kernels (mode 2) against the re-merge (mode 0)."""
    b = synth.generate(synth.config("C4", n_docs=60))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    rng = np.random.default_rng(7)
    parts = [split(c, 4, rng) for c in docs]
    X, Y = DocStore(engine, a_stride=8), DocStore(engine, a_stride=8)
    X.set_incremental(2)
    Y.set_incremental(False)
    hs = [X.open() for _ in docs]
    assert [Y.open() for _ in docs] == hs
    ref = Ref(X)
    inc = 0
    for rd in range(4):
        items = [(h, parts[i][rd]) for i, h in enumerate(hs) if rd == 0 or parts[i][rd]]
        for st in (X, Y):
            assert (st.apply(items).docs["status"] == 0).all()
        inc += X.last_routing()["incremental"]
        assert Y.last_routing()["incremental"] == 0
    assert inc > 0
    req = hs * 3
    have = [rand_have(rng, ref.clock(h), len(X.enc[h].actors)) for h in req]
    assert check(X, ref, req, have) > 0
    gx, cx = X.missing_changes_rows(req, have)
    gy, cy = Y.missing_changes_rows(req, have)
    assert gx == gy
    np.testing.assert_array_equal(cx, cy)


def test_after_reset_and_moved_segments(engine):
    store = DocStore(engine, a_stride=8)
    h0, h1, h2 = store.open(), store.open(), store.open()
    first = [ch(A, 1, {}, s("x", 1)), ch(B, 1, {A: 1}, s("y", 1)), ch(A, 2, {B: 1}, s("x", 2))]
    store.apply([(h0, first), (h1, first), (h2, first)])
    store.reset([h1])
    # h0 outgrows its segments (they move), h1 starts again with another log
    more = [ch(A, k, {}, s("x", k)) for k in range(3, 80)] + [ch(Cc, 1, {A: 40}, s("z", 1))]
    res = store.apply([(h0, more), (h1, [ch(B, 2, {}, s("y", 2)), ch(B, 1, {}, s("y", 1))])])
    assert (res.docs["status"] == 0).all()
    assert store.info(h1)["n_changes"] == 2 and store.info(h0)["n_changes"] == 81
    ref = Ref(store)
    hs = [h0, h1, h2, h0, h1, h2, h0]
    have = [[(2, 1)], [(0, 1)], [(1, 1)], [(0, 50), (1, 1)], [], [(0, 2)], [(1, 1), (0, 10)]]
    assert check(store, ref, hs, have) > 0
    assert store.changes_since(h1, {}) == [1, 0]
    assert store.changes_since(h2, {B: 1}) == [2]
    assert store.changes_since(h0, {Cc: 1}) == list(range(41, 80))      # cccc:1 has heard aaaa:40 (aaaa:k is log k)


def test_after_a_rolled_back_round(engine):
    store = DocStore(engine, a_stride=8)
    h, h2 = store.open(), store.open()
    ok = [ch(A, 1, {}, s("x", 1)), ch(B, 1, {}, s("x", 2))]
    store.apply([(h, ok), (h2, ok)])
    bad = [ch(Cc, 1, {}, s("z", 5)), ch(A, 1, {}, s("x", 99))]            # seq 1 reused with new content
    r = store.apply([(h, bad), (h2, [ch(Cc, 1, {A: 1}, s("w", 1))])])
    assert r.docs["status"][0] == 1 and r.docs["status"][1] == 0
    assert store.changes_since(h, {}) == [0, 1] and store.changes_since(h, {A: 1}) == [1]
    assert store.changes_since(h, {Cc: 1}) == [0, 1]                      # (an actor the rolled-back round brought)
    assert store.changes_since(h2, {Cc: 1}) == [1]
    ref = Ref(store)
    assert check(store, ref, [h, h2, h], [[(0, 1)], [(2, 1), (1, 0)], [(1, 1), (0, 1)]]) > 0


# ---- the call itself ----------------------------------------------------------------------------
def test_cap_and_errors(engine):
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in HAND]
    store.apply([(h, c[1]) for h, c in zip(hs, HAND)])
    req = [hs[1], hs[0], hs[3], hs[1]]
    have = [[], [(0, 1)], [], [(1, 1)]]
    want = [[0, 1, 2, 3, 4], [0], [0, 3], [1, 2, 3, 4]]
    total = sum(len(w) for w in want)
    st, rng, out, tot = raw_call(store, req, have, 0, total - 1)
    assert st == NOMEM and tot == total
    assert [int(c) for c in rng[:, 1]] == [len(w) for w in want]
    st, rng, out, tot = raw_call(store, req, have, 0, total)
    assert st == 0 and tot == total
    assert [[int(x) for x in out[int(a):int(a) + int(c)]] for a, c in rng] == want
    # the blocks tile [0, total) in some order
    spans = sorted((int(a), int(c)) for a, c in rng)
    assert spans[0][0] == 0 and all(spans[i][0] + spans[i][1] == spans[i + 1][0] for i in range(3))
    assert spans[3][0] + spans[3][1] == total
    # n == 0
    st, _, _, tot = raw_call(store, [], [], 0, 0)
    assert st == 0 and tot == 0
    for bad_req, bad_have, msg in (([hs[0], 9999], [[], []], "bad handle"),
                                   ([hs[0]], [[(8, 1)]], "rank"),
                                   ([hs[1], hs[0]], [[], [(0, 1), (1, 1), (0, 2)]], "repeated")):
        assert raw_call(store, bad_req, bad_have, 0, 64)[0] == INVALID
        with pytest.raises(EngineError, match=msg):
            store.missing_changes_rows(bad_req, bad_have)
    assert raw_call(store, [hs[0]], [[]], 4, 64)[0] == INVALID            # an unknown flag
    # a batch in flight
    store.submit([(hs[0], [ch(A, 3, {}, s("x", 3))])])
    assert raw_call(store, req, have, 0, total)[0] == INVALID
    with pytest.raises(EngineError, match="in flight"):
        store.missing_changes(req[:1], [{}])
    store.wait()
    assert store.changes_since(hs[0], {A: 2}) == [2]
