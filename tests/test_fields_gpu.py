"""The fields a proposed change touches, on the device (hm_store_fields / hm_fields_host /
hm_fields_device) against tests/fields_ref.py applied to the CPU oracle's merge of the same log, bit
for bit: closure rows, ready flags, every row of every field, at the smallest shapes that take each
path of csrc/field_kernels.hip."""
import ctypes

import numpy as np
import pytest

from hypermerge_amd.columnar import CBatch, CResults, encode
from hypermerge_amd.engine import FIELD_OP_DT, EngineError, pack_entries, pack_fields
from hypermerge_amd.store import DocStore
import oracle.oracle as O

from fields_ref import doc_ref, rows_of
from kat_cases import ch, inc, ins, link, mk, s
from test_missing_changes_host import A, B, Cc, CHAIN, D

pytestmark = pytest.mark.gpu

NOMEM, INVALID = 34, 32


class Ref:
    """The restatement on the oracle's merge of a resident document's log (merged once per handle)."""

    def __init__(self, store):
        self.store, self.merged = store, {}

    def get(self, h):
        if h not in self.merged:
            b = self.store.enc[h].log_batch(self.store.S)
            self.merged[h] = (b, O.merge(b))
        return self.merged[h]

    def __call__(self, h, entries, regs):
        b, o = self.get(h)
        return doc_ref(b, o, 0, entries, regs)

    def clock(self, h):
        return self.get(h)[1].clock

    def n_regs(self, h):
        return int(self.get(h)[0].docs["n_regs"][0])


def check(store, ref, hs, have, fields, cap=None):
    """One call for all requests; flags, closure rows and every field's rows equal the restatement.
    Returns (rows, requests not ready, rows not covered)."""
    got, clo = store.fields_rows(hs, have, fields, cap)
    n_rows = n_late = n_unc = 0
    for j, h in enumerate(hs):
        ready, deps, want = ref(h, have[j], fields[j])
        assert got[j][0] == ready, (j, h, have[j])
        assert [int(x) for x in clo[j]] == deps, (j, h, have[j])
        assert [rows_of(f) for f in got[j][1]] == want, (j, h, have[j], fields[j])
        n_rows += sum(len(f) for f in want)
        n_late += not ready
        n_unc += sum(1 for f in want for r in f if not r[7])
    return n_rows, n_late, n_unc


def rand_have(rng, clock, n_actors, late=False):
    """entries over a random subset of the ranks, in random order, seqs from 0 to the clock (late: one
    of them one past it)"""
    k = int(rng.integers(0, n_actors + 1))
    ranks = [int(a) for a in rng.permutation(n_actors)[:k]]
    ents = [(a, int(rng.integers(0, int(clock[a]) + 1))) for a in ranks]
    if late and ents:
        a = ents[-1][0]
        ents[-1] = (a, int(clock[a]) + 1)
    return ents


def raw_call(store, hs, have, fields, cap, field_off=None):
    hs = np.ascontiguousarray(hs, np.uint32)
    n = len(hs)
    off, ea, es = pack_entries(have, n)
    foff, freg = pack_fields(fields, n)
    if field_off is not None:
        foff = np.array(field_off, np.uint32)
    nf = len(freg)
    flags = np.full(max(n, 1), 77, np.uint32)
    rng = np.full((nf + 1, 2), 77, np.uint32)
    rows = np.zeros(max(cap, 1), FIELD_OP_DT)
    tot = ctypes.c_uint32(77)
    st = store._L.hm_store_fields(store._h, n, hs.ctypes.data, off.ctypes.data, ea.ctypes.data, es.ctypes.data,
                                  foff.ctypes.data, freg.ctypes.data, flags.ctypes.data, None, rng.ctypes.data,
                                  rows.ctypes.data, cap, ctypes.byref(tot))
    return st, flags, rng, rows, tot.value


# ---- hand cases ---------------------------------------------------------------------------------
HAND_DOC = [ch(A, 1, {}, s("c", 1, datatype="counter"), mk("makeMap", "M"), link("m", "M")), ch(B, 1, {A: 1}, inc("c", 0.5)),
            ch(D, 1, {Cc: 1}, s("w", 1))]


def test_hand_cases_through_the_store(engine):
    store = DocStore(engine, a_stride=8)
    h, g = store.open(), store.open()
    res = store.apply([(h, CHAIN), (g, HAND_DOC)])
    assert (res.docs["status"] == 0).all()
    # the order-dependent closure (tests/test_fields_ref.py spells the answers out)
    got = store.fields([h, h, h], [{A: 2, B: 1}, {B: 1, A: 2}, {A: 3}], [[("00000000-0000-0000-0000-000000000000", "y")]] * 3)
    one = dict(op=2, action=5, datatype=0, vtag=3, value=3, actor=B, seq=3)
    assert got == [(True, [[dict(one, covered=False)]]), (True, [[dict(one, covered=True)]]), (False, [[]])]
    # an actor the document has never seen: dropped at seq 0, not ready above
    got = store.fields([h, h], [{"nobody": 0, B: 3}, {"nobody": 1, B: 3}], [[0], [0]])
    assert got[0][0] and len(got[0][1][0]) == 1 and got[1] == (False, [[]])
    # a counter turned FLOAT, a link, a register only a queued change names, one past n_regs, an unknown key
    ref = Ref(store)
    assert check(store, ref, [g, g, g, h], [[(1, 1)], [], [(3, 1)], [(0, 1)]], [[0, 1, 2, 3], [0, 1, 2, 3], [0], []]) == (4, 1, 2)
    got = store.fields([g], [{B: 1}], [[("00000000-0000-0000-0000-000000000000", "c"), ("00000000-0000-0000-0000-000000000000", "zz"), ("nope", "c")]])
    assert [len(f) for f in got[0][1]] == [1, 0, 0] and got[0][1][0][0]["vtag"] == 4


# ---- shapes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,n_actors", [(8, 7), (256, 200)])
def test_strides(engine, S, n_actors):
    """One and four closure columns per lane.  Every writer's first change sets one of five keys (up
    to 40 concurrent survivors per key: a request for all of them has more than 64 rows at S = 256), a
    change of the last writer has heard all of them, then second changes of some."""
    actors = [f"w{i:03d}" for i in range(n_actors - 1)]
    last = "zzzz"
    changes = [ch(last, 1, {a: 1 for a in actors}, s("all", 1))]
    changes += [ch(a, 1, {}, s("k%d" % (i % 5), i)) for i, a in enumerate(actors)]
    changes += [ch(a, 2, {last: 1}, s("late", i), s("k1", -i)) for i, a in enumerate(actors[::3])]
    changes.append(ch(last, 2, {actors[0]: 2}, s("all", 2)))
    store = DocStore(engine, a_stride=S)
    h, h2 = store.open(), store.open()
    res = store.apply([(h, changes), (h2, changes[1:4])])
    assert (res.docs["status"] == 0).all()
    ref = Ref(store)
    rng = np.random.default_rng(S)
    hs = [h, h2] * 10
    have = [rand_have(rng, ref.clock(x), len(store.enc[x].actors), late=j % 5 == 3) for j, x in enumerate(hs)]
    z = n_actors - 1                                    # rank of "zzzz"
    # w000:2 has heard zzzz:1 and through it every first change
    have[0], have[2], have[4] = [(z, 1)], [(0, 2), (z, 0), (1, 0)], [(1, 0), (z, 0), (0, 2)]
    # entries that are not causally closed, in both orders: zzzz:2 has heard w000:2; w000 listed after it is
    # SET back to 1 (w000:2's ops are not covered), listed before it ends at 2
    have[6], have[8] = [(z, 2), (0, 1)], [(0, 1), (z, 2)]
    have[1] = [(0, 2)]                                  # not ready: the second document has w000:1 only
    fields = [list(range(ref.n_regs(x) + 2)) for x in hs]
    rows, late, unc = check(store, ref, hs, have, fields)
    assert rows > (64 if S == 256 else 20) and late >= 1 and unc > 0
    assert ref(h, have[6], fields[0])[1] != ref(h, have[8], fields[0])[1]      # the order matters


def test_long_log_empty_changes_many_fields(engine):
    """A document of 150 changes (the locate strides them; every third has no op, so op_first repeats
    along the log) over 80 keys: a request with more than 64 fields, one with a register repeated, one
    with none; handles repeat."""
    changes = []
    for k in range(1, 76):
        ops_a = [] if k % 3 == 0 else [s("k%d" % (k % 80), k), s("k%d" % ((k * 7) % 80), -k)]
        ops_b = [] if k % 3 == 1 else [s("k%d" % ((k + 40) % 80), k + 1000)]
        changes += [ch(A, k, {B: k - 1} if k > 1 else {}, *ops_a), ch(B, k, {A: k - 1} if k % 5 == 0 else {}, *ops_b)]
    changes.append(ch(Cc, 1, {}))                                           # the log ends on an empty change
    store = DocStore(engine, a_stride=8)
    h = store.open()
    res = store.apply([(h, changes)])
    assert int(res.docs["status"][0]) == 0 and int(res.docs["hist_len"][0]) == 151
    ref = Ref(store)
    nr = ref.n_regs(h)
    assert nr > 64
    rng = np.random.default_rng(1)
    hs = [h] * 8
    have = [rand_have(rng, ref.clock(h), 3) for _ in hs]
    have[0], have[1] = [(0, 75), (1, 75)], [(1, 10)]
    fields = [list(range(nr)), list(range(nr))[::-1], [], [3, 3, 3], [nr, 0, nr + 1000, 0xFFFFFFFF]] + \
             [[int(x) for x in rng.integers(0, nr, size=5)] for _ in range(3)]
    rows, late, unc = check(store, ref, hs, have, fields)
    assert rows > 2 * 64 and late == 0 and unc > 0


def test_list_element_registers(engine):
    changes = [ch(A, 1, {}, mk("makeList", "L"), link("l", "L"), ins("L", "_head", 1), s("aaaa:1", "x", obj="L"),
                  ins("L", "aaaa:1", 2), s("aaaa:2", "y", obj="L")),
               ch(B, 1, {A: 1}, s("aaaa:1", "b", obj="L"), ins("L", "_head", 1), s("bbbb:1", "z", obj="L")),
               ch(A, 2, {}, s("aaaa:1", "a2", obj="L"), {"action": "del", "obj": "L", "key": "aaaa:2"})]
    store = DocStore(engine, a_stride=8)
    h = store.open()
    assert int(store.apply([(h, changes)]).docs["status"][0]) == 0
    ref = Ref(store)
    regs = list(range(ref.n_regs(h)))
    assert check(store, ref, [h] * 4, [[], [(0, 2)], [(1, 1)], [(1, 1), (0, 2)]], [regs] * 4)[0] >= 4 * 4
    got = store.fields([h], [{A: 2}], [[("L", "aaaa:1"), ("L", "aaaa:2"), ("L", "bbbb:1")]])[0]
    assert [[(o["actor"], o["covered"]) for o in f] for f in got[1]] == [[(B, False), (A, True)], [], [(B, False)]]


def test_incremental_and_remerge_stores_agree(engine):
    """Survivor rows written by the incremental kernels (mode 2) against the re-merge (mode 0)."""
    X, Y = DocStore(engine, a_stride=8), DocStore(engine, a_stride=8)
    X.set_incremental(2)
    Y.set_incremental(False)
    hs = [X.open() for _ in range(6)]
    assert [Y.open() for _ in range(6)] == hs
    rounds = [[ch(A, 1, {}, s("x", 1), s("c", 5, datatype="counter"))], [ch(B, 1, {}, s("x", 2), s("y", 2))],
              [ch(Cc, 1, {A: 1}, s("x", 3), inc("c", 2))], [ch(A, 2, {B: 1}, s("y", 4), s("x", 4))]]
    inc_n = 0
    for rd in rounds:
        for st in (X, Y):
            assert (st.apply([(h, rd) for h in hs]).docs["status"] == 0).all()
        inc_n += X.last_routing()["incremental"]
    assert inc_n > 0
    ref = Ref(X)
    rng = np.random.default_rng(5)
    have = [rand_have(rng, ref.clock(h), 3) for h in hs]
    fields = [[0, 1, 2, 3]] * len(hs)
    assert check(X, ref, hs, have, fields)[0] > 0
    gx, cx = X.fields_rows(hs, have, fields)
    gy, cy = Y.fields_rows(hs, have, fields)
    assert [[rows_of(f) for f in g[1]] for g in gx] == [[rows_of(f) for f in g[1]] for g in gy]
    np.testing.assert_array_equal(cx, cy)


# ---- the call itself ----------------------------------------------------------------------------
def test_cap_and_errors(engine):
    store = DocStore(engine, a_stride=8)
    h, g = store.open(), store.open()
    store.apply([(h, CHAIN), (g, HAND_DOC)])
    ref = Ref(store)
    req, have, fields = [h, g, h, g], [[], [(1, 1)], [(0, 3)], [(0, 1)]], [[0, 1], [0, 1, 2], [0, 1], [1, 9]]
    want = [ref(x, e, f) for x, e, f in zip(req, have, fields)]
    total = sum(len(f) for w in want for f in w[2])
    assert total == 2 + 2 + 0 + 1
    st, flags, rng, rows, tot = raw_call(store, req, have, fields, total - 1)
    assert st == NOMEM and tot == total
    assert [int(c) for c in rng[:9, 1]] == [len(f) for w in want for f in w[2]]
    assert [int(x) for x in flags] == [0, 0, 1, 0]
    st, flags, rng, rows, tot = raw_call(store, req, have, fields, total)
    assert st == 0 and tot == total and [int(x) for x in flags] == [0, 0, 1, 0]
    k = 0
    for w in want:
        for f in w[2]:
            assert rows_of(rows[int(rng[k, 0]):int(rng[k, 0]) + int(rng[k, 1])]) == f
            k += 1
    # the requests' blocks tile [0, total) in some order, fields in order inside a block
    spans = sorted((int(a), int(c)) for a, c in rng[:9] if c)
    assert spans[0][0] == 0 and all(spans[i][0] + spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))
    assert spans[-1][0] + spans[-1][1] == total
    assert int(rng[1, 0]) == int(rng[0, 0]) + int(rng[0, 1])
    # n == 0, and cap 0 with no row table
    assert raw_call(store, [], [], [], 0)[::4] == (0, 0)
    assert store._L.hm_store_fields(store._h, 1, np.array([h], np.uint32).ctypes.data, np.zeros(2, np.uint32).ctypes.data, None, None,
                                    np.array([0, 1], np.uint32).ctypes.data, np.zeros(1, np.uint32).ctypes.data,
                                    np.zeros(1, np.uint32).ctypes.data, None, np.zeros(2, np.uint32).ctypes.data, None, 0,
                                    ctypes.byref(ctypes.c_uint32())) == NOMEM
    before = [store.info(x) for x in (h, g)]
    for bad_req, bad_have, bad_fields, msg in (([h, 9999], [[], []], [[0], [0]], "bad handle"),
                                               ([h], [[(8, 1)]], [[0]], "rank"),
                                               ([g, h], [[], [(0, 1), (1, 1), (0, 2)]], [[0], [0]], "repeated")):
        assert raw_call(store, bad_req, bad_have, bad_fields, 64)[0] == INVALID
        with pytest.raises(EngineError, match=msg):
            store.fields_rows(bad_req, bad_have, bad_fields)
    assert raw_call(store, [h, g], [[], []], [[0, 1], [0]], 64, field_off=[0, 2, 1])[0] == INVALID     # field_off decreases
    assert raw_call(store, [h, g], [[], []], [[0, 1], [0]], 64, field_off=[1, 2, 3])[0] == INVALID
    assert [store.info(x) for x in (h, g)] == before                                               # the store unchanged
    assert check(store, ref, req, have, fields)[0] == total
    # a batch in flight
    store.submit([(h, [ch(A, 3, {}, s("x", 3))])])
    assert raw_call(store, req, have, fields, total)[0] == INVALID
    with pytest.raises(EngineError, match="in flight"):
        store.fields_rows(req, have, fields)
    store.wait()
    assert store.fields([h], [{A: 3}], [[1]])[0][1][0][0]["seq"] == 3


# ---- a merged cold batch ------------------------------------------------------------------------
def cold():
    bad = [ch(A, 1, {}, s("x", 1)), ch(A, 1, {}, s("x", 2)), ch(A, 3, {}, s("x", 3))]         # INCONSISTENT_SEQ
    lst = [ch(A, 1, {}, mk("makeList", "L"), link("l", "L"), ins("L", "_head", 1), s("aaaa:1", "x", obj="L")),
           ch(B, 1, {}, s("l", 7))]
    b = encode([CHAIN, bad, HAND_DOC, lst, []], 8)
    o = O.merge(b)
    assert [int(x) for x in o.docs["status"]] == [0, 1, 0, 0, 0]
    have = [[(0, 2), (1, 1)], [(0, 0)], [(1, 1)], [(1, 1)], []]
    fields = [[1, 0, 1], [0, 1], [0, 1, 2, 3], [0, 1, 0], [0]]
    return b, o, have, fields


def test_cold_batch_host(engine):
    b, o, have, fields = cold()
    r = engine.merge(b)
    n_rows = 0
    for hv in (have, [[(1, 1), (0, 2)], [(0, 1)], [], [(0, 1), (1, 1)], [(0, 1)]]):
        got, clo = engine.fields(b, r, hv, fields, closure=True)
        for d in range(b.n_docs):
            ready, deps, want = doc_ref(b, o, d, hv[d], fields[d])
            assert got[d][0] == ready and [int(x) for x in clo[d]] == deps, (d, hv[d])
            assert [rows_of(f) for f in got[d][1]] == want, (d, hv[d])
            n_rows += sum(len(f) for f in want)
        # the document whose merge threw: no rows, ready exactly when every seq is 0
        assert got[1][0] == (hv[1][0][1] == 0) and [len(f) for f in got[1][1]] == [0, 0]
    assert n_rows > 10
    # cap too small: the exact total, then success at that size
    total = sum(len(f) for d in range(b.n_docs) for f in doc_ref(b, o, d, have[d], fields[d])[2])
    with pytest.raises(EngineError, match="cap below"):
        engine.fields(b, r, have, fields, cap=0)
    assert sum(len(f) for g in engine.fields(b, r, have, fields, cap=total) for f in g[1]) == total
    with pytest.raises(EngineError, match="repeated"):
        engine.fields(b, r, [[(0, 1), (0, 2)], [], [], [], []], fields)


def test_cold_batch_device(engine):
    import torch
    b, o, have, fields = cold()
    r = engine.merge(b)
    n, S = b.n_docs, 8
    dev = torch.device("cuda", 0)
    off, ea, es = pack_entries(have, n)
    foff, freg = pack_fields(fields, n)
    nf = int(foff[-1])
    t = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
         for x in (b.docs, b.changes, b.deps, b.ops, r.docs, r.clock, r.hist, r.all_deps, r.regs, r.surv, off, ea, es, foff, freg)]
    cb = CBatch(n, len(b.changes), len(b.deps), len(b.ops), len(r.regs), S, 0, 0, 0, 0, 0, 0,
                t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), None)
    cr = CResults(t[4].data_ptr(), t[5].data_ptr(), None, None, t[6].data_ptr(), t[7].data_ptr(), t[8].data_ptr(), t[9].data_ptr())
    cap = 64
    z = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)
    flags, clo, rng, rows, cnt = z(n), z(n * S), z(2 * nf), z(cap * 6), z(2)
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    engine.fields_device(cb, cr, t[10].data_ptr(), t[11].data_ptr(), t[12].data_ptr(), int(off[-1]), t[13].data_ptr(),
                         t[14].data_ptr(), nf, flags.data_ptr(), clo.data_ptr(), rng.data_ptr(), rows.data_ptr(), cap,
                         cnt.data_ptr(), cnt.data_ptr() + 4, st)
    torch.cuda.synchronize()
    rg = rng.cpu().numpy().view(np.uint32).reshape(nf, 2)
    rw = rows.cpu().numpy().view(FIELD_OP_DT)
    fl = flags.cpu().numpy().view(np.uint32)
    cl = clo.cpu().numpy().view(np.uint32).reshape(n, S)
    total = 0
    for d in range(n):
        ready, deps, want = doc_ref(b, o, d, have[d], fields[d])
        assert (int(fl[d]) == 0) == ready and [int(x) for x in cl[d]] == deps
        for k, f in enumerate(want):
            a, c = rg[int(foff[d]) + k]
            assert rows_of(rw[int(a):int(a) + int(c)]) == f, (d, k)
            total += len(f)
    assert [int(x) for x in cnt.cpu().numpy()] == [total, 0]
    # the offsets are checked on the device: a field_off that decreases marks the call and writes no row
    bad_off = torch.from_numpy(np.array([0, 3, 5, 9, 12, 11], np.uint32).view(np.uint8).copy()).to(dev)
    cnt.zero_()
    rng.fill_(-1)
    torch.cuda.synchronize()
    engine.fields_device(cb, cr, t[10].data_ptr(), t[11].data_ptr(), t[12].data_ptr(), int(off[-1]), bad_off.data_ptr(),
                         t[14].data_ptr(), nf, flags.data_ptr(), clo.data_ptr(), rng.data_ptr(), rows.data_ptr(), cap,
                         cnt.data_ptr(), cnt.data_ptr() + 4, st)
    torch.cuda.synchronize()
    assert int(cnt.cpu().numpy()[1]) == 16
    rg = rng.cpu().numpy().view(np.uint32).reshape(nf, 2)
    assert [int(c) for c in rg[0:3, 1]] == [len(f) for f in doc_ref(b, o, 0, have[0], fields[0])[2]]       # request 0 is sound
