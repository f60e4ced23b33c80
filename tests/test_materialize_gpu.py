"""Resident documents materialized at a past history point on the device (hm_store_past_sizes /
hm_store_materialize / hm_materialize_device): the gathered tables and both index maps against the
numpy restatement in tests/past_ref.py (pinned on the oracle by tests/test_past_ref.py), bit for bit,
and every result table against ``oracle.merge`` of the restatement's batch."""
import ctypes
import os
import re

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import (CHANGE_DT, DEP_DT, DOC_DT, DOC_RESULT_DT, OP_DT, REG_RESULT_DT, SURV_RESULT_DT,
                                     CBatch, CResults, Results, decode_doc)
from hypermerge_amd.engine import CPastOut, CPastSummary, EngineError
from hypermerge_amd.store import DocStore, RowStore, slice_changes
import oracle.oracle as O

from kat_cases import A, B, Cc, D, ch, d, inc, ins, link, mk, s
from past_ref import Source, clock_at, gather, hist_len, select, source_of
from test_gpu_parity import assert_same
from test_missing_changes_gpu import read_history

pytestmark = pytest.mark.gpu

NOMEM, INVALID = 34, 32
_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hypermerge_amd", "csrc", "past_kernels.h")
T = int(re.search(r"#define HM_PAST_TILE (\d+)u", open(_H).read()).group(1))     # history positions per bitmap tile


def same_bytes(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=str(what))
    assert got.tobytes() == want.tobytes(), what


def enc_source(store, h):
    """a DocStore document's log (from its host encoder) with the oracle's hist"""
    b = store.enc[h].log_batch(store.S)
    return source_of(b, O.merge(b).hist, 0)


def check(store, srcs, hs, history=None, clocks=None):
    """One materialize call: the gathered batch and the maps equal the restatement bit for bit, the
    result tables equal the oracle's merge of the restatement's batch.  Returns (batch, oracle results)."""
    b, r, clog, olog = store.materialize(hs, history=history, clocks=clocks)
    reqs = [(srcs[int(h)], None if history is None else int(history[i]), None if clocks is None else clocks[i])
            for i, h in enumerate(hs)]
    want, wclog, wolog = gather(reqs, store.S)
    for f in ("docs", "changes", "deps", "ops"):
        same_bytes(getattr(b, f), getattr(want, f), f)
    same_bytes(clog, wclog, "change_log")
    same_bytes(olog, wolog, "op_log")
    o = O.merge(want, threads=8)
    assert_same(want, r, o)
    cnt, tot = store.past_sizes(hs, history=history, clocks=clocks)
    np.testing.assert_array_equal(cnt, np.stack([want.docs[f] for f in ("n_changes", "n_deps", "n_ops", "n_regs")], 1))
    assert [int(x) for x in tot] == [len(want.changes), len(want.deps), len(want.ops), int(want.docs["n_regs"].sum())]
    return want, o


# ---- hand cases ---------------------------------------------------------------------------------
SHUFFLED = [ch(B, 2, {A: 2}, s("y", 2)), ch(A, 3, {B: 2}, s("x", 3), s("w", 1)), ch(A, 1, {}, s("x", 1)),
            ch(B, 1, {A: 1}, s("y", 1), d("x")), ch(A, 2, {B: 1}, s("x", 2)), ch(Cc, 1, {A: 3}, s("z", 1))]
QUEUED_DUP = [ch(A, 1, {}, s("x", 1)), ch(Cc, 1, {D: 1}, s("q", 9)), ch(A, 1, {}, s("x", 1)), ch(B, 1, {A: 1}, s("x", 2)),
              ch(A, 2, {}, s("k", 3))]
COUNTER = [ch(A, 1, {}, s("n", 10, datatype="counter")), ch(B, 1, {A: 1}, inc("n", 5)), ch(A, 2, {B: 1}, inc("n", -2)),
           ch(B, 2, {A: 2}, s("n", 1, datatype="counter")), ch(A, 3, {B: 2}, inc("n", 0.5))]
TEXT = [ch(A, 1, {}, mk("makeText", "T"), link("t", "T")), ch(A, 2, {}, ins("T", "_head", 1)),
        ch(A, 3, {}, s(f"{A}:1", "h", obj="T")), ch(B, 1, {A: 3}, ins("T", f"{A}:1", 1), s(f"{B}:1", "i", obj="T")),
        ch(A, 4, {B: 1}, d(f"{A}:1", obj="T")), ch(B, 2, {A: 4}, ins("T", "_head", 2), s(f"{B}:2", "!", obj="T"))]
HAND = [SHUFFLED, QUEUED_DUP, COUNTER, TEXT]


def test_hand_cases_in_one_call(engine):
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in HAND]
    empty = store.open()
    res = store.apply(list(zip(hs, HAND)))
    assert (res.docs["status"] == 0).all()
    assert int(res.docs["n_queued"][1]) == 1 and int(res.docs["hist_len"][1]) == 3
    srcs = {h: enc_source(store, h) for h in hs + [empty]}
    req, hist = [], []
    for h in hs + [empty]:
        H = hist_len(srcs[h])
        for k in (0, 1, max(H - 1, 0), H, H + 5):
            req.append(h)
            hist.append(k)
    want, o = check(store, srcs, req, history=hist)
    assert [int(x) for x in o.docs["hist_len"][:5]] == [0, 1, 5, 6, 6] and not o.docs["n_queued"].any()
    # the shuffled document's whole history, in history order, is not its arrival order
    b, r, clog, _ = store.materialize([hs[0]], history=[99])
    assert [int(x) for x in clog] == [2, 3, 4, 0, 1, 5]
    # the counter between its set and the incs, then with each inc (10, 15, 13), then the second set
    b, r, _, _ = store.materialize([hs[2]] * 5, history=[1, 2, 3, 4, 5])
    n_reg = int(r.regs[0]["n_surv"])
    vals = [int(r.surv[int(b.docs["op_off"][i]) + int(r.regs[int(b.docs["reg_off"][i])]["surv_off"])]["value"]) for i in range(4)]
    assert n_reg == 1 and vals == [10, 15, 13, 1]
    # the text: the element is there but unset after the insert, visible after the set, gone after the delete
    b, r, _, _ = store.materialize([hs[3]] * 4, history=[2, 3, 4, 5])
    e = store.enc[hs[3]].regs[(1, f"{A}:1")]
    seen = [(int(r.regs[int(b.docs["reg_off"][i]) + e]["n_surv"]), int(r.regs[int(b.docs["reg_off"][i]) + e]["list_index"]))
            for i in range(4)]
    assert seen == [(0, -1), (1, 0), (1, 0), (0, -1)]


# ---- wave-loop and tile boundaries ------------------------------------------------------------------
def test_wave_and_tile_boundaries(engine):
    """Single-op changes of one actor, delivered in reversed blocks of 7 (log [A7 .. A1, A14 .. A8, ...],
    history A1 .. An, so no slot equals its log index), with history lengths around the bitmap tile
    and prefixes around the 64-lane stride and the tile."""
    store = DocStore(engine, a_stride=8)
    lens = [T - 1, T, T + 1, 2 * T + 3]
    hs = [store.open() for _ in lens]
    items = []
    for h, n in zip(hs, lens):
        seqs = []
        for k0 in range(1, n + 1, 7):
            seqs += list(range(min(k0 + 6, n), k0 - 1, -1))
        items.append((h, [ch(A, q, {}, s("k%d" % (q % 5), q)) for q in seqs]))
    res = store.apply(items)
    assert [int(x) for x in res.docs["hist_len"]] == lens and not res.docs["n_queued"].any()
    srcs = {h: enc_source(store, h) for h in hs}
    req, hist = [], []
    for h, n in zip(hs, lens):
        for k in (63, 64, 65, T - 1, T, T + 1, n - 1, n, n + 5):
            req.append(h)
            hist.append(k)
    want, _ = check(store, srcs, req, history=hist)
    assert int(want.docs["n_changes"].max()) == 2 * T + 3
    rows = np.zeros((2, 8), np.uint32)
    rows[0, 0], rows[1, 0] = T + 1, 2 * T + 2                    # the same cuts as clocks
    check(store, srcs, [hs[3], hs[3]], clocks=rows)


# ---- clock rows ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c4(engine):
    b = synth.generate(synth.config("C4", n_docs=300))
    o = O.merge(b, threads=8)
    store = RowStore(engine, a_stride=b.a_stride)
    h0 = store.open_n(b.n_docs)
    hs = np.arange(h0, h0 + b.n_docs, dtype=np.uint32)
    store.submit_batch(b, hs)
    assert (store.wait().docs["status"] == 0).all()
    return store, b, o, {int(h): source_of(b, o.hist, i) for i, h in enumerate(hs)}, hs


def test_random_clock_cuts(c4):
    store, b, o, srcs, hs = c4
    S = b.a_stride
    rng = np.random.default_rng(5)
    clock = o.clock.reshape(-1, S).astype(np.int64)
    rows = rng.integers(0, clock + 2).astype(np.uint32)         # per actor: from nothing to one past its last seq
    want, wo = check(store, srcs, hs, clocks=rows)
    assert 0 < len(want.changes) < len(b.changes)
    # ... and the documents' own clocks give their whole histories
    full, fo = check(store, srcs, hs, clocks=o.clock.reshape(-1, S))
    np.testing.assert_array_equal(fo.docs["hist_len"], o.docs["hist_len"])
    np.testing.assert_array_equal(fo.clock, o.clock)


def test_clock_at_a_history_length_is_that_prefix(c4):
    store, b, o, srcs, hs = c4
    S = b.a_stride
    rng = np.random.default_rng(6)
    p = rng.integers(0, o.docs["hist_len"].astype(np.int64) + 1)
    slices = read_history(store, hs, np.zeros(len(hs), np.uint32), p)      # history.slice(0, p) from the store
    rows = np.zeros((len(hs), S), np.uint32)
    for i, h in enumerate(hs):
        for j in slices[i]:                                     # (in history order: an actor's seqs ascend)
            c = srcs[int(h)].changes[j]
            rows[i, int(c["actor"])] = int(c["seq"])
    bc, rc, clog_c, olog_c = store.materialize(hs, clocks=rows)
    bp, rp, clog_p, olog_p = store.materialize(hs, history=p)
    assert [int(x) for x in clog_c] == [j for sl in slices for j in sl]
    for x, y in ((bc.docs, bp.docs), (bc.changes, bp.changes), (bc.deps, bp.deps), (bc.ops, bp.ops), (clog_c, clog_p),
                 (olog_c, olog_p), (rc.docs, rp.docs), (rc.hist, rp.hist), (rc.regs, rp.regs), (rc.clock, rp.clock)):
        same_bytes(x, y, "clock at p against prefix p")
    np.testing.assert_array_equal(rp.docs["hist_len"], p)
    assert not rp.docs["n_queued"].any()


def test_clock_that_is_not_causally_closed(engine):
    store = DocStore(engine, a_stride=8)
    h = store.open()
    store.apply([(h, SHUFFLED)])
    srcs = {h: enc_source(store, h)}
    rows = np.zeros((2, 8), np.uint32)
    rows[0, 1] = 2                                              # bbbb:1 and bbbb:2 without any change of aaaa
    rows[1, 0], rows[1, 2] = 1, 1                               # aaaa:1 and cccc:1 (which needs aaaa:3)
    want, o = check(store, srcs, [h, h], clocks=rows)
    assert [int(x) for x in o.docs["n_queued"]] == [2, 1] and [int(x) for x in o.docs["hist_len"]] == [0, 1]
    b, r, clog, _ = store.materialize([h, h], clocks=[{B: 2, "nobody": 7}, {A: 1, Cc: 1}])
    assert [int(x) for x in r.docs["n_queued"]] == [2, 1] and [int(x) for x in clog] == [3, 0, 2, 5]


def test_stride_128_with_70_actors(engine):
    """The clock row spans more than one 64-lane column: every writer's first change, a change of the
    last writer that has heard all of them (it arrives first and waits), second changes of some."""
    n_actors, S = 70, 128
    actors = [f"w{i:03d}" for i in range(n_actors - 1)]
    last = "zzzz"
    changes = [ch(last, 1, {a: 1 for a in actors}, s("all", 1))]
    changes += [ch(a, 1, {}, s("k%d" % (i % 5), i)) for i, a in enumerate(actors)]
    changes += [ch(a, 2, {last: 1}, s("late", i)) for i, a in enumerate(actors[::3])]
    store = DocStore(engine, a_stride=S)
    h = store.open()
    assert int(store.apply([(h, changes)]).docs["status"][0]) == 0
    srcs = {h: enc_source(store, h)}
    rng = np.random.default_rng(128)
    rows = np.zeros((6, S), np.uint32)
    rows[:, :n_actors] = rng.integers(0, 3, size=(6, n_actors))
    rows[0, :n_actors] = 2                                      # everything
    rows[1, :n_actors] = 1                                      # the first changes and zzzz:1
    rows[2] = 0
    rows[2, 64:n_actors] = 2                                    # only ranks of the second lane column
    want, o = check(store, srcs, [h] * 6, clocks=rows)
    assert [int(x) for x in o.docs["hist_len"][:2]] == [len(changes), n_actors]
    assert int(want.docs["n_changes"][2]) == (n_actors - 64) + len([i for i in range(0, n_actors - 1, 3) if i >= 64])
    check(store, srcs, [h] * 3, history=[63, 64, 65])


# ---- many requests ------------------------------------------------------------------------------
def fed(engine, batches, rounds=1):
    """a RowStore holding the documents of the batches (one stride), fed in `rounds` slices of each
    document's arrival order; (store, {handle: Source})"""
    S = batches[0].a_stride
    store = RowStore(engine, a_stride=S)
    srcs = {}
    for b in batches:
        assert b.a_stride == S
        o = O.merge(b, threads=8)
        assert (o.docs["status"] == 0).all()
        h0 = store.open_n(b.n_docs)
        hs = np.arange(h0, h0 + b.n_docs, dtype=np.uint32)
        n = b.docs["n_changes"].astype(np.int64)
        # (later rounds of six changes each: small enough to apply on the resident state)
        cuts = [np.zeros_like(n)] + [np.maximum(n - 6 * (rounds - k), 0) for k in range(1, rounds + 1)]
        for k in range(rounds):
            part = b if rounds == 1 else slice_changes(b, cuts[k], cuts[k + 1])
            store.submit_batch(part, hs)
            assert (store.wait().docs["status"] == 0).all()
        for i, h in enumerate(hs):
            srcs[int(h)] = source_of(b, o.hist, i)
    return store, srcs


def random_prefixes(rng, srcs):
    hs = np.array(sorted(srcs), np.uint32)
    return hs, np.array([rng.integers(0, len(srcs[int(h)].changes) + 2) for h in hs], np.uint32)


def test_many_requests(engine):
    """5,000 map documents and 50 text documents of thousands of ops (the large merge kernel under the
    gathered rows) in one call, a random prefix each; 200 documents of nested maps and lists with
    queued and duplicate changes in another store (their stride is 4)."""
    store, srcs = fed(engine, [synth.generate(synth.config("C4", n_docs=5000)), synth.generate(synth.config("C3", n_docs=50))])
    hs, p = random_prefixes(np.random.default_rng(1), srcs)
    want, o = check(store, srcs, hs, history=p)
    assert int(want.docs["n_ops"].max()) > 1000 and len(want.docs) == 5050
    store5, srcs5 = fed(engine, [synth.generate(synth.config("C5", n_docs=200))])
    hs5, p5 = random_prefixes(np.random.default_rng(2), srcs5)
    check(store5, srcs5, hs5, history=p5)
    assert any((sr.hist == -2).any() for sr in srcs5.values())


def test_many_requests_after_incremental_rounds(engine):
    """The same documents fed in three rounds (all but the last 12 changes, then 6 and 6): the later two
    apply incrementally where the store's envelope takes them, segments have moved and have slack —
    with lists and text (C3, C5) and with queued and duplicate rows (C5) in the moved segments too."""
    store, srcs = fed(engine, [synth.generate(synth.config("C4", n_docs=5000)), synth.generate(synth.config("C3", n_docs=50))],
                      rounds=3)
    assert store.last_routing()["incremental"] > 0
    hs, p = random_prefixes(np.random.default_rng(3), srcs)
    want, _ = check(store, srcs, hs, history=p)
    assert int(want.docs["n_ops"].max()) > 1000 and len(want.docs) == 5050
    store5, srcs5 = fed(engine, [synth.generate(synth.config("C5", n_docs=200))], rounds=3)
    hs5, p5 = random_prefixes(np.random.default_rng(2), srcs5)
    check(store5, srcs5, hs5, history=p5)
    assert any((sr.hist == -2).any() for sr in srcs5.values())
    # clocks by actor id need a host encoder: a store fed prebuilt rows takes rank rows
    with pytest.raises(EngineError, match="rank rows"):
        store5.materialize(hs5[:1], clocks=[{"aaaa": 1}])


# ---- the call itself ----------------------------------------------------------------------------
class Raw:
    """hm_store_materialize with caller capacities; every output pre-filled with 0xA5"""

    def __init__(self, store, n, caps):
        S = store.S
        nc, nd, no, nr = caps
        fill = lambda k, dt: np.frombuffer(bytes([0xA5]) * (max(k, 1) * np.dtype(dt).itemsize), dt).copy()
        self.docs, self.changes, self.deps, self.ops = fill(n, DOC_DT), fill(nc, CHANGE_DT), fill(nd, DEP_DT), fill(no, OP_DT)
        self.clog, self.olog = fill(nc, np.uint32), fill(no, np.uint32)
        self.res = Results(fill(n, DOC_RESULT_DT), fill(n * S, np.uint32), fill(n * S, np.uint32), fill(n * S, np.uint32),
                           fill(nc, np.int32), fill(nc * S, np.uint32), fill(nr, REG_RESULT_DT), fill(no, SURV_RESULT_DT))
        self.out = CPastOut(nc, nd, no, nr, self.docs.ctypes.data, self.changes.ctypes.data, self.deps.ctypes.data,
                            self.ops.ctypes.data, self.clog.ctypes.data, self.olog.ctypes.data, self.res.c_struct())
        self.tot = np.full(4, 77, np.uint64)

    def arrays(self):
        r = self.res
        return [self.docs, self.changes, self.deps, self.ops, self.clog, self.olog, r.docs, r.clock, r.back_clock, r.heads,
                r.hist, r.all_deps, r.regs, r.surv]

    def untouched(self):
        return all(a.tobytes() == bytes([0xA5]) * a.nbytes for a in self.arrays())


def raw_call(store, hs, caps, history=None, clocks=None):
    hs = np.ascontiguousarray(hs, np.uint32)
    hl = None if history is None else np.ascontiguousarray(history, np.uint32)
    rows = None if clocks is None else np.ascontiguousarray(clocks, np.uint32)
    R = Raw(store, len(hs), caps)
    st = store._L.hm_store_materialize(store._h, len(hs), hs.ctypes.data, hl.ctypes.data if hl is not None else None,
                                       rows.ctypes.data if rows is not None else None, ctypes.byref(R.out), R.tot.ctypes.data)
    return st, R


def test_caps_errors_and_untouched_state(engine):
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in HAND]
    store.apply(list(zip(hs, HAND)))
    srcs = {h: enc_source(store, h) for h in hs}
    req, hist = [hs[0], hs[3], hs[0], hs[2]], [4, 5, 6, 2]
    want, wclog, wolog = gather([(srcs[h], k, None) for h, k in zip(req, hist)], 8)
    exact = [len(want.changes), len(want.deps), len(want.ops), int(want.docs["n_regs"].sum())]
    before = [store.read(h)[1] for h in hs]
    for short in range(4):                                      # one row short in each table in turn
        caps = list(exact)
        caps[short] -= 1
        st, R = raw_call(store, req, caps, history=hist)
        assert st == NOMEM and [int(x) for x in R.tot] == exact and R.untouched(), short
    st, R = raw_call(store, req, exact, history=hist)
    assert st == 0 and [int(x) for x in R.tot] == exact
    for got, w in ((R.docs, want.docs), (R.changes, want.changes), (R.deps, want.deps), (R.ops, want.ops), (R.clog, wclog),
                   (R.olog, wolog)):
        same_bytes(got, w, "exact capacities")
    assert_same(want, R.res, O.merge(want))
    # a handle outside the store, both selectors, neither
    rows = np.zeros((len(req), 8), np.uint32)
    for bad in (dict(hs=[hs[0], 9999], caps=exact, history=[1, 1]), dict(hs=req, caps=exact, history=hist, clocks=rows),
                dict(hs=req, caps=exact)):
        st, R = raw_call(store, bad.pop("hs"), bad.pop("caps"), **bad)
        assert st == INVALID and R.untouched(), bad
    with pytest.raises(EngineError, match="bad handle"):
        store.materialize([hs[0], 9999], history=[1, 1])
    with pytest.raises(EngineError, match="exactly one"):
        store.materialize(req, history=hist, clocks=rows)
    with pytest.raises(EngineError, match="exactly one"):
        store.past_sizes(req)
    # n == 0
    st, R = raw_call(store, [], [0, 0, 0, 0], history=[])
    assert st == 0 and not R.tot.any()
    # the resident state is only read
    after = [store.read(h)[1] for h in hs]
    for x, y in zip(before, after):
        for f in ("docs", "clock", "back_clock", "heads", "hist", "all_deps", "regs", "surv"):
            same_bytes(getattr(y, f), getattr(x, f), f)
    # a batch in flight
    store.submit([(hs[0], [ch(A, 4, {}, s("x", 4))])])
    st, R = raw_call(store, req, exact, history=hist)
    assert st == INVALID and R.untouched()
    with pytest.raises(EngineError, match="in flight"):
        store.past_sizes(req, history=hist)
    store.wait()
    b, r, clog, _ = store.materialize([hs[0]], history=[99])
    assert [int(x) for x in clog] == [2, 3, 4, 0, 1, 5, 6]


# ---- a merged cold batch on the device ----------------------------------------------------------
def test_materialize_device_equals_the_store_form(engine):
    import torch
    b = synth.generate(synth.config("C5", n_docs=120, arrival=2, shuffle_pct=30))
    S, n = b.a_stride, b.n_docs
    store, srcs = fed(engine, [b])
    rng = np.random.default_rng(9)
    req = rng.integers(0, n, size=200).astype(np.uint32)       # documents repeat
    p = np.array([rng.integers(0, len(srcs[int(h)].changes) + 2) for h in req], np.uint32)
    sb, sr, sclog, solog = store.materialize(req, history=p)
    r = engine.merge(b)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    t = [up(x) for x in (b.docs, b.changes, b.deps, b.ops, r.docs, r.hist, req, p)]
    cb = CBatch(n, len(b.changes), len(b.deps), len(b.ops), 0, S, 0, 0, 0, 0, 0, 0,
                t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), None)
    cr = CResults(t[4].data_ptr(), None, None, None, t[5].data_ptr(), None, None, None)
    nq = len(req)
    caps = [len(sb.changes), len(sb.deps), len(sb.ops), int(sb.docs["n_regs"].sum())]
    z = lambda nbytes: torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)
    g = [z(nq * 48), z(caps[0] * 24), z(caps[1] * 8), z(caps[2] * 32), z(caps[0] * 4), z(caps[2] * 4)]
    summ = z(64)
    work = z(int(engine._L.hm_materialize_work_bytes(nq)))
    out = CPastOut(caps[0], caps[1], caps[2], caps[3], *[x.data_ptr() for x in g], CResults())
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    engine.materialize_device(cb, cr, nq, t[6].data_ptr(), t[7].data_ptr(), 0, out, summ.data_ptr(), work.data_ptr(), stream)
    torch.cuda.synchronize()
    sm = CPastSummary.from_buffer_copy(summ.cpu().numpy().tobytes())
    assert list(sm.totals) == caps and sm.bad == 0
    down = lambda x, dt, k: np.frombuffer(x.cpu().numpy().tobytes()[:k * np.dtype(dt).itemsize], dt)
    for got, w, what in ((down(g[0], DOC_DT, nq), sb.docs, "docs"), (down(g[1], CHANGE_DT, caps[0]), sb.changes, "changes"),
                         (down(g[2], DEP_DT, caps[1]), sb.deps, "deps"), (down(g[3], OP_DT, caps[2]), sb.ops, "ops"),
                         (down(g[4], np.uint32, caps[0]), sclog, "change_log"), (down(g[5], np.uint32, caps[2]), solog, "op_log")):
        same_bytes(got, w, what)
    cnt = down(work, np.uint32, 8 * nq).reshape(2, nq, 4)
    np.testing.assert_array_equal(cnt[0], np.stack([sb.docs[f] for f in ("n_changes", "n_deps", "n_ops", "n_regs")], 1))
    np.testing.assert_array_equal(cnt[1], np.stack([sb.docs[f] for f in ("change_off", "dep_off", "op_off", "reg_off")], 1))
    assert (sm.max_changes, sm.max_ops, sm.max_regs, sm.max_objs, sm.max_deps, sm.doc_flags) == tuple(
        int(sb.docs[f].max()) for f in ("n_changes", "n_ops", "n_regs", "n_objs", "n_deps")) + (int(np.bitwise_or.reduce(sb.docs["flags"])),)
    # the caller's own merge of the gathered batch, sized by the summary
    res = [z(nq * 32), z(nq * S * 4), z(nq * S * 4), z(nq * S * 4), z(caps[0] * 4), z(caps[0] * S * 4), z(caps[3] * 16), z(caps[2] * 16)]
    gb = CBatch(nq, caps[0], caps[1], caps[2], caps[3], S, sm.max_changes, sm.max_ops, sm.max_regs, sm.max_objs, sm.doc_flags,
                sm.max_deps, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), None)
    engine.merge_device(gb, CResults(*[x.data_ptr() for x in res]), stream)
    torch.cuda.synchronize()
    got = Results(down(res[0], DOC_RESULT_DT, nq), down(res[1], np.uint32, nq * S), down(res[2], np.uint32, nq * S),
                  down(res[3], np.uint32, nq * S), down(res[4], np.int32, caps[0]), down(res[5], np.uint32, caps[0] * S),
                  down(res[6], REG_RESULT_DT, caps[3]), down(res[7], SURV_RESULT_DT, caps[2]))
    assert_same(sb, got, sr)
    # no request: the summary is zeroed and nothing else is touched (no work buffer is needed)
    summ.fill_(0xA5)
    engine.materialize_device(cb, cr, 0, 0, t[7].data_ptr(), 0, CPastOut(), summ.data_ptr(), 0, stream)
    torch.cuda.synchronize()
    assert not summ.cpu().numpy().any()
    with pytest.raises(EngineError, match="aligned"):
        engine.materialize_device(cb, cr, nq, t[6].data_ptr(), t[7].data_ptr(), 0, out, summ.data_ptr(), work.data_ptr() + 4, stream)
    # too small a capacity: nothing is gathered, the summary still says what is needed
    g2 = z(nq * 48)
    out2 = CPastOut(caps[0] - 1, caps[1], caps[2], caps[3], g2.data_ptr(), *[x.data_ptr() for x in g[1:]], CResults())
    engine.materialize_device(cb, cr, nq, t[6].data_ptr(), t[7].data_ptr(), 0, out2, summ.data_ptr(), work.data_ptr(), stream)
    torch.cuda.synchronize()
    assert list(CPastSummary.from_buffer_copy(summ.cpu().numpy().tobytes()).totals) == caps
    assert not g2.cpu().numpy().any()


# ---- the route that existed before ---------------------------------------------------------------
def test_equals_history_prefix_and_host_rebuild(engine):
    """hm_doc_history_prefix + hm_doc_log + a batch rebuilt on the host + a cold merge, per document,
    against one materialize call."""
    b0 = synth.generate(synth.config("C5", n_docs=100, arrival=2, shuffle_pct=30, dup_pct=10))
    docs = [decode_doc(b0, i) for i in range(b0.n_docs)]
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in docs]
    assert (store.apply(list(zip(hs, docs))).docs["status"] == 0).all()
    rng = np.random.default_rng(4)
    p = [int(rng.integers(0, len(c) + 2)) for c in docs]
    b, r, clog, olog = store.materialize(hs, history=p)
    reqs = []
    for h, k in zip(hs, p):
        idx = store.history_prefix(h, k)
        cr_, dr, orr = store.log(h)
        hist = np.full(len(cr_), -1, np.int32)
        hist[idx] = np.arange(len(idx))
        e = store.enc[h]
        reqs.append((Source(cr_, dr, orr, len(e.reg_list), len(e.obj_list), len(e.actors), e.flags, hist), len(idx), None))
    old, oclog, oolog = gather(reqs, 8)
    for f in ("docs", "changes", "deps", "ops"):
        same_bytes(getattr(b, f), getattr(old, f), f)
    same_bytes(clog, oclog, "change_log")
    same_bytes(olog, oolog, "op_log")
    assert_same(old, r, engine.merge(old))
