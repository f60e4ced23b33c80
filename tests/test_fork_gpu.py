"""Resident documents forked at a clock on the device (hm_store_fork_submit: the past kernels' gather
with an optional actor-major order table, handed to the device-table submit).  Per request three
things are compared: the fork's read() / info() against ``oracle.merge`` of the rows tests/fork_ref.py
says it receives (pinned on the oracle by tests/test_fork_ref.py), bit for bit; against the read() of a
control handle that received those rows through RowStore.submit_batch; and, in history order, against
materialize() of the same selector."""
import numpy as np
import pytest

from hypermerge_amd.columnar import Batch, encode
from hypermerge_amd.engine import EngineError
from hypermerge_amd.store import DocStore, RowStore
import oracle.oracle as O

from fork_ref import NONE, gather_fork
from fuzz_docs import gen_docs
from kat_cases import A, B, ch, s
from past_ref import clock_at, gather, hist_len, select, source_of
from test_gpu_parity import assert_same
from test_materialize_gpu import HAND, T, enc_source, same_bytes

pytestmark = pytest.mark.gpu

INVALID = 32
READ = ("docs", "clock", "back_clock", "heads", "hist", "all_deps", "regs", "surv")


def order_rows(S, orders):
    rows = np.full((len(orders), S), NONE, np.uint32)
    for i, o in enumerate(orders):
        rows[i, :len(o)] = o
    return rows


def requests(srcs, hs, history, clocks, order):
    return [(srcs[int(h)], None if history is None else int(history[i]), None if clocks is None else clocks[i],
             None if order is None else order[i]) for i, h in enumerate(hs)]


def check_forks(store, ctl, reqs, hs, new, res, oracle=None):
    """The forks `new` of one call against the restatement's rows: the result rows and every read()
    against a control that received those rows through submit_batch (in the store `ctl`), the log
    against the rows themselves, read() / info() against the oracle's merge of each fork's rows
    (oracle: the requests to merge, default all).  Returns (the restatement's batch, the control handles)."""
    S, n = store.S, len(hs)
    want, _, _ = gather_fork(reqs, S)
    c0 = ctl.open_n(n)
    chs = np.arange(c0, c0 + n, dtype=np.uint32)
    ctl.submit_batch(want, chs)
    cres = ctl.wait()
    for f in ("docs", "clock", "back_clock", "heads"):
        same_bytes(getattr(res, f), getattr(cres, f), "result rows: " + f)
    for i in range(n):
        r = want.docs[i]
        c_lo, d_lo, o_lo = int(r["change_off"]), int(r["dep_off"]), int(r["op_off"])
        fb, fr = store.read(new[i])
        _, cr = ctl.read(int(chs[i]))
        for f in READ:
            same_bytes(getattr(fr, f), getattr(cr, f), (i, f))
        assert store.info(new[i]) == ctl.info(int(chs[i])), i
        lc, ld, lo = store.log(new[i])
        wc = want.changes[c_lo:c_lo + int(r["n_changes"])].copy()
        wc["dep_off"] -= d_lo
        wc["op_first"] -= o_lo
        same_bytes(lc, wc, (i, "log changes"))
        same_bytes(ld, want.deps[d_lo:d_lo + int(r["n_deps"])], (i, "log deps"))
        same_bytes(lo, want.ops[o_lo:o_lo + int(r["n_ops"])], (i, "log ops"))
        if oracle is None or i in oracle:
            one, _, _ = gather_fork([reqs[i]], S)
            o = O.merge(one)
            assert_same(one, fr, o)
            inf = store.info(new[i])
            assert [inf[f] for f in ("n_changes", "n_deps", "n_ops", "n_regs", "n_objs", "n_actors")] == \
                [int(one.docs[f][0]) for f in ("n_changes", "n_deps", "n_ops", "n_regs", "n_objs", "n_actors")]
            assert (inf["hist_len"], inf["n_queued"], inf["status"]) == \
                (int(o.docs["hist_len"][0]), int(o.docs["n_queued"][0]), int(o.docs["status"][0]))
    return want, chs


def fork_and_check(store, ctl, srcs, hs, history=None, clocks=None, order=None, oracle=None, min_clock=False):
    hs = np.asarray(hs, np.uint32)
    reqs = requests(srcs, hs, history, clocks, order)
    new = store.fork(hs, history=history, clocks=clocks, order=None if order is None else order_rows(store.S, order),
                     min_clock=min_clock)
    res = store.fork_result
    assert (res.docs["status"] == 0).all()
    want, _ = check_forks(store, ctl, reqs, hs, new, res, oracle)
    if order is None:                                            # history order: what materialize gives for the selector
        mb, mr, _, _ = store.materialize(hs, history=history, clocks=clocks)
        for f in ("docs", "changes", "deps", "ops"):
            same_bytes(getattr(mb, f), getattr(want, f), "materialize: " + f)
        for f in ("status", "hist_len", "n_queued", "n_surv"):
            np.testing.assert_array_equal(res.docs[f], mr.docs[f], err_msg="materialize: " + f)
        for f in ("clock", "back_clock", "heads"):
            same_bytes(getattr(res, f).reshape(-1), getattr(mr, f), "materialize: " + f)
        for i, h in enumerate(new):
            r = mb.docs[i]
            _, fr = store.read(h)
            c_lo, g_lo, o_lo = int(r["change_off"]), int(r["reg_off"]), int(r["op_off"])
            same_bytes(fr.hist, mr.hist[c_lo:c_lo + int(r["n_changes"])], (i, "materialize: hist"))
            same_bytes(fr.regs, mr.regs[g_lo:g_lo + int(r["n_regs"])], (i, "materialize: regs"))
            k = int(mr.docs["n_surv"][i])
            same_bytes(fr.surv[:k], mr.surv[o_lo:o_lo + k], (i, "materialize: surv"))
    return new, want


def clock_rows(S, *clocks):
    rows = np.zeros((len(clocks), S), np.uint32)
    for i, c in enumerate(clocks):
        rows[i, :len(c)] = c
    return rows


# ---- hand cases, strides --------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 12])
def test_hand_cases_in_one_call_with_a_repeated_source(engine, S):
    """Shuffled arrival, queued and duplicate changes, an f64 counter and a text: every document at
    several clocks, in rank order, reversed rank order and history order, and at history lengths."""
    store, ctl = DocStore(engine, a_stride=S), RowStore(engine, a_stride=S)
    hs = [store.open() for _ in HAND]
    res = store.apply(list(zip(hs, HAND)))
    assert (res.docs["status"] == 0).all() and int(res.docs["n_queued"][1]) == 1
    srcs = {h: enc_source(store, h) for h in hs}
    req, rows, order = [], [], []
    for h in hs:
        na = srcs[h].n_actors
        top = res.clock[h].astype(np.int64)
        for k in (top, np.maximum(top - 1, 0), np.minimum(top, 1), top + 3):
            for o in (list(range(na)), list(range(na))[::-1]):
                req.append(h)
                rows.append(k.astype(np.uint32))
                order.append(o)
    rows = np.stack(rows)
    new, want = fork_and_check(store, ctl, srcs, req, clocks=rows, order=order)
    assert len(new) == 32 and int(want.docs["n_changes"].max()) == 6
    fork_and_check(store, ctl, srcs, req, clocks=rows)
    hist = [k for h in hs for k in (0, 1, hist_len(srcs[h]) - 1, hist_len(srcs[h]) + 5)]
    fork_and_check(store, ctl, srcs, [h for h in hs for _ in range(4)], history=hist)
    # the shuffled document: its history is A1 B1 A2 B2 A3 C1, handed over actor by actor it is not
    f = store.fork([hs[0]], clocks=[{A: 3, B: 2}], order="clock")[0]
    assert [(int(c["actor"]), int(c["seq"])) for c in store.log(f)[0]] == [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2)]
    _, r = store.read(f)
    assert int(r.docs["hist_len"][0]) == 5 and [int(x) for x in r.hist] == [0, 2, 4, 1, 3]
    g = store.fork([hs[0]], clocks=[{B: 2, A: 3, "nobody": 4}], order="clock")[0]
    assert [(int(c["actor"]), int(c["seq"])) for c in store.log(g)[0]] == [(1, 1), (1, 2), (0, 1), (0, 2), (0, 3)]
    _, r = store.read(g)
    assert int(r.docs["hist_len"][0]) == 5 and int(r.docs["n_queued"][0]) == 0
    # the sources are only read
    for h in hs:
        b, r = store.read(h)
        assert_same(b, r, O.merge(b))


# ---- wave and tile boundaries ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_actors(engine):
    """aaaa and bbbb, 400 concurrent single-op changes each, arriving alternately: the history
    interleaves them, so no actor-major position but the first equals its history position."""
    store = DocStore(engine, a_stride=8)
    h = store.open()
    log = [ch(a, q, {}, s("%s%d" % (a[0], q % 7), q)) for q in range(1, 401) for a in (A, B)]
    res = store.apply([(h, log)])
    assert int(res.docs["status"][0]) == 0 and int(res.docs["hist_len"][0]) == 800
    return store, RowStore(engine, a_stride=8), h, {h: enc_source(store, h)}


def test_wave_and_tile_boundaries(two_actors):
    """Selections of 64 and 65 changes (one actor, and two with the second's block across the 64th
    position); of HM_PAST_TILE and HM_PAST_TILE + 1 changes with bbbb's block (from position 300)
    reaching the tile's last position and the next tile's first; the whole document, where aaaa's or
    bbbb's block straddles the tile edge."""
    store, ctl, h, srcs = two_actors
    assert T == 512
    cuts = [(64, 0), (65, 0), (32, 32), (32, 33), (63, 2), (300, T - 300), (300, T + 1 - 300), (T - 300, 300), (T + 1 - 300, 300),
            (400, 400), (400, T - 400), (T, T), (0, 65)]
    rows = clock_rows(8, *cuts)
    for order in ([0, 1], [1, 0]):
        new, want = fork_and_check(store, ctl, srcs, [h] * len(cuts), clocks=rows, order=[order] * len(cuts), oracle={0, 3, 5, 6, 9})
        assert [int(x) for x in want.docs["n_changes"]] == [64, 65, 64, 65, 65, T, T + 1, T, T + 1, 800, T, 800, 65]
    new, want = fork_and_check(store, ctl, srcs, [h] * len(cuts), clocks=rows, oracle={1, 6})
    # actor-major against history order: the same changes, another log
    a, b = store.fork([h, h], clocks=rows[6:7].repeat(2, 0), order=order_rows(8, [[0, 1], [1, 0]]))
    ka = [(int(c["actor"]), int(c["seq"])) for c in store.log(a)[0]]
    assert ka == [(0, q) for q in range(1, 301)] + [(1, q) for q in range(1, T + 2 - 300)]
    assert sorted(ka) == sorted((int(c["actor"]), int(c["seq"])) for c in store.log(b)[0])


def test_empty_selection(two_actors):
    """An all-zero clock (with and without an order row) and history = 0: the destination stays an
    empty document with its parent's totals and an empty document's result row."""
    store, ctl, h, srcs = two_actors
    new, want = fork_and_check(store, ctl, srcs, [h, h], clocks=clock_rows(8, (0, 0), (0, 0)), order=[[0, 1], []])
    assert not want.docs["n_changes"].any()
    new2, _ = fork_and_check(store, ctl, srcs, [h], history=[0])
    res = store.fork_result
    assert (int(res.docs["hist_len"][0]), int(res.docs["n_queued"][0]), int(res.docs["n_surv"][0])) == (0, 0, 0)
    for f in new + new2:
        inf = store.info(f)
        assert inf["n_changes"] == 0 and inf["n_regs"] == srcs[h].n_regs and inf["n_actors"] == 2
    # ... and takes changes like any document
    r = store.apply([(new[0], [ch(A, 1, {}, s("a1", 1))])])
    assert int(r.docs["status"][0]) == 0 and int(r.docs["hist_len"][0]) == 1
    b, rr = store.read(new[0])
    assert_same(b, rr, O.merge(b))


# ---- refusals -------------------------------------------------------------------------------------
def test_refusals_leave_source_and_destination_unchanged(engine):
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in HAND]
    store.apply(list(zip(hs, HAND)))
    e1, e2, e3 = store.open(), store.open(), store.open()
    src, full = hs[0], store.open()
    store.apply([(full, HAND[2])])
    state = lambda: [[getattr(store.read(h)[1], f).tobytes() for f in READ] + [store.info(h)] for h in hs + [e1, e2, e3, full]]
    before = state()
    k = clock_rows(8, (3, 2, 1), (3, 2, 1))
    ok_order = order_rows(8, [[0, 1, 2], [2, 1, 0]])

    def raw(n, src_h, hist, rows, order, dst):
        keep = [None if a is None else np.ascontiguousarray(a, np.uint32) for a in (src_h, hist, rows, order, dst)]
        return store._L.hm_store_fork_submit(store._h, n, *[None if a is None else a.ctypes.data for a in keep], 0, None)

    cases = {
        "both selectors": ([src, src], [1, 1], k, None, [e1, e2]),
        "neither selector": ([src, src], None, None, None, [e1, e2]),
        "an order with a history length": ([src, src], [1, 1], None, ok_order, [e1, e2]),
        "order: a selected actor not listed": ([src, src], None, k, order_rows(8, [[0, 1, 2], [0, 1]]), [e1, e2]),
        "order: a rank twice": ([src, src], None, k, order_rows(8, [[0, 1, 2], [0, 1, 2, 1]]), [e1, e2]),
        "order: a rank outside the document": ([src, src], None, k, order_rows(8, [[0, 1, 2], [0, 1, 2, 5]]), [e1, e2]),
        "source outside the store": ([src, 9999], None, k, ok_order, [e1, e2]),
        "destination outside the store": ([src, src], None, k, ok_order, [e1, 9999]),
        "destination repeated": ([src, src], None, k, ok_order, [e1, e1]),
        "destination not empty": ([src, src], None, k, ok_order, [e1, full]),
        "destination is a source": ([e1, src], None, k, None, [e2, e1]),
        "destination is its own source": ([src, e2], None, k, None, [e1, e2]),
    }
    for what, (sh, hist, rows, order, dst) in cases.items():
        assert raw(2, sh, hist, rows, order, dst) == INVALID, what
        assert state() == before, what
    assert raw(0, [src], [1], None, None, [e1]) == INVALID
    with pytest.raises(EngineError, match="not listed"):
        store.fork_submit([src], clocks=k[:1], order=order_rows(8, [[0]]), into=[e1])
    with pytest.raises(EngineError, match="destination"):
        store.fork_submit([src], clocks=k[:1], into=[full])
    # a batch in flight
    store.submit([(full, [ch(A, 4, {}, s("n", 4))])])
    assert raw(2, [src, src], None, k, ok_order, [e1, e2]) == INVALID
    store.wait()
    # ... and a fork batch in flight refuses every read and a second fork
    new, bid = store.fork_submit([src, src], clocks=k, order=ok_order, into=[e1, e2])
    assert raw(1, [src], [1], None, None, [e3]) == INVALID
    with pytest.raises(EngineError, match="in flight"):
        store.info(e1)
    with pytest.raises(EngineError, match="in flight"):
        store.materialize([src], history=[1])
    r = store.wait()
    assert (r.docs["status"] == 0).all() and [int(x) for x in r.docs["hist_len"]] == [6, 6]
    for got, want in zip(state()[:len(hs)], before[:len(hs)]):
        assert got == want


# ---- undo -----------------------------------------------------------------------------------------
def test_undo_leaves_the_destinations_empty_and_reusable(engine):
    store, ctl = DocStore(engine, a_stride=8), RowStore(engine, a_stride=8)
    hs = [store.open() for _ in HAND]
    store.apply(list(zip(hs, HAND)))
    srcs = {h: enc_source(store, h) for h in hs}
    empty = store.open()
    blank = [getattr(store.read(empty)[1], f).tobytes() for f in READ]
    rows = clock_rows(8, (3, 2, 1), (2, 1))
    new, bid = store.fork_submit([hs[0], hs[3]], clocks=rows, order=order_rows(8, [[2, 1, 0], [1, 0]]), min_clock=True)
    assert (store.wait().docs["status"] == 0).all() and store.info(new[0])["n_changes"] == 6
    store._check(store._L.hm_batch_undo(store._h, bid), "hm_batch_undo")
    assert store._L.hm_batch_undo(store._h, bid) != 0                       # once only
    for f in new:
        inf = store.info(f)
        assert (inf["n_changes"], inf["n_deps"], inf["n_ops"], inf["n_regs"], inf["n_actors"], inf["hist_len"]) == (0,) * 6
        assert [getattr(store.read(f)[1], x).tobytes() for x in READ] == blank
    # the same handles take another fork (of other parents, in history order, without a minimumClock)
    reqs = requests(srcs, [hs[2], hs[1]], [3, 9], None, None)
    again, _ = store.fork_submit([hs[2], hs[1]], history=[3, 9], into=new)
    res = store.wait()
    assert again == new and [int(x) for x in res.docs["hist_len"]] == [3, 3]
    check_forks(store, ctl, reqs, [hs[2], hs[1]], new, res)
    assert store.fork([hs[0]], history=[2], min_clock=True) and int(store.fork_result.docs["status"][0]) == 0
    for h in hs:
        b, r = store.read(h)
        assert_same(b, r, O.merge(b))


# ---- minimumClock ---------------------------------------------------------------------------------
def test_min_clock_flag(engine):
    """The parent's minimumClock {aaaa: 3, bbbb: 2} (set before its changes arrive): a fork below it
    compares as the parent did then, a fork without the flag has none (min_cmp of the empty clock)."""
    store = DocStore(engine, a_stride=8)
    p, q = store.open(), store.open()
    store.apply([(p, HAND[0][2:3]), (q, HAND[0][2:3])])                      # aaaa:1: the actor tables exist
    store.apply([(p, [ch(B, 1, {A: 1}, s("y", 1))]), (q, [ch(B, 1, {A: 1}, s("y", 1))])])
    store.set_min_clock(p, {A: 3, B: 2})
    rest = [c for c in HAND[0] if (c["actor"], c["seq"]) not in ((A, 1), (B, 1))]
    rp = store.apply([(p, rest), (q, rest)])
    below, at = clock_rows(8, (2, 1)), clock_rows(8, (3, 2))
    with_flag = store.fork([p, p], clocks=np.concatenate([below, at]), order=order_rows(8, [[0, 1], [1, 0]]), min_clock=True)
    r_on = store.fork_result
    without = store.fork([p, p], clocks=np.concatenate([below, at]), order=order_rows(8, [[0, 1], [1, 0]]))
    r_off = store.fork_result
    plain = store.fork([q, q], clocks=np.concatenate([below, at]), order=order_rows(8, [[0, 1], [1, 0]]), min_clock=True)
    r_plain = store.fork_result
    # the control: fresh documents with that minimumClock receiving the same changes in one round
    c1, c2 = store.open(), store.open()
    pick = lambda n: [c for c in HAND[0] if (c["actor"], c["seq"]) in n]
    store.apply([(c1, pick([(A, 1)])), (c2, pick([(A, 1)]))])
    store.apply([(c1, pick([(B, 1)])), (c2, pick([(B, 1)]))])
    store.set_min_clock(c1, {A: 3, B: 2})
    store.set_min_clock(c2, {A: 3, B: 2})
    rc = store.apply([(c1, pick([(A, 2)])), (c2, pick([(A, 2), (A, 3), (B, 2)]))])
    assert [int(x) for x in r_on.docs["min_cmp"]] == [int(x) for x in rc.docs["min_cmp"]]
    assert int(r_on.docs["min_cmp"][0]) != int(r_on.docs["min_cmp"][1])       # below it, then satisfied
    # without the flag, and from a parent that has none: the comparison with no minimumClock
    assert [int(x) for x in r_off.docs["min_cmp"]] == [int(x) for x in r_plain.docs["min_cmp"]] == [int(rp.docs["min_cmp"][1])] * 2
    # the fork keeps the row: its next change is compared with it
    nxt = [ch(A, 3, {B: 1}, s("x", 3))]
    r2 = store.apply([(with_flag[0], nxt), (without[0], nxt), (c1, nxt)])
    assert int(r2.docs["min_cmp"][0]) == int(r2.docs["min_cmp"][2])
    assert int(r2.docs["status"].max()) == 0


# ---- a fork lives on ------------------------------------------------------------------------------
def one_doc(b, S):
    return Batch(b.docs.copy(), b.changes.copy(), b.deps.copy(), b.ops.copy(), S)


def tail_batch(src, S, p):
    """The applied changes at history positions >= p, in history order, as a one-document batch."""
    hist = np.where(src.hist >= p, src.hist - p, -1).astype(np.int32)
    return gather([(src._replace(hist=hist), len(src.changes), None)], S)[0]


def append_doc(a, b, S):
    """One document's rows a followed by its later rows b (both one-document batches of its id space)."""
    d = a.docs.copy()
    cb = b.changes.copy()
    cb["dep_off"] += len(a.deps)
    cb["op_first"] += len(a.ops)
    d["n_changes"], d["n_deps"], d["n_ops"] = len(a.changes) + len(cb), len(a.deps) + len(b.deps), len(a.ops) + len(b.ops)
    return Batch(d, np.concatenate([a.changes, cb]), np.concatenate([a.deps, b.deps]), np.concatenate([a.ops, b.ops]), S)


@pytest.mark.parametrize("mode", [None, 2])
def test_a_fork_lives_on(engine, mode):
    """Parents hold all but their last three history entries.  Forked at the parent's clock and at a
    clock below it, in a random actor order; then the withheld changes go to parent, fork and control
    in one round (incrementally where the plan routes them so).  Parent, fork and control equal the
    oracle on their logs, and waiting, missing_changes and op_diffs answer for the fork as for its
    control."""
    from hypermerge_amd import synth
    b = synth.generate(synth.config("C5", n_docs=24, arrival=2, shuffle_pct=30, dup_pct=0))
    S, n = b.a_stride, b.n_docs
    full = O.merge(b)
    assert (full.docs["status"] == 0).all()
    store, ctl = RowStore(engine, a_stride=S), RowStore(engine, a_stride=S)
    if mode is not None:
        store.set_incremental(mode)
        ctl.set_incremental(mode)
    rng = np.random.default_rng(11)
    whole = [source_of(b, full.hist, i) for i in range(n)]
    cut = [max(hist_len(w) - 3, 0) for w in whole]
    head = [gather([(w, p, None)], S)[0] for w, p in zip(whole, cut)]
    tail = [tail_batch(w, S, p) for w, p in zip(whole, cut)]
    cat = lambda parts: gather([(source_of(x, np.arange(len(x.changes)), 0), len(x.changes), None) for x in parts], S)[0]
    p0 = store.open_n(n)
    ps = np.arange(p0, p0 + n, dtype=np.uint32)
    store.submit_batch(cat(head), ps)
    assert (store.wait().docs["status"] == 0).all()
    srcs = {int(h): source_of(x, O.merge(x).hist, 0) for h, x in zip(ps, head)}
    # even requests: the parent's whole clock; odd ones: a cut below it
    rows, order = np.zeros((n, S), np.uint32), []
    for i, h in enumerate(ps):
        top = clock_at(srcs[int(h)], S, 1 << 30).astype(np.int64)
        rows[i] = top if i % 2 == 0 else rng.integers(0, top + 1)
        order.append([int(x) for x in rng.permutation(srcs[int(h)].n_actors)])
    reqs = requests(srcs, ps, None, rows, order)
    new = store.fork(ps, clocks=rows, order=order_rows(S, order))
    want, cs = check_forks(store, ctl, reqs, ps, new, store.fork_result, oracle=set(range(0, n, 5)))
    # the withheld round
    late = cat(tail)
    store.submit_batch(cat(tail + tail), np.concatenate([ps, np.asarray(new, np.uint32)]))
    rs = store.wait()
    ctl.submit_batch(late, cs)
    rc = ctl.wait()
    assert (rs.docs["status"] == 0).all() and (rc.docs["status"] == 0).all()
    if mode == 2:
        assert store.last_routing()["incremental"] > 0
    for f in ("docs", "clock", "back_clock", "heads"):
        same_bytes(getattr(rs, f)[n:], getattr(rc, f), "the withheld round: " + f)
    queued = 0
    for i in range(n):
        fork_rows = gather_fork([reqs[i]], S)[0]
        for h, log in ((int(ps[i]), append_doc(head[i], tail[i], S)), (new[i], append_doc(fork_rows, tail[i], S))):
            _, r = store.read(h)
            assert_same(log, r, O.merge(log))
        _, fr = store.read(new[i])
        _, cr = ctl.read(int(cs[i]))
        for f in READ:
            same_bytes(getattr(fr, f), getattr(cr, f), (i, f))
        queued += int(fr.docs["n_queued"][0])
    assert queued > 0                                            # below the parent's clock the late changes wait
    fh = np.asarray(new, np.uint32)
    for x, y in zip(store.waiting(fh), ctl.waiting(cs)):
        same_bytes(x, y, "waiting")
    have = [[(a, int(q)) for a, q in enumerate(rows[i] // 2) if a < srcs[int(ps[i])].n_actors] for i in range(n)]
    (ga, gc), (wa, wc) = store.missing_changes_rows(fh, have), ctl.missing_changes_rows(cs, have)
    assert ga == wa and sum(len(x) for x in ga) > 0
    same_bytes(gc, wc, "missing_changes: closure")
    hl = np.array([store.info(int(h))["hist_len"] for h in fh], np.uint32)
    for lists in (False, True):
        got, wnt = store.op_diffs(fh, np.zeros(n, np.uint32), hl, lists=lists), ctl.op_diffs(cs, np.zeros(n, np.uint32), hl, lists=lists)
        for x, y in zip(got, wnt):
            same_bytes(x, y, ("op_diffs", lists))


# ---- arena growth ---------------------------------------------------------------------------------
def test_a_fork_whose_rows_exceed_the_arenas_free_rows(engine):
    """Nine forks of a 4,200-change document (an 8,192-row change segment each) into arenas with fewer
    free rows: the submit compacts the store — the source segments the gather read move — and plans again."""
    S, k = 8, 4200
    b = encode([[ch(A if q % 3 else B, (q - q // 3) if q % 3 else q // 3, {}, s("k%d" % (q % 9), q)) for q in range(1, k + 1)]], S)
    full = O.merge(b)
    assert int(full.docs["status"][0]) == 0 and int(full.docs["hist_len"][0]) == k
    store, ctl = RowStore(engine, a_stride=S), RowStore(engine, a_stride=S)
    h = store.open_n(1)
    store.submit_batch(b, np.array([h], np.uint32))
    assert int(store.wait().docs["status"][0]) == 0
    srcs = {h: source_of(b, full.hist, 0)}
    a0 = store.arena()
    free = [c - u for c, u in zip(a0["cap"], a0["used"])]
    n = 9
    top = full.clock[:S].astype(np.int64)
    rows = np.stack([np.maximum(top - i, 0) for i in range(n)]).astype(np.uint32)
    seg = 8192                                                   # rows of a segment made for 4,100 .. 4,200 rows
    assert (k - 2 * n) + (k - 2 * n) // 4 > seg // 2 and k + k // 4 <= seg
    assert n * seg > free[0] and n * seg > free[2], (free, "the forks' segments must not fit the free rows")
    order = [[0, 1] if i % 2 else [1, 0] for i in range(n)]
    new, want = fork_and_check(store, ctl, srcs, [h] * n, clocks=rows, order=order, oracle={0, n - 1})
    a1 = store.arena()
    assert a1["cap"][0] > a0["cap"][0] and a1["cap"][2] > a0["cap"][2]      # compacted
    _, r = store.read(h)
    assert_same(b, r, full)


# ---- fuzz -----------------------------------------------------------------------------------------
FUZZ_SEEDS = tuple(range(9100, 9140))


def test_fuzz_documents_at_random_clocks_and_orders(engine):
    """40 documents of the full-vocabulary generator (counters, tables, nested lists and texts, queued
    and duplicate deliveries), each at a random clock in a random actor order and in history order."""
    docs = gen_docs("default", FUZZ_SEEDS)
    S = 8
    store, ctl = DocStore(engine, a_stride=S), RowStore(engine, a_stride=S)
    hs = [store.open() for _ in docs]
    res = store.apply(list(zip(hs, docs)))
    assert (res.docs["status"] == 0).all()                       # no document is skipped
    srcs = {h: enc_source(store, h) for h in hs}
    rng = np.random.default_rng(13)
    rows = np.stack([rng.integers(0, res.clock[h].astype(np.int64) + 2) for h in hs]).astype(np.uint32)
    order = [[int(x) for x in rng.permutation(srcs[h].n_actors)] for h in hs]
    new, want = fork_and_check(store, ctl, srcs, hs, clocks=rows, order=order)
    old, plain = fork_and_check(store, ctl, srcs, hs, clocks=rows)
    assert int(want.docs["n_changes"].sum()) > 300
    keys = lambda b, i: [(int(c["actor"]), int(c["seq"])) for c in
                         b.changes[int(b.docs["change_off"][i]):int(b.docs["change_off"][i]) + int(b.docs["n_changes"][i])]]
    differ = [i for i in range(len(hs)) if keys(want, i) != keys(plain, i)]
    assert len(differ) >= 10 and all(sorted(keys(want, i)) == sorted(keys(plain, i)) for i in range(len(hs)))
    # a fork whose two histories differ still ends in the same state where nothing is left queued
    done = [i for i in differ if not store.read(new[i])[1].docs["n_queued"][0] and not store.read(old[i])[1].docs["n_queued"][0]]
    assert done
    for i in done:
        a, c = store.read(new[i])[1], store.read(old[i])[1]
        for f in ("clock", "heads"):
            same_bytes(getattr(a, f), getattr(c, f), (i, f))
        assert int(a.docs["n_surv"][0]) == int(c.docs["n_surv"][0])
