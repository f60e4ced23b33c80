"""What blocked documents wait for, on the device (hm_store_blocked / hm_store_waiting /
hm_store_read_queue / hm_missing_deps_*) against Automerge 0.12 getMissingDeps restated in
tests/waiting_ref.py and applied to the CPU oracle's merge of the same log."""
import ctypes

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import CBatch, CResults, decode_doc, encode
from hypermerge_amd.engine import EngineError
from hypermerge_amd.store import DocStore, slice_changes
import oracle.oracle as O

from kat_cases import ch, s
from test_store_gpu import split
from test_waiting_host import HAND, OWN_DEP_ABOVE_SEQ, A, B, Cc
from waiting_ref import doc_ref, unmet_min

pytestmark = pytest.mark.gpu


def expected(store, h):
    """(missing row, queue, oracle n_queued) of a resident document from the oracle's merge of its log."""
    b = store.enc[h].log_batch(store.S)
    o = O.merge(b)
    row, q = doc_ref(b, o, 0)
    return row, q, int(o.docs["n_queued"][0])


def check_handles(store, hs):
    """waiting + queues of the listed handles equal the restatement; returns the blocked ones."""
    hs = list(hs)
    miss, unmet, nq = store.waiting(hs)
    off, q = store.queues(hs, nq)
    blocked = []
    for j, h in enumerate(hs):
        row, queue, n_queued = expected(store, h)
        np.testing.assert_array_equal(miss[j], row, err_msg=f"handle {h}")
        assert [int(x) for x in q[off[j]:off[j + 1]]] == queue, h
        assert int(nq[j]) == len(queue) == n_queued, h
        assert not unmet[j].any(), h
        if queue:
            blocked.append(h)
    return blocked


def named(store, h, row):
    return {store.enc[h].actors[a]: int(v) for a, v in enumerate(row) if v}


def test_known_answers(engine):
    store = DocStore(engine, a_stride=8)
    cases = HAND + [OWN_DEP_ABOVE_SEQ]
    hs = [store.open() for _ in cases]
    empty = store.open()
    store.apply([(h, c[1]) for h, c in zip(hs, cases)])
    miss, unmet, nq = store.waiting(hs + [empty])
    want_blocked = []
    for j, (h, (name, _, _, want, queue)) in enumerate(zip(hs, cases)):
        assert named(store, h, miss[j]) == want, name
        assert store.queue(h) == queue, name
        assert int(nq[j]) == len(queue), name
        assert store.missing_deps(h) == want, name
        if queue:
            want_blocked.append(h)
    assert not miss[-1].any() and int(nq[-1]) == 0 and store.queue(empty) == []
    assert not unmet.any()
    assert [int(x) for x in store.blocked()] == want_blocked
    assert check_handles(store, hs + [empty]) == want_blocked
    # the next round delivers what own_gap waits for
    h = hs[0]
    assert HAND[0][0] == "own_gap"
    store.apply([(h, [ch(A, 2, {A: 1}, s("x", 2))])])
    assert store.missing_deps(h) == {} and store.queue(h) == []
    assert [int(x) for x in store.blocked()] == want_blocked[1:]
    assert store.info(h)["n_queued"] == 0 and store.info(h)["hist_len"] == 3


def test_unmet_minimum_clock(engine):
    store = DocStore(engine, a_stride=8)
    h, h2 = store.open(), store.open()
    changes = [ch(A, 1, {}, s("x", 1)), ch(A, 2, {}, s("x", 2)), ch(B, 1, {}, s("y", 1))]
    store.apply([(h, changes), (h2, changes)])
    store.set_min_clock(h, {A: 3, B: 1})
    _, g = store.read(h)
    assert named(store, h, g.back_clock) == {A: 2, B: 1}
    miss, unmet, nq = store.waiting([h, h2])
    assert named(store, h, unmet[0]) == {A: 3}
    np.testing.assert_array_equal(unmet[0], unmet_min(g.back_clock, [3, 1, 0, 0, 0, 0, 0, 0]))
    assert not unmet[1].any() and not miss.any() and not nq.any()


def test_queue_longer_than_a_wave(engine):
    """99 queued changes behind 70 applied ones: the queue spans several 64-lane strides."""
    store = DocStore(engine, a_stride=8)
    h = store.open()
    changes = [ch(B, k, {}, s("y", k)) for k in range(1, 71)] + [ch(A, k, {}, s("x", k)) for k in range(2, 101)]
    store.apply([(h, changes)])
    q = store.queue(h)
    assert q == list(range(70, 169))
    assert check_handles(store, [h]) == [h]
    assert store.missing_deps(h) == {A: 99}            # A:100 needs A:99, the largest need


@pytest.mark.parametrize("S,n_actors", [(16, 9), (16, 16), (256, 65), (256, 200)])
def test_wide_rows(engine, S, n_actors):
    """One change depends on every other actor's first change; every second one is withheld."""
    actors = [f"w{i:03d}" for i in range(n_actors - 1)]
    last = "zzzz"
    held = actors[1::2]
    changes = [ch(a, 1, {}, s("k%d" % (i % 5), i)) for i, a in enumerate(actors) if a not in held]
    changes.append(ch(last, 1, {a: 1 for a in actors}, s("all", 1)))
    changes += [ch(a, 3, {}, s("late", 3)) for a in held[:3]]              # own-actor gaps on wide ranks
    store = DocStore(engine, a_stride=S)
    h = store.open()
    store.apply([(h, changes)])
    want = {a: 1 for a in held}
    want.update({a: 2 for a in held[:3]})
    assert store.missing_deps(h) == want
    assert check_handles(store, [h]) == [h]
    assert [int(x) for x in store.blocked()] == [h]


@pytest.mark.parametrize("name,n,rounds,extra", [
    ("C2", 300, 6, {"arrival": 2, "shuffle_pct": 30}),
    ("C5", 400, 5, {}),
    ("C4", 200, 4, {"arrival": 2, "shuffle_pct": 30}),
])
def test_rounds(engine, name, n, rounds, extra):
    """The feeds of test_store_gpu.py::test_incremental_parity: after every round blocked() is
    exactly the oracle's documents with n_queued > 0 and their rows / queues are as restated."""
    b = synth.generate(synth.config(name, n_docs=n, **extra))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    rng = np.random.default_rng(7)
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in docs]
    parts = [split(c, rounds, rng) for c in docs]
    for rd in range(rounds):
        items = [(h, parts[i][rd]) for i, h in enumerate(hs) if rd == 0 or parts[i][rd]]
        res = store.apply(items)
        assert (res.docs["status"] == 0).all(), res.docs["status"]
        want = [h for h in hs if expected(store, h)[2] > 0]
        got = [int(x) for x in store.blocked()]
        print(f"{name} round {rd}: {len(want)} of {n} blocked")
        assert got == want
        assert check_handles(store, got) == got
        if rd < rounds - 1:
            assert 5 * len(want) >= n, (rd, len(want))       # the comparison is not vacuous
        else:
            assert not want


def test_errors_and_edges(engine):
    store = DocStore(engine, a_stride=8)
    L = store._L
    hs = [store.open() for _ in range(4)]
    store.apply([(hs[0], HAND[0][1]), (hs[1], HAND[7][1]), (hs[2], HAND[5][1]), (hs[3], HAND[3][1])])
    n = ctypes.c_uint32()
    out = np.full(4, 0xFFFFFFFF, np.uint32)
    assert L.hm_store_blocked(store._h, out.ctypes.data, 2, ctypes.byref(n)) == 34      # HM_ERR_NOMEM
    assert n.value == 3
    assert L.hm_store_blocked(store._h, out.ctypes.data, 3, ctypes.byref(n)) == 0
    assert n.value == 3 and list(out) == [hs[0], hs[2], hs[3], 0xFFFFFFFF]
    with pytest.raises(EngineError, match="bad handle"):
        store.waiting([hs[0], 9999])
    with pytest.raises(EngineError, match="bad handle"):
        store.queues([9999], [0])
    with pytest.raises(EngineError):                     # a queue length that is not the document's
        store.queues([hs[0]], [2])
    # more than 256 requests, handles repeated
    req = [hs[i % 4] for i in range(300)] + [hs[2]] * 30
    miss, _, nq = store.waiting(req)
    off, q = store.queues(req, nq)
    one = {h: expected(store, h) for h in hs}
    for j, h in enumerate(req):
        np.testing.assert_array_equal(miss[j], one[h][0])
        assert [int(x) for x in q[off[j]:off[j + 1]]] == one[h][1]
    # out_off may start past zero (rows before it are the caller's) and must not decrease
    two = np.array([hs[3], hs[0]], np.uint32)
    offs = np.array([5, 7, 8], np.uint32)
    rows = np.full(9, 0xFFFFFFFF, np.uint32)
    assert L.hm_store_read_queue(store._h, 2, two.ctypes.data, offs.ctypes.data, rows.ctypes.data) == 0
    assert list(rows) == [0xFFFFFFFF] * 5 + one[hs[3]][1] + one[hs[0]][1] + [0xFFFFFFFF]
    offs = np.array([2, 1, 2], np.uint32)
    assert L.hm_store_read_queue(store._h, 2, two.ctypes.data, offs.ctypes.data, rows.ctypes.data) == 32   # HM_ERR_INVALID
    # a batch in flight
    store.submit([(hs[1], [ch(Cc, 2, {}, s("z", 2))])])
    with pytest.raises(EngineError, match="in flight"):
        store.blocked()
    with pytest.raises(EngineError, match="in flight"):
        store.waiting([hs[0]])
    with pytest.raises(EngineError, match="in flight"):
        store.queues([hs[0]], [1])
    store.wait()
    assert [int(x) for x in store.blocked()] == hs


def _cold_batches():
    b = synth.generate(synth.config("C2", n_docs=300, arrival=2, shuffle_pct=30))
    nch = b.docs["n_changes"].astype(np.int64)
    part = slice_changes(b, np.zeros(b.n_docs, np.int64), nch * 2 // 3)
    part.docs["reg_off"] = np.cumsum(part.docs["n_regs"]) - part.docs["n_regs"]       # (a cold batch's own output rows)
    bad = [ch(A, 1, {}, s("x", 1)), ch(A, 1, {}, s("x", 2)), ch(A, 3, {}, s("x", 3))]     # INCONSISTENT_SEQ
    hand = encode([c[1] for c in HAND[:4]] + [bad] + [c[1] for c in HAND[4:]], 8)
    return part, hand


def test_cold_batches(engine):
    import torch
    dev = torch.device("cuda", 0)
    part, hand = _cold_batches()
    for b, min_blocked in ((part, b_min(part)), (hand, 1)):
        o = O.merge(b)
        r = engine.merge(b)
        got = engine.missing_deps(b, r)
        want = np.stack([doc_ref(b, o, d)[0] for d in range(b.n_docs)])
        np.testing.assert_array_equal(got, want)
        assert (want.any(axis=1) == ((o.docs["n_queued"] > 0) & (o.docs["status"] == 0))).all()
        assert int(want.any(axis=1).sum()) >= min_blocked
        # the same from device tensors
        t = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)
             for x in (b.docs, b.changes, b.deps, r.docs, r.clock, r.hist)]
        out = torch.zeros(b.n_docs * b.a_stride, dtype=torch.int32, device=dev)
        cb = CBatch(b.n_docs, len(b.changes), len(b.deps), len(b.ops), 0, b.a_stride, 0, 0, 0, 0, 0, 0,
                    t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), None, None)
        cr = CResults(t[3].data_ptr(), t[4].data_ptr(), None, None, t[5].data_ptr(), None, None, None)
        torch.cuda.synchronize()
        engine.missing_deps_device(cb, cr, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32).reshape(b.n_docs, b.a_stride), want)
    o = O.merge(hand)
    assert int(o.docs["status"][4]) == 1 and not engine.missing_deps(hand, engine.merge(hand))[4].any()


def b_min(b):
    return b.n_docs // 5
