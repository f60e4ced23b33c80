"""Resident document store (hm_store_* / hm_batch_submit / hm_batch_wait) vs the
CPU restatement: documents receive their changes over several applyChanges calls
(DocBackend.init, then applyRemoteChanges, src/DocBackend.ts:144-185); after every
call the device state of each document must be bit-exact with the oracle's cold
merge of that document's whole log, and its canonical rendering must equal the
rendering of one cold applyChanges over the concatenated changes."""
import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd import clock as C
from hypermerge_amd.columnar import decode_doc, encode
from hypermerge_amd.render import canonical_json
from hypermerge_amd.store import DocStore
import oracle.oracle as O

from kat_cases import ch, s, d, ins, mk, link
from hypermerge_amd.columnar import ROOT_ID as R

pytestmark = pytest.mark.gpu


def assert_doc_matches_oracle(store, h):
    b, g = store.read(h)
    o = O.merge(b)
    S = b.a_stride
    assert int(g.docs["status"][0]) == int(o.docs["status"][0])
    for f in ("hist_len", "n_queued", "n_surv"):
        assert int(g.docs[f][0]) == int(o.docs[f][0]), f
    for f in ("clock", "back_clock", "heads", "hist", "all_deps", "regs"):
        np.testing.assert_array_equal(getattr(g, f), getattr(o, f), err_msg=f)
    n = int(o.docs["n_surv"][0])
    np.testing.assert_array_equal(g.surv[:n], o.surv[:n])
    return b, g


def split(changes, k, rng):
    cuts = sorted(rng.integers(0, len(changes) + 1, size=k - 1)) if k > 1 else []
    parts, prev = [], 0
    for c in list(cuts) + [len(changes)]:
        parts.append(changes[prev:c])
        prev = c
    return parts


@pytest.mark.parametrize("name,n,rounds,extra", [
    ("C4", 600, 4, {}),
    ("C2", 400, 3, {}),
    ("C5", 400, 5, {}),                                   # nested maps + lists, blocked + duplicate changes
    ("C2", 300, 6, {"arrival": 2, "shuffle_pct": 30}),    # changes that wait in the queue across calls
    ("C3", 40, 3, {"changes_per_actor": 40}),             # text documents (RGA)
])
def test_incremental_parity(engine, name, n, rounds, extra):
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
        # the per-call results (RemotePatchMsg.history, DocBackend.clock) agree with the device state
        for j in rng.choice(len(items), size=min(25, len(items)), replace=False):
            h = items[j][0]
            bb, g = assert_doc_matches_oracle(store, h)
            assert int(res.docs["hist_len"][j]) == int(g.docs["hist_len"][0])
            np.testing.assert_array_equal(res.back_clock[j], g.back_clock)
    # final state: every document, and the rendering equals one cold applyChanges of all changes
    cold = encode(docs, 8)
    co = O.merge(cold)
    for i, h in enumerate(hs):
        bb, g = assert_doc_matches_oracle(store, h) if i % 7 == 0 else store.read(h)
        assert canonical_json(bb, g, 0) == canonical_json(cold, co, i), i


def test_new_actor_reranks_existing_rows(engine):
    """An actor whose id sorts before the document's existing actors arrives later:
    every earlier row is re-ranked on the device (actor order = string order)."""
    R = "00000000-0000-0000-0000-000000000000"
    store = DocStore(engine, a_stride=8)
    h = store.open()
    first = [ch("mmmm", 1, {}, s("x", 1)), ch("zzzz", 1, {}, s("x", 2)), ch("mmmm", 2, {"zzzz": 1}, s("y", 3))]
    later = [ch("aaaa", 1, {}, s("x", 9)), ch("bbbb", 1, {"mmmm": 2}, s("y", 4))]
    r1 = store.apply([(h, first)])
    assert r1.docs["status"][0] == 0
    r2 = store.apply([(h, later)])
    assert r2.docs["status"][0] == 0
    bb, g = assert_doc_matches_oracle(store, h)
    cold = encode([first + later], 8)
    assert canonical_json(bb, g, 0) == canonical_json(cold, O.merge(cold), 0)
    assert store.enc[h].actors == ["aaaa", "bbbb", "mmmm", "zzzz"]
    c, dp, op = store.log(h)
    assert list(c["actor"]) == [2, 3, 2, 0, 1]


def test_throwing_apply_rolls_back(engine):
    """A mismatched duplicate throws 'Inconsistent reuse of sequence number': the
    document keeps its previous state (DocBackend.back is not reassigned) and later
    calls merge on top of that state."""
    store = DocStore(engine, a_stride=8)
    h, h2 = store.open(), store.open()
    ok = [ch("aaaa", 1, {}, s("x", 1)), ch("bbbb", 1, {}, s("x", 2))]
    r = store.apply([(h, ok), (h2, ok)])
    assert (r.docs["status"] == 0).all()
    before = canonical_json(*store.read(h), 0)
    bad = [ch("cccc", 1, {}, s("z", 5)), ch("aaaa", 1, {}, s("x", 99))]       # seq 1 reused with new content
    r = store.apply([(h, bad), (h2, [ch("cccc", 1, {}, s("w", 1))])])
    assert r.docs["status"][0] == 1 and r.docs["status"][1] == 0
    assert canonical_json(*store.read(h), 0) == before
    assert store.info(h)["n_changes"] == 2 and store.enc[h].actors == ["aaaa", "bbbb"]
    r = store.apply([(h, [ch("cccc", 1, {"aaaa": 1}, s("x", 3))])])
    assert r.docs["status"][0] == 0
    bb, g = assert_doc_matches_oracle(store, h)
    cold = encode([ok + [ch("cccc", 1, {"aaaa": 1}, s("x", 3))]], 8)
    assert canonical_json(bb, g, 0) == canonical_json(cold, O.merge(cold), 0)


def test_arena_compaction_keeps_state(engine):
    """Enough documents and growth to overflow the initial arenas several times."""
    b = synth.generate(synth.config("C4", n_docs=3000))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in docs]
    for rd in range(4):
        r = store.apply([(h, docs[i][rd * 16:(rd + 1) * 16]) for i, h in enumerate(hs)])
        assert (r.docs["status"] == 0).all()
    cold = encode(docs, 8)
    co = O.merge(cold)
    for i in range(0, len(hs), 97):
        bb, g = assert_doc_matches_oracle(store, hs[i])
        assert canonical_json(bb, g, 0) == canonical_json(cold, co, i)


@pytest.mark.parametrize("mode", [1, 2])
def test_one_change_per_call_growth(engine, mode):
    """Text documents fed one change per call: their log segments outgrow their capacity again
    and again (a move keeps a quarter of headroom), and under mode 1 they cross the small-list
    bound (256 ops) mid-way — re-merged without element positions before it, incremental on the
    resident list order after it; every few calls and at the end the state equals the oracle's."""
    b = synth.generate(synth.config("C3", n_docs=6, changes_per_actor=320))   # ~40 changes, ~600 ops
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    store = DocStore(engine, a_stride=8)
    store.set_incremental(mode)
    hs = [store.open() for _ in docs]
    inc = 0
    for k in range(max(len(c) for c in docs)):
        items = [(h, docs[i][k:k + 1]) for i, h in enumerate(hs) if k < len(docs[i])]
        r = store.apply(items)
        assert (r.docs["status"] == 0).all(), (k, r.docs["status"])
        inc += store.last_routing()["incremental"]
        if k % 16 == 15:
            for h in hs[::2]:
                assert_doc_matches_oracle(store, h)
    assert inc > 0                                   # (past 256 ops the rounds go incremental)
    cold = encode(docs, 8)
    co = O.merge(cold)
    for i, h in enumerate(hs):
        bb, g = assert_doc_matches_oracle(store, h)
        assert canonical_json(bb, g, 0) == canonical_json(cold, co, i), i


def test_min_clock_and_clock_store(engine):
    """minimumClock comparison (DocBackend.testMinimumClockSatisfied) and the batched
    ClockStore.update(self, doc, doc.clock) flags against src/Clock.ts semantics."""
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in range(3)]
    peers = {hs[0]: {"aaaa": 2, "bbbb": 1}, hs[1]: {"aaaa": 1}, hs[2]: {"aaaa": 5, "cccc": 1}}
    first = {hs[0]: [ch("aaaa", 1, {}, s("x", 1))],
             hs[1]: [ch("aaaa", 1, {}, s("x", 1)), ch("aaaa", 2, {}, s("x", 2))],
             hs[2]: [ch("aaaa", 1, {}, s("x", 1))]}
    r = store.apply([(h, first[h]) for h in hs], extra_actors={h: list(peers[h]) for h in hs})
    for h in hs:
        store.set_min_clock(h, peers[h])
    # the min_cmp of the first merge saw empty minimum clocks; merge again with no new changes
    r = store.apply([(h, []) for h in hs])
    for j, h in enumerate(hs):
        bc = {a: int(v) for a, v in zip(store.enc[h].actors, r.back_clock[j]) if v}
        exp = {"EQ": 0, "GT": 1, "LT": 2, "CONCUR": 3}[C.cmp(bc, peers[h])]
        assert int(r.docs["min_cmp"][j]) == exp, (h, bc, peers[h])
    # ClockStore: first update writes every row; a repeat writes nothing and differs nowhere
    w, df, st = store.clock_update(hs)
    assert w.all() and not df.any()
    w, df, st = store.clock_update(hs)
    assert not w.any() and not df.any()
    # a queued change still advances DocBackend.clock (src/DocBackend.ts:135-142)
    r = store.apply([(hs[0], [ch("aaaa", 3, {}, s("y", 1))])])       # needs aaaa:2 -> queued
    assert int(r.docs["n_queued"][0]) == 1
    w, df, st = store.clock_update([hs[0]])
    assert w[0] and not df[0]
    assert int(st[0][store.enc[hs[0]].actors.index("aaaa")]) == 3


def test_bad_remap_leaves_store_unchanged(engine):
    """hm_batch_submit validates every actor re-rank row before it moves any document meta or
    arena pointer: a rejected batch leaves every document (earlier rows included) readable
    and unchanged."""
    import ctypes
    from hypermerge_amd.columnar import CBatch, DOC_DT, CHANGE_DT, DEP_DT, OP_DT
    from hypermerge_amd.engine import EngineError
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in range(2)]
    store.apply([(hs[0], [ch("bbbb", 1, {}, s("x", 1))]), (hs[1], [ch("cccc", 1, {}, s("y", 2))])])
    before = [store.read(h) for h in hs]
    # rows for both documents; the second row's remap sends the existing rank 0 out of range
    docs = np.zeros(2, DOC_DT)
    docs["n_regs"], docs["n_objs"], docs["n_actors"] = 1, 1, 1
    remap = np.tile(np.arange(8, dtype=np.uint8), (2, 1))
    remap[1, 0] = 5
    hs_arr = np.array(hs, np.uint32)
    cb = CBatch(2, 0, 0, 0, 2, 8, 0, 0, 0, 0, 0, 0, docs.ctypes.data, None, None, None, None)
    bid = ctypes.c_uint64()
    st = store._L.hm_batch_submit(store._h, ctypes.byref(cb), hs_arr.ctypes.data, remap.ctypes.data, ctypes.byref(bid))
    assert st == 32                                      # HM_ERR_INVALID, nothing in flight
    after = [store.read(h) for h in hs]
    for (b0, g0), (b1, g1) in zip(before, after):
        for f in ("docs", "clock", "back_clock", "heads", "hist", "all_deps", "regs"):
            np.testing.assert_array_equal(getattr(g0, f), getattr(g1, f), err_msg=f)
        np.testing.assert_array_equal(b0.changes, b1.changes)
    for h in hs:
        assert_doc_matches_oracle(store, h)
    # and the store still takes work
    store.apply([(hs[0], [ch("bbbb", 2, {}, s("x", 3))])])
    assert_doc_matches_oracle(store, hs[0])


@pytest.mark.parametrize("name,n,extra,hi,expect_inc,S", [
    ("C4", 300, {}, 2, 0.9, 8),                            # generation order: every arrival applies at once
    ("C4", 300, {"arrival": 1}, 3, True, 8),               # actor-major: some arrivals wait -> re-merge
    ("C2", 200, {}, 2, 0.9, 8),                            # counter sets and incs applied incrementally
    ("C5", 150, {}, 2, True, 8),                           # two lists, nested objects, duplicates
    ("C1", 1, {"changes_per_actor": 300}, 4, True, 8),     # one long two-actor document
    ("FC", 60, {}, 2, True, 8),                            # integral and f64 counters, shuffled (queued) arrivals
    ("C4", 200, {}, 6, 0.9, 16),                           # 16 lanes per document (inc_group_kernel<16>)
    ("C2", 120, {}, 8, 0.9, 64),                           # one document per wave (inc_group_kernel<64>)
    ("C4", 200, {}, 8, 0.9, 8),                            # up to 8 changes per call: the rounds of over 8 ops deferred to the wave kernel (nno > G)
    ("C3", 40, {"changes_per_actor": 240}, 2, 0.9, 8),     # text: inserts / deletes on the resident element order
    ("C3", 20, {"changes_per_actor": 30, "arrival": 2, "shuffle_pct": 20}, 3, True, 8),   # text, shuffled arrivals
    # rounds longer than the group passes hold (> 8 changes or > 64 ops): the one-lane pass
    ("C4", 200, {}, 16, 0.9, 8),
    ("C2", 150, {}, 24, 0.9, 8),                           # counters, up to 24 changes per call
    ("FC", 60, {}, 16, True, 8),                           # integral / f64 counters, shuffled arrivals
    ("C4", 120, {}, 16, 0.9, 16),
    # strides the lane pass is not instantiated for (it addresses rows with its template stride):
    # long rounds take the group passes' tiles, short ones the group pass at its own stride
    ("C2", 100, {}, 16, True, 5),
    ("C4", 100, {}, 16, True, 12),
    ("C4", 100, {}, 2, 0.9, 12),
    # ... and in tiles of the group / wave passes: list and text documents, strides over 16
    ("C3", 20, {"changes_per_actor": 120}, 20, True, 8),       # (new actors mid-way re-rank: re-merge)
    ("C5", 100, {}, 12, True, 8),
    ("C2", 80, {}, 24, 0.9, 64),
    # nested maps created as the documents go (makeMap / makeTable + link): object creation applies
    # incrementally on both passes
    ("NM", 120, {}, 2, 0.8, 8),
    ("NM", 120, {}, 12, 0.8, 8),
])
def test_incremental_apply_equals_full_remerge(engine, name, n, extra, hi, expect_inc, S):
    """applyRemoteChanges with 1..hi new changes per document per call
    (src/DocBackend.ts:169-185): the incremental path (inc_group_kernel) and the whole-log
    re-merge give identical per-call results and device state, and sampled documents are
    bit-exact with the oracle's cold merge of their log after every call."""
    if name == "FC":
        from test_gpu_parity import _float_counter_docs
        docs = _float_counter_docs(n, 31)
    elif name == "NM":
        docs = _nested_map_docs(n, 5)
    else:
        b = synth.generate(synth.config(name, n_docs=n, **extra))
        docs = [decode_doc(b, i) for i in range(b.n_docs)]
    rng = np.random.default_rng(11)
    A, B = DocStore(engine, a_stride=S), DocStore(engine, a_stride=S)
    A.set_incremental(2)                                   # (every eligible document, small list ones too)
    B.set_incremental(False)
    ha = [A.open() for _ in docs]
    hb = [B.open() for _ in docs]
    pos = [len(c) // 2 for c in docs]
    ra, rb = A.apply([(h, docs[i][:pos[i]]) for i, h in enumerate(ha)]), B.apply(
        [(h, docs[i][:pos[i]]) for i, h in enumerate(hb)])
    np.testing.assert_array_equal(ra.docs, rb.docs)
    # minimumClocks on some documents, so min_cmp moves as the clocks advance
    for i in range(0, len(docs), 5):
        mc = {}
        for c in docs[i][:pos[i] + 3]:
            mc[c["actor"]] = max(mc.get(c["actor"], 0), c["seq"])
        mc = {a: q for a, q in mc.items() if a in A.enc[ha[i]].actors}
        A.set_min_clock(ha[i], mc)
        B.set_min_clock(hb[i], mc)
    routed = {"incremental": 0, "remerged": 0, "handed_back": 0}
    rnd = 0
    while any(p < len(c) for p, c in zip(pos, docs)):
        take = {i: int(rng.integers(1, hi + 1)) for i in range(len(docs)) if pos[i] < len(docs[i])}
        items_a = [(ha[i], docs[i][pos[i]:pos[i] + k]) for i, k in take.items()]
        items_b = [(hb[i], docs[i][pos[i]:pos[i] + k]) for i, k in take.items()]
        ra, rb = A.apply(items_a), B.apply(items_b)
        for k, v in A.last_routing().items():
            routed[k] += v
        for f in ("docs", "clock", "back_clock", "heads"):
            np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg=f"{f} round {rnd}")
        for i, k in take.items():
            pos[i] += k
        for i in rng.choice(list(take), size=min(6, len(take)), replace=False):
            assert_doc_matches_oracle(A, ha[i])
        rnd += 1
    for i in range(len(docs)):
        ba, ga = A.read(ha[i])
        bb, gb = B.read(hb[i])
        for f in ("docs", "clock", "back_clock", "heads", "hist", "all_deps", "regs", "surv"):
            np.testing.assert_array_equal(getattr(ga, f), getattr(gb, f), err_msg=f"{f} doc {i}")
    if expect_inc:
        assert routed["incremental"] > 0, routed
    if isinstance(expect_inc, float):           # the share of calls applied incrementally
        assert routed["incremental"] >= expect_inc * sum(routed.values()), routed
    print(name, extra, routed)


def _nested_map_docs(n_docs, seed, n_actors=4):
    """Documents of maps and tables created as they go (makeMap / makeTable + link into ROOT or into
    an earlier map) and sets / deletes / counters on them, in generation order: every change is
    causally ready on arrival, so object creation is the only thing the incremental passes have to
    take beyond map ops."""
    import random
    rng = random.Random(seed)
    docs = []
    for di in range(n_docs):
        actors = [f"nm{di:04d}{i}" for i in range(n_actors)]
        seqs = {a: 0 for a in actors}
        heard = {a: {} for a in actors}
        objs = [R]
        chs = []
        for i in range(rng.randint(10, 50)):
            a = rng.choice(actors)
            seqs[a] += 1
            ops = []
            if rng.random() < 0.3 and len(objs) < 40:
                o = f"{di:08x}-{len(objs):04x}-4000-8000-{rng.randrange(16 ** 12):012x}"
                ops.append(mk("makeTable" if rng.random() < 0.2 else "makeMap", o))
                ops.append(link(f"k{rng.randrange(4)}", o, rng.choice(objs)))
                objs.append(o)
            for _ in range(rng.randint(1, 3)):
                obj = rng.choice(objs)
                r = rng.random()
                if r < 0.15:
                    ops.append(d(f"k{rng.randrange(4)}", obj))
                elif r < 0.25:
                    ops.append({"action": "set", "obj": obj, "key": "n", "value": rng.randint(0, 9), "datatype": "counter"})
                else:
                    ops.append(s(f"k{rng.randrange(4)}", rng.randrange(100), obj))
            deps = {b: q for b, q in heard[a].items() if b != a}
            chs.append(ch(a, seqs[a], deps, *ops))
            for b in actors:
                if b == a or rng.random() < 0.6:
                    heard[b][a] = seqs[a]
        docs.append(chs)
    return docs


def _growing_conflicts(n_cycles, actors=("a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8")):
    """One register that repeatedly goes from one survivor to eight: each cycle starts with a
    set that has seen everything (the list shrinks to one, in place), then the other actors set
    it concurrently one after another, each having seen only its own chain (the list grows by
    one per set: every growth moves the list to the end of the document's survivor slots)."""
    seq = {a: 0 for a in actors}
    out = []
    for c in range(n_cycles):
        lead = actors[c % len(actors)]
        seq[lead] += 1
        out.append(ch(lead, seq[lead], {a: q for a, q in seq.items() if a != lead and q}, s("k", c * 100)))
        for a in actors:
            if a == lead:
                continue
            seq[a] += 1
            deps = {lead: seq[lead]} if a != lead else {}
            out.append(ch(a, seq[a], deps, s("k", c * 100 + len(out) % 97), s(f"x{len(out)}", a)))
    return out


def test_survivor_slots_run_out_and_repack(engine):
    """Lists that grow faster than the op log fill a document's survivor slots: the incremental
    path then hands the document to the re-merge (which packs its survivors again) and goes on
    incrementally; every call equals the re-merge store and the oracle."""
    log = _growing_conflicts(12)
    A, B = DocStore(engine, a_stride=8), DocStore(engine, a_stride=8)
    B.set_incremental(False)
    ha, hb = A.open(), B.open()
    routed = {"incremental": 0, "remerged": 0, "handed_back": 0}
    for i in range(0, len(log), 1):
        ra, rb = A.apply([(ha, log[i:i + 1])]), B.apply([(hb, log[i:i + 1])])
        for k, v in A.last_routing().items():
            routed[k] += v
        for f in ("docs", "clock", "back_clock", "heads"):
            np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg=f"{f} call {i}")
        if i % 9 == 0:
            assert_doc_matches_oracle(A, ha)
    assert_doc_matches_oracle(A, ha)
    assert routed["incremental"] > len(log) // 2 and routed["handed_back"] > 0, routed


def test_batch_undo_restores_previous_state(engine):
    """hm_batch_undo: every document of the last waited batch back to its state before it
    (incremental and re-merged documents alike); the next batch merges on top of that."""
    b = synth.generate(synth.config("C4", n_docs=60))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in docs]
    store.apply([(h, docs[i][:40]) for i, h in enumerate(hs)])
    before = [canonical_json(*store.read(h), 0) for h in hs]
    snaps = [store.enc[h].snapshot() for h in hs]
    store.submit([(h, docs[i][40:43]) for i, h in enumerate(hs)])
    bid = store._pending[0]
    r = store.wait()
    assert (r.docs["status"] == 0).all()
    store._check(store._L.hm_batch_undo(store._h, bid), "hm_batch_undo")
    for i, h in enumerate(hs):
        store.enc[h].restore(snaps[i])
        assert canonical_json(*store.read(h), 0) == before[i], i
    assert store._L.hm_batch_undo(store._h, bid) != 0                      # once only
    store.apply([(h, docs[i][40:]) for i, h in enumerate(hs)])
    cold = encode(docs, 8)
    co = O.merge(cold)
    for i in range(0, len(hs), 7):
        bb, g = assert_doc_matches_oracle(store, hs[i])
        assert canonical_json(bb, g, 0) == canonical_json(cold, co, i)


def test_device_submit_equals_host_submit(engine):
    """hm_batch_submit_device / hm_batch_wait_device (rows already in HBM) give the host entry
    points' results and state."""
    import torch
    from hypermerge_amd.store import RowStore, slice_changes
    b = synth.generate(synth.config("C4", n_docs=500))
    n, S = b.n_docs, b.a_stride
    nch = b.docs["n_changes"].astype(np.int64)
    dev = torch.device("cuda", 0)
    A, B = RowStore(engine, a_stride=S), RowStore(engine, a_stride=S)
    ha, hb = A.open_n(n), B.open_n(n)

    def on_dev(x, hs):
        return (len(x.changes), len(x.deps), len(x.ops)), [
            torch.from_numpy(np.ascontiguousarray(y).view(np.uint8).reshape(-1)).to(dev)
            for y in (x.docs, x.changes, x.deps, x.ops, np.ascontiguousarray(hs, np.uint32))]
    pos = np.zeros(n, np.int64)
    rng = np.random.default_rng(3)
    out = torch.empty(n * (32 + 12 * S), dtype=torch.uint8, device=dev)
    first = True
    while (pos < nch).any():
        hi = np.minimum(pos + (40 if first else rng.integers(1, 4, n)), nch)
        first = False
        sel = np.nonzero(hi > pos)[0]
        sub = slice_changes(b, pos, hi, sel)
        A.submit_batch(sub, sel + ha)
        ra = A.wait()
        cnt, t = on_dev(sub, sel + hb)
        assert B.submit_device(len(sel), cnt, *t) > 0
        assert B.wait_device(out) == 0
        got = out[:len(sel) * (32 + 12 * S)].cpu().numpy()
        k = len(sel)
        np.testing.assert_array_equal(got[:k * 32].view(ra.docs.dtype), ra.docs)
        rows = got[k * 32:].view(np.uint32).reshape(3, k, S)
        np.testing.assert_array_equal(rows[0], ra.clock)
        np.testing.assert_array_equal(rows[1], ra.back_clock)
        np.testing.assert_array_equal(rows[2], ra.heads)
        pos = np.maximum(pos, hi)
    for i in range(0, n, 37):
        _, ga = A.read(ha + i)
        _, gb = B.read(hb + i)
        for f in ("hist", "all_deps", "regs", "surv", "clock", "heads"):
            np.testing.assert_array_equal(getattr(ga, f), getattr(gb, f), err_msg=f)


def _text_rounds():
    """A text object edited round by round: typing at the end, at the head, in the middle after an
    element that already has children (a larger elem counter: first child), a child under that
    child, a concurrent insert that sorts after the existing child (placed after its subtree: the
    wave pass's scan), deletes, an insert after a deleted element, a value overwrite, a run of
    inserts in one change, and a map key beside the text."""
    T = "text-1"
    A, B, C = "aaaa", "bbbb", "cccc"
    rounds = [[ch(A, 1, {}, mk("makeText", T), link("t", T), ins(T, "_head", 1), s(f"{A}:1", "h", T),
                  ins(T, f"{A}:1", 2), s(f"{A}:2", "e", T))]]
    rounds.append([ch(A, 2, {}, ins(T, f"{A}:2", 3), s(f"{A}:3", "y", T))])                    # typing at the end
    rounds.append([ch(B, 1, {A: 2}, ins(T, "_head", 4), s(f"{B}:4", "<", T))])                 # at the head
    rounds.append([ch(B, 2, {A: 2}, ins(T, f"{A}:1", 5), s(f"{B}:5", "+", T))])                # after h: first child
    rounds.append([ch(C, 1, {B: 2}, ins(T, f"{B}:5", 6), s(f"{C}:6", "c", T))])                # under that child
    rounds.append([ch(A, 3, {A: 2}, ins(T, f"{A}:1", 4), s(f"{A}:4", "x", T))])                # concurrent, sorts later
    rounds.append([ch(A, 4, {B: 2}, d(f"{A}:2", T)), ch(B, 3, {A: 3}, s(f"{A}:3", "Y", T))])    # delete, overwrite
    rounds.append([ch(B, 4, {A: 4, B: 3}, ins(T, f"{A}:2", 9), s(f"{B}:9", "!", T),             # after a deleted one
                      ins(T, f"{B}:9", 10), s(f"{B}:10", "?", T), ins(T, f"{B}:10", 11), s(f"{B}:11", ".", T),
                      s("title", "doc"))])
    rounds.append([ch(A, 5, {B: 4}, d(f"{B}:10", T), ins(T, f"{B}:11", 12), s(f"{A}:12", "z", T)),
                   ch(A, 6, {}, ins(T, f"{A}:12", 13), s(f"{A}:13", "w", T))])
    return rounds


def _lists_rounds():
    """Four list objects in one document (a list, a text, and two lists that stay empty until a
    later round, then get their first elements in one change), edited round by round: an append at the end of the first list and an insert
    at the head of the second in one change (both at the same point of the concatenated order),
    inserts in the middle, at a head, into the empty list, deletes, an overwrite, a change that
    touches every list, and a concurrent insert that sorts after an existing child."""
    L, T, E, F = "list-1", "text-2", "list-3", "list-4"
    A, B = "aaaa", "bbbb"
    rounds = [[ch(A, 1, {}, mk("makeList", L), link("l", L), mk("makeText", T), link("t", T), mk("makeList", E),
                  link("e", E), mk("makeList", F), link("f", F), ins(L, "_head", 1), s(f"{A}:1", 10, L), ins(L, f"{A}:1", 2), s(f"{A}:2", 20, L),
                  ins(T, "_head", 3), s(f"{A}:3", "x", T))]]
    rounds.append([ch(A, 2, {}, ins(L, f"{A}:2", 4), s(f"{A}:4", 30, L), ins(T, "_head", 5), s(f"{A}:5", "y", T))])
    rounds.append([ch(B, 1, {A: 2}, ins(T, f"{A}:3", 6), s(f"{B}:6", "z", T), d(f"{A}:1", L))])
    rounds.append([ch(B, 2, {A: 2}, ins(L, "_head", 7), s(f"{B}:7", 5, L), ins(F, "_head", 14), s(f"{B}:14", "F", F),
                      ins(E, "_head", 8), s(f"{B}:8", "e", E))])                               # two empty lists at one point
    rounds.append([ch(A, 3, {B: 2}, ins(E, f"{B}:8", 9), s(f"{A}:9", "f", E), s(f"{A}:4", 31, L),
                      ins(T, f"{A}:5", 10), s(f"{A}:10", "w", T), ins(L, f"{B}:7", 11), s(f"{A}:11", 6, L))])
    rounds.append([ch(B, 3, {A: 3}, ins(L, f"{B}:7", 4), s(f"{B}:4", 7, L))])                  # concurrent, sorts later
    rounds.append([ch(A, 4, {B: 3}, d(f"{A}:10", T), ins(E, "_head", 12), s(f"{A}:12", "g", E)),
                   ch(A, 5, {}, ins(L, f"{A}:4", 13), s(f"{A}:13", 40, L), s("title", "lists"))])
    return rounds


def test_incremental_edits_on_several_lists(engine):
    """The incremental path with a document's lists end to end in one resident order (the list
    directory): every call equal to the whole-log re-merge and to the oracle's cold merge."""
    rounds = _lists_rounds()
    A, B = DocStore(engine, a_stride=8), DocStore(engine, a_stride=8)
    A.set_incremental(2)                                   # (every eligible document, small list ones too)
    B.set_incremental(False)
    ha, hb = A.open(), B.open()
    routed = []
    for i, r in enumerate(rounds):
        ra, rb = A.apply([(ha, r)]), B.apply([(hb, r)])
        routed.append(A.last_routing()["incremental"])
        for f in ("docs", "clock", "back_clock", "heads"):
            np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg=f"{f} round {i}")
        assert int(ra.docs["status"][0]) == 0, (i, ra.docs)
        bb, g = assert_doc_matches_oracle(A, ha)
        _, gb = B.read(hb)
        np.testing.assert_array_equal(g.regs, gb.regs, err_msg=f"round {i}")
    assert sum(routed[1:]) == len(rounds) - 1, routed          # every round after the load: incremental


def test_rowstore_text_rounds_with_declared_registers(engine):
    """Resident text documents fed prebuilt rows whose document totals are declared up front
    (RowStore + slice_changes: n_regs is the whole log's, so a new element's register id was
    reserved but never touched): typing rounds of 1-2 changes go incremental, and every round's
    results and the final device state equal the whole-log re-merge's."""
    from hypermerge_amd.store import RowStore, slice_changes
    b = synth.generate(synth.config("C3", n_docs=24))
    n = b.n_docs
    nch = b.docs["n_changes"].astype(np.int64)
    pos = np.maximum(nch - 10, 0)
    A, B = RowStore(engine, a_stride=b.a_stride), RowStore(engine, a_stride=b.a_stride)
    A.set_incremental(2)
    B.set_incremental(False)
    ha, hb = A.open_n(n), B.open_n(n)
    for st, h0 in ((A, ha), (B, hb)):
        st.submit_batch(slice_changes(b, np.zeros(n, np.int64), pos), np.arange(h0, h0 + n))
        st.wait()
    rng = np.random.default_rng(3)
    routed = {"incremental": 0, "remerged": 0, "handed_back": 0}
    while (pos < nch).any():
        hi = np.minimum(pos + rng.integers(1, 3, n), nch)
        sel = np.nonzero(hi > pos)[0]
        sub = slice_changes(b, pos, hi, sel)
        A.submit_batch(sub, sel + ha)
        ra = A.wait()
        for k, v in A.last_routing().items():
            routed[k] += v
        B.submit_batch(sub, sel + hb)
        rb = B.wait()
        for f in ("docs", "clock", "back_clock", "heads"):
            np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg=f)
        pos = np.maximum(pos, hi)
    for i in range(n):
        _, ga = A.read(ha + i)
        _, gb = B.read(hb + i)
        for f in ("docs", "clock", "back_clock", "heads", "hist", "all_deps", "regs", "surv"):
            np.testing.assert_array_equal(getattr(ga, f), getattr(gb, f), err_msg=f"{f} doc {i}")
    assert routed["incremental"] >= 0.9 * sum(routed.values()), routed


def test_incremental_text_edits_equal_remerge_and_oracle(engine):
    """Row a11 on the incremental path: list / text ops applied on the resident element order
    (lorder / epos), each call equal to the whole-log re-merge and to the oracle's cold merge."""
    rounds = _text_rounds()
    A, B = DocStore(engine, a_stride=8), DocStore(engine, a_stride=8)
    A.set_incremental(2)                                   # (every eligible document, small list ones too)
    B.set_incremental(False)
    ha, hb = A.open(), B.open()
    routed = []
    for i, r in enumerate(rounds):
        ra, rb = A.apply([(ha, r)]), B.apply([(hb, r)])
        routed.append(A.last_routing()["incremental"])
        for f in ("docs", "clock", "back_clock", "heads"):
            np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg=f"{f} round {i}")
        assert int(ra.docs["status"][0]) == 0, (i, ra.docs)
        bb, g = assert_doc_matches_oracle(A, ha)
        _, gb = B.read(hb)
        np.testing.assert_array_equal(g.regs, gb.regs, err_msg=f"round {i}")
    assert sum(routed[1:]) == len(rounds) - 1, routed          # every round after the load: incremental


def test_default_cost_rule_on_long_c4_rounds_matches_oracle(engine):
    """The default routing (mode 1) sends a round whose new rows exceed 1/HM_INC_COST of the log to
    the re-merge and shorter ones to the incremental passes: C4 documents fed rounds of 1-24
    changes (both sides of the rule in one call) stay bit-exact with the oracle's cold merge of
    their log after every call, and both routes are taken."""
    b = synth.generate(synth.config("C4", n_docs=300))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    rng = np.random.default_rng(23)
    store = DocStore(engine, a_stride=8)            # (incremental mode 1: the default)
    hs = [store.open() for _ in docs]
    pos = [24] * len(docs)
    r = store.apply([(h, docs[i][:24]) for i, h in enumerate(hs)])
    assert (r.docs["status"] == 0).all()
    routed = {"incremental": 0, "remerged": 0, "handed_back": 0}
    while any(p < len(c) for p, c in zip(pos, docs)):
        take = {i: int(rng.choice([1, 2, 12, 24])) for i in range(len(docs)) if pos[i] < len(docs[i])}
        r = store.apply([(hs[i], docs[i][pos[i]:pos[i] + k]) for i, k in take.items()])
        assert (r.docs["status"] == 0).all()
        for k, v in store.last_routing().items():
            routed[k] += v
        for i, k in take.items():
            pos[i] += k
        for i in list(take)[::5]:
            assert_doc_matches_oracle(store, hs[i])
    assert routed["incremental"] > 0 and routed["remerged"] > 0, routed
    for h in hs:
        assert_doc_matches_oracle(store, h)


def test_inc_state_count_follows_every_writer(engine):
    """hm_store_inc_states: the documents whose resident state a submit can use, kept on the
    device by inc_meta (built / dropped after a re-merge), doc_rows (cleared for documents that keep
    none), hm_doc_reset and hm_store_set_incremental; a store with none plans whole re-merges and
    launches no incremental kernel, with results equal to a re-merge-only store."""
    b = synth.generate(synth.config("C4", n_docs=120))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    A, B = DocStore(engine, a_stride=8), DocStore(engine, a_stride=8)
    B.set_incremental(False)
    ha = [A.open() for _ in docs]
    hb = [B.open() for _ in docs]
    assert A.inc_states() == 0
    pos = [len(c) - 6 for c in docs]
    A.apply([(h, docs[i][:pos[i]]) for i, h in enumerate(ha)])
    B.apply([(h, docs[i][:pos[i]]) for i, h in enumerate(hb)])
    assert A.inc_states() == len(docs)                      # clean map documents: every one
    A.reset(ha[:10])
    B.reset(hb[:10])
    assert A.inc_states() == len(docs) - 10
    for i in range(10):
        pos[i] = 0
    # switched off and on: every state dropped; the next submit re-merges all and rebuilds them
    A.set_incremental(False)
    A.set_incremental(True)
    assert A.inc_states() == 0
    for rnd in range(3):
        items = [(i, docs[i][pos[i]:pos[i] + 2 if rnd else len(docs[i]) - 4]) for i in range(len(docs))]
        ra = A.apply([(ha[i], c) for i, c in items])
        rb = B.apply([(hb[i], c) for i, c in items])
        for f in ("docs", "clock", "back_clock", "heads"):
            np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg=f"{f} round {rnd}")
        r = A.last_routing()
        if rnd == 0:
            assert r["incremental"] == 0 and r["remerged"] == len(docs), r
        else:
            assert r["incremental"] >= 0.9 * len(docs), r
        assert A.inc_states() == len(docs)
        for i, c in items:
            pos[i] += len(c)
    # mode 1: small list documents keep no state (C5: none routes incremental, none is counted)
    b5 = synth.generate(synth.config("C5", n_docs=60))
    d5 = [decode_doc(b5, i) for i in range(b5.n_docs)]
    small = bool((b5.docs["n_ops"] <= 256).all())
    C5 = DocStore(engine, a_stride=8)
    h5 = [C5.open() for _ in d5]
    C5.apply([(h, d5[i][:len(d5[i]) - 2]) for i, h in enumerate(h5)])
    if small:
        assert C5.inc_states() == 0
    C5.set_incremental(2)
    C5.apply([(h, d5[i][len(d5[i]) - 2:len(d5[i]) - 1]) for i, h in enumerate(h5)])
    n2 = C5.inc_states()
    assert 0 < n2 <= len(d5)
