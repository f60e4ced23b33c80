"""getMissingChanges / getChanges / getChangesForActor: the test reference
(tests/missing_changes_ref.py) on hand cases whose answers are written out here from the rule
(transitiveDeps folds the have-clock's entries in order, merging the named change's allDeps and then
SETTING the entry's own column; the answer is history.filter(seq > deps[actor])), the slice property
on synthetic documents, and the new C-ABI names (no GPU here)."""
import ctypes

import numpy as np

from hypermerge_amd import engine, synth
from hypermerge_amd.columnar import encode
import oracle.oracle as O

from kat_cases import ch, s
from missing_changes_ref import ONLY_LISTED, RAW, clocks_by_history, doc_ref, missing_changes

A, B, Cc, D = "aaaa", "bbbb", "cccc", "dddd"
FOR_ACTOR = RAW | ONLY_LISTED

CHAIN = [ch(B, 1, {}, s("y", 1)), ch(B, 2, {}, s("y", 2)), ch(B, 3, {}, s("y", 3)), ch(A, 1, {}, s("x", 1)),
         ch(A, 2, {B: 3}, s("x", 2))]

# (name, changes in arrival order, [(have-clock in key order, flags, log indices wanted)])
HAND = [
    # (i) A2 arrives first and waits in the queue: history is [A1, A2] = log [1, 0]
    ("history_order", [ch(A, 2, {}, s("x", 2)), ch(A, 1, {}, s("x", 1))],
     [({}, 0, [1, 0]), ({A: 1}, 0, [0]), ({A: 2}, 0, []),
      ({A: 0}, FOR_ACTOR, [1, 0]), ({A: 1}, FOR_ACTOR, [0])]),                               # (v)
    # (ii) A2's allDeps is {A:1, B:3}.  {A:2, B:1}: B is set to 1 after A2's closure raised it to 3,
    # so B2 and B3 are reported; {B:1, A:2}: the closure of A2 comes last and B stays 3
    ("entry_order", CHAIN,
     [({A: 2, B: 1}, 0, [1, 2]), ({B: 1, A: 2}, 0, []), ({A: 2}, 0, []), ({B: 3}, 0, [3, 4]), ({}, 0, [0, 1, 2, 3, 4]),
      ({B: 1}, FOR_ACTOR, [1, 2]), ({A: 0}, FOR_ACTOR, [3, 4]), ({B: 3}, FOR_ACTOR, []),                  # (v)
      ({A: 2, B: 1}, RAW, [1, 2]), ({B: 1, A: 2}, RAW, [1, 2])]),
    # (iii) A:5 is beyond what is applied (nothing folds, nothing of A is missing), B:0 is skipped,
    # cccc has no change at all (known only as the dependency dddd's queued change waits for)
    ("beyond_zero_absent", [ch(A, 1, {}, s("x", 1)), ch(A, 2, {}, s("x", 2)), ch(B, 1, {A: 1}, s("y", 1)),
                            ch(D, 1, {Cc: 1}, s("w", 1))],
     [({A: 5, B: 0, Cc: 2}, 0, [2]), ({Cc: 7}, 0, [0, 1, 2]), ({B: 0}, 0, [0, 1, 2]), ({B: 1}, 0, [1]),
      ({D: 0}, FOR_ACTOR, []), ({Cc: 0}, FOR_ACTOR, []), ({A: 5}, FOR_ACTOR, [])]),
    # (iv) log 1 is a duplicate of log 0 (a no-op), log 2 waits for B1: neither is ever reported
    ("duplicate_and_queued", [ch(A, 1, {}, s("x", 1)), ch(A, 1, {}, s("x", 1)), ch(B, 2, {}, s("y", 2)),
                              ch(A, 2, {}, s("x", 2))],
     [({}, 0, [0, 3]), ({A: 1}, 0, [3]), ({B: 1}, 0, [0, 3]), ({B: 0}, FOR_ACTOR, []), ({A: 0}, FOR_ACTOR, [0, 3])]),
]


def ranked(actors, clock):
    """the clock's entries as (rank, seq) in its key order; actors the document has never seen dropped"""
    rank = {a: i for i, a in enumerate(actors)}
    return [(rank[a], q) for a, q in clock.items() if a in rank]


def test_reference_on_hand_cases():
    for name, changes, queries in HAND:
        b = encode([changes], 8)
        o = O.merge(b)
        assert int(o.docs["status"][0]) == 0, name
        for clock, flags, want in queries:
            got, _ = doc_ref(b, o, 0, ranked(b.doc_actors[0], clock), flags)
            assert got == want, (name, clock, flags)
    # what the cases rest on
    b = encode([HAND[3][1]], 8)
    assert list(O.merge(b).hist) == [0, -2, -1, 1]
    b = encode([CHAIN], 8)
    o = O.merge(b)
    assert list(o.all_deps[4 * 8:4 * 8 + 2]) == [1, 3]          # allDeps of A2 = {A:1, B:3}


def test_for_actor_is_a_filter_by_actor():
    for name, changes, _ in HAND:
        b = encode([changes], 8)
        o = O.merge(b)
        order = sorted((int(p), i) for i, p in enumerate(o.hist) if p >= 0)
        for a in range(len(b.doc_actors[0])):
            for after in range(4):
                want = [i for _, i in order if int(b.changes[i]["actor"]) == a and int(b.changes[i]["seq"]) > after]
                assert doc_ref(b, o, 0, [(a, after)], FOR_ACTOR)[0] == want, (name, a, after)


def _slice_property(name, n_docs, extra):
    b = synth.generate(synth.config(name, n_docs=n_docs, **extra))
    o = O.merge(b)
    S = b.a_stride
    checked = 0
    for d in range(b.n_docs):
        if int(o.docs["status"][d]) != 0:
            continue
        c0, n = int(b.docs[d]["change_off"]), int(b.docs[d]["n_changes"])
        ch_rows, hist, ad = b.changes[c0:c0 + n], o.hist[c0:c0 + n], o.all_deps[c0 * S:(c0 + n) * S]
        clocks, history = clocks_by_history(ch_rows, hist, S)
        assert len(history) == int(o.docs["hist_len"][d])
        for p, clock in enumerate(clocks):
            have = [(a, q) for a, q in enumerate(clock) if q]
            got, deps = missing_changes(ch_rows, hist, ad, S, have)
            assert got == history[p:], (name, d, p)
            assert deps == clock, (name, d, p)                 # a causally closed clock is its own closure
            checked += 1
    return checked


def test_slice_property_c2():
    assert _slice_property("C2", 12, {"arrival": 2, "shuffle_pct": 30}) > 100


def test_slice_property_c5():
    assert _slice_property("C5", 12, {}) > 100


def test_new_symbols_exported_with_signatures():
    L = engine.lib()
    want = {"hm_store_missing_changes": 12, "hm_missing_changes_device": 15, "hm_missing_changes_host": 12,
            "hm_docset_missing_changes": 9}
    for n, k in want.items():
        assert n in engine.EXPORTS, n
        f = getattr(L, n)
        assert f.argtypes and f.argtypes[0] is ctypes.c_void_p and len(f.argtypes) == k, n
    assert (engine.MC_RAW, engine.MC_ONLY_LISTED) == (RAW, ONLY_LISTED)


def test_pack_entries():
    off, ea, es = engine.pack_entries(np.array([[0, 3, 0, 2], [0, 0, 0, 0], [1, 0, 0, 0]], np.uint32), 3)
    assert list(off) == [0, 2, 2, 3] and list(ea[:3]) == [1, 3, 0] and list(es[:3]) == [3, 2, 1]
    off, ea, es = engine.pack_entries([[(3, 2), (1, 3)], [], [(0, -4)]], 3)
    assert list(off) == [0, 2, 2, 3] and list(ea[:3]) == [3, 1, 0] and list(es[:3]) == [2, 3, 0]


def test_python_faces_exist():
    from hypermerge_amd.docset import DocSet
    from hypermerge_amd.store import DocStore
    for m in ("missing_changes", "missing_changes_rows", "changes_since", "changes_for_actor"):
        assert callable(getattr(DocStore, m)), m
    assert callable(DocSet.missing_changes)
    for m in ("missing_changes", "missing_changes_device"):
        assert callable(getattr(engine.Engine, m)), m
