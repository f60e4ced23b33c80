"""getMissingDeps: the test reference (tests/waiting_ref.py) on hand cases whose answers are written
out here from the rule (a queued change needs deps.set(actor, seq - 1); the row keeps, per actor,
the largest need opSet.clock lacks), and the new C-ABI names (no GPU here)."""
import ctypes

import numpy as np

from hypermerge_amd import engine
from hypermerge_amd.columnar import encode
import oracle.oracle as O

from kat_cases import ch, s
from waiting_ref import doc_ref, missing_deps, unmet_min

A, B, Cc = "aaaa", "bbbb", "cccc"

# (name, changes, extra actors, {actor: seq} missing, queue)
HAND = [
    ("own_gap", [ch(A, 1, {}, s("x", 1)), ch(A, 3, {A: 2}, s("x", 3))], (), {A: 2}, [1]),
    ("unknown_actor", [ch(A, 1, {B: 7}, s("x", 1))], (), {B: 7}, [0]),
    # A3 names A:1 as its dep; deps.set(A, seq - 1) makes that A:2
    ("own_dep_overridden", [ch(A, 1, {}, s("x", 1)), ch(A, 3, {A: 1}, s("x", 3))], (), {A: 2}, [1]),
    ("max_of_two", [ch(A, 1, {}, s("x", 1)), ch(B, 1, {A: 2}, s("y", 1)), ch(Cc, 1, {A: 5}, s("z", 1))], (),
     {A: 5}, [1, 2]),
    ("applied_dep_dropped", [ch(A, 1, {}, s("x", 1)), ch(B, 1, {A: 1, Cc: 4}, s("y", 1))], (), {Cc: 4}, [1]),
    # A1 waits for B1, B1 waits for A1: neither applies
    ("cycle", [ch(A, 1, {B: 1}, s("x", 1)), ch(B, 1, {A: 1}, s("y", 1))], (), {A: 1, B: 1}, [0, 1]),
    ("duplicate_copies", [ch(A, 2, {}, s("x", 2)), ch(A, 2, {}, s("x", 2))], (), {A: 1}, [0, 1]),
    ("nothing_queued", [ch(A, 1, {}, s("x", 1)), ch(B, 1, {A: 1}, s("y", 1))], (), {}, []),
]
# an own-actor dep above seq - 1 is overridden too: A3 waits for A:2, not for the A:7 it names (a kernel
# that took the larger of the two passed every case above and every generated document).  Kept out of
# HAND, whose order and last documents other tests build on.
OWN_DEP_ABOVE_SEQ = ("own_dep_above_seq", [ch(A, 1, {}, s("x", 1)), ch(A, 3, {A: 7, B: 1}, s("x", 3))], (), {A: 2, B: 1}, [1])


def test_reference_on_hand_cases():
    for name, changes, extra, want, queue in HAND + [OWN_DEP_ABOVE_SEQ]:
        b = encode([changes], 8)
        o = O.merge(b)
        row, q = doc_ref(b, o, 0)
        got = {b.doc_actors[0][a]: int(v) for a, v in enumerate(row) if v}
        assert got == want, name
        assert q == queue, name
        assert int(o.docs["n_queued"][0]) == len(queue), name
        assert (len(queue) > 0) == bool(row.any()), name


def test_reference_rows_directly():
    """missing_deps on rows written by hand (ranks 0..2): change 0 applied, change 1 a duplicate
    no-op, changes 2 and 3 queued."""
    from hypermerge_amd.columnar import CHANGE_DT, DEP_DT
    changes = np.array([(0, 0, 1, 0, 0, 0, 0), (0, 0, 1, 0, 0, 0, 0), (1, 2, 2, 0, 0, 0, 1), (2, 1, 1, 2, 0, 0, 2)], CHANGE_DT)
    deps = np.array([(0, 0, 1), (2, 0, 3), (0, 0, 4)], DEP_DT)
    m, q = missing_deps(changes, deps, [0, -2, -1, -1], [1, 0, 0, 0], 4)
    # change 2 (rank 1, seq 2): needs {0:1 (met), 2:3, 1:1}; change 3 (rank 2, seq 1): {0:4, 2:0}
    assert m == [4, 1, 3, 0] and q == [2, 3]
    np.testing.assert_array_equal(unmet_min([2, 1, 0, 0], [3, 1, 0, 0]), [3, 0, 0, 0])


def test_new_symbols_exported_with_signatures():
    L = engine.lib()
    names = ("hm_store_blocked", "hm_store_waiting", "hm_store_read_queue", "hm_missing_deps_device",
             "hm_missing_deps_host", "hm_docset_blocked", "hm_docset_waiting")
    for n in names:
        assert n in engine.EXPORTS, n
        f = getattr(L, n)
        assert f.argtypes and f.argtypes[0] is ctypes.c_void_p, n
    assert len(L.hm_store_waiting.argtypes) == 6
    assert len(L.hm_store_read_queue.argtypes) == 5
    assert len(L.hm_store_blocked.argtypes) == 4
    assert len(L.hm_missing_deps_device.argtypes) == 5
    assert len(L.hm_missing_deps_host.argtypes) == 4


def test_python_faces_exist():
    from hypermerge_amd.docset import DocSet
    from hypermerge_amd.store import DocStore
    for m in ("blocked", "waiting", "queue", "queues", "missing_deps"):
        assert callable(getattr(DocStore, m)), m
    for m in ("blocked", "waiting"):
        assert callable(getattr(DocSet, m)), m
    for m in ("missing_deps", "missing_deps_device"):
        assert callable(getattr(engine.Engine, m)), m
