"""The general merge kernel (csrc/merge_large.hip) on the edge documents of tests/general_edges.py:
two documents per run-time size comparison, one on each side of it.

Parity runs on the product library in this process: both engines against the oracle, bit for bit,
each pair alone, after 400 small fuzz documents of mixed routes in the same batch (more documents
than the launch has workgroups, so a workgroup meets an edge document with another route's LDS and
scratch behind it) and before them.

The census runs on the check library (libhmgpu_check.so, HM_PATH_CENSUS) in a child process:
every edge document merged alone by the general-only engine must move exactly the census slots
general_edges.route() predicts from its shape, so a pair "for the LDS path" cannot go on passing
down the pool path.

The wall times in the docstrings are whole-test times on an MI355X host, reference side included."""
import json
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

from hypermerge_amd.columnar import encode
from hypermerge_amd.render import canonical_json
import oracle.oracle as O

from general_edges import RES_EXITS, SLOTS, UNREACHED_EXITS, YES_NO, clear_hint, encode_pair, pairs
from test_fuzz_docs import default_docs
from test_gpu_parity import assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_LIB = os.path.join(ROOT, "hypermerge_amd", "_lib", "libhmgpu_check.so")
TABLES = ("docs", "clock", "back_clock", "heads", "hist", "all_deps", "regs", "surv")
N_FILLERS = 400

pytestmark = pytest.mark.gpu


def parity(eng, b, o, rows):
    g = eng.merge(b)
    assert assert_same(b, g, o) == 0
    assert (g.docs["status"] == 0).all()
    for d in rows:
        assert canonical_json(b, g, d) == canonical_json(b, o, d), d
    return g


@pytest.mark.parametrize("p", pairs(), ids=[p.name for p in pairs()])
def test_pair_alone(engine, engine_general, p):
    """Wall under 0.2 s a case, but 1.6 s for the 32,766-register chains, 0.8 s for the 19,201-change
    chains and 0.5 s for the 65,536-op chains."""
    b = encode_pair(p)
    o = O.merge(b)
    assert (o.docs["status"] == 0).all()
    parity(engine, b, o, range(2))
    parity(engine_general, b, o, range(2))


@lru_cache(maxsize=None)
def mixed(edges_first):
    """(batch, oracle, rows of the edge documents): every pair's two documents after / before the fillers"""
    edge_docs = [d for p in pairs() for d in p.docs]
    unhinted = [2 * i + k for i, p in enumerate(pairs()) if not p.list_hint for k in range(2)]
    fillers = list(default_docs()[:N_FILLERS])
    first = 0 if edges_first else len(fillers)
    b = encode(edge_docs + fillers if edges_first else fillers + edge_docs)
    clear_hint(b, [first + r for r in unhinted])
    o = O.merge(b, threads=8)
    assert (o.docs["status"] == 0).all()
    return b, o, range(first, first + len(edge_docs))


@pytest.mark.parametrize("edges_first", [False, True], ids=["after_fillers", "before_fillers"])
def test_pairs_among_small_documents(engine, engine_general, edges_first):
    """Every pair in one batch with 400 small documents, merged twice by each engine: bit-exact with
    the oracle, and the second merge's bytes equal the first's.  Wall 5 s a case."""
    b, o, rows = mixed(edges_first)
    for eng in (engine, engine_general):
        g1 = parity(eng, b, o, rows)
        g2 = eng.merge(b)
        for f in TABLES:
            assert getattr(g1, f).tobytes() == getattr(g2, f).tobytes(), f


SCRIPT = r'''
import ctypes, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from hypermerge_amd import engine as E
from hypermerge_amd.columnar import encode
import oracle.oracle as O
from general_edges import SLOTS, clear_hint, pairs, route, shape_of
L = E.lib()
assert hasattr(L, "hm_debug_large_paths"), "not the check build"
L.hm_debug_large_paths.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
eng = E.Engine(0, E.GENERAL_ONLY)
cnt = (ctypes.c_ulonglong * len(SLOTS))()
def census():
    assert L.hm_debug_large_paths(cnt, len(SLOTS), 1) == len(SLOTS)
    return {s: int(v) for s, v in zip(SLOTS, cnt) if v}
from test_gpu_parity import assert_same
def same(b, g, o):
    try:
        return assert_same(b, g, o) == 0 and bool((g.docs["status"] == 0).all())
    except AssertionError as e:
        print(e, file=sys.stderr, flush=True)
        return False
census()
out = {"pairs": {}}
for p in pairs():
    r = []
    for i in range(2):
        b = clear_hint(encode([p.docs[i]]), () if p.list_hint else (0,))
        g, o = eng.merge(b), O.merge(b)
        r.append({"got": census(), "want": dict(route(shape_of(b, 0, fold=p.fold[i], late=p.late[i]))[1]), "same": same(b, g, o)})
    out["pairs"][p.name] = r
from test_general_edges_gpu import mixed
for first in (False, True):
    b, o, rows = mixed(first)
    g = eng.merge(b)
    out["mixed_" + ("before" if first else "after")] = {"got": census(), "same": same(b, g, o)}
from test_fuzz_gpu import cold
b, o, _ = cold()
g = eng.merge(b)
out["fuzz"] = {"got": census(), "same": same(b, g, o), "docs": int(b.n_docs)}
print(json.dumps(out))
'''


@lru_cache(maxsize=None)
def census_run():
    env = dict(os.environ, HMGPU_LIB=CHECK_LIB)
    p = subprocess.run([sys.executable, "-c", SCRIPT, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


needs_check = pytest.mark.skipif(not os.path.exists(CHECK_LIB), reason="check build not built (hypermerge_amd/build.py)")


@needs_check
def test_census_of_each_edge_document():
    """Each document of each pair, merged alone by the general-only engine of the check build: the
    census slots that moved are exactly those the restatement predicts (counts included), the two
    documents of a pair differ in the slots under test, and the results equal the oracle's.
    Wall 8 s (the child process: this test, the mixed batches and the fuzz corpus)."""
    got = census_run()["pairs"]
    for p in pairs():
        lo, hi = got[p.name]
        for side in (lo, hi):
            assert side["same"], p.name
            assert side["got"] == side["want"], (p.name, side)
        assert lo["got"].get(p.slots[0], 0) > 0 and hi["got"].get(p.slots[0], 0) == 0, (p.name, lo, hi)
        assert hi["got"].get(p.slots[1], 0) > 0 and lo["got"].get(p.slots[1], 0) == 0, (p.name, lo, hi)


@needs_check
@pytest.mark.parametrize("which", ["after", "before"])
def test_census_of_the_mixed_batches(which):
    """More documents than workgroups: workgroups reuse the scratch of an earlier document, and
    every document is counted once at the gate and once where it finished.  Wall 0.1 s."""
    r = census_run()["mixed_" + which]
    c = r["got"]
    assert r["same"]
    assert c.get("SCRATCH_REUSED", 0) > 0, c
    n_docs = N_FILLERS + 2 * len(pairs())
    assert c.get("GATE_PASSED", 0) + c.get("GATE_REFUSED", 0) == n_docs, c
    assert c.get("RES_DONE", 0) + c.get("POOL_DONE", 0) == n_docs, c
    assert sum(c.get(x, 0) for x in RES_EXITS) + c.get("RES_DONE", 0) == c.get("GATE_PASSED", 0), c


@needs_check
def test_census_of_the_fuzz_corpus():
    """test_fuzz_gpu.cold()'s batch (300 default, 40 wide, 6 long documents) through the same census,
    printed.  Asserted: together with the edge documents the corpus takes every exit of the all-LDS
    path that a document which merges can take (not RES_OUT_ROWS and RES_OUT_TABLE: general_edges'
    docstring) and both sides of every yes / no slot.
    Measured: of its 346 documents the corpus sends 307 through the gate and one to the end of the
    all-LDS path (167 leave it not ready, 139 for counters); every pool-path decision it takes is a
    "yes" (staged, ltab, closure in LDS, l3, lop, obj_lds, tour_lds), with all three histories and
    both survivor tests.  Hit by the edge documents alone: the exits RES_OUT_FOLD, RES_OUT_LATE,
    RES_OUT_LONG_LIST, RES_OUT_TAIL and RES_OUT_TOUR, and the "no" side of every yes / no slot
    but the scratch's.  That is a finding about the fuzz generator's sizes, not a failure.
    Wall 0.1 s."""
    run = census_run()
    fuzz = run["fuzz"]
    assert fuzz["same"]
    print("fuzz corpus:", {s: fuzz["got"].get(s, 0) for s in SLOTS})
    assert fuzz["got"].get("GATE_PASSED", 0) + fuzz["got"].get("GATE_REFUSED", 0) == fuzz["docs"]
    hit = set(fuzz["got"]) | set(run["mixed_after"]["got"])
    for r in run["pairs"].values():
        hit |= set(r[0]["got"]) | set(r[1]["got"])
    want = {x for x in RES_EXITS if x not in UNREACHED_EXITS} | {x for yn in YES_NO for x in yn}
    print("hit by the edge documents alone:", sorted(x for x in want if x not in fuzz["got"]))
    assert want <= hit, sorted(want - hit)
