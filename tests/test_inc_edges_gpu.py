"""The incremental apply passes (csrc/inc_kernels.hip) and plan_kernel's route on the rounds of
tests/inc_edges.py: two rounds per run-time limit, one on each side of it.

Parity runs on the product library in this process: each side of each pair applied to an
incremental store (the pair's mode) and to a re-merging one, the per-call results and the whole
state equal, the incremental store bit-exact with the oracle's cold merge, last_routing() exactly
what inc_edges.route() says, and the same again after one more ordinary change (a pass that
finished DONE with a damaged resident state shows there).  Then every round of a stride and mode in
one apply, among 300 small fuzz documents, the edge documents' handles opened after and before
the fillers'.

The census runs on the check library (libhmgpu_check.so, HM_INC_CENSUS) in a child process: every
side alone must move exactly the slots route() predicts, counts included.

The wall times in the docstrings are whole-test times on an MI355X host, reference side included."""
import json
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

from hypermerge_amd.store import DocStore

from inc_edges import EXITS, FAILG, FAMILY_SLOTS, PASSES, UNREACHABLE, family, follow_up, pairs
from test_fuzz_docs import default_docs
from test_store_gpu import assert_doc_matches_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_LIB = os.path.join(ROOT, "hypermerge_amd", "_lib", "libhmgpu_check.so")
TABLES = ("docs", "clock", "back_clock", "heads", "hist", "all_deps", "regs", "surv")
N_FILLERS = 300
GROUPS = sorted({(p.S, p.mode) for p in pairs()})

pytestmark = pytest.mark.gpu

def stores(engine, S, mode):
    """a fresh incremental store of the mode and a re-merging one"""
    A, B = DocStore(engine, a_stride=S), DocStore(engine, a_stride=S)
    A.set_incremental(mode)
    B.set_incremental(False)
    return A, B


@pytest.fixture
def pair_of_stores(engine):
    made = []

    def make(S, mode):
        made.append(stores(engine, S, mode))
        return made[-1]
    yield make
    for A, B in made:
        A.close()
        B.close()


def same_call(ra, rb):
    for f in ("docs", "clock", "back_clock", "heads"):
        np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg=f)


def same_state(A, ha, B, hb):
    _, ga = assert_doc_matches_oracle(A, ha)
    _, gb = B.read(hb)
    for f in TABLES:
        np.testing.assert_array_equal(getattr(ga, f), getattr(gb, f), err_msg=f)


@pytest.mark.parametrize("side", [0, 1], ids=["near", "far"])
@pytest.mark.parametrize("p", pairs(), ids=[p.name for p in pairs()])
def test_pair_side_alone(pair_of_stores, p, side):
    """Wall 0.02 s a case; 0.44 s for the round of 4,096 ops (its oracle merges, one per tile), 0.05 s for
    those of 256 changes."""
    A, B = pair_of_stores(p.S, p.mode)
    base, new = p.sides[side]
    ha, hb = A.open(), B.open()
    same_call(A.apply([(ha, base)]), B.apply([(hb, base)]))
    ra, rb = A.apply([(ha, new)]), B.apply([(hb, new)])
    got = A.last_routing()
    same_call(ra, rb)
    assert int(ra.docs["status"][0]) == p.status[side]
    assert p.status[side] or int(ra.docs["n_queued"][0]) == p.queued[side]
    same_state(A, ha, B, hb)
    assert got == p.route(side)[2], got
    nxt = follow_up(A.enc[ha], p.S, 1)
    same_call(A.apply([(ha, nxt)]), B.apply([(hb, nxt)]))
    same_state(A, ha, B, hb)


def filler_rounds():
    """(first halves, the next one to three changes) of the filler documents"""
    rng = np.random.default_rng(5)
    docs = list(default_docs()[:N_FILLERS])
    pos = [len(c) // 2 for c in docs]
    return [c[:k] for c, k in zip(docs, pos)], [c[k:k + int(rng.integers(1, 4))] for c, k in zip(docs, pos)]


def filler_routing(A):
    """last_routing() of the fillers' round applied alone"""
    first, nxt = filler_rounds()
    hs = [A.open() for _ in first]
    A.apply(list(zip(hs, first)))
    A.apply([(h, c) for h, c in zip(hs, nxt) if c])
    return A.last_routing()


@pytest.mark.parametrize("edges_first", [False, True], ids=["after_fillers", "before_fillers"])
@pytest.mark.parametrize("S,mode", GROUPS, ids=[f"s{S}m{m}" for S, m in GROUPS])
def test_pairs_in_one_call(pair_of_stores, S, mode, edges_first):
    """Every round of the stride and mode in one apply with the fillers' rounds, so that groups,
    waves and the defer / bail lists are shared; last_routing() is the sum of the predictions and
    the fillers' own.  Wall 0.45 to 0.95 s a case, the fillers' round alone included."""
    A, B = pair_of_stores(S, mode)
    first, nxt = filler_rounds()
    edges = [(p, k) for p in pairs() if (p.S, p.mode) == (S, mode) for k in range(2)]
    want = dict(filler_routing(pair_of_stores(S, mode)[0]))
    for p, k in edges:
        for f, v in p.route(k)[2].items():
            want[f] += v
    hs = {}
    for st in (A, B):
        he = [st.open() for _ in edges] if edges_first else None
        hf = [st.open() for _ in first]
        hs[st] = (he or [st.open() for _ in edges], hf)
    def items(st, edge_changes, filler_changes):
        he, hf = hs[st]
        e = [(h, c) for h, c in zip(he, edge_changes)]
        f = [(h, c) for h, c in zip(hf, filler_changes) if c]
        return e + f if edges_first else f + e
    bases, news = [p.sides[k][0] for p, k in edges], [p.sides[k][1] for p, k in edges]
    same_call(A.apply(items(A, bases, first)), B.apply(items(B, bases, first)))
    ra, rb = A.apply(items(A, news, nxt)), B.apply(items(B, news, nxt))
    got = A.last_routing()
    same_call(ra, rb)
    for (p, k), ha, hb in zip(edges, hs[A][0], hs[B][0]):
        same_state(A, ha, B, hb)
    assert got == want, (got, want)
    follow = [follow_up(A.enc[h], S, 2) for h in hs[A][0]]
    same_call(A.apply(items(A, follow, [[]] * len(first))), B.apply(items(B, follow, [[]] * len(first))))
    for ha, hb in zip(hs[A][0], hs[B][0]):
        same_state(A, ha, B, hb)


def test_actors_past_the_stride(pair_of_stores):
    """n_actors == S is the pair actors_s8; a round that would need S + 1 is refused by the store on
    the host, and the document goes on as it was.  Wall 0.02 s."""
    from hypermerge_amd.engine import EngineError
    from kat_cases import ch, s
    p = next(p for p in pairs() if p.name == "actors_s8")
    A, B = pair_of_stores(p.S, p.mode)
    base, new = p.sides[1]
    ha, hb = A.open(), B.open()
    A.apply([(ha, base)]), B.apply([(hb, base)])
    A.apply([(ha, new)]), B.apply([(hb, new)])
    assert len(A.enc[ha].actors) == p.S and A.last_routing() == p.route(1)[2]
    for st, h in ((A, ha), (B, hb)):
        with pytest.raises(EngineError):
            st.apply([(h, [ch("zz-ninth", 1, {}, s("n", 3))])])
    same_state(A, ha, B, hb)
    nxt = follow_up(A.enc[ha], p.S, 1)
    same_call(A.apply([(ha, nxt)]), B.apply([(hb, nxt)]))
    same_state(A, ha, B, hb)
    assert A.last_routing() == {"incremental": 1, "remerged": 0, "handed_back": 0}


SCRIPT = r'''
import ctypes, json, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from hypermerge_amd import engine as E
from hypermerge_amd.store import DocStore
from inc_edges import PASSES, SLOTS, follow_up, pairs, route
L = E.lib()
NS = len(PASSES) * len(SLOTS)
L.hm_debug_inc_paths.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
cnt = (ctypes.c_ulonglong * NS)()
assert L.hm_debug_inc_paths(cnt, NS, 1) == NS, "not the check build"
def census():
    assert L.hm_debug_inc_paths(cnt, NS, 1) == NS
    return {PASSES[i // len(SLOTS)] + "." + SLOTS[i % len(SLOTS)]: int(v) for i, v in enumerate(cnt) if v}
from test_store_gpu import assert_doc_matches_oracle
def exact(st, h):
    try:
        assert_doc_matches_oracle(st, h)
        return True
    except AssertionError as e:
        print(e, file=sys.stderr, flush=True)
        return False
eng = E.Engine(0)
out = {"pairs": {}, "mixed": {}, "corpora": {}}
t0 = time.time()
for p in pairs():
    r = []
    for k in range(2):
        A = DocStore(eng, a_stride=p.S)
        A.set_incremental(p.mode)
        h = A.open()
        base, new = p.sides[k]
        A.apply([(h, base)])
        census()
        A.apply([(h, new)])
        got = census()
        want = {a + "." + b: n for (a, b), n in p.route(k)[1].items() if n}
        r.append({"got": got, "want": want, "same": exact(A, h)})
        A.close()
    out["pairs"][p.name] = r
out["t_pairs"] = time.time() - t0
from test_inc_edges_gpu import GROUPS, filler_rounds
first, nxt = filler_rounds()
for S, mode in GROUPS:
    A = DocStore(eng, a_stride=S)
    A.set_incremental(mode)
    edges = [(p, k) for p in pairs() if (p.S, p.mode) == (S, mode) for k in range(2)]
    hf = [A.open() for _ in first]
    he = [A.open() for _ in edges]
    A.apply(list(zip(hf, first)) + [(h, p.sides[k][0]) for h, (p, k) in zip(he, edges)])
    census()
    A.apply([(h, c) for h, c in zip(hf, nxt) if c] + [(h, p.sides[k][1]) for h, (p, k) in zip(he, edges)])
    out["mixed"]["s%dm%d" % (S, mode)] = {"got": census(), "same": all(exact(A, h) for h in he), "routing": A.last_routing()}
    A.close()
# the corpora of test_store_gpu's C4 / C2 / C5 / C3 configurations (50 documents each) and test_fuzz_gpu's incremental leg
from hypermerge_amd import synth
from hypermerge_amd.columnar import decode_doc
from test_fuzz_docs import default_docs, gen_docs
def corpus(docs, S, hi, seed=11):
    rng = np.random.default_rng(seed)
    A = DocStore(eng, a_stride=S)
    A.set_incremental(2)
    hs = [A.open() for _ in docs]
    pos = [len(c) // 2 for c in docs]
    A.apply([(h, docs[i][:pos[i]]) for i, h in enumerate(hs)])
    census()
    tot = {}
    while any(q < len(c) for q, c in zip(pos, docs)):
        take = {i: int(rng.integers(1, hi + 1)) for i in range(len(docs)) if pos[i] < len(docs[i])}
        A.apply([(hs[i], docs[i][pos[i]:pos[i] + k]) for i, k in take.items()])
        for i, k in take.items():
            pos[i] += k
        for s, v in census().items():
            tot[s] = tot.get(s, 0) + v
    ok = all(exact(A, h) for h in hs[::7])
    A.close()
    return {"got": tot, "same": ok}
for name, extra, hi, S in (("C4", {}, 2, 8), ("C4", {}, 8, 8), ("C4", {}, 16, 8), ("C4", {}, 6, 16), ("C4", {}, 16, 12),
                           ("C2", {}, 8, 64), ("C2", {}, 24, 8), ("C5", {}, 2, 8), ("C5", {}, 12, 8),
                           ("C3", {"changes_per_actor": 120}, 20, 8)):
    b = synth.generate(synth.config(name, n_docs=20 if name == "C3" else 50, **extra))
    out["corpora"]["%s hi=%d S=%d" % (name, hi, S)] = corpus([decode_doc(b, i) for i in range(b.n_docs)], S, hi)
out["corpora"]["fuzz default S=8"] = corpus(list(default_docs()[:80]), 8, 3)
out["corpora"]["fuzz wide S=64"] = corpus(gen_docs("wide", range(10)), 64, 3, 12)
out["t_all"] = time.time() - t0
print(json.dumps(out))
'''


@lru_cache(maxsize=None)
def census_run():
    env = dict(os.environ, HMGPU_LIB=CHECK_LIB)
    p = subprocess.run([sys.executable, "-c", SCRIPT, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


needs_check = pytest.mark.skipif(not os.path.exists(CHECK_LIB), reason="check build not built (hypermerge_amd/build.py)")


def by_pass(c):
    return {P: {k.split(".", 1)[1]: v for k, v in c.items() if k.startswith(P + ".")} for P in PASSES}


@needs_check
def test_census_of_each_side():
    """Each side of each pair alone in a store of the check build: the census slots that moved are
    exactly those the restatement predicts (counts included), the pair's declared slots move as
    declared, and the state equals the oracle's.  Wall 6.9 s: the child process (4.4 s of it after the
    imports: 2.0 s the pairs), shared with the tests below."""
    got = census_run()["pairs"]
    bad = {p.name + "/" + "near far".split()[k]: got[p.name][k] for p in pairs() for k in range(2)
           if not got[p.name][k]["same"] or got[p.name][k]["got"] != got[p.name][k]["want"]}
    assert not bad, json.dumps(bad, indent=1)
    for p in pairs():
        lo, hi = got[p.name]
        s0, s1 = (".".join(x) for x in p.slots)
        assert lo["got"].get(s0, 0) > 0 and hi["got"].get(s1, 0) > 0, (p.name, lo, hi)
        if not p.plain:
            assert lo["got"].get(s0, 0) != hi["got"].get(s0, 0) and lo["got"].get(s1, 0) != hi["got"].get(s1, 0), (p.name, lo, hi)


@needs_check
@pytest.mark.parametrize("S,mode", GROUPS, ids=[f"s{S}m{m}" for S, m in GROUPS])
def test_census_of_the_mixed_call(S, mode):
    """Per pass ENTER == DONE + the exits, and every defer at G < 64 is an ENTER of WAVE or WAVE_TILED."""
    r = census_run()["mixed"]["s%dm%d" % (S, mode)]
    assert r["same"]
    c = by_pass(r["got"])
    for P in PASSES[:-1]:
        assert c[P].get("ENTER", 0) == c[P].get("DONE", 0) + sum(c[P].get(x, 0) for x in EXITS), (P, c[P])
    defers = sum(c[P].get(x, 0) for P in ("GROUP8", "GROUP16") for x in FAILG + ("DEFER_LIST",))
    if S <= 16:
        assert c["WAVE"].get("ENTER", 0) + c["WAVE_TILED"].get("ENTER", 0) >= defers
    done = sum(c[P].get("DONE", 0) for P in PASSES[:-1])
    assert done == r["routing"]["incremental"], (done, r["routing"])


@needs_check
def test_census_of_the_corpora():
    """test_store_gpu's C4 / C2 / C5 / C3 configurations at 50 documents (C3: 20) and test_fuzz_gpu's
    incremental leg through the same census, printed.  Asserted: pairs and corpora together hit every
    (family of passes, slot) that inc_edges.UNREACHABLE does not list.  The slots only the pairs hit are
    printed: that list is the finding.
    Measured: the corpora reach LONG_OPS (C4's rounds of over 8 ops), LONG_DEPS, LONG_CHANGES (stride
    12), tiles, the lane pass, both log searches in the lane and group passes, one BAIL_NO_ROOM in the
    wave pass, and of inc_meta_kernel the dirty, valid, valid-with-lists and lists-over ends.  Hit by
    the pairs alone: in every family BAIL_COUNTER, BAIL_MAKE, BAIL_NOT_READY, BAIL_OP and BAIL_ROWS;
    N_UP and TOT_OLD in the group and wave passes; BAIL_NO_ROOM in the lane and group passes;
    BAIL_LSV; and of the wave pass BAIL_INS_REG, BAIL_LP_PARENT, BAIL_LP_CLASH, BAIL_TILE_BIG,
    TILE_LATER_FAILED and SRC_LOOP.  Nothing is hit by the corpora alone.  Wall 0.01 s."""
    run = census_run()
    hit_pairs, hit_corp = set(), set()
    fam = lambda k: (family(k.split(".", 1)[0]), k.split(".", 1)[1])
    for r in run["pairs"].values():
        for side in r:
            hit_pairs |= {fam(k) for k in side["got"]}
    for name, r in run["corpora"].items():
        assert r["same"], name
        print(name, r["got"])
        hit_corp |= {fam(k) for k in r["got"]}
    print("wall of the child: pairs %.1f s, all %.1f s" % (run["t_pairs"], run["t_all"]))
    want = {(f, x) for f, slots in FAMILY_SLOTS.items() for x in slots} - set(UNREACHABLE)
    print("hit by the pairs alone:", sorted(want - hit_corp))
    print("hit by the corpora alone:", sorted(hit_corp - hit_pairs))
    assert want <= hit_pairs | hit_corp, sorted(want - hit_pairs - hit_corp)
    assert not (hit_pairs | hit_corp) & set(UNREACHABLE), (hit_pairs | hit_corp) & set(UNREACHABLE)
