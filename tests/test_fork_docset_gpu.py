"""hm_docset_fork against a control: a second docset with the same flags whose fresh document
receives, in one apply, each listed actor's changes 1 .. k in the clock's entry order (what Repo.merge
hands a new document).  Equal as parsed JSON: the result row, the patch with DocBackend.clock and the
call's clock, view, the log's part of info, materialize_patch at the full history, and the patches of
one further identical round on both.  A fork keeps its parent's id spaces: info's a_stride / n_actors /
n_objs / n_regs must equal the parent's (not the control's), and views are compared as objects, since
hm_docset_view lists a map's keys in register order."""
import json
import random

import pytest

from hypermerge_amd.columnar import encode
from hypermerge_amd.docset import ROOT, DocSet, view_objects
import oracle.oracle as O

from fuzz_docs import gen_docs
from kat_cases import A, B, Cc, ch, s
from test_materialize_gpu import QUEUED_DUP, SHUFFLED, TEXT

pytestmark = pytest.mark.gpu

FLAVOURS = {"default": {}, "device_diffs": {"device_diffs": True}, "no_patches": {"patches": False}}
SEEDS = tuple(range(9100, 9112))
LOG_INFO = ("n_changes", "n_ops", "hist_len", "n_queued")


def blocks(changes):
    return [json.dumps(c, separators=(",", ":")).encode() for c in changes]


def first_copies(log):
    out = {}
    for c in log:
        out.setdefault((c["actor"], c["seq"]), c)
    return out


def applied_top(log):
    """opSet.clock of the log by actor id, from the oracle"""
    b = encode([log])
    o = O.merge(b)
    assert int(o.docs["status"][0]) == 0
    return {a: int(q) for a, q in zip(b.doc_actors[0], o.clock[:len(b.doc_actors[0])]) if q}


def handed_over(log, clock):
    """the changes Repo.merge hands a new document for `clock`: actor after actor in key order, seqs ascending"""
    have, top = first_copies(log), applied_top(log)
    return [have[(a, q)] for a, k in clock.items() for q in range(1, min(int(k), top.get(a, 0)) + 1)]


def rows_equal(x, y):
    return all(int(x[f]) == int(y[f]) for f in ("status", "hist_len", "n_queued", "n_surv", "min_cmp", "err_change", "err_op"))


def same_view(ds, d, ctl, c):
    """hm_docset_view lists a map's keys in register order, which a fork inherits from its parent: the
    views are compared as objects (keys by name, list elements in order)"""
    return view_objects(ds.view(d)) == view_objects(ctl.view(c))


def documents():
    return [SHUFFLED, TEXT, QUEUED_DUP] + gen_docs("default", SEEDS)


def random_clock(rng, log):
    top = applied_top(log)
    actors = list(top)
    rng.shuffle(actors)
    clock = {a: rng.randint(0, top[a] + 1) for a in actors}
    if rng.random() < 0.5:
        clock["nobody"] = 3                                      # an id the parent never saw: dropped
    return clock


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_fork_equals_a_fresh_document_fed_actor_by_actor(engine, flavour):
    kw = FLAVOURS[flavour]
    ds, ctl = DocSet(engine, **kw), DocSet(engine, **kw)
    logs = documents()
    n = len(logs)
    p0 = ds.open(n)
    parents = list(range(p0, p0 + n))
    res, _ = ds.apply(parents, [blocks(l) for l in logs])
    assert (res["status"] == 0).all()
    views = [ds.view(p) for p in parents]
    rng = random.Random(21)
    clocks = [random_clock(rng, l) for l in logs]
    clocks[0] = {B: 2, A: 3}                                     # the shuffled document, bbbb handed over first
    forks, fres, fjs = ds.fork(parents, clocks=clocks)
    assert forks == list(range(p0 + n, p0 + 2 * n))
    handed = [handed_over(l, k) for l, k in zip(logs, clocks)]
    c0 = ctl.open(n)
    ctls = list(range(c0, c0 + n))
    cres, cjs = ctl.apply(ctls, [blocks(h) for h in handed])
    differs = 0
    for i in range(n):
        assert rows_equal(fres[i], cres[i]), (i, fres[i], cres[i])
        for part in ("p", "b", "c"):
            assert fjs[part][i] == cjs[part][i], (i, part)
        assert same_view(ds, forks[i], ctl, ctls[i]), i
        fi, ci = ds.info(forks[i]), ctl.info(ctls[i])
        assert [fi[f] for f in LOG_INFO] == [ci[f] for f in LOG_INFO], i
        assert fi["n_changes"] == len(handed[i])
        pi = ds.info(parents[i])                                 # the id spaces are the parent's: its totals and class
        assert [fi[f] for f in ("a_stride", "n_actors", "n_objs", "n_regs")] == [pi[f] for f in ("a_stride", "n_actors", "n_objs", "n_regs")], i
        assert ds.view(parents[i]) == views[i]                   # the parent is only read
        keys = [(c["actor"], c["seq"]) for c in handed[i]]
        in_history = [(logs[i][j]["actor"], logs[i][j]["seq"]) for j in ds.history_prefix(parents[i], 1 << 20)]
        differs += [k for k in in_history if k in set(keys)] != keys
    assert differs >= 3                                          # the hand-over order is not the parents' history order
    # actors the fork does not hold appear nowhere
    assert "nobody" not in json.dumps(fjs)
    i = 0
    assert set(fjs["p"][i]["clock"]) == {A, B} and Cc not in json.dumps([fjs["p"][i], fjs["b"][i], fjs["c"][i], ds.view(forks[i])])
    if flavour != "no_patches":
        big = [1 << 20] * n
        got, want = ds.materialize_patch(forks, history=big, lists=True), ctl.materialize_patch(ctls, history=big, lists=True)
        for i in range(n):
            assert (got[i]["history"], got[i]["patch"]) == (want[i]["history"], want[i]["patch"]), i
    # one further round on both: everything the fork was not handed — a later block past the fork's
    # clock is applied, not dropped as a duplicate
    rest = []
    for l, h in zip(logs, handed):
        took = {(c["actor"], c["seq"]) for c in h}
        rest.append([c for k, c in first_copies(l).items() if k not in took])
    before = [ds.info(f)["hist_len"] for f in forks]
    r2, j2 = ds.apply(forks, [blocks(x) for x in rest])
    c2, k2 = ctl.apply(ctls, [blocks(x) for x in rest])
    grew = 0
    for i in range(n):
        assert rows_equal(r2[i], c2[i]), i
        for part in ("p", "b", "c"):
            assert j2[part][i] == k2[part][i], (i, part)
        assert same_view(ds, forks[i], ctl, ctls[i]), i
        grew += int(r2[i]["hist_len"]) > before[i]
        if int(r2[i]["status"]) == 0:
            assert int(r2[i]["hist_len"]) == ds.info(parents[i])["hist_len"], i     # the fork has caught up with its parent
    assert grew >= n // 2
    # a block at or below the fork's clock with other content: Automerge's inconsistent reuse, as on the control
    j = next(i for i in range(n) if handed[i])
    bad = dict(handed[j][0], ops=[dict(action="set", obj=ROOT, key="other", value=1)])
    r3, _ = ds.apply([forks[j]], [blocks([bad])])
    c3, _ = ctl.apply([ctls[j]], [blocks([bad])])
    assert int(r3[0]["status"]) != 0 and rows_equal(r3[0], c3[0])
    assert same_view(ds, forks[j], ctl, ctls[j])


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_fork_at_a_history_length_and_of_an_unplaced_parent(engine, flavour):
    kw = FLAVOURS[flavour]
    ds, ctl = DocSet(engine, **kw), DocSet(engine, **kw)
    logs = documents()[:8]
    n = len(logs)
    p0 = ds.open(n + 1)                                          # the last one never receives anything
    parents = list(range(p0, p0 + n))
    ds.apply(parents, [blocks(l) for l in logs])
    rng = random.Random(5)
    hist = [rng.randint(0, ds.info(p)["hist_len"] + 1) for p in parents]
    forks, fres, fjs = ds.fork(parents + [p0 + n], history=hist + [4])
    prefix = [[l[j] for j in ds.history_prefix(p, k)] for l, p, k in zip(logs, parents, hist)]
    c0 = ctl.open(n + 1)
    ctls = list(range(c0, c0 + n + 1))
    cres, cjs = ctl.apply(ctls, [blocks(x) for x in prefix] + [[]])
    for i in range(n + 1):
        assert rows_equal(fres[i], cres[i]), i
        for part in ("p", "b", "c"):
            assert fjs[part][i] == cjs[part][i], (i, part)
        assert same_view(ds, forks[i], ctl, ctls[i]), i
    assert [int(x) for x in fres["hist_len"][:n]] == [min(k, ds.info(p)["hist_len"]) for k, p in zip(hist, parents)]
    # the empty fork of the unplaced parent takes changes like any new document
    r, j = ds.apply([forks[n]], [blocks(SHUFFLED)])
    c, k = ctl.apply([ctls[n]], [blocks(SHUFFLED)])
    assert rows_equal(r[0], c[0]) and j == k and int(r[0]["hist_len"]) == 6
    # both selectors, neither
    with pytest.raises(Exception):
        ds.fork(parents[:1])
    with pytest.raises(Exception):
        ds.fork(parents[:1], clocks=[{A: 1}], history=[1])


def test_a_failed_fork_call_leaves_nothing_behind(engine, monkeypatch):
    """The call is all-or-nothing: with the read of what the patches need failing (the docset's test
    switch), the fork batch is undone, the new documents stay empty and unplaced, and the next fork
    call gives what it would have given."""
    ds, ctl = DocSet(engine), DocSet(engine)
    p = ds.open(1)
    ds.apply([p], [blocks(SHUFFLED)])
    monkeypatch.setenv("HM_DOCSET_INJECT_FAIL", "read")
    with pytest.raises(Exception, match="injected"):
        ds.fork([p, p], clocks=[{A: 3, B: 2}, {B: 1, A: 1}])
    monkeypatch.delenv("HM_DOCSET_INJECT_FAIL")
    for d in (p + 1, p + 2):
        inf = ds.info(d)
        assert (inf["n_changes"], inf["hist_len"], inf["n_actors"]) == (0, 0, 0)
    forks, fres, fjs = ds.fork([p], clocks=[{A: 3, B: 2}])
    c = ctl.open(1)
    cres, cjs = ctl.apply([c], [blocks(handed_over(SHUFFLED, {A: 3, B: 2}))])
    assert rows_equal(fres[0], cres[0]) and fjs == cjs and same_view(ds, forks[0], ctl, c)
    # the documents the failed call opened are usable
    r, _ = ds.apply([p + 1], [blocks(SHUFFLED)])
    assert int(r[0]["status"]) == 0 and int(r[0]["hist_len"]) == 6
