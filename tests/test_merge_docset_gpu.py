"""hm_docset_merge_from against a control: a second docset with the same flags whose documents hold the
destinations' logs and then receive, in one apply round, the JSON blocks of the changes the merge hands
over, in hand-over order (tests/test_merge_ref.py's restatement says which).  Equal as parsed JSON: the
result rows, the patches with DocBackend.clock and the call's clock, under every flavour; the views as
objects (a merged document interns everything its source names, so its register order is its own: under net
diffs, where a patch can list every register in that order, the sources meet their changes in hand-over
order, see handed_first); then a later apply
round and materialize_patch on both.  The stride classes are 8, 16, ...: the destination that crosses
its class is the one whose ninth actor arrives with the merge."""
import json

import pytest

from hypermerge_amd.docset import DocSet, view_objects
from hypermerge_amd.engine import EngineError

from fuzz_docs import gen_docs
from kat_cases import A, B, Cc, ch, s
from merge_cases import HAND_BY_NAME, SHUFFLED, TEXT, Z, case, fuzz_pair
from test_merge_ref import Pair

pytestmark = pytest.mark.gpu

FLAVOURS = {"default": {}, "device_diffs": {"device_diffs": True}, "net_diffs": {"net_diffs": True}, "no_patches": {"patches": False}}
LOG_INFO = ("n_changes", "n_ops", "hist_len", "n_queued")
ROW = ("status", "hist_len", "n_queued", "n_surv", "min_cmp", "err_change", "err_op")
NINE = ["w%d" % i for i in range(9)]


def blocks(changes):
    return [json.dumps(c, separators=(",", ":")).encode() for c in changes]


def same_class_cases():
    """Destinations and sources that stay in the 8-actor class (the destination of `five` has 4 actors and gains a fifth)."""
    five = case("five", SHUFFLED, [ch(a, 1, {}, s("k" + a, 1)) for a in ("d1", "d2", "d3", "d4")] + [SHUFFLED[2]], {A: 3, B: 2})
    fuzz = [fuzz_pair(chs, seed) for chs, seed in zip(gen_docs("default", range(9300, 9306)), range(9300, 9306))]
    return [HAND_BY_NAME[k] for k in ("repo_merge", "shuffled", "text", "counter", "links", "unblocks", "empty", "not_closed")] + [five] + fuzz


def cross_class_cases():
    eight = [ch("v%d" % i, 1, {}, s("k%d" % i, i)) for i in range(8)]
    nine = [ch(a, 1, {}, s("n" + a, i)) for i, a in enumerate(NINE)] + [ch(NINE[0], 2, {NINE[8]: 1}, s("late", 1))]
    return [
        # the destination holds 8 actors and gains a ninth: it moves to the 16-actor class
        case("crosses", [ch("aa", 1, {}, s("x", 1)), ch("aa", 2, {}, s("y", 2))], eight, {"aa": 2}),
        # a 9-actor source into a small destination, which moves to the source's class
        case("wide_source", nine, [ch(Z, 1, {}, s("own", 1))], {a: 2 for a in NINE}),
    ]


def run(ds, ctl, cases, dst, src, cdst):
    """One merge_from call on ds, the handed changes in one apply round on ctl; compares everything."""
    pairs = [Pair(c, 16) for c in cases]
    handed = [p.handed() for p in pairs]
    res, js = ds.merge_from(dst, src, [c["clock"] for c in cases])
    cres, cjs = ctl.apply(cdst, [blocks(h) for h in handed])
    for i, c in enumerate(cases):
        assert all(int(res[i][f]) == int(cres[i][f]) for f in ROW), (c["name"], res[i], cres[i])
        for part in ("p", "b", "c"):
            assert js[part][i] == cjs[part][i], (c["name"], part)
        assert view_objects(ds.view(dst[i])) == view_objects(ctl.view(cdst[i])), c["name"]
        fi, ci = ds.info(dst[i]), ctl.info(cdst[i])
        assert [fi[f] for f in LOG_INFO] == [ci[f] for f in LOG_INFO], c["name"]
    return handed, res


def later_round(ds, ctl, cases, dst, cdst, flavour):
    """A further change of a new actor on every merged destination and its control; then the whole patch."""
    extra = [[ch("later", 1, {}, s("after", i))] for i in range(len(dst))]
    r2, j2 = ds.apply(dst, [blocks(x) for x in extra])
    c2, k2 = ctl.apply(cdst, [blocks(x) for x in extra])
    for i, c in enumerate(cases):
        assert all(int(r2[i][f]) == int(c2[i][f]) for f in ROW), c["name"]
        for part in ("p", "b", "c"):
            assert j2[part][i] == k2[part][i], (c["name"], part)
        assert view_objects(ds.view(dst[i])) == view_objects(ctl.view(cdst[i])), c["name"]
    if flavour in ("default", "device_diffs"):                   # (materialize_patch renders per-op diffs: those docsets alone)
        big = [1 << 20] * len(dst)
        got, want = ds.materialize_patch(dst, history=big, lists=True), ctl.materialize_patch(cdst, history=big, lists=True)
        for i, c in enumerate(cases):
            assert (got[i]["history"], got[i]["patch"]) == (want[i]["history"], want[i]["patch"]), c["name"]


def handed_first(c):
    """The source's changes with the ones the merge hands over first, in hand-over order.  A net-diffs round
    that finds or leaves queued changes is rendered from every register in register order, and a merged
    document's new registers are numbered in its source's order: a source that met its changes in this
    order numbers them as the control does, which meets them in the apply round, so the patches compare
    exactly.  (What the source holds and what is handed over do not depend on its arrival order.)"""
    handed = Pair(c, 16).handed()
    took = {id(x) for x in handed}
    return dict(c, src=handed + [x for x in c["src"] if id(x) not in took])


def load(ds, ctl, cases):
    n = len(cases)
    d0, c0 = ds.open(2 * n), ctl.open(n)
    src, dst, cdst = list(range(d0, d0 + n)), list(range(d0 + n, d0 + 2 * n)), list(range(c0, c0 + n))
    res, _ = ds.apply(src + dst, [blocks(c["src"]) for c in cases] + [blocks(c["dst"]) for c in cases])
    assert (res["status"] == 0).all()
    cres, _ = ctl.apply(cdst, [blocks(c["dst"]) for c in cases])
    assert (cres["status"] == 0).all()
    return src, dst, cdst


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_same_class_and_cross_class_requests_in_one_call(engine, flavour):
    kw = FLAVOURS[flavour]
    ds, ctl = DocSet(engine, **kw), DocSet(engine, **kw)
    same, cross = same_class_cases(), cross_class_cases()
    cases = same + cross
    if flavour == "net_diffs":
        cases = [handed_first(c) for c in cases]
    src, dst, cdst = load(ds, ctl, cases)
    views = [ds.view(p) for p in src]
    assert [ds.info(d)["a_stride"] for d in dst[len(same):]] == [8, 8]
    handed, res = run(ds, ctl, cases, dst, src, cdst)
    assert ds.merge_stats() == {"device": len(same), "host": len(cross)}
    assert [ds.info(d)["a_stride"] for d in dst] == [8] * len(same) + [16, 16]
    assert sum(len(h) > 0 for h in handed) >= len(cases) - 2 and (res["status"] == 0).all()
    i = [c["name"] for c in cases].index("unblocks")
    assert ctl.info(cdst[i])["n_queued"] == 0 and int(res[i]["n_queued"]) == 0
    i = [c["name"] for c in cases].index("five")
    assert ds.info(dst[i])["n_actors"] == 7                       # d1 .. d4 and aaaa, then bbbb and (interned) cccc
    for p, v in zip(src, views):
        assert ds.view(p) == v                                     # the sources are only read
    later_round(ds, ctl, cases, dst, cdst, flavour)
    # once more: everything was handed over, so nothing is selected and nothing changes
    before = [ds.view(d) for d in dst]
    res2, js2 = ds.merge_from(dst[:3], src[:3], [c["clock"] for c in cases[:3]])
    assert (res2["status"] == 0).all() and [ds.view(d) for d in dst] == before
    if flavour != "no_patches":
        assert all(p["diffs"] == [] for p in js2["p"])


@pytest.mark.parametrize("flavour", ["default", "device_diffs"])
def test_host_routes(engine, flavour):
    """A destination not placed yet, a source not placed yet (nothing to hand), a destination in a wider
    class than its source — and a same-class request beside them, which takes the host route too: its
    class takes a host-route round in this call."""
    kw = FLAVOURS[flavour]
    ds, ctl = DocSet(engine, **kw), DocSet(engine, **kw)
    nine = [ch(a, 1, {}, s("n" + a, i)) for i, a in enumerate(NINE)]
    cases = [case("unplaced_destination", TEXT, [], {A: 4, B: 2}),
             case("unplaced_source", [], [ch(Z, 1, {}, s("own", 1))], {A: 4}),
             case("wider_destination", SHUFFLED, nine, {B: 2, A: 3, Cc: 1}),
             HAND_BY_NAME["shuffled"]]
    n = len(cases)
    d0, c0 = ds.open(2 * n), ctl.open(n)
    src, dst, cdst = list(range(d0, d0 + n)), list(range(d0 + n, d0 + 2 * n)), list(range(c0, c0 + n))
    fed = [(h, c[k]) for c, p, d in zip(cases, src, dst) for h, k in ((p, "src"), (d, "dst")) if c[k]]
    res, _ = ds.apply([h for h, _ in fed], [blocks(x) for _, x in fed])
    assert (res["status"] == 0).all()
    fed = [(h, c["dst"]) for c, h in zip(cases, cdst) if c["dst"]]
    ctl.apply([h for h, _ in fed], [blocks(x) for _, x in fed])
    handed, res = run(ds, ctl, cases, dst, src, cdst)
    assert ds.merge_stats() == {"device": 0, "host": n}
    assert [len(h) for h in handed] == [6, 0, 6, 6]
    assert [ds.info(d)["a_stride"] for d in dst] == [8, 8, 16, 8]
    later_round(ds, ctl, cases, dst, cdst, flavour)
    # alone, the same-class request moves its rows on the device
    e0 = ds.open(1)
    ds.apply([e0], [blocks([ch(Z, 1, {}, s("own", 1))])])
    ds.merge_from([e0], [src[3]], [{A: 3}])
    assert ds.merge_stats() == {"device": 1, "host": n}


def test_refusals_and_a_failed_call(engine, monkeypatch):
    ds, ctl = DocSet(engine), DocSet(engine)
    cases = [HAND_BY_NAME["shuffled"], HAND_BY_NAME["text"]]
    src, dst, cdst = load(ds, ctl, cases)
    before = [ds.view(d) for d in dst + src], [ds.info(d) for d in dst + src]
    clocks = [c["clock"] for c in cases]
    with pytest.raises(EngineError, match="bad or repeated docset document"):
        ds.merge_from([dst[0], dst[0]], src, clocks)                 # a destination named twice
    with pytest.raises(EngineError, match="a destination of the same call"):
        ds.merge_from([dst[0], src[0]], src, clocks)                 # a destination that is a source
    with pytest.raises(EngineError, match="bad or repeated docset document"):
        ds.merge_from([dst[0], 99999], src, clocks)
    with pytest.raises(EngineError, match="bad docset document"):
        ds.merge_from(dst, [src[0], 99999], clocks)
    monkeypatch.setenv("HM_DOCSET_INJECT_FAIL", "read")
    with pytest.raises(EngineError, match="injected"):
        ds.merge_from(dst, src, clocks)
    monkeypatch.delenv("HM_DOCSET_INJECT_FAIL")
    assert ([ds.view(d) for d in dst + src], [ds.info(d) for d in dst + src]) == before
    assert ds.merge_stats() == {"device": 0, "host": 0}
    run(ds, ctl, cases, dst, src, cdst)
    assert ds.merge_stats() == {"device": 2, "host": 0}


def test_a_failed_mixed_call_is_undone_on_every_route(engine, monkeypatch):
    """A same-class request beside a destination not placed yet (so both take the host route, in one class)
    and a class-crossing one: with the read of what the patches need failing, nothing is left behind, and
    the same call then gives what it would have given."""
    ds, ctl = DocSet(engine), DocSet(engine)
    cases = [HAND_BY_NAME["shuffled"], case("unplaced_destination", TEXT, [], {A: 4, B: 2})] + cross_class_cases()[:1]
    n = len(cases)
    d0, c0 = ds.open(2 * n), ctl.open(n)
    src, dst, cdst = list(range(d0, d0 + n)), list(range(d0 + n, d0 + 2 * n)), list(range(c0, c0 + n))
    fed = [(h, c[k]) for c, p, d in zip(cases, src, dst) for h, k in ((p, "src"), (d, "dst")) if c[k]]
    ds.apply([h for h, _ in fed], [blocks(x) for _, x in fed])
    fed = [(h, c["dst"]) for c, h in zip(cases, cdst) if c["dst"]]
    ctl.apply([h for h, _ in fed], [blocks(x) for _, x in fed])
    before = [ds.view(d) for d in dst + src], [ds.info(d) for d in dst + src]
    monkeypatch.setenv("HM_DOCSET_INJECT_FAIL", "read")
    with pytest.raises(EngineError, match="injected"):
        ds.merge_from(dst, src, [c["clock"] for c in cases])
    monkeypatch.delenv("HM_DOCSET_INJECT_FAIL")
    assert ([ds.view(d) for d in dst + src], [ds.info(d) for d in dst + src]) == before
    assert ds.merge_stats() == {"device": 0, "host": 0}
    run(ds, ctl, cases, dst, src, cdst)
    assert ds.merge_stats() == {"device": 0, "host": n}


def test_a_docset_outlives_its_engine():
    """A docset that is closed (or collected) after its engine was closed does not touch the engine's
    stream: a failing test keeps its docsets alive past the session engine's teardown."""
    from hypermerge_amd.engine import Engine
    e = Engine(0)
    ds = DocSet(e)
    d = ds.open(1)
    ds.apply([d], [blocks(SHUFFLED)])
    e.close()
    ds.close()
    assert ds._h is None
