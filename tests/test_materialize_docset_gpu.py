"""hm_docset_materialize: documents by id at a history length or at a clock given by actor id, in two
stride classes and after a move to a wider class.  The view at the whole history is hm_docset_view's;
views at earlier points equal the rendering of the CPU oracle's merge of that prefix of the history."""
import json

import pytest

from hypermerge_amd.columnar import encode
from hypermerge_amd.docset import DocSet, render_objects, view_objects
from hypermerge_amd.engine import EngineError
from hypermerge_amd.render import doc_summary
import oracle.oracle as O

from kat_cases import ch, d, inc, ins, link, mk, s

pytestmark = pytest.mark.gpu

A, B, Cc = "aaaa", "bbbb", "cccc"


def _blocks(changes):
    return [json.dumps(c, separators=(",", ":")).encode() for c in changes]


def _history(log):
    """the log's changes in history order (the oracle's hist)"""
    b = encode([log])
    o = O.merge(b)
    assert int(o.docs["status"][0]) == 0
    return [log[i] for _, i in sorted((int(h), i) for i, h in enumerate(o.hist) if h >= 0)]


def _summary(changes):
    b = encode([changes])
    return doc_summary(b, O.merge(b), 0)


def _state(entry):
    return render_objects(view_objects(entry["view"]))


def _same(entry, changes):
    want = _summary(changes)
    assert _state(entry) == json.loads(json.dumps(want["state"]))
    assert entry["history"] == len(want["history"])
    assert entry["deps"] == want["deps"] and entry["clock"] == want["clock"]


def test_docset_materialize(engine):
    ds = DocSet(engine)
    first = ds.open(4)
    small, wide, mover, unplaced = range(first, first + 4)
    writers = [f"w{i:02d}" for i in range(11)]
    logs = {
        # lists, a counter, a nested map; delivered out of order (bbbb:1 waits for aaaa:2)
        small: [ch(B, 1, {A: 2}, ins("L", f"{A}:1", 1), s(f"{B}:1", "b", obj="L"), inc("n", 4)),
                ch(A, 1, {}, mk("makeList", "L"), link("l", "L"), s("n", 1, datatype="counter")),
                ch(A, 2, {}, ins("L", "_head", 1), s(f"{A}:1", "a", obj="L")),
                ch(A, 3, {B: 1}, d(f"{A}:1", obj="L"), mk("makeMap", "M"), link("m", "M"), s("k", "v", obj="M")),
                ch(Cc, 1, {A: 1}, s("n", 7, datatype="counter"), s("x", "c"))],
        wide: [ch(w, 1, {}, s("k", i)) for i, w in enumerate(writers)]
              + [ch("zzzz", 1, {w: 1 for w in writers[:6]}, s("k", "six")), ch(writers[8], 2, {"zzzz": 1}, s("k", 99))],
        mover: [ch(B, 2, {}, s("y", 2)), ch(B, 1, {}, s("y", 1)), ch(A, 1, {B: 2}, s("x", 1))],
    }
    ids = [small, wide, mover]
    res, _ = ds.apply(ids, [_blocks(logs[x]) for x in ids])
    assert (res["status"] == 0).all()
    assert ds.info(small)["a_stride"] == 8 and ds.info(wide)["a_stride"] == 16
    hist = {x: _history(logs[x]) for x in ids}
    assert [(c["actor"], c["seq"]) for c in hist[small]] == [(A, 1), (A, 2), (B, 1), (A, 3), (Cc, 1)]

    # every history length of every document in one call (both classes, documents repeated), one past the end too
    req = [(x, n) for x in ids for n in range(len(hist[x]) + 2)] + [(unplaced, 3)]
    got = ds.materialize([x for x, _ in req], history=[n for _, n in req])
    assert [g["doc"] for g in got] == [x for x, _ in req]
    for (x, n), g in zip(req[:-1], got):
        _same(g, hist[x][:n])
        if n >= len(hist[x]):
            assert g["view"] == ds.view(x)                      # the whole history: the resident document
    assert got[-1] == {"doc": unplaced, "clock": {}, "deps": {}, "history": 0, "view": ds.view(unplaced)}
    # the list element before it has a value, the counter between its set and the inc, the object not made yet
    assert _state(got[1]) == {"map": [["l", {"value": {"list": []}}], ["n", {"value": 1, "datatype": "counter"}]]}
    assert _state(got[3])["map"][1] == ["n", {"value": 5, "datatype": "counter"}]
    assert "M" not in got[3]["view"] and "M" in got[4]["view"]
    assert got[3]["clock"] == {A: 2, B: 1}

    # clocks by actor id, in an order that is not the rank order; an id the document has never seen
    clocks = [{B: 1, A: 2}, {A: 1}, {"nobody": 3, Cc: 1, A: 1}, {}, {A: 3, B: 1, Cc: 1}]
    got = ds.materialize([small] * len(clocks), clocks=clocks)
    pick = lambda log, c: [x for x in log if x["seq"] <= c.get(x["actor"], 0)]
    for c, g in zip(clocks, got):
        _same(g, pick(hist[small], c))
    assert got[4]["view"] == ds.view(small) and got[3]["history"] == 0
    # a clock that is not causally closed: bbbb:1 without aaaa:2 stays queued, as applyChanges leaves it
    (g,) = ds.materialize([small], clocks=[{B: 1, A: 1}])
    assert g["history"] == 1 and g["clock"] == {A: 1}
    got = ds.materialize([wide, wide], clocks=[{"zzzz": 1, **{w: 1 for w in writers[:6]}}, {writers[9]: 1, "w08": 2}])
    _same(got[0], pick(hist[wide], {"zzzz": 1, **{w: 1 for w in writers[:6]}}))
    assert got[1]["history"] == 2 and got[1]["clock"] == {"w08": 1, "w09": 1}      # w08:2 needs zzzz:1: it stays queued

    # the mover outgrows its class and keeps answering, by id and by actor id
    r2 = [ch(w, 1, {B: 1}, s("m", i)) for i, w in enumerate(writers[:8])] + [ch(A, 2, {writers[7]: 1}, s("x", 2))]
    res, _ = ds.apply([mover], [_blocks(r2)])
    assert (res["status"] == 0).all() and ds.info(mover)["a_stride"] == 16
    h2 = _history(logs[mover] + r2)
    ns = [0, 2, 3, 7, len(h2)]
    got = ds.materialize([mover] * len(ns) + [small], history=ns + [2])
    for n, g in zip(ns, got):
        _same(g, h2[:n])
    assert got[len(ns) - 1]["view"] == ds.view(mover)
    _same(got[-1], hist[small][:2])
    (g,) = ds.materialize([mover], clocks=[{B: 2, A: 1}])
    _same(g, h2[:3])
    assert ds.materialize([], history=[]) == []
    with pytest.raises(EngineError):
        ds.materialize([mover, 9999], history=[1, 1])
    with pytest.raises(EngineError, match="exactly one"):
        ds.materialize([mover])
