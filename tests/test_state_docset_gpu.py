"""hm_docset_views / hm_docset_get_patch: the documents of three stride classes, one not placed yet and
one moved to a wider class by a late writer, in one call.  views(docs)[i] is hm_docset_view(docs[i])
byte for byte; get_patch's diffs rebuild the view from an empty document, its clock / deps are those
of the document's last apply round, and the call is the same text whatever the docset's patch flags."""
import ctypes
import json

import numpy as np
import pytest

from hypermerge_amd.docset import ROOT, DocSet, _text, apply_diffs, view_objects
from hypermerge_amd.engine import EngineError

from fuzz_docs import gen_doc
from kat_cases import A, B, ch, s
from state_cases import KNOWN

pytestmark = pytest.mark.gpu


def _blocks(changes):
    return [json.dumps(c, separators=(",", ":")).encode() for c in changes]


def view_bytes(ds, doc):
    t = ctypes.c_void_p()
    ds.engine._check(ds._L.hm_docset_view(ds._h, doc, ctypes.byref(t)), "hm_docset_view")
    return _text(ds._L, t, raw=True)[0]


def logs(detached=True):
    """per document its rounds of changes: 3, 9 and 20 writers (strides 8, 16, 32), the known answers,
    and a document whose second round brings the writers that move it from stride 8 to 16.
    detached=False leaves out the known answer that deletes a detached list element: a docset created
    with HM_DOCSET_DEVICE_DIFFS refuses that round in hm_docset_apply (the element-diff kernels take an
    assign on an element no applied ins made for tables that are not a merge's), before any state call."""
    rng = np.random.default_rng(31)
    docs = [gen_doc(400 + i, n_actors=3, profile="default") for i in range(8)]
    docs += [gen_doc(seed, n_actors=9, profile="wide") for seed in (421, 422, 423)]
    docs += [gen_doc(seed, n_actors=20, n_changes=60, profile="wide") for seed in (440, 442)]
    assert [len({c["actor"] for c in chs}) for chs in docs[8:]] == [9, 9, 9, 20, 20]       # (every writer writes)
    docs += [KNOWN[k][0] for k in sorted(KNOWN) if KNOWN[k][0] and (detached or k != "detached_element")]
    out = []
    for chs in docs:
        cut = int(rng.integers(1, len(chs) + 1))
        out.append([chs[:cut], chs[cut:]])
    writers = [f"w{i:02d}" for i in range(9)]
    out.append([[ch(A, 1, {}, s("x", 1)), ch(B, 1, {}, s("x", 2))], [ch(w, 1, {A: 1}, s("x", i), s(w, i)) for i, w in enumerate(writers)]])
    return out


def fed(ds, rounds):
    """(ids, the last round's patch per document); one id more is opened and never written"""
    first = ds.open(len(rounds) + 1)
    ids = list(range(first, first + len(rounds)))
    last = {}
    for rd in range(2):
        sel = [i for i in range(len(rounds)) if rounds[i][rd]]
        res, js = ds.apply([ids[i] for i in sel], [_blocks(rounds[i][rd]) for i in sel])
        assert (res["status"] == 0).all()
        for k, i in enumerate(sel):
            last[ids[i]] = js["p"][k]
    return ids, last, first + len(rounds)


def test_views_and_get_patch(engine):
    rounds = logs()
    ds = DocSet(engine)
    ids, last, unplaced = fed(ds, rounds)
    strides = [ds.info(x)["a_stride"] for x in ids]
    assert {8, 16, 32} <= set(strides) and strides[-1] == 16 and ds.info(unplaced)["a_stride"] == 0
    req = ids + [unplaced] + ids[::-3] + [unplaced, ids[0], ids[0]]                     # (every class, documents repeated)
    # byte for byte what hm_docset_view returns, one document at a time
    raw = ds.views(req, raw=True)
    assert raw == b"[" + b",".join(view_bytes(ds, x) for x in req) + b"]"
    views = ds.views(req)
    assert views == [ds.view(x) for x in req] and views[len(ids)] == ds.view(unplaced)
    assert sum(len(o["elems"]) for v in views for o in v.values()) > 100 and any(len(v) > 3 for v in views)
    # the patches: the diffs rebuild the view, clock / deps are the last round's
    got = ds.get_patch(req)
    assert [g["doc"] for g in got] == req
    kinds = set()
    for x, g, v in zip(req, got, views):
        p = g["patch"]
        assert list(p) == ["clock", "deps", "canUndo", "canRedo", "diffs"] and p["canUndo"] is False and p["canRedo"] is False
        objects = {ROOT: {"type": "map", "keys": {}, "elems": []}}
        apply_diffs(objects, p["diffs"])
        assert objects == view_objects(v), x
        if x == unplaced:
            assert g == {"doc": x, "history": 0, "patch": {"clock": {}, "deps": {}, "canUndo": False, "canRedo": False, "diffs": []}}
            continue
        assert p["clock"] == last[x]["clock"] and p["deps"] == last[x]["deps"], x
        assert g["history"] == ds.info(x)["hist_len"]
        # creates first (view order, never ROOT), then per object its sets, then its inserts with index and elemId
        acts = [d["action"] for d in p["diffs"]]
        nc = acts.count("create")
        assert acts[:nc] == ["create"] * nc and [d["obj"] for d in p["diffs"][:nc]] == [u for u in v if u != ROOT]
        rest = p["diffs"][nc:]
        want = []
        for u, o in v.items():
            want += [("set", u, k) for k, _ in o["keys"]] + [("insert", u, i, e) for i, (e, _) in enumerate(o["elems"])]
        assert [(d["action"], d["obj"], d["key"]) if d["action"] == "set" else (d["action"], d["obj"], d["index"], d["elemId"]) for d in rest] == want
        kinds |= {(d["action"], d["type"]) for d in rest} | {k for d in rest for k in d if k in ("conflicts", "link", "datatype")}
    assert {("set", "map"), ("set", "table"), ("insert", "list"), ("insert", "text"), "conflicts", "link", "datatype"} <= kinds
    assert ds.views([]) == [] and ds.get_patch([]) == []
    with pytest.raises(EngineError, match="bad docset document"):
        ds.views([ids[0], 99999])
    with pytest.raises(EngineError, match="bad docset document"):
        ds.get_patch([99999])


def test_get_patch_is_the_same_whatever_the_patch_flags(engine):
    rounds = logs(detached=False)
    texts = []
    for kw in ({}, {"net_diffs": True}, {"device_diffs": True}):
        ds = DocSet(engine, **kw)
        ids, _, unplaced = fed(ds, rounds)
        req = np.ascontiguousarray(ids + [unplaced], np.uint32)
        t = ctypes.c_void_p()
        engine._check(ds._L.hm_docset_get_patch(ds._h, len(req), req.ctypes.data, ctypes.byref(t)), "hm_docset_get_patch")
        texts.append(_text(ds._L, t, raw=True)[0])
        assert ds.views(req, raw=True) == b"[" + b",".join(view_bytes(ds, int(x)) for x in req) + b"]"
        ds.close()
    assert texts[0] == texts[1] == texts[2] and len(texts[0]) > 10000
