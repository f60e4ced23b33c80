"""hm_docset_materialize_patch_at (DocSet.materialize_patch(docs, clocks=...)): for a prefix's clock the
"patch" member is byte for byte the one materialize_patch gives at that history length; for causal-past
and cut clocks it is the patch oracle/js/backend.js returns for one applyChanges call on init() with
the selected changes in history order (tests/js/run_clock_patch.js), with the history and queued
counts of that call."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import decode_doc
from hypermerge_amd.docset import DocSet
from hypermerge_amd.engine import EngineError

from clock_diffs_ref import census, clocks_of
from fuzz_docs import gen_docs
from list_diffs_cases import LHAND
from op_diffs_cases import HAND, chain_doc, sources
from past_ref import select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.gpu

EMPTY = {"clock": {}, "deps": {}, "canUndo": False, "canRedo": False, "diffs": []}


def _blocks(changes):
    return [json.dumps(c, separators=(",", ":")).encode() for c in changes]


def _raw(ds, ids, clocks=None, history=None, lists=True):
    """the reply's text as it came (the patch members are compared as bytes)"""
    import ctypes
    from hypermerge_amd.docset import _text
    ids = np.ascontiguousarray(ids, np.uint32)
    t = ctypes.c_void_p()
    if clocks is not None:
        eoff, data, aoff, sq = ds._clock_entries(len(ids), clocks)
        st = ds._L.hm_docset_materialize_patch_at(ds._h, len(ids), ids.ctypes.data, eoff.ctypes.data, data.ctypes.data, aoff.ctypes.data,
                                                  sq.ctypes.data, 1 if lists else 0, ctypes.byref(t))
    else:
        hl = np.ascontiguousarray(history, np.uint32)
        st = ds._L.hm_docset_materialize_patch_ex(ds._h, len(ids), ids.ctypes.data, hl.ctypes.data, 1 if lists else 0, ctypes.byref(t))
    assert st == 0
    return _text(ds._L, t)[0]


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_patch_at_prefix_causal_past_and_cut_clocks(engine):
    b5 = synth.generate(synth.config("C5", n_docs=8, arrival=2, shuffle_pct=40, dup_pct=15))
    docs = [decode_doc(b5, i) for i in range(b5.n_docs)] + gen_docs("default", range(100, 110))
    docs += [HAND[k] for k in sorted(HAND)] + [LHAND[k][0] for k in sorted(LHAND)] + [chain_doc(40, 3)] + gen_docs("wide", range(200, 203))
    b, r, srcs = sources(docs, 64)                                            # (the CPU oracle: history order, all_deps)
    ds = DocSet(engine)
    first = ds.open(len(docs) + 1)
    ids = list(range(first, first + len(docs)))
    unplaced = first + len(docs)
    res, _ = ds.apply(ids, [_blocks(c) for c in docs])
    assert (res["status"] == 0).all()
    rng = np.random.default_rng(23)
    req, clocks, kinds, feed, rows = [], [], [], [], []
    for i, (src, ad) in enumerate(srcs):
        for kind, k in clocks_of(src, ad, 64, rng, n_past=3, n_cut=3):
            req.append(ids[i]); kinds.append(kind); rows.append((src, ad, 64, k))
            clocks.append({a: int(k[x]) for x, a in enumerate(b.doc_actors[i]) if k[x]})
            feed.append([docs[i][int(j)] for j in select(src, clock=k)])
    n, closed, queued = census(rows)
    assert closed >= 50 and queued >= 50, (n, closed, queued)                 # (clocks that are no prefix, of both kinds)
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_clock_patch.js")], input=json.dumps({"docs": feed}),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    want = json.loads(p.stdout.strip().splitlines()[-1])["docs"]
    got = ds.materialize_patch(req, clocks=clocks, lists=True)
    for x, g, w, kind in zip(req, got, want, kinds):
        assert w["err"] is None
        assert g["doc"] == x and (g["history"], g["queued"]) == (w["history"], w["queued"]), (x, kind)
        assert g["patch"] == w["patch"], (x, kind)
    # a prefix's clock: the patch member of the history-length call, byte for byte
    at = [j for j, kind in enumerate(kinds) if kind == "prefix"]
    assert all(got[j]["queued"] == 0 for j in at)
    by_clock = _raw(ds, [req[j] for j in at], clocks=[clocks[j] for j in at])
    by_len = _raw(ds, [req[j] for j in at], history=[got[j]["history"] for j in at])
    assert by_clock.count('"queued":0,') == len(at) and by_clock.replace('"queued":0,', "") == by_len   # (a quote inside a string is escaped)
    # without the option a selection that assigns list elements is handed to the host
    plain = ds.materialize_patch(req, clocks=clocks)
    elem = lambda w: any(x["type"] in ("list", "text") and x["action"] != "create" for x in w["patch"]["diffs"])
    for g, w, full in zip(plain, want, got):
        assert (g["patch"] is None and g.get("host") is True) if elem(w) else g == full
    assert any(g["patch"] is None for g in plain) and any(g["patch"] is not None for g in plain)
    # an unknown actor id is dropped; a document twice with two clocks; one not placed yet; no request
    j = next(j for j, kind in enumerate(kinds) if kind == "past" and got[j]["history"] > 1)
    j2 = next(k for k in range(len(req)) if req[k] == req[j] and got[k]["patch"] != got[j]["patch"])
    more = ds.materialize_patch([req[j], req[j2], req[j], unplaced], clocks=[dict(clocks[j], nobody=9), clocks[j2], clocks[j], {"a": 3}], lists=True)
    assert more[0] == got[j] == more[2] and more[1] == got[j2]
    assert more[3] == {"doc": unplaced, "history": 0, "queued": 0, "patch": EMPTY}
    assert ds.materialize_patch([], clocks=[]) == []
    with pytest.raises(EngineError):
        ds.materialize_patch([req[0], 9999], clocks=[{}, {}])
    with pytest.raises(ValueError):
        ds.materialize_patch([req[0]], [1], clocks=[{}])
    with pytest.raises(ValueError):
        ds.materialize_patch([req[0]])
