"""hm_docset_materialize_patch_ex with HM_ODF_LISTS: the patch of text and list documents at every
history length carries the element diffs (insert / set / remove at the index of that moment) from
the device: equal to the JS restatement's diffs at every call boundary of a one-change-per-call feed
(oracle/js/backend.js through tests/js/run_op_diffs.js) and to tests/list_diffs_ref.py's rendering at
every length in between, and never null.  Without the option the same docset answers as before."""
import json
import os
import shutil
import subprocess

import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import decode_doc
from hypermerge_amd.docset import DocSet

from list_diffs_cases import LHAND
from list_diffs_ref import list_diffs, render
from op_diffs_cases import HAND, sources
from past_ref import hist_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.gpu


def _blocks(changes):
    return [json.dumps(c, separators=(",", ":")).encode() for c in changes]


def _docs():
    b5 = synth.generate(synth.config("C5", n_docs=10, arrival=2, shuffle_pct=40))
    b3 = synth.generate(synth.config("C3", n_docs=2, changes_per_actor=40))
    return ([HAND["text"]] + [decode_doc(b5, i) for i in range(b5.n_docs)] + [decode_doc(b3, i) for i in range(b3.n_docs)] +
            [LHAND[k][0] for k in sorted(LHAND)])


def test_patches_of_list_documents_at_every_history_length(engine):
    docs = _docs()
    b, r, srcs = sources(docs)
    ds = DocSet(engine)
    first = ds.open(len(docs))
    ids = list(range(first, first + len(docs)))
    res, _ = ds.apply(ids, [_blocks(c) for c in docs])
    assert (res["status"] == 0).all()
    req = [(x, n) for x, (src, _) in zip(ids, srcs) for n in range(hist_len(src) + 2)]
    got = ds.materialize_patch([x for x, _ in req], [n for _, n in req], lists=True)
    elements = 0
    for (x, n), g in zip(req, got):
        src, ad = srcs[x - first]
        assert g["patch"] is not None and "host" not in g, (x, n)
        assert g["history"] == min(n, hist_len(src))
        want = render(b, x - first, src, list_diffs(src, ad, b.a_stride, 0, n))
        assert g["patch"]["diffs"] == want, (x, n)
        elements += sum(1 for w in want if "index" in w)
    assert elements > 1000
    assert "null" not in json.dumps(got)
    # without the option: as before, null from the first element assign on
    old = ds.materialize_patch([ids[0]] * 3, [2, 3, 4])
    assert old[0]["patch"] is not None and old[1] == {"doc": ids[0], "history": 3, "patch": None, "host": True} and old[2]["patch"] is None


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_patches_at_call_boundaries_equal_the_js_restatement(engine):
    docs = _docs()
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_op_diffs.js")], input=json.dumps({"docs": docs}),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    js = json.loads(p.stdout.strip().splitlines()[-1])["docs"]
    ds = DocSet(engine)
    first = ds.open(len(docs))
    ids = list(range(first, first + len(docs)))
    res, _ = ds.apply(ids, [_blocks(c) for c in docs])
    assert (res["status"] == 0).all()
    req, want = [], []
    for x, j in zip(ids, js):
        assert j["err"] is None
        so_far = []
        for h, diffs in j["calls"]:
            so_far = so_far + diffs
            req.append((x, h)); want.append(so_far)
    got = ds.materialize_patch([x for x, _ in req], [h for _, h in req], lists=True)
    assert len(got) > 300
    for (x, h), g, w in zip(req, got, want):
        assert g["history"] == h and g["patch"] is not None and g["patch"]["diffs"] == w, (x, h)
