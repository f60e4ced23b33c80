"""tests/list_diffs_ref.py (the sequential restatement the list-diff tests compare the device with)
pinned three ways: on the JS restatement (oracle/js/backend.js emits the same diffs call by call,
over whole histories and over slices cut at call boundaries), on the C oracle (the visible elements
in pos order after every prefix are the merge's list_index order), and on cases written out by hand."""
import json
import os
import shutil
import subprocess
from collections import Counter
from functools import lru_cache

import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import decode_doc
import oracle.oracle as O

from list_diffs_cases import LHAND, busy_list, prepends, typed_list
from list_diffs_ref import ELEM_INSERT, ELEM_REMOVE, ELEM_SET, list_diffs, render, visible_after
from op_diffs_cases import HAND, chain_doc, sources
from op_diffs_ref import LISTS, op_diffs
from past_ref import gather, hist_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@lru_cache(maxsize=None)
def _generated():
    docs = []
    for cpa in (40, 60):
        b = synth.generate(synth.config("C3", n_docs=3, changes_per_actor=cpa), threads=2)
        docs += [decode_doc(b, i) for i in range(b.n_docs)]
    for kw in ({"arrival": 0, "shuffle_pct": 0}, {"arrival": 2, "shuffle_pct": 40}):
        b = synth.generate(synth.config("C5", n_docs=30, **kw), threads=2)
        docs += [decode_doc(b, i) for i in range(b.n_docs)]
    return tuple(docs)


def generated():
    return list(_generated())


def _js_calls(docs):
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_op_diffs.js")], input=json.dumps({"docs": docs}),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])["docs"]


def _against_js(docs):
    """every call's slice [at, h), a middle slice of several calls, and the whole history"""
    b, r, srcs = sources(docs)
    S = b.a_stride
    kinds = Counter()
    for d, (j, (src, ad)) in enumerate(zip(_js_calls(docs), srcs)):
        assert j["err"] is None, (d, j["err"])
        at, whole, cuts = 0, [], [0]
        for h, diffs in j["calls"]:
            if h != at:
                mine = list_diffs(src, ad, S, at, h)
                assert mine.flags == 0 and mine.bad == 0
                assert render(b, d, src, mine) == diffs, (d, at, h)
                cuts.append(h)
            else:
                assert diffs == [], d
            whole += [(h, x) for x in diffs]
            at = h
        full = list_diffs(src, ad, S, 0, at + 9)
        assert full.flags == 0 and render(b, d, src, full) == [x for _, x in whole], d
        lo, hi = cuts[len(cuts) // 3], cuts[(2 * len(cuts)) // 3]
        assert render(b, d, src, list_diffs(src, ad, S, lo, hi)) == [x for h, x in whole if lo < h <= hi], (d, lo, hi)
        for _, x in whole:
            if x["type"] in ("list", "text") and x["action"] != "create":
                kinds[x["action"]] += 1
    return kinds


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_restatement_emits_the_same_element_diffs_on_generated_documents():
    kinds = _against_js(generated() + [HAND["text"]])
    assert kinds["insert"] >= 1 and kinds["set"] >= 1 and kinds["remove"] >= 1, kinds


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_restatement_emits_the_same_element_diffs_on_the_hand_and_boundary_documents():
    docs = [LHAND[k][0] for k in sorted(LHAND)] + [typed_list(65), prepends(70), busy_list(130)]
    kinds = _against_js(docs)
    assert kinds["insert"] >= 1 and kinds["set"] >= 1 and kinds["remove"] >= 1, kinds


def test_hand_written_cases():
    names = sorted(LHAND)
    b, r, srcs = sources([LHAND[k][0] for k in names])
    for name, (src, ad) in zip(names, srcs):
        got = list_diffs(src, ad, b.a_stride, 0, 99)
        assert got.flags == 0 and got.bad == 0
        assert [(k, kind, ix, [x[0] for x in sv]) for k, kind, ix, sv in got.rows] == LHAND[name][1], name
    # the counter element after the inc: 10 + 5, still an INT
    src, ad = srcs[names.index("counter_inc_then_invisible")]
    assert list_diffs(src, ad, b.a_stride, 0, 99).rows[3][3] == [(3, 3, 15)]
    # a slice from the middle: the visibility built before it counts
    src, ad = srcs[names.index("tombstone_before")]
    assert [(k, kind, ix) for k, kind, ix, _ in list_diffs(src, ad, b.a_stride, 2, 3).rows] == [(9, ELEM_SET, 1)]


def test_without_the_hint_and_on_map_documents_it_is_op_diffs_ref():
    docs = [HAND[k] for k in sorted(HAND)] + [chain_doc(30, 3)]
    b, r, srcs = sources(docs)
    for d, (src, ad) in enumerate(srcs):
        H = hist_len(src)
        for f, t in [(0, H), (1, H), (0, 2), (H // 2, H + 3)]:
            want = op_diffs(src, ad, b.a_stride, f, t)
            got = list_diffs(src, ad, b.a_stride, f, t, hint=False)
            assert got.flags == want.flags and [(k, kind, sv) for k, kind, _, sv in got.rows] == want.rows
            if not want.flags & LISTS:                           # (a range without element assigns: the same rows)
                got = list_diffs(src, ad, b.a_stride, f, t)
                assert [(k, kind, sv) for k, kind, _, sv in got.rows] == want.rows and all(ix is None for _, _, ix, _ in got.rows)


def test_visible_elements_in_pos_order_are_the_oracles_list_of_every_prefix():
    docs = generated() + [LHAND[k][0] for k in sorted(LHAND)] + [prepends(9), busy_list(40)]
    b, r, srcs = sources(docs)
    S = b.a_stride
    seen = 0
    for d, (src, ad) in enumerate(srcs):
        for n in range(hist_len(src) + 1):
            g, clog, olog = gather([(src, n, None)], S)
            o = O.merge(g)
            assert int(o.docs["status"][0]) == 0
            want = {}
            for reg in range(src.n_regs):
                row = o.regs[reg]
                if int(row["list_index"]) >= 0:
                    want.setdefault(int(row["obj"]), []).append((int(row["list_index"]), reg))
            want = {obj: [reg for _, reg in sorted(v)] for obj, v in want.items()}
            assert visible_after(src, ad, S, n) == want, (d, n)
            seen += sum(len(v) for v in want.values())
    assert seen > 1000
