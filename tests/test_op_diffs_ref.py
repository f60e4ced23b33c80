"""tests/op_diffs_ref.py (the sequential restatement the op-diff tests compare the device with)
pinned three ways: on the C oracle (the last row per register over every prefix is the merge of
that prefix), on the JS restatement (oracle/js/backend.js emits the same diffs call by call), and on
one case written out by hand."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import V_INT, decode_doc
import oracle.oracle as O

from kat_cases import CASES
from op_diffs_cases import HAND, TIE_FLIP, TIE_FLIP_ORDERS, chain_doc, one_register_doc, sources
from op_diffs_ref import CREATE, LISTS, REMOVE, SET_ROW, op_diffs, registers_after, render
from past_ref import gather, hist_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


def seeded_docs():
    b = synth.generate(synth.config("C2", n_docs=6, arrival=2, shuffle_pct=40, dup_pct=15))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    b = synth.generate(synth.config("C4", n_docs=4))
    docs += [decode_doc(b, i) for i in range(b.n_docs)]
    return docs + [HAND["counter_int_float"], HAND["tie_flip"], HAND["make_link"], one_register_doc(40), chain_doc(30, 3)]


def test_last_row_per_register_is_the_oracles_merge_of_every_prefix():
    b, r, srcs = sources(seeded_docs())
    S = b.a_stride
    for d, (src, ad) in enumerate(srcs):
        for n in range(hist_len(src) + 1):
            g, clog, olog = gather([(src, n, None)], S)
            o = O.merge(g)
            assert int(o.docs["status"][0]) == 0
            mine = registers_after(src, ad, S, n)
            for reg in range(src.n_regs):
                row = o.regs[reg]
                want = [(int(olog[int(x["op"])]), int(x["vtag"]), int(x["value"]))
                        for x in o.surv[int(row["surv_off"]):int(row["surv_off"]) + int(row["n_surv"])]]
                assert mine.get(reg, []) == want, (d, n, reg)


def _js_calls(docs):
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_op_diffs.js")], input=json.dumps({"docs": docs}),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])["docs"]


def _against_js(docs, want_lists=()):
    b, r, srcs = sources(docs)
    S = b.a_stride
    for d, (j, (src, ad)) in enumerate(zip(_js_calls(docs), srcs)):
        assert j["err"] is None, (d, j["err"])
        at, whole = 0, []
        for h, diffs in j["calls"]:                          # one applyChanges call each: a slice [at, h)
            mine = op_diffs(src, ad, S, at, h)
            if mine.flags & LISTS:
                assert d in want_lists and any(x["type"] in ("list", "text") and x["action"] != "create" for x in diffs), d
            else:
                assert render(b, d, src, mine) == diffs, (d, at, h)
            whole += diffs
            at = h
        full = op_diffs(src, ad, S, 0, at + 9)
        assert (full.flags & LISTS != 0) == (d in want_lists), d
        if not full.flags:
            assert render(b, d, src, full) == whole, d


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_restatement_emits_the_same_diffs_on_the_known_answer_cases():
    names = ["concurrent_set", "causal_overwrite", "set_concurrent_del", "causal_del", "same_change_set_del",
             "counter_causal", "counter_concurrent_inc", "counter_concurrent_sets", "counter_float_order",
             "counter_float_history_order", "counter_int_then_float", "counter_float_concurrent",
             "forty_actors_concurrent", "forty_actors_chain", "tie_two_sets", "tie_three_sets",
             "tie_flipped_by_concurrent", "blocked_pass_order", "blocked_pass_order2", "queued_clock_quirk",
             "duplicate_noop", "heads", "nested_map", "link_vs_set"]
    by_name = {c[0]: c[1] for c in CASES}
    docs = [by_name[n] for n in names]
    b, r, srcs = sources(docs, 64)
    for d, (j, (src, ad)) in enumerate(zip(_js_calls(docs), srcs)):
        assert j["err"] is None
        whole = [x for _, diffs in j["calls"] for x in diffs]
        assert render(b, d, src, op_diffs(src, ad, 64, 0, 1 << 30)) == whole, names[d]


@pytest.mark.skipif(NODE is None, reason="node not installed")
@pytest.mark.parametrize("kw", [{}, {"arrival": 2, "shuffle_pct": 30}])
def test_js_restatement_emits_the_same_diffs_on_generated_documents(kw):
    b = synth.generate(synth.config("C2", n_docs=25, **kw), threads=2)
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    docs += [HAND[k] for k in sorted(HAND)] + [chain_doc(40, 3), one_register_doc(30)]
    _against_js(docs, want_lists={25 + sorted(HAND).index("text")})


def test_hand_written_tie_flip():
    b, r, [(src, ad)] = sources([TIE_FLIP])
    assert [int(x) for x in src.hist] == [0, 1, 2]
    got = op_diffs(src, ad, 8, 0, 3)
    assert got.flags == 0
    assert [(k, kind, [x[0] for x in sv]) for k, kind, sv in got.rows] == \
        [(k, SET_ROW, order) for k, order in enumerate(TIE_FLIP_ORDERS)]
    assert all(x[1] == V_INT and x[2] == x[0] + 1 for _, _, sv in got.rows for x in sv)   # op i set the value i + 1
    # a slice from the middle holds the same rows for its ops: the state before it counts
    assert op_diffs(src, ad, 8, 1, 2).rows == got.rows[3:4]
    assert op_diffs(src, ad, 8, 2, 2).rows == [] and op_diffs(src, ad, 8, 3, 9).rows == []


def test_hand_written_remove_and_text_flag():
    b, r, srcs = sources([HAND["del_then_reset"], HAND["text"]])
    src, ad = srcs[0]
    assert [(k, kind, len(sv)) for k, kind, sv in op_diffs(src, ad, 8, 0, 9).rows] == [(0, SET_ROW, 1), (1, REMOVE, 0), (2, SET_ROW, 1)]
    src, ad = srcs[1]
    early = op_diffs(src, ad, 8, 0, 2)                       # make, link, ins (nothing), set; then a set
    assert early.flags == 0 and [kind for _, kind, _ in early.rows] == [CREATE, SET_ROW, SET_ROW, SET_ROW]
    assert op_diffs(src, ad, 8, 0, 3) == (LISTS, []) and op_diffs(src, ad, 8, 2, 3) == (LISTS, [])
    late = op_diffs(src, ad, 8, 3, 4)                        # after the element assigns: answered again
    assert late.flags == 0 and [kind for _, kind, _ in late.rows] == [SET_ROW]
