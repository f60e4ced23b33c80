"""The full-vocabulary document generator (tests/fuzz_docs.py) on the CPU: the two restatements
(oracle/oracle.c and oracle/js/backend.js) and the Python diff references agree on its documents,
its injected faults throw where they were put, and a census of the oracle's results keeps it from
going vacuous.  The GPU legs over the same documents are tests/test_fuzz_gpu.py."""
import json
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from hypermerge_amd.columnar import (DEL, DT_COUNTER, INC, INS, LINK, MAKE_LIST, MAKE_MAP, MAKE_TABLE, MAKE_TEXT, NONE, SET,
                                     STATUS, encode)
from hypermerge_amd.render import doc_state
import oracle.oracle as O

from fuzz_docs import FAULTS, gen_doc_info, gen_docs
from repo_harness import plain
from test_list_diffs_ref import _against_js as element_diffs_against_js
from op_diffs_cases import sources
from op_diffs_ref import LISTS, op_diffs, render
from test_op_diffs_ref import _js_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
needs_node = pytest.mark.skipif(NODE is None, reason="node not installed")
CODE = {v: k for k, v in STATUS.items()}


@lru_cache(maxsize=None)
def default_docs(n=400):
    return tuple(gen_docs("default", range(n)))


@lru_cache(maxsize=None)
def fault_docs(n=80):
    """[(changes, info)]: n documents, the five kinds in turn"""
    return tuple(gen_doc_info(5000 + i, fault=FAULTS[i % len(FAULTS)]) for i in range(n))


def js_backend(docs, seed=2):
    """every document through the JS restatement's DocBackend in three calls"""
    rng = np.random.default_rng(seed)
    chunks = []
    for chs in docs:
        lo, hi = sorted(int(x) for x in rng.integers(0, len(chs) + 1, size=2))
        chunks.append([chs[:lo], chs[lo:hi], chs[hi:]])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_cpu_backend.js")],
                       input=json.dumps({"docs": chunks}), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])["docs"]


def assert_js_equals_oracle(docs):
    js = js_backend(docs)
    b = encode(docs)
    r = O.merge(b)
    S = b.a_stride
    for i, (chs, j) in enumerate(zip(docs, js)):
        st = int(r.docs["status"][i])
        assert (j["err"] is None) == (st == 0), (i, j["err"], st)
        if st:
            continue
        c0, nc = int(b.docs["change_off"][i]), int(b.docs["n_changes"][i])
        pos = r.hist[c0:c0 + nc]
        order = [chs[k] for k in np.argsort(np.where(pos >= 0, pos, 1 << 30), kind="stable")[:int((pos >= 0).sum())]]
        assert j["history"] == [[c["actor"], c["seq"]] for c in order], i
        assert j["queued"] == int(r.docs["n_queued"][i]), i
        actors = b.doc_actors[i]
        assert j["clock"] == {actors[a]: int(v) for a, v in enumerate(r.clock[i * S:(i + 1) * S]) if v}, i
        assert j["doc"] == plain(doc_state(b, r, i)), i
    return b, r


def test_plain_renders_a_table_as_a_map_of_its_rows():
    from kat_cases import A, ch, link, mk, s
    doc = [ch(A, 1, {}, mk("makeTable", "t"), link("tab", "t"), mk("makeMap", "row"), link("r1", "row", obj="t"),
              s("name", "x", obj="row"), s("note", 3, obj="t"))]
    b = encode([doc])
    state = doc_state(b, O.merge(b), 0)
    assert "table" in state["map"][0][1]["value"]
    assert plain(state) == {"tab": {"r1": {"name": "x"}, "note": 3}}


@needs_node
def test_js_restatement_matches_oracle_on_default_documents():
    b, r = assert_js_equals_oracle(list(default_docs()))
    assert (r.docs["status"] == 0).all()


@needs_node
def test_js_restatement_matches_oracle_on_wide_documents():
    b, r = assert_js_equals_oracle(gen_docs("wide", range(40)))
    assert (r.docs["status"] == 0).all() and int(b.docs["n_actors"].max()) > 8


def fault_positions(chs, info):
    """arrival indices of the changes holding the injected (actor, seq)"""
    return [i for i, c in enumerate(chs) if (c["actor"], c["seq"]) == (info["actor"], info["seq"])]


def assert_fault_is_where_it_was_put(chs, info, row):
    """The generator writes no other throwing op, so the injected kind is what the document throws:
    at one of the arrival positions of the injected change (delivery may copy it; of the two
    changes of an INCONSISTENT_SEQ pair the one applied second throws), at the injected op."""
    assert int(row["status"]) == CODE[info["kind"]], (info, row)
    where = fault_positions(chs, info)
    assert int(row["err_change"]) in where, (info, row, where)
    if info["op"] is None:
        assert len(where) >= 2 and int(row["err_op"]) == NONE
    else:
        assert int(row["err_op"]) == info["op"], (info, row)
        if len(where) == 1:
            assert int(row["err_change"]) == where[0]


def test_fault_documents_throw_the_injected_kind_at_the_injected_op():
    docs = fault_docs()
    b = encode([chs for chs, _ in docs])
    r = O.merge(b)
    for i, (chs, info) in enumerate(docs):
        assert_fault_is_where_it_was_put(chs, info, r.docs[i])
    assert {info["kind"] for _, info in docs} == set(FAULTS)


@needs_node
def test_js_restatement_errors_on_the_fault_documents():
    docs = [chs for chs, _ in fault_docs()]
    js = js_backend(docs)
    assert all(j["err"] is not None for j in js), [i for i, j in enumerate(js) if j["err"] is None]
    assert_js_equals_oracle(docs)


def has_element_assigns(chs, doc=None):
    """do the changes assign an element of a list or text (made anywhere in the document)?"""
    lists = {op["obj"] for c in (doc or chs) for op in c["ops"] if op["action"] in ("makeList", "makeText")}
    return any(op["action"] in ("set", "del", "link", "inc") and op["obj"] in lists for c in chs for op in c["ops"])


def map_diffs_against_js(docs):
    """test_op_diffs_ref._against_js, for documents whose element assigns need not emit a diff (an
    inc or a del of an element that is not visible emits none): a slice is flagged LISTS exactly
    when it holds an assign on a list or text object, and every other slice renders as the JS
    restatement's diffs of that call."""
    b, r, srcs = sources(docs)
    S = b.a_stride
    answered = 0
    for d, (j, (src, ad)) in enumerate(zip(_js_calls(docs), srcs)):
        assert j["err"] is None, (d, j["err"])
        order = [i for _, i in sorted((int(h), i) for i, h in enumerate(src.hist) if h >= 0)]
        at, whole = 0, []
        for h, diffs in j["calls"]:
            mine = op_diffs(src, ad, S, at, h)
            assert bool(mine.flags & LISTS) == has_element_assigns([docs[d][i] for i in order[at:h]], docs[d]), (d, at, h)
            if not mine.flags:
                assert render(b, d, src, mine) == diffs, (d, at, h)
                answered += h > at
            whole += diffs
            at = h
        full = op_diffs(src, ad, S, 0, at + 9)
        assert bool(full.flags & LISTS) == has_element_assigns(docs[d]), d
        if not full.flags:
            assert render(b, d, src, full) == whole, d
    return answered


@needs_node
def test_python_diff_references_match_js_on_default_documents():
    docs = list(default_docs()[:100])
    kinds = element_diffs_against_js(docs)
    assert kinds["insert"] >= 100 and kinds["set"] >= 100 and kinds["remove"] >= 100, kinds
    assert map_diffs_against_js(docs) >= 500


def census(b, r):
    """What the documents hold, from the batch and the oracle's results alone."""
    out = dict(lists=0, reordered=0, multi=int((r.regs["n_surv"] > 1).sum()), link_under_elem=0, list_in_list=0,
               inc_counter_elem=0, unassigned_elem=0, table_row=0, many_lists=0, small=0, large=0)
    for d in range(b.n_docs):
        row = b.docs[d]
        o0, m, g0, R = int(row["op_off"]), int(row["n_ops"]), int(row["reg_off"]), int(row["n_regs"])
        c0, nc = int(row["change_off"]), int(row["n_changes"])
        ops, regs, surv = b.ops[o0:o0 + m], r.regs[g0:g0 + R], r.surv[o0:o0 + m]
        kind = {int(op["obj"]): int(op["action"]) for op in ops if op["action"] <= MAKE_TEXT}
        is_list = lambda obj: kind.get(int(obj)) in (MAKE_LIST, MAKE_TEXT)
        n_lists = sum(k in (MAKE_LIST, MAKE_TEXT) for k in kind.values())
        out["lists"] += n_lists > 0
        out["many_lists"] += n_lists > 2
        out["reordered"] += not np.array_equal(r.hist[c0:c0 + nc], np.arange(nc))
        out["small" if m <= 256 else "large"] += 1
        assigned = {int(op["reg"]) for op in ops if op["action"] in (SET, DEL, LINK, INC)}
        inced = {int(op["reg"]) for op in ops if op["action"] == INC and is_list(op["obj"])}
        flags = set()
        for g in range(R):
            rr = regs[g]
            live = surv[int(rr["surv_off"]):int(rr["surv_off"]) + int(rr["n_surv"])]
            for x in live:
                op = ops[int(x["op"])]
                if op["action"] == LINK and is_list(op["obj"]) and int(rr["list_index"]) >= 0:
                    flags.add("link_under_elem")
                    if is_list(op["value"]):
                        flags.add("list_in_list")
                if op["action"] == LINK and kind.get(int(op["obj"])) == MAKE_TABLE and kind.get(int(op["value"])) == MAKE_MAP:
                    flags.add("table_row")
                if (g in inced and op["action"] == SET and op["datatype"] == DT_COUNTER
                        and (int(x["vtag"]), int(x["value"])) != (int(op["vtag"]), int(op["value"]))):
                    flags.add("inc_counter_elem")               # the survivor no longer holds what was set
        for op in ops:
            if op["action"] == INS and int(op["reg"]) not in assigned:
                flags.add("unassigned_elem")
        for f in flags:
            out[f] += 1
    return out


def test_census_of_the_default_documents():
    docs = list(default_docs())
    b = encode(docs, 6)
    r = O.merge(b)
    assert (r.docs["status"] == 0).all(), np.unique(r.docs["status"])       # (so none is UNSUPPORTED either)
    c = census(b, r)
    print(c)
    assert c["lists"] >= 300, c
    assert c["reordered"] >= 150, c
    assert c["multi"] >= 500, c
    for k in ("link_under_elem", "list_in_list", "inc_counter_elem", "unassigned_elem", "table_row", "many_lists",
              "small", "large"):
        assert c[k] >= 1, (k, c)
