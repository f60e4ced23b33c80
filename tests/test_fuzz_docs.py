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

from clock_diffs_ref import applied_at, causal_past, selected_at
from fields_ref import NONE as FNONE
from fields_ref import base_entries
from fields_ref import doc_ref as fields_doc_ref
from fuzz_docs import FAULTS, assigned, base_clock, gen_doc_info, gen_docs, withheld
from missing_changes_ref import closure
from missing_changes_ref import doc_ref as changes_doc_ref
from past_ref import source_of
from repo_harness import plain
from test_fields_gpu import rand_have
from test_fields_ref import against_js as fields_against_js
from test_fields_ref import requests_for
from test_list_diffs_ref import _against_js as element_diffs_against_js
from test_past_ref import prefix_replay_property
from op_diffs_cases import sources
from op_diffs_ref import LISTS, op_diffs, render
from test_op_diffs_ref import _js_calls
from waiting_ref import doc_ref as waiting_doc_ref

# sha256 of a sample of gen_doc's output, as it was before withheld() was added beside it
GEN_DOC_DIGEST = "e29921eb3f15d75b843b6b106a38b98bc72e6646d7a7697fd6c2e9dcbd06acb3"

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
        assert bool(full.flags & LISTS) == has_element_assigns([docs[d][i] for i in order], docs[d]), d   # (queued ones never ran)
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


# ---- documents for the resident-state queries: full, and with one to three changes withheld -----
QUERY_SETS = {"default": (range(1000, 1060), 8), "wide": (range(1100, 1112), 64), "long": (range(1200, 1204), 8)}


@lru_cache(maxsize=None)
def query_docs(profile):
    """[(full arrival list, kept, dropped)] of QUERY_SETS[profile]: document i withheld with seed 7000 + i"""
    seeds, _ = QUERY_SETS[profile]
    out = []
    for i, chs in enumerate(gen_docs(profile, seeds)):
        kept, dropped = withheld(chs, 7000 + i)
        out.append((chs, kept, dropped))
    return tuple(out)


@lru_cache(maxsize=None)
def withheld_merge(profile):
    """(batch, the oracle's merge) of the withheld documents at the profile's stride"""
    b = encode([kept for _, kept, _ in query_docs(profile)], QUERY_SETS[profile][1])
    return b, O.merge(b)


def test_withheld_keeps_no_copy_of_what_it_drops_and_gen_doc_is_unchanged():
    for profile in QUERY_SETS:
        for chs, kept, dropped in query_docs(profile):
            gone = [(c["actor"], c["seq"]) for c in dropped]
            assert 1 <= len(gone) <= 3 and gone == sorted(set(gone))
            assert kept and not any((c["actor"], c["seq"]) in gone for c in kept)
            assert [c for c in chs if (c["actor"], c["seq"]) not in gone] == kept
    import hashlib
    digest = hashlib.sha256(json.dumps([gen_docs("default", range(5)), gen_docs("wide", range(2)), gen_docs("long", range(1))],
                                       sort_keys=True).encode()).hexdigest()
    assert digest == GEN_DOC_DIGEST, digest


@needs_node
@pytest.mark.parametrize("profile", ["default", "wide"])
def test_js_restatement_matches_oracle_on_withheld_documents(profile):
    """history, clock, state and the queued count of documents that end blocked"""
    docs = [kept for _, kept, _ in query_docs(profile)]
    b, r = assert_js_equals_oracle(docs)
    assert (r.docs["status"] == 0).all() and 2 * int((r.docs["n_queued"] > 0).sum()) >= len(docs)


def proposal(b, d, c):
    """a dropped change as a would-be local change for document d of b (test_fields_ref.requests_for's form):
    its base clock, and the (obj, key) of its assigns as fields"""
    fields = [list(f) for f in assigned(c)]
    regs = []
    for obj, key in fields:
        oid = b.doc_objs[d].index(obj) if obj in b.doc_objs[d] else None
        regs.append(b.doc_regs[d].index((oid, key)) if (oid, key) in b.doc_regs[d] else FNONE)
    assert base_entries({}, c["actor"], c["seq"], c["deps"])[1] == any(q > 0 for q in base_clock(c).values())
    return {"actor": c["actor"], "seq": c["seq"], "deps": dict(c["deps"]), "fields": fields, "regs": regs}


@needs_node
def test_fields_reference_matches_js_on_fuzz_documents():
    """12 default and 4 wide documents, full and withheld: test_fields_ref.requests_for's would-be
    changes, and on the withheld ones every dropped change as the proposal it is."""
    sets = [query_docs("default")[:12], query_docs("wide")[:4]]
    docs = [chs for qs in sets for chs, _, _ in qs] + [kept for qs in sets for _, kept, _ in qs]
    dropped = [[] for qs in sets for _ in qs] + [dr for qs in sets for _, _, dr in qs]
    b = encode(docs, 64)
    o = O.merge(b)
    assert (o.docs["status"] == 0).all()
    rng = np.random.default_rng(9)
    reqs = {d: requests_for(b, o, d, rng, 8) + [proposal(b, d, c) for c in dropped[d]] for d in range(b.n_docs)}
    n_rows, n_unc, n_late = fields_against_js(docs, b, o, reqs)
    print(n_rows, n_unc, n_late)
    assert n_rows > 1000 and n_unc > 100 and n_late > 30


def test_closure_folds_agree():
    """missing_changes_ref.closure (fields_ref folds with the same function) and clock_diffs_ref's
    causal_past are both defined on one entry that names an applied change: its allDeps row with its
    own seq.  A closed clock folded entry by entry, in any order, is itself."""
    n = 0
    for profile in QUERY_SETS:
        b, o = withheld_merge(profile)
        S = b.a_stride
        rng = np.random.default_rng(3)
        for d in range(b.n_docs):
            c0, nc = int(b.docs["change_off"][d]), int(b.docs["n_changes"][d])
            src = source_of(b, o.hist, d)
            ad = o.all_deps[c0 * S:(c0 + nc) * S]
            for ci in np.flatnonzero(src.hist >= 0):
                a, q = int(src.changes[ci]["actor"]), int(src.changes[ci]["seq"])
                past = [int(x) for x in causal_past(src, ad, S, int(ci))]
                assert closure(src.changes, src.hist, ad, S, [(a, q)]) == past, (profile, d, ci)
                ents = [(r, past[r]) for r in rng.permutation(S) if past[r]]
                assert closure(src.changes, src.hist, ad, S, ents) == past, (profile, d, ci)
                assert int(applied_at(src, ad, S, past).sum()) == int(selected_at(src, past).sum())
                n += 1
    assert n > 1000


def query_requests(b, o, d, rng):
    """six requests for document d: test_fields_gpu.rand_have entries, the sixth one past the clock"""
    S = b.a_stride
    clock = o.clock[d * S:(d + 1) * S]
    return [rand_have(rng, clock, len(b.doc_actors[d]), late=j == 5) for j in range(6)]


def query_census(profile):
    """What the withheld documents and their requests hold, from the oracle and the references alone."""
    b, o = withheld_merge(profile)
    S = b.a_stride
    rng = np.random.default_rng(1)
    c = dict(docs=b.n_docs, status0=int((o.docs["status"] == 0).sum()), blocked=int((o.docs["n_queued"] > 0).sum()),
             rows2=0, longest=int(o.docs["n_queued"].max()), dup=0, requests=0, late=0, order=0, rows=0, uncovered=0,
             multi=0, partial=0, proposals=0, ready=0, assign=0, unknown=0)
    for d in range(b.n_docs):
        c0, nc = int(b.docs["change_off"][d]), int(b.docs["n_changes"][d])
        changes, hist, ad = b.changes[c0:c0 + nc], o.hist[c0:c0 + nc], o.all_deps[c0 * S:(c0 + nc) * S]
        c["rows2"] += int(np.count_nonzero(waiting_doc_ref(b, o, d)[0])) >= 2
        c["dup"] += bool((hist == -2).any())
        H = int((hist >= 0).sum())
        regs = list(range(int(b.docs["n_regs"][d])))
        for ents in query_requests(b, o, d, rng):
            ready, _, fl = fields_doc_ref(b, o, d, ents, regs)
            c["requests"] += 1
            c["late"] += not ready
            c["order"] += closure(changes, hist, ad, S, ents) != closure(changes, hist, ad, S, ents[::-1])
            c["rows"] += sum(len(f) for f in fl)
            c["uncovered"] += sum(1 for f in fl for r in f if not r[7])
            c["multi"] += sum(1 for f in fl if len(f) > 1)
            c["partial"] += 0 < len(changes_doc_ref(b, o, d, ents)[0]) < H
        rank = {a: i for i, a in enumerate(b.doc_actors[d])}
        for ch_ in query_docs(profile)[d][2]:
            p = proposal(b, d, ch_)
            ents, unknown = base_entries(rank, p["actor"], p["seq"], p["deps"])
            c["proposals"] += 1
            c["ready"] += fields_doc_ref(b, o, d, ents, p["regs"])[0] and not unknown
            c["assign"] += bool(p["fields"])
            c["unknown"] += unknown
    return c


@pytest.mark.parametrize("profile,order", [("default", 10), ("wide", 5), ("long", 1)])
def test_census_of_the_withheld_documents(profile, order):
    c = query_census(profile)
    print(profile, c)
    assert c["status0"] == c["docs"], c
    assert 2 * c["blocked"] >= c["docs"] and 4 * c["rows2"] >= c["docs"] and c["dup"] >= 1, c
    if profile == "long":
        assert c["longest"] > 64, c
    assert 1 <= c["late"] and 4 * c["late"] <= c["requests"], c
    assert c["order"] >= order, c
    assert 0 < c["uncovered"] < c["rows"], c
    assert 4 * c["partial"] >= c["requests"], c
    if profile == "default":
        assert c["multi"] >= 100, c
    assert c["unknown"] == 0, c                          # no withheld change names an actor its document never saw
    assert 4 * c["ready"] >= c["proposals"] and 4 * (c["proposals"] - c["ready"]) >= c["proposals"], c
    assert 4 * c["assign"] >= (2 if profile == "long" else 3) * c["proposals"], c     # (long: nine proposals in all)


def blocked_docs():
    """the 20 withheld default documents that go through test_fuzz_gpu's materialize and diff legs"""
    return [kept for _, kept, _ in query_docs("default")[:20]]


def test_prefix_replay_holds_on_blocked_documents():
    b = encode(blocked_docs(), 8)
    o = O.merge(b)
    assert (o.docs["status"] == 0).all() and 2 * int((o.docs["n_queued"] > 0).sum()) >= b.n_docs and (o.hist == -2).any()
    prefix_replay_property(b, o, every=3)


@needs_node
def test_python_diff_references_match_js_on_blocked_documents():
    docs = blocked_docs()
    kinds = element_diffs_against_js(docs)
    assert kinds["insert"] >= 20 and kinds["set"] >= 20 and kinds["remove"] >= 5, kinds
    assert map_diffs_against_js(docs) >= 50
