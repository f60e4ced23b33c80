"""The fields a proposed change touches: the test reference (tests/fields_ref.py) pinned three ways
(no GPU here) — on the C oracle's merges of synthetic documents against the dependency graph walked
change by change, on the JS restatement (oracle/js/backend.js through tests/js/run_fields.js) for
seeded would-be changes, and on cases written out by hand — and the new C-ABI names."""
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from hypermerge_amd import engine, synth
from hypermerge_amd.columnar import decode_doc, encode
import oracle.oracle as O

from fields_ref import NONE, base_entries, doc_ref
from kat_cases import ch, inc, link, mk, s
from test_missing_changes_host import A, B, Cc, CHAIN, D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SET, LINK = 5, 7
V_NULL, V_FALSE, V_TRUE, V_INT, V_FLOAT, V_STR, V_OBJ = range(7)
DATATYPE = {0: None, 1: "counter", 2: "timestamp"}


def value_of(b, d, vtag, value):
    """A survivor's resolved value as the JS value it stands for."""
    if vtag == V_INT:
        return value - (1 << 64) if value >= 1 << 63 else value
    if vtag == V_FLOAT:
        return struct.unpack("<d", struct.pack("<Q", value))[0]
    if vtag == V_STR:
        return b.strings[value]
    if vtag == V_OBJ:
        return b.doc_objs[d][value]
    return {V_NULL: None, V_FALSE: False, V_TRUE: True}[vtag]


def as_ops(b, d, rows):
    """fields_ref rows as the op dicts the JS side and the docset print."""
    out = []
    for op, action, dt, vtag, value, a, q, cov in rows:
        o = {"action": "link" if action == LINK else "set", "value": value_of(b, d, vtag, value),
             "actor": b.doc_actors[d][a], "seq": q, "covered": cov}
        if DATATYPE[dt]:
            o["datatype"] = DATATYPE[dt]
        out.append(o)
    return out


# ---- (1) the C oracle's merges against the dependency graph --------------------------------------
def ancestors(b, o, d, a, q):
    """Per rank the largest seq among (a, q) and the changes it reaches through dep rows and its
    actor's earlier changes: walked change by change, all_deps not read."""
    row = b.docs[d]
    c0, n = int(row["change_off"]), int(row["n_changes"])
    at = {(int(c["actor"]), int(c["seq"])): c0 + i for i, c in enumerate(b.changes[c0:c0 + n]) if o.hist[c0 + i] >= 0}
    top = [0] * b.a_stride
    todo = [(a, q)]
    while todo:
        x, y = todo.pop()
        if y <= top[x]:
            continue
        for k in range(top[x] + 1, y + 1):                  # (x, k) for every k up to y: one actor's chain
            c = b.changes[at[(x, k)]]
            for dep in b.deps[int(c["dep_off"]):int(c["dep_off"]) + int(c["n_deps"])]:
                todo.append((int(dep["actor"]), int(dep["seq"])))
        top[x] = y
    return top


@pytest.mark.parametrize("name,n,kw", [("C2", 10, {"arrival": 2, "shuffle_pct": 30}), ("C3", 2, {"changes_per_actor": 20}),
                                       ("C5", 10, {})])
def test_reference_on_oracle_merges(name, n, kw):
    b = synth.generate(synth.config(name, n_docs=n, **kw), threads=2)
    o = O.merge(b)
    S = b.a_stride
    rng = np.random.default_rng(4)
    rows_seen = uncovered = 0
    for d in range(b.n_docs):
        if int(o.docs["status"][d]) != 0:
            continue
        row = b.docs[d]
        c0, nc, o0, r0, nr = (int(row[f]) for f in ("change_off", "n_changes", "op_off", "reg_off", "n_regs"))
        clock = [int(x) for x in o.clock[d * S:(d + 1) * S]]
        live = [r for r in range(nr) if int(o.regs[r0 + r]["n_surv"])]
        regs = [int(x) for x in rng.permutation(live)[:40]] + [nr, nr + 7]
        applied = [c0 + i for i in range(nc) if o.hist[c0 + i] >= 0]
        picks = [int(x) for x in rng.permutation(applied)[:4]]
        whole = [(a, q) for a, q in enumerate(clock) if q]
        for entries, top in [(whole, clock), ([], [0] * S)] + [
                ([(int(b.changes[i]["actor"]), int(b.changes[i]["seq"]))],
                 ancestors(b, o, d, int(b.changes[i]["actor"]), int(b.changes[i]["seq"]))) for i in picks]:
            ready, deps, fl = doc_ref(b, o, d, entries, regs)
            assert ready and deps == top, (name, d, entries)
            assert fl[-1] == [] and fl[-2] == []
            for reg, rows in zip(regs, fl):
                if reg >= nr:
                    continue
                assert len(rows) == int(o.regs[r0 + reg]["n_surv"])
                for k, (op, action, dt, vtag, value, a, q, cov) in enumerate(rows):
                    p = b.ops[o0 + op]
                    assert int(p["reg"]) == reg and action == int(p["action"]) and action in (SET, LINK)
                    c = [i for i in applied if int(b.changes[i]["op_first"]) <= o0 + op < int(b.changes[i]["op_first"]) + int(b.changes[i]["n_ops"])]
                    assert len(c) == 1 and (a, q) == (int(b.changes[c[0]]["actor"]), int(b.changes[c[0]]["seq"]))
                    assert cov == (top[a] >= q), (name, d, entries, reg, k)
                    sv = o.surv[o0 + int(o.regs[r0 + reg]["surv_off"]) + k]
                    assert (op, vtag, value) == (int(sv["op"]), int(sv["vtag"]), int(sv["value"]))
                    rows_seen += 1
                    uncovered += not cov
        # one past the clock is not ready
        a = int(np.argmax(clock))
        assert doc_ref(b, o, d, [(a, clock[a] + 1)], regs) == (False, [0] * S, [[] for _ in regs])
    assert rows_seen > 100 and uncovered > 20        # (the inputs reach both answers)


# ---- (2) the JS restatement ---------------------------------------------------------------------
def requests_for(b, o, d, rng, k):
    """k would-be changes for document d: an actor of the document or a new one, deps a random part
    of the clock (not causally closed in general, its own actor among them at times), a few one past
    the clock (not ready); fields: live registers, an untouched key, an unknown object."""
    S = b.a_stride
    actors = b.doc_actors[d]
    clock = {actors[a]: int(q) for a, q in enumerate(o.clock[d * S:(d + 1) * S]) if q}
    r0, nr = int(b.docs[d]["reg_off"]), int(b.docs[d]["n_regs"])
    live = [r for r in range(nr) if int(o.regs[r0 + r]["n_surv"])]
    out = []
    for j in range(k):
        actor = "zz-new" if j % 3 == 0 or not clock else list(clock)[int(rng.integers(0, len(clock)))]
        seq = clock.get(actor, 0) + 1
        names = [a for a in rng.permutation(list(clock))[:int(rng.integers(0, len(clock) + 1))]]
        deps = {str(a): int(rng.integers(0, clock[a] + 1)) for a in names}
        if j % 4 == 3 and clock:
            late = list(clock)[int(rng.integers(0, len(clock)))]
            if late == actor:
                seq += 1
            else:
                deps[late] = clock[late] + 1
        regs = [int(x) for x in rng.permutation(live)[:6]]
        fields = [[b.doc_objs[d][b.doc_regs[d][r][0]], b.doc_regs[d][r][1]] for r in regs]
        fields += [[b.doc_objs[d][0], "no-such-key"], ["no-such-object", "k"]]
        out.append({"actor": actor, "seq": seq, "deps": deps, "fields": fields, "regs": regs + [NONE, NONE]})
    return out


def against_js(docs, b, o, reqs):
    """The would-be changes reqs {document: [request]} (requests_for's form) through the JS restatement
    of applyLocalChange's bookkeeping against the reference on (b, o): ready flags and every field's
    ops.  Returns (rows, rows not covered, requests not ready)."""
    keep = sorted(reqs)
    payload = {"docs": [{"changes": docs[d], "reqs": [{k: r[k] for k in ("actor", "seq", "deps", "fields")} for r in reqs[d]]}
                        for d in keep]}
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_fields.js")], input=json.dumps(payload),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    js = json.loads(p.stdout.strip().splitlines()[-1])["docs"]
    n_rows = n_unc = n_late = 0
    for d, got in zip(keep, js):
        rank = {a: i for i, a in enumerate(b.doc_actors[d])}
        for r, g in zip(reqs[d], got):
            ents, unknown = base_entries(rank, r["actor"], r["seq"], r["deps"])
            ready, _, fl = doc_ref(b, o, d, ents, r["regs"])
            ready = ready and not unknown
            want = {"ready": ready, "fields": [as_ops(b, d, rows) if ready else [] for rows in fl]}
            assert g == want, (d, r)
            n_late += not ready
            n_rows += sum(len(f) for f in want["fields"])
            n_unc += sum(1 for f in want["fields"] for x in f if not x["covered"])
    return n_rows, n_unc, n_late


@pytest.mark.skipif(NODE is None, reason="node not installed")
@pytest.mark.parametrize("name,n,kw", [("C2", 12, {"arrival": 2, "shuffle_pct": 30}), ("C3", 4, {"changes_per_actor": 15}),
                                       ("C5", 12, {})])
def test_reference_matches_js_restatement(name, n, kw):
    b0 = synth.generate(synth.config(name, n_docs=n, **kw), threads=2)
    docs = [decode_doc(b0, i) for i in range(b0.n_docs)]
    b = encode(docs, 8)
    o = O.merge(b)
    rng = np.random.default_rng(9)
    keep = [d for d in range(b.n_docs) if int(o.docs["status"][d]) == 0]
    n_rows, n_unc, n_late = against_js(docs, b, o, {d: requests_for(b, o, d, rng, 8) for d in keep})
    assert n_rows > 100 and n_unc > 10 and n_late > 5


# ---- (3) by hand --------------------------------------------------------------------------------
F15 = struct.unpack("<Q", struct.pack("<d", 1.5))[0]


def test_reference_on_hand_cases():
    # CHAIN: B1 B2 B3 set y, A1 sets x, A2 (deps B:3) sets x; allDeps(A2) = {A:1, B:3}.  y's one op is
    # B3's (op 2).  {A:2, B:1}: B is SET to 1 after A2's closure raised it to 3: B3 is not covered;
    # {B:1, A:2}: A2's closure comes last and B stays 3: covered
    b = encode([CHAIN], 8)
    o = O.merge(b)
    y, x = b.doc_regs[0].index((0, "y")), b.doc_regs[0].index((0, "x"))
    assert doc_ref(b, o, 0, [(0, 2), (1, 1)], [y, x]) == (
        True, [2, 1, 0, 0, 0, 0, 0, 0], [[(2, SET, 0, V_INT, 3, 1, 3, False)], [(4, SET, 0, V_INT, 2, 0, 2, True)]])
    assert doc_ref(b, o, 0, [(1, 1), (0, 2)], [y, x]) == (
        True, [2, 3, 0, 0, 0, 0, 0, 0], [[(2, SET, 0, V_INT, 3, 1, 3, True)], [(4, SET, 0, V_INT, 2, 0, 2, True)]])
    # the would-be change cccc:1 with those deps: its own actor (never seen, seq - 1 = 0) is dropped
    rank = {a: i for i, a in enumerate(b.doc_actors[0])}
    assert base_entries(rank, Cc, 1, {A: 2, B: 1}) == ([(0, 2), (1, 1)], False)
    assert base_entries(rank, A, 3, {B: 1, A: 1}) == ([(1, 1), (0, 2)], False)      # the own actor keeps its place
    assert base_entries(rank, A, 3, {B: 1}) == ([(1, 1), (0, 2)], False)            # ... or goes last
    assert base_entries(rank, Cc, 2, {})[1] and base_entries(rank, A, 3, {Cc: 1})[1]
    # an actor id in decimal digits only is an array index to JS: Object.keys lists it first, by number
    # (found by the fuzz documents' random hex names, tests/test_fuzz_docs.py)
    digits = {"19613698": 0, "5a5c4689": 1, "777": 2, "0123": 3}
    assert base_entries(digits, "5a5c4689", 7, {"5a5c4689": 2, "19613698": 3, "0123": 1, "777": 4}) == \
        ([(2, 4), (0, 3), (1, 6), (3, 1)], False)
    # not ready: aaaa:3 is not applied
    assert doc_ref(b, o, 0, [(0, 3)], [y, x]) == (False, [0] * 8, [[], []])

    # a counter turned FLOAT by a later inc, a link, a register only a queued change names, one past n_regs
    h = [ch(A, 1, {}, s("c", 1, datatype="counter"), mk("makeMap", "M"), link("m", "M")), ch(B, 1, {A: 1}, inc("c", 0.5)),
         ch(D, 1, {Cc: 1}, s("w", 1))]
    b = encode([h], 8)
    o = O.merge(b)
    assert list(o.hist) == [0, 1, -1] and b.doc_regs[0] == [(0, "c"), (0, "m"), (0, "w")]
    M = b.doc_objs[0].index("M")
    want = [[(0, SET, 1, V_FLOAT, F15, 0, 1, True)], [(2, LINK, 0, V_OBJ, M, 0, 1, True)], [], []]
    assert doc_ref(b, o, 0, [(1, 1)], [0, 1, 2, 3]) == (True, [1, 1, 0, 0, 0, 0, 0, 0], want)
    none = [[r[:7] + (False,) for r in f] for f in want]
    assert doc_ref(b, o, 0, [], [0, 1, 2, 3]) == (True, [0] * 8, none)
    assert doc_ref(b, o, 0, [(3, 1)], [0]) == (False, [0] * 8, [[]])               # dddd:1 is queued, not applied
    assert as_ops(b, 0, want[0] + want[1]) == [
        {"action": "set", "value": 1.5, "datatype": "counter", "actor": A, "seq": 1, "covered": True},
        {"action": "link", "value": "M", "actor": A, "seq": 1, "covered": True}]


# ---- (4) the C-ABI names ------------------------------------------------------------------------
def test_new_symbols_exported_and_declared():
    src = open(os.path.join(ROOT, "include", "hypermerge_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = engine.lib()
    for name in ("hm_store_fields", "hm_fields_device", "hm_fields_host", "hm_docset_fields"):
        assert name in engine.EXPORTS and hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, src), name
    assert engine.FIELD_OP_DT.itemsize == 24                      # sizeof(hm_field_op)
    assert [engine.FIELD_OP_DT.fields[f][1] for f in ("op", "seq", "actor", "action", "datatype", "vtag", "covered", "value")] == \
        [0, 4, 8, 10, 11, 12, 13, 16]
    assert (engine.FLD_NOT_READY, engine.FLD_BAD_ROWS) == (1, 2)
    assert L.hm_abi_version() == 4
