"""tests/state_ref.py — the contract of the state calls restated over the CPU oracle's merge — pinned
without a GPU: hand-written answers (tests/state_cases.py), and on the full-vocabulary documents
(tests/fuzz_docs.py) the document rebuilt from the reference rows alone against
hypermerge_amd/render.py's rendering of the same merge.

fuzz_docs.gen_doc never inserts after an element nobody inserted, so none of its documents holds a
detached element.  GRAFTED adds a few of its documents with one more change that does exactly that
to one of the document's lists; the census below counts the dead registers, conflicts and visible
elements on the generator's documents alone and the detached elements on the whole set."""
from functools import lru_cache

import numpy as np

from hypermerge_amd import render
from hypermerge_amd.columnar import INS, MAKE_LIST, MAKE_TEXT, NONE, V_FLOAT, V_INT, encode
import oracle.oracle as O

from fuzz_docs import MAKES, gen_docs
from state_cases import KNOWN, named_rows
from state_ref import BAD_ROWS, State, pack, state_of, view_of
from test_fuzz_docs import QUERY_SETS

HEAD = 0xFFFFFFFF


def grafted(chs):
    """chs plus one change by a new actor that inserts into the document's first list / text after
    an element nobody inserted (None: the document makes no list)"""
    for c in chs:
        for op in c["ops"]:
            if op["action"] in (MAKES["list"], MAKES["text"]):
                return chs + [{"actor": "zzgraft", "seq": 1, "deps": {c["actor"]: c["seq"]},
                               "ops": [{"action": "ins", "obj": op["obj"], "key": "nobody:99", "elem": 1}]}]
    return None


@lru_cache(maxsize=None)
def fuzz_set(profile):
    """(the generator's documents, then the grafted ones; how many are the generator's; the stride)"""
    seeds, S = QUERY_SETS[profile]
    docs = gen_docs(profile, seeds)
    extra = [g for g in (grafted(chs) for chs in docs[:6]) if g is not None and len({c["actor"] for c in g}) <= S]
    return tuple(docs + extra), len(docs), S


@lru_cache(maxsize=None)
def fuzz_merge(profile):
    docs, _, S = fuzz_set(profile)
    b = encode(list(docs), S)
    return b, O.merge(b)


def detached_elements(b, r, d):
    """registers of applied ins ops whose chain of predecessors never reaches _head"""
    doc = b.docs[d]
    c0, par = int(doc["change_off"]), {}
    for ci in range(int(doc["n_changes"])):
        if r.hist[c0 + ci] < 0:
            continue
        c = b.changes[c0 + ci]
        for o in b.ops[int(c["op_first"]):int(c["op_first"]) + int(c["n_ops"])]:
            if o["action"] == INS:
                par[int(o["reg"])] = int(o["parent"])
    out = []
    for g in par:
        x, seen = g, set()
        while x in par and par[x] != HEAD and par[x] not in seen:
            seen.add(par[x])
            x = par[x]
        if par.get(x) != HEAD:
            out.append(g)
    return out


def test_known_answers():
    names = sorted(KNOWN)
    b = encode([KNOWN[k][0] for k in names])
    r = O.merge(b)
    assert (r.docs["status"] == 0).all()
    states = [state_of(b, r, i) for i in range(len(names))]
    for i, k in enumerate(names):
        assert states[i].flags == 0 and named_rows(b, i, states[i]) == KNOWN[k][1], k
        assert view_of(b, i, states[i]) == render.doc_state(b, r, i), k
    by = dict(zip(names, states))
    regs = lambda k: [g for g, _, _, _ in by[k].rows]
    assert regs("deleted_key_between") == [0, 2]                          # register 1 is dead
    assert [(vt, v) for _, vt, v in by["counter_later_inc"].rows[0][3]] == [(V_INT, 13)]
    assert [(vt, v) for _, vt, v in by["counter_float"].rows[0][3]] == [(V_FLOAT, int(np.float64(3.5).view(np.uint64)))]
    assert [len(sv) for _, _, _, sv in by["two_writer_conflict"].rows] == [2]
    assert by["empty"].rows == [] and by["all_deleted"].rows == []
    # the detached elements are registers of the document, and none of them has a row
    i = names.index("detached_element")
    gone = detached_elements(b, r, i)
    assert len(gone) == 3 and not set(gone) & set(regs("detached_element"))
    # the tables of the whole call
    rows, surv, rng, fl = pack(states)
    assert rng[:, 1].sum() == len(rows) and rng[:, 3].sum() == len(surv) and not fl.any()
    assert [int(x) for x in rng[names.index("all_deleted")]][1::2] == [0, 0]
    assert (rows[:, 4] == np.concatenate([[0], np.cumsum(rows[:, 3])[:-1]])).all()   # survivors in row order


def test_a_document_that_threw_and_rows_outside_the_slots():
    from kat_cases import A, ch, s
    b = encode([[ch(A, 1, {}, s("x", 1))], [ch(A, 1, {}, s("x", 1, obj="nope"))], [ch(A, 1, {}, s("x", 1), s("y", 2))]])
    r = O.merge(b)
    assert [int(x) for x in r.docs["status"]] == [0, 2, 0]
    assert state_of(b, r, 1) == State(0, [])
    assert len(state_of(b, r, 2).rows) == 2
    # a survivor list that leaves the document's slots: no rows, nothing read
    g = int(b.docs["reg_off"][2]) + 1
    r.regs["surv_off"][g] = int(b.docs["n_ops"][2])
    assert state_of(b, r, 2) == State(BAD_ROWS, [])
    # an object id the document does not have, and an untouched register, are not live
    r.regs["surv_off"][g] = 1
    r.regs["obj"][g] = int(b.docs["n_objs"][2])
    assert [x[0] for x in state_of(b, r, 2).rows] == [0]
    r.regs["obj"][g] = NONE
    assert [x[0] for x in state_of(b, r, 2).rows] == [0]


def test_full_vocabulary_documents_rebuild_from_their_rows():
    census = dict(dead=0, conflict=0, visible=0, detached=0, docs=0)
    for profile in ("default", "wide", "long"):
        b, r = fuzz_merge(profile)
        n_gen = fuzz_set(profile)[1]
        assert (r.docs["status"] == 0).all()
        for i in range(b.n_docs):
            st = state_of(b, r, i)
            assert st.flags == 0
            assert view_of(b, i, st) == render.doc_state(b, r, i), (profile, i)
            assert [x[0] for x in st.rows] == sorted(x[0] for x in st.rows)
            doc = b.docs[i]
            ops = b.ops[int(doc["op_off"]):int(doc["op_off"]) + int(doc["n_ops"])]
            lists = {int(o["obj"]) for o in ops if o["action"] in (MAKE_LIST, MAKE_TEXT)}
            census["docs"] += 1
            census["detached"] += len(detached_elements(b, r, i))
            if i < n_gen:
                census["dead"] += int(doc["n_regs"]) - len(st.rows)
                census["conflict"] += sum(1 for x in st.rows if len(x[3]) > 1)
                census["visible"] += sum(1 for x in st.rows if x[1] in lists and x[2] >= 0)
    assert all(census[k] >= 1 for k in ("dead", "conflict", "visible", "detached")), census
