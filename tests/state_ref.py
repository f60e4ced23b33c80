"""What a document holds now, as the state calls hand it out (hm_store_state / hm_state_device /
hm_state_host), restated in Python over a merge's result tables (test reference only).  The tables
are ``oracle.merge``'s of the document's log, never the engine's.

The contract (include/hypermerge_amd.h):

    a register is live when n_surv > 0, obj != NONE and obj < n_objs
    one row (reg, obj, index, survivors) per live register, in ascending register id
    the survivors are the register's, winner first, op / vtag / value unchanged
    a live register whose surv_off + n_surv runs outside the document's slots flags the request
    BAD_ROWS, which then has no rows
    a document whose status is not OK offers nothing

``view_of`` is the consumer's half: it places the rows the way the docset's renderer does (keyed rows
under their object's keys; on a list / text object a row without an index is dropped, the others go
to elems[index], no sort) and renders hypermerge_amd/render.py's canonical form."""
from typing import List, NamedTuple, Tuple

import numpy as np

from hypermerge_amd.columnar import LINK, MAKE_LIST, MAKE_TABLE, MAKE_TEXT, NONE, SURV_RESULT_DT, V_OBJ, js_key
from hypermerge_amd.render import _DT_NAMES, _scalar

BAD_ROWS = 1                                # HM_ST_BAD_ROWS


class State(NamedTuple):
    flags: int
    rows: List[Tuple[int, int, int, List[Tuple[int, int, int]]]]   # (reg, obj, index, [(op, vtag, value bits)])


def state_of(b, r, d: int) -> State:
    """document d of batch b with the merge results r"""
    doc = b.docs[d]
    if int(r.docs["status"][d]) != 0:
        return State(0, [])
    n_ops, n_objs = int(doc["n_ops"]), int(doc["n_objs"])
    regs = r.regs[int(doc["reg_off"]):int(doc["reg_off"]) + int(doc["n_regs"])]
    surv = r.surv[int(doc["op_off"]):int(doc["op_off"]) + n_ops]
    rows = []
    for g, rr in enumerate(regs):
        ns, so, obj = int(rr["n_surv"]), int(rr["surv_off"]), int(rr["obj"])
        if ns == 0 or obj == NONE or obj >= n_objs:
            continue
        if so + ns > n_ops:
            return State(BAD_ROWS, [])
        rows.append((g, obj, int(rr["list_index"]), [(int(x["op"]), int(x["vtag"]), int(x["value"])) for x in surv[so:so + ns]]))
    return State(0, rows)


def pack(states):
    """A list of State as the tables a call returns: (rows [R, 5] i64 = reg, obj, index, n_surv, surv_off;
    survivors SURV_RESULT_DT; ranges [n, 4] = first row, rows, first survivor, survivors; flags [n])."""
    rows, surv, rng, flags = [], [], [], []
    for s in states:
        r0, s0 = len(rows), len(surv)
        for g, obj, idx, sv in s.rows:
            rows.append((g, obj, idx, len(sv), len(surv)))
            surv.extend(sv)
        rng.append((r0, len(rows) - r0, s0, len(surv) - s0))
        flags.append(s.flags)
    return (np.array(rows, np.int64).reshape(-1, 5), np.array(surv, SURV_RESULT_DT), np.array(rng, np.uint32).reshape(-1, 4),
            np.array(flags, np.uint32))


def view_of(b, d: int, state: State):
    """The document rebuilt from its state rows alone (and the log's op rows, for the objects' types
    and the ops' actors and datatypes), in render.doc_state's form."""
    doc = b.docs[d]
    ops = b.ops[int(doc["op_off"]):int(doc["op_off"]) + int(doc["n_ops"])]
    actors = b.doc_actors[d]
    op_actor = np.zeros(len(ops), np.int64)
    for c in b.changes[int(doc["change_off"]):int(doc["change_off"]) + int(doc["n_changes"])]:
        k = int(c["op_first"]) - int(doc["op_off"])
        op_actor[k:k + int(c["n_ops"])] = int(c["actor"])
    objtype = {0: -1}
    for op in ops:
        if op["action"] <= MAKE_TEXT:
            objtype.setdefault(int(op["obj"]), int(op["action"]))
    is_list = lambda o: objtype.get(o, -1) in (MAKE_LIST, MAKE_TEXT)
    keys, elems, n_el = {}, {}, {}
    for _, obj, idx, _ in state.rows:
        if is_list(obj) and idx >= 0:
            n_el[obj] = n_el.get(obj, 0) + 1
    for row in state.rows:
        g, obj, idx, sv = row
        if not is_list(obj):
            keys.setdefault(obj, []).append(row)
        elif idx >= 0:
            slot = elems.setdefault(obj, [None] * n_el[obj])
            assert idx < len(slot) and slot[idx] is None, "indices are dense and distinct"
            slot[idx] = row
    assert all(x is not None for sl in elems.values() for x in sl)

    def value_of(k, vtag, value, depth):
        if ops[k]["action"] == LINK or vtag == V_OBJ:
            return render(int(value), depth + 1)
        return _scalar(b, vtag, value)

    def entry(row, depth):
        sv = row[3]
        e = {"value": value_of(sv[0][0], sv[0][1], sv[0][2], depth)}
        if ops[sv[0][0]]["datatype"]:
            e["datatype"] = _DT_NAMES[int(ops[sv[0][0]]["datatype"])]
        if len(sv) > 1:
            e["conflicts"] = [[actors[op_actor[k]], value_of(k, vt, v, depth)] for k, vt, v in sv[1:]]
        return e

    def render(o, depth=0):
        if depth > 64:
            return {"cycle": b.doc_objs[d][o]}
        t = objtype.get(o, -1)
        if t in (MAKE_LIST, MAKE_TEXT):
            return {"text" if t == MAKE_TEXT else "list": [entry(x, depth) for x in elems.get(o, [])]}
        keyed = sorted(((b.doc_regs[d][x[0]][1], x) for x in keys.get(o, [])), key=lambda kx: js_key(kx[0]))
        return {"table" if t == MAKE_TABLE else "map": [[k, entry(x, depth)] for k, x in keyed]}

    return render(0)
