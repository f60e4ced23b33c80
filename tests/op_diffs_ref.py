"""What each applied op of a history slice did to its document, restated sequentially in Python
(test reference only).  Inputs are one document's log rows (past_ref.Source) with hist and all_deps
from ``oracle.merge`` of the log, never from the engine.

The document's applied changes are replayed in application order (history position of the change,
op index in the change; hist < 0 contributes nothing) over per-register survivor lists, exactly as
oracle/js/backend.js applyAssign does it:

    inc          every survivor that is a numeric counter set and that the inc's change covers
                 (all_deps[change][actor(x)] >= seq(x)) takes the inc: INT + INT stays INT (int64),
                 anything else is an f64 sum tagged FLOAT
    set/del/link the survivors the change covers are dropped; set / link append themselves
    then         the list is reversed and stably sorted by actor rank descending

A make op emits ``create``; an assign on a map / table register (reg != NONE, reg < n_regs) emits
the register as it stands after the op (``set`` with the survivors, or ``remove``); ``ins`` emits
nothing.  Only the ops of changes at history positions from <= p < to emit rows; the state is
built from position 0.  A range holding an assign on an object made by makeList / makeText is
flagged LISTS and has no rows."""
import struct
from typing import List, NamedTuple, Tuple

import numpy as np

from hypermerge_amd.columnar import DEL, DT_COUNTER, INC, LINK, MAKE_LIST, MAKE_TEXT, NONE, SET, V_FLOAT, V_INT

CREATE, SET_ROW, REMOVE = 0, 1, 2          # HM_OD_CREATE / HM_OD_SET / HM_OD_REMOVE
LISTS = 1                                   # HM_OD_LISTS
M64 = (1 << 64) - 1


class Diffs(NamedTuple):
    flags: int
    rows: List[Tuple[int, int, List[Tuple[int, int, int]]]]   # (op, kind, [(op, vtag, value bits)])


def _f64(vt: int, bits: int) -> float:
    if vt == V_INT:
        return float(bits - (1 << 64) if bits >> 63 else bits)
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def op_diffs(src, all_deps: np.ndarray, S: int, frm: int, to: int) -> Diffs:
    """src: past_ref.Source; all_deps: the document's [n_changes, S] rows (log order)."""
    all_deps = np.asarray(all_deps, np.uint32).reshape(len(src.changes), S)
    order = sorted((int(h), i) for i, h in enumerate(src.hist) if h >= 0)
    regs = {}                                # reg -> [[op, vtag, value bits, actor, seq, datatype]]
    otype = {}
    rows, lists = [], False
    for p, ci in order:
        if p >= to:
            break
        c = src.changes[ci]
        ad, actor, seq = all_deps[ci], int(c["actor"]), int(c["seq"])
        live = p >= frm
        for k in range(int(c["op_first"]), int(c["op_first"]) + int(c["n_ops"])):
            o = src.ops[k]
            act, obj, reg = int(o["action"]), int(o["obj"]), int(o["reg"])
            if act <= MAKE_TEXT:
                otype[obj] = act
                if live:
                    rows.append((k, CREATE, []))
                continue
            if act not in (SET, DEL, LINK, INC):
                continue
            if otype.get(obj) in (MAKE_LIST, MAKE_TEXT):
                lists |= live
                continue
            if reg == NONE or reg >= src.n_regs:
                continue
            sv = regs.setdefault(reg, [])
            covers = lambda x: x[3] < S and int(ad[x[3]]) >= x[4]
            if act == INC:
                ivt, ival = int(o["vtag"]), int(o["value"])
                for x in sv:
                    if x[5] != DT_COUNTER or x[1] not in (V_INT, V_FLOAT) or not covers(x):
                        continue
                    if x[1] == V_INT and ivt == V_INT:
                        x[2] = (x[2] + ival) & M64
                    else:
                        x[2] = _bits(_f64(x[1], x[2]) + _f64(ivt, ival))
                        x[1] = V_FLOAT
            else:
                sv[:] = [x for x in sv if not covers(x)]
            if act in (SET, LINK):
                sv.append([k, int(o["vtag"]), int(o["value"]), actor, seq, int(o["datatype"])])
            sv.reverse()
            sv.sort(key=lambda x: -x[3])     # (stable)
            if live:
                rows.append((k, SET_ROW if sv else REMOVE, [(x[0], x[1], x[2]) for x in sv]))
    return Diffs(LISTS, []) if lists else Diffs(0, rows)


def registers_after(src, all_deps: np.ndarray, S: int, n: int):
    """reg -> survivors [(op, vtag, value bits)] of the last row per register over [0, n)."""
    out = {}
    for k, kind, sv in op_diffs(src, all_deps, S, 0, n).rows:
        if kind != CREATE:
            out[int(src.ops[k]["reg"])] = sv
    return out


def pack(results):
    """A list of Diffs as the tables the engine returns: (rows [R, 4] u32 = op, kind, n_surv, surv_off;
    survivors [(op, vtag, value)]; ranges [n, 2]; flags [n])."""
    rows, surv, rng, flags = [], [], [], []
    for r in results:
        rng.append((len(rows), len(r.rows)))
        flags.append(r.flags)
        for k, kind, sv in r.rows:
            rows.append((k, kind, len(sv), len(surv)))
            surv.extend(sv)
    return rows, surv, rng, flags


def render(b, d: int, src, diffs: Diffs):
    """The rows as the diff objects oracle/js/backend.js emits (document d of the encoded batch b,
    whose string tables name the objects, keys, values and actors)."""
    from hypermerge_amd.columnar import DT_TIMESTAMP, V_FALSE, V_NULL, V_OBJ, V_STR, V_TRUE
    objs, regs, actors = b.doc_objs[d], b.doc_regs[d], b.doc_actors[d]
    types = ["map", "table", "list", "text"]
    otype = {int(o["obj"]): types[int(o["action"])] for o in src.ops if int(o["action"]) <= MAKE_TEXT}
    actor_of = np.zeros(len(src.ops), np.int64)
    for c in src.changes:
        actor_of[int(c["op_first"]):int(c["op_first"]) + int(c["n_ops"])] = int(c["actor"])

    def value(k, vt, bits):
        o = src.ops[k]
        if vt == V_NULL:
            v = None
        elif vt in (V_FALSE, V_TRUE):
            v = vt == V_TRUE
        elif vt == V_INT:
            v = bits - (1 << 64) if bits >> 63 else bits
        elif vt == V_FLOAT:
            v = _f64(vt, bits)
        elif vt == V_STR:
            v = b.strings[bits]
        else:
            assert vt == V_OBJ
            v = objs[bits]
        r = {"value": v}
        if int(o["action"]) == LINK:
            r["link"] = True
        if int(o["datatype"]) == DT_COUNTER:
            r["datatype"] = "counter"
        elif int(o["datatype"]) == DT_TIMESTAMP:
            r["datatype"] = "timestamp"
        return r

    out = []
    for k, kind, sv in diffs.rows:
        o = src.ops[k]
        obj = int(o["obj"])
        if kind == CREATE:
            out.append({"action": "create", "obj": objs[obj], "type": types[int(o["action"])]})
            continue
        e = {"action": "set" if kind == SET_ROW else "remove", "type": otype.get(obj, "map"), "obj": objs[obj],
             "key": regs[int(o["reg"])][1]}
        if sv:
            e.update(value(*sv[0]))
            if len(sv) > 1:
                e["conflicts"] = [dict(actor=actors[int(actor_of[x[0]])], **value(*x)) for x in sv[1:]]
        out.append(e)
    return out
