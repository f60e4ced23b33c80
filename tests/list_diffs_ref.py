"""What each applied op of a history slice did to its document, list / text elements included,
restated sequentially in Python (test reference only; the map / table part repeats
tests/op_diffs_ref.py, which stays the reference of the calls without the option).

An element assign k (set / del / link / inc) on the register of element e of list L, with
``after`` = the register holds survivors after k and ``before`` = it did after the previous
applied assign on e (False without one):

    before  after   row
    yes     yes     ELEM_SET at index
    yes     no      ELEM_REMOVE at index
    no      yes     ELEM_INSERT at index (the diff also names the element id)
    no      no      no row

``index`` = the elements f != e of L that precede e in L's RGA order and are visible (their last
applied assign left survivors) just before k.  RGA order is the pre-order from ``_head`` of the tree
of the applied ``ins`` ops of the prefix [0, to), the children of one parent by (elem, actor rank)
descending; the order of the whole prefix serves every moment inside it.  ``pos`` numbers it across
the document, the lists end to end in object order.  Nothing of oracle/js/backend.js's elemIds
bookkeeping is kept: visibility is a set, the index a count over it.

Rows are ``(op, kind, index | None, survivors)``.  An element assign on a register that no applied
ins made sets BAD_ROWS and emits nothing."""
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from hypermerge_amd.columnar import DEL, DT_COUNTER, INC, INS, LINK, MAKE_LIST, MAKE_TEXT, NONE, SET, V_FLOAT, V_INT

from op_diffs_ref import CREATE, LISTS, M64, REMOVE, SET_ROW, _bits, _f64

ELEM_INSERT, ELEM_SET, ELEM_REMOVE = 3, 4, 5     # HM_OD_ELEM_*
HEAD = NONE                                       # HM_HEAD
BAD_ROWS = 2                                      # HM_OD_BAD_ROWS


class ListDiffs(NamedTuple):
    flags: int
    rows: List[Tuple[int, int, Optional[int], List[Tuple[int, int, int]]]]
    bad: int = 0


def rga_positions(src, to: int):
    """(pos by element register, first pos by object) over the applied ins ops of the prefix [0, to)"""
    kids = {}                                 # parent key -> [(elem, actor rank, reg)]
    for i, h in enumerate(src.hist):
        if not 0 <= int(h) < to:
            continue
        c = src.changes[i]
        for k in range(int(c["op_first"]), int(c["op_first"]) + int(c["n_ops"])):
            o = src.ops[k]
            if int(o["action"]) != INS:
                continue
            parent = int(o["parent"])
            key = ("head", int(o["obj"])) if parent == HEAD else ("reg", parent)
            kids.setdefault(key, []).append((int(o["elem"]), int(c["actor"]), int(o["reg"])))
    pos, first = {}, {}
    for obj in sorted(x[1] for x in kids if x[0] == "head"):
        first[obj] = len(pos)
        stack = [("head", obj)]
        while stack:                          # pre-order; children by (elem, rank) descending
            key = stack.pop()
            if key[0] == "reg":
                pos[key[1]] = len(pos)
            for _, _, reg in sorted(kids.get(key, [])):          # (ascending onto a stack: popped descending)
                stack.append(("reg", reg))
    return pos, first


def list_diffs(src, all_deps: np.ndarray, S: int, frm: int, to: int, hint: bool = True) -> ListDiffs:
    """src: past_ref.Source; all_deps: the document's [n_changes, S] rows (log order).  hint = the
    document's HM_DOC_HAS_LISTS: without it an element assign in the range flags LISTS, as
    op_diffs_ref does."""
    all_deps = np.asarray(all_deps, np.uint32).reshape(len(src.changes), S)
    order = sorted((int(h), i) for i, h in enumerate(src.hist) if h >= 0)
    pos, first = rga_positions(src, min(to, len(order))) if hint else ({}, {})
    regs, otype, visible = {}, {}, {}         # visible: obj -> {reg: pos}
    rows, lists, bad = [], False, 0
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
                    rows.append((k, CREATE, None, []))
                continue
            if act not in (SET, DEL, LINK, INC):
                continue
            element = otype.get(obj) in (MAKE_LIST, MAKE_TEXT)
            if element and not hint:
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
            out = [(x[0], x[1], x[2]) for x in sv]
            if not element:
                if live:
                    rows.append((k, SET_ROW if sv else REMOVE, None, out))
                continue
            if reg not in pos or obj not in first:
                bad |= BAD_ROWS
                continue
            vis = visible.setdefault(obj, {})
            before, after = reg in vis, bool(sv)
            index = sum(1 for f, q in vis.items() if f != reg and q < pos[reg])
            if after:
                vis[reg] = pos[reg]
            else:
                vis.pop(reg, None)
            if live and (before or after):
                rows.append((k, ELEM_SET if before and after else ELEM_REMOVE if before else ELEM_INSERT, index, out))
    return ListDiffs(LISTS, [], bad) if lists else ListDiffs(0, rows, bad)


def visible_after(src, all_deps, S: int, n: int):
    """the element registers visible after the prefix [0, n), ordered by pos, per object"""
    pos, _ = rga_positions(src, n)
    last = {}
    for k, kind, index, sv in list_diffs(src, all_deps, S, 0, n).rows:
        if kind in (ELEM_INSERT, ELEM_SET, ELEM_REMOVE):
            last[int(src.ops[k]["reg"])] = (int(src.ops[k]["obj"]), kind != ELEM_REMOVE)
    out = {}
    for reg, (obj, vis) in last.items():
        if vis:
            out.setdefault(obj, []).append(reg)
    return {obj: sorted(r, key=pos.__getitem__) for obj, r in out.items()}


def pack(results):
    """A list of ListDiffs as the tables the engine returns: (rows [R, 4] u32 = op, kind, n_surv,
    surv_off; survivors [(op, vtag, value)]; ranges [n, 2]; flags [n]; index [R], NONE where a row
    has none)."""
    rows, surv, rng, flags, index = [], [], [], [], []
    for r in results:
        rng.append((len(rows), len(r.rows)))
        flags.append(r.flags)
        for k, kind, ix, sv in r.rows:
            rows.append((k, kind, len(sv), len(surv)))
            index.append(NONE if ix is None else ix)
            surv.extend(sv)
    return rows, surv, rng, flags, index


def render(b, d: int, src, diffs: ListDiffs):
    """The rows as the diff objects oracle/js/backend.js emits (document d of the encoded batch b)."""
    import op_diffs_ref
    regs = b.doc_regs[d]
    objs = b.doc_objs[d]
    types = ["map", "table", "list", "text"]
    otype = {int(o["obj"]): types[int(o["action"])] for o in src.ops if int(o["action"]) <= MAKE_TEXT}
    out = []
    for k, kind, index, sv in diffs.rows:
        plain = op_diffs_ref.render(b, d, src, op_diffs_ref.Diffs(0, [(k, SET_ROW if sv else REMOVE, sv) if kind > REMOVE else (k, kind, sv)]))[0]
        if kind <= REMOVE:
            out.append(plain)
            continue
        o = src.ops[k]
        e = {x: v for x, v in plain.items() if x not in ("key", "action")}
        e.update(action={ELEM_INSERT: "insert", ELEM_SET: "set", ELEM_REMOVE: "remove"}[kind], index=index,
                 type=otype[int(o["obj"])], obj=objs[int(o["obj"])])
        if kind == ELEM_INSERT:
            e["elemId"] = regs[int(o["reg"])][1]
        out.append(e)
    return out
