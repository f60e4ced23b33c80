"""Documents the list-diff tests share.  LHAND: hand-written cases, each naming the rule it
exercises, with the rows it must give written out by hand as (op, kind, index, [survivor ops]) in
application order (ops are numbered through the document in the order written).  Below them the
generated boundary documents of the device tests."""
from kat_cases import A, B, Cc, ch, d, inc, ins, link, mk, s

from list_diffs_ref import ELEM_INSERT as INS_, ELEM_REMOVE as REM_, ELEM_SET as SET_
from op_diffs_ref import CREATE, SET_ROW


def e(actor, n):
    return f"{actor}:{n}"


def typed(obj, actor, first, n, after="_head", value=lambda i: chr(97 + i % 26)):
    """n elements typed one after another by one actor: ins + set each (elems first .. first + n - 1)"""
    ops = []
    for i in range(n):
        ops += [ins(obj, after, first + i), s(e(actor, first + i), value(i), obj=obj)]
        after = e(actor, first + i)
    return ops


_ABC = [ch(A, 1, {}, mk("makeText", "T"), link("t", "T"), *typed("T", A, 1, 3))]      # ops 0..7: "abc"
_LIST1 = [mk("makeList", "L"), link("l", "L"), ins("L", "_head", 1)]                  # ops 0..2

LHAND = {
    # a tombstone before the edited element: the index skips it
    "tombstone_before": (
        _ABC + [ch(A, 2, {}, d(e(A, 2), obj="T")), ch(A, 3, {}, s(e(A, 3), "C", obj="T"))],
        [(0, CREATE, None, []), (1, SET_ROW, None, [1]), (3, INS_, 0, [3]), (5, INS_, 1, [5]), (7, INS_, 2, [7]),
         (8, REM_, 1, []), (9, SET_, 1, [9])]),
    # a delete, then a re-set of the same element: remove, then insert again at the index of that
    # moment (a:3 was typed after a:2 in between and follows it in the order)
    "del_then_reset": (
        [ch(A, 1, {}, mk("makeList", "L"), link("l", "L"), *typed("L", A, 1, 2, value=lambda i: i)),   # ops 0..5
         ch(A, 2, {}, d(e(A, 2), obj="L")),
         ch(A, 3, {}, ins("L", e(A, 2), 3), s(e(A, 3), 3, obj="L")),
         ch(A, 4, {}, s(e(A, 2), "again", obj="L"))],
        [(0, CREATE, None, []), (1, SET_ROW, None, [1]), (3, INS_, 0, [3]), (5, INS_, 1, [5]),
         (6, REM_, 1, []), (8, INS_, 1, [8]), (9, INS_, 1, [9])]),
    # two concurrent dels of one element: the second finds it invisible and emits nothing
    "concurrent_dels": (
        [ch(A, 1, {}, *_LIST1, s(e(A, 1), "x", obj="L")), ch(B, 1, {A: 1}, d(e(A, 1), obj="L")), ch(Cc, 1, {A: 1}, d(e(A, 1), obj="L"))],
        [(0, CREATE, None, []), (1, SET_ROW, None, [1]), (3, INS_, 0, [3]), (4, REM_, 0, [])]),
    # an inc on a counter element is an element set; after the del the element is invisible and an
    # inc on it emits nothing
    "counter_inc_then_invisible": (
        [ch(A, 1, {}, *_LIST1, s(e(A, 1), 10, obj="L", datatype="counter")), ch(B, 1, {A: 1}, inc(e(A, 1), 5, obj="L")),
         ch(A, 2, {}, d(e(A, 1), obj="L")), ch(B, 2, {A: 2}, inc(e(A, 1), 7, obj="L"))],
        [(0, CREATE, None, []), (1, SET_ROW, None, [1]), (3, INS_, 0, [3]), (4, SET_, 0, [3]), (5, REM_, 0, [])]),
    # two actors set one element concurrently: an element set with conflicts, the higher actor first
    "concurrent_sets": (
        [ch(A, 1, {}, *_LIST1, s(e(A, 1), 1, obj="L")), ch(A, 2, {}, s(e(A, 1), 2, obj="L")), ch(B, 1, {A: 1}, s(e(A, 1), 3, obj="L"))],
        [(0, CREATE, None, []), (1, SET_ROW, None, [1]), (3, INS_, 0, [3]), (4, SET_, 0, [4]), (5, SET_, 0, [5, 4])]),
    # two lists in one document: the index counts within the element's own list
    "two_lists": (
        [ch(A, 1, {}, mk("makeList", "L1"), link("p", "L1"), *typed("L1", A, 1, 2, value=lambda i: i),    # ops 0..5
             mk("makeList", "L2"), link("q", "L2"), *typed("L2", A, 3, 1, value=lambda i: "z")),          # ops 6..9
         ch(A, 2, {}, s(e(A, 2), "two", obj="L1"), ins("L2", e(A, 3), 4), s(e(A, 4), "y", obj="L2"))],    # ops 10..12
        [(0, CREATE, None, []), (1, SET_ROW, None, [1]), (3, INS_, 0, [3]), (5, INS_, 1, [5]),
         (6, CREATE, None, []), (7, SET_ROW, None, [7]), (9, INS_, 0, [9]),
         (10, SET_, 1, [10]), (12, INS_, 1, [12])]),
    # three actors insert concurrently at _head and after a:1: siblings go by (elem, actor) descending.
    # The final order is c:2 b:2 a:2 a:1 a:4 c:3 b:3.
    "sibling_order": (
        [ch(A, 1, {}, *_LIST1, s(e(A, 1), "x", obj="L")),                                   # ops 0..3
         ch(A, 2, {}, ins("L", "_head", 2), s(e(A, 2), "a2", obj="L")),                       # 4, 5
         ch(B, 1, {A: 1}, ins("L", "_head", 2), s(e(B, 2), "b2", obj="L")),                   # 6, 7
         ch(Cc, 1, {A: 1}, ins("L", "_head", 2), s(e(Cc, 2), "c2", obj="L")),                 # 8, 9
         ch(B, 2, {}, ins("L", e(A, 1), 3), s(e(B, 3), "b3", obj="L")),                       # 10, 11
         ch(Cc, 2, {}, ins("L", e(A, 1), 3), s(e(Cc, 3), "c3", obj="L")),                     # 12, 13
         ch(A, 3, {}, ins("L", e(A, 1), 4), s(e(A, 4), "a4", obj="L"))],                      # 14, 15
        [(0, CREATE, None, []), (1, SET_ROW, None, [1]), (3, INS_, 0, [3]), (5, INS_, 0, [5]), (7, INS_, 0, [7]), (9, INS_, 0, [9]),
         (11, INS_, 4, [11]), (13, INS_, 4, [13]), (15, INS_, 4, [15])]),
}


# ---- generated boundary documents ---------------------------------------------------------------------
def typed_list(n, per_change=7):
    """a list of n elements typed as one chain (each after the one before: depth n)"""
    ops = typed("L", A, 1, n, value=lambda i: i)
    out = [ch(A, 1, {}, mk("makeList", "L"), link("l", "L"), *ops[:2 * per_change])]
    for k, i in enumerate(range(2 * per_change, len(ops), 2 * per_change)):
        out.append(ch(A, 2 + k, {}, *ops[i:i + 2 * per_change]))
    return out


def prepends(n):
    """n prepends at _head by two actors in turn: one sibling run of n"""
    out = [ch(A, 1, {}, mk("makeText", "T"), link("t", "T"))]
    seq = {A: 1, B: 0}
    for i in range(n):
        a = (A, B)[i % 2]
        seq[a] += 1
        deps = {A: 1} if a == B else {}
        out.append(ch(a, seq[a], deps, ins("T", "_head", 1 + i // 2), s(e(a, 1 + i // 2), i, obj="T")))
    return out


def busy_list(n_assigns, n_elems=9):
    """n_elems elements, then n_assigns assigns on them by three actors: dels, re-sets, concurrent
    sets and counters, several transitions of different elements in one change"""
    out = [ch(A, 1, {}, mk("makeList", "L"), link("l", "L"), *typed("L", A, 1, n_elems, value=lambda i: i))]
    seq, last, k = {A: 1}, {A: 1}, 0
    while k < n_assigns:
        a = (A, B, Cc)[len(out) % 3]
        seq[a] = seq.get(a, 0) + 1
        deps = {x: q for x, q in last.items() if x != a} if len(out) % 4 != 2 else {A: 1}
        ops = []
        for _ in range(min(1 + len(out) % 5, n_assigns - k)):
            el = e(A, 1 + (k * 5) % n_elems)
            if k % 3 == 1:
                ops.append(d(el, obj="L"))
            elif k % 7 == 3:
                ops.append(s(el, k, obj="L", datatype="counter"))
            elif k % 7 == 5:
                ops.append(inc(el, 2, obj="L"))
            else:
                ops.append(s(el, k, obj="L"))
            k += 1
        out.append(ch(a, seq[a], deps, *ops))
        last[a] = seq[a]
    return out


def long_text(n_changes):
    """a text of n_changes one-op changes after its first: every element is inserted up front, the
    changes set and delete them in turn, so that visibility crosses the history tiles"""
    n_el = 12
    out = [ch(A, 1, {}, mk("makeText", "T"), link("t", "T"), *[ins("T", "_head" if i == 0 else e(A, i), i + 1) for i in range(n_el)])]
    for i in range(n_changes - 1):
        el = e(A, 1 + (i * 7) % n_el)
        out.append(ch(A, 2 + i, {}, d(el, obj="T") if i % 5 == 4 else s(el, i, obj="T")))
    return out
