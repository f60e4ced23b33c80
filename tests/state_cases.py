"""Hand-written documents for the state calls (test input only): each with the rows the contract of
tests/state_ref.py gives, written out by hand as (object, key or elemId, index, [value, ...]) with the
winner first; an object is named by the id its make op gave it ("" = ROOT), a linked object's value
is that id."""
from hypermerge_amd.columnar import ROOT_ID

from kat_cases import A, B, Cc, ch, d, inc, ins, link, mk, s

R = ""

KNOWN = {
    "empty": ([], []),
    # the dead register between two live ones is skipped, the ids stay the document's own
    "deleted_key_between": ([ch(A, 1, {}, s("a", 1), s("b", 2), s("c", 3)), ch(A, 2, {}, d("b"))],
                            [(R, "a", -1, [1]), (R, "c", -1, [3])]),
    # the higher actor wins, the other is the conflict
    "two_writer_conflict": ([ch(A, 1, {}, s("x", 1)), ch(B, 1, {}, s("x", 2))], [(R, "x", -1, [2, 1])]),
    # 10 + 5 - 2 as an INT; the concurrent inc does not count
    "counter_later_inc": ([ch(A, 1, {}, s("n", 10, datatype="counter")), ch(B, 1, {A: 1}, inc("n", 5)),
                           ch(A, 2, {B: 1}, inc("n", -2)), ch(Cc, 1, {}, inc("n", 100))], [(R, "n", -1, [13])]),
    # ... and a non-integral inc turns it into a FLOAT
    "counter_float": ([ch(A, 1, {}, s("n", 1, datatype="counter")), ch(A, 2, {}, inc("n", 2)), ch(B, 1, {A: 2}, inc("n", 0.5))],
                      [(R, "n", -1, [3.5])]),
    # the deleted element has no row and the indices stay dense
    "text_deleted_element": ([ch(A, 1, {}, mk("makeText", "T"), link("t", "T"),
                                 ins("T", "_head", 1), s(f"{A}:1", "h", obj="T"),
                                 ins("T", f"{A}:1", 2), s(f"{A}:2", "i", obj="T"),
                                 ins("T", f"{A}:2", 3), s(f"{A}:3", "!", obj="T")),
                              ch(A, 2, {}, d(f"{A}:2", obj="T"))],
                             [(R, "t", -1, ["T"]), ("T", f"{A}:1", 0, ["h"]), ("T", f"{A}:3", 1, ["!"])]),
    # an element inserted and never assigned (an inc on it changes nothing)
    "element_never_assigned": ([ch(A, 1, {}, mk("makeList", "L"), link("l", "L"), ins("L", "_head", 1),
                                   ins("L", f"{A}:1", 2), s(f"{A}:2", "x", obj="L"), inc(f"{A}:1", 3, obj="L"))],
                               [(R, "l", -1, ["L"]), ("L", f"{A}:2", 0, ["x"])]),
    # elements never attached to _head (a missing parent, a cycle of inserts) hold nothing
    "detached_element": ([ch(A, 1, {}, mk("makeList", "L"), link("l", "L"),
                             ins("L", "zzzz:9", 1), ins("L", f"{A}:3", 2), ins("L", f"{A}:2", 3),
                             ins("L", "_head", 4), s(f"{A}:4", "v", obj="L"), d(f"{A}:1", obj="L"))],
                         [(R, "l", -1, ["L"]), ("L", f"{A}:4", 0, ["v"])]),
    # two lists and a nested map: the rows come in register order, whatever object they belong to
    "two_lists_nested_map": ([ch(A, 1, {}, mk("makeList", "L1"), link("one", "L1"), ins("L1", "_head", 1), s(f"{A}:1", 1, obj="L1"),
                                 mk("makeMap", "M"), link("m", "M"), s("k", "v", obj="M"),
                                 mk("makeList", "L2"), link("two", "L2"), ins("L2", "_head", 2), s(f"{A}:2", 2, obj="L2")),
                              ch(B, 1, {A: 1}, ins("L1", "_head", 1), s(f"{B}:1", 0, obj="L1"), s("k2", True, obj="M"),
                                 ins("L2", f"{A}:2", 3), s(f"{B}:3", 3, obj="L2"))],
                             [(R, "one", -1, ["L1"]), ("L1", f"{A}:1", 1, [1]), (R, "m", -1, ["M"]), ("M", "k", -1, ["v"]),
                              (R, "two", -1, ["L2"]), ("L2", f"{A}:2", 0, [2]), ("L1", f"{B}:1", 0, [0]), ("M", "k2", -1, [True]),
                              ("L2", f"{B}:3", 1, [3])]),
    # every key deleted: no rows at all
    "all_deleted": ([ch(A, 1, {}, s("a", 1), s("b", 2)), ch(B, 1, {A: 1}, d("a"), d("b"))], []),
}


def named_rows(b, d_, state):
    """a State's rows in KNOWN's form (document d_ of the encoded batch b)"""
    from hypermerge_amd.columnar import V_OBJ
    from hypermerge_amd.render import _scalar
    objs, regs = b.doc_objs[d_], b.doc_regs[d_]
    name = lambda o: R if objs[o] == ROOT_ID else objs[o]
    val = lambda vt, v: name(int(v)) if vt == V_OBJ else _scalar(b, vt, v)
    return [(name(obj), regs[g][1], idx, [val(vt, v) for _, vt, v in sv]) for g, obj, idx, sv in state.rows]
