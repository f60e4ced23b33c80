"""Hand-built documents for tests/test_small_diet_gpu.py and tests/test_small_diet_docs.py: the
smallest shapes at which merge_small_kernel's map launches take another path (the size class's
loop bounds, the fold check's listed-dep count, list ops meeting a launch without the list carve).

Every group is a list of (name, changes, expected oracle status); a group is one launch (one size
class, one set of batch flags), mixed with generated documents by the GPU test."""
import random

from hypermerge_amd.columnar import ROOT_ID

OK, UNKNOWN_OBJECT, DUPLICATE_OBJECT = 0, 2, 3


def uid(i):
    return f"{i:08x}-1111-4000-8000-000000000000"


def S(key, value, obj=ROOT_ID, **kw):
    return dict({"action": "set", "obj": obj, "key": key, "value": value}, **kw)


def C(actor, seq, deps=None, ops=()):
    return {"actor": actor, "seq": seq, "deps": dict(deps or {}), "ops": list(ops)}


def chain(per_change, keys=16, actor="aa"):
    """One actor, consecutive seqs, per_change[i] set ops over `keys` keys of the root map."""
    out, j = [], 0
    for i, n in enumerate(per_change):
        out.append(C(actor, i + 1, {}, [S(f"k{(j + x) % keys}", j + x) for x in range(n)]))
        j += n
    return out


def regs_doc(R, conflict):
    """R registers (distinct root keys), 8 ops per change; optionally a concurrent set on k0."""
    if R == 0:
        return [C("aa", 1), C("aa", 2), C("bb", 1, {"aa": 1})]
    full, rest = divmod(R, 8)
    d = chain([8] * full + ([rest] if rest else []), keys=R)
    if conflict:
        d.append(C("bb", 1, {}, [S("k0", "other")]))
    return d


def objs_doc(O):
    """Root map and O - 1 child maps: made and linked in one change, set in the next."""
    c1 = [op for i in range(1, O) for op in ({"action": "makeMap", "obj": uid(i)},
                                             {"action": "link", "obj": ROOT_ID, "key": f"c{i}", "value": uid(i)})]
    c2 = [S("x", i, obj=uid(i)) for i in range(1, O)] or [S("x", 0)]
    return [C("aa", 1, {}, c1 or [S("y", 1)]), C("aa", 2, {}, c2)]


def dup_make_doc():
    return [C("aa", 1, {}, [{"action": "makeMap", "obj": uid(1)}, {"action": "link", "obj": ROOT_ID, "key": "c", "value": uid(1)}]),
            C("aa", 2, {}, [{"action": "makeMap", "obj": uid(1)}])]


def dep_doc(target, actors=8):
    """A document whose dep table has exactly `target` rows (each change lists other actors' latest)."""
    latest, out, total, i = {}, [], 0, 0
    while total < target or i < actors:
        a = f"a{i % actors}"
        others = [x for x in sorted(latest) if x != a]
        k = min(len(others), target - total)
        out.append(C(a, latest.get(a, 0) + 1, {x: latest[x] for x in others[:k]}, [S(f"k{i % 8}", i)]))
        latest[a] = latest.get(a, 0) + 1
        total += k
        i += 1
    assert total == target and len(out) <= 64
    return out


def fold_doc(kind, k):
    """Author `z` lists k foreign actors f0 < f1 < ... (the fold's key order), one listed dep an
    ancestor of another.  equal: each f_i knows f_{i-1} (nothing is lowered: fold == closure).
    differ: f_{k-2}:1 knows f_{k-1}:2, the later key then sets f_{k-1} back to 1 (fold != closure)."""
    f = [f"f{i}" for i in range(k)]
    ch = []
    if kind == "equal":
        for i in range(k):
            ch.append(C(f[i], 1, {f[i - 1]: 1} if i else {}, [S(f"k{i}", i)]))
    else:
        ch += [C(f[k - 1], 1, {}, [S("k", 0)]), C(f[k - 1], 2, {}, [S("k", 1)])]
        for i in range(k - 2, -1, -1):
            ch.append(C(f[i], 1, {f[i + 1]: 2 if i == k - 2 else 1}, [S(f"k{i}", i)]))
    ch.append(C("z", 1, {x: 1 for x in f}, [S("kz", 9)]))
    return ch


def fold_walk_docs():
    """Three listed deps a < b < c where the ancestor pair is only met at the second, or only at
    the third, listed dep in history order."""
    top_equal = [C("a", 1, {}, [S("k", 1)]), C("b", 1, {}, [S("k", 2)]), C("c", 1, {"a": 1}, [S("k", 3)]),
                 C("z", 1, {"a": 1, "b": 1, "c": 1}, [S("k", 4)])]
    top_differ = [C("c", 1, {}, [S("k", 1)]), C("c", 2, {}, [S("k", 2)]), C("b", 1, {}, [S("k", 3)]),
                  C("a", 1, {"c": 2}, [S("k", 4)]), C("z", 1, {"a": 1, "b": 1, "c": 1}, [S("k", 5)])]
    mid_differ = [C("c", 1, {}, [S("k", 1)]), C("c", 2, {}, [S("k", 2)]), C("a", 1, {"c": 2}, [S("k", 3)]),
                  C("b", 1, {}, [S("k", 4)]), C("z", 1, {"a": 1, "b": 1, "c": 1}, [S("k", 5)])]
    own = [C("z", 1, {}, [S("k", 1)]), C("a", 1, {}, [S("k", 2)]), C("z", 2, {"z": 1, "a": 1}, [S("k", 3)])]
    return [("fold_top_equal", top_equal), ("fold_top_differ", top_differ), ("fold_mid_differ", mid_differ), ("fold_own_actor", own)]


def shuffled_dup(changes, seed):
    r = random.Random(seed)
    out = list(changes)
    r.shuffle(out)
    out.insert(r.randrange(len(out) + 1), dict(out[r.randrange(len(out))]))
    return out


def list_docs():
    mk = [{"action": "makeList", "obj": uid(7)}, {"action": "link", "obj": ROOT_ID, "key": "l", "value": uid(7)},
          {"action": "ins", "obj": uid(7), "key": "_head", "elem": 1}]
    el = S("aa:1", 5, obj=uid(7))
    throw = S("q", 1, obj=uid(99))                       # an object nothing made
    return [("list_ins", [C("aa", 1, {}, mk)], OK),
            ("list_set_elem", [C("aa", 1, {}, mk + [el])], OK),
            ("list_and_throw", [C("aa", 1, {}, mk + [el]), C("aa", 2, {}, [throw])], UNKNOWN_OBJECT),
            ("throw_only", [C("aa", 1, {}, [S("k", 1)]), C("aa", 2, {}, [throw])], UNKNOWN_OBJECT)]


def tie_docs():
    two = [C("aa", 1, {}, [S("k", 1), S("k", 2)]), C("bb", 1, {}, [S("k", 3)])]
    three = [C("aa", 1, {}, [S("k", 1), S("k", 2), S("k", 3)]), C("bb", 1, {}, [S("k", 4), S("j", 5)])]
    return [("tie_even", two, OK), ("tie_odd", three, OK)]


def counter_doc():
    return [C("aa", 1, {}, [S("c", 10, datatype="counter"), S("k", 1)]),
            C("aa", 2, {}, [{"action": "inc", "obj": ROOT_ID, "key": "c", "value": 3}]),
            C("bb", 1, {"aa": 1}, [{"action": "inc", "obj": ROOT_ID, "key": "c", "value": 5}])]


def groups():
    """name -> dict(docs=[(name, changes, status)], instantiation=(opl, class, lists, counters) or None,
    filler=(config, overrides), strides, clear_list_flag)."""
    few = [("regs0", regs_doc(0, False), OK), ("regs1", regs_doc(1, False), OK), ("regs31", regs_doc(31, True), OK),
           ("regs32", regs_doc(32, True), OK), ("objs1", objs_doc(1), OK), ("ops64", chain([8] * 8), OK),
           ("ops65", chain([8] * 7 + [9]), OK), ("ops128", chain([8] * 16), OK), ("ops_0_1_9", chain([0, 1, 9]), OK),
           ("last_change_empty", chain([3, 0]), OK)] + tie_docs()
    fold = [(f"fold_{kind}{k}", fold_doc(kind, k), OK) for kind in ("equal", "differ") for k in (2, 3, 5)]
    fold += [(n, d, OK) for n, d in fold_walk_docs()]
    fold += [(n + "_shuffled_dup", shuffled_dup(d, i), OK) for i, (n, d, _) in enumerate(list(fold))]
    wide = [("objs2", objs_doc(2), OK), ("objs16", objs_doc(16), OK), ("dup_make", dup_make_doc(), DUPLICATE_OBJECT)] + \
           [(f"deps{t}", dep_doc(t), OK) for t in (0, 64, 65, 128)] + fold
    four = {"config": "C4", "over": {"actors": 4, "changes_per_actor": 16}}
    eight = {"config": "C4", "over": {}}
    return {
        "class0_4actors": dict(docs=few, inst=(2, 0, 0, 0), filler=four, strides=(4, 5, 8, 16)),
        "class0_8actors": dict(docs=wide, inst=(2, 0, 0, 0), filler=eight, strides=(8, 16)),
        "class2": dict(docs=[(f"regs{r}", regs_doc(r, False), OK) for r in (33, 64, 65, 128)], inst=(2, 2, 0, 0),
                       filler=eight, strides=(8,)),
        "class1": dict(docs=[("regs129", regs_doc(129, False), OK)], inst=None, cls=1, filler=eight, strides=(8,)),
        "nolist": dict(docs=list_docs(), inst=(2, 0, 0, 0), filler=eight, strides=(8,), clear_list_flag=True,
                       deferred=("list_ins", "list_set_elem", "list_and_throw"), kept=("throw_only",)),
        "counter": dict(docs=[("counter", counter_doc(), OK)], inst=(2, 0, 0, 1), filler=eight, strides=(8,)),
    }
