"""Documents the op-diff tests share: hand-written cases (each names the rule it exercises) and
generated boundary documents.  ``sources(docs, S)`` encodes them and returns, per document, the log
(past_ref.Source) and the all_deps rows of ``oracle.merge``."""
import numpy as np

from hypermerge_amd.columnar import encode
import oracle.oracle as O

from kat_cases import A, B, Cc, D, ch, d, inc, ins, link, mk, s
from past_ref import source_of

# three sets of one key in one change, then a concurrent del, then a concurrent inc (ops 0..4):
#   after op 0 (set 1)   [op0]
#   after op 1 (set 2)   [op0, op1] reversed            -> [op1, op0]
#   after op 2 (set 3)   [op1, op0, op2] reversed       -> [op2, op0, op1]
#   after op 3 (B's del) nothing covered, reversed      -> [op1, op0, op2]
#   after op 4 (C's inc) no counter, reversed           -> [op2, op0, op1]
TIE_FLIP = [ch(A, 1, {}, s("x", 1), s("x", 2), s("x", 3)), ch(B, 1, {}, d("x")), ch(Cc, 1, {}, inc("x", 5))]
TIE_FLIP_ORDERS = [[0], [1, 0], [2, 0, 1], [1, 0, 2], [2, 0, 1]]

HAND = {
    # conflicts across three actors, then an overwrite that covers all of them
    "three_actor_conflict_overwrite": [ch(A, 1, {}, s("x", 1)), ch(B, 1, {}, s("x", 2)), ch(Cc, 1, {}, s("x", 3)),
                                       ch(A, 2, {B: 1, Cc: 1}, s("x", 4))],
    # a del giving remove, then a re-set
    "del_then_reset": [ch(A, 1, {}, s("x", 1)), ch(B, 1, {A: 1}, d("x")), ch(A, 2, {B: 1}, s("x", "again"))],
    "tie_flip": TIE_FLIP,
    # an integer counter with an ancestor inc and a concurrent inc, then a float inc turning INT into FLOAT
    "counter_int_float": [ch(A, 1, {}, s("n", 10, datatype="counter")), ch(B, 1, {A: 1}, inc("n", 5)),
                          ch(Cc, 1, {}, inc("n", 100)), ch(A, 2, {B: 1}, inc("n", 0.5))],
    # makeMap / makeTable with link
    "make_link": [ch(A, 1, {}, mk("makeMap", "m1"), link("child", "m1"), s("k", "v", obj="m1")),
                  ch(B, 1, {A: 1}, mk("makeTable", "t1"), link("tab", "t1"), s("row", 7, obj="t1"), link("child", "t1"))],
    # a shuffled arrival with queued and duplicate changes: bbbb:1 waits for aaaa:1, aaaa:1 twice,
    # cccc:1 needs dddd:1 and stays queued
    "shuffled_queued_duplicate": [ch(B, 1, {A: 1}, s("y", 2), s("x", 8)), ch(Cc, 1, {D: 1}, s("q", 9)), ch(A, 1, {}, s("x", 1)),
                                  ch(A, 1, {}, s("x", 1)), ch(A, 2, {B: 1}, s("x", 5), d("y"))],
    # survivors that predate `from`: two concurrent sets early, a concurrent third much later
    "survivors_before_from": [ch(A, 1, {}, s("x", 1)), ch(B, 1, {}, s("x", 2)), ch(A, 2, {}, s("y", 1)), ch(A, 3, {}, s("y", 2)),
                              ch(Cc, 1, {}, s("x", 3)), ch(D, 1, {A: 1}, s("x", 4))],
    # a text document: make + ins + map ops first, element assigns later
    "text": [ch(A, 1, {}, mk("makeText", "T"), link("t", "T"), ins("T", "_head", 1), s("title", "doc")),
             ch(A, 2, {}, s("title", "doc2")),
             ch(A, 3, {}, s(f"{A}:1", "h", obj="T"), ins("T", f"{A}:1", 2), s(f"{A}:2", "i", obj="T")),
             ch(B, 1, {A: 3}, s("title", "doc3"))],
}


def chain_doc(n_changes, ops_per_change=1, n_keys=7, actors=(A, B, Cc)):
    """n_changes changes by a few actors, each depending on everything before it every third change
    (so sets conflict in between), ops_per_change ops over n_keys keys with dels and counters mixed in"""
    out, seq, last = [], {}, {}
    k = 0
    for i in range(n_changes):
        a = actors[i % len(actors)]
        seq[a] = seq.get(a, 0) + 1
        deps = {x: q for x, q in last.items() if x != a} if i % 3 == 0 else {}
        ops = []
        for _ in range(ops_per_change):
            key = f"k{k % n_keys}"
            if k % 11 == 5:
                ops.append(d(key))
            elif k % 7 == 3:
                ops.append(s("cnt", k, datatype="counter"))
            elif k % 7 == 4:
                ops.append(inc("cnt", 1 if k % 2 else 0.25))
            else:
                ops.append(s(key, k))
            k += 1
        out.append(ch(a, seq[a], deps, *ops))
        last[a] = seq[a]
    return out


def one_register_doc(n_assigns):
    """n_assigns assigns on one key: runs of concurrent sets by three actors, a covering set every
    ninth op, two-set changes (ties) and a del now and then"""
    out, seq, last = [], {}, {}
    k = 0
    while k < n_assigns:
        a = (A, B, Cc)[len(out) % 3]
        seq[a] = seq.get(a, 0) + 1
        deps = {x: q for x, q in last.items() if x != a} if len(out) % 9 == 8 else {}
        ops = [d("x")] if len(out) % 13 == 6 else [s("x", k)]
        k += 1
        if len(out) % 5 == 2 and k < n_assigns:
            ops.append(s("x", 1000 + k))
            k += 1
        out.append(ch(a, seq[a], deps, *ops))
        last[a] = seq[a]
    return out


def wide_doc(n_actors=70):
    """n_actors actors set one key concurrently; then the lowest and the highest actor each set it
    again knowing ranks on one side of 64 only"""
    names = [f"w{i:03d}" for i in range(n_actors)]
    out = [ch(a, 1, {}, s("x", i), s(f"own{i % 5}", i)) for i, a in enumerate(names)]
    k = n_actors - 10                      # (70 actors: ranks 60 .. 67, past the first 64 columns)
    out.append(ch(names[0], 2, {a: 1 for a in names[k:k + 8]}, s("x", "low")))
    out.append(ch(names[-1], 2, {a: 1 for a in names[2:10]}, s("x", "high")))
    out.append(ch(names[k + 5], 2, {names[0]: 2}, d("x")))
    return out


def sources(docs, S=8):
    """(batch, oracle results, [(Source, all_deps rows)] per document)"""
    b = encode(docs, S)
    r = O.merge(b)
    assert (r.docs["status"] == 0).all(), r.docs["status"]
    out = []
    for i in range(b.n_docs):
        c0, nc = int(b.docs["change_off"][i]), int(b.docs["n_changes"][i])
        out.append((source_of(b, r.hist, i), np.asarray(r.all_deps).reshape(-1, S)[c0:c0 + nc].copy()))
    return b, r, out
