"""Documents on both sides of every run-time size comparison of the general merge kernel
(hypermerge_amd/csrc/merge_large.hip), and a restatement of that kernel's size arithmetic.

The kernel places every table of a document by comparisons against its LDS arena of LARENA words,
taken at run time.  ``route`` follows one document through them, from nothing but the document's
shape (Shape: row counts, table size, what its ops hold), and returns

* the comparisons the kernel evaluates on that document's way, each with its outcome, and
* the slots of the check build's path census (hm_large_path in csrc/merge_kernels.h, SLOTS here)
  that one merge of the document alone moves.

``pairs()`` gives, for each comparison, two documents of the same make-up: one where the comparison
holds with nothing to spare (or as close as one generator step allows: one change, op, insert,
assign, object or actor) and one a single step past it.  The edges are found by bisection over the
restated arithmetic, not written down, so a pair follows the arithmetic if a constant moves.
tests/test_general_edges.py pins shapes, sides and the oracle's status without a GPU;
tests/test_general_edges_gpu.py merges them and reads the census.

Comparisons no document reaches (the arithmetic, in the kernel's names):

* ``n * AS + T > stage_base`` (merge_doc_res).  Behind the dispatcher's gate 8n + 2·n_deps <=
  LARENA/4 = 9600, so n <= 1200, A <= 8 (AS <= 9), and T <= 4n + 64 by the clause before it:
  n·AS + T + 8n + 2·n_deps <= 13·1200 + 64 + 9600 = 25264 < LARENA - 1.  The other clause of that
  exit, T > 4n + 64 (sparse seqs), is reachable, but the pool path then reports the document
  UNSUPPORTED where the oracle merges it: an envelope document, not an edge document (none here).
* ``ltab`` with A <= 8: n·A + T + 8n + 2·n_deps <= 8n + (4n + 64) + 9600 <= 24064.  The ltab pair
  has 128 actors (two closure buffers).
* ``E < 0xFFFF`` (tour_lds) is implied by E <= LARENA = 38400 < 65535.
* ``NP >= 32767`` and ``n >= 65536`` inside l34_res: the dispatcher's gate has refused both; the
  gate's own R + O < 32767 is the ``links`` pair.  (Past the gate tail >= 8·NP anyway.)
* malformed rows (RES_OUT_ROWS) are envelope cases (kat_cases.ENVELOPE_CASES), not edge documents.
"""
from collections import Counter
from dataclasses import dataclass
from functools import lru_cache
from typing import Callable, Dict, List, Tuple

import numpy as np

from kat_cases import A as ACT, B as ACT_B, Cc as ACT_C
from kat_cases import ch, ins, link, mk, s

LARENA, LA_MAX, SEG_SHORT, RES_SEG_MAX = 38400, 64, 8, 64
MAKE_LIST, MAKE_TEXT, INS, SET, INC = 2, 3, 4, 5, 8
DT_COUNTER = 1

# hm_large_path (csrc/merge_kernels.h), in order; test_general_edges.py compares the two
SLOTS = ["GATE_PASSED", "GATE_REFUSED",
         "RES_OUT_ROWS", "RES_OUT_TABLE", "RES_OUT_NOT_READY", "RES_OUT_FOLD", "RES_OUT_TAIL", "RES_OUT_COUNTERS",
         "RES_OUT_LONG_LIST", "RES_OUT_TOUR", "RES_OUT_LATE", "RES_DONE",
         "STAGED", "STAGED_NO", "LTAB", "LTAB_NO", "CLOSURE_LDS", "CLOSURE_LDS_NO", "L3", "L3_NO", "LOP", "LOP_NO",
         "OBJ_LDS", "OBJ_LDS_NO", "TOUR_LDS", "TOUR_LDS_NO", "SCRATCH_REUSED", "SCRATCH_CARVED",
         "HIST_FAST", "HIST_PARALLEL", "HIST_SERIAL", "REG_SHORT", "REG_LONG", "POOL_DONE"]
RES_EXITS = [x for x in SLOTS if x.startswith("RES_OUT_")]
YES_NO = [(x, x + "_NO") for x in SLOTS if x + "_NO" in SLOTS] + [("SCRATCH_REUSED", "SCRATCH_CARVED")]
# exits no document that merges normally takes (module docstring)
UNREACHED_EXITS = ("RES_OUT_ROWS", "RES_OUT_TABLE")


def cdiv(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Shape:
    """What the kernel's comparisons read of one document (every change applied, none twice)."""
    n: int                  # changes
    nd: int                 # listed dep rows
    A: int                  # actors
    m: int                  # ops
    R: int                  # registers
    O: int                  # objects (the root included)
    T: int                  # first-arrival table: sum over actors of (max seq - min seq + 1)
    N: int = 0              # insert ops
    nl: int = 0             # list and text objects
    lists: bool = False     # an insert, or an assign on a list or text object
    short_regs: int = 0     # registers with 1..SEG_SHORT assigns (set / del / link / inc)
    long_regs: int = 0      # ... with more
    max_assign: int = 0
    counters: bool = False  # an inc op or a counter datatype
    ready: bool = True      # every change's deps and predecessor arrive before it
    fold: bool = False      # a listed dep dominated by another: the literal fold lowers an entry
    late: bool = False      # an insert after an element inserted later


def staging_words(n, nd):
    return 8 * n + 2 * nd               # change rows (6n), dep rows (2 nd), hist (n), h2a (n)


def stage_base(n, nd):
    return (LARENA - staging_words(n, nd)) & ~1


def res_layout(sh: Shape) -> Tuple[int, int]:
    """(dead_end, tail) of l34_res's layout, in words from the arena's start"""
    n, m, R, NP, AS = sh.n, sh.m, sh.R, sh.R + sh.O, sh.A | 1
    off = sh.T + n * AS + 6 * n                                   # L1 table, closure rows, six per-change words
    off += m + 3 * cdiv(m, 2) + m // 32 + 1                       # o_w; o_chg, a_k, s_list (16 bit); s_bits
    dead_end = off
    off += 5 * R + cdiv(R, 4) + cdiv(R, 2)                        # r_ins .. r_soff; r_obj (8 bit); r_node
    off += cdiv(m, 2)                                             # s_op
    off += 5 * cdiv(R, 2) + R + cdiv(R, 4)                        # n_pi .. n_op; n_key; n_list
    off += 2 * NP + cdiv(NP, 2)                                   # p_cnt, p_off; p_fc
    return dead_end, off


def l2words(sh: Shape):
    return (sh.n * sh.A if sh.A <= 8 else 2 * sh.n * sh.A) + sh.T


def l3_words(sh: Shape):
    return sh.n * (sh.A + 5) + (sh.m + 1) // 2


def tour_entries(sh: Shape):
    return 2 * (sh.N + sh.nl)           # E


def route(sh: Shape, alone=True) -> Tuple[Dict[str, bool], Counter]:
    """(comparisons evaluated on this document's way -> outcome, census slots one merge moves)"""
    dec: Dict[str, bool] = {}
    cen: Counter = Counter()
    n, nd, A, m, R, O, T = sh.n, sh.nd, sh.A, sh.m, sh.R, sh.O, sh.T
    assert n >= 1 and O >= 1 and T <= 4 * n + 64 and R <= 1 << 20 and n < 65536
    dec["actors"] = A <= 8
    dec["objects"] = O <= LA_MAX
    dec["ops"] = m < 65536
    dec["links"] = R + O < 32767
    dec["staging"] = staging_words(n, nd) <= LARENA // 4
    if all(dec.values()):
        cen["GATE_PASSED"] += 1
        sb = stage_base(n, nd)
        dead_end, tail = res_layout(sh)
        dec["res_table"] = n * (A | 1) + T <= sb
        dec["ready"] = sh.ready
        Nn = min(sh.N, R)
        if not dec["res_table"]:
            out = "RES_OUT_TABLE"
        elif not sh.ready:
            out = "RES_OUT_NOT_READY"
        else:
            dec["fold_same"] = not sh.fold
            if sh.fold:
                out = "RES_OUT_FOLD"
            else:
                dec["res_tail"] = tail <= sb
                if not dec["res_tail"]:
                    out = "RES_OUT_TAIL"
                else:
                    dec["no_counters"] = not sh.counters
                    dec["res_seg_max"] = sh.max_assign <= RES_SEG_MAX
                    dec["res_tour"] = 2 * (Nn + O) + Nn <= dead_end
                    if sh.counters:
                        out = "RES_OUT_COUNTERS"
                    elif not dec["res_seg_max"]:
                        out = "RES_OUT_LONG_LIST"
                    elif not dec["res_tour"]:
                        out = "RES_OUT_TOUR"
                    else:
                        dec["in_order"] = not sh.late
                        out = "RES_OUT_LATE" if sh.late else "RES_DONE"
        cen[out] += 1
        if out == "RES_DONE":
            return dec, cen
    else:
        cen["GATE_REFUSED"] += 1
    # ---- the pool path (merge_doc_large), from the start ----
    staged = dec["staging"]
    cen["STAGED" if staged else "STAGED_NO"] += 1
    if alone:
        cen["SCRATCH_CARVED"] += 1      # a workgroup's first pool document of a launch
    if staged:
        dec["ltab"] = l2words(sh) <= stage_base(n, nd)
        ltab = closure = dec["ltab"]
    else:
        ltab = False
        dec["closure_lds"] = closure = l2words(sh) <= LARENA
    cen["LTAB" if ltab else "LTAB_NO"] += 1
    cen["HIST_FAST" if sh.ready else "HIST_PARALLEL"] += 1      # (no duplicates here: never the serial emulation)
    cen["CLOSURE_LDS" if closure else "CLOSURE_LDS_NO"] += 1
    dec["l3"] = l3_words(sh) <= LARENA
    lop = False
    if dec["l3"]:
        dec["lop"] = lop = O < 255 and l3_words(sh) + m <= LARENA
    cen["L3" if dec["l3"] else "L3_NO"] += 1
    cen["LOP" if lop else "LOP_NO"] += 1
    cen["OBJ_LDS" if dec["objects"] else "OBJ_LDS_NO"] += 1
    dec["seg_short"] = sh.long_regs == 0
    if sh.short_regs:
        cen["REG_SHORT"] += sh.short_regs
    if sh.long_regs:
        cen["REG_LONG"] += sh.long_regs
    if sh.lists:
        E = tour_entries(sh)
        dec["tour_lds"] = E <= LARENA and E < 0xFFFF
        cen["TOUR_LDS" if dec["tour_lds"] else "TOUR_LDS_NO"] += 1
    cen["POOL_DONE"] += 1
    return dec, cen


def shape_of(b, d, fold=False, late=False) -> Shape:
    """Shape of document d of an encoded batch (fold and late are what the generator built in)."""
    doc = b.docs[d]
    n, m, R, O = int(doc["n_changes"]), int(doc["n_ops"]), int(doc["n_regs"]), int(doc["n_objs"])
    chs = b.changes[int(doc["change_off"]): int(doc["change_off"]) + n]
    deps = b.deps[int(doc["dep_off"]): int(doc["dep_off"]) + int(doc["n_deps"])]
    ops = b.ops[int(doc["op_off"]): int(doc["op_off"]) + m]
    act, seq = chs["actor"].astype(np.int64), chs["seq"].astype(np.int64)
    T = sum(int(seq[act == a].max() - seq[act == a].min() + 1) for a in np.unique(act))
    seen, ready, dp = set(), True, 0
    for a, q, k in zip(act.tolist(), seq.tolist(), chs["n_deps"].tolist()):
        need = [(int(deps["actor"][dp + j]), int(deps["seq"][dp + j])) for j in range(k)]
        dp += k
        ready &= (q == 1 or (a, q - 1) in seen) and all(x in seen for x in need if x[0] != a and x[1])
        assert (a, q) not in seen
        seen.add((a, q))
    action = ops["action"]
    otype = np.zeros(O, np.int64)
    makes = action < INS
    otype[ops["obj"][makes]] = action[makes]
    is_list = (otype == MAKE_LIST) | (otype == MAKE_TEXT)
    assign = (action >= SET) & (action <= INC)
    cnt = np.bincount(ops["reg"][assign], minlength=R)
    N = int((action == INS).sum())
    return Shape(n=n, nd=int(doc["n_deps"]), A=int(doc["n_actors"]), m=m, R=R, O=O, T=T, N=N, nl=int(is_list.sum()),
                 lists=bool(N or is_list[ops["obj"][assign]].any()),
                 short_regs=int(((cnt >= 1) & (cnt <= SEG_SHORT)).sum()), long_regs=int((cnt > SEG_SHORT).sum()),
                 max_assign=int(cnt.max()) if R else 0,
                 counters=bool(((action == INC) | (ops["datatype"] == DT_COUNTER)).any()),
                 ready=ready, fold=fold, late=late)


# ---------------------------------------------------------------------------------------------
# generators (one step = one unit of the family's parameter) and their shapes in closed form
# ---------------------------------------------------------------------------------------------
def chain(n, m, K):
    """One actor, n changes in order, no listed deps (n_deps = 0, T = n); m set ops spread evenly,
    op j on key j mod K (min(K, m) registers, ceil(m / K) assigns on the fullest)."""
    out, j = [], 0
    for i in range(n):
        k = m // n + (1 if i < m % n else 0)
        out.append(ch(ACT, i + 1, {}, *[s(f"k{(j + x) % K}", j + x) for x in range(k)]))
        j += k
    return out


def chain_shape(n, m, K):
    R = min(K, m)
    full, rest = divmod(m, K) if m >= K else (1, 0)
    per = [full + 1] * rest + [full] * (R - rest)
    return Shape(n=n, nd=0, A=1, m=m, R=R, O=1, T=n, short_regs=sum(1 for x in per if x <= SEG_SHORT),
                 long_regs=sum(1 for x in per if x > SEG_SHORT), max_assign=max(per))


def text(n, N):
    """One actor, n changes; the first makes a text and links it, then N inserts spread evenly,
    each after the one before: m = N + 2, R = N + 1, O = 2, never an assign on an element."""
    out, e = [], 0
    for i in range(n):
        k = N // n + (1 if i < N % n else 0)
        ops = [mk("makeText", "T"), link("t", "T")] if i == 0 else []
        for _ in range(k):
            e += 1
            ops.append(ins("T", "_head" if e == 1 else f"{ACT}:{e - 1}", e))
        out.append(ch(ACT, i + 1, {}, *ops))
    return out


def text_shape(n, N):
    return Shape(n=n, nd=0, A=1, m=N + 2, R=N + 1, O=2, T=n, N=N, nl=1, lists=N > 0, short_regs=1, max_assign=1)


def actor(i):
    return f"a{i:03d}"


def round_robin(A, n, K):
    """A actors, n changes dealt round robin (change j: actor j mod A, its next seq), no listed
    deps, one set each on key j mod K: T = n, every actor's changes concurrent with the others'."""
    return [ch(actor(j % A), j // A + 1, {}, s(f"k{j % K}", j)) for j in range(n)]


def round_robin_shape(A, n, K):
    c = chain_shape(n, n, K)
    return Shape(n=n, nd=0, A=min(A, n), m=n, R=c.R, O=1, T=n, short_regs=c.short_regs, long_regs=c.long_regs,
                 max_assign=c.max_assign)


def objects(k):
    """one change that makes k maps and links each from the root: O = k + 1"""
    return [ch(ACT, 1, {}, *[op for i in range(k) for op in (mk("makeMap", f"o{i}"), link(f"l{i}", f"o{i}"))])]


def objects_shape(k):
    return Shape(n=1, nd=0, A=1, m=2 * k, R=k, O=k + 1, T=1, short_regs=k, max_assign=1 if k else 0)


def nine_on_a_key(k):
    """Nine actors, one change each; the first k set "k", the others "j"; every odd one has seen
    the one before it (so it overwrites that one, and is concurrent with the rest)."""
    return [ch(actor(i), 1, {actor(i - 1): 1} if i % 2 else {}, s("k" if i < k else "j", i)) for i in range(9)]


def edge(pred: Callable[[int], bool], lo: int, hi: int) -> int:
    """the largest x in [lo, hi) with pred(x), pred true at lo, false at hi, monotone between"""
    assert pred(lo) and not pred(hi), (lo, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


def holds(shape_fn, key):
    return lambda x: route(shape_fn(x))[0].get(key, False)


@dataclass
class EdgePair:
    name: str
    comparison: str                     # the key of route()'s comparisons the pair straddles
    slots: Tuple[str, str]              # the census slot each side moves and the other does not
    docs: Tuple[list, list]             # (the comparison holds, one step past it)
    step: str                           # change / op / insert / assign / object / actor: one more of it;
                                        # order / dep: the same rows, two ops or arrivals swapped / one dep's seq lowered
    what: str
    moves_with: Tuple[str, ...] = ()    # comparisons that cannot but flip with it
    fold: Tuple[bool, bool] = (False, False)
    late: Tuple[bool, bool] = (False, False)
    list_hint: bool = True              # False: HM_DOC_HAS_LISTS cleared on both documents


@lru_cache(maxsize=None)
def pairs() -> List[EdgePair]:
    P: List[EdgePair] = []

    def add(name, comparison, slots, lo_hi, step, what, **kw):
        P.append(EdgePair(name, comparison, slots, lo_hi, step, what, **kw))

    # ---- the dispatcher's gate ----
    x = edge(holds(lambda n: chain_shape(n, n, 256), "staging"), 64, 4000)
    add("staging", "staging", ("GATE_PASSED", "GATE_REFUSED"), (chain(x, x, 256), chain(x + 1, x + 1, 256)), "change",
        f"chain of {x} / {x + 1} changes, one set each on 256 keys: 8n = LARENA/4; past it the pool path, rows in HBM")
    add("actors", "actors", ("GATE_PASSED", "GATE_REFUSED"), (round_robin(8, 8, 8), round_robin(9, 9, 9)), "actor",
        "8 / 9 actors, one concurrent change each")
    x = edge(holds(objects_shape, "objects"), 1, 200)
    add("objects", "objects", ("GATE_PASSED", "OBJ_LDS_NO"), (objects(x), objects(x + 1)), "object",
        f"one change making and linking {x} / {x + 1} maps: O = LA_MAX / LA_MAX + 1 with the root")
    x = edge(holds(lambda m: chain_shape(512, m, 2048), "ops"), 60000, 70000)
    add("ops", "ops", ("GATE_PASSED", "GATE_REFUSED"), (chain(512, x, 2048), chain(512, x + 1, 2048)), "op",
        f"chain of 512 changes with {x} / {x + 1} sets on 2048 keys: 16-bit op indices")
    x = edge(holds(lambda m: chain_shape(8, m, m), "links"), 30000, 40000)
    add("links", "links", ("GATE_PASSED", "GATE_REFUSED"), (chain(8, x, x), chain(8, x + 1, x + 1)), "op",
        f"chain of 8 changes with {x} / {x + 1} sets, each on a key of its own: R + O = 32766 / 32767")
    # ---- the all-LDS path's exits ----
    x = edge(holds(lambda m: chain_shape(8, m, m), "res_tail"), 100, 10000)
    add("res_tail", "res_tail", ("RES_DONE", "RES_OUT_TAIL"), (chain(8, x, x), chain(8, x + 1, x + 1)), "op",
        f"chain of 8 changes with {x} / {x + 1} sets, each on a key of its own: tail against stage_base")
    x = edge(holds(lambda N: text_shape(16, N), "res_tour"), 16, 5000)
    for hint in (True, False):
        add("res_tour" + ("" if hint else "_nohint"), "res_tour", ("RES_DONE", "RES_OUT_TOUR"), (text(16, x), text(16, x + 1)),
            "insert", f"text of {x} / {x + 1} inserts in 16 changes, no assigns: 3N + 2·O against dead_end", list_hint=hint)
    add("res_seg_max", "res_seg_max", ("RES_DONE", "RES_OUT_LONG_LIST"), (chain(64, 64, 1), chain(65, 65, 1)), "assign",
        "chain of 64 / 65 changes setting one key: RES_SEG_MAX assigns on a register", moves_with=("seg_short",))
    add("counter", "no_counters", ("RES_DONE", "RES_OUT_COUNTERS"),
        ([ch(ACT, 1, {}, s("c", 1), s("x", 1)), ch(ACT, 2, {}, s("x", 2))],
         [ch(ACT, 1, {}, s("c", 1), s("x", 1)), ch(ACT, 2, {}, s("x", 2), s("n", 3, datatype="counter"))]), "op",
        "two changes; the second document's last op sets a counter")
    t0 = ch(ACT, 1, {}, mk("makeText", "T"), link("t", "T"), ins("T", "_head", 1))
    add("late", "in_order", ("RES_DONE", "RES_OUT_LATE"),
        ([t0, ch(ACT, 2, {}, ins("T", f"{ACT}:1", 3), ins("T", f"{ACT}:3", 2))],
         [t0, ch(ACT, 2, {}, ins("T", f"{ACT}:3", 2), ins("T", f"{ACT}:1", 3))]), "order",
        "a text of three elements; the second document inserts element 2 after element 3, one op before 3 itself",
        late=(False, True))
    f0 = [ch(ACT_B, 1, {}, s("b", 1)), ch(ACT_B, 2, {}, s("b", 2)), ch(ACT, 1, {ACT_B: 2}, s("a", 1))]
    add("fold", "fold_same", ("RES_DONE", "RES_OUT_FOLD"),
        (f0 + [ch(ACT_C, 1, {ACT: 1, ACT_B: 2}, s("c", 1))], f0 + [ch(ACT_C, 1, {ACT: 1, ACT_B: 1}, s("c", 1))]), "dep",
        "the last change lists (A, 1), which has seen (B, 2), and then (B, 2) / (B, 1): the literal fold ends at B = 1",
        fold=(False, True))
    c3 = [ch(ACT, i + 1, {}, s("x", i)) for i in range(3)]
    add("queued", "ready", ("RES_DONE", "RES_OUT_NOT_READY"), (c3, [c3[0], c3[2], c3[1]]), "order",
        "a chain of three changes in order / the third before the second: one queued change")
    # ---- the pool path ----
    add("seg_short", "seg_short", ("REG_SHORT", "REG_LONG"), (nine_on_a_key(8), nine_on_a_key(9)), "assign",
        "nine actors, one set each: SEG_SHORT / SEG_SHORT + 1 of them on one key (the pool path: nine actors)")
    x = edge(holds(lambda n: round_robin_shape(128, n, 64), "ltab"), 128, 1000)
    add("ltab", "ltab", ("LTAB", "LTAB_NO"), (round_robin(128, x, 64), round_robin(128, x + 1, 64)), "change",
        f"128 actors, {x} / {x + 1} changes round robin: 2·n·A + T against stage_base; the closure rounds follow ltab")
    x = edge(holds(lambda n: chain_shape(n, n, 4096), "closure_lds"), 2000, 30000)
    add("closure_lds", "closure_lds", ("CLOSURE_LDS", "CLOSURE_LDS_NO"), (chain(x, x, 4096), chain(x + 1, x + 1, 4096)), "change",
        f"chain of {x} / {x + 1} changes, one set each on 4096 keys: n·A + T = LARENA (rows in place)")
    x = edge(holds(lambda n: round_robin_shape(9, n, 512), "closure_lds"), 1300, 4000)
    add("closure_lds_a9", "closure_lds", ("CLOSURE_LDS", "CLOSURE_LDS_NO"), (round_robin(9, x, 512), round_robin(9, x + 1, 512)),
        "change", f"9 actors, {x} / {x + 1} changes round robin: 2·n·A + T against LARENA (two row buffers)")
    x = edge(holds(lambda m: chain_shape(5400, m, 1024), "l3"), 5400, 40000)
    add("l3", "l3", ("L3", "L3_NO"), (chain(5400, x, 1024), chain(5400, x + 1, 1024)), "op",
        f"chain of 5400 changes with {x} / {x + 1} sets on 1024 keys: n·(A + 5) + ceil(m / 2) = LARENA")
    x = edge(holds(lambda m: chain_shape(5000, m, 1024), "lop"), 5000, 20000)
    add("lop", "lop", ("LOP", "LOP_NO"), (chain(5000, x, 1024), chain(5000, x + 1, 1024)), "op",
        f"chain of 5000 changes with {x} / {x + 1} sets on 1024 keys: l3_words + m = LARENA")
    x = edge(holds(lambda N: text_shape(4, N), "tour_lds"), 10000, 30000)
    for hint in (True, False):
        add("tour_lds" + ("" if hint else "_nohint"), "tour_lds", ("TOUR_LDS", "TOUR_LDS_NO"), (text(4, x), text(4, x + 1)),
            "insert", f"text of {x} / {x + 1} inserts in 4 changes: E = 2·(N + 1) = LARENA", list_hint=hint)
    return P


def encode_pair(p: EdgePair):
    """the pair's two documents as one batch (its list hint cleared where the pair says so)"""
    from hypermerge_amd.columnar import encode
    return clear_hint(encode(list(p.docs)), range(2) if not p.list_hint else ())


def clear_hint(b, rows):
    for d in rows:
        b.docs["flags"][d] &= ~np.uint16(1)
    return b


def pair_shapes(p: EdgePair, b, first=0):
    return tuple(shape_of(b, first + i, fold=p.fold[i], late=p.late[i]) for i in range(2))
