"""Rounds on both sides of the run-time limits of the incremental apply passes
(hypermerge_amd/csrc/inc_kernels.hip) and of plan_kernel's route (csrc/store_kernels.hip), and a
restatement of both.

A *round* is one submit of new changes against one resident document (a base log loaded by one
earlier submit into an empty document, which re-merges it and lets inc_meta_kernel build the
incremental state).  ``round_of`` gathers what the comparisons read of it (Round); ``route`` walks the
plan's route, then the checks of the pass that picks the document up, in the kernel's order, and
returns

* the passes that see the document, in order (a defer at strides <= 16 adds WAVE / WAVE_TILED),
* the slots of the check build's exit census (hm_inc_pass x hm_inc_slot in csrc/store_kernels.h,
  PASSES x SLOTS here) that one submit of that document alone moves, counts included, the
  inc_meta_kernel row of a re-merge among them, and
* what DocStore.last_routing() reports for it (incremental / remerged / handed_back).

``pairs()`` gives, per comparison, two rounds of the same make-up, the first satisfying it with
nothing to spare and the second one generator step past it (one change, op, dep, survivor, object,
list, or one row of the base log where the comparison reads the resident state).  The limits
(HM_INC_*, NC, TB, LSV, LKF, META_LCH, the register tails) are read out of the two sources, so a
pair follows a constant that moves.  tests/test_inc_edges.py pins sides and oracle status without
a GPU; tests/test_inc_edges_gpu.py applies the rounds and reads the census.

Survivor counts (a register's list before a tile or before a lane-pass change) are taken from the
oracle's merge of the log up to there: the restatement covers the passes' *decisions*, not
applyAssign.

Comparisons no round reaches through the store (slots in UNREACHABLE, the arithmetic here):

* ``nt >= 2 * G`` (FOLD_STEPS).  A change adds at most one fold step per dep row that names another
  actor plus one for its own predecessor, so nt <= nnd + nnc, and the check before it bounds that by
  G + NC = 16 (G = 8), 24 (G = 16), 72 (G = 64).  The check refuses the step of index 2 G, the
  (2 G + 1)th, so 16 steps at G = 8 pass with nothing to spare (pair fold_steps_g8: 15 / 16 steps, both
  DONE) and no round has a 17th.  The plan's HM_INC_MAX_TGT = 128 is the
  same bound for the wave pass and cannot bind either (a tile holds at most 64 dep rows).
* BAIL_DESC (``nnc == 0 || NA > S || S > G || n_old_r > n_r``): plan_kernel routes a row
  incrementally only with n_changes > 0, n_actors <= S and n_regs covering the document's, and the
  launch picks G >= S.
* BAIL_STATE: plan_kernel reads the same IncState flags first and re-merges (inc = false); the lane
  pass's extra HM_IST_LIST needs a list object, whose document the plan never routes to a lane.
* BAIL_NO_SOURCE: a fold source (actor, seq <= clock[actor]) of a clean document (nothing queued)
  is an applied row of the log.
* DEFER_LIST.  Group passes (HM_INC_LIST_GROUPS = 0): plan_kernel marks the same ops (an object
  that is neither ROOT nor in mapmask) `wave`, route 2, which the G < 64 launches skip.  Lane pass:
  its defers need an ins / makeList / makeText or an op on a list element, all of which put
  HM_DOC_HAS_LISTS on the row or the document, and `lane` requires !lists.  The lane pass's
  header comment ("list ops, a moved segment" deferred) describes exits the plan has closed: a
  moved segment is copied by the lane itself.
* META_NOCKEY and the seq < 2^24 side of bad_c as a *ready* change: causallyReady needs seq ==
  clock + 1, so a seq of 2^24 that applies needs 16,777,215 changes of one actor before it.  The
  not-ready twin is the pair seq_wide (BAIL_ROWS against BAIL_NOT_READY).
* the plan's ``m.n_o + r.n_ops <= HM_INC_SMALL_LIST_OPS`` (mode 1): a list document holds a state
  only when doc_rows_kernel / inc_meta_kernel kept one, m.n_o > 256, so the sum is over the bound
  whenever the plan gets that far; the reachable edge is the state's (pair small_list_state).
* BAIL_LP_DUP (list_plan's scan meets an element of the new one's parent and key): a key is elem << 8 |
  actor rank, ranks are below 64, so an equal key is the same elemId and so the same register.  If
  the round inserted it, the first `bad` fires; if the log did, the merge wrote the list's object
  into that register (valued or not: pairs ins_reg, ins_reg_bare) and BAIL_INS_REG fires first.
* LONG_CHANGES / LONG_OPS / LONG_DEPS at G = 64: inc_group_kernel<64, false> skips every document with
  nnc > NC, nno > 64 or nnd > 64 (the tiled launch's), and inc_doc_tiled cuts tiles that fit.
* BAIL_LP_STALE: epos / lorder disagree only for a register that is no element, which the first
  `bad` (position outside the list) or the oracle's MISSING_ELEM catches first for any op a
  generator can state; kept as a guard.
* BAIL_MAKE_LISTS: the plan re-merges a list document's object creation itself (pair list_make).
* META_LIST_REFUSED (the `bad` / `!ok` exits of inc_meta_kernel's list rebuild): an applied insert of
  elem >= 2^24 never reaches it, because the merge kernels report that document UNSUPPORTED and the
  store rolls the round back (pair elem_wide: status 16 on the far side); an applied insert into an
  object that is no list of the directory, or an element position past the count, needs a log the
  merge itself would have refused.
* n_actors == S + 1: the store refuses the submit on the host (EngineError) before any kernel.
"""
import os
import re
from collections import Counter
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Dict, List, Optional, Tuple

import numpy as np

from kat_cases import ch, d as dl, inc as incr, ins, link, mk, s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypermerge_amd", "csrc")
MAKE_MAP, MAKE_TABLE, MAKE_LIST, MAKE_TEXT, INS, SET, DEL, LINK, INC = range(9)
V_INT, V_FLOAT, DT_COUNTER, HAS_LISTS, NONE = 3, 4, 1, 1, 0xFFFFFFFF
TWO53 = 1 << 53


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


@lru_cache(maxsize=None)
def limits() -> Dict[str, int]:
    """the constants of the two sources, by regex (as test_materialize_gpu.py reads HM_PAST_TILE)"""
    h, k = _src("store_kernels.h"), _src("inc_kernels.hip")
    L = {n: _const(h, rf"#define {n} (\d+)") for n in
         ("HM_INC_MAX_NEW_C", "HM_INC_MAX_NEW_O", "HM_INC_MAX_TGT", "HM_INC_LANE_MAX_C", "HM_INC_LANE_MAX_O",
          "HM_INC_TILED_MAX_C", "HM_INC_TILED_MAX_O", "HM_INC_LISTS", "HM_INC_SMALL_LIST_OPS", "HM_INC_COST")}
    L["NC"] = L["HM_INC_MAX_NEW_C"]
    L["TB"] = _const(k, r"constexpr uint32_t TB = (\d+);")
    L["LSV"] = _const(k, r"constexpr uint32_t LSV = (\d+);")
    L["LKF"] = _const(k, r"constexpr uint32_t LKF = (\d+);")
    L["META_LCH"] = _const(k, r"constexpr uint32_t META_LCH = (\d+);")
    L["KT_ROWS"] = _const(k, r"KT = G >= 32 \? 1u : (\d+)u / G;")       # rows of the log in tk[] at G < 32
    L["LANE_TAIL"] = _const(k, r"uint32_t tail\[(\d+)\];")
    L["SEQ_BITS"] = _const(k, r"cq >= \(1u << (\d+)\)")
    L["MAP_IDS"] = _const(k, r"o_obj == 0 \|\| o_obj >= (\d+) \|\|")
    L["LIST_GROUPS"] = _const(h, r"#define HM_INC_LIST_GROUPS (\d+)")
    return L


PASSES = ["LANE8", "LANE16", "GROUP8", "GROUP16", "WAVE", "WAVE_TILED", "META"]
# hm_inc_slot (csrc/store_kernels.h), in order; test_inc_edges.py compares the two
SLOTS = ["ENTER", "DONE", "LONG_CHANGES", "LONG_OPS", "LONG_DEPS", "FOLD_STEPS", "N_UP", "TOT_OLD", "DEFER_LIST",
         "BAIL_DESC", "BAIL_STATE", "BAIL_ROWS", "BAIL_OP", "BAIL_MAKE", "BAIL_MAKE_LISTS", "BAIL_COUNTER", "BAIL_NOT_READY",
         "BAIL_NO_SOURCE", "BAIL_NO_ROOM", "BAIL_LSV", "BAIL_INS_REG", "BAIL_LP_PARENT", "BAIL_LP_STALE", "BAIL_LP_DUP",
         "BAIL_LP_CLASH", "BAIL_TILE_BIG", "TILE_LATER_FAILED", "TILES", "SRC_TAIL", "SRC_LOOP",
         "META_DIRTY", "META_VALID", "META_VALID_LISTS", "META_NOCKEY", "META_LISTS_OVER", "META_LIST_REFUSED"]
FAILG = ("LONG_CHANGES", "LONG_OPS", "LONG_DEPS", "FOLD_STEPS", "N_UP", "TOT_OLD")     # defer at G < 64, bail at G = 64
EXITS = FAILG + ("DEFER_LIST",) + tuple(x for x in SLOTS if x.startswith("BAIL_"))
EVENTS = ("TILE_LATER_FAILED", "TILES", "SRC_TAIL", "SRC_LOOP", "META_LISTS_OVER", "META_LIST_REFUSED")
META_ENDS = ("META_DIRTY", "META_VALID", "META_VALID_LISTS", "META_NOCKEY")
_COMMON = ("ENTER", "DONE", "BAIL_DESC", "BAIL_STATE", "BAIL_ROWS", "BAIL_OP", "BAIL_MAKE", "BAIL_COUNTER", "BAIL_NOT_READY",
           "BAIL_NO_SOURCE", "BAIL_NO_ROOM", "SRC_TAIL", "SRC_LOOP")
_GROUPS = _COMMON + FAILG + ("BAIL_MAKE_LISTS",)
# the slots each family of passes has a counting site for (LANE8 / 16, GROUP8 / 16, WAVE / WAVE_TILED, META)
FAMILY_SLOTS = {
    "LANE": _COMMON + ("DEFER_LIST", "BAIL_LSV"),
    "GROUP": _GROUPS + ("DEFER_LIST",),
    "WAVE": _GROUPS + ("BAIL_INS_REG", "BAIL_LP_PARENT", "BAIL_LP_STALE", "BAIL_LP_DUP", "BAIL_LP_CLASH", "BAIL_TILE_BIG",
                       "TILE_LATER_FAILED", "TILES"),
    "META": ("ENTER",) + META_ENDS + ("META_LISTS_OVER", "META_LIST_REFUSED"),
}


def family(P):
    return "LANE" if P.startswith("LANE") else "GROUP" if P.startswith("GROUP") else "WAVE" if P.startswith("WAVE") else "META"


# (family, slot) no round reaches through the store, each with its reason in the module docstring
_EVERY = ("LANE", "GROUP", "WAVE")
UNREACHABLE = {(f, x): why for fams, x, why in (
    (("GROUP", "WAVE"), "FOLD_STEPS", "nt <= nnd + nnc <= G + NC <= 2 G, and the step of index 2 G is the first refused"),
    (_EVERY, "BAIL_DESC", "the plan's inc already requires it"),
    (_EVERY, "BAIL_STATE", "the plan reads the same flags first"),
    (_EVERY, "BAIL_NO_SOURCE", "a clean document's fold sources are applied rows"),
    (("LANE", "GROUP"), "DEFER_LIST", "the plan routes list ops to the wave pass and list documents away from the lane pass"),
    (("GROUP", "WAVE"), "BAIL_MAKE_LISTS", "the plan re-merges object creation in a list document"),
    (("WAVE",), "LONG_CHANGES", "the G = 64 launches split on the same comparison: a long round takes tiles, and a tile fits"),
    (("WAVE",), "LONG_OPS", "as LONG_CHANGES"),
    (("WAVE",), "LONG_DEPS", "as LONG_CHANGES"),
    (("WAVE",), "BAIL_LP_STALE", "a guard behind the first `bad`"),
    (("WAVE",), "BAIL_LP_DUP", "an equal key is the same elemId, the same register: BAIL_INS_REG or the first `bad` takes it"),
    (("META",), "META_NOCKEY", "a ready seq of 2^24 needs 2^24 - 1 changes of one actor"),
    (("META",), "META_LIST_REFUSED", "the merge refuses an elem of 2^24 itself (UNSUPPORTED, rolled back); its other causes need a corrupt log"),
) for f in fams}


def cdiv(a, b):
    return -(-a // b)


def grow_rows(x):
    return x if x > 0xC0000000 else x + (x >> 2)


def pow2c(x):
    x = max(x, 16)
    return 1 << (x - 1).bit_length()


def group_of(S):
    return 8 if S <= 8 else 16 if S <= 16 else 64


def tail_rows(G):
    """rows of the log the group pass holds in registers (KT * G)"""
    return G if G >= 32 else (limits()["KT_ROWS"] // G) * G


# ---------------------------------------------------------------------------------------------
# the resident state after a re-merge (what inc_meta_kernel and doc_rows_kernel leave), from the oracle
# ---------------------------------------------------------------------------------------------
@dataclass
class Resident:
    S: int
    n_c: int
    n_d: int
    n_o: int
    n_r: int
    n_objs: int
    n_actors: int
    lists: bool                    # HM_DOC_HAS_LISTS
    clean: bool                    # status OK, nothing queued
    valid: bool                    # IncState.flags & VALID
    nockey: bool
    list_resident: bool            # HM_IST_LIST
    list_objs: Tuple[int, ...]     # the directory (object ids, ascending)
    lists_over: bool
    list_refused: bool
    s_used: Optional[int]
    cabs: int
    mapmask: int
    clock: Tuple[int, ...]
    keys: Tuple[Tuple[int, int, bool], ...]     # the log's (actor, seq, applied), in log order
    reg_surv: Tuple[int, ...]
    caps: Tuple[int, int, int, int]             # c, d, o, r
    in_meta: bool = True           # the re-merge listed it for inc_meta_kernel (not mode 1's small list documents)
    reg_obj: Tuple[int, ...] = ()  # hm_reg_result.obj per register (NONE: untouched)
    lorder: Tuple[int, ...] = ()   # the resident list order: element registers, the directory's lists end to end
    epar: Dict[int, int] = field(default_factory=dict, compare=False)     # element register -> parent register | NONE
    ekey: Dict[int, int] = field(default_factory=dict, compare=False)     # element register -> elem << 8 | actor
    lspan: Dict[int, Tuple[int, int]] = field(default_factory=dict, compare=False)   # list object -> (base, elements)


def list_order(ops, op_actor, applied_op, objs):
    """RGA order of every list in objs (ascending ids), end to end: a parent's children by key
    (elem << 8 | actor) descending, pre-order; (lorder, epar, ekey, {obj: (base, count)})"""
    lorder, epar, ekey, span = [], {}, {}, {}
    for ob in objs:
        kids: Dict[int, list] = {}
        for o, a, ok in zip(ops, op_actor, applied_op):
            if int(o["action"]) == INS and int(o["obj"]) == ob and ok and int(o["reg"]) not in ekey:
                reg, par = int(o["reg"]), int(o["parent"])
                epar[reg], ekey[reg] = par, (int(o["elem"]) << 8) | (int(a) & 0xFF)
                kids.setdefault(par, []).append(reg)
        base, stack = len(lorder), sorted(kids.get(NONE, []), key=lambda x: ekey[x])
        while stack:
            x = stack.pop()
            lorder.append(x)
            stack += sorted(kids.get(x, []), key=lambda y: ekey[y])
        span[ob] = (base, len(lorder) - base)
    return tuple(lorder), epar, ekey, span


def first_caps(n_c, n_d, n_o, n_r):
    return tuple(pow2c(grow_rows(x)) if x > 0 else 0 for x in (n_c, n_d, n_o, n_r))


def resident_of(enc, S, mode, caps=None) -> Resident:
    """the state a re-merge of enc's whole log leaves (enc: a store.DocEncoder holding the log)"""
    import oracle.oracle as O
    b = enc.log_batch(S)
    o = O.merge(b)
    doc, res = b.docs[0], o.docs[0]
    n_c, n_d, n_o, n_r = int(doc["n_changes"]), int(doc["n_deps"]), int(doc["n_ops"]), int(doc["n_regs"])
    ops, chs = b.ops, b.changes
    lists = bool(int(doc["flags"]) & HAS_LISTS)
    clean = int(res["status"]) == 0 and int(res["n_queued"]) == 0
    small = mode == 1 and lists and n_o <= limits()["HM_INC_SMALL_LIST_OPS"] and not (limits()["LIST_GROUPS"] and S <= 16)
    applied = o.hist[:n_c] >= 0
    act = ops["action"]
    lobj = sorted({int(x) for x in ops["obj"][(act == MAKE_LIST) | (act == MAKE_TEXT)]})
    over = len(lobj) > limits()["HM_INC_LISTS"]
    op_chg = np.repeat(np.arange(n_c), chs["n_ops"]) if n_o else np.zeros(0, int)
    ins_ok = all(int(e) < (1 << limits()["SEQ_BITS"]) for e, a, c in zip(ops["elem"], act, op_chg) if a == INS and applied[c])
    list_res = bool(lobj) and not over and ins_ok
    counts = (ops["vtag"] == V_INT) & ((act == INC) | ((act == SET) & (ops["datatype"] == DT_COUNTER)))
    cabs = sum(abs(int(np.int64(np.uint64(v)))) for v in ops["value"][counts])
    mask = 1
    for x in ops["obj"][(act == MAKE_MAP) | (act == MAKE_TABLE)]:
        if int(x) < 64:
            mask |= 1 << int(x)
    valid = clean and not small
    lo, ep, ek, sp = list_order(ops, chs["actor"][op_chg] if n_o else [], applied[op_chg] if n_o else [],
                                lobj[:limits()["HM_INC_LISTS"]]) if valid and list_res else ((), {}, {}, {})
    return Resident(
        reg_obj=tuple(int(x) for x in o.regs["obj"][:n_r]), lorder=lo, epar=ep, ekey=ek, lspan=sp,
        S=S, n_c=n_c, n_d=n_d, n_o=n_o, n_r=n_r, n_objs=int(doc["n_objs"]), n_actors=int(doc["n_actors"]),
        lists=lists, clean=clean, valid=valid, nockey=bool((chs["seq"] >= (1 << limits()["SEQ_BITS"])).any()),
        list_resident=valid and list_res, list_objs=tuple(lobj[:limits()["HM_INC_LISTS"]]), lists_over=over,
        list_refused=bool(lobj) and not over and not ins_ok, s_used=int(res["n_surv"]), cabs=min(cabs, 1 << 62),
        mapmask=mask, clock=tuple(int(x) for x in o.clock[:S]),
        keys=tuple((int(a), int(q), bool(p)) for a, q, p in zip(chs["actor"], chs["seq"], applied)),
        reg_surv=tuple(int(x) for x in o.regs["n_surv"][:n_r]), caps=caps or first_caps(n_c, n_d, n_o, n_r),
        in_meta=not small)


# ---------------------------------------------------------------------------------------------
# one round
# ---------------------------------------------------------------------------------------------
@dataclass
class Round:
    """Everything the comparisons read of one submit against one resident document."""
    S: int                          # the store's stride
    res: Resident                   # resident log size, actors, registers, objects, lists, s_used, caps
    n_actors: int                   # actors after the round
    n_r: int
    n_objs: int
    flags: int                      # the row's document flags
    remapped: bool                  # a new actor sorts before an old one
    changes: np.ndarray             # the new change, dep and op rows (doc-local offsets)
    deps: np.ndarray
    ops: np.ndarray
    o_cap: int                      # the op segment's capacity after the append
    moved: Tuple[bool, bool, bool, bool]        # segments the append moves (c, d, o, r)
    prefix: tuple = field(default=(), repr=False, compare=False)      # (base changes, round changes): later states
    # filled by summary(): fold steps, per touched register (old survivors, pushes), largest change,
    # the distance back of each fold source, counter sum
    nt: int = 0
    touched: Tuple[Tuple[int, int], ...] = ()
    largest: Tuple[int, int] = (0, 0)
    src_back: Tuple[int, ...] = ()
    cabs: int = 0

    @property
    def nnc(self):
        return len(self.changes)

    @property
    def nno(self):
        return len(self.ops)

    @property
    def nnd(self):
        return len(self.deps)


def _encoder(changes):
    from hypermerge_amd.store import DocEncoder, StringPool
    e = DocEncoder(StringPool())
    a = e.encode(changes) if changes else None
    return e, a


@lru_cache(maxsize=None)
def _resident_cached(key, S, mode):
    e, _ = _encoder(list(_LOGS[key]))
    return resident_of(e, S, mode)


_LOGS: Dict[int, tuple] = {}


def resident_after(changes, S, mode) -> Resident:
    """the resident state after `changes` were loaded by one submit into an empty document"""
    import json
    key = hash(json.dumps(changes, sort_keys=True))
    _LOGS[key] = tuple(changes)
    return _resident_cached(key, S, mode)


def round_of(base, new, S, mode) -> Round:
    res = resident_after(base, S, mode)
    e, _ = _encoder(base)
    a = e.encode(new)
    need = (res.n_c + len(a.changes), res.n_d + len(a.deps), res.n_o + len(a.ops), a.n_regs)
    moved = tuple(n > c for n, c in zip(need, res.caps))
    o_cap = pow2c(grow_rows(need[2])) if moved[2] else res.caps[2]
    r = Round(S=S, res=res, n_actors=a.n_actors, n_r=a.n_regs, n_objs=a.n_objs, flags=a.flags, remapped=a.remap is not None,
              changes=a.changes, deps=a.deps, ops=a.ops, o_cap=o_cap, moved=moved, prefix=(tuple(base), tuple(new)))
    return summary(r)


def fold_targets(r: Round, c0=0, c1=None):
    """the fold steps of changes c0 .. c1 - 1 as (change, actor, seq), in the kernels' order: the
    listed deps (one on the change's own actor reads seq - 1), then {actor: seq - 1} unless listed"""
    out = []
    for j in range(c0, len(r.changes) if c1 is None else c1):
        c = r.changes[j]
        a, q, own = int(c["actor"]), int(c["seq"]), False
        for t in range(int(c["n_deps"])):
            dp = r.deps[int(c["dep_off"]) + t]
            da, dq = int(dp["actor"]), int(dp["seq"])
            if da == a:
                dq, own = q - 1, True
            if dq:
                out.append((j, da, dq))
        if not own and q - 1:
            out.append((j, a, q - 1))
    return out


def counter_add(ops):
    act = ops["action"]
    m = (ops["vtag"] == V_INT) & ((act == INC) | ((act == SET) & (ops["datatype"] == DT_COUNTER)))
    return sum(abs(int(np.int64(np.uint64(v)))) for v in ops["value"][m])


def summary(r: Round) -> Round:
    tg = fold_targets(r)
    r.nt = len(tg)
    pos = {(a, q): i for i, (a, q, p) in enumerate(r.res.keys) if p}
    new = {(int(c["actor"]), int(c["seq"])) for c in r.changes}
    r.src_back = tuple(r.res.n_c - pos[(a, q)] for _, a, q in tg if (a, q) not in new and (a, q) in pos)
    seen, touched = set(), []
    for k, o in enumerate(r.ops):
        reg = int(o["reg"])
        if o["action"] >= SET and reg not in seen:
            seen.add(reg)
            push = int(((r.ops["reg"][k:] == reg) & ((r.ops["action"][k:] == SET) | (r.ops["action"][k:] == LINK))).sum())
            touched.append((r.res.reg_surv[reg] if reg < r.res.n_r else 0, push))
    r.touched = tuple(touched)
    if len(r.changes):
        r.largest = (int(r.changes["n_ops"].max()), int(r.changes["n_deps"].max()))
    r.cabs = r.res.cabs + counter_add(r.ops)
    return r


# ---------------------------------------------------------------------------------------------
# the restatement: plan_kernel's route, then the passes
# ---------------------------------------------------------------------------------------------
def plan_route(r: Round, mode: int) -> int:
    """AppendDesc.inc & HM_DINC_ROUTE: 0 re-merge, 1 group pass, 2 wave pass, 3 lane pass"""
    L, m, S = limits(), r.res, r.S
    if not mode or not m.valid:                 # (a store where no document holds a state plans no incremental route)
        return 0
    lists = bool((r.flags | (HAS_LISTS if m.lists else 0)) & HAS_LISTS)
    tgt = r.nnd + r.nnc
    small = r.nnc <= L["HM_INC_MAX_NEW_C"] and r.nno <= L["HM_INC_MAX_NEW_O"] and tgt <= L["HM_INC_MAX_TGT"]
    lane = not small and S in (8, 16) and not lists and r.nnc <= L["HM_INC_LANE_MAX_C"] and r.nno <= L["HM_INC_LANE_MAX_O"]
    longr = lane or (not small and (lists or S not in (8, 16)) and r.nnc <= L["HM_INC_TILED_MAX_C"] and
                     r.nno <= L["HM_INC_TILED_MAX_O"])
    inc = m.clean and not r.remapped and r.nnc > 0 and (small or longr) and r.n_actors <= S
    small_lists = L["HM_INC_SMALL_LIST_OPS"] if mode == 1 and not (L["LIST_GROUPS"] and S <= 16) else 0
    if inc and lists and m.n_o + r.nno <= small_lists:
        inc = False
    wave = False
    if inc:
        if m.nockey:
            inc = False
        elif lists:
            for o in r.ops:
                obj = int(o["obj"])
                other = obj != 0 and (obj >= 64 or not (m.mapmask >> obj) & 1)
                if o["action"] <= MAKE_TEXT or (other and not m.list_resident):
                    inc = False
                    break
                wave |= other
        if inc and S <= 16 and lists:           # the readiness pre-check of list documents
            ck = list(m.clock) + [0] * 16
            for c in r.changes:
                a = int(c["actor"])
                if a >= S or int(c["seq"]) != ck[a] + 1:
                    inc = False
                    break
                for t in range(int(c["n_deps"])):
                    dp = r.deps[int(c["dep_off"]) + t]
                    if int(dp["actor"]) != a and (int(dp["actor"]) >= S or int(dp["seq"]) > ck[int(dp["actor"])]):
                        inc = False
                ck[a] = int(c["seq"])
                if not inc:
                    break
    if inc and wave and m.n_o + r.nno <= small_lists:
        inc = False
    if inc and mode == 1 and L["HM_INC_COST"] * (r.nnc + r.nno) > m.n_c + m.n_o + r.nnc + r.nno:
        inc = False
    return 0 if not inc else 2 if wave else 3 if lane else 1


class _Exit(Exception):
    def __init__(self, slot):
        self.slot = slot


def _tile_state(r: Round, c0: int, mode: int) -> Resident:
    """the document as tile / change c0 of the round finds it (survivors, clock and log from the
    oracle's merge of the log up to there; s_used is not followed: None)"""
    if c0 == 0:
        return r.res
    base, new = r.prefix
    st = resident_after(list(base) + list(new[:c0]), r.S, mode)
    return st


def _group_doc(r: Round, G: int, cen: Counter, P: str, c0: int, c1: int, st: Resident, s_used):
    """inc_doc<G> on changes c0 .. c1 - 1 of the round, st = the state they find; raises _Exit(slot)"""
    L, S = limits(), r.S
    chs = r.changes[c0:c1]
    o0 = int(chs["op_first"][0]) if len(chs) else 0
    d0 = int(chs["dep_off"][0]) if len(chs) else 0
    ops = r.ops[o0:o0 + int(chs["n_ops"].sum())]
    nnc, nno, nnd = len(chs), len(ops), int(chs["n_deps"].sum())
    NA = r.n_actors
    n_old_r = st.n_r if c0 == 0 else r.n_r
    if nnc == 0 or NA > S or S > G:
        raise _Exit("BAIL_DESC")
    if nnc > L["NC"]:
        raise _Exit("LONG_CHANGES")
    if nno > G:
        raise _Exit("LONG_OPS")
    if nnd > G:
        raise _Exit("LONG_DEPS")
    if not st.valid or st.nockey:
        raise _Exit("BAIL_STATE")
    LST = G == 64
    wide = 1 << L["SEQ_BITS"]
    bad_c = any(int(c["actor"]) >= NA or int(c["seq"]) == 0 or int(c["seq"]) >= wide for c in chs)
    nl = min(len(st.list_objs), L["HM_INC_LISTS"]) if st.list_resident else 0
    known, slot_o, any_list = st.mapmask, None, False
    lists_doc = bool((r.flags | (HAS_LISTS if r.res.lists else 0)) & HAS_LISTS)
    for o in ops:
        act, obj, reg, vt = int(o["action"]), int(o["obj"]), int(o["reg"]), int(o["vtag"])
        val = int(np.int64(np.uint64(o["value"])))
        is_mk = act in (MAKE_MAP, MAKE_TABLE)
        other = obj != 0 and (obj >= 64 or not (st.mapmask >> obj) & 1)
        li = (obj in st.list_objs[:nl]) if LST else bool(nl and other)
        lst = not is_mk and li
        any_list |= lst
        why = None
        if is_mk and lists_doc:
            why = "BAIL_MAKE_LISTS"
        elif is_mk and (obj == 0 or obj >= L["MAP_IDS"] or (known >> obj) & 1):
            why = "BAIL_MAKE"
        elif (act not in (SET, DEL, LINK, INC) and not is_mk and not (lst and act == INS)) or \
                (act == INC and vt not in (V_INT, V_FLOAT)) or obj >= r.n_objs or (not is_mk and reg >= r.n_r) or \
                (vt == V_INT and abs(val) > TWO53) or \
                (act == INS and (int(o["elem"]) >= wide or (int(o["parent"]) != NONE and int(o["parent"]) >= r.n_r))) or \
                (not is_mk and not lst and obj != 0 and (obj >= 64 or not (known >> obj) & 1)):
            why = "BAIL_OP"
        if why:
            order = ("BAIL_MAKE_LISTS", "BAIL_MAKE", "BAIL_OP")
            slot_o = why if slot_o is None or order.index(why) < order.index(slot_o) else slot_o
        if is_mk and obj < 64:
            known |= 1 << obj
    if bad_c:
        raise _Exit("BAIL_ROWS")
    if slot_o:
        raise _Exit(slot_o)
    if not LST and any_list:
        raise _Exit("DEFER_LIST")
    if st.cabs + counter_add(ops) > TWO53:
        raise _Exit("BAIL_COUNTER")
    # causallyReady in arrival order; the fold steps
    ck = list(st.clock) + [0] * (64 - len(st.clock))
    nt, targets = 0, []
    for j, c in enumerate(chs):
        a, q = int(c["actor"]), int(c["seq"])
        if ck[a] + 1 != q:
            raise _Exit("BAIL_NOT_READY")
        own = False
        nd = int(c["n_deps"])
        for t in range(nd + 1):
            if t < nd:
                dp = r.deps[int(c["dep_off"]) + t]
                da, dq = int(dp["actor"]), int(dp["seq"])
                if da >= NA:
                    raise _Exit("BAIL_ROWS")
                if da == a:
                    dq, own = q - 1, True
            else:
                if own:
                    break
                da, dq = a, q - 1
            if ck[da] < dq:
                raise _Exit("BAIL_NOT_READY")
            if dq == 0:
                continue
            if nt >= 2 * G:
                raise _Exit("FOLD_STEPS")
            in_round = any(int(x["actor"]) == da and int(x["seq"]) == dq for x in chs[:j])
            targets.append((da, dq, in_round))
            nt += 1
        ck[a] = q
    pos = {(a, q): i for i, (a, q, p) in enumerate(st.keys) if p}
    for da, dq, in_round in targets:
        if in_round:
            continue
        i = pos.get((da, dq))
        back = st.n_c - i if i is not None else None          # 1 = the log's last row
        if back is not None and back <= tail_rows(G):
            cen[(P, "SRC_TAIL")] += 1
        else:
            cen[(P, "SRC_LOOP")] += 1
        if back is None:
            raise _Exit("BAIL_NO_SOURCE")
    # first-touch registers
    seen, tot_old, grow = set(), 0, 0
    n_up_bad = False
    for k, o in enumerate(ops):
        reg = int(o["reg"])
        if o["action"] >= SET and reg not in seen:
            seen.add(reg)
            push = int(((ops["reg"][k:] == reg) & ((ops["action"][k:] == SET) | (ops["action"][k:] == LINK))).sum())
            n_old = st.reg_surv[reg] if reg < min(n_old_r, len(st.reg_surv)) else 0
            n_up_bad |= n_old + push > G
            tot_old += n_old
            grow += n_old + push
    if n_up_bad:
        raise _Exit("N_UP")
    if tot_old > 2 * G:
        raise _Exit("TOT_OLD")
    if s_used is not None and s_used + grow > r.o_cap:
        raise _Exit("BAIL_NO_ROOM")
    if LST and any_list:
        _list_plan(r, G, chs, ops, st, n_old_r, nl)


def _list_plan(r, G, chs, ops, st, n_old_r, nl):
    """the exits of the list phase (the ins-register check, then list_plan), in the kernel's order"""
    op_actor = np.repeat(chs["actor"], chs["n_ops"])
    dirl = st.list_objs[:nl]
    epos = {reg: i for i, reg in enumerate(st.lorder)}
    L = []                                               # per op: (is list op, ins, list index, reg, parent, key)
    for o, a in zip(ops, op_actor):
        act, obj = int(o["action"]), int(o["obj"])
        lst = act not in (MAKE_MAP, MAKE_TABLE) and obj in dirl
        L.append((lst, lst and act == INS, dirl.index(obj) if lst else None, int(o["reg"]), int(o["parent"]),
                  (int(o["elem"]) << 8) | (int(a) & 0xFF)))
    for lst, is_ins, li, reg, par, key in L:
        if is_ins and reg < n_old_r and reg < len(st.reg_obj) and (st.reg_obj[reg] != NONE or st.reg_surv[reg] != 0):
            raise _Exit("BAIL_INS_REG")
    bad, roots = False, []
    for g, (lst, is_ins, li, reg, par, key) in enumerate(L):
        if not lst:
            continue
        lb, lc = st.lspan[dirl[li]]
        pnew = ecr = None
        for k in range(g):
            if not L[k][1]:
                continue
            if is_ins and L[k][3] == reg:
                bad = True
            if is_ins and L[k][3] == par:
                pnew, bad = k, bad or L[k][2] != li
            if not is_ins and L[k][3] == reg:
                ecr, bad = k, bad or L[k][2] != li
        if is_ins and pnew is None:
            pold = None
            if par != NONE:
                pold = epos.get(par) if par < n_old_r else None
                bad |= pold is None or not lb <= pold < lb + lc
            roots.append([g, par, key, pold, lb, lc, li, lb if par == NONE else (pold or 0) + 1])
        if not is_ins and ecr is None:
            eold = epos.get(reg) if reg < n_old_r else None
            bad |= eold is None or not lb <= eold < lb + lc
    if bad:
        raise _Exit("BAIL_LP_PARENT")
    for rt in roots:
        g, par, key, pold, lb, lc, li, ins_at = rt
        end = lb + lc
        if not ins_at < end:
            continue
        nxt = st.lorder[ins_at]
        if not (st.epar[nxt] == par and not key > st.ekey[nxt]):
            continue
        found, dup = end, False
        for j0 in range(ins_at, end, G):
            stops = []
            for j in range(j0, min(j0 + G, end)):
                y = st.lorder[j]
                if st.epar[y] == par:
                    dup |= st.ekey[y] == key
                    stops.append(st.ekey[y] < key)
                else:
                    stops.append(par != NONE and (st.epar[y] == NONE or epos[st.epar[y]] < pold))
            if any(stops):
                found = j0 + stops.index(True)
                break
        if dup:
            raise _Exit("BAIL_LP_DUP")
        rt[7] = found
    akeys = [((rt[7] << 4) | ((8 | rt[6]) if rt[1] == NONE else 0), rt[1]) for rt in roots]
    if any(a[0] == b[0] and a[1] != b[1] for a in akeys for b in akeys):
        raise _Exit("BAIL_LP_CLASH")


def _group_pass(r: Round, G: int, tiled: bool, cen: Counter, mode: int) -> str:
    """one document in inc_group_kernel<G, tiled>: 'DONE', 'DEFER' or 'BAIL'"""
    P = {8: "GROUP8", 16: "GROUP16"}.get(G, "WAVE_TILED" if tiled else "WAVE")
    cen[(P, "ENTER")] += 1
    L = limits()
    try:
        if not tiled:
            _group_doc(r, G, cen, P, 0, r.nnc, r.res, r.res.s_used)
        else:
            c0 = 0
            while c0 < r.nnc:
                so = sd = k = 0
                for c in r.changes[c0:c0 + L["NC"]]:
                    so, sd = so + int(c["n_ops"]), sd + int(c["n_deps"])
                    if so > G or sd > G:
                        break
                    k += 1
                if k == 0:
                    raise _Exit("BAIL_TILE_BIG")
                cen[(P, "TILES")] += 1
                try:
                    _group_doc(r, G, cen, P, c0, c0 + k, _tile_state(r, c0, mode), r.res.s_used if c0 == 0 else None)
                except _Exit as e:
                    cen[(P, e.slot)] += 1
                    if c0:
                        cen[(P, "TILE_LATER_FAILED")] += 1
                        return "BAIL"
                    return "DEFER" if G < 64 and e.slot in FAILG + ("DEFER_LIST",) else "BAIL"
                c0 += k
    except _Exit as e:
        cen[(P, e.slot)] += 1
        return "DEFER" if (G < 64 and e.slot in FAILG) or e.slot == "DEFER_LIST" else "BAIL"
    cen[(P, "DONE")] += 1
    return "DONE"


def _lane_pass(r: Round, cen: Counter, mode: int) -> str:
    L, S, st = limits(), r.S, r.res
    P = "LANE8" if S == 8 else "LANE16"
    cen[(P, "ENTER")] += 1
    NA, wide = r.n_actors, 1 << L["SEQ_BITS"]
    lists = bool((r.flags | (HAS_LISTS if st.lists else 0)) & HAS_LISTS)
    try:
        if r.nnc == 0 or NA > S:
            raise _Exit("BAIL_DESC")
        if not st.valid or st.nockey or st.list_resident:
            raise _Exit("BAIL_STATE")
        cur = list(st.clock) + [0] * 16
        mm, cadd, defer = st.mapmask, 0, False
        for c in r.changes:
            a, q = int(c["actor"]), int(c["seq"])
            if a >= NA or q == 0 or q >= wide:
                raise _Exit("BAIL_ROWS")
            if cur[a] + 1 != q:
                raise _Exit("BAIL_NOT_READY")
            for t in range(int(c["n_deps"])):
                dp = r.deps[int(c["dep_off"]) + t]
                if int(dp["actor"]) >= NA:
                    raise _Exit("BAIL_ROWS")
                if int(dp["actor"]) != a and cur[int(dp["actor"])] < int(dp["seq"]):
                    raise _Exit("BAIL_NOT_READY")
            for o in r.ops[int(c["op_first"]):int(c["op_first"]) + int(c["n_ops"])]:
                act, obj, reg, vt = int(o["action"]), int(o["obj"]), int(o["reg"]), int(o["vtag"])
                val = int(np.int64(np.uint64(o["value"])))
                if act in (MAKE_MAP, MAKE_TABLE):
                    if lists:
                        defer = True
                        continue
                    if obj == 0 or obj >= L["MAP_IDS"] or obj >= r.n_objs or (mm >> obj) & 1:
                        raise _Exit("BAIL_MAKE")
                    mm |= 1 << obj
                    continue
                if act in (INS, MAKE_LIST, MAKE_TEXT):
                    defer = True
                    continue
                if act not in (SET, DEL, LINK, INC) or obj >= r.n_objs or reg >= r.n_r:
                    raise _Exit("BAIL_OP")
                if obj != 0 and (obj >= 64 or not (mm >> obj) & 1):
                    if lists:
                        defer = True
                        continue
                    raise _Exit("BAIL_OP")
                if (act == INC and vt not in (V_INT, V_FLOAT)) or (vt == V_INT and abs(val) > TWO53):
                    raise _Exit("BAIL_OP")
                if vt == V_INT and (act == INC or (act == SET and int(o["datatype"]) == DT_COUNTER)):
                    cadd += abs(val)
            cur[a] = q
        if defer:
            raise _Exit("DEFER_LIST")
        if st.cabs + cadd > TWO53:
            raise _Exit("BAIL_COUNTER")
        # apply: each change's fold sources (the last LANE_TAIL rows in registers), then its ops
        keys = [(a, q) for a, q, p in st.keys if p]
        slot = [i for i, (a, q, p) in enumerate(st.keys) if p]
        pos = dict(zip(keys, slot))
        used = st.s_used
        for j, c in enumerate(r.changes):
            end = st.n_c + j
            for _, da, dq in fold_targets(r, j, j + 1):
                i = pos.get((da, dq))
                if i is not None and end - i <= L["LANE_TAIL"]:
                    cen[(P, "SRC_TAIL")] += 1
                else:
                    cen[(P, "SRC_LOOP")] += 1
                    if i is None:
                        raise _Exit("BAIL_NO_SOURCE")
            pos[(int(c["actor"]), int(c["seq"]))] = end
            cops = [o for o in r.ops[int(c["op_first"]):int(c["op_first"]) + int(c["n_ops"])]
                    if int(o["action"]) not in (MAKE_MAP, MAKE_TABLE)]
            if not cops:
                continue
            regs = [int(o["reg"]) for o in cops]
            assert len(set(regs)) == len(regs), "the lane restatement takes one op per register and change"
            before, after = _tile_state(r, j, mode).reg_surv, _tile_state(r, j + 1, mode).reg_surv
            for reg in regs:
                n = before[reg] if reg < len(before) else 0
                if n > L["LSV"]:
                    raise _Exit("BAIL_LSV")
                cnt = after[reg]
                if cnt > n:
                    if used + cnt > r.o_cap:
                        raise _Exit("BAIL_NO_ROOM")
                    used += cnt
    except _Exit as e:
        cen[(P, e.slot)] += 1
        return "BAIL"                          # (the lane pass's defers re-merge too)
    cen[(P, "DONE")] += 1
    return "DONE"


def meta_slots(after: Resident, cen: Counter):
    """inc_meta_kernel on a re-merged document"""
    if not after.in_meta:
        return
    cen[("META", "ENTER")] += 1
    if not after.clean:
        cen[("META", "META_DIRTY")] += 1
        return
    if after.lists_over:
        cen[("META", "META_LISTS_OVER")] += 1
    if after.list_refused:
        cen[("META", "META_LIST_REFUSED")] += 1
    cen[("META", "META_NOCKEY" if after.nockey else "META_VALID_LISTS" if after.list_resident else "META_VALID")] += 1


def route(r: Round, mode: int, refused=False):
    """(passes in order, census slots moved {(pass, slot): count}, last_routing()); refused: the
    re-merge reports the document (a counter past 2^53: HM_ERR_UNSUPPORTED; a document that throws),
    the store rolls the round back and re-merges the log as it was"""
    cen: Counter = Counter()
    passes: List[str] = []
    rt = plan_route(r, mode)
    S, G = r.S, group_of(r.S)
    out = "COLD"
    if rt == 3:
        passes.append("LANE8" if S == 8 else "LANE16")
        out = _lane_pass(r, cen, mode)
    elif rt:
        tl = r.nnc > limits()["NC"] or r.nno > 64 or r.nnd > 64
        if G < 64 and rt == 1:
            passes.append("GROUP%d" % G)
            out = _group_pass(r, G, False, cen, mode)
        if G == 64 or rt == 2 or out == "DEFER":
            passes.append("WAVE_TILED" if tl else "WAVE")
            out = _group_pass(r, 64, tl, cen, mode)
    if out != "DONE":
        base, new = r.prefix
        if refused:
            cen[("META", "ENTER")] += 1
            cen[("META", "META_DIRTY")] += 1
            meta_slots(resident_after(list(base), S, mode), cen)
        else:
            meta_slots(resident_after(list(base) + list(new), S, mode), cen)
    routing = {"incremental": int(out == "DONE"), "remerged": int(rt == 0), "handed_back": int(rt != 0 and out != "DONE")}
    return passes, cen, routing


# ---------------------------------------------------------------------------------------------
# generators and the pairs
# ---------------------------------------------------------------------------------------------
def actor(i):
    return f"a{i:02d}"


A0, A1 = actor(0), actor(1)


def chain(n, first=1, who=A0, key="k", ops=1, keys=None):
    """n changes of one actor in order, no listed deps, `ops` sets each (key j of `keys` keys, or a key of its own)"""
    out, j = [], (first - 1) * ops
    for i in range(n):
        out.append(ch(who, first + i, {}, *[s(f"{key}{(j + x) % keys if keys else j + x}", j + x) for x in range(ops)]))
        j += ops
    return out


def crowd(n, key="k"):
    """n actors, one concurrent change each, every one setting `key`: a register of n survivors"""
    return [ch(actor(i), 1, {}, s(key, i)) for i in range(n)]


def text_base(n_lists=1, elems=1):
    """one change that makes n_lists lists, links each and inserts `elems` elements into each"""
    ops = []
    for k in range(n_lists):
        ops += [mk("makeList", f"L{k}"), link(f"l{k}", f"L{k}")]
        ops += [ins(f"L{k}", "_head" if e == 0 else f"{A0}:{k * 1000 + e}", k * 1000 + e + 1) for e in range(elems)]
    return [ch(A0, 1, {}, *ops)]


@dataclass
class EdgePair:
    name: str
    S: int
    mode: int
    sides: Tuple[Tuple[list, list], Tuple[list, list]]     # (base log, round) with the comparison held / one step past it
    slots: Tuple[Tuple[str, str], Tuple[str, str]]         # the (pass, slot) each side moves and the other does not
    step: str               # change / op / dep: one more row in the round; base: one more row in the base log;
                            # same: the same row counts, one field of one row differs (named in `what`)
    what: str
    queued: Tuple[int, int] = (0, 0)                       # the oracle's queue after base + round
    status: Tuple[int, int] = (0, 0)                       # the store's status of the round (16: UNSUPPORTED, 2 / 4 / 5: it
                                                           # throws in the oracle too; rolled back either way)
    rows: int = 1                                          # rows the step adds (base: to the base log's changes + deps + ops)
    moved: Optional[Tuple[tuple, tuple]] = None            # Round.moved of each side, where the pair is about it
    plain: bool = False                                    # no comparison between the sides: results and census only

    def rounds(self):
        return tuple(round_of(b, n, self.S, self.mode) for b, n in self.sides)

    def route(self, k):
        return route(self.rounds()[k], self.mode, self.status[k] != 0)


@lru_cache(maxsize=None)
def pairs() -> List[EdgePair]:
    L = limits()
    NC, LSV = L["NC"], L["LSV"]
    P: List[EdgePair] = []

    def add(name, S, sides, slots, step, what, mode=2, **kw):
        P.append(EdgePair(name, S, mode, sides, slots, step, what, **kw))

    def same_base(base, near, far):
        return ((base, near), (base, far))

    b4 = chain(4)
    # ---- plan: small ----
    for S in (8, 16, 12, 32):
        G = group_of(S)
        first = "GROUP%d" % G if G < 64 else "WAVE"
        far = ("LANE%d" % S, "ENTER") if S in (8, 16) else ("WAVE_TILED", "TILES")
        add(f"small_changes_s{S}", S, same_base(b4, chain(NC, 5), chain(NC + 1, 5)), ((first, "DONE"), far), "change",
            f"{NC} / {NC + 1} changes of one op: small against the lane pass (strides 8, 16) or tiles of {NC} + 1 "
            "(stride 12 through GROUP16's nnc > NC defer, stride 32 directly)")
    mo = L["HM_INC_MAX_NEW_O"]
    for S in (8, 16):
        add(f"small_ops_s{S}", S, same_base(b4, chain(1, 5, ops=mo), chain(1, 5, ops=mo + 1)),
            (("WAVE", "DONE"), ("LANE%d" % S, "ENTER")), "op",
            f"one change of {mo} / {mo + 1} sets: small (the group pass defers nno > G to the wave) against the lane pass")
    add("small_ops_s32", 32, same_base(b4, chain(1, 5, ops=mo), chain(1, 5, ops=mo + 1)),
        (("WAVE", "DONE"), ("WAVE_TILED", "BAIL_TILE_BIG")), "op",
        f"one change of {mo} / {mo + 1} sets at stride 32: the second needs tiles and no tile holds it (k == 0)")
    # tgt = changes + dep rows: 8 changes of 15 deps each at stride 16, the far side one dep row more
    c16 = crowd(16, "z")
    def fan(n_extra):
        out = []
        for i in range(NC):
            deps = {actor(x): 1 for x in range(16) if x != i}
            if i < n_extra:
                deps[actor(i)] = 1
            out.append(ch(actor(i), 2, deps, s(f"f{i}", i)))
        return out
    spare = L["HM_INC_MAX_TGT"] - NC - NC * 15
    add("small_tgt", 16, same_base(c16, fan(spare), fan(spare + 1)), (("WAVE_TILED", "DONE"), ("LANE16", "ENTER")), "dep",
        f"{NC} changes listing 15 deps each, {spare} / {spare + 1} of them their own actor too: tgt = "
        f"{L['HM_INC_MAX_TGT']} / {L['HM_INC_MAX_TGT'] + 1}; small rounds of over 64 dep rows take the wave pass's tiles")
    # ---- plan: lane and longr ----
    lc, lo = L["HM_INC_LANE_MAX_C"], L["HM_INC_LANE_MAX_O"]
    for S in (8, 16):
        add(f"lane_changes_s{S}", S, same_base(b4, chain(lc, 5, keys=16), chain(lc + 1, 5, keys=16)),
            ((f"LANE{S}", "DONE"), ("META", "ENTER")), "change", f"{lc} / {lc + 1} changes: the lane pass against the re-merge")
        add(f"lane_ops_s{S}", S, same_base(b4, chain(8, 5, ops=lo // 8), chain(8, 5, ops=lo // 8)[:7] +
                                           chain(1, 12, ops=lo // 8 + 1, key="y")),
            ((f"LANE{S}", "DONE"), ("META", "ENTER")), "op", f"8 changes of {lo} / {lo + 1} ops in all")
    add("lane_changes_s12", 12, same_base(b4, chain(lc, 5, keys=16), chain(lc + 1, 5, keys=16)),
        (("WAVE_TILED", "TILES"), ("WAVE_TILED", "TILES")), "change",
        f"the same {lc} / {lc + 1} changes at stride 12: both take tiles ({lc // NC} / {lc // NC + 1} of them)")
    tc, to = L["HM_INC_TILED_MAX_C"], L["HM_INC_TILED_MAX_O"]
    add("longr_changes_s32", 32, same_base(b4, chain(tc, 5, keys=16), chain(tc + 1, 5, keys=16)),
        (("WAVE_TILED", "DONE"), ("META", "ENTER")), "change", f"{tc} / {tc + 1} changes of a map document at stride 32")
    add("longr_ops_s32", 32, same_base(b4, chain(to // 64, 5, ops=64, keys=256),
                                       chain(to // 64 - 1, 5, ops=64, keys=256) + chain(1, 4 + to // 64, ops=65, key="y")),
        (("WAVE_TILED", "DONE"), ("META", "ENTER")), "op", f"{to // 64} changes of 64 ops, the last of 65: {to} / {to + 1}")
    tb = text_base(1, 2)
    def typing(n, first_elem=10):
        return [ch(A0, 2 + i, {}, ins("L0", f"{A0}:{2 if i == 0 else first_elem + i - 1}", first_elem + i)) for i in range(n)]
    add("longr_changes_list_s8", 8, same_base(tb, typing(tc), typing(tc + 1)), (("WAVE_TILED", "DONE"), ("META", "ENTER")),
        "change", f"{tc} / {tc + 1} changes of one insert each into a list at stride 8 (route 2, tiles)")
    # ---- plan: actors ----
    add("remap", 8, same_base(chain(4, who="m00"), [ch("zzz", 1, {}, s("n", 1))], [ch("aaa", 1, {}, s("n", 1))]),
        (("GROUP8", "DONE"), ("META", "ENTER")), "same",
        "a new actor whose id sorts last (ranks keep) / first (the log's rows are re-ranked: re-merge)")
    # ---- plan: list documents ----
    add("list_make", 8, same_base(tb, [ch(A0, 2, {}, ins("L0", f"{A0}:2", 3), s("x", 1))],
                                  [ch(A0, 2, {}, ins("L0", f"{A0}:2", 3), mk("makeMap", "M"))]),
        (("WAVE", "DONE"), ("META", "ENTER")), "same", "a round of an insert and a set / an insert and a makeMap (object creation)")
    late = ch(A0, 2, {A1: 1}, ins("L0", f"{A0}:2", 3))
    tb2 = tb + [ch(A1, 1, {}, s("y", 1))]
    add("list_ready_s8", 8, ((tb2, [late]), (tb, [late])), (("WAVE", "DONE"), ("META", "META_DIRTY")), "base",
        "a list round whose dep is in the clock / one past it at stride 8: the plan's readiness pre-check re-merges",
        queued=(0, 1), rows=2)
    add("list_ready_s32", 32, ((tb2, [late]), (tb, [late])), (("WAVE", "DONE"), ("WAVE", "BAIL_NOT_READY")), "base",
        "the same at stride 32 (no pre-check): the wave pass finds it and hands the document back", queued=(0, 1), rows=2)
    # ---- mode 1 ----
    sl = L["HM_INC_SMALL_LIST_OPS"]
    add("small_list_state", 32, ((text_base(1, sl - 1), [ch(A0, 2, {}, s("x", 1))]), (text_base(1, sl - 2), [ch(A0, 2, {}, s("x", 1))])),
        (("WAVE", "DONE"), ("META", "ENTER")), "base",
        f"mode 1: a list document of {sl + 1} / {sl} ops before the round: the second kept no state", mode=1)
    k = L["HM_INC_COST"]
    add("cost", 8, same_base(chain(k - 1), chain(1, k), chain(1, k, ops=2)), (("GROUP8", "DONE"), ("META", "ENTER")), "op",
        f"mode 1: {k} (new changes + ops) == the log's rows after the round ({k - 1} + {k - 1} + 2) / one op more", mode=1)
    # ---- group pass ----
    for G, S in ((8, 8), (16, 16), (64, 64)):
        gp = "GROUP%d" % G if G < 64 else "WAVE"
        npad = 24 if G < 64 else 200
        if G < 64:
          add(f"nno_g{G}", S, same_base(b4, chain(1, 5, ops=G), chain(1, 5, ops=G + 1)), ((gp, "DONE"), (gp, "LONG_OPS")), "op",
            f"one change of {G} / {G + 1} ops: nno > G defers to the wave")
        cw = crowd(G, "z")
        all_deps = {actor(x): 1 for x in range(G)}
        second = lambda dep: ch(A1, 2, dep, s("q", 1))
        if G < 64:
          add(f"nnd_g{G}", S, same_base(cw, [ch(A0, 2, all_deps, s("p", 1)), second({})], [ch(A0, 2, all_deps, s("p", 1)), second({actor(2): 1})]),
            ((gp, "DONE"), (gp, "LONG_DEPS")), "dep", f"two changes of {G} + 0 / {G} + 1 dep rows")
        seen = {actor(x): 1 for x in range(1, G)}
        pad = chain(npad, 3, keys=1, key="pad")          # ops that leave one survivor: slots to spare in the op segment
        add(f"n_up_g{G}", S, same_base(crowd(G - 1) + [ch(actor(G - 1), 1, {}, s("other", 1))] + chain(npad, 2, keys=1, key="pad"),
                                       [ch(actor(G - 1), 2, {}, s("k", 1)), ch(actor(G - 1), 3, {}, s("j", 1))],
                                       [ch(actor(G - 1), 2, {}, s("k", 1)), ch(actor(G - 1), 3, {}, s("k", 2))]),
            ((gp, "DONE"), (gp, "N_UP")), "same",
            f"a register of {G - 1} survivors and one / two pushes in the round (the second change sets j / k): n_up = {G} / {G + 1}")
        two = [ch(actor(i), 1, {}, s("k0", i), s("k1", i)) for i in range(G)] + [ch(A0, 2, {}, s("k2", 1))]
        add(f"tot_old_g{G}", S, same_base(two + pad, [ch(A0, 3 + npad, seen, dl("k0"), dl("k1"), s("k3", 1))],
                                          [ch(A0, 3 + npad, seen, dl("k0"), dl("k1"), s("k2", 2))]),
            ((gp, "DONE"), (gp, "TOT_OLD")), "same",
            f"deletes on two registers of {G} survivors, and a set on a fresh register / one of 1 survivor: tot_old = {2 * G} / {2 * G + 1}")
    ring = lambda n: [ch(actor(i), 2, {actor((i + 1) % 8): 1} if i < n else {}, s(f"r{i}", i)) for i in range(NC)]
    add("fold_steps_g8", 8, same_base(crowd(8, "z"), ring(NC - 1), ring(NC)), (("GROUP8", "SRC_TAIL"), ("GROUP8", "SRC_TAIL")), "dep",
        f"{NC} changes of {NC} actors, {NC - 1} / {NC} of them listing one dep: {2 * NC - 1} / {2 * NC} fold steps, nt = 2 G - 1 at the last")
    for S in (8, 16, 32):
        G = group_of(S)
        gp = "GROUP%d" % G if G < 64 else "WAVE"
        t = tail_rows(G)
        src = [ch(A1, 1, {}, s("y", 1))]
        add(f"src_tail_s{S}", S, ((src + chain(t - 1), [ch(A1, 2, {}, s("y", 2))]), (src + chain(t), [ch(A1, 2, {}, s("y", 2))])),
            ((gp, "SRC_TAIL"), (gp, "SRC_LOOP")), "base",
            f"a fold source {t} / {t + 1} rows back (the log's row 0): the last row in registers, the first the loop finds", rows=2)
    add("src_in_round", 8, same_base(crowd(2, "z"), [ch(A0, 2, {}, s("p", 1)), ch(A1, 2, {}, s("q", 1))],
                                     [ch(A0, 2, {}, s("p", 1)), ch(A0, 3, {}, s("q", 1))]),
        (("GROUP8", "SRC_TAIL"), ("GROUP8", "SRC_TAIL")), "same",
        "two changes folding two rows of the log / the second folds the first (src1): two / one log searches")
    # ---- wave pass and every group size: room, counters, elem, object ids, lists ----
    room_base = chain(12)                      # 12 ops, 12 survivors, o_cap = pow2c(12 + 3) = 16
    for S in (8, 32):
        gp = "GROUP8" if S == 8 else "WAVE"
        add(f"room_s{S}", S, same_base(room_base, [ch(A1, 1, {}, s("k0", 1), s("k1", 1), dl("fresh"))],
                                       [ch(A1, 1, {}, s("k0", 1), s("k1", 1), s("fresh", 1))]),
            ((gp, "DONE"), (gp, "BAIL_NO_ROOM")), "same",
            "12 survivors in 16 slots; two concurrent sets on old keys (grow 2 + 2) and a del / a set on a fresh key: "
            "s_used + grow = o_cap / o_cap + 1")
    cb = [ch(A0, 1, {}, s("c", TWO53 - 5, datatype="counter"))]
    for S in (8, 32):
        gp = "GROUP8" if S == 8 else "WAVE"
        add("counter_int" + ("_s8" if S == 8 else ""), S, same_base(cb, [ch(A0, 2, {}, incr("c", 5))], [ch(A0, 2, {}, incr("c", 6))]),
            ((gp, "DONE"), (gp, "BAIL_COUNTER")), "same",
            "a counter of 2^53 - 5 and an inc of 5 / 6: cabs = 2^53 / 2^53 + 1 (which the re-merge refuses too: UNSUPPORTED)",
            status=(0, 16))
    add("counter_f64", 32, same_base(cb, [ch(A0, 2, {}, incr("c", 5), incr("c", 0.5))], [ch(A0, 2, {}, incr("c", 5), incr("c", 1))]),
        (("WAVE", "DONE"), ("WAVE", "BAIL_COUNTER")), "same",
        "the same with a second inc of 0.5 (f64: does not count) / of 1", status=(0, 16))
    wide = 1 << L["SEQ_BITS"]
    add("elem_wide", 32, same_base(tb, [ch(A0, 2, {}, ins("L0", f"{A0}:2", wide - 1))], [ch(A0, 2, {}, ins("L0", f"{A0}:2", wide))]),
        (("WAVE", "DONE"), ("WAVE", "BAIL_OP")), "same",
        "an insert of elem 2^24 - 1 / 2^24 (which the re-merge refuses too: UNSUPPORTED)", status=(0, 16))
    for S in (8, 32):
        gp = "GROUP8" if S == 8 else "WAVE"
        add("seq_wide" + ("_s32" if S == 32 else ""), S, same_base(b4, [ch(A1, wide - 1, {}, s("y", 1))], [ch(A1, wide, {}, s("y", 1))]),
            ((gp, "BAIL_NOT_READY"), (gp, "BAIL_ROWS")), "same",
            "a change of seq 2^24 - 1 / 2^24 of an actor the document has not seen: both wait in the queue", queued=(1, 1))
    add("lane_seq_wide", 8, same_base(b4, [ch(A1, wide - 1, {}, s("y", 1))] + chain(NC, 5), [ch(A1, wide, {}, s("y", 1))] + chain(NC, 5)),
        (("LANE8", "BAIL_NOT_READY"), ("LANE8", "BAIL_ROWS")), "same", "the same at the head of a round of nine changes", queued=(1, 1))
    # ---- the list phase: the ins-register check and list_plan, each exit with a twin inside the envelope ----
    e = lambda n: f"{A0}:{n}"
    lb = [ch(A0, 1, {}, mk("makeList", "L0"), link("l0", "L0"), ins("L0", "_head", 1), ins("L0", e(1), 5))]
    lbv = [ch(A0, 1, {}, mk("makeList", "L0"), link("l0", "L0"), ins("L0", "_head", 1), ins("L0", e(1), 5), s(e(5), "v", obj="L0"))]
    add("lp_parent", 32, same_base(lb, [ch(A0, 2, {}, ins("L0", e(5), 10), ins("L0", e(10), 11))],
                                   [ch(A0, 2, {}, ins("L0", e(10), 11), ins("L0", e(5), 10))]),
        (("WAVE", "DONE"), ("WAVE", "BAIL_LP_PARENT")), "same",
        "an insert after an element the round inserted one op earlier / one op later (the oracle merges both: the re-merge "
        "sees the whole change)")
    add("ins_reg_bare", 32, same_base(lb, [ch(A0, 2, {}, ins("L0", e(1), 4))], [ch(A0, 2, {}, ins("L0", e(1), 5))]),
        (("WAVE", "DONE"), ("WAVE", "BAIL_INS_REG")), "same",
        "under a parent whose first child is elem 5 (no value yet): elem 4, placed by the scan / elem 5 again: its register "
        "holds the list's object (DUPLICATE_ELEM)",
        status=(0, 4))
    add("ins_reg", 32, same_base(lbv, [ch(A0, 2, {}, ins("L0", e(1), 4))], [ch(A0, 2, {}, ins("L0", e(1), 5))]),
        (("WAVE", "DONE"), ("WAVE", "BAIL_INS_REG")), "same",
        "the same where element 5 holds a value: its register has a survivor (DUPLICATE_ELEM)", status=(0, 4))
    add("lp_clash", 32, same_base(lb, [ch(A0, 2, {}, ins("L0", e(1), 7), ins("L0", e(5), 10))],
                                  [ch(A0, 2, {}, ins("L0", e(1), 3), ins("L0", e(5), 10))]),
        (("WAVE", "DONE"), ("WAVE", "BAIL_LP_CLASH")), "same",
        "element 1 has the child 5; the round inserts under 1 an elem 7 (before 5) / 3 (after 5's subtree) and under 5 "
        "an elem 10: the second round's two anchors, of different parents, share an insertion point")
    # ---- a map created in the round ----
    for S, tail_, gp in ((8, [], "GROUP8"), (8, chain(NC, 3), "LANE8")):
        add("made_order" + ("_lane" if tail_ else ""), S,
            same_base(b4[:1], [ch(A0, 2, {}, mk("makeMap", "M"), link("m", "M"), s("x", 1, obj="M"))] + tail_,
                      [ch(A0, 2, {}, s("x", 1, obj="M"), mk("makeMap", "M"), link("m", "M"))] + tail_),
            ((gp, "DONE"), (gp, "BAIL_OP")), "same",
            "a set on a map the same change created two ops earlier / creates one op later (UNKNOWN_OBJECT in the oracle too)"
            + (", at the head of a round of nine changes" if tail_ else ""), status=(0, 2))
    # ---- actors ----
    add("actors_s8", 8, same_base(crowd(6, "z"), [ch(actor(6), 1, {}, s("n", 1))], [ch(actor(6), 1, {}, s("n", 1)), ch(actor(7), 1, {}, s("n", 2))]),
        (("GROUP8", "DONE"), ("GROUP8", "DONE")), "change",
        "new actors that sort last: 7 / 8 = S actors after the round (a ninth is refused by the store on the host: "
        "test_inc_edges_gpu.test_actors_past_the_stride)", plain=True, rows=2)
    ids = L["MAP_IDS"]
    def maps(n):
        return [ch(A0, 1, {}, *[op for i in range(n) for op in (mk("makeMap", f"o{i}"), link(f"l{i}", f"o{i}"))])]
    def one_more(n):
        return [ch(A0, 2, {}, mk("makeMap", f"o{n}"), link(f"l{n}", f"o{n}"))]
    for S in (8, 32):
        gp = "GROUP8" if S == 8 else "WAVE"
        add(f"map_ids_s{S}", S, ((maps(ids - 2), one_more(ids - 2)), (maps(ids - 1), one_more(ids - 1))),
            ((gp, "DONE"), (gp, "BAIL_MAKE")), "base", f"makeMap of object id {ids - 1} / {ids} (mapmask holds ids below {ids})", rows=2)
    nl = L["HM_INC_LISTS"]
    def into_first(n):
        return [ch(A0, 2, {}, ins("L0", f"{A0}:1", 999))]
    add("lists", 32, ((text_base(nl), into_first(nl)), (text_base(nl + 1), into_first(nl + 1))),
        (("WAVE", "DONE"), ("META", "META_LISTS_OVER")), "base",
        f"{nl} / {nl + 1} list objects: the ninth drops the resident order, and the list round re-merges", rows=3)
    # ---- tiles ----
    add("tile_ops", 32, same_base(b4, chain(1, 5, ops=32) + chain(1, 6, ops=32, key="y"), chain(1, 5, ops=33) + chain(1, 6, ops=32, key="y")),
        (("WAVE", "DONE"), ("WAVE_TILED", "TILES")), "op", "two changes of 32 + 32 / 33 + 32 ops: one round / two tiles split on ops")
    c32 = crowd(32, "z")
    d32 = {actor(x): 1 for x in range(32)}
    d31 = {actor(x): 1 for x in range(31)}
    add("tile_deps", 32, same_base(c32, [ch(A0, 2, d32, s("p", 1)), ch(A1, 2, d32, s("q", 1))],
                                   [ch(A0, 2, d32, s("p", 1)), ch(A1, 2, d32, s("q", 1)), ch(actor(2), 2, {A0: 2}, s("r", 1))]),
        (("WAVE", "DONE"), ("WAVE_TILED", "TILES")), "change", "64 dep rows in two changes / a third change with one more: a tile boundary on dep rows", rows=3)
    ready9 = chain(NC, 5) + [ch(A0, 5 + NC, {}, s("late", 1))]
    unready9 = chain(NC, 5) + [ch(A0, 5 + NC, {A1: 1}, s("late", 1))]
    add("tile_later_failed", 32, same_base(b4, ready9, unready9), (("WAVE_TILED", "DONE"), ("WAVE_TILED", "TILE_LATER_FAILED")), "dep",
        "nine changes; the ninth (the second tile) lists a dep the document has not seen: the re-merge rewrites the first tile's rows",
        queued=(0, 1))
    # ---- lane pass ----
    long_tail = chain(NC, 2, key="w")          # eight more changes: the round is past `small`
    for S in (8, 16):
        lp = f"LANE{S}"
        if S >= LSV + 1:
            add(f"lsv_s{S}", S, ((crowd(LSV) + [ch(actor(LSV), 1, {}, s("j", 1))], [ch(A0, 2, {}, s("k", 9))] + long_tail[:0] + chain(NC, 3, key="w")),
                                 (crowd(LSV + 1), [ch(A0, 2, {}, s("k", 9))] + chain(NC, 3, key="w"))),
                ((lp, "DONE"), (lp, "BAIL_LSV")), "same",
                f"a register of {LSV} / {LSV + 1} survivors set by a round of nine changes (the ninth actor set j / k)")
        T = L["LANE_TAIL"]
        for back in (T, 2 * T):
            src = [ch(A1, 1, {}, s("y", 1))]
            rnd = [ch(A1, 2, {}, s("y", 2))] + chain(NC, back, key="w")
            add(f"lane_src_{back}_s{S}", S, ((src + chain(back - 1), rnd), (src + chain(back), [rnd[0]] + chain(NC, back + 1, key="w"))),
                ((lp, "SRC_TAIL"), (lp, "SRC_LOOP")) if back == T else ((lp, "SRC_LOOP"), (lp, "SRC_LOOP")), "base",
                f"the lane pass's first fold source {back} / {back + 1} rows back: " +
                ("in the tail registers / found by the loop" if back == T else "the loop's first step of 8 rows / its second"),
                plain=back != T, rows=2)
    c4 = crowd(4, "z")
    def lane_deps(own):
        out = []
        for nd in range(4):
            deps = {actor(x): 1 for x in range(1, nd + 1)}
            if own and nd:
                deps[A0] = 1 + nd                        # (its own actor: read as seq - 1)
            out.append(ch(A0, 2 + nd, deps, s(f"d{nd}", nd)))
        return out + chain(NC, 6, key="w")
    add("lane_deps", 8, same_base(c4, lane_deps(False), lane_deps(True)), (("LANE8", "DONE"), ("LANE8", "DONE")), "dep",
        "changes of 0, 1, 2, 3 listed deps (across LKF = 2), without / with a dep on the change's own actor: the same "
        "fold steps in another order, no comparison between them", plain=True)
    def typing_ops(n, per, last=None):
        out, elem, prev = [], 10, 2
        for i in range(n):
            k = last if last is not None and i == n - 1 else per
            ops = []
            for _ in range(k):
                ops.append(ins("L0", e(prev), elem))
                prev, elem = elem, elem + 1
            out.append(ch(A0, 2 + i, {}, *ops))
        return out
    add("longr_ops_list_s8", 8, same_base(tb, typing_ops(to // 64, 64), typing_ops(to // 64, 64, 65)),
        (("WAVE_TILED", "DONE"), ("META", "ENTER")), "op", f"{to // 64} changes of 64 inserts, the last of 65: {to} / {to + 1} ops of a list document")
    add("tile_big_list_s8", 8, same_base(tb, typing_ops(NC + 1, 1, 64), typing_ops(NC + 1, 1, 65)),
        (("WAVE_TILED", "DONE"), ("WAVE_TILED", "BAIL_TILE_BIG")), "op",
        f"a list round of {NC} changes of one insert and a ninth of 64 / 65: the second tile holds it / no tile does (k == 0)")
    # ---- lane pass: segments the append moves, each alone ----
    mb = chain(52, keys=40) + [ch(A0, 53 + i, {}) for i in range(48)]        # 100 changes, 52 ops, 40 registers
    res = resident_after(mb, 8, 2)
    room = [c - n for c, n in zip(res.caps, (res.n_c, res.n_d, res.n_o, res.n_r))]
    def lane_round(n_changes, n_ops, new_keys):
        out, j = [], 0
        for i in range(n_changes):
            k = n_ops // NC + (1 if i < n_ops % NC else 0) if i < NC else 0
            out.append(ch(A0, 101 + i, {}, *[s(f"n{j + x}" if j + x < new_keys else f"k{(j + x) % 40}", j + x) for x in range(k)]))
            j += k
        return out
    for seg, near, far in (("c", lane_round(room[0], NC + 1, 0), lane_round(room[0] + 1, NC + 1, 0)),
                           ("o", lane_round(NC + 1, room[2], 0), lane_round(NC + 1, room[2] + 1, 0)),
                           ("r", lane_round(NC + 1, room[3], room[3]), lane_round(NC + 1, room[3] + 1, room[3] + 1))):
        add(f"lane_moved_{seg}", 8, same_base(mb, near, far), (("LANE8", "DONE"), ("LANE8", "DONE")),
            "change" if seg == "c" else "op", f"a lane round that fills the {seg} segment / outgrows it alone (the lane copies the moved rows)",
            plain=True, moved=((False,) * 4, tuple(x == seg for x in "cdor")))
    # ---- lane pass: the exits it shares with the group passes ----
    add("lane_not_ready", 8, same_base(b4, chain(NC, 5) + [ch(A0, 5 + NC, {}, s("late", 1))], chain(NC, 5) + [ch(A0, 5 + NC, {A1: 1}, s("late", 1))]),
        (("LANE8", "DONE"), ("LANE8", "BAIL_NOT_READY")), "dep", "nine changes; the ninth lists a dep the document has not seen", queued=(0, 1))
    add("lane_counter", 8, same_base(cb, [ch(A0, 2, {}, incr("c", 5))] + chain(NC, 3), [ch(A0, 2, {}, incr("c", 6))] + chain(NC, 3)),
        (("LANE8", "DONE"), ("LANE8", "BAIL_COUNTER")), "same", "the counter bound at the head of a round of nine changes", status=(0, 16))
    add("lane_map_ids", 8, ((maps(ids - 2), one_more(ids - 2) + chain(NC, 3)), (maps(ids - 1), one_more(ids - 1) + chain(NC, 3))),
        (("LANE8", "DONE"), ("LANE8", "BAIL_MAKE")), "base", f"makeMap of object id {ids - 1} / {ids} at the head of a round of nine changes", rows=2)
    idle = [ch(A1, 4 + i, {}) for i in range(NC - 2)]
    add("lane_room", 8, same_base(room_base, [ch(A1, 1, {}, s("k0", 1)), ch(A1, 2, {}, s("k1", 1)), ch(A1, 3, {}, dl("fresh"))] + idle,
                                  [ch(A1, 1, {}, s("k0", 1)), ch(A1, 2, {}, s("k1", 1)), ch(A1, 3, {}, s("fresh", 1))] + idle),
        (("LANE8", "DONE"), ("LANE8", "BAIL_NO_ROOM")), "same",
        "12 survivors in 16 slots; a new actor's sets on two old keys (2 + 2 slots at the end) and a del / a set on a fresh key; "
        "six changes without ops make the round nine long")
    # ---- inc_meta_kernel ----
    lch = L["META_LCH"]
    add("meta_lch", 8, ((chain(lch, keys=16), chain(1, lch + 1, keys=16)), (chain(lch + 1, keys=16), chain(1, lch + 2, keys=16))),
        (("GROUP8", "DONE"), ("GROUP8", "DONE")), "base",
        f"a document of {lch} / {lch + 1} changes re-merged (the op -> change searches in LDS / in HBM), then one incremental "
        "round on the survivor metadata it left", plain=True, rows=2)
    add("meta_dirty", 8, ((chain(2), chain(1, 3)), ([chain(3)[0], chain(3)[2]], [chain(3)[1]])),
        (("GROUP8", "DONE"), ("META", "META_VALID")), "same",
        "a document of changes 1, 2 given 3 / left with 3 queued behind a missing 2 (no state) and given 2")
    return P


def follow_up(enc, S, tag):
    """one ordinary change for the round after the edge round: a new actor that sorts last, or (a
    document of S actors) the next change of its last actor"""
    if len(enc.actors) < S:
        return [ch("zzzz-follow", 1, {}, s("follow", tag))]
    a = enc.actors[-1]
    q = max(int(c["seq"]) for c in enc.log_changes[enc.log_changes["actor"] == len(enc.actors) - 1])
    return [ch(a, q + 1, {}, s("follow", tag))]
