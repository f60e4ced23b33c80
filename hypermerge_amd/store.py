"""Resident document store: Python face of ``hm_store_*`` / ``hm_doc_*`` /
``hm_batch_submit`` / ``hm_batch_wait`` (include/hypermerge_amd.h).

``DocStore`` keeps every open document's Automerge BackendState on the GPU
(the ``DocBackend.back`` of src/DocBackend.ts:50).  ``DocEncoder`` is the
per-document host interner that turns decoded ``Change`` dicts into columnar
rows across successive ``applyChanges`` calls: actor ids keep their JS string
order as the *rank*, so a new actor can re-rank the document's earlier rows
(the engine applies the returned remap on the device); object UUIDs,
``(object, key)`` / ``(list, elemId)`` registers and change contents keep the
ids they were first given.
"""
from __future__ import annotations

import ctypes
import sys
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .columnar import (ACTIONS, CHANGE_DT, DEP_DT, DOC_DT, DOC_RESULT_DT, OP_DT, REG_RESULT_DT,
                       SURV_RESULT_DT, DATATYPES, DOC_HAS_COUNTERS, DOC_HAS_LISTS, DT_COUNTER, HEAD,
                       INC, INS, LINK, MAKE_LIST, MAKE_TEXT, NONE, ROOT_ID, SET, DEL, V_NULL, V_OBJ,
                       Batch, CBatch, Results, _value, content_key, js_key)
from .engine import MC_ONLY_LISTED, MC_RAW, CPastOut, Engine, EngineError, lib, pack_entries, pack_fields, unpack_fields, FIELD_OP_DT


class StringPool:
    """Store-wide pool of map keys and string values (host only; ids are shipped)."""

    def __init__(self) -> None:
        self.index: Dict[str, int] = {}
        self.strings: List[str] = []

    def intern(self, s: str) -> int:
        i = self.index.get(s)
        if i is None:
            i = self.index[s] = len(self.strings)
            self.strings.append(s)
        return i


@dataclass
class Append:
    """New rows of one document (offsets local to this append) + its totals after it."""
    changes: np.ndarray
    deps: np.ndarray
    ops: np.ndarray
    n_actors: int
    n_regs: int
    n_objs: int
    flags: int
    remap: Optional[np.ndarray]      # old rank -> new rank (None: unchanged)


class DocEncoder:
    """Interner state of one document across applyChanges calls."""

    def __init__(self, pool: StringPool, keep_log: bool = True) -> None:
        self.pool = pool
        self.actors: List[str] = []                  # rank -> actor id
        self.objs: Dict[str, int] = {ROOT_ID: 0}
        self.obj_list: List[str] = [ROOT_ID]
        self.regs: Dict[Tuple[int, str], int] = {}
        self.reg_list: List[Tuple[int, str]] = []
        self.content: Dict[str, int] = {}
        self.flags = 0
        self.keep_log = keep_log
        self.log_changes = np.zeros(0, CHANGE_DT)    # doc-local offsets
        self.log_deps = np.zeros(0, DEP_DT)
        self.log_ops = np.zeros(0, OP_DT)

    # -- interning -----------------------------------------------------------------------------
    def _obj(self, u: str) -> int:
        i = self.objs.get(u)
        if i is None:
            i = self.objs[u] = len(self.obj_list)
            self.obj_list.append(u)
        return i

    def _reg(self, o: int, key: str) -> int:
        i = self.regs.get((o, key))
        if i is None:
            i = self.regs[(o, key)] = len(self.reg_list)
            self.reg_list.append((o, key))
        return i

    def snapshot(self):
        """State to restore if the append is rolled back (a throwing applyChanges)."""
        return (list(self.actors), dict(self.objs), list(self.obj_list), dict(self.regs), list(self.reg_list),
                dict(self.content), self.flags, self.log_changes, self.log_deps, self.log_ops)

    def restore(self, snap) -> None:
        (self.actors, self.objs, self.obj_list, self.regs, self.reg_list, self.content, self.flags,
         self.log_changes, self.log_deps, self.log_ops) = snap

    def encode(self, changes: Sequence[Dict[str, Any]], extra_actors: Sequence[str] = ()) -> Append:
        new_actors = set(extra_actors)
        for c in changes:
            new_actors.add(c["actor"])
            new_actors.update((c.get("deps") or {}).keys())
        new_actors -= set(self.actors)
        remap = None
        if new_actors:
            ranked = sorted(set(self.actors) | new_actors, key=js_key)
            rank = {a: i for i, a in enumerate(ranked)}
            if self.actors:
                mp = np.array([rank[a] for a in self.actors], np.uint8)
                if not np.array_equal(mp, np.arange(len(self.actors), dtype=np.uint8)):
                    remap = mp
            self.actors = ranked
        rank = {a: i for i, a in enumerate(self.actors)}
        ch_rows, dep_rows, op_rows = [], [], []
        flags = 0
        for c in changes:
            deps = c.get("deps") or {}
            dep_off = len(dep_rows)
            for da, ds in deps.items():
                dep_rows.append((rank[da], 0, int(ds)))
            ck = content_key(c)
            cid = self.content.get(ck)
            if cid is None:
                cid = self.content[ck] = len(self.content)
            op_first = len(op_rows)
            for op in c.get("ops", []):
                act = ACTIONS[op["action"]]
                o = self._obj(op["obj"])
                reg, parent, elem, key = NONE, NONE, 0, 0
                vt, val = V_NULL, 0
                if act == INS:
                    elem = int(op["elem"])
                    reg = self._reg(o, f"{c['actor']}:{elem}")
                    parent = HEAD if op["key"] == "_head" else self._reg(o, op["key"])
                elif act in (SET, DEL, LINK, INC):
                    reg = self._reg(o, op["key"])
                    key = self.pool.intern(op["key"])
                    if act == LINK:
                        vt, val = V_OBJ, self._obj(op["value"])
                    elif act in (SET, INC):
                        vt, val = _value(op.get("value"), self.pool.index, self.pool.strings, self.objs)
                dt = DATATYPES[op.get("datatype")]
                if act in (MAKE_LIST, MAKE_TEXT):
                    flags |= DOC_HAS_LISTS
                if act == INC or dt == DT_COUNTER:
                    flags |= DOC_HAS_COUNTERS
                op_rows.append((o, reg, parent, elem, act, dt, vt, 0, key, val))
            ch_rows.append((rank[c["actor"]], len(deps), int(c["seq"]), dep_off, len(op_rows) - op_first,
                            op_first, cid))
        self.flags |= flags
        a = Append(np.array(ch_rows, CHANGE_DT) if ch_rows else np.zeros(0, CHANGE_DT),
                   np.array(dep_rows, DEP_DT) if dep_rows else np.zeros(0, DEP_DT),
                   np.array(op_rows, OP_DT) if op_rows else np.zeros(0, OP_DT),
                   len(self.actors), len(self.reg_list), len(self.obj_list), flags, remap)
        if self.keep_log:
            lc = self.log_changes.copy()
            ld = self.log_deps.copy()
            if remap is not None:
                lc["actor"] = remap[lc["actor"]]
                ld["actor"] = remap[ld["actor"]]
            nc = a.changes.copy()
            nc["dep_off"] += len(ld)
            nc["op_first"] += len(self.log_ops)
            self.log_changes = np.concatenate([lc, nc])
            self.log_deps = np.concatenate([ld, a.deps])
            self.log_ops = np.concatenate([self.log_ops, a.ops])
        return a

    def log_batch(self, a_stride: int) -> Batch:
        """The document's whole log as a one-document batch (oracle / rendering)."""
        doc = np.zeros(1, DOC_DT)
        d = doc[0]
        d["n_changes"], d["n_deps"], d["n_ops"] = len(self.log_changes), len(self.log_deps), len(self.log_ops)
        d["n_regs"], d["n_objs"], d["n_actors"], d["flags"] = len(self.reg_list), len(self.obj_list), \
            len(self.actors), self.flags
        return Batch(doc, self.log_changes.copy(), self.log_deps.copy(), self.log_ops.copy(), a_stride, None,
                     self.pool.strings, [list(self.actors)], [list(self.obj_list)], [list(self.reg_list)])


def merge_maps(es: DocEncoder, ed: DocEncoder, S: int):
    """The maps that carry rows of the document encoded by `es` into the document encoded by `ed`
    (hm_merge_maps), interning into `ed` every actor, object, register and content key `es` holds.
    Returns (totals [4] = ed's n_actors, n_regs, n_objs afterwards and es's flags, the rank row [S]
    (NONE beyond es's actors), the object, register and content maps, ed's old rank -> new rank as
    bytes or None when no rank of ed moved).  ed's host log mirror is re-ranked with it."""
    mp = None
    if ed is not es:
        new = set(es.actors) - set(ed.actors)
        if new:
            if len(ed.actors) + len(new) > S:
                raise ValueError(f"{len(ed.actors) + len(new)} actors > a_stride {S}")
            ranked = sorted(set(ed.actors) | new, key=js_key)
            at = {a: r for r, a in enumerate(ranked)}
            m = np.array([at[a] for a in ed.actors], np.uint8)
            if len(m) and not np.array_equal(m, np.arange(len(m), dtype=np.uint8)):
                mp = m
                if ed.keep_log:
                    ed.log_changes, ed.log_deps = ed.log_changes.copy(), ed.log_deps.copy()
                    ed.log_changes["actor"] = mp[ed.log_changes["actor"]]
                    ed.log_deps["actor"] = mp[ed.log_deps["actor"]]
            ed.actors = ranked
    at = {a: r for r, a in enumerate(ed.actors)}
    rank = np.full(S, NONE, np.uint32)
    rank[:len(es.actors)] = [at[a] for a in es.actors]
    om = np.array([ed._obj(u) for u in es.obj_list], np.uint32)
    rm = np.array([ed._reg(int(om[o]), k) for o, k in es.reg_list], np.uint32).reshape(-1)
    cm = np.full(len(es.content), NONE, np.uint32)
    for ck, c in es.content.items():
        j = ed.content.get(ck)
        if j is None:
            j = ed.content[ck] = len(ed.content)
        cm[c] = j
    ed.flags |= es.flags
    return np.array([len(ed.actors), len(ed.reg_list), len(ed.obj_list), es.flags], np.uint32), rank, om, rm, cm, mp


class _StoreConfig(ctypes.Structure):
    _fields_ = [("a_stride", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class _DocInfo(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("n_changes", "n_deps", "n_ops", "n_regs", "n_objs", "n_actors",
                                                "hist_len", "n_queued", "n_surv")] + [("status", ctypes.c_int32)]


def _p(a: Optional[np.ndarray]):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@dataclass
class BatchResult:
    docs: np.ndarray            # DOC_RESULT_DT per batch row
    clock: np.ndarray           # [n, S] opSet.clock
    back_clock: np.ndarray      # [n, S] DocBackend.clock
    heads: np.ndarray           # [n, S] opSet.deps


class _MergeMaps(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in ("totals", "rank", "obj_off", "obj_map", "reg_off", "reg_map",
                                                "str_off", "str_map", "content_off", "content_map")]


@dataclass
class MergeMaps:
    """hm_merge_maps: per request the destination's totals after the merge and the maps from the
    source's id spaces into the destination's."""
    totals: np.ndarray                         # [n, 4] n_actors, n_regs, n_objs, flags
    rank: np.ndarray                           # [n, S] source rank -> destination rank
    objs: Sequence[np.ndarray]                 # per request: source object id -> destination object id
    regs: Sequence[np.ndarray]
    strs: Optional[Sequence[np.ndarray]] = None      # None: identity
    content: Optional[Sequence[np.ndarray]] = None

    def c_struct(self, n: int, S: int):
        """(the ctypes struct, the arrays it points into); built once per (n, S): a caller that merges with the
        same maps again pays no second flattening"""
        made = getattr(self, "_made", None)
        if made is not None and made[0] == (n, S):
            return made[1], made[2]

        def csr(parts):
            if parts is None:
                return None, None
            assert len(parts) == n
            off = np.zeros(n + 1, np.uint32)
            np.cumsum([len(p) for p in parts], out=off[1:])
            flat = np.concatenate([np.asarray(p, np.uint32) for p in parts]) if n else np.zeros(0, np.uint32)
            return off, np.ascontiguousarray(flat if len(flat) else np.zeros(1, np.uint32), np.uint32)
        tot = np.ascontiguousarray(self.totals, np.uint32).reshape(n, 4)
        rank = np.ascontiguousarray(self.rank, np.uint32).reshape(n, S)
        keep = [tot, rank]
        for parts in (self.objs, self.regs, self.strs, self.content):
            keep.extend(csr(parts))
        self._made = ((n, S), _MergeMaps(*[None if a is None else a.ctypes.data for a in keep]), keep)
        return self._made[1], self._made[2]


class DocStore:
    """Device-resident documents of one repo (one GPU)."""

    def __init__(self, engine: Engine, a_stride: int = 8) -> None:
        L = lib()
        self._L, self.engine, self.S = L, engine, a_stride
        h = ctypes.c_void_p()
        engine._check(L.hm_store_create(engine._h, ctypes.byref(_StoreConfig(a_stride, 0)), ctypes.byref(h)),
                      "hm_store_create")
        self._h = h
        self.pool = StringPool()
        self.enc: List[DocEncoder] = []
        self._pending = None

    def close(self) -> None:
        if getattr(self, "_h", None):
            if getattr(self.engine, "_h", None):               # (the store lives on its engine's stream)
                self._L.hm_store_destroy(self._h)
            self._h = None

    def __del__(self):
        # (at interpreter exit finalizers run in any order: the engine may be gone, and the
        # process releases the device anyway)
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int, what: str) -> None:
        self.engine._check(st, what)

    def set_incremental(self, on) -> None:
        """Incremental applyRemoteChanges on the resident state (default on); off = every submit
        re-merges each touched document's whole log; 2 = also small list documents (no cost
        policy).  Results are identical."""
        mode = 2 if on == 2 else int(bool(on))
        self._check(self._L.hm_store_set_incremental(self._h, mode), "hm_store_set_incremental")

    def last_routing(self) -> Dict[str, int]:
        """How the last submit's documents were merged: incremental / re-merged / handed back."""
        out = np.zeros(3, np.uint32)
        self._check(self._L.hm_store_last_routing(self._h, _p(out)), "hm_store_last_routing")
        return {"incremental": int(out[0]), "remerged": int(out[1]), "handed_back": int(out[2])}

    def inc_states(self) -> int:
        """Documents whose resident incremental state a submit can use (hm_store_inc_states)."""
        out = np.zeros(1, np.uint32)
        self._check(self._L.hm_store_inc_states(self._h, _p(out)), "hm_store_inc_states")
        return int(out[0])

    def arena(self) -> Dict[str, List[int]]:
        """The four row arenas (changes, deps, ops, registers): capacities and bump pointers in
        rows (hm_store_arena_info).  free = cap - used is what a submit's growth must fit."""
        cap, used = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
        self._check(self._L.hm_store_arena_info(self._h, _p(cap), _p(used)), "hm_store_arena_info")
        return {"cap": [int(x) for x in cap], "used": [int(x) for x in used]}

    def last_kernel_ms(self) -> Dict[str, float]:
        """Device time of the last submit (HIP events): the incremental kernels and the re-merge."""
        out = np.zeros(2, np.float32)
        self._check(self._L.hm_store_last_kernel_ms(self._h, _p(out)), "hm_store_last_kernel_ms")
        return {"incremental_ms": float(out[0]), "remerge_ms": float(out[1])}

    def open(self) -> int:
        h = ctypes.c_uint32()
        self._check(self._L.hm_doc_open(self._h, ctypes.byref(h)), "hm_doc_open")
        assert h.value == len(self.enc)
        self.enc.append(DocEncoder(self.pool))
        return h.value

    def reset(self, handles) -> None:
        """hm_doc_reset: the handles become empty documents again (their rows are dead space
        until the store compacts)."""
        hs = np.ascontiguousarray(handles, np.uint32)
        self._check(self._L.hm_doc_reset(self._h, _p(hs), len(hs)), "hm_doc_reset")
        for h in hs:
            if h < len(self.enc):
                self.enc[h] = DocEncoder(self.pool)

    # -- applyChanges over many documents -----------------------------------------------------
    def submit(self, items: Sequence[Tuple[int, Sequence[Dict[str, Any]]]],
               extra_actors: Optional[Dict[int, Sequence[str]]] = None) -> int:
        """items: (handle, changes) per document (each handle once)."""
        S = self.S
        appends, snaps = [], []
        for h, changes in items:
            e = self.enc[h]
            snaps.append(e.snapshot())
            a = e.encode(changes, (extra_actors or {}).get(h, ()))
            if a.n_actors > S:
                for (hh, _), sn in zip(items, snaps):
                    self.enc[hh].restore(sn)
                raise EngineError(f"document {h} has {a.n_actors} actors > store a_stride {S}")
            appends.append(a)
        return self._submit_rows([h for h, _ in items], appends, snaps)

    def _submit_rows(self, handles: List[int], appends: List[Append], snaps) -> int:
        S = self.S
        n = len(handles)
        docs = np.zeros(n, DOC_DT)
        chs, dps, ops = [], [], []
        nc = nd = no = 0
        remap = None
        for i, a in enumerate(appends):
            d = docs[i]
            d["change_off"], d["n_changes"], d["dep_off"], d["n_deps"] = nc, len(a.changes), nd, len(a.deps)
            d["op_off"], d["n_ops"] = no, len(a.ops)
            d["n_regs"], d["n_objs"], d["n_actors"], d["flags"] = a.n_regs, a.n_objs, a.n_actors, a.flags
            c = a.changes.copy()
            c["dep_off"] += nd
            c["op_first"] += no
            chs.append(c); dps.append(a.deps); ops.append(a.ops)
            nc += len(a.changes); nd += len(a.deps); no += len(a.ops)
            if a.remap is not None:
                if remap is None:
                    remap = np.tile(np.arange(S, dtype=np.uint8), (n, 1))
                remap[i, :len(a.remap)] = a.remap
        ch = np.concatenate(chs) if chs else np.zeros(0, CHANGE_DT)
        dp = np.concatenate(dps) if dps else np.zeros(0, DEP_DT)
        op = np.concatenate(ops) if ops else np.zeros(0, OP_DT)
        hs = np.array(handles, np.uint32)
        keep = (docs, ch, dp, op, hs, remap)
        cb = CBatch(n, len(ch), len(dp), len(op), int(docs["n_regs"].sum()) if n else 0, S, 0, 0, 0, 0, 0, 0,
                    docs.ctypes.data, ch.ctypes.data, dp.ctypes.data, op.ctypes.data, None)
        bid = ctypes.c_uint64()
        self._check(self._L.hm_batch_submit(self._h, ctypes.byref(cb), _p(hs), _p(remap), ctypes.byref(bid)),
                    "hm_batch_submit")
        self._pending = (bid.value, handles, snaps, keep)
        return bid.value

    def wait(self) -> BatchResult:
        bid, handles, snaps, _ = self._pending
        self._pending = None
        n, S = len(handles), self.S
        r = BatchResult(np.zeros(n, DOC_RESULT_DT), np.zeros((n, S), np.uint32), np.zeros((n, S), np.uint32),
                        np.zeros((n, S), np.uint32))
        self._check(self._L.hm_batch_wait(self._h, ctypes.c_uint64(bid), _p(r.docs), _p(r.clock),
                                          _p(r.back_clock), _p(r.heads)), "hm_batch_wait")
        for i, h in enumerate(handles):          # rolled-back documents: the interner rolls back too
            if r.docs[i]["status"] != 0:
                self.enc[h].restore(snaps[i])
        src, self._forked = getattr(self, "_forked", None), None
        if src is not None:                      # a fork batch: the forks' encoders are their parents', cloned
            self._clone_encoders(src, handles, r.docs["status"])
        if getattr(self, "_merged", False):      # a merge batch: the destinations' host logs follow the device's
            self._merged = False
            self._refresh_logs(handles, r.docs["status"])
        return r

    def apply(self, items, extra_actors=None) -> BatchResult:
        self.submit(items, extra_actors)
        return self.wait()

    # -- reads -------------------------------------------------------------------------------
    def info(self, h: int) -> Dict[str, int]:
        i = _DocInfo()
        self._check(self._L.hm_doc_info(self._h, h, ctypes.byref(i)), "hm_doc_info")
        return {f: getattr(i, f) for f, _ in _DocInfo._fields_}

    def read(self, h: int) -> Tuple[Batch, Results]:
        """The document's log and merged state as a one-document (Batch, Results); the Batch is
        None for a store fed prebuilt rows (RowStore: no host encoder keeps the log)."""
        inf = self.info(h)
        S = self.S
        b = self.enc[h].log_batch(S) if h < len(self.enc) else None
        r = Results(np.zeros(1, DOC_RESULT_DT), np.zeros(S, np.uint32), np.zeros(S, np.uint32),
                    np.zeros(S, np.uint32), np.zeros(inf["n_changes"], np.int32),
                    np.zeros(inf["n_changes"] * S, np.uint32), np.zeros(inf["n_regs"], REG_RESULT_DT),
                    np.zeros(inf["n_ops"], SURV_RESULT_DT))
        self._check(self._L.hm_doc_read(self._h, h, _p(r.hist), _p(r.all_deps), _p(r.regs), _p(r.surv),
                                        _p(r.clock), _p(r.back_clock), _p(r.heads)), "hm_doc_read")
        d = r.docs[0]
        d["status"], d["hist_len"], d["n_queued"], d["n_surv"] = inf["status"], inf["hist_len"], inf["n_queued"], \
            inf["n_surv"]
        d["err_change"] = d["err_op"] = NONE
        r.surv[inf["n_surv"]:] = 0
        return b, r

    def log(self, h: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        inf = self.info(h)
        c = np.zeros(inf["n_changes"], CHANGE_DT)
        d = np.zeros(inf["n_deps"], DEP_DT)
        o = np.zeros(inf["n_ops"], OP_DT)
        self._check(self._L.hm_doc_log(self._h, h, _p(c), _p(d), _p(o)), "hm_doc_log")
        return c, d, o

    def history_prefix(self, h: int, n: int) -> List[int]:
        out = np.zeros(max(n, 1), np.uint32)
        k = self._L.hm_doc_history_prefix(self._h, h, n, _p(out))
        if k < 0:
            self._check(k, "hm_doc_history_prefix")
        return [int(x) for x in out[:k]]

    # -- what blocked documents wait for (getMissingDeps); all read the rounds already waited for ----
    def blocked(self) -> np.ndarray:
        """Handles of the documents that hold queued changes, ascending (hm_store_blocked)."""
        n = ctypes.c_uint32()
        out = np.zeros(1024, np.uint32)
        st = self._L.hm_store_blocked(self._h, _p(out), len(out), ctypes.byref(n))
        if st == 34:                                  # HM_ERR_NOMEM: n = the count needed
            out = np.zeros(n.value, np.uint32)
            st = self._L.hm_store_blocked(self._h, _p(out), len(out), ctypes.byref(n))
        self._check(st, "hm_store_blocked")
        return out[:n.value].copy()

    def waiting(self, handles) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(missing [n, S], unmet_min [n, S], n_queued [n]) of the listed documents: per actor rank
        the largest seq a queued change needs and opSet.clock lacks, the minimumClock entries
        DocBackend.clock has not reached, and the queue length (hm_store_waiting)."""
        hs = np.ascontiguousarray(handles, np.uint32)
        n = len(hs)
        miss = np.zeros((n, self.S), np.uint32)
        unmet = np.zeros((n, self.S), np.uint32)
        nq = np.zeros(n, np.uint32)
        self._check(self._L.hm_store_waiting(self._h, n, _p(hs), _p(miss), _p(unmet), _p(nq)), "hm_store_waiting")
        return miss, unmet, nq

    def queues(self, handles, n_queued) -> Tuple[np.ndarray, np.ndarray]:
        """opSet.queue of the listed documents as log indices in queue order: (offsets [n + 1],
        indices); n_queued from waiting() (hm_store_read_queue)."""
        hs = np.ascontiguousarray(handles, np.uint32)
        off = np.zeros(len(hs) + 1, np.uint32)
        np.cumsum(np.asarray(n_queued, np.uint32), out=off[1:])
        out = np.zeros(max(int(off[-1]), 1), np.uint32)
        self._check(self._L.hm_store_read_queue(self._h, len(hs), _p(hs), _p(off), _p(out)), "hm_store_read_queue")
        return off, out[:int(off[-1])]

    def queue(self, h: int) -> List[int]:
        """opSet.queue of one document (log indices, queue order)."""
        _, _, nq = self.waiting([h])
        return [int(x) for x in self.queues([h], nq)[1]]

    def missing_deps(self, h: int) -> Dict[str, int]:
        """Backend.getMissingDeps of one document: {actorId: seq}."""
        miss, _, _ = self.waiting([h])
        actors = self.enc[h].actors
        return {actors[a]: int(s) for a, s in enumerate(miss[0]) if s}

    # -- what a peer lacks (getMissingChanges / getChanges / getChangesForActor) ----------------------
    def missing_changes_rows(self, handles, have, flags: int = 0) -> Tuple[List[List[int]], np.ndarray]:
        """hm_store_missing_changes over rank entries: `have` as engine.pack_entries takes it.
        Returns (per request the log indices in history order, the [n, S] transitiveDeps rows)."""
        hs = np.ascontiguousarray(handles, np.uint32)
        n = len(hs)
        off, ea, es = pack_entries(have, n)
        rng = np.zeros((max(n, 1), 2), np.uint32)
        clo = np.zeros((max(n, 1), self.S), np.uint32)
        tot = ctypes.c_uint32()
        cap = 4096
        out = np.zeros(cap, np.uint32)
        args = (self._h, n, _p(hs), _p(off), _p(ea), _p(es), flags, _p(clo), _p(rng))
        st = self._L.hm_store_missing_changes(*args, _p(out), cap, ctypes.byref(tot))
        if st == 34 and tot.value > cap:              # HM_ERR_NOMEM: tot = the rows needed
            cap = tot.value
            out = np.zeros(cap, np.uint32)
            st = self._L.hm_store_missing_changes(*args, _p(out), cap, ctypes.byref(tot))
        self._check(st, "hm_store_missing_changes")
        return [[int(x) for x in out[int(o):int(o) + int(c)]] for o, c in rng[:n]], clo[:n]

    def missing_changes(self, handles, clocks, flags: int = 0) -> List[List[int]]:
        """Backend.getMissingChanges of many documents in one call: clocks[i] is the peer's
        {actorId: seq} for document handles[i], read in its insertion order (the answer depends on
        it when the clock is not causally closed); an actor the document has never seen names none
        of its changes and is dropped.  Per request the log indices, in history order, of the
        applied changes the peer lacks."""
        have = []
        for h, clock in zip(handles, clocks):
            rank = {a: i for i, a in enumerate(self.enc[h].actors)}
            have.append([(rank[a], q) for a, q in clock.items() if a in rank])
        return self.missing_changes_rows(handles, have, flags)[0]

    def changes_since(self, h: int, clock: Dict[str, int]) -> List[int]:
        """getMissingChanges of one document (getChanges(old, new) with old's opSet.clock)."""
        return self.missing_changes([h], [clock])[0]

    def changes_for_actor(self, h: int, actor: str, after: int = 0) -> List[int]:
        """Backend.getChangesForActor: the actor's applied changes with seq > after, history order."""
        return self.missing_changes([h], [{actor: after}], MC_RAW | MC_ONLY_LISTED)[0]

    # -- the fields a proposed change touches (undo bookkeeping of applyLocalChange) ------------------
    def fields_rows(self, handles, have, fields, cap: Optional[int] = None):
        """hm_store_fields over rank entries and registers: `have` as engine.pack_entries takes it
        (the would-be change's deps in key order with its own actor at seq - 1), fields: per request
        a sequence of registers.  Returns (per request (ready, [FIELD_OP_DT rows of each field, winner
        first]), the [n, S] transitiveDeps rows)."""
        hs = np.ascontiguousarray(handles, np.uint32)
        n = len(hs)
        off, ea, es = pack_entries(have, n)
        foff, freg = pack_fields(fields, n)
        nf = int(foff[-1])
        flags = np.zeros(max(n, 1), np.uint32)
        rng = np.zeros((nf + 1, 2), np.uint32)
        clo = np.zeros((max(n, 1), self.S), np.uint32)
        tot = ctypes.c_uint32()
        grow, cap = cap is None, max(64, 2 * nf) if cap is None else cap
        rows = np.zeros(max(cap, 1), FIELD_OP_DT)
        args = (self._h, n, _p(hs), _p(off), _p(ea), _p(es), _p(foff), _p(freg), _p(flags), _p(clo), _p(rng))
        st = self._L.hm_store_fields(*args, _p(rows), cap, ctypes.byref(tot))
        if grow and st == 34 and tot.value > cap:     # HM_ERR_NOMEM: tot = the rows needed
            cap = tot.value
            rows = np.zeros(cap, FIELD_OP_DT)
            st = self._L.hm_store_fields(*args, _p(rows), cap, ctypes.byref(tot))
        self._check(st, "hm_store_fields")
        return unpack_fields(n, foff, flags, rng, rows), clo[:n]

    def fields(self, handles, clocks, fields):
        """The fields proposed changes touch, many requests per call: clocks[i] is the would-be
        change's base clock {actorId: seq} for document handles[i] (base = {...deps}; base[actor] =
        seq - 1), read in its insertion order; fields[i] a sequence of registers, each a number or
        an (object uuid, key) pair (looked up, never interned: an unknown one is an empty field).  An actor the document
        has never seen is dropped when its seq is 0 and makes the request not ready otherwise.  Per
        request (ready, [per field its current ops, winner first, as dicts of op / action / datatype /
        vtag / value / actor (id) / seq / covered])."""
        have, sent, late = [], [], set()
        for j, (h, clock) in enumerate(zip(handles, clocks)):
            rank = {a: i for i, a in enumerate(self.enc[h].actors)}
            if any(a not in rank and q > 0 for a, q in clock.items()):
                late.add(j)
                continue
            have.append([(rank[a], q) for a, q in clock.items() if a in rank])
            sent.append(j)
        def reg_of(h, f):
            if isinstance(f, tuple):
                enc = self.enc[h]
                o = enc.objs.get(f[0])
                return 0xFFFFFFFF if o is None else enc.regs.get((o, f[1]), 0xFFFFFFFF)
            return f
        regs = [[reg_of(handles[j], f) for f in fields[j]] for j in sent]
        got, _ = self.fields_rows([handles[j] for j in sent], have, regs) if sent else ([], None)
        out = [(False, [[] for _ in fields[j]]) for j in range(len(handles))]
        for j, (ready, fl) in zip(sent, got):
            actors = self.enc[handles[j]].actors
            out[j] = (ready, [[dict(op=int(r["op"]), action=int(r["action"]), datatype=int(r["datatype"]), vtag=int(r["vtag"]),
                                    value=int(r["value"]), actor=actors[int(r["actor"])], seq=int(r["seq"]),
                                    covered=bool(r["covered"])) for r in f] for f in fl])
        return out

    # -- a document as it was (MaterializeMsg / loadDocument at a clock) ------------------------------
    def _selector(self, hs: np.ndarray, history, clocks):
        n = len(hs)
        if (history is None) == (clocks is None):
            return None, None                          # (the library refuses it: HM_ERR_INVALID)
        if history is not None:
            hl = np.ascontiguousarray(np.minimum(np.asarray(history, np.int64), 0xFFFFFFFF), np.uint32)
            assert hl.shape == (n,), hl.shape
            return hl, None
        if isinstance(clocks, np.ndarray):
            rows = np.ascontiguousarray(clocks, np.uint32)
        else:                                          # {actorId: seq} per request (ids the document never saw: dropped)
            rows = np.zeros((n, self.S), np.uint32)
            for i, (h, clock) in enumerate(zip(hs, clocks)):
                if h >= len(self.enc):                 # (a RowStore keeps no actor tables: rank rows there)
                    raise EngineError(f"clocks by actor id need the document's host encoder (handle {int(h)} has none): "
                                      "pass [n, a_stride] rank rows")
                rank = {a: r for r, a in enumerate(self.enc[h].actors)}
                for a, q in clock.items():
                    if a in rank:
                        rows[i, rank[a]] = min(max(int(q), 0), 0xFFFFFFFF)
        assert rows.shape == (n, self.S), rows.shape
        return None, rows

    def past_sizes(self, handles, history=None, clocks=None) -> Tuple[np.ndarray, np.ndarray]:
        """hm_store_past_sizes: ([n, 4] changes / deps / ops / registers per request, their [4] totals) of
        the documents `handles` as they were at history length history[i] or at the clock clocks[i]
        (an [n, S] array of rank-indexed rows, or {actorId: seq} per request)."""
        hs = np.ascontiguousarray(handles, np.uint32)
        n = len(hs)
        hl, rows = self._selector(hs, history, clocks)
        cnt = np.zeros((max(n, 1), 4), np.uint32)
        tot = np.zeros(4, np.uint64)
        self._check(self._L.hm_store_past_sizes(self._h, n, _p(hs), _p(hl), _p(rows), _p(cnt), _p(tot)),
                    "hm_store_past_sizes")
        return cnt[:n], tot

    def materialize(self, handles, history=None, clocks=None) -> Tuple[Batch, Results, np.ndarray, np.ndarray]:
        """hm_store_materialize: the documents `handles` (a handle may repeat) as they were at history
        length history[i] (clamped, as history.slice(0, n) clamps) or at the clock clocks[i]: the
        applied changes selected, gathered on the device in history order into a cold batch (request
        i = document i) and merged from Backend.init().  Returns (the gathered Batch, its Results,
        change_log, op_log): change_log[j] / op_log[k] = the document-local log index of gathered
        change j / op k.  The resident documents are only read.  (The sizes are asked first, to allocate
        the tables: a caller that keeps buffers calls hm_store_materialize with its capacities.)"""
        hs = np.ascontiguousarray(handles, np.uint32)
        n, S = len(hs), self.S
        hl, rows = self._selector(hs, history, clocks)
        _, tot = self.past_sizes(hs, hl, rows) if (hl is not None or rows is not None) else (None, np.zeros(4, np.uint64))
        nc, nd, no, nr = (int(x) for x in tot)
        b = Batch(np.zeros(n, DOC_DT), np.zeros(nc, CHANGE_DT), np.zeros(nd, DEP_DT), np.zeros(no, OP_DT), S)
        r = Results(np.zeros(n, DOC_RESULT_DT), np.zeros(n * S, np.uint32), np.zeros(n * S, np.uint32),
                    np.zeros(n * S, np.uint32), np.zeros(nc, np.int32), np.zeros(nc * S, np.uint32),
                    np.zeros(nr, REG_RESULT_DT), np.zeros(no, SURV_RESULT_DT))
        clog, olog = np.zeros(nc, np.uint32), np.zeros(no, np.uint32)
        out = CPastOut(nc, nd, no, nr, b.docs.ctypes.data, b.changes.ctypes.data, b.deps.ctypes.data, b.ops.ctypes.data,
                       clog.ctypes.data, olog.ctypes.data, r.c_struct())
        self._check(self._L.hm_store_materialize(self._h, n, _p(hs), _p(hl), _p(rows), ctypes.byref(out), None),
                    "hm_store_materialize")
        return b, r, clog, olog

    # -- a document as it was, kept: Repo.fork / Repo.merge into a fresh document ----------------------
    def _open_forks(self, n: int) -> List[int]:
        return [self.open() for _ in range(n)]

    def _order_rows(self, hs: np.ndarray, clocks, order) -> Optional[np.ndarray]:
        """[n, S] rank rows (NONE ends a row) of fork()'s `order`."""
        if order is None:
            return None
        n, S = len(hs), self.S
        if isinstance(order, np.ndarray):
            rows = np.ascontiguousarray(order, np.uint32)
            assert rows.shape == (n, S), rows.shape
            return rows
        if isinstance(order, str):
            assert order == "clock", order
            if clocks is None or isinstance(clocks, np.ndarray):
                raise EngineError("order='clock' reads the key order of {actorId: seq} clocks")
            order = [list(c.keys()) for c in clocks]
        rows = np.full((n, S), NONE, np.uint32)
        for i, (h, row) in enumerate(zip(hs, order)):
            rank = {a: r for r, a in enumerate(self.enc[h].actors)} if h < len(self.enc) else {}
            k = 0
            for a in row:
                if isinstance(a, str):
                    if a not in rank:                  # (an id the parent never saw names no change)
                        continue
                    a = rank[a]
                if k >= S:
                    raise EngineError(f"request {i}: more than a_stride {S} actors in the order")
                rows[i, k] = int(a)
                k += 1
        return rows

    def fork_submit(self, handles, history=None, clocks=None, order=None, min_clock=False, into=None) -> Tuple[List[int], int]:
        """hm_store_fork_submit: (the forks' handles, the batch id); wait() returns one row per fork.
        into: empty documents to fork into (default: newly opened ones)."""
        hs = np.ascontiguousarray(handles, np.uint32)
        n = len(hs)
        hl, rows = self._selector(hs, history, clocks)
        orow = self._order_rows(hs, clocks, order)
        new = self._open_forks(n) if into is None else [int(h) for h in into]
        dst = np.array(new, np.uint32)
        assert len(dst) == n
        bid = ctypes.c_uint64()
        self._check(self._L.hm_store_fork_submit(self._h, n, _p(hs), _p(hl), _p(rows), _p(orow), _p(dst),
                                                 1 if min_clock else 0, ctypes.byref(bid)), "hm_store_fork_submit")
        snaps = [self.enc[h].snapshot() if h < len(self.enc) else None for h in new]
        self._pending = (bid.value, new, snaps, (hs, hl, rows, orow, dst))
        self._forked = [int(h) for h in hs]
        return new, bid.value

    def fork(self, handles, history=None, clocks=None, order=None, min_clock=False) -> List[int]:
        """New resident documents: document handles[i] (a handle may repeat) as it was at history
        length history[i] or at the clock clocks[i] (materialize's selectors), indistinguishable from
        a fresh document that received the selected changes in one applyChanges round — in the
        parent's history order (order=None), or actor after actor, each actor's seqs ascending
        (a clock only): order = 'clock' (the {actorId: seq} clocks' own key order, what Repo.merge
        hands over), per request a sequence of actor ids or ranks, or [n, S] rank rows ending in NONE.
        min_clock: the forks get their parent's minimumClock.  The forks keep the parent's id spaces;
        their host encoders are the parents', cloned, so they take later submits.  Returns the new
        handles; the batch's result rows are left in self.fork_result."""
        new, _ = self.fork_submit(handles, history, clocks, order, min_clock)
        self.fork_result = self.wait()
        return new

    def _clone_encoders(self, src: List[int], dst: List[int], status) -> None:
        for p, h, st in zip(src, dst, status):
            if st != 0 or p >= len(self.enc) or h >= len(self.enc):
                continue
            e, f = self.enc[p], DocEncoder(self.pool, self.enc[p].keep_log)
            f.actors, f.objs, f.obj_list = list(e.actors), dict(e.objs), list(e.obj_list)
            f.regs, f.reg_list, f.content, f.flags = dict(e.regs), list(e.reg_list), dict(e.content), e.flags
            if f.keep_log:                             # (the host mirror of the log, for rendering and the oracle)
                f.log_changes, f.log_deps, f.log_ops = self.log(h)
            self.enc[h] = f

    # -- Repo.merge into a document that already holds changes -----------------------------------------
    def _merge_rows(self, dst, src, rows, have, orow, maps: "MergeMaps", remap) -> int:
        """hm_store_merge_from_submit over rank rows and explicit maps; returns the batch id."""
        hs, ds = np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(dst, np.uint32)
        n, S = len(hs), self.S
        assert len(ds) == n
        u32 = lambda a, shape: None if a is None else np.ascontiguousarray(a, np.uint32).reshape(shape)
        rows, have, orow = u32(rows, (n, S)), u32(have, (n, S)), u32(orow, (n, S))
        remap = None if remap is None else np.ascontiguousarray(remap, np.uint8).reshape(n, S)
        cm, keep = maps.c_struct(n, S)
        bid = ctypes.c_uint64()
        self._check(self._L.hm_store_merge_from_submit(self._h, n, _p(hs), _p(have), _p(rows), _p(orow), _p(ds),
                                                       ctypes.byref(cm), _p(remap), ctypes.byref(bid)),
                    "hm_store_merge_from_submit")
        self._merge_keep = (hs, ds, rows, have, orow, remap, cm, keep)
        return bid.value

    def merge_from_submit(self, dst, src, clocks, have=None, order="clock") -> int:
        """merge_from without the wait (wait() returns one row per request); returns the batch id."""
        hs, ds = np.ascontiguousarray(src, np.uint32), [int(h) for h in dst]
        n, S = len(hs), self.S
        _, rows = self._selector(hs, None, clocks)
        orow = self._order_rows(hs, clocks, order)
        snaps, done = [], []
        try:
            totals, rank = np.zeros((n, 4), np.uint32), np.full((n, S), NONE, np.uint32)
            objs, regs, cids, hv = [], [], [], np.zeros((n, S), np.uint32)
            remap = None
            for i, (p, h) in enumerate(zip(hs, ds)):
                if h >= len(self.enc) or p >= len(self.enc):
                    raise EngineError(f"request {i}: merge_from needs both documents' host encoders")
                es, ed = self.enc[p], self.enc[h]
                snaps.append(ed.snapshot())
                done.append(h)
                if have is None:                                   # DocBackend.clock of the destination, in source ranks
                    back = np.zeros(S, np.uint32)
                    self._check(self._L.hm_doc_read(self._h, h, None, None, None, None, None, _p(back), None), "hm_doc_read")
                    was = {a: r for r, a in enumerate(ed.actors)}
                    for r, a in enumerate(es.actors):
                        if a in was:
                            hv[i, r] = back[was[a]]
                else:
                    hv[i] = have[i]
                try:
                    totals[i], rank[i], om, rm, cm, mp = merge_maps(es, ed, S)
                except ValueError as e:
                    raise EngineError(f"document {h}: {e}")
                if mp is not None:
                    if remap is None:
                        remap = np.tile(np.arange(S, dtype=np.uint8), (n, 1))
                    remap[i, :len(mp)] = mp
                objs.append(om); regs.append(rm); cids.append(cm)
            bid = self._merge_rows(ds, hs, rows, hv, orow, MergeMaps(totals, rank, objs, regs, None, cids), remap)
        except Exception:
            for h, sn in zip(reversed(done), reversed(snaps)):
                self.enc[h].restore(sn)
            raise
        self._pending = (bid, ds, snaps, self._merge_keep)
        self._merged = True
        return bid

    def merge_from(self, dst, src, clocks, have=None, order="clock") -> BatchResult:
        """Repo.merge(target, source) for resident documents, many per call: document dst[i] is handed
        the changes of document src[i] (only read; may repeat) that are applied there with
        have[a] < seq <= clocks[i][a] — in the clock's key order, actor after actor (order='clock', what
        syncReadyActors does), in another actor order (see fork), or in the source's history order
        (order=None).  clocks: {actorId: seq} per request or [n, S] rows in the source's ranks.  have
        ([n, S], source ranks) defaults to the destination's DocBackend.clock row: what it was handed
        before.  The rows go from the source's resident log to the destination's on the device, renamed
        through maps built here from the two host encoders; the destination is re-ranked when a new actor
        sorts before one of its own; content ids are mapped by the change's canonical content key (actor
        and seq included), so a change the destination already holds keeps its id.

        Deviation: every actor, object, register and content key of the SOURCE is interned into the
        destination's encoder, not only those of the selected rows (deps and links may name any), so
        the destination's totals can grow past what the handed changes mention.  A merge that throws
        rolls the destination and its encoder back.  Returns wait()'s rows: the destinations' whole logs."""
        self.merge_from_submit(dst, src, clocks, have, order)
        return self.wait()

    def _refresh_logs(self, handles, status) -> None:
        for h, st in zip(handles, status):
            if st == 0 and h < len(self.enc) and self.enc[h].keep_log:
                e = self.enc[h]
                e.log_changes, e.log_deps, e.log_ops = self.log(h)

    def op_diff_sizes(self, handles, frm, to, lists=False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """hm_store_op_diff_sizes: ([n, 2] diff rows / survivor rows per request, flags [n], their [2] totals).
        lists=True: the sizes of op_diffs(..., lists=True)."""
        hs, f, t = (np.ascontiguousarray(x, np.uint32) for x in (handles, frm, to))
        n = len(hs)
        assert len(f) == n and len(t) == n
        cnt, fl, tot = np.zeros((max(n, 1), 2), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(2, np.uint64)
        self._check(self._L.hm_store_op_diff_sizes_ex(self._h, n, _p(hs), _p(f), _p(t), _p(cnt), _p(fl), _p(tot), 1 if lists else 0),
                    "hm_store_op_diff_sizes")
        return cnt[:n], fl[:n], tot

    def op_diffs(self, handles, frm, to, cap=None, lists=False, once=False):
        """hm_store_op_diffs: what each applied op of the history slices [frm[i], to[i]) of the documents
        `handles` (a handle may repeat) did: per make op a create row, per assign on a map / table
        register the register as it stands after that op.  Returns (rows OP_DIFF_DT, survivors
        SURV_RESULT_DT, ranges [n, 2] = first row and rows per request, flags [n]); a request flagged
        OD_LISTS (its range assigns list / text elements) has no rows and is replayed on the host.
        cap = (rows, survivors) the tables hold; None: the sizes are asked first.
        lists=True (hm_store_op_diffs_ex with HM_ODF_LISTS): list / text element assigns are answered
        as OD_ELEM_INSERT / OD_ELEM_SET / OD_ELEM_REMOVE rows, nothing is flagged, and the rows' index
        table ([rows] u32: the element's index at the moment of the op, NONE for the other rows) is
        returned as a fifth element.
        once=True (HM_ODF_ONCE): one walk, no sizes asked first: cap (None: a row per request) is a
        guess, and the call is repeated once with the sizes it reports when the guess was too small.
        A request's rows then lie at ranges[i] in a block of their own (blocks in any order, gaps
        between them), the tables returned are as long as the call's totals."""
        from .engine import COpDiffOut, OP_DIFF_DT
        hs, f, t = (np.ascontiguousarray(x, np.uint32) for x in (handles, frm, to))
        n = len(hs)
        assert len(f) == n and len(t) == n
        if cap is None:
            cap = (n, n) if once else tuple(int(x) for x in self.op_diff_sizes(hs, f, t, lists)[2]) if n else (0, 0)
        opts = (1 if lists else 0) | (2 if once else 0)
        for attempt in range(2):
            rows, surv = np.zeros(max(cap[0], 1), OP_DIFF_DT), np.zeros(max(cap[1], 1), SURV_RESULT_DT)
            rng, fl = np.zeros((max(n, 1), 2), np.uint32), np.zeros(max(n, 1), np.uint32)
            tot, index = np.zeros(2, np.uint64), np.zeros(max(cap[0], 1), np.uint32)
            out = COpDiffOut(cap[0], cap[1], rows.ctypes.data, surv.ctypes.data, rng.ctypes.data, fl.ctypes.data)
            st = self._L.hm_store_op_diffs_ex(self._h, n, _p(hs), _p(f), _p(t), ctypes.byref(out),
                                              _p(index) if lists else None, _p(tot), opts)
            if not (once and st == 34 and attempt == 0 and (int(tot[0]) > cap[0] or int(tot[1]) > cap[1])):
                break
            cap = (int(tot[0]), int(tot[1]))                  # HM_ERR_NOMEM: the sizes are known now
        self._check(st, "hm_store_op_diffs")
        base = (rows[:int(tot[0])], surv[:int(tot[1])], rng[:n], fl[:n])
        return base + (index[:int(tot[0])],) if lists else base

    def op_diff_sizes_at(self, handles, clocks, lists=False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """hm_store_op_diff_sizes_at: op_diff_sizes for op_diffs_at's requests."""
        hs = np.ascontiguousarray(handles, np.uint32)
        n = len(hs)
        _, rows = self._selector(hs, None, clocks)
        cnt, fl, tot = np.zeros((max(n, 1), 2), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(2, np.uint64)
        self._check(self._L.hm_store_op_diff_sizes_at(self._h, n, _p(hs), _p(rows), _p(cnt), _p(fl), _p(tot), 1 if lists else 0),
                    "hm_store_op_diff_sizes_at")
        return cnt[:n], fl[:n], tot

    def op_diffs_at(self, handles, clocks, cap=None, lists=False):
        """hm_store_op_diffs_at: the per-op patch of the documents `handles` (a handle may repeat) as they
        stood at the clocks clocks[i] (an [n, S] array of rank-indexed rows, or {actorId: seq} per
        request, as materialize takes them): what each op of the changes applied at that clock did,
        from the empty document, in the resident history order.  Returns what op_diffs returns (with
        lists=True the index table as a fifth element).  cap = (rows, survivors) the tables hold; None:
        the sizes are asked first."""
        from .engine import COpDiffOut, OP_DIFF_DT
        hs = np.ascontiguousarray(handles, np.uint32)
        n = len(hs)
        _, crow = self._selector(hs, None, clocks)
        if cap is None:
            cap = tuple(int(x) for x in self.op_diff_sizes_at(hs, crow, lists)[2]) if n else (0, 0)
        rows, surv = np.zeros(max(cap[0], 1), OP_DIFF_DT), np.zeros(max(cap[1], 1), SURV_RESULT_DT)
        rng, fl = np.zeros((max(n, 1), 2), np.uint32), np.zeros(max(n, 1), np.uint32)
        tot, index = np.zeros(2, np.uint64), np.zeros(max(cap[0], 1), np.uint32)
        out = COpDiffOut(cap[0], cap[1], rows.ctypes.data, surv.ctypes.data, rng.ctypes.data, fl.ctypes.data)
        self._check(self._L.hm_store_op_diffs_at(self._h, n, _p(hs), _p(crow), ctypes.byref(out),
                                                 _p(index) if lists else None, _p(tot), 1 if lists else 0), "hm_store_op_diffs_at")
        base = (rows[:int(tot[0])], surv[:int(tot[1])], rng[:n], fl[:n])
        return base + (index[:int(tot[0])],) if lists else base

    def state_sizes(self, handles) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """hm_store_state_sizes: ([n, 2] state rows / survivor rows per request, flags [n], their [2] totals)."""
        hs = np.ascontiguousarray(handles, np.uint32)
        n = len(hs)
        cnt, fl, tot = np.zeros((max(n, 1), 2), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(2, np.uint64)
        self._check(self._L.hm_store_state_sizes(self._h, n, _p(hs), _p(cnt), _p(fl), _p(tot)), "hm_store_state_sizes")
        return cnt[:n], fl[:n], tot

    def state(self, handles, cap=None, clocks=False):
        """hm_store_state: what the documents `handles` (a handle may repeat) hold now, in one device
        call: per live register (n_surv > 0, obj known) one STATE_ROW_DT row in ascending register id,
        request after request, and the survivors in row order (winner first).  Returns (rows, survivors
        SURV_RESULT_DT, ranges [n, 4] = first row, rows, first survivor, survivors per request, flags
        [n]); a request flagged ST_BAD_ROWS has no rows.  cap = (rows, survivors) the tables hold; None:
        the sizes are asked first.  clocks=True: the requests' opSet.clock and opSet.deps rows
        ([n, a_stride] each) as a fifth and sixth element."""
        from .engine import CStateOut, STATE_ROW_DT
        hs = np.ascontiguousarray(handles, np.uint32)
        n = len(hs)
        if cap is None:
            cap = tuple(int(x) for x in self.state_sizes(hs)[2]) if n else (0, 0)
        rows, surv = np.zeros(max(cap[0], 1), STATE_ROW_DT), np.zeros(max(cap[1], 1), SURV_RESULT_DT)
        rng, fl, tot = np.zeros((max(n, 1), 4), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(2, np.uint64)
        ck, hd = np.zeros((max(n, 1), self.S), np.uint32), np.zeros((max(n, 1), self.S), np.uint32)
        out = CStateOut(cap[0], cap[1], rows.ctypes.data, surv.ctypes.data, rng.ctypes.data, fl.ctypes.data)
        self._check(self._L.hm_store_state(self._h, n, _p(hs), ctypes.byref(out), _p(ck) if clocks else None,
                                           _p(hd) if clocks else None, _p(tot)), "hm_store_state")
        base = (rows[:int(tot[0])], surv[:int(tot[1])], rng[:n], fl[:n])
        return base + (ck[:n], hd[:n]) if clocks else base

    def set_min_clock(self, h: int, clock: Dict[str, int]) -> None:
        """minimumClock (actor id -> seq); its actors must already be in the document's actor table."""
        e = self.enc[h]
        row = np.zeros(self.S, np.uint32)
        rank = {a: i for i, a in enumerate(e.actors)}
        for a, s in clock.items():
            row[rank[a]] = min(int(s), 0xFFFFFFFF)
        self._check(self._L.hm_doc_set_min_clock(self._h, h, _p(row)), "hm_doc_set_min_clock")

    def clock_update(self, handles: Sequence[int]):
        """Batched ClockStore.update(self, doc, doc.clock): (written, differs, stored rows)."""
        n = len(handles)
        hs = np.array(handles, np.uint32)
        w = np.zeros(max(n, 1), np.uint8)
        df = np.zeros(max(n, 1), np.uint8)
        st = np.zeros((max(n, 1), self.S), np.uint32)
        self._check(self._L.hm_store_clock_update(self._h, n, _p(hs), _p(w), _p(df), _p(st)),
                    "hm_store_clock_update")
        return w[:n].astype(bool), df[:n].astype(bool), st[:n]


def slice_changes(b: Batch, lo: np.ndarray, hi: np.ndarray, docs: Optional[np.ndarray] = None) -> Batch:
    """For each document d of `docs` (default: all), its changes lo[d] .. hi[d]-1 (document-local
    arrival indices) with their dep and op rows, as a batch with batch-local offsets.  Document
    totals (n_actors / n_regs / n_objs / flags) are kept: the rows' ids are the batch's own."""
    idx = np.arange(b.n_docs) if docs is None else np.asarray(docs, np.int64)
    drow = b.docs[idx].copy()
    lo = np.asarray(lo, np.int64)[idx]
    cnt = np.asarray(hi, np.int64)[idx] - lo
    cnt = np.maximum(cnt, 0)
    tot = int(cnt.sum())
    excl = np.zeros(len(idx) + 1, np.int64)
    np.cumsum(cnt, out=excl[1:])
    ci = np.repeat(drow["change_off"].astype(np.int64) + lo - excl[:-1], cnt) + np.arange(tot)
    ch = b.changes[ci].copy()

    def rows(first, n, table):
        n = n.astype(np.int64)
        off = np.zeros(len(n) + 1, np.int64)
        np.cumsum(n, out=off[1:])
        ri = np.repeat(first.astype(np.int64) - off[:-1], n) + np.arange(int(off[-1]))
        return table[ri].copy(), off
    dp, doff = rows(ch["dep_off"], ch["n_deps"], b.deps)
    op, ooff = rows(ch["op_first"], ch["n_ops"], b.ops)
    ch["dep_off"] = doff[:-1]
    ch["op_first"] = ooff[:-1]
    drow["change_off"] = excl[:-1]
    drow["n_changes"] = cnt
    drow["dep_off"] = doff[excl[:-1]]
    drow["n_deps"] = doff[excl[1:]] - doff[excl[:-1]]
    drow["op_off"] = ooff[excl[:-1]]
    drow["n_ops"] = ooff[excl[1:]] - ooff[excl[:-1]]
    drow["reg_off"] = 0
    return Batch(drow, ch, dp, op, b.a_stride)


class RowStore(DocStore):
    """Resident documents fed with prebuilt columnar rows (no per-document host encoder): actor
    ranks, register and object ids in the rows are the caller's, stable across submits (e.g. a
    synthetic feed, or rows from hm_decode_blocks over a repo-wide interner)."""

    def open_n(self, n: int) -> int:
        first = ctypes.c_uint32()
        self._check(self._L.hm_doc_open_n(self._h, n, ctypes.byref(first)), "hm_doc_open_n")
        return first.value

    def _open_forks(self, n: int) -> List[int]:
        h0 = self.open_n(n)
        return list(range(h0, h0 + n))

    def fork_submit(self, handles, history=None, clocks=None, order=None, min_clock=False, into=None) -> Tuple[List[int], int]:
        """DocStore.fork_submit over rank rows (clocks [n, S]; order [n, S] or sequences of ranks)."""
        new, bid = super().fork_submit(handles, history, clocks, order, min_clock, into)
        self._pending = (bid, len(new), None, self._pending[3])
        self._forked = None
        return new, bid

    def merge_from_submit(self, dst, src, clocks, maps: MergeMaps, have=None, order=None, remap=None) -> int:
        """hm_store_merge_from_submit with explicit maps: clocks / have [n, S] rows in the sources' ranks,
        order [n, S] rank rows or None (history order), remap [n, S] bytes (the destinations' old rank
        -> new rank) or None.  wait() returns one row per request."""
        bid = self._merge_rows(dst, src, clocks, have, self._order_rows(np.ascontiguousarray(src, np.uint32), None, order),
                               maps, remap)
        self._pending = (bid, len(dst), None, self._merge_keep)
        return bid

    def merge_from(self, dst, src, clocks, maps: MergeMaps, have=None, order=None, remap=None) -> BatchResult:
        self.merge_from_submit(dst, src, clocks, maps, have, order, remap)
        return self.wait()

    def submit_batch(self, b: Batch, handles: np.ndarray) -> int:
        hs = np.ascontiguousarray(handles, np.uint32)
        keep = (b, hs)
        # the store reads the tables and per-document totals only (no launch-size hints)
        cb = CBatch(b.n_docs, len(b.changes), len(b.deps), len(b.ops), 0, b.a_stride, 0, 0, 0, 0, 0, 0,
                    b.docs.ctypes.data, b.changes.ctypes.data, b.deps.ctypes.data, b.ops.ctypes.data, None)
        bid = ctypes.c_uint64()
        self._check(self._L.hm_batch_submit(self._h, ctypes.byref(cb), _p(hs), None, ctypes.byref(bid)),
                    "hm_batch_submit")
        self._pending = (bid.value, len(hs), None, keep)
        return bid.value

    def submit_device(self, n_docs: int, counts, docs, changes, deps, ops, handles) -> int:
        """hm_batch_submit_device: the batch's tables and handles already in HBM (torch tensors or
        device pointers, read in place until wait_device returns); counts = (n_changes, n_deps, n_ops)."""
        ptr = [int(getattr(t, "data_ptr", lambda: t)()) for t in (docs, changes, deps, ops, handles)]
        cb = CBatch(n_docs, int(counts[0]), int(counts[1]), int(counts[2]), 0, self.S, 0, 0, 0, 0, 0, 0,
                    ptr[0], ptr[1], ptr[2], ptr[3], None)
        bid = ctypes.c_uint64()
        self._check(self._L.hm_batch_submit_device(self._h, ctypes.byref(cb), ctypes.c_void_p(ptr[4]), None,
                                                   ctypes.byref(bid)), "hm_batch_submit_device")
        self._pending = (bid.value, n_docs, None, (docs, changes, deps, ops, handles))
        return bid.value

    def wait_device(self, out) -> int:
        """hm_batch_wait_device: the gathered result rows into device memory `out` (a torch tensor of at
        least n * (32 + 12 * a_stride) bytes); returns the number of rows whose status is not OK."""
        bid, n, _, _ = self._pending
        self._pending = None
        nf = ctypes.c_uint32()
        self._check(self._L.hm_batch_wait_device(self._h, ctypes.c_uint64(bid), ctypes.c_void_p(int(out.data_ptr())),
                                                 ctypes.byref(nf)), "hm_batch_wait_device")
        return nf.value

    def wait(self, out: Optional[BatchResult] = None) -> BatchResult:
        """Results of the submitted batch; `out` (arrays of at least the batch's size, e.g. kept
        between rounds by a long-running host) is filled instead of fresh arrays."""
        bid, n, _, _ = self._pending
        self._pending = None
        S = self.S
        if out is not None and len(out.docs) >= n:
            r = BatchResult(out.docs[:n], out.clock[:n], out.back_clock[:n], out.heads[:n])
        else:
            r = BatchResult(np.zeros(n, DOC_RESULT_DT), np.zeros((n, S), np.uint32), np.zeros((n, S), np.uint32),
                            np.zeros((n, S), np.uint32))
        self._check(self._L.hm_batch_wait(self._h, ctypes.c_uint64(bid), _p(r.docs), _p(r.clock),
                                          _p(r.back_clock), _p(r.heads)), "hm_batch_wait")
        return r
