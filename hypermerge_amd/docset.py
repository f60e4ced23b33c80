"""ctypes face of the docset (include/hypermerge_amd.h hm_docset_*, csrc/docset.cpp): the
Node drop-in's host engine — raw hypercore blocks of many documents in, one applyChanges round
each (src/DocBackend.ts:169-185), results + patches + DocBackend.clock out as JSON.

Used by the Python tests; the production caller is the N-API addon (js/hmgpu_node.c)."""
from __future__ import annotations

import ctypes
import sys
import json
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .columnar import DOC_RESULT_DT
from .decode import pack_offsets
from .engine import Engine, lib

NO_PATCHES = 1          # HM_DOCSET_NO_PATCHES
BINARY = 2              # HM_DOCSET_BINARY
NET_DIFFS = 4           # HM_DOCSET_NET_DIFFS
DEVICE_DIFFS = 8        # HM_DOCSET_DEVICE_DIFFS


class _Cfg(ctypes.Structure):
    _fields_ = [("threads", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class _Info(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in ("a_stride", "n_changes", "n_ops", "n_actors", "n_objs", "n_regs",
                                               "hist_len", "n_queued")]


def _text(L, t, raw: bool = False) -> Tuple[Any, np.ndarray]:
    n = ctypes.c_size_t()
    p = L.hm_text_data(t, ctypes.byref(n))
    s = ctypes.string_at(p, n.value) if n.value else b""
    if not raw:
        s = s.decode("utf-8", "surrogatepass")
    k = ctypes.c_uint32()
    rp = L.hm_text_results(t, ctypes.byref(k))
    res = np.zeros(k.value, DOC_RESULT_DT)
    if k.value:
        ctypes.memmove(res.ctypes.data, rp, k.value * DOC_RESULT_DT.itemsize)
    L.hm_text_free(t)
    return s, res


class DocSet:
    def __init__(self, engine: Engine, threads: int = 0, patches: bool = True, net_diffs: bool = False,
                 binary: bool = False, device_diffs: bool = False):
        """binary: results in the HMP1 form the Node host reads (HM_DOCSET_BINARY).  `apply` reads
        JSON only: of a binary docset it reads the calls that fall back to JSON (a string with a
        lone surrogate among the call's patches); `apply_raw` returns either form as bytes.
        device_diffs (HM_DOCSET_DEVICE_DIFFS): every round's per-op diffs are rendered from the
        device's op-diff rows instead of replayed on the host; the same patches."""
        self._L, self.engine = lib(), engine
        h = ctypes.c_void_p()
        cfg = _Cfg(threads, (0 if patches else NO_PATCHES) | (NET_DIFFS if net_diffs else 0) | (BINARY if binary else 0) |
                   (DEVICE_DIFFS if device_diffs else 0))
        engine._check(self._L.hm_docset_create(engine._h, ctypes.byref(cfg), ctypes.byref(h)), "hm_docset_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.engine, "_h", None):               # (its stores live on the engine's stream)
                self._L.hm_docset_destroy(self._h)
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

    def open(self, n: int = 1) -> int:
        first = ctypes.c_uint32()
        self.engine._check(self._L.hm_docset_open(self._h, n, ctypes.byref(first)), "hm_docset_open")
        return first.value

    def apply(self, docs: Sequence[int], blocks: Sequence[Sequence[bytes]]) -> Tuple[np.ndarray, Dict[str, Any]]:
        """One applyChanges round: docs[i] receives blocks[i] (one JSON Change per block).
        Returns (per-document hm_doc_result rows, {"p": [patch|None], "b": [DocBackend.clock|None]})."""
        data, bo, db = pack_offsets(blocks)
        ids = np.ascontiguousarray(docs, np.uint32)
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_apply(self._h, data.ctypes.data, bo.ctypes.data, db.ctypes.data,
                                                   ids.ctypes.data, len(ids), ctypes.byref(t)), "hm_docset_apply")
        s, res = _text(self._L, t)
        return res, json.loads(s)

    def apply_raw(self, docs: Sequence[int], blocks: Sequence[Sequence[bytes]]) -> Tuple[np.ndarray, bytes]:
        """`apply` with the call's text as it came: the JSON's bytes, or the HMP1 words of a binary docset."""
        data, bo, db = pack_offsets(blocks)
        ids = np.ascontiguousarray(docs, np.uint32)
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_apply(self._h, data.ctypes.data, bo.ctypes.data, db.ctypes.data,
                                                   ids.ctypes.data, len(ids), ctypes.byref(t)), "hm_docset_apply")
        s, res = _text(self._L, t, raw=True)
        return res, s

    def info(self, doc: int) -> Dict[str, int]:
        i = _Info()
        self.engine._check(self._L.hm_docset_doc_info(self._h, doc, ctypes.byref(i)), "hm_docset_doc_info")
        return {f: int(getattr(i, f)) for f, _ in _Info._fields_}

    def history_prefix(self, doc: int, n: int) -> List[int]:
        out = np.zeros(max(n, 1), np.uint32)
        k = self._L.hm_docset_history_prefix(self._h, doc, n, out.ctypes.data)
        if k < 0:
            self.engine._check(-k, "hm_docset_history_prefix")
        return [int(x) for x in out[:k]]

    def clock_update(self, docs: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, List[Dict[str, int]]]:
        ids = np.ascontiguousarray(docs, np.uint32)
        w = np.zeros(max(len(ids), 1), np.uint8)
        d = np.zeros(max(len(ids), 1), np.uint8)
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_clock_update(self._h, len(ids), ids.ctypes.data, w.ctypes.data, d.ctypes.data,
                                                          ctypes.byref(t)), "hm_docset_clock_update")
        s, _ = _text(self._L, t)
        return w[:len(ids)], d[:len(ids)], json.loads(s)

    def view(self, doc: int) -> Dict[str, Any]:
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_view(self._h, doc, ctypes.byref(t)), "hm_docset_view")
        s, _ = _text(self._L, t)
        return json.loads(s)

    def views(self, docs: Sequence[int], raw: bool = False):
        """hm_docset_views: what view(doc) returns for every document of `docs` (a document may
        repeat), from one device call per stride class.  raw=True: the call's text as it came (a
        JSON array whose element i is hm_docset_view(docs[i])'s bytes)."""
        ids = np.ascontiguousarray(docs, np.uint32)
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_views(self._h, len(ids), ids.ctypes.data if len(ids) else None, ctypes.byref(t)),
                           "hm_docset_views")
        s, _ = _text(self._L, t, raw=raw)
        return s if raw else json.loads(s)

    def get_patch(self, docs: Sequence[int]) -> List[Dict[str, Any]]:
        """hm_docset_get_patch: Backend.getPatch per document, {"doc", "history", "patch": {"clock",
        "deps", "canUndo": False, "canRedo": False, "diffs"}}: the diffs build the document from an
        empty one (creates, then per object its sets and its inserts)."""
        ids = np.ascontiguousarray(docs, np.uint32)
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_get_patch(self._h, len(ids), ids.ctypes.data if len(ids) else None, ctypes.byref(t)),
                           "hm_docset_get_patch")
        s, _ = _text(self._L, t)
        return json.loads(s)

    def blocked(self) -> List[int]:
        """Documents that hold queued changes (every stride class), ids ascending."""
        n = ctypes.c_uint32()
        out = np.zeros(1024, np.uint32)
        st = self._L.hm_docset_blocked(self._h, out.ctypes.data, len(out), ctypes.byref(n))
        if st == 34:                                  # HM_ERR_NOMEM: n = the count needed
            out = np.zeros(n.value, np.uint32)
            st = self._L.hm_docset_blocked(self._h, out.ctypes.data, len(out), ctypes.byref(n))
        self.engine._check(st, "hm_docset_blocked")
        return [int(x) for x in out[:n.value]]

    def waiting(self, docs: Sequence[int]) -> List[Dict[str, Any]]:
        """Per document {"queued": [log indices in queue order], "missing": {actorId: seq}}
        (Backend.getMissingDeps of the rounds applied so far)."""
        ids = np.ascontiguousarray(docs, np.uint32)
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_waiting(self._h, len(ids), ids.ctypes.data, ctypes.byref(t)),
                           "hm_docset_waiting")
        s, _ = _text(self._L, t)
        return json.loads(s)

    def missing_changes(self, docs: Sequence[int], clocks: Sequence[Dict[str, float]], flags: int = 0) -> List[List[int]]:
        """Backend.getMissingChanges of many documents: clocks[i] is the peer's {actorId: seq} for
        document docs[i], read in its insertion order.  Per request the log indices, in history
        order, of the applied changes that peer lacks (hm_docset_missing_changes)."""
        ids = np.ascontiguousarray(docs, np.uint32)
        assert len(clocks) == len(ids)
        eoff = np.zeros(len(ids) + 1, np.uint32)
        names: List[bytes] = []
        seqs: List[float] = []
        for i, clock in enumerate(clocks):
            for a, q in clock.items():
                names.append(a.encode("utf-8", "surrogatepass"))
                seqs.append(float(q))
            eoff[i + 1] = len(names)
        aoff = np.zeros(len(names) + 1, np.uint32)
        np.cumsum([len(x) for x in names], out=aoff[1:])
        data = np.frombuffer(b"".join(names) + b"\0", np.uint8)
        sq = np.array(seqs + [0.0], np.float64)
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_missing_changes(self._h, len(ids), ids.ctypes.data, eoff.ctypes.data,
                                                             data.ctypes.data, aoff.ctypes.data, sq.ctypes.data, flags,
                                                             ctypes.byref(t)), "hm_docset_missing_changes")
        s, _ = _text(self._L, t)
        return json.loads(s)

    def fields(self, docs: Sequence[int], clocks: Sequence[Dict[str, float]],
               fields: Sequence[Sequence[Tuple[str, str]]]) -> List[Dict[str, Any]]:
        """The fields proposed changes touch (hm_docset_fields): clocks[i] is the would-be change's
        base clock {actorId: seq} for document docs[i] (base = {...deps}; base[actor] = seq - 1), read
        in its insertion order; fields[i] a sequence of (object uuid, key) — an elemId as key for
        list / text.  Per request {"ready": bool, "fields": [[op, ...], ...]}, a field's current ops
        winner first, op = {"action", "value", "datatype"?, "actor", "seq", "covered"}."""
        ids = np.ascontiguousarray(docs, np.uint32)
        assert len(clocks) == len(ids) and len(fields) == len(ids)
        eoff = np.zeros(len(ids) + 1, np.uint32)
        foff = np.zeros(len(ids) + 1, np.uint32)
        actors: List[bytes] = []
        seqs: List[float] = []
        names: List[bytes] = []
        for i, (clock, fl) in enumerate(zip(clocks, fields)):
            for a, q in clock.items():
                actors.append(a.encode("utf-8", "surrogatepass"))
                seqs.append(float(q))
            eoff[i + 1] = len(actors)
            for obj, key in fl:
                names += [obj.encode("utf-8", "surrogatepass"), key.encode("utf-8", "surrogatepass")]
            foff[i + 1] = len(names) // 2
        aoff = np.zeros(len(actors) + 1, np.uint32)
        np.cumsum([len(x) for x in actors], out=aoff[1:])
        noff = np.zeros(len(names) + 1, np.uint32)
        np.cumsum([len(x) for x in names], out=noff[1:])
        adata = np.frombuffer(b"".join(actors) + b"\0", np.uint8)
        ndata = np.frombuffer(b"".join(names) + b"\0", np.uint8)
        sq = np.array(seqs + [0.0], np.float64)
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_fields(self._h, len(ids), ids.ctypes.data, eoff.ctypes.data, adata.ctypes.data,
                                                    aoff.ctypes.data, sq.ctypes.data, foff.ctypes.data, ndata.ctypes.data,
                                                    noff.ctypes.data, ctypes.byref(t)), "hm_docset_fields")
        s, _ = _text(self._L, t)
        return json.loads(s)

    @staticmethod
    def _clock_entries(n: int, clocks: Sequence[Dict[str, float]]):
        """{actorId: seq} per request as the entry tables of hm_docset_materialize(_patch_at)"""
        assert len(clocks) == n
        eoff = np.zeros(n + 1, np.uint32)
        names: List[bytes] = []
        seqs: List[float] = []
        for i, clock in enumerate(clocks):
            for a, q in clock.items():
                names.append(a.encode("utf-8", "surrogatepass"))
                seqs.append(float(q))
            eoff[i + 1] = len(names)
        aoff = np.zeros(len(names) + 1, np.uint32)
        np.cumsum([len(x) for x in names], out=aoff[1:])
        data = np.frombuffer(b"".join(names) + b"\0", np.uint8)
        return eoff, data, aoff, np.array(seqs + [0.0], np.float64)

    def materialize(self, docs: Sequence[int], history: Optional[Sequence[int]] = None,
                    clocks: Optional[Sequence[Dict[str, float]]] = None) -> List[Dict[str, Any]]:
        """Documents as they were (RepoBackend's MaterializeMsg, many per call): docs[i] at history
        length history[i] (history.slice(0, n) replayed from Backend.init()), or at the clock clocks[i]
        ({actorId: seq}: each actor's changes up to that seq).  Per request {"doc", "clock", "deps",
        "history", "view"}, the view as ``view`` gives it (hm_docset_materialize)."""
        ids = np.ascontiguousarray(docs, np.uint32)
        hl = eoff = data = aoff = sq = None
        if history is not None:
            hl = np.ascontiguousarray(np.minimum(np.asarray(history, np.int64), 0xFFFFFFFF), np.uint32)
            assert len(hl) == len(ids)
        if clocks is not None:
            eoff, data, aoff, sq = self._clock_entries(len(ids), clocks)
        p = lambda a: None if a is None else a.ctypes.data
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_materialize(self._h, len(ids), ids.ctypes.data, p(hl), p(eoff), p(data), p(aoff),
                                                         p(sq), ctypes.byref(t)), "hm_docset_materialize")
        s, _ = _text(self._L, t)
        return json.loads(s)

    def materialize_patch(self, docs: Sequence[int], history: Optional[Sequence[int]] = None,
                          clocks: Optional[Sequence[Dict[str, float]]] = None, lists: bool = False) -> List[Dict[str, Any]]:
        """The patches of documents as they were (RepoBackend's MaterializeMsg reply, many per call):
        docs[i] at history length history[i].  Per request {"doc", "history", "patch"}: the patch is
        Backend.applyChanges(Backend.init(), history.slice(0, n))'s {clock, deps, canUndo, canRedo, diffs}
        with the per-op diffs read off the resident tables on the device; a prefix that assigns list
        / text elements has "patch": None and "host": True and is replayed by the caller
        (hm_docset_materialize_patch).  lists=True (hm_docset_materialize_patch_ex with HM_ODF_LISTS):
        the element diffs (insert / set / remove at the index of that moment) come from the device too,
        and no document fed through this package has "patch": None.
        clocks instead of history (exactly one of the two): docs[i] at the clock clocks[i] ({actorId:
        seq}, an id the document never saw is dropped), the patch loadDocument sends for a document
        opened at a cursor (hm_docset_materialize_patch_at).  Per request {"doc", "history": the changes
        applied at the clock, "queued": the selected changes that are not, "patch"}; the diffs are in
        the resident history order."""
        ids = np.ascontiguousarray(docs, np.uint32)
        if (history is None) == (clocks is None):
            raise ValueError("materialize_patch takes exactly one of history and clocks")
        if clocks is not None:
            eoff, data, aoff, sq = self._clock_entries(len(ids), clocks)
            t = ctypes.c_void_p()
            self.engine._check(self._L.hm_docset_materialize_patch_at(self._h, len(ids), ids.ctypes.data if len(ids) else None,
                                                                      eoff.ctypes.data, data.ctypes.data, aoff.ctypes.data, sq.ctypes.data,
                                                                      1 if lists else 0, ctypes.byref(t)),
                               "hm_docset_materialize_patch_at")
            s, _ = _text(self._L, t)
            return json.loads(s)
        hl = np.ascontiguousarray(np.minimum(np.asarray(history, np.int64), 0xFFFFFFFF), np.uint32)
        assert len(hl) == len(ids)
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_materialize_patch_ex(self._h, len(ids), ids.ctypes.data if len(ids) else None,
                                                                  hl.ctypes.data if len(ids) else None, 1 if lists else 0, ctypes.byref(t)),
                           "hm_docset_materialize_patch")
        s, _ = _text(self._L, t)
        return json.loads(s)

    def _fork(self, docs, clocks, history):
        ids = np.ascontiguousarray(docs, np.uint32)
        if (history is None) == (clocks is None):
            raise ValueError("fork takes exactly one of history and clocks")
        hl = eoff = data = aoff = sq = None
        if history is not None:
            hl = np.ascontiguousarray(np.minimum(np.asarray(history, np.int64), 0xFFFFFFFF), np.uint32)
            assert len(hl) == len(ids)
        else:
            eoff, data, aoff, sq = self._clock_entries(len(ids), clocks)
        p = lambda a: None if a is None else a.ctypes.data
        first, t = ctypes.c_uint32(), ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_fork(self._h, len(ids), ids.ctypes.data if len(ids) else None, p(hl), p(eoff),
                                                  p(data), p(aoff), p(sq), ctypes.byref(first), ctypes.byref(t)), "hm_docset_fork")
        return list(range(first.value, first.value + len(ids))), t

    def fork(self, docs: Sequence[int], clocks: Optional[Sequence[Dict[str, float]]] = None,
             history: Optional[Sequence[int]] = None) -> Tuple[List[int], np.ndarray, Dict[str, Any]]:
        """Repo.fork / Repo.merge into a fresh document, many per call (hm_docset_fork): new documents
        that are docs[i] (may repeat) at the clock clocks[i] ({actorId: seq}: the changes are handed
        over actor after actor in the clock's key order, an id the parent never saw is dropped) or at
        history length history[i] (in the parent's history order).  Returns (the new documents' ids,
        and what `apply` returns for a first round handing them those changes: the result rows and
        {"p", "b", "c"})."""
        new, t = self._fork(docs, clocks, history)
        s, res = _text(self._L, t)
        return new, res, json.loads(s)

    def fork_raw(self, docs, clocks=None, history=None) -> Tuple[List[int], np.ndarray, bytes]:
        """`fork` with the call's text as it came (the HMP1 words of a binary docset)."""
        new, t = self._fork(docs, clocks, history)
        s, res = _text(self._L, t, raw=True)
        return new, res, s

    def _merge_from(self, dst_docs, src_docs, clocks):
        dst, src = np.ascontiguousarray(dst_docs, np.uint32), np.ascontiguousarray(src_docs, np.uint32)
        if len(dst) != len(src) or len(clocks) != len(dst):
            raise ValueError("merge_from takes one source and one clock per destination")
        eoff, data, aoff, sq = self._clock_entries(len(dst), clocks)
        t = ctypes.c_void_p()
        self.engine._check(self._L.hm_docset_merge_from(self._h, len(dst), dst.ctypes.data if len(dst) else None,
                                                        src.ctypes.data if len(src) else None, eoff.ctypes.data, data.ctypes.data,
                                                        aoff.ctypes.data, sq.ctypes.data, ctypes.byref(t)), "hm_docset_merge_from")
        return t

    def merge_from(self, dst_docs: Sequence[int], src_docs: Sequence[int],
                   clocks: Sequence[Dict[str, float]]) -> Tuple[np.ndarray, Dict[str, Any]]:
        """Repo.merge(target, source) into documents that may already hold changes, many per call
        (hm_docset_merge_from): dst_docs[i] (each once, none a source of the call) is handed
        src_docs[i]'s applied changes above what it was handed before (its DocBackend.clock) up to
        clocks[i] ({actorId: seq}), actor after actor in the clock's key order.  Returns what `apply`
        returns for a round handing the destinations those changes: the result rows and {"p", "b", "c"}
        (one combined patch per destination)."""
        s, res = _text(self._L, self._merge_from(dst_docs, src_docs, clocks))
        return res, json.loads(s)

    def merge_from_raw(self, dst_docs, src_docs, clocks) -> Tuple[np.ndarray, bytes]:
        """`merge_from` with the call's text as it came (the HMP1 words of a binary docset)."""
        s, res = _text(self._L, self._merge_from(dst_docs, src_docs, clocks), raw=True)
        return res, s

    def merge_stats(self) -> Dict[str, int]:
        """hm_docset_merge_stats: merge requests that moved their rows on the device / through the host."""
        out = np.zeros(2, np.uint64)
        self.engine._check(self._L.hm_docset_merge_stats(self._h, out.ctypes.data), "hm_docset_merge_stats")
        return {"device": int(out[0]), "host": int(out[1])}

    def handles(self, a_stride: int) -> Dict[str, int]:
        """hm_docset_handles: handles opened in the a_stride store and released ones awaiting reuse."""
        o, f = ctypes.c_uint32(), ctypes.c_uint32()
        self.engine._check(self._L.hm_docset_handles(self._h, a_stride, ctypes.byref(o), ctypes.byref(f)),
                           "hm_docset_handles")
        return {"opened": o.value, "free": f.value}

    def routing(self) -> Dict[str, int]:
        """hm_docset_routing: document rounds by store route so far."""
        out = np.zeros(3, np.uint64)
        self.engine._check(self._L.hm_docset_routing(self._h, out.ctypes.data), "hm_docset_routing")
        return {"incremental": int(out[0]), "remerged": int(out[1]), "handed_back": int(out[2])}

    def stats(self) -> Dict[str, int]:
        out = np.zeros(8, np.uint64)
        self.engine._check(self._L.hm_docset_stats(self._h, out.ctypes.data), "hm_docset_stats")
        return {"calls": int(out[0]), "docs": int(out[1]), "moves": int(out[2]), "hit_patches": int(out[3]),
                "full_patches": int(out[4]), "op_patches": int(out[5]), "replay_mismatch": int(out[6])}

    def diff_stats(self) -> Dict[str, int]:
        """hm_docset_diff_stats (device_diffs=True): document rounds rendered from device rows, store
        op-diff calls, and the calls among them that were repeated with larger tables."""
        out = np.zeros(4, np.uint64)
        self.engine._check(self._L.hm_docset_diff_stats(self._h, out.ctypes.data), "hm_docset_diff_stats")
        return {"rounds": int(out[0]), "calls": int(out[1]), "repeated": int(out[2])}


# ---- test helpers: the frontend's view of a document rebuilt from patches ----
ROOT = "00000000-0000-0000-0000-000000000000"


def apply_diffs(objects: Dict[str, Dict[str, Any]], diffs: Sequence[Dict[str, Any]]) -> None:
    """Frontend.applyPatch's effect on a document (src/DocFrontend.ts:162-179), restated."""
    for d in diffs:
        if d["action"] == "create":
            objects[d["obj"]] = {"type": d["type"], "keys": {}, "elems": []}
            continue
        o = objects[d["obj"]]
        e = {"value": d.get("value"), "link": bool(d.get("link")), "datatype": d.get("datatype"),
             "conflicts": d.get("conflicts")}
        if d["type"] in ("list", "text"):
            if d["action"] == "insert":
                o["elems"].insert(d["index"], e)
            elif d["action"] == "set":
                o["elems"][d["index"]] = e
            elif d["action"] == "remove":
                del o["elems"][d["index"]]
            else:
                raise ValueError(d)
        elif d["action"] == "set":
            o["keys"][d["key"]] = e
        elif d["action"] == "remove":
            o["keys"].pop(d["key"], None)          # a per-op remove may name an absent key
        else:
            raise ValueError(d)


def render_objects(objects: Dict[str, Dict[str, Any]], uuid: str = ROOT, depth: int = 0) -> Any:
    """The frontend document in hypermerge_amd/render.py's canonical form."""
    from .columnar import js_key
    o = objects.get(uuid)
    if o is None or depth > 64:
        return {"cycle": uuid}

    def val(v, link):
        return render_objects(objects, v, depth + 1) if link else v

    def ent(e):
        r = {"value": val(e["value"], e["link"])}
        if e.get("datatype"):
            r["datatype"] = e["datatype"]
        if e.get("conflicts"):
            r["conflicts"] = [[c["actor"], val(c.get("value"), c.get("link"))] for c in e["conflicts"]]
        return r
    if o["type"] in ("list", "text"):
        return {o["type"]: [ent(e) for e in o["elems"]]}
    keys = sorted(o["keys"], key=js_key)
    return {"table" if o["type"] == "table" else "map": [[k, ent(o["keys"][k])] for k in keys]}


def view_objects(view: Dict[str, Any]) -> Dict[str, Dict[str, Any]]:
    """hm_docset_view's JSON -> the apply_diffs object form."""
    out = {}
    for uuid, ov in view.items():
        conv = lambda e: {"value": e.get("value"), "link": bool(e.get("link")), "datatype": e.get("datatype"),  # noqa: E731
                          "conflicts": e.get("conflicts")}
        out[uuid] = {"type": ov["type"], "keys": {k: conv(e) for k, e in ov["keys"]},
                     "elems": [conv(e) for _, e in ov["elems"]]}
    return out
