"""A document as it was, restated in numpy (test reference only): from a document's log rows and its
hist, the cold batch the past kernels must gather and the two index maps.

    prefix n:  the applied changes (hist >= 0) at history positions < min(n, hist_len)
    clock row: the applied changes with seq <= clock[actor rank]
    queued (hist -1) and duplicate (hist -2) changes are never selected

The selected changes are laid out in history order, their dep and op rows behind one another in
that order (dep_off / op_first rewritten to the gathered tables); requests lie in request order.
Register, object and rank ids are the document's own, so a gathered document row keeps the
document's n_regs / n_objs / n_actors / flags.  hist comes from ``oracle.merge`` of the log, never from
the engine."""
from typing import NamedTuple

import numpy as np

from hypermerge_amd.columnar import CHANGE_DT, DEP_DT, DOC_DT, OP_DT, Batch


class Source(NamedTuple):
    """One document's log with document-local dep_off / op_first, its totals and its hist."""
    changes: np.ndarray
    deps: np.ndarray
    ops: np.ndarray
    n_regs: int
    n_objs: int
    n_actors: int
    flags: int
    hist: np.ndarray


def source_of(b: Batch, hist: np.ndarray, d: int = 0) -> Source:
    """Document d of batch b (offsets made document-local) with hist = the oracle's for b."""
    r = b.docs[d]
    c0, nc, d0, nd, o0, no = (int(r[f]) for f in ("change_off", "n_changes", "dep_off", "n_deps", "op_off", "n_ops"))
    ch = b.changes[c0:c0 + nc].copy()
    ch["dep_off"] -= d0
    ch["op_first"] -= o0
    return Source(ch, b.deps[d0:d0 + nd].copy(), b.ops[o0:o0 + no].copy(), int(r["n_regs"]), int(r["n_objs"]),
                  int(r["n_actors"]), int(r["flags"]), np.asarray(hist[c0:c0 + nc], np.int32).copy())


def select(src: Source, prefix=None, clock=None) -> np.ndarray:
    """Log indices of the selected changes, in history order."""
    assert (prefix is None) != (clock is None)
    h = src.hist.astype(np.int64)
    if prefix is not None:
        ok = (h >= 0) & (h < int(prefix))
    else:
        ok = (h >= 0) & (src.changes["seq"].astype(np.int64) <= np.asarray(clock, np.int64)[src.changes["actor"]])
    idx = np.flatnonzero(ok)
    return idx[np.argsort(h[idx], kind="stable")]


def _ranges(first: np.ndarray, count: np.ndarray) -> np.ndarray:
    """first[0] .. first[0] + count[0] - 1, first[1] .. : the rows of consecutive ranges."""
    count = count.astype(np.int64)
    off = np.zeros(len(count) + 1, np.int64)
    np.cumsum(count, out=off[1:])
    return np.repeat(first.astype(np.int64) - off[:-1], count) + np.arange(int(off[-1])), off


def gather(requests, S: int):
    """requests: (Source, prefix | None, clock row | None) each.  Returns (Batch, change_log, op_log):
    the gathered cold batch, the document-local log index of every gathered change and the
    document-local log op index of every gathered op."""
    n = len(requests)
    docs = np.zeros(n, DOC_DT)
    chs, dps, ops, clog, olog = [], [], [], [], []
    nc = nd = no = nr = 0
    for q, (src, prefix, clock) in enumerate(requests):
        sel = select(src, prefix, clock)
        ch = src.changes[sel].copy()
        di, doff = _ranges(ch["dep_off"], ch["n_deps"])
        oi, ooff = _ranges(ch["op_first"], ch["n_ops"])
        ch["dep_off"] = nd + doff[:-1]
        ch["op_first"] = no + ooff[:-1]
        row = docs[q]
        row["change_off"], row["dep_off"], row["op_off"], row["reg_off"] = nc, nd, no, nr
        row["n_changes"], row["n_deps"], row["n_ops"] = len(sel), len(di), len(oi)
        row["n_regs"], row["n_objs"], row["n_actors"], row["flags"] = src.n_regs, src.n_objs, src.n_actors, src.flags
        chs.append(ch); dps.append(src.deps[di]); ops.append(src.ops[oi]); clog.append(sel); olog.append(oi)
        nc += len(sel); nd += len(di); no += len(oi); nr += src.n_regs
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return Batch(docs, cat(chs, CHANGE_DT), cat(dps, DEP_DT), cat(ops, OP_DT), S), cat(clog, np.uint32), cat(olog, np.uint32)


def clock_at(src: Source, S: int, p: int) -> np.ndarray:
    """opSet.clock as it stood when the history had p entries."""
    clock = np.zeros(S, np.uint32)
    for i in select(src, prefix=p):
        clock[int(src.changes[i]["actor"])] = int(src.changes[i]["seq"])
    return clock


def hist_len(src: Source) -> int:
    return int((src.hist >= 0).sum())
