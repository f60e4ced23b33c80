"""A merge into a live document, restated in numpy (test reference only), on tests/past_ref.py's
Source / gather and tests/fork_ref.py's order rows: the rows a destination receives from a source
(Repo.merge = cursors.update + syncReadyActors, src/RepoBackend.ts:213-217), renamed into the
destination's id spaces, and the destination's log afterwards.

    selection   the source's applied changes with have[a] < seq <= clock[a] (source ranks)
    positions   history order: the source's own, restricted to the selection;
                actor-major: base[a] + seq - have[a] - 1, base = the running sum over the order row of
                max(0, min(clock[a], opSet.clock[a]) - have[a]) — dense, since an actor's applied changes are
                exactly its seqs 1 .. opSet.clock[a]
    rename      change: actor through rank, content_id through content; dep: actor through rank;
                op: obj through objs, reg (unless NONE: make*) and parent (unless HEAD) through regs,
                key (set / del / link / inc) through strs, value through strs (V_STR) or objs (V_OBJ);
                elem and everything else stay; the doc row takes the destination's totals, flags OR-ed
    log         the destination's rows (ranks through its remap) followed by the renamed rows

A map that does not cover an id met (short slice, a NONE entry, an image beyond the totals) is BadMap:
the call is refused."""
from typing import NamedTuple, Optional

import numpy as np

from hypermerge_amd.columnar import HEAD, NONE, SET, V_OBJ, V_STR, Batch

from fork_ref import order_ranks
from past_ref import Source, gather


class Maps(NamedTuple):
    totals: np.ndarray                # n_actors, n_regs, n_objs, flags of the destination after the merge
    rank: np.ndarray                  # [S] source rank -> destination rank (NONE: no such source rank)
    objs: np.ndarray
    regs: np.ndarray
    strs: Optional[np.ndarray] = None
    content: Optional[np.ndarray] = None


class BadMap(Exception):
    pass


def opset_clock(src: Source, S: int) -> np.ndarray:
    clock = np.zeros(S, np.int64)
    ok = src.hist >= 0
    np.maximum.at(clock, src.changes["actor"][ok].astype(np.int64), src.changes["seq"][ok].astype(np.int64))
    return clock


def select(src: Source, clock, have) -> np.ndarray:
    """Log indices of the selected changes (any order)."""
    a, q = src.changes["actor"].astype(np.int64), src.changes["seq"].astype(np.int64)
    lo = np.zeros(len(clock), np.int64) if have is None else np.asarray(have, np.int64)
    return np.flatnonzero((src.hist >= 0) & (q > lo[a]) & (q <= np.asarray(clock, np.int64)[a]))


def check_order(src: Source, clock, have, order) -> bool:
    ranks = order_ranks(order)
    if any(r >= src.n_actors for r in ranks) or len(set(ranks)) != len(ranks):
        return False
    return set(int(a) for a in src.changes["actor"][select(src, clock, have)]) <= set(ranks)


def positioned(src: Source, clock, have, order) -> Source:
    """src with hist = every selected change's output position (-1 elsewhere)."""
    sel = select(src, clock, have)
    pos = np.full(len(src.changes), -1, np.int32)
    if order is None:
        pos[sel] = src.hist[sel]
        return src._replace(hist=pos)
    assert check_order(src, clock, have, order)
    S = len(clock)
    lo = np.zeros(S, np.int64) if have is None else np.asarray(have, np.int64)
    top = np.minimum(np.asarray(clock, np.int64), opset_clock(src, S))
    base, run = {}, 0
    for r in order_ranks(order):
        base[r] = run
        run += int(max(0, top[r] - lo[r]))
    for i in sel:
        c = src.changes[i]
        pos[i] = base[int(c["actor"])] + int(c["seq"]) - int(lo[int(c["actor"])]) - 1
    assert np.array_equal(np.sort(pos[pos >= 0]), np.arange(run)), "positions are dense"
    return src._replace(hist=pos)


def _through(m, ids, limit=None):
    """ids through the map m (None: identity); BadMap for an id beyond it, a NONE entry, an image >= limit."""
    ids = np.asarray(ids, np.int64)
    if m is None:
        return ids
    m = np.asarray(m, np.int64)
    if len(ids) and int(ids.max()) >= len(m):
        raise BadMap("an id beyond its slice")
    out = m[ids]
    if (out == NONE).any() or (limit is not None and (out >= limit).any()):
        raise BadMap("an entry of NONE, or an image beyond the totals")
    return out


def rename(b: Batch, maps: Maps) -> Batch:
    """A one-document gathered batch carried into the destination's id spaces."""
    na, nr, nob, fl = (int(x) for x in maps.totals)
    ch, dp, op, docs = b.changes.copy(), b.deps.copy(), b.ops.copy(), b.docs.copy()
    ch["actor"] = _through(maps.rank, ch["actor"], na)
    ch["content_id"] = _through(maps.content, ch["content_id"])
    dp["actor"] = _through(maps.rank, dp["actor"], na)
    op["obj"] = _through(maps.objs, op["obj"], nob)
    k = op["reg"] != NONE
    op["reg"][k] = _through(maps.regs, op["reg"][k], nr)
    k = op["parent"] != HEAD
    op["parent"][k] = _through(maps.regs, op["parent"][k], nr)
    k = op["action"] >= SET
    op["key"][k] = _through(maps.strs, op["key"][k])
    k = op["vtag"] == V_STR
    op["value"][k] = _through(maps.strs, op["value"][k])
    k = op["vtag"] == V_OBJ
    op["value"][k] = _through(maps.objs, op["value"][k], nob)
    docs["n_actors"], docs["n_regs"], docs["n_objs"] = na, nr, nob
    docs["flags"] |= fl
    return Batch(docs, ch, dp, op, b.a_stride)


def rows_for(src: Source, clock, have, order, maps: Maps, S: int) -> Batch:
    """The renamed rows one destination receives, as a one-document batch (offsets from 0)."""
    one, _, _ = gather([(positioned(src, clock, have, order), len(src.changes), None)], S)
    return rename(one, maps)


def gathered(requests, S: int) -> Batch:
    """requests: (Source, clock, have | None, order | None, Maps) each: the renamed tables in request order."""
    parts = [rows_for(*r, S) for r in requests]
    docs = np.concatenate([p.docs for p in parts])
    nc = nd = no = 0
    chs = []
    for i, p in enumerate(parts):
        c = p.changes.copy()
        c["dep_off"] += nd
        c["op_first"] += no
        docs[i]["change_off"], docs[i]["dep_off"], docs[i]["op_off"] = nc, nd, no
        chs.append(c)
        nc += len(p.changes); nd += len(p.deps); no += len(p.ops)
    reg_off = np.concatenate([[0], np.cumsum([int(r[0].n_regs) for r in requests])[:-1]])
    docs["reg_off"] = reg_off
    return Batch(docs, np.concatenate(chs), np.concatenate([p.deps for p in parts]), np.concatenate([p.ops for p in parts]), S)


def merged_log(dst: Batch, remap, rows: Batch) -> Batch:
    """The destination's log after the merge: its one-document log `dst` (ranks through remap, its old
    rank -> new rank, or None) followed by the renamed rows; totals and flags from the rows' doc row."""
    ch, dp = dst.changes.copy(), dst.deps.copy()
    d0, o0 = int(dst.docs["dep_off"][0]), int(dst.docs["op_off"][0])
    ch["dep_off"] -= d0
    ch["op_first"] -= o0
    if remap is not None:
        m = np.asarray(remap, np.int64)
        ch["actor"], dp["actor"] = m[ch["actor"]], m[dp["actor"]]
    add = rows.changes.copy()
    add["dep_off"] += len(dp)
    add["op_first"] += len(dst.ops)
    docs = rows.docs.copy()
    docs["change_off"] = docs["dep_off"] = docs["op_off"] = docs["reg_off"] = 0
    docs["n_changes"], docs["n_deps"], docs["n_ops"] = len(ch) + len(add), len(dp) + len(rows.deps), len(dst.ops) + len(rows.ops)
    docs["flags"] |= dst.docs["flags"]
    return Batch(docs, np.concatenate([ch, add]), np.concatenate([dp, rows.deps]), np.concatenate([dst.ops, rows.ops]), dst.a_stride)
