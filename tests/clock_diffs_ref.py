"""The per-op patch of a document as it stood at a clock, restated in numpy and Python (test
reference only).  Inputs are one document's log rows (past_ref.Source) with hist and all_deps from
``oracle.merge`` of the log, never from the engine.

    selected at K   hist >= 0 and seq <= K[actor]                  (past_ref.select with a clock)
    applied at K    selected, and all_deps[c][a] <= K[a] for every rank a: the whole causal past of
                    the change is selected too (all_deps holds seq - 1 in the change's own column)
    queued at K     selected and not applied: what applyChanges(Backend.init(), selected) leaves in
                    opSet.queue

The changes applied at K, in the resident history order, are the history of that applyChanges call.
The diffs are the rule of tests/op_diffs_ref.py / tests/list_diffs_ref.py run over that history from
position 0, every row in range: the same functions over a Source whose hist numbers the applied
changes 0, 1, ... in history order and holds -1 everywhere else.  Rows carry the document's own op
indices."""
from typing import List, NamedTuple, Tuple

import numpy as np

from list_diffs_ref import ListDiffs, list_diffs
from op_diffs_ref import Diffs, op_diffs
from past_ref import Source, clock_at, hist_len


def selected_at(src: Source, clock) -> np.ndarray:
    """mask over the log: the changes a clock selects"""
    k = np.asarray(clock, np.int64)
    return (src.hist >= 0) & (src.changes["seq"].astype(np.int64) <= k[src.changes["actor"]])


def applied_at(src: Source, all_deps, S: int, clock) -> np.ndarray:
    """mask over the log: the changes applied at the clock"""
    ad = np.asarray(all_deps, np.int64).reshape(len(src.changes), S)
    k = np.asarray(clock, np.int64).reshape(1, S)
    return selected_at(src, clock) & (ad <= k).all(axis=1)


def restricted(src: Source, mask: np.ndarray) -> Source:
    """the document with only the masked changes applied, numbered densely in history order"""
    hist = np.full(len(src.hist), -1, np.int32)
    idx = np.flatnonzero(mask)
    idx = idx[np.argsort(src.hist[idx], kind="stable")]
    hist[idx] = np.arange(len(idx), dtype=np.int32)
    return src._replace(hist=hist)


class AtClock(NamedTuple):
    diffs: object          # Diffs (lists=False) or ListDiffs
    applied: int
    queued: int


def clock_diffs(src: Source, all_deps, S: int, clock, lists: bool = False) -> AtClock:
    """lists=False: op_diffs_ref's rows (a document that assigns list elements is flagged LISTS);
    lists=True: list_diffs_ref's rows, the document's HM_DOC_HAS_LISTS taken as set."""
    m = applied_at(src, all_deps, S, clock)
    sub = restricted(src, m)
    n = int(m.sum())
    d = list_diffs(sub, all_deps, S, 0, n) if lists else op_diffs(sub, all_deps, S, 0, n)
    return AtClock(d, n, int(selected_at(src, clock).sum()) - n)


def causal_past(src: Source, all_deps, S: int, ci: int) -> np.ndarray:
    """the clock of applied change ci and everything before it: its all_deps row with its own seq"""
    k = np.asarray(all_deps, np.uint32).reshape(len(src.changes), S)[ci].copy()
    k[int(src.changes[ci]["actor"])] = int(src.changes[ci]["seq"])
    return k


def is_prefix(src: Source, mask: np.ndarray) -> bool:
    """do the masked changes occupy history positions 0 .. count - 1"""
    h = src.hist[mask]
    return len(h) == 0 or int(h.max()) == len(h) - 1


def clocks_of(src: Source, all_deps, S: int, rng, n_past: int = 4, n_cut: int = 4) -> List[Tuple[str, np.ndarray]]:
    """the clocks a document is asked at: prefixes {0, 1, middle, full}, the causal pasts of n_past
    random applied changes (closed, usually no prefix), n_cut cuts (a prefix clock with one or two
    actors' entries lowered: usually not closed)"""
    H = hist_len(src)
    out = [("prefix", clock_at(src, S, p)) for p in sorted({0, min(1, H), H // 2, H})]
    applied = np.flatnonzero(src.hist >= 0)
    if len(applied):
        for ci in rng.choice(applied, size=n_past):
            out.append(("past", causal_past(src, all_deps, S, int(ci))))
        for _ in range(n_cut):
            k = clock_at(src, S, int(rng.integers(H // 2, H + 1)))
            nz = np.flatnonzero(k)
            for a in rng.choice(nz, size=min(len(nz), int(rng.integers(1, 3))), replace=False) if len(nz) else []:
                k[a] = int(rng.integers(0, k[a]))
            out.append(("cut", k))
    return out


def census(requests) -> Tuple[int, int, int]:
    """over (Source, all_deps, S, clock) requests: (requests, those that select a non-empty set with
    nothing queued and are no history prefix, those that leave changes queued)"""
    closed = queued = 0
    for src, ad, S, k in requests:
        m, sel = applied_at(src, ad, S, k), selected_at(src, k)
        q = int(sel.sum()) - int(m.sum())
        queued += q > 0
        closed += q == 0 and m.any() and not is_prefix(src, m)
    return len(requests), closed, queued


def pack(results, lists: bool):
    """AtClock results as the tables the engine returns (op_diffs_ref.pack / list_diffs_ref.pack)"""
    import list_diffs_ref
    import op_diffs_ref
    return (list_diffs_ref.pack if lists else op_diffs_ref.pack)([r.diffs for r in results])


__all__ = ["AtClock", "Diffs", "ListDiffs", "applied_at", "causal_past", "census", "clock_diffs", "clocks_of", "is_prefix", "pack",
           "restricted", "selected_at"]
