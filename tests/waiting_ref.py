"""Automerge 0.12 getMissingDeps restated over the columnar rows (test reference only).

A queued change (hist == -1) needs every (actor, seq) of deps.set(actor, seq - 1) — causallyReady's
rule, oracle/oracle.c causally_ready — and the missing row holds, per actor rank, the largest
needed seq that opSet.clock has not reached.  Expected values in the tests come from here applied
to ``oracle.merge`` of the same log, never from the engine."""
import numpy as np


def missing_deps(changes, deps, hist, clock, S):
    """rows of one document (changes[i].dep_off indexes `deps`); clock = opSet.clock.
    Returns (missing [S] with 0 = no entry, opSet.queue as ascending log indices)."""
    missing = [0] * S
    queue = []
    for i, c in enumerate(changes):
        if hist[i] != -1:                                  # applied (>= 0) or duplicate no-op (-2)
            continue
        queue.append(i)
        off, n = int(c["dep_off"]), int(c["n_deps"])
        need = {int(d["actor"]): int(d["seq"]) for d in deps[off:off + n]}
        need[int(c["actor"])] = int(c["seq"]) - 1          # overrides an explicit own-actor dep
        for a, s in need.items():
            if int(clock[a]) < s:
                missing[a] = max(missing[a], s)
    return missing, queue


def doc_ref(b, o, d=0):
    """(missing row, queue) of document d of batch b with oracle results o; a document whose merge
    threw has a zero row and no queue."""
    S = b.a_stride
    row = b.docs[d]
    if int(o.docs["status"][d]) != 0:
        return np.zeros(S, np.uint32), []
    c0, n = int(row["change_off"]), int(row["n_changes"])
    m, q = missing_deps(b.changes[c0:c0 + n], b.deps, o.hist[c0:c0 + n], o.clock[d * S:(d + 1) * S], S)
    return np.array(m, np.uint32), q


def unmet_min(back_clock, min_clock):
    """min_clock[a] where DocBackend.clock[a] < min_clock[a], else 0."""
    back_clock = np.asarray(back_clock, np.uint32)
    min_clock = np.asarray(min_clock, np.uint32)
    return np.where(back_clock < min_clock, min_clock, 0).astype(np.uint32)
