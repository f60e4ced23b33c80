"""Automerge 0.12 getMissingChanges / getChanges / getChangesForActor restated over the columnar
rows plus the oracle's hist and all_deps (test reference only).

    transitiveDeps(have): deps = {}; for (actor, seq) of have in ITS key order, seq > 0:
        deps = max-merge(deps, states[actor][seq-1].allDeps)   (no such state: nothing merged)
        deps[actor] = seq                                      (set after the merge)
    getMissingChanges(have) = history.filter(c => c.seq > (deps[c.actor] || 0))

states[actor][seq-1] is the applied change (actor, seq): the row i with hist[i] >= 0; its allDeps is
all_deps[i*S : (i+1)*S].  Expected values in the tests come from here applied to ``oracle.merge`` of
the same log (or are written out by hand), never from the engine."""
import numpy as np

RAW, ONLY_LISTED = 1, 2


def closure(changes, hist, all_deps, S, entries):
    """transitiveDeps of the ordered (rank, seq) entries, as a rank-indexed list."""
    state = {(int(c["actor"]), int(c["seq"])): i for i, c in enumerate(changes) if hist[i] >= 0}
    deps = [0] * S
    for a, q in entries:
        if q <= 0:
            continue
        i = state.get((a, q))
        if i is not None:
            row = all_deps[i * S:(i + 1) * S]
            deps = [max(x, int(y)) for x, y in zip(deps, row)]
        deps[a] = q
    return deps


def missing_changes(changes, hist, all_deps, S, entries, flags=0):
    """(log indices of the missing changes in history order, threshold row)."""
    if flags & RAW:
        deps = [0] * S
        for a, q in entries:
            deps[a] = q
    else:
        deps = closure(changes, hist, all_deps, S, entries)
    listed = {a for a, _ in entries}
    out = []
    for i, c in enumerate(changes):
        a = int(c["actor"])
        if hist[i] < 0 or (flags & ONLY_LISTED and a not in listed):
            continue
        if int(c["seq"]) > deps[a]:
            out.append((int(hist[i]), i))
    return [i for _, i in sorted(out)], deps


def doc_ref(b, o, d, entries, flags=0):
    """The same for document d of batch b with oracle results o (a document whose merge threw
    offers nothing)."""
    S = b.a_stride
    row = b.docs[d]
    c0, n = int(row["change_off"]), int(row["n_changes"])
    if int(o.docs["status"][d]) != 0:
        n = 0
    return missing_changes(b.changes[c0:c0 + n], o.hist[c0:c0 + n], o.all_deps[c0 * S:(c0 + n) * S], S, entries, flags)


def clocks_by_history(changes, hist, S):
    """opSet.clock as it stood when the history had p entries, p = 0 .. hist_len: [hist_len + 1][S]."""
    order = sorted((int(hist[i]), i) for i in range(len(changes)) if hist[i] >= 0)
    clock = [0] * S
    out = [list(clock)]
    for _, i in order:
        clock[int(changes[i]["actor"])] = int(changes[i]["seq"])
        out.append(list(clock))
    return out, [i for _, i in order]
