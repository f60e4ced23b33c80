"""A fork's rows, restated in numpy (test reference only), on tests/past_ref.py's Source / select /
gather: the changes a fork of a document at a clock receives, in the order it receives them.

    history order      past_ref.gather as it stands (the parent's own order)
    actor-major order  Repo.merge hands the new document each listed actor's changes 1 .. clock[actor],
                       actor after actor (src/RepoBackend.ts:213-217 cursors.update + syncReadyActors;
                       loadDocument hands doc.init the same shape)

In actor-major order the caller lists actor ranks in hand-over order.  Actor a contributes its applied
changes with seq 1 .. min(clock[a], opSet.clock[a]); an actor's applied changes are exactly its seqs
1 .. opSet.clock[a], so the output position of a change is base[a] + seq - 1 with base the running sum
over the order row.  That position is dense, as a history position is: the actor-major gather is
past_ref.gather over a Source whose hist holds those positions."""
import numpy as np

from past_ref import Source, gather, select

NONE = 0xFFFFFFFF


def order_ranks(order) -> list:
    """The ranks of an order row: NONE ends it."""
    out = []
    for r in order:
        if int(r) == NONE:
            break
        out.append(int(r))
    return out


def check_order(src: Source, clock, order) -> bool:
    """What the count pass accepts: ranks below n_actors, none twice, every rank with a selected change listed."""
    ranks = order_ranks(order)
    if any(r >= src.n_actors for r in ranks) or len(set(ranks)) != len(ranks):
        return False
    sel = select(src, clock=clock)
    return set(int(a) for a in src.changes["actor"][sel]) <= set(ranks)


def actor_major(src: Source, clock, order) -> Source:
    """src with hist = the actor-major output position of every selected change (-1 elsewhere)."""
    assert check_order(src, clock, order)
    clock = np.asarray(clock, np.int64)
    applied = src.hist >= 0
    have = np.zeros(len(clock), np.int64)                     # opSet.clock, from the applied changes
    np.maximum.at(have, src.changes["actor"][applied].astype(np.int64), src.changes["seq"][applied].astype(np.int64))
    base, run = {}, 0
    for r in order_ranks(order):
        base[r] = run
        run += int(min(clock[r], have[r]))
    pos = np.full(len(src.changes), -1, np.int32)
    for i in select(src, clock=clock):
        c = src.changes[i]
        pos[i] = base[int(c["actor"])] + int(c["seq"]) - 1
    taken = np.sort(pos[pos >= 0])
    assert np.array_equal(taken, np.arange(run)), "positions are dense"
    return src._replace(hist=pos)


def gather_fork(requests, S: int):
    """requests: (Source, prefix | None, clock row | None, order row | None) each; past_ref.gather's
    return: (Batch, change_log, op_log) of the rows the forks receive."""
    plain = []
    for src, prefix, clock, order in requests:
        if order is None:
            plain.append((src, prefix, clock))
        else:
            assert prefix is None and clock is not None
            plain.append((actor_major(src, clock, order), len(src.changes), None))
    return gather(plain, S)
