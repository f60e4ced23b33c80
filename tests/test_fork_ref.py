"""tests/fork_ref.py (the numpy restatement the fork tests compare the device with) pinned on the CPU
oracle with hand cases: the hand-over order decides the fork's history, a clock that is not causally
closed leaves queued changes, a clock above opSet.clock clamps, an actor at 0 contributes nothing."""
import numpy as np

from hypermerge_amd import synth
from hypermerge_amd.columnar import decode_doc, encode
import oracle.oracle as O

from fork_ref import NONE, actor_major, check_order, gather_fork
from kat_cases import A, B, Cc, D, ch, s
from past_ref import hist_len, select, source_of

S = 8


def row(*ranks):
    r = np.full(S, NONE, np.uint32)
    r[:len(ranks)] = ranks
    return r


def clock(**kw):
    r = np.zeros(S, np.uint32)
    for k, v in kw.items():
        r[int(k[1:])] = v
    return r


def keys(batch, d=0):
    r = batch.docs[d]
    return [(int(c["actor"]), int(c["seq"])) for c in batch.changes[int(r["change_off"]):int(r["change_off"]) + int(r["n_changes"])]]


def one(log):
    b = encode([log], S)
    o = O.merge(b)
    assert int(o.docs["status"][0]) == 0
    return source_of(b, o.hist, 0)


def test_the_order_decides_the_forks_history():
    """Concurrent A:1 {} and B:1 {}; the parent received B:1 first, so its history is B, A.  Handed over
    in the order (A, B) the fork's history is A, B; in history order it is the parent's."""
    src = one([ch(B, 1, {}, s("y", 1)), ch(A, 1, {}, s("x", 1))])
    assert [int(x) for x in src.hist] == [0, 1]                 # B:1 then A:1 (ranks: A = 0, B = 1)
    k = clock(r0=1, r1=1)
    g, clog, _ = gather_fork([(src, None, k, None), (src, None, k, row(0, 1)), (src, None, k, row(1, 0))], S)
    assert keys(g, 0) == [(1, 1), (0, 1)] and keys(g, 1) == [(0, 1), (1, 1)] and keys(g, 2) == [(1, 1), (0, 1)]
    assert [int(x) for x in clog] == [0, 1, 1, 0, 0, 1]
    o = O.merge(g)
    assert not o.docs["status"].any() and not o.docs["n_queued"].any()
    np.testing.assert_array_equal(o.hist, [0, 1, 0, 1, 0, 1])    # every fork applies its rows as handed over
    # ... which is what a fresh document does with those changes in that order
    fresh = O.merge(encode([[ch(A, 1, {}, s("x", 1)), ch(B, 1, {}, s("y", 1))]], S))
    np.testing.assert_array_equal(fresh.hist, [0, 1])
    np.testing.assert_array_equal(fresh.clock, o.clock[S:2 * S])
    # the states agree whatever the order: the same register winners
    for f in ("clock", "heads"):
        a = getattr(o, f).reshape(3, S)
        assert (a == a[0]).all(), f


def test_a_clock_that_is_not_causally_closed_leaves_queued_changes():
    log = [ch(A, 1, {}, s("x", 1)), ch(B, 1, {A: 1}, s("y", 1)), ch(A, 2, {B: 1}, s("x", 2)), ch(B, 2, {A: 2}, s("y", 2)),
           ch(Cc, 1, {A: 2}, s("z", 1))]
    src = one(log)
    g, clog, _ = gather_fork([(src, None, clock(r1=2), row(1)), (src, None, clock(r0=1, r2=1), row(2, 0)),
                              (src, None, clock(r0=1, r2=1), row(0, 2))], S)
    assert keys(g, 0) == [(1, 1), (1, 2)] and keys(g, 1) == [(2, 1), (0, 1)] and keys(g, 2) == [(0, 1), (2, 1)]
    o = O.merge(g)
    assert [int(x) for x in o.docs["n_queued"]] == [2, 1, 1] and [int(x) for x in o.docs["hist_len"]] == [0, 1, 1]
    # handed over first, cccc:1 waits in the queue and aaaa:1 is the history's first entry either way
    np.testing.assert_array_equal(o.hist, [-1, -1, -1, 0, 0, -1])


def test_a_clock_above_the_documents_clamps_and_an_actor_at_zero_gives_nothing():
    log = [ch(A, 1, {}, s("x", 1)), ch(B, 1, {}, s("y", 1)), ch(A, 2, {}, s("x", 2)), ch(Cc, 1, {D: 1}, s("q", 9))]
    src = one(log)                                              # cccc:1 stays queued: never selected
    assert int(src.hist[3]) == -1 and src.n_actors == 4
    k = clock(r0=99, r1=7, r2=5)
    g, clog, _ = gather_fork([(src, None, k, row(1, 2, 0)), (src, None, clock(r0=2), row(1, 0)),
                              (src, None, clock(r0=2), row(0)), (src, None, clock(), row())], S)
    # bbbb's base is 0, cccc (nothing applied: min(5, 0) = 0 rows) leaves aaaa's base at 1
    assert keys(g, 0) == [(1, 1), (0, 1), (0, 2)]
    assert keys(g, 1) == [(0, 1), (0, 2)] and keys(g, 2) == [(0, 1), (0, 2)] and keys(g, 3) == []
    assert [int(x) for x in clog] == [1, 0, 2, 0, 2, 0, 2]
    o = O.merge(g)
    assert [int(x) for x in o.docs["hist_len"]] == [3, 2, 2, 0] and not o.docs["n_queued"].any()
    # the fork keeps the parent's totals
    for f, v in (("n_regs", src.n_regs), ("n_objs", src.n_objs), ("n_actors", src.n_actors), ("flags", src.flags)):
        assert (g.docs[f] == v).all(), f


def test_order_rows_the_count_pass_refuses():
    src = one([ch(A, 1, {}, s("x", 1)), ch(B, 1, {}, s("y", 1))])
    k = clock(r0=1, r1=1)
    assert check_order(src, k, row(0, 1)) and check_order(src, k, row(1, 0))
    assert not check_order(src, k, row(0))                      # bbbb has a selected change and is not listed
    assert not check_order(src, k, row(0, 1, 0))                # a rank twice
    assert not check_order(src, k, row(0, 1, 2))                # a rank the document does not have
    assert check_order(src, clock(r0=1), row(0))                # bbbb at 0 need not be listed
    r = row(0, 1)
    r[3] = 1                                                    # (behind the NONE that ends the row: not read)
    assert check_order(src, k, r)


def test_actor_major_selects_what_history_order_selects():
    """Documents fed out of order with duplicates: at random clocks both orders hold the same changes,
    the actor-major rows lie actor after actor with ascending seqs, and where both replays apply
    everything they reach the same clock and heads."""
    b = synth.generate(synth.config("C5", n_docs=12, arrival=2, shuffle_pct=40, dup_pct=15))
    b = encode([decode_doc(b, i) for i in range(b.n_docs)], S)
    full = O.merge(b)
    assert (full.docs["status"] == 0).all() and (full.hist == -2).any()
    rng = np.random.default_rng(7)
    differs = 0
    for d in range(b.n_docs):
        src = source_of(b, full.hist, d)
        top = full.clock[d * S:(d + 1) * S].astype(np.int64)
        for _ in range(4):
            k = rng.integers(0, top + 2).astype(np.uint32)
            order = rng.permutation(src.n_actors)
            am = actor_major(src, k, row(*order))
            sel_h, sel_a = select(src, clock=k), select(am, prefix=len(src.changes))
            assert sorted(sel_h) == sorted(sel_a)
            ks = [(int(src.changes[i]["actor"]), int(src.changes[i]["seq"])) for i in sel_a]
            want = [(int(a), q) for a in order for q in range(1, int(min(k[a], top[a])) + 1)]
            assert ks == want
            differs += list(sel_h) != list(sel_a)
            g, _, _ = gather_fork([(src, None, k, None), (src, None, k, row(*order))], S)
            o = O.merge(g)
            assert not o.docs["status"].any()
            np.testing.assert_array_equal(o.docs["n_queued"][0], o.docs["n_queued"][1])
            np.testing.assert_array_equal(o.clock[:S], o.clock[S:])
            np.testing.assert_array_equal(o.heads[:S], o.heads[S:])
    assert differs > 10
