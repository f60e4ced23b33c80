"""tests/past_ref.py (the numpy restatement the materialize tests compare the device with) pinned on
the CPU oracle: replaying a gathered prefix from Backend.init() applies every change at once, in
order; the whole history gives the full merge's state; a clock recorded at history length p selects
the prefix p; and one case with its expected rows written out by hand."""
import numpy as np

from hypermerge_amd import synth
from hypermerge_amd.columnar import SET, V_INT, decode_doc, encode
import oracle.oracle as O

from kat_cases import A, B, Cc, D, ch, s
from past_ref import clock_at, gather, hist_len, select, source_of


def shuffled_docs():
    """documents fed out of order with duplicate copies, plus one holding a change that stays queued"""
    b = synth.generate(synth.config("C5", n_docs=6, arrival=2, shuffle_pct=40, dup_pct=15))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    docs.append([ch(B, 1, {A: 1}, s("y", 2)), ch(Cc, 1, {D: 1}, s("q", 9)), ch(A, 1, {}, s("x", 1)),
                 ch(A, 1, {}, s("x", 1)), ch(A, 2, {B: 1}, s("x", 5))])
    return encode(docs, 8)


def test_prefix_replays_in_order_and_whole_history_is_the_full_merge():
    b = shuffled_docs()
    full = O.merge(b)
    assert (full.docs["status"] == 0).all()
    assert (full.hist == -2).any() and (full.hist == -1).any()
    assert int(full.docs["n_queued"][b.n_docs - 1]) == 1
    prefix_replay_property(b, full)


def prefix_replay_property(b, full, every=1):
    """Every document of b (full = the oracle's merge of it): replaying the gathered prefix k from
    Backend.init() applies every change at once and in order, for k = 0, every, 2 * every, ..,
    hist_len and hist_len + 5; the whole history gives the full merge's state."""
    S = b.a_stride
    for d in range(b.n_docs):
        src = source_of(b, full.hist, d)
        H = hist_len(src)
        assert H == int(full.docs["hist_len"][d])
        for k in list(range(0, H, every)) + [H, H + 5]:
            g, clog, olog = gather([(src, k, None)], S)
            o = O.merge(g)
            kk = min(k, H)
            assert int(o.docs["status"][0]) == 0 and int(o.docs["n_queued"][0]) == 0, (d, k)
            assert int(o.docs["hist_len"][0]) == kk == len(clog)
            np.testing.assert_array_equal(o.hist, np.arange(kk))
            assert sorted(int(src.hist[i]) for i in clog) == list(range(kk))
        # k = hist_len (the last iteration clamps to it): the state is the full merge's
        np.testing.assert_array_equal(o.clock, full.clock[d * S:(d + 1) * S])
        np.testing.assert_array_equal(o.heads, full.heads[d * S:(d + 1) * S])
        r0, nr, o0 = int(b.docs["reg_off"][d]), int(b.docs["n_regs"][d]), int(b.docs["op_off"][d])
        assert len(o.regs) == nr
        for g_ in range(nr):
            fr, pr = full.regs[r0 + g_], o.regs[g_]
            assert (int(fr["n_surv"]), int(fr["list_index"]), int(fr["obj"])) == \
                (int(pr["n_surv"]), int(pr["list_index"]), int(pr["obj"])), (d, g_)
            for j in range(int(fr["n_surv"])):
                fs, ps = full.surv[o0 + int(fr["surv_off"]) + j], o.surv[int(pr["surv_off"]) + j]
                assert int(fs["op"]) == int(olog[int(ps["op"])]), (d, g_, j)          # through the op map
                assert (int(fs["vtag"]), int(fs["value"])) == (int(ps["vtag"]), int(ps["value"]))


def test_clock_at_a_history_length_selects_that_prefix():
    b = shuffled_docs()
    S = b.a_stride
    full = O.merge(b)
    for d in range(b.n_docs):
        src = source_of(b, full.hist, d)
        for p in range(hist_len(src) + 1):
            assert list(select(src, clock=clock_at(src, S, p))) == list(select(src, prefix=p)), (d, p)
    # a clock that is not causally closed leaves the replay with a queued change
    src = source_of(b, full.hist, b.n_docs - 1)
    row = np.zeros(S, np.uint32)
    row[1] = 1                                         # bbbb:1 without the aaaa:1 it depends on
    g, clog, _ = gather([(src, None, row)], S)
    assert [int(x) for x in clog] == [0]
    o = O.merge(g)
    assert int(o.docs["n_queued"][0]) == 1 and int(o.docs["hist_len"][0]) == 0


def test_hand_written_rows():
    """log: bbbb:1 (needs aaaa:1), aaaa:1, aaaa:1 again (a duplicate), cccc:1 (needs dddd:1: queued);
    history: aaaa:1, bbbb:1."""
    log = [ch(B, 1, {A: 1}, s("y", 2)), ch(A, 1, {}, s("x", 1), s("z", 3)), ch(A, 1, {}, s("x", 1), s("z", 3)),
           ch(Cc, 1, {D: 1}, s("q", 9))]
    b = encode([log, log[:2]], 8)
    o = O.merge(b)
    assert [int(x) for x in o.hist] == [1, 0, -2, -1, 1, 0]
    one, two = source_of(b, o.hist, 0), source_of(b, o.hist, 1)
    row = np.zeros(8, np.uint32)
    row[0], row[2] = 1, 1                              # aaaa:1 and the queued cccc:1 (not applied: never selected)
    g, clog, olog = gather([(one, 2, None), (two, 1, None), (one, 0, None), (one, None, row)], 8)
    tup = lambda a: [tuple(int(x) if np.ndim(x) == 0 else tuple(int(y) for y in x) for x in r) for r in a]
    assert tup(g.docs) == [(0, 2, 0, 1, 0, 3, 0, 4, 1, 4, 0, (0, 0)),      # regs y, x, z, q; actors a, b, c, d
                           (2, 1, 1, 0, 3, 2, 4, 3, 1, 2, 0, (0, 0)),
                           (3, 0, 1, 0, 5, 0, 7, 4, 1, 4, 0, (0, 0)),
                           (3, 1, 1, 0, 5, 2, 11, 4, 1, 4, 0, (0, 0))]
    cid = [int(c["content_id"]) for c in b.changes]
    #       actor n_deps seq dep_off n_ops op_first content_id
    assert tup(g.changes) == [(0, 0, 1, 0, 2, 0, cid[1]), (1, 1, 1, 0, 1, 2, cid[0]),
                              (0, 0, 1, 1, 2, 3, cid[5]),
                              (0, 0, 1, 1, 2, 5, cid[1])]
    assert tup(g.deps) == [(0, 0, 1)]
    assert [int(x) for x in clog] == [1, 0, 1, 1]
    assert [int(x) for x in olog] == [1, 2, 0, 1, 2, 1, 2]
    assert [(int(r["reg"]), int(r["action"]), int(r["vtag"]), int(r["value"])) for r in g.ops] == \
        [(1, SET, V_INT, 1), (2, SET, V_INT, 3), (0, SET, V_INT, 2), (1, SET, V_INT, 1), (2, SET, V_INT, 3),
         (1, SET, V_INT, 1), (2, SET, V_INT, 3)]
    r = O.merge(g)
    assert [int(x) for x in r.docs["hist_len"]] == [2, 1, 0, 1] and not r.docs["n_queued"].any()
