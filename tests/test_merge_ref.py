"""tests/merge_ref.py pinned on the oracle (CPU only): the destination's log followed by the rows the
restatement says it receives, renamed through store.merge_maps, equals — row for row, and in
``oracle.merge`` — the same Python changes encoded directly by the destination's encoder in its final
id space."""
import numpy as np
import pytest

from hypermerge_amd.columnar import NONE
from hypermerge_amd.store import DocEncoder, StringPool, merge_maps
import oracle.oracle as O

from fuzz_docs import gen_docs
from merge_cases import A, B, HAND, INCONSISTENT, fuzz_pair, one_actor_70, permuted_maps, two_actors_300
from merge_ref import BadMap, Maps, check_order, merged_log, positioned, rename, rows_for, select
from past_ref import gather, source_of

RESULT = ("docs", "clock", "back_clock", "heads", "hist", "all_deps", "regs", "surv")
# seeds of fuzz_docs documents for merge_cases.fuzz_pair; test_fuzz_pairs (this file's restatement alone, no
# GPU) requires that at least FUZZ_MIN_QUALIFY of the pairs select changes through maps that are not the identity
FUZZ_SEEDS = tuple(range(9300, 9340))
FUZZ_MIN_QUALIFY = 30


def clone(e):
    f = DocEncoder(e.pool)
    f.restore(e.snapshot())
    return f


class Pair:
    """One case restated: the two encoders, the source with the oracle's hist, the rank-space rows, the
    maps, the rows the destination receives and its log afterwards."""

    def __init__(self, case, S, es=None, ed0=None):
        """es / ed0: encoders that already hold the two documents (a store's: its string ids), cloned."""
        self.case, self.S = case, S
        if es is None:
            pool = StringPool()
            self.es, self.ed0 = DocEncoder(pool), DocEncoder(pool)
            self.es.encode(case["src"])
            self.ed0.encode(case["dst"])
        else:
            self.es, self.ed0 = clone(es), clone(ed0)
        sb, self.dst_log = self.es.log_batch(S), self.ed0.log_batch(S)
        self.src = source_of(sb, O.merge(sb).hist, 0)
        self.dst_res = O.merge(self.dst_log)
        srank = {a: r for r, a in enumerate(self.es.actors)}
        self.clock, self.have = np.zeros(S, np.uint32), np.zeros(S, np.uint32)
        for a, q in case["clock"].items():
            if a in srank:
                self.clock[srank[a]] = q
        if case["have"] is None:                                  # DocBackend.clock of the destination, in source ranks
            back = self.dst_res.back_clock[:S]
            for r, a in enumerate(self.ed0.actors):
                if a in srank:
                    self.have[srank[a]] = back[r]
        else:
            for a, q in case["have"].items():
                self.have[srank[a]] = q
        self.order = None
        if case["order"] == "clock":
            ranks = [srank[a] for a in case["clock"] if a in srank]
            self.order = np.array(ranks + [NONE] * (S - len(ranks)), np.uint32)
        self.ed = clone(self.ed0)
        totals, rank, om, rm, cm, self.remap = merge_maps(self.es, self.ed, S)
        self.maps = Maps(totals, rank, om, rm, None, cm)
        self.rows = rows_for(self.src, self.clock, self.have, self.order, self.maps, S)
        self.log = merged_log(self.dst_log, self.remap, self.rows)

    def handed(self):
        """The selected changes as Python dicts, in hand-over order."""
        pos = positioned(self.src, self.clock, self.have, self.order).hist
        return [self.case["src"][i] for i in sorted(np.flatnonzero(pos >= 0), key=lambda i: pos[i])]

    def identity_maps(self):
        m = self.maps
        ident = lambda a: np.array_equal(a, np.arange(len(a)))
        return ident(m.objs) and ident(m.regs) and ident(m.rank[:len(self.es.actors)]) and self.remap is None


def pin(case, S=8):
    p = Pair(case, S)
    direct = clone(p.ed)
    direct.encode(p.handed())
    want = direct.log_batch(S)
    for f in ("docs", "changes", "deps", "ops"):
        np.testing.assert_array_equal(getattr(p.log, f), getattr(want, f), err_msg=f"{case['name']}: {f}")
    got, ref = O.merge(p.log), O.merge(want)
    for f in RESULT:
        np.testing.assert_array_equal(getattr(got, f), getattr(ref, f), err_msg=f"{case['name']}: {f}")
    return p, got


@pytest.mark.parametrize("case", HAND, ids=[c["name"] for c in HAND])
@pytest.mark.parametrize("S", [8, 12])
def test_hand_cases(case, S):
    pin(case, S)


def test_hand_case_facts():
    by = {c["name"]: pin(c) for c in HAND}
    p, r = by["repo_merge"]
    assert p.remap is not None and list(p.remap) == [1] and int(r.docs["hist_len"][0]) == 2
    p, r = by["shuffled"]
    assert [(int(c["actor"]), int(c["seq"])) for c in p.rows.changes] == [(1, 1), (1, 2), (0, 1), (0, 2), (0, 3), (2, 1)]
    assert int(r.docs["n_queued"][0]) == 0 and int(r.docs["hist_len"][0]) == 7
    p, r = by["shuffled_history_order"]
    assert [(int(c["actor"]), int(c["seq"])) for c in p.rows.changes] == [(0, 1), (1, 1), (0, 2), (1, 2), (0, 3), (2, 1)]
    p, r = by["text"]
    assert list(p.have[:2]) == [2, 0] and len(p.rows.changes) == 4
    assert int((p.rows.ops["parent"] == 0xFFFFFFFF).sum()) > 0 and not p.identity_maps()
    p, r = by["unblocks"]
    assert int(p.dst_res.docs["n_queued"][0]) == 1 and int(r.docs["n_queued"][0]) == 0
    p, r = by["rehanded"]
    assert sorted(int(x) for x in r.hist) == [-2, -2, 0, 1, 2, 3]
    p, r = by["empty"]
    assert len(p.rows.changes) == 0
    p, r = by["not_closed"]
    assert int(r.docs["n_queued"][0]) == 2
    p, r = pin(INCONSISTENT)
    assert int(r.docs["status"][0]) == 1                            # HM_ERR_INCONSISTENT_SEQ


def test_shapes():
    p, r = pin(one_actor_70())
    assert len(p.rows.changes) == 67 and int(p.have[0]) == 3
    p, r = pin(two_actors_300())
    assert len(p.rows.changes) == 580 and list(p.have[:2]) == [10, 0]
    assert [(int(c["actor"]), int(c["seq"])) for c in p.rows.changes[[0, 289, 290, 579]]] == [(0, 11), (0, 300), (1, 1), (1, 290)]
    p, r = pin(permuted_maps())
    assert len(p.maps.objs) >= 65 and len(p.maps.regs) >= 65 and not p.identity_maps()
    assert sorted(p.maps.objs) != list(p.maps.objs) and len(set(p.maps.objs)) == len(p.maps.objs)


def test_order_check_and_bad_maps():
    p = Pair(HAND[1], 8)
    assert check_order(p.src, p.clock, p.have, p.order)
    assert not check_order(p.src, p.clock, p.have, np.array([0, 1] + [NONE] * 6, np.uint32))      # cccc:1 selected, rank 2 not listed
    lo = p.have.copy()
    lo[2] = 1                                                      # ... unless have takes it out of the selection
    assert check_order(p.src, p.clock, lo, np.array([0, 1] + [NONE] * 6, np.uint32))
    assert len(select(p.src, p.clock, lo)) == 5
    one, _, _ = gather([(positioned(p.src, p.clock, p.have, p.order), len(p.src.changes), None)], 8)
    with pytest.raises(BadMap):
        rename(one, p.maps._replace(regs=p.maps.regs[:2]))
    holed = p.maps.objs.copy()
    holed[0] = NONE
    with pytest.raises(BadMap):
        rename(one, p.maps._replace(objs=holed))


def fuzz_pairs():
    return [fuzz_pair(chs, seed) for chs, seed in zip(gen_docs("default", FUZZ_SEEDS), FUZZ_SEEDS)]


def test_fuzz_pairs():
    qualify = 0
    for case in fuzz_pairs():
        p, r = pin(case)
        qualify += len(p.rows.changes) > 0 and not p.identity_maps()
    assert qualify >= FUZZ_MIN_QUALIFY, qualify
