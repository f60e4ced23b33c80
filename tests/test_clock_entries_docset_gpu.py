"""Every docset entry point that takes a clock reads it alike: materialize, materialize_patch(clocks=),
fork, merge_from, missing_changes and fields answer an odd clock — keys in an order that is not the
rank order, actor ids no document has seen, seqs that are fractional, negative, NaN, beyond u32 or above
what the actor has applied — exactly as they answer its normal form, which this file computes by its
own model of the rule: an id the document never saw is dropped, a seq is truncated toward zero, a
non-positive or NaN seq is 0, and seqs stop at 2^32 - 1.  (fields differs in one point, on purpose: an
unseen id with a seq above 0 names a change the document has not applied, so the request is not
ready.)  The answers to normal clocks are checked against the CPU references elsewhere; this file pins
only the equivalence.  Three documents: one in the narrowest class, one whose queued change's deps
intern enough actors for the next class while three actors have changes, one not placed yet."""
import json

import pytest

from hypermerge_amd.docset import ROOT, DocSet

from kat_cases import A, B, Cc, ch, s
from test_materialize_gpu import SHUFFLED

pytestmark = pytest.mark.gpu

FLAVOURS = {"default": {}, "device_diffs": {"device_diffs": True}}
UNSEEN0, UNSEEN3 = "nobody0", "nobody3"
DEPS_ONLY = [f"dep{i}" for i in range(7)]                        # interned by a queued change's deps: seen, nothing applied
WIDE = SHUFFLED + [ch(Cc, 2, {a: 1 for a in DEPS_ONLY}, s("q", 1))]
LOGS = [SHUFFLED, WIDE, []]
SEEN = [{A, B, Cc}, {A, B, Cc, *DEPS_ONLY}, set()]
NAN = float("nan")
ODD = [{B: 2.9, UNSEEN0: 0, Cc: -1, A: 1e12, UNSEEN3: 3},        # (aaaa has applied 3, bbbb 2, cccc 1)
       {DEPS_ONLY[3]: 5, Cc: NAN, UNSEEN3: 3, B: 7, A: 2.9},
       {A: 2.9, UNSEEN3: 3, B: NAN}]
ODD_FIELDS = [{B: 2.9, UNSEEN0: 0, Cc: -1, A: 3.7},
              {A: 1e12, B: NAN, UNSEEN0: 0, DEPS_ONLY[0]: 0.5},
              {UNSEEN0: 0, A: -1, B: NAN}]
FIELDS = [[(ROOT, "x"), (ROOT, "y"), (ROOT, "never")]] * 3
ROW = ("status", "hist_len", "n_queued", "n_surv", "min_cmp", "err_change", "err_op")


def normal(clock, seen):
    def seq(q):
        return min(int(q), 2 ** 32 - 1) if q > 0 else 0          # (NaN > 0 is False)
    return {a: seq(q) for a, q in clock.items() if a in seen}


def blocks(changes):
    return [json.dumps(c, separators=(",", ":")).encode() for c in changes]


def rows(res):
    return [[int(r[f]) for f in ROW] for r in res]


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_every_entry_point_reads_a_clock_alike(engine, flavour):
    ds = DocSet(engine, **FLAVOURS[flavour])
    first = ds.open(3)
    docs = list(range(first, first + 3))
    res, _ = ds.apply(docs[:2], [blocks(l) for l in LOGS[:2]])
    assert (res["status"] == 0).all()
    assert [ds.info(d)["a_stride"] for d in docs] == [8, 16, 0] and ds.info(docs[1])["n_queued"] == 1
    norm = [normal(c, k) for c, k in zip(ODD, SEEN)]
    assert norm == [{B: 2, Cc: 0, A: 4294967295}, {DEPS_ONLY[3]: 5, Cc: 0, B: 7, A: 2}, {}]
    assert [list(c) for c in norm[:2]] == [[B, Cc, A], [DEPS_ONLY[3], Cc, B, A]]     # (the key order is kept)

    assert ds.materialize(docs, clocks=ODD) == ds.materialize(docs, clocks=norm)
    assert ds.materialize_patch(docs, clocks=ODD) == ds.materialize_patch(docs, clocks=norm)
    assert ds.missing_changes(docs, ODD) == ds.missing_changes(docs, norm)

    f_odd, r_odd, js_odd = ds.fork(docs, clocks=ODD)
    f_norm, r_norm, js_norm = ds.fork(docs, clocks=norm)
    assert rows(r_odd) == rows(r_norm) and js_odd == js_norm
    assert [ds.view(d) for d in f_odd] == [ds.view(d) for d in f_norm]
    assert ds.info(f_odd[0])["n_changes"] == 5                   # bbbb 1..2, then aaaa 1..3; nothing of cccc

    # merge_from into fresh destinations per clock: one seeded in the source's class (the device route),
    # one not placed yet and one in the wider class (the host route; the latter's source holds nothing)
    seeds = [SHUFFLED[2:3], [], WIDE]
    answers = []
    for clocks in (ODD, norm):
        d0 = ds.open(3)
        dst = list(range(d0, d0 + 3))
        res, _ = ds.apply([dst[0], dst[2]], [blocks(seeds[0]), blocks(seeds[2])])
        assert (res["status"] == 0).all()
        before = ds.merge_stats()
        res, js = ds.merge_from(dst, docs, clocks)
        after = ds.merge_stats()
        assert (after["device"] - before["device"], after["host"] - before["host"]) == (1, 2)
        answers.append((rows(res), js, [ds.view(d) for d in dst]))
    assert answers[0] == answers[1]
    assert answers[0][0][0][1] == 5                              # (hist_len: the seed and four more changes)

    norm_f = [normal(c, k) for c, k in zip(ODD_FIELDS, SEEN)]
    got = ds.fields(docs, ODD_FIELDS, FIELDS)
    assert got == ds.fields(docs, norm_f, FIELDS)
    assert got[0]["ready"] is True and got[0]["fields"][0] and got[2]["ready"] is True
    late = [dict(c, **{UNSEEN3: 3}) for c in ODD_FIELDS]
    assert [g["ready"] for g in ds.fields(docs, late, FIELDS)] == [False, False, False]
