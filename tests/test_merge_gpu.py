"""Resident documents merged into documents that already hold changes (hm_store_merge_from_submit: the
past kernels' gather with the have bound, the rename pass, the device-table submit).  Per request the
destination's read(), info() and log() are compared bit for bit with ``oracle.merge`` of the log
tests/merge_ref.py says it holds (pinned on the oracle by tests/test_merge_ref.py)."""
import numpy as np
import pytest

from hypermerge_amd.columnar import NONE
from hypermerge_amd.engine import EngineError
from hypermerge_amd.store import DocEncoder, DocStore, MergeMaps, RowStore, StringPool, merge_maps
import oracle.oracle as O

from kat_cases import A, B, ch, s
from merge_cases import HAND, HAND_BY_NAME, INCONSISTENT, SHUFFLED, Z, case, fuzz_pair, one_actor_70, permuted_maps, two_actors_300
from merge_ref import Maps, rename, rows_for
from past_ref import gather, source_of
from test_materialize_gpu import same_bytes
from test_merge_ref import FUZZ_MIN_QUALIFY, Pair, clone, fuzz_pairs

pytestmark = pytest.mark.gpu

INVALID = 32
READ = ("clock", "back_clock", "heads", "hist", "all_deps", "regs", "surv")
INFO = ("n_changes", "n_deps", "n_ops", "n_regs", "n_objs", "n_actors")


def state(store, h):
    r = store.read(h)[1]
    return [getattr(r, f).tobytes() for f in READ] + [r.docs.tobytes(), store.info(h)] + [x.tobytes() for x in store.log(h)]


def same_as_oracle(store, h, log, what):
    """The document h against the one-document batch `log` and the oracle's merge of it, bit for bit."""
    o = O.merge(log)
    _, r = store.read(h)
    inf = store.info(h)
    assert [inf[f] for f in INFO] == [int(log.docs[f][0]) for f in INFO], what
    assert (inf["status"], inf["hist_len"], inf["n_queued"], inf["n_surv"]) == \
        tuple(int(o.docs[f][0]) for f in ("status", "hist_len", "n_queued", "n_surv")), what
    S, k = store.S, int(o.docs["n_surv"][0])
    for f in ("clock", "back_clock", "heads"):
        same_bytes(getattr(r, f), getattr(o, f)[:S], (what, f))
    for f in ("hist", "all_deps", "regs"):
        same_bytes(getattr(r, f), getattr(o, f), (what, f))
    same_bytes(r.surv[:k], o.surv[:k], (what, "surv"))
    lc, ld, lo = store.log(h)
    same_bytes(lc, log.changes, (what, "log changes"))
    same_bytes(ld, log.deps, (what, "log deps"))
    same_bytes(lo, log.ops, (what, "log ops"))
    return o


def load(store, cases):
    """Every case's two documents, in one apply round; returns (sources, destinations)."""
    hs = [(store.open(), store.open()) for _ in cases]
    res = store.apply([(h, c[k]) for (p, d), c in zip(hs, cases) for h, k in ((p, "src"), (d, "dst"))])
    assert (res.docs["status"] == 0).all()
    return [p for p, _ in hs], [d for _, d in hs]


def merge_and_check(store, cases, srcs, dsts, expect_status=None):
    """One merge_from call over the cases (all of one order kind); every destination against the restatement."""
    S = store.S
    pairs = [Pair(c, S, store.enc[p], store.enc[d]) for c, p, d in zip(cases, srcs, dsts)]
    before = [state(store, d) for d in dsts]
    order = cases[0]["order"]
    assert all(c["order"] == order for c in cases)
    have = None if all(c["have"] is None for c in cases) else np.stack([p.have for p in pairs])
    res = store.merge_from(dsts, srcs, [c["clock"] for c in cases], have=have, order=order)
    for i, (p, d) in enumerate(zip(pairs, dsts)):
        o = O.merge(p.log)
        st = int(o.docs["status"][0])
        assert int(res.docs["status"][i]) == st == (0 if expect_status is None else expect_status[i]), p.case["name"]
        if st:                                                   # thrown: only this destination is rolled back
            assert state(store, d) == before[i], p.case["name"]
            continue
        same_as_oracle(store, d, p.log, p.case["name"])
        for f in ("hist_len", "n_queued", "n_surv"):
            assert int(res.docs[f][i]) == int(o.docs[f][0]), (p.case["name"], f)
        for f in ("clock", "back_clock", "heads"):
            same_bytes(getattr(res, f)[i], getattr(o, f)[:S], (p.case["name"], "result row", f))
        b, _ = store.read(d)                                     # the host encoder follows: it takes later changes
        same_bytes(b.changes, p.log.changes, (p.case["name"], "host log"))
        assert store.enc[d].actors == p.ed.actors and store.enc[d].reg_list == p.ed.reg_list
    return pairs, res


ALL = HAND + [one_actor_70(), two_actors_300(), permuted_maps()]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("S", [8, 12])
def test_hand_cases_and_shapes(engine, S, mode):
    """Every hand case and the wave / tile / map shapes, the actor-major ones in one call; the same bytes
    (the oracle's) whatever the incremental mode."""
    store = DocStore(engine, a_stride=S)
    store.set_incremental(mode)
    major = [c for c in ALL if c["order"] == "clock" and c["have"] is None]
    rest = [c for c in ALL if c not in major]
    srcs, dsts = load(store, major + rest)
    pairs, res = merge_and_check(store, major, srcs[:len(major)], dsts[:len(major)])
    by = {p.case["name"]: (p, i) for i, p in enumerate(pairs)}
    p, i = by["repo_merge"]
    assert list(p.remap) == [1] and store.enc[dsts[i]].actors == [A, B]        # the destination's survivors were re-ranked
    p, i = by["unblocks"]
    assert int(p.dst_res.docs["n_queued"][0]) == 1 and int(res.docs["n_queued"][i]) == 0
    p, i = by["empty"]
    assert len(p.rows.changes) == 0 and int(res.docs["hist_len"][i]) == 3
    p, i = by["two_actors_300"]
    assert len(p.rows.changes) == 580
    p, i = by["permuted_maps"]
    assert len(p.maps.objs) >= 65 and not p.identity_maps()
    for c, p_, d in zip(rest, srcs[len(major):], dsts[len(major):]):
        pr, res = merge_and_check(store, [c], [p_], [d])
        if c["name"] == "rehanded":
            assert sorted(int(x) for x in store.read(d)[1].hist) == [-2, -2, 0, 1, 2, 3]
    # the sources were only read
    for c, p_ in zip(major + rest, srcs):
        b, r = store.read(p_)
        same_as_oracle(store, p_, b, ("source", c["name"]))
    # a merged destination takes later changes like any document
    d = dsts[[c["name"] for c in major].index("repo_merge")]
    r = store.apply([(d, [ch(B, 2, {A: 1}, s("baz", "mine"))])])
    assert int(r.docs["status"][0]) == 0 and int(r.docs["hist_len"][0]) == 3
    b, _ = store.read(d)
    same_as_oracle(store, d, b, "a later change")


def test_history_order_is_materialize_restricted_by_have(engine):
    """In history order the rows a destination receives are materialize()'s for the same clock, without
    the changes at or below have, renamed."""
    store = DocStore(engine, a_stride=8)
    cases = [case("h1", SHUFFLED, [SHUFFLED[2], ch(Z, 1, {}, s("q", 1))], {A: 3, B: 2, "cccc": 1}, order=None),
             case("h2", two_actors_300()["src"], two_actors_300()["dst"], {A: 300, B: 290}, order=None)]
    srcs, dsts = load(store, cases)
    S = store.S
    pairs = [Pair(c, S, store.enc[p], store.enc[d]) for c, p, d in zip(cases, srcs, dsts)]
    rows = np.stack([p.clock for p in pairs])
    mb, mr, _, _ = store.materialize(srcs, clocks=rows)
    n_before = [store.info(d)["n_changes"] for d in dsts]
    merge_and_check(store, cases, srcs, dsts)
    for i, (p, d) in enumerate(zip(pairs, dsts)):
        one = source_of(mb, np.arange(len(mb.changes)), i)        # the materialized rows, already in history order
        keep = one.changes["seq"] > p.have[one.changes["actor"]]
        pos = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        want = rename(gather([(one._replace(hist=pos), len(pos), None)], S)[0], p.maps)
        lc, ld, lo = store.log(d)
        k = n_before[i]
        assert len(lc) - k == int(keep.sum()) > 0
        same_bytes(lo[int(lc[k]["op_first"]):], want.ops, (i, "ops"))
        for f in ("actor", "seq", "n_deps", "n_ops", "content_id"):
            np.testing.assert_array_equal(lc[k:][f], want.changes[f], err_msg=str((i, f)))
        same_bytes(ld[int(lc[k]["dep_off"]):], want.deps, (i, "deps"))
    assert len(pairs[1].rows.changes) == 580


def test_inconsistent_seq_rolls_back_only_its_destination(engine):
    store = DocStore(engine, a_stride=8)
    cases = [HAND_BY_NAME["rehanded"], INCONSISTENT, dict(HAND_BY_NAME["shuffled"], have={})]
    srcs, dsts = load(store, cases)
    enc_before = store.enc[dsts[1]].snapshot()
    merge_and_check(store, cases, srcs, dsts, expect_status=[0, 1, 0])
    assert store.enc[dsts[1]].actors == enc_before[0] and store.enc[dsts[1]].reg_list == enc_before[4]
    r = store.apply([(dsts[1], [ch(Z, 2, {}, s("q", 2))])])         # ... and lives on
    assert int(r.docs["status"][0]) == 0
    b, _ = store.read(dsts[1])
    same_as_oracle(store, dsts[1], b, "after the rollback")


def test_repeated_source_and_300_requests(engine):
    """One source into three destinations at three clocks; then 300 requests in one call."""
    store = DocStore(engine, a_stride=8)
    src = store.open()
    sources = [store.open() for _ in range(3)]
    n = 300
    dsts = [store.open() for _ in range(n)]
    store.apply([(src, SHUFFLED)] + [(h, c["src"]) for h, c in zip(sources, (HAND_BY_NAME["text"], HAND_BY_NAME["counter"], HAND_BY_NAME["links"]))])
    store.apply([(d, [ch(Z, 1, {}, s("own", i), s("k%d" % (i % 5), i))]) for i, d in enumerate(dsts)])
    clocks = [{A: 3, B: 2, "cccc": 1}, {B: 1, A: 1}, {"cccc": 1, A: 2}]
    cases = [case("rep%d" % i, SHUFFLED, None, clocks[i]) for i in range(3)]
    merge_and_check(store, cases, [src] * 3, dsts[:3])
    pool = [(src, SHUFFLED, {B: 2, A: 3})] + [(h, c["src"], c["clock"]) for h, c in
                                               zip(sources, (HAND_BY_NAME["text"], HAND_BY_NAME["counter"], HAND_BY_NAME["links"]))]
    pick = [0 if i < 3 else i % 4 for i in range(n)]             # (the first three hold part of the shuffled document already)
    cases = [case("many%d" % i, pool[k][1], None, pool[k][2]) for i, k in enumerate(pick)]
    pairs, res = merge_and_check(store, cases, [pool[k][0] for k in pick], dsts)
    assert (res.docs["status"] == 0).all() and int(res.docs["hist_len"][3]) > 1


def test_undo_restores_every_destination(engine):
    store = DocStore(engine, a_stride=8)
    cases = [HAND_BY_NAME[k] for k in ("repo_merge", "shuffled", "text", "unblocks", "empty")]
    srcs, dsts = load(store, cases)
    before = [state(store, h) for h in dsts + srcs]
    snaps = [store.enc[d].snapshot() for d in dsts]
    bid = store.merge_from_submit(dsts, srcs, [c["clock"] for c in cases])
    res = store.wait()
    assert (res.docs["status"] == 0).all() and state(store, dsts[0]) != before[0]
    store._check(store._L.hm_batch_undo(store._h, bid), "hm_batch_undo")
    for d, sn in zip(dsts, snaps):                                 # (the caller's interners go back with it)
        store.enc[d].restore(sn)
    assert [state(store, h) for h in dsts + srcs] == before
    # ... and the same merge again gives the merged documents
    merge_and_check(store, cases, srcs, dsts)


def raw_args(store, pairs, srcs, dsts):
    """hm_store_merge_from_submit's arguments for the pairs, as merge_from would build them."""
    n, S = len(pairs), store.S
    maps = MergeMaps(np.stack([p.maps.totals for p in pairs]), np.stack([p.maps.rank for p in pairs]),
                     [p.maps.objs for p in pairs], [p.maps.regs for p in pairs], None, [p.maps.content for p in pairs])
    remap = np.tile(np.arange(S, dtype=np.uint8), (n, 1))
    for i, p in enumerate(pairs):
        if p.remap is not None:
            remap[i, :len(p.remap)] = p.remap
    return dict(dst=list(dsts), src=list(srcs), rows=np.stack([p.clock for p in pairs]), have=np.stack([p.have for p in pairs]),
                orow=np.stack([p.order for p in pairs]), maps=maps, remap=remap)


def test_refusals_leave_every_byte_unchanged(engine):
    store = DocStore(engine, a_stride=8)
    cases = [HAND_BY_NAME["shuffled"], HAND_BY_NAME["text"]]
    srcs, dsts = load(store, cases)
    wide = store.open()
    store.apply([(wide, [ch("a%d" % i, 1, {}, s("k", i)) for i in range(7)])])
    pairs = [Pair(c, 8, store.enc[p], store.enc[d]) for c, p, d in zip(cases, srcs, dsts)]
    everything = dsts + srcs + [wide]
    before = [state(store, h) for h in everything]

    def refused(what, **change):
        a = raw_args(store, pairs, srcs, dsts)
        a.update(change)
        with pytest.raises(EngineError):
            store._merge_rows(**a)
        assert [state(store, h) for h in everything] == before, what

    ok = raw_args(store, pairs, srcs, dsts)
    refused("a destination that is also a source", dst=[dsts[0], srcs[0]])
    refused("a destination that is its own source", src=[srcs[0], dsts[1]])
    refused("a destination named twice", dst=[dsts[0], dsts[0]])
    refused("a destination outside the store", dst=[dsts[0], 99999])
    refused("a source outside the store", src=[srcs[0], 99999])
    low = ok["maps"].totals.copy()
    low[1, 1] = store.info(dsts[1])["n_regs"] - 1
    refused("totals below the current ones", maps=MergeMaps(low, ok["maps"].rank, ok["maps"].objs, ok["maps"].regs, None, ok["maps"].content))
    many = ok["maps"].totals.copy()
    many[0, 0] = 9
    refused("n_actors > S", maps=MergeMaps(many, ok["maps"].rank, ok["maps"].objs, ok["maps"].regs, None, ok["maps"].content))
    short = [ok["maps"].regs[0], ok["maps"].regs[1][:2]]
    refused("a map slice shorter than an id met", maps=MergeMaps(ok["maps"].totals, ok["maps"].rank, ok["maps"].objs, short, None, ok["maps"].content))
    holed = [ok["maps"].objs[0].copy(), ok["maps"].objs[1]]
    holed[0][0] = NONE
    refused("a NONE map entry on a selected row", maps=MergeMaps(ok["maps"].totals, ok["maps"].rank, holed, ok["maps"].regs, None, ok["maps"].content))
    norank = ok["maps"].rank.copy()
    norank[0, 1] = NONE
    refused("a NONE rank entry on a selected row", maps=MergeMaps(ok["maps"].totals, norank, ok["maps"].objs, ok["maps"].regs, None, ok["maps"].content))
    twice = ok["orow"].copy()
    twice[0, :4] = [1, 0, 2, 1]
    refused("a bad order row: a rank twice", orow=twice)
    unlisted = ok["orow"].copy()
    unlisted[0, 2] = NONE
    refused("a bad order row: a selected actor not listed", orow=unlisted)
    refused("no clock", rows=None)
    assert store._L.hm_store_merge_from_submit(store._h, 0, None, None, None, None, None, None, None, None) == INVALID
    # the Python face restores the destinations' interners when the library refuses
    enc = store.enc[dsts[0]].snapshot()
    with pytest.raises(EngineError, match="destination"):
        store.merge_from([dsts[0], dsts[0]], srcs, [c["clock"] for c in cases])
    assert store.enc[dsts[0]].snapshot()[:7] == enc[:7]
    with pytest.raises(EngineError, match="actors"):
        store.merge_from([wide], [srcs[0]], [cases[0]["clock"]])
    assert [state(store, h) for h in everything] == before
    # a batch in flight
    store.submit([(wide, [ch("a0", 2, {}, s("k", 9))])])
    with pytest.raises(EngineError, match="in flight"):
        store._merge_rows(**raw_args(store, pairs, srcs, dsts))
    store.wait()
    # a merge batch in flight refuses reads and a second merge; afterwards the merge stands
    store.merge_from_submit(dsts, srcs, [c["clock"] for c in cases])
    with pytest.raises(EngineError, match="in flight"):
        store.info(dsts[0])
    with pytest.raises(EngineError, match="in flight"):
        store._merge_rows(**raw_args(store, pairs, srcs, dsts))
    assert (store.wait().docs["status"] == 0).all()
    for p, d in zip(pairs, dsts):
        same_as_oracle(store, d, p.log, p.case["name"])


def test_row_store_with_a_string_map(engine):
    """RowStore.merge_from with explicit maps: the two documents' rows come from interners with string pools
    of their own, so keys and string values go through a string map that is not the identity."""
    S = 8
    c = HAND_BY_NAME["links"]
    ps, pd = StringPool(), StringPool()
    for w in ("padding", "so", "that", "ids", "differ"):
        pd.intern(w)
    es, ed = DocEncoder(ps), DocEncoder(pd)
    es.encode(c["src"])
    ed.encode(c["dst"])
    sb, db = es.log_batch(S), ed.log_batch(S)
    store = RowStore(engine, a_stride=S)
    h0 = store.open_n(2)
    src, dst = h0, h0 + 1
    both = gather([(source_of(sb, np.arange(len(sb.changes)), 0), len(sb.changes), None),
               (source_of(db, np.arange(len(db.changes)), 0), len(db.changes), None)], S)[0]
    store.submit_batch(both, np.array([src, dst], np.uint32))
    assert (store.wait().docs["status"] == 0).all()
    final = clone(ed)
    totals, rank, om, rm, cm, mp = merge_maps(es, final, S)
    strs = np.array([pd.intern(x) for x in ps.strings], np.uint32)
    assert not np.array_equal(strs, np.arange(len(strs)))
    srank = {a: r for r, a in enumerate(es.actors)}
    clock = np.zeros((1, S), np.uint32)
    for a, q in c["clock"].items():
        clock[0, srank[a]] = q
    order = [[srank[a] for a in c["clock"]]]
    remap = None if mp is None else np.concatenate([mp, np.arange(len(mp), S, dtype=np.uint8)])[None, :]
    res = store.merge_from([dst], [src], clock, MergeMaps(totals[None, :], rank[None, :], [om], [rm], [strs], [cm]),
                           order=order, remap=remap)
    assert int(res.docs["status"][0]) == 0
    # the same changes encoded directly by the destination's interner
    direct = clone(final)
    direct.encode([x for a in c["clock"] for x in sorted((y for y in c["src"] if y["actor"] == a), key=lambda y: y["seq"])
                   if x["seq"] <= c["clock"][a]])
    want = direct.log_batch(S)
    lc, ld, lo = store.log(dst)
    same_bytes(lc, want.changes, "changes")
    same_bytes(ld, want.deps, "deps")
    same_bytes(lo, want.ops, "ops")
    o = O.merge(want)
    r = store.read(dst)[1]
    for f in ("hist", "all_deps", "regs"):
        same_bytes(getattr(r, f), getattr(o, f), f)
    # and the restatement renames as the device does
    src_ref = source_of(sb, O.merge(sb).hist, 0)
    ref_rows = rows_for(src_ref, clock[0], None, np.array(order[0] + [NONE] * (S - len(order[0])), np.uint32),
                        Maps(totals, rank, om, rm, strs, cm), S)
    same_bytes(lo[len(db.ops):], ref_rows.ops, "restated ops")


def test_fuzz_pairs(engine):
    """The pairs test_merge_ref.py pins, in one call: at least FUZZ_MIN_QUALIFY merges select changes
    through maps that are not the identity, and none is skipped."""
    store = DocStore(engine, a_stride=8)
    cases = fuzz_pairs()
    srcs, dsts = load(store, cases)
    pairs, res = merge_and_check(store, cases, srcs, dsts)
    assert (res.docs["status"] == 0).all()
    qualify = sum(len(p.rows.changes) > 0 and not p.identity_maps() for p in pairs)
    assert qualify >= FUZZ_MIN_QUALIFY, qualify
    assert sum(len(p.rows.changes) for p in pairs) > 200
