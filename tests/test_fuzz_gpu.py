"""Every device path on the documents of the full-vocabulary generator (tests/fuzz_docs.py): cold
merge on both kernels, fault documents, the resident store's incremental passes, materialize at past
points, per-op and element diffs (two-pass and one-walk) and the docset's device-diff rounds, each
against the reference its own suite uses (the oracle, tests/past_ref.py, tests/op_diffs_ref.py,
tests/list_diffs_ref.py).  tests/test_fuzz_docs.py pins those references on the same documents
without a GPU.

The wall times in the docstrings are whole-test times on an MI355X host, reference side included."""
import dataclasses
import json
from functools import lru_cache

import numpy as np
import pytest

from hypermerge_amd.columnar import encode
from hypermerge_amd.docset import ROOT, apply_diffs, render_objects, view_objects
from hypermerge_amd.render import canonical_json
from hypermerge_amd.store import DocStore
import oracle.oracle as O

from clock_diffs_ref import census as clock_census
from clock_diffs_ref import clocks_of
from fuzz_docs import gen_docs
from list_diffs_ref import pack as pack_lists
from op_diffs_ref import pack as pack_maps
from past_ref import clock_at, hist_len
from test_clock_diffs_gpu import check as check_diffs_at
from test_docset_gpu import _blocks, _chunks, _oracle
from test_fuzz_docs import blocked_docs, default_docs, fault_docs
from test_gpu_parity import assert_same
from test_list_diffs_gpu import check as check_element_diffs
from test_materialize_gpu import check as check_materialize
from test_materialize_gpu import enc_source as past_source
from test_once_diffs_gpu import first_difference, per_request, ref_tables
from test_op_diffs_gpu import check as check_op_diffs
from test_op_diffs_gpu import enc_source as diff_source
from test_op_diffs_gpu import ranges_of
from test_round_diffs_docset_gpu import Pair
from test_store_gpu import assert_doc_matches_oracle, split

pytestmark = pytest.mark.gpu


def cold_reference(docs):
    """(batch, the oracle's merge, its canonical rendering of every document)"""
    b = encode(docs)
    o = O.merge(b, threads=8)
    assert (o.docs["status"] == 0).all()
    return b, o, [canonical_json(b, o, d) for d in range(b.n_docs)]


@lru_cache(maxsize=None)
def cold():
    """300 default, 40 wide and 6 long documents in one batch"""
    b, o, want = cold_reference(list(default_docs()[:300]) + gen_docs("wide", range(40)) + gen_docs("long", range(6)))
    assert int(b.docs["n_actors"].max()) > 8 and int(b.docs["n_changes"].max()) > 64
    assert (b.docs["n_ops"] <= 256).any() and (b.docs["n_ops"] > 256).any()
    return b, o, want


def cold_leg(eng, ref, list_hint=True):
    """every result table bit-exact with the oracle, no document outside the envelope, and the
    canonical rendering of every document"""
    b, o, want = ref
    if not list_hint:
        b = dataclasses.replace(b, docs=b.docs.copy())
        b.docs["flags"] &= ~np.uint16(1)
    g = eng.merge(b)
    assert assert_same(b, g, o) == 0
    assert (g.docs["status"] == 0).all()
    for d in range(b.n_docs):
        assert canonical_json(b, g, d) == want[d], d


@pytest.mark.parametrize("general", [False, True], ids=["small", "general"])
def test_cold_merge(engine, engine_general, general):
    """Wall 3.0 s for the first case (it builds the shared reference), 0.1 s for the second."""
    cold_leg(engine_general if general else engine, cold())


def test_cold_merge_without_list_hint(engine_general):
    """HM_DOC_HAS_LISTS is a launch hint only: cleared, the same results.  Wall 0.1 s."""
    cold_leg(engine_general, cold(), list_hint=False)


def fault_leg(engines, faulty, clean):
    """documents that throw alternate with as many that do not: status and the throwing (change, op)
    equal the oracle's per document, the clean neighbours are untouched"""
    docs = [x for pair in zip(faulty, clean) for x in pair]
    b = encode(docs)
    o = O.merge(b)
    assert (o.docs["status"][0::2] != 0).all() and (o.docs["status"][1::2] == 0).all()
    assert len(set(int(x) for x in o.docs["status"])) == 6
    for eng in engines:
        fault_check(eng, b, o)


def fault_check(eng, b, o):
    g = eng.merge(b)
    assert assert_same(b, g, o) == 0
    for f in ("status", "err_change", "err_op"):
        np.testing.assert_array_equal(g.docs[f], o.docs[f], err_msg=f)
    for d in range(b.n_docs):
        assert canonical_json(b, g, d) == canonical_json(b, o, d), d


@pytest.mark.parametrize("general", [False, True], ids=["small", "general"])
def test_fault_documents_among_clean_ones(engine, engine_general, general):
    """80 documents that throw (16 of each kind) among 80 clean ones.  Wall 0.2 s each."""
    fault_leg([engine_general if general else engine], [chs for chs, _ in fault_docs()], list(default_docs()[300:380]))


def incremental_against_remerge(engine, docs, S, seed):
    """test_store_gpu.test_incremental_apply_equals_full_remerge's body: the first half of every
    document loaded, then rounds of 1-3 changes into an incremental store and a re-merging one."""
    rng = np.random.default_rng(seed)
    A, B = DocStore(engine, a_stride=S), DocStore(engine, a_stride=S)
    A.set_incremental(2)
    B.set_incremental(False)
    ha = [A.open() for _ in docs]
    hb = [B.open() for _ in docs]
    pos = [len(c) // 2 for c in docs]
    ra = A.apply([(h, docs[i][:pos[i]]) for i, h in enumerate(ha)])
    rb = B.apply([(h, docs[i][:pos[i]]) for i, h in enumerate(hb)])
    np.testing.assert_array_equal(ra.docs, rb.docs)
    assert (ra.docs["status"] == 0).all()
    for i in range(0, len(docs), 5):                          # minimumClocks, so min_cmp moves as the clocks advance
        mc = {}
        for c in docs[i][:pos[i] + 3]:
            mc[c["actor"]] = max(mc.get(c["actor"], 0), c["seq"])
        mc = {a: q for a, q in mc.items() if a in A.enc[ha[i]].actors}
        A.set_min_clock(ha[i], mc)
        B.set_min_clock(hb[i], mc)
    routed = {"incremental": 0, "remerged": 0, "handed_back": 0}
    rnd = 0
    while any(p < len(c) for p, c in zip(pos, docs)):
        take = {i: int(rng.integers(1, 4)) for i in range(len(docs)) if pos[i] < len(docs[i])}
        ra = A.apply([(ha[i], docs[i][pos[i]:pos[i] + k]) for i, k in take.items()])
        rb = B.apply([(hb[i], docs[i][pos[i]:pos[i] + k]) for i, k in take.items()])
        for k, v in A.last_routing().items():
            routed[k] += v
        assert (ra.docs["status"] == 0).all(), f"round {rnd}"
        for f in ("docs", "clock", "back_clock", "heads"):
            np.testing.assert_array_equal(getattr(ra, f), getattr(rb, f), err_msg=f"{f} round {rnd}")
        for i, k in take.items():
            pos[i] += k
        for i in rng.choice(list(take), size=min(6, len(take)), replace=False):
            assert_doc_matches_oracle(A, ha[i])
        rnd += 1
    cold_b = encode(docs, S)
    cold_o = O.merge(cold_b)
    for i in range(len(docs)):
        ba, ga = assert_doc_matches_oracle(A, ha[i])
        bb, gb = B.read(hb[i])
        for f in ("docs", "clock", "back_clock", "heads", "hist", "all_deps", "regs", "surv"):
            np.testing.assert_array_equal(getattr(ga, f), getattr(gb, f), err_msg=f"{f} doc {i}")
        assert canonical_json(ba, ga, 0) == canonical_json(cold_b, cold_o, i), i
    return A, B, routed


def first_throwing_prefix(chs):
    """the smallest n for which applyChanges(chs[:n]) throws, with that status"""
    b = encode([chs[:n] for n in range(len(chs) + 1)])
    st = O.merge(b).docs["status"]
    n = int(np.flatnonzero(st)[0])
    return n, int(st[n])


def test_resident_store_incremental_equals_remerge_and_oracle(engine):
    """80 default documents at stride 8 and 10 wide ones at stride 64, then a fault round on the
    stride-8 stores.  Wall 0.9 s."""
    A, B, routed = incremental_against_remerge(engine, list(default_docs()[:80]), 8, 11)
    assert routed["incremental"] > 0, routed
    _, _, wide = incremental_against_remerge(engine, gen_docs("wide", range(10)), 64, 12)
    print("routed", routed, "wide", wide)
    fault_round(A, B, [chs for chs, _ in fault_docs()[:20]])


def fault_round(A, B, faulty):
    """On both stores: the call that throws leaves the document as it was (its clean neighbour, fed
    the same call without the throwing change, applies), and the next clean call merges on top."""
    cut = [first_throwing_prefix(chs) for chs in faulty]
    for store in (A, B):
        hf = [store.open() for _ in faulty]
        hn = [store.open() for _ in faulty]
        lo = [n // 2 for n, _ in cut]
        r = store.apply([(h, chs[:k]) for h, chs, k in zip(hf + hn, faulty + faulty, lo + lo)])
        assert (r.docs["status"] == 0).all()
        before = [canonical_json(*store.read(h), 0) for h in hf]
        r = store.apply([(h, chs[k:n]) for h, chs, k, (n, _) in zip(hf, faulty, lo, cut)] +
                        [(h, chs[k:n - 1]) for h, chs, k, (n, _) in zip(hn, faulty, lo, cut)])
        assert [int(x) for x in r.docs["status"][:len(hf)]] == [st for _, st in cut]
        assert (r.docs["status"][len(hf):] == 0).all()
        assert [canonical_json(*store.read(h), 0) for h in hf] == before
        assert [store.info(h)["n_changes"] for h in hf] == lo
        r = store.apply([(h, chs[k:n - 1]) for h, chs, k, (n, _) in zip(hf, faulty, lo, cut)])
        assert (r.docs["status"] == 0).all()
        want_b = encode([chs[:n - 1] for chs, (n, _) in zip(faulty, cut)], 8)
        want_o = O.merge(want_b)
        for i, (h, h2) in enumerate(zip(hf, hn)):
            for x in (h, h2):
                bb, g = assert_doc_matches_oracle(store, x)
                assert canonical_json(bb, g, 0) == canonical_json(want_b, want_o, i), i


ROUNDS = 3


@pytest.fixture(scope="module")
def fed(engine):
    """40 default documents fed to one store in three rounds"""
    return feed_store(engine, list(default_docs()[100:140]))


def feed_store(engine, docs):
    """(store, handles, the history length of every document after every round)"""
    rng = np.random.default_rng(21)
    parts = [split(c, ROUNDS, rng) for c in docs]
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in docs]
    marks = [[0] for _ in docs]
    for rd in range(ROUNDS):
        res = store.apply([(h, parts[i][rd]) for i, h in enumerate(hs)])
        assert (res.docs["status"] == 0).all()
        for i in range(len(docs)):
            marks[i].append(int(res.docs["hist_len"][i]))
    return store, hs, marks


def test_materialize_at_past_points(fed):
    """Wall 0.1 s."""
    materialize_leg(*fed)


def materialize_leg(store, hs, marks, min_hist=30):
    """History lengths 0, 1, a random middle, H and H + 5 of every document, then the clocks
    (past_ref.clock_at) of the same points."""
    srcs = {h: past_source(store, h) for h in hs}
    rng = np.random.default_rng(22)
    req, hist = [], []
    for h in hs:
        H = hist_len(srcs[h])
        for k in (0, 1, int(rng.integers(0, H + 1)), H, H + 5):
            req.append(h)
            hist.append(k)
    want, o = check_materialize(store, srcs, req, history=hist)
    assert int(o.docs["hist_len"].max()) > min_hist and (want.docs["flags"] & 1).any()
    rows = np.stack([clock_at(srcs[h], store.S, k) for h, k in zip(req, hist)])
    check_materialize(store, srcs, req, clocks=rows)


def diff_requests(hs, srcs, marks):
    req, frm, to = [], [], []
    for h, m in zip(hs, marks):
        bounds = [(a, b) for a, b in zip(m, m[1:])] + [(m[1], m[-1])]
        for f, t in ranges_of(hist_len(srcs[h][0])) + bounds:
            req.append(h); frm.append(f); to.append(t)
    return req, frm, to


def test_op_and_element_diffs(fed):
    """Wall 0.5 s."""
    diffs_leg(*fed)


def diffs_leg(store, hs, marks):
    """ranges_of(H) and every round boundary of every document: the per-op rows (list slices
    flagged), the element rows (lists=True), and the one-walk form of both against the two-pass
    call and the references."""
    srcs = {h: diff_source(store, h) for h in hs}
    req, frm, to = diff_requests(hs, srcs, marks)
    want_m = check_op_diffs(store, srcs, req, frm, to)
    want_l = check_element_diffs(store, srcs, req, frm, to)
    assert want_m[3].any() and not want_m[3].all() and not want_l[3].any()
    assert {0, 1, 2, 3, 4, 5} <= {int(k) for k in want_l[0][:, 1]}
    h3 = [np.array(x, np.uint32) for x in (req, frm, to)]
    triples = list(zip(req, frm, to))
    for lists, res, packer in ((True, want_l[5], pack_lists), (False, want_m[4], pack_maps)):
        two = store.op_diffs(*h3, lists=lists)
        one = store.op_diffs(*h3, lists=lists, once=True)
        np.testing.assert_array_equal(one[3], two[3])
        first_difference(per_request(one, lists), per_request(two, lists), triples, f"one walk against two passes, lists={lists}")
        first_difference(per_request(one, lists), per_request(ref_tables(res, packer), lists), triples,
                         f"one walk against the reference, lists={lists}")


def test_docset_rounds(engine):
    """30 documents.  Wall 0.2 s."""
    docset_leg(engine, list(default_docs()[200:230]))


def docset_leg(engine, docs):
    """Four rounds to a device-diffs docset and a replaying one: the texts of every call
    byte-identical (Pair.apply), the patches rebuild the oracle's document and both views equal it
    after every round."""
    chunked = _chunks(docs, np.random.default_rng(23))
    pair = Pair(engine)
    first = pair.open(len(docs))
    ids = list(range(first, first + len(docs)))
    objects = [{ROOT: {"type": "map", "keys": {}, "elems": []}} for _ in docs]
    logs = [[] for _ in docs]
    for r in range(4):
        sel = [i for i in range(len(docs)) if chunked[i][r]]
        res, js = pair.apply([ids[i] for i in sel], [_blocks(chunked[i][r]) for i in sel])
        assert (res["status"] == 0).all()
        for k, i in enumerate(sel):
            d = ids[i]
            logs[i] += chunked[i][r]
            apply_diffs(objects[i], js["p"][k]["diffs"])
            s = _oracle(logs[i])
            state = json.loads(json.dumps(s["state"]))
            assert int(res[k]["hist_len"]) == len(s["history"]) and int(res[k]["n_queued"]) == s["queued"], (i, r)
            assert js["p"][k]["clock"] == s["clock"] and js["b"][k] == s["backend_clock"], (i, r)
            assert render_objects(objects[i]) == state, (i, r)
            for ds in (pair.device, pair.replay):
                assert render_objects(view_objects(ds.view(d))) == state, (i, r)
    pair.check_counters()


# ---- documents that end blocked (fuzz_docs.withheld) through the same legs --------------------------
@pytest.fixture(scope="module")
def fed_blocked(engine):
    """20 default documents, each with one to three changes withheld, fed in three rounds"""
    store, hs, marks = feed_store(engine, blocked_docs())
    nq = store.waiting(hs)[2]
    assert 2 * int((nq > 0).sum()) >= len(hs), nq
    return store, hs, marks


def queued_clocks(store, hs, srcs):
    """per blocked document the clock of its whole history, and the same clock naming a queued
    change's (actor, seq): queued changes are never selected, so both select the same changes"""
    req, plain, named = [], [], []
    for h in hs:
        src = srcs[h]
        queued = np.flatnonzero(src.hist == -1)
        if not len(queued):
            continue
        k = clock_at(src, store.S, hist_len(src))
        up = k.copy()
        for i in queued:
            a = int(src.changes[i]["actor"])
            up[a] = max(int(up[a]), int(src.changes[i]["seq"]))
        assert (up != k).any()
        req.append(h); plain.append(k); named.append(up)
    return req, plain, named


def test_blocked_documents_materialize(fed_blocked):
    """History lengths and clocks come from hist_len of the blocked state.  Wall under 0.1 s."""
    store, hs, marks = fed_blocked
    materialize_leg(store, hs, marks, min_hist=20)
    srcs = {h: past_source(store, h) for h in hs}
    req, plain, named = queued_clocks(store, hs, srcs)
    assert 2 * len(req) >= len(hs)
    a, _ = check_materialize(store, srcs, req, clocks=np.stack(named))
    b, _ = check_materialize(store, srcs, req, clocks=np.stack(plain))
    for f in ("docs", "changes", "deps", "ops"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def test_blocked_documents_op_and_element_diffs(fed_blocked):
    """Wall 0.1 s."""
    diffs_leg(*fed_blocked)


def test_blocked_documents_diffs_at_clocks(fed_blocked):
    """hm_store_op_diffs_at at prefix, causal-past and cut clocks, and at the clocks that name queued
    changes.  Wall 0.1 s."""
    store, hs, _ = fed_blocked
    srcs = {h: diff_source(store, h) for h in hs}
    rng = np.random.default_rng(24)
    req, ks = [], []
    for h in hs:
        for _, k in clocks_of(*srcs[h], store.S, rng):
            req.append(h); ks.append(k)
    n, closed, queued = clock_census([(*srcs[h], store.S, k) for h, k in zip(req, ks)])
    assert 8 * closed >= n and 8 * queued >= n, (n, closed, queued)
    memo = {}
    check_diffs_at(store, srcs, req, ks, memo=memo)
    qreq, plain, named = queued_clocks(store, hs, {h: srcs[h][0] for h in hs})
    a = check_diffs_at(store, srcs, qreq, named, memo=memo)
    b = check_diffs_at(store, srcs, qreq, plain, memo=memo)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
