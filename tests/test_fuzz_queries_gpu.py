"""The three read-only queries on the resident state — what blocked documents wait for
(csrc/waiting_kernels.hip), which changes a peer lacks (csrc/changes_kernels.hip), the fields a
proposed change touches (csrc/field_kernels.hip) — on the documents of the full-vocabulary generator
(tests/fuzz_docs.py), delivered in full and with one to three changes withheld (``withheld``: every
change that depends on a withheld one stays queued, and the withheld changes are the proposals of the
fields query).  Every expected value is tests/waiting_ref.py, tests/missing_changes_ref.py or
tests/fields_ref.py applied to the CPU oracle's merge of the document's own log; tests/test_fuzz_docs.py
pins those references on the same documents without a GPU and counts what the documents hold.

The last section sends more requests in one call than the query, diff and materialize kernels launch
workgroups (65,535), so that a workgroup takes a second request with the first one's LDS behind it.

The wall times in the docstrings are whole-test times on an MI355X host, reference side included."""
import ctypes
from collections import Counter

import numpy as np
import pytest

from hypermerge_amd.columnar import CBatch, CResults, encode
from hypermerge_amd.docset import DocSet
from hypermerge_amd.engine import FIELD_OP_DT, pack_entries, pack_fields
from hypermerge_amd.store import DocStore, slice_changes
import oracle.oracle as O

import fields_ref
import missing_changes_ref
import waiting_ref
from fields_ref import rows_of
from fuzz_docs import assigned, base_clock, gen_doc, quiet_tail, withheld
from kat_cases import A, B, Cc, D, ch, ins, link, mk, s
from missing_changes_ref import ONLY_LISTED, RAW
from op_diffs_cases import chain_doc
from past_ref import clock_at, hist_len
from test_clock_diffs_gpu import check as check_diffs_at
from test_fields_docset_gpu import _want as docset_fields_want
from test_fields_gpu import Ref as FieldsRef
from test_fields_gpu import check as check_fields
from test_fields_gpu import rand_have as fields_have
from test_fuzz_docs import fault_docs, query_docs
from test_list_diffs_gpu import check as check_element_diffs
from test_materialize_gpu import check as check_materialize
from test_materialize_gpu import enc_source as past_source
from test_missing_changes_docset_gpu import _want as docset_changes_want
from test_missing_changes_gpu import Ref as ChangesRef
from test_missing_changes_gpu import check as check_changes
from test_missing_changes_gpu import rand_have as changes_have
from test_missing_changes_gpu import read_history
from test_missing_changes_host import FOR_ACTOR
from test_op_diffs_gpu import enc_source as diff_source
from test_store_gpu import split
from test_waiting_docset_gpu import _blocks
from test_waiting_docset_gpu import _want as docset_waiting_want
from test_waiting_gpu import check_handles, expected

pytestmark = pytest.mark.gpu

INVALID = 32
GRID = 65535          # the workgroups changes_kernel, fields_kernel, od_walk_kernel and past_fill_kernel launch at most
WAIT_PASS = 4096 * 4  # the requests of one pass of waiting_kernel: 4096 workgroups of four waves
ALL_FLAGS = (0, RAW, ONLY_LISTED, FOR_ACTOR)


# ---- the documents --------------------------------------------------------------------------------
def stride_docs(S):
    """[(what arrives, the changes withheld from it)]: every second document is withheld"""
    if S == 8:
        trip = query_docs("default")[:40]
    elif S == 16:
        trip = []
        for i in range(8):
            chs = gen_doc(300 + i, n_actors=9 + i, profile="wide")
            trip.append((chs,) + withheld(chs, 7000 + i))
    else:
        trip = query_docs("wide")[:10]
    return [(kept, dropped) if i % 2 else (full, []) for i, (full, kept, dropped) in enumerate(trip)]


def proposal_want(store, ref, h, c):
    """what store.fields answers for the dropped change c as a proposal on handle h: the reference on
    the entries in the clock's own order, the registers found in the host encoder's tables"""
    enc = store.enc[h]
    rank = {a: i for i, a in enumerate(enc.actors)}
    base = base_clock(c)
    fl = assigned(c)
    if any(a not in rank and q > 0 for a, q in base.items()):
        return False, [[] for _ in fl]
    regs = [enc.regs.get((enc.objs.get(o), k), 0xFFFFFFFF) if o in enc.objs else 0xFFFFFFFF for o, k in fl]
    ready, _, rows = ref(h, [(rank[a], q) for a, q in base.items() if a in rank], regs)
    return ready, [[dict(op=r[0], action=r[1], datatype=r[2], vtag=r[3], value=r[4], actor=enc.actors[r[5]], seq=r[6], covered=r[7])
                    for r in f] for f in rows]


def same_fields(x, y):
    (gx, cx), (gy, cy) = x, y
    np.testing.assert_array_equal(cx, cy)
    assert [g[0] for g in gx] == [g[0] for g in gy]
    assert [[f.tobytes() for f in g[1]] for g in gx] == [[f.tobytes() for f in g[1]] for g in gy]


# ---- (a) stores fed in rounds ---------------------------------------------------------------------
def query_round(X, Y, hs, rng, clocks, lens, proposals, seen):
    """All three queries over every handle of the incremental store X against the references, and the
    re-merging store Y's tables against X's.  clocks / lens: per earlier round, every handle's
    opSet.clock by actor id and history length."""
    # what blocked documents wait for
    want = [h for h in hs if expected(X, h)[2] > 0]
    assert [int(x) for x in X.blocked()] == want == [int(x) for x in Y.blocked()]
    assert check_handles(X, hs) == want
    wx, wy = X.waiting(hs), Y.waiting(hs)
    for a, b in zip(wx, wy):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(X.queues(hs, wx[2]), Y.queues(hs, wy[2])):
        np.testing.assert_array_equal(a, b)
    seen["blocked"] += len(want)
    seen["rows2"] += int((np.count_nonzero(wx[0], axis=1) >= 2).sum())
    # which changes a peer lacks
    cref = ChangesRef(X)
    req = list(hs) * 2
    have = [changes_have(rng, cref.clock(h), len(X.enc[h].actors)) for h in req]
    req, have = req + req, have + [e[::-1] for e in have]
    for flags in ALL_FLAGS:
        seen["changes"] += check_changes(X, cref, req, have, flags)
        gx, gy = X.missing_changes_rows(req, have, flags), Y.missing_changes_rows(req, have, flags)
        assert gx[0] == gy[0]
        np.testing.assert_array_equal(gx[1], gy[1])
    seen["past_clock"] += sum(1 for h, e in zip(req, have) for a, q in e if q > int(cref.clock(h)[a]))
    seen["order"] += sum(1 for h, e in zip(req[:len(hs) * 2], have) if cref(h, e)[1] != cref(h, e[::-1])[1])
    now = [X.info(h)["hist_len"] for h in hs]
    for ck, hl in zip(clocks, lens):                 # the slice property, no restatement involved
        got = X.missing_changes(hs, [ck[h] for h in hs])
        assert got == read_history(X, hs, [hl[h] for h in hs], now) == Y.missing_changes(hs, [ck[h] for h in hs])
        seen["slices"] += sum(1 for g in got if g)
    nobody = [dict({"nobody": 9}, **clocks[-1][h]) for h in hs] if clocks else [{"nobody": 9} for _ in hs]
    known = [{a: q for a, q in c.items() if a != "nobody"} for c in nobody]
    assert X.missing_changes(hs, nobody) == X.missing_changes(hs, known)
    # the fields a proposed change touches
    fref = FieldsRef(X)
    req = list(hs) * 2
    have = [fields_have(rng, fref.clock(h), len(X.enc[h].actors), late=j % 5 == 4) for j, h in enumerate(req)]
    fields = []
    for h in req:
        nr = fref.n_regs(h)
        fields.append(list(range(nr)) + [nr, nr + 1000, 0xFFFFFFFF] + ([nr // 2] * 2 if nr else []))
    rows, late, unc = check_fields(X, fref, req, have, fields)
    same_fields(X.fields_rows(req, have, fields), Y.fields_rows(req, have, fields))
    seen["rows"] += rows; seen["late"] += late; seen["uncovered"] += unc
    # the withheld changes as proposals, by actor id and (obj, key)
    ph = [h for h, c in proposals]
    if ph:
        got = X.fields(ph, [base_clock(c) for _, c in proposals], [assigned(c) for _, c in proposals])
        assert got == [proposal_want(X, fref, h, c) for h, c in proposals]
        assert got == Y.fields(ph, [base_clock(c) for _, c in proposals], [assigned(c) for _, c in proposals])
    return [g[0] for g in got] if ph else []


@pytest.mark.parametrize("S", [8, 16, 64])
def test_stores_fed_in_rounds(engine, S):
    """An incremental (mode 2) and a re-merging (mode 0) store, 40 / 8 / 10 documents at strides 8 /
    16 / 64, every second one withheld, in four rounds; a fifth brings the full documents a tail of
    changes that meets what the plan routes incrementally (fuzz_docs.quiet_tail: the document clean,
    no new actor, no new object), a sixth brings half of the withheld documents what was withheld.
    Every query after every round.  Wall 0.6 / 0.2 / 0.3 s.

    Counted over the six rounds, from the references (stride 8 / 16 / 64): blocked documents 109 / 30 /
    30, missing rows with two or more entries 89 / 30 / 30, field requests not ready 62 / 16 / 24, field
    rows 12199 / 2541 / 3256 of which not covered 7620 / 1269 / 1195, closures that depend on the
    entries' order 62 / 18 / 26, entries one past the clock 370 / 350 / 732, non-empty slices since an
    earlier round's clock 451 / 92 / 110, rows of missing changes 24872 / 5170 / 5646; withheld changes
    as proposals 38 / 9 / 11, ready before the last round 23 / 4 / 5 and after it 29 / 5 / 7; documents
    routed to the incremental kernels 24 / 1 / 3, of which 16 / 1 / 3 in the tail round."""
    docs = stride_docs(S)
    rng = np.random.default_rng(100 + S)
    tails = [quiet_tail(kept) if not dropped else (kept, []) for kept, dropped in docs]
    parts = [split(head, 4, rng) for head, _ in tails]
    X, Y = DocStore(engine, a_stride=S), DocStore(engine, a_stride=S)
    X.set_incremental(2)
    Y.set_incremental(False)
    hs = [X.open() for _ in docs]
    assert [Y.open() for _ in docs] == hs
    proposals = [(h, c) for h, (_, dropped) in zip(hs, docs) for c in dropped]
    late_docs = [h for h, (_, dropped) in zip(hs, docs) if dropped][::2]
    rounds = [[(h, parts[i][rd]) for i, h in enumerate(hs) if rd == 0 or parts[i][rd]] for rd in range(4)]
    rounds.append([(h, tail) for h, (_, tail) in zip(hs, tails) if tail])
    rounds.append([(h, docs[hs.index(h)][1]) for h in late_docs])
    assert 2 * len(rounds[4]) >= sum(1 for _, dropped in docs if not dropped)      # most full documents have a tail
    clocks, lens, seen, routed, ready, per_round = [], [], Counter(), 0, [], []
    for items in rounds:
        rx, ry = X.apply(items), Y.apply(items)
        assert (rx.docs["status"] == 0).all() and (ry.docs["status"] == 0).all()
        routed += X.last_routing()["incremental"]
        per_round.append(X.last_routing()["incremental"])
        assert Y.last_routing()["incremental"] == 0
        ready.append(query_round(X, Y, hs, rng, clocks, lens, proposals, seen))
        ck, hl = (dict(clocks[-1]), dict(lens[-1])) if clocks else ({h: {} for h in hs}, {h: 0 for h in hs})
        for j, (h, _) in enumerate(items):
            ck[h] = {X.enc[h].actors[a]: int(q) for a, q in enumerate(rx.clock[j]) if q}
            hl[h] = int(rx.docs["hist_len"][j])
        clocks.append(ck)
        lens.append(hl)
    flipped = sum(1 for a, b in zip(ready[4], ready[5]) if b and not a)
    print(f"stride {S}: incremental {routed} {per_round}, {dict(seen)}, proposals {len(proposals)} ready {sum(ready[4])} -> {sum(ready[5])}")
    assert routed > 0 and per_round[4] > 0, per_round       # the tail round: the queries after it read incremental state
    assert seen["blocked"] >= len(docs) and seen["rows2"] >= len(docs) // 2, seen
    assert seen["late"] >= 5 and seen["uncovered"] > 0 and seen["rows"] > 1000 and seen["order"] >= 5, seen
    assert seen["past_clock"] >= 20 and seen["slices"] >= len(docs) and seen["changes"] > 1000, seen
    assert 0 < sum(ready[4]) < len(proposals) and flipped > 0, (ready[4], ready[5])
    assert not [h for h in late_docs if expected(X, h)[2]]        # what was withheld has arrived: nothing waits


# ---- (b) cold batches -----------------------------------------------------------------------------
def cold_docs(S):
    clean = [kept for kept, _ in stride_docs(8)]
    if S == 64:
        clean = clean[:20] + [kept for kept, _ in stride_docs(16)] + [kept for kept, _ in stride_docs(64)]
    faulty = [chs for chs, _ in fault_docs()[:20]]
    step = len(clean) // len(faulty)
    out = []
    for i, c in enumerate(clean):
        out.append(c)
        if i % step == 0 and i // step < len(faulty):
            out.append(faulty[i // step])
    return out


def to_device(arrays):
    import torch
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev) for x in arrays]


def device_queries(engine, b, r, have, fields, cap_log, cap_rows):
    """hm_missing_deps_device / hm_missing_changes_device / hm_fields_device on device copies of the
    batch and its results: (missing rows, (ranges, log, closure, total, bad), (flags, ranges, rows,
    closure, total, bad))"""
    import torch
    n, S = b.n_docs, b.a_stride
    off, ea, es = pack_entries(have, n)
    foff, freg = pack_fields(fields, n)
    nf = int(foff[-1])
    t = to_device((b.docs, b.changes, b.deps, b.ops, r.docs, r.clock, r.hist, r.all_deps, r.regs, r.surv, off, ea, es, foff, freg))
    cb = CBatch(n, len(b.changes), len(b.deps), len(b.ops), len(r.regs), S, 0, 0, 0, 0, 0, 0,
                t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), None)
    cr = CResults(t[4].data_ptr(), t[5].data_ptr(), None, None, t[6].data_ptr(), t[7].data_ptr(), t[8].data_ptr(), t[9].data_ptr())
    z = lambda k: torch.zeros(max(k, 1), dtype=torch.int32, device=torch.device("cuda", 0))
    u32 = lambda x: x.cpu().numpy().view(np.uint32)
    st = torch.cuda.current_stream().cuda_stream
    miss, rng_c, log, clo_c, cnt_c = z(n * S), z(2 * n), z(cap_log), z(n * S), z(2)
    flags, clo_f, rng_f, rows, cnt_f = z(n), z(n * S), z(2 * nf), z(cap_rows * 6), z(2)
    torch.cuda.synchronize()
    engine.missing_deps_device(cb, cr, miss.data_ptr(), st)
    engine.missing_changes_device(cb, cr, t[10].data_ptr(), t[11].data_ptr(), t[12].data_ptr(), int(off[-1]), 0, clo_c.data_ptr(),
                                  rng_c.data_ptr(), log.data_ptr(), cap_log, cnt_c.data_ptr(), cnt_c.data_ptr() + 4, st)
    engine.fields_device(cb, cr, t[10].data_ptr(), t[11].data_ptr(), t[12].data_ptr(), int(off[-1]), t[13].data_ptr(),
                         t[14].data_ptr(), nf, flags.data_ptr(), clo_f.data_ptr(), rng_f.data_ptr(), rows.data_ptr(), cap_rows,
                         cnt_f.data_ptr(), cnt_f.data_ptr() + 4, st)
    torch.cuda.synchronize()
    cc, cf = u32(cnt_c), u32(cnt_f)
    return (u32(miss)[:n * S].reshape(n, S),
            (u32(rng_c)[:2 * n].reshape(n, 2), u32(log), u32(clo_c)[:n * S].reshape(n, S), int(cc[0]), int(cc[1])),
            (u32(flags)[:n], u32(rng_f)[:2 * nf].reshape(nf, 2), rows.cpu().numpy().view(FIELD_OP_DT),
             u32(clo_f)[:n * S].reshape(n, S), int(cf[0]), int(cf[1])))


@pytest.mark.parametrize("S", [8, 64])
def test_cold_batches_with_documents_that_threw(engine, S):
    """The stores' documents and 20 documents that throw (four of each kind) in one cold batch: the
    three queries in their host and device-pointer forms.  A document that threw offers nothing.
    Wall 0.1 / 0.1 s.  Stride 8 / 64: 60 / 58 documents, 18 / 18 blocked, 17 / 16 requests not ready,
    1224 / 1411 field rows of which 875 / 813 not covered."""
    docs = cold_docs(S)
    b = encode(docs, S)
    o = O.merge(b)
    r = engine.merge(b)
    n = b.n_docs
    threw = np.flatnonzero(o.docs["status"])
    assert len(threw) == 20 and len({int(x) for x in o.docs["status"][threw]}) == 5
    np.testing.assert_array_equal(r.docs["status"], o.docs["status"])
    rng = np.random.default_rng(S)
    clock = lambda d: o.clock[d * S:(d + 1) * S]
    have = [fields_have(rng, clock(d), len(b.doc_actors[d]), late=d % 5 == 4) for d in range(n)]
    for d in threw[::2]:                                        # entries above a clock of zeros: not ready; the others: seq 0
        have[d] = [(0, 1)]
    for d in threw[1::2]:
        have[d] = [(a, 0) for a in range(min(3, len(b.doc_actors[d])))]
    fields = [list(range(int(b.docs["n_regs"][d]))) + [int(b.docs["n_regs"][d]), 0xFFFFFFFF] for d in range(n)]
    w_miss = np.stack([waiting_ref.doc_ref(b, o, d)[0] for d in range(n)])
    w_chg = {f: [missing_changes_ref.doc_ref(b, o, d, have[d], f) for d in range(n)] for f in ALL_FLAGS}
    w_fld = [fields_ref.doc_ref(b, o, d, have[d], fields[d]) for d in range(n)]
    # host forms
    np.testing.assert_array_equal(engine.missing_deps(b, r), w_miss)
    for f in ALL_FLAGS:
        got, clo = engine.missing_changes(b, r, have, f, closure=True)
        assert got == [w[0] for w in w_chg[f]], f
        assert [[int(x) for x in row] for row in clo] == [w[1] for w in w_chg[f]], f
    got, clo = engine.fields(b, r, have, fields, closure=True)
    for d in range(n):
        assert (got[d][0], [int(x) for x in clo[d]], [rows_of(f) for f in got[d][1]]) == w_fld[d], d
    # a document that threw: a zero row, no changes, no field rows, and ready exactly when every seq is 0
    for d in threw:
        assert not w_miss[d].any() and all(w_chg[f][d][0] == [] for f in ALL_FLAGS) and not any(w_fld[d][2]), d
    assert [w_fld[d][0] for d in threw] == [False, True] * 10
    blocked = int(w_miss.any(axis=1).sum())
    n_late = sum(1 for w in w_fld if not w[0])
    n_rows = sum(len(f) for w in w_fld for f in w[2])
    n_unc = sum(1 for w in w_fld for f in w[2] for x in f if not x[7])
    print(f"stride {S}: {n} documents, {blocked} blocked, {n_late} not ready, {n_rows} field rows, {n_unc} not covered")
    assert 4 * blocked >= n - 20 and n_late >= 10 + 3 and n_unc > 0 and n_rows > 500
    # device-pointer forms
    miss, (rg, log, clo, tot, bad), (fl, frg, rows, fclo, ftot, fbad) = device_queries(engine, b, r, have, fields, len(b.changes), n_rows)
    np.testing.assert_array_equal(miss, w_miss)
    assert (tot, bad, ftot, fbad) == (sum(len(w[0]) for w in w_chg[0]), 0, n_rows, 0)
    foff = pack_fields(fields, n)[0]
    for d in range(n):
        assert [int(x) for x in log[int(rg[d, 0]):int(rg[d, 0]) + int(rg[d, 1])]] == w_chg[0][d][0], d
        assert [int(x) for x in clo[d]] == w_chg[0][d][1], d
        per = [rows_of(rows[int(a):int(a) + int(c)]) for a, c in frg[int(foff[d]):int(foff[d + 1])]]
        assert (int(fl[d]) == 0, [int(x) for x in fclo[d]], per) == w_fld[d], d


# ---- (c) the docset ---------------------------------------------------------------------------------
def test_docset_rounds(engine):
    """20 documents, full and withheld, as JSON blocks in three rounds; one wide document outgrows the
    stride-8 class on the way (8 -> 32 here).  Wall 0.2 s.  Over the rounds: 27 blocked documents, 43 requests not ready, 82 field
    rows of which 54 not covered, 1729 rows of missing changes."""
    docs = stride_docs(8)[:17] + [stride_docs(16)[1], stride_docs(16)[2], stride_docs(64)[1]]
    rng = np.random.default_rng(31)
    parts = [split(kept, 3, rng) for kept, _ in docs]
    mover = len(docs) - 1                                  # its first round: the changes of its first five actors
    kept = docs[mover][0]
    few = sorted({c["actor"] for c in kept})[:5]
    early = [c for c in kept if c["actor"] in few and set(c["deps"]) <= set(few)]
    parts[mover] = [early, [c for c in kept if c not in early], []]
    ds = DocSet(engine)
    first = ds.open(len(docs))
    ids = list(range(first, first + len(docs)))
    logs = [[] for _ in docs]
    strides, seen = [], Counter()
    for rd in range(3):
        sel = [i for i in range(len(docs)) if parts[i][rd]]
        res, _ = ds.apply([ids[i] for i in sel], [_blocks(parts[i][rd]) for i in sel])
        assert (res["status"] == 0).all()
        for i in sel:
            logs[i] += parts[i][rd]
        strides.append(ds.info(ids[mover])["a_stride"])
        wait = [docset_waiting_want(logs[i]) for i in range(len(docs))]
        assert ds.waiting(ids) == wait
        assert ds.blocked() == [ids[i] for i, w in enumerate(wait) if w["queued"]]
        seen["blocked"] += sum(1 for w in wait if w["queued"])
        clocks = []
        for i, log in enumerate(logs):
            seqs = {}
            for c in log[:len(log) // 2 + 1]:
                seqs[c["actor"]] = max(seqs.get(c["actor"], 0), c["seq"])
            names = [a for a in rng.permutation(sorted(seqs))[:int(rng.integers(0, len(seqs) + 1))]]
            clocks.append({str(a): int(rng.integers(0, seqs[a] + 1)) for a in names})
        for flags in ALL_FLAGS:
            got = ds.missing_changes(ids, clocks, flags)
            assert got == [docset_changes_want(logs[i], clocks[i], flags) for i in range(len(docs))], flags
            seen["changes"] += sum(len(g) for g in got)
        req = [(i, base_clock(c), assigned(c)) for i, (_, dropped) in enumerate(docs) for c in dropped]
        for i, log in enumerate(logs):                      # and what the document's own last change touched, from a clock of ours
            req.append((i, clocks[i], (assigned(log[-1]) if log else []) + [("no-such-object", "k")]))
        got = ds.fields([ids[i] for i, _, _ in req], [c for _, c, _ in req], [f for _, _, f in req])
        want = [docset_fields_want(logs[i], c, f) for i, c, f in req]
        assert got == want
        seen["late"] += sum(1 for w in want if not w["ready"])
        seen["rows"] += sum(len(f) for w in want for f in w["fields"])
        seen["uncovered"] += sum(1 for w in want for f in w["fields"] for x in f if not x["covered"])
    print(strides, dict(seen))
    assert strides[0] == 8 and strides[-1] > 8
    assert seen["blocked"] >= 10 and seen["late"] >= 5 and seen["uncovered"] > 0 and seen["rows"] > 50 and seen["changes"] > 500, seen


# ---- (d) the second trip of the grid-stride loops ---------------------------------------------------------
KINDS = ("full", "late", "empty", "blocked")
BLOCKED = [[ch(A, 1, {}, s("x", 1)), ch(A, 3, {}, s("x", 3)), ch(B, 1, {Cc: 2}, s("y", 1)), ch(B, 2, {D: 1}, s("y", 2))],
           [ch(B, 1, {A: 1}, s("y", 2)), ch(Cc, 1, {D: 1}, s("q", 9)), ch(A, 1, {}, s("x", 1)), ch(A, 1, {}, s("x", 1)),
            ch(A, 2, {B: 1}, s("x", 5)), ch(D, 2, {}, s("w", 1))]]
LIST_DOC = [ch(A, 1, {}, mk("makeList", "L"), link("l", "L"), ins("L", "_head", 1), s("aaaa:1", "x", obj="L"),
               ins("L", "aaaa:1", 2), s("aaaa:2", "y", obj="L")),
            ch(B, 1, {A: 1}, s("aaaa:1", "b", obj="L"), ins("L", "_head", 1), s("bbbb:1", "z", obj="L")),
            ch(A, 2, {}, s("aaaa:1", "a2", obj="L"), {"action": "del", "obj": "L", "key": "aaaa:2"})]


@pytest.fixture(scope="module")
def tiny(engine):
    """40 tiny documents, two blocked ones, a list document and an empty handle in one store"""
    docs = [chain_doc(3 + i % 5, 1 + i % 2) for i in range(40)] + BLOCKED + [LIST_DOC]
    store = DocStore(engine, a_stride=8)
    hs = [store.open() for _ in docs]
    res = store.apply(list(zip(hs, docs)))
    assert (res.docs["status"] == 0).all() and [int(x) for x in res.docs["n_queued"][40:42]] == [3, 2]
    empty = store.open()
    return store, {"full": hs[:40] + [hs[42]], "late": hs[:40], "blocked": hs[40:42], "empty": [empty]}


def kind_of(q, n_first=GRID):
    """Request q's kind: request q + n_first — the same workgroup's next — is of another kind, and
    over q < 12 every ordered pair of distinct kinds occurs."""
    if q < n_first:
        return KINDS[q % 4]
    k = q - n_first
    return KINDS[(k + 1 + (k // 4) % 3) % 4]


def second_trip_kinds(n, n_first=GRID):
    kinds = [kind_of(q, n_first) for q in range(n)]
    pairs = {(kinds[q], kinds[q + n_first]) for q in range(n - n_first)}
    assert len(pairs) == 12 and all(a != b for a, b in pairs)
    return kinds


def by_kind(tiny, n, make, n_first=GRID, variants=7):
    """n requests: request q = make(kind, handle, variant), over a small pool per kind, so that the
    distinct requests stay a few hundred.  Returns (requests, index of every request's first equal)."""
    _, pool = tiny
    req, first, rep = [], {}, []
    for q, kind in enumerate(second_trip_kinds(n, n_first)):
        hs = pool[kind]
        key = (kind, hs[(q // 4) % len(hs)], (q // 3) % variants)
        if key not in first:
            first[key] = (q, make(*key))
        rep.append(first[key][0])
        req.append(first[key][1])
    return req, np.array(rep)


def entries_for(store, cref, kind, h, v):
    return entries_of(cref.clock(h), len(store.enc[h].actors), kind, h, v)


def entries_of(clock, na, kind, h, v):
    """ordered entries of a request: ready ones for full / blocked, one past the clock for late"""
    rng = np.random.default_rng(1000 * h + v)
    if kind == "empty":
        return [[], [(0, 0)], [(0, 3), (7, 1)], [(5, 0), (2, 0)]][v % 4]
    ents = fields_have(rng, clock, na, late=kind == "late")
    if kind == "late" and not ents:
        ents = [(0, int(clock[0]) + 1)]
    return ents


def test_second_trip_missing_changes(tiny):
    """65,535 + 600 requests in one call: the 600 of the second trip differ in kind from the request
    their workgroup answered first.  Every distinct request against the reference, every other one
    against its first equal.  Then a bad handle on the first trip and a repeated-rank request on the
    second: the store call is refused (it copies nothing back then: the tables of a refused call
    are read in test_second_trip_refused_requests_device_forms), and the same call without them
    is right.  Wall 0.6 s."""
    store, pool = tiny
    cref = ChangesRef(store)
    n = GRID + 600
    req, rep = by_kind(tiny, n, lambda kind, h, v: (h, entries_for(store, cref, kind, h, v)))
    hs, have = [h for h, _ in req], [e for _, e in req]
    distinct = np.unique(rep)
    assert 100 < len(distinct) < 1000
    answers = {}
    for flags in (0, FOR_ACTOR):
        got, clo = answers[flags] = store.missing_changes_rows(hs, have, flags)
        for q in distinct:
            want, deps = cref(hs[q], have[q], flags)
            assert got[q] == want and [int(x) for x in clo[q]] == deps, (q, hs[q], have[q], flags)
        assert got == [got[q] for q in rep], np.flatnonzero([g != got[q] for g, q in zip(got, rep)])[:5]
        np.testing.assert_array_equal(clo, clo[rep])
    whole = answers[0][0]
    assert sum(1 for q in range(GRID, n) if whole[q]) >= 100 and sum(1 for q in range(GRID, n) if not whole[q]) >= 100
    bad = list(have)
    bad[GRID + 7] = [(0, 1), (1, 1), (0, 2)]
    with pytest.raises(Exception, match="repeated"):
        store.missing_changes_rows(hs, bad)
    with pytest.raises(Exception, match="bad handle"):
        store.missing_changes_rows(hs[:3] + [9999] + hs[4:], have)
    assert store.missing_changes_rows(hs, have, FOR_ACTOR)[0] == got


def raw_fields(store, hs, have, fields, cap):
    """hm_store_fields with every output table, whatever the status"""
    hs = np.ascontiguousarray(hs, np.uint32)
    n = len(hs)
    off, ea, es = pack_entries(have, n)
    foff, freg = pack_fields(fields, n)
    nf = int(foff[-1])
    flags, rng = np.full(n, 77, np.uint32), np.full((nf + 1, 2), 77, np.uint32)
    clo, rows, tot = np.full((n, store.S), 77, np.uint32), np.zeros(cap, FIELD_OP_DT), ctypes.c_uint32(77)
    st = store._L.hm_store_fields(store._h, n, hs.ctypes.data, off.ctypes.data, ea.ctypes.data, es.ctypes.data, foff.ctypes.data,
                                  freg.ctypes.data, flags.ctypes.data, clo.ctypes.data, rng.ctypes.data, rows.ctypes.data, cap,
                                  ctypes.byref(tot))
    return st, flags, clo, rng[:nf], foff, tot.value


def test_second_trip_fields(tiny):
    """The same 66,135 requests as field requests (every register, one past the last, one repeated):
    ready flags, closure rows and every field's rows.  Then, through the raw call, a bad-rank request,
    a repeated-rank request and a bad handle on either trip: the call is refused, those requests'
    flags, closure rows and ranges are zero, and the requests their workgroups answer on the other
    trip keep their flags, closure rows and row counts (a refused store call does not copy the row
    table back: test_second_trip_refused_requests_device_forms reads the neighbours' rows).  Wall 1.2 s."""
    store, pool = tiny
    cref, fref = ChangesRef(store), FieldsRef(store)

    def make(kind, h, v):
        nr = fref.n_regs(h)
        regs = list(range(nr)) + [nr] + ([v % nr] * 2 if nr else [0])
        return h, entries_for(store, cref, kind, h, v), regs[v % 2:]
    n = GRID + 600
    req, rep = by_kind(tiny, n, make)
    hs, have, fields = [r[0] for r in req], [r[1] for r in req], [r[2] for r in req]
    distinct = np.unique(rep)
    got, clo = store.fields_rows(hs, have, fields)
    kinds = second_trip_kinds(n)
    n_rows = n_unc = 0
    for q in distinct:
        ready, deps, want = fref(hs[q], have[q], fields[q])
        assert (got[q][0], [int(x) for x in clo[q]], [rows_of(f) for f in got[q][1]]) == (ready, deps, want), (q, req[q])
        assert ready == (kinds[q] != "late" and not (kinds[q] == "empty" and any(sq for _, sq in have[q]))), (q, req[q])
        n_rows += sum(len(f) for f in want)
        n_unc += sum(1 for f in want for x in f if not x[7])
    np.testing.assert_array_equal(clo, clo[rep])
    flat = [(g[0], [f.tobytes() for f in g[1]]) for g in got]
    assert flat == [flat[q] for q in rep], np.flatnonzero([x != flat[q] for x, q in zip(flat, rep)])[:5]
    late2 = sum(1 for q in range(GRID, n) if not got[q][0])
    assert n_rows > 500 and n_unc > 50 and 100 <= late2 <= 500, (n_rows, n_unc, late2)
    # refused requests on either trip
    cap = sum(len(f) for g in got for f in g[1])
    st, flags, rclo, rng, foff, tot = raw_fields(store, hs, have, fields, cap)
    assert st == 0 and tot == cap
    wrong = {5: [(8, 1)], 6: [(0, 1), (1, 1), (0, 2)], 7: None, GRID + 9: [(9, 0)], GRID + 10: [(2, 0), (2, 0)], GRID + 12: None}
    bad, bad_hs = list(have), list(hs)
    for q, e in wrong.items():
        if e is None:
            bad_hs[q] = 9999                                        # a handle the store never opened
        else:
            bad[q] = e
    st2, flags2, rclo2, rng2, _, _ = raw_fields(store, bad_hs, bad, fields, cap)
    assert st2 == INVALID
    ok = np.ones(n, bool)
    ok[list(wrong)] = False
    np.testing.assert_array_equal(flags2[ok], flags[ok])
    np.testing.assert_array_equal(rclo2[ok], rclo[ok])
    fok = np.repeat(ok, np.diff(foff.astype(np.int64)))
    np.testing.assert_array_equal(rng2[fok, 1], rng[fok, 1])
    for q in wrong:
        assert int(flags2[q]) == 0 and not rclo2[q].any() and not rng2[int(foff[q]):int(foff[q + 1])].any(), q
        other = q + GRID if q < GRID else q - GRID
        assert ok[other] and [int(c) for c in rng2[int(foff[other]):int(foff[other + 1]), 1]] == [len(f) for f in got[other][1]]
    for e, msg in (([(8, 1)], "rank"), ([(0, 1), (1, 1), (0, 2)], "repeated")):
        bad = list(have)
        bad[GRID + 11] = e
        with pytest.raises(Exception, match=msg):
            store.fields_rows(hs, bad, fields)


def field_rows(rows):
    """fields_ref rows as FIELD_OP_DT bytes"""
    t = np.zeros(len(rows), FIELD_OP_DT)
    for i, (op, action, dt, vtag, value, a, q, cov) in enumerate(rows):
        t[i] = (op, q, a, action, dt, vtag, int(cov), 0, value)
    return t.tobytes()


def test_second_trip_refused_requests_device_forms(engine):
    """changes_kernel and fields_kernel through hm_missing_changes_device / hm_fields_device, where a
    refused call's `bad` word and tables can be read: the tiny documents tiled into a cold batch of
    66,135 (request q = document q), a bad-rank and a repeated-rank request on each trip.  The `bad`
    words name both, the refused requests' ranges, closure rows and flags are zero, and every other
    request — the ones the same workgroups answer 65,535 requests earlier or later among them — has its
    reference's range contents, closure row, ready flag and field rows.  (A cold batch has no handles:
    the bad handle is in the store-form tests.)  Wall 0.7 s."""
    docs = [chain_doc(3 + i % 5, 1 + i % 2) for i in range(40)] + BLOCKED + [LIST_DOC, []]
    small = encode(docs, 8)
    so = O.merge(small)
    assert (so.docs["status"] == 0).all()
    pool = {"full": list(range(40)) + [42], "late": list(range(40)), "blocked": [40, 41], "empty": [43]}

    def make(kind, d, v):
        ents = entries_of(so.clock[d * 8:(d + 1) * 8], len(small.doc_actors[d]), kind, d, v)
        nr = int(small.docs["n_regs"][d])
        return d, ents, (list(range(nr)) + [nr] + ([v % nr] * 2 if nr else [0]))[v % 2:]
    n = GRID + 600
    req, rep = by_kind((None, pool), n, make)
    src = np.array([r[0] for r in req])
    b = slice_changes(small, np.zeros(small.n_docs, np.int64), small.docs["n_changes"], docs=src)
    b.docs["reg_off"] = np.cumsum(b.docs["n_regs"]) - b.docs["n_regs"]
    o = O.merge(b, threads=8)
    assert (o.docs["status"] == 0).all()
    have, fields = [r[1] for r in req], [r[2] for r in req]
    wrong = {5: [(8, 1)], 6: [(0, 1), (1, 1), (0, 2)], GRID + 9: [(9, 0)], GRID + 10: [(2, 0), (2, 0)]}
    for q, e in wrong.items():
        have[q] = e
    want = {}
    for q in range(n):                                            # one reference answer per distinct request
        if q not in wrong and rep[q] not in want:
            d, ents, regs = req[q]
            chg, deps = missing_changes_ref.doc_ref(small, so, d, ents)
            ready, fdeps, rows = fields_ref.doc_ref(small, so, d, ents, regs)
            want[rep[q]] = (chg, deps, ready, fdeps, [field_rows(f) for f in rows])
    assert 100 < len(want) < 1000
    good = [q for q in range(n) if q not in wrong]
    n_log = sum(len(want[rep[q]][0]) for q in good)
    n_rows = sum(len(f) // FIELD_OP_DT.itemsize for q in good for f in want[rep[q]][4])
    _, (rg, log, clo, tot, bad), (fl, frg, rows, fclo, ftot, fbad) = device_queries(engine, b, o, have, fields, n_log, n_rows)
    assert (tot, bad, ftot, fbad) == (n_log, 2 | 4, n_rows, 2 | 4)       # HM_MC_ / HM_FD_ BAD_RANK | BAD_REPEAT
    foff = pack_fields(fields, n)[0]
    for q in wrong:
        assert not rg[q].any() and not clo[q].any() and int(fl[q]) == 0 and not fclo[q].any(), q
        assert not frg[int(foff[q]):int(foff[q + 1])].any(), q
    raw = rows.view(np.uint8).reshape(-1, FIELD_OP_DT.itemsize)
    checked = 0
    for q in good:
        chg, deps, ready, fdeps, per = want[rep[q]]
        a, c = int(rg[q, 0]), int(rg[q, 1])
        assert [int(x) for x in log[a:a + c]] == chg and [int(x) for x in clo[q]] == deps, (q, req[q])
        got = [raw[int(x):int(x) + int(y)].tobytes() for x, y in frg[int(foff[q]):int(foff[q + 1])]]
        assert ((int(fl[q]) == 0), [int(x) for x in fclo[q]], got) == (ready, fdeps, per), (q, req[q])
        checked += q >= GRID or q + GRID in wrong
    for q in wrong:                                               # the same workgroup's other request was among them
        assert (q + GRID if q < GRID else q - GRID) in good
    assert checked >= 598


def ranges_for(src, kind, v):
    """a history slice: whole or inner for full / blocked, empty or inverted for late, anything for empty"""
    H = hist_len(src)
    if kind == "late":
        return [(H, H + 3), (2, 2), (5, 3), (H + 4, H + 9)][v % 4]
    if kind == "empty":
        return [(0, 0), (0, 7), (3, 1), (2, 9)][v % 4]
    return [(0, H), (0, H + 7), (0, 1), (H // 2, H), (max(H - 1, 0), H), (H // 3, H // 2 + 1), (1, H)][v % 7]


def test_second_trip_op_diffs(tiny):
    """od_walk_kernel: 66,135 history slices in the two-pass call with lists=True, against
    tests/list_diffs_ref.py (test_list_diffs_gpu.check memoizes the distinct ones).  Wall 0.1 s."""
    store, pool = tiny
    hs_all = sorted({h for v in pool.values() for h in v})
    srcs = {h: diff_source(store, h) for h in hs_all}
    n = GRID + 600
    req, rep = by_kind(tiny, n, lambda kind, h, v: (h,) + ranges_for(srcs[h][0], kind, v))
    want = check_element_diffs(store, srcs, [r[0] for r in req], [r[1] for r in req], [r[2] for r in req], memo={})
    cnt = want[2][:, 1]
    assert (cnt[GRID:] > 0).sum() >= 100 and (cnt[GRID:] == 0).sum() >= 100 and len(want[0]) > n
    assert {3, 4, 5} & {int(k) for k in want[0][:, 1]}            # element rows of the list document


def clocks_for(src, S, kind, v):
    H = hist_len(src)
    if kind == "late":                                             # a clock that selects nothing, or leaves changes queued
        k = clock_at(src, S, H)
        if v % 2 or not k.any():
            return np.zeros(S, np.uint32)
        k[int(np.flatnonzero(k)[0])] = 0
        return k
    if kind == "empty":
        return [np.zeros(S, np.uint32), np.full(S, 0xFFFFFFFF, np.uint32)][v % 2]
    return clock_at(src, S, [H, H // 2, 1, max(H - 1, 0)][v % 4])


def test_second_trip_op_diffs_at(tiny):
    """od_walk_kernel through hm_store_op_diffs_at: 66,135 clocks, element rows asked, against
    tests/clock_diffs_ref.py.  Wall 0.1 s."""
    store, pool = tiny
    hs_all = sorted({h for v in pool.values() for h in v})
    srcs = {h: diff_source(store, h) for h in hs_all}
    n = GRID + 600
    req, rep = by_kind(tiny, n, lambda kind, h, v: (h, clocks_for(srcs[h][0], 8, kind, v)), variants=4)
    want = check_diffs_at(store, srcs, [r[0] for r in req], [r[1] for r in req], memo={}, lists=(True,))
    cnt = want[2][:, 1]
    assert (cnt[GRID:] > 0).sum() >= 100 and (cnt[GRID:] == 0).sum() >= 100 and len(want[0]) > n


def test_second_trip_materialize(tiny):
    """past_fill_kernel: 66,135 documents gathered at history lengths in one call, through
    test_materialize_gpu.check (the gathered batch against tests/past_ref.py, its merge against the
    oracle's).  past_count_kernel launches min(ceil(n / 4), 65,535) workgroups of four waves and
    strides on, so it takes a second trip only above 262,140 requests; it is not brought there (its
    loop keeps nothing in LDS between requests).  Wall 2.0 s."""
    store, pool = tiny
    hs_all = sorted({h for v in pool.values() for h in v})
    srcs = {h: past_source(store, h) for h in hs_all}

    def make(kind, h, v):
        H = hist_len(srcs[h])
        if kind == "late":                                         # nothing, or past the end
            return h, [0, H + 5][v % 2]
        return h, [0, 3][v % 2] if kind == "empty" else [H, H // 2, 1, max(H - 1, 0)][v % 4]
    n = GRID + 600
    req, rep = by_kind(tiny, n, make, variants=4)
    want, o = check_materialize(store, srcs, [r[0] for r in req], history=[r[1] for r in req])
    nc = want.docs["n_changes"]
    assert (nc[GRID:] > 0).sum() >= 100 and (nc[GRID:] == 0).sum() >= 100 and (o.docs["status"] == 0).all()


def test_second_pass_waiting(tiny):
    """waiting_kernel launches at most 4,096 workgroups of four waves (hm_launch_waiting) and
    strides on: 16,384 + 600 requests take a wave through a second document, its LDS row behind it.
    blocked_kernel's grid is capped at 2,048 workgroups of 256 handles; a store of more than 524,288
    handles is not built here.  Wall under 0.1 s."""
    store, pool = tiny
    n = WAIT_PASS + 600
    kinds = second_trip_kinds(n, WAIT_PASS)
    hs = [pool[k][(q // 4) % len(pool[k])] for q, k in enumerate(kinds)]
    miss, unmet, nq = store.waiting(hs)
    off, queue = store.queues(hs, nq)
    one = {h: expected(store, h) for h in set(hs)}
    np.testing.assert_array_equal(miss, np.stack([one[h][0] for h in hs]))
    np.testing.assert_array_equal(nq, [one[h][2] for h in hs])
    np.testing.assert_array_equal(queue, np.concatenate([np.array(one[h][1], np.uint32) for h in hs]))
    assert not unmet.any()
    assert (nq[WAIT_PASS:] > 0).sum() == 150 and (miss[WAIT_PASS:].any(axis=1)).sum() == 150
