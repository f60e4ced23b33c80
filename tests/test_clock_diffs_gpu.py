"""A document's per-op patch at a clock on the device (hm_store_op_diff_sizes_at / hm_store_op_diffs_at
/ hm_op_diffs_at_host / hm_op_diffs_at_device): rows, survivors, indices, ranges, flags and totals
against the restatement in tests/clock_diffs_ref.py (pinned on both oracles by
tests/test_clock_diffs_ref.py), bit for bit; where the clock is a history prefix's, also against the
existing device call on [0, p)."""
import ctypes

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import NONE, SURV_RESULT_DT, CBatch, CResults, decode_doc
from hypermerge_amd.engine import OD_LISTS, OP_DIFF_DT, COpDiffOut, COpDiffSummary, EngineError

from clock_diffs_ref import applied_at, census, clock_diffs, clocks_of, pack
from fuzz_docs import gen_doc, gen_docs
from kat_cases import A, B, Cc, ch, d, s
from list_diffs_cases import LHAND, e, long_text
from list_diffs_ref import ELEM_INSERT, ELEM_REMOVE, ELEM_SET
from op_diffs_cases import HAND, chain_doc, wide_doc
from past_ref import clock_at, hist_len
from test_list_diffs_gpu import merged, same5
from test_op_diffs_gpu import T, opened, same

pytestmark = pytest.mark.gpu

NOMEM, INVALID = 34, 32


def expected(srcs, S, hs, clocks, lists, memo=None):
    memo = {} if memo is None else memo
    res = []
    for h, k in zip(hs, clocks):
        key = (int(h), bytes(np.asarray(k, np.uint32)), lists)
        if key not in memo:
            memo[key] = clock_diffs(*srcs[int(h)], S, k, lists)
            assert not lists or memo[key].diffs.bad == 0
        res.append(memo[key])
    t = pack(res, lists)
    out = (np.array(t[0], np.uint32).reshape(-1, 4), np.array([tuple(x) for x in t[1]], SURV_RESULT_DT),
           np.array(t[2], np.uint32).reshape(-1, 2), np.array(t[3], np.uint32))
    return out + (np.array(t[4], np.uint32),) if lists else out


def rows_of(hs, clocks, S):
    return np.ascontiguousarray(hs, np.uint32), np.ascontiguousarray(np.array(clocks, np.uint32).reshape(len(hs), S))


def check(store, srcs, hs, clocks, memo=None, lists=(True, False)):
    """both option words; returns the expectation with lists (without, when only that is asked)"""
    hs, ks = rows_of(hs, clocks, store.S)
    want = None
    for opt in lists:
        w = expected(srcs, store.S, hs, ks, opt, memo)
        got = store.op_diffs_at(hs, ks, lists=opt)
        (same5 if opt else same)(got, w, f"lists={opt}")
        cnt, fl, tot = store.op_diff_sizes_at(hs, ks, lists=opt)
        np.testing.assert_array_equal(cnt[:, 0], w[2][:, 1])
        np.testing.assert_array_equal(fl, w[3])
        assert [int(x) for x in tot] == [len(w[0]), len(w[1])]
        want = w if opt or want is None else want
    return want


def asked(srcs, hs, S, rng, **kw):
    """(handles, clocks, kinds, prefix lengths | None) of clocks_of per document, in one call's order"""
    req, ks, kinds = [], [], []
    for h in hs:
        for kind, k in clocks_of(*srcs[h], S, rng, **kw):
            req.append(h); ks.append(k); kinds.append(kind)
    return req, ks, kinds


def prefixes_agree(store, srcs, hs):
    """a prefix's clock gives what the existing call gives on [0, p), table for table"""
    req, ks, ps = [], [], []
    for h in hs:
        H = hist_len(srcs[h][0])
        for p in sorted({0, min(1, H), H // 2, H}):
            req.append(h); ks.append(clock_at(srcs[h][0], store.S, p)); ps.append(p)
    r, k = rows_of(req, ks, store.S)
    for opt in (True, False):
        at, ex = store.op_diffs_at(r, k, lists=opt), store.op_diffs(r, [0] * len(r), ps, lists=opt)
        assert len(at) == len(ex) and all(x.tobytes() == y.tobytes() for x, y in zip(at, ex)), opt


# ---- generated documents at strides 8, 16 and 64 --------------------------------------------------------
@pytest.mark.parametrize("S,docs", [(8, lambda: gen_docs("default", range(100, 116))),
                                    (16, lambda: [gen_doc(300 + i, n_actors=9 + i, profile="wide") for i in range(8)] + gen_docs("default", range(116, 120))),
                                    (64, lambda: gen_docs("wide", range(200, 212)))])
def test_fuzz_documents_at_prefix_causal_past_and_cut_clocks(engine, S, docs):
    store, hs, srcs = opened(engine, docs(), S)
    req, ks, kinds = asked(srcs, hs, S, np.random.default_rng(S))
    n, closed, queued = census([(*srcs[h], S, k) for h, k in zip(req, ks)])
    assert 4 * closed >= n and 4 * queued >= n, (n, closed, queued)
    want = check(store, srcs, req, ks, memo={})
    assert {ELEM_INSERT, ELEM_SET, ELEM_REMOVE} <= {int(k) for k in want[0][:, 1]}
    prefixes_agree(store, srcs, hs)


def test_one_wide_document_at_stride_256(engine):
    store, hs, srcs = opened(engine, [wide_doc(200)], 256)
    src, ad = srcs[hs[0]]
    req, ks, kinds = asked(srcs, hs, 256, np.random.default_rng(256), n_past=3, n_cut=3)
    last = len(src.changes) - 1                                               # (knows one side of rank 64 only)
    from clock_diffs_ref import causal_past
    ks.append(causal_past(src, ad, 256, last)); req.append(hs[0])
    assert 0 < int(applied_at(src, ad, 256, ks[-1]).sum()) < hist_len(src)
    check(store, srcs, req, ks, memo={})
    prefixes_agree(store, srcs, hs)


def test_the_zero_clock_and_a_clock_above_every_seq(engine):
    store, hs, srcs = opened(engine, [HAND[k] for k in sorted(HAND)] + [LHAND["two_lists"][0]])
    zero, top = np.zeros(8, np.uint32), np.full(8, 0xFFFFFFFF, np.uint32)
    req, ks = hs + hs, [zero] * len(hs) + [top] * len(hs)
    want = check(store, srcs, req, ks)
    assert not want[2][:len(hs), 1].any() and want[2][len(hs):, 1].all()
    r, k = rows_of(hs, [top] * len(hs), 8)
    for opt in (True, False):
        at, ex = store.op_diffs_at(r, k, lists=opt), store.op_diffs(r, [0] * len(hs), [hist_len(srcs[h][0]) for h in hs], lists=opt)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(at, ex))


# ---- histories that span tiles ---------------------------------------------------------------------------
def test_clocks_cutting_inside_the_first_and_the_second_tile(engine):
    lens = [T - 1, T, T + 1, 2 * T + 76]
    store, hs, srcs = opened(engine, [chain_doc(n, n_keys=40, actors=(A, B)) for n in lens])
    req, ks = [], []
    for h, n in zip(hs, lens):
        src, ad = srcs[h]
        assert hist_len(src) == n
        full = clock_at(src, 8, n)
        for cut in (T // 3, T - 2, T + 40, n):                               # positions inside tile 0, at its end, inside tile 1
            k = clock_at(src, 8, min(cut, n))
            req.append(h); ks.append(k)
            low = full.copy()                                                # one actor held back: the other's later changes queue
            low[0] = k[0]
            req.append(h); ks.append(low)
    n, closed, queued = census([(*srcs[h], 8, k) for h, k in zip(req, ks)])
    assert queued >= 4
    check(store, srcs, req, ks, memo={}, lists=(False,))
    prefixes_agree(store, srcs, hs)


# ---- resident logs holding queued and duplicate changes --------------------------------------------------
@pytest.fixture(scope="module")
def c5():
    b = synth.generate(synth.config("C5", n_docs=16, arrival=2, shuffle_pct=40, dup_pct=15))
    return [decode_doc(b, i) for i in range(b.n_docs)]


def test_queued_and_duplicate_changes_are_never_selected(engine, c5):
    first = LHAND["tombstone_before"][0][0]
    waits = [ch(B, 1, {A: 1}, d(e(A, 2), obj="T"), s(e(A, 1), "B", obj="T")), ch(Cc, 1, {"dddd": 1}, d(e(A, 1), obj="T")), first, first,
             ch(A, 2, {B: 1}, s(e(A, 2), "again", obj="T"))]
    store, hs, srcs = opened(engine, c5 + [waits])
    assert [int(x) for x in srcs[hs[-1]][0].hist] == [1, -1, 0, -2, 2]
    assert any((srcs[h][0].hist == -2).any() for h in hs[:-1])
    req, ks, kinds = asked(srcs, hs, 8, np.random.default_rng(5))
    req += [hs[-1]] * 2
    ks += [np.full(8, 9, np.uint32), np.array([1, 1, 1, 0, 0, 0, 0, 0], np.uint32)]   # (c:1 is selected by no clock)
    want = check(store, srcs, req, ks, memo={})
    assert {ELEM_INSERT, ELEM_SET, ELEM_REMOVE} <= {int(k) for k in want[0][:, 1]}
    assert int(want[2][-2, 1]) == len(clock_diffs(*srcs[hs[-1]], 8, ks[-2], True).diffs.rows) > 0


# ---- lists -----------------------------------------------------------------------------------------------
def test_a_text_document_and_element_indices(engine, c5):
    store, hs, srcs = opened(engine, [long_text(300), c5[0]])
    req, ks, kinds = asked(srcs, hs, 8, np.random.default_rng(9))
    hs_, ks_ = rows_of(req, ks, 8)
    want = expected(srcs, 8, hs_, ks_, True)
    same5(store.op_diffs_at(hs_, ks_, lists=True), want)
    assert (want[4] != NONE).sum() > 100 and int(want[4][want[4] != NONE].max()) >= 5
    plain = store.op_diffs_at(hs_, ks_)                                       # without the option: flagged, no rows
    same(plain, expected(srcs, 8, hs_, ks_, False))
    assert (plain[3] & OD_LISTS).any() and not plain[2][plain[3] != 0, 1].any()


# ---- many requests ---------------------------------------------------------------------------------------
def test_five_thousand_requests_over_tiny_documents(engine):
    docs = [chain_doc(3 + i % 5, 1 + i % 2) for i in range(40)]
    store, hs, srcs = opened(engine, docs)
    rng = np.random.default_rng(50)
    pool = {h: [k for _, k in clocks_of(*srcs[h], 8, rng)] for h in hs}
    req = rng.integers(0, len(hs), size=5000)
    ks = [pool[hs[i]][int(rng.integers(0, len(pool[hs[i]])))] for i in req]
    want = check(store, srcs, [hs[i] for i in req], ks, memo={}, lists=(False,))
    assert len(want[0]) > 5000 and (want[2][:, 1] == 0).any()


# ---- the call itself -------------------------------------------------------------------------------------
class Raw:
    def __init__(self, n, caps):
        fill = lambda k, dt: np.frombuffer(bytes([0xA5]) * (max(k, 1) * np.dtype(dt).itemsize), dt).copy()
        self.bufs = [fill(caps[0], OP_DIFF_DT), fill(caps[1], SURV_RESULT_DT), fill(2 * n, np.uint32), fill(n, np.uint32), fill(caps[0], np.uint32)]
        self.out = COpDiffOut(caps[0], caps[1], *[x.ctypes.data for x in self.bufs[:4]])
        self.tot = np.full(2, 77, np.uint64)

    def untouched(self):
        return all(a.tobytes() == bytes([0xA5]) * a.nbytes for a in self.bufs)

    def tables(self):
        return (self.bufs[0], self.bufs[1], self.bufs[2].reshape(-1, 2), self.bufs[3], self.bufs[4])


def raw_call(store, hs, ks, caps, opts=1):
    hs, ks = rows_of(hs, ks, store.S) if len(hs) else (np.zeros(0, np.uint32), np.zeros((0, store.S), np.uint32))
    R = Raw(len(hs), caps)
    p = lambda a: a.ctypes.data if a.size else None
    st = store._L.hm_store_op_diffs_at(store._h, len(hs), p(hs), p(ks), ctypes.byref(R.out), R.bufs[4].ctypes.data, R.tot.ctypes.data, opts)
    return st, R


def test_capacities_errors_and_untouched_outputs(engine):
    store, hs, srcs = opened(engine, [LHAND[k][0] for k in sorted(LHAND)] + [HAND["tie_flip"]])
    req, ks, kinds = asked(srcs, hs, 8, np.random.default_rng(3), n_past=1, n_cut=1)
    hs_, ks_ = rows_of(req, ks, 8)
    want = expected(srcs, 8, hs_, ks_, True)
    exact = [len(want[0]), len(want[1])]
    assert min(exact) > 1
    for short in range(2):                                                    # one row short in each table in turn
        caps = list(exact)
        caps[short] -= 1
        st, R = raw_call(store, req, ks, caps)
        assert st == NOMEM and [int(x) for x in R.tot] == exact and R.untouched(), short
    st, R = raw_call(store, req, ks, exact)
    assert st == 0 and [int(x) for x in R.tot] == exact
    same5(R.tables(), want, "exact capacities")
    st, R = raw_call(store, [hs[0], 9999], [ks[0], ks[0]], exact)             # a handle outside the store
    assert st == INVALID and R.untouched()
    with pytest.raises(EngineError, match="bad handle"):
        store.op_diffs_at([hs[0], 9999], np.zeros((2, 8), np.uint32))
    st, R = raw_call(store, [], [], [0, 0])                                   # n == 0
    assert st == 0 and not R.tot.any() and R.untouched()
    assert all(len(x) == 0 for x in store.op_diffs_at([], np.zeros((0, 8), np.uint32), lists=True))
    for opts in (2, 3):                                                       # HM_ODF_ONCE is not offered with a clock
        st, R = raw_call(store, req, ks, exact, opts)
        assert st == INVALID and R.untouched()
    assert store._L.hm_store_op_diff_sizes_at(store._h, 1, hs_.ctypes.data, ks_.ctypes.data, None, None, None, 2) == INVALID
    store.submit([(hs[-1], [ch(A, 9, {}, s("x", 4))])])                       # a batch in flight
    st, R = raw_call(store, req, ks, exact)
    assert st == INVALID and R.untouched()
    with pytest.raises(EngineError, match="in flight"):
        store.op_diff_sizes_at(hs_, ks_)
    store.wait()
    same5(store.op_diffs_at(hs_, ks_, lists=True), want, "after the wait")


# ---- cold batches ----------------------------------------------------------------------------------------
def device_call(engine, b, r, req, ks, caps):
    """hm_op_diffs_at_device over the batch uploaded as it is, the per-document maxima as launch hints"""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    hs_, ks_ = rows_of(req, ks, b.a_stride)
    t = [up(x) for x in (b.docs, b.changes, b.deps, b.ops, r.docs, r.hist, r.all_deps, hs_, ks_)]
    cb = CBatch(b.n_docs, len(b.changes), len(b.deps), len(b.ops), int(b.docs["n_regs"].sum()), b.a_stride, int(b.docs["n_changes"].max()),
                int(b.docs["n_ops"].max()), int(b.docs["n_regs"].max()), int(b.docs["n_objs"].max()), 0, 0, t[0].data_ptr(), t[1].data_ptr(),
                t[2].data_ptr(), t[3].data_ptr(), None)
    cr = CResults(t[4].data_ptr(), None, None, None, t[5].data_ptr(), t[6].data_ptr(), None, None)
    nq = len(req)
    z = lambda nbytes: torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)
    down = lambda x, dt, k: np.frombuffer(x.cpu().numpy().tobytes()[:k * np.dtype(dt).itemsize], dt)
    wb = engine.op_diffs_at_work_bytes(cb, nq, lists=True)
    assert wb > engine.op_diffs_work_bytes(cb, nq, lists=True)                # (the bitmap words)
    g = [z(caps[0] * 16), z(caps[1] * 16), z(nq * 8), z(nq * 4), z(caps[0] * 4)]
    summ, work = z(64), z(wb)
    out = COpDiffOut(caps[0], caps[1], *[x.data_ptr() for x in g[:4]])
    torch.cuda.synchronize()
    engine.op_diffs_at_device(cb, cr, nq, t[7].data_ptr(), t[8].data_ptr(), out, summ.data_ptr(), work.data_ptr(),
                              torch.cuda.current_stream().cuda_stream, lists=True, out_index=g[4].data_ptr())
    torch.cuda.synchronize()
    tables = (down(g[0], OP_DIFF_DT, caps[0]), down(g[1], SURV_RESULT_DT, caps[1]), down(g[2], np.uint32, 2 * nq).reshape(-1, 2),
              down(g[3], np.uint32, nq), down(g[4], np.uint32, caps[0]))
    return tables, COpDiffSummary.from_buffer_copy(summ.cpu().numpy().tobytes())


def test_cold_batch_host_and_device_forms_equal_the_store_form(engine, c5):
    docs = c5[:5] + [LHAND[k][0] for k in sorted(LHAND)] + [chain_doc(70, 3), gen_doc(101)]
    b, r, srcs = merged(engine, docs)
    req, ks, kinds = asked(srcs, list(range(b.n_docs)), b.a_stride, np.random.default_rng(11))
    hs_, ks_ = rows_of(req, ks, b.a_stride)
    want = expected(srcs, b.a_stride, hs_, ks_, True)
    same5(engine.op_diffs_at_host(b, r, hs_, ks_, lists=True), want, "host tables")
    same(engine.op_diffs_at_host(b, r, hs_, ks_), expected(srcs, b.a_stride, hs_, ks_, False), "host tables, no lists")
    caps = (len(want[0]), len(want[1]))
    tables, sm = device_call(engine, b, r, req, ks, caps)
    assert list(sm.totals)[:2] == list(caps) and sm.bad == 0 and sm.flags == 0
    same5(tables, want, "device tables")
    store, hs, _ = opened(engine, docs)                                       # the resident form of the same logs
    by_id = [{a: int(k[x]) for x, a in enumerate(b.doc_actors[i]) if k[x]} for i, k in zip(req, ks)]
    by_id[0]["an actor the document never saw"] = 7
    same5(store.op_diffs_at([hs[i] for i in req], by_id, lists=True), want, "store, clocks by actor id")
    same5(store.op_diffs_at([hs[i] for i in req], ks_, lists=True), want, "store, rank rows")
