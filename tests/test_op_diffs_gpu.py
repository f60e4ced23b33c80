"""Per-op diffs of history slices on the device (hm_store_op_diff_sizes / hm_store_op_diffs /
hm_op_diffs_device / hm_op_diffs_host): rows, survivors, ranges and flags against the sequential
restatement in tests/op_diffs_ref.py (pinned on both oracles by tests/test_op_diffs_ref.py), bit for
bit."""
import ctypes
import os
import re

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import SURV_RESULT_DT, CBatch, CResults
from hypermerge_amd.engine import OD_LISTS, OP_DIFF_DT, COpDiffOut, COpDiffSummary, EngineError
from hypermerge_amd.store import DocStore, RowStore, slice_changes
import oracle.oracle as O

from kat_cases import A, ch, s
from op_diffs_cases import HAND, TIE_FLIP_ORDERS, chain_doc, one_register_doc, wide_doc
from op_diffs_ref import CREATE, REMOVE, SET_ROW, op_diffs, pack
from past_ref import hist_len, source_of

pytestmark = pytest.mark.gpu

NOMEM, INVALID = 34, 32
_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hypermerge_amd", "csrc", "op_diff_kernels.h")
T = int(re.search(r"#define HM_OD_TILE (\d+)u", open(_H).read()).group(1))       # history positions per bitmap tile


def enc_source(store, h):
    """a DocStore document's log (from its host encoder) with the oracle's hist and all_deps rows"""
    b = store.enc[h].log_batch(store.S)
    o = O.merge(b)
    assert int(o.docs["status"][0]) == 0
    return source_of(b, o.hist, 0), np.asarray(o.all_deps).reshape(-1, store.S).copy()


def batch_sources(b, o, hs):
    S, out = b.a_stride, {}
    for i, h in enumerate(hs):
        c0, nc = int(b.docs["change_off"][i]), int(b.docs["n_changes"][i])
        out[int(h)] = (source_of(b, o.hist, i), np.asarray(o.all_deps).reshape(-1, S)[c0:c0 + nc].copy())
    return out


def expected(srcs, S, hs, frm, to, memo=None):
    memo = {} if memo is None else memo
    res = []
    for h, f, t in zip(hs, frm, to):
        key = (int(h), int(f), int(t))
        if key not in memo:
            memo[key] = op_diffs(*srcs[int(h)], S, int(f), int(t))
        res.append(memo[key])
    rows, surv, rng, fl = pack(res)
    return (np.array(rows, np.uint32).reshape(-1, 4), np.array([tuple(x) for x in surv], SURV_RESULT_DT),
            np.array(rng, np.uint32).reshape(-1, 2), np.array(fl, np.uint32), res)


def same(got, want, what=""):
    rows, surv, rng, fl = got
    wrows, wsurv, wrng, wfl = want[:4]
    np.testing.assert_array_equal(fl, wfl, err_msg=f"flags {what}")
    np.testing.assert_array_equal(rng, wrng, err_msg=f"ranges {what}")
    np.testing.assert_array_equal(np.stack([rows[f] for f in ("op", "kind", "n_surv", "surv_off")], 1).reshape(-1, 4), wrows,
                                  err_msg=f"rows {what}")
    assert surv.tobytes() == wsurv.tobytes(), f"survivors {what}"


def check(store, srcs, hs, frm, to, memo=None):
    want = expected(srcs, store.S, hs, frm, to, memo)
    same(store.op_diffs(hs, frm, to), want)
    cnt, fl, tot = store.op_diff_sizes(hs, frm, to)
    np.testing.assert_array_equal(cnt[:, 0], want[2][:, 1])
    np.testing.assert_array_equal(fl, want[3])
    assert [int(x) for x in tot] == [len(want[0]), len(want[1])]
    return want


def opened(engine, docs, S=8):
    store = DocStore(engine, a_stride=S)
    hs = [store.open() for _ in docs]
    res = store.apply(list(zip(hs, docs)))
    assert (res.docs["status"] == 0).all()
    return store, hs, {h: enc_source(store, h) for h in hs}


def ranges_of(H, extra=()):
    """the ranges every document is asked for: whole, empty, inverted, past the end, slices"""
    r = [(0, H), (0, H + 7), (0, 1), (H // 2, H), (max(H - 1, 0), H), (H // 3, H // 2 + 1), (2, 2), (5, 3), (H, H + 3), (H + 4, H + 9)]
    return r + [x for x in extra if x[0] <= H + 1]


# ---- hand cases -----------------------------------------------------------------------------------
def test_hand_cases_in_one_call(engine):
    names = sorted(HAND)
    store, hs, srcs = opened(engine, [HAND[k] for k in names])
    empty = store.open()
    srcs[empty] = enc_source(store, empty)
    req, frm, to = [], [], []
    for h in hs + [empty]:
        for f, t in ranges_of(hist_len(srcs[h][0])):
            req.append(h); frm.append(f); to.append(t)
    want = check(store, srcs, req, frm, to)
    by = {n: h for n, h in zip(names, hs)}
    one = lambda n, f, t: expected(srcs, 8, [by[n]], [f], [t])[4][0]
    # the tie flips as written out by hand; a del gives remove and the re-set a set
    rows, surv, rng, fl = store.op_diffs([by["tie_flip"], by["del_then_reset"]], [0, 0], [9, 9])
    assert [[int(x) for x in surv["op"][int(r["surv_off"]):int(r["surv_off"]) + int(r["n_surv"])]] for r in rows[:5]] == TIE_FLIP_ORDERS
    assert [int(k) for k in rows["kind"][5:]] == [SET_ROW, REMOVE, SET_ROW]
    # three actors in conflict, winner first by rank, then one survivor
    assert [len(sv) for _, _, sv in one("three_actor_conflict_overwrite", 0, 9).rows] == [1, 2, 3, 1]
    # the counter: 10, 15 (the ancestor's inc), 15 (the concurrent inc), 15.5 as a FLOAT
    vals = [sv[0][1:] for _, _, sv in one("counter_int_float", 0, 9).rows]
    assert vals == [(3, 10), (3, 15), (3, 15), (4, int(np.float64(15.5).view(np.uint64)))]
    # the queued change and the duplicate emit nothing: four applied changes
    sq = one("shuffled_queued_duplicate", 0, 99)
    assert len(sq.rows) == 5 and hist_len(srcs[by["shuffled_queued_duplicate"]][0]) == 3
    # survivors that predate `from`
    late = one("survivors_before_from", 4, 5)
    assert [len(sv) for _, _, sv in late.rows] == [3] and late.rows[0][2][1][0] == 1 and late.rows[0][2][2][0] == 0
    # the text document: flagged with no rows once the range holds an element assign, answered before and after
    rows, surv, rng, fl = store.op_diffs([by["text"]] * 4, [0, 0, 2, 3], [2, 3, 3, 4])
    assert [int(x) for x in fl] == [0, OD_LISTS, OD_LISTS, 0] and [int(x) for x in rng[:, 1]] == [4, 0, 0, 1]
    assert [int(k) for k in rows["kind"][:4]] == [CREATE, SET_ROW, SET_ROW, SET_ROW]
    assert any(k == CREATE for k in want[0][:, 1])


# ---- wave-step, op-count, tile and chain boundaries ------------------------------------------------
def test_boundaries(engine):
    docs = [chain_doc(n) for n in (1, 63, 64, 65)]                            # changes around the lane stride
    docs += [chain_doc(85, 3), chain_doc(64, 4), chain_doc(257)]              # 255, 256 and 257 ops
    docs += [one_register_doc(n) for n in (1, 64, 65, 130)]                   # one chain within and across steps
    docs += [[ch(A, 1, {}, s("z", 0)), ch(A, 2, {}, *[s(f"r{i}", i) for i in range(70)]), ch(A, 3, {}, s("r69", 1), s("r0", 2))]]
    store, hs, srcs = opened(engine, docs)
    assert [len(srcs[h][0].ops) for h in hs[4:7]] == [255, 256, 257]
    req, frm, to = [], [], []
    for h in hs:
        for f, t in ranges_of(hist_len(srcs[h][0]), [(63, 65), (64, 65), (1, 64)]):
            req.append(h); frm.append(f); to.append(t)
    want = check(store, srcs, req, frm, to)
    assert int(want[0][:, 2].max()) >= 3                                      # conflicts among the survivors


def test_tile_boundaries(engine):
    lens = [T - 1, T, T + 1, 2 * T + 1]
    store, hs, srcs = opened(engine, [chain_doc(n, n_keys=40) for n in lens])
    req, frm, to = [], [], []
    for h, n in zip(hs, lens):
        assert hist_len(srcs[h][0]) == n
        for f, t in [(0, n), (T - 1, T + 1), (T, n), (n - 1, n + 5), (T - 2, T - 1), (n, n), (n - 3, n - 1)]:
            req.append(h); frm.append(f); to.append(t)
    check(store, srcs, req, frm, to)


def test_stride_128_with_70_actors(engine):
    """conflicts among ranks on both sides of 64: the survivors' order and the covering test read
    columns of both halves of the all_deps row"""
    store, hs, srcs = opened(engine, [wide_doc(70)], S=128)
    H = hist_len(srcs[hs[0]][0])
    rg = [(0, H), (60, 70), (69, H), (H - 2, H), (64, 65)]
    want = check(store, srcs, [hs[0]] * len(rg), [f for f, _ in rg], [t for _, t in rg])
    assert int(want[0][:, 2].max()) == 70
    last = want[4][0].rows
    assert last[-1][1] == SET_ROW and 1 < len(last[-1][2]) < 70               # the late del covers one side only


# ---- the three sources ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c4():
    b = synth.generate(synth.config("C4", n_docs=300))
    o = O.merge(b, threads=8)
    assert (o.docs["status"] == 0).all()
    return b, o, batch_sources(b, o, range(b.n_docs))


def fed(engine, b, rounds, incremental):
    store = RowStore(engine, a_stride=b.a_stride)
    store.set_incremental(incremental)
    h0 = store.open_n(b.n_docs)
    hs = np.arange(h0, h0 + b.n_docs, dtype=np.uint32)
    n = b.docs["n_changes"].astype(np.int64)
    cuts = [np.zeros_like(n)] + [np.maximum(n - 6 * (rounds - k), 0) for k in range(1, rounds + 1)]
    for k in range(rounds):
        store.submit_batch(b if rounds == 1 else slice_changes(b, cuts[k], cuts[k + 1]), hs)
        assert (store.wait().docs["status"] == 0).all()
    return store, hs


def mixed_requests(rng, srcs, n):
    hs = rng.integers(0, len(srcs), size=n).astype(np.uint32)                # handles repeat
    H = np.array([hist_len(srcs[int(h)][0]) for h in hs], np.int64)
    kind = rng.integers(0, 4, size=n)
    frm = np.where(kind == 0, 0, rng.integers(0, H + 2))
    to = np.where(kind <= 1, H + rng.integers(0, 3, size=n), rng.integers(0, H + 2))
    return hs, frm.astype(np.uint32), to.astype(np.uint32)


def test_incremental_remerged_and_device_sources_agree(engine, c4):
    import torch
    b, o, srcs = c4
    S, n = b.a_stride, b.n_docs
    hs, frm, to = mixed_requests(np.random.default_rng(11), srcs, 400)
    want = expected(srcs, S, hs, frm, to)
    inc, _ = fed(engine, b, 3, 2)
    assert inc.last_routing()["incremental"] > 0
    same(inc.op_diffs(hs, frm, to), want, "after incremental rounds")
    cold, _ = fed(engine, b, 1, 0)
    same(cold.op_diffs(hs, frm, to), want, "after a re-merge")
    r = engine.merge(b)
    same(engine.op_diffs_host(b, r, hs, frm, to), want, "host tables")
    # the merged batch in device memory
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    t = [up(x) for x in (b.docs, b.changes, b.deps, b.ops, r.docs, r.hist, r.all_deps, hs, frm, to)]
    cb = CBatch(n, len(b.changes), len(b.deps), len(b.ops), 0, S, 0, 0, 0, 0, 0, 0,
                t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), None)
    cr = CResults(t[4].data_ptr(), None, None, None, t[5].data_ptr(), t[6].data_ptr(), None, None)
    nq, caps = len(hs), (len(want[0]), len(want[1]))
    z = lambda nbytes: torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)
    g = [z(caps[0] * 16), z(caps[1] * 16), z(nq * 8), z(nq * 4)]
    summ, work = z(64), z(engine.op_diffs_work_bytes(cb, nq))
    out = COpDiffOut(caps[0], caps[1], *[x.data_ptr() for x in g])
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    engine.op_diffs_device(cb, cr, nq, t[7].data_ptr(), t[8].data_ptr(), t[9].data_ptr(), out, summ.data_ptr(), work.data_ptr(), stream)
    torch.cuda.synchronize()
    sm = COpDiffSummary.from_buffer_copy(summ.cpu().numpy().tobytes())
    assert list(sm.totals)[:2] == list(caps) and sm.bad == 0 and sm.flags == int(np.bitwise_or.reduce(want[3]))
    down = lambda x, dt, k: np.frombuffer(x.cpu().numpy().tobytes()[:k * np.dtype(dt).itemsize], dt)
    same((down(g[0], OP_DIFF_DT, caps[0]), down(g[1], SURV_RESULT_DT, caps[1]), down(g[2], np.uint32, 2 * nq).reshape(-1, 2),
          down(g[3], np.uint32, nq)), want, "device tables")
    # too small a capacity: nothing is written, the summary still says what is needed
    g2 = [z(caps[0] * 16), z(caps[1] * 16), z(nq * 8), z(nq * 4)]
    out2 = COpDiffOut(caps[0], caps[1] - 1, *[x.data_ptr() for x in g2])
    engine.op_diffs_device(cb, cr, nq, t[7].data_ptr(), t[8].data_ptr(), t[9].data_ptr(), out2, summ.data_ptr(), work.data_ptr(), stream)
    torch.cuda.synchronize()
    assert list(COpDiffSummary.from_buffer_copy(summ.cpu().numpy().tobytes()).totals)[:2] == list(caps)
    assert not any(x.cpu().numpy().any() for x in g2)
    # no request: the summary is zeroed and nothing else is touched
    summ.fill_(0xA5)
    engine.op_diffs_device(cb, cr, 0, 0, 0, 0, COpDiffOut(), summ.data_ptr(), 0, stream)
    torch.cuda.synchronize()
    assert not summ.cpu().numpy().any()
    with pytest.raises(EngineError, match="aligned"):
        engine.op_diffs_device(cb, cr, nq, t[7].data_ptr(), t[8].data_ptr(), t[9].data_ptr(), out, summ.data_ptr(), work.data_ptr() + 4, stream)


def test_many_requests(engine, c4):
    """5,000 requests over 300 documents in one call: handles repeat, ranges are mixed, and the scan's
    chunk of 4096 requests is crossed"""
    b, o, srcs = c4
    store, _ = fed(engine, b, 1, 1)
    hs, frm, to = mixed_requests(np.random.default_rng(12), srcs, 5000)
    want = check(store, srcs, hs, frm, to, memo={})
    assert len(want[0]) > 20000 and (want[2][:, 1] == 0).any()


# ---- the call itself ----------------------------------------------------------------------------------
class Raw:
    """hm_store_op_diffs with caller capacities; every output pre-filled with 0xA5"""

    def __init__(self, n, caps):
        fill = lambda k, dt: np.frombuffer(bytes([0xA5]) * (max(k, 1) * np.dtype(dt).itemsize), dt).copy()
        self.rows, self.surv, self.rng, self.fl = fill(caps[0], OP_DIFF_DT), fill(caps[1], SURV_RESULT_DT), fill(2 * n, np.uint32), fill(n, np.uint32)
        self.out = COpDiffOut(caps[0], caps[1], self.rows.ctypes.data, self.surv.ctypes.data, self.rng.ctypes.data, self.fl.ctypes.data)
        self.tot = np.full(2, 77, np.uint64)

    def untouched(self):
        return all(a.tobytes() == bytes([0xA5]) * a.nbytes for a in (self.rows, self.surv, self.rng, self.fl))


def raw_call(store, hs, frm, to, caps):
    hs, frm, to = (np.ascontiguousarray(x, np.uint32) for x in (hs, frm, to))
    R = Raw(len(hs), caps)
    p = lambda a: a.ctypes.data if len(a) else None
    st = store._L.hm_store_op_diffs(store._h, len(hs), p(hs), p(frm), p(to), ctypes.byref(R.out), R.tot.ctypes.data)
    return st, R


def test_caps_errors_and_untouched_outputs(engine):
    names = sorted(HAND)
    store, hs, srcs = opened(engine, [HAND[k] for k in names])
    req, frm, to = [hs[0], hs[2], hs[0], hs[5]], [0, 0, 1, 0], [9, 9, 2, 9]
    want = expected(srcs, 8, req, frm, to)
    exact = [len(want[0]), len(want[1])]
    for short in range(2):                                      # one row short in each table in turn
        caps = list(exact)
        caps[short] -= 1
        st, R = raw_call(store, req, frm, to, caps)
        assert st == NOMEM and [int(x) for x in R.tot] == exact and R.untouched(), short
    st, R = raw_call(store, req, frm, to, exact)
    assert st == 0 and [int(x) for x in R.tot] == exact
    same((R.rows, R.surv, R.rng.reshape(-1, 2), R.fl), want, "exact capacities")
    st, R = raw_call(store, [hs[0], 9999], [0, 0], [9, 9], exact)
    assert st == INVALID and R.untouched()
    with pytest.raises(EngineError, match="bad handle"):
        store.op_diffs([hs[0], 9999], [0, 0], [9, 9])
    st, R = raw_call(store, [], [], [], [0, 0])                 # n == 0
    assert st == 0 and not R.tot.any() and R.untouched()
    rows, surv, rng, fl = store.op_diffs([], [], [])
    assert len(rows) == len(surv) == len(rng) == len(fl) == 0
    # a batch in flight
    store.submit([(hs[0], [ch(A, 9, {}, s("x", 4))])])
    st, R = raw_call(store, req, frm, to, exact)
    assert st == INVALID and R.untouched()
    with pytest.raises(EngineError, match="in flight"):
        store.op_diff_sizes(req, frm, to)
    store.wait()
    same(store.op_diffs(req, frm, to), want, "after the wait")
