"""The current state of many documents in one device call (hm_store_state_sizes / hm_store_state /
hm_state_host / hm_state_device, csrc/state_kernels.hip): rows, survivors, ranges and flags against
tests/state_ref.py applied to the CPU oracle's merge of each document's own log (pinned without a
GPU by tests/test_state_ref.py), table for table."""
import ctypes

import numpy as np
import pytest

from hypermerge_amd.columnar import SURV_RESULT_DT, CBatch, CResults, encode
from hypermerge_amd.engine import STATE_ROW_DT, CStateOut, CStateSummary, EngineError
from hypermerge_amd.store import DocStore
import oracle.oracle as O

from fuzz_docs import gen_doc, quiet_tail, withheld
from kat_cases import A, ch, d, s
from state_cases import KNOWN
from state_ref import State, pack, state_of
from test_fuzz_docs import fault_docs, query_docs
from test_store_gpu import split

pytestmark = pytest.mark.gpu

NOMEM, INVALID = 34, 32
WG = 256                                     # HM_ST_WG: registers of a chunk
GRID = 65535                                 # HM_ST_MAX_GRID: the workgroups a launch has at most


# ---- the reference ----------------------------------------------------------------------------------
def want_of(store, h, memo=None):
    """(State, clock row, heads row) of a DocStore document: the contract on the oracle's merge of its log"""
    if memo is not None and h in memo:
        return memo[h]
    b = store.enc[h].log_batch(store.S)
    o = O.merge(b)
    w = (state_of(b, o, 0), np.asarray(o.clock, np.uint32)[:store.S].copy(), np.asarray(o.heads, np.uint32)[:store.S].copy())
    if memo is not None:
        memo[h] = w
    return w


def same(got, want, what=""):
    rows, surv, rng, fl = got[:4]
    wrows, wsurv, wrng, wfl = pack(want)
    np.testing.assert_array_equal(fl, wfl, err_msg=f"flags {what}")
    np.testing.assert_array_equal(rng, wrng, err_msg=f"ranges {what}")
    np.testing.assert_array_equal(np.stack([rows[f].astype(np.int64) for f in ("reg", "obj", "index", "n_surv", "surv_off")], 1).reshape(-1, 5),
                                  wrows, err_msg=f"rows {what}")
    assert surv.tobytes() == wsurv.tobytes(), f"survivors {what}"
    return wrows, wsurv, wrng, wfl


def check(store, hs, memo=None, what=""):
    want = [want_of(store, int(h), memo) for h in hs]
    got = store.state(hs, clocks=True)
    packed = same(got, [w[0] for w in want], what)
    np.testing.assert_array_equal(got[4], np.array([w[1] for w in want], np.uint32).reshape(len(hs), store.S), err_msg=f"clock {what}")
    np.testing.assert_array_equal(got[5], np.array([w[2] for w in want], np.uint32).reshape(len(hs), store.S), err_msg=f"heads {what}")
    cnt, fl, tot = store.state_sizes(hs)
    np.testing.assert_array_equal(cnt, packed[2][:, 1::2])
    np.testing.assert_array_equal(fl, packed[3])
    assert [int(x) for x in tot] == [len(packed[0]), len(packed[1])]
    return packed


# ---- the documents ------------------------------------------------------------------------------------
def stride_docs(S):
    """the known-answer documents and the full-vocabulary ones of a stride: 30 / 8 / 6 of them"""
    known = [KNOWN[k][0] for k in sorted(KNOWN)]
    if S == 8:
        return known + [full for full, _, _ in query_docs("default")[:28]] + [full for full, _, _ in query_docs("long")[:2]]
    if S == 16:
        return known + [gen_doc(300 + i, n_actors=9 + i, profile="wide") for i in range(8)]
    return known + [full for full, _, _ in query_docs("wide")[:6]]


def map_doc(n_keys, every_third_deleted=False):
    chs = [ch(A, 1, {}, *[s(f"k{i:03d}", i) for i in range(n_keys)])]
    if every_third_deleted:
        chs.append(ch(A, 2, {}, *[d(f"k{i:03d}") for i in range(0, n_keys, 3)]))
    return chs


def opened(engine, docs, S=8, incremental=None):
    store = DocStore(engine, a_stride=S)
    if incremental is not None:
        store.set_incremental(incremental)
    hs = [store.open() for _ in docs]
    items = [(h, c) for h, c in zip(hs, docs) if c]
    if items:
        assert (store.apply(items).docs["status"] == 0).all()
    return store, hs


# ---- store form -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 16, 64])
def test_remerged_and_incremental_stores(engine, S):
    """The known answers and 30 / 8 / 6 full-vocabulary documents: after one re-merge, and after rounds
    under set_incremental(2) (three rounds of the head, then the quiet tail one change a round), where
    survivor lists have moved inside the op segment's slots."""
    docs = stride_docs(S)
    cold, hs = opened(engine, docs, S, incremental=0)
    memo = {}
    want = check(cold, hs, memo, "after a re-merge")
    assert (want[0][:, 3] > 1).any() and (want[0][:, 2] >= 0).any()                  # conflicts, list elements
    assert sum(int(cold.info(h)["n_regs"]) for h in hs) > len(want[0])                # dead registers were skipped
    rng = np.random.default_rng(50 + S)
    inc = DocStore(engine, a_stride=S)
    inc.set_incremental(2)
    assert [inc.open() for _ in docs] == hs
    tails = [quiet_tail(c) if c else (c, []) for c in docs]
    parts = [split(head, 3, rng) for head, _ in tails]
    rounds = [[(h, parts[i][rd]) for i, h in enumerate(hs) if parts[i][rd]] for rd in range(3)]
    rounds += [[(h, tail[k:k + 1]) for h, (_, tail) in zip(hs, tails) if len(tail) > k] for k in range(3)]
    routed = 0
    for rd, items in enumerate(x for x in rounds if x):
        assert (inc.apply(items).docs["status"] == 0).all()
        routed += inc.last_routing()["incremental"]
        check(inc, hs, {}, f"after round {rd}")
    assert routed > 0
    # (the two stores' logs differ in arrival order, so in op and register ids: each is held to its own log's merge)
    assert [int(x) for x in inc.state_sizes(hs)[2]] == [len(want[0]), len(want[1])]


def test_withheld_changes_contribute_nothing(engine):
    trip = query_docs("default")[:12]
    store, hs = opened(engine, [kept for _, kept, _ in trip])
    assert sum(int(store.info(h)["n_queued"]) for h in hs) > 0
    check(store, hs, {}, "withheld")
    full, _ = opened(engine, [f for f, _, _ in trip])
    got, ref = store.state(hs), full.state(hs)
    assert len(got[0]) < len(ref[0])                                                  # the queued changes' registers are missing


def test_reset_repeated_empty_and_bad_handles(engine):
    docs = [KNOWN[k][0] for k in sorted(KNOWN)]
    store, hs = opened(engine, docs)
    memo = {}
    check(store, hs, memo)
    rep = [hs[3], hs[1], hs[3], hs[3], hs[8], hs[1]]                                  # a handle may repeat
    check(store, rep, memo, "repeated")
    store.reset([hs[3]])
    assert want_of(store, hs[3])[0] == State(0, [])
    rows, surv, rng, fl = check(store, hs, {}, "after a reset")
    assert [int(x) for x in rng[3]][1::2] == [0, 0]
    # n == 0 launches nothing and answers empty tables
    rows, surv, rng, fl = store.state([])
    assert len(rows) == len(surv) == len(rng) == len(fl) == 0
    st, R = raw_call(store, [], [0, 0])
    assert st == 0 and not R.tot.any() and R.untouched()
    # a handle outside the store
    st, R = raw_call(store, [hs[0], 9999], [64, 64])
    assert st == INVALID and R.untouched()
    with pytest.raises(EngineError, match="bad handle"):
        store.state([hs[0], 9999])
    with pytest.raises(EngineError, match="bad handle"):
        store.state_sizes([9999])
    # between submit and wait
    store.submit([(hs[1], [ch(A, 9, {}, s("late", 4))])])
    st, R = raw_call(store, hs, [64, 64])
    assert st == INVALID and R.untouched()
    with pytest.raises(EngineError, match="in flight"):
        store.state_sizes(hs)
    store.wait()
    check(store, hs, {}, "after the wait")


class Raw:
    """hm_store_state with caller capacities; every output pre-filled with 0xA5"""

    def __init__(self, n, caps, S):
        fill = lambda k, dt: np.frombuffer(bytes([0xA5]) * (max(k, 1) * np.dtype(dt).itemsize), dt).copy()
        self.rows, self.surv, self.rng, self.fl = fill(caps[0], STATE_ROW_DT), fill(caps[1], SURV_RESULT_DT), fill(4 * n, np.uint32), fill(n, np.uint32)
        self.clock, self.heads = fill(n * S, np.uint32), fill(n * S, np.uint32)
        self.out = CStateOut(caps[0], caps[1], self.rows.ctypes.data, self.surv.ctypes.data, self.rng.ctypes.data, self.fl.ctypes.data)
        self.tot = np.full(2, 77, np.uint64)

    def untouched(self):
        return all(a.tobytes() == bytes([0xA5]) * a.nbytes for a in (self.rows, self.surv, self.rng, self.fl, self.clock, self.heads))


def raw_call(store, hs, caps):
    hs = np.ascontiguousarray(hs, np.uint32)
    R = Raw(len(hs), caps, store.S)
    st = store._L.hm_store_state(store._h, len(hs), hs.ctypes.data if len(hs) else None, ctypes.byref(R.out),
                                 R.clock.ctypes.data, R.heads.ctypes.data, R.tot.ctypes.data)
    return st, R


def test_capacities_one_short(engine):
    docs = [KNOWN[k][0] for k in sorted(KNOWN)]
    store, hs = opened(engine, docs)
    want = [want_of(store, h) for h in hs]
    wrows, wsurv, _, _ = pack([w[0] for w in want])
    exact = [len(wrows), len(wsurv)]
    assert exact[1] > exact[0] > 0
    for short in range(2):                                      # one row short in each table in turn
        caps = list(exact)
        caps[short] -= 1
        st, R = raw_call(store, hs, caps)
        assert st == NOMEM and [int(x) for x in R.tot] == exact and R.untouched(), short
    st, R = raw_call(store, hs, exact)                          # the same call with those totals
    assert st == 0 and [int(x) for x in R.tot] == exact
    same((R.rows, R.surv, R.rng.reshape(-1, 4), R.fl), [w[0] for w in want], "exact capacities")
    np.testing.assert_array_equal(R.clock.reshape(len(hs), -1), np.array([w[1] for w in want]))
    np.testing.assert_array_equal(R.heads.reshape(len(hs), -1), np.array([w[2] for w in want]))


def test_chunk_edges(engine):
    """One-change map documents of 63 / 64 / 65 and 255 / 256 / 257 registers (a wave, a chunk), each
    also with every third key deleted, and a key that holds 8 survivors: the ranks across the waves of
    a chunk and the totals carried into the next chunk."""
    sizes = (1, 63, 64, 65, WG - 1, WG, WG + 1, 2 * WG + 1)
    docs = [map_doc(n) for n in sizes] + [map_doc(n, True) for n in sizes]
    docs.append([ch(f"w{i}", 1, {}, s("x", i)) for i in range(8)])
    store, hs = opened(engine, docs)
    rows, surv, rng, fl = check(store, hs, {})
    k = len(sizes)
    assert [int(x) for x in rng[:k, 1]] == list(sizes)
    assert [int(x) for x in rng[k:2 * k, 1]] == [n - (n + 2) // 3 for n in sizes]
    assert [int(x) for x in rng[-1]][1::2] == [1, 8]
    # in any order, and with the widest document first and last
    order = [hs[7], hs[-1], hs[15], hs[2], hs[5], hs[13], hs[7]]
    check(store, order, {}, "reordered")
    # the same documents after incremental rounds that move survivor lists: every key set again by a second writer
    inc, hs2 = opened(engine, [map_doc(n) for n in sizes], incremental=2)
    for rd in range(2):
        items = [(h, [ch("zz", rd + 1, {}, *[s(f"k{i:03d}", -i) for i in range(rd, n, 2)][:60])]) for h, n in zip(hs2, sizes)]
        assert (inc.apply(items).docs["status"] == 0).all()
        check(inc, hs2, {}, f"incremental round {rd}")
    assert inc.last_routing()["incremental"] > 0


def test_more_requests_than_workgroups(engine):
    """65,537 requests over seven small documents in one call: a workgroup takes a second request."""
    docs = [KNOWN[k][0] for k in ("two_lists_nested_map", "two_writer_conflict", "empty", "text_deleted_element", "all_deleted")]
    docs += [map_doc(WG + 3, True), map_doc(5)]
    store, hs = opened(engine, docs)
    n = GRID + 2
    small = np.array(hs[:5] + hs[6:], np.uint32)
    req = small[np.random.default_rng(3).integers(0, len(small), size=n)]
    req[GRID - 1], req[GRID], req[GRID + 1], req[0], req[1] = hs[5], hs[0], hs[5], hs[0], hs[5]   # (the two-chunk document at the seam)
    memo = {}
    states = [want_of(store, int(h), memo)[0] for h in req]
    rows, surv, rng, fl = store.state(req)
    wrows, wsurv, wrng, wfl = pack(states)
    np.testing.assert_array_equal(rng, wrng)
    assert not fl.any() and surv.tobytes() == wsurv.tobytes()
    np.testing.assert_array_equal(np.stack([rows[f].astype(np.int64) for f in ("reg", "obj", "index", "n_surv", "surv_off")], 1), wrows)


def test_clock_and_heads_rows_are_hm_doc_reads(engine):
    docs = [full for full, _, _ in query_docs("default")[:10]]
    store, hs = opened(engine, docs)
    got = store.state(hs[::-1], clocks=True)
    for i, h in enumerate(hs[::-1]):
        _, r = store.read(h)
        np.testing.assert_array_equal(got[4][i], r.clock)
        np.testing.assert_array_equal(got[5][i], r.heads)
    assert got[4].any() and got[5].any() and (got[4] != got[5]).any()


# ---- cold batches -----------------------------------------------------------------------------------------
def cold_docs(S):
    docs = stride_docs(S)
    faulty = [chs for chs, _ in fault_docs()[:10]] if S == 8 else []
    out = []
    for i, c in enumerate(docs):
        out.append(c)
        if i % 3 == 0 and i // 3 < len(faulty):
            out.append(faulty[i // 3])
    return out


@pytest.mark.parametrize("S", [8, 64])
def test_cold_batch_host_form(engine, S):
    """hm_state_host on the stores' documents as one cold batch; at stride 8 with ten documents that
    throw (two of each kind) among them: a document whose status is not OK gets no rows."""
    b = encode(cold_docs(S), S)
    o = O.merge(b)
    r = engine.merge(b)
    np.testing.assert_array_equal(r.docs["status"], o.docs["status"])
    want = [state_of(b, o, i) for i in range(b.n_docs)]
    got = engine.state_host(b, r, clocks=True)
    same(got, want, "every document")
    bad = [i for i in range(b.n_docs) if int(o.docs["status"][i]) != 0]
    assert len(bad) == (10 if S == 8 else 0) and all(want[i] == State(0, []) for i in bad)
    ok = [i for i in range(b.n_docs) if i not in bad]
    np.testing.assert_array_equal(got[4][ok], np.asarray(o.clock).reshape(b.n_docs, S)[ok])
    np.testing.assert_array_equal(got[5][ok], np.asarray(o.heads).reshape(b.n_docs, S)[ok])
    # chosen documents, repeated and out of order; capacities one short
    idx = np.array([5, 0, 5, b.n_docs - 1, 1, 1, 3], np.uint32)
    pick = [want[int(i)] for i in idx]
    same(engine.state_host(b, r, idx), pick, "chosen documents")
    exact = [len(pack(pick)[0]), len(pack(pick)[1])]
    with pytest.raises(EngineError, match="capacity"):
        engine.state_host(b, r, idx, cap=(exact[0], exact[1] - 1))
    same(engine.state_host(b, r, idx, cap=tuple(exact)), pick, "exact capacities")
    with pytest.raises(EngineError, match="outside the batch"):
        engine.state_host(b, r, np.array([0, b.n_docs], np.uint32))


def test_cold_batch_device_form_on_a_side_stream(engine):
    import torch
    S = 8
    b = encode(cold_docs(S), S)
    o = O.merge(b)
    r = engine.merge(b)
    n = b.n_docs
    idx = np.concatenate([np.arange(n, dtype=np.uint32), np.array([2, 2, 0], np.uint32)])
    want = [state_of(b, o, int(i)) for i in idx]
    wrows, wsurv, wrng, wfl = pack(want)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    t = [up(x) for x in (b.docs, r.docs, r.regs, r.surv, r.clock, r.heads, idx)]
    cb = CBatch(n, len(b.changes), len(b.deps), len(b.ops), len(r.regs), S, 0, 0, 0, 0, 0, 0, t[0].data_ptr(), None, None, None, None)
    cr = CResults(t[1].data_ptr(), t[4].data_ptr(), None, t[5].data_ptr(), None, None, t[2].data_ptr(), t[3].data_ptr())
    nq, caps = len(idx), (len(wrows), len(wsurv))
    z = lambda nbytes: torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)
    g = [z(caps[0] * 20), z(caps[1] * 16), z(nq * 16), z(nq * 4), z(nq * S * 4), z(nq * S * 4)]
    summ, work = z(64), z(engine.state_work_bytes(nq))
    out = CStateOut(caps[0], caps[1], *[x.data_ptr() for x in g[:4]])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    engine.state_device(cb, cr, nq, t[6].data_ptr(), out, summ.data_ptr(), work.data_ptr(), side.cuda_stream, g[4].data_ptr(), g[5].data_ptr())
    side.synchronize()
    sm = CStateSummary.from_buffer_copy(summ.cpu().numpy().tobytes())
    assert list(sm.totals) == list(caps) and sm.bad == 0 and sm.flags == 0
    assert sm.max_rows == int(wrng[:, 1].max()) and sm.max_surv == int(wrng[:, 3].max())
    down = lambda x, dt, k: np.frombuffer(x.cpu().numpy().tobytes()[:k * np.dtype(dt).itemsize], dt)
    same((down(g[0], STATE_ROW_DT, caps[0]), down(g[1], SURV_RESULT_DT, caps[1]), down(g[2], np.uint32, 4 * nq).reshape(-1, 4),
          down(g[3], np.uint32, nq)), want, "device tables")
    ok = np.array([int(o.docs["status"][int(i)]) == 0 for i in idx])
    np.testing.assert_array_equal(down(g[4], np.uint32, nq * S).reshape(nq, S)[ok], np.asarray(o.clock).reshape(n, S)[idx][ok])
    np.testing.assert_array_equal(down(g[5], np.uint32, nq * S).reshape(nq, S)[ok], np.asarray(o.heads).reshape(n, S)[idx][ok])
    # the per-request counts and offsets stay at the head of the work memory
    wk = down(work, np.uint32, 8 * nq)
    np.testing.assert_array_equal(wk[:4 * nq].reshape(nq, 4)[:, :2], wrng[:, 1::2])
    np.testing.assert_array_equal(wk[4 * nq:].reshape(nq, 4)[:, :2], wrng[:, 0::2])
    # too small a capacity: nothing is written, the summary still says what is needed
    g2 = [z(caps[0] * 20), z(caps[1] * 16), z(nq * 16), z(nq * 4), z(nq * S * 4), z(nq * S * 4)]
    out2 = CStateOut(caps[0] - 1, caps[1], *[x.data_ptr() for x in g2[:4]])
    engine.state_device(cb, cr, nq, t[6].data_ptr(), out2, summ.data_ptr(), work.data_ptr(), side.cuda_stream, g2[4].data_ptr(), g2[5].data_ptr())
    side.synchronize()
    assert list(CStateSummary.from_buffer_copy(summ.cpu().numpy().tobytes()).totals) == list(caps)
    assert not any(x.cpu().numpy().any() for x in g2)
    # a document outside the batch: flagged in the summary, an empty range, the others answered
    t_bad = up(np.array([1, n + 4, 3], np.uint32))
    g3 = [z(caps[0] * 20), z(caps[1] * 16), z(3 * 16), z(3 * 4)]
    engine.state_device(cb, cr, 3, t_bad.data_ptr(), CStateOut(caps[0], caps[1], *[x.data_ptr() for x in g3]), summ.data_ptr(),
                        work.data_ptr(), side.cuda_stream)
    side.synchronize()
    sm = CStateSummary.from_buffer_copy(summ.cpu().numpy().tobytes())
    assert sm.bad == 1
    np.testing.assert_array_equal(down(g3[2], np.uint32, 12).reshape(3, 4)[:, 1], [len(want[1].rows), 0, len(want[3].rows)])
    # no request: the summary is zeroed and nothing else is touched
    summ.fill_(0xA5)
    engine.state_device(cb, cr, 0, 0, CStateOut(), summ.data_ptr(), 0, side.cuda_stream)
    side.synchronize()
    assert not summ.cpu().numpy().any()
    with pytest.raises(EngineError, match="aligned"):
        engine.state_device(cb, cr, nq, t[6].data_ptr(), out, summ.data_ptr(), work.data_ptr() + 4, side.cuda_stream)
