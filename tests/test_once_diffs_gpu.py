"""The one-walk form of the op-diff call (hm_store_op_diffs_ex with HM_ODF_ONCE): its rows, survivors
(through surv_off), indices, counts and flags against the call without the bit, bit for bit and
request by request, and against tests/op_diffs_ref.py / tests/list_diffs_ref.py; the capacity rule;
the calls that refuse the bit.

One store holds every document and every request is asked in one call of more than 4,096 requests
(a wave serves several), so the references are computed once and shared by the tests."""
import ctypes

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import NONE, SURV_RESULT_DT, CBatch, CResults, decode_doc
from hypermerge_amd.docset import DocSet
from hypermerge_amd.engine import OD_LISTS, ODF_LISTS, ODF_ONCE, OP_DIFF_DT, COpDiffOut, COpDiffSummary

from list_diffs_cases import LHAND
from list_diffs_ref import list_diffs
from list_diffs_ref import pack as pack_lists
from op_diffs_cases import HAND, chain_doc
from op_diffs_ref import op_diffs
from op_diffs_ref import pack as pack_maps
from past_ref import hist_len
from test_op_diffs_gpu import T, opened

pytestmark = pytest.mark.gpu

NOMEM, INVALID = 34, 32
LONG = 620                                                    # applied changes of the long map document (> HM_OD_TILE)


def documents():
    """(documents, the index of the long map document)"""
    docs = [HAND[k] for k in sorted(HAND)] + [LHAND[k][0] for k in sorted(LHAND)]
    b5 = synth.generate(synth.config("C5", n_docs=10, arrival=2, shuffle_pct=40))
    docs += [decode_doc(b5, i) for i in range(b5.n_docs)]
    b3 = synth.generate(synth.config("C3", n_docs=2, changes_per_actor=40))
    docs += [decode_doc(b3, i) for i in range(b3.n_docs)]
    docs.append(chain_doc(LONG, 1))
    return docs, len(docs) - 1


def requests(hs, srcs, long_h):
    """per document the whole history, its last position, every one-position slice and an empty
    slice; on the long document slices across position HM_OD_TILE; then the list again until the
    call holds more than 4,096 requests (every handle repeats)"""
    req = []
    for h in hs:
        H = hist_len(srcs[h][0])
        req += [(h, 0, H), (h, max(H - 1, 0), H), (h, H // 2, H // 2)] + [(h, k, k + 1) for k in range(H)]
    assert T == 512 and hist_len(srcs[long_h][0]) == LONG
    req += [(long_h, T - 12, T + 18), (long_h, T - 1, T + 1), (long_h, T, LONG)]
    base = list(req)
    while len(req) <= 4096:
        req += base
    return req


def per_request(tables, lists):
    """the tables of a call, two-pass or one-walk, as one comparable value per request: (flags, the
    rows' op / kind / n_surv, their indices, the survivors each row's surv_off leads to)"""
    rows, surv, rng, fl = tables[:4]
    index = tables[4] if lists else None
    out = []
    for i in range(len(rng)):
        a, n = int(rng[i][0]), int(rng[i][1])
        r = rows[a:a + n]
        sv = [surv[int(o):int(o) + int(k)].tobytes() for o, k in zip(r["surv_off"], r["n_surv"])]
        out.append((int(fl[i]), r["op"].tobytes(), r["kind"].tobytes(), r["n_surv"].tobytes(),
                    index[a:a + n].tobytes() if lists else b"", b"".join(sv)))
    return out


def ref_tables(results, packer):
    t = packer(results)
    rows = np.array([tuple(x) for x in t[0]], OP_DIFF_DT) if t[0] else np.zeros(0, OP_DIFF_DT)
    base = (rows, np.array([tuple(x) for x in t[1]], SURV_RESULT_DT), np.array(t[2], np.uint32).reshape(-1, 2), np.array(t[3], np.uint32))
    return base + (np.array(t[4], np.uint32),) if len(t) == 5 else base


def first_difference(got, want, req, what):
    assert len(got) == len(want) == len(req)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{what}: request {i} {req[i]}"


@pytest.fixture(scope="module")
def world(engine):
    docs, long_i = documents()
    store, hs, srcs = opened(engine, docs)
    req = requests(hs, srcs, hs[long_i])
    h3 = [np.array([r[k] for r in req], np.uint32) for k in range(3)]
    memo_l, memo_m = {}, {}
    for r in req:
        if r not in memo_l:
            memo_l[r] = list_diffs(*srcs[r[0]], store.S, r[1], r[2])
            assert memo_l[r].bad == 0
            memo_m[r] = op_diffs(*srcs[r[0]], store.S, r[1], r[2])
    slice_ops = 0                                             # the ops of the slices' applied changes
    for h, f, t in req:
        src = srcs[h][0]
        slice_ops += int(sum(int(c["n_ops"]) for c, p in zip(src.changes, src.hist) if f <= int(p) < t))
    return dict(store=store, hs=hs, srcs=srcs, req=req, h3=h3, long_h=hs[long_i], slice_ops=slice_ops,
                want_l=per_request(ref_tables([memo_l[r] for r in req], pack_lists), True),
                want_m=per_request(ref_tables([memo_m[r] for r in req], pack_maps), False))


def test_lists_one_walk_equals_the_two_pass_call_and_the_reference(world):
    s, req = world["store"], world["req"]
    assert len(req) > 4096
    two = s.op_diffs(*world["h3"], lists=True)
    one = s.op_diffs(*world["h3"], lists=True, once=True)
    assert not two[3].any() and not one[3].any()
    a, b = per_request(two, True), per_request(one, True)
    first_difference(b, a, req, "one walk against two passes")
    first_difference(b, world["want_l"], req, "one walk against list_diffs_ref")
    np.testing.assert_array_equal(one[2][:, 1], two[2][:, 1])                 # the counts
    kinds = set(int(k) for k in two[0]["kind"])
    assert {0, 1, 2, 3, 4, 5} <= kinds
    # the blocks do not overlap: every request's rows lie in a block of its own
    used = one[2][one[2][:, 1] > 0].astype(np.int64)
    used = used[np.argsort(used[:, 0])]
    assert (used[:-1, 0] + used[:-1, 1] <= used[1:, 0]).all()
    # and the survivors of different rows do not overlap either
    rows = np.concatenate([one[0][int(f):int(f) + int(n)] for f, n in one[2]])
    rows = rows[rows["n_surv"] > 0]
    so = np.sort(rows, order="surv_off")
    assert (so["surv_off"][:-1].astype(np.int64) + so["n_surv"][:-1] <= so["surv_off"][1:]).all()
    assert int(rows["n_surv"].sum()) == len(two[1]) == len(one[1])           # the survivor total is exact


def test_without_lists_a_list_document_is_flagged_where_the_two_pass_call_flags_it(world):
    s, req = world["store"], world["req"]
    two = s.op_diffs(*world["h3"])
    one = s.op_diffs(*world["h3"], once=True)
    np.testing.assert_array_equal(one[3], two[3])
    assert (two[3] & OD_LISTS).any() and not (two[3] & OD_LISTS).all()
    assert not one[2][one[3] != 0, 1].any()                                   # a flagged request: (block, 0)
    first_difference(per_request(one, False), per_request(two, False), req, "one walk against two passes, no lists")
    first_difference(per_request(one, False), world["want_m"], req, "one walk against op_diffs_ref")


def test_slices_of_the_long_document_start_above_the_first_tile(world):
    s, h = world["store"], world["long_h"]
    rg = [(T - 12, T + 18), (T + 1, T + 2), (LONG - 1, LONG), (T, T), (0, LONG)]
    h3 = ([h] * len(rg), [f for f, _ in rg], [t for _, t in rg])
    two, one = s.op_diffs(*h3, lists=True), s.op_diffs(*h3, lists=True, once=True, cap=(1, 1))   # (a guess that is too small)
    first_difference(per_request(one, True), per_request(two, True), list(zip(*h3)), "the long document")
    assert [int(n) for n in one[2][:, 1]] == [30, 1, 1, 0, LONG]              # one op per change, none an ins
    assert (one[4] == NONE).all()


def raw_once(store, h3, caps, opts=ODF_LISTS | ODF_ONCE, totals=True):
    fill = lambda k, dt: np.frombuffer(bytes([0xA5]) * (max(k, 1) * np.dtype(dt).itemsize), dt).copy()
    n = len(h3[0])
    bufs = [fill(caps[0], OP_DIFF_DT), fill(caps[1], SURV_RESULT_DT), fill(2 * n, np.uint32), fill(n, np.uint32), fill(caps[0], np.uint32)]
    out = COpDiffOut(caps[0], caps[1], *[x.ctypes.data for x in bufs[:4]])
    tot = np.full(2, 77, np.uint64)
    st = store._L.hm_store_op_diffs_ex(store._h, n, *[x.ctypes.data for x in h3], ctypes.byref(out), bufs[4].ctypes.data,
                                       tot.ctypes.data if totals else None, opts)
    untouched = all(a.tobytes() == bytes([0xA5]) * a.nbytes for a in bufs)
    return st, [int(x) for x in tot], bufs, untouched


def test_capacity_rule(world):
    s, h3, req = world["store"], world["h3"], world["req"]
    _, _, two_tot = s.op_diff_sizes(*h3, lists=True)
    st, tot, _, untouched = raw_once(s, h3, (0, 0))
    assert st == NOMEM and untouched
    # the row total: the ops of the slices, which bound the rows; the survivor total is exact
    assert int(two_tot[0]) <= tot[0] <= world["slice_ops"] and tot[1] == int(two_tot[1])
    assert tot[0] == world["slice_ops"]
    for short in (0, 1):
        caps = list(tot)
        caps[short] -= 1
        st, again, _, untouched = raw_once(s, h3, caps)
        assert st == NOMEM and again == tot and untouched, short
    st, again, bufs, _ = raw_once(s, h3, tot)
    assert st == 0 and again == tot
    got = per_request((bufs[0], bufs[1], bufs[2].reshape(-1, 2), bufs[3], bufs[4]), True)
    first_difference(got, world["want_l"], req, "tables of exactly the reported sizes")


def test_the_calls_that_refuse_the_bit(world, engine):
    s, h3 = world["store"], [x[:4].copy() for x in world["h3"]]
    L = s._L
    cnt, fl, tot = np.zeros(8, np.uint32), np.zeros(4, np.uint32), np.zeros(2, np.uint64)
    for opts in (ODF_ONCE, ODF_ONCE | ODF_LISTS):
        assert L.hm_store_op_diff_sizes_ex(s._h, 4, *[x.ctypes.data for x in h3], cnt.ctypes.data, fl.ctypes.data, tot.ctypes.data, opts) == INVALID
        cb, cr, out, sm = CBatch(), CResults(), COpDiffOut(), COpDiffSummary()
        assert L.hm_op_diffs_work_bytes_ex(ctypes.byref(cb), 4, opts) == 0
        assert L.hm_op_diffs_host_ex(engine._h, ctypes.byref(cb), ctypes.byref(cr), 0, None, None, None, ctypes.byref(out), None, None, opts) == INVALID
        assert L.hm_op_diffs_device_ex(engine._h, ctypes.byref(cb), ctypes.byref(cr), 0, None, None, None, ctypes.byref(out), None,
                                       ctypes.byref(sm), None, None, opts) == INVALID
        ds = DocSet(engine)
        t = ctypes.c_void_p()
        assert L.hm_docset_materialize_patch_ex(ds._h, 0, None, None, opts, ctypes.byref(t)) == INVALID
        ds.close()
    # the one-walk call itself: an unknown bit, and no place for the sizes a repeated call needs
    assert raw_once(s, h3, (64, 64), opts=4 | ODF_ONCE)[0] == INVALID
    st, _, _, untouched = raw_once(s, h3, (64, 64), totals=False)
    assert st == INVALID and untouched
