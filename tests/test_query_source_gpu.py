"""The rule the device queries share for finding a request's document (csrc/doc_source.h): a
segment that runs past the declared table length is clamped to empty.  The hand-case cold batch of
test_waiting_gpu.py is merged whole; hm_missing_deps_device, hm_missing_changes_device and
hm_materialize_device are then called with a CBatch whose n_changes / n_deps / n_ops stop before the
last document's rows (the device tables stay whole, so a wrong clamp reads valid memory and gives
a wrong answer).  The last document answers as an empty one, no bad bit is set, and every other
document answers as in the uncut call."""
import numpy as np
import pytest

from hypermerge_amd.columnar import CBatch, CResults, CHANGE_DT, DEP_DT, DOC_DT, OP_DT
from hypermerge_amd.engine import CPastOut, CPastSummary

from test_waiting_gpu import _cold_batches

pytestmark = pytest.mark.gpu


def _ask(engine, b, t, n_changes, n_deps, n_ops):
    """The three device entries on the uploaded tables t with the declared table lengths."""
    import torch
    dev = torch.device("cuda", 0)
    n, S = b.n_docs, b.a_stride
    cb = CBatch(n, n_changes, n_deps, n_ops, 0, S, 0, 0, 0, 0, 0, 0,
                t["docs"].data_ptr(), t["changes"].data_ptr(), t["deps"].data_ptr(), t["ops"].data_ptr(), None)
    cr = CResults(t["rdocs"].data_ptr(), t["clock"].data_ptr(), None, None, t["hist"].data_ptr(), t["all_deps"].data_ptr(),
                  None, None)
    stream = torch.cuda.current_stream().cuda_stream
    z = lambda nbytes: torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)
    u32 = lambda x, k: x.cpu().numpy().view(np.uint32)[:k].copy()
    got = {}
    # getMissingDeps
    miss = z(n * S * 4)
    engine.missing_deps_device(cb, cr, miss.data_ptr(), stream)
    # getMissingChanges with an empty have-clock: every applied change, in history order
    cap = len(b.changes)
    eoff, rng, log, cnt = z((n + 1) * 4), z(n * 8), z(cap * 4), z(8)
    engine.missing_changes_device(cb, cr, eoff.data_ptr(), 0, 0, 0, 0, 0, rng.data_ptr(), log.data_ptr(), cap,
                                  cnt.data_ptr(), cnt.data_ptr() + 4, stream)
    # every document at its whole history
    caps = [len(b.changes), len(b.deps), len(b.ops), int(b.docs["n_regs"].sum())]
    g = [z(n * 48), z(caps[0] * 24), z(caps[1] * 8), z(caps[2] * 32), z(caps[0] * 4), z(caps[2] * 4)]
    summ, work = z(64), z(int(engine._L.hm_materialize_work_bytes(n)))
    out = CPastOut(caps[0], caps[1], caps[2], caps[3], *[x.data_ptr() for x in g], CResults())
    engine.materialize_device(cb, cr, n, 0, t["hist_len"].data_ptr(), 0, out, summ.data_ptr(), work.data_ptr(), stream)
    torch.cuda.synchronize()
    got["missing"] = u32(miss, n * S).reshape(n, S)
    got["range"] = u32(rng, 2 * n).reshape(n, 2)
    lg = u32(log, cap)
    got["lists"] = [[int(x) for x in lg[int(a):int(a) + int(c)]] for a, c in got["range"]]
    got["total"], got["mc_bad"] = (int(x) for x in u32(cnt, 2))
    got["summary"] = CPastSummary.from_buffer_copy(summ.cpu().numpy().tobytes()[:64])
    got["counts"] = u32(work, 4 * n).reshape(n, 4)
    down = lambda x, dt, k: np.frombuffer(x.cpu().numpy().tobytes()[:k * np.dtype(dt).itemsize], dt)
    tot = [int(x) for x in got["summary"].totals]
    got["docs"] = down(g[0], DOC_DT, n)
    got["tables"] = [down(g[1], CHANGE_DT, tot[0]), down(g[2], DEP_DT, tot[1]), down(g[3], OP_DT, tot[2]),
                     down(g[4], np.uint32, tot[0]), down(g[5], np.uint32, tot[2])]
    return got


@pytest.mark.parametrize("cut", [1, 2])     # 1: the last document; 2: also the one before it, which has a queue
def test_segment_past_the_declared_tables_is_an_empty_document(engine, cut):
    import torch
    dev = torch.device("cuda", 0)
    _, b = _cold_batches()
    n, S = b.n_docs, b.a_stride
    assert 8 <= n <= 12 and S == 8
    r = engine.merge(b)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    t = {"docs": up(b.docs), "changes": up(b.changes), "deps": up(b.deps), "ops": up(b.ops), "rdocs": up(r.docs),
         "clock": up(r.clock), "hist": up(r.hist), "all_deps": up(r.all_deps), "hist_len": up(b.docs["n_changes"].astype(np.uint32))}
    whole = _ask(engine, b, t, len(b.changes), len(b.deps), len(b.ops))
    k = n - cut                              # the first document whose rows are cut off
    d = b.docs[k]
    assert all(int(b.docs[f][k:].sum()) for f in ("n_changes", "n_deps", "n_ops"))    # (there is something to cut)
    part = _ask(engine, b, t, int(d["change_off"]), int(d["dep_off"]), int(d["op_off"]))
    # the uncut call is not trivial where the cut documents are
    assert whole["lists"][n - 1] and whole["counts"][n - 1, :3].all()
    if cut == 2:
        assert whole["missing"][k].any()                               # (both of its changes wait in the queue)
    # no bad bit
    assert whole["mc_bad"] == 0 and part["mc_bad"] == 0
    assert whole["summary"].bad == 0 and part["summary"].bad == 0
    # the cut documents answer as empty documents
    assert not part["missing"][k:].any()
    assert not part["range"][k:].any()
    assert not part["counts"][k:, :3].any()
    for f in ("n_changes", "n_deps", "n_ops"):
        assert not part["docs"][f][k:].any(), f
    for f in ("n_regs", "n_objs", "n_actors", "flags"):                 # (the totals are the document's own)
        np.testing.assert_array_equal(part["docs"][f][k:], whole["docs"][f][k:], err_msg=f)
    # every other document answers as in the uncut call
    np.testing.assert_array_equal(part["missing"][:k], whole["missing"][:k])
    assert part["lists"][:k] == whole["lists"][:k]
    assert part["total"] == sum(len(x) for x in whole["lists"][:k])
    np.testing.assert_array_equal(part["counts"][:k], whole["counts"][:k])
    assert part["docs"][:k].tobytes() == whole["docs"][:k].tobytes()
    assert [int(x) for x in part["summary"].totals[:3]] == [int(whole["counts"][:k, c].sum()) for c in range(3)]
    for p, w in zip(part["tables"], whole["tables"]):                   # (request order: the others' rows come first)
        assert p.tobytes() == w[:len(p)].tobytes()
