#!/usr/bin/env python3
"""Times hm_store_materialize on a resident C4 store: every document at half its history, one request
each, in one call ("A document as it was").  Recorded, not gated.

The store is fed as tools/bench_missing_changes.py feeds its store: --docs C4 documents resident with
all but their last 4 changes, then rounds in which each document receives its next 1-2 changes.

Legs (each synchronous, a host clock around it; after --warmup runs, --reps runs taken alternately):
  materialize        one hm_store_materialize call for all documents, returning only the per-request
                     hm_doc_result rows: count + scan + fill + merge on the device, almost no copy back
  materialize_view   the same call returning what a renderer reads (doc rows, op_log, hm_doc_result,
                     clock, heads, registers, survivors) into pageable host arrays
  merge_prebuilt     hm_merge_device on the same prefixes already laid out as a cold batch in HBM, results
                     left in HBM: the floor the gather adds to
  old_route          --old documents only: per document hm_doc_history_prefix + hm_doc_log, the batch
                     rebuilt on the host in numpy, then one hm_merge_host of those documents (the route
                     a caller had before; its hm_doc_history_prefix is this tree's).  old_route_scaled
                     multiplies its median by docs / old: an extrapolation, not a measurement.
gather_bytes: what the gather must move, from shapes: per request 64 B DevDoc + 48 B doc row, 4 B of hist
per log change, and per selected change / dep / op the row read and written plus its 4 B map entry.

Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rebuild(changes, deps, ops, idx):
    """the rows of the log changes idx (document-local offsets), in that order, offsets rewritten"""
    ch = changes[idx].copy()

    def rows(first, n, table):
        n = n.astype(np.int64)
        off = np.zeros(len(n) + 1, np.int64)
        np.cumsum(n, out=off[1:])
        return table[np.repeat(first.astype(np.int64) - off[:-1], n) + np.arange(int(off[-1]))], off
    dp, doff = rows(ch["dep_off"], ch["n_deps"], deps)
    op, ooff = rows(ch["op_first"], ch["n_ops"], ops)
    ch["dep_off"], ch["op_first"] = doff[:-1], ooff[:-1]
    return ch, dp, op


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--old", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tail", type=int, default=4)
    args = ap.parse_args()
    import torch
    from hypermerge_amd import synth
    from hypermerge_amd.columnar import (CHANGE_DT, DEP_DT, DOC_DT, DOC_RESULT_DT, OP_DT, REG_RESULT_DT, SURV_RESULT_DT,
                                         Batch, CBatch, CResults)
    from hypermerge_amd.engine import CPastOut, Engine
    from hypermerge_amd.store import RowStore, slice_changes
    note = lambda m: print(f"[bench_materialize] {m}", file=sys.stderr, flush=True)      # noqa: E731
    eng = Engine(0)
    b = synth.generate(synth.config("C4", n_docs=args.docs), threads=min(16, os.cpu_count() or 1))
    n, S = b.n_docs, b.a_stride
    nch = b.docs["n_changes"].astype(np.int64)
    note(f"{n} documents, {len(b.changes)} changes generated")
    st = RowStore(eng, a_stride=S)
    st.open_n(n)
    pos = np.maximum(nch - args.tail, 0)
    st.submit_batch(slice_changes(b, np.zeros(n, np.int64), pos), np.arange(n, dtype=np.uint32))
    res = st.wait()
    assert (res.docs["status"] == 0).all()
    hist_len = res.docs["hist_len"].astype(np.uint32)
    rng = np.random.default_rng(5)
    rounds = 0
    while (pos < nch).any():
        hi = np.minimum(pos + rng.integers(1, 3, n), nch)
        sel = np.nonzero(hi > pos)[0]
        st.submit_batch(slice_changes(b, pos, hi, sel), sel.astype(np.uint32))
        res = st.wait()
        assert (res.docs["status"] == 0).all()
        hist_len[sel] = res.docs["hist_len"]
        pos = np.maximum(pos, hi)
        rounds += 1
    note(f"{rounds} rounds fed")

    hs = np.arange(n, dtype=np.uint32)
    half = (hist_len // 2).astype(np.uint32)
    cnt, tot = st.past_sizes(hs, history=half)
    tc, td, to, tr = (int(x) for x in tot)
    assert (cnt[:, 0] == half).all()
    gather_bytes = n * (64 + 48) + 4 * int(nch.sum()) + tc * (24 * 2 + 4) + td * 16 + to * (32 * 2 + 4)
    L, p = st._L, lambda a: a.ctypes.data      # noqa: E731
    docs_r = np.zeros(n, DOC_RESULT_DT)
    lean = CPastOut(0, 0, 0, 0, None, None, None, None, None, None, CResults(p(docs_r), None, None, None, None, None, None, None))
    rows, olog = np.zeros(n, DOC_DT), np.zeros(to, np.uint32)
    clock, heads = np.zeros(n * S, np.uint32), np.zeros(n * S, np.uint32)
    regs, surv = np.zeros(tr, REG_RESULT_DT), np.zeros(to, SURV_RESULT_DT)
    docs_v = np.zeros(n, DOC_RESULT_DT)
    view = CPastOut(0, 0, to, tr, p(rows), None, None, None, None, p(olog),
                    CResults(p(docs_v), p(clock), None, p(heads), None, None, p(regs), p(surv)))

    def call(out):
        rc = L.hm_store_materialize(st._h, n, p(hs), p(half), None, ctypes.byref(out), None)
        assert rc == 0, rc

    # the same prefixes as a cold batch in HBM (built once from one materialize call)
    g, _, _, _ = st.materialize(hs, history=half)
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)      # noqa: E731
    t = [up(x) for x in (g.docs, g.changes, g.deps, g.ops)]
    z = lambda k: torch.zeros(max(k, 16), dtype=torch.uint8, device=dev)      # noqa: E731
    rt = [z(n * 32), z(n * S * 4), z(n * S * 4), z(n * S * 4), z(tc * 4), z(tc * S * 4), z(tr * 16), z(to * 16)]
    cb = g.c_struct()
    gb = CBatch(n, tc, td, to, tr, S, cb.max_changes, cb.max_ops, cb.max_regs, cb.max_objs, cb.doc_flags, cb.max_deps,
                t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), None)
    gr = CResults(*[x.data_ptr() for x in rt])
    stream = torch.cuda.current_stream().cuda_stream

    def prebuilt():
        eng.merge_device(gb, gr, stream)
        torch.cuda.synchronize()

    # the route a caller had before, on the first --old documents
    k = min(args.old, n)

    def old_route():
        chs, dps, ops = [], [], []
        d = np.zeros(k, DOC_DT)
        nc = nd = no = nr = 0
        for h in range(k):
            idx = np.array(st.history_prefix(h, int(half[h])), np.int64)
            c, dd, oo = st.log(h)
            c, dd, oo = rebuild(c, dd, oo, idx)
            c["dep_off"] += nd
            c["op_first"] += no
            row = d[h]
            row["change_off"], row["n_changes"], row["dep_off"], row["n_deps"] = nc, len(c), nd, len(dd)
            row["op_off"], row["n_ops"], row["reg_off"] = no, len(oo), nr
            for f in ("n_regs", "n_objs", "n_actors", "flags"):
                row[f] = b.docs[f][h]
            chs.append(c); dps.append(dd); ops.append(oo)
            nc += len(c); nd += len(dd); no += len(oo); nr += int(b.docs["n_regs"][h])
        ob = Batch(d, np.concatenate(chs).astype(CHANGE_DT), np.concatenate(dps).astype(DEP_DT),
                   np.concatenate(ops).astype(OP_DT), S)
        return ob, eng.merge(ob)

    legs = (("materialize", lambda: call(lean)), ("materialize_view", lambda: call(view)), ("merge_prebuilt", prebuilt),
            ("old_route", old_route))
    for _ in range(args.warmup):
        for _, f in legs:
            f()
    ms = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, f in legs:
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    # the three routes agree: hist_len of every request, and the first --old documents' registers
    ob, orr = old_route()
    pre = np.frombuffer(rt[0].cpu().numpy().tobytes()[:n * 32], DOC_RESULT_DT)
    same = lambda x, y: all((x[f] == y[f]).all() for f in ("status", "hist_len", "n_queued", "n_surv"))      # noqa: E731
    equal = bool((docs_r["hist_len"] == half).all() and same(docs_v, docs_r) and same(pre, docs_r)
                 and all((orr.docs[f] == docs_r[f][:k]).all() for f in ("status", "hist_len", "n_queued", "n_surv")) and (ob.changes == g.changes[:len(ob.changes)]).all()
                 and (orr.regs == regs[:len(orr.regs)]).all())
    out = {"docs": n, "a_stride": S, "rounds": rounds, "requests": n, "log_changes": int(nch.sum()), "changes": tc, "deps": td,
           "ops": to, "regs": tr, "gather_bytes": gather_bytes, "old_docs": k, "reps": args.reps, "warmup": args.warmup,
           "equal": equal}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 3) for x in v]}
    out["old_route_scaled"] = {"median_ms": out["old_route"]["median_ms"] * n / k, "extrapolated": True}
    out["gather_over_floor_ms"] = out["materialize"]["median_ms"] - out["merge_prebuilt"]["median_ms"]
    print(json.dumps(out))
    assert equal


if __name__ == "__main__":
    main()
