#!/usr/bin/env python3
"""Times forking resident documents at a mid-history point: the device route (hm_store_fork_submit: the
rows gathered on the device and handed to the device-table submit) against the host route the parent
commit offers (hm_store_materialize to host tables, then hm_batch_submit of them: the same gather and
merge plus two PCIe crossings).  DESIGN.md §5, "Forks".  Recorded, not gated.

--docs documents of --workload (C2 / C3 / ...) are resident in a RowStore.  Every leg forks all of them
in one call into the same --docs destination handles: after each call the batch is undone
(hm_batch_undo, outside the clock), which leaves the destinations empty with their segments in place,
so no timed call allocates segments or compacts the store.  Legs (a host clock around submit + wait,
--warmup runs first, then --reps runs taken alternately):
  fork_history       device route, history length = half the history, history order
  fork_clock         device route, the clock at that history length, history order
  fork_actor_major   device route, the same clock handed over actor after actor (ranks ascending)
  host_history       hm_store_materialize (history length, the four gathered tables and the result rows
                     to preallocated pageable host arrays) + hm_batch_submit of them + wait
--docset N: the docset level on the first N documents (default 0 = skipped): hm_docset_fork at each
document's clock at half its history against re-applying the blocks of those changes, already packed,
to fresh documents through hm_docset_apply (the fork's clock entries are packed outside the clock too).  Each docset run takes fresh documents (a docset call
cannot be undone from outside), so those legs include what growing the stores costs either route.
--legs a,b: only those legs (a profiler run of one kind of fill).

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2")
    ap.add_argument("--docs", type=int, default=10_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--docset", type=int, default=0)
    ap.add_argument("--legs", default="")
    args = ap.parse_args()
    from hypermerge_amd import synth
    from hypermerge_amd.columnar import (CHANGE_DT, DEP_DT, DOC_DT, DOC_RESULT_DT, OP_DT, Batch, CResults, decode_doc)
    from hypermerge_amd.engine import CPastOut, Engine
    from hypermerge_amd.store import RowStore
    note = lambda m: print(f"[bench_fork] {m}", file=sys.stderr, flush=True)      # noqa: E731
    eng = Engine(0)
    b = synth.generate(synth.config(args.workload, n_docs=args.docs), threads=min(16, os.cpu_count() or 1))
    n, S = b.n_docs, b.a_stride
    st = RowStore(eng, a_stride=S)
    p0 = st.open_n(n)
    hs = np.arange(p0, p0 + n, dtype=np.uint32)
    st.submit_batch(b, hs)
    res = st.wait()
    assert (res.docs["status"] == 0).all()
    half = (res.docs["hist_len"] // 2).astype(np.uint32)
    note(f"{n} {args.workload} documents, {len(b.changes)} changes, {len(b.ops)} ops resident (stride {S})")
    # the clock at half the history, from the gathered prefix
    g, r, _, _ = st.materialize(hs, history=half)
    clock = r.clock.reshape(n, S).copy()
    order = np.full((n, S), 0xFFFFFFFF, np.uint32)
    na = b.docs["n_actors"].astype(np.int64)
    for a in range(S):
        order[na > a, a] = a
    cnt, tot = st.past_sizes(hs, history=half)
    tc, td, to, tr = (int(x) for x in tot)
    d0 = st.open_n(n)
    dst = np.arange(d0, d0 + n, dtype=np.uint32)
    L, p = st._L, lambda a: a.ctypes.data      # noqa: E731

    def undo(bid):
        st._check(L.hm_batch_undo(st._h, ctypes.c_uint64(bid)), "hm_batch_undo")

    def device(history=None, clocks=None, order=None):
        def run():
            t0 = time.perf_counter()
            _, bid = st.fork_submit(hs, history=history, clocks=clocks, order=order, into=dst)
            rr = st.wait()
            dt = time.perf_counter() - t0
            assert (rr.docs["status"] == 0).all()
            run.last = rr
            undo(bid)
            return dt
        return run

    hb = Batch(np.zeros(n, DOC_DT), np.zeros(tc, CHANGE_DT), np.zeros(td, DEP_DT), np.zeros(to, OP_DT), S)
    hres = np.zeros(n, DOC_RESULT_DT)
    hout = CPastOut(tc, td, to, tr, p(hb.docs), p(hb.changes), p(hb.deps), p(hb.ops), None, None,
                    CResults(p(hres), None, None, None, None, None, None, None))

    def host():
        t0 = time.perf_counter()
        rc = L.hm_store_materialize(st._h, n, p(hs), p(half), None, ctypes.byref(hout), None)
        assert rc == 0, rc
        bid = st.submit_batch(hb, dst)
        rr = st.wait()
        dt = time.perf_counter() - t0
        assert (rr.docs["status"] == 0).all()
        host.last = rr
        undo(bid)
        return dt

    legs = {"fork_history": device(history=half), "fork_clock": device(clocks=clock),
            "fork_actor_major": device(clocks=clock, order=order), "host_history": host}
    if args.legs:
        legs = {k: legs[k] for k in args.legs.split(",")}
    for _ in range(args.warmup):
        for f in legs.values():
            f()
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, f in legs.items():
            ms[k].append(f() * 1e3)
    out = {"workload": args.workload, "docs": n, "a_stride": S, "log_changes": int(len(b.changes)), "changes": tc, "deps": td,
           "ops": to, "regs": tr, "reps": args.reps, "warmup": args.warmup}
    for k, v in ms.items():
        out[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 3) for x in v]}
    if "fork_history" in ms and "host_history" in ms:
        same = all((legs["fork_history"].last.docs[f] == legs["host_history"].last.docs[f]).all()
                   for f in ("status", "hist_len", "n_queued", "n_surv"))
        out["equal"] = bool(same and (legs["fork_history"].last.docs["hist_len"] == half).all())
        out["host_over_device"] = out["host_history"]["median_ms"] / out["fork_history"]["median_ms"]
        assert out["equal"]

    if args.docset:
        from hypermerge_amd.decode import pack_offsets
        from hypermerge_amd.docset import DocSet, _text
        k = min(args.docset, n)
        docs = [decode_doc(b, i) for i in range(k)]
        ds = DocSet(eng)
        first = ds.open(k)
        ids = list(range(first, first + k))
        blocks = lambda chs: [json.dumps(c, separators=(",", ":")).encode() for c in chs]      # noqa: E731
        rs, _ = ds.apply(ids, [blocks(d) for d in docs])
        assert (rs["status"] == 0).all()
        clocks, handed = [], []
        for i, d in enumerate(docs):
            ck = {}
            for j in ds.history_prefix(ids[i], int(half[i])):
                ck[d[j]["actor"]] = max(ck.get(d[j]["actor"], 0), int(d[j]["seq"]))
            clocks.append(ck)
            have = {}
            for c in d:
                have.setdefault((c["actor"], c["seq"]), c)
            handed.append([have[(a, q)] for a, kk in ck.items() for q in range(1, kk + 1)])
        data, bo, db = pack_offsets([blocks(h) for h in handed])
        eoff, adata, aoff, sq = ds._clock_entries(k, clocks)      # (both legs' inputs are packed outside the clock)
        idarr = np.ascontiguousarray(ids, np.uint32)
        dms = {"docset_fork": [], "docset_reapply": []}
        for rep in range(args.warmup + args.reps):
            ft, f0 = ctypes.c_void_p(), ctypes.c_uint32()
            t0 = time.perf_counter()
            eng._check(ds._L.hm_docset_fork(ds._h, k, idarr.ctypes.data, None, eoff.ctypes.data, adata.ctypes.data, aoff.ctypes.data,
                                            sq.ctypes.data, ctypes.byref(f0), ctypes.byref(ft)), "hm_docset_fork")
            t1 = time.perf_counter()
            _, fr = _text(ds._L, ft, raw=True)
            fresh = np.arange(ds.open(k), ds.open(0), dtype=np.uint32)
            tt = ctypes.c_void_p()
            t2 = time.perf_counter()
            eng._check(ds._L.hm_docset_apply(ds._h, data.ctypes.data, bo.ctypes.data, db.ctypes.data, fresh.ctypes.data, k,
                                             ctypes.byref(tt)), "hm_docset_apply")
            t3 = time.perf_counter()
            ds._L.hm_text_free(tt)
            assert (fr["status"] == 0).all()
            if rep >= args.warmup:
                dms["docset_fork"].append((t1 - t0) * 1e3)
                dms["docset_reapply"].append((t3 - t2) * 1e3)
        for kk, v in dms.items():
            out[kk] = {"docs": k, "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 3) for x in v]}
        out["docset_reapply_over_fork"] = out["docset_reapply"]["median_ms"] / out["docset_fork"]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
