#!/usr/bin/env python3
"""Times merging resident documents into documents that already hold changes: the device route
(hm_store_merge_from_submit: the rows gathered and renamed on the device and handed to the device-table
submit) against the host route (the same rows, already laid out as host tables in the destination's ids,
sent with hm_batch_submit: what a caller pays after decoding the source's blocks again, the decode itself
not counted).  DESIGN.md §5, "Merges".  Recorded, not gated.

--docs documents of --workload (C2 / C3 / ...) are resident in a RowStore as the sources.  Each has a
destination that holds the changes of its odd-ranked actors; every leg hands all destinations, in one
call, the even-ranked actors' changes (about half of each source; a document of one actor hands everything
to an empty destination).  Source and destination rows come from one generator, so the maps are the
identity; the rename pass reads and writes every row all the same.  After each call the batch is undone
(hm_batch_undo, outside the clock).  Legs (a host clock around submit + wait, --warmup runs first, then
--reps runs):
  merge_history      device route, the source's history order
  merge_actor_major  device route, actor after actor (ranks ascending)
  host_submit        hm_batch_submit of the rows merge_history moves, from pageable host tables, + wait
--legs a,b: only those legs (one route per process; a profiler run of one kind).

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
    ap.add_argument("--legs", default="")
    args = ap.parse_args()
    from hypermerge_amd import synth
    from hypermerge_amd.engine import Engine
    from hypermerge_amd.store import MergeMaps, RowStore
    note = lambda m: print(f"[bench_merge_from] {m}", file=sys.stderr, flush=True)      # noqa: E731
    eng = Engine(0)
    b = synth.generate(synth.config(args.workload, n_docs=args.docs), threads=min(16, os.cpu_count() or 1))
    n, S = b.n_docs, b.a_stride
    st = RowStore(eng, a_stride=S)
    p0 = st.open_n(n)
    hs = np.arange(p0, p0 + n, dtype=np.uint32)
    st.submit_batch(b, hs)
    res = st.wait()
    assert (res.docs["status"] == 0).all()
    top = res.clock.reshape(n, S).copy()
    odd = (np.arange(S) % 2 == 1)[None, :]
    keep, hand = np.where(odd, top, 0).astype(np.uint32), np.where(odd, 0, top).astype(np.uint32)
    # the destinations: the odd-ranked actors' changes, gathered once and submitted as ordinary rows
    held, hr, _, _ = st.materialize(hs, clocks=keep)
    d0 = st.open_n(n)
    dst = np.arange(d0, d0 + n, dtype=np.uint32)
    st.submit_batch(held, dst)
    assert (st.wait().docs["status"] == 0).all()
    # the rows the merge moves (history order), as host tables, for the host route
    rows, _, _, _ = st.materialize(hs, clocks=hand)
    note(f"{n} {args.workload} documents (stride {S}): {len(b.changes)} changes resident, destinations hold {len(held.changes)}, "
         f"the merge hands {len(rows.changes)} changes / {len(rows.ops)} ops")
    order = np.full((n, S), 0xFFFFFFFF, np.uint32)
    na = b.docs["n_actors"].astype(np.int64)
    for k, a in enumerate(range(0, S, 2)):
        order[na > a, k] = a
    totals = np.stack([b.docs["n_actors"], b.docs["n_regs"], b.docs["n_objs"], b.docs["flags"]], axis=1).astype(np.uint32)
    maps = MergeMaps(totals, np.tile(np.arange(S, dtype=np.uint32), (n, 1)),
                     [np.arange(int(x), dtype=np.uint32) for x in b.docs["n_objs"]],
                     [np.arange(int(x), dtype=np.uint32) for x in b.docs["n_regs"]])
    L = st._L

    def undo(bid):
        st._check(L.hm_batch_undo(st._h, ctypes.c_uint64(bid)), "hm_batch_undo")

    def device(order_rows):
        def run():
            t0 = time.perf_counter()
            bid = st.merge_from_submit(dst, hs, hand, maps, order=order_rows)
            rr = st.wait()
            dt = time.perf_counter() - t0
            assert (rr.docs["status"] == 0).all()
            run.last = rr
            undo(bid)
            return dt
        return run

    def host():
        t0 = time.perf_counter()
        bid = st.submit_batch(rows, dst)
        rr = st.wait()
        dt = time.perf_counter() - t0
        assert (rr.docs["status"] == 0).all()
        host.last = rr
        undo(bid)
        return dt

    legs = {"merge_history": device(None), "merge_actor_major": device(order), "host_submit": host}
    if args.legs:
        legs = {k: legs[k] for k in args.legs.split(",")}
    for _ in range(args.warmup):
        for f in legs.values():
            f()
    ms = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, f in legs.items():
            ms[k].append(f() * 1e3)
    out = {"workload": args.workload, "docs": n, "a_stride": S, "log_changes": int(len(b.changes)), "held_changes": int(len(held.changes)),
           "changes": int(len(rows.changes)), "deps": int(len(rows.deps)), "ops": int(len(rows.ops)), "reps": args.reps, "warmup": args.warmup}
    for k, v in ms.items():
        out[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 3) for x in v]}
    last = [f.last for f in legs.values()]
    out["hist_len_sum"] = int(last[0].docs["hist_len"].sum())
    out["n_queued_sum"] = int(last[0].docs["n_queued"].sum())
    out["equal"] = bool(all((x.docs[f] == last[0].docs[f]).all() for x in last[1:] for f in ("status", "hist_len", "n_queued", "n_surv")))
    assert out["equal"]
    if "merge_history" in ms and "host_submit" in ms:
        out["host_over_device"] = out["host_submit"]["median_ms"] / out["merge_history"]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
