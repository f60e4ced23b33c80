#!/usr/bin/env python3
"""Times the blocked sweep and the waiting pass on a resident C4 store ("What blocked
documents wait for").  Two RowStores of --docs documents: one holds every document's whole log
(nothing blocked), one the first half of every document's changes in shuffled arrival order
(arrival=2, shuffle_pct=30: one round that leaves many documents blocked).  Each call is
synchronous (it ends in a stream synchronise and a copy of its result to the host), so a host
clock around it measures the call; the median of --reps runs after --warmup is reported, with the
bytes each kernel has to read.  The comparison reaches the same rows through the per-document reads
(hm_doc_info + hm_doc_read + hm_doc_log and the host restatement) on --per-doc of the blocked
documents, scaled to all of them: an extrapolation, not a measurement of the whole list.

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(f, warmup, reps):
    for _ in range(warmup):
        f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def host_missing(changes, deps, hist, clock, S):
    """getMissingDeps of one document from its rows (what a host does with the per-document reads)."""
    missing = np.zeros(S, np.uint32)
    queue = np.nonzero(hist == -1)[0]
    for i in queue:
        c = changes[i]
        need = {int(d["actor"]): int(d["seq"]) for d in deps[int(c["dep_off"]):int(c["dep_off"]) + int(c["n_deps"])]}
        need[int(c["actor"])] = int(c["seq"]) - 1
        for a, q in need.items():
            if clock[a] < q:
                missing[a] = max(missing[a], q)
    return missing, queue


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--per-doc", type=int, default=1000)
    args = ap.parse_args()
    from hypermerge_amd import synth
    from hypermerge_amd.engine import Engine
    from hypermerge_amd.store import RowStore, slice_changes
    eng = Engine(0)
    b = synth.generate(synth.config("C4", n_docs=args.docs, arrival=2, shuffle_pct=30))
    n, S = b.n_docs, b.a_stride
    nch = b.docs["n_changes"].astype(np.int64)
    zero = np.zeros(n, np.int64)
    out = {"docs": n, "a_stride": S, "reps": args.reps}
    note = lambda m: print(f"[waiting_time] {m}", file=sys.stderr, flush=True)      # noqa: E731
    note(f"{n} documents, {len(b.changes)} changes generated")

    full = RowStore(eng, a_stride=S)
    full.open_n(n)
    full.submit_batch(b, np.arange(n, dtype=np.uint32))
    assert (full.wait().docs["status"] == 0).all()
    assert len(full.blocked()) == 0
    out["blocked_none"] = dict(timed(full.blocked, args.warmup, args.reps), blocked=0, read_bytes=n * 32)
    full.close()
    note("whole logs: nothing blocked, timed")

    half = slice_changes(b, zero, nch // 2)
    st = RowStore(eng, a_stride=S)
    st.open_n(n)
    st.submit_batch(half, np.arange(n, dtype=np.uint32))
    res = st.wait()
    assert (res.docs["status"] == 0).all()
    hs = st.blocked()
    assert len(hs) == int((res.docs["n_queued"] > 0).sum())
    out["blocked_some"] = dict(timed(st.blocked, args.warmup, args.reps), blocked=int(len(hs)), read_bytes=n * 32)
    note(f"half logs: {len(hs)} blocked, sweep timed")
    miss, unmet, nq = st.waiting(hs)
    off, q = st.queues(hs, nq)
    # what the waiting pass reads per requested document: its handle and DevDoc, its history positions,
    # the change and dep rows of its queued changes, its clock / back clock / minimumClock rows
    ch0 = half.docs["change_off"].astype(np.int64)[hs]
    qrows = np.repeat(ch0, nq) + q
    dep_rows = int(half.changes["n_deps"][qrows].astype(np.int64).sum())
    n_c = int(half.docs["n_changes"].astype(np.int64)[hs].sum())
    out["waiting"] = dict(timed(lambda: st.waiting(hs), args.warmup, args.reps), requests=int(len(hs)),
                          queued=int(nq.sum()),
                          read_bytes=int(len(hs)) * (4 + 64 + 3 * 4 * S) + 4 * n_c + 24 * int(nq.sum()) + 8 * dep_rows,
                          written_bytes=int(len(hs)) * (2 * 4 * S + 4))
    out["read_queue"] = dict(timed(lambda: st.queues(hs, nq), args.warmup, args.reps), requests=int(len(hs)),
                             read_bytes=int(len(hs)) * (8 + 64) + 4 * n_c, written_bytes=4 * int(nq.sum()))

    note("waiting pass and queue read timed")
    # the same answers one document at a time (the only way without these calls)
    k = min(args.per_doc, len(hs))
    step = max(1, len(hs) // max(k, 1))
    pick = hs[::step][:k]
    t0 = time.perf_counter()
    same = True
    for j, h in zip(range(0, len(hs), step), pick):
        _, g = st.read(int(h))
        c, d, _ = st.log(int(h))
        m, qq = host_missing(c, d, g.hist, g.clock, S)
        same &= bool((m == miss[j]).all()) and list(qq) == list(q[off[j]:off[j + 1]])
    dt = (time.perf_counter() - t0) * 1e3
    out["per_document"] = {"docs": int(k), "ms": dt, "equal": same, "ms_per_doc": dt / max(k, 1),
                           "extrapolated_ms_all_blocked": dt / max(k, 1) * len(hs)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
