#!/usr/bin/env python3
"""Times hm_store_missing_changes on a resident C4 store against hm_store_read_history of the same
rows ("What a peer lacks").

The store is fed as bench.py's resident leg feeds its stores: --docs C4 documents (that leg's
size by default) resident with all but their last 4 changes, then rounds in which each document
receives its next 1-2 changes.  `have` is each document's opSet.clock from before the last round, so
the answer is the history the last round added: the same rows hm_store_read_history returns for
(hist_len before that round, hist_len now), which is the comparison — that call moves the same
output and needs no fold.  Both calls are synchronous (host tables in, host rows out, ending in a
stream synchronise), so a host clock around each measures the call.  After --warmup runs of each,
--reps runs of each are taken alternately; median and range are reported, and the two answers are
compared.

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
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tail", type=int, default=4)
    args = ap.parse_args()
    from hypermerge_amd import synth
    from hypermerge_amd.engine import Engine
    from hypermerge_amd.store import RowStore, slice_changes
    note = lambda m: print(f"[bench_missing_changes] {m}", file=sys.stderr, flush=True)      # noqa: E731
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
    clock = res.clock.copy()
    hist_len = res.docs["hist_len"].astype(np.uint32)
    rng = np.random.default_rng(5)
    rounds = 0
    while (pos < nch).any():
        have, before = clock.copy(), hist_len.copy()
        hi = np.minimum(pos + rng.integers(1, 3, n), nch)
        sel = np.nonzero(hi > pos)[0]
        st.submit_batch(slice_changes(b, pos, hi, sel), sel.astype(np.uint32))
        res = st.wait()
        assert (res.docs["status"] == 0).all()
        clock[sel] = res.clock
        hist_len[sel] = res.docs["hist_len"]
        pos = np.maximum(pos, hi)
        rounds += 1
    note(f"{rounds} rounds fed; the last one touched {len(sel)} documents")

    # the entry tables: each document's non-zero clock columns, in rank order
    rows, cols = np.nonzero(have)
    eoff = np.zeros(n + 1, np.uint32)
    np.cumsum(np.bincount(rows, minlength=n), out=eoff[1:])
    eact = np.ascontiguousarray(cols.astype(np.uint16))
    eseq = np.ascontiguousarray(have[rows, cols].astype(np.uint32))
    hs = np.arange(n, dtype=np.uint32)
    want = (hist_len - before).astype(np.uint32)
    total = int(want.sum())
    off = np.zeros(n + 1, np.uint32)
    np.cumsum(want, out=off[1:])
    L, p = st._L, lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    rng_out = np.zeros((n, 2), np.uint32)
    log_a = np.zeros(max(total, 1), np.uint32)
    log_b = np.zeros(max(total, 1), np.uint32)
    tot = ctypes.c_uint32()

    def missing():
        rc = L.hm_store_missing_changes(st._h, n, p(hs), p(eoff), p(eact), p(eseq), 0, None, p(rng_out), p(log_a), total,
                                        ctypes.byref(tot))
        assert rc == 0 and tot.value == total, (rc, tot.value, total)

    def history():
        rc = L.hm_store_read_history(st._h, n, p(hs), p(before), p(hist_len), p(off), p(log_b), None)
        assert rc == 0, rc

    for _ in range(args.warmup):
        missing()
        history()
    ms = {"missing_changes": [], "read_history": []}
    for _ in range(args.reps):
        for name, f in (("missing_changes", missing), ("read_history", history)):
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    # the same rows: each request's block against the history slice
    assert (rng_out[:, 1] == want).all()
    idx = np.repeat(rng_out[:, 0].astype(np.int64) - off[:-1].astype(np.int64), want) + np.arange(total)
    same = bool((log_a[idx] == log_b[:total]).all())
    out = {"docs": n, "a_stride": S, "rounds": rounds, "requests": n, "entries": int(eoff[-1]), "rows": total,
           "documents_with_rows": int((want > 0).sum()), "reps": args.reps, "warmup": args.warmup, "equal": same}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 3) for x in v]}
    out["ratio_median"] = out["missing_changes"]["median_ms"] / out["read_history"]["median_ms"]
    print(json.dumps(out))
    assert same


if __name__ == "__main__":
    main()
