#!/usr/bin/env python3
"""Times the per-op diff calls on a resident C4 store ("Per-op diffs").  Recorded, not gated.

The store is fed as tools/bench_materialize.py feeds its store: --docs C4 documents resident with all
but their last 4 changes, then rounds in which each document receives its next 1-2 changes.

Two request sets, one request per document: `full` = the whole history [0, hist_len), `last` = the
slice the last round added [hist_len before it, hist_len).  Legs (each synchronous, a host clock
around it; after --warmup runs, --reps runs taken alternately):
  sizes_*         hm_store_op_diff_sizes, totals only: staging + need + count + scan, 64 B read back
  diffs_*         hm_store_op_diffs into pageable host tables: the same plus the fill pass and the rows'
                  and survivors' copy back
  read_history_*  hm_store_read_history of the same slices with their all_deps rows: what the parent
                  commit reads from the device before it replays the slices' ops on host threads
The kernel split comes from a separate run under a kernel trace (one kernel name per launch:
od_need_kernel, od_walk_kernel<false> = count, past_scan_kernel<false/true>, od_walk_kernel<true> =
fill).  The parent's host replay (docset.cpp Replay on 16 threads) is not driven from here: it
lives behind hm_docset_apply's rounds, whose patches this tree still renders that way.

--ex times the same C4 legs through the *_ex calls with HM_ODF_LISTS (C4 documents carry no list hint:
the order phase is skipped, the other instantiation of the walk runs).

--lists times the element diffs instead (HM_ODF_LISTS, the index table copied back with the rows): a
C5 store of --c5-docs documents and a C3 store of --c3-docs documents, fed the same way; `full` and
`last`, sizes and rows, with the row counts by kind, and read_history_* of the same slices for the
read-back the route without the option does before its host replay (which still has no entry point
of its own to time).

--once adds, to whichever stores the other options chose, the one-walk call (HM_ODF_ONCE) on the same
request sets, taken alternately with the two-pass legs:
  once_*        hm_store_op_diffs_ex with the bit into tables of exactly the sizes it reports (a right
                guess): staging + need + one walk, 64 B read back, the rows' and survivors' copy back
  once_retry_*  the same after a call whose tables were too small (a wrong guess: two walks)
`once_sets` records the one-walk totals (the row total is the ops of the slices, an upper bound).

--at-clock times the clock-selected call instead, on whichever stores the other options chose: one request
per document, its clock the causal past of the change in the middle of its history (that change's
all_deps row with its own seq: closed, and in general no history prefix).  Legs:
  at_sizes      hm_store_op_diff_sizes_at, totals only
  at_diffs      hm_store_op_diffs_at into pageable host tables
  at_baseline   the route the parent commit offers for the same answer: hm_store_materialize at the clock
                (select, gather and re-merge on the device, every table copied back) followed by
                hm_op_diffs_host_ex over the gathered batch's whole history
  prefix_diffs  hm_store_op_diffs(_ex) over [0, middle + 1) of the same documents: the walk over the same
                number of tiles without the select phase (it answers more changes than the clock does:
                `sets` records both), the nearest the host clock comes to the select phase's share
The baseline's rows are checked against the call's (kinds and survivor counts, row for row).

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
    ap.add_argument("--ex", action="store_true", help="the C4 legs through the *_ex calls with HM_ODF_LISTS")
    ap.add_argument("--lists", action="store_true", help="C5 and C3 stores, element diffs answered")
    ap.add_argument("--c5-docs", type=int, default=100_000)
    ap.add_argument("--c3-docs", type=int, default=500)
    ap.add_argument("--once", action="store_true", help="add the one-walk legs (HM_ODF_ONCE)")
    ap.add_argument("--at-clock", action="store_true", help="the clock-selected legs instead (hm_store_op_diffs_at)")
    args = ap.parse_args()
    from hypermerge_amd import synth
    from hypermerge_amd.engine import Engine
    note = lambda m: print(f"[bench_op_diffs] {m}", file=sys.stderr, flush=True)      # noqa: E731
    eng = Engine(0)
    if args.lists:
        res = {"reps": args.reps, "warmup": args.warmup, "opts": "HM_ODF_LISTS"}
        for name, docs in (("C5", args.c5_docs), ("C3", args.c3_docs)):
            res[name] = run(args, eng, synth.generate(synth.config(name, n_docs=docs), threads=min(16, os.cpu_count() or 1)), 1, note)
        print(json.dumps(res))
        return
    res = run(args, eng, synth.generate(synth.config("C4", n_docs=args.docs), threads=min(16, os.cpu_count() or 1)), 1 if args.ex else 0, note)
    res["opts"] = "HM_ODF_LISTS" if args.ex else 0
    print(json.dumps(res))
    assert res.get("tail_equal", True) and res.get("baseline_equal", True)


def run(args, eng, b, opts, note):
    """the legs over one resident store of b's documents; opts = the *_ex calls' option word (0: the calls without it)"""
    from hypermerge_amd.columnar import SURV_RESULT_DT
    from hypermerge_amd.engine import OP_DIFF_DT, COpDiffOut
    from hypermerge_amd.store import RowStore, slice_changes
    n, S = b.n_docs, b.a_stride
    nch = b.docs["n_changes"].astype(np.int64)
    note(f"{n} documents, {len(b.changes)} changes, {len(b.ops)} ops generated")
    st = RowStore(eng, a_stride=S)
    st.open_n(n)
    pos = np.maximum(nch - args.tail, 0)
    st.submit_batch(slice_changes(b, np.zeros(n, np.int64), pos), np.arange(n, dtype=np.uint32))
    res = st.wait()
    assert (res.docs["status"] == 0).all()
    hist_len = res.docs["hist_len"].astype(np.uint32)
    before = hist_len.copy()
    rng = np.random.default_rng(5)
    rounds = 0
    while (pos < nch).any():
        hi = np.minimum(pos + rng.integers(1, 3, n), nch)
        sel = np.nonzero(hi > pos)[0]
        before = hist_len.copy()
        st.submit_batch(slice_changes(b, pos, hi, sel), sel.astype(np.uint32))
        res = st.wait()
        assert (res.docs["status"] == 0).all()
        hist_len[sel] = res.docs["hist_len"]
        pos = np.maximum(pos, hi)
        rounds += 1
    note(f"{rounds} rounds fed")

    if args.at_clock:
        return run_at_clock(args, eng, b, st, hist_len, opts, rounds)
    hs = np.arange(n, dtype=np.uint32)
    sets = {"full": (np.zeros(n, np.uint32), hist_len.copy()), "last": (before, hist_len.copy())}
    L, p = st._L, lambda a: a.ctypes.data      # noqa: E731
    out, legs = {}, []
    keep, keep1 = [], []
    for name, (frm, to) in sets.items():
        cnt, fl, tot = st.op_diff_sizes(hs, frm, to, lists=bool(opts))
        tr, ts = int(tot[0]), int(tot[1])
        out[name] = {"requests": n, "history_positions": int((to.astype(np.int64) - frm).clip(0).sum()), "rows": tr,
                     "survivors": ts, "flagged": int((fl != 0).sum()), "copy_back_bytes": 16 * (tr + ts) + 12 * n}
        rows, surv = np.zeros(max(tr, 1), OP_DIFF_DT), np.zeros(max(ts, 1), SURV_RESULT_DT)
        rg, flg, t2 = np.zeros(2 * n, np.uint32), np.zeros(n, np.uint32), np.zeros(2, np.uint64)
        index = np.zeros(max(tr, 1), np.uint32)
        if opts:
            out[name]["copy_back_bytes"] += 4 * tr
        o = COpDiffOut(tr, ts, p(rows), p(surv), p(rg), p(flg))
        off = np.zeros(n + 1, np.uint32)
        np.cumsum((to.astype(np.int64) - frm).clip(0), out=off[1:])
        hlog, had = np.zeros(max(int(off[-1]), 1), np.uint32), np.zeros(max(int(off[-1]), 1) * S, np.uint32)
        keep.append((rows, surv, rg, flg, t2, o, off, hlog, had, frm, to, index))

        def sizes(frm=frm, to=to, t2=t2):
            if opts:
                assert L.hm_store_op_diff_sizes_ex(st._h, n, p(hs), p(frm), p(to), None, None, p(t2), opts) == 0
            else:
                assert L.hm_store_op_diff_sizes(st._h, n, p(hs), p(frm), p(to), None, None, p(t2)) == 0

        def diffs(frm=frm, to=to, o=o, t2=t2, index=index):
            if opts:
                assert L.hm_store_op_diffs_ex(st._h, n, p(hs), p(frm), p(to), ctypes.byref(o), p(index), p(t2), opts) == 0
            else:
                assert L.hm_store_op_diffs(st._h, n, p(hs), p(frm), p(to), ctypes.byref(o), p(t2)) == 0

        def read_history(frm=frm, to=to, off=off, hlog=hlog, had=had):
            assert L.hm_store_read_history(st._h, n, p(hs), p(frm), p(to), p(off), p(hlog), p(had)) == 0
        legs += [(f"sizes_{name}", sizes), (f"diffs_{name}", diffs), (f"read_history_{name}", read_history)]
        if args.once:
            t1 = np.zeros(2, np.uint64)
            none = COpDiffOut(0, 0, None, None, p(rg), p(flg))
            assert L.hm_store_op_diffs_ex(st._h, n, p(hs), p(frm), p(to), ctypes.byref(none), None, p(t1), opts | 2) == (34 if tr else 0)
            o_r, o_s = int(t1[0]), int(t1[1])
            out[name]["once_rows"], out[name]["once_survivors"] = o_r, o_s
            rows1, surv1, index1 = np.zeros(max(o_r, 1), OP_DIFF_DT), np.zeros(max(o_s, 1), SURV_RESULT_DT), np.zeros(max(o_r, 1), np.uint32)
            rg1, flg1 = np.zeros(2 * n, np.uint32), np.zeros(n, np.uint32)
            o1 = COpDiffOut(o_r, o_s, p(rows1), p(surv1), p(rg1), p(flg1))
            small = COpDiffOut(o_r // 2, o_s // 2, p(rows1), p(surv1), p(rg1), p(flg1))
            keep1.append((rows1, surv1, index1, rg1, flg1, t1, o1, small, none))

            def once(frm=frm, to=to, o1=o1, t1=t1, index1=index1):
                assert L.hm_store_op_diffs_ex(st._h, n, p(hs), p(frm), p(to), ctypes.byref(o1), p(index1) if opts else None, p(t1), opts | 2) == 0

            def once_retry(frm=frm, to=to, o1=o1, small=small, t1=t1, index1=index1):
                assert L.hm_store_op_diffs_ex(st._h, n, p(hs), p(frm), p(to), ctypes.byref(small), p(index1) if opts else None, p(t1), opts | 2) == 34
                assert L.hm_store_op_diffs_ex(st._h, n, p(hs), p(frm), p(to), ctypes.byref(o1), p(index1) if opts else None, p(t1), opts | 2) == 0
            legs += [(f"once_{name}", once), (f"once_retry_{name}", once_retry)]
    for _ in range(args.warmup):
        for _, f in legs:
            f()
    ms = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, f in legs:
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    # the last round's rows are the tail of the whole history's rows, document for document
    full, last = keep[0], keep[1]
    ok = True
    for d in rng.integers(0, n, size=min(n, 2000)):
        f0, fn = int(full[2][2 * d]), int(full[2][2 * d + 1])
        l0, ln = int(last[2][2 * d]), int(last[2][2 * d + 1])
        a, c = full[0][f0 + fn - ln:f0 + fn], last[0][l0:l0 + ln]
        ok &= bool((a["op"] == c["op"]).all() and (a["kind"] == c["kind"]).all() and (a["n_surv"] == c["n_surv"]).all())
    for name, k in zip(sets, keep):                            # rows by kind (create, set, remove, element insert / set / remove)
        out[name]["rows_by_kind"] = [int(x) for x in np.bincount(k[0]["kind"][:out[name]["rows"]], minlength=6)]
    res = {"docs": n, "a_stride": S, "rounds": rounds, "log_changes": int(nch.sum()), "log_ops": int(len(b.ops)),
           "reps": args.reps, "warmup": args.warmup, "tail_equal": ok, "sets": out}
    for name, v in ms.items():
        res[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 3) for x in v]}
    return res


def run_at_clock(args, eng, b, st, hist_len, opts, rounds):
    """the --at-clock legs over the resident store st of b's documents"""
    from hypermerge_amd.columnar import SURV_RESULT_DT
    from hypermerge_amd.engine import OP_DIFF_DT, COpDiffOut
    from hypermerge_amd.store import CPastOut
    n, S = b.n_docs, b.a_stride
    L, p = st._L, lambda a: a.ctypes.data      # noqa: E731
    hs = np.arange(n, dtype=np.uint32)
    # each document's clock: the causal past of the change at the middle history position
    mid = (hist_len // 2).astype(np.uint32)
    to = np.minimum(mid + 1, hist_len).astype(np.uint32)
    off = np.zeros(n + 1, np.uint32)
    np.cumsum((to.astype(np.int64) - mid).clip(0), out=off[1:])
    hlog, had = np.zeros(max(int(off[-1]), 1), np.uint32), np.zeros((max(int(off[-1]), 1), S), np.uint32)
    assert L.hm_store_read_history(st._h, n, p(hs), p(mid), p(to), p(off), p(hlog), p(had)) == 0
    K = np.zeros((n, S), np.uint32)
    have = np.nonzero(to > mid)[0]
    K[have] = had[off[have]]
    ch = b.changes[b.docs["change_off"][have].astype(np.int64) + hlog[off[have]]]
    K[have, ch["actor"]] = ch["seq"]
    zero = np.zeros(n, np.uint32)

    def tables(tr, ts):
        rows, surv = np.zeros(max(tr, 1), OP_DIFF_DT), np.zeros(max(ts, 1), SURV_RESULT_DT)
        rg, flg, index = np.zeros(2 * n, np.uint32), np.zeros(n, np.uint32), np.zeros(max(tr, 1), np.uint32)
        return rows, surv, rg, flg, index, COpDiffOut(tr, ts, p(rows), p(surv), p(rg), p(flg))
    t2 = np.zeros(2, np.uint64)
    cnt, fl, tot = st.op_diff_sizes_at(hs, K, lists=bool(opts))
    A = tables(int(tot[0]), int(tot[1]))
    _, _, ptot = st.op_diff_sizes(hs, zero, to, lists=bool(opts))
    P = tables(int(ptot[0]), int(ptot[1]))
    gb, gr, clog, olog = st.materialize(hs, clocks=K)           # (sizes the baseline's tables)
    pout = CPastOut(len(gb.changes), len(gb.deps), len(gb.ops), len(gr.regs), p(gb.docs), p(gb.changes), p(gb.deps), p(gb.ops),
                    p(clog), p(olog), gr.c_struct())
    B = tables(int(tot[0]), int(tot[1]))
    cb, cr, hl = gb.c_struct(), gr.c_struct(), np.ascontiguousarray(gr.docs["hist_len"], np.uint32)   # (the same every run)
    sets = {"requests": n, "applied_at_clock": int(gr.docs["hist_len"].sum()), "queued_at_clock": int(gr.docs["n_queued"].sum()),
            "prefix_positions": int(to.sum()), "rows": int(tot[0]), "survivors": int(tot[1]), "flagged": int((fl != 0).sum()),
            "prefix_rows": int(ptot[0]), "gathered_changes": len(gb.changes), "gathered_ops": len(gb.ops)}

    def at_sizes():
        assert L.hm_store_op_diff_sizes_at(st._h, n, p(hs), p(K), None, None, p(t2), opts) == 0

    def at_diffs():
        assert L.hm_store_op_diffs_at(st._h, n, p(hs), p(K), ctypes.byref(A[5]), p(A[4]), p(t2), opts) == 0

    def at_baseline():
        assert L.hm_store_materialize(st._h, n, p(hs), None, p(K), ctypes.byref(pout), None) == 0
        assert L.hm_op_diffs_host_ex(eng._h, ctypes.byref(cb), ctypes.byref(cr), n, None, p(zero), p(hl), ctypes.byref(B[5]), p(B[4]), p(t2), opts) == 0

    def prefix_diffs():
        if opts:
            assert L.hm_store_op_diffs_ex(st._h, n, p(hs), p(zero), p(to), ctypes.byref(P[5]), p(P[4]), p(t2), opts) == 0
        else:
            assert L.hm_store_op_diffs(st._h, n, p(hs), p(zero), p(to), ctypes.byref(P[5]), p(t2)) == 0
    legs = [("at_sizes", at_sizes), ("at_diffs", at_diffs), ("at_baseline", at_baseline), ("prefix_diffs", prefix_diffs)]
    for _ in range(args.warmup):
        for _, f in legs:
            f()
    ms = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, f in legs:
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    tr = int(tot[0])
    same = bool((A[2] == B[2]).all() and (A[0]["kind"][:tr] == B[0]["kind"][:tr]).all() and (A[0]["n_surv"][:tr] == B[0]["n_surv"][:tr]).all() and
                (A[4][:tr] == B[4][:tr]).all())
    res = {"docs": n, "a_stride": S, "rounds": rounds, "log_changes": int(b.docs["n_changes"].sum()), "log_ops": int(len(b.ops)),
           "reps": args.reps, "warmup": args.warmup, "baseline_equal": same, "sets": sets}
    for name, v in ms.items():
        res[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 3) for x in v]}
    return res


if __name__ == "__main__":
    main()
