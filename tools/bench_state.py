#!/usr/bin/env python3
"""Times hm_store_state — what every resident document holds now, in one device call — against the two
routes a caller had before it ("The state now").  Recorded, not gated.

Workloads (--only picks one): c4 = --c4-docs resident C4 map documents, c3 = --c3-docs C3 text
documents.  Each store is fed all but the last --tail changes of every document in one submit (a
re-merge: survivor lists packed in register order), measured, then fed two rounds in which each
document receives its next 1-2 changes (the incremental path: lists that grew have moved to the end
of their op segment's slots), and measured again.

Legs (each synchronous, a host clock around it; after --warmup runs, --reps runs taken alternately):
  state               one hm_store_state call over all documents, clock and heads rows included, into
                      pageable host arrays sized by one hm_store_state_sizes call made beforehand
  state_sizes         the count pass alone (hm_store_state_sizes, totals only)
  doc_read_sample     a loop of hm_doc_info + hm_doc_read (registers, survivors, clock, heads) over the
                      first --sample documents: a sample, reported as such; doc_read_scaled multiplies
                      its median by docs / sample and says so ("extrapolated": true)
  materialize_full    hm_store_materialize at every document's full history length, returning what a
                      renderer reads (doc rows, op_log, hm_doc_result, clock, heads, registers,
                      survivors): the logs are gathered and re-merged
state_bytes: what the call must move, from shapes: per document 16 B per register and 16 B per live
survivor read, 20 B per row and 16 B per survivor written (DevDoc, clock and heads rows not counted);
state_gbps = state_bytes / the state leg's median.

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


def legs_of(st, n, S, sample, n_regs_total, hist_len):
    from hypermerge_amd.columnar import DOC_DT, DOC_RESULT_DT, REG_RESULT_DT, SURV_RESULT_DT, CResults
    from hypermerge_amd.engine import CPastOut, CStateOut, STATE_ROW_DT
    from hypermerge_amd.store import _DocInfo
    L, p = st._L, lambda a: a.ctypes.data      # noqa: E731
    hs = np.arange(n, dtype=np.uint32)
    cnt, fl, tot = st.state_sizes(hs)
    assert not fl.any()
    tr, ts = int(tot[0]), int(tot[1])
    rows, surv = np.zeros(max(tr, 1), STATE_ROW_DT), np.zeros(max(ts, 1), SURV_RESULT_DT)
    rng, flags, totals = np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32), np.zeros(2, np.uint64)
    clock, heads = np.zeros((n, S), np.uint32), np.zeros((n, S), np.uint32)
    out = CStateOut(tr, ts, p(rows), p(surv), p(rng), p(flags))

    def state(keep=(rows, surv, rng, flags, clock, heads)):
        rc = L.hm_store_state(st._h, n, p(hs), ctypes.byref(out), p(clock), p(heads), p(totals))
        assert rc == 0, rc

    def sizes():
        rc = L.hm_store_state_sizes(st._h, n, p(hs), None, None, p(totals))
        assert rc == 0, rc

    k = min(sample, n)
    read = {}

    def doc_read():
        inf = _DocInfo()
        for h in range(k):
            assert L.hm_doc_info(st._h, h, ctypes.byref(inf)) == 0
            rg, sv = np.zeros(inf.n_regs + 1, REG_RESULT_DT), np.zeros(inf.n_ops + 1, SURV_RESULT_DT)
            ck, hd = np.zeros(S, np.uint32), np.zeros(S, np.uint32)
            assert L.hm_doc_read(st._h, h, None, None, p(rg), p(sv), p(ck), None, p(hd)) == 0
            read[h] = (rg[:inf.n_regs], sv[:inf.n_surv], ck, hd)

    info = [st.info(h) for h in range(k)]
    full = np.ascontiguousarray(hist_len, np.uint32)
    _, ptot = st.past_sizes(hs, history=full)
    to, trg = int(ptot[2]), int(ptot[3])
    m_rows, m_olog = np.zeros(n, DOC_DT), np.zeros(max(to, 1), np.uint32)
    m_clock, m_heads = np.zeros(n * S, np.uint32), np.zeros(n * S, np.uint32)
    m_regs, m_surv, m_docs = np.zeros(max(trg, 1), REG_RESULT_DT), np.zeros(max(to, 1), SURV_RESULT_DT), np.zeros(n, DOC_RESULT_DT)
    view = CPastOut(0, 0, to, trg, p(m_rows), None, None, None, None, p(m_olog),
                    CResults(p(m_docs), p(m_clock), None, p(m_heads), None, None, p(m_regs), p(m_surv)))

    # (the two out structs hold raw addresses: every array they name stays referenced from the legs)
    keep = (rows, surv, rng, flags, clock, heads, totals, m_rows, m_olog, m_clock, m_heads, m_regs, m_surv, m_docs, full, hs)

    def materialize(keep=keep):
        rc = L.hm_store_materialize(st._h, n, p(hs), p(full), None, ctypes.byref(view), None)
        assert rc == 0, rc

    def agree():
        """the three routes hold the same documents: rows against hm_doc_read's live registers on the
        sample, live registers and survivors against the full-history materialize on all documents"""
        state(); doc_read(); materialize()
        ok = True
        for h in range(k):
            rg, sv, ck, hd = read[h]
            live = np.nonzero((rg["n_surv"] > 0) & (rg["obj"] != 0xFFFFFFFF) & (rg["obj"] < info[h]["n_objs"]))[0]
            r = rows[int(rng[h, 0]):int(rng[h, 0]) + int(rng[h, 1])]
            ok &= bool((r["reg"] == live).all() and (r["n_surv"] == rg["n_surv"][live]).all() and (r["index"] == rg["list_index"][live]).all())
            ok &= surv[int(rng[h, 2]):int(rng[h, 2]) + int(rng[h, 3])].tobytes() == sv.tobytes()
            ok &= bool((clock[h] == ck).all() and (heads[h] == hd).all())
        mlive = (m_regs[:trg]["n_surv"] > 0) & (m_regs[:trg]["obj"] != 0xFFFFFFFF)
        ok &= int(mlive.sum()) == tr and int(m_regs[:trg]["n_surv"][mlive].sum()) == ts
        ok &= bool((m_clock.reshape(n, S) == clock).all())
        return ok

    state_bytes = 16 * n_regs_total + 16 * ts + 20 * tr + 16 * ts
    return (("state", state), ("state_sizes", sizes), ("doc_read_sample", doc_read), ("materialize_full", materialize)), agree, \
        {"rows": tr, "survivors": ts, "state_bytes": state_bytes, "sample": k}


def measure(st, n, S, args, n_regs_total, hist_len):
    legs, agree, shape = legs_of(st, n, S, args.sample, n_regs_total, hist_len)
    for _ in range(args.warmup):
        for _, f in legs:
            f()
    ms = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, f in legs:
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    out = dict(shape)
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "runs_ms": [round(x, 3) for x in v]}
    out["doc_read_scaled"] = {"median_ms": out["doc_read_sample"]["median_ms"] * n / shape["sample"], "extrapolated": True}
    out["state_gbps"] = shape["state_bytes"] / (out["state"]["median_ms"] * 1e-3) / 1e9
    out["state_over_materialize"] = out["state"]["median_ms"] / out["materialize_full"]["median_ms"]
    out["equal"] = agree()
    return out


def workload(eng, name, n_docs, args):
    from hypermerge_amd import synth
    from hypermerge_amd.store import RowStore, slice_changes
    note = lambda m: print(f"[bench_state] {name}: {m}", file=sys.stderr, flush=True)      # noqa: E731
    b = synth.generate(synth.config(name, n_docs=n_docs), threads=min(16, os.cpu_count() or 1))
    n, S = b.n_docs, b.a_stride
    nch = b.docs["n_changes"].astype(np.int64)
    note(f"{n} documents, {len(b.changes)} changes, {len(b.ops)} ops, {int(b.docs['n_regs'].sum())} registers generated")
    st = RowStore(eng, a_stride=S)
    st.open_n(n)
    pos = np.maximum(nch - args.tail, 0)
    st.submit_batch(slice_changes(b, np.zeros(n, np.int64), pos), np.arange(n, dtype=np.uint32))
    res = st.wait()
    assert (res.docs["status"] == 0).all()
    hist_len = res.docs["hist_len"].astype(np.uint32)
    n_regs_total = int(b.docs["n_regs"].sum())
    out = {"workload": name, "docs": n, "a_stride": S, "registers": n_regs_total, "ops": len(b.ops)}
    out["after_remerge"] = measure(st, n, S, args, n_regs_total, hist_len)
    note(f"after the re-merge: {json.dumps({k: out['after_remerge'][k]['median_ms'] for k in ('state', 'materialize_full', 'doc_read_sample')})}")
    rng = np.random.default_rng(5)
    routed = 0
    for _ in range(2):
        hi = np.minimum(pos + rng.integers(1, 3, n), nch)
        sel = np.nonzero(hi > pos)[0]
        st.submit_batch(slice_changes(b, pos, hi, sel), sel.astype(np.uint32))
        res = st.wait()
        assert (res.docs["status"] == 0).all()
        hist_len[sel] = res.docs["hist_len"]
        routed += st.last_routing()["incremental"]
        pos = np.maximum(pos, hi)
    out["incremental_document_rounds"] = routed
    out["after_incremental"] = measure(st, n, S, args, n_regs_total, hist_len)
    note(f"after two rounds ({routed} incremental): {json.dumps({k: out['after_incremental'][k]['median_ms'] for k in ('state', 'materialize_full', 'doc_read_sample')})}")
    st.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c4-docs", type=int, default=100_000)
    ap.add_argument("--c3-docs", type=int, default=10_000)
    ap.add_argument("--only", choices=("c4", "c3"), default=None)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tail", type=int, default=4)
    args = ap.parse_args()
    from hypermerge_amd.engine import Engine
    eng = Engine(0)
    out = {"reps": args.reps, "warmup": args.warmup, "tail": args.tail, "workloads": []}
    if args.only != "c3":
        out["workloads"].append(workload(eng, "C4", args.c4_docs, args))
    if args.only != "c4":
        out["workloads"].append(workload(eng, "C3", args.c3_docs, args))
    print(json.dumps(out))
    assert all(w[k]["equal"] for w in out["workloads"] for k in ("after_remerge", "after_incremental"))


if __name__ == "__main__":
    main()
