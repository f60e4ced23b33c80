#!/usr/bin/env python3
"""Where a docset's rounds get their per-op diffs: the host replay against the device's op-diff rows
(HM_DOCSET_DEVICE_DIFFS), on the shapes of bench.py's Node legs ("Round diffs from the
device").  Recorded, not gated.

Shapes: C2 (--c2-docs documents x 4 actors x 64 changes), C5 (--c5-docs nested maps / lists, 20% of
the changes delivered before their deps) and C3 (--c3-docs text documents), each fed to a docset in
rounds of --round changes per document, one hm_docset_apply call per round over every document.

The documents of a shape are generated and rendered as blocks once, into a temporary file.  Each
(shape, route) then runs in a child process of its own, the two routes alternately, --reps times, so
that a route's resident memory is not the other's freed pages.  A child loads the blocks, then —
with HM_DOCSET_PROFILE set and stderr caught — creates the docset and feeds it.  Per child:
  phases_ms      the docset's phase marks summed over the calls (decode, merge, read history | read
                 diffs, commit, read regs, diffs, verify, render)
  diffs_route_ms read history + diffs + verify (replay) or read diffs + diffs (device): what the two
                 routes do differently
  wall_s         the feed's calls, host clock
  rss_per_doc    the growth of the process's resident memory over docset creation and feed, per document
  diff_stats     rounds rendered from device rows, store calls, calls repeated with larger tables
  text_digest    a hash of every call's text: equal across the routes
Prints one JSON line: per shape and route the children's records and the medians."""
import argparse
import hashlib
import json
import os
import pickle
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASE = re.compile(r"^\[hm_docset\] (.+?)\s+([0-9.]+) ms$")


def documents(name, n, threads):
    """`n` synthetic `name` documents as Change JSON texts per document (map documents: the native
    block renderer's texts; documents with lists: decode_doc's changes)"""
    from hypermerge_amd import synth
    cfg = synth.config(name, n_docs=n)
    b = synth.generate(cfg, threads=threads)
    if name not in ("C2", "C4"):
        from hypermerge_amd.columnar import decode_doc
        return [[json.dumps(c).encode() for c in decode_doc(b, i)] for i in range(b.n_docs)]
    data, bo, db = synth.blocks(cfg, b)
    raw, bo = data.tobytes(), bo.tolist()
    return [[raw[bo[i]:bo[i + 1]] for i in range(int(db[d]), int(db[d + 1]))] for d in range(len(db) - 1)]


def rss_bytes():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


def child(args):
    from hypermerge_amd.docset import DocSet
    from hypermerge_amd.engine import Engine
    with open(args.blocks, "rb") as f:
        docs = pickle.load(f)
    n = len(docs)
    rounds = []
    for r in range((max(len(d) for d in docs) + args.round - 1) // args.round):
        sel = [i for i in range(n) if r * args.round < len(docs[i])]
        rounds.append((sel, [docs[i][r * args.round:(r + 1) * args.round] for i in sel]))
    n_changes = sum(len(d) for d in docs)
    eng = Engine(0)
    warm = DocSet(eng)                                        # (the first call of a process loads the kernels)
    w = warm.open(1)
    warm.apply_raw([w], [docs[0][:1]])
    warm.close()
    err = tempfile.TemporaryFile()
    saved = os.dup(2)
    rss0 = rss_bytes()
    ds = DocSet(eng, device_diffs=args.route == "device")
    first = ds.open(n)
    digest = hashlib.sha256()
    os.environ["HM_DOCSET_PROFILE"] = "1"
    sys.stderr.flush()
    os.dup2(err.fileno(), 2)
    try:
        t0 = time.perf_counter()
        for sel, blocks in rounds:
            res, text = ds.apply_raw([first + i for i in sel], blocks)
            digest.update(text)
        wall = time.perf_counter() - t0
    finally:
        os.dup2(saved, 2)
        del os.environ["HM_DOCSET_PROFILE"]
    rss1 = rss_bytes()
    err.seek(0)
    phases = {}
    for line in err.read().decode().splitlines():
        m = PHASE.match(line.strip())
        if m:
            phases[m.group(1)] = phases.get(m.group(1), 0.0) + float(m.group(2))
    keys = ("read diffs", "diffs") if args.route == "device" else ("read history", "diffs", "verify")
    print(json.dumps({"shape": args.shape, "route": args.route, "docs": n, "changes": n_changes, "calls": len(rounds), "wall_s": wall,
                      "phases_ms": {k: round(v, 3) for k, v in phases.items()}, "diffs_route_ms": round(sum(phases.get(k, 0.0) for k in keys), 3),
                      "rss_per_doc": (rss1 - rss0) / n, "diff_stats": ds.diff_stats(), "stats": ds.stats(), "text_digest": digest.hexdigest()[:16]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2-docs", type=int, default=20000)
    ap.add_argument("--c5-docs", type=int, default=5000)
    ap.add_argument("--c3-docs", type=int, default=500)
    ap.add_argument("--round", type=int, default=16, help="changes per document and call")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", help="(child) the shape to feed")
    ap.add_argument("--route", choices=["replay", "device"], help="(child) where the diffs come from")
    ap.add_argument("--blocks", help="(child) the file of the shape's rendered blocks")
    args = ap.parse_args()
    if args.shape:
        return child(args)
    out = {"round": args.round, "reps": args.reps}
    for shape, n in (("C2", args.c2_docs), ("C5", args.c5_docs), ("C3", args.c3_docs)):
        if n <= 0:
            continue
        runs = {"replay": [], "device": []}
        with tempfile.NamedTemporaryFile(suffix=".blocks") as tf:
            pickle.dump(documents(shape, n, min(16, os.cpu_count() or 1)), tf)
            tf.flush()
            print(f"[bench_docset_diffs] {shape}: {n} documents rendered", file=sys.stderr, flush=True)
            for _ in range(args.reps):
                for route in ("replay", "device"):
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", shape, "--route", route, "--blocks", tf.name,
                                        "--round", str(args.round)], capture_output=True, text=True, timeout=900)
                    if p.returncode != 0:
                        raise SystemExit(f"{shape} {route}: exit {p.returncode}\n{p.stderr[-2000:]}")
                    runs[route].append(json.loads(p.stdout.strip().splitlines()[-1]))
                    print(f"[bench_docset_diffs] {shape} {route}: {runs[route][-1]['diffs_route_ms']:.1f} ms", file=sys.stderr, flush=True)
        rec = {"docs": n, "same_texts": len({r["text_digest"] for v in runs.values() for r in v}) == 1}
        for route, v in runs.items():
            med = lambda f: statistics.median(f(r) for r in v)      # noqa: E731
            rng = lambda f: [min(f(r) for r in v), max(f(r) for r in v)]      # noqa: E731
            rec[route] = {"diffs_route_ms": {"median": med(lambda r: r["diffs_route_ms"]), "range": rng(lambda r: r["diffs_route_ms"])},
                          "wall_s": {"median": med(lambda r: r["wall_s"]), "range": rng(lambda r: r["wall_s"])},
                          "rss_per_doc": {"median": med(lambda r: r["rss_per_doc"]), "range": rng(lambda r: r["rss_per_doc"])},
                          "repeated_share": (sum(r["diff_stats"]["repeated"] for r in v) / max(1, sum(r["diff_stats"]["calls"] - r["diff_stats"]["repeated"] for r in v))),
                          "runs": v}
        out[shape] = rec
        assert rec["same_texts"], shape
    print(json.dumps(out))


if __name__ == "__main__":
    main()
