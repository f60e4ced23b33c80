#!/usr/bin/env python3
"""Local-change latency on resident documents, once per undo route of the Node drop-in, and
hm_store_fields on its own (needs the GPU; not part of bench.py).

  documents   "text": one text document of C3's size (one writer, ~3.7k ops: makeText and 1850
              inserted characters in changes of 50), "map": one small map document (8 keys)
  backend     tools/bench_local_change.js: inserts (a keystroke: ins + set), deletes and undo / redo
              requests through GpuDocBackend in sync mode, each request issued to an engine with
              undo: 'view' and to one with undo: 'fields', alternating which goes first; time = host
              clock from applyLocalChange to engine.idle() (the round's device work has finished)
  store       hm_store_fields alone for 1, 1k and 100k requests (two fields each, the base clock
              the document's whole clock) over 1024 resident map documents and the text document;
              time = host clock around the synchronous call, tables packed beforehand
Every figure is the median and the 10th / 90th percentile of the kept samples, in microseconds.
Writes one JSON object to --out (default: stdout only)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = "00000000-0000-0000-0000-000000000000"


def text_doc(chars=1850, per_change=50):
    changes, prev, e = [], "_head", 0
    for k in range(chars // per_change):
        ops = [{"action": "makeText", "obj": "T"}, {"action": "link", "obj": R, "key": "text", "value": "T"}] if k == 0 else []
        for _ in range(per_change):
            e += 1
            ops += [{"action": "ins", "obj": "T", "key": prev, "elem": e}, {"action": "set", "obj": "T", "key": f"aaaa:{e}", "value": "a"}]
            prev = f"aaaa:{e}"
        changes.append({"actor": "aaaa", "seq": k + 1, "deps": {}, "ops": ops})
    return changes, prev


def map_doc(i=0):
    return [{"actor": "aaaa", "seq": 1, "deps": {}, "ops": [{"action": "set", "obj": R, "key": f"k{k}", "value": i + k} for k in range(8)]},
            {"actor": "bbbb", "seq": 1, "deps": {}, "ops": [{"action": "set", "obj": R, "key": "k0", "value": -i}]}]


def stats(us):
    a = np.sort(np.asarray(us, np.float64))
    return {"median_us": round(float(np.median(a)), 1), "p10_us": round(float(np.percentile(a, 10)), 1),
            "p90_us": round(float(np.percentile(a, 90)), 1), "samples": len(a)}


def bench_backend(args):
    text, last = text_doc()
    cfg = {"docs": {"text": {"changes": text, "text": "T", "last": last}, "map": {"changes": map_doc()}},
           "inserts": args.inserts, "deletes": args.deletes, "undos": args.undos}
    p = subprocess.run(["node", os.path.join(ROOT, "tools", "bench_local_change.js")], input=json.dumps(cfg),
                       capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(p.stderr[-4000:])
    got = json.loads(p.stdout.strip().splitlines()[-1])
    return {doc: {route: {kind: stats(v) for kind, v in kinds.items() if v} for route, kinds in routes.items()}
            for doc, routes in got.items()}


def bench_store(args):
    from hypermerge_amd.engine import FIELD_OP_DT, Engine, pack_entries, pack_fields
    from hypermerge_amd.store import DocStore
    eng = Engine(0)
    store = DocStore(eng, a_stride=8)
    hs = [store.open() for _ in range(1025)]
    text, _ = text_doc()
    res = store.apply([(hs[0], text)] + [(h, map_doc(i)) for i, h in enumerate(hs[1:])])
    assert (res.docs["status"] == 0).all()
    out = {}
    for n in (1, 1000, 100000):
        req = np.array([hs[0]] if n == 1 else [hs[1 + (i % 1024)] for i in range(n)], np.uint32)
        have = [[(0, len(text))] if n == 1 else [(0, 1), (1, 1)] for _ in range(n)]
        fields = [[5, 6] if n == 1 else [0, 3] for _ in range(n)]
        off, ea, es = pack_entries(have, n)
        foff, freg = pack_fields(fields, n)
        flags, rng = np.zeros(n, np.uint32), np.zeros((2 * n + 1, 2), np.uint32)
        cap = 4 * n
        rows, tot = np.zeros(cap, FIELD_OP_DT), ctypes.c_uint32()
        call = lambda: store._L.hm_store_fields(store._h, n, req.ctypes.data, off.ctypes.data, ea.ctypes.data, es.ctypes.data,
                                                foff.ctypes.data, freg.ctypes.data, flags.ctypes.data, None, rng.ctypes.data,
                                                rows.ctypes.data, cap, ctypes.byref(tot))
        us = []
        for i in range(args.reps + 5):
            t0 = time.perf_counter()
            st = call()
            dt = time.perf_counter() - t0
            assert st == 0 and tot.value > 0, (st, tot.value)
            if i >= 5:
                us.append(dt * 1e6)
        out[str(n)] = dict(stats(us), rows=int(tot.value))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--inserts", type=int, default=200)
    ap.add_argument("--deletes", type=int, default=200)
    ap.add_argument("--undos", type=int, default=50)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out")
    args = ap.parse_args()
    out = {"backend": bench_backend(args), "store_fields": bench_store(args)}
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
