"""merge_small_kernel at five waves per SIMD (map documents of <= 128 ops in the small LDS
carves): results bit-exact with the oracle on every result table, through the product library
and through the check build (libhmgpu_check.so, which re-reads every asynchronously loaded row
set with counted loads and must count no difference), and the persistent grid's residency.

Batches hold 3 x grid + 7 documents (grid = resident workgroups per CU x CUs, as the launcher
computes it), so every wave loads next documents and the waves take unequal counts.  They come
from the C4 generator (8 actors, and a 4-actor variant of it that launches the same five-wave
instantiation) and the C2 generator in generation, actor-major and shuffled order, with edge documents
(one change; changes without ops; no dep rows at all; exactly 64 ops; exactly 65 ops) first and
last, so their rows lie at both ends of every table.  Row strides 4, 5, 8 and 16, each where the
batch allows it: a batch's a_stride is at least its largest n_actors (include/hypermerge_amd.h;
the oracle, like every host consumer, sizes its rows by it), so the 4-actor batches run under all
four and the 8-actor C4 batches under 8 and 16."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "hypermerge_amd", "_lib")
LIBS = {"product": os.path.join(LIBDIR, "libhmgpu.so"), "check": os.path.join(LIBDIR, "libhmgpu_check.so")}
MIN_PER_CU = 20          # C4 instantiation: 5 waves on each of a CU's 4 SIMDs

pytestmark = pytest.mark.gpu

SCRIPT = r'''
import ctypes, dataclasses, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from hypermerge_amd import synth, engine as E
from hypermerge_amd.columnar import Batch, ROOT_ID, decode_doc, encode
import oracle.oracle as O

TABLES = ("docs", "clock", "back_clock", "heads", "hist", "all_deps", "regs", "surv")
L = E.lib()
L.hm_debug_async_check.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
cnt = (ctypes.c_ulonglong * 2)()
check_build = L.hm_debug_async_check(cnt, 1) == 1
eng = E.Engine(0)


def edge_docs(src):
    """One of each edge kind, from a generated document's changes and by hand."""
    log = decode_doc(src, 0)
    def sets(n0, n):   # n set ops over 16 keys of the root map
        return [{"action": "set", "obj": ROOT_ID, "key": f"k{j % 16}", "value": j} for j in range(n0, n0 + n)]
    def chain(per_change):   # one actor, consecutive seqs
        out, j = [], 0
        for i, n in enumerate(per_change):
            out.append({"actor": "aa", "seq": i + 1, "deps": {}, "ops": sets(j, n)})
            j += n
        return out
    one = [dict(chain([3])[0])]
    no_ops = [dict(c, ops=[]) for c in log]
    no_deps = chain([2] * 9)
    ops64 = chain([8] * 8)
    ops65 = chain([8] * 7 + [9])
    assert sum(len(c["ops"]) for c in ops64) == 64 and sum(len(c["ops"]) for c in ops65) == 65
    return [one, no_ops, no_deps, ops64, ops65]


def concat(parts, S):
    """Batches one after the other (offsets of the later ones shifted)."""
    docs, chs, deps, ops = [], [], [], []
    nc = nd = no = nr = 0
    for b in parts:
        d, c = b.docs.copy(), b.changes.copy()
        d["change_off"] += nc; d["dep_off"] += nd; d["op_off"] += no; d["reg_off"] += nr
        c["dep_off"] += nd; c["op_first"] += no
        docs.append(d); chs.append(c); deps.append(b.deps); ops.append(b.ops)
        nc += len(b.changes); nd += len(b.deps); no += len(b.ops); nr += int(b.docs["n_regs"].sum())
    return Batch(np.concatenate(docs), np.concatenate(chs), np.concatenate(deps), np.concatenate(ops), S)


out = {}
SOURCES = {"C4": ("C4", {}), "C4a4": ("C4", {"actors": 4, "changes_per_actor": 16}), "C2": ("C2", {})}
probe = {n: synth.generate(synth.config(c, n_docs=4096, **kw)) for n, (c, kw) in SOURCES.items()}
assert eng.small_occupancy(probe["C4a4"]) == eng.small_occupancy(probe["C4"])      # <2, no lists, class 0>, no counters
for name, (cfg_name, kw) in SOURCES.items():
    per_cu, cus = eng.small_occupancy(probe[name])[:2]
    grid = per_cu * cus
    edges = encode(edge_docs(probe[name]), 8)
    n_synth = 3 * grid + 7 - 2 * edges.n_docs
    for arrival, extra in ((0, {}), (1, {}), (2, {"shuffle_pct": 30})):
        body = synth.generate(synth.config(cfg_name, n_docs=n_synth, arrival=arrival, **kw, **extra))
        b8 = concat([edges, body, edges], 8)
        assert b8.n_docs == 3 * grid + 7
        assert eng.small_occupancy(b8) == eng.small_occupancy(probe[name]), "the batch launches another instantiation than the probe"
        for S in (s for s in (4, 5, 8, 16) if s >= int(b8.docs["n_actors"].max())):
            b = dataclasses.replace(b8, a_stride=S)          # (the tables do not depend on the row stride)
            g = eng.merge(b)
            o = O.merge(b, threads=16)
            bad = [f for f in TABLES if not np.array_equal(getattr(g, f), getattr(o, f))]
            ne = edges.n_docs
            r = {"bad_tables": bad, "launch": list(eng.small_occupancy(b8)),
                 "edges_ok": bool((o.docs["status"][:ne] == 0).all() and (o.docs["status"][-ne:] == 0).all())}
            if check_build:
                assert L.hm_debug_async_check(cnt, 1) == 1
                r.update(checked=int(cnt[0]), mismatches=int(cnt[1]))
            out[f"{name}/arrival{arrival}/S{S}"] = r
            print(name, arrival, S, r, file=sys.stderr, flush=True)
print(json.dumps({"check_build": check_build, "cases": out}))
'''


@pytest.mark.parametrize("which", ["product", "check"])
def test_bit_exact_with_oracle(which):
    assert os.path.exists(LIBS[which]), "library not built (hypermerge_amd/build.py)"
    env = dict(os.environ, HMGPU_LIB=LIBS[which])
    p = subprocess.run([sys.executable, "-c", SCRIPT, ROOT], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["check_build"] == (which == "check")
    assert len(got["cases"]) == 3 * 2 + 3 * 4 + 3 * 4        # C4 under 8 and 16; its 4-actor variant and C2 under 4, 5, 8 and 16
    checked = 0
    for case, r in got["cases"].items():
        assert r["bad_tables"] == [], (case, r)
        assert r["edges_ok"], (case, r)                      # every edge document, first and last, merges with status 0
        if not case.startswith("C2/"):
            assert r["launch"][0] >= MIN_PER_CU and r["launch"][2:] == [2, 0, 0, 0], (case, r)   # the five-wave instantiation
        if which == "check":
            assert r["mismatches"] == 0, (case, r)
            checked += r["checked"]
    if which == "check":
        assert checked > 100000, got                         # the asynchronous path (C4 and its variant) was taken and checked


def test_c4_grid_is_resident_at_five_waves():
    """The launcher's own figure (registers and LDS of the instantiation): a later register creep
    that costs the fifth wave fails here instead of silently shrinking the grid."""
    sys.path.insert(0, ROOT)
    from hypermerge_amd import synth
    from hypermerge_amd.engine import Engine
    per_cu, cus, opl, cls, lists, counters = Engine(0).small_occupancy(synth.generate(synth.config("C4", n_docs=64)))
    assert (opl, cls, lists, counters) == (2, 0, 0, 0)
    assert per_cu >= MIN_PER_CU, per_cu
    assert (per_cu * cus) % 8 == 0, (per_cu, cus)            # the XCD remap needs a multiple of 8
