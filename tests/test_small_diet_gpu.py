"""merge_small_kernel's map launches after the instruction-stream diet (loop bounds taken from the
size class, the fold check's suspect test without per-lane walks, one packed word pair per op, one
LDS row per register, list documents handed to the general kernel before any error key): every
result table bit-exact with the oracle, through the product library and through the check build
(libhmgpu_check.so must count checked documents and no mismatch).

The documents are the hand-built ones of tests/small_diet_docs.py (checked against the oracle alone
by tests/test_small_diet_docs.py), one launch per group, mixed with generated C4 documents.  The
persistent grid is one wave per resident workgroup, at most one per document, so a wave only goes
on to a next document in a batch larger than the grid: a batch is 40 generated documents, the hand-built
ones, a grid's worth of generated ones, the hand-built ones again, 8 more.  Each hand-built document is
so merged once as a wave's first document (followed by a generated one) and once as its second
(rows loaded asynchronously behind a generated one's stores).  The launch's instantiation is
asserted where the group is built for one; the documents a launch without the list carve must
hand over are asserted through Engine.last_deferred."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "hypermerge_amd", "_lib")
LIBS = {"product": os.path.join(LIBDIR, "libhmgpu.so"), "check": os.path.join(LIBDIR, "libhmgpu_check.so")}

pytestmark = pytest.mark.gpu

SCRIPT = r'''
import ctypes, dataclasses, json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from hypermerge_amd import synth, engine as E
from hypermerge_amd.columnar import Batch, encode
import oracle.oracle as O
from small_diet_docs import groups

L = E.lib()
L.hm_debug_async_check.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
cnt = (ctypes.c_ulonglong * 2)()
check_build = L.hm_debug_async_check(cnt, 1) == 1
eng = E.Engine(0)


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


def rows(mask, counts):
    return np.repeat(mask, counts)


out = {}
for gname, g in groups().items():
    names = [n for n, _, _ in g["docs"]]
    hand = encode([d for _, d, _ in g["docs"]], 8)
    f = g["filler"]
    gen = lambda n, **kw: synth.generate(synth.config(f["config"], n_docs=n, **f["over"], **kw))
    head, tail = gen(40), gen(8, arrival=1)
    def build(mid):
        b = concat([head, hand, mid, hand, tail], 8)
        if g.get("clear_list_flag"):
            b.docs["flags"] &= ~np.uint16(1)                  # HM_DOC_HAS_LISTS is a launch hint only
        return b
    per_cu, cus = eng.small_occupancy(build(gen(8)))[:2]
    grid = int(per_cu) * int(cus)
    b8 = build(gen(grid, arrival=2, shuffle_pct=30))
    assert list(eng.small_occupancy(b8)[:2]) == [per_cu, cus], "the batch launches another grid than the probe"
    firsts = (head.n_docs, head.n_docs + hand.n_docs + grid)
    for S in g["strides"]:
        b = dataclasses.replace(b8, a_stride=S)
        launch = [int(x) for x in eng.small_occupancy(b)[2:]]
        gr = eng.merge(b)
        deferred = set(int(x) for x in eng.last_deferred(b.n_docs))
        o = O.merge(b, threads=4)
        ok = o.docs["status"] == 0
        bad = []
        if not np.array_equal(gr.docs["status"], o.docs["status"]): bad.append("docs.status")
        for fld in ("err_change", "err_op"):
            if not np.array_equal(gr.docs[fld][~ok], o.docs[fld][~ok]): bad.append("docs." + fld)
        if not np.array_equal(gr.docs[ok], o.docs[ok]): bad.append("docs")
        for fld in ("clock", "back_clock", "heads"):
            m = rows(ok, S)
            if not np.array_equal(getattr(gr, fld)[m], getattr(o, fld)[m]): bad.append(fld)
        cm = rows(ok, b.docs["n_changes"])
        if not np.array_equal(gr.hist[cm], o.hist[cm]): bad.append("hist")
        if not np.array_equal(gr.all_deps[rows(cm, S)], o.all_deps[rows(cm, S)]): bad.append("all_deps")
        if not np.array_equal(gr.regs[rows(ok, b.docs["n_regs"])], o.regs[rows(ok, b.docs["n_regs"])]): bad.append("regs")
        sm = rows(ok, b.docs["n_ops"])                        # a document's survivor rows: all n_ops of them
        if not np.array_equal(gr.surv[sm], o.surv[sm]): bad.append("surv")
        hand_rows = set(first + i for first in firsts for i in range(len(names)))
        r = {"bad_tables": bad, "launch": launch, "grid": grid, "n_docs": b.n_docs,
             "status": [{n: int(o.docs["status"][first + i]) for i, n in enumerate(names)} for first in firsts],
             "filler_ok": bool(all(ok[d] for d in range(b.n_docs) if d not in hand_rows)),
             "deferred": [sorted(n for i, n in enumerate(names) if first + i in deferred) for first in firsts]}
        if check_build:
            assert L.hm_debug_async_check(cnt, 1) == 1
            r.update(checked=int(cnt[0]), mismatches=int(cnt[1]))
        out[f"{gname}/S{S}"] = r
        print(gname, S, r, file=sys.stderr, flush=True)
print(json.dumps({"check_build": check_build, "cases": out}))
'''


@pytest.fixture(scope="module")
def expected():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from small_diet_docs import groups
    return groups()


@pytest.mark.parametrize("which", ["product", "check"])
def test_bit_exact_with_oracle(which, expected):
    assert os.path.exists(LIBS[which]), "library not built (hypermerge_amd/build.py)"
    env = dict(os.environ, HMGPU_LIB=LIBS[which])
    p = subprocess.run([sys.executable, "-c", SCRIPT, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["check_build"] == (which == "check")
    assert len(got["cases"]) == sum(len(g["strides"]) for g in expected.values())
    checked = 0
    for case, r in got["cases"].items():
        g = expected[case.split("/")[0]]
        assert r["bad_tables"] == [], (case, r)
        assert r["filler_ok"], (case, r)
        assert r["n_docs"] > r["grid"] + 40, (case, r)          # waves go on to second documents
        assert r["status"] == [{n: s for n, _, s in g["docs"]}] * 2, (case, r)
        if g.get("inst"):
            assert tuple(r["launch"]) == g["inst"], (case, r)
        if g.get("cls") is not None:
            assert r["launch"][1] == g["cls"] and r["launch"][2] == 0, (case, r)
        # a launch without the list carve hands the list documents to the general kernel, and keeps
        # the document that only throws
        for copy in r["deferred"]:
            assert all(n in copy for n in g.get("deferred", ())), (case, r)
            assert not any(n in copy for n in g.get("kept", ())), (case, r)
        if which == "check":
            assert r["mismatches"] == 0, (case, r)
            checked += r["checked"]
    if which == "check":
        assert checked > 0, got
