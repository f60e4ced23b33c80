"""tests/clock_diffs_ref.py (the restatement the clock-diff tests compare the device with) pinned
three ways: on the existing route (past_ref gathers at the clock, the C oracle merges the gathered
batch, op_diffs_ref / list_diffs_ref run over that merge's whole history: the same rows, op for op,
and the oracle queues exactly selected minus applied-at-clock), on the JS restatement (the patch of
one applyChanges call on Backend.init() with the selected changes in history order), and by
properties."""
import json
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import decode_doc
import oracle.oracle as O

from clock_diffs_ref import applied_at, census, clock_diffs, clocks_of, is_prefix, selected_at
from fuzz_docs import gen_docs
from list_diffs_ref import ELEM_INSERT, ELEM_REMOVE, ELEM_SET, list_diffs, render, rga_positions
from op_diffs_cases import sources
from op_diffs_ref import CREATE, LISTS, op_diffs
from past_ref import clock_at, gather, hist_len, select, source_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
SEED = 1701


def synthetic():
    b = synth.generate(synth.config("C3", n_docs=2, changes_per_actor=30), threads=2)
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    b = synth.generate(synth.config("C5", n_docs=10, arrival=2, shuffle_pct=40, dup_pct=15), threads=2)
    return docs + [decode_doc(b, i) for i in range(b.n_docs)]


@lru_cache(maxsize=None)
def corpus():
    """[(docs, batch, [(Source, all_deps)], S, [[(kind, clock)] per document])]: fuzz documents of the
    default and wide profiles and synthetic C3 / C5 ones, with the clocks each is asked at"""
    out = []
    rng = np.random.default_rng(SEED)
    for docs, S in ((gen_docs("default", range(100, 116)) + synthetic(), 8), (gen_docs("wide", range(200, 204)), 64)):
        b, r, srcs = sources(docs, S)
        for d, (src, _) in enumerate(srcs):
            assert len(src.changes) == len(docs[d])           # (log order is arrival order)
        out.append((docs, b, srcs, S, [clocks_of(src, ad, S, rng) for src, ad in srcs]))
    return tuple(out)


def requests():
    return [(d, src, ad, S, kind, k, part) for part, (docs, b, srcs, S, clocks) in enumerate(corpus())
            for d, ((src, ad), ks) in enumerate(zip(srcs, clocks)) for kind, k in ks]


def test_census_of_the_generated_clocks():
    """a quarter of the clocks are closed without being a prefix, a quarter leave changes queued"""
    n, closed, queued = census([(src, ad, S, k) for _, src, ad, S, _, k, _ in requests()])
    assert n >= 150 and 4 * closed >= n and 4 * queued >= n, (n, closed, queued)


def test_the_gathered_batch_merged_by_the_oracle_gives_the_same_rows():
    kinds = set()
    for d, src, ad, S, kind, k, _ in requests():
        g, clog, olog = gather([(src, None, k)], S)
        o = O.merge(g)
        assert int(o.docs["status"][0]) == 0
        mine = clock_diffs(src, ad, S, k, lists=True)
        assert int(o.docs["n_queued"][0]) == mine.queued and int(o.docs["hist_len"][0]) == mine.applied, (d, kind)
        # the cold merge applies the same changes in the same order
        m = applied_at(src, ad, S, k)
        idx = np.flatnonzero(m)
        idx = idx[np.argsort(src.hist[idx], kind="stable")]
        gh = np.asarray(o.hist[:len(clog)])
        assert [int(clog[i]) for i in np.argsort(gh, kind="stable") if gh[i] >= 0] == [int(x) for x in idx], (d, kind)
        gsrc, gad = source_of(g, o.hist, 0), np.asarray(o.all_deps).reshape(-1, S)
        via = list_diffs(gsrc, gad, S, 0, hist_len(gsrc))
        assert via.bad == 0 and mine.diffs.bad == 0 and via.flags == mine.diffs.flags == 0
        back = lambda sv: [(int(olog[x]), vt, v) for x, vt, v in sv]
        assert [(int(olog[op]), kd, ix, back(sv)) for op, kd, ix, sv in via.rows] == mine.diffs.rows, (d, kind)
        plain, vplain = clock_diffs(src, ad, S, k).diffs, op_diffs(gsrc, gad, S, 0, hist_len(gsrc))
        assert plain.flags == vplain.flags and [(int(olog[op]), kd, back(sv)) for op, kd, sv in vplain.rows] == plain.rows
        kinds |= {kd for _, kd, _, _ in mine.diffs.rows}
    assert {CREATE, ELEM_INSERT, ELEM_SET, ELEM_REMOVE} <= kinds


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_restatement_gives_the_same_patch_for_the_selected_changes():
    reqs = requests()
    feed = []
    for d, src, ad, S, kind, k, part in reqs:
        docs = corpus()[part][0]
        feed.append([docs[d][int(i)] for i in select(src, clock=k)])         # selected, in history order
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_clock_patch.js")], input=json.dumps({"docs": feed}),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])["docs"]
    for (d, src, ad, S, kind, k, part), j in zip(reqs, got):
        assert j["err"] is None, (d, kind, j["err"])
        mine = clock_diffs(src, ad, S, k, lists=True)
        assert (j["history"], j["queued"]) == (mine.applied, mine.queued), (d, kind)
        assert render(corpus()[part][1], d, src, mine.diffs) == j["patch"]["diffs"], (d, kind)


def test_a_prefix_clock_gives_the_rows_of_the_prefix_slice():
    for part, (docs, b, srcs, S, _) in enumerate(corpus()):
        for src, ad in srcs:
            H = hist_len(src)
            for p in sorted({0, 1, H // 3, H // 2, H - 1, H} & set(range(H + 1))):
                k = clock_at(src, S, p)
                m = applied_at(src, ad, S, k)
                assert is_prefix(src, m) and int(m.sum()) == min(p, H) and not (selected_at(src, k) & ~m).any()
                assert clock_diffs(src, ad, S, k, lists=True).diffs == list_diffs(src, ad, S, 0, p)
                assert clock_diffs(src, ad, S, k).diffs == op_diffs(src, ad, S, 0, p)


def test_last_row_per_register_and_visible_elements_are_the_merge_at_the_clock():
    seen = 0
    for d, src, ad, S, kind, k, _ in requests():
        if kind == "prefix":
            continue
        g, clog, olog = gather([(src, None, k)], S)
        o = O.merge(g)
        at = clock_diffs(src, ad, S, k, lists=True)
        last, elem = {}, {}
        for op, kd, ix, sv in at.diffs.rows:
            if kd == CREATE:
                continue
            reg = int(src.ops[op]["reg"])
            last[reg] = sv
            if kd in (ELEM_INSERT, ELEM_SET, ELEM_REMOVE):
                elem[reg] = (int(src.ops[op]["obj"]), kd != ELEM_REMOVE)
        want_vis = {}
        for reg in range(src.n_regs):
            row = o.regs[reg]
            want = [(int(olog[int(x["op"])]), int(x["vtag"]), int(x["value"]))
                    for x in o.surv[int(row["surv_off"]):int(row["surv_off"]) + int(row["n_surv"])]]
            assert last.get(reg, []) == want, (d, kind, reg)
            if int(row["list_index"]) >= 0:
                want_vis.setdefault(int(row["obj"]), []).append((int(row["list_index"]), reg))
        from clock_diffs_ref import restricted
        pos, _ = rga_positions(restricted(src, applied_at(src, ad, S, k)), at.applied)
        vis = {}
        for reg, (obj, v) in elem.items():
            if v:
                vis.setdefault(obj, []).append(reg)
        assert {obj: sorted(r, key=pos.__getitem__) for obj, r in vis.items()} == \
            {obj: [reg for _, reg in sorted(v)] for obj, v in want_vis.items()}, (d, kind)
        seen += sum(len(v) for v in want_vis.values())
    assert seen > 300


def test_without_lists_a_document_that_assigns_elements_is_flagged():
    flagged = 0
    for d, src, ad, S, kind, k, _ in requests():
        a, b = clock_diffs(src, ad, S, k), clock_diffs(src, ad, S, k, lists=True)
        has = any(kd in (ELEM_INSERT, ELEM_SET, ELEM_REMOVE) for _, kd, _, _ in b.diffs.rows)
        # (an element assign whose register stays invisible emits no row and still flags)
        assert (a.diffs.flags == LISTS) or not has
        flagged += a.diffs.flags == LISTS
        if not a.diffs.flags:
            assert [(op, kd, sv) for op, kd, _, sv in b.diffs.rows] == a.diffs.rows
    assert flagged > 10
