"""tests/inc_edges.py without a GPU: every pair's base log and base + round merge in the oracle with
status 0 and the queue the pair states, the two sides of a pair differ in exactly the step named,
the restatement routes them differently with the pair's declared slots among the differences, the
census names follow the kernel's header, and every slot of the enum is moved by some pair's
prediction or listed with the reason no round reaches it."""
import os
import re

import numpy as np
import pytest

import oracle.oracle as O
from hypermerge_amd.columnar import encode
from inc_edges import (EVENTS, EXITS, FAILG, FAMILY_SLOTS, META_ENDS, PASSES, SLOTS, UNREACHABLE, family, fold_targets, group_of,
                       limits, pairs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [p.name for p in pairs()]


def enum_names(src, name):
    body = re.search(rf"enum {name} \{{(.*?)\}};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return [x.strip().split("=")[0].strip() for x in body.split(",") if x.strip()]


def test_slots_follow_the_header():
    h = open(os.path.join(ROOT, "hypermerge_amd", "csrc", "store_kernels.h")).read()
    assert enum_names(h, "hm_inc_slot") == ["HM_IS_" + x for x in SLOTS] + ["HM_IS_N"]
    assert enum_names(h, "hm_inc_pass") == ["HM_IP_" + x for x in PASSES] + ["HM_IP_N"]
    k = open(os.path.join(ROOT, "hypermerge_amd", "csrc", "inc_kernels.hip")).read()
    for x in SLOTS:                                   # every slot is counted somewhere in the kernels
        assert re.search(rf"HM_IS_{x}\b", k), x
    assert set(EXITS) | set(EVENTS) | set(META_ENDS) | {"ENTER", "DONE"} == set(SLOTS)
    L = limits()                                      # relations the generators lean on, not values
    assert L["NC"] == L["HM_INC_MAX_NEW_C"] <= 8 <= L["LSV"] + 1 and L["LANE_TAIL"] <= L["KT_ROWS"] <= 64
    assert L["HM_INC_MAX_NEW_O"] == 64 and L["HM_INC_LANE_MAX_C"] > L["NC"] and L["META_LCH"] > L["HM_INC_TILED_MAX_C"]
    assert {x for f in FAMILY_SLOTS.values() for x in f} == set(SLOTS)


@pytest.mark.parametrize("p", pairs(), ids=IDS)
def test_pair_sides(p):
    rounds = p.rounds()
    docs = [d for base, new in p.sides for d in (base, list(base) + list(new))]
    o = O.merge(encode(docs, p.S)).docs
    thrown = tuple(x if x != 16 else 0 for x in p.status)        # (UNSUPPORTED is the engine's word: the oracle merges it)
    assert (o["status"][0::2] == 0).all() and tuple(int(x) for x in o["status"][1::2]) == thrown, o["status"]
    for k in range(2):
        if not thrown[k]:
            assert int(o["n_queued"][2 * k + 1]) == p.queued[k]
    if p.name != "meta_dirty":                        # (whose second base is the document with a queued change)
        assert (o["n_queued"][0::2] == 0).all()
    lo, hi = rounds
    base = [(r.res.n_c, r.res.n_d, r.res.n_o) for r in rounds]
    rows = [(r.nnc, r.nnd, r.nno) for r in rounds]
    if p.moved:
        assert (lo.moved, hi.moved) == p.moved
    elif p.plain and p.step != "base":
        assert base[0] == base[1]
    elif p.step == "change":                          # one change more, with the p.rows - 1 rows it carries
        assert base[0] == base[1] and hi.nnc - lo.nnc == 1 and sum(rows[1]) - sum(rows[0]) == max(p.rows, 2 if hi.nno > lo.nno else 1)
    elif p.step == "op":
        assert base[0] == base[1] and (hi.nnc, hi.nnd, hi.nno) == (lo.nnc, lo.nnd, lo.nno + 1)
    elif p.step == "dep":
        assert base[0] == base[1] and (hi.nnc, hi.nnd, hi.nno) == (lo.nnc, lo.nnd + 1, lo.nno)
    elif p.step == "base":                            # the same round; the base log one step longer: p.rows rows
        assert rows[0] == rows[1] and abs(sum(base[1]) - sum(base[0])) == p.rows
    else:
        assert p.step == "same" and base[0] == base[1] and rows[0] == rows[1]
    (pl, cl, rl), (ph, chi, rh) = p.route(0), p.route(1)
    assert sum(rl.values()) == 1 and sum(rh.values()) == 1
    for c in (cl, chi):                               # every pass that saw the document counted one way out
        for P in PASSES[:-1]:
            assert c[(P, "ENTER")] == c[(P, "DONE")] + sum(c[(P, x)] for x in EXITS)
        assert c[("META", "ENTER")] == sum(c[("META", x)] for x in META_ENDS)
    assert cl[p.slots[0]] > 0 and chi[p.slots[1]] > 0, (cl, chi)
    if not p.plain:
        assert cl != chi
        assert cl[p.slots[0]] != chi[p.slots[0]] and cl[p.slots[1]] != chi[p.slots[1]], (cl, chi)


def test_every_slot_has_a_pair_or_a_reason():
    """per family of passes: a new exit in the kernel needs a pair (or a written reason) before this passes"""
    moved = set()
    for p in pairs():
        for k in range(2):
            moved |= {(family(P), slot) for (P, slot), n in p.route(k)[1].items() if n}
    assert not moved & set(UNREACHABLE), moved & set(UNREACHABLE)
    every = {(f, x) for f, slots in FAMILY_SLOTS.items() for x in slots}
    assert moved <= every and set(UNREACHABLE) <= every
    left = sorted(every - moved - set(UNREACHABLE))
    assert not left, left


def test_unreachable_arithmetic():
    """the module docstring's bounds, evaluated"""
    L = limits()
    for G in (8, 16, 64):
        assert G + L["NC"] <= 2 * G                   # nt <= nnd + nnc, and 2 G steps pass: FOLD_STEPS
    assert L["HM_INC_MAX_TGT"] >= 64 + L["NC"]        # the plan's tgt bound is no tighter than a tile's
    for p in pairs():
        for r in p.rounds():
            assert len(fold_targets(r)) <= r.nnd + r.nnc
            assert r.res.s_used <= r.res.caps[2] and max(r.res.reg_surv, default=0) <= r.n_actors
    assert set(FAILG) < set(EXITS) and group_of(8) == 8 and group_of(12) == 16 and group_of(17) == 64
    assert (1 << L["SEQ_BITS"]) - 1 > 4096 * 64       # no tiny document holds a ready change of seq 2^24
