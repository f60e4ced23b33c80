"""tests/general_edges.py without a GPU: every edge document merges with status 0 in the oracle, the
restated arithmetic puts the two documents of each pair on opposite sides of the pair's comparison
and of no other one, the closed-form shapes the edges were bisected over equal the encoded
documents' shapes, and the census slot names follow the kernel's header."""
import os
import re

import pytest

import oracle.oracle as O
from general_edges import (LARENA, RES_EXITS, SLOTS, UNREACHED_EXITS, YES_NO, chain, chain_shape, encode_pair, objects,
                           objects_shape, pair_shapes, pairs, res_layout, round_robin, round_robin_shape, route, shape_of,
                           stage_base, text, text_shape)
from hypermerge_amd.columnar import encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [p.name for p in pairs()]


def test_slots_follow_the_header():
    src = open(os.path.join(ROOT, "hypermerge_amd", "csrc", "merge_kernels.h")).read()
    body = re.search(r"enum hm_large_path \{(.*?)\};", src, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    names = [x.strip().split("=")[0].strip() for x in body.split(",") if x.strip()]
    assert names == ["HM_LP_" + x for x in SLOTS] + ["HM_LP_N"]
    large = open(os.path.join(ROOT, "hypermerge_amd", "csrc", "merge_large.hip")).read()
    for name, val in (("LARENA", LARENA), ("LA_MAX", 64), ("SEG_SHORT", 8), ("RES_SEG_MAX", 64)):
        assert re.search(rf"#define {name} {val}\b", large), name
    for x in SLOTS:                                   # every slot is counted somewhere (a "_NO" slot through its pair)
        assert re.search(rf"HM_LP_{x}\b", large) or x.endswith(("_NO", "_CARVED")), x


@pytest.mark.parametrize("p", pairs(), ids=IDS)
def test_pair_straddles_its_comparison_and_no_other(p):
    b = encode_pair(p)
    o = O.merge(b)
    assert (o.docs["status"] == 0).all(), o.docs["status"]
    assert (o.docs["n_queued"] == 0).all() and (o.docs["hist_len"] == b.docs["n_changes"]).all()
    lo, hi = pair_shapes(p, b)
    (dl, cl), (dh, ch_) = route(lo), route(hi)
    assert dl[p.comparison] is True and dh[p.comparison] is False
    moved = {k for k in dl if k in dh and dl[k] != dh[k]}
    assert moved - set(p.moves_with) == {p.comparison}, moved
    assert cl[p.slots[0]] > 0 and ch_[p.slots[0]] == 0, (cl, ch_)
    assert ch_[p.slots[1]] > 0 and cl[p.slots[1]] == 0, (cl, ch_)
    # one generator step apart
    d = b.docs
    steps = {"change": "n_changes", "op": "n_ops", "insert": "n_ops", "assign": None, "object": "n_objs", "actor": "n_actors"}
    f = steps.get(p.step)
    if p.step in ("order", "dep"):
        assert all(int(d[x][0]) == int(d[x][1]) for x in ("n_changes", "n_deps", "n_ops", "n_regs", "n_objs", "n_actors"))
    elif f:
        assert int(d[f][1]) - int(d[f][0]) == 1
    else:
        assert hi.max_assign - lo.max_assign == 1


def test_throwing_fallbacks_have_their_status():
    """The data-dependent fallbacks are taken by documents that merge; the same documents with the
    one throwing op each case names still throw that one status (the pool path's, after the
    fallback).  A set on the late pair's element 2 before element 3 exists: MISSING_ELEM."""
    late = next(p for p in pairs() if p.name == "late").docs[1]
    c = dict(late[1], ops=late[1]["ops"][:1] + [{"action": "set", "obj": "T", "key": f"{late[0]['actor']}:2", "value": "x"}]
             + late[1]["ops"][1:])
    o = O.merge(encode([[late[0], c]]))
    assert int(o.docs["status"][0]) == 5


def test_closed_form_shapes_equal_the_encoded_ones():
    for docs, want in ((chain(7, 30, 4), chain_shape(7, 30, 4)), (chain(3, 5, 9), chain_shape(3, 5, 9)),
                       (chain(9, 100, 11), chain_shape(9, 100, 11)), (text(3, 10), text_shape(3, 10)),
                       (round_robin(5, 23, 3), round_robin_shape(5, 23, 3)), (objects(4), objects_shape(4))):
        assert shape_of(encode([docs]), 0) == want


def test_unreachable_comparisons():
    """the arithmetic of the module docstring, evaluated"""
    n = LARENA // 4 // 8                                            # the gate's most changes
    assert n == 1200 and n * 9 + (4 * n + 64) + 8 * n <= LARENA - 2          # n·AS + T never over stage_base
    assert 8 * n + (4 * n + 64) <= stage_base(n, 0)                 # ltab always holds with A <= 8
    assert LARENA < 0xFFFF                                          # E <= LARENA implies E < 0xFFFF
    big = chain_shape(8, 32766, 32766)                              # R + O = 32767: tail is far over any limit
    assert res_layout(big)[1] > 8 * 32767 > LARENA
    assert set(UNREACHED_EXITS) < set(RES_EXITS) and len(YES_NO) == 8
