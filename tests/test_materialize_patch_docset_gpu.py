"""hm_docset_materialize_patch: fed in rounds, the patch of a document at each round boundary's history
length holds the concatenation of the diffs hm_docset_apply's patches returned so far (the host
replay of each round is the second oracle), with the boundary's clock and deps; a shuffled feed leaves
changes queued across rounds; a text document is handed back to the host."""
import json

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import decode_doc
from hypermerge_amd.docset import DocSet
from hypermerge_amd.engine import EngineError

from op_diffs_cases import HAND, chain_doc, one_register_doc, wide_doc

pytestmark = pytest.mark.gpu


def _blocks(changes):
    return [json.dumps(c, separators=(",", ":")).encode() for c in changes]


def test_patch_at_round_boundaries_is_the_rounds_diffs_so_far(engine):
    b = synth.generate(synth.config("C2", n_docs=12, counter_pct=20))
    logs = [decode_doc(b, i) for i in range(b.n_docs)]
    b = synth.generate(synth.config("C2", n_docs=8, arrival=2, shuffle_pct=40, dup_pct=10))     # changes stay queued across rounds
    logs += [decode_doc(b, i) for i in range(b.n_docs)]
    names = [k for k in sorted(HAND) if k != "text"]
    logs += [HAND[k] for k in names] + [chain_doc(40, 3), one_register_doc(50), wide_doc(20)]
    ds = DocSet(engine)
    first = ds.open(len(logs) + 2)
    ids = list(range(first, first + len(logs)))
    text, unplaced = first + len(logs), first + len(logs) + 1
    rng = np.random.default_rng(3)
    cuts = [[0] + sorted(int(x) for x in rng.integers(0, len(l) + 1, size=3)) + [len(l)] for l in logs]
    diffs = {x: [] for x in ids}
    queued_seen = False
    for r in range(4):
        part = [(x, logs[i][cuts[i][r]:cuts[i][r + 1]]) for i, x in enumerate(ids)]
        part = [(x, c) for x, c in part if c]
        res, out = ds.apply([x for x, _ in part], [_blocks(c) for _, c in part])
        assert (res["status"] == 0).all()
        queued_seen |= bool(res["n_queued"].any())
        patches = {x: p for (x, _), p in zip(part, out["p"])}
        for x, p in patches.items():
            diffs[x] += p["diffs"]
        placed = [x for x in ids if ds.info(x)["a_stride"]]
        got = ds.materialize_patch(placed, [ds.info(x)["hist_len"] for x in placed])
        for x, g in zip(placed, got):
            assert g["doc"] == x and g["history"] == ds.info(x)["hist_len"]
            assert g["patch"]["diffs"] == diffs[x], (r, x)
            assert (g["patch"]["canUndo"], g["patch"]["canRedo"]) == (False, False)
            if x in patches:
                assert g["patch"]["clock"] == patches[x]["clock"] and g["patch"]["deps"] == patches[x]["deps"], (r, x)
    assert queued_seen
    # an earlier boundary, a length past the end, a document asked twice, one not placed yet
    x = ids[0]
    h = ds.info(x)["hist_len"]
    got = ds.materialize_patch([x, x, x, unplaced], [h, h + 9, 0, 4])
    assert got[0] == got[1] and got[2]["patch"]["diffs"] == [] and got[2]["patch"]["clock"] == {}
    assert got[3] == {"doc": unplaced, "history": 0, "patch": {"clock": {}, "deps": {}, "canUndo": False, "canRedo": False, "diffs": []}}
    # the text document: answered before its first element assign, handed to the host from there
    res, _ = ds.apply([text], [_blocks(HAND["text"])])
    assert (res["status"] == 0).all()
    got = ds.materialize_patch([text] * 3, [2, 3, 4])
    assert [a["action"] for a in got[0]["patch"]["diffs"]] == ["create", "set", "set", "set"]
    assert got[1] == {"doc": text, "history": 3, "patch": None, "host": True} and got[2]["patch"] is None and got[2]["host"] is True
    assert ds.materialize_patch([], []) == []
    with pytest.raises(EngineError):
        ds.materialize_patch([x, 9999], [1, 1])
