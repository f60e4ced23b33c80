"""Backend.getPatch(state), GpuEngine.getPatches(states) and GpuEngine.views(states) of the Node drop-in
(hm_docset_get_patch / hm_docset_views under them) against the route they replace, restated in
tests/js/run_state_patch.js from addon.docsetView: map, counter, table, list and text documents fed
in rounds, on one shard and across two; a frontend that applies the patch to an empty document
arrives at the document of materializeAt(history)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def documents():
    from hypermerge_amd import synth
    from hypermerge_amd.columnar import decode_doc
    from fuzz_docs import gen_doc
    from state_cases import KNOWN
    docs = []
    for name, n, over in (("C4", 6, {}), ("C2", 4, {"counter_pct": 30}), ("C3", 2, {"changes_per_actor": 30}), ("C5", 6, {})):
        b = synth.generate(synth.config(name, n_docs=n, **over))
        docs += [decode_doc(b, i) for i in range(b.n_docs)]
    docs += [gen_doc(900 + i, profile="default") for i in range(12)]     # tables, counters on elements, several lists
    docs += [gen_doc(950, n_actors=11, profile="wide")]                  # a second stride class
    docs += [KNOWN[k][0] for k in sorted(KNOWN) if KNOWN[k][0]]
    rng = np.random.default_rng(23)
    chunked = []
    for chs in docs:
        cuts = sorted(int(x) for x in rng.integers(1, len(chs) + 1, size=2))
        chunked.append([chs[:cuts[0]], chs[cuts[0]:cuts[1]], chs[cuts[1]:]])
    return chunked


@pytest.mark.parametrize("devices", [[0], [0, 0]])
def test_get_patch_equals_the_view_route(devices):
    chunked = documents()
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_state_patch.js"), json.dumps(devices)],
                       input=json.dumps({"docs": chunked}), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["docs"] == len(chunked) + 1 and got["shards"] == len(devices)
    assert got["mismatches"] == [] and got["manyMismatches"] == [] and got["viewMismatches"] == []
    assert got["frontendMismatches"] == []
    # (what the documents hold: every kind of diff entry the patch can carry went through the comparison)
    assert got["diffs"] > 500 and got["inserts"] > 100 and got["conflicts"] > 5 and got["counters"] > 0 and got["tables"] > 0, got
