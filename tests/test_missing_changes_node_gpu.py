"""Backend.getMissingChanges / getChanges / getChangesForActor and GpuEngine.missingChanges of the
Node drop-in (GpuDocBackend.js over the docset's hm_docset_missing_changes) against Automerge 0.12's
rules restated in tests/js/run_missing_changes.js over oracle/js/backend.js's OpSet fed the same
chunks, after each of 3 rounds of a shuffled C2 feed; getChanges(old, new) with old a fork of the
document that stopped after the first chunk."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_change_queries_match_js_restatement(mode):
    from hypermerge_amd import synth
    from hypermerge_amd.columnar import decode_doc
    b = synth.generate(synth.config("C2", n_docs=40, arrival=2, shuffle_pct=30))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    rng = np.random.default_rng(5)
    chunked = []
    for chs in docs:
        cuts = sorted(int(x) for x in rng.integers(1, len(chs) + 1, size=2))
        chunked.append([chs[:cuts[0]], chs[cuts[0]:cuts[1]], chs[cuts[1]:]])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_missing_changes.js")],
                       input=json.dumps({"docs": chunked, "mode": mode}), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["nMismatches"] == 0, got["mismatches"]
    assert len(got["rounds"]) == 3
    for r in got["rounds"]:
        assert r["compared"] == 5 * len(docs) and r["nonEmpty"] >= len(docs)
    # most documents went on after the fork stopped: getChanges had something to return
    assert got["forks"] >= len(docs) // 2
