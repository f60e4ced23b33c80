"""getMissingDeps / opSet.queue / engine.blocked() of the Node drop-in (GpuDocBackend.js over the
docset's hm_docset_blocked / hm_docset_waiting) against the values restated from
oracle/js/backend.js on the same chunks, after each of 3 rounds of a shuffled C2 feed."""
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
def test_missing_deps_queue_and_blocked_match_js_restatement(mode):
    from hypermerge_amd import synth
    from hypermerge_amd.columnar import decode_doc
    b = synth.generate(synth.config("C2", n_docs=120, arrival=2, shuffle_pct=30))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    rng = np.random.default_rng(5)
    chunked = []
    for chs in docs:
        cuts = sorted(int(x) for x in rng.integers(1, len(chs) + 1, size=2))
        chunked.append([chs[:cuts[0]], chs[cuts[0]:cuts[1]], chs[cuts[1]:]])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_waiting.js")],
                       input=json.dumps({"docs": chunked, "mode": mode}), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["nMismatches"] == 0, got["mismatches"]
    assert len(got["rounds"]) == 3
    for r in got["rounds"]:
        assert r["blocked"] == r["nonEmpty"]
    # documents with a non-empty queue were compared (the shuffled feed blocks many mid-way), and
    # the whole feed leaves none blocked
    assert max(r["nonEmpty"] for r in got["rounds"]) >= 12
    assert got["rounds"][-1]["blocked"] == 0
