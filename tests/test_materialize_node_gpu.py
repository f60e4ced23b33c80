"""DocBackend.materializeAt(n) and GpuEngine.materialize of the Node drop-in (hm_docset_materialize under
them): the reference's tests/repo.test.ts:129-164 document at every n, and seeded documents with
lists and counters against oracle/js/backend.js, document for document (tests/js/run_materialize_at.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


@pytest.mark.parametrize("mode", ["batched", "async"])
def test_materialize_at_equals_js_backend(mode):
    from hypermerge_amd import synth
    from hypermerge_amd.columnar import decode_doc
    b = synth.generate(synth.config("C2", n_docs=24, counter_pct=20))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    b5 = synth.generate(synth.config("C5", n_docs=24))          # nested maps and lists, queued and duplicate changes
    docs += [decode_doc(b5, i) for i in range(b5.n_docs)]
    ops = {o["action"] for c in docs for ch in [c] for x in ch for o in x["ops"]}
    assert {"ins", "inc", "makeList"} <= ops or {"ins", "inc", "makeText"} <= ops, ops
    rng = np.random.default_rng(12)
    chunked = []
    for chs in docs:
        cuts = sorted(int(x) for x in rng.integers(1, len(chs) + 1, size=2))
        chunked.append([chs[:cuts[0]], chs[cuts[0]:cuts[1]], chs[cuts[1]:]])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_materialize_at.js")],
                       input=json.dumps({"docs": chunked, "mode": mode}), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    # the reference's materialize test: foo = bar0, bar1, bar2, bar3; n clamps as slice does
    sc = got["scenario"]
    assert sc["before"] is True
    assert sc["0"] == {"doc": {}, "history": 0, "clock": {}}
    for n in (1, 2, 3, 4):
        assert sc[str(n)] == {"doc": {"foo": "bar%d" % (n - 1)}, "history": n, "clock": {"aaaaaaaa": n}}, n
    assert sc["5"] == sc["4"]
    assert got["docs"] == len(docs) and got["checked"] > 10 * len(docs)
    assert got["mismatches"] == []
    assert got["single"] == 8
