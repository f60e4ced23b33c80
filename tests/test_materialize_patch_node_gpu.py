"""DocBackend.materializePatchAt(n) and GpuEngine.materializePatch of the Node drop-in
(hm_docset_materialize_patch under them) against oracle/js/backend.js
applyChanges(init(), history.slice(0, n)): clock, deps and diffs deep-equal at every history length
of seeded map and counter documents, fed in rounds, arrival order and shuffled; the list documents
come back with patch: null once a prefix assigns an element (tests/js/run_materialize_patch.js)."""
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
def test_materialize_patch_at_equals_js_backend(mode):
    from hypermerge_amd import synth
    from hypermerge_amd.columnar import decode_doc
    from op_diffs_cases import HAND, chain_doc, one_register_doc
    b = synth.generate(synth.config("C2", n_docs=16, counter_pct=20))
    docs = [decode_doc(b, i) for i in range(b.n_docs)]
    b = synth.generate(synth.config("C2", n_docs=8, arrival=2, shuffle_pct=30))
    docs += [decode_doc(b, i) for i in range(b.n_docs)]
    b5 = synth.generate(synth.config("C5", n_docs=6))            # nested maps and lists
    docs += [decode_doc(b5, i) for i in range(b5.n_docs)]
    docs += [HAND[k] for k in sorted(HAND)] + [chain_doc(30, 3), one_register_doc(40)]
    rng = np.random.default_rng(12)
    chunked = []
    for chs in docs:
        cuts = sorted(int(x) for x in rng.integers(1, len(chs) + 1, size=2))
        chunked.append([chs[:cuts[0]], chs[cuts[0]:cuts[1]], chs[cuts[1]:]])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_materialize_patch.js")],
                       input=json.dumps({"docs": chunked, "mode": mode}), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["before"] is True
    assert got["docs"] == len(docs) and got["checked"] > 5 * len(docs)
    assert got["mismatches"] == []
    assert 0 < got["nulls"] < got["checked"] // 2                # the list documents, and only past their first element assign
    assert got["single"] == 8
