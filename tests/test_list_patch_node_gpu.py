"""DocBackend.materializePatchAt(n, { lists: true }) and GpuEngine.materializePatch(reqs, { lists:
true }) of the Node drop-in (hm_docset_materialize_patch_ex under them) against oracle/js/backend.js
applyChanges(init(), history.slice(0, n)): clock, deps and diffs, the list / text element diffs
included, deep-equal at every history length of text, list and map documents fed in rounds, and no
patch: null; without the option the same engine still hands the list prefixes back
(tests/js/run_list_patch.js)."""
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
def test_materialize_patch_at_with_lists_equals_js_backend(mode):
    from hypermerge_amd import synth
    from hypermerge_amd.columnar import decode_doc
    from list_diffs_cases import LHAND
    from op_diffs_cases import HAND, chain_doc
    b5 = synth.generate(synth.config("C5", n_docs=12))               # nested maps and lists, some changes early
    docs = [decode_doc(b5, i) for i in range(b5.n_docs)]
    b3 = synth.generate(synth.config("C3", n_docs=2, changes_per_actor=40))
    docs += [decode_doc(b3, i) for i in range(b3.n_docs)]
    b2 = synth.generate(synth.config("C2", n_docs=4, counter_pct=20))
    docs += [decode_doc(b2, i) for i in range(b2.n_docs)]
    docs += [HAND[k] for k in sorted(HAND)] + [LHAND[k][0] for k in sorted(LHAND)] + [chain_doc(30, 3)]
    rng = np.random.default_rng(14)
    chunked = []
    for chs in docs:
        cuts = sorted(int(x) for x in rng.integers(1, len(chs) + 1, size=2))
        chunked.append([chs[:cuts[0]], chs[cuts[0]:cuts[1]], chs[cuts[1]:]])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_list_patch.js")],
                       input=json.dumps({"docs": chunked, "mode": mode}), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["docs"] == len(docs) and got["checked"] > 5 * len(docs)
    assert got["mismatches"] == [] and got["nulls"] == 0
    assert got["elementDiffs"] > 1000
    assert got["plainMismatches"] == 0 and 0 < got["plainNulls"] < got["checked"]   # the count run_materialize_patch.js's rule gives
    assert got["single"] == 8
