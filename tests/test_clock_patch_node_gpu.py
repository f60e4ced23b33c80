"""DocBackend.materializePatchAt({ clock }) and GpuEngine.materializePatch([{ state | id, clock }]) of
the Node drop-in (hm_docset_materialize_patch_at under them) against oracle/js/backend.js: one
applyChanges call on init() with the changes the clock selects; history, queued, clock, deps and
diffs deep-equal for prefix, causal-past and cut clocks of text, list and map documents fed in
rounds; a prefix's clock gives the history-length call's patch byte for byte
(tests/js/run_clock_patch_at.js)."""
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
def test_materialize_patch_at_a_clock_equals_js_backend(mode):
    from hypermerge_amd import synth
    from hypermerge_amd.columnar import decode_doc
    from list_diffs_cases import LHAND
    from op_diffs_cases import HAND, chain_doc
    b5 = synth.generate(synth.config("C5", n_docs=12))
    docs = [decode_doc(b5, i) for i in range(b5.n_docs)]
    b3 = synth.generate(synth.config("C3", n_docs=2, changes_per_actor=40))
    docs += [decode_doc(b3, i) for i in range(b3.n_docs)]
    b2 = synth.generate(synth.config("C2", n_docs=4, counter_pct=20))
    docs += [decode_doc(b2, i) for i in range(b2.n_docs)]
    docs += [HAND[k] for k in sorted(HAND)] + [LHAND[k][0] for k in sorted(LHAND)] + [chain_doc(30, 3)]
    rng = np.random.default_rng(17)
    chunked = []
    for chs in docs:
        cuts = sorted(int(x) for x in rng.integers(1, len(chs) + 1, size=2))
        chunked.append([chs[:cuts[0]], chs[cuts[0]:cuts[1]], chs[cuts[1]:]])
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_clock_patch_at.js")],
                       input=json.dumps({"docs": chunked, "mode": mode}), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["docs"] == len(docs) and got["checked"] > 8 * len(docs)
    assert got["mismatches"] == []
    assert got["prefixes"] > 2 * len(docs) and got["prefixMismatches"] == 0
    assert got["closed"] >= 10 and got["queued"] >= 10, got                   # (clocks that are no prefix, of both kinds)
    assert got["elementDiffs"] > 500
    assert got["plainMismatches"] == 0
    assert got["single"] == 8 and got["unknown"] is True
