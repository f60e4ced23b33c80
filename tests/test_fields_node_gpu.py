"""Local undo / redo through the Node drop-in with undo: 'fields' (the undo ops built from
hm_docset_fields' answer for the fields a request touches) against the JS restatement
(oracle/js/backend.js) fed the same steps by tests/js/run_fields_undo.js: the same messages, canUndo /
canRedo, throws, documents and undo / redo stacks after every step, on feeds where a remote set lands
between a request's construction and its application on a field the request touches twice, where an
inc meets a concurrent counter set, and where a request is not causally ready."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


@pytest.mark.parametrize("mode", ["sync", "batched", "async"])
def test_exact_undo_matches_restatement(mode):
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_fields_undo.js"), mode, "24"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(got["gpu"]) == len(got["cpu"]) == 24
    undos = redos = throws = 0
    for d, (g, c) in enumerate(zip(got["gpu"], got["cpu"])):
        for step, (gs, cs) in enumerate(zip(g["trace"], c["trace"])):
            assert gs == cs, (d, step)
        assert len(g["trace"]) == len(c["trace"]) and g["msgs"] == c["msgs"], d
        throws += sum(1 for t in c["trace"] if t[1] is not None)
        undos += sum(1 for m in c["msgs"] if m[0] == "LocalPatchMsg" and m[3])
        redos += sum(1 for m in c["msgs"] if m[0] == "LocalPatchMsg" and m[2])
    assert throws > 0 and undos > 0 and redos > 0, (throws, undos, redos)
    # the inputs reach the cases the default route gets wrong
    assert got["counts"]["retouchedUncovered"] > 0 and got["counts"]["notReady"] > 0, got["counts"]
