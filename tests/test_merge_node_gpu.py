"""Repo.merge into a document that already holds changes, through DocBackend.mergeFrom of the Node drop-in
(tests/js/run_repo_merge.js): the reference's "Test document merging" scenario (tests/golden/repo_scenarios.json
"merge": {foo: 'bar'}, then {foo: 'bar', baz: 'bah'}; a later change of the source does not reach the
destination), and a conflicting key on both sides against the JS restatement, message for message — on the
device (one docset) and through the host hand-over (source and destination on different shards)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


@pytest.mark.parametrize("mode,diffs,shards", [("sync", "ops", 1), ("batched", "ops", 1), ("async", "ops", 1), ("sync", "device", 1),
                                               ("async", "device", 1), ("batched", "ops", 2)])
def test_repo_merge_scenario_and_a_conflicting_key(mode, diffs, shards):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "repo_scenarios.json")))["scenarios"]["merge"]
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_repo_merge.js"), mode, diffs, str(shards)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    for key, want in gold["renders"].items():
        assert got["renders"][key] == want, (key, got["renders"][key])
    assert got["renders"]["R/D1"] == [{"foo": "bar"}, {"foo": "bar", "baz": "bah"}]
    assert got["messages"]["R/D1"] == ["ReadyMsg", "LocalPatchMsg", "RemotePatchMsg"]
    assert got["messages"]["R/D2"] == ["ReadyMsg", "LocalPatchMsg", "LocalPatchMsg"]
    assert got["d1Clock"] == {"D1": 1, "D2": 1} and got["d1History"] == 2 and got["d1Log"] == 2
    assert got["mismatches"] == [], json.dumps(got["mismatches"])[:3000]
    assert got["crossShard"] == (1 if shards == 2 else 0)
