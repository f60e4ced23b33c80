"""DocBackend.initFrom / GpuEngine.fork of the Node drop-in (hypermerge_amd/js) against the JS restatement
(oracle/js/backend.js): a fork made on the device must be, message for message, init(changes, actorId)
with the changes Repo.merge hands a new document for the clock — each listed actor's changes
1 .. clock[actor] in the clock's key order (tests/js/run_fork.js).  Map documents, text documents and
the full-vocabulary generator's documents, whose cut clocks leave queued changes behind; every route:
sync, batched and 'async', and diffs: 'device'."""
import json
import os
import shutil
import subprocess

import pytest

from fuzz_docs import gen_docs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def documents():
    from hypermerge_amd import synth
    from hypermerge_amd.columnar import decode_doc
    docs = []
    for name, n in (("C2", 12), ("C3", 3), ("C5", 12)):
        b = synth.generate(synth.config(name, n_docs=n))
        docs += [decode_doc(b, i) for i in range(b.n_docs)]
    return docs + gen_docs("default", range(9100, 9116))


@pytest.mark.parametrize("mode,diffs", [("sync", "ops"), ("batched", "ops"), ("async", "ops"), ("batched", "device"),
                                        ("async", "device")])
def test_init_from_equals_init_with_the_handed_changes(mode, diffs):
    docs = documents()
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_fork.js")],
                       input=json.dumps({"docs": docs, "mode": mode, "diffs": diffs}), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["docs"] == len(docs)
    assert got["mismatches"] == [], json.dumps(got["mismatches"])[:3000]
    assert got["queued"] > 0                                     # forks whose clock is not causally closed
    assert got["reordered"] > 5                                  # the hand-over order is not the parent's history order


@pytest.mark.parametrize("mode,diffs", [("sync", "ops"), ("batched", "ops"), ("async", "ops"), ("sync", "device")])
def test_repo_fork_scenario_with_the_fork_made_on_the_device(mode, diffs):
    """tests/repo.test.ts:103-127 (tests/golden/repo_scenarios.json "fork": create(), merge(fork, parent), a
    change on the fork) with the merge into the still empty document made by GpuEngine.fork
    (DocBackend.mergeFrom) instead of re-feeding the parent's blocks: the watched documents render exactly
    what the reference test expects, with the reference's message types."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "repo_scenarios.json")))["scenarios"]["fork"]
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_repo_fork.js"), mode, diffs],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["forks"] == 1
    for key, want in gold["renders"].items():
        assert got["renders"][key] == want, (key, got["renders"][key])
    assert got["messages"] == {"R/D1": ["ReadyMsg", "LocalPatchMsg"], "R/F": ["ReadyMsg", "RemotePatchMsg", "LocalPatchMsg"]}
    assert got["forkClock"] == {"D1": 1, "F": 1} and got["forkHistory"] == 2 and got["forkLog"] == 2
