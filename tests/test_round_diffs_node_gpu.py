"""GpuDocBackend with GpuEngine({diffs: 'device'}): a C2 feed and a C5 feed (shuffled arrival, so rounds
apply nothing or apply earlier-queued changes) through the Node drop-in, in sync and in async mode.
Every delivered message's patch equals the JS restatement's (oracle/js/backend.js) for the same
documents fed in the same chunks; the rounds were rendered from device rows, nothing was replayed."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import decode_doc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.gpu


def chunked_feed(name, n, shuffled):
    b = synth.generate(synth.config(name, n_docs=n))
    rng = np.random.default_rng(31)
    out = []
    for i in range(b.n_docs):
        chs = list(decode_doc(b, i))
        if shuffled:
            rng.shuffle(chs)
        cuts = sorted(rng.integers(1, len(chs) + 1, size=3))
        out.append([chs[:cuts[0]], chs[cuts[0]:cuts[1]], chs[cuts[1]:cuts[2]], chs[cuts[2]:]])
    return out


@pytest.fixture(scope="module")
def feeds():
    return [chunked_feed("C2", 40, False), chunked_feed("C5", 40, True)]


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_patch_sequences_equal_the_js_restatement(feeds, mode):
    assert NODE is not None, "node is needed for the Node drop-in"
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_round_diffs.js")], input=json.dumps({"feeds": feeds, "mode": mode}),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout)["feeds"]
    assert len(got) == 2
    for f, feed in enumerate(got):
        st = feed["stats"]
        assert feed["diffs"] == "device"
        assert st["deviceRounds"] > 0 and st["diffCalls"] > 0 and st["diffCallsRepeated"] <= st["diffCalls"]
        assert st["opPatches"] == 0 and st["replayMismatch"] == 0 and st["hitPatches"] == 0 and st["fullPatches"] == 0
        n_diffs = n_list = 0
        for i, d in enumerate(feed["docs"]):
            assert len(d["gpu"]) == len(d["cpu"]) > 0, (f, i)
            for k, (g, c) in enumerate(zip(d["gpu"], d["cpu"])):
                assert g == c, (f, i, k)
                diffs = c.get("patch", {}).get("diffs", [])
                n_diffs += len(diffs)
                n_list += sum(1 for x in diffs if "index" in x)
        assert n_diffs > 0 and (f == 0 or n_list > 0)
