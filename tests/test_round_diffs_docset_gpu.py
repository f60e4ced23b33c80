"""A docset that renders its rounds from the device's per-op diff rows (HM_DOCSET_DEVICE_DIFFS) next
to one that replays them on the host, on one engine and fed identically: after every call their
texts (the JSON's "p", "b", "c", or the HMP1 words) and result rows are equal, byte for byte.  The
per-call diffs of a one-change-per-call feed also equal the JS restatement's
(tests/js/run_op_diffs.js over oracle/js/backend.js)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from hypermerge_amd import synth
from hypermerge_amd.columnar import ROOT_ID as R
from hypermerge_amd.columnar import decode_doc
from hypermerge_amd.docset import DocSet
from hypermerge_amd.engine import EngineError

from list_diffs_cases import LHAND
from op_diffs_cases import HAND, chain_doc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.gpu

LONG = 620


def _blocks(changes):
    return [json.dumps(c, separators=(",", ":")).encode() for c in changes]


def documents():
    docs = [HAND[k] for k in sorted(HAND)] + [LHAND[k][0] for k in sorted(LHAND)]
    b5 = synth.generate(synth.config("C5", n_docs=10, arrival=2, shuffle_pct=40))
    docs += [decode_doc(b5, i) for i in range(b5.n_docs)]
    b3 = synth.generate(synth.config("C3", n_docs=2, changes_per_actor=40))
    docs += [decode_doc(b3, i) for i in range(b3.n_docs)]
    docs.append(chain_doc(LONG, 1))
    return docs


class Pair:
    """the replay docset and the device-diffs docset, fed the same calls"""

    def __init__(self, engine, binary=False):
        self.binary = binary
        self.replay, self.device = DocSet(engine, binary=binary), DocSet(engine, binary=binary, device_diffs=True)
        self.rounds = 0                                       # successful document rounds so far

    def open(self, n):
        first = self.replay.open(n)
        assert self.device.open(n) == first
        return first

    def apply(self, ids, blocks):
        ra, ta = self.replay.apply_raw(ids, blocks)
        rb, tb = self.device.apply_raw(ids, blocks)
        assert ta == tb, f"texts differ ({len(ta)} / {len(tb)} bytes)"
        assert ta[:4] == (b"HMP1" if self.binary else b'{"p"')
        assert ra.dtype == rb.dtype and all((ra[f] == rb[f]).all() for f in ra.dtype.names)
        self.rounds += int((ra["status"] == 0).sum())
        return ra, (None if self.binary else json.loads(ta.decode("utf-8", "surrogatepass")))

    def fails(self, ids, blocks):
        for ds in (self.replay, self.device):
            with pytest.raises(EngineError):
                ds.apply_raw(ids, blocks)

    def check_counters(self):
        a, b = self.replay.stats(), self.device.stats()
        assert a["op_patches"] == self.rounds and a["replay_mismatch"] == 0
        assert b["op_patches"] == 0 and b["replay_mismatch"] == 0 and b["hit_patches"] == 0 and b["full_patches"] == 0
        out = np.zeros(8, np.uint64)
        self.device.engine._check(self.device._L.hm_docset_stats(self.device._h, out.ctypes.data), "hm_docset_stats")
        assert int(out[5]) == int(out[6]) == int(out[7]) == 0                 # per-op replays, mismatches, checks skipped
        assert a["calls"] == b["calls"] and a["docs"] == b["docs"] and a["moves"] == b["moves"]
        assert self.replay.diff_stats() == {"rounds": 0, "calls": 0, "repeated": 0}
        d = self.device.diff_stats()
        assert d["rounds"] == self.rounds and d["calls"] >= d["repeated"]
        return d


def feed(pair, ids, parts):
    """parts[i] = document i's changes in calls; one call per step for every document that has one left.
    Returns per document the (history length, diffs | None) of each of its calls."""
    seen = [[] for _ in ids]
    for r in range(max(len(p) for p in parts)):
        sel = [i for i in range(len(ids)) if r < len(parts[i])]
        res, js = pair.apply([ids[i] for i in sel], [_blocks(parts[i][r]) for i in sel])
        assert (res["status"] == 0).all()
        for k, i in enumerate(sel):
            seen[i].append((int(res[k]["hist_len"]), None if js is None else js["p"][k]["diffs"]))
    return seen


def chunks_over_64_ops(changes):
    out, cur, ops = [], [], 0
    for c in changes:
        cur.append(c); ops += len(c["ops"])
        if ops > 64:
            out.append(cur); cur, ops = [], 0
    return out + ([cur] if cur else [])


def test_one_change_per_call_equals_the_replay_and_the_js_restatement(engine):
    assert NODE is not None, "node is needed for the JS restatement"
    docs = documents()
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "run_op_diffs.js")], input=json.dumps({"docs": docs}),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    js = json.loads(p.stdout.strip().splitlines()[-1])["docs"]
    pair = Pair(engine)
    first = pair.open(len(docs))
    ids = list(range(first, first + len(docs)))
    seen = feed(pair, ids, [[[c] for c in d] for d in docs])
    nothing = late = elements = 0
    for i, (got, j) in enumerate(zip(seen, js)):
        assert j["err"] is None and len(got) == len(j["calls"]) == len(docs[i])
        prev = 0
        for k, ((h, diffs), (jh, jd)) in enumerate(zip(got, j["calls"])):
            assert h == jh and diffs == jd, (i, k)
            nothing += h == prev
            late += h > prev + 1
            elements += sum(1 for x in diffs if "index" in x)
            prev = h
    assert nothing > 0 and late > 0 and elements > 100        # rounds that applied nothing / earlier-queued changes / list rows
    d = pair.check_counters()
    assert d["calls"] >= LONG                                 # one store call per class and call
    # the patch of a past state still comes from the same rows on the docset that keeps no replay state
    hl = [len(x) for x in docs]
    assert pair.device.materialize_patch(ids, hl, lists=True) == pair.replay.materialize_patch(ids, hl, lists=True)
    assert all(x["patch"] is not None for x in pair.device.materialize_patch(ids, hl, lists=True))


@pytest.mark.parametrize("binary", [False, True])
def test_chunks_of_more_than_64_ops_mixed_classes_and_a_ninth_actor(engine, binary):
    docs = documents()
    # a call mixing stride classes: twelve actors next to the narrow documents
    wide = [{"actor": f"w{i:02d}", "seq": 1, "deps": {}, "ops": [{"action": "set", "obj": R, "key": f"k{i % 3}", "value": i}]}
            for i in range(12)]
    wide.append({"actor": "w00", "seq": 2, "deps": {"w05": 1, "w11": 1}, "ops": [{"action": "del", "obj": R, "key": "k2"},
                                                                             {"action": "set", "obj": R, "key": "k1", "value": "w"}]})
    # a document that gains its ninth actor mid-feed (it moves to the 16-wide store), a list in it
    L = "11111111-2222-3333-4444-555555555555"
    grow = [{"actor": "g0", "seq": 1, "deps": {}, "ops": [{"action": "makeList", "obj": L}, {"action": "link", "obj": R, "key": "l", "value": L},
                                                         {"action": "ins", "obj": L, "key": "_head", "elem": 1},
                                                         {"action": "set", "obj": L, "key": "g0:1", "value": "a"}]}]
    grow += [{"actor": f"g{i}", "seq": 1, "deps": {"g0": 1}, "ops": [{"action": "set", "obj": L, "key": "g0:1", "value": i},
                                                                    {"action": "set", "obj": R, "key": "x", "value": i}]} for i in range(1, 8)]
    ninth = [{"actor": "g8", "seq": 1, "deps": {f"g{i}": 1 for i in range(8)},
              "ops": [{"action": "ins", "obj": L, "key": "g0:1", "elem": 2}, {"action": "set", "obj": L, "key": "g8:2", "value": "b"},
                      {"action": "set", "obj": R, "key": "x", "value": "all"}]},
             {"actor": "g3", "seq": 2, "deps": {}, "ops": [{"action": "del", "obj": L, "key": "g0:1"}, {"action": "inc", "obj": R, "key": "x", "value": 1}]}]
    pair = Pair(engine, binary)
    first = pair.open(len(docs) + 2)
    ids = list(range(first, first + len(docs) + 2))
    parts = [chunks_over_64_ops(d) for d in docs] + [[wide[:10], wide[10:]], [grow[:4], grow[4:], ninth[:1], ninth[1:]]]
    assert max(sum(len(c["ops"]) for c in call) for p in parts for call in p) > 64
    feed(pair, ids, parts)
    assert pair.replay.info(ids[-2])["a_stride"] == 16 and pair.device.info(ids[-1])["a_stride"] == 16
    assert pair.device.stats()["moves"] == 1
    pair.check_counters()
    for x in (ids[-1], ids[-2], ids[0]):
        assert pair.device.view(x) == pair.replay.view(x)


def test_a_guess_that_is_too_small_repeats_the_store_call_once(engine):
    """the survivor table is guessed at two survivors per handed op on a new docset: eight actors
    setting the same forty keys concurrently leave 1 + 2 + .. + 8 per key, the store reports the sizes
    and the call is repeated with them; the patch is the replay's and no failure is left behind"""
    conc = [{"actor": f"a{i}", "seq": 1, "deps": {}, "ops": [{"action": "set", "obj": R, "key": f"k{k}", "value": 10 * k + i} for k in range(40)]}
            for i in range(8)]
    pair = Pair(engine)
    d = pair.open(1)
    err = lambda: engine._L.hm_engine_last_error(engine._h)
    before = err()
    res, js = pair.apply([d], [_blocks(conc)])
    diffs = js["p"][0]["diffs"]
    assert len(diffs) == 320 and sum(1 + len(x.get("conflicts", [])) for x in diffs) == 40 * 36 > 2 * 320 + 64
    assert pair.device.diff_stats() == {"rounds": 1, "calls": 2, "repeated": 1}
    assert err() == before                                    # the repeated call left no failure behind
    pair.check_counters()


def test_a_round_that_applies_a_long_queued_change(engine):
    """a one-op change lets a queued hundred-op change apply: the round's slice holds more ops than
    the round handed in (the guess counts the log of a document that holds queued changes)"""
    big = {"actor": "bb", "seq": 1, "deps": {"aa": 1}, "ops": [{"action": "set", "obj": R, "key": f"k{i}", "value": i} for i in range(100)]}
    small = {"actor": "aa", "seq": 1, "deps": {}, "ops": [{"action": "set", "obj": R, "key": "k0", "value": "first"}]}
    pair = Pair(engine)
    d = pair.open(1)
    res, js = pair.apply([d], [_blocks([big])])
    assert int(res[0]["hist_len"]) == 0 and int(res[0]["n_queued"]) == 1 and js["p"][0]["diffs"] == []
    assert pair.device.diff_stats() == {"rounds": 1, "calls": 0, "repeated": 0}   # (nothing applied: nothing asked)
    res, js = pair.apply([d], [_blocks([small])])
    assert int(res[0]["hist_len"]) == 2 and len(js["p"][0]["diffs"]) == 101
    assert pair.device.diff_stats() == {"rounds": 2, "calls": 1, "repeated": 0}
    pair.check_counters()


def test_failed_documents_and_failed_calls_roll_back_alike(engine, monkeypatch):
    docs = documents()[:6]
    pair = Pair(engine)
    first = pair.open(len(docs) + 2)
    ids = list(range(first, first + len(docs) + 2))
    half = [d[:len(d) // 2] for d in docs]
    ok = [{"actor": "o0", "seq": 1, "deps": {}, "ops": [{"action": "set", "obj": R, "key": "z", "value": 9}]}]
    throws = [{"actor": "b0", "seq": 1, "deps": {}, "ops": [{"action": "set", "obj": "no-such-object", "key": "k", "value": 2}]}]
    pair.apply(ids, [_blocks(h) for h in half] + [_blocks(ok), _blocks(ok)])
    # one document's block does not decode, one's merge throws: both roll back, the others are answered
    rest = [d[len(d) // 2:] for d in docs]
    res, js = pair.apply(ids, [_blocks(r) for r in rest] + [[b'{"actor": "x", oops'], _blocks(throws)])
    assert (res["status"][:-2] == 0).all() and res["status"][-2] == 32 and res["status"][-1] not in (0, 32)
    assert js["p"][-2] is None and js["p"][-1] is None and all(p is not None for p in js["p"][:-2])
    for ds in (pair.replay, pair.device):
        assert ds.info(ids[-1])["n_changes"] == 1 and ds.info(ids[-2])["n_changes"] == 1
    # a failed call is undone on both; the same round then applies cleanly on both
    nxt = [{"actor": "o0", "seq": 2, "deps": {}, "ops": [{"action": "set", "obj": R, "key": "z", "value": 10},
                                                        {"action": "set", "obj": R, "key": "y", "value": 1}]}]
    for where in ("read", "wait:0"):
        info0 = [pair.device.info(x) for x in ids]
        stats0 = pair.device.diff_stats()
        monkeypatch.setenv("HM_DOCSET_INJECT_FAIL", where)
        pair.fails(ids[-2:], [_blocks(nxt), _blocks(nxt)])
        monkeypatch.delenv("HM_DOCSET_INJECT_FAIL")
        assert [pair.device.info(x) for x in ids] == info0 and pair.device.diff_stats() == stats0
    res, js = pair.apply(ids[-2:], [_blocks(nxt), _blocks(nxt)])
    assert (res["status"] == 0).all() and len(js["p"][0]["diffs"]) == 2
    pair.check_counters()
    for x in ids:
        assert pair.device.view(x) == pair.replay.view(x)


def test_the_refused_flag_combinations(engine):
    for kw in ({"net_diffs": True}, {"patches": False}, {"net_diffs": True, "patches": False}):
        with pytest.raises(EngineError, match="HM_DOCSET_DEVICE_DIFFS"):
            DocSet(engine, device_diffs=True, **kw)
    DocSet(engine, device_diffs=True, binary=True).close()
