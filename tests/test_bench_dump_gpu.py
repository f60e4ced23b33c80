"""bench.py --dump-outputs: a plain run writes what its last timed step computed, for a seeded
sample of documents, and those arrays are the oracle's results for the same synthetic shard."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = 6000          # above the sample size: the sampled path, several workgroups


@pytest.mark.gpu
def test_dump_outputs_are_the_last_steps_results(tmp_path):
    from hypermerge_amd import synth
    import oracle.oracle as O
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert DOCS > bench.DUMP_DOCS
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--docs", str(DOCS), "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "changes/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    assert line["full"] is False and "roofline" not in line and "legs" not in line
    assert line["dump_outputs"]["docs"] == bench.DUMP_DOCS and line["dump_outputs"]["of"] == DOCS
    assert sorted(os.listdir(tmp_path)) == ["dump"]           # a plain run writes nothing else

    b = synth.generate(synth.config("C4", n_docs=DOCS, shard=0, n_shards=1))
    o = O.merge(b)
    S, d = b.a_stride, b.docs
    sel = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(DOCS, bench.DUMP_DOCS, replace=False))
    ci = bench._ranges(d["change_off"][sel], d["n_changes"][sel])
    want = {"docs": o.docs[sel], "clock": o.clock.reshape(-1, S)[sel], "back_clock": o.back_clock.reshape(-1, S)[sel],
            "heads": o.heads.reshape(-1, S)[sel], "hist": o.hist[ci], "all_deps": o.all_deps.reshape(-1, S)[ci],
            "regs": o.regs[bench._ranges(d["reg_off"][sel], d["n_regs"][sel])],
            "surv": o.surv[bench._ranges(d["op_off"][sel], o.docs["n_surv"][sel])]}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in want)
    total = 0
    for n, w in want.items():
        got = np.load(out / (n + ".npy"))
        total += got.nbytes
        assert got.dtype == np.float64 and len(got) == len(w) > 0, n
        assert np.array_equal(got, bench._as_f64(w)), n
    assert total <= 64 << 20 and total == line["dump_outputs"]["bytes"]
