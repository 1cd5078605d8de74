"""bench.py without --full (the headline steps only) and its --dump-outputs files: two runs with the same arguments
write the same arrays, and the visit counters in them are the CPU oracle's for every launch since reset()."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

B, SIZE, LAUNCH, STEPS, WARMUP = 2048, 30, 600, 3, 1
NAMES = ("state", "step_in_episode", "episodes", "sample_instances", "visits_s", "visits_sa")


def _bench(out_dir):
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--instances", str(B), "--size", str(SIZE), "--launch-steps", str(LAUNCH),
           "--steps", str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_run_dumps_what_the_timed_steps_computed(need_gpu, tmp_path):
    from colosseum_amd.mdp.fast_batch import deepsea_episodic_tables
    from oracle import oracle as O

    lines = [_bench(tmp_path / "a"), _bench(tmp_path / "b")]
    for line in lines:
        assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0 and line["value"] > 0
        for k in ("metric", "unit", "higher_is_better", "dtype", "roofline"):
            assert k in line, k
        assert not {"vi", "dense", "cpu_baseline", "sustained", "strong"} & set(line)
    files = sorted(n + ".npy" for n in NAMES)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == files
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    out = {}
    for n in NAMES:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, b), n
        out[n] = a
    # B is below the sample size: every instance is in the sample, in order
    assert np.array_equal(out["sample_instances"], np.arange(B))
    seeds = np.arange(B)
    tables = deepsea_episodic_tables(seeds, SIZE, with_dp=False)
    S = out["visits_s"].shape[1]
    start = int(tables["start_state"][0])
    assert np.array_equal(out["episodes"], out["visits_s"][:, start])
    n, n_steps = 256, LAUNCH * (lines[0]["config"]["settle_launches"] + WARMUP + STEPS)
    _, _, ovs, ovsa = O.batch_rollout(tables, 0, n, n_steps, rng_mode=1, philox_keys=seeds.astype(np.uint64), want_visits=True)
    assert np.array_equal(out["visits_s"][:n], ovs.reshape(n, S))
    assert np.array_equal(out["visits_sa"][:n], ovsa.reshape(n, -1))
