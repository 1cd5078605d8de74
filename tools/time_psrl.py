"""Times the device PSRL agent (K12, BatchedPSRLEpisodic, Philox sampler) against what the library offered before it: a
Python loop of BatchedMDP.step + the NumPy twin's bookkeeping and sampling (tests/helpers_psrl.py) +
dynamic_programming.episodic_value_iteration per instance, on the same batch.

    python tools/time_psrl.py [--out profiles] [--batch all|frozenlake20|small] [--episodes N] [--reps 2]

Philox environments.  Both sides run over the SAME window, the first --episodes episodes per instance (creation, with its
solve on the prior, included), --reps times on fresh batches after a warm-up on the timed shape; both values are printed.
The host loop costs S * A * S numpy gammas and one solve per instance and episode, so on the large batch it is run on the
first --baseline-instances instances of the batch only and its rate is per instance-step all the same (stated in the
JSON).  Also reported: the kernels' share of a round from CMDP_STAT_PSRL_* (HIP-event time of the last round's k_psrl_sample
and k_vi_episodic_dense against the wall time per round).  No ratio is asserted anywhere.  JSON goes to
--out/k12_psrl.json, one entry per batch."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from colosseum_amd import _lib as L  # noqa: E402
from colosseum_amd import dynamic_programming as dp  # noqa: E402
from colosseum_amd.agents import BatchedPSRLEpisodic  # noqa: E402
from colosseum_amd.batched import BatchedMDP  # noqa: E402
from colosseum_amd.mdp import make_model  # noqa: E402
from helpers_psrl import PSRLTwin  # noqa: E402

BATCHES = {
    "frozenlake20": ("FrozenLakeEpisodic", dict(size=20, p_frozen=0.9, p_rand=0.1), 1000),
    "small": ("FrozenLakeEpisodic", dict(size=4, p_frozen=0.9, p_rand=0.1), 16),
}


def make_env(name, B=None, n_models=1):   # one model: instances of a batch share the horizon, which depends on the seed
    fam, kw, full = BATCHES[name]
    B = full if B is None else min(B, full)
    base = [make_model(fam, seed=s, **kw) for s in range(min(n_models, B))]
    env = BatchedMDP([base[b % len(base)] for b in range(B)], rng_mode=L.RNG_PHILOX,
                     philox_keys=np.arange(B, dtype=np.uint64) * 7919 + 5)
    env.reset()
    return env


def device_run(name, episodes):
    env = make_env(name)
    t = time.perf_counter()
    agent = BatchedPSRLEpisodic(env, np.arange(env.B), 10 ** 6, sampler="philox")
    create_s = time.perf_counter() - t
    first = agent.stats()
    t = time.perf_counter()
    agent.run(episodes * env.H)
    run_s = time.perf_counter() - t
    st = agent.stats()
    total = create_s + run_s
    r = dict(B=env.B, S=int(env.n_states[0]), A=env.A, H=env.H, episodes=episodes, create_s=create_s, run_s=run_s,
             steps_per_s=env.B * episodes * env.H / total, rounds=st["rounds"], solves=st["solves"],
             wall_ms_per_round=1e3 * total / st["rounds"], first_round_sample_kernel_ms=first["sample_kernel_ms"],
             first_round_vi_kernel_ms=first["vi_kernel_ms"], last_round_sample_kernel_ms=st["sample_kernel_ms"],
             last_round_vi_kernel_ms=st["vi_kernel_ms"])
    r["kernels_share_of_a_round"] = (st["sample_kernel_ms"] + st["vi_kernel_ms"]) / r["wall_ms_per_round"]
    env.close()
    return r


def baseline_run(name, episodes, instances):
    """The parent commit's public API: step() per transition, the twin's bookkeeping and numpy sampling, one
    episodic_value_iteration per instance and episode."""
    env = make_env(name, B=instances)
    B, H = env.B, env.H
    t = time.perf_counter()
    twins = [PSRLTwin(b, int(env.n_states[b]), env.A, H, env.rewards_range[1],
                      lambda H_, T, R: dp.episodic_value_iteration(H_, np.ascontiguousarray(T), np.ascontiguousarray(R))[0])
             for b in range(B)]
    for tw in twins:
        tw.before_start_interacting()
    cur = env.state()[0].copy()
    for _ in range(episodes):
        for h in range(H):
            acts = np.array([twins[b].select_action(h, int(cur[b])) for b in range(B)], np.int32)
            obs, rew = env.step(acts)[:2]
            for b in range(B):
                twins[b].step_update(int(cur[b]), int(acts[b]), float(rew[b]), int(obs[b]), h == H - 1)
            cur = np.asarray(obs, np.int32).copy()
        for tw in twins:
            tw.episode_end_update()
        cur = env.reset().copy()
    run_s = time.perf_counter() - t
    env.close()
    return dict(instances=B, episodes=episodes, run_s=run_s, steps_per_s=B * episodes * H / run_s)


def time_batch(name, args):
    device_run(name, 1)   # warm-up on the timed shape
    devs = [device_run(name, args.episodes) for _ in range(args.reps)]
    res = dict(batch=name, window_episodes=args.episodes, sampler="philox", device=devs,
               device_steps_per_s=[d["steps_per_s"] for d in devs])
    if not args.device_only:
        bases = [baseline_run(name, args.episodes, args.baseline_instances) for _ in range(args.reps)]
        res.update(parent_api_loop=bases, parent_steps_per_s=[b["steps_per_s"] for b in bases],
                   parent_loop_note="run on the first --baseline-instances instances of the batch; its rate is per instance-step")
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--batch", default="all", choices=sorted(BATCHES) + ["all"])
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2, help="timed repetitions of each side, fresh batch each")
    ap.add_argument("--baseline-instances", type=int, default=8)
    ap.add_argument("--device-only", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    names = sorted(BATCHES, reverse=True) if args.batch == "all" else [args.batch]   # the small batch first
    res = {name: time_batch(name, args) for name in names}
    with open(os.path.join(args.out, "k12_psrl.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
