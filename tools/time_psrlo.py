"""Times the continuous PSRL agent with optimistic sampling (K18, BatchedPSRLContinuousOptimistic) next to the plain agent (K13,
BatchedPSRLContinuous) on the same batches, both with the Philox sampler (--sampler).

    python tools/time_psrlo.py [--out profiles] [--batch all|frozenlake5|frozenlake10] [--reps 4] [--steps 150] [--host-steps 10]

Per batch and agent: creation (the solve on the prior, warm-up), then --reps rounds of episode_end_update(), each on a fresh
sample of the same tables: HIP-event times of the round's sample kernel (k_psrlo_sample / k_psrl_sample) and solve kernel
(k_vi_discounted_dense), the round's summed sweeps, the host time of the reference sampler's draws.  Then --steps steps of
run() on a fresh equal batch, in chunks, wall time ending in each call's synchronisation (--max-seconds, off by default, stops
it after the chunk that passes it; the steps taken are recorded).  The host route -- BatchedMDP.step, the NumPy twin of tests/helpers_psrlo.py and
discounted_value_iteration_dense_batch per solve -- on the first 8 instances for --host-steps steps (0: the eight solves on
the prior alone; solves per second are recorded next to steps per second).  The reference's own
steps per second come from golden G23's metadata.  No ratio is asserted.  JSON goes to --out/k18_psrlo.json."""
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
from colosseum_amd.agents import BatchedPSRLContinuous, BatchedPSRLContinuousOptimistic  # noqa: E402
from colosseum_amd.batched import BatchedMDP  # noqa: E402
from colosseum_amd.mdp import make_model  # noqa: E402

BATCHES = {"frozenlake5": (5, 256), "frozenlake10": (10, 64)}   # FrozenLakeContinuous size -> instances
COMPACT_ONLY = {"frozenlake20": (20, 64)}                       # --sample-solver: the compact route alone
HORIZON = 10 ** 6


def make_env(name, B=None):
    size, n = {**BATCHES, **COMPACT_ONLY}[name]
    B = B or n
    base = [make_model("FrozenLakeContinuous", seed=s, size=size, p_frozen=0.9) for s in range(4)]
    env = BatchedMDP([base[b % 4] for b in range(B)], rng_mode=L.RNG_PHILOX, philox_keys=np.arange(B, dtype=np.uint64) * 7919 + 5)
    env.reset()
    return env


def make_agent(env, kind, sampler):
    if kind == "optimistic":
        return BatchedPSRLContinuousOptimistic(env, np.arange(env.B), HORIZON, sampler=sampler)
    return BatchedPSRLContinuous(env, np.arange(env.B), HORIZON, sampler=sampler, no_optimistic_sampling=True)


def time_agent(name, kind, args):
    env = make_env(name)
    agent = make_agent(env, kind, args.sampler)
    res = dict(B=env.B, S=[int(s) for s in sorted(set(env.n_states.tolist()))], A=env.A, sampler=args.sampler)
    if kind == "optimistic":
        res.update(psi=sorted(set(agent.psi.tolist())), eta=sorted(set(agent.eta.tolist())),
                   T_ext_bytes=int(sum(int(S) * env.A * int(k) * int(S) * 4 for S, k in zip(env.n_states, agent.psi))))
    else:
        res.update(T_bytes=int(sum(int(S) * env.A * int(S) * 4 for S in env.n_states)))
    agent.episode_end_update()   # warm-up
    rounds, ref0 = [], agent.stats()["reference_ms"]
    for _ in range(args.reps):
        agent.episode_end_update()
        st = agent.stats()
        rounds.append(dict(sample_kernel_ms=st["sample_kernel_ms"], vi_kernel_ms=st["vi_kernel_ms"], sweeps=st["sweeps"],
                           reference_ms=st["reference_ms"] - ref0))
        ref0 = st["reference_ms"]
    env.close()
    env = make_env(name)
    agent = make_agent(env, kind, args.sampler)
    taken, t0 = 0, time.perf_counter()
    while taken < args.steps and (args.max_seconds <= 0 or time.perf_counter() - t0 < args.max_seconds):
        n = min(args.chunk, args.steps - taken)
        agent.run(n)
        taken += n
    run_s = time.perf_counter() - t0
    st = agent.stats()
    res.update(rounds=rounds, vi_kernel_ms_median=float(np.median([r["vi_kernel_ms"] for r in rounds])),
               sample_kernel_ms_median=float(np.median([r["sample_kernel_ms"] for r in rounds])), run_steps=taken, run_s=run_s,
               steps_per_s=env.B * taken / run_s, run_rounds=st["rounds"] - 1, run_solves=st["solves"] - env.B,
               run_reference_ms=st["reference_ms"])
    env.close()
    return res


def time_sample_routes(name, routes, args):
    """The optimistic agent's sample routes on one batch: alternated rounds, then a timed run() per route."""
    envs = {r: make_env(name) for r in routes}
    agents = {r: BatchedPSRLContinuousOptimistic(envs[r], np.arange(envs[r].B), HORIZON, sampler=args.sampler, sample_solver=r)
              for r in routes}   # creation: the solve on the prior, warm-up
    env = envs[routes[0]]
    res = dict(B=env.B, S=[int(s) for s in sorted(set(env.n_states.tolist()))], A=env.A, sampler=args.sampler,
               psi=sorted(set(agents[routes[0]].psi.tolist())),
               T_ext_bytes=int(sum(int(S) * env.A * int(k) * int(S) * 4 for S, k in zip(env.n_states, agents[routes[0]].psi))),
               routes={r: dict(rounds=[]) for r in routes})
    for _ in range(args.reps):
        for r in routes:
            agents[r].episode_end_update()
            st = agents[r].stats()
            assert st["sample_solver"] == r and st["unconverged"] == 0
            res["routes"][r]["rounds"].append(dict(sample_kernel_ms=st["sample_kernel_ms"], vi_kernel_ms=st["vi_kernel_ms"],
                                                   sweeps=st["sweeps"]))
    for r in routes:
        out = res["routes"][r]
        scheme = np.zeros(env.B, np.int32)   # of the last solves, without fetching the samples
        L.check(L.load().cmdp_psrlc_last_sample_optimistic(agents[r]._h, *([None] * 7), L.ptr(scheme), None))
        out.update(sample_bytes=agents[r].stats()["sample_bytes"], scheme=sorted(set(scheme.tolist())),
                   vi_kernel_ms_median=float(np.median([x["vi_kernel_ms"] for x in out["rounds"]])),
                   sample_kernel_ms_median=float(np.median([x["sample_kernel_ms"] for x in out["rounds"]])))
        envs[r].close()
    for r in routes:
        env = make_env(name)
        agent = BatchedPSRLContinuousOptimistic(env, np.arange(env.B), HORIZON, sampler=args.sampler, sample_solver=r)
        chunk = args.chunk if r == "compact" else max(1, args.chunk // 5)   # a dense round of the larger shape takes seconds
        taken, t0 = 0, time.perf_counter()
        while taken < args.steps and (args.max_seconds <= 0 or time.perf_counter() - t0 < args.max_seconds):
            n = min(chunk, args.steps - taken)
            agent.run(n)
            taken += n
        run_s = time.perf_counter() - t0
        st = agent.stats()
        res["routes"][r].update(run_steps=taken, run_s=run_s, steps_per_s=env.B * taken / run_s, run_rounds=st["rounds"] - 1,
                                run_solves=st["solves"] - env.B, sample_bytes_after_run=st["sample_bytes"])
        env.close()
    return res


def time_host_route(name, args):
    """The same agent with the model, the sample and the actor on the host: one device call per step and per solve."""
    from helpers_psrlo import PSRLOTwin
    from colosseum_amd.agents import optimistic_sampling_scalars

    B = 8
    env = make_env(name, B)
    twins = []
    for b in range(B):
        psi, _, eta, _ = optimistic_sampling_scalars(int(env.n_states[b]), env.A, HORIZON)
        twins.append(PSRLOTwin(b, int(env.n_states[b]), env.A, env.rewards_range[1], psi, eta,
                               lambda T, R: dp.discounted_value_iteration_dense_batch([(T, R)])[0][0]))
    cur = env.state()[0].copy()
    t0 = time.perf_counter()
    solves = 0
    for tw in twins:
        tw.before_start_interacting()
        solves += 1
    for _ in range(args.host_steps):
        acts = np.array([tw.select_action(int(cur[b])) for b, tw in enumerate(twins)], np.int32)
        obs, rew, _ = env.step(acts)
        for b, tw in enumerate(twins):
            s, a = int(cur[b]), int(acts[b])
            tw.step_update(s, a, float(rew[b]), int(obs[b]))
            if tw.is_episode_end(s, a):
                tw.episode_end_update()
                solves += 1
        cur = obs.copy()
    dt = time.perf_counter() - t0
    env.close()
    return dict(B=B, steps=args.host_steps, solves=solves, run_s=dt, steps_per_s=B * args.host_steps / dt, solves_per_s=solves / dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--batch", default="all", choices=sorted(BATCHES) + sorted(COMPACT_ONLY) + ["all"],
                    help="frozenlake20 with --sample-solver only")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--chunk", type=int, default=10)
    ap.add_argument("--max-seconds", type=float, default=0.0, help="> 0: the timed run() stops after the chunk that passes this")
    ap.add_argument("--sampler", default="philox", choices=["philox", "reference"])
    ap.add_argument("--host-steps", type=int, default=10)
    ap.add_argument("--sample-solver", default=None, choices=["dense", "compact", "both"],
                    help="time the optimistic agent's sample routes (K19) instead: writes k19_psrlo_compact.json")
    args = ap.parse_args()
    if L.load().cmdp_device_count() == 0:
        raise SystemExit("no HIP device visible: times are taken on the GPU only")
    os.makedirs(args.out, exist_ok=True)
    if args.sample_solver:
        routes = ["dense", "compact"] if args.sample_solver == "both" else [args.sample_solver]
        names = sorted(BATCHES, key=lambda n: BATCHES[n][0]) if args.batch == "all" else [args.batch]
        path = os.path.join(args.out, "k19_psrlo_compact.json")
        res = json.load(open(path)) if os.path.exists(path) else {}
        for name in names + (sorted(COMPACT_ONLY) if args.batch == "all" and "compact" in routes else []):
            res[name] = time_sample_routes(name, routes if name in BATCHES else ["compact"], args)
            print(json.dumps({name: res[name]}), flush=True)
            with open(path, "w") as f:   # a shape at a time: what has been measured is kept
                json.dump(res, f, indent=1)
        return
    z = np.load(os.path.join(ROOT, "tests", "golden", "G23_psrlo.npz"))
    ref = [dict(cls=m["cls"], S=m["S"], A=m["A"], psi=m["psi"], steps_per_s=m["reference_steps_per_second"])
           for m in json.loads(str(z["cases"]))]
    names = sorted(BATCHES, key=lambda n: BATCHES[n][0]) if args.batch == "all" else [args.batch]
    res = dict(reference_steps_per_second_one_core=ref)
    for name in names:
        res[name] = {}
        for part, f in (("optimistic", lambda: time_agent(name, "optimistic", args)), ("plain", lambda: time_agent(name, "plain", args)),
                        ("host_route", lambda: time_host_route(name, args))):
            res[name][part] = f()
            print(json.dumps({name: {part: res[name][part]}}), flush=True)   # a part at a time: a long batch shows where it is
    path = os.path.join(args.out, "k18_psrlo.json")
    if args.batch != "all" and os.path.exists(path):   # one batch per call: keep the others
        old = json.load(open(path))
        old.update(res)
        res = old
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
