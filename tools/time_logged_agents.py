"""Wall time of a logged run of the park-and-solve agents, one configuration per process.

    python tools/time_logged_agents.py --agent ucrl2 --route native --reuse 1
    python tools/time_logged_agents.py --agent psrl --route python
    python tools/time_logged_agents.py --agent psrlo --route native --instances 64 --size 10 --min-steps 50 --append profiles/logged_psrlc.json

A batch of FrozenLake instances (default 1 000 of size 20, about 360 states each: eight lakes repeated under different keys and seeds), `--steps` steps logged every `--log-every`, through
`BatchedContinuousLoop` (UCRL2; "psrlc" / "psrlo": the continuous PSRL agent with plain / optimistic sampling, built by the
`benchmark.make_psrl_continuous` on its default routes with the Philox sampler and `--min-steps`) or `BatchedEpisodicLoop` (PSRL) on the route asked for: "native" is the library's logged
driver, "python" the Python-driven loop (`loop.native = False`).  Prints one JSON line: the wall time of `loop.run` alone,
and for UCRL2 the policy-solve counters and -- on the Python-driven route, where every row returns to Python -- the sum of
the HIP-event times of the K14 launches.  On a tree without the logged driver only `--route python` runs; counters it does
not have are reported as null.  `--append FILE` also appends the record to the JSON list in FILE."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402

from colosseum_amd import _lib as L  # noqa: E402
from colosseum_amd import benchmark as bm  # noqa: E402


def usable_continuous(models):
    """Per model: optimal - worst average reward > 0.0002, which `MDPLoop` asserts (agent_mdp_interaction.py:379-382; a lake
    whose goal cannot be reached has none).  The two baselines as `BatchedContinuousLoop` computes them."""
    from colosseum_amd.batched import BatchedMDP
    from colosseum_amd.dynamic_programming import get_policy_from_q_values
    from colosseum_amd.markov_chain import get_average_reward_batch

    env = BatchedMDP(models, with_env=False)
    A = env.A
    Q, _, _ = env.value_iteration()
    Qw, _, _ = env.value_iteration(R=[-m.reward_matrix() for m in models])
    probs = []
    for b, m in enumerate(models):
        T, R = m.dense()
        starts = list(zip(m.start_states.tolist(), m.start_probs.tolist()))
        for q in (Q, Qw):
            probs.append((T, R, get_policy_from_q_values(env.split_rows(q)[b].reshape(m.n_states, A), True), starts))
    vals = get_average_reward_batch(probs, builtin_sum=True)
    env.close()
    return [float(vals[2 * b]) - float(vals[2 * b + 1]) > 0.0002 for b in range(len(models))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agent", choices=["ucrl2", "psrl", "psrlc", "psrlo"], required=True)
    ap.add_argument("--route", choices=["native", "python"], required=True)
    ap.add_argument("--reuse", type=int, choices=[0, 1], help="UCRL2: the policy reuse (default: the library's)")
    ap.add_argument("--instances", type=int, default=1000)
    ap.add_argument("--size", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--log-every", type=int, default=100)
    ap.add_argument("--base-models", type=int, default=8, help="distinct lakes (seeds 0 ..) the batch repeats")
    ap.add_argument("--min-steps", type=int, default=0, help="psrlc / psrlo: min_steps_before_new_episode")
    ap.add_argument("--append", help="a JSON file holding a list: the record is appended to it")
    args = ap.parse_args()
    cls = "FrozenLakeEpisodic" if args.agent == "psrl" else "FrozenLakeContinuous"
    # as tools/time_ucrl2.py: a few lakes, repeated under different keys and agent seeds.  A continuous batch shares the scheme
    # the reference's rule picks for its baselines, and MDPLoop refuses a lake whose goal cannot be reached
    from colosseum_amd.hardness import _vi_rule
    from colosseum_amd.mdp import make_model

    base = [make_model(cls, seed=s, size=args.size, p_frozen=0.9, p_rand=0.1) for s in range(2 * args.base_models)]
    scheme = [_vi_rule(m.n_states, m.n_actions, len(m.csr()[1])) for m in base]
    base = [m for m, k in zip(base, scheme) if k == max(set(scheme), key=scheme.count)]
    if args.agent != "psrl":
        base = [m for m, ok in zip(base, usable_continuous(base)) if ok]
    base = base[:args.base_models]
    models = [base[b % len(base)] for b in range(args.instances)]
    assert len(models) == args.instances
    from colosseum_amd.agents import BatchedPSRLEpisodic, BatchedUCRL2Continuous
    from colosseum_amd.batched import BatchedMDP
    from colosseum_amd.experiment.batched_loop import BatchedContinuousLoop, BatchedEpisodicLoop

    t0 = time.time()
    seeds = list(range(args.instances))
    env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=np.arange(args.instances, dtype=np.uint64) * 7919 + 5)
    if args.agent == "ucrl2":
        agent = BatchedUCRL2Continuous(env, seeds, optimization_horizon=args.steps, **bm.DEFAULT_AGENT_CONFIGS.get(
            "UCRL2Continuous", dict(bound_type_p="bernstein", alpha_p=0.9883750006754203, alpha_r=0.10294276593728004)))
        loop = BatchedContinuousLoop(env, agent)
        if args.reuse is not None:
            agent._set_policy_reuse(bool(args.reuse))
    elif args.agent in ("psrlc", "psrlo"):
        agent = bm.make_psrl_continuous(env, seeds, optimization_horizon=args.steps, sampler="philox",
                                        no_optimistic_sampling=args.agent == "psrlc", min_steps_before_new_episode=args.min_steps,
                                        **bm.DEFAULT_AGENT_CONFIGS["PSRLContinuous"])
        loop = BatchedContinuousLoop(env, agent)
    else:
        agent = BatchedPSRLEpisodic(env, seeds, optimization_horizon=args.steps, sampler="philox")
        loop = BatchedEpisodicLoop(env, agent)
    loop.native = args.route == "native"
    k14 = {"ms": 0.0, "launches": 0}
    if args.agent == "ucrl2" and args.route == "python":
        inner = agent.average_reward

        def timed(need=None):
            before = agent.stats().get("policy_solved")
            out = inner(need)
            s = agent.stats()
            if before is None or s["policy_solved"] != before:   # (a request that reused every policy launches nothing)
                k14["ms"] += s["policy_kernel_ms"]
                k14["launches"] += 1
            return out

        agent.average_reward = timed
    setup_s = time.time() - t0
    t1 = time.time()
    rows = loop._run_native(args.steps, args.log_every, np.inf) if loop.native else loop.run(args.steps, args.log_every)
    wall = time.time() - t1
    stats = agent.stats()
    record = dict(
        agent=args.agent, route=args.route, reuse=args.reuse, instances=args.instances, mdp=cls, size=args.size,
        base_models=len(base), n_states=[int(m.n_states) for m in base], horizon=int(env.H), steps=args.steps, log_every=args.log_every, rows=len(rows[0]),
        setup_s=round(setup_s, 3), run_wall_s=round(wall, 3), policy_solved=stats.get("policy_solved"),
        policy_reused=stats.get("policy_reused"), k14_ms_sum=round(k14["ms"], 3) if k14["launches"] else None,
        k14_launches=k14["launches"] or None, rounds=stats.get("rounds"), solves=stats.get("solves"),
        mean_normalized_cumulative_regret=float(np.nanmean([float(t[-1]["normalized_cumulative_regret"]) for t in rows])))
    if args.agent in ("psrlc", "psrlo"):
        record.update(min_steps=args.min_steps, sweeps_last_round=stats.get("sweeps"), policy_solver=agent.policy_solver,
                      sample_solver=getattr(agent, "sample_solver", None), agent_class=type(agent).__name__)
    print(json.dumps(record))
    if args.append:
        old = json.load(open(args.append)) if os.path.exists(args.append) else []
        with open(args.append, "w") as f:
            json.dump(old + [record], f, indent=1)
            f.write("\n")
    agent.close()
    env.close()


if __name__ == "__main__":
    main()
