"""Times the two routes behind BatchedPSRLContinuous.policy() / policy_solve() / average_reward() on the same agent and
the same posterior tables: "dense" (k_psrlc_map_fill writes the dense MAP model [S, A, S] of every instance, then
k_vi_discounted_dense sweeps it -- the route as it has been launched since K13) and "tables" (K17 k_vi_discounted_map
straight on the tables, csrc/cmdp_map_dvi.h).  K17's two forms -- every instance's tables staged in LDS
(CMDP_MAPDVI_STAGE=1) and left in global memory (CMDP_MAPDVI_STAGE=0) -- are timed next to the picker's own choice.

    python tools/time_psrlc_policy.py --out FILE.json --batch NAME [--steps 200]

Batches: 256 x FrozenLake-5, 128 x FrozenLake-10, 64 x FrozenLake-20 and 1 000 x FrozenLake-20, Philox environments and
sampler.  Two stages of one agent: fresh (the prior) and after --steps steps.  Those steps are taken under a sweep limit
of 1 for the agent's OWN solves (which nothing here measures and which would take minutes at 1 000 instances, almost every
early step ending an artificial episode): the tables then hold the counts of --steps steps of a near-random walk; the limit
is lifted before anything is timed.  Per stage: one warm-up call per route on the timed shape, then the routes ALTERNATE,
twice; per route the best of two of CMDP_STAT_PSRL_POLICY_KERNEL_MS after policy_solve() (HIP events around the route's
kernels: map fill + dense solve, or K17) and of the wall time of average_reward(), with both values kept; the sweeps per
instance; the bytes of workspace the route allocates.  Numbers only: no ratio is formed or asserted.  One batch per
process, at most 16 CPU threads; results of several batches are merged into FILE.json:

    timeout -k 10 120 python tools/time_psrlc_policy.py --out profiles/k17_map_dvi.json --batch frozenlake5 && \\
    timeout -k 10 120 python tools/time_psrlc_policy.py --out profiles/k17_map_dvi.json --batch frozenlake10 && \\
    timeout -k 10 180 python tools/time_psrlc_policy.py --out profiles/k17_map_dvi.json --batch frozenlake20 && \\
    timeout -k 10 420 python tools/time_psrlc_policy.py --out profiles/k17_map_dvi.json --batch frozenlake20x1000"""
import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16"))))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from colosseum_amd import _lib as L  # noqa: E402
from colosseum_amd import dynamic_programming as dp  # noqa: E402
from colosseum_amd.agents import BatchedPSRLContinuous  # noqa: E402
from colosseum_amd.batched import BatchedMDP  # noqa: E402
from colosseum_amd.mdp import make_model  # noqa: E402

BATCHES = {   # FrozenLakeContinuous size, instances
    "frozenlake5": (5, 256),
    "frozenlake10": (10, 128),
    "frozenlake20": (20, 64),
    "frozenlake20x1000": (20, 1000),
}
# route name -> (set_policy_solver's argument, CMDP_MAPDVI_STAGE or None for the picker's own choice)
ROUTES = {"dense": ("dense", None), "tables": ("tables", None), "tables_staged_in_lds": ("tables", "1"),
          "tables_global_memory": ("tables", "0")}


def set_route(agent, name):
    solver, stage = ROUTES[name]
    if stage is None:
        os.environ.pop("CMDP_MAPDVI_STAGE", None)
    else:
        os.environ["CMDP_MAPDVI_STAGE"] = stage
    agent.set_policy_solver(solver)


def make_agent(name):
    size, B = BATCHES[name]
    base = [make_model("FrozenLakeContinuous", seed=s, size=size, p_frozen=0.9) for s in range(4)]
    env = BatchedMDP([base[b % 4] for b in range(B)], rng_mode=L.RNG_PHILOX, philox_keys=np.arange(B, dtype=np.uint64) * 7919 + 5)
    env.reset()
    return env, BatchedPSRLContinuous(env, np.arange(B), 10 ** 6, sampler="philox", no_optimistic_sampling=True)


def workspace_bytes(agent):
    """What a route allocates beyond the buffers both share (Q, V, policy, sweeps, scheme, status, list)."""
    env = agent.env
    R = int(env.row_off[-1])
    dense_t = sum((int(S) * env.A * int(S) + 3) & ~3 for S in env.n_states)   # every instance padded to 16 bytes
    tables = 4 * (agent._nz + R)
    return dict(dense=4 * (dense_t + 2 * R), tables=tables, tables_staged_in_lds=tables, tables_global_memory=tables)


def stage(agent):
    out = {r: dict(policy_kernel_ms=[], average_reward_wall_s=[]) for r in ROUTES}
    for r in ROUTES:   # warm-up on the timed shape: the route's code objects and its workspace
        set_route(agent, r)
        agent.policy_solve()
        agent.average_reward()
    for _ in range(2):
        for r in ROUTES:
            set_route(agent, r)
            sol = agent.policy_solve()
            out[r]["policy_kernel_ms"].append(agent.stats()["policy_kernel_ms"])
            t = time.perf_counter()
            agent.average_reward()
            out[r]["average_reward_wall_s"].append(time.perf_counter() - t)
            sw = sol["sweeps"]
            out[r]["sweeps_per_instance"] = dict(min=int(sw.min()), median=float(np.median(sw)), max=int(sw.max()))
            out[r]["jacobi_instances"] = int((sol["scheme"] == L.SCHEME_JACOBI).sum())
    for r in ROUTES:
        out[r]["policy_kernel_ms_best"] = min(out[r]["policy_kernel_ms"])
        out[r]["average_reward_wall_s_best"] = min(out[r]["average_reward_wall_s"])
    set_route(agent, "dense")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", required=True, choices=sorted(BATCHES))
    ap.add_argument("--steps", type=int, default=200, help="steps before the second stage")
    args = ap.parse_args()
    if L.load().cmdp_device_count() == 0:
        raise SystemExit("no HIP device visible: times are taken on the GPU only")
    env, agent = make_agent(args.batch)
    ws = workspace_bytes(agent)
    res = dict(B=env.B, S=[int(s) for s in sorted(set(env.n_states.tolist()))], A=env.A, layout_positions=int(agent._nz),
               workspace_bytes=ws, steps=args.steps, stages={})
    res["stages"]["fresh"] = stage(agent)
    print(args.batch, "fresh", json.dumps(res["stages"]["fresh"]), flush=True)
    agent._set_max_sweeps(1)   # the agent's own solves during the steps: see the module's text
    t = time.perf_counter()
    agent.run(args.steps)
    res["run_wall_s_at_sweep_limit_1"] = time.perf_counter() - t
    agent._set_max_sweeps(dp.DP_MAX_ITERATION)
    key = f"after_{args.steps}_steps"
    res["stages"][key] = stage(agent)
    print(args.batch, key, json.dumps(res["stages"][key]), flush=True)
    env.close()
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged[args.batch] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
