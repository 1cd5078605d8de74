"""Times the PSRL agent's MAP-policy evaluation on the device (K15 k_vi_episodic_map + greedy policy + the handle's episodic
policy evaluation, BatchedPSRLEpisodic.evaluate) against the host route: the dense model of an instance ->
hyper_params / hyper_params.sum(-1) -> dp.episodic_value_iteration -> dp.argmax_3d, what
current_optimal_stochastic_policy does per instance.

    python tools/time_psrl_policy.py --out FILE.json [--batch frozenlake20|small] [--host-instances N]

The batches are those of tools/time_psrl.py (Philox environments and sampler).  Three stages of one agent: fresh (the
prior), after 3 and after 30 episodes.  Per stage, after a warm-up call on the timed shape: the wall time of evaluate() and of
policy_solve() for the whole batch (best of two, both printed), K15's HIP-event time, the host route on the first
--host-instances instances (per instance, best of two; only their dense models are built), and
dp.episodic_value_iteration_dense_batch (kernel K12's solver) on the dense MAP estimates of those instances in one call.
Numbers only: no ratio is formed or asserted.  One batch per process; results of several batches are merged into FILE.json:

    timeout -k 10 300 python tools/time_psrl_policy.py --out profiles/k15_map_vi.json --batch small && \\
    timeout -k 10 900 python tools/time_psrl_policy.py --out profiles/k15_map_vi.json --batch frozenlake20"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from colosseum_amd import _lib as L  # noqa: E402
from colosseum_amd import dynamic_programming as dp  # noqa: E402
from colosseum_amd.agents import BatchedPSRLEpisodic  # noqa: E402
from time_psrl import BATCHES, make_env  # noqa: E402

STAGES = (0, 3, 30)   # episodes completed when the stage is measured


def best_of_two(f):
    out = []
    for _ in range(2):
        t = time.perf_counter()
        f()
        out.append(time.perf_counter() - t)
    return out


def host_tables(agent):
    """The model's tables as cmdp_psrl_model returns them (layout form; nothing dense)."""
    env = agent.env
    R = int(env.row_off[-1])
    rp, tp, prior = np.zeros(R * 4, np.float32), np.zeros(agent._nz, np.float32), np.zeros(env.B, np.float32)
    L.check(agent._lib.cmdp_psrl_model(agent._h, L.ptr(rp), L.ptr(tp), L.ptr(prior), None))
    return rp.reshape(R, 4), tp, prior


def host_route(agent, tables, b):
    """Instance b as model() -> map_estimate() -> current_optimal_stochastic_policy() treat it.  Returns (policy, dense MAP, mu)."""
    env = agent.env
    rp, tp, prior = tables
    S, H = int(env.n_states[b]), int(env.H)
    r0, r1 = int(env.row_off[b]), int(env.row_off[b + 1])
    z0, z1 = int(agent._ptr[r0]), int(agent._ptr[r1])
    M = np.full((r1 - r0, S), prior[b], np.float32)
    M[agent._rows[z0:z1] - r0, agent._col[z0:z1]] = tp[z0:z1]
    t = M.reshape(S, env.A, S)
    T, R = t / t.sum(-1, keepdims=True), rp[r0:r1, 0].reshape(S, env.A)
    Q = dp.episodic_value_iteration(H, np.ascontiguousarray(T), np.ascontiguousarray(R))[0]
    return dp.argmax_3d(Q), T, R


def stage(agent, n_host):
    env, B, H = agent.env, agent.env.B, int(agent.env.H)
    agent.evaluate()   # warm-up on the timed shape
    ev = best_of_two(agent.evaluate)
    kernel_ms = agent.stats()["policy_kernel_ms"]
    solve = best_of_two(agent.policy_solve)
    fetch = best_of_two(lambda: host_tables(agent))
    tables = host_tables(agent)
    host, maps = [], []
    for b in range(n_host):
        dp.release_handles()
        host_route(agent, tables, b)   # warm-up
        ts = []
        for _ in range(2):
            dp.release_handles()   # the route builds its device handle per call of a new model, as it does per log row
            t = time.perf_counter()
            _, T, R = host_route(agent, tables, b)
            ts.append(time.perf_counter() - t)
        host.append(min(ts))
        maps.append((T, R))
    dp.release_handles()
    dp.episodic_value_iteration_dense_batch(maps, H)   # warm-up
    dense = best_of_two(lambda: dp.episodic_value_iteration_dense_batch(maps, H))
    return dict(evaluate_wall_s=ev, evaluate_wall_s_best=min(ev), k15_kernel_ms=kernel_ms, policy_solve_wall_s=solve,
                device_evaluate_s_per_instance=min(ev) / B, host_instances=n_host, host_table_fetch_s=fetch,
                host_route_s_each=host, host_route_s_per_instance=float(np.mean(host)),
                dense_batch_wall_s=dense, dense_batch_s_per_instance=min(dense) / n_host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", default="small", choices=sorted(BATCHES))
    ap.add_argument("--host-instances", type=int, default=8)
    args = ap.parse_args()
    env = make_env(args.batch)
    agent = BatchedPSRLEpisodic(env, np.arange(env.B), 10 ** 6, sampler="philox")
    res = dict(B=env.B, S=int(env.n_states[0]), A=env.A, H=int(env.H), layout_positions=int(agent._nz), stages={})
    at = 0
    for upto in STAGES:
        if upto > at:
            agent.run((upto - at) * env.H)
            at = upto
        res["stages"][str(upto)] = r = stage(agent, min(args.host_instances, env.B))
        print(args.batch, "episodes", upto, json.dumps({k: v for k, v in r.items() if k != "host_route_s_each"}), flush=True)
    env.close()
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged[args.batch] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
