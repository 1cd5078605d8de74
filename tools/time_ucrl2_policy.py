"""Times the UCRL2 agent's policy evaluation on the device (K14 k_vi_model + greedy policy + the chain kernels,
BatchedUCRL2Continuous.average_reward) against the host route it replaces: model() -> dp.discounted_value_iteration ->
dp.argmax_2d per instance, what current_optimal_stochastic_policy did before K14.

    python tools/time_ucrl2_policy.py --out FILE.json [--batch frozenlake20|minigrid784|small] [--host-instances N]

The batches are those of tools/time_ucrl2.py.  Three stages of one agent: fresh (every row of the estimated model uniform),
after 2 000 steps and after 20 000 steps.  Per stage: the wall time of average_reward() (two repetitions), K14's HIP-event
time, the schemes taken and the sweeps, and the host route on the first --host-instances instances, per instance (the dense
model of those instances only is built; the device's policy is compared with the host's on them).  One batch per process;
results of several batches are merged into FILE.json.  A job runs each batch as a step of its own under its own time limit,
the second only after the first ended well (the host route of a fresh MiniGridEmpty-784 instance takes 20 s and more):

    timeout -k 10 600 python tools/time_ucrl2_policy.py --out profiles/k14_model_vi.json --batch frozenlake20 && \\
    timeout -k 10 500 python tools/time_ucrl2_policy.py --out profiles/k14_model_vi.json --batch minigrid784 --host-instances 2"""
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
from colosseum_amd.agents import BatchedUCRL2Continuous  # noqa: E402
from time_ucrl2 import ALPHA, BATCHES, make_env  # noqa: E402

STAGES = (0, 2_000, 20_000)   # steps taken when the stage is measured


def host_models(agent, n):
    """Dense (P, estimated_rewards) of the first n instances, as model() builds them for all."""
    env = agent.env
    R = int(env.row_off[-1])
    P, uni, er = np.zeros(agent._nz, np.float32), np.zeros(R, np.float32), np.zeros(R, np.float32)
    L.check(agent._lib.cmdp_ucrl2_model(agent._h, None, L.ptr(P), L.ptr(uni), L.ptr(er), None, None, None, None, None))
    out = []
    for b in range(n):
        S = int(env.n_states[b])
        r0, r1 = int(env.row_off[b]), int(env.row_off[b + 1])
        z0, z1 = int(agent._ptr[r0]), int(agent._ptr[r1])
        M = np.zeros((r1 - r0, S), np.float32)
        M[agent._rows[z0:z1] - r0, agent._col[z0:z1]] = P[z0:z1]
        u = uni[r0:r1]
        M[u > 0] = u[u > 0, None]
        out.append((M.reshape(S, env.A, S), er[r0:r1].reshape(S, env.A)))
    return out


def stage(agent, n_host):
    env, B = agent.env, agent.env.B
    walls = []
    for _ in range(2):
        t = time.perf_counter()
        agent.average_reward()
        walls.append(time.perf_counter() - t)
    kernel_ms = agent.stats()["policy_kernel_ms"]
    sol = agent.policy_solve()
    pis = agent.policy()
    t = time.perf_counter()
    models = host_models(agent, n_host)
    fetch_s = time.perf_counter() - t
    host_s, same = [], True
    for b, (P, R) in enumerate(models):
        dp.release_handles()
        t = time.perf_counter()
        Q, _ = dp.discounted_value_iteration(P, R)
        pi = dp.argmax_2d(Q)
        host_s.append(time.perf_counter() - t)
        same = same and np.array_equal(pi, pis[b]) and np.array_equal(Q, sol["Q"][b])
    dp.release_handles()
    dev = min(walls) / B
    return dict(average_reward_wall_s=walls, k14_kernel_ms=kernel_ms, device_s_per_instance=dev,
                schemes={"jacobi": int((sol["scheme"] == L.SCHEME_JACOBI).sum()), "gauss_seidel": int((sol["scheme"] == L.SCHEME_GAUSS_SEIDEL).sum())},
                sweeps_min=int(sol["sweeps"].min()), sweeps_max=int(sol["sweeps"].max()), sweeps_mean=float(sol["sweeps"].mean()),
                host_instances=n_host, host_s_per_instance=float(np.mean(host_s)), host_s_each=host_s, host_fetch_s=fetch_s,
                host_equals_device_bit_for_bit=bool(same), host_over_device=float(np.mean(host_s)) / dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", default="frozenlake20", choices=sorted(BATCHES))
    ap.add_argument("--host-instances", type=int, default=8)
    args = ap.parse_args()
    env = make_env(args.batch)
    agent = BatchedUCRL2Continuous(env, np.arange(env.B), STAGES[-1], alpha_r=ALPHA, alpha_p=ALPHA, bound_type_p="bernstein")
    agent.average_reward()   # warm-up: allocations, the chain plan
    res = dict(B=env.B, S=int(env.n_states[0]), A=env.A, stages={})
    at = 0
    for upto in STAGES:
        if upto > at:
            agent.run(upto - at)
            at = upto
        res["stages"][str(upto)] = r = stage(agent, min(args.host_instances, env.B))
        print(args.batch, "steps", upto, json.dumps({k: v for k, v in r.items() if k != "host_s_each"}), flush=True)
    env.close()
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged[args.batch] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
