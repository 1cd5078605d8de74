"""Times config C2 at full size under CMDP_POLICY_RANDOM_REFERENCE (the reference's RandomActor stream, generated on the device
by K16 k_mt_actions and consumed by K1E) and, in the same run, under CMDP_POLICY_RANDOM (the Philox stream) beside it.

    python tools/time_reference_stream.py --out profiles/reference_stream.json [--instances 65536] [--launches 10]

65 536 x DeepSeaEpisodic(seed=i, size=30), 30 000 transitions per launch, action seeds = instance index.  Per policy: W untimed
launches, then K back to back between two HIP events on the handle's stream (ms per launch), and the library's own HIP-event
times of the last launch: K16 (CMDP_STAT_ACTIONS_KERNEL_MS) and the walk k_rollout_epi (CMDP_STAT_ROLLOUT_KERNEL_MS)
separately.  After the timed region one more launch is made synchronously, and 64 sampled instances are checked -- visit
counts, the last launch's reward sum, final state and in-episode time -- against the CPU oracle fed
np.random.RandomState(i).randint(0, 2, .) through its host-actions entry.  The file records what was measured; it carries no
target for the new mode.  Keys of the file other than "c2" (written by hand from compiler remarks and bench.py runs, as the
file says) are kept."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from colosseum_amd import _lib as L  # noqa: E402
from colosseum_amd.batched import BatchedMDP  # noqa: E402
from colosseum_amd.mdp import make_model  # noqa: E402
from colosseum_amd.mdp.fast_batch import deepsea_episodic_tables  # noqa: E402


class HipEvents:
    def __init__(self):
        L.load()
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.hip.hipEventDestroy.argtypes = [C.c_void_p]

    def create(self):
        e = C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(e)) == 0
        return e

    def record(self, e, stream):
        assert self.hip.hipEventRecord(e, C.c_void_p(stream)) == 0

    def elapsed_ms(self, a, b):
        assert self.hip.hipEventSynchronize(b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), a, b) == 0
        return float(ms.value)

    def destroy(self, e):
        self.hip.hipEventDestroy(e)


def stat(env, which):
    v = C.c_double()
    L.check(L.load().cmdp_stat(env.handle, which, C.byref(v)))
    return float(v.value)


def timed(env, ev, policy, n_launch, steps, warmup):
    for _ in range(warmup):
        env.rollout_async(steps, policy=policy)
    env.synchronize()
    a, b = ev.create(), ev.create()
    t0 = time.perf_counter()
    ev.record(a, env.stream)
    for _ in range(n_launch):
        env.rollout_async(steps, policy=policy)
    ev.record(b, env.stream)
    env.synchronize()
    wall = time.perf_counter() - t0
    ms = ev.elapsed_ms(a, b)
    ev.destroy(a)
    ev.destroy(b)
    out = dict(launches=n_launch, event_ms_per_launch=ms / n_launch, wall_ms_per_launch=wall * 1e3 / n_launch,
               walk_kernel_ms=stat(env, L.STAT_ROLLOUT_KERNEL_MS), reward_scan_kernel_ms=stat(env, L.STAT_HIST_KERNEL_MS))
    if policy == "reference":
        out["k16_kernel_ms"] = stat(env, L.STAT_ACTIONS_KERNEL_MS)
    out["transitions_per_s"] = env.B * steps / (out["event_ms_per_launch"] * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--instances", type=int, default=65536)
    ap.add_argument("--size", type=int, default=30)
    ap.add_argument("--launch-steps", type=int, default=30000)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--check-instances", type=int, default=64)
    args = ap.parse_args()
    from oracle import oracle as O   # the checker, used after the timed region only

    B, steps = args.instances, args.launch_steps
    seeds = np.arange(B, dtype=np.int64)
    tables = deepsea_episodic_tables(seeds, args.size, with_dp=False)
    ev = HipEvents()
    res = dict(instances=B, size=args.size, transitions_per_launch=steps, warmup_launches=args.warmup)
    for policy in (None, "reference"):
        env = BatchedMDP(tables=tables, rng_mode=L.RNG_PHILOX, philox_keys=seeds.astype(np.uint64))
        assert env.lds_plan()["kernel"] == "k_rollout_epi"
        if policy == "reference":
            env.set_action_streams(seeds)
        env.reset()
        r = timed(env, ev, policy, args.launches, steps, args.warmup)
        r["k1e_form"] = env.k1e_plan()["last_form"]
        res["philox" if policy is None else "reference"] = r
        print(policy or "philox", json.dumps(r), flush=True)
        if policy == "reference":
            # ---- after the timed region: one synchronous launch, then the sampled check against the oracle ----
            n_launch = args.warmup + args.launches + 1
            out = env.rollout(steps, policy="reference")
            vs, vsa = env.visits()
            cur, h, _ = env.state()
            sample = np.unique(np.linspace(0, B - 1, args.check_instances).astype(np.int64))
            ok = True
            for i in sample:
                m = make_model("DeepSeaEpisodic", seed=int(i), size=args.size)
                acts = np.random.RandomState(int(i)).randint(0, 2, n_launch * steps).astype(np.int8)
                e = O.OracleEnv(m, rng_mode=1, philox_key=int(i))
                e.reset()
                for k in range(n_launch):
                    ref = e.rollout(steps, acts[k * steps:(k + 1) * steps], trace=False)
                ovs, ovsa = e.visits()
                ocur, oh, _ = e.state()
                same = (np.array_equal(env.split_states(vs)[i], ovs) and np.array_equal(env.split_rows(vsa)[i].reshape(-1, 2), ovsa)
                        and out["reward_sum"][i] == ref["reward_sum"] and cur[i] == ocur and h[i] == oh)
                if not same:
                    print("MISMATCH at instance", int(i), flush=True)
                ok = ok and same
            res["check"] = dict(instances=[int(i) for i in sample], launches_from_reset=n_launch, equals_oracle_on_numpy_actions=bool(ok),
                                compared="visit counts (state, state-action), reward sum of the last launch, final state, in-episode time")
            print("check", ok, flush=True)
        env.close()
    res["reference_over_philox"] = res["reference"]["event_ms_per_launch"] / res["philox"]["event_ms_per_launch"]
    merged = json.load(open(args.out)) if os.path.exists(args.out) else {}
    merged["c2"] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
        f.write("\n")
    if not res["check"]["equals_oracle_on_numpy_actions"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
