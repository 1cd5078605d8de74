"""Times extended value iteration (K10 k_evi via extended_value_iteration_batch) on batches of agent-shaped problems.

    python tools/time_evi.py --out DIR [--reps N] [--cases NAME,...]

Each case is B estimated models of one benchmark-sized continuous MDP, counts drawn at an early visit budget (mostly
unvisited, uniform rows) or a late one (mostly sparse rows), UCRL2's Bernstein bounds.  Whole batched calls (upload,
one launch, read-back, synchronised) are timed after a warm-up; solves/s, sweeps/s and the time per sweep per instance
are reported, and the float64 restatement's time on a few instances (numba is not available, so the reference's own
speed is not timed).  Outputs are checked against the restatement after the timed region.  JSON goes to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from colosseum_amd import dynamic_programming as dp  # noqa: E402
from colosseum_amd.mdp import make_model  # noqa: E402
from helpers_evi import agent_problem, bound, evi_f64  # noqa: E402

ALPHA = 0.1  # alpha_p = alpha_r: bounds of a tuned agent (at 1.0 every row is one-hot and a solve is one sweep)
CASES = {
    "frozenlake20_early": ("FrozenLakeContinuous", dict(size=20, p_frozen=0.9, p_rand=0.1), 1000, 2, 0.9),
    "frozenlake20_late": ("FrozenLakeContinuous", dict(size=20, p_frozen=0.9, p_rand=0.1), 1000, 200, 0.05),
    "minigrid_empty_784_early": ("MiniGridEmptyContinuous", dict(size=14), 90, 2, 0.9),
    "minigrid_empty_784_late": ("MiniGridEmptyContinuous", dict(size=14), 90, 200, 0.05),
}


def build(name, n_models=8):
    fam, kw, B, visits, unvisited = CASES[name]
    models = [make_model(fam, seed=s, **kw).dense() for s in range(n_models)]
    return [agent_problem(*models[b % n_models], visits, 10_000 + b, "bernstein", None, ALPHA, 1.0, unvisited)
            for b in range(B)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="directory for time_evi.json")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--check", type=int, default=3, help="instances checked against the float64 restatement")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    results = []
    for name in args.cases.split(","):
        probs = build(name)
        S, A = probs[0][1].shape
        dp.extended_value_iteration_batch(probs)  # warm-up: workspace, code object
        times = []
        for _ in range(args.reps):
            t = time.perf_counter()
            out, sweeps = dp.extended_value_iteration_batch(probs)
            times.append(time.perf_counter() - t)
        med = float(np.median(times))
        B, tot = len(probs), int(sweeps.sum())
        checked, f64_s = [], []
        for i in range(min(args.check, B)):  # after the timed region
            t = time.perf_counter()
            span_r, Q_r, V_r, sw_r, last_ptp, umax, _ = evi_f64(*probs[i])
            f64_s.append(time.perf_counter() - t)
            b = 2 * bound(max(sw_r, int(sweeps[i])), umax + 2.0, 1)
            ok = out[i] is not None and span_r is not None and abs(float(out[i][0]) - span_r) <= b and \
                np.abs(out[i][1] - Q_r).max() <= b and np.abs(out[i][2] - V_r).max() <= b
            checked.append(bool(ok))
        r = dict(case=name, B=B, S=int(S), A=int(A), reps=args.reps, call_s_median=med, call_s=times,
                 solves_per_s=B / med, sweeps_total=tot, sweeps_min=int(sweeps.min()), sweeps_max=int(sweeps.max()),
                 sweeps_per_s=tot / med, us_per_sweep_per_instance=1e6 * med / max(tot, 1) * 1.0,
                 wall_us_per_max_sweep=1e6 * med / max(int(sweeps.max()), 1),
                 f64_restatement_s_per_solve=float(np.mean(f64_s)) if f64_s else None, checked_ok=checked,
                 uniform_row_fraction=float(np.mean([(p[0] == p[0][:, :, :1]).all(-1).mean() for p in probs[:16]])))
        print(json.dumps(r), flush=True)
        results.append(r)
        assert all(checked), f"{name}: outputs outside the float64 bound"
    with open(os.path.join(args.out, "time_evi.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
