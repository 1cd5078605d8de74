"""Times the continuous PSRL agent (K13, BatchedPSRLContinuous, Philox sampler) and the two forms of its solver
k_vi_discounted_dense: four wavefronts per instance (a workgroup splits a state's rows, one barrier per state in Gauss-Seidel)
against one wavefront per instance (CMDP_DDV_WAVES=1).  The results of the two forms are the same bits (asserted here on
the Q of every round that is timed); only the time differs.

    python tools/time_psrlc.py [--out profiles] [--batch all|frozenlake5|frozenlake10|frozenlake20] [--reps 5] [--steps 200]

Per batch: the agent is created (solve on the prior, warm-up of both forms), then --reps rounds of episode_end_update() per
form, ALTERNATING the forms, each on a fresh posterior sample of the same tables; the kernel time is the HIP-event time of the
round's k_vi_discounted_dense (CMDP_STAT_PSRL_VI_KERNEL_MS), reported per round with the round's summed sweeps and the
schemes the rule picked.  Then --steps steps of run() per form on fresh equal batches: wall time ending in the call's
synchronisation, rounds and solves.  No ratio is asserted anywhere.  JSON goes to --out/k13_psrlc.json, one entry per batch."""
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
from colosseum_amd.agents import BatchedPSRLContinuous  # noqa: E402
from colosseum_amd.batched import BatchedMDP  # noqa: E402
from colosseum_amd.mdp import make_model  # noqa: E402

BATCHES = {   # FrozenLakeContinuous size -> instances
    "frozenlake5": (5, 256),
    "frozenlake10": (10, 128),
    "frozenlake20": (20, 64),
}
FORMS = {"workgroup_4_waves": None, "one_wavefront": "1"}


def set_form(form):
    if FORMS[form] is None:
        os.environ.pop("CMDP_DDV_WAVES", None)
    else:
        os.environ["CMDP_DDV_WAVES"] = FORMS[form]


def make_agent(name):
    size, B = BATCHES[name]
    base = [make_model("FrozenLakeContinuous", seed=s, size=size, p_frozen=0.9) for s in range(4)]
    env = BatchedMDP([base[b % 4] for b in range(B)], rng_mode=L.RNG_PHILOX, philox_keys=np.arange(B, dtype=np.uint64) * 7919 + 5)
    env.reset()
    return env, BatchedPSRLContinuous(env, np.arange(B), 10 ** 6, sampler="philox", no_optimistic_sampling=True)


def time_batch(name, args):
    res = dict(batch=name, forms={})
    env, agent = make_agent(name)
    res.update(B=env.B, S=[int(s) for s in sorted(set(env.n_states.tolist()))], A=env.A)
    for form in FORMS:   # warm-up: both forms' code objects
        set_form(form)
        agent.episode_end_update()
    rounds = {form: [] for form in FORMS}
    for _ in range(args.reps):
        for form in FORMS:
            set_form(form)
            agent.episode_end_update()
            st, ls = agent.stats(), agent.last_sample()
            rounds[form].append(dict(vi_kernel_ms=st["vi_kernel_ms"], sample_kernel_ms=st["sample_kernel_ms"], sweeps=st["sweeps"],
                                     jacobi=int((ls["scheme"] == L.SCHEME_JACOBI).sum()), unconverged=int((ls["status"] != 0).sum())))
            # the other form on the same sample: the same bits
            other = [f for f in FORMS if f != form][0]
            set_form(other)
            b = 0
            (Q, _, n, _), = dp.discounted_value_iteration_dense_batch([(ls["T"][b], ls["R"][b])])
            assert np.array_equal(Q, ls["Q"][b]) and n == ls["sweeps"][b], (name, form)
    env.close()
    for form in FORMS:
        set_form(form)
        env, agent = make_agent(name)
        t = time.perf_counter()
        agent.run(args.steps)
        run_s = time.perf_counter() - t
        st = agent.stats()
        ms = [r["vi_kernel_ms"] for r in rounds[form]]
        res["forms"][form] = dict(rounds=rounds[form], vi_kernel_ms_min=min(ms), vi_kernel_ms_median=float(np.median(ms)),
                                  run_steps=args.steps, run_s=run_s, steps_per_s=env.B * args.steps / run_s,
                                  run_rounds=st["rounds"] - 1, run_solves=st["solves"] - env.B)
        env.close()
    set_form("workgroup_4_waves")
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--batch", default="all", choices=sorted(BATCHES) + ["all"])
    ap.add_argument("--reps", type=int, default=5, help="timed rounds per form, alternating")
    ap.add_argument("--steps", type=int, default=200, help="steps of the timed run() per form")
    args = ap.parse_args()
    if L.load().cmdp_device_count() == 0:
        raise SystemExit("no HIP device visible: times are taken on the GPU only")
    os.makedirs(args.out, exist_ok=True)
    names = sorted(BATCHES, key=lambda n: BATCHES[n][0]) if args.batch == "all" else [args.batch]   # the small batch first
    res = {name: time_batch(name, args) for name in names}
    with open(os.path.join(args.out, "k13_psrlc.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
