"""Writes tests/golden/G18_extended_vi.npz: inputs and the reference's own outputs of `extended_value_iteration`
(colosseum/dynamic_programming/infinite_horizon.py:67-118) on small agent-shaped problems.

Runs on a development box that has the reference tree (oracle/ref_env.install()), never on the GPU box.  Without numba
the reference runs as plain NumPy; its sweep count and the last ptp(u2 - u1) are recorded by counting its np.ptp calls
(one per sweep, one more for the returned span).  The estimated models come from seeded multinomial counts over the
families' continuous forms (some pairs unvisited: uniform rows), the bounds from UCRL2's Chernoff and Bernstein
formulas (ucrl2.py:22-31,240-308); a case is kept only when it converges well within the reference's 10**6 sweeps.

    python tools/gen_golden_evi.py [out.npz]"""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ref_env  # noqa: E402

np = ref_env.install()

from helpers_evi import agent_problem  # noqa: E402
from colosseum_amd.mdp import make_model  # noqa: E402

MAX_SWEEPS_KEPT = 20000

# (family, parameters, visits per pair, bound kind, bound scale, iteration or None, unvisited fraction)
CASES = [
    ("RiverSwimContinuous", dict(size=6), 20, "chernoff", 0.1, None, 0.3),
    ("RiverSwimContinuous", dict(size=8), 200, "bernstein", 0.1, None, 0.1),
    ("RiverSwimContinuous", dict(size=8), 5, "chernoff", 0.02, 10, 0.0),
    ("DeepSeaContinuous", dict(size=6), 30, "bernstein", 0.1, None, 0.2),
    ("DeepSeaContinuous", dict(size=8), 100, "chernoff", 0.05, 500, 0.4),
    ("FrozenLakeContinuous", dict(size=4, p_frozen=0.9, p_rand=0.1), 50, "bernstein", 0.05, None, 0.25),
    ("FrozenLakeContinuous", dict(size=5, p_frozen=0.8, p_rand=0.2), 400, "bernstein", 1.0, None, 0.1),
    ("FrozenLakeContinuous", dict(size=5, p_frozen=0.9, p_rand=0.1), 40, "chernoff", 0.03, 100, 0.3),
    ("MiniGridEmptyContinuous", dict(size=4), 10, "chernoff", 1.0, None, 0.5),
    ("MiniGridEmptyContinuous", dict(size=4), 300, "bernstein", 0.2, None, 0.2),
    ("MiniGridEmptyContinuous", dict(size=3), 50, "chernoff", 0.02, 50, 0.1),
    ("DeepSeaContinuous", dict(size=5), 1000, "bernstein", 0.05, None, 0.0),
    ("RiverSwimContinuous", dict(size=10), 2000, "bernstein", 0.1, None, 0.05),
    ("FrozenLakeContinuous", dict(size=4, p_frozen=0.9, p_rand=0.05), 3000, "chernoff", 0.01, 3000, 0.05),
]


def run_reference(evi_mod, problem):
    calls = []
    real = np

    class CountingNumpy(types.ModuleType):
        def __getattr__(self, name):
            return getattr(real, name)

        @staticmethod
        def ptp(x):
            calls.append(float(real.ptp(x)))
            return real.ptp(x)

    evi_mod.np = CountingNumpy("numpy")
    try:
        res = evi_mod.extended_value_iteration(*problem)
    finally:
        evi_mod.np = real
    return res, len(calls) - 1, calls[-2]


def main(out):
    from colosseum.dynamic_programming import infinite_horizon as ih

    arrays, meta = {}, []
    for i, (fam, kw, visits, kind, scale, it, unv) in enumerate(CASES):
        m = make_model(fam, seed=i, **kw)
        T_true, R_true = m.dense()
        P, Rh, br, bp, rmax = agent_problem(T_true, R_true, visits, 1000 + i, kind, it, scale, 1.0, unv)
        if i % 4 == 3:  # an r_max below some optimistic rewards caps r_opt
            rmax = 0.9
        res, sweeps, last_ptp = run_reference(ih, (P, Rh, br, bp, rmax))
        assert res is not None and sweeps <= MAX_SWEEPS_KEPT, (fam, sweeps)
        span, Q, V = res
        S, A = Rh.shape
        onehot = int(((P.max(-1) + bp[:, :, 0] / 2) >= 1).sum())
        print(f"case {i}: {fam} S={S} A={A} {kind} sweeps={sweeps} span={float(span):.5g} "
              f"rows with max p + beta_p0 / 2 >= 1: {onehot}", flush=True)
        for k, v in dict(T=P, R=Rh, beta_r=br, beta_p=bp, Q=Q, V=V).items():
            arrays[f"c{i}_{k}"] = np.asarray(v)
        meta.append(dict(family=fam, params=kw, S=S, A=A, kind=kind, r_max=rmax, span=float(span), sweeps=sweeps,
                         last_ptp=last_ptp, epsilon=1e-3))
    np.savez_compressed(out, cases=json.dumps(meta), **arrays)
    print(f"wrote {out}: {len(meta)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "G18_extended_vi.npz"))
