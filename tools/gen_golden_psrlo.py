"""Writes tests/golden/G23_psrlo.npz: the reference's PSRLContinuous (colosseum/agent/agents/infinite_horizon/
posterior_sampling.py) on its DEFAULT path, optimistic sampling with psi extended actions per real action, driven as
MDPLoop.run drives it (reset, before_start_interacting, then per step select_action -> step -> step_update -> is_episode_end
-> episode_end_update; the environment is never reset) on small continuous MDPs.

Runs on a development box that has the reference tree (oracle/ref_env.install()), never on the GPU box.  Recorded, data only:
per step (s, a_real, s', ended), the extended action and the reward; per solve the SHA-256 of the bytes of T_ext and R_ext,
the count of non-zero elements of T_ext, the z drawn (-1: none), n1 / n2 (posterior / simple rows) and the Q [S, A * psi] the
agent installed; for a thin subset of solves (the first three, the first mixed, the first all-posterior, the last) T_ext and R
themselves -- not for the 43-state case; at the end both hyper-parameter arrays and N, the reference's psi and eta, and its
own steps per second on one core.  The properties the cases were chosen for are asserted, so a regenerated golden cannot lose
them.

    python tools/gen_golden_psrlo.py [out.npz]"""
import hashlib
import importlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ref_env  # noqa: E402

np = ref_env.install()

from gen_golden_psrlc import import_reference_psrlc  # noqa: E402

# (reference class, module, parameters, agent keywords, steps, what the case must show)
CASES = [
    ("RiverSwimContinuous", "river_swim", dict(seed=0, size=5), dict(), 600,
     dict(S=5, A=2, psi=26, eta=50, n_solves=36, mixed=3, scheme="gauss_seidel", one_posterior_row=3, simple_nonzero=49)),
    ("RiverSwimContinuous", "river_swim", dict(seed=6, size=4), dict(eta_weight=1e-10, max_psi=5), 600,
     dict(S=4, A=2, psi=5, eta=5, n_solves=32, mixed=10, all_posterior=7, all_simple=15)),
    ("DeepSeaContinuous", "deep_sea", dict(seed=1, size=4, make_reward_stochastic=True, reward_variance_multiplier=0.7),
     dict(psi_weight=0.05), 600, dict(S=10, A=2, psi=2, eta=100, n_solves=46, mixed=0, all_posterior=0)),
    ("FrozenLakeContinuous", "frozen_lake", dict(seed=2, size=3, p_frozen=0.9), dict(eta_weight=1e-10, max_psi=3), 600,
     dict(S=9, A=4, psi=3, eta=5, n_solves=106, mixed=72)),
    ("SimpleGridContinuous", "simple_grid", dict(seed=3, size=3), dict(max_psi=7, eta_weight=2e-6), 600,
     dict(S=9, A=5, psi=7, eta=5, n_solves=154, mixed=121, gauss_left_over=True)),
    ("FrozenLakeContinuous", "frozen_lake", dict(seed=7, size=7, p_frozen=0.9), dict(), 60,
     dict(S=43, A=4, psi=60, eta=430, n_solves=36, scheme="jacobi")),
]
NO_SAMPLES = 5   # the 43-state case: hashes, nnz and Q only


class LoggedStream:
    """The agent's RandomState with its randint calls recorded."""

    def __init__(self, rng, log):
        self._rng, self._log = rng, log

    def randint(self, *a, **k):
        v = self._rng.randint(*a, **k)
        self._log.append(int(v))
        return v

    def __getattr__(self, name):
        return getattr(self._rng, name)


def sha(T, R):
    return hashlib.sha256(np.ascontiguousarray(T).tobytes() + np.ascontiguousarray(R).tobytes()).hexdigest()


def main(out):
    from colosseum.utils.acme.specs import make_mdp_spec

    ps = import_reference_psrlc()
    out = os.path.abspath(out)
    os.chdir(tempfile.mkdtemp())   # the reference's MDPs write their hardness cache into the working directory
    arrays, meta = {}, []
    for i, (cls, mod, kw, akw, STEPS, want) in enumerate(CASES):
        mdp = getattr(importlib.import_module("colosseum.mdp." + mod), cls)(**kw)
        agent = ps.PSRLContinuous(seed=kw["seed"], mdp_specs=make_mdp_spec(mdp), optimization_horizon=STEPS, **akw)
        assert not agent.no_optimistic_sampling
        S, A, psi = agent._n_states, agent._n_actions, agent.psi
        zlog, extended, solves = [], [], []
        agent._rng = LoggedStream(agent._rng, zlog)
        to_real = agent.extended_action_to_real
        agent.extended_action_to_real = lambda j: (extended.append(int(j)), to_real(j))[1]
        real_vi = ps.discounted_value_iteration

        def vi(T_, R_, _log=solves):
            Q, V = real_vi(T_, R_)
            n2 = int((agent.N.sum(-1) < agent.eta).sum())
            z = list(zlog[-psi:]) if n2 else []
            assert len(z) == (psi if n2 else 0)
            _log.append(dict(T=np.array(T_), R_ext=np.array(R_), Q=np.array(Q), z=z + [-1] * (psi - len(z)), n=(S * A - n2, n2),
                             simple=agent.N.sum(-1) < agent.eta))
            return Q, V

        ps.discounted_value_iteration = vi
        steps = np.zeros((STEPS, 4), np.int32)
        rewards = np.zeros(STEPS, np.float64)
        ties = 0
        t0 = time.perf_counter()
        try:
            ts = mdp.reset()
            agent.before_start_interacting()
            for t in range(STEPS):
                q = solves[-1]["Q"][ts.observation]
                ties += int((q == q.max()).sum() > 1)
                a = agent.select_action(ts, t)
                new_ts = mdp.step(a)
                agent.step_update(ts, a, new_ts, t)
                ended = agent.is_episode_end(ts, a, new_ts, t)
                if ended:
                    agent.episode_end_update()
                assert not new_ts.last() and type(new_ts.reward) is float
                steps[t] = (ts.observation, a, new_ts.observation, int(ended))
                rewards[t] = new_ts.reward
                ts = new_ts
        finally:
            ps.discounted_value_iteration = real_vi
        dt = time.perf_counter() - t0
        rm, tm = agent._mdp_model._rewards_model, agent._mdp_model._transitions_model
        n = len(solves)
        assert len(extended) == STEPS and n == int(steps[:, 3].sum()) + 1
        assert all(s["T"].dtype == np.float32 and s["R_ext"].dtype == np.float32 and s["Q"].dtype == np.float32 for s in solves)
        assert all(s["T"].shape == (S, A * psi, S) and s["Q"].shape == (S, A * psi) for s in solves)
        assert all(np.array_equal(s["R_ext"][:, j], s["R_ext"][:, j % A]) for s in solves for j in range(A * psi))
        assert (np.array(extended) // psi == steps[:, 1]).all()
        kinds = ["mixed" if a and b else "all_posterior" if a else "all_simple" for a, b in (s["n"] for s in solves)]
        count = {k: kinds.count(k) for k in ("mixed", "all_posterior", "all_simple")}
        nnz = np.array([int((s["T"] != 0).sum()) for s in solves], np.int64)
        size = S * A * psi * S
        jacobi = [bool(size > 300 * 3 * 300 and k / size < 0.2) for k in nnz]
        # simple rows whose P_minus is not all zero: at some k more than the one element at z is non-zero
        simple_nonzero = int(sum((((s["T"].reshape(S, A, psi, S) != 0).sum(-1).max(-1) > 1) & s["simple"]).sum() for s in solves))
        got = dict(simple_nonzero=simple_nonzero, S=S, A=A, psi=psi, eta=agent.eta, n_solves=n, mixed=count["mixed"], all_posterior=count["all_posterior"],
                   all_simple=count["all_simple"], scheme="jacobi" if all(jacobi) else "gauss_seidel" if not any(jacobi) else "both",
                   one_posterior_row=sum(s["n"][0] == 1 for s in solves), gauss_left_over=bool(agent._rng.get_state()[3]))
        for k, v in want.items():
            assert got[k] == v, (i, k, got[k], v)
        kept = {0, 1, 2, n - 1}
        for kind in ("mixed", "all_posterior"):
            if kind in kinds:
                kept.add(kinds.index(kind))
        kept = sorted(kept) if i != NO_SAMPLES else []
        p = f"c{i}_"
        arrays[p + "steps"], arrays[p + "rewards"] = steps, rewards
        arrays[p + "extended"] = np.array(extended, np.int32)
        arrays[p + "Q"] = np.stack([s["Q"] for s in solves])
        arrays[p + "sha"] = np.array([sha(s["T"], s["R_ext"]) for s in solves])
        arrays[p + "nnz"] = nnz
        arrays[p + "z"] = np.array([s["z"] for s in solves], np.int32)
        arrays[p + "n12"] = np.array([s["n"] for s in solves], np.int32)
        arrays[p + "kept"] = np.array(kept, np.int64)
        if kept:
            arrays[p + "T"] = np.stack([solves[k]["T"] for k in kept])
            arrays[p + "R"] = np.stack([solves[k]["R_ext"][:, :A] for k in kept])
        arrays[p + "final_reward_hp"], arrays[p + "final_transition_hp"] = rm.hyper_params, tm.hyper_params
        arrays[p + "final_N"] = agent.N.astype(np.int32)
        meta.append(dict(cls=cls, params=kw, agent_params=akw, seed=kw["seed"], S=int(S), A=int(A), T=STEPS, psi=int(psi),
                         eta=float(agent.eta), omega=float(agent.omega), r_max=float(agent._mdp_model._reward_range[1]),
                         n_solves=n, calls=count, tie_broken_steps=ties, simple_rows_with_nonzero_p_minus=simple_nonzero,
                         scheme=got["scheme"], one_posterior_row=got["one_posterior_row"], gauss_left_over=got["gauss_left_over"],
                         reference_steps_per_second=STEPS / dt))
        print(f"case {i}: {cls} {kw} {akw} S={S} A={A} psi={psi} eta={agent.eta}: {n} solves {count}, {ties} tie-broken steps, "
              f"{simple_nonzero} simple rows with non-zero P_minus, {got['scheme']}, {STEPS / dt:.0f} steps/s", flush=True)
    np.savez_compressed(out, cases=json.dumps(meta), **arrays)
    print(f"wrote {out}: {len(meta)} cases, {os.path.getsize(out)} bytes")
    assert os.path.getsize(out) <= 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "G23_psrlo.npz"))
