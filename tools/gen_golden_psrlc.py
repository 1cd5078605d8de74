"""Writes tests/golden/G22_psrlc.npz: the reference's PSRLContinuous (colosseum/agent/agents/infinite_horizon/
posterior_sampling.py with BayesianMDPModel, N_NIG and M_DIR) with no_optimistic_sampling=True, driven as MDPLoop.run drives
it (colosseum/experiment/agent_mdp_interaction.py:224-298: reset, before_start_interacting, then per step select_action ->
step -> step_update -> is_episode_end -> episode_end_update; the environment is never reset) on small continuous MDPs.

Runs on a development box that has the reference tree (oracle/ref_env.install()), never on the GPU box.  Recorded, data
only: per step (s, a, s', ended) and the reward; per solve the Q [S, A] the agent installed and the SHA-256 of the bytes of
the sampled T and R; for a thin subset of solves (the first three, every fiftieth, the last) T and R themselves; the final
hyper-parameters of both models and N.sum(-1); the reference's own steps per second on one core.

    python tools/gen_golden_psrlc.py [out.npz]"""
import hashlib
import importlib
import json
import os
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import ref_env  # noqa: E402

np = ref_env.install()

STEPS = 600
# (reference class, module, parameters, rewards_prior_prms, transitions_prior_prms); None: the reference's defaults
CASES = [
    ("RiverSwimContinuous", "river_swim", dict(seed=0, size=5), None, None),
    ("DeepSeaContinuous", "deep_sea", dict(seed=1, size=4, make_reward_stochastic=True, reward_variance_multiplier=0.7), None, None),
    ("FrozenLakeContinuous", "frozen_lake", dict(seed=2, size=3, p_frozen=0.9), [1.0, 1, 2, 2], [0.3]),
    ("SimpleGridContinuous", "simple_grid", dict(seed=3, size=3), None, [1.7]),
    # a small prior: float32 gamma variates underflow to exactly 0, with probability about exp(-104 * prior) per element.
    # At 0.02 that is one element in eight, so the samples hold zeros but a row of 16 zeros has probability 3e-15 ...
    ("FrozenLakeContinuous", "frozen_lake", dict(seed=4, size=4, p_frozen=0.9), None, [0.02]),
    # ... at 0.001 it is nine in ten and a row in six is the zero row, until its pair has been visited
    ("FrozenLakeContinuous", "frozen_lake", dict(seed=5, size=4, p_frozen=0.9), None, [0.001]),
]
ZEROS_CASE, ZERO_ROWS_CASE = 4, 5


def import_reference_psrlc():
    """The agents packages' __init__ files import TensorFlow agents: register bare packages with the real __path__ and
    import the tabular agent's module directly (as tools/gen_golden_psrl.py does)."""
    base = os.path.join(ref_env.REFERENCE, "colosseum", "agent")
    import colosseum.agent  # noqa: F401

    for sub in ("agents", "agents.infinite_horizon"):
        name = "colosseum.agent." + sub
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                m = types.ModuleType(name)
                m.__path__ = [os.path.join(base, *sub.split("."))]
                sys.modules[name] = m
    from colosseum.agent.agents.infinite_horizon import posterior_sampling

    return posterior_sampling


def sha(T, R):
    return hashlib.sha256(np.ascontiguousarray(T).tobytes() + np.ascontiguousarray(R).tobytes()).hexdigest()


def main(out):
    from colosseum.agent.mdp_models.bayesian_models import RewardsConjugateModel, TransitionsConjugateModel
    from colosseum.utils.acme.specs import make_mdp_spec

    ps = import_reference_psrlc()
    out = os.path.abspath(out)
    os.chdir(tempfile.mkdtemp())   # the reference's MDPs write their hardness cache into the working directory
    arrays, meta = {}, []
    for i, (cls, mod, kw, rprm, tprm) in enumerate(CASES):
        mdp = getattr(importlib.import_module("colosseum.mdp." + mod), cls)(**kw)
        agent = ps.PSRLContinuous(
            seed=kw["seed"], mdp_specs=make_mdp_spec(mdp), optimization_horizon=STEPS,
            reward_prior_model=None if rprm is None else RewardsConjugateModel.N_NIG,
            transitions_prior_model=None if tprm is None else TransitionsConjugateModel.M_DIR,
            rewards_prior_prms=rprm, transitions_prior_prms=tprm, no_optimistic_sampling=True)
        solves = []
        real_vi = ps.discounted_value_iteration

        def vi(T_, R_, _log=solves):
            Q, V = real_vi(T_, R_)
            _log.append(dict(T=np.array(T_), R=np.array(R_), Q=np.array(Q)))
            return Q, V

        ps.discounted_value_iteration = vi
        steps = np.zeros((STEPS, 4), np.int32)
        rewards = np.zeros(STEPS, np.float64)
        reward_types = set()
        t0 = time.perf_counter()
        try:
            ts = mdp.reset()
            agent.before_start_interacting()
            for t in range(STEPS):
                a = agent.select_action(ts, t)
                new_ts = mdp.step(a)
                agent.step_update(ts, a, new_ts, t)
                ended = agent.is_episode_end(ts, a, new_ts, t)
                if ended:
                    agent.episode_end_update()
                assert not new_ts.last()
                steps[t] = (ts.observation, a, new_ts.observation, int(ended))
                rewards[t] = new_ts.reward
                reward_types.add(type(new_ts.reward).__name__)
                ts = new_ts
        finally:
            ps.discounted_value_iteration = real_vi
        dt = time.perf_counter() - t0
        rm, tm = agent._mdp_model._rewards_model, agent._mdp_model._transitions_model
        S, A = tm.hyper_params.shape[:2]
        assert rm.hyper_params.dtype == np.float32 and tm.hyper_params.dtype == np.float32
        assert all(s["T"].dtype == np.float32 and s["R"].dtype == np.float32 and s["Q"].dtype == np.float32 for s in solves)
        n = len(solves)
        assert n == int(steps[:, 3].sum()) + 1 and n > 1 and int(steps[:, 3].sum()) < STEPS
        zeros = int(sum((s["T"] == 0).sum() for s in solves))
        zero_rows = int(sum((s["T"].sum(-1) == 0).sum() for s in solves))
        if i == ZEROS_CASE:
            assert zeros > 0, zeros
        if i == ZERO_ROWS_CASE:
            assert zeros > 0 and zero_rows > 0, (zeros, zero_rows)
        kept = sorted(set([0, 1, 2, n - 1] + list(range(0, n, 50))) & set(range(n)))
        if i == ZERO_ROWS_CASE:   # ... and a sample with a zero row among those kept
            kept = sorted(set(kept) | {next(k for k, s in enumerate(solves) if (s["T"].sum(-1) == 0).any())})
        p = f"c{i}_"
        arrays[p + "steps"], arrays[p + "rewards"] = steps, rewards
        arrays[p + "Q"] = np.stack([s["Q"] for s in solves])
        arrays[p + "sha"] = np.array([sha(s["T"], s["R"]) for s in solves])
        arrays[p + "nnz"] = np.array([int((s["T"] != 0).sum()) for s in solves], np.int64)
        arrays[p + "kept"] = np.array(kept, np.int64)
        arrays[p + "T"] = np.stack([solves[k]["T"] for k in kept])
        arrays[p + "R"] = np.stack([solves[k]["R"] for k in kept])
        arrays[p + "final_reward_hp"], arrays[p + "final_transition_hp"] = rm.hyper_params, tm.hyper_params
        arrays[p + "final_N_sa"] = agent.N.sum(-1).astype(np.int32)
        meta.append(dict(cls=cls, params=kw, seed=kw["seed"], S=int(S), A=int(A), T=STEPS, rewards_prior_prms=rprm,
                         transitions_prior_prms=tprm, r_max=float(agent._mdp_model._reward_range[1]),
                         reward_types=sorted(reward_types), n_solves=n, zeros=zeros, zero_rows=zero_rows,
                         reference_steps_per_second=STEPS / dt))
        print(f"case {i}: {cls} {kw} S={S} A={A}: {n} solves, {zeros} zeros, {zero_rows} zero rows, {STEPS / dt:.0f} steps/s, "
              f"reward types {sorted(reward_types)}", flush=True)
    np.savez_compressed(out, cases=json.dumps(meta), **arrays)
    print(f"wrote {out}: {len(meta)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "G22_psrlc.npz"))
