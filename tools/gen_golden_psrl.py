"""Writes tests/golden/G20_psrl.npz: the reference's PSRLEpisodic (colosseum/agent/agents/episodic/posterior_sampling.py
with BayesianMDPModel, N_NIG and M_DIR) driven as MDPLoop.run drives it (colosseum/experiment/agent_mdp_interaction.py:
224-298: reset, before_start_interacting, then per step select_action -> step -> step_update -> is_episode_end ->
episode_end_update, and reset() after a last step) on small episodic MDPs.

Runs on a development box that has the reference tree (oracle/ref_env.install()), never on the GPU box.  Recorded, data
only: per step (h, s, a, s', last) and the reward; per episode the Q [H + 1, S, A] the agent installed and the SHA-256 of
the bytes of the sampled T and R; for a thin subset of episodes (the first three, every fiftieth, the last) T and R
themselves; the final hyper-parameters of both models; the reference's own steps per second on one core.

    python tools/gen_golden_psrl.py [out.npz]"""
import hashlib
import importlib
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)

import ref_env  # noqa: E402

np = ref_env.install()

# (reference class, module, parameters, rewards_prior_prms, transitions_prior_prms, steps); None: the reference's defaults
CASES = [
    ("DeepSeaEpisodic", "deep_sea", dict(seed=0, size=3), None, None, 1500),
    ("RiverSwimEpisodic", "river_swim", dict(seed=2, size=6), [0.6, 2, 1.5, 3], [0.3], 1500),
    ("SimpleGridEpisodic", "simple_grid", dict(seed=4, size=3, n_starting_states=3), None, [1.7], 1500),
    ("DeepSeaEpisodic", "deep_sea", dict(seed=5, size=4, make_reward_stochastic=True, reward_variance_multiplier=0.7),
     None, None, 1500),
    ("FrozenLakeEpisodic", "frozen_lake", dict(seed=6, size=3, p_frozen=0.9, p_rand=0.1, make_reward_stochastic=True),
     [1.0, 1, 2, 2], None, 1500),
]


def import_reference_psrl():
    """The agents packages' __init__ files import TensorFlow agents: register bare packages with the real __path__ and
    import the tabular agent's module directly (as tools/gen_golden_ucrl2.py does)."""
    base = os.path.join(ref_env.REFERENCE, "colosseum", "agent")
    import colosseum.agent  # noqa: F401

    for sub in ("agents", "agents.episodic"):
        name = "colosseum.agent." + sub
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                m = types.ModuleType(name)
                m.__path__ = [os.path.join(base, *sub.split("."))]
                sys.modules[name] = m
    from colosseum.agent.agents.episodic import posterior_sampling

    return posterior_sampling


def sha(T, R):
    return hashlib.sha256(np.ascontiguousarray(T).tobytes() + np.ascontiguousarray(R).tobytes()).hexdigest()


def main(out):
    from colosseum.agent.mdp_models.bayesian_models import RewardsConjugateModel, TransitionsConjugateModel
    from colosseum.utils.acme.specs import make_mdp_spec

    ps = import_reference_psrl()
    arrays, meta = {}, []
    for i, (cls, mod, kw, rprm, tprm, T) in enumerate(CASES):
        mdp = getattr(importlib.import_module("colosseum.mdp." + mod), cls)(**kw)
        agent = ps.PSRLEpisodic(
            seed=kw["seed"], mdp_specs=make_mdp_spec(mdp), optimization_horizon=T,
            reward_prior_model=None if rprm is None else RewardsConjugateModel.N_NIG,
            transitions_prior_model=None if tprm is None else TransitionsConjugateModel.M_DIR,
            rewards_prior_prms=rprm, transitions_prior_prms=tprm)
        solves = []
        real_vi = ps.episodic_value_iteration

        def vi(H, T_, R_, _log=solves):
            Q, V = real_vi(H, T_, R_)
            _log.append(dict(T=np.array(T_), R=np.array(R_), Q=np.array(Q)))
            return Q, V

        ps.episodic_value_iteration = vi
        steps = np.zeros((T, 5), np.int32)
        rewards = np.zeros(T, np.float64)
        reward_types = set()
        t0 = time.perf_counter()
        try:
            ts = mdp.reset()
            agent.before_start_interacting()
            for t in range(T):
                h = mdp.h
                a = agent.select_action(ts, h)
                new_ts = mdp.step(a)
                agent.step_update(ts, a, new_ts, h)
                if agent.is_episode_end(ts, a, new_ts, h):
                    agent.episode_end_update()
                steps[t] = (h, ts.observation, a, new_ts.observation, int(new_ts.last()))
                rewards[t] = new_ts.reward
                reward_types.add(type(new_ts.reward).__name__)
                ts = new_ts
                if new_ts.last():
                    ts = mdp.reset()
        finally:
            ps.episodic_value_iteration = real_vi
        dt = time.perf_counter() - t0
        rm, tm = agent._mdp_model._rewards_model, agent._mdp_model._transitions_model
        S, A = tm.hyper_params.shape[:2]
        H = int(agent._time_horizon)
        assert rm.hyper_params.dtype == np.float32 and tm.hyper_params.dtype == np.float32
        assert all(s["T"].dtype == np.float32 and s["R"].dtype == np.float32 and s["Q"].dtype == np.float32 for s in solves)
        n = len(solves)
        assert n == int(steps[:, 4].sum()) + 1
        kept = sorted(set([0, 1, 2, n - 1] + list(range(0, n, 50))) & set(range(n)))
        p = f"c{i}_"
        arrays[p + "steps"], arrays[p + "rewards"] = steps, rewards
        arrays[p + "Q"] = np.stack([s["Q"] for s in solves])
        arrays[p + "sha"] = np.array([sha(s["T"], s["R"]) for s in solves])
        arrays[p + "kept"] = np.array(kept, np.int64)
        arrays[p + "T"] = np.stack([solves[k]["T"] for k in kept])
        arrays[p + "R"] = np.stack([solves[k]["R"] for k in kept])
        arrays[p + "final_reward_hp"], arrays[p + "final_transition_hp"] = rm.hyper_params, tm.hyper_params
        meta.append(dict(cls=cls, params=kw, seed=kw["seed"], S=int(S), A=int(A), H=H, T=T, rewards_prior_prms=rprm,
                         transitions_prior_prms=tprm, r_max=float(agent._mdp_model._reward_range[1]),
                         reward_types=sorted(reward_types), n_solves=n,
                         n_start_states=int(len(np.unique(steps[steps[:, 0] == 0, 1]))),
                         reference_steps_per_second=T / dt))
        print(f"case {i}: {cls} {kw} S={S} A={A} H={H}: {n} solves, {T / dt:.0f} steps/s, reward types "
              f"{sorted(reward_types)}, start states {meta[-1]['n_start_states']}", flush=True)
    np.savez_compressed(out, cases=json.dumps(meta), **arrays)
    print(f"wrote {out}: {len(meta)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "G20_psrl.npz"))
