"""Writes tests/golden/G21_psrl_map.npz: what the reference's PSRLEpisodic reports as its current best policy
(colosseum/agent/agents/episodic/posterior_sampling.py:78-82: get_map_estimate -> episodic_value_iteration -> argmax_3d)
at three stages of a run driven as MDPLoop.run drives it -- on the prior (episode 0), after a few and after a few dozen
episodes -- on four of golden G20's small MDPs.

Runs on a development box that has the reference tree (oracle/ref_env.install()), never on the GPU box.  Recorded, data
only, per case and stage: the hyper-parameters of both conjugate models, get_map_estimate() (T_map, R_map),
current_optimal_stochastic_policy() and the float32 Q of episodic_value_iteration on the MAP estimate.

    python tools/gen_golden_psrl_map.py [out.npz]"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import gen_golden_psrl as g20  # noqa: E402  (installs the reference through oracle/ref_env)

np = g20.np
CASES = [g20.CASES[i] for i in (0, 1, 2, 4)]
STAGES = (0, 3, 30)   # episodes completed when the stage is recorded


def main(out):
    from colosseum.agent.mdp_models.bayesian_models import RewardsConjugateModel, TransitionsConjugateModel
    from colosseum.utils.acme.specs import make_mdp_spec

    ps = g20.import_reference_psrl()
    arrays, meta = {}, []
    for i, (cls, mod, kw, rprm, tprm, T) in enumerate(CASES):
        mdp = getattr(importlib.import_module("colosseum.mdp." + mod), cls)(**kw)
        agent = ps.PSRLEpisodic(
            seed=kw["seed"], mdp_specs=make_mdp_spec(mdp), optimization_horizon=T,
            reward_prior_model=None if rprm is None else RewardsConjugateModel.N_NIG,
            transitions_prior_model=None if tprm is None else TransitionsConjugateModel.M_DIR,
            rewards_prior_prms=rprm, transitions_prior_prms=tprm)
        rm, tm = agent._mdp_model._rewards_model, agent._mdp_model._transitions_model
        H = int(agent._time_horizon)

        def record(stage, steps):
            T_map, R_map = agent._mdp_model.get_map_estimate()
            Q, _ = ps.episodic_value_iteration(H, T_map, R_map)
            pol = agent.current_optimal_stochastic_policy
            pol = pol() if callable(pol) else pol
            assert T_map.dtype == np.float32 and R_map.dtype == np.float32 and Q.dtype == np.float32
            p = f"c{i}_e{stage}_"
            arrays[p + "reward_hp"], arrays[p + "transition_hp"] = np.array(rm.hyper_params), np.array(tm.hyper_params)
            arrays[p + "T_map"], arrays[p + "R_map"] = np.array(T_map), np.array(R_map)
            arrays[p + "Q"], arrays[p + "policy"] = np.array(Q), np.array(pol, np.float32)
            return dict(episodes=stage, steps=steps)

        ts = mdp.reset()
        agent.before_start_interacting()
        stages, episodes, t = [record(0, 0)], 0, 0
        while episodes < STAGES[-1]:
            h = mdp.h
            a = agent.select_action(ts, h)
            new_ts = mdp.step(a)
            agent.step_update(ts, a, new_ts, h)
            if agent.is_episode_end(ts, a, new_ts, h):
                agent.episode_end_update()
            t += 1
            ts = new_ts
            if new_ts.last():
                ts = mdp.reset()
                episodes += 1
                if episodes in STAGES:
                    stages.append(record(episodes, t))
        S, A = tm.hyper_params.shape[:2]
        meta.append(dict(cls=cls, params=kw, seed=kw["seed"], S=int(S), A=int(A), H=H, rewards_prior_prms=rprm,
                         transitions_prior_prms=tprm, stages=stages))
        print(f"case {i}: {cls} {kw} S={S} A={A} H={H}: stages {stages}", flush=True)
    np.savez_compressed(out, cases=json.dumps(meta), **arrays)
    print(f"wrote {out}: {len(meta)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "G21_psrl_map.npz"))
