"""Writes tests/golden/G24_psrlc_gate.npz: the reference's PSRLContinuous (colosseum/agent/agents/infinite_horizon/
posterior_sampling.py) with min_steps_before_new_episode > 0, on both of its sampling paths, driven as MDPLoop.run drives it
(colosseum/experiment/agent_mdp_interaction.py:224-298: reset, before_start_interacting, then per step h = mdp.h read BEFORE the
step, select_action -> step -> step_update -> is_episode_end(ts, a, ts', h) -> episode_end_update; the environment is never
reset) for 300 steps on two small continuous MDPs of G22's.

Runs on a development box that has the reference tree (oracle/ref_env.install()), never on the GPU box.  Recorded, data only:
per step (s, a_real, s', ended, last_change after the step) and the reward; on the optimistic path the extended action; per
solve the Q the agent installed ([S, A] or [S, A * psi]).  What the cases must show is asserted, so a regenerated golden
cannot lose it.

    python tools/gen_golden_psrlc_gate.py [out.npz]"""
import importlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ref_env  # noqa: E402

np = ref_env.install()

from gen_golden_psrlc import import_reference_psrlc  # noqa: E402

STEPS = 300
MDPS = [("RiverSwimContinuous", "river_swim", dict(seed=0, size=5)),
        ("FrozenLakeContinuous", "frozen_lake", dict(seed=2, size=3, p_frozen=0.9))]
MIN_STEPS = (1, 7, 10_000)
MAX_PSI = 4


def main(out):
    from colosseum.utils.acme.specs import make_mdp_spec

    ps = import_reference_psrlc()
    out = os.path.abspath(out)
    os.chdir(tempfile.mkdtemp())   # the reference's MDPs write their hardness cache into the working directory
    arrays, meta = {}, []
    for cls, mod, kw in MDPS:
        for plain in (True, False):
            for m in MIN_STEPS:
                i = len(meta)
                mdp = getattr(importlib.import_module("colosseum.mdp." + mod), cls)(**kw)
                akw = dict(no_optimistic_sampling=True) if plain else dict(max_psi=MAX_PSI)
                agent = ps.PSRLContinuous(seed=kw["seed"], mdp_specs=make_mdp_spec(mdp), optimization_horizon=STEPS,
                                          min_steps_before_new_episode=m, **akw)
                assert agent.no_optimistic_sampling == plain and agent.last_change == 0
                S, A = agent._n_states, agent._n_actions
                extended, solves = [], []
                to_real = agent.extended_action_to_real
                agent.extended_action_to_real = lambda j: (extended.append(int(j)), to_real(j))[1]
                real_vi = ps.discounted_value_iteration

                def vi(T_, R_, _log=solves):
                    Q, V = real_vi(T_, R_)
                    _log.append(np.array(Q))
                    return Q, V

                ps.discounted_value_iteration = vi
                steps = np.zeros((STEPS, 5), np.int32)
                rewards = np.zeros(STEPS, np.float64)
                try:
                    ts = mdp.reset()
                    agent.before_start_interacting()
                    assert agent.last_change == 0   # episode_end_update does not touch it
                    for t in range(STEPS):
                        h = mdp.h
                        assert h == t
                        a = agent.select_action(ts, h)
                        new_ts = mdp.step(a)
                        agent.step_update(ts, a, new_ts, h)
                        before = agent.last_change
                        ended = agent.is_episode_end(ts, a, new_ts, h)
                        assert agent.last_change == (h if h - before >= m else before)
                        if ended:
                            agent.episode_end_update()
                        assert not new_ts.last() and type(new_ts.reward) is float
                        steps[t] = (ts.observation, a, new_ts.observation, int(ended), agent.last_change)
                        rewards[t] = new_ts.reward
                        ts = new_ts
                finally:
                    ps.discounted_value_iteration = real_vi
                n = len(solves)
                ends = int(steps[:, 3].sum())
                assert n == ends + 1 and all(q.dtype == np.float32 for q in solves)
                width = A if plain else A * agent.psi
                assert all(q.shape == (S, width) for q in solves)
                if m == 1:       # the gate suppresses step 0's first visit and nothing else
                    assert steps[0, 3] == 0 and steps[1, 3] == 1 and (steps[1:, 4] == np.arange(1, STEPS)).all()
                elif m == 7:     # a check at most every 7 steps; some pass without ending the episode
                    passed = np.flatnonzero(np.diff(np.concatenate([[0], steps[:, 4]])) > 0)
                    assert 1 <= ends <= STEPS // 7 and (np.diff(passed) >= 7).all() and len(passed) >= ends
                else:            # no check ever passes
                    assert ends == 0 and (steps[:, 4] == 0).all()
                p = f"c{i}_"
                arrays[p + "steps"], arrays[p + "rewards"] = steps, rewards
                arrays[p + "Q"] = np.stack(solves)
                if not plain:
                    assert len(extended) == STEPS and (np.array(extended) // agent.psi == steps[:, 1]).all()
                    arrays[p + "extended"] = np.array(extended, np.int32)
                meta.append(dict(cls=cls, params=kw, seed=kw["seed"], S=int(S), A=int(A), T=STEPS, min_steps=m, plain=plain,
                                 psi=None if plain else int(agent.psi), eta=None if plain else float(agent.eta),
                                 max_psi=None if plain else MAX_PSI, r_max=float(agent._mdp_model._reward_range[1]), n_solves=n))
                print(f"case {i}: {cls} {kw} plain={plain} m={m} S={S} A={A}: {n} solves", flush=True)
    np.savez_compressed(out, cases=json.dumps(meta), **arrays)
    print(f"wrote {out}: {len(meta)} cases, {os.path.getsize(out)} bytes")
    assert os.path.getsize(out) <= 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "G24_psrlc_gate.npz"))
