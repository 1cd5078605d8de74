"""Kernel K15 (csrc/cmdp_map_vi.h) on the device: `episodic_value_iteration_map_batch` on generated tables of every shape
the kernel branches on, and the PSRL agent's policy / policy_solve / evaluate on its own tables.

The reference of every Q is helpers_map_vi.restatement -- float64 value iteration on the float32 MAP estimate formed as
the reference forms it -- and the bound is helpers_psrl.bound_episodic(H, qmax, 1), as it is.  The MAP transition estimate
itself (t at the layout's positions, c elsewhere) is compared bit for bit with the host definition cmdp_psrl_map_rows,
which tests/test_map_vi.py holds against numpy's.

Stages of the agent tests.  Everything without an exclusion (Q within the bound, policy() == argmax_3d of the device's Q,
the policy greedy for the restatement up to rounding at every (h, s), evaluate() == the handle's policy evaluation of
policy()) is checked fresh and after 3 and 30 episodes and at two later stages.  Against the host route (the MAP estimate
through the library's episodic_value_iteration and argmax_3d, as current_optimal_stochastic_policy computes it) the
policies must agree at every (h, s) whose two best Q64 differ by more than twice the bound, at every stage.  The share of
(h, s) this leaves out is capped at one third per instance at the two LATER stages: rows the agent has not visited tie
exactly (same prior row, same prior mean), and layer H ties everywhere (1 / (H + 1) of all (h, s)).  On the CPU twin
(helpers_psrl.PSRLTwin on the CPU oracle's environments, 16 seeds) the host route alone left out 0.94 of FrozenLake-4's
(h, s) after 3 episodes, up to 0.66 after 30, 0.31 after 150, 0.22 after 300 and 0.21 after 600; on the ragged batch's
MDPs up to 0.86 / 0.44 after 3 / 30 and at most 0.22 from 100 episodes on.  So the cap is asserted at 300 and 600 episodes
(FrozenLake-4) and at 150 and 300 (ragged batch); at 3 and 30 episodes the share is printed (on the device: 1.0 and
0.63 for FrozenLake-4, 0.86 and 0.32-0.41 for the ragged batch; 0.27 at most where the cap is asserted)."""
import numpy as np
import pytest

import helpers_map_vi as M
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp
from colosseum_amd.agents import BatchedPSRLEpisodic
from colosseum_amd.batched import BatchedMDP
from colosseum_amd.mdp import make_model

pytestmark = pytest.mark.gpu

CAP = 1.0 / 3.0


# ---- the kernel on generated tables ----------------------------------------------------------------------------------
def shape_problems():
    """One ragged batch: S in {1, 5, 13, 70, 129, 131, 359, 600} with A in {1, 2, 4}; rows with 0, 1 and > 64 layout
    positions and a row whose layout is the whole row."""
    rng = np.random.RandomState(7)
    probs = []
    for i, (S, A) in enumerate(((1, 2), (5, 1), (13, 4), (70, 2), (129, 1), (131, 4), (359, 2), (600, 4))):
        thp, mu, prior = M.tables(S, A, seed=i)
        keep = np.zeros(thp.shape, bool)
        if S >= 5:
            thp[1, 0] = prior                                   # no position
            thp[2, A - 1] = prior
            thp[2, A - 1, S - 1] = prior + np.float32(1.0)      # one position, the last column
            thp[0, 0] = (rng.gamma(0.3, size=S) * 20 + 1e-3).astype(np.float32)
            keep[0, 0] = True                                   # the whole row
        if S >= 70:
            cols = rng.choice(S, 67, replace=False)
            thp[3, 0, cols] += rng.randint(1, 9, size=67).astype(np.float32)   # longer than a wavefront
        probs.append((thp, mu, prior, keep))
    return probs


@pytest.mark.parametrize("H", [1, 7])
def test_shapes(need_gpu, H):
    probs = shape_problems()
    outs = dp.episodic_value_iteration_map_batch(probs, H, return_map=True)
    worst = 0.0
    for (thp, mu, prior, keep), (Q, V, t, c) in zip(probs, outs):
        S, A, _ = thp.shape
        row_ptr, col, hp = dp.map_layout_from_dense(thp, prior, keep)
        n = np.diff(row_ptr)
        if S >= 5:
            assert n[0] == S and n[A] == 0 and n[2 * A + A - 1] == 1
        if S >= 70:
            assert n[3 * A] > 64
        _, c_ref, t_ref = dp.psrl_map_rows(row_ptr, col, hp, prior, S, A)
        assert np.array_equal(t, t_ref) and np.array_equal(c, c_ref), (S, A)
        worst = max(worst, M.check_solve(Q, V, thp, mu, H))
    print(f"H = {H}: worst |Q - Q64| / bound {worst:.3f}")
    # the table form of the same problems gives the same bits
    tab = [dp.map_layout_from_dense(thp, prior, keep) + (prior, mu) for thp, mu, prior, keep in probs[:4]]
    for (Q, V), (Q2, V2, _, _) in zip(dp.episodic_value_iteration_map_batch(tab, H), outs):
        assert np.array_equal(Q, Q2) and np.array_equal(V, V2)


def test_lds_limit(need_gpu):
    S, A, H = 4096, 2, 2
    rng = np.random.RandomState(3)
    prior = np.float32(1.0 / S)
    thp = np.full((S, A, S), prior, np.float32)
    rows, cols = rng.randint(S * A, size=6 * S), rng.randint(S, size=6 * S)
    np.add.at(thp.reshape(S * A, S), (rows, cols), np.float32(1.0))
    thp[5, 1] = (rng.gamma(0.3, size=S) + 1e-3).astype(np.float32)   # one full row: every run and merge of the pairwise sum
    mu = rng.uniform(size=(S, A)).astype(np.float32)
    (Q, V, t, c), = dp.episodic_value_iteration_map_batch([(thp, mu, prior)], H, return_map=True)
    row_ptr, col, hp = dp.map_layout_from_dense(thp, prior)
    _, c_ref, t_ref = dp.psrl_map_rows(row_ptr, col, hp, prior, S, A)
    assert np.array_equal(t, t_ref) and np.array_equal(c, c_ref)
    M.check_solve(Q, V, thp, mu, H)
    with pytest.raises(L.CmdpError) as e:
        dp.episodic_value_iteration_map_batch([(np.zeros(4097 * 2 + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32),
                                                prior, np.zeros((4097, 2), np.float32))], H)
    assert e.value.code == L.ERR_UNSUPPORTED


def test_staging_threshold(need_gpu):
    """An instance's tables live in LDS while 8 spad + 8 (S A + 1) + 8 S A + 8 nz <= 128 KB (csrc/cmdp_map_vi.h
    map_vi_stage_bytes) and in global memory beyond: at S = 600, A = 4 the last layout that fits has 10 983 positions.
    That one, the first that does not, and both in one launch."""
    S, A, H = 600, 4, 5
    fits = (128 * 1024 - (8 * 600 + 8 * (S * A + 1) + 8 * S * A)) // 8
    assert fits == 10983
    rng = np.random.RandomState(11)
    prior = np.float32(1.0 / S)
    mu = rng.uniform(size=(S, A)).astype(np.float32)
    probs = []
    for nz in (fits, fits + 1):
        pos = rng.choice(S * A * S, nz, replace=False)
        thp = np.full(S * A * S, prior, np.float32)
        thp[pos] += rng.randint(1, 6, size=nz).astype(np.float32)
        row_ptr, col, hp = dp.map_layout_from_dense(thp.reshape(S, A, S), prior)
        assert row_ptr[-1] == nz
        probs.append((thp.reshape(S, A, S), (row_ptr, col, hp, prior, mu)))
    alone = [dp.episodic_value_iteration_map_batch([tab], H, return_map=True)[0] for _, tab in probs]
    together = dp.episodic_value_iteration_map_batch([tab for _, tab in probs], H, return_map=True)
    for (thp, tab), one, two in zip(probs, alone, together):
        _, c_ref, t_ref = dp.psrl_map_rows(tab[0], tab[1], tab[2], prior, S, A)
        assert np.array_equal(one[2], t_ref) and np.array_equal(one[3], c_ref)
        M.check_solve(one[0], one[1], thp, mu, H)
        assert all(np.array_equal(x, y) for x, y in zip(one, two))   # the launch's other instance changes nothing


# ---- the agent ---------------------------------------------------------------------------------------------------------
def frozen_lake_models():
    return [make_model("FrozenLakeEpisodic", seed=0, size=4, p_frozen=0.9, p_rand=0.1)] * 16


def ragged_models():
    return [make_model("DeepSeaEpisodic", seed=1, size=5), M.custom_model(7, 2, 5, 7, 3), M.custom_model(23, 2, 5, 23, 70),
            make_model("DeepSeaEpisodic", seed=2, size=5, p_rand=0.2), M.custom_model(70, 2, 5, 70, 70)]


BATCHES = {"frozenlake4": (frozen_lake_models, (300, 600)), "ragged": (ragged_models, (150, 300))}


def make_env(models, with_dp=True):
    env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=np.arange(len(models), dtype=np.uint64) * 7919 + 5, with_dp=with_dp)
    env.reset()
    return env


def make_agent(models, sampler, with_dp=True):
    env = make_env(models, with_dp)
    return env, BatchedPSRLEpisodic(env, np.arange(env.B) + 11, 10 ** 6, sampler=sampler)


def check_stage(env, agent, capped):
    H = int(env.H)
    m = agent.model()
    Qs = agent.policy_solve()["Q"]
    pol = agent.policy()
    V0 = agent.evaluate()
    assert agent.stats()["policy_kernel_ms"] > 0
    shares = []
    for b in range(env.B):
        thp, rhp = m["transitions"][b], m["rewards"][b]
        Q64, _, tol = M.restatement(thp, rhp[:, :, 0], H)
        M.check_solve(Qs[b], None, thp, rhp[:, :, 0], H)
        assert np.array_equal(pol[b], dp.argmax_3d(Qs[b])), b    # the tie-break stream, draw for draw
        M.check_greedy(pol[b], Q64, tol)
        shares.append(M.compare_policies(pol[b], M.host_route(thp, rhp, H), Q64, tol))
    # evaluate(): the handle's own episodic policy evaluation of policy() on the true MDP
    _, V = env.episodic_policy_evaluation([p[:H] for p in pol])
    ref = np.concatenate([v[:int(env.n_states[b])] for b, v in enumerate(env.split_states(V, H + 1))])
    assert V0.dtype == np.float32 and np.array_equal(V0, ref)
    if capped:
        assert max(shares) <= CAP, shares
    return max(shares)


@pytest.mark.parametrize("sampler", ["reference", "philox"])
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_agent(need_gpu, batch, sampler):
    models, late = BATCHES[batch]
    env, agent = make_agent(models(), sampler)
    H = int(env.H)
    done, report = 0, {}
    for episodes in (0, 3, 30) + late:
        agent.run((episodes - done) * H)
        done = episodes
        assert (agent.model()["episode"] == episodes + 1).all()
        report[episodes] = round(check_stage(env, agent, capped=episodes in late), 3)
    print(f"{batch} / {sampler}: largest share of (h, s) left out of the host-route comparison per stage {report}")
    dp.release_handles()


def test_mask(need_gpu):
    env, agent = make_agent(ragged_models(), "philox")
    agent.run(40 * env.H)
    full_pi, full_Q, full_V0 = agent.policy(), agent.policy_solve()["Q"], env.split_states(agent.evaluate())
    mask = np.array([1, 0, 0, 1, 1], bool)
    pi, Q, V0 = agent.policy(mask), agent.policy_solve(mask)["Q"], env.split_states(agent.evaluate(mask))
    assert len(pi) == 3
    for k, b in enumerate(np.flatnonzero(mask)):
        assert np.array_equal(pi[k], full_pi[b]), b
    for b in range(env.B):
        if mask[b]:
            assert np.array_equal(Q[b], full_Q[b]) and np.array_equal(V0[b], full_V0[b]), b
        else:
            assert (Q[b] == 0).all() and (V0[b] == 0).all(), b
    assert all(np.array_equal(x, y) for x, y in zip(agent.policy(), full_pi))   # nothing of the masked call is left behind
    assert agent.policy(np.zeros(5, bool)) == []
    for bad in (np.ones(4, bool), np.ones(6, bool), np.ones((5, 1), bool)):
        with pytest.raises(AssertionError):
            agent.policy(bad)
        with pytest.raises(AssertionError):
            agent.evaluate(bad)


@pytest.mark.parametrize("sampler", ["reference", "philox"])
def test_non_interference(need_gpu, sampler):
    """run(n), evaluate(), policy(), run(n) leaves the traces, the model, the last sample and the environment where
    run(2 n) leaves them on an equal batch; one instance is out of phase (a masked reset two steps into the episode)."""

    def start():
        env = make_env(ragged_models())
        env.step(np.zeros(env.B, np.int32))
        env.step(np.ones(env.B, np.int32))
        env.reset(mask=np.array([1, 0, 1, 1, 1], bool))
        assert sorted(set(env.state()[1].tolist())) == [0, 2]
        return env, BatchedPSRLEpisodic(env, np.arange(env.B) + 3, 10 ** 6, sampler=sampler)

    n = 33   # not a multiple of the horizon: the calls in between fall inside an episode
    env1, a1 = start()
    env2, a2 = start()
    first = a1.run(n, trace=True)
    a1.evaluate()
    a1.policy()
    a1.policy_solve(np.array([0, 1, 0, 1, 0], bool))
    second = a1.run(n, trace=True)
    whole = a2.run(2 * n, trace=True)
    for k in ("actions", "observations", "rewards"):
        assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    assert np.array_equal(second["cumulative_reward"], whole["cumulative_reward"])
    m1, m2, l1, l2 = a1.model(), a2.model(), a1.last_sample(), a2.last_sample()
    for b in range(env1.B):
        for k in ("transitions", "rewards"):
            assert np.array_equal(m1[k][b], m2[k][b]), (k, b)
        for k in ("T", "R", "Q"):
            assert np.array_equal(l1[k][b], l2[k][b]), (k, b)
    assert np.array_equal(m1["episode"], m2["episode"])
    for x, y in zip(env1.state(), env2.state()):
        assert np.array_equal(x, y)
    # ... and the two agents, now in the same state, report the same policy and value
    assert all(np.array_equal(x, y) for x, y in zip(a1.policy(), a2.policy()))
    assert np.array_equal(a1.evaluate(), a2.evaluate())


def test_evaluate_needs_the_dp_half(need_gpu):
    env, agent = make_agent(ragged_models()[:2], "philox", with_dp=False)
    agent.run(3 * env.H)
    with pytest.raises(L.CmdpError) as e:
        agent.evaluate()
    assert e.value.code == L.ERR_UNSUPPORTED and "DP half" in str(e.value)
    pol = agent.policy()            # the policy itself needs the model only
    assert pol[0].shape == (env.H + 1, int(env.n_states[0]), env.A) and agent.stats()["policy_kernel_ms"] > 0
