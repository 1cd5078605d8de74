"""Kernel K14 (k_vi_model) on the device: cmdp_vi_discounted_model against the CPU oracle bit for bit -- Q, V, sweeps and the
scheme taken, no tolerance anywhere -- on the generated shapes of tests/helpers_model_vi.py with each scheme forced and
under AUTO, the AUTO edges inside one mixed batch, max_sweeps per instance, repeatability, the refusals; then the UCRL2
agent's policy(), policy_solve() and average_reward() against the host route on the agent's own model."""
import ctypes as C

import numpy as np
import pytest

import helpers_model_vi as H
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp
from colosseum_amd.agents import BatchedUCRL2Continuous
from colosseum_amd.batched import BatchedMDP
from colosseum_amd.mdp import make_model

pytestmark = pytest.mark.gpu

J, G = L.SCHEME_JACOBI, L.SCHEME_GAUSS_SEIDEL


def check(fixtures, got, gamma, schemes, **ref_kw):
    for fx, (Q, V, sw, used, status), scheme in zip(fixtures, got, schemes):
        rQ, rV, it = fx.reference(gamma, scheme, **ref_kw)
        assert used == scheme, (fx.name, gamma, used, scheme)
        assert status == L.OK and sw == it, (fx.name, gamma, scheme, sw, it)
        assert np.array_equal(V, rV), (fx.name, gamma, scheme, np.flatnonzero(V != rV)[:5])
        assert np.array_equal(Q, rQ), (fx.name, gamma, scheme, np.flatnonzero(Q != rQ)[:5])


@pytest.mark.parametrize("gamma", H.GAMMAS)
@pytest.mark.parametrize("scheme", [J, G, L.SCHEME_AUTO], ids=["jacobi", "gauss_seidel", "auto"])
def test_generated_shapes_equal_the_oracle(need_gpu, scheme, gamma):
    fixtures = [fx for fx, g in H.grid() if g == gamma]
    assert len(fixtures) >= 40
    got = H.solve(fixtures, gamma=gamma, scheme=scheme)
    check(fixtures, got, gamma, [scheme or fx.rule() for fx in fixtures])


def test_auto_on_both_sides_of_the_size_edge_and_of_the_density_edge(need_gpu):
    thr, dens = H.EDGE_THRESHOLDS
    batch = H.edge_batch()
    fixtures, meant = [fx for fx, _ in batch], [m for _, m in batch]
    got = H.solve(fixtures, size_threshold=thr, density_threshold=dens)
    check(fixtures, got, 0.99, meant)
    # the same batch at the default thresholds: none is above the size edge
    check(fixtures, H.solve(fixtures), 0.99, [G] * len(fixtures))


def test_max_sweeps_per_instance_alone_in_a_batch_and_repeated(need_gpu):
    pick = {"S65_A5_every_other_state", "S64_A2_one_action", "S63_A5_two_c", "S2_A5_all_uniform", "S65_A2_no_uniform",
            "S257_A2_state_last"}
    fixtures = [H.make_fixture(S, A, mix, 9000 + i) for i, (S, A, mix) in enumerate(
        (S, A, mix) for S in H.STATES for A in H.ACTIONS for mix in H.MIXES) if f"S{S}_A{A}_{mix}" in pick]
    assert len(fixtures) == len(pick)
    gamma = 0.9
    for scheme in (J, G):
        counts = [fx.reference(gamma, scheme)[2] for fx in fixtures]
        mid = int(np.argmax(counts))   # the instance that needs the most sweeps: one fewer cuts it alone
        n = counts[mid]
        assert n > 3
        # exactly the oracle's count suffices
        got = H.solve(fixtures, gamma=gamma, scheme=scheme, max_sweeps=max(fx.reference(gamma, scheme)[2] for fx in fixtures))
        check(fixtures, got, gamma, [scheme] * len(fixtures))
        alone = H.solve([fixtures[mid]], gamma=gamma, scheme=scheme, max_sweeps=n)
        check([fixtures[mid]], alone, gamma, [scheme])
        # one sweep fewer: that instance alone reports CMDP_ERR_MAX_ITER, its neighbours are what they were
        short = H.solve([fixtures[mid]], gamma=gamma, scheme=scheme, max_sweeps=n - 1)[0]
        assert short[4] == L.ERR_MAX_ITER and short[2] == n - 1 and short[3] == scheme
        others = [fx for fx in fixtures if fx.reference(gamma, scheme)[2] < n]
        mixed = others[:2] + [fixtures[mid]] + others[2:]
        assert len(others) >= 2
        res = H.solve(mixed, gamma=gamma, scheme=scheme, max_sweeps=n - 1)
        assert res[2][4] == L.ERR_MAX_ITER and res[2][2] == n - 1
        check(others, res[:2] + res[3:], gamma, [scheme] * len(others))
        # the same batch again: identical bits; the instance alone equals the instance in the middle of the batch
        again = H.solve(mixed, gamma=gamma, scheme=scheme, max_sweeps=n - 1)
        for x, y in zip(res, again):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2:] == y[2:]
        assert np.array_equal(short[0], res[2][0]) and np.array_equal(short[1], res[2][1])
        inside = H.solve(mixed, gamma=gamma, scheme=scheme)[2]
        assert np.array_equal(inside[0], alone[0][0]) and np.array_equal(inside[1], alone[0][1]) and inside[2:] == alone[0][2:]


def test_python_batch_equals_the_single_calls(need_gpu):
    fixtures = [H.make_fixture(S, A, mix, 50 + S) for S, A, mix in ((9, 2, "every_other_state"), (30, 3, "state_0"), (5, 1, "all_uniform"))]
    probs = [fx.dense() for fx in fixtures]
    res, sweeps, schemes = dp.discounted_value_iteration_batch(probs)
    for fx, (T, R), (Q, V), sw, sc in zip(fixtures, probs, res, sweeps, schemes):
        rQ, rV = dp.discounted_value_iteration(T, R)
        assert np.array_equal(Q, rQ) and np.array_equal(V, rV) and sc == G and sw == fx.reference(0.99, G)[2]
    res, sweeps, schemes = dp.discounted_value_iteration_batch(probs, sparse_n_states_threshold=0, sparse_nnz_per_threshold=0.6)
    for fx, (T, R), r, sw, sc in zip(fixtures, probs, res, sweeps, schemes):
        assert sc == fx.rule(0, 0.6)
        rQ, rV = dp.discounted_value_iteration(T, R, sparse_n_states_threshold=0, sparse_nnz_per_threshold=0.6)
        assert np.array_equal(r[0], rQ) and np.array_equal(r[1], rV)
    assert set(schemes) == {J, G}
    res, sweeps, _ = dp.discounted_value_iteration_batch(probs, scheme=J, max_sweeps=3)
    assert res == [None] * 3 and (sweeps == 3).all()


def test_refusals(need_gpu):
    for S, A, word in ((4097, 1, "4096"), (2, 65, "64")):
        rows = S * A
        args = dict(n_states=np.array([S], np.int32), n_actions=np.array([A], np.int32), ptr=np.zeros(rows + 1, np.int64), col=None,
                    val=None, uni=np.full(rows, np.float32(1.0) / np.float32(S), np.float32), R=np.zeros(rows, np.float32))
        rc, msg, _ = H.call_raw(args, 1)
        assert rc == L.ERR_UNSUPPORTED and word in msg, msg
    T = np.full((2, 65, 2), 0.5, np.float32)
    with pytest.raises(L.CmdpError) as ei:
        dp.discounted_value_iteration_batch([(T, np.zeros((2, 65), np.float32))])
    assert ei.value.code == L.ERR_UNSUPPORTED
    # the largest shape taken: 4096 states, every row uniform
    S = 4096
    fx = H.Fixture(S, 1, np.full(S, np.float32(1.0) / np.float32(S)), np.zeros(S + 1, np.int64), [], [],
                   np.full((S, 1), 0.25, np.float32), "S4096_uniform")
    for scheme in (J, G):
        check([fx], H.solve([fx], gamma=0.5, scheme=scheme), 0.5, [scheme])


# ---- the UCRL2 agent ---------------------------------------------------------------------------------------------------
def agent_models(case):
    if case == "frozen_lake":
        return [make_model("FrozenLakeContinuous", seed=i, size=4, p_frozen=0.9) for i in range(3)]
    return [make_model("DeepSeaContinuous", seed=i, size=4) for i in range(2)]


def make_agent(models, rng):
    if rng == "mt":
        env = BatchedMDP(models, rng_mode=L.RNG_MT_COMPAT)
    else:
        env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=np.arange(len(models), dtype=np.uint64) * 7919 + 5)
    env.reset()
    return env, BatchedUCRL2Continuous(env, np.arange(len(models)) + 11, 100_000, alpha_r=0.1, alpha_p=0.1)


def host_route(agent, **kw):
    """What current_optimal_stochastic_policy did on the host: model() -> discounted_value_iteration -> argmax_2d."""
    m = agent.model()
    Qs = [dp.discounted_value_iteration(P, R, **kw)[0] for P, R in zip(m["P"], m["estimated_rewards"])]
    return Qs, [dp.argmax_2d(Q) for Q in Qs]


@pytest.mark.parametrize("rng", ["mt", "philox"])
@pytest.mark.parametrize("case", ["frozen_lake", "deep_sea"])
def test_agent_policy_equals_the_host_route(need_gpu, case, rng):
    models = agent_models(case)
    env, agent = make_agent(models, rng)
    B = env.B
    v = C.c_double()
    jacobi_seen = False
    for steps in (0, 50, 550):   # fresh (every row uniform), after 50 steps, after 600 steps
        if steps:
            agent.run(steps)
        Qs, pis = host_route(agent)
        got, sol = agent.policy(), agent.policy_solve()
        assert len(got) == B and (sol["scheme"] == G).all() and (sol["sweeps"] > 0).all()
        for b in range(B):
            assert got[b].dtype == np.float32 and np.array_equal(got[b], pis[b]), (steps, b)
            assert np.array_equal(sol["Q"][b], Qs[b]), (steps, b)
        assert np.array_equal(np.concatenate([p.ravel() for p in agent.current_optimal_stochastic_policy()]),
                              np.concatenate([p.ravel() for p in pis]))
        assert agent.stats()["policy_kernel_ms"] > 0
        L.check(L.load().cmdp_stat(env._h, L.STAT_UCRL2_POLICY_KERNEL_MS, C.byref(v)))
        assert v.value > 0
        # the Jacobi branch: size threshold 0, the sparse instances fall below the density edge
        agent._set_policy_size_threshold(0)
        Qj, pj = host_route(agent, sparse_n_states_threshold=0)
        sol = agent.policy_solve()
        m = agent.model()
        want = [dp._vi_rule(P.size, np.count_nonzero(P), 0, 0.2) for P in m["P"]]
        assert sol["scheme"].tolist() == want
        jacobi_seen = jacobi_seen or J in want
        got = agent.policy()
        for b in range(B):
            assert np.array_equal(sol["Q"][b], Qj[b]) and np.array_equal(got[b], pj[b]), (steps, b)
        agent._set_policy_size_threshold(H.SIZE_THRESHOLD)
        # average reward of that policy from the current states, masked, in both orders of the chain kernel
        mask = np.arange(B) % 2 == 0
        acts = [p.argmax(1).astype(np.int32) for p in pis]
        for exact in (1, 0):
            env.set_option(L.OPT_CHAIN_EXACT_ORDER, exact)
            want_avg, _ = env.average_reward(acts, env.state()[0], mask=mask)
            got_avg = agent.average_reward(mask)
            sel = np.flatnonzero(mask)
            assert len(got_avg) == len(sel)
            for x, b in zip(got_avg, sel):
                assert type(x) is type(want_avg[b]) and x == want_avg[b], (steps, exact, b)
            full, _ = env.average_reward(acts, env.state()[0])
            assert [type(x) for x in agent.average_reward()] == [type(x) for x in full] and agent.average_reward() == full
        # outputs of masked-out instances are left as they were
        R = int(env.row_off[-1])
        pi, Q = np.full(R, 7.0, np.float32), np.full(R, 7.0, np.float32)
        sw, sc = np.full(B, -3, np.int64), np.full(B, -3, np.int32)
        L.check(L.load().cmdp_ucrl2_policy(agent._h, L.ptr(mask.astype(np.uint8)), L.ptr(pi), L.ptr(Q), L.ptr(sw), L.ptr(sc)))
        for b in range(B):
            r0, r1 = int(env.row_off[b]), int(env.row_off[b + 1])
            if mask[b]:
                assert np.array_equal(pi[r0:r1], pis[b].ravel()) and np.array_equal(Q[r0:r1], Qs[b].ravel()) and sw[b] > 0 and sc[b] == G
            else:
                assert (pi[r0:r1] == 7.0).all() and (Q[r0:r1] == 7.0).all() and sw[b] == -3 and sc[b] == -3
        assert [p.shape for p in agent.policy(mask)] == [pis[b].shape for b in np.flatnonzero(mask)]
    assert jacobi_seen   # after 600 steps the visited rows are sparse enough for the density edge
    env.close()


def test_policy_and_average_reward_do_not_touch_the_agent(need_gpu):
    models = agent_models("frozen_lake")
    (env1, a1), (env2, a2) = make_agent(models, "philox"), make_agent(models, "philox")
    for n in (40, 200, 361):
        a2.policy()
        a2.average_reward(np.array([1, 0, 1], bool))
        a2.average_reward()
        o1, o2 = a1.run(n, trace=True), a2.run(n, trace=True)
        a2.policy_solve()
        for k in ("actions", "observations", "rewards", "cumulative_reward", "steps_taken"):
            assert np.array_equal(o1[k], o2[k]), (n, k)
        m1, m2, l1, l2 = a1.model(), a2.model(), a1.last_solve(), a2.last_solve()
        for k, x in m1.items():
            for b in range(env1.B):
                assert np.array_equal(x[b], m2[k][b]), (n, k, b)
        for k, x in l1.items():
            for b in range(env1.B):
                assert np.array_equal(x[b], l2[k][b]), (n, k, b)
        assert np.array_equal(env1.state()[0], env2.state()[0])
    env1.close()
    env2.close()
