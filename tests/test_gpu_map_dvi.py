"""Kernel K17 (k_vi_discounted_map, csrc/cmdp_map_dvi.h) on the device: the stand-alone entry
dp.discounted_value_iteration_map_batch on the generated ragged batches of tests/helpers_map_dvi.py (which tests/test_map_dvi.py
holds, through the NumPy twin of the definition, against the float64 restatement on the CPU), against the dense route's
kernel on the dense MAP arrays, and the tables route of BatchedPSRLContinuous against its dense route.

Every comparison is with the float64 restatement helpers_psrlc.vi_discounted_f64 on the dense MAP model, run for the
device's sweep count, within helpers_map_dvi.bound_discounted_map; two solves that may stop a sweep apart are compared within
the sum of their bounds plus what the restatement moves between the two sweep counts."""
import functools

import numpy as np
import pytest

import helpers_map_dvi as M
from helpers_psrlc import GAMMA32, GAUSS_SEIDEL, JACOBI, bound_discounted, vi_discounted_f64, vi_rule
from test_gpu_psrlc import make_env, undecided_states
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp
from colosseum_amd.agents import BatchedPSRLContinuous
from colosseum_amd.mdp import make_model

pytestmark = pytest.mark.gpu

EPS = 1e-3
BATCHES = [("small", GAMMA32), ("large", M.GAMMA09)]


@functools.lru_cache(maxsize=None)
def host_map(which, i):
    """(t, c, dense T_map, nnz of the dense array) of a generated problem, on the host."""
    row_ptr, col, hp, prior, mu = problems(which)[i]
    S, A = mu.shape
    _, c, t = dp.psrl_map_rows(row_ptr, col, hp, prior, S, A)
    return t, c, M.map_dense(row_ptr, col, t, c, S, A), M.dense_nnz(row_ptr, t, c, S)


def problems(which):
    return M.rule_problems() if which == "rule" else M.ragged_problems(which)


@functools.lru_cache(maxsize=None)
def q64(which, i, gamma, scheme, n):
    """The float64 restatement of problem i for n sweeps, computed once: (Q64, d_n, d_{n-1}, qmax)."""
    return vi_discounted_f64(host_map(which, i)[2], problems(which)[i][4], gamma, scheme, n)


def check_map_solve(which, i, Q, V, n, scheme, gamma, converged=True):
    """check_solve of tests/test_gpu_psrlc.py with K17's bound.  Returns (|Q - Q64| / bound, bound)."""
    S = Q.shape[0]
    assert np.array_equal(V, Q.max(-1)), (which, i)
    Q64, d_n, d_prev, qmax = q64(which, i, gamma, scheme, n)
    bound = M.bound_discounted_map(n, gamma, qmax, S)
    err = float(np.abs(Q.astype(np.float64) - Q64).max())
    print(f"{which}[{i}] S {S} A {Q.shape[1]} scheme {scheme}: {n} sweeps, |Q - Q64| {err:.3e}, bound {bound:.3e}, "
          f"d_n {d_n:.3e}, d_(n-1) {d_prev:.3e}")
    assert err <= bound, (which, i, err, bound, n, scheme)
    if converged:
        assert d_n < EPS + 2 * bound, (which, i, d_n, bound, n)
    assert n == 1 or d_prev >= EPS - 2 * bound, (which, i, d_prev, bound, n)
    return err / bound, bound


@pytest.mark.parametrize("scheme", [JACOBI, GAUSS_SEIDEL], ids=["jacobi", "gauss_seidel"])
@pytest.mark.parametrize("which,gamma", BATCHES, ids=[b[0] for b in BATCHES])
def test_ragged_batch_forced_scheme(need_gpu, which, gamma, scheme):
    ps = problems(which)
    outs = dp.discounted_value_iteration_map_batch(ps, gamma=gamma, scheme=scheme, return_map=True)
    assert (dp.discounted_value_iteration_map_batch.status == 0).all()
    sweeps = []
    for i, (Q, V, n, used, t, c) in enumerate(outs):
        ht, hc, _, _ = host_map(which, i)
        assert np.array_equal(t, ht) and np.array_equal(c.ravel(), hc.ravel()), (which, i)   # psrl_map_rows, bit for bit
        assert used == scheme
        check_map_solve(which, i, Q, V, n, scheme, gamma)
        sweeps.append(n)
    if which == "small":   # one launch: the instance with mu = 0 stops after its first sweep, others take hundreds
        assert sweeps[-1] == 1 and max(sweeps) > 200 and not outs[-1][0].any()
    again = dp.discounted_value_iteration_map_batch(ps, gamma=gamma, scheme=scheme, return_map=True)
    for a, b in zip(outs, again):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # without the MAP model's outputs: the same solve
    plain = dp.discounted_value_iteration_map_batch(ps, gamma=gamma, scheme=scheme)
    assert all(len(p) == 4 and np.array_equal(p[0], o[0]) and p[2] == o[2] for p, o in zip(plain, outs))


@pytest.mark.parametrize("scheme", [JACOBI, GAUSS_SEIDEL], ids=["jacobi", "gauss_seidel"])
@pytest.mark.parametrize("which,gamma", BATCHES, ids=[b[0] for b in BATCHES])
def test_against_the_dense_routes_kernel(need_gpu, which, gamma, scheme):
    """k_vi_discounted_dense on the dense MAP arrays of the same problems.  Both stop by a rule that one sweep more or less
    satisfies, so the sweeps are not asserted equal: Q lies within the sum of the two derived bounds plus what the float64
    restatement moves between the two sweep counts."""
    ps = problems(which)
    tab = dp.discounted_value_iteration_map_batch(ps, gamma=gamma, scheme=scheme)
    den = dp.discounted_value_iteration_dense_batch([(host_map(which, i)[2], p[4]) for i, p in enumerate(ps)], gamma=gamma,
                                                    scheme=scheme)
    for i, ((Qt, _, nt, ut), (Qd, _, nd, ud)) in enumerate(zip(tab, den)):
        S = Qt.shape[0]
        assert ut == ud == scheme
        Qa, _, _, qa = q64(which, i, gamma, scheme, nt)
        Qb, _, _, qb = q64(which, i, gamma, scheme, nd)
        tol = M.bound_discounted_map(nt, gamma, qa, S) + bound_discounted(nd, gamma, qb, S) + float(np.abs(Qa - Qb).max())
        err = float(np.abs(Qt.astype(np.float64) - Qd).max())
        print(f"{which}[{i}]: sweeps {nt} (tables) {nd} (dense), |Q_tables - Q_dense| {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol, (which, i, err, tol, nt, nd)


def test_the_rule_bites_per_instance(need_gpu):
    """scheme=None: two instances of one shape in one launch, at a lowered size threshold.  scheme_used is vi_rule on the
    dense MAP array's count of non-zero elements, as the dense route's kernel counts it."""
    ps = problems("rule")
    nnz = [host_map("rule", i)[3] for i in range(2)]
    want = [vi_rule(*p[4].shape, k, 100) for p, k in zip(ps, nnz)]
    assert want == [GAUSS_SEIDEL, JACOBI]
    outs = dp.discounted_value_iteration_map_batch(ps, gamma=M.GAMMA09, sparse_n_states_threshold=100, return_map=True)
    for i, (Q, V, n, used, t, c) in enumerate(outs):
        ht, hc, _, _ = host_map("rule", i)
        assert np.array_equal(t, ht) and np.array_equal(c.ravel(), hc.ravel()), i
        assert used == want[i], (i, used)
        check_map_solve("rule", i, Q, V, n, used, M.GAMMA09)
    assert not outs[1][5].any()   # c underflowed: the model is as sparse as its layout
    dense = dp.discounted_value_iteration_dense_batch([(host_map("rule", i)[2], p[4]) for i, p in enumerate(ps)], gamma=M.GAMMA09,
                                                      sparse_n_states_threshold=100)
    assert [o[3] for o in dense] == want
    # at the reference's threshold both are Gauss-Seidel; the density threshold is strict, as the reference's `<`
    outs = dp.discounted_value_iteration_map_batch(ps, gamma=M.GAMMA09)
    assert [o[3] for o in outs] == [GAUSS_SEIDEL] * 2
    S, A = ps[1][4].shape
    outs = dp.discounted_value_iteration_map_batch(ps, gamma=M.GAMMA09, sparse_n_states_threshold=100,
                                                   sparse_nnz_per_threshold=nnz[1] / (S * A * S))
    assert [o[3] for o in outs] == [GAUSS_SEIDEL] * 2


@pytest.mark.parametrize("scheme", [JACOBI, GAUSS_SEIDEL], ids=["jacobi", "gauss_seidel"])
def test_max_sweeps(need_gpu, scheme):
    """max_sweeps = 1: CMDP_ERR_MAX_ITER for the instances that need more, with the last sweep's values, and 0 for the one
    that converges in its first sweep, in the same launch."""
    ps = problems("small")
    outs = dp.discounted_value_iteration_map_batch(ps, scheme=scheme, max_sweeps=1)
    status = dp.discounted_value_iteration_map_batch.status
    assert (status[:-1] == L.ERR_MAX_ITER).all() and status[-1] == 0
    for i, (Q, V, n, used) in enumerate(outs):
        assert n == 1 and used == scheme
        check_map_solve("small", i, Q, V, 1, scheme, GAMMA32, converged=bool(status[i] == 0))
    full = dp.discounted_value_iteration_map_batch(ps, scheme=scheme)
    assert np.array_equal(full[-1][0], outs[-1][0]) and full[-1][2] == 1
    three = dp.discounted_value_iteration_map_batch(ps[3:5], scheme=scheme, max_sweeps=3)
    assert (dp.discounted_value_iteration_map_batch.status == L.ERR_MAX_ITER).all()
    for i, (Q, V, n, used) in zip((3, 4), three):
        assert n == 3
        check_map_solve("small", i, Q, V, 3, scheme, GAMMA32, converged=False)


# ---- the agent ---------------------------------------------------------------------------------------------------------
def trained_agent():
    models = [make_model("FrozenLakeContinuous", seed=i, size=4, p_frozen=0.9) for i in range(3)]
    env = make_env(models, "philox", False)
    agent = BatchedPSRLContinuous(env, [21, 22, 23], 10_000, no_optimistic_sampling=True)
    agent.run(400)
    return env, agent


def test_agent_tables_route_against_its_dense_route(need_gpu):
    """Three FrozenLakeContinuous-4 instances after 400 steps (reference sampler, fixed seeds, chosen so that at most 5 % of
    the batch's states are undecided; that condition is computed below from the float64 restatement alone and asserted)."""
    env, agent = trained_agent()
    assert agent.policy_solver == "dense"
    ls0, m0 = agent.last_sample(), agent.model()
    maps = agent.map_estimate()
    den, pi_d, avg_d = agent.policy_solve(), agent.policy(), agent.average_reward()
    agent.set_policy_solver("tables")
    assert agent.policy_solver == "tables"
    tab, pi_t, avg_t = agent.policy_solve(), agent.policy(), agent.average_reward()
    assert agent.stats()["policy_kernel_ms"] > 0
    again = agent.policy_solve()
    # nothing the agent acts or learns with has moved
    ls1, m1 = agent.last_sample(), agent.model()
    for b in range(3):
        assert all(np.array_equal(ls0[k][b], ls1[k][b]) for k in ("T", "R", "Q"))
        assert all(np.array_equal(m0[k][b], m1[k][b]) for k in ("transitions", "rewards", "N_sa", "nu_k"))
    assert np.array_equal(tab["scheme"], den["scheme"]) and (tab["scheme"] == GAUSS_SEIDEL).all()
    n_und, n_states, decided_all = 0, 0, []
    for b, (T_map, R_map) in enumerate(maps):
        S = int(env.n_states[b])
        Qt, Qd, nt, nd = tab["Q"][b], den["Q"][b], int(tab["sweeps"][b]), int(den["sweeps"][b])
        assert np.array_equal(Qt, again["Q"][b]) and nt == again["sweeps"][b]
        Qa, d_n, d_prev, qa = vi_discounted_f64(T_map, R_map, GAMMA32, GAUSS_SEIDEL, nt)
        Qb, _, _, qb = vi_discounted_f64(T_map, R_map, GAMMA32, GAUSS_SEIDEL, nd)
        bt = M.bound_discounted_map(nt, GAMMA32, qa, S)
        assert np.abs(Qt.astype(np.float64) - Qa).max() <= bt, b
        assert d_n < EPS + 2 * bt and d_prev >= EPS - 2 * bt, b
        bound = bt + bound_discounted(nd, GAMMA32, qb, S) + float(np.abs(Qa - Qb).max())
        err = float(np.abs(Qt.astype(np.float64) - Qd).max())
        print(f"instance {b}: sweeps {nt} (tables) {nd} (dense), |Q_tables - Q_dense| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (b, err, bound)
        und = undecided_states(Qa, bound)
        pi = pi_t[b]
        assert pi.shape == (S, 4) and np.array_equal(pi.sum(1), np.ones(S)) and set(np.unique(pi)) == {0.0, 1.0}
        assert np.array_equal(pi, dp.argmax_2d(Qt)), b          # the device's argmax of the device's Q
        assert np.array_equal(pi[~und], pi_d[b][~und]), b
        decided_all.append(not und.any())
        n_und += int(und.sum())
        n_states += S
    assert n_und <= 0.05 * n_states, (n_und, n_states)
    for b in range(3):
        if decided_all[b]:
            assert avg_t[b] == avg_d[b] and type(avg_t[b]) is type(avg_d[b]), b
    print(f"undecided states {n_und} of {n_states}; instances compared on average reward: {sum(decided_all)}")
    # a mask: the selected instances only, zeros elsewhere, as on the dense route
    mask = np.array([0, 1, 0], bool)
    one = agent.policy(mask)
    assert len(one) == 1 and np.array_equal(one[0], pi_t[1])
    sm = agent.policy_solve(mask)
    assert np.array_equal(sm["Q"][1], tab["Q"][1]) and not sm["Q"][0].any() and not sm["Q"][2].any()
    assert sm["sweeps"][0] == 0 and sm["sweeps"][1] == tab["sweeps"][1] and sm["scheme"][2] == 0
    assert agent.average_reward(mask)[0] == avg_t[1]
    # back to the dense route: the dense bits
    agent.set_policy_solver("dense")
    back = agent.policy_solve()
    assert all(np.array_equal(x, y) for x, y in zip(back["Q"], den["Q"])) and np.array_equal(back["sweeps"], den["sweeps"])
    assert all(np.array_equal(x, y) for x, y in zip(agent.policy(), pi_d))
    with pytest.raises(ValueError):
        agent.set_policy_solver("sparse")
    assert agent.policy_solver == "dense"
    env.close()


def test_agent_that_only_used_the_tables_route(need_gpu):
    """The hooks of the dense route reach the tables route: the sweep limit surfaces as CMDP_ERR_MAX_ITER in the same way,
    and the size threshold enters the rule (the MAP model is dense, so it stays Gauss-Seidel)."""
    env, agent = trained_agent()
    agent.set_policy_solver("tables")
    first = agent.policy_solve()
    assert (first["sweeps"] > 100).all() and (first["scheme"] == GAUSS_SEIDEL).all()
    agent._set_size_threshold(100)
    low = agent.policy_solve()
    assert (low["scheme"] == GAUSS_SEIDEL).all() and all(np.array_equal(x, y) for x, y in zip(low["Q"], first["Q"]))
    agent._set_max_sweeps(2)
    errors = []
    for route in ("tables", "dense"):
        agent.set_policy_solver(route)
        for call in (agent.policy_solve, agent.policy, agent.average_reward):
            with pytest.raises(L.DynamicProgrammingMaxIterationExceeded, match="did not converge in 2 sweeps") as e:
                call()
        errors.append(str(e.value))
    assert errors[0] == errors[1]
    agent._set_max_sweeps(dp.DP_MAX_ITERATION)
    agent.set_policy_solver("tables")
    ok = agent.policy_solve()
    assert all(np.array_equal(x, y) for x, y in zip(ok["Q"], first["Q"])) and np.array_equal(ok["sweeps"], first["sweeps"])
    env.close()
