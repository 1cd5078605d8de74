"""The COMPACT route of the optimistic continuous PSRL agent (K19: k_vi_discounted_optimistic on the compact sample,
csrc/cmdp_psrlo_vi.h; `BatchedPSRLContinuousOptimistic(sample_solver="compact")`, `set_sample_solver`,
`dynamic_programming.discounted_value_iteration_optimistic_batch`) on the GPU, against the NumPy twin of tests/helpers_psrlo.py
and the definitions of tests/helpers_psrlo_compact.py.

As in test_gpu_psrlo.py the twin is fed the device's transitions and takes the device's Q, so a rounding difference between
the two routes cannot fork a run.  What differs from the dense route's checks: the sample the twin is held against is the
EXPANSION last_sample() produces from the compact sample (bit for bit, as there), and the Q is not bit-equal to the dense
batch call on that expansion -- a simple row's terms are added in another order -- but within the derived bound of the
float64 restatement for the device's own sweep count (check_solve), and within the sum of both kernels' bounds, plus what the
float64 restatement moves between the two sweep counts, of the dense kernel's Q (both stop by a rule one sweep more or less
satisfies; the same comparison test_gpu_map_dvi.py makes for K17).  EVERY followed solve is held against the dense kernel's Q:
equal bits pass at once, anything else must lie within that tolerance; the float64 restatement's own checks (check_solve) run
on Follower.check_q64's sub-sample, as on the dense route.  How often the bits were equal and how often the two kernels
stopped at different sweep counts is counted and printed."""
import numpy as np
import pytest

import helpers_psrlo_compact as HC
from helpers_psrlc import GAMMA32, GAUSS_SEIDEL, JACOBI, vi_discounted_f64, vi_rule
from helpers_psrlo import philox_z
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp
from colosseum_amd.agents import BatchedPSRLContinuous, BatchedPSRLContinuousOptimistic
from colosseum_amd.mdp import make_model
from test_gpu_psrlc import EPS, check_solve, make_env
from test_gpu_psrlo import HORIZON, OFollower

pytestmark = pytest.mark.gpu

BITS = dict(equal=0, solves=0, sweeps_differ=0)   # over the whole file, printed: solves whose Q had the dense kernel's bits; whose sweeps differed


def against_dense(T, R_ext, Q, n, used, Qd, nd, gamma=GAMMA32):
    """|Q - Q_dense| within the sum of both bounds plus the float64 restatement's move between the two sweep counts."""
    S = T.shape[0]
    Qa, _, _, qa = vi_discounted_f64(T, R_ext, gamma, used, n)
    Qb, qb = (Qa, qa) if nd == n else vi_discounted_f64(T, R_ext, gamma, used, nd)[::3]
    tol = HC.bound_compact(n, gamma, qa, S) + HC.bound_compact(nd, gamma, qb, S) + float(np.abs(Qa - Qb).max())
    err = float(np.abs(Q.astype(np.float64) - Qd).max())
    assert err <= tol, (err, tol, n, nd, used)
    return err / tol


class CFollower(OFollower):
    """OFollower with the compact route's checks of a solve in place of the dense route's bit-equality."""

    def after_rounds(self, ended):
        if not ended:
            return
        ls = self.agent.last_sample()
        for b in ended:
            tw = self.twins[b]
            self.pending[b] = ls["Q"][b].copy()
            if self.sampler == "philox":
                tw.z_restated, tw.k_posterior = philox_z(self.seeds[b], tw.episode, tw.S, tw.psi), 0
                assert ls["z"][b].tolist() == tw.z_restated, (b, tw.episode)
                self.device[b] = (ls["T"][b], ls["R"][b])
                tw.episode_end_update()
            elif tw.episode == 0:
                tw.before_start_interacting()
            else:
                tw.episode_end_update()
            n1, n2 = tw.last_n
            assert np.array_equal(ls["simple"][b], tw.last_simple), (b, tw.episode)
            if self.sampler == "reference":
                assert ls["z"][b].tolist() == (tw.last_z if n2 else [-1] * tw.psi), (b, tw.episode)
            assert np.array_equal(ls["R"][b], tw.last_R) and np.array_equal(ls["R_ext"][b], tw.last_R_ext), (b, tw.episode)
            assert ls["T"][b].dtype == np.float32 and np.array_equal(ls["T"][b], tw.last_T), (b, tw.episode, n1, n2)
            self.kinds.add("mixed" if n1 and n2 else "all_posterior" if n1 else "all_simple")
            nz = (ls["T"][b].reshape(tw.S, tw.A, tw.psi, tw.S) != 0).sum(-1).max(-1)
            self.nonzero_p_minus += int(((nz > 1) & tw.last_simple).sum())
        outs = dp.discounted_value_iteration_dense_batch([(ls["T"][b], ls["R_ext"][b]) for b in ended],
                                                         sparse_n_states_threshold=self.agent_threshold())
        for b, (Qd, _, nd, used_d) in zip(ended, outs):
            T, Q, n, used = ls["T"][b], ls["Q"][b], int(ls["sweeps"][b]), int(ls["scheme"][b])
            assert ls["status"][b] == 0, b
            assert used == used_d == vi_rule(T.shape[0], T.shape[1], int((T != 0).sum()), self.agent_threshold()), b
            same = bool(np.array_equal(Q, Qd))
            BITS["solves"] += 1
            BITS["equal"] += same
            BITS["sweeps_differ"] += n != nd
            if not same:   # every solve: the dense kernel's bits, or within both bounds of them
                against_dense(T, ls["R_ext"][b], Q, n, used, Qd, nd)
            if self.check_q64(b):
                self.worst = max(self.worst, check_solve(T, ls["R_ext"][b], Q, Q.max(-1), n, used, GAMMA32, EPS))
                self.n_q64 += 1
            self.n_solves[b] += 1

    def external_update(self):
        self.agent.episode_end_update()
        self.kinds.clear()
        self.after_rounds(list(range(self.env.B)))
        self.episodes = self.agent.model()["episode"].copy()
        self.compare_models()


def build(models, rng="mt", seeds=None, sampler="reference", route="compact", **akw):
    env = make_env(models, rng, False)
    seeds = np.arange(len(models)) + 11 if seeds is None else seeds
    agent = BatchedPSRLContinuousOptimistic(env, seeds, HORIZON, sampler=sampler, sample_solver=route, **akw)
    assert agent.sample_solver == route and agent.stats()["sample_solver"] == route
    return env, agent, CFollower(env, agent, seeds, sampler=sampler)


def report(name, f):
    print(f"{name}: {int(f.n_solves.sum())} solves, {f.n_q64} against float64 and the dense kernel, worst |Q - Q64| / bound "
          f"{f.worst:.3f}, rounds {sorted(f.kinds)}; dense kernel's bits in {BITS['equal']} of {BITS['solves']} solves so far, "
          f"sweep counts differed in {BITS['sweeps_differ']}")


# ---- 1. followed agents ----------------------------------------------------------------------------------------------------
def test_ragged_batch_followed_then_an_external_update(need_gpu):
    models = [make_model("RiverSwimContinuous", seed=s, size=size) for s, size in enumerate((3, 5, 8))]
    env, agent, f = build(models, eta_weight=1e-10, psi_weight=0.25)
    assert agent.psi.tolist() == [3, 6, 11] and agent.eta.tolist() == [5.0] * 3 and [int(S) % 4 for S in env.n_states] == [3, 1, 0]
    f.follow(40, chunk=16)
    f.external_update()   # 6 pairs and 40 visits in the first instance: a pair has passed eta = 5 (pigeonhole)
    assert f.kinds & {"mixed", "all_posterior"}
    # the byte count of include/cmdp.h with blocks in use: a block holds the psi * n1 * S floats of the last draw (n1 never
    # decreases) and, grown by doubling from below that, less than twice as many, never more than psi * S * A * S
    simple = agent.last_sample()["simple"]
    S, psi = np.asarray(env.n_states, np.int64), agent.psi.astype(np.int64)
    nz = np.array([np.diff(agent._ptr)[int(env.row_off[b]):int(env.row_off[b + 1])].sum() for b in range(env.B)], np.int64)
    fixed = 4 * (max(1, int((psi * nz).sum())) + int((S * env.A * psi).sum())) + 8 * env.B
    need = psi * np.array([int((~m).sum()) for m in simple], np.int64) * S
    assert need.sum() > 0
    got = agent.stats()["sample_bytes"]
    assert fixed + 4 * int(need.sum()) <= got <= fixed + 4 * int(np.minimum(2 * need, psi * S * env.A * S).sum()), (got, fixed, need)
    report("ragged", f)
    env.close()


def test_riverswim5_defaults(need_gpu):
    models = [make_model("RiverSwimContinuous", seed=0, size=5)]
    env, agent, f = build(models, seeds=[0])
    assert agent.psi.tolist() == [26] and agent.eta.tolist() == [50.0]
    f.follow(600, chunk=64)
    assert f.nonzero_p_minus > 0 and "all_simple" in f.kinds
    st = agent.stats()
    assert st["solves"] == f.n_solves.sum() and st["unconverged"] == 0 and st["sweeps"] > 0 and st["sample_solver"] == "compact"
    report("riverswim5", f)
    env.close()


def test_riverswim4_small_eta_philox(need_gpu):
    models = [make_model("RiverSwimContinuous", seed=6, size=4)]
    env, agent, f = build(models, seeds=[6], sampler="philox", eta_weight=1e-10, max_psi=5)
    assert agent.psi.tolist() == [5] and agent.eta.tolist() == [5.0] and agent.stats()["reference_ms"] == 0
    f.follow(600, chunk=64)
    assert "all_simple" in f.kinds and f.kinds & {"mixed", "all_posterior"}
    report("riverswim4 philox", f)
    env.close()


@pytest.mark.parametrize("scheme", [GAUSS_SEIDEL, JACOBI], ids=["gauss_seidel", "jacobi"])
def test_frozenlake4_psi60(need_gpu, scheme):
    """240 extended actions.  At the reference's size threshold every solve is Gauss-Seidel; at a lowered one the simple rows'
    few non-zeros make every extended sample sparse by the reference's rule: Jacobi."""
    models = [make_model("FrozenLakeContinuous", seed=4, size=4, p_frozen=0.9)]
    env, agent, f = build(models, seeds=[4])
    assert agent.psi.tolist() == [60]
    if scheme == JACOBI:
        f.size_threshold = 100
        agent._set_size_threshold(100)
    f.follow(4, chunk=4)   # a handful of rounds: the dense kernel's solve of the expansion, the yardstick, takes most of a second
    assert (agent.last_sample()["scheme"] == scheme).all()
    report(f"frozenlake4 scheme {scheme}", f)
    env.close()


def test_frozenlake4_psi70_a_second_trip_over_the_samples(need_gpu):
    models = [make_model("FrozenLakeContinuous", seed=4, size=4, p_frozen=0.9)]
    env, agent, f = build(models, seeds=[4], max_psi=70)
    assert agent.psi.tolist() == [70]
    f.external_update()
    f.size_threshold = 100
    agent._set_size_threshold(100)
    f.external_update()
    assert agent.last_sample()["scheme"].tolist() == [JACOBI]
    report("frozenlake4 psi 70", f)
    env.close()


# ---- 2. the stand-alone call on generated compact problems -----------------------------------------------------------------
def generated(rng, S, A, psi, n_post):
    """A layout of 1 to 4 positions per row (one row without any); simple rows: sub-stochastic float32 values at the layout, a z
    per sample that lies inside some rows' layouts and outside others', a bump that makes the row sum to about one; `n_post`
    posterior rows: Dirichlet draws cast to float32, one with float32 zeros (a small shape underflows), one all zero."""
    rows = S * A
    lens = rng.randint(1, min(4, S) + 1, size=rows)
    lens[rng.randint(rows)] = 0
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(S, n, replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    simple = np.ones(rows, bool)
    simple[rng.choice(rows, n_post, replace=False)] = False
    z = rng.randint(S, size=psi).astype(np.int32)
    z[0] = col[0]                                     # inside the first non-empty row's layout at least once
    T = np.zeros((rows, psi, S), np.float32)
    k_post = 0
    for row in range(rows):
        cs = col[row_ptr[row]:row_ptr[row + 1]]
        if simple[row]:
            for k in range(psi):
                v = (rng.dirichlet(np.ones(len(cs) + 1)) * rng.rand()).astype(np.float32) if len(cs) else np.ones(1, np.float32)
                T[row, k, cs] = v[:len(cs)]
                if rng.rand() < 0.2 and len(cs):
                    T[row, k, cs[0]] = 0          # a zero inside the layout
                T[row, k, z[k]] = np.float32(1) - T[row, k].sum(dtype=np.float64).astype(np.float32) + T[row, k, z[k]]
        else:
            shape = 1e-3 if k_post == 0 else 0.3      # shape 1e-3: most variates underflow to float32 zero
            g = rng.gamma(shape, size=(psi, S)).astype(np.float32)
            T[row] = g / (np.float32(1e-5) + g.sum(-1, keepdims=True))
            if k_post == 1:
                T[row] = 0
            k_post += 1
    T_ext = T.reshape(S, A * psi, S)
    R = rng.normal(size=(S, A)).astype(np.float32)
    c = HC.compact_of(T_ext, psi, simple, z, row_ptr, col, R)
    assert np.array_equal(HC.expand(c), T_ext)
    return c, T_ext


# S = 5 and 257: scalar rows; 16, 100, 260: 16-byte rows; 100: more than 64 columns; 257, 260: more than 256
CASES = [(5, 2, 2, 3), (5, 4, 60, 4), (16, 2, 70, 5), (16, 4, 60, 6), (100, 2, 60, 4), (100, 4, 2, 9), (257, 2, 3, 5), (260, 4, 2, 7)]
GAMMA09 = float(np.float32(0.9))   # 90 sweeps or so: the float64 restatements stay quick


@pytest.fixture(scope="module")
def problems():
    rng = np.random.RandomState(19)
    return [generated(rng, *case) for case in CASES]


@pytest.mark.parametrize("scheme", [JACOBI, GAUSS_SEIDEL, None], ids=["jacobi", "gauss_seidel", "auto"])
def test_standalone_on_generated_problems(need_gpu, problems, scheme):
    cs = [c for c, _ in problems]
    assert any((c["post"] == 0).all(-1).any() for c in cs) and any(((c["post"] == 0).sum(-1) > 0).any() for c in cs)
    thr = 20000   # AUTO: the small problems are Gauss-Seidel by size, the larger ones by their count of non-zero elements
    outs = dp.discounted_value_iteration_optimistic_batch(cs, gamma=GAMMA09, scheme=scheme, sparse_n_states_threshold=thr)
    assert (dp.discounted_value_iteration_optimistic_batch.status == 0).all()
    dense = dp.discounted_value_iteration_dense_batch([(T, HC.r_ext(c)) for c, T in problems], gamma=GAMMA09, scheme=scheme,
                                                      sparse_n_states_threshold=thr)
    worst, used_all = 0.0, set()
    for (c, T), (Q, V, n, used), (Qd, _, nd, used_d) in zip(problems, outs, dense):
        S, AX = Q.shape
        want = scheme if scheme is not None else vi_rule(S, AX, HC.nonzero_count(c), thr)
        assert used == used_d == want and HC.nonzero_count(c) == int((T != 0).sum())
        used_all.add(used)
        assert 10 < n < 1000
        worst = max(worst, check_solve(T, HC.r_ext(c), Q, V, n, used, GAMMA09, EPS))
        against_dense(T, HC.r_ext(c), Q, n, used, Qd, nd, GAMMA09)
        BITS["solves"] += 1
        BITS["equal"] += bool(np.array_equal(Q, Qd))
        BITS["sweeps_differ"] += n != nd
    if scheme is None:
        assert used_all == {JACOBI, GAUSS_SEIDEL}
    print(f"scheme {scheme}: worst |Q - Q64| / bound {worst:.3f}; dense kernel's bits in {BITS['equal']} of {BITS['solves']} so far")


def test_standalone_float64_on_the_compact_form_and_ragged_launch(need_gpu, problems):
    """count = 3 of different S, A and psi in one launch equals the problems solved in the big launch; the float64 solver on the
    compact form (row sums in the kernel's order) is within the bound too."""
    three = [problems[i][0] for i in (0, 1, 2)]
    for scheme in (JACOBI, GAUSS_SEIDEL):
        outs = dp.discounted_value_iteration_optimistic_batch(three, gamma=GAMMA09, scheme=scheme)
        alone = [dp.discounted_value_iteration_optimistic_batch([c], gamma=GAMMA09, scheme=scheme)[0] for c in three]
        for c, (Q, V, n, used), (Q1, V1, n1, _) in zip(three, outs, alone):
            assert np.array_equal(Q, Q1) and np.array_equal(V, V1) and n == n1
            Q64, _, _, qmax = HC.vi_compact_f64(c, GAMMA09, scheme, n)
            assert np.abs(Q.astype(np.float64) - Q64).max() <= HC.bound_compact(n, GAMMA09, qmax, c["S"])


def test_standalone_row_descriptors_from_global_memory(need_gpu, problems, monkeypatch):
    """The sweeps read the row flags and ranges from LDS when they fit 64 KB (about 13 000 real rows) and from global memory
    beyond; CMDP_POV_DESC=0 takes the second form at any size.  The results do not depend on the form."""
    cs = [c for c, _ in problems]
    for scheme in (JACOBI, GAUSS_SEIDEL):
        monkeypatch.delenv("CMDP_POV_DESC", raising=False)
        staged = dp.discounted_value_iteration_optimistic_batch(cs, gamma=GAMMA09, scheme=scheme)
        monkeypatch.setenv("CMDP_POV_DESC", "0")
        plain = dp.discounted_value_iteration_optimistic_batch(cs, gamma=GAMMA09, scheme=scheme)
        assert (dp.discounted_value_iteration_optimistic_batch.status == 0).all()
        for (Q, V, n, used), (Q2, V2, n2, used2) in zip(staged, plain):
            assert np.array_equal(Q, Q2) and np.array_equal(V, V2) and n == n2 and used == used2 == scheme


def test_standalone_refusals(need_gpu, problems):
    c = dict(problems[0][0])
    lib = L.load()
    with pytest.raises(L.CmdpError) as ei:
        dp.discounted_value_iteration_optimistic_batch([dict(c, z=np.full(c["psi"], c["S"], np.int32))])
    assert ei.value.code == L.ERR_INVALID and b"z[" in lib.cmdp_last_error()
    bad = c["pidx"].copy()
    bad[np.flatnonzero(~c["simple"])[0]] = 1
    with pytest.raises(L.CmdpError) as ei:
        dp.discounted_value_iteration_optimistic_batch([dict(c, pidx=bad)])
    assert ei.value.code == L.ERR_INVALID and b"pidx" in lib.cmdp_last_error()
    with pytest.raises(L.CmdpError) as ei:
        dp.discounted_value_iteration_optimistic_batch([c], max_sweeps=0)
    assert ei.value.code == L.ERR_INVALID


# ---- 3. routes on one handle -----------------------------------------------------------------------------------------------
def test_switching_routes_on_one_handle(need_gpu):
    models = [make_model("RiverSwimContinuous", seed=s, size=5) for s in (0, 1)]
    env, agent, f = build(models, seeds=[0, 1], route="dense", eta_weight=1e-10, max_psi=6)
    dense_checks = OFollower.after_rounds
    f.after_rounds = lambda ended: dense_checks(f, ended)      # the dense route's checks: Q bit-equal to the dense batch call
    f.follow(20, chunk=8)
    dense_bytes = agent.stats()["sample_bytes"]
    agent.set_sample_solver("compact")
    assert agent.sample_solver == "compact" and agent.stats()["sample_solver"] == "dense"   # the last round was dense
    del f.after_rounds
    f.follow(40, chunk=8)   # instances that have not parked since keep their dense sample: last_sample serves both forms
    st = agent.stats()
    assert st["sample_solver"] == "compact" and st["sample_bytes"] >= dense_bytes
    f.external_update()
    assert f.kinds & {"mixed", "all_posterior"}
    agent.set_sample_solver("dense")
    f.after_rounds = lambda ended: dense_checks(f, ended)
    f.external_update()
    f.follow(16, chunk=8)
    assert agent.sample_solver == "dense" and agent.stats()["sample_solver"] == "dense"
    with pytest.raises(ValueError):
        agent.set_sample_solver("sparse")
    assert agent.sample_solver == "dense"
    with pytest.raises(ValueError):
        BatchedPSRLContinuousOptimistic(env, [0, 1], HORIZON, sample_solver="tables")
    lib = L.load()
    assert lib.cmdp_psrlc_set_option(agent._h, L.PSRLC_OPT_SAMPLE_SOLVER, 2) == L.ERR_INVALID
    env.close()
    env_p = make_env(models, "mt", False)
    plain = BatchedPSRLContinuous(env_p, [0, 1], HORIZON, no_optimistic_sampling=True)
    assert not hasattr(plain, "set_sample_solver")
    assert lib.cmdp_psrlc_set_option(plain._h, L.PSRLC_OPT_SAMPLE_SOLVER, 1) == L.ERR_UNSUPPORTED
    assert b"plainly" in lib.cmdp_last_error()
    env_p.close()


# ---- 4. the sweep limit ----------------------------------------------------------------------------------------------------
def test_sweep_limit(need_gpu):
    models = [make_model("RiverSwimContinuous", seed=s, size=5) for s in (0, 1)]
    env = make_env(models, "mt", False)
    agent = BatchedPSRLContinuousOptimistic(env, [0, 1], HORIZON, sample_solver="compact", max_psi=6)
    assert agent.stats()["unconverged"] == 0
    agent._set_max_sweeps(3)
    agent.episode_end_update()
    ls = agent.last_sample()
    assert (ls["status"] == L.ERR_MAX_ITER).all() and (ls["sweeps"] == 3).all() and agent.stats()["unconverged"] == 2
    for b in range(2):
        check_solve(ls["T"][b], ls["R_ext"][b], ls["Q"][b], ls["Q"][b].max(-1), 3, int(ls["scheme"][b]), GAMMA32, EPS, converged=False)
    env.close()


# ---- 5. the Philox sample is a pure function, and the same on both routes --------------------------------------------------
def test_philox_purity_and_equality_with_the_dense_route(need_gpu):
    mk = lambda: [make_model("RiverSwimContinuous", seed=s, size=size) for s, size in enumerate((4, 5, 8))]  # noqa: E731
    seeds = np.array([3, 4, 5])

    def handle(route):
        env = make_env(mk(), "mt", False)
        return env, BatchedPSRLContinuousOptimistic(env, seeds, HORIZON, sampler="philox", sample_solver=route, eta_weight=1e-10,
                                                    max_psi=6)

    def same(la, lb, keys, tag):
        for b in range(3):
            for k in keys:
                assert np.array_equal(la[k][b], lb[k][b]), (tag, k, b)

    (e1, a1), (e2, a2), (e3, a3), (e4, a4) = handle("compact"), handle("compact"), handle("dense"), handle("dense")
    for update in range(3):   # creation, then two external updates: no steps, so the tables are equal by construction
        if update:
            for a in (a1, a2, a3, a4):
                a.episode_end_update()
        l1, l2, l3 = a1.last_sample(), a2.last_sample(), a3.last_sample()
        same(l1, l2, ("z", "simple", "T", "Q", "R", "R_ext"), update)
        same(l1, l3, ("z", "simple", "T", "R", "R_ext"), update)
    # posterior rows need visits.  Handles of one route walk the same steps (equal seeds, one deterministic kernel), so their
    # tables stay equal: two compact handles, and two dense ones of which one then switches to compact for the sample
    for a in (a1, a2, a3, a4):
        a.run(60)
    m3, m4 = a3.model(), a4.model()
    assert np.array_equal(m3["episode"], m4["episode"]) and all(np.array_equal(x, y) for x, y in zip(m3["N"], m4["N"]))
    a4.set_sample_solver("compact")
    for a in (a1, a2, a3, a4):
        a.episode_end_update()
    l1, l2, l3, l4 = (a.last_sample() for a in (a1, a2, a3, a4))
    assert not all(s.all() for s in l1["simple"]) and not all(s.all() for s in l4["simple"])   # posterior rows took part
    same(l1, l2, ("z", "simple", "T", "Q", "R", "R_ext"), "compact pair")
    same(l4, l3, ("z", "simple", "T", "R", "R_ext"), "compact against dense")
    for e in (e1, e2, e3, e4):
        e.close()


# ---- 6. memory -------------------------------------------------------------------------------------------------------------
def test_memory_of_the_two_routes(need_gpu):
    """8 x FrozenLake-10.  psi is lowered to 12: creating the DENSE handle solves its first sample, a chain over S * A * psi
    rows a sweep that takes seconds at psi = 60; the byte counts scale with psi alike on both routes."""
    models = [make_model("FrozenLakeContinuous", seed=s, size=10, p_frozen=0.9) for s in range(8)]
    out = {}
    for route in ("compact", "dense"):
        env = make_env(models, "mt", False)
        agent = BatchedPSRLContinuousOptimistic(env, np.arange(8), HORIZON, sampler="philox", sample_solver=route, max_psi=12)
        assert agent.psi.tolist() == [12] * 8
        out[route] = agent.stats()["sample_bytes"]
        if route == "compact":   # the formula of include/cmdp.h on a fresh handle: nothing is posterior, every block is empty
            nz = np.diff(agent._ptr)
            per_instance = [int(nz[int(env.row_off[b]):int(env.row_off[b + 1])].sum()) for b in range(8)]
            S = np.asarray(env.n_states, np.int64)
            want = 4 * (max(1, int((agent.psi * per_instance).sum())) + int((S * env.A * agent.psi).sum())) + 8 * 8
            assert out[route] == want, (out[route], want)
            assert agent.last_sample()["simple"][0].all()
        env.close()
    T_ext = sum(int(m.n_states) ** 2 * 4 * 12 * 4 for m in models)
    assert out["dense"] >= T_ext > 10 * out["compact"], out
    print(f"8 x FrozenLake-10 at psi = 12: sample routes hold {out['dense']} bytes (dense), {out['compact']} (compact)")
