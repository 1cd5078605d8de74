"""The device PSRL agent for the continuous setting (K13, colosseum_amd.agents.BatchedPSRLContinuous) and its solver
(k_vi_discounted_dense) against the NumPy twin and the float64 restatement of tests/helpers_psrlc.py, which tests/test_psrlc.py
holds against the reference (golden G22) on the CPU.

The solve is not the reference's BLAS product and stops by a rule that one sweep more or less satisfies, so trajectories are
not compared with the reference's: the twin is fed the DEVICE's transitions, artificial episode by artificial episode
(run(stop_at_episode_end=True, trace=True)), and after every call, for every instance:
  * every action is the twin actor's choice under the Q the device held (tie-break stream included) and the call ended at
    the step the reference's is_episode_end gives;
  * model() equals the twin's two hyper-parameter arrays, N.sum(-1) and nu_k bit for bit;
  * last_sample()'s T and R equal the twin's own numpy draws bit for bit (reference sampler) or the restatement of
    k_psrl_sample within the tolerance derived in helpers_psrl (Philox sampler);
  * the new Q is bit-equal to discounted_value_iteration_dense_batch on the same (T, R), with the same sweeps and scheme, and
    (first solves, every eighth, see Follower.check_q64) within bound_discounted of the float64 restatement run for the
    device's sweep count, whose last two differences straddle epsilon within two bounds."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers_psrl import U, numpy_sampler, philox_sample
from helpers_psrlc import GAMMA32, GAUSS_SEIDEL, JACOBI, PSRLCTwin, bound_discounted, vi_discounted_f64, vi_rule
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp
from colosseum_amd.agents import BatchedPSRLContinuous, BatchedPSRLEpisodic
from colosseum_amd.batched import BatchedMDP
from colosseum_amd.mdp import make_model

pytestmark = pytest.mark.gpu

G22 = os.path.join(ROOT, "tests", "golden", "G22_psrlc.npz")
EPS = 1e-3


def g22():
    z = np.load(G22)
    return z, json.loads(str(z["cases"]))


def check_solve(T, R, Q, V, n, scheme, gamma, eps, converged=True):
    """What every solve of the kernel must satisfy, for the device's sweep count n.  Returns |Q - Q64| / bound."""
    assert np.array_equal(V, Q.max(-1))
    Q64, d_n, d_prev, qmax = vi_discounted_f64(T, R, gamma, scheme, n)
    bound = bound_discounted(n, gamma, qmax, T.shape[0])
    err = float(np.abs(Q.astype(np.float64) - Q64).max())
    assert err <= bound, (err, bound, n, scheme)
    if converged:
        assert d_n < eps + 2 * bound, (d_n, bound, n)
    assert n == 1 or d_prev >= eps - 2 * bound, (d_prev, bound, n)
    return err / bound


def dirichlet_problem(rng, S, A, shape=0.3, zero_rows=()):
    T = rng.gamma(shape, size=(S, A, S)).astype(np.float32)
    T = T / (np.float32(1e-5) + T.sum(-1, keepdims=True))
    for s, a in zero_rows:
        T[s, a] = 0
    return T, rng.normal(size=(S, A)).astype(np.float32)


# ---- the solver through discounted_value_iteration_dense_batch ----------------------------------------------------------
# scalar loads, a tail, more than one column per lane: S = 3 and 65 with A = 2 and 5 (5 actions: more rows than wavefronts);
# 16-byte loads and more than one trip of the vector loop (260 > 256): S = 8 and 260 with A = 4
SHAPES = [(3, 2), (65, 5), (8, 4), (65, 2), (260, 4), (3, 5)]


@pytest.mark.parametrize("scheme", [JACOBI, GAUSS_SEIDEL], ids=["jacobi", "gauss_seidel"])
def test_solver_shapes_ragged_forced_scheme(need_gpu, scheme):
    rng = np.random.RandomState(3)
    probs = [dirichlet_problem(rng, S, A, zero_rows=((0, 1), (S - 1, 0)) if S == 65 else ()) for S, A in SHAPES]
    gamma = float(np.float32(0.9))   # 90 sweeps or so: the float64 restatement of the 260-state problem stays quick
    outs = dp.discounted_value_iteration_dense_batch(probs, gamma=gamma, scheme=scheme)
    assert (dp.discounted_value_iteration_dense_batch.status == 0).all()
    worst = 0.0
    for (T, R), (Q, V, n, used) in zip(probs, outs):
        assert used == scheme and 10 < n < 1000
        worst = max(worst, check_solve(T, R, Q, V, n, scheme, gamma, EPS))
    print(f"scheme {scheme}: worst |Q - Q64| / bound {worst:.3f}")
    # gamma = 0.99, the agent's: the small shapes
    small = [p for p in probs if p[0].shape[0] <= 8]
    for (T, R), (Q, V, n, used) in zip(small, dp.discounted_value_iteration_dense_batch(small, scheme=scheme)):
        assert used == scheme and n > 100
        check_solve(T, R, Q, V, n, scheme, GAMMA32, EPS)


def test_solver_applies_the_rule_per_instance(need_gpu):
    """One dense and one mostly-zero T of the same shape in the same launch, at a lowered size threshold: the count of
    non-zero elements decides per instance.  At the reference's threshold both are Gauss-Seidel."""
    rng = np.random.RandomState(5)
    dense = dirichlet_problem(rng, 20, 4)
    T, R = dirichlet_problem(rng, 20, 4)
    T[rng.rand(*T.shape) < 0.9] = 0
    sparse = (T, R)
    unaligned = dirichlet_problem(rng, 21, 3)
    Tu = unaligned[0]
    Tu[rng.rand(*Tu.shape) < 0.9] = 0
    probs = [dense, sparse, unaligned]
    nnz = [int((p[0] != 0).sum()) for p in probs]
    want = [vi_rule(*p[0].shape[:2], k, 100) for p, k in zip(probs, nnz)]
    assert want == [GAUSS_SEIDEL, JACOBI, JACOBI]
    gamma = float(np.float32(0.9))
    outs = dp.discounted_value_iteration_dense_batch(probs, gamma=gamma, sparse_n_states_threshold=100)
    for (T, R), (Q, V, n, used), w in zip(probs, outs, want):
        assert used == w
        check_solve(T, R, Q, V, n, used, gamma, EPS)
    outs = dp.discounted_value_iteration_dense_batch(probs, gamma=gamma)
    assert [o[3] for o in outs] == [GAUSS_SEIDEL] * 3
    # the density threshold is strict, as the reference's `<`
    k = nnz[1]
    outs = dp.discounted_value_iteration_dense_batch([sparse, sparse], gamma=gamma, sparse_n_states_threshold=100,
                                                     sparse_nnz_per_threshold=k / sparse[0].size)
    assert [o[3] for o in outs] == [GAUSS_SEIDEL] * 2


def test_solver_max_sweeps(need_gpu):
    rng = np.random.RandomState(7)
    probs = [dirichlet_problem(rng, 8, 4), dirichlet_problem(rng, 5, 2)]
    for scheme in (JACOBI, GAUSS_SEIDEL):
        outs = dp.discounted_value_iteration_dense_batch(probs, scheme=scheme, max_sweeps=3)
        assert (dp.discounted_value_iteration_dense_batch.status == L.ERR_MAX_ITER).all()
        for (T, R), (Q, V, n, used) in zip(probs, outs):
            assert n == 3 and used == scheme
            check_solve(T, R, Q, V, 3, scheme, GAMMA32, EPS, converged=False)   # the last sweep's values


def test_solver_against_the_references_q(need_gpu):
    """Every (T, R) stored in G22 in one launch against the Q the reference recorded: both sides stop within
    gamma eps / (1 - gamma) of the fixed point, so they differ by at most twice that plus the kernel's rounding bound."""
    z, meta = g22()
    probs, refs = [], []
    for i, m in enumerate(meta):
        for j, k in enumerate(z[f"c{i}_kept"].tolist()):
            probs.append((z[f"c{i}_T"][j], z[f"c{i}_R"][j]))
            refs.append(z[f"c{i}_Q"][k])
    assert any((T.sum(-1) == 0).any() for T, _ in probs)
    worst = 0.0
    for (T, R), (Q, V, n, used), ref in zip(probs, dp.discounted_value_iteration_dense_batch(probs), refs):
        assert used == GAUSS_SEIDEL
        qmax = float(np.abs(ref).max()) + 1.0
        tol = 2 * GAMMA32 * EPS / (1 - GAMMA32) + bound_discounted(n, GAMMA32, qmax, T.shape[0])
        err = float(np.abs(Q.astype(np.float64) - ref).max())
        worst = max(worst, err)
        assert err <= tol, (err, tol)
    print(f"{len(probs)} samples of G22: worst |Q - Q_reference| {worst:.3e} (tolerance {tol:.3e})")


# ---- the agent ---------------------------------------------------------------------------------------------------------
def make_env(models, rng, beta, keys=None):
    """rng "mt": CMDP_RNG_MT_COMPAT (Beta rewards reported as their means); "philox": Beta rewards drawn on the device."""
    if rng == "mt":
        env = BatchedMDP(models, rng_mode=L.RNG_MT_COMPAT, flags=L.FLAG_REWARD_MEANS if beta else 0)
    else:
        keys = np.arange(len(models), dtype=np.uint64) * 7919 + 5 if keys is None else keys
        env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=keys)
    env.reset()
    return env


class Follower:
    """The twins of a batch and the checks of one call."""

    def __init__(self, env, agent, seeds, sampler, rprm=None, tprm=None, q64_every=8):
        self.env, self.agent, self.sampler, self.seeds = env, agent, sampler, [int(s) for s in seeds]
        self.q64_every = q64_every
        self.pending = [None] * env.B
        self.twins = []
        for b in range(env.B):
            self.twins.append(PSRLCTwin(self.seeds[b], int(env.n_states[b]), env.A, env.rewards_range[1],
                                        (lambda T, R, _b=b: self.pending[_b][2]),
                                        sampler=(lambda tw, _b=b: self.twin_sample(_b, tw)), rewards_prior_prms=rprm,
                                        transitions_prior_prms=tprm))
        self.cur = env.state()[0].copy()
        self.actions = [[] for _ in range(env.B)]
        self.episodes = agent.model()["episode"].copy()
        assert (self.episodes == 1).all()
        self.n_solves = np.zeros(env.B, np.int64)
        self.n_q64 = 0
        self.worst = 0.0
        self.after_rounds(list(range(env.B)))
        self.compare_models()

    def twin_sample(self, b, tw):
        """Reference sampler: the twin's own numpy draws.  Philox sampler: the device's sample, once it has been held
        against the restatement of k_psrl_sample on the twin's tables."""
        T_d, R_d, _ = self.pending[b]
        if self.sampler == "reference":
            T, R = numpy_sampler(tw)
            assert np.array_equal(T_d, T.reshape(T_d.shape)) and np.array_equal(R_d, R.reshape(R_d.shape)), (b, tw.episode)
            return T_d, R_d
        T, R, tol_T, tol_R, row_target = philox_sample(self.seeds[b], tw.episode, tw.transition_hp, tw.reward_hp)
        assert (np.abs(T_d.astype(np.float64) - T) <= tol_T).all(), (b, tw.episode, np.abs(T_d - T).max())
        assert (np.abs(R_d.astype(np.float64) - R) <= tol_R).all(), (b, tw.episode, np.abs(R_d - R).max())
        rs = T_d.astype(np.float64).sum(-1)
        assert (np.abs(rs - row_target) <= (tw.S + 4) * U).all(), (b, tw.episode, np.abs(rs - row_target).max())
        assert (T_d >= 0).all()
        return T_d, R_d

    def check_q64(self, b):
        """The float64 restatement costs a Python loop over the states per sweep: the first three solves of an instance and
        every `q64_every`-th after them are held against it; the bit-equality with the stand-alone entry, which is held
        against it in the solver tests above, covers every solve."""
        k = int(self.n_solves[b])
        return k < 3 or k % self.q64_every == 0

    def after_rounds(self, ended):
        """The instances in `ended` have just sampled and solved: their twins do the same with the device's Q injected."""
        if not ended:
            return
        ls = self.agent.last_sample()
        for b in ended:
            self.pending[b] = (ls["T"][b], ls["R"][b], ls["Q"][b].copy())
            self.twins[b].episode_end_update()
        outs = dp.discounted_value_iteration_dense_batch([(ls["T"][b], ls["R"][b]) for b in ended],
                                                         sparse_n_states_threshold=self.agent_threshold())
        for b, (Q, V, n, used) in zip(ended, outs):
            assert np.array_equal(Q, ls["Q"][b]), b      # the same kernel on the host-packed form of the same inputs
            assert n == ls["sweeps"][b] and used == ls["scheme"][b] and ls["status"][b] == 0, b
            T = ls["T"][b]
            assert used == vi_rule(T.shape[0], T.shape[1], int((T != 0).sum()), self.agent_threshold()), b
            if self.check_q64(b):
                self.worst = max(self.worst, check_solve(T, ls["R"][b], Q, V, n, used, GAMMA32, EPS))
                self.n_q64 += 1
            self.n_solves[b] += 1

    def agent_threshold(self):
        return getattr(self, "size_threshold", 300 * 3 * 300)

    def compare_models(self):
        m = self.agent.model()
        for b, tw in enumerate(self.twins):
            assert np.array_equal(m["transitions"][b], tw.transition_hp), b
            assert np.array_equal(m["rewards"][b], tw.reward_hp), b
            assert np.array_equal(m["N_sa"][b], tw.N.sum(-1)) and np.array_equal(m["nu_k"][b], tw.nu_k()), b
            assert m["episode"][b] == tw.episode, b
        return m

    def call(self, n, train=True, stop=True):
        """One run(n, stop_at_episode_end=stop, trace=True) and its checks; returns steps_taken.  An instance that trains must
        not end an episode before its last step of the call (its Q changes there): stop, or a call short enough."""
        B = self.env.B
        mask = np.broadcast_to(np.asarray(train, bool), (B,))
        out = self.agent.run(n, train=train, trace=True, stop_at_episode_end=stop)
        taken = out["steps_taken"]
        ep_after = self.agent.model()["episode"]
        ended = []
        for b in range(B):
            tw, k = self.twins[b], int(taken[b])
            assert 1 <= k <= n, b
            s = int(self.cur[b])
            end = False
            for i in range(k):
                a, s2, r = int(out["actions"][i, b]), int(out["observations"][i, b]), float(out["rewards"][i, b])
                assert not end, (b, i, "the device walked on under the old Q after an episode end")
                assert tw.select_action(s) == a, (b, i)
                self.actions[b].append(a)
                assert 0 <= s2 < tw.S
                if mask[b]:
                    tw.step_update(s, a, r, s2)
                    end = tw.is_episode_end(s, a)
                s = s2
            if mask[b]:
                assert end == (ep_after[b] == self.episodes[b] + 1), b
                assert end or k == n, b              # stopped early only by an episode end
                if end:
                    ended.append(b)
            else:
                assert k == n and ep_after[b] == self.episodes[b], b
            self.cur[b] = s
        assert np.array_equal(self.env.state()[0], self.cur)
        self.after_rounds(ended)
        self.episodes = ep_after.copy()
        self.compare_models()
        return taken

    def follow(self, T, chunk=64):
        done = np.zeros(self.env.B, np.int64)
        while done.min() < T:
            done += self.call(chunk)
        return done


def build(models, rng, sampler, beta=False, seeds=None, rprm=None, tprm=None, env=None, **fkw):
    env = env or make_env(models, rng, beta)
    seeds = np.arange(len(models)) + 11 if seeds is None else seeds
    kw = {}
    if rprm is not None:
        kw.update(reward_prior_model="N_NIG", rewards_prior_prms=rprm)
    if tprm is not None:
        kw.update(transitions_prior_model="M_DIR", transitions_prior_prms=tprm)
    agent = BatchedPSRLContinuous(env, seeds, 100_000, sampler=sampler, no_optimistic_sampling=True, **kw)
    return env, agent, Follower(env, agent, seeds, sampler, rprm, tprm, **fkw)


G22_RUNS = [(0, "mt"), (1, "philox"), (2, "mt"), (3, "philox"), (4, "mt"), (5, "mt")]


@pytest.mark.parametrize("case,rng", G22_RUNS, ids=[f"c{c}_{r}" for c, r in G22_RUNS])
def test_g22_mdps_full_length_reference_sampler(need_gpu, case, rng):
    z, meta = g22()
    m = meta[case]
    model = make_model(m["cls"], **m["params"])
    assert (model.n_states, model.n_actions) == (m["S"], m["A"])
    env, agent, f = build([model], rng, "reference", beta=bool(m["params"].get("make_reward_stochastic")), seeds=[m["seed"]],
                          rprm=m["rewards_prior_prms"], tprm=m["transitions_prior_prms"], q64_every=16)
    f.follow(m["T"])
    # reported, not asserted: the first step at which the device's action stream leaves the reference's (the solve is not
    # BLAS's and stops a sweep earlier or later; with another environment stream the trajectories differ from the start)
    ref = z[f"c{case}_steps"][:, 1]
    mine = np.array(f.actions[0][:len(ref)])
    d = np.flatnonzero(mine != ref[:len(mine)])
    print(f"case {case} ({rng}): {int(f.n_solves[0])} solves ({f.n_q64} against float64, worst |Q - Q64| / bound {f.worst:.3f}); "
          f"actions leave the reference's at step {int(d[0]) if len(d) else None} of {len(mine)}")
    st = agent.stats()
    assert st["solves"] == f.n_solves[0] and st["reference_ms"] > 0 and st["unconverged"] == 0 and st["sweeps"] > 0
    env.close()


@pytest.mark.parametrize("sampler", ["reference", "philox"])
@pytest.mark.parametrize("rng", ["mt", "philox"])
def test_uniform_batch(need_gpu, rng, sampler):
    models = [make_model("DeepSeaContinuous", seed=s, size=4, p_rand=0.2) for s in range(6)]
    assert len({m.n_states for m in models}) == 1
    env, agent, f = build(models, rng, sampler)
    # every instance is stopped at its own episode ends, so the followed instances end at different step counts
    done = f.follow(30 if sampler == "philox" else 60, chunk=16)
    m1, l1, cur1 = agent.model(), agent.last_sample(), env.state()[0]
    # the same steps in calls that do NOT stop (walk, round, walk, ... inside cmdp_psrlc_run) on a fresh equal batch: where an
    # instance has taken the steps of its followed run it has the same actions, tables, counters, sample, Q and state
    env2 = make_env(models, rng, False)
    agent2 = BatchedPSRLContinuous(env2, f.seeds, 100_000, sampler=sampler, no_optimistic_sampling=True)
    at, acts = 0, []
    for d in sorted(set(done.tolist())):
        out = agent2.run(d - at, trace=True)
        assert (out["steps_taken"] == d - at).all()
        acts.append(out["actions"])
        at = d
        m2, l2, cur2 = agent2.model(), agent2.last_sample(), env2.state()[0]
        for b in np.flatnonzero(done == d):
            for k in ("transitions", "rewards", "N_sa", "nu_k"):
                assert np.array_equal(m1[k][b], m2[k][b]), (k, b)
            for k in ("T", "R", "Q"):
                assert np.array_equal(l1[k][b], l2[k][b]), (k, b)
            assert m1["episode"][b] == m2["episode"][b] and cur1[b] == cur2[b], b
    acts = np.concatenate(acts)
    for b in range(env.B):
        assert np.array_equal(acts[:done[b], b], np.array(f.actions[b])), b
    env.close()
    env2.close()


@pytest.mark.parametrize("sampler", ["reference", "philox"])
def test_ragged_batch_with_beta_rewards(need_gpu, sampler):
    """Different S_b at one A in one batch; Beta rewards drawn on the device (philox) and as means (mt)."""
    models = [make_model("FrozenLakeContinuous", seed=s, size=size, p_frozen=0.9, make_reward_stochastic=True)
              for s, size in enumerate((3, 4, 5))]
    assert len({m.n_states for m in models}) == 3
    for rng in ("philox", "mt"):
        env, agent, f = build(models, rng, sampler, beta=True, tprm=[0.4], rprm=[0.5, 2, 1.5, 3])
        f.follow(30, chunk=16)
        env.close()


def test_philox_rows_longer_than_a_wavefront(need_gpu):
    """FrozenLake of size 9 (73 states once the holes are gone, > 64): several columns per lane in k_psrl_sample, row * S +
    column beyond one wavefront; scalar loads in the solver (73 is odd)."""
    models = [make_model("FrozenLakeContinuous", seed=0, size=9, p_frozen=0.9)]
    assert models[0].n_states > 64 and models[0].n_states % 4
    env, agent, f = build(models, "philox", "philox", q64_every=4)
    f.follow(6, chunk=4)
    env.close()


def test_philox_sample_is_a_pure_function(need_gpu):
    """Two agents on equal batches give equal bits; a batch split in two gives the same per-instance samples."""
    mk = lambda: [make_model("DeepSeaContinuous", seed=s, size=4) for s in range(4)]  # noqa: E731
    seeds = np.array([3, 4, 5, 6])
    keys = np.arange(4, dtype=np.uint64) * 7919 + 5

    def run(models, seeds, keys):
        env = make_env(models, "philox", False, keys=keys)
        ag = BatchedPSRLContinuous(env, seeds, 1000, sampler="philox", no_optimistic_sampling=True)
        ag.run(50)
        out = ag.last_sample(), ag.model()
        env.close()
        return out

    a, ma = run(mk(), seeds, keys)
    b, mb = run(mk(), seeds, keys)
    lo, mlo = run(mk()[:2], seeds[:2], keys[:2])
    hi, mhi = run(mk()[2:], seeds[2:], keys[2:])
    for k in ("T", "R", "Q"):
        for i in range(4):
            assert np.array_equal(a[k][i], b[k][i]), (k, i)
            assert np.array_equal(a[k][i], (lo if i < 2 else hi)[k][i % 2]), (k, i)
    assert (ma["episode"] > 2).all() and np.array_equal(ma["episode"], mb["episode"])
    assert np.array_equal(ma["transitions"][3], mhi["transitions"][1]) and np.array_equal(ma["nu_k"][0], mlo["nu_k"][0])


def test_train_false_mask_stop_and_external_update(need_gpu):
    models = [make_model("RiverSwimContinuous", seed=s, size=5) for s in range(4)]
    env, agent, f = build(models, "philox", "reference")
    f.follow(30, chunk=8)
    # frozen: tables, counters, Q and the sample stay, nothing is drawn, nobody parks
    before, ls0 = agent.model(), agent.last_sample()
    f.call(7, train=False, stop=False)
    f.call(5, train=False, stop=True)
    after, ls1 = agent.model(), agent.last_sample()
    for b in range(4):
        for k in ("transitions", "rewards", "N_sa", "nu_k"):
            assert np.array_equal(before[k][b], after[k][b]), (k, b)
        assert np.array_equal(ls0["Q"][b], ls1["Q"][b]) and np.array_equal(ls0["T"][b], ls1["T"][b])
    assert np.array_equal(before["episode"], after["episode"])
    # a per-instance mask: the frozen ones take every step of the call, the others stop at their episode ends
    f.call(6, train=np.array([True, False, True, False]), stop=True)
    # an external episode_end_update(): one more sample for every instance, every nu_k back to 0, N.sum(-1) kept
    m0 = f.compare_models()
    assert any(x.any() for x in m0["nu_k"])
    agent.episode_end_update()
    f.after_rounds(list(range(4)))
    f.episodes = agent.model()["episode"].copy()
    m1 = f.compare_models()
    assert np.array_equal(m1["episode"], m0["episode"] + 1) and not any(x.any() for x in m1["nu_k"])
    assert all(np.array_equal(x, y) for x, y in zip(m0["N_sa"], m1["N_sa"]))
    f.follow(12, chunk=8)
    # stop off: the call takes all its steps across episode ends; the model's updates do not depend on Q, so the twins
    # replay them and count the episodes the reference's rule ends
    n = 40
    ep0 = agent.model()["episode"].copy()
    out = agent.run(n, trace=True, stop_at_episode_end=False)
    assert (out["steps_taken"] == n).all()
    for b, tw in enumerate(f.twins):
        s, ends = int(f.cur[b]), 0
        for i in range(n):
            a, s2 = int(out["actions"][i, b]), int(out["observations"][i, b])
            tw.step_update(s, a, float(out["rewards"][i, b]), s2)
            if tw.is_episode_end(s, a):
                tw.episode_transition_data = dict()
                ends += 1
            s = s2
        m = agent.model()
        assert m["episode"][b] == ep0[b] + ends and ends > 0, b
        assert np.array_equal(m["transitions"][b], tw.transition_hp) and np.array_equal(m["rewards"][b], tw.reward_hp), b
        assert np.array_equal(m["N_sa"][b], tw.N.sum(-1)) and np.array_equal(m["nu_k"][b], tw.nu_k()), b
    env.close()


def test_scheme_rule_inside_the_agent(need_gpu):
    """At a lowered size threshold the agent's own solves take Jacobi on the mostly-zero samples of a small prior and
    Gauss-Seidel on dense ones, per instance in the same rounds."""
    models = [make_model("FrozenLakeContinuous", seed=s, size=4, p_frozen=0.9) for s in range(2)]
    env = make_env(models, "mt", False)
    seeds = [5, 6]
    agent = BatchedPSRLContinuous(env, seeds, 1000, transitions_prior_model="M_DIR", transitions_prior_prms=[0.001],
                                  no_optimistic_sampling=True)
    agent._set_size_threshold(100)
    f = Follower(env, agent, seeds, "reference", None, [0.001], q64_every=4)
    f.size_threshold = 100
    f.follow(20, chunk=8)
    ls = agent.last_sample()
    assert (ls["scheme"] == JACOBI).all() and any((T.sum(-1) == 0).any() for T in ls["T"])
    env.close()
    dense = make_env(models, "mt", False)
    agent = BatchedPSRLContinuous(dense, seeds, 1000, no_optimistic_sampling=True)
    agent._set_size_threshold(100)
    agent.run(20)
    assert (agent.last_sample()["scheme"] == GAUSS_SEIDEL).all()
    # a solve that reaches the sweep limit keeps the last sweep's Q and is counted
    agent._set_max_sweeps(2)
    un0 = agent.stats()["unconverged"]
    agent.episode_end_update()
    ls = agent.last_sample()
    assert (ls["status"] == L.ERR_MAX_ITER).all() and (ls["sweeps"] == 2).all()
    st = agent.stats()
    assert st["unconverged"] == un0 + 2 and st["sweeps"] == 4
    outs = dp.discounted_value_iteration_dense_batch(list(zip(ls["T"], ls["R"])), sparse_n_states_threshold=100, max_sweeps=2)
    assert all(np.array_equal(o[0], q) for o, q in zip(outs, ls["Q"]))
    dense.close()


def undecided_states(Q64, bound):
    """States where the gap between the best and the second-best DISTINCT float64 value does not exceed 2 * bound."""
    out = np.zeros(len(Q64), bool)
    for s, q in enumerate(Q64):
        v = np.unique(q)
        out[s] = len(v) > 1 and v[-1] - v[-2] <= 2 * bound
    return out


def test_policy_solve_and_average_reward_against_the_host_route(need_gpu):
    """policy() / policy_solve() / average_reward() against map_estimate -> dp.discounted_value_iteration ->
    get_policy_from_q_values -> BatchedMDP.average_reward.  The trained agents (three FrozenLake instances after 400 steps,
    reference sampler, fixed seeds) were chosen so that at most 5 % of the batch's states are undecided; that condition is
    computed on the CPU from the float64 restatement alone and asserted below."""
    models = [make_model("FrozenLakeContinuous", seed=i, size=4, p_frozen=0.9) for i in range(3)]
    env = make_env(models, "philox", False)
    agent = BatchedPSRLContinuous(env, [21, 22, 23], 10_000, no_optimistic_sampling=True)
    agent.run(400)
    ls0, m0 = agent.last_sample(), agent.model()
    maps = agent.map_estimate()
    sol = agent.policy_solve()
    pis = agent.current_optimal_stochastic_policy()
    avg = agent.average_reward()
    assert len(pis) == 3 and len(avg) == 3
    # nothing the agent acts or learns with has moved
    ls1, m1 = agent.last_sample(), agent.model()
    for b in range(3):
        assert all(np.array_equal(ls0[k][b], ls1[k][b]) for k in ("T", "R", "Q"))
        assert all(np.array_equal(m0[k][b], m1[k][b]) for k in ("transitions", "rewards", "N_sa", "nu_k"))
    host_pi, decided_all, n_und, n_states = [], [], 0, 0
    for b, (T_map, R_map) in enumerate(maps):
        S = int(env.n_states[b])
        assert T_map.dtype == np.float32 and R_map.dtype == np.float32
        Q, n, used = sol["Q"][b], int(sol["sweeps"][b]), int(sol["scheme"][b])
        assert used == GAUSS_SEIDEL
        # the device's dense MAP model is the host's, bit for bit: the stand-alone entry on map_estimate() gives the same Q
        (Qs, Vs, ns, us), = dp.discounted_value_iteration_dense_batch([(T_map, R_map)])
        assert np.array_equal(Qs, Q) and ns == n, b
        check_solve(T_map, R_map, Q, Q.max(-1), n, used, GAMMA32, EPS)
        Q64, _, _, qmax = vi_discounted_f64(T_map, R_map, GAMMA32, used, n)
        # The host route runs the same sweeps from V = 0 with float32 chains over the S entries of a row: every product and
        # every partial sum rounded, (S + 3) U max(1, qmax) per sweep and row (helpers_psrl.bound_episodic's BLAS line),
        # propagated as in bound_discounted.  It may stop a sweep earlier or later than the device: the float64 restatement
        # at ITS sweep count says by how much that moves Q.  All of it is computed from the float64 restatement alone.
        Qh, _, nh = dp._handle(T_map, R_map).value_iteration(0.99, EPS, L.SCHEME_GAUSS_SEIDEL, dp.DP_MAX_ITERATION)
        nh = int(np.ravel(nh)[0])
        Qh = Qh.reshape(S, 4)
        assert np.array_equal(Qh, dp.discounted_value_iteration(T_map, R_map)[0])
        Q64h, _, _, _ = vi_discounted_f64(T_map, R_map, GAMMA32, used, nh)
        bound_h = (S + 3) * U * max(1.0, qmax) * (1 - GAMMA32 ** nh) / (1 - GAMMA32) * (1 + 2.0 ** -20)
        bound = max(bound_discounted(n, GAMMA32, qmax, S), bound_h + float(np.abs(Q64h - Q64).max()))
        assert np.abs(Qh.astype(np.float64) - Q64).max() <= bound, b    # Q agrees within the bound
        und = undecided_states(Q64, bound)
        pi_h = dp.get_policy_from_q_values(Qh, True)
        pi = pis[b]
        assert pi.shape == (S, 4) and np.array_equal(pi.sum(1), np.ones(S)) and set(np.unique(pi)) == {0.0, 1.0}
        assert np.array_equal(pi, dp.argmax_2d(Q)), b          # the device's argmax of the device's Q
        assert np.array_equal(pi[~und], pi_h[~und]), b
        host_pi.append(pi_h)
        decided_all.append(not und.any())
        n_und += int(und.sum())
        n_states += S
    assert n_und <= 0.05 * n_states, (n_und, n_states)
    ref, _ = env.average_reward([p.argmax(-1) for p in host_pi], env.state()[0])
    for b in range(3):
        if decided_all[b]:
            assert avg[b] == ref[b] and type(avg[b]) is type(ref[b]), b
    print(f"undecided states {n_und} of {n_states}; instances compared on average reward: {sum(decided_all)}")
    # a mask: the selected instances only, zeros elsewhere
    mask = np.array([0, 1, 0], bool)
    one = agent.policy(mask)
    assert len(one) == 1 and np.array_equal(one[0], pis[1])
    sm = agent.policy_solve(mask)
    assert np.array_equal(sm["Q"][1], sol["Q"][1]) and not sm["Q"][0].any() and sm["sweeps"][0] == 0
    assert agent.average_reward(mask)[0] == avg[1]
    assert agent.stats()["policy_kernel_ms"] > 0
    env.close()


def test_refusals(need_gpu):
    lib = L.load()

    def refused(env, code, word, **kw):
        with pytest.raises(L.CmdpError) as ei:
            BatchedPSRLContinuous(env, np.arange(env.B), 1000, no_optimistic_sampling=True, **kw)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    env = BatchedMDP([make_model("DeepSeaEpisodic", seed=0, size=4)])
    env.reset()
    refused(env, L.ERR_UNSUPPORTED, "episodic")
    env.close()
    m = make_model("DeepSeaContinuous", seed=0, size=4, make_reward_stochastic=True)
    env = BatchedMDP([m], flags=L.FLAG_REWARD_CACHE)
    env.reset()
    refused(env, L.ERR_UNSUPPORTED, "REWARD_CACHE")
    env.close()
    env = BatchedMDP([make_model("MiniGridEmptyContinuous", seed=0, size=33)], with_dp=False)   # 33 * 33 * 4 = 4356 states
    assert env.n_states[0] > 4096
    env.reset()
    refused(env, L.ERR_UNSUPPORTED, "4096")
    env.close()
    cont = make_env([make_model("RiverSwimContinuous", seed=0, size=5)], "mt", False)
    with pytest.raises(L.CmdpError) as e:   # ... and the episodic agent points at this one
        BatchedPSRLEpisodic(cont, [0], 100)
    assert e.value.code == L.ERR_UNSUPPORTED and "cmdp_psrlc_create" in str(e.value)
    h = C.c_void_p()
    seeds, rp, tp = np.zeros(1, np.int32), np.ones(4, np.float32), np.ones(1, np.float32)
    for actor in (L.ACTOR_EPSILON_GREEDY, L.ACTOR_BOLTZMANN):
        assert lib.cmdp_psrlc_create(C.byref(h), cont._h, L.ptr(seeds), 100, L.ptr(rp), L.ptr(tp), 0, actor) == L.ERR_UNSUPPORTED
    for bad in (np.array([1, 1, 0, 1], np.float32), np.array([np.nan, 1, 1, 1], np.float32), np.array([1, -1, 1, 1], np.float32)):
        assert lib.cmdp_psrlc_create(C.byref(h), cont._h, L.ptr(seeds), 100, L.ptr(bad), L.ptr(tp), 0, 0) == L.ERR_INVALID
    for bad in (np.zeros(1, np.float32), np.array([np.inf], np.float32)):
        assert lib.cmdp_psrlc_create(C.byref(h), cont._h, L.ptr(seeds), 100, L.ptr(rp), L.ptr(bad), 0, 0) == L.ERR_INVALID
    assert not h.value
    agent = BatchedPSRLContinuous(cont, [0], 100, no_optimistic_sampling=True)
    with pytest.raises(L.CmdpError) as e:
        agent.run(1 << 25)
    assert e.value.code == L.ERR_OVERFLOW
    with pytest.raises(L.CmdpError) as e:
        agent.run((1 << 24) + 1)
    assert e.value.code == L.ERR_OVERFLOW and "2^24" in str(e.value)
    with pytest.raises(NotImplementedError):
        agent.run_logged(None, 1)
    cont.close()


def test_agent_destroyed_after_its_environment(need_gpu):
    """Garbage collection picks the order: cmdp_destroy orphans the handle's agents, which then refuse to run and free
    only their own memory."""
    env = make_env([make_model("DeepSeaContinuous", seed=0, size=4)], "mt", False)
    agent = BatchedPSRLContinuous(env, [0], 100, no_optimistic_sampling=True)
    agent.run(50)
    env._agents = []   # as when the weak references are already dead
    env.close()
    with pytest.raises(L.CmdpError) as ei:
        agent.run(10)
    assert ei.value.code == L.ERR_INVALID
    with pytest.raises(L.CmdpError):
        agent.policy()
    agent.close()
