"""The device PSRL agent (K12, colosseum_amd.agents.BatchedPSRLEpisodic) against the NumPy twin of tests/helpers_psrl.py,
which tests/test_psrl.py holds against the reference bit for bit.

The solve is not the reference's BLAS product, so trajectories are not compared with the reference's: the twin is fed the
DEVICE's transitions, episode by episode (run(stop_at_episode_end=True, trace=True)), and after every call, for every
instance:
  * every action is the twin actor's choice under the Q the device held (tie-break stream included) and the episode ended
    at the step the environment's horizon gives;
  * model() equals the twin's two hyper-parameter arrays bit for bit;
  * last_sample()'s T and R equal the twin's own numpy draws bit for bit (reference sampler) or the helper's restatement of
    k_psrl_sample within the tolerance derived there (Philox sampler);
  * the new Q is bit-equal to episodic_value_iteration_dense_batch on the same (T, R) and within
    bound_episodic(H, qmax, 1) of the float64 restatement."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from helpers_psrl import (MOMENT_REWARD_PRIOR, MOMENT_SAMPLES, U, PSRLTwin, bound_episodic, check_all_rows, numpy_sampler,
                          philox_sample, vi_episodic_f64)
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp
from colosseum_amd.agents import BatchedPSRLEpisodic
from colosseum_amd.batched import BatchedMDP
from colosseum_amd.mdp import make_model

pytestmark = pytest.mark.gpu

G20 = os.path.join(ROOT, "tests", "golden", "G20_psrl.npz")


def g20():
    z = np.load(G20)
    return z, json.loads(str(z["cases"]))


def make_env(models, rng, beta, reset=True):
    """rng "mt": CMDP_RNG_MT_COMPAT (Beta rewards reported as their means); "philox": Beta rewards drawn on the device."""
    if rng == "mt":
        env = BatchedMDP(models, rng_mode=L.RNG_MT_COMPAT, flags=L.FLAG_REWARD_MEANS if beta else 0)
    else:
        env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=np.arange(len(models), dtype=np.uint64) * 7919 + 5)
    if reset:
        env.reset()
    return env


class Follower:
    """The twins of a batch and the checks of one call."""

    def __init__(self, env, agent, seeds, sampler, rprm=None, tprm=None):
        self.env, self.agent, self.sampler, self.seeds = env, agent, sampler, [int(s) for s in seeds]
        self.H = int(env.H)
        self.pending = [None] * env.B
        self.twins = []
        for b in range(env.B):
            self.twins.append(PSRLTwin(self.seeds[b], int(env.n_states[b]), env.A, self.H, env.rewards_range[1],
                                       (lambda H, T, R, _b=b: self.pending[_b][2]),
                                       sampler=(lambda tw, _b=b: self.twin_sample(_b, tw)), rewards_prior_prms=rprm,
                                       transitions_prior_prms=tprm))
        self.cur, self.h = (x.copy() for x in env.state()[:2])
        self.actions = [[] for _ in range(env.B)]
        self.episodes = agent.model()["episode"].copy()
        assert (self.episodes == 1).all()
        self.n_solves = 0
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
        # every row sums to sum / (1e-5 + sum) within the rounding derived in helpers_psrl.philox_sample
        rs = T_d.astype(np.float64).sum(-1)
        assert (np.abs(rs - row_target) <= (tw.S + 4) * U).all(), (b, tw.episode, np.abs(rs - row_target).max())
        assert (T_d >= 0).all()
        return T_d, R_d

    def after_rounds(self, ended):
        """The instances in `ended` have just sampled and solved: their twins do the same with the device's Q injected."""
        if not ended:
            return
        ls = self.agent.last_sample()
        for b in ended:
            self.pending[b] = (ls["T"][b], ls["R"][b], ls["Q"][b].copy())
            self.twins[b].episode_end_update()
        outs = dp.episodic_value_iteration_dense_batch([(ls["T"][b], ls["R"][b]) for b in ended], self.H)
        for b, (Q, V) in zip(ended, outs):
            assert np.array_equal(Q, ls["Q"][b]), b      # the same kernel on the host-packed form of the same inputs
            assert np.array_equal(V, Q.max(-1)) and (Q[self.H] == 0).all(), b
            Q64, _, qmax = vi_episodic_f64(self.H, ls["T"][b], ls["R"][b])
            err, tol = float(np.abs(ls["Q"][b] - Q64).max()), bound_episodic(self.H, qmax, 1)
            self.worst = max(self.worst, err / tol)
            self.n_solves += 1
            assert err <= tol, (b, err, tol)

    def compare_models(self):
        m = self.agent.model()
        for b, tw in enumerate(self.twins):
            assert np.array_equal(m["transitions"][b], tw.transition_hp), b
            assert np.array_equal(m["rewards"][b], tw.reward_hp), b
            assert m["episode"][b] == tw.episode, b
        return m

    def call(self, n, train=True, stop=True):
        """One run(n, stop_at_episode_end=stop, trace=True) and its checks; returns steps_taken."""
        B, H = self.env.B, self.H
        mask = np.broadcast_to(np.asarray(train, bool), (B,))
        out = self.agent.run(n, train=train, trace=True, stop_at_episode_end=stop)
        taken = out["steps_taken"]
        ep_after = self.agent.model()["episode"]
        ended = []
        for b in range(B):
            tw, k = self.twins[b], int(taken[b])
            assert 1 <= k <= n, b
            if not mask[b]:
                assert k == n and ep_after[b] == self.episodes[b], b
            s, h = int(self.cur[b]), int(self.h[b])
            for i in range(k):
                a, s2, r = int(out["actions"][i, b]), int(out["observations"][i, b]), float(out["rewards"][i, b])
                assert tw.select_action(h, s) == a, (b, i)
                self.actions[b].append(a)
                last = h + 1 >= H
                assert (s2 == -1) == last, (b, i, h)   # the episode ends where the environment's horizon says
                if mask[b]:
                    tw.step_update(s, a, r, s2, last)
                    if last:
                        assert stop and i == k - 1, "only the episode-by-episode loop is followed"
                        ended.append(b)
                if last:
                    assert i == k - 1 or not mask[b], (b, i)
                    s, h = None, 0   # the state after the reset is the environment's to say
                    if i < k - 1:
                        pytest.fail("a frozen instance crossed an episode end inside one followed call: use calls of <= H steps")
                else:
                    s, h = s2, h + 1
            if stop and k < n:
                assert ep_after[b] == self.episodes[b] + 1, b
        cur, hh, _ = self.env.state()
        for b in range(B):
            if int(self.h[b]) + int(taken[b]) < H:   # no reset in between: the walk's last observation
                assert hh[b] == self.h[b] + taken[b], b
            else:
                assert hh[b] == 0, b
        self.cur, self.h = cur.copy(), hh.copy()
        self.after_rounds(ended)
        self.episodes = ep_after.copy()
        self.compare_models()
        return taken

    def follow(self, T):
        done = np.zeros(self.env.B, np.int64)
        while done.min() < T:
            done += self.call(self.H)
        return done


def build(models, rng, sampler, beta=False, seeds=None, rprm=None, tprm=None, env=None):
    env = env or make_env(models, rng, beta)
    seeds = np.arange(len(models)) + 11 if seeds is None else seeds
    kw = {}
    if rprm is not None:
        kw.update(reward_prior_model="N_NIG", rewards_prior_prms=rprm)
    if tprm is not None:
        kw.update(transitions_prior_model="M_DIR", transitions_prior_prms=tprm)
    agent = BatchedPSRLEpisodic(env, seeds, 100_000, sampler=sampler, **kw)
    return env, agent, Follower(env, agent, seeds, sampler, rprm, tprm)


# G20's MDPs for their full length with the reference sampler: case -> environment flavour
G20_RUNS = [(0, "mt"), (1, "philox"), (2, "mt"), (3, "philox"), (3, "mt"), (4, "philox")]


@pytest.mark.parametrize("case,rng", G20_RUNS, ids=[f"c{c}_{r}" for c, r in G20_RUNS])
def test_g20_mdps_full_length_reference_sampler(need_gpu, case, rng):
    z, meta = g20()
    m = meta[case]
    model = make_model(m["cls"], **m["params"])
    assert (model.n_states, model.n_actions) == (m["S"], m["A"])
    env, agent, f = build([model], rng, "reference", beta=bool(m["params"].get("make_reward_stochastic")), seeds=[m["seed"]],
                          rprm=m["rewards_prior_prms"], tprm=m["transitions_prior_prms"])
    assert env.H == m["H"]
    f.follow(m["T"])
    # reported, not asserted: the first step at which the device's action stream leaves the reference's (the solve is not
    # BLAS's, a near-tie may part the two; with another environment stream the trajectories differ from the start)
    ref = z[f"c{case}_steps"][:, 2]
    mine = np.array(f.actions[0][:len(ref)])
    d = np.flatnonzero(mine != ref[:len(mine)])
    print(f"case {case} ({rng}): {f.n_solves} solves, worst |Q - Q64| / bound {f.worst:.3f}; actions leave the reference's at "
          f"step {int(d[0]) if len(d) else None} of {len(mine)}")
    st = agent.stats()
    assert st["solves"] == f.n_solves and st["reference_ms"] > 0


@pytest.mark.parametrize("sampler", ["reference", "philox"])
@pytest.mark.parametrize("rng", ["mt", "philox"])
def test_uniform_batch(need_gpu, rng, sampler):
    models = [make_model("DeepSeaEpisodic", seed=s, size=5, p_rand=0.2) for s in range(6)]
    assert len({m.n_states for m in models}) == 1
    env, agent, f = build(models, rng, sampler)
    done = f.follow(60 if sampler == "philox" else 150)
    # the same steps in ONE call (walk, round, walk, ... inside cmdp_psrl_run) on a fresh equal batch: the same actions,
    # tables, sample and Q as the episode-by-episode run that was followed
    assert len(set(done.tolist())) == 1
    env2 = make_env(models, rng, False)
    agent2 = BatchedPSRLEpisodic(env2, f.seeds, 100_000, sampler=sampler)
    out = agent2.run(int(done[0]), trace=True)
    assert (out["steps_taken"] == done).all()
    m1, m2, l1, l2 = agent.model(), agent2.model(), agent.last_sample(), agent2.last_sample()
    for b in range(env.B):
        assert np.array_equal(out["actions"][:, b], np.array(f.actions[b])), b
        for k in ("transitions", "rewards"):
            assert np.array_equal(m1[k][b], m2[k][b]), (k, b)
        for k in ("T", "R", "Q"):
            assert np.array_equal(l1[k][b], l2[k][b]), (k, b)
    assert np.array_equal(m1["episode"], m2["episode"]) and np.array_equal(env.state()[0], env2.state()[0])


def test_philox_rows_longer_than_a_wavefront(need_gpu):
    """S > 64: several columns per lane in k_psrl_sample, row * S + column beyond one wavefront, ragged S."""
    models = [make_model("FrozenLakeEpisodic", seed=s, size=12, p_frozen=0.9, H=16) for s in range(2)]
    assert min(m.n_states for m in models) > 64
    env, agent, f = build(models, "philox", "philox")
    f.follow(2 * env.H)


@pytest.mark.parametrize("sampler", ["reference", "philox"])
def test_ragged_batch_with_beta_rewards(need_gpu, sampler):
    """Different S_b in one batch (H must be shared: DeepSea's horizon is its size, so the family is mixed at one horizon);
    Beta rewards drawn on the device (philox) and as means (mt)."""
    mk = lambda size, seed: make_model("RiverSwimEpisodic", seed=seed, size=size, H=8, make_reward_stochastic=True)  # noqa: E731
    models = [mk(4, 0), mk(7, 1), mk(5, 2), mk(8, 3)]
    assert len({m.n_states for m in models}) == 4
    for rng in ("philox", "mt"):
        env, agent, f = build(models, rng, sampler, beta=True, tprm=[0.4], rprm=[0.5, 2, 1.5, 3])
        f.follow(48)


def test_philox_sample_is_a_pure_function(need_gpu):
    """Two agents on equal batches give equal bits; a batch split in two gives the same per-instance samples."""
    mk = lambda: [make_model("DeepSeaEpisodic", seed=s, size=4) for s in range(4)]  # noqa: E731
    seeds = np.array([3, 4, 5, 6])
    keys = np.arange(4, dtype=np.uint64) * 7919 + 5

    def run(models, seeds, keys):
        env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=keys)
        env.reset()
        ag = BatchedPSRLEpisodic(env, seeds, 1000, sampler="philox")
        ag.run(5 * env.H)
        ls, m = ag.last_sample(), ag.model()
        return ls, m

    a, ma = run(mk(), seeds, keys)
    b, mb = run(mk(), seeds, keys)
    lo, mlo = run(mk()[:2], seeds[:2], keys[:2])
    hi, mhi = run(mk()[2:], seeds[2:], keys[2:])
    for k in ("T", "R", "Q"):
        for i in range(4):
            assert np.array_equal(a[k][i], b[k][i]), (k, i)
            assert np.array_equal(a[k][i], (lo if i < 2 else hi)[k][i % 2]), (k, i)
    assert (ma["episode"] == 6).all() and np.array_equal(ma["transitions"][3], mhi["transitions"][1])


def test_dense_solver_against_the_reference(need_gpu):
    """cmdp_vi_episodic_dense on every (T, R) stored in G20 within bound_episodic(H, qmax, S) of the Q the reference recorded."""
    z, meta = g20()
    for i, m in enumerate(meta):
        kept = z[f"c{i}_kept"]
        outs = dp.episodic_value_iteration_dense_batch(list(zip(z[f"c{i}_T"], z[f"c{i}_R"])), m["H"])
        for j, k in enumerate(kept):
            _, _, qmax = vi_episodic_f64(m["H"], z[f"c{i}_T"][j], z[f"c{i}_R"][j])
            err, tol = np.abs(outs[j][0] - z[f"c{i}_Q"][k]).max(), bound_episodic(m["H"], qmax, m["S"])
            assert err <= tol, (i, int(k), err, tol)


def test_dense_solver_large_and_unaligned(need_gpu):
    """Row lengths that are and are not multiples of four (16-byte and scalar loads), several loads per lane, ragged."""
    rng = np.random.RandomState(0)
    probs = []
    for S, A in ((3, 2), (64, 3), (257, 2), (1024, 2), (130, 5)):
        T = rng.gamma(0.3, size=(S, A, S)).astype(np.float32)
        T = T / (np.float32(1e-5) + T.sum(-1, keepdims=True))
        probs.append((T, rng.normal(size=(S, A)).astype(np.float32)))
    for (T, R), (Q, V) in zip(probs, dp.episodic_value_iteration_dense_batch(probs, 12)):
        Q64, V64, qmax = vi_episodic_f64(12, T, R)
        assert np.abs(Q - Q64).max() <= bound_episodic(12, qmax, 1) and np.array_equal(V, Q.max(-1))


def test_philox_distribution(need_gpu):
    """The posterior sample of many episodes and instances at fixed tables: two instances are trained for some episodes (so
    Dirichlet parameters lie below and above one and the visited N_NIG rows have been updated), then every instance draws
    MOMENT_SAMPLES successive posterior samples on its frozen tables (episode_end_update: no step, no update).  For EVERY
    (s, a) row the sample mean and variance of the T elements and of R lie within six standard errors of the analytic
    Dirichlet / Student-t values.  Keys are fixed: the outcome is deterministic.  The same check with the same sizes is
    passed by the reference sampler in tests/test_psrl.py."""
    S, A = 6, 2
    models = [make_model("DeepSeaEpisodic", seed=s, size=3) for s in range(2)]
    assert all((m.n_states, m.n_actions) == (S, A) for m in models)
    env = make_env(models, "mt", False)
    agent = BatchedPSRLEpisodic(env, [0, 1], 100_000, reward_prior_model="N_NIG", rewards_prior_prms=MOMENT_REWARD_PRIOR,
                                sampler="philox")
    agent.run(20 * env.H)
    m = agent.model()
    first = int(m["episode"][0])
    assert first == 21
    Ts, Rs = [[], []], [[], []]
    for _ in range(MOMENT_SAMPLES):
        agent.episode_end_update()
        ls = agent.last_sample()
        for b in range(2):
            Ts[b].append(ls["T"][b].copy())
            Rs[b].append(ls["R"][b].copy())
    m2 = agent.model()
    assert (m2["episode"] == first + MOMENT_SAMPLES).all()
    for b in range(2):
        thp, rhp = m["transitions"][b], m["rewards"][b]
        assert np.array_equal(thp, m2["transitions"][b]) and np.array_equal(rhp, m2["rewards"][b])   # frozen
        assert (thp < 1).any() and (thp > 1).any() and (rhp[:, :, 1] > rhp[:, :, 1].min()).any()
        w = check_all_rows(np.array(Ts[b]), np.array(Rs[b]), thp, rhp)
        print(f"instance {b}: worst deviation {w:.2f} standard errors over {S * A} rows, episodes {first}..{first + MOMENT_SAMPLES - 1}")


def test_train_false_mask_and_phase(need_gpu):
    models = [make_model("DeepSeaEpisodic", seed=s, size=4) for s in range(4)]
    # out of phase before creation: two instances are two steps into their episode, the others were reset again
    env = make_env(models, "philox", False)
    env.step(np.zeros(4, np.int32))
    env.step(np.ones(4, np.int32))
    env.reset(mask=np.array([1, 0, 1, 0], bool))
    assert sorted(set(env.state()[1].tolist())) == [0, 2]
    env, agent, f = build(models, "philox", "reference", env=env)
    f.follow(40)
    # frozen: tables, Q and the sample stay, nothing is drawn; per-instance mask
    before, ls0 = agent.model(), agent.last_sample()
    f.call(2, train=False, stop=False)
    after, ls1 = agent.model(), agent.last_sample()
    for b in range(4):
        assert np.array_equal(before["transitions"][b], after["transitions"][b]) and np.array_equal(before["rewards"][b], after["rewards"][b])
        assert np.array_equal(ls0["Q"][b], ls1["Q"][b]) and np.array_equal(ls0["T"][b], ls1["T"][b])
    assert np.array_equal(before["episode"], after["episode"])
    f.call(2, train=np.array([True, False, True, False]), stop=True)
    f.follow(int(f.env.H) * 3)
    # a frozen agent walks across episode ends: the environment resets, the episode counter stays
    ep = agent.model()["episode"].copy()
    out = agent.run(3 * env.H, train=False)
    assert (out["steps_taken"] == 3 * env.H).all() and np.array_equal(agent.model()["episode"], ep)


def test_refusals(need_gpu):
    lib = L.load()
    cont = make_env([make_model("RiverSwimContinuous", seed=0, size=5)], "mt", False)
    with pytest.raises(L.CmdpError) as e:
        BatchedPSRLEpisodic(cont, [0], 100)
    assert e.value.code == L.ERR_UNSUPPORTED and "continuous" in str(e.value)
    m = make_model("DeepSeaEpisodic", seed=0, size=4, make_reward_stochastic=True)
    rc = BatchedMDP([m], rng_mode=L.RNG_MT_COMPAT, flags=L.FLAG_REWARD_CACHE)
    rc.reset()
    with pytest.raises(L.CmdpError) as e:
        BatchedPSRLEpisodic(rc, [0], 100)
    assert e.value.code == L.ERR_UNSUPPORTED and "REWARD_CACHE" in str(e.value)
    env = make_env([make_model("DeepSeaEpisodic", seed=0, size=4)], "mt", False)
    h = C.c_void_p()
    seeds, rp, tp = np.zeros(1, np.int32), np.ones(4, np.float32), np.ones(1, np.float32)
    for actor in (L.ACTOR_EPSILON_GREEDY, L.ACTOR_BOLTZMANN):
        assert lib.cmdp_psrl_create(C.byref(h), env._h, L.ptr(seeds), 100, L.ptr(rp), L.ptr(tp), 0, actor) == L.ERR_UNSUPPORTED
    bad = np.array([1, 1, 0, 1], np.float32)
    assert lib.cmdp_psrl_create(C.byref(h), env._h, L.ptr(seeds), 100, L.ptr(bad), L.ptr(tp), 0, 0) == L.ERR_INVALID
    for kw in (dict(epsilon_greedy=0.1), dict(boltzmann_temperature=2.0), dict(reward_prior_model="N_N", rewards_prior_prms=[0, 1])):
        with pytest.raises(NotImplementedError):
            BatchedPSRLEpisodic(env, [0], 100, **kw)
    agent = BatchedPSRLEpisodic(env, [0], 100)
    pol = agent.current_optimal_stochastic_policy()[0]
    assert pol.ndim == 3 and pol.shape[1:] == (10, 2)
    T_map, R_map = agent.map_estimate()[0]
    assert np.allclose(T_map.sum(-1), 1.0) and R_map.shape == (10, 2)
    with pytest.raises(L.CmdpError) as e:
        agent.run(1 << 25)
    assert e.value.code == L.ERR_OVERFLOW


def test_agent_destroyed_after_its_environment(need_gpu):
    """Garbage collection picks the order: cmdp_destroy orphans the handle's agents, which then refuse to run and free
    only their own memory (the path tests/test_gpu_ucrl2.py holds the UCRL2 agent to)."""
    env = make_env([make_model("DeepSeaEpisodic", seed=0, size=4)], "mt", False)
    agent = BatchedPSRLEpisodic(env, [0], 100)
    agent.run(50)
    env._agents = []   # as when the weak references are already dead
    env.close()
    with pytest.raises(L.CmdpError) as ei:
        agent.run(10)
    assert ei.value.code == L.ERR_INVALID
    agent.close()
