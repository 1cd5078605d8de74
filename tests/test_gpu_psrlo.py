"""The device PSRL agent for the continuous setting with OPTIMISTIC sampling (K18,
colosseum_amd.agents.BatchedPSRLContinuousOptimistic: k_psrlc_walk<GATE, true>, k_psrlo_sample, K13's solver on the extended arrays) against
the NumPy twin of tests/helpers_psrlo.py, which tests/test_psrlo.py holds against the reference (golden G23) on the CPU.

As in test_gpu_psrlc.py the twin is fed the DEVICE's transitions, artificial episode by artificial episode, and after every
call, for every instance:
  * every action is the twin actor's choice on the EXTENDED Q the device held (tie-break over all A * psi values), mapped to
    the real action j // psi, and the call ended at the step the reference's is_episode_end gives;
  * model() equals the twin's two hyper-parameter arrays, N [S, A, S], N.sum(-1) and nu_k bit for bit;
  * last_sample()'s T_ext, R, R_ext, z and simple mask equal the twin's own NumPy draws and float64 chain bit for bit;
  * the new Q is bit-equal to discounted_value_iteration_dense_batch on the same (T_ext, R_ext), with the same sweeps and
    scheme, and (first solves, every eighth) within bound_discounted of the float64 restatement.

A batch shares n_actions and the rewards range, so the ragged batch is RiverSwim of sizes 3, 5 and 8 (S = 8 takes the
16-byte stores, 3 and 5 the scalar ones, in one launch); FrozenLake of size 4 runs in a batch of its own.  The solve is a
chain from state to state over A * psi rows, about a microsecond a row and several hundred sweeps, so these two batches
lower psi (psi_weight, max_psi) to stay at seconds; RiverSwim-5 and RiverSwim-4 run at the issue's psi."""
import ctypes as C

import numpy as np
import pytest

from helpers_psrlc import GAMMA32, JACOBI, vi_rule
from helpers_psrlo import PSRLOTwin, philox_posterior_rows, philox_rewards, philox_z
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp
from colosseum_amd.agents import BatchedPSRLContinuousOptimistic, optimistic_sampling_scalars
from colosseum_amd.batched import BatchedMDP
from colosseum_amd.mdp import make_model
from test_gpu_psrlc import EPS, Follower, check_solve, make_env

pytestmark = pytest.mark.gpu

HORIZON = 600


class OFollower(Follower):
    """The optimistic twins of a batch; the checks of one call are Follower's."""

    def __init__(self, env, agent, seeds, q64_every=8, sampler="reference"):
        self.env, self.agent, self.seeds, self.sampler = env, agent, [int(s) for s in seeds], sampler
        self.q64_every = q64_every
        self.pending = [None] * env.B
        self.device = [None] * env.B   # Philox sampler: the device's (T_ext, R) of the sample the twin is drawing
        self.nonzero_p_minus = 0       # simple rows of S >= 5 whose P_minus is not all zero (more than z is non-zero at some k)
        self.twins = [PSRLOTwin(self.seeds[b], int(env.n_states[b]), env.A, env.rewards_range[1], int(agent.psi[b]),
                                float(agent.eta[b]), (lambda T, R, _b=b: self.pending[_b])) for b in range(env.B)]
        if sampler == "philox":
            for b, tw in enumerate(self.twins):
                tw.sample_sa = lambda tw, rows, _b=b: self.philox_rows(_b, tw, rows)
                tw.sample_R = lambda tw, _b=b: self.philox_R(_b, tw)
                tw.randint = lambda tw: tw.z_restated[len(tw.last_z)]
        self.cur = env.state()[0].copy()
        self.actions = [[] for _ in range(env.B)]
        self.episodes = agent.model()["episode"].copy()
        assert (self.episodes == 1).all()
        self.n_solves = np.zeros(env.B, np.int64)
        self.n_q64 = 0
        self.worst = 0.0
        self.kinds = set()
        self.after_rounds(list(range(env.B)))
        self.compare_models()

    def philox_rows(self, b, tw, rows):
        """Sample k of the posterior rows: the device's, once held against the restatement on the twin's tables within the
        tolerance helpers_psrl derives for k_psrl_sample's rows."""
        k = tw.k_posterior
        tw.k_posterior += 1
        T, tol = philox_posterior_rows(self.seeds[b], tw.episode, tw.transition_hp, tw.psi, rows, k)
        T_d = self.device[b][0].reshape(tw.S, tw.A, tw.psi, tw.S)[rows[0], rows[1], k]
        assert (np.abs(T_d.astype(np.float64) - T) <= tol).all(), (b, tw.episode, k, np.abs(T_d - T).max())
        assert (T_d >= 0).all() and (np.abs(T_d.astype(np.float64).sum(-1) - 1) < 1e-3).all()
        return T_d

    def philox_R(self, b, tw):
        R, tol = philox_rewards(self.seeds[b], tw.episode, tw.transition_hp, tw.reward_hp)
        R_d = self.device[b][1]
        assert (np.abs(R_d.astype(np.float64) - R) <= tol).all(), (b, tw.episode)
        return R_d

    def after_rounds(self, ended):
        if not ended:
            return
        ls = self.agent.last_sample()
        for b in ended:
            tw = self.twins[b]
            self.pending[b] = ls["Q"][b].copy()
            if self.sampler == "philox":   # z restated; posterior rows and rewards within tolerance; SIMPLE rows bit-equal given z
                tw.z_restated, tw.k_posterior = philox_z(self.seeds[b], tw.episode, tw.S, tw.psi), 0
                assert ls["z"][b].tolist() == tw.z_restated, (b, tw.episode)
                self.device[b] = (ls["T"][b], ls["R"][b])
                tw.episode_end_update()   # no agent stream, so no randn skip at the first sample
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
        for b, (Q, V, n, used) in zip(ended, outs):
            assert np.array_equal(Q, ls["Q"][b]), b
            assert n == ls["sweeps"][b] and used == ls["scheme"][b] and ls["status"][b] == 0, b
            T = ls["T"][b]
            assert used == vi_rule(T.shape[0], T.shape[1], int((T != 0).sum()), self.agent_threshold()), b
            if self.check_q64(b):
                self.worst = max(self.worst, check_solve(T, ls["R_ext"][b], Q, V, n, used, GAMMA32, EPS))
                self.n_q64 += 1
            self.n_solves[b] += 1

    def compare_models(self):
        m = self.agent.model()
        for b, tw in enumerate(self.twins):
            assert np.array_equal(m["transitions"][b], tw.transition_hp), b
            assert np.array_equal(m["rewards"][b], tw.reward_hp), b
            assert m["N"][b].dtype == np.int32 and np.array_equal(m["N"][b], tw.N), b
            assert np.array_equal(m["N_sa"][b], tw.N.sum(-1)) and np.array_equal(m["nu_k"][b], tw.nu_k()), b
            assert m["episode"][b] == tw.episode and m["psi"][b] == tw.psi and m["eta"][b] == tw.eta, b
        return m


def build(models, rng, seeds=None, beta=False, sampler="reference", **akw):
    env = make_env(models, rng, beta)
    seeds = np.arange(len(models)) + 11 if seeds is None else seeds
    agent = BatchedPSRLContinuousOptimistic(env, seeds, HORIZON, sampler=sampler, **akw)
    for b, m in enumerate(models):
        want = optimistic_sampling_scalars(m.n_states, m.n_actions, HORIZON, **{k: v for k, v in akw.items() if k != "sampler"})
        assert (agent.psi[b], agent.eta[b]) == (want[0], want[2])
    return env, agent, OFollower(env, agent, seeds, sampler=sampler)


def test_riverswim5_defaults_two_seeds(need_gpu):
    """psi = 26, eta = 50: 52 extended actions, ties between equal z at almost every step; simple rows for most of the run and
    the first posterior rows (a pair visited 50 times) towards its end."""
    models = [make_model("RiverSwimContinuous", seed=s, size=5) for s in (0, 1)]
    env, agent, f = build(models, "mt", seeds=[0, 1])
    assert agent.psi.tolist() == [26, 26] and agent.eta.tolist() == [50.0, 50.0]
    f.follow(600, chunk=64)
    assert "all_simple" in f.kinds   # which other kinds of call occur depends on the trajectory: printed
    # the float64 chain ran on non-zero data: P_minus > 0 needs about 21 visits of a pair whose successor is certain (1 >
    # sqrt(3 L / N) + 3 L / N with L = log 20), which 600 steps of either instance give many times over
    assert f.nonzero_p_minus > 0
    st = agent.stats()
    assert st["solves"] == f.n_solves.sum() and st["reference_ms"] > 0 and st["unconverged"] == 0 and st["sweeps"] > 0
    print(f"{int(f.n_solves.sum())} solves, {f.n_q64} against float64, worst |Q - Q64| / bound {f.worst:.3f}, calls {sorted(f.kinds)}, "
          f"{f.nonzero_p_minus} simple rows with non-zero P_minus")
    env.close()


def test_riverswim4_small_eta_all_three_kinds_of_call(need_gpu):
    models = [make_model("RiverSwimContinuous", seed=6, size=4)]
    env, agent, f = build(models, "mt", seeds=[6], eta_weight=1e-10, max_psi=5)
    assert agent.psi.tolist() == [5] and agent.eta.tolist() == [5.0]
    f.follow(600, chunk=64)
    # 8 pairs and 600 visits: a pair passes eta = 5 (pigeonhole); whether all do depends on the trajectory: printed
    assert "all_simple" in f.kinds and f.kinds & {"mixed", "all_posterior"}
    print(f"calls {sorted(f.kinds)}")
    env.close()


def test_deepsea4_at_the_lower_clamp_of_psi(need_gpu):
    models = [make_model("DeepSeaContinuous", seed=1, size=4, make_reward_stochastic=True, reward_variance_multiplier=0.7)]
    env, agent, f = build(models, "philox", seeds=[1], beta=True, psi_weight=0.05)
    assert agent.psi.tolist() == [2] and agent.eta.tolist() == [100.0]
    f.follow(120, chunk=32)
    assert f.kinds == {"all_simple"}
    env.close()


def test_ragged_batch_per_instance_psi_and_both_store_paths(need_gpu):
    models = [make_model("RiverSwimContinuous", seed=s, size=size) for s, size in enumerate((3, 5, 8))]
    env, agent, f = build(models, "mt", eta_weight=1e-10, psi_weight=0.25)
    assert agent.psi.tolist() == [3, 6, 11] and agent.eta.tolist() == [5.0] * 3 and [int(S) % 4 for S in env.n_states] == [3, 1, 0]
    done = f.follow(40, chunk=16)
    m1, l1, cur1 = agent.model(), agent.last_sample(), env.state()[0]
    # a run that does not stop (walk, round, walk, ... inside one call) on a fresh equal batch equals the followed run
    env2 = make_env(models, "mt", False)
    agent2 = BatchedPSRLContinuousOptimistic(env2, f.seeds, HORIZON, eta_weight=1e-10, psi_weight=0.25)
    at, acts = 0, []
    for d in sorted(set(done.tolist())):
        out = agent2.run(d - at, trace=True)
        assert (out["steps_taken"] == d - at).all()
        acts.append(out["actions"])
        at = d
        m2, l2, cur2 = agent2.model(), agent2.last_sample(), env2.state()[0]
        for b in np.flatnonzero(done == d):
            for k in ("transitions", "rewards", "N", "N_sa", "nu_k"):
                assert np.array_equal(m1[k][b], m2[k][b]), (k, b)
            for k in ("T", "R", "R_ext", "Q", "z", "simple"):
                assert np.array_equal(l1[k][b], l2[k][b]), (k, b)
            assert m1["episode"][b] == m2["episode"][b] and cur1[b] == cur2[b], b
    acts = np.concatenate(acts)
    for b in range(env.B):
        assert np.array_equal(acts[:done[b], b], np.array(f.actions[b])), b
    # an external episode_end_update(): 6 pairs and 40 visits in the first instance, so a pair has passed eta = 5 (pigeonhole)
    # and this call has posterior rows next to simple ones or nothing but posterior rows
    agent.episode_end_update()
    f.kinds.clear()
    f.after_rounds(list(range(env.B)))
    f.episodes = agent.model()["episode"].copy()
    f.compare_models()
    assert f.kinds & {"mixed", "all_posterior"}
    # the MAP policy is the plain agent's, on real actions
    pi = agent.policy()
    assert [p.shape for p in pi] == [(int(S), env.A) for S in env.n_states] and all((p.sum(-1) == 1).all() for p in pi)
    env.close()
    env2.close()


def test_frozenlake4_and_jacobi_on_the_extended_array(need_gpu):
    """Four real actions.  At a lowered size threshold the simple rows' few non-zeros make every extended sample sparse by the
    reference's rule: Jacobi.  First at the default psi = 60 (240 extended actions; two solves), then followed at psi = 8."""
    models = [make_model("FrozenLakeContinuous", seed=4, size=4, p_frozen=0.9)]
    env = make_env(models, "mt", False)
    agent = BatchedPSRLContinuousOptimistic(env, [4], HORIZON)
    agent._set_size_threshold(100)
    agent.episode_end_update()
    ls = agent.last_sample()
    assert ls["scheme"].tolist() == [JACOBI] and agent.psi.tolist() == [60] and ls["Q"][0].shape == (models[0].n_states, 240)
    env.close()
    env = make_env(models, "mt", False)
    agent = BatchedPSRLContinuousOptimistic(env, [4], HORIZON, max_psi=8)
    f = OFollower(env, agent, [4])
    f.size_threshold = 100
    agent._set_size_threshold(100)
    f.follow(16, chunk=8)
    assert (agent.last_sample()["scheme"] == JACOBI).all() and agent.psi.tolist() == [8]
    env.close()


def test_plain_entry_refuses_an_optimistic_handle_and_create_refusals(need_gpu):
    lib = L.load()
    models = [make_model("RiverSwimContinuous", seed=0, size=5)]
    env = make_env(models, "mt", False)
    agent = BatchedPSRLContinuousOptimistic(env, [0], HORIZON)
    T = np.zeros(5 * 2 * 5, np.float32)
    assert lib.cmdp_psrlc_last_sample(agent._h, L.ptr(T), None, None, None, None, None) == L.ERR_UNSUPPORTED
    assert b"optimistic" in lib.cmdp_last_error() and not T.any()
    seeds, rp, tp = np.zeros(1, np.int32), np.ones(4, np.float32), np.full(1, 0.2, np.float32)
    h = C.c_void_p()

    def create(e, psi=(26,), eta=(50.0,), l4=(3.0,), sampler=L.PSRL_SAMPLER_REFERENCE, B=1, null=None):
        a = dict(psi=np.array(psi * B, np.int32), eta=np.array(eta * B, np.float64), l4=np.array(l4 * B, np.float64))
        if null:
            a[null] = None
        s, r, t = np.zeros(B, np.int32), np.ones(4 * B, np.float32), np.full(B, 0.2, np.float32)
        return lib.cmdp_psrlc_create_optimistic(C.byref(h), e._h, L.ptr(s), 1000, L.ptr(r), L.ptr(t),
                                                None if a["psi"] is None else L.ptr(a["psi"]), None if a["eta"] is None else L.ptr(a["eta"]),
                                                None if a["l4"] is None else L.ptr(a["l4"]), sampler, L.ACTOR_GREEDY)

    for null in ("psi", "eta", "l4"):
        assert create(env, null=null) == L.ERR_INVALID and b"null" in lib.cmdp_last_error()
    assert create(env, psi=(0,)) == L.ERR_INVALID and b"psi" in lib.cmdp_last_error()
    assert create(env, eta=(0.0,)) == L.ERR_INVALID and b"eta" in lib.cmdp_last_error()
    assert create(env, l4=(float("nan"),)) == L.ERR_INVALID and b"log4s" in lib.cmdp_last_error()
    assert not h.value
    # a plain handle has no extended sample and no N
    from colosseum_amd.agents import BatchedPSRLContinuous
    env_p = make_env(models, "mt", False)
    plain = BatchedPSRLContinuous(env_p, [0], HORIZON, no_optimistic_sampling=True)
    assert lib.cmdp_psrlc_last_sample_optimistic(plain._h, *([None] * 9)) == L.ERR_UNSUPPORTED
    assert lib.cmdp_psrlc_counts(plain._h, L.ptr(np.zeros(64, np.int32))) == L.ERR_UNSUPPORTED
    env_p.close()
    env.close()
    # S * A * psi * S reaching 2^32, and a batch beyond the device's memory: refused by name before anything is allocated
    big = make_model("FrozenLakeContinuous", seed=0, size=20, p_frozen=0.9)
    S = big.n_states
    psi_over = -(-(1 << 32) // (S * 4 * S))
    env = BatchedMDP([big] * 24, rng_mode=L.RNG_MT_COMPAT)
    env.reset()
    assert create(env, psi=(psi_over,), B=24) == L.ERR_UNSUPPORTED and b"2^32" in lib.cmdp_last_error()
    tx, q, plain = (S * 4 * (psi_over - 1) * S + 3) & ~3, S * 4 * (psi_over - 1), (S * 4 * S + 3) & ~3
    need = 24 * (2 * tx + 3 * q + plain) * 4   # T_ext and its upload, bump / R_ext / Q, the plain-sized sample workspace
    assert need > 300 * 10 ** 9   # more than the device has
    assert create(env, psi=(psi_over - 1,), B=24) == L.ERR_OVERFLOW and str(need).encode() in lib.cmdp_last_error()
    assert not h.value
    env.close()


def test_philox_sampler_followed(need_gpu):
    """The device's own sampler against its restatement (helpers_psrlo): z equal; posterior rows and rewards within the derived
    tolerance; simple rows, R_ext and everything downstream bit-equal given them.  eta = 5, so all three kinds of call occur."""
    models = [make_model("RiverSwimContinuous", seed=s, size=size) for s, size in enumerate((4, 5, 8))]
    env, agent, f = build(models, "mt", sampler="philox", eta_weight=1e-10, max_psi=6)
    assert agent.psi.tolist() == [6, 6, 6] and agent.stats()["reference_ms"] == 0
    f.follow(60, chunk=16)
    agent.episode_end_update()   # 8 pairs and 60 visits in the first instance: a pair has passed eta = 5
    f.kinds.clear()
    f.after_rounds(list(range(env.B)))
    f.episodes = agent.model()["episode"].copy()
    f.compare_models()
    assert f.kinds & {"mixed", "all_posterior"}
    env.close()


def test_philox_sample_is_a_pure_function_of_seed_episode_and_tables(need_gpu):
    """Equal batches give equal bits; a batch split in two or reversed gives the same per-instance samples."""
    mk = lambda: [make_model("RiverSwimContinuous", seed=s, size=5) for s in range(4)]  # noqa: E731
    seeds = np.array([3, 4, 5, 6])

    def run(models, seeds):
        env = make_env(models, "mt", False)
        ag = BatchedPSRLContinuousOptimistic(env, seeds, HORIZON, sampler="philox", eta_weight=1e-10, max_psi=6)
        ag.run(50)
        ag.episode_end_update()   # 10 pairs and 50 visits: a pair has passed eta = 5, so this sample has posterior rows
        out = ag.last_sample(), ag.model()
        env.close()
        return out

    a, ma = run(mk(), seeds)
    b, mb = run(mk(), seeds)
    lo, _ = run(mk()[:2], seeds[:2])
    hi, mhi = run(mk()[2:], seeds[2:])
    rev, mrev = run(mk()[::-1], seeds[::-1])
    for k in ("T", "R", "R_ext", "Q", "z", "simple"):
        for i in range(4):
            assert np.array_equal(a[k][i], b[k][i]), (k, i)
            assert np.array_equal(a[k][i], (lo if i < 2 else hi)[k][i % 2]), (k, i)
            assert np.array_equal(a[k][i], rev[k][3 - i]), (k, i)
    assert (ma["episode"] > 2).all() and np.array_equal(ma["episode"], mb["episode"])
    assert np.array_equal(ma["N"][3], mhi["N"][1]) and np.array_equal(ma["N"][0], mrev["N"][3])
    assert not all(s.all() for s in a["simple"])   # posterior rows took part


def test_chain_on_nonzero_p_minus_with_sixteen_byte_rows(need_gpu):
    """RiverSwim of size 8 at its default eta = 80 and psi lowered to 6: every row stays simple for the whole run, and a pair
    visited some 24 times with a dominant successor has P_minus > 0 (1 > sqrt(3 L / N) + 3 L / N with L = log 32), so the
    pairwise float64 sum (S = 8: the eight-accumulator form), the += / -= chain and the per-k layout values run on non-zero
    data, written with 16-byte stores."""
    models = [make_model("RiverSwimContinuous", seed=2, size=8)]
    env, agent, f = build(models, "mt", seeds=[2], max_psi=6)
    assert agent.psi.tolist() == [6] and agent.eta.tolist() == [80.0]
    f.follow(400, chunk=64)
    print(f"{f.nonzero_p_minus} simple rows with non-zero P_minus in {int(f.n_solves[0])} samples, calls {sorted(f.kinds)}")
    assert f.nonzero_p_minus > 0
    env.close()


# (size, seed, steps): seed and step count chosen with PSRLOTwin on the CPU over seeds 0..19 at max_psi = 3 -- `steps` is the step
# of the first episode_end_update whose sample has a non-zero P_minus (its tenth sample in both runs: pair (0, a) visited 64
# times by then), so the followed run ends with that sample.  The device's run reaches it at the same step.
SPLIT_PLAN_RUNS = [(144, 17, 66), (264, 13, 66)]


@pytest.mark.parametrize("size,seed,steps", SPLIT_PLAN_RUNS, ids=[f"S{c[0]}" for c in SPLIT_PLAN_RUNS])
def test_chain_on_nonzero_p_minus_where_the_pairwise_sum_splits(need_gpu, size, seed, steps):
    """The float64 pairwise sum of the chain beyond one run of its plan (mapvi_plan first splits at S = 129): S = 144 is two runs
    (72 + 72) and one merge; S = 264 splits into 128 + 136 and the right half into 64 + 72, three runs with two partial sums
    waiting on the stack.  eta stays at its default 10 S, so every row is simple for the whole run; max_psi = 3 keeps a sample
    at six extended actions.  A row of zeros sums right by accident, so what makes the test mean something is P_minus > 0 in a
    summed row: P_hat > sqrt(3 L P_hat / N) + 3 L / N with L = log 4S, which for a successor that is certain (P_hat = 1) is
    1 > sqrt(3 L / N) + 3 L / N: N >= 50 visits of the pair at S = 144 (L = 6.356) and N >= 55 at S = 264 (L = 6.962), a few more
    for a successor that merely dominates (52 and 57 at P_hat = 0.97).  The seeds are those for which the twin's
    RiverSwim agent gets a pair there soonest, and `steps` ends the run at the episode_end_update that first samples it.  The
    float64 restatement of the solve is a Python loop over the states per sweep and not what this test is about: it is held
    for the first three solves only."""
    models = [make_model("RiverSwimContinuous", seed=seed, size=size)]
    env = make_env(models, "mt", False)
    agent = BatchedPSRLContinuousOptimistic(env, [seed], HORIZON, max_psi=3)
    assert env.n_states.tolist() == [size] and agent.psi.tolist() == [3] and agent.eta.tolist() == [10.0 * size]
    f = OFollower(env, agent, [seed], q64_every=10 ** 6)
    f.follow(steps, chunk=64)
    print(f"S = {size}: {f.nonzero_p_minus} simple rows with non-zero P_minus in {int(f.n_solves[0])} samples, calls {sorted(f.kinds)}")
    assert f.kinds == {"all_simple"}
    assert f.nonzero_p_minus > 0
    env.close()
