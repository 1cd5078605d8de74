"""Test helper: a NumPy restatement of the reference's PSRLContinuous on its DEFAULT path, optimistic sampling
(colosseum/agent/agents/infinite_horizon/posterior_sampling.py, no_optimistic_sampling=False), on top of helpers_psrlc's twin
of the plain path.  tests/test_psrlo.py holds it against the reference's own run (golden G23) bit for bit, which is what
entitles tests/test_gpu_psrlo.py to use it as the reference of the device agent on the GPU box, where the reference is absent.

The expressions are kept as the reference writes them, the inexact `+=` / `-=` pair on P_minus included."""
import numpy as np

from helpers_psrl import KEY_HI, U, philox4x32_10, philox_gamma_np, philox_sample
from helpers_psrlc import PSRLCTwin


def numpy_sample_sa(twin, rows):
    """M_DIR.sample_sa (conjugate_transitions.py:48-54, :62-63) on the twin's transitions stream; `rows` = (s indices, a indices)."""
    hyper_params = twin.transition_hp[rows]
    r = twin.rng_t.standard_gamma(hyper_params, (1, *hyper_params.shape)).astype(np.float32).squeeze()
    return r / (1e-5 + r.sum(-1, keepdims=True))


def numpy_sample_R(twin):
    """N_NIG.sample (conjugate_rewards.py:84-99) on the twin's rewards stream."""
    S, A = twin.S, twin.A
    (mu, lambda0, alpha, beta) = twin.reward_hp.reshape(S * A, -1).T
    tau = twin.rng_r.gamma(shape=alpha, scale=1.0 / beta).astype(np.float32)
    var = 1.0 / (lambda0 * tau)
    mean = twin.rng_r.normal(loc=mu, scale=np.sqrt(var), size=(1, *mu.shape)).astype(np.float32)
    return mean.reshape(S, A).squeeze()


class PSRLOTwin(PSRLCTwin):
    """`solver(T_ext [S, A * psi, S], R_ext [S, A * psi])` -> Q [S, A * psi] float32.  `sample_sa(twin, rows)`, `sample_R(twin)` and
    `randint(twin)` are the three draws of an episode_end_update, injectable."""

    def __init__(self, seed, n_states, n_actions, r_max, psi, eta, solver, sample_sa=numpy_sample_sa, sample_R=numpy_sample_R,
                 randint=None, rewards_prior_prms=None, transitions_prior_prms=None):
        super().__init__(seed, n_states, n_actions, r_max, solver, None, rewards_prior_prms, transitions_prior_prms)
        self.psi, self.eta = int(psi), eta
        self.sample_sa, self.sample_R = sample_sa, sample_R
        self.randint = randint or (lambda tw: tw.rng_a.randint(tw.S))
        self.rng_a = np.random.RandomState(seed)   # BaseAgent._rng: the agent's own stream
        self.Qs = np.zeros((self.psi, self.S, self.A, self.S), np.float32)   # the reference's self.Q
        self.last_z, self.last_simple, self.last_R_ext, self.last_n = [], None, None, (0, 0)

    def optimistic_sampling(self):
        """:411-443."""
        Nsum = self.N.sum(-1)
        cond = Nsum < self.eta
        indices_2 = list(np.where(cond))
        indices_1 = list(np.where(~cond))
        do_simple_sampling = len(indices_2[0]) > 0
        do_posterior_sampling = len(indices_1[0]) > 0
        if do_simple_sampling:
            P_hat = self.N / np.maximum(Nsum[..., None], 1)
            N = np.maximum(self.N, 1)
            P_minus = P_hat - np.minimum(np.sqrt(3 * P_hat * np.log(4 * self.S) / N) + 3 * np.log(4 * self.S) / N, P_hat)
            assert P_minus.dtype == np.float64
        self.last_z = []
        for psi in range(self.psi):
            if do_posterior_sampling:
                self.Qs[tuple([np.array([psi] * len(indices_1[0]))] + indices_1)] = self.sample_sa(self, tuple(indices_1))
            if do_simple_sampling:
                z = self.randint(self)
                self.last_z.append(int(z))
                summing = 1 - P_minus.sum(-1)
                P_minus[:, :, z] += summing
                self.Qs[tuple([np.array([psi] * len(indices_2[0]))] + indices_2)] = P_minus[tuple(indices_2)]
                P_minus[:, :, z] -= summing
        self.last_simple = cond
        self.last_n = (len(indices_1[0]), len(indices_2[0]))

    def episode_end_update(self):
        """:360-377."""
        self.optimistic_sampling()
        T = np.moveaxis(self.Qs, 0, 2)
        T = T.reshape((self.S, -1, self.S))
        R = self.sample_R(self)
        self.last_R = R
        R = np.tile(R, (1, self.psi))
        self.last_T, self.last_R_ext = T, R
        self.Q = self.solver(T, R)
        self.episode_transition_data = dict()
        self.episode += 1

    def before_start_interacting(self):
        """:379-383; the Q of the randn is replaced at once, the stream's position stays."""
        self.rng_a.randn(self.S, self.A * self.psi)
        self.episode_end_update()

    def select_action(self, s):
        """The extended action of the greedy actor, then extended_action_to_real (:445-452)."""
        self.last_extended = super().select_action(s)
        return int(self.last_extended / self.psi)


# ---- the device's Philox sampler (k_psrlo_sample with CMDP_PSRL_SAMPLER_PHILOX), restated ------------------------------------
def philox_z(seed, episode, S, psi):
    """z_k = (w0 * S) >> 32 of the block (n = episode << 32 | k, domain 9, draw 0)."""
    k = np.arange(psi, dtype=np.uint32)
    w = philox4x32_10(k, np.full(psi, episode, np.uint32), np.full(psi, 9, np.uint32), np.zeros(psi, np.uint32),
                      np.full(psi, np.uint32(np.int64(seed) & 0xFFFFFFFF)), np.full(psi, KEY_HI, np.uint32))
    return ((w[0].astype(np.uint64) * np.uint64(S)) >> np.uint64(32)).astype(np.int64).tolist()


def philox_posterior_rows(seed, episode, transition_hp, psi, rows, k):
    """Sample k of the posterior rows `rows` = (s indices, a indices): element c of extended row j = (s * A + a) * psi + k is the
    gamma variate on domain 8 with n = episode << 32 | (j * S + c); then the row as k_psrl_sample's.  Returns (rows [n1, S]
    float32, tolerance) with helpers_psrl.philox_sample's derivation of the tolerance: the arithmetic is the same."""
    S, A, _ = transition_hp.shape
    key = (np.uint32(np.int64(seed) & 0xFFFFFFFF), np.uint32(KEY_HI))
    ep = np.uint64(int(episode)) << np.uint64(32)
    j = (np.asarray(rows[0], np.uint64) * np.uint64(A) + np.asarray(rows[1], np.uint64)) * np.uint64(psi) + np.uint64(k)
    pos = (j[:, None] * np.uint64(S) + np.arange(S, dtype=np.uint64)[None, :]).ravel()
    g, _ = philox_gamma_np(transition_hp[rows].astype(np.float64).ravel(), ep | pos, key, 8)
    r = g.astype(np.float32).reshape(len(j), S)
    den = np.float32(1e-5) + r.astype(np.float64).sum(-1, keepdims=True).astype(np.float32)
    T = r / den
    assert T.dtype == np.float32
    return T, (8 * U + 3e-12) * T.astype(np.float64) + 1e-37


def philox_rewards(seed, episode, transition_hp, reward_hp):
    """The reward sample is k_psrl_sample's (domain 7): (R [S, A], tolerance)."""
    _, R, _, tol_R, _ = philox_sample(seed, episode, transition_hp, reward_hp)
    return R, tol_R
