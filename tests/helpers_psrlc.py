"""Test helper: a NumPy restatement of the reference's PSRLContinuous on its plain-sampling path
(colosseum/agent/agents/infinite_horizon/posterior_sampling.py, no_optimistic_sampling=True) with its BayesianMDPModel
(N_NIG rewards, M_DIR transitions) and greedy QValuesActor, whose SAMPLER and SOLVER are injected.  tests/test_psrlc.py holds
it against the reference's own run (golden G22) bit for bit, which is what entitles tests/test_gpu_psrlc.py to use it as the
reference of the device agent on the GPU box, where the reference is absent.

Also here: the stamped form of the artificial-episode rule the device keeps, the float64 restatement of the solve, a float32
restatement of the kernel's arithmetic and the derived rounding bound."""
import numpy as np

from helpers_psrl import U, PSRLTwin, numpy_sampler

JACOBI, GAUSS_SEIDEL = 1, 2   # CMDP_SCHEME_JACOBI / CMDP_SCHEME_GAUSS_SEIDEL
GAMMA32 = float(np.float32(0.99))   # `gamma = np.float32(gamma)` (infinite_horizon.py:127, 149)


def vi_rule(S, A, nnz, size_threshold=300 * 3 * 300, density_threshold=0.2):
    """infinite_horizon.py:28-36 on the count of non-zero elements of a dense T [S, A, S]."""
    size = S * A * S
    return JACOBI if size > size_threshold and nnz / size < density_threshold else GAUSS_SEIDEL


class PSRLCTwin(PSRLTwin):
    """`sampler(twin)` -> (T [S, A, S], R [S, A]) float32; `solver(T, R)` -> Q [S, A] float32."""

    def __init__(self, seed, n_states, n_actions, r_max, solver, sampler=numpy_sampler, rewards_prior_prms=None,
                 transitions_prior_prms=None):
        super().__init__(seed, n_states, n_actions, 0, r_max, solver, sampler, rewards_prior_prms, transitions_prior_prms)
        self.N = np.zeros((self.S, self.A, self.S), np.int32)
        self.episode_transition_data = dict()

    def select_action(self, s):
        q = self.Q[s]
        return int(self._rng.choice(np.where(q == q.max())[0]))

    def step_update(self, s, a, r, s2):
        """PSRLContinuous.step_update (:390-409): the model's update (never a last step), N, episode_transition_data."""
        super().step_update(s, a, r, s2, False)
        self.N[s, a, s2] += 1
        self.episode_transition_data.setdefault((s, a), []).append(s2)

    def is_episode_end(self, s, a):
        """:346-358 with min_steps_before_new_episode = 0."""
        nu_k = len(self.episode_transition_data[s, a])
        N_tau = self.N[s, a].sum()
        return bool(N_tau >= 2 * (N_tau - nu_k))

    def episode_end_update(self):
        self.last_T, self.last_R = self.sampler(self)
        self.Q = self.solver(self.last_T, self.last_R)
        self.episode_transition_data = dict()
        self.episode += 1

    before_start_interacting = episode_end_update

    def nu_k(self):
        out = np.zeros((self.S, self.A), np.int32)
        for (s, a), v in self.episode_transition_data.items():
            out[s, a] = len(v)
        return out


class StampedRule:
    """The device's form of the rule (csrc/cmdp_psrlc.h): n_sa never cleared; nu with the episode it was written in, 0 when
    that is not the current episode."""

    def __init__(self, S, A):
        self.n_sa, self.nu, self.stamp = (np.zeros((S, A), np.int32) for _ in range(3))
        self.episode = 1   # the agent exists: the solve on the prior has been counted

    def visit(self, s, a):
        n = self.n_sa[s, a] + 1
        nu = (self.nu[s, a] if self.stamp[s, a] == self.episode else 0) + 1
        self.n_sa[s, a], self.nu[s, a], self.stamp[s, a] = n, nu, self.episode
        return bool(n >= 2 * (n - nu))

    def episode_end_update(self):
        self.episode += 1


# ---- the solve ---------------------------------------------------------------------------------------------------------
def vi_discounted_f64(T, R, gamma, scheme, n):
    """Exactly `n` sweeps of `scheme` from V = 0 in float64, no stopping rule.  Returns (Q64 [S, A], d_n, d_{n-1}, qmax):
    d_k = max_s |V_k[s] - V_{k-1}[s]| (d_0 = inf), qmax the largest |Q| any sweep produced."""
    T, R = np.asarray(T, np.float64), np.asarray(R, np.float64)
    S, A, _ = T.shape
    V, Q = np.zeros(S), np.zeros((S, A))
    d, d_prev, qmax = np.inf, np.inf, 0.0
    gT = gamma * T
    for _ in range(n):
        V_old = V.copy()
        if scheme == JACOBI:
            Q = R + gamma * (T @ V_old)
            V = Q.max(-1)
        else:
            for s in range(S):
                Q[s] = R[s] + gT[s] @ V
                V[s] = Q[s].max()
        d_prev, d = d, float(np.abs(V_old - V).max())
        qmax = max(qmax, float(np.abs(Q).max()))
    return Q.copy(), d, d_prev, qmax


def bound_discounted(n, gamma, qmax, S):
    """Largest |Q - Q64| the kernel's float32 solve (csrc/cmdp_psrlc.h) may show after `n` sweeps against vi_discounted_f64
    on the same float32 (T, R) with the same float32 gamma, derived the way helpers_psrl.bound_episodic is.

    One row update.  The products of two float32 values are exact in float64 and the float64 sum of S <= 4096 terms is off
    by at most S 2^-53 of sum_j |term_j| <= qmax.  What is rounded to float32, with M = max(1, qmax) and a sampled row
    non-negative and summing to less than one (so |T[s, a] . V| <= max |V| <= qmax):
      Gauss-Seidel  fl32(gamma T_j): sum_j U gamma T_j |V_j| <= U gamma M;  Q = float(R + acc): U M            <= 2 U M
      Jacobi        tv = float(T . V_old): U M;  gamma * tv: U gamma M;  R + .: U M                              <= 3 U M
    and one more U M is allowed for the float32 subtraction of the stopping rule, so that d (device) and d (float64) differ by
    at most twice this bound: e = (4 U + S 2^-52) M per sweep and row.

    Sweeps.  With equal V on both sides a row's values differ by at most e; with V differing by at most E the exact row map
    moves by at most gamma E (its coefficients gamma T_j sum to less than gamma).  In a Gauss-Seidel sweep the states before
    s already carry the new error E_k and the others the old E_{k-1} <= max(E_{k-1}, E_k), so by induction over s,
    E_k <= gamma max(E_{k-1}, E_k) + e, hence E_k <= gamma E_{k-1} + e wherever E_{k-1} >= E_k and E_k <= e / (1 - gamma)
    otherwise; Jacobi gives E_k <= gamma E_{k-1} + e directly.  From E_0 = 0: E_n <= e (1 - gamma^n) / (1 - gamma), and
    never more than e / (1 - gamma).  The factor 1 + 2^-20 covers qmax being taken from the restatement instead of the
    computed values."""
    e = (4 * U + S * 2.0 ** -52) * max(1.0, qmax)
    return e * (1.0 - gamma ** n) / (1.0 - gamma) * (1 + 2.0 ** -20)


def vi_discounted_kernel_f32(T, R, gamma32, scheme, epsilon, max_sweeps):
    """The kernel's arithmetic restated in NumPy (the float64 row sums in NumPy's order, not the wavefront's: the two differ
    by the float64 accumulation the bound carries).  Returns (Q, V, sweeps, converged)."""
    T, R = np.asarray(T, np.float32), np.asarray(R, np.float32)
    S, A, _ = T.shape
    g = np.float32(gamma32)
    V, Q = np.zeros(S, np.float32), np.zeros((S, A), np.float32)
    T64 = T.astype(np.float64)
    gT64 = (g * T).astype(np.float64)   # fl32(gamma * T[s, a, j]), then exact in float64
    assert (g * T).dtype == np.float32
    for sweep in range(1, int(max_sweeps) + 1):
        V_old = V.copy()
        if scheme == JACOBI:
            tv = (T64 @ V_old.astype(np.float64)).astype(np.float32)
            Q = R + g * tv
            assert Q.dtype == np.float32
            V = Q.max(-1)
        else:
            for s in range(S):
                Q[s] = (R[s].astype(np.float64) + gT64[s] @ V.astype(np.float64)).astype(np.float32)
                V[s] = Q[s].max()
        diff = np.abs(V_old - V).max()
        assert diff.dtype == np.float32
        if float(diff) < epsilon:
            return Q, V, sweep, True
    return Q, V, int(max_sweeps), False
