"""Test helper: a NumPy restatement of the reference's PSRLEpisodic (colosseum/agent/agents/episodic/posterior_sampling.py)
with its BayesianMDPModel (N_NIG rewards, M_DIR transitions) and greedy QValuesActor, whose SAMPLER and SOLVER are
injected.  tests/test_psrl.py holds it against the reference's own run (golden G20) bit for bit, which is what entitles
tests/test_gpu_psrl.py to use it as the reference of the device agent on the GPU box, where the reference is absent.

The expressions are kept as the reference writes them: which operation runs in float32 and which in float64 is decided by
NumPy's promotion (NEP 50) from the operand types.  Rewards are PYTHON floats there; callers pass `float(r)`.

Also here: the NumPy restatement of the device's Philox sampler (k_psrl_sample), the float64 restatement of the solve, the
derived error bounds, and the moment check shared by the CPU and GPU distribution tests."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.numpy_port import philox4x32_10  # noqa: E402

U = 2.0 ** -24  # float32 unit roundoff
KEY_HI = 0x5053524C


def numpy_sampler(twin):
    """M_DIR.sample (conjugate_transitions.py:48-60) and N_NIG.sample (conjugate_rewards.py:84-99) on the twin's own two
    RandomState(seed) streams, as the reference writes them."""
    S, A = twin.S, twin.A
    hyper_params = twin.transition_hp.reshape(S * A, -1)
    r = twin.rng_t.standard_gamma(hyper_params, (1, *hyper_params.shape)).astype(np.float32).squeeze()
    r = r / (1e-5 + r.sum(-1, keepdims=True))
    T = r.reshape((S, A, -1))
    (mu, lambda0, alpha, beta) = twin.reward_hp.reshape(S * A, -1).T
    tau = twin.rng_r.gamma(shape=alpha, scale=1.0 / beta).astype(np.float32)
    var = 1.0 / (lambda0 * tau)
    mean = twin.rng_r.normal(loc=mu, scale=np.sqrt(var), size=(1, *mu.shape)).astype(np.float32)
    return T, mean.reshape(S, A).squeeze()


class PSRLTwin:
    """`sampler(twin)` -> (T [S, A, S], R [S, A]) float32; `solver(H, T, R)` -> Q [H + 1, S, A] float32."""

    def __init__(self, seed, n_states, n_actions, H, r_max, solver, sampler=numpy_sampler, rewards_prior_prms=None,
                 transitions_prior_prms=None):
        S, A = self.S, self.A = int(n_states), int(n_actions)
        self.H = int(H)
        self.solver, self.sampler = solver, sampler
        if rewards_prior_prms is None:
            rewards_prior_prms = [r_max, 1, 1, 1]           # bayesian_model.py:48-53
        if transitions_prior_prms is None:
            transitions_prior_prms = [1.0 / S]
        # base_conjugate.py:49 and N_NIG.__init__ (conjugate_rewards.py:54-63)
        self.reward_hp = np.tile(rewards_prior_prms, (S, A, 1)).astype(np.float32)
        for i in range(S):
            for j in range(A):
                mu, n_mu, tau, n_tau = self.reward_hp[i, j]
                self.reward_hp[i, j] = (mu, n_mu, n_tau * 0.5, (0.5 * n_tau) / tau)
        # M_DIR.__init__ (conjugate_transitions.py:39-42)
        self.transition_hp = np.tile(np.tile(transitions_prior_prms, (S, A, 1)).astype(np.float32), (1, 1, S))
        assert self.transition_hp.shape == (S, A, S)
        self.rng_t = np.random.RandomState(seed)   # M_DIR._rng
        self.rng_r = np.random.RandomState(seed)   # N_NIG._rng
        self._rng = np.random.RandomState(seed)    # the actor's stream (agent/actors/base.py:33)
        self.Q = None
        self.episode = 0
        self.last_T = self.last_R = None

    def select_action(self, h, s):
        q = self.Q[h, s]
        return int(self._rng.choice(np.where(q == q.max())[0]))

    def step_update(self, s, a, r, s2, last):
        """BayesianMDPModel.step_update (bayesian_model.py:80-93) with N_NIG.update_sa for rs = [r] and M_DIR.update_sa."""
        rs = [r]
        (mu0, lambda0, alpha0, beta0) = self.reward_hp[s, a]
        n = len(rs)
        y_bar = np.mean(rs)
        lambda1 = lambda0 + n
        mu1 = (lambda0 * mu0 + n * y_bar) / lambda1
        alpha1 = alpha0 + (n * 0.5)
        ssq = n * np.var(rs)
        prior_disc = lambda0 * n * ((y_bar - mu0) ** 2) / lambda1
        beta1 = beta0 + 0.5 * (ssq + prior_disc)
        self.reward_hp[s, a] = (mu1, lambda1, alpha1, beta1)
        if not last:
            x = np.zeros(self.S)
            x[s2] = 1
            self.transition_hp[s, a] += np.array([x]).sum(0)

    def episode_end_update(self):
        self.last_T, self.last_R = self.sampler(self)
        self.Q = self.solver(self.H, self.last_T, self.last_R)
        self.episode += 1

    before_start_interacting = episode_end_update


# ---- the device's Philox sampler, restated -----------------------------------------------------------------------------
def _u53(w0, w1):
    return ((w0 >> np.uint32(5)).astype(np.float64) * 67108864.0 + (w1 >> np.uint32(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)


def philox_gamma_np(shape, n, key, domain, draw=None):
    """csrc/cmdp_device.h philox_gamma for arrays: element i uses counter (n[i] lo, n[i] hi, domain, draw) and `key`.
    Returns (variates float64, draw counters after the call)."""
    shape = np.array(shape, np.float64).ravel()
    n = np.asarray(n, np.uint64).ravel()
    lo, hi = (n & np.uint64(0xFFFFFFFF)).astype(np.uint32), (n >> np.uint64(32)).astype(np.uint32)
    draw = np.zeros(len(shape), np.uint32) if draw is None else draw.copy()
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    blk = lambda ix: philox4x32_10(lo[ix], hi[ix], np.full(len(ix), domain, np.uint32), draw[ix],  # noqa: E731
                                   np.full(len(ix), k0, np.uint32), np.full(len(ix), k1, np.uint32))
    boost = np.ones(len(shape))
    lt = np.flatnonzero(shape < 1.0)
    if len(lt):
        w = blk(lt)
        draw[lt] += np.uint32(1)
        boost[lt] = (1.0 - _u53(w[0], w[1])) ** (1.0 / shape[lt])
        shape[lt] += 1.0
    d = shape - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out = boost * d
    pending = np.ones(len(shape), bool)
    for _ in range(64):
        ix = np.flatnonzero(pending)
        if not len(ix):
            break
        w = blk(ix)
        draw[ix] += np.uint32(1)
        z = np.sqrt(-2.0 * np.log(1.0 - _u53(w[0], w[1]))) * np.cos(6.283185307179586476925286766559 * _u53(w[2], w[3]))
        v = 1.0 + c[ix] * z
        ok = v > 0.0
        ix, z, v = ix[ok], z[ok], v[ok]
        if not len(ix):
            continue
        v = v * v * v
        w = blk(ix)
        draw[ix] += np.uint32(1)
        u3 = _u53(w[0], w[1])
        with np.errstate(divide="ignore"):
            acc = np.log(u3) < 0.5 * z * z + d[ix] - d[ix] * v + d[ix] * np.log(v)
        out[ix[acc]] = boost[ix[acc]] * d[ix[acc]] * v[acc]
        pending[ix[acc]] = False
    return out, draw


def philox_sample(seed, episode, transition_hp, reward_hp):
    """k_psrl_sample restated: (T, R, tolerance of T elementwise, tolerance of R elementwise, row_target [S, A]).

    row_target = sum / (1e-5 + sum) in float64, sum the float64 sum of the row's float32 variates: what a row of T adds up
    to.  The device's row differs from it by its S quotient roundings (U T_c each, U in all since the row sums to less
    than one), the rounding of the sum and of the denominator (2 U), float32's 1e-5 (U) and the variates' ulp (which moves
    numerator and denominator together: below U): the tests allow (S + 4) U.

    Tolerances.  The project's figure for philox_gamma on the device against libm is rtol 1e-12 in float64
    (csrc/cmdp_device.h, the Beta sampler's comment).  Two float64 values that close round to the same float32 or to
    neighbours, so a float32 variate is off by at most one ulp = 2 U relative (+ 1e-12); so is the float64 sum of the
    variates, its rounding to float32 adds one more ulp (2 U), and the quotient of the two, rounded once, one more:
    |dT| <= (2 U + 4 U + 2 U + 3e-12) T = (8 U + 3e-12) T, plus 1e-37 absolute for variates in float32's subnormal range
    (spacing 2^-149, divided by a denominator >= 1e-5).  R = float(mu + sd * z): tau one ulp, var = 1 / (lambda tau) two
    more roundings, the root halves the relative error and adds an ulp: sd within 5 U; z within 1e-12; the final rounding
    one ulp of |R|: |dR| <= (5 U + 1e-12) |sd z| + 2 U |R|."""
    S, A, _ = transition_hp.shape
    key = (np.uint32(np.int64(seed) & 0xFFFFFFFF), np.uint32(KEY_HI))
    ep = np.uint64(int(episode)) << np.uint64(32)
    pos = np.arange(S * A * S, dtype=np.uint64)
    g, _ = philox_gamma_np(transition_hp.astype(np.float64).ravel(), ep | pos, key, 6)
    r = g.astype(np.float32).reshape(S * A, S)
    den = np.float32(1e-5) + r.astype(np.float64).sum(-1, keepdims=True).astype(np.float32)
    T = (r / den).reshape(S, A, S)
    s64 = r.astype(np.float64).sum(-1)
    row_target = (s64 / (1e-5 + s64)).reshape(S, A)
    hp = reward_hp.reshape(S * A, 4)
    n = ep | np.arange(S * A, dtype=np.uint64)
    ga, draw = philox_gamma_np(hp[:, 2].astype(np.float64), n, key, 7)
    tau = ((np.float32(1.0) / hp[:, 3]).astype(np.float64) * ga).astype(np.float32)
    sd = np.sqrt(np.float32(1.0) / (hp[:, 1] * tau))
    assert sd.dtype == np.float32
    lo, hi = (n & np.uint64(0xFFFFFFFF)).astype(np.uint32), (n >> np.uint64(32)).astype(np.uint32)
    w = philox4x32_10(lo, hi, np.full(S * A, 7, np.uint32), draw, np.full(S * A, key[0], np.uint32), np.full(S * A, key[1], np.uint32))
    z = np.sqrt(-2.0 * np.log(1.0 - _u53(w[0], w[1]))) * np.cos(6.283185307179586476925286766559 * _u53(w[2], w[3]))
    R64 = hp[:, 0].astype(np.float64) + sd.astype(np.float64) * z
    R = R64.astype(np.float32).reshape(S, A)
    tol_T = (8 * U + 3e-12) * T.astype(np.float64) + 1e-37
    tol_R = ((5 * U + 1e-12) * np.abs(sd.astype(np.float64) * z) + 2 * U * np.abs(R64)).reshape(S, A)
    return T, R, tol_T, tol_R, row_target


# ---- the solve ---------------------------------------------------------------------------------------------------------
def vi_episodic_f64(H, T, R):
    """episodic_value_iteration (finite_horizon.py:11-26) in float64.  Returns (Q [H + 1, S, A], V, qmax = max |Q|)."""
    T, R = np.asarray(T, np.float64), np.asarray(R, np.float64)
    S, A, _ = T.shape
    Q, V = np.zeros((H + 1, S, A)), np.zeros((H + 1, S))
    for h in range(H - 1, -1, -1):
        Q[h] = R + T @ V[h + 1]
        V[h] = Q[h].max(-1)
    return Q, V, float(np.abs(Q).max())


def bound_episodic(H, qmax, n_terms):
    """Largest |Q - Q64| a float32 solve may show against vi_episodic_f64 on the same float32 (T, R), derived the way
    helpers_evi.bound is.  Per layer, a row's float32 evaluation of R + sum_j T_j V_j differs from the exact one by
      the kernel (n_terms = 1): the products of two float32 values are exact in float64 and the float64 sum of S <= 4096
        terms is off by at most S 2^-53 of it, so what counts is the ONE rounding of Q to float32:        U qmax
      a BLAS sgemv of S terms (n_terms = S, the reference): every product rounded (sum_j U T_j |V_j| <= U qmax, the row
        sums to less than one), n_terms partial sums of magnitude <= qmax rounded, and R + dot rounded: (n_terms + 2) U qmax
    with qmax the largest |Q| of the float64 restatement (V = max_a Q is no larger).  A sampled row is non-negative and
    sums to sum / (1e-5 + sum) < 1, so the layer map is a non-expansion in the sup norm: the errors of at most H layers
    add.  When the two sides of a comparison are the kernel and the reference, the kernel's own U qmax per layer is on
    top: n_terms + 3 in all.  The factor 1 + 2^-20 covers the float64 accumulation and qmax being taken from the
    restatement instead of the computed values."""
    per_layer = 1 if n_terms == 1 else n_terms + 3
    return H * per_layer * U * max(1.0, qmax) * (1 + 2.0 ** -20)


# ---- moments -----------------------------------------------------------------------------------------------------------
def moment_tables(S, A, n_transitions=60, seed=0):
    """Tables for the distribution tests that need no device: a twin with the distribution tests' priors, updated by
    `n_transitions` fixed pseudo-random transitions (so Dirichlet parameters lie below and above one and the visited N_NIG
    rows have been updated).  Returns (transition_hp, reward_hp)."""
    tw = PSRLTwin(0, S, A, 3, 1.0, None, rewards_prior_prms=MOMENT_REWARD_PRIOR)
    rng = np.random.RandomState(seed)
    for _ in range(n_transitions):
        s, a, s2 = int(rng.randint(S)), int(rng.randint(A)), int(rng.randint(S))
        tw.step_update(s, a, float(rng.uniform()), s2, bool(rng.randint(4) == 0))
    return tw.transition_hp, tw.reward_hp


# the distribution tests' reward prior (mu, n_mu, tau, n_tau): alpha = 10, so that R's marginal is a Student-t with 20
# degrees of freedom and its sample variance has a usable standard error; the transition prior is the default 1 / S
MOMENT_REWARD_PRIOR = [0.6, 2, 1.5, 20]
MOMENT_SAMPLES = 2000


def check_all_rows(Ts, Rs, transition_hp, reward_hp):
    """check_moments for EVERY (s, a) row: Ts [n, S, A, S], Rs [n, S, A] samples at the fixed tables.  Returns the worst
    deviation in standard errors."""
    S, A, _ = transition_hp.shape
    return max(check_moments(Ts[:, s, a], Rs[:, s, a], transition_hp[s, a], reward_hp[s, a]) for s in range(S) for a in range(A))


def check_moments(Ts, Rs, alpha, nig, n_se=6.0):
    """Ts [n, S] samples of ONE Dirichlet row with parameters alpha [S]; Rs [n] samples of one N_NIG pair (mu, lambda,
    alpha, beta), alpha > 2.  Sample mean and variance of every T element and of R within n_se standard errors of the
    analytic values: the element's marginal is Beta(a, a0 - a) with raw moments prod_i (a + i) / (a0 + i); R is
    mu + sqrt(beta / (alpha lambda)) t_{2 alpha}, variance beta / (lambda (alpha - 1)), fourth central moment
    3 var^2 (nu - 2) / (nu - 4).  Returns the largest deviation seen, in standard errors."""
    Ts, Rs = np.asarray(Ts, np.float64), np.asarray(Rs, np.float64)
    n = len(Ts)
    a, a0 = np.asarray(alpha, np.float64), float(np.sum(alpha))
    m = [np.ones_like(a)]
    for i in range(4):
        m.append(m[-1] * (a + i) / (a0 + i))
    mean, var = m[1], m[2] - m[1] ** 2
    mu4 = m[4] - 4 * m[3] * mean + 6 * m[2] * mean ** 2 - 3 * mean ** 4
    worst = 0.0

    def one(x, mean, var, mu4):
        se_m, se_v = np.sqrt(var / n), np.sqrt(np.maximum(mu4 - var ** 2, 0) / n)
        dm, dv = np.abs(x.mean(0) - mean) / se_m, np.abs(x.var(0) - var) / se_v
        return float(max(np.max(dm), np.max(dv)))

    worst = max(worst, one(Ts, mean, var, mu4))
    mu_, lam, al, be = (float(v) for v in nig)
    nu = 2 * al
    assert nu > 4
    rv = be / (lam * (al - 1))
    worst = max(worst, one(Rs[:, None], np.array([mu_]), np.array([rv]), np.array([3 * rv ** 2 * (nu - 2) / (nu - 4)])))
    assert worst <= n_se, worst
    return worst
