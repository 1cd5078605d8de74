"""Extended value iteration (reference colosseum/dynamic_programming/infinite_horizon.py:67-118, _max_proba :222-251):
a float64 NumPy restatement with the kernel's tie order, agent-shaped problem generators and the derived error bound."""
import math

import numpy as np

U = 2.0 ** -24  # float32 unit roundoff


def evi_f64(T, R, beta_r, beta_p, r_max, epsilon=1e-3, max_sweeps=10 ** 6):
    """Steps 1-5 of the reference in float64, argsort ties broken by ascending state index (a stable sort).  Returns
    (span, Q, V, sweeps, last_ptp, max|u1| of the last sweep, ptp(u2) of the last sweep) with span None when max_sweeps pass without
    convergence.  The walk of _max_proba is vectorised over the rows: an entry k of the ascending order is walked when
    the mass still to remove before it is > 0 or it is the row's first nonzero (the loop body runs once before its
    first check)."""
    T = np.asarray(T, np.float64)
    S, A, _ = T.shape
    R = np.asarray(R, np.float64)
    br = np.asarray(beta_r, np.float64)
    bp0 = np.asarray(beta_p, np.float64).reshape(S, A, -1)[:, :, 0]
    ropt = np.minimum(float(np.float32(r_max)), R + br)
    u1 = np.zeros(S)
    order = np.arange(S)
    for sweep in range(1, max_sweeps + 1):
        best = order[-1]
        Q = np.empty((S, A))
        u2 = np.empty(S)
        uo = u1[order]
        for a in range(A):
            x = T[:, a, :][:, order]                      # [S, S] rows in ascending-u order, best last
            pb = x[:, -1]
            min1 = np.minimum(1.0, pb + bp0[:, a] / 2)
            excess = min1 - pb
            rem = excess[:, None] - (np.cumsum(x, axis=1) - x)
            nz = x > 0
            first = nz & (np.cumsum(nz, axis=1) == 1)
            walked = nz & ((rem > 0) | first)
            x2 = x.copy()
            x2[:, -1] = min1
            x2 = np.where(walked, np.maximum(0.0, x - rem), x2)
            onehot = min1 == 1.0
            x2[onehot] = 0.0
            x2[onehot, -1] = 1.0
            v = ropt[:, a] + x2 @ uo - u1
            Q[:, a] = v
            w = v + u1
            if a == 0:
                u2[:] = w
            else:
                take = (w > u2) | (np.abs(w - u2) < epsilon)
                u2[take] = w[take]
        V = Q.max(axis=1)
        d = u2 - u1
        ptp = d.max() - d.min()
        umax = float(np.abs(u1).max())
        if ptp < epsilon:
            return float(u1.max() - u1.min()), Q, V, sweep, float(ptp), umax, float(u2.max() - u2.min())
        u1 = u2
        order = np.argsort(u1, kind="stable")
    return None, Q, V, max_sweeps, float(ptp), umax, float(u2.max() - u2.min())


def bound(sweeps, umax, n_terms=1):
    """Largest |x - x_ref| a float32 solve may show against the float64 restatement after `sweeps` sweeps, for x one of
    u, Q, V and the span.  Per sweep, each row's float32 evaluation differs from the exact one by at most
      p2 stored in float32 (p2_j (1 + U) for every j, p2[s] - 1 rounded once):     2 U max|u|
      the dot product, n_terms roundings of partial sums of magnitude <= 2 max|u|:  2 n_terms U max|u|
      v and v + u1[s] rounded to float32:                                          2 U max|u|
    with max|u| the largest value any sweep reads (the last sweep's, u grows by the gain every sweep).  The sweep is a
    non-expansion in the sup norm, so the differences add up over the sweeps; Q and the span carry one more sweep's
    error and V = max Q no more than Q.  n_terms is 1 for the kernel (one rounding of a float64 sum) and S for a
    BLAS sdot of S terms (the reference)."""
    d = (2 * n_terms + 4) * U * max(1.0, umax)
    return (sweeps + 1) * d


def dense_from_counts(N):
    """The agent's estimate (ucrl2.py:238): P = N / sum N per visited pair, uniform 1/S where nothing was counted."""
    S = N.shape[0]
    tot = N.sum(-1, keepdims=True)
    return np.where(tot > 0, N / np.maximum(tot, 1), 1.0 / S).astype(np.float32)


def _chernoff(it, N, delta, sqrt_C, log_C, range_=1.0):
    return range_ * np.sqrt(sqrt_C * math.log(log_C * (it + 1) / delta) / np.maximum(1, N))


def _bernstein(scale_a, log_scale_a, scale_b, log_scale_b, alpha_1, alpha_2):
    return alpha_1 * np.sqrt(scale_a * math.log(log_scale_a)) + alpha_2 * scale_b * math.log(log_scale_b)


def ucrl2_bounds(P, nobs, var_r, it, kind, r_max=1.0, delta=0.05, alpha_r=1.0, alpha_p=1.0):
    """beta_r [S,A] and beta_p ([S,A,1] Chernoff, [S,A,S] Bernstein) by the formulas of ucrl2.py:22-31,240-308."""
    S, A = nobs.shape
    if kind == "chernoff":
        br = alpha_r * _chernoff(it, nobs, delta, 3.5, 2 * S * A, r_max)
        bp = alpha_p * _chernoff(it, nobs, delta, 14 * S, 2 * A).reshape(S, A, 1)
        return br, bp
    N = np.maximum(1, nobs)
    Nm1 = np.maximum(1, nobs - 1)
    lv = 2.0 * S * A * (it + 1) / delta
    br = _bernstein(14 * (var_r / Nm1) / N, lv, 49.0 * r_max / (3.0 * Nm1), lv, math.sqrt(alpha_r), alpha_r)
    var_p = P * (1.0 - P)
    bp = _bernstein(14 * var_p / N[:, :, None], lv, 49.0 / (3.0 * Nm1[:, :, None]), lv, math.sqrt(alpha_p), alpha_p)
    return br, bp


def agent_problem(T_true, R_true, visits, seed, kind="bernstein", it=None, scale=1.0, r_max=1.0, unvisited=0.3):
    """An agent-shaped EVI input: multinomial counts of `visits` draws per pair from the true rows (a fraction
    `unvisited` of the pairs never visited: uniform rows), the mean rewards observed with noise, UCRL2's bounds at
    iteration `it` (the total visits by default) times `scale`.  Returns (T, estimated_rewards, beta_r, beta_p, r_max):
    T and the rewards float32, the bounds float64, as the agent passes them."""
    rng = np.random.default_rng(seed)
    S, A, _ = T_true.shape
    n = rng.poisson(visits, size=(S, A)) * (rng.random((S, A)) >= unvisited)
    N = np.zeros((S, A, S))
    for s in range(S):
        for a in range(A):
            if n[s, a]:
                p = np.asarray(T_true[s, a], np.float64)
                N[s, a] = rng.multinomial(n[s, a], p / p.sum())
    P = dense_from_counts(N)
    nobs = N.sum(-1)
    Rh = np.where(nobs > 0, np.clip(R_true + rng.normal(0, 0.1, (S, A)) / np.sqrt(np.maximum(nobs, 1)), 0, 1), 0)
    var_r = rng.random((S, A)) * 0.25
    br, bp = ucrl2_bounds(P.astype(np.float64), nobs, var_r, int(nobs.sum()) if it is None else it, kind, r_max)
    return P, Rh.astype(np.float32), br * scale, bp * scale, float(r_max)


def random_problem(S, A, seed, density="mixed", kind="chernoff", scale=0.05, r_max=1.0):
    """A synthetic EVI input: rows with `density` "sparse" (1-3 successors), "uniform" (1/S everywhere), "dense"
    (random full support) or "mixed" (all three), rewards in [0, 1), bounds of either shape times `scale`."""
    rng = np.random.default_rng(seed)
    T = np.zeros((S, A, S), np.float32)
    kinds = {"sparse": [0], "uniform": [1], "dense": [2], "mixed": [0, 1, 2]}[density]
    for s in range(S):
        for a in range(A):
            k = kinds[rng.integers(len(kinds))]
            if k == 1:
                T[s, a] = np.float32(1.0 / S)
            elif k == 0:
                m = int(rng.integers(1, min(3, S) + 1))
                js = rng.choice(S, m, replace=False)
                c = rng.integers(1, 20, m)
                T[s, a, js] = c / c.sum()
            else:
                c = rng.integers(1, 20, S)
                T[s, a] = c / c.sum()
    R = rng.random((S, A)).astype(np.float32)
    br = rng.random((S, A)) * scale
    bp = rng.random((S, A, 1 if kind == "chernoff" else S)) * scale
    return T, R, br, bp, float(r_max)
