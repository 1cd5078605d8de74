"""Test helper for K17 (csrc/cmdp_map_dvi.h): a NumPy twin of the kernel's definition, the derived rounding bound against the
float64 restatement helpers_psrlc.vi_discounted_f64 on the dense MAP model, and the generated problems the CPU and the GPU
tests share.  Nothing here needs a device: the prologue is the host-only cmdp_psrl_map_rows (dp.psrl_map_rows)."""
import functools

import numpy as np

from helpers_psrl import U
from helpers_psrlc import GAUSS_SEIDEL, JACOBI
from colosseum_amd import dynamic_programming as dp

GAMMA09 = float(np.float32(0.9))


def sv64(V):
    """SV of the definition: 64 partial sums, partial l adding double(V[l]), double(V[l + 64]), ... in ascending order to +0,
    combined by the xor butterfly 32, 16, 8, 4, 2, 1."""
    x = np.zeros(64)
    V = np.asarray(V, np.float64)
    for k in range(0, len(V), 64):
        part = V[k:k + 64]
        x[:len(part)] = x[:len(part)] + part
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[idx ^ o]
    assert (x == x[0]).all()
    return float(x[0])


def map_dense(row_ptr, col, t, c, S, A):
    """The dense float32 T_map [S, A, S] of a table form's (t, c)."""
    row_ptr = np.asarray(row_ptr, np.int64)
    T = np.repeat(np.asarray(c, np.float32).reshape(S * A, 1), S, axis=1)
    T[np.repeat(np.arange(S * A), np.diff(row_ptr)), np.asarray(col, np.int64)] = np.asarray(t, np.float32)
    return T.reshape(S, A, S)


def dense_nnz(row_ptr, t, c, S):
    """The count CMDP_SCHEME_AUTO takes: layout positions with t != 0 plus S - len for every row with c != 0."""
    ln = np.diff(np.asarray(row_ptr, np.int64))
    return int((np.asarray(t) != 0).sum() + ((S - ln) * (np.asarray(c).ravel() != 0)).sum())


def map_dvi_twin(row_ptr, col, hp, prior, mu, gamma32, scheme, epsilon=1e-3, max_sweeps=10 ** 6):
    """The definition of csrc/cmdp_map_dvi.h in NumPy: float64 where it says float64, the two sums over e one term after the
    other in layout order from +0, every operation rounded on its own.  Returns (Q, V, sweeps, converged)."""
    mu = np.asarray(mu, np.float32)
    S, A = mu.shape
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    _, c, t = dp.psrl_map_rows(row_ptr, col, hp, prior, S, A)
    c = c.reshape(S * A)
    g = np.float32(gamma32)
    gs = scheme == GAUSS_SEIDEL
    assert scheme in (JACOBI, GAUSS_SEIDEL)
    ln = np.diff(row_ptr)
    full = ln == S
    # per state the rows' positions side by side: a position a row does not have is (column S, 0) and V[S] stays +0
    coef = (g * t if gs else t).astype(np.float32)
    k_row = ((g * c) if gs else c).astype(np.float32).astype(np.float64)
    assert coef.dtype == np.float32
    pads = []
    for s in range(S):
        m = int(ln[s * A:(s + 1) * A].max()) if A else 0
        cc, ww = np.full((A, m), S, np.int64), np.zeros((A, m))
        for a in range(A):
            r = s * A + a
            cc[a, :ln[r]] = col[row_ptr[r]:row_ptr[r + 1]]
            ww[a, :ln[r]] = coef[row_ptr[r]:row_ptr[r + 1]]
        pads.append((cc, ww))
    V = np.zeros(S + 1, np.float32)
    Q = np.zeros((S, A), np.float32)
    mu64 = mu.astype(np.float64)

    def sums(s, X):
        cc, ww = pads[s]
        x = X[cc].astype(np.float64)
        sub, dot = np.zeros(A), np.zeros(A)
        for k in range(cc.shape[1]):
            sub = sub + x[:, k]
            dot = dot + ww[:, k] * x[:, k]    # a product of two float32 values: exact
        return sub, dot

    for sweep in range(1, int(max_sweeps) + 1):
        V_old = V.copy()
        SV = sv64(V_old[:S])
        for s in range(S):
            sub, dot = sums(s, V if gs else V_old)
            rows = slice(s * A, (s + 1) * A)
            inner = np.where(full[rows], dot, k_row[rows] * (SV - sub) + dot)
            if gs:
                Q[s] = (mu64[s] + inner).astype(np.float32)
                v = Q[s].max()
                SV = SV + (float(v) - float(V[s]))
                V[s] = v
            else:
                tv = inner.astype(np.float32)
                Q[s] = mu[s] + g * tv
        if not gs:
            V[:S] = Q.max(-1)
        assert Q.dtype == np.float32 and V.dtype == np.float32
        diff = np.abs(V_old - V).max()
        assert diff.dtype == np.float32
        if float(diff) < epsilon:
            return Q, V[:S].copy(), sweep, True
    return Q, V[:S].copy(), int(max_sweeps), False


def bound_discounted_map(n, gamma, qmax, S):
    """Largest |Q - Q64| K17's solve (csrc/cmdp_map_dvi.h) may show after `n` sweeps against helpers_psrlc.vi_discounted_f64 on
    the dense float32 MAP model (t at the layout's columns, c elsewhere) with the same float32 gamma and mu, derived the way
    helpers_psrlc.bound_discounted is.  M = max(1, qmax), u = 2^-53, |V_j| <= qmax on both sides.

    One row update, float32.  The same roundings as the dense kernel's row: Gauss-Seidel fl32(gamma t_e) and fl32(gamma c),
    whose relative errors U weigh sum_e gamma t_e |V| + gamma c |sum_off V| <= gamma M, then Q = float(.): U M -- 2 U M;
    Jacobi tv = float(.), gamma * tv, R + . -- 3 U M; and one more U M for the float32 subtraction of the stopping rule, so
    that d (device) and d (float64) differ by at most twice the bound: 4 U M per sweep and row, as in bound_discounted.

    One row update, float64: what the factored form adds.  With D = SV - sub standing for the exact sum of V over the columns
    outside the layout,
      SV at the start of a sweep   a sum of S terms in some order: at most S u sum_j |V_j| <= S u S qmax
      SV's updates within a sweep  SV + (V_new - V[s]): the difference of two float32 values is rounded by at most
                                   u 2 qmax, the sum by at most u |SV| <= u S qmax, and a state late in the sweep sees up
                                   to S of them: S u (S + 2) qmax
      sub                          len <= S terms: S u S qmax
      SV - sub                     u S qmax
    so |D - D_exact| <= u qmax S (3 S + 3).  It is multiplied by gc <= gamma c (1 + U), and c (S - len) <= 1 up to the float32
    rounding of the row sum and of the division, (1 + 2 S U): a row with a single column outside its layout has c as large
    as 1, so nothing of S (3 S + 3) is divided away in the worst case.  (A row with len == S leaves the term out: its D would
    be rounding error alone.)  Then the product gc D: u gamma qmax; dot: S u gamma qmax; the two additions: u gamma qmax and
    2 u M.  Together at most u M (3 S (S + 1) + S + 4); 2^-52 instead of 2^-53 covers the second-order terms and the
    (1 + 2 S U) above.  The Jacobi row has the same terms without gamma.
      e = (4 U + (3 S (S + 1) + S + 4) 2^-52) M per sweep and row.

    Sweeps.  As in bound_discounted, with the exact row map's coefficients gamma T_j summing to at most
    gamma' = gamma (1 + S U) instead of less than gamma: a MAP row sums to one only up to the float32 rounding of its row
    sum and divisions.  E_n <= e (1 - gamma'^n) / (1 - gamma'), for gamma' < 1.  The factor 1 + 2^-20 covers qmax being taken
    from the restatement instead of the computed values."""
    e = (4 * U + (3.0 * S * (S + 1) + S + 4) * 2.0 ** -52) * max(1.0, qmax)
    g = gamma * (1.0 + S * U)
    assert g < 1.0
    return e * (1.0 - g ** n) / (1.0 - g) * (1 + 2.0 ** -20)


# ---- generated problems ------------------------------------------------------------------------------------------------
def make_problem(rng, S, A, prior=None, lens=None, max_len=6, min_len=0, max_count=10 ** 5, mu_scale=1.0):
    """A table-form problem (row_ptr, col, hp, prior, mu): per row `len` random ascending columns (lens: {row: len}
    overrides; otherwise uniform in [min_len, min(S, max_len)]), hp = prior + an integer count up to max_count, mu normal
    of both signs times mu_scale.  prior None: 1 / S."""
    prior = np.float32(1.0 / S if prior is None else prior)
    ln = rng.randint(min_len, min(S, max_len) + 1, size=S * A)
    ln = np.maximum(ln, min(min_len, S))
    for r, k in (lens or {}).items():
        ln[r] = k
    row_ptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(S, k, replace=False)) for k in ln] + [np.zeros(0, np.int64)]).astype(np.int32)
    counts = rng.randint(0, max_count + 1, size=len(col))
    counts[rng.rand(len(col)) < 0.3] //= 1000    # small counts next to large ones
    hp = (prior + counts.astype(np.float32)).astype(np.float32)
    mu = (mu_scale * rng.normal(size=(S, A))).astype(np.float32)
    return row_ptr, col, hp, prior, mu


@functools.lru_cache(maxsize=None)
def ragged_problems(which):
    """The shapes at which K17 can go wrong, as two batches by the gamma their float64 restatement can afford.

    "small" (gamma = 0.99: hundreds of sweeps).  S = 1 with an empty layout (c = 1) and with len == S; S = 2, 3, 5: not a
    multiple of 4; A = 1, 3, 4, 5, 16, 17, 64, 65: every depth of the max over the actions, and one action more than the
    wavefront has lanes; an instance with mu = 0, which converges in its first sweep next to instances that take hundreds;
    S = 64 at four actions; a prior of 1 / S and user priors.
    "large" (gamma = 0.9).  S = 63, 64, 65, 129, 200: around one wavefront, past the pairwise sum's 128-element block, a row
    with len == S, rows with an empty layout, a row of 70 > 64 positions, and (129, 64): 8256 rows, whose tables exceed what
    the picker keeps in LDS, so it reads them from global memory in the same launch as the staged ones."""
    rng = np.random.RandomState(17 if which == "small" else 19)
    if which == "small":
        ps = [make_problem(rng, 1, 1, lens={0: 0}),
              make_problem(rng, 1, 3, prior=0.7, lens={0: 1, 1: 0, 2: 1}),
              make_problem(rng, 2, 4, lens={0: 2, 3: 0}),
              make_problem(rng, 3, 5, prior=2.5, lens={1: 3, 2: 0}),
              make_problem(rng, 5, 64, lens={7: 5, 8: 0}),
              make_problem(rng, 3, 65, prior=0.4, lens={64: 3, 130: 0}),
              make_problem(rng, 5, 16), make_problem(rng, 5, 17, prior=0.05),
              make_problem(rng, 64, 4, lens={0: 0, 255: 64}),
              make_problem(rng, 5, 4, mu_scale=0.0)]
        assert not ps[-1][4].any()
        return ps
    ps = [make_problem(rng, 63, 4, lens={5: 63, 6: 0}),
          make_problem(rng, 64, 3, prior=0.3),
          make_problem(rng, 65, 5, lens={0: 65, 324: 0}),
          make_problem(rng, 129, 1, prior=1.5, lens={128: 129, 3: 0}),
          make_problem(rng, 200, 4, lens={11: 70, 12: 0, 799: 200}),
          make_problem(rng, 129, 64, max_len=2)]
    return ps


def rule_problems():
    """Two instances of one shape whose scheme differs under a lowered size threshold: with a prior of 1 / S every element
    of the dense MAP model is non-zero (Gauss-Seidel); with the smallest subnormal as the user prior under counts of thousands c =
    prior / rowsum underflows to +0, the model is as sparse as the layout (density <= 6 / 63 < 0.2) and the rule takes Jacobi."""
    rng = np.random.RandomState(23)
    dense = make_problem(rng, 63, 4, min_len=1)
    sparse = make_problem(rng, 63, 4, prior=np.float32(1e-45), min_len=1)
    row_ptr, col, hp, prior, mu = sparse
    hp = np.maximum(hp, np.float32(1000.0))    # every row sums to at least 1000: c = 0 in float32
    return [dense, (row_ptr, col, hp, prior, mu)]
