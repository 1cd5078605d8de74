"""Synthetic CSR batches of exactly controlled shape for the discounted sweep kernels, a host mirror of the kernel choice
of `pick_sweep` (colosseum_amd/csrc/cmdp_dp_plan.h), the table of compiled register-resident instantiations, and float64
references (policy iteration and linear solves) of the discounted solutions.  Host only: no GPU is touched here."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP_PLAN_H = os.path.join(ROOT, "colosseum_amd", "csrc", "cmdp_dp_plan.h")

# CMDP_OPT_DP_KERNEL values and the STAT_DP_KERNEL codes of the sweep families
AUTO, WORKGROUP, FORCE_K2R, FORCE_K2U, FORCE_K2W = 0, 1, 2, 5, 7
FAMILY_CODE = {"K2": 1, "K2R": 2, "K2U": 5, "GS": 6, "K2W": 7}
FORCE_OF = {"K2R": FORCE_K2R, "K2U": FORCE_K2U, "K2W": FORCE_K2W}
UNSUPPORTED = "unsupported"

LDS_BUDGET = 160 * 1024  # kLdsBudget
DP_BLOCK = 256           # kDpBlock

# ---- the compiled register-resident instantiations ---------------------------------------------------------------------
# K2R key (A, K, spt); K2U key (A, U, K, spt); K2W key (A, st_w).  K = max row nnz rounded up to 4 or 8, U = distinct
# successors per state rounded up to 5 or 8, spt = states per lane (256 lanes), st_w = states per lane of one wavefront.
K2R_KEYS = [(2, 4, 1), (2, 4, 2), (2, 4, 4), (3, 4, 1), (3, 4, 2), (3, 4, 4), (4, 4, 1), (4, 4, 2), (4, 4, 4),
            (2, 8, 1), (2, 8, 2), (3, 8, 1), (3, 8, 2), (4, 8, 1), (4, 8, 2)]
K2U_KEYS = [(a, 5, k, s) for a in (2, 3, 4) for k in (4, 8) for s in (1, 2, 4)] + \
           [(3, 8, 8, 1), (3, 8, 8, 2), (4, 8, 4, 1), (4, 8, 4, 2), (4, 8, 8, 1), (4, 8, 8, 2)]
K2W_KEYS = [(2, 5), (2, 6), (2, 7), (3, 5), (3, 6), (3, 7), (4, 5)]
K2W_VI_ONLY = [(4, 6)]   # with four actions and six states per lane only value iteration keeps its tables in registers


def compiled_cases():
    """{(family, key, mode)} of the test's table: 93 register-resident kernels."""
    out = set()
    for fam, keys in (("K2R", K2R_KEYS), ("K2U", K2U_KEYS), ("K2W", K2W_KEYS)):
        for k in keys:
            out |= {(fam, k, "VI"), (fam, k, "PE")}
    out |= {("K2W", k, "VI") for k in K2W_VI_ONLY}
    return out


def shapes():
    """The 47 (family, key) shapes, each with the modes it is compiled for."""
    d = {}
    for fam, key, mode in sorted(compiled_cases()):
        d.setdefault((fam, key), []).append(mode)
    return d


def parse_compiled(path=DP_PLAN_H):
    """The same set as `compiled_cases`, read from the shape lists `CMDP_K2R_SHAPES`, `CMDP_K2U_SHAPES` and
    `CMDP_K2W_SHAPES` of cmdp_dp_plan.h: one X(...) per shape, the K2W rows marked VI_PE or VI."""
    src = open(path).read()
    out = set()
    for fam in ("K2R", "K2U", "K2W"):
        body = re.search(r"#define CMDP_%s_SHAPES\(X\)((?:[^\n]*\\\n)*[^\n]*)" % fam, src).group(1)
        for args in re.findall(r"\bX\(([^)]*)\)", body):
            args = [a.strip() for a in args.split(",")]
            modes = args.pop().split("_") if fam == "K2W" else ["VI", "PE"]
            out |= {(fam, tuple(int(x) for x in args), m) for m in modes}
    return out


# ---- host mirror of the shape statistics (cmdp_create) and of the kernel choice (pick_sweep) -----------------------------
def shape_stats(t):
    """(A, max row nnz, max distinct successors per state (0 when some row is not strictly ascending, or when the
    statistic is not gathered), max S, max nnz of one instance) as cmdp_create computes them."""
    A, off, ptr, col = int(t["A"]), t["state_off"], t["csr_ptr"], t["csr_col"]
    S = np.diff(off)
    row_nnz = np.diff(ptr)
    max_row = int(row_nnz.max()) if len(row_nnz) else 0
    max_S = int(S.max())
    inst_nnz = int(max(ptr[off[b + 1] * A] - ptr[off[b] * A] for b in range(len(S))))
    uniq = 0
    if A <= 4 and max_row <= 8 and max_S <= 1024:
        same_row = np.ones(len(col), bool)
        same_row[ptr[:-1][row_nnz > 0]] = False  # first entry of every row
        if np.all(np.diff(col)[same_row[1:]] > 0):
            for s in range(int(off[-1])):
                uniq = max(uniq, len(np.unique(col[ptr[s * A]:ptr[(s + 1) * A]])))
    return A, max_row, uniq, max_S, inst_nnz


def select(stats, mode, scheme=1, forced=AUTO):
    """(family, key) that pick_sweep chooses for a batch with `stats` (shape_stats), or (UNSUPPORTED, reason).
    family K2 has key "lds" / "hbm" (where the CSR lives), GS has key None."""
    A, nnz, mu, S, inst_nnz = stats
    if scheme == 1 and forced != WORKGROUP:
        K = 4 if nnz <= 4 else (8 if nnz <= 8 else 0)
        spt = 1 if S <= 256 else (2 if S <= 512 else (4 if S <= 1024 else 0))
        U = 0 if mu == 0 else (5 if mu <= 5 else (8 if mu <= 8 else 0))
        want_u = (U > 0 and K > 0 and spt > 0 and spt * U <= 20 and forced != FORCE_K2R
                  and (forced in (FORCE_K2U, FORCE_K2W) or 2 * U <= A * K))
        if forced == FORCE_K2U and not want_u:
            return UNSUPPORTED, "K2U shape"
        sptw = (S + 63) // 64
        want_w = want_u and U == 5 and K == 4 and sptw <= 7 and (forced == FORCE_K2W or (forced == AUTO and sptw >= 5))
        if forced == FORCE_K2W and not want_w:
            return UNSUPPORTED, "K2W shape"
        if want_w:
            st_w = max(5, sptw)
            if (A, st_w) in K2W_KEYS or ((A, st_w) in K2W_VI_ONLY and mode == "VI"):
                return "K2W", (A, st_w)
            if forced == FORCE_K2W:
                return UNSUPPORTED, "K2W instantiation"
        if want_u:
            if (A, U, K, spt) in K2U_KEYS:
                return "K2U", (A, U, K, spt)
            if forced == FORCE_K2U:
                return UNSUPPORTED, "K2U instantiation"
        if (A, K, spt) in K2R_KEYS:
            return "K2R", (A, K, spt)
        if forced == FORCE_K2R:
            return UNSUPPORTED, "K2R instantiation"
    if scheme == 1:
        base = 2 * 4 * S + 4 * 4 * (DP_BLOCK // 64)
        csr = 4 * (S * A + 1) + 8 * inst_nnz + 4 * S * A
        if base > LDS_BUDGET:
            return UNSUPPORTED, "LDS"
        return "K2", ("lds" if base + csr <= LDS_BUDGET // 2 else "hbm")
    if 4 * S > LDS_BUDGET:
        return UNSUPPORTED, "LDS"
    return "GS", None


def k_round(nnz):
    return 4 if nnz <= 4 else 8


def u_round(u):
    return 5 if u <= 5 else 8


# ---- the synthetic generator -----------------------------------------------------------------------------------------
def _row_probs(rng, n, zeros):
    """float32 probabilities of one row of n entries: Dirichlet, one-hot (the others explicit zeros when allowed, else
    ~1e-7), or Dirichlet with entries of ~1e-7 mixed in."""
    kind = rng.random()
    if n > 1 and kind < 0.15:
        p = np.full(n, 0.0 if zeros else 1e-7, np.float64)
        p[rng.integers(n)] = 1.0 - p.sum()
    else:
        p = rng.dirichlet(np.full(n, 0.7))
        if n > 1 and kind < 0.35:
            p[rng.integers(n)] = 1.2e-7
        if zeros and n > 1 and rng.random() < 0.2:
            p[rng.integers(n)] = 0.0
        p = p / p.sum()
    return p.astype(np.float32)


def generate(A, sizes, nnz, uniq, seed, sorted_rows=True, zeros=False, rewards="unit", dense_states=False):
    """tables for BatchedMDP(tables=..., with_env=False): one instance per entry of `sizes` (ragged).
    Every state draws a successor set of min(uniq, S) columns (the first state of every instance, every state when
    dense_states, half the others; the rest a random size below), and each of its A rows takes a subset of it of at most
    k = min(nnz, set size) columns, the rows together covering the set and one row holding exactly k.  So the batch's max
    row nnz is exactly `nnz` and its max distinct successors per state exactly `uniq` as soon as one instance has `uniq`
    states.  Rows list their columns in ascending order; sorted_rows=False reverses one row of two or more entries
    (forcing U = 0).  rewards: "unit" U[0, 1), "neg" U[-1, 0), "equal" 0.5 everywhere (ties in Q)."""
    assert 1 <= nnz <= uniq and A * nnz >= uniq, (A, nnz, uniq)
    rng = np.random.default_rng(seed)
    ptr, col, val, R = [0], [], [], []
    for S in sizes:
        u_max = min(uniq, S)
        for s in range(S):
            u = u_max if (s == 0 or dense_states or rng.random() < 0.5) else int(rng.integers(1, u_max + 1))
            succ = rng.choice(S, size=u, replace=False)
            k_max = min(nnz, u)
            want = rng.integers(1, k_max + 1, size=A)
            want[int(rng.integers(A))] = k_max
            rows = [set() for _ in range(A)]
            for c in succ[rng.permutation(u)]:   # every successor lands in some row (A * k_max >= u) ...
                free = [a for a in range(A) if len(rows[a]) < want[a]] or [a for a in range(A) if len(rows[a]) < k_max]
                rows[int(rng.choice(free))].add(int(c))
            for a in range(A):                   # ... then rows are topped up to their drawn sizes
                while len(rows[a]) < want[a]:
                    rows[a].add(int(succ[int(rng.integers(u))]))
            for a in range(A):
                p = _row_probs(rng, len(rows[a]), zeros)
                col.extend(sorted(rows[a]))
                val.extend(p.tolist())
                ptr.append(ptr[-1] + len(rows[a]))
        if rewards == "unit":
            R.append(rng.random(S * A))
        elif rewards == "neg":
            R.append(-rng.random(S * A))
        else:
            R.append(np.full(S * A, 0.5))
    ptr, col = np.asarray(ptr, np.int64), np.asarray(col, np.int32)
    val = np.asarray(val, np.float32)
    if not sorted_rows:   # the last row of two or more entries, in descending column order
        r = int(np.flatnonzero(np.diff(ptr) >= 2)[-1])
        col[ptr[r]:ptr[r + 1]] = col[ptr[r]:ptr[r + 1]][::-1].copy()
        val[ptr[r]:ptr[r + 1]] = val[ptr[r]:ptr[r + 1]][::-1].copy()
    rr = {"unit": (0.0, 1.0), "neg": (-1.0, 0.0), "equal": (0.0, 1.0)}[rewards]
    return dict(B=len(sizes), A=A, H=0, rewards_range=rr,
                state_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                csr_ptr=ptr, csr_col=col, csr_val=val, R=np.concatenate(R).astype(np.float32))


def instance(t, b):
    """(S, A, (ptr, col, val), R[S, A]) of instance b of a table dict."""
    A, off, ptr = int(t["A"]), t["state_off"], t["csr_ptr"]
    s0, s1 = int(off[b]), int(off[b + 1])
    p = ptr[s0 * A: s1 * A + 1]
    lp = (p - p[0]).astype(np.int64)
    col = t["csr_col"][p[0]:p[-1]]
    val = t["csr_val"][p[0]:p[-1]]
    return s1 - s0, A, (lp, col, val), t["R"][s0 * A: s1 * A].reshape(s1 - s0, A)


def policies(t, kind, seed):
    """One float32 policy [S_b, A] per instance: "dirichlet" or "onehot"."""
    rng = np.random.default_rng(seed)
    A, out = int(t["A"]), []
    for S in np.diff(t["state_off"]):
        if kind == "dirichlet":
            out.append(rng.dirichlet(np.ones(A), int(S)).astype(np.float32))
        else:
            p = np.zeros((int(S), A), np.float32)
            p[np.arange(S), rng.integers(A, size=int(S))] = 1.0
            out.append(p)
    return out


def shape_batch(fam, key, seed):
    """The ragged batch of one register-resident shape: the instance that sets it at the top of its states-per-lane band,
    a one-state instance and a mid-size one (B = 3, no multiple of 64)."""
    if fam == "K2W":
        A, st_w = key
        S, nnz, uniq = 64 * st_w, 4, 5
    elif fam == "K2U":
        A, U, K, spt = key
        S, uniq = 256 * spt, U
        nnz = 4 if K == 4 else (5 if U == 5 else 8)   # U = 5 allows at most 5 per row
    else:
        A, K, spt = key
        S = 256 * spt
        nnz = K
        uniq = 9 if K == 8 else 7   # no K2U shape: the automatic choice is K2R too
    sizes = [S // 2 + 3, 1, S]
    return generate(A, sizes, nnz, uniq, seed, sorted_rows=fam != "K2R" or K == 8,
                    zeros=bool(seed % 2), dense_states=True)


# ---- float64 references --------------------------------------------------------------------------------------------
def dense_P(S, A, csr):
    """P[S*A, S] float64 holding the float32 probabilities exactly (entries of the same column summed)."""
    ptr, col, val = csr
    P = np.zeros((S * A, S), np.float64)
    rows = np.repeat(np.arange(S * A), np.diff(ptr))
    np.add.at(P, (rows, col), val.astype(np.float64))
    return P


def pe_f64(S, A, csr, R, pi, gamma):
    """V^pi = (I - gamma P_pi)^-1 r_pi and Q^pi = R + gamma P V^pi, float64."""
    P = dense_P(S, A, csr).reshape(S, A, S)
    pi = np.asarray(pi, np.float64).reshape(S, A)
    Ppi = np.einsum("sa,sat->st", pi, P)
    rpi = (pi * np.asarray(R, np.float64).reshape(S, A)).sum(1)
    V = np.linalg.solve(np.eye(S) - gamma * Ppi, rpi)
    return np.asarray(R, np.float64).reshape(S, A) + gamma * (P @ V), V


def vi_f64(S, A, csr, R, gamma):
    """Q*, V* by float64 policy iteration (an action is only replaced by a strictly better one, so ties cannot cycle);
    the returned pair satisfies the Bellman optimality equation to ~1e-12."""
    P = dense_P(S, A, csr).reshape(S, A, S)
    R64 = np.asarray(R, np.float64).reshape(S, A)
    act = np.zeros(S, np.int64)
    for _ in range(200):
        pi = np.zeros((S, A))
        pi[np.arange(S), act] = 1.0
        Ppi = P[np.arange(S), act]
        V = np.linalg.solve(np.eye(S) - gamma * Ppi, R64[np.arange(S), act])
        Q = R64 + gamma * (P @ V)
        best = Q.argmax(1)
        tol = 1e-12 * max(1.0, float(np.abs(V).max()))
        better = Q[np.arange(S), best] > Q[np.arange(S), act] + tol
        if not better.any():
            res = np.abs(Q.max(1) - V).max()
            assert res <= 1e-9 * max(1.0, float(np.abs(V).max())), res
            return Q, V
        act = np.where(better, best, act)
    raise AssertionError("float64 policy iteration did not settle")


def f64_bound(gamma, eps, K, vmax):
    """Largest |V - V_ref| a float32 Jacobi / Gauss-Seidel solve stopped at max|V_n - V_n-1| < eps may show against the
    exact float64 solution V_ref of the same (float32-valued) tables.

    Let T be the exact backup and T~ its float32 evaluation, |T~V - TV| <= d for every V the sweeps meet.  Then
      |V_n - V*| <= |T~V_n-1 - TV_n-1| + |TV_n-1 - TV*| <= d + gamma |V_n-1 - V*|
                 <= d + gamma (|V_n-1 - V_n| + |V_n - V*|) < d + gamma eps + gamma |V_n - V*|,
    so |V_n - V*| < (gamma eps + d) / (1 - gamma).  One backup of a row of k <= K entries is k products and k - 1 sums
    (recursive summation: error <= (k - 1 + 1) u sum_j p_j |v_j| <= K u max|V| for probabilities summing to 1 in float32),
    one product by gamma and one sum with R (2 u max|Q|), and for policy evaluation the A-term sum over pi (A u max|Q|,
    A <= K + 2); with the unit roundoff u = 2^-24 every term is covered by d = (K + 2) 2^-23 max|V|, max|V| read as the
    larger of max|V| and max|Q|.  Q = R + gamma P V gains one more backup: |Q_n - Q_ref| <= gamma (eps + bound) + d
    <= eps + bound."""
    d = (K + 2) * 2.0 ** -23 * vmax
    return (gamma * eps + d) / (1.0 - gamma)
