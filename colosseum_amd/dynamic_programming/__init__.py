"""Drop-in for `colosseum.dynamic_programming` (reference colosseum/dynamic_programming/*.py): the same
free functions on dense float32 `T[S,A,S]`, `R[S,A]`, executed by the HIP sweep kernels of libcmdp.so.

Signatures, defaults, return conventions (`None` when `max_abs_value` is exceeded, the
`DynamicProgrammingMaxIterationExceeded` exception after 10**6 sweeps) follow the reference."""
import numpy as np

from .. import _lib as L
from .._lib import DynamicProgrammingMaxIterationExceeded  # noqa: F401
from ..dp_handle import DPBatch, csr_from_dense

DP_MAX_ITERATION = int(1e6)
ARGMAX_SEED = 42

# The reference's functions take dense arrays and own no state; an `MDPLoop` calls them with the SAME (T, R) at every
# logging step.  The device handle of a (T, R) pair (CSR extraction, allocation, upload) is therefore kept and found
# again by content: a few of them, least recently used first out.
_HANDLES = {}
_MAX_HANDLES = 4


def _handle(T, R):
    import hashlib

    T = np.ascontiguousarray(T, np.float32)
    R = np.ascontiguousarray(R, np.float32)
    key = (T.shape, hashlib.blake2b(T.data, digest_size=16).digest(), hashlib.blake2b(R.data, digest_size=16).digest())
    dp = _HANDLES.pop(key, None)
    if dp is None:
        S, A, _ = T.shape
        dp = DPBatch([(S, A, csr_from_dense(T), R)])
        dp.nnz = int(dp._keep["csr_ptr"][-1])
        while len(_HANDLES) >= _MAX_HANDLES:
            _HANDLES.pop(next(iter(_HANDLES))).close()
    _HANDLES[key] = dp  # most recently used last
    return dp


def release_handles():
    """Frees the cached device handles (they are also freed at interpreter exit)."""
    while _HANDLES:
        _HANDLES.popitem()[1].close()


def _vi_rule(T_size, nnz, sparse_n_states_threshold, sparse_nnz_per_threshold):
    """reference infinite_horizon.py:28-36."""
    if T_size > sparse_n_states_threshold and nnz / T_size < sparse_nnz_per_threshold:
        return L.SCHEME_JACOBI
    return L.SCHEME_GAUSS_SEIDEL


def discounted_value_iteration(T, R, gamma=0.99, epsilon=1e-3, max_abs_value=None,
                               sparse_n_states_threshold=300 * 3 * 300, sparse_nnz_per_threshold=0.2):
    """reference infinite_horizon.py:14-44.  Returns (Q [S,A], V [S]) float32, or None."""
    S, A, _ = T.shape
    dp = _handle(T, R)
    scheme = _vi_rule(T.size, dp.nnz, sparse_n_states_threshold, sparse_nnz_per_threshold)
    try:
        Q, V, _ = dp.value_iteration(gamma, epsilon, scheme, DP_MAX_ITERATION, max_abs_value)
    except L.CmdpError as e:
        if e.code == L.ERR_MAX_VALUE:
            return None
        raise
    return Q.reshape(S, A), V


def discounted_policy_evaluation(T, R, pi, gamma=0.99, epsilon=1e-7, sparse_n_states_threshold=200,
                                 sparse_nnz_per_threshold=0.2):
    """reference infinite_horizon.py:47-64."""
    S, A, _ = T.shape
    dp = _handle(T, R)
    scheme = (L.SCHEME_JACOBI if (S > sparse_n_states_threshold and dp.nnz / T.size < sparse_nnz_per_threshold)
              else L.SCHEME_GAUSS_SEIDEL)
    Q, V, _ = dp.policy_evaluation(np.asarray(pi, np.float32).ravel(), gamma, epsilon, scheme, DP_MAX_ITERATION)
    return Q.reshape(S, A), V


def episodic_value_iteration(H, T, R, max_value=None):
    """reference finite_horizon.py:11-26.  Returns (Q [H+1,S,A], V [H+1,S]) or None when a value exceeds
    `max_value`."""
    S, A, _ = T.shape
    Q, V = _handle(T, R).episodic_value_iteration(int(H))
    Q, V = Q.reshape(H + 1, S, A), V.reshape(H + 1, S)
    if max_value is not None and (V > max_value).any():
        return None
    return Q, V


def episodic_value_iteration_dense_batch(problems, H):
    """`episodic_value_iteration(H, T, R)` for many dense (T [S, A, S], R [S, A]) float32 problems in one launch of
    k_vi_episodic_dense (the PSRL agent's solver; the problems may differ in S and A): the dot products are accumulated in
    float64 in a fixed order and rounded once.  Returns [(Q [H + 1, S, A], V [H + 1, S]) per problem]."""
    problems = [(np.ascontiguousarray(T, np.float32), np.ascontiguousarray(R, np.float32)) for T, R in problems]
    if not problems:
        return []
    S = np.array([T.shape[0] for T, _ in problems], np.int32)
    A = np.array([T.shape[1] for T, _ in problems], np.int32)
    for (T, R), s, a in zip(problems, S, A):
        assert T.shape == (s, a, s) and R.shape == (s, a), (T.shape, R.shape)
    Tc = np.concatenate([T.ravel() for T, _ in problems])
    Rc = np.concatenate([R.ravel() for _, R in problems])
    H = int(H)
    Q = np.zeros((H + 1) * int((S * A).sum()), np.float32)
    V = np.zeros((H + 1) * int(S.sum()), np.float32)
    L.check(L.load().cmdp_vi_episodic_dense(len(problems), L.ptr(S), L.ptr(A), H, L.ptr(Tc), L.ptr(Rc), L.ptr(Q), L.ptr(V)))
    out, q0, v0 = [], 0, 0
    for s, a in zip(S.tolist(), A.tolist()):
        nq, nv = (H + 1) * s * a, (H + 1) * s
        out.append((Q[q0:q0 + nq].reshape(H + 1, s, a), V[v0:v0 + nv].reshape(H + 1, s)))
        q0, v0 = q0 + nq, v0 + nv
    return out


def discounted_value_iteration_dense_batch(problems, gamma=0.99, epsilon=1e-3, sparse_n_states_threshold=300 * 3 * 300,
                                           sparse_nnz_per_threshold=0.2, scheme=None, max_sweeps=DP_MAX_ITERATION):
    """`discounted_value_iteration(T, R)` for many dense (T [S, A, S], R [S, A]) float32 problems in one launch of
    k_vi_discounted_dense (the continuous PSRL agent's solver; the problems may differ in S and A).  The reference's rule
    picks Jacobi or Gauss-Seidel per problem from its count of non-zero elements unless `scheme` (L.SCHEME_JACOBI /
    L.SCHEME_GAUSS_SEIDEL) forces one; the row sums are accumulated in float64 in a fixed order.  A problem that takes
    `max_sweeps` sweeps returns the last sweep's values.  Returns [(Q [S, A], V [S], sweeps, scheme) per problem]; `status`
    of the last call (0 or L.ERR_MAX_ITER per problem) is left in `discounted_value_iteration_dense_batch.status`."""
    problems = [(np.ascontiguousarray(T, np.float32), np.ascontiguousarray(R, np.float32)) for T, R in problems]
    if not problems:
        return []
    S = np.array([T.shape[0] for T, _ in problems], np.int32)
    A = np.array([T.shape[1] for T, _ in problems], np.int32)
    for (T, R), s, a in zip(problems, S, A):
        assert T.shape == (s, a, s) and R.shape == (s, a), (T.shape, R.shape)
    n = len(problems)
    Tc = np.concatenate([T.ravel() for T, _ in problems])
    Rc = np.concatenate([R.ravel() for _, R in problems])
    Q, V = np.zeros(int((S * A).sum()), np.float32), np.zeros(int(S.sum()), np.float32)
    sweeps, used, status = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
    L.check(L.load().cmdp_vi_discounted_dense(n, L.ptr(S), L.ptr(A), L.ptr(Tc), L.ptr(Rc), float(gamma), float(epsilon),
                                              L.SCHEME_AUTO if scheme is None else int(scheme), int(sparse_n_states_threshold),
                                              float(sparse_nnz_per_threshold), int(max_sweeps), L.ptr(Q), L.ptr(V), L.ptr(sweeps),
                                              L.ptr(used), L.ptr(status)))
    discounted_value_iteration_dense_batch.status = status
    out, q0, v0 = [], 0, 0
    for b, (s, a) in enumerate(zip(S.tolist(), A.tolist())):
        out.append((Q[q0:q0 + s * a].reshape(s, a), V[v0:v0 + s], int(sweeps[b]), int(used[b])))
        q0, v0 = q0 + s * a, v0 + s
    return out


def optimistic_compact_from_dense(T_ext, psi, row_ptr, col, R, simple=None, z=None):
    """The compact form (csrc/cmdp_psrlo_vi.h) of an extended sample `T_ext` [S, A * psi, S] float32 over the layout
    (`row_ptr` [S * A + 1], `col`) of its real rows, with the real rewards `R` [S, A]: a dict of S, A, psi, row_ptr, col,
    `simple` [S * A] bool, `z` [psi], `pmk` [psi, nz], `bump` [psi, S * A], `pidx` [S * A] (-1 on simple rows), `post`
    [psi, n1, S] and R.  A real row can be simple when each of its psi copies is zero outside its layout columns and z_k.
    Without `z`, z_k is the column outside the layout most such rows are non-zero at in copy k (0 when there is none);
    without `simple`, every row that can be simple under that z is; the others are posterior rows, kept dense.
    `optimistic_expand` is the inverse and is asserted to give `T_ext` back bit for bit."""
    T = np.ascontiguousarray(T_ext, np.float32)
    S, AX, S2 = T.shape
    psi = int(psi)
    A = AX // psi
    assert S == S2 and A * psi == AX, T.shape
    rows = S * A
    row_ptr, col = np.asarray(row_ptr, np.int64), np.asarray(col, np.int32)
    assert row_ptr.shape == (rows + 1,) and row_ptr[0] == 0 and len(col) == row_ptr[-1]
    Tk = T.reshape(rows, psi, S)                     # extended row j = a * psi + k of state s: real row s * A + a, copy k
    inlay = np.zeros((rows, S), bool)
    inlay[np.repeat(np.arange(rows), np.diff(row_ptr)), col] = True
    off = (Tk != 0) & ~inlay[:, None, :]             # non-zeros outside the layout
    if z is None:
        cand = (off.sum(-1) <= 1).all(-1)
        z = np.zeros(psi, np.int32)
        for k in range(psi):
            votes = off[cand, k].sum(0)
            z[k] = int(votes.argmax()) if votes.any() else 0
    z = np.asarray(z, np.int32)
    outside = off.copy()
    outside[:, np.arange(psi), np.clip(z, 0, S - 1)] = False
    can = ~outside.any((1, 2))
    simple = can if simple is None else np.asarray(simple, bool).reshape(rows)
    assert not (simple & ~can).any(), "a row marked simple is non-zero outside its layout and z"
    assert not simple.any() or ((z >= 0) & (z < S)).all()
    nz = len(col)
    erow = np.repeat(np.arange(rows), np.diff(row_ptr))
    pmk = np.ascontiguousarray(Tk[erow, :, col].T) if nz else np.zeros((psi, 0), np.float32)
    pmk = pmk * simple[erow][None, :].astype(np.float32)
    bump = np.where(simple[None, :], Tk[:, np.arange(psi), np.clip(z, 0, S - 1)].T, np.float32(0)).astype(np.float32)
    pidx = np.where(simple, -1, np.cumsum(~simple) - 1).astype(np.int32)
    post = np.ascontiguousarray(np.moveaxis(Tk[~simple], 0, 1))
    out = dict(S=S, A=A, psi=psi, row_ptr=row_ptr, col=col, simple=simple, z=z, pmk=np.ascontiguousarray(pmk, np.float32),
               bump=np.ascontiguousarray(bump), pidx=pidx, post=post, R=np.ascontiguousarray(R, np.float32).reshape(S, A))
    assert np.array_equal(optimistic_expand(out), T)
    return out


def optimistic_expand(p):
    """T_ext [S, A * psi, S] float32 of a compact sample (the dict of `optimistic_compact_from_dense`): zeros, the layout's
    values, then z_k for a simple row; the dense rows for a posterior one."""
    S, A, psi = p["S"], p["A"], p["psi"]
    rows = S * A
    row_ptr, col, simple = p["row_ptr"], p["col"], np.asarray(p["simple"], bool).reshape(rows)
    Tk = np.zeros((rows, psi, S), np.float32)
    erow = np.repeat(np.arange(rows), np.diff(row_ptr))
    keep = simple[erow]
    Tk[erow[keep], :, col[keep]] = p["pmk"][:, keep].T
    if simple.any():
        Tk[np.flatnonzero(simple)[:, None], np.arange(psi)[None, :], np.asarray(p["z"])[None, :]] = p["bump"][:, simple].T
    if (~simple).any():
        Tk[~simple] = np.moveaxis(np.asarray(p["post"], np.float32).reshape(psi, -1, S), 0, 1)
    return Tk.reshape(S, A * psi, S)


def discounted_value_iteration_optimistic_batch(problems, gamma=0.99, epsilon=1e-3, sparse_n_states_threshold=300 * 3 * 300,
                                                sparse_nnz_per_threshold=0.2, scheme=None, max_sweeps=DP_MAX_ITERATION):
    """`discounted_value_iteration(T_ext, R_ext)` on many COMPACT optimistic samples (dicts of
    `optimistic_compact_from_dense`; they may differ in S, A and psi) in one launch of k_vi_discounted_optimistic (K19), the
    optimistic PSRL agent's solver on its compact route: T_ext is never built, R_ext[s, j] = R[s, j % A] is computed.  The
    arguments and the returns are `discounted_value_iteration_dense_batch`'s, with Q [S, A * psi]; the rule counts the
    non-zero elements the expansion would hold.  `status` of the last call is left in
    `discounted_value_iteration_optimistic_batch.status`."""
    if not problems:
        return []
    n = len(problems)
    S = np.array([p["S"] for p in problems], np.int32)
    A = np.array([p["A"] for p in problems], np.int32)
    psi = np.array([p["psi"] for p in problems], np.int32)
    ptr, at = [np.zeros(1, np.int64)], 0
    for p in problems:
        rp = np.asarray(p["row_ptr"], np.int64)
        assert rp.shape == (p["S"] * p["A"] + 1,) and np.shape(p["pmk"]) == (p["psi"], int(rp[-1]))
        assert np.shape(p["bump"]) == (p["psi"], p["S"] * p["A"]) and np.shape(p["z"]) == (p["psi"],)
        ptr.append(rp[1:] + at)
        at += int(rp[-1])
    cat = lambda key, dt: np.ascontiguousarray(np.concatenate([np.asarray(p[key], dt).ravel() for p in problems]), dt)  # noqa: E731
    ptr = np.concatenate(ptr)
    col, simple, z = cat("col", np.int32), cat("simple", np.uint8), cat("z", np.int32)
    pmk, bump, pidx, post, R = cat("pmk", np.float32), cat("bump", np.float32), cat("pidx", np.int32), cat("post", np.float32), cat("R", np.float32)
    Q, V = np.zeros(int((S * A * psi).sum()), np.float32), np.zeros(int(S.sum()), np.float32)
    sweeps, used, status = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
    L.check(L.load().cmdp_vi_discounted_optimistic(n, L.ptr(S), L.ptr(A), L.ptr(psi), L.ptr(ptr), L.ptr(col), L.ptr(simple), L.ptr(z),
                                                   L.ptr(pmk), L.ptr(bump), L.ptr(pidx), L.ptr(post) if len(post) else None, L.ptr(R),
                                                   float(gamma), float(epsilon), L.SCHEME_AUTO if scheme is None else int(scheme),
                                                   int(sparse_n_states_threshold), float(sparse_nnz_per_threshold), int(max_sweeps),
                                                   L.ptr(Q), L.ptr(V), L.ptr(sweeps), L.ptr(used), L.ptr(status)))
    discounted_value_iteration_optimistic_batch.status = status
    out, q0, v0 = [], 0, 0
    for b, (s, ax) in enumerate(zip(S.tolist(), (A * psi).tolist())):
        out.append((Q[q0:q0 + s * ax].reshape(s, ax), V[v0:v0 + s], int(sweeps[b]), int(used[b])))
        q0, v0 = q0 + s * ax, v0 + s
    return out


def map_layout_from_dense(transition_hp, prior, keep=None):
    """Table form of dense M_DIR hyper-parameters [S, A, S] over `prior`: the positions that differ from the prior, plus
    those `keep` (bool [S, A, S]) names, per row in ascending column order -> (row_ptr [S * A + 1], col, hp)."""
    thp = np.ascontiguousarray(transition_hp, np.float32)
    S, A, S2 = thp.shape
    assert S == S2, thp.shape
    m = thp != np.float32(prior)
    if keep is not None:
        m = m | np.asarray(keep, bool).reshape(thp.shape)
    m = m.reshape(S * A, S)
    rows, cols = np.nonzero(m)
    row_ptr = np.concatenate([[0], np.cumsum(m.sum(-1))]).astype(np.int64)
    return row_ptr, cols.astype(np.int32), thp.reshape(S * A, S)[rows, cols]


def map_layout_to_dense(row_ptr, col, hp, prior, S, A):
    """The dense [S, A, S] float32 hyper-parameters of a table form."""
    row_ptr = np.asarray(row_ptr, np.int64)
    M = np.full((S * A, S), prior, np.float32)
    M[np.repeat(np.arange(S * A), np.diff(row_ptr)), np.asarray(col, np.int64)] = np.asarray(hp, np.float32)
    return M.reshape(S, A, S)


def psrl_map_rows(row_ptr, col, hp, prior, S, A):
    """M_DIR.get_map_estimate of one instance in table form, on the host (cmdp_psrl_map_rows; no device needed):
    (rowsum [S, A], c [S, A], t per layout position) float32 -- numpy's pairwise float32 row sums of the dense array, the
    MAP value of every element outside the layout and of the layout's elements."""
    row_ptr = np.ascontiguousarray(row_ptr, np.int64)
    col, hp = np.ascontiguousarray(col, np.int32), np.ascontiguousarray(hp, np.float32)
    S, A = int(S), int(A)
    if S < 1 or A < 1 or row_ptr.shape != (S * A + 1,) or col.shape != hp.shape or len(col) < int(row_ptr[-1]) or row_ptr[0] < 0:
        raise ValueError("row_ptr must have S * A + 1 entries that index col and hp, S and A must be >= 1")
    rowsum, c, t = np.zeros(S * A, np.float32), np.zeros(S * A, np.float32), np.zeros(len(hp), np.float32)
    L.check(L.load().cmdp_psrl_map_rows(S, A, L.ptr(row_ptr), L.ptr(col), L.ptr(hp), float(prior), L.ptr(rowsum), L.ptr(c), L.ptr(t)))
    return rowsum.reshape(S, A), c.reshape(S, A), t


def _map_problem(p):
    if len(p) == 5:
        row_ptr, col, hp, prior, mu = p
        mu = np.ascontiguousarray(mu, np.float32)
        if mu.ndim != 2:
            raise ValueError("mu must be [S, A]")
        row_ptr = np.ascontiguousarray(row_ptr, np.int64)
        col, hp = np.ascontiguousarray(col, np.int32), np.ascontiguousarray(hp, np.float32)
        if row_ptr.shape != (mu.size + 1,) or row_ptr[0] != 0 or col.shape != (int(row_ptr[-1]),) or hp.shape != col.shape:
            raise ValueError("table form: row_ptr [S * A + 1] from 0, col and hp with row_ptr[-1] entries")
    elif len(p) in (3, 4):
        thp, mu, prior = p[:3]
        mu = np.ascontiguousarray(mu, np.float32)
        if np.ndim(thp) != 3 or mu.shape != np.shape(thp)[:2] or np.shape(thp)[0] != np.shape(thp)[2]:
            raise ValueError("dense form: transition_hp [S, A, S], reward_mu [S, A], prior")
        row_ptr, col, hp = map_layout_from_dense(thp, prior, p[3] if len(p) == 4 else None)
    else:
        raise ValueError("a problem is (row_ptr, col, hp, prior, mu) or (transition_hp, reward_mu, prior[, keep])")
    return row_ptr, col, hp, np.float32(prior), mu


def episodic_value_iteration_map_batch(problems, H, return_map=False):
    """`episodic_value_iteration(H, *get_map_estimate())` for many Bayesian models in one launch of kernel K15, without
    the dense MAP array.  A problem is the table form (row_ptr, col, hp, prior, mu [S, A]) -- per row the ascending columns
    `col` where the M_DIR hyper-parameters are `hp`, `prior` everywhere else -- or the dense form (transition_hp
    [S, A, S], reward_mu [S, A], prior[, keep]), packed by `map_layout_from_dense`.  The problems may differ in S and A.
    Returns [(Q [H + 1, S, A], V [H + 1, S])]; with `return_map` [(Q, V, t, c)]: the MAP transition estimate at the
    layout's positions and, per row [S, A], elsewhere."""
    ps = [_map_problem(p) for p in problems]
    H = int(H)
    if H < 1:
        raise ValueError("H < 1")
    if not ps:
        return []
    S = np.array([p[4].shape[0] for p in ps], np.int32)
    A = np.array([p[4].shape[1] for p in ps], np.int32)
    nz = np.array([len(p[1]) for p in ps], np.int64)
    nz_off = np.concatenate([[0], np.cumsum(nz)])
    ptr = np.concatenate([p[0][:-1] + nz_off[i] for i, p in enumerate(ps)] + [nz_off[-1:]]).astype(np.int64)
    col = np.concatenate([p[1] for p in ps]).astype(np.int32)
    hp = np.concatenate([p[2] for p in ps]).astype(np.float32)
    prior = np.array([p[3] for p in ps], np.float32)
    mu = np.concatenate([p[4].ravel() for p in ps]).astype(np.float32)
    Q = np.zeros((H + 1) * int((S.astype(np.int64) * A).sum()), np.float32)
    V = np.zeros((H + 1) * int(S.sum()), np.float32)
    t, c = np.zeros(len(hp), np.float32), np.zeros(len(mu), np.float32)
    L.check(L.load().cmdp_vi_episodic_map(len(ps), L.ptr(S), L.ptr(A), H, L.ptr(ptr), L.ptr(col), L.ptr(hp), L.ptr(prior),
                                          L.ptr(mu), L.ptr(Q), L.ptr(V), L.ptr(t) if return_map else None,
                                          L.ptr(c) if return_map else None))
    out, q0, v0, r0 = [], 0, 0, 0
    for i, (s, a) in enumerate(zip(S.tolist(), A.tolist())):
        nq, nv = (H + 1) * s * a, (H + 1) * s
        one = (Q[q0:q0 + nq].reshape(H + 1, s, a), V[v0:v0 + nv].reshape(H + 1, s))
        if return_map:
            one += (t[nz_off[i]:nz_off[i + 1]], c[r0:r0 + s * a].reshape(s, a))
        out.append(one)
        q0, v0, r0 = q0 + nq, v0 + nv, r0 + s * a
    return out


def discounted_value_iteration_map_batch(problems, gamma=0.99, epsilon=1e-3, sparse_n_states_threshold=300 * 3 * 300,
                                         sparse_nnz_per_threshold=0.2, scheme=None, max_sweeps=DP_MAX_ITERATION, return_map=False):
    """`discounted_value_iteration(*get_map_estimate())` for many Bayesian models in one launch of kernel K17, without the
    dense MAP array.  A problem is the table form (row_ptr, col, hp, prior, mu [S, A]) or the dense form (transition_hp
    [S, A, S], reward_mu [S, A], prior[, keep]), as for `episodic_value_iteration_map_batch`; the problems may differ in S
    and A.  The solver's arguments are `discounted_value_iteration_dense_batch`'s: the reference's rule picks Jacobi or
    Gauss-Seidel per problem from the count of non-zero elements of its dense MAP array unless `scheme` forces one, and a
    problem that takes `max_sweeps` sweeps returns the last sweep's values.  Returns [(Q [S, A], V [S], sweeps, scheme)];
    with `return_map` [(Q, V, sweeps, scheme, t, c)]: the MAP transition estimate at the layout's positions and, per row
    [S, A], elsewhere.  `status` of the last call (0 or L.ERR_MAX_ITER per problem) is left in
    `discounted_value_iteration_map_batch.status`."""
    ps = [_map_problem(p) for p in problems]
    gamma, epsilon = float(gamma), float(epsilon)
    if not np.isfinite(gamma):
        raise ValueError("gamma must be finite")
    if not (np.isfinite(epsilon) and epsilon >= 0.0):
        raise ValueError("epsilon must be a finite value >= 0")
    if int(max_sweeps) < 1:
        raise ValueError("max_sweeps < 1")
    if scheme is not None and int(scheme) not in (L.SCHEME_JACOBI, L.SCHEME_GAUSS_SEIDEL):
        raise ValueError("scheme is None, L.SCHEME_JACOBI or L.SCHEME_GAUSS_SEIDEL")
    if int(sparse_n_states_threshold) < 0 or np.isnan(float(sparse_nnz_per_threshold)):
        raise ValueError("sparse_n_states_threshold must be >= 0 and sparse_nnz_per_threshold a number")
    if not ps:
        return []
    S = np.array([p[4].shape[0] for p in ps], np.int32)
    A = np.array([p[4].shape[1] for p in ps], np.int32)
    n = len(ps)
    nz = np.array([len(p[1]) for p in ps], np.int64)
    nz_off = np.concatenate([[0], np.cumsum(nz)])
    ptr = np.concatenate([p[0][:-1] + nz_off[i] for i, p in enumerate(ps)] + [nz_off[-1:]]).astype(np.int64)
    col = np.concatenate([p[1] for p in ps]).astype(np.int32)
    hp = np.concatenate([p[2] for p in ps]).astype(np.float32)
    prior = np.array([p[3] for p in ps], np.float32)
    mu = np.concatenate([p[4].ravel() for p in ps]).astype(np.float32)
    Q, V = np.zeros(int((S.astype(np.int64) * A).sum()), np.float32), np.zeros(int(S.sum()), np.float32)
    sweeps, used, status = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int32)
    t, c = np.zeros(len(hp), np.float32), np.zeros(len(mu), np.float32)
    L.check(L.load().cmdp_vi_discounted_map(n, L.ptr(S), L.ptr(A), L.ptr(ptr), L.ptr(col), L.ptr(hp), L.ptr(prior), L.ptr(mu),
                                            gamma, epsilon, L.SCHEME_AUTO if scheme is None else int(scheme),
                                            int(sparse_n_states_threshold), float(sparse_nnz_per_threshold), int(max_sweeps),
                                            L.ptr(Q), L.ptr(V), L.ptr(sweeps), L.ptr(used), L.ptr(status),
                                            L.ptr(t) if return_map else None, L.ptr(c) if return_map else None))
    discounted_value_iteration_map_batch.status = status
    out, q0, v0 = [], 0, 0
    for i, (s, a) in enumerate(zip(S.tolist(), A.tolist())):
        one = (Q[q0:q0 + s * a].reshape(s, a), V[v0:v0 + s], int(sweeps[i]), int(used[i]))
        if return_map:
            one += (t[nz_off[i]:nz_off[i + 1]], c[q0:q0 + s * a].reshape(s, a))
        out.append(one)
        q0, v0 = q0 + s * a, v0 + s
    return out


def episodic_policy_evaluation(H, T, R, policy):
    """reference finite_horizon.py:29-42; policy [H,S,A]."""
    S, A, _ = T.shape
    Q, V = _handle(T, R).episodic_policy_evaluation(np.asarray(policy, np.float32).ravel(), int(H))
    return Q.reshape(H + 1, S, A), V.reshape(H + 1, S)


def discounted_policy_iteration(T, R, gamma=0.99, epsilon=1e-7):
    """reference infinite_horizon.py:208-219 (the initial Q is drawn from the unseeded global numpy RNG
    there too)."""
    S, A, _ = T.shape
    Q = np.random.rand(S, A)
    pi = argmax_2d(Q)
    for _ in range(DP_MAX_ITERATION):
        old_pi = pi.copy()
        Q, V = discounted_policy_evaluation(T, R, pi, gamma, epsilon)
        pi = argmax_2d(Q)
        if (pi != old_pi).sum() == 0:
            return Q, V, pi
    raise DynamicProgrammingMaxIterationExceeded()


# ---- the row form of kernels K10 and K14: CSR rows, or one value for a row that holds it at every state -------------
def _row_form(T):
    """Dense T [S, A, S] -> (S, A, ptr, col, val, uniform): `uniform[r]` = c > 0 for a row that is c at every state (such a
    row has no CSR entries), the other rows as CSR with ascending columns and no explicit zeros."""
    T = np.asarray(T)
    if T.ndim != 3 or T.shape[0] != T.shape[2] or T.shape[0] < 1 or T.shape[1] < 1:
        raise ValueError(f"T must be [S, A, S] with S, A >= 1, got shape {T.shape}")
    S, A, _ = T.shape
    T = np.ascontiguousarray(T, np.float32)
    if not np.isfinite(T).all() or (T < 0).any():
        raise ValueError("T must hold finite probabilities >= 0")
    T2 = T.reshape(S * A, S)
    uniform = np.where((T2[:, 0] > 0) & (T2 == T2[:, :1]).all(axis=1), T2[:, 0], np.float32(0)).astype(np.float32)
    rows, cols = np.nonzero(T2 * (uniform == 0)[:, None])
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=S * A))]).astype(np.int64)
    return S, A, ptr, cols.astype(np.int32), T2[rows, cols], uniform


def _pack_rows(P):
    """Row forms `(S, A, ptr, col, val, uniform, ...)` of a batch -> the concatenated (S, A, ptr, col, val, uniform) of the
    C ABI, the row pointers shifted by the entries of the instances before."""
    S = np.array([p[0] for p in P], np.int32)
    A = np.array([p[1] for p in P], np.int32)
    nz_off = np.concatenate([[0], np.cumsum([len(p[3]) for p in P])])
    ptr = np.concatenate([[0]] + [p[2][1:] + nz_off[b] for b, p in enumerate(P)]).astype(np.int64)
    cat = lambda i, dt: np.ascontiguousarray(np.concatenate([p[i] for p in P]), dt)  # noqa: E731
    return S, A, ptr, cat(3, np.int32), cat(4, np.float32), cat(5, np.float32)


def _split_rows(B, S, A, status, Q, V):
    """[(Q [S, A], V [S]) or None where status is not OK] per instance of a packed batch."""
    out, q0, v0 = [], 0, 0
    for b in range(B):
        s, a = int(S[b]), int(A[b])
        out.append((Q[q0:q0 + s * a].reshape(s, a).copy(), V[v0:v0 + s].copy()) if status[b] == L.OK else None)
        q0 += s * a
        v0 += s
    return out


# ---- discounted value iteration on the row form (reference infinite_horizon.py:14-44), kernel K14 -------------------
def _vi_problem(T, R):
    """One (T, R) pair -> (S, A, ptr, col, val, uniform, R, nnz) in the C ABI's types; nnz as `sparse.COO(T).nnz`."""
    S, A, ptr, col, val, uniform = _row_form(T)
    R = np.ascontiguousarray(R, np.float32)
    if R.shape != (S, A):
        raise ValueError(f"R must be [S, A] = {(S, A)}, got {R.shape}")
    return S, A, ptr, col, val, uniform, R.ravel(), int(len(col) + S * np.count_nonzero(uniform))


def discounted_value_iteration_batch(problems, gamma=0.99, epsilon=1e-3, sparse_n_states_threshold=300 * 3 * 300,
                                     sparse_nnz_per_threshold=0.2, scheme=None, max_sweeps=DP_MAX_ITERATION):
    """`discounted_value_iteration` for many dense (T, R) problems in one launch (kernel K14); the problems may differ in S
    and A.  Rows that hold one value at every state (an estimated model's unvisited pairs) cost one shared chain of
    additions instead of one each.  scheme None: the reference's rule per problem, else L.SCHEME_JACOBI /
    L.SCHEME_GAUSS_SEIDEL for all.  Returns ([(Q, V) or None per problem], sweeps [B] int64, schemes [B] int32): None where a
    problem did not converge within max_sweeps, which leaves the others unaffected.  Q, V and sweeps are bit for bit those
    of `discounted_value_iteration` on each problem."""
    eps = float(epsilon)
    if not np.isfinite(eps) or eps < 0:
        raise ValueError(f"epsilon must be finite and >= 0, got {epsilon}")
    if int(max_sweeps) < 1:
        raise ValueError(f"max_sweeps must be >= 1, got {max_sweeps}")
    if scheme not in (None, L.SCHEME_AUTO, L.SCHEME_JACOBI, L.SCHEME_GAUSS_SEIDEL):
        raise ValueError(f"scheme must be None, SCHEME_JACOBI or SCHEME_GAUSS_SEIDEL, got {scheme}")
    P = [_vi_problem(*p) for p in problems]
    B = len(P)
    if B == 0:
        return [], np.zeros(0, np.int64), np.zeros(0, np.int32)
    S, A, ptr, col, val, uni = _pack_rows(P)
    R = np.ascontiguousarray(np.concatenate([p[6] for p in P]), np.float32)
    Q = np.empty(int((S.astype(np.int64) * A).sum()), np.float32)
    V = np.empty(int(S.sum()), np.float32)
    sweeps, schemes, status = np.empty(B, np.int64), np.empty(B, np.int32), np.empty(B, np.int32)
    L.check(L.load().cmdp_vi_discounted_model(B, L.ptr(S), L.ptr(A), L.ptr(ptr), L.ptr(col), L.ptr(val), L.ptr(uni), L.ptr(R),
                                              float(gamma), eps, int(scheme or L.SCHEME_AUTO), int(sparse_n_states_threshold),
                                              float(sparse_nnz_per_threshold), int(max_sweeps), L.ptr(Q), L.ptr(V),
                                              L.ptr(sweeps), L.ptr(schemes), L.ptr(status)))
    return _split_rows(B, S, A, status, Q, V), sweeps, schemes


# ---- extended value iteration (reference infinite_horizon.py:67-118, _max_proba :222-251), kernel K10 --------------
def _evi_problem(T, estimated_rewards, beta_r, beta_p, r_max):
    """One (T, estimated_rewards, beta_r, beta_p, r_max) 5-tuple -> (S, A, ptr, col, val, uniform, R, beta_r, beta_p0,
    r_max) in the C ABI's types.  beta_p is [S, A, 1] (Chernoff) or [S, A, S] (Bernstein); only element 0 of each row
    is read, as in the reference."""
    S, A, ptr, col, val, uniform = _row_form(T)
    R = np.ascontiguousarray(estimated_rewards, np.float32)
    br = np.ascontiguousarray(beta_r, np.float64)  # float32 bounds are widened: the one precision difference
    bp = np.asarray(beta_p, np.float64)
    if R.shape != (S, A):
        raise ValueError(f"estimated_rewards must be [S, A] = {(S, A)}, got {R.shape}")
    if br.shape != (S, A):
        raise ValueError(f"beta_r must be [S, A] = {(S, A)}, got {br.shape}")
    if bp.ndim != 3 or bp.shape[:2] != (S, A) or bp.shape[2] not in (1, S):
        raise ValueError(f"beta_p must be [S, A, 1] or [S, A, S] with S, A = {(S, A)}, got {bp.shape}")
    return (S, A, ptr, col, val, uniform, R.ravel(), br.ravel(), np.ascontiguousarray(bp[:, :, 0], np.float64).ravel(),
            float(r_max))


def _evi_run(problems, epsilon, max_sweeps):
    """Packs the problems into one cmdp_extended_vi call: [(span, Q, V) or None], sweeps [B] int64."""
    eps = float(epsilon)
    if not np.isfinite(eps) or eps < 0:
        raise ValueError(f"epsilon must be finite and >= 0, got {epsilon}")
    if int(max_sweeps) < 1:
        raise ValueError(f"max_sweeps must be >= 1, got {max_sweeps}")
    P = [_evi_problem(*p) for p in problems]
    B = len(P)
    if B == 0:
        return [], np.zeros(0, np.int64)
    S, A, ptr, col, val, uni = _pack_rows(P)
    cat = lambda i, dt: np.ascontiguousarray(np.concatenate([p[i] for p in P]), dt)  # noqa: E731
    R, br, bp0 = cat(6, np.float32), cat(7, np.float64), cat(8, np.float64)
    rmax = np.array([p[9] for p in P], np.float64)
    rows = (S.astype(np.int64) * A).sum()
    Q = np.empty(rows, np.float32)
    V = np.empty(int(S.sum()), np.float32)
    span = np.empty(B, np.float64)
    sweeps = np.empty(B, np.int64)
    status = np.empty(B, np.int32)
    L.check(L.load().cmdp_extended_vi(B, L.ptr(S), L.ptr(A), L.ptr(ptr), L.ptr(col), L.ptr(val), L.ptr(uni), L.ptr(R),
                                      L.ptr(br), L.ptr(bp0), L.ptr(rmax), eps, int(max_sweeps), L.ptr(Q), L.ptr(V),
                                      L.ptr(span), L.ptr(sweeps), L.ptr(status)))
    out, q0, v0 = [], 0, 0
    for b in range(B):
        s, a = int(S[b]), int(A[b])
        if status[b] == L.OK:
            out.append((np.float32(span[b]), Q[q0:q0 + s * a].reshape(s, a).copy(), V[v0:v0 + s].copy()))
        else:
            out.append(None)
        q0 += s * a
        v0 += s
    return out, sweeps


def extended_value_iteration(T, estimated_rewards, beta_r, beta_p, r_max, epsilon=1e-3):
    """reference infinite_horizon.py:67-118 (UCRL2's optimistic solver).  Returns (span, Q [S,A] float32, V [S]
    float32), span the float32 ptp of the value vector the last sweep read, or None after DP_MAX_ITERATION sweeps.
    beta_p is [S,A,1] or [S,A,S]; only element 0 of each row is read, as in the reference.  The reference's agent
    passes float64 bounds; float32 bounds are widened to float64 here (the one precision difference to a call with
    float32 bounds there).  Ties in the value vector are ordered by ascending state index."""
    return _evi_run([(T, estimated_rewards, beta_r, beta_p, r_max)], epsilon, DP_MAX_ITERATION)[0][0]


def extended_value_iteration_batch(problems, epsilon=1e-3, max_sweeps=DP_MAX_ITERATION):
    """`extended_value_iteration` for many (T, estimated_rewards, beta_r, beta_p, r_max) problems in one launch; the
    problems may differ in S and A.  Returns ([(span, Q, V) or None per problem], sweeps [B] int64): None where a
    problem did not converge within max_sweeps, which leaves the others unaffected."""
    return _evi_run(list(problems), epsilon, max_sweeps)


# ---- argmax with uniform random tie-break (reference dynamic_programming/utils.py:12-100) ----------------
# The reference re-seeds *numba's* generator with 42 on every call; without numba the tie winner cannot be
# reproduced (SURVEY 8c caveat 1).  Tie-free rows are exact; ties are broken by RandomState(42).choice,
# which is what the reference computes when its njit decorators are the identity.
def _pick(rs, row):
    return rs.choice(np.where(row == row.max())[0])


def _pick_rows(M):
    """`_pick` for every row of M [n, A], in row order, from ONE RandomState(ARGMAX_SEED): rows with a single maximum are
    taken in one vectorised pass -- `RandomState.choice` on one candidate draws nothing, so the stream is consumed by the
    tie rows only, in their order, exactly as the row-by-row loop does."""
    M = np.asarray(M)
    n = len(M)
    if n == 0:
        return np.zeros(0, np.int64)
    is_max = M == M.max(axis=1, keepdims=True)
    picks = is_max.argmax(axis=1)
    ties = np.flatnonzero(is_max.sum(axis=1) != 1)   # also rows of NaNs (no element equals the maximum): left to `_pick`
    if len(ties):
        rs = np.random.RandomState(ARGMAX_SEED)
        for s in ties.tolist():
            picks[s] = _pick(rs, M[s])
    return picks


def argmax_2d(A):
    X = np.zeros_like(A, np.float32)
    X[np.arange(len(A)), _pick_rows(A)] = 1
    return X


def argmax_3d(A):
    H, S = A.shape[:2]
    X = np.zeros(A.shape, np.float32)
    X.reshape(H * S, -1)[np.arange(H * S), _pick_rows(A.reshape(H * S, -1))] = 1.0
    return X


def get_deterministic_policy_from_q_values(Q):
    return _pick_rows(Q).astype(np.int32)


def get_deterministic_policy_from_q_values_finite_horizon(Q):
    H, S = Q.shape[:2]
    return _pick_rows(Q.reshape(H * S, -1)).astype(np.int32).reshape(H, S)


def get_policy_from_q_values(Q, stochastic_form=False):
    if Q.ndim == 3:
        return argmax_3d(Q) if stochastic_form else get_deterministic_policy_from_q_values_finite_horizon(Q)
    return argmax_2d(Q) if stochastic_form else get_deterministic_policy_from_q_values(Q)
