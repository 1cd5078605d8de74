"""Test helper: the NumPy definition of the COMPACT optimistic sample and of its solve (kernel K19,
csrc/cmdp_psrlo_vi.h), written here independently of the package's own host helpers:

  * the compact form of a PSRLOTwin sample over a layout of the real rows, and its expansion -- zeros, then the layout's
    values, then z_k -- which must give the twin's T_ext back bit for bit;
  * the count of non-zero elements the expansion would hold, from the compact form alone;
  * a simple row's terms in the order the kernel adds them (ascending column, z_k merged in, the bump standing once where z_k
    is a layout column) and the float64 sum in that order;
  * a float64 solver on the compact form, n sweeps without a stopping rule, the counterpart of helpers_psrlc.vi_discounted_f64.

The rounding bound.  helpers_psrlc.bound_discounted allows, per sweep and row, e = (4 U + S 2^-52) M: what the float32
roundings of the wrap-up cost (the same on both routes: fl32(gamma t) per term and float(R + acc) under Gauss-Seidel,
float(acc), gamma * tv and R + . under Jacobi, plus the stopping rule's subtraction) and S 2^-53 of sum |term| for the float64
accumulation of at most S exact products IN ANY ORDER.  A posterior row's sum is the dense kernel's, term for term.  A simple
row's sum adds len + 1 <= S exact products one at a time, which that second part covers with room to spare; its float32
roundings are the dense definition's.  The recursion over the sweeps only uses that the row map contracts by gamma, which
holds for the expansion as for any sampled T.  So the bound carries over unchanged: `bound_compact` is `bound_discounted`."""
import numpy as np

from helpers_psrlc import JACOBI, bound_discounted

bound_compact = bound_discounted


def layout_from_support(T_true):
    """(row_ptr [S * A + 1], col) of the positions with T_true [S, A, S] != 0, per real row in ascending column order."""
    S, A, _ = T_true.shape
    m = np.asarray(T_true).reshape(S * A, S) != 0
    rows, cols = np.nonzero(m)
    return np.concatenate([[0], np.cumsum(m.sum(-1))]).astype(np.int64), cols.astype(np.int32)


def compact_of(T_ext, psi, simple, z, row_ptr, col, R):
    """The compact form of a sample: `simple` [S, A] bool and `z` (psi values, or none / -1 when no row is simple) as the
    sampler gave them.  Returns the dict the package's stand-alone call takes."""
    T = np.asarray(T_ext)
    assert T.dtype == np.float32
    S, AX, _ = T.shape
    A = AX // psi
    rows = S * A
    simple = np.asarray(simple, bool).reshape(rows)
    z = np.asarray(z, np.int64).reshape(-1)
    if not simple.any():
        z = np.zeros(psi, np.int64)
    assert len(z) == psi and (z >= 0).all() and (z < S).all()
    nz = int(row_ptr[-1])
    pmk, bump = np.zeros((psi, nz), np.float32), np.zeros((psi, rows), np.float32)
    pidx, post, n1 = np.full(rows, -1, np.int32), [], 0
    for row in range(rows):
        s, a = divmod(row, A)
        ext = T[s, a * psi:(a + 1) * psi]             # the psi extended rows of the real row, [psi, S]
        if simple[row]:
            cs = col[row_ptr[row]:row_ptr[row + 1]]
            for k in range(psi):
                seen = np.zeros(S, bool)
                seen[cs] = True
                seen[z[k]] = True
                assert not ext[k][~seen].any(), (row, k, "a simple row is non-zero outside its layout and z_k")
                pmk[k, row_ptr[row]:row_ptr[row + 1]] = ext[k][cs]
                bump[k, row] = ext[k][z[k]]
        else:
            pidx[row] = n1
            n1 += 1
            post.append(ext)
    post = np.stack(post, 1) if post else np.zeros((psi, 0, S), np.float32)   # [psi, n1, S]
    return dict(S=S, A=A, psi=psi, row_ptr=np.asarray(row_ptr, np.int64), col=np.asarray(col, np.int32), simple=simple,
                z=z.astype(np.int32), pmk=pmk, bump=bump, pidx=pidx, post=np.ascontiguousarray(post, np.float32),
                R=np.ascontiguousarray(R, np.float32).reshape(S, A))


def compact_of_twin(tw, row_ptr, col):
    return compact_of(tw.last_T, tw.psi, tw.last_simple, tw.last_z if tw.last_n[1] else [], row_ptr, col, tw.last_R)


def expand(c):
    """T_ext [S, A * psi, S] float32 by Phase 2's rule."""
    S, A, psi = c["S"], c["A"], c["psi"]
    T = np.zeros((S, A * psi, S), np.float32)
    for row in range(S * A):
        s, a = divmod(row, A)
        for k in range(psi):
            out = T[s, a * psi + k]
            if c["simple"][row]:
                e0, e1 = c["row_ptr"][row], c["row_ptr"][row + 1]
                out[c["col"][e0:e1]] = c["pmk"][k, e0:e1]
                out[c["z"][k]] = c["bump"][k, row]
            else:
                out[:] = c["post"][k, c["pidx"][row]]
    return T


def nonzero_count(c):
    """(T_ext != 0).sum() of the expansion from the compact form: a z_k inside the layout counts once, as the bump."""
    S, A, psi = c["S"], c["A"], c["psi"]
    n = int((c["post"] != 0).sum())
    for row in np.flatnonzero(c["simple"]):
        e0, e1 = c["row_ptr"][row], c["row_ptr"][row + 1]
        cs = c["col"][e0:e1]
        for k in range(psi):
            n += int(c["bump"][k, row] != 0) + int(((c["pmk"][k, e0:e1] != 0) & (cs != c["z"][k])).sum())
    return n


def simple_row_terms(c, row, k):
    """(columns ascending, float32 values) of sample k of the simple real row `row`, as the kernel walks them."""
    e0, e1 = c["row_ptr"][row], c["row_ptr"][row + 1]
    cs, vs = c["col"][e0:e1].tolist(), c["pmk"][k, e0:e1].tolist()
    zk, b = int(c["z"][k]), float(c["bump"][k, row])
    if zk in cs:
        vs[cs.index(zk)] = b
    else:
        i = int(np.searchsorted(cs, zk))
        cs.insert(i, zk)
        vs.insert(i, b)
    return np.array(cs, np.int64), np.array(vs, np.float32)


def simple_row_sum(c, row, k, V, gamma32=None):
    """The sum in the stated order: one term at a time in float64 to +0; with `gamma32` the terms are
    double(fl32(gamma * t)) * double(V[c]) (Gauss-Seidel), without it double(t) * double(V[c]) (Jacobi)."""
    cs, vs = simple_row_terms(c, row, k)
    if gamma32 is not None:
        vs = np.float32(gamma32) * vs
        assert vs.dtype == np.float32
    acc = 0.0
    for cc, v in zip(cs.tolist(), vs.astype(np.float64).tolist()):
        acc += v * float(V[cc])
    return acc


def _padded(c):
    """Every extended row as (columns, float64 values) padded to one length, ascending: [S, A * psi, Lmax] twice."""
    S, A, psi = c["S"], c["A"], c["psi"]
    rows = []
    for row in range(S * A):
        for k in range(psi):
            if c["simple"][row]:
                rows.append(simple_row_terms(c, row, k))
            else:
                rows.append((np.arange(S), c["post"][k, c["pidx"][row]]))
    lmax = max(len(r[0]) for r in rows)
    cols, vals = np.zeros((len(rows), lmax), np.int64), np.zeros((len(rows), lmax))
    for i, (cs, vs) in enumerate(rows):
        cols[i, :len(cs)], vals[i, :len(cs)] = cs, vs
    return cols.reshape(S, A * psi, lmax), vals.reshape(S, A * psi, lmax)


def r_ext(c):
    """R_ext[s, j] = R[s, j % A] -- np.tile(R, (1, psi))."""
    return np.tile(c["R"], (1, c["psi"]))


def vi_compact_f64(c, gamma, scheme, n):
    """Exactly `n` sweeps of `scheme` from V = 0 in float64 on the compact form, every row sum in the stated order.  Returns
    as helpers_psrlc.vi_discounted_f64: (Q64 [S, A * psi], d_n, d_{n-1}, qmax)."""
    S = c["S"]
    cols, vals = _padded(c)
    R = r_ext(c).astype(np.float64)
    V, Q = np.zeros(S), np.zeros(R.shape)
    d, d_prev, qmax = np.inf, np.inf, 0.0
    gv = gamma * vals
    for _ in range(n):
        V_old = V.copy()
        if scheme == JACOBI:
            acc = np.zeros(R.shape)
            for i in range(cols.shape[-1]):
                acc += vals[..., i] * V_old[cols[..., i]]
            Q = R + gamma * acc
            V = Q.max(-1)
        else:
            for s in range(S):
                acc = np.zeros(R.shape[1])
                for i in range(cols.shape[-1]):
                    acc += gv[s, :, i] * V[cols[s, :, i]]
                Q[s] = R[s] + acc
                V[s] = Q[s].max()
        d_prev, d = d, float(np.abs(V_old - V).max())
        qmax = max(qmax, float(np.abs(Q).max()))
    return Q.copy(), d, d_prev, qmax
