"""Test helper for kernel K14 (cmdp_vi_discounted_model): generated models in the kernel's row form, the call, and the
reference -- `oracle.vi_discounted` on the CSR of the dense model, a uniform row expanded to its S entries in column order
and explicit zeros dropped (what `csr_from_dense` of the dense model holds)."""
import numpy as np

from colosseum_amd import _lib as L
from oracle import oracle as O

STATES = (1, 2, 63, 64, 65, 257)
ACTIONS = (1, 2, 5, 64)
MIXES = ("all_uniform", "no_uniform", "state_0", "state_last", "every_other_state", "one_action", "explicit_zeros",
         "full_csr_row", "two_c")
GAMMAS = (0.99, 0.5, 0.0)
EPS = 1e-3
SIZE_THRESHOLD, DENSITY_THRESHOLD = 300 * 3 * 300, 0.2


class Fixture:
    """One model: the row form the kernel is given (`ptr`, `col`, `val`, `uni`, `R`) and `csr`, the CSR of its dense form."""

    def __init__(self, S, A, uni, ptr, col, val, R, name=""):
        self.S, self.A, self.name = S, A, name
        self.R = np.ascontiguousarray(R, np.float32).reshape(S * A)
        self.uni, self.ptr = np.ascontiguousarray(uni, np.float32), np.ascontiguousarray(ptr, np.int64)
        self.col, self.val = np.ascontiguousarray(col, np.int32), np.ascontiguousarray(val, np.float32)
        assert len(self.uni) == S * A == len(self.ptr) - 1 and len(self.col) == len(self.val) == self.ptr[-1]
        T = np.zeros((S * A, S), np.float32)
        T[np.repeat(np.arange(S * A), np.diff(self.ptr)), self.col] = self.val
        T[self.uni > 0] = self.uni[self.uni > 0, None]
        rows, cols = np.nonzero(T)   # row by row, columns ascending
        dptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=S * A))]).astype(np.int64)
        self.csr = (dptr, cols.astype(np.int32), T[rows, cols])
        self.nnz = int(dptr[-1])   # sparse.COO(T).nnz of the dense model
        self._ref = {}

    @classmethod
    def from_rows(cls, S, A, rows, R, name=""):
        """rows: per row either a float32 c (uniform) or (cols, vals) with ascending columns."""
        ptr, col, val, uni = [0], [np.zeros(0, np.int32)], [np.zeros(0, np.float32)], []
        for r in rows:
            if isinstance(r, tuple):
                col.append(np.asarray(r[0], np.int32)); val.append(np.asarray(r[1], np.float32)); uni.append(0.0)
                ptr.append(ptr[-1] + len(r[0]))
            else:
                uni.append(r)
                ptr.append(ptr[-1])
        return cls(S, A, uni, ptr, np.concatenate(col), np.concatenate(val), R, name)

    def dense(self):
        T = np.zeros((self.S * self.A, self.S), np.float32)
        p, c, v = self.csr
        T[np.repeat(np.arange(self.S * self.A), np.diff(p)), c] = v
        return T.reshape(self.S, self.A, self.S), self.R.reshape(self.S, self.A)

    def rule(self, size_threshold=SIZE_THRESHOLD, density_threshold=DENSITY_THRESHOLD):
        """reference infinite_horizon.py:28-36 in Python's own arithmetic."""
        size = self.S * self.A * self.S
        return L.SCHEME_JACOBI if size > size_threshold and self.nnz / size < density_threshold else L.SCHEME_GAUSS_SEIDEL

    def reference(self, gamma, scheme, eps=EPS, max_sweeps=1_000_000):
        """(Q [S * A], V [S], sweeps or -5) of the oracle; computed once per (gamma, scheme, eps, max_sweeps)."""
        key = (float(gamma), int(scheme), float(eps), int(max_sweeps))
        if key not in self._ref:
            Q, V, it, _ = O.vi_discounted(self.S, self.A, self.csr, self.R, gamma, eps, scheme, max_sweeps)
            self._ref[key] = (Q.reshape(-1), V, it)
        return self._ref[key]


def sparse_rows(rng, S, n, zeros=False):
    """n CSR rows of 1 .. min(4, S) entries: (counts [n], cols, vals), columns distinct and ascending within a row."""
    kmax = min(4, S)
    k = rng.integers(1, kmax + 1, size=n)
    # distinct columns: a start and steps of 1 .. S // kmax, whose sum stays below S
    steps = rng.integers(1, S // kmax + 1, size=(n, kmax))
    steps[:, 0] = 0
    cols = (rng.integers(0, S, size=(n, 1)) + np.cumsum(steps, axis=1)) % S
    w = rng.random((n, kmax)) + 0.05
    keep = np.arange(kmax)[None, :] < k[:, None]
    w = (w / np.where(keep, w, 0).sum(axis=1, keepdims=True)).astype(np.float32)
    if zeros:
        w[np.arange(n), rng.integers(0, kmax, size=n) % k] = 0.0
    cols = np.where(keep, cols, S)   # dropped entries sort to the end
    order = np.argsort(cols, axis=1, kind="stable")
    cols, w = np.take_along_axis(cols, order, 1), np.take_along_axis(w, order, 1)
    keep = cols < S
    return k, cols[keep].astype(np.int32), w[keep]


def make_fixture(S, A, mix, seed):
    rng = np.random.default_rng(seed)
    c = np.float32(1.0) / np.float32(S)   # np.ones(float32) / n_states, UCRL2's value
    c2 = np.float32(0.5) / np.float32(S + 1)
    s, a = np.divmod(np.arange(S * A), A)
    no, full = np.float32(0), np.float32(-1)   # -1: a full row of c given as CSR
    if mix == "all_uniform":
        u = np.full(S * A, c)
    elif mix == "no_uniform":
        u = np.full(S * A, no)
    elif mix == "state_0":
        u = np.where(s == 0, c, no)
    elif mix == "state_last":
        u = np.where(s == S - 1, c, no)
    elif mix == "every_other_state":
        u = np.where(s % 2 == 0, c, no)
    elif mix == "one_action":
        u = np.where(a == s % A, c, no)
    elif mix == "explicit_zeros":
        u = np.where(s == 1, c, no)
    elif mix == "full_csr_row":
        u = np.where(s % 3 == 0, full, no)
    else:   # two_c: the second value alone in odd states, next to the first in the states divisible by four
        u = np.where(s % 4 == 0, np.where(a == A - 1, c2, c), np.where(s % 2 == 1, c2, no))
    u = u.astype(np.float32)
    sparse = np.flatnonzero(u == 0)
    k, cols, vals = sparse_rows(rng, S, len(sparse), zeros=mix == "explicit_zeros")
    count = np.zeros(S * A, np.int64)
    count[sparse] = k
    count[u < 0] = S
    ptr = np.concatenate([[0], np.cumsum(count)])
    col, val = np.zeros(ptr[-1], np.int32), np.zeros(ptr[-1], np.float32)
    where = np.repeat(u == 0, count)
    col[where], val[where] = cols, vals
    col[~where], val[~where] = np.tile(np.arange(S, dtype=np.int32), int((u < 0).sum())), c
    R = (rng.random((S, A)) * 0.05).astype(np.float32)
    R[R == 0] = np.float32(0.01)
    return Fixture(S, A, np.maximum(u, 0), ptr, col, val, R, f"S{S}_A{A}_{mix}")


_GRID = None


def grid():
    """Every (S, A, mix) once, with the gamma it is solved at: the three gammas in rotation, 0.99 (some 390 sweeps) left to
    the models whose dense form the CPU oracle sweeps quickly."""
    global _GRID
    if _GRID is None:
        _GRID = []
        for i, S in enumerate(STATES):
            for j, A in enumerate(ACTIONS):
                for k, mix in enumerate(MIXES):
                    fx = make_fixture(S, A, mix, 1000 * i + 100 * j + k)
                    gamma = GAMMAS[(i + j + k) % 3]
                    if gamma == 0.99 and fx.nnz > 30_000:
                        gamma = GAMMAS[1 + (i + j + k) % 2]
                    _GRID.append((fx, gamma))
    return _GRID


def edge_batch():
    """One mixed-size batch for AUTO with size_threshold 50 and density_threshold 0.25: (fixture, the scheme meant for it)
    on both sides of the size edge (S * A * S = 50 is not above it, 72 is) and of the density edge (18 / 72 = 0.25 exactly is
    not below it, 17 / 72 is)."""
    rng = np.random.default_rng(77)

    def model(S, A, nnz, n_uniform):
        per = np.full(S * A, 1)
        per[:n_uniform] = S
        left = nnz - int(per.sum())
        assert left >= 0
        for r in range(n_uniform, S * A):
            add = min(left, S - 1)
            per[r] += add
            left -= add
        assert left == 0
        rows = []
        for r in range(S * A):
            if r < n_uniform:
                rows.append(np.float32(1.0) / np.float32(S))
            else:
                cols = np.sort(rng.choice(S, size=int(per[r]), replace=False)).astype(np.int32)
                rows.append((cols, rng.dirichlet(np.ones(len(cols))).astype(np.float32)))
        return Fixture.from_rows(S, A, rows, (rng.random((S, A)) * 0.05 + 0.001).astype(np.float32), f"edge_S{S}_A{A}_nnz{nnz}")

    J, G = L.SCHEME_JACOBI, L.SCHEME_GAUSS_SEIDEL
    return [(model(5, 2, 10, 0), G),    # size 50 == threshold, density 0.2
            (model(6, 2, 17, 0), J),    # size 72, density just below 0.25
            (model(6, 2, 18, 0), G),    # density exactly 0.25
            (model(6, 2, 17, 1), J),    # a uniform row counts S entries: 6 + 11
            (model(6, 2, 23, 2), G),    # two uniform rows and ten entries: above the density edge
            (model(7, 1, 12, 0), G),    # size 49: below the size edge
            (model(9, 3, 27, 0), J)]    # size 243, density 0.11


EDGE_THRESHOLDS = (50, 0.25)


def pack(fixtures):
    S = np.array([f.S for f in fixtures], np.int32)
    A = np.array([f.A for f in fixtures], np.int32)
    off = np.concatenate([[0], np.cumsum([len(f.col) for f in fixtures])])
    ptr = np.concatenate([[0]] + [f.ptr[1:] + off[b] for b, f in enumerate(fixtures)]).astype(np.int64)
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([getattr(f, k) for f in fixtures]), dt)  # noqa: E731
    return dict(n_states=S, n_actions=A, ptr=ptr, col=cat("col", np.int32), val=cat("val", np.float32),
                uni=cat("uni", np.float32), R=cat("R", np.float32))


def call_raw(args, count, gamma=0.99, eps=EPS, scheme=L.SCHEME_AUTO, size_threshold=SIZE_THRESHOLD,
             density_threshold=DENSITY_THRESHOLD, max_sweeps=1_000_000, out=None):
    """cmdp_vi_discounted_model on packed arguments: (rc, message, out)."""
    lib = L.load()
    if out is None:
        nr = int((args["n_states"].astype(np.int64) * args["n_actions"]).sum()) if count > 0 else 1
        ns = int(args["n_states"].sum()) if count > 0 else 1
        n = max(count, 1)
        out = dict(Q=np.zeros(max(nr, 1), np.float32), V=np.zeros(max(ns, 1), np.float32), sweeps=np.zeros(n, np.int64),
                   scheme=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
    rc = lib.cmdp_vi_discounted_model(count, *[L.ptr(args[k]) for k in ("n_states", "n_actions", "ptr", "col", "val", "uni", "R")],
                                      float(gamma), float(eps), int(scheme), int(size_threshold), float(density_threshold),
                                      int(max_sweeps), *[L.ptr(out[k]) for k in ("Q", "V", "sweeps", "scheme", "status")])
    return rc, lib.cmdp_last_error().decode(), out


def solve(fixtures, **kw):
    """The batch through the kernel: per instance (Q [S * A], V [S], sweeps, scheme_used, status)."""
    rc, msg, out = call_raw(pack(fixtures), len(fixtures), **kw)
    assert rc == L.OK, msg
    res, q0, v0 = [], 0, 0
    for b, f in enumerate(fixtures):
        n = f.S * f.A
        res.append((out["Q"][q0:q0 + n], out["V"][v0:v0 + f.S], int(out["sweeps"][b]), int(out["scheme"][b]), int(out["status"][b])))
        q0 += n
        v0 += f.S
    return res
