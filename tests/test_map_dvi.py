"""Discounted value iteration on the MAP model from its tables (kernel K17), what needs no device: the NumPy twin of the
kernel's definition (tests/helpers_map_dvi.py) against the float64 restatement on the dense MAP model within the derived
bound, and the argument checks of the Python entry, of set_policy_solver and of the C ABI."""
import os

import numpy as np
import pytest

import helpers_map_dvi as M
from conftest import ROOT
from helpers_psrlc import GAMMA32, GAUSS_SEIDEL, JACOBI, vi_discounted_f64, vi_rule
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp
from colosseum_amd.agents import BatchedPSRLContinuous

EPS = 1e-3


@pytest.mark.parametrize("scheme", [JACOBI, GAUSS_SEIDEL], ids=["jacobi", "gauss_seidel"])
@pytest.mark.parametrize("which,gamma", [("small", GAMMA32), ("large", M.GAMMA09)], ids=["small", "large"])
def test_twin_within_the_bound_of_the_float64_restatement(which, gamma, scheme):
    """The definition itself, at the twin's own sweep count: |Q - Q64| <= bound_discounted_map and the restatement's last two
    differences straddle epsilon within two bounds."""
    worst, counts = 0.0, []
    for row_ptr, col, hp, prior, mu in M.ragged_problems(which):
        S, A = mu.shape
        Q, V, n, ok = M.map_dvi_twin(row_ptr, col, hp, prior, mu, gamma, scheme, EPS)
        assert ok and np.array_equal(V, Q.max(-1))
        _, c, t = dp.psrl_map_rows(row_ptr, col, hp, prior, S, A)
        T = M.map_dense(row_ptr, col, t, c, S, A)
        Q64, d_n, d_prev, qmax = vi_discounted_f64(T, mu, gamma, scheme, n)
        bound = M.bound_discounted_map(n, gamma, qmax, S)
        err = float(np.abs(Q.astype(np.float64) - Q64).max())
        assert err <= bound, (S, A, err, bound, n)
        assert d_n < EPS + 2 * bound and (n == 1 or d_prev >= EPS - 2 * bound), (S, A, d_n, d_prev, bound)
        worst = max(worst, err / bound)
        counts.append(n)
    print(f"{which}, scheme {scheme}: sweeps {counts}, worst |Q - Q64| / bound {worst:.3f}")
    if which == "small":   # the instance with mu = 0 stops after its first sweep, others take hundreds
        assert counts[-1] == 1 and max(counts) > 200


def test_generated_problems_hold_the_cases_they_are_for():
    small, large = M.ragged_problems("small"), M.ragged_problems("large")
    shapes = [p[4].shape for p in small + large]
    assert {s for s, _ in shapes} == {1, 2, 3, 5, 63, 64, 65, 129, 200}
    assert {a for _, a in shapes} >= {1, 3, 4, 5, 64, 65}
    lens = [np.diff(p[0]) for p in small + large]
    assert any((ln == 0).any() for ln in lens) and any((ln > 64).any() and (ln < p[4].shape[0]).any() for ln, p in zip(lens, small + large))
    assert sum(bool((ln == p[4].shape[0]).any()) for ln, p in zip(lens, small + large)) >= 4   # len == S
    assert any(p[4].min() < 0 < p[4].max() for p in small)
    for p in small + large:   # hp = prior + an integer count up to 10^5
        k = p[2].astype(np.float64) - float(p[3])
        assert (k > -1e-3).all() and (k <= 1e5 + 1).all()
    # the rule's two instances: c underflows to zero under the subnormal prior, and the dense count decides
    dense, sparse = M.rule_problems()
    want = []
    for row_ptr, col, hp, prior, mu in (dense, sparse):
        S, A = mu.shape
        _, c, t = dp.psrl_map_rows(row_ptr, col, hp, prior, S, A)
        nnz = M.dense_nnz(row_ptr, t, c, S)
        assert nnz == int((M.map_dense(row_ptr, col, t, c, S, A) != 0).sum())
        want.append(vi_rule(S, A, nnz, 100))
        assert vi_rule(S, A, nnz) == GAUSS_SEIDEL
    assert want == [GAUSS_SEIDEL, JACOBI]


def test_python_entry_refuses_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(L, "load", no_load)
    p = M.ragged_problems("small")[2]
    f = dp.discounted_value_iteration_map_batch
    for kw in (dict(epsilon=-1e-3), dict(epsilon=float("nan")), dict(epsilon=float("inf")), dict(max_sweeps=0), dict(scheme=0),
               dict(scheme=3), dict(gamma=float("inf")), dict(sparse_n_states_threshold=-1), dict(sparse_nnz_per_threshold=float("nan"))):
        with pytest.raises(ValueError):
            f([p], **kw)
    row_ptr, col, hp, prior, mu = p
    for bad in ((row_ptr[:-1], col, hp, prior, mu), (row_ptr, col[:-1], hp, prior, mu), (row_ptr, col, hp[:-1], prior, mu),
                (row_ptr, col, hp, prior, mu.ravel()), (row_ptr + 1, col, hp, prior, mu), (row_ptr, col),
                (np.zeros((2, 3, 3), np.float32), np.zeros((2, 3), np.float32), 0.5),
                (np.zeros((2, 3, 2), np.float32), np.zeros((3, 2), np.float32), 0.5)):
        with pytest.raises(ValueError):
            f([bad])
    assert f([]) == []


def test_set_policy_solver_checks_its_argument_first():
    assert BatchedPSRLContinuous._POLICY_SOLVERS == ("dense", "tables")
    for bad in ("sparse", "", None, 1, "Tables"):
        with pytest.raises(ValueError, match="policy solver"):
            BatchedPSRLContinuous.set_policy_solver(None, bad)   # no agent is needed to be refused
    assert isinstance(BatchedPSRLContinuous.policy_solver, property)


def test_option_id_is_the_headers():
    src = open(os.path.join(ROOT, "include", "cmdp.h")).read()
    assert f"CMDP_PSRLC_OPT_POLICY_SOLVER = {L.PSRLC_OPT_POLICY_SOLVER}" in src and L.PSRLC_OPT_POLICY_SOLVER == 3
    assert "cmdp_vi_discounted_map" in L.EXPORTS
    assert L.load().cmdp_psrlc_set_option(None, L.PSRLC_OPT_POLICY_SOLVER, 1) == L.ERR_INVALID   # a null agent


def test_abi_refusals():
    """Every null or invalid argument of cmdp_vi_discounted_map, by name, before the device is touched."""
    lib = L.load()
    S, A = np.array([2], np.int32), np.array([2], np.int32)
    ptr = np.array([0, 1, 1, 3, 3], np.int64)
    col, hp = np.array([1, 0, 1], np.int32), np.array([2.5, 1.5, 3.5], np.float32)
    prior, mu = np.array([0.5], np.float32), np.array([0.1, -0.2, 0.3, 0.0], np.float32)
    Q, V = np.zeros(4, np.float32), np.zeros(2, np.float32)
    sw, sc, stt = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(1, np.int32)
    good = dict(count=1, S=S, A=A, ptr=ptr, col=col, hp=hp, prior=prior, mu=mu, gamma=0.99, eps=1e-3, scheme=L.SCHEME_AUTO,
                size=270000, dens=0.2, sweeps=100, Q=Q, V=V, sw=sw, sc=sc, st=stt, t=None, c=None)

    def call(**kw):
        a = dict(good, **kw)
        p = lambda x: None if x is None else L.ptr(x)  # noqa: E731
        return lib.cmdp_vi_discounted_map(a["count"], p(a["S"]), p(a["A"]), p(a["ptr"]), p(a["col"]), p(a["hp"]), p(a["prior"]),
                                          p(a["mu"]), a["gamma"], a["eps"], a["scheme"], a["size"], a["dens"], a["sweeps"],
                                          p(a["Q"]), p(a["V"]), p(a["sw"]), p(a["sc"]), p(a["st"]), p(a["t"]), p(a["c"]))

    def refused(code, word, **kw):
        assert call(**kw) == code and word in lib.cmdp_last_error(), (kw.keys(), lib.cmdp_last_error())

    refused(L.ERR_INVALID, b"negative", count=-1)
    assert call(count=0) == L.OK
    for key, name in (("S", b"n_states"), ("A", b"n_actions"), ("ptr", b"row_ptr"), ("col", b"col"), ("hp", b"hp"),
                      ("prior", b"prior"), ("mu", b"mu"), ("Q", b"Q"), ("V", b"V"), ("sw", b"sweeps"), ("sc", b"scheme_used"),
                      ("st", b"status")):
        refused(L.ERR_INVALID, name + b" is null", **{key: None})
    refused(L.ERR_INVALID, b"gamma", gamma=float("nan"))
    refused(L.ERR_INVALID, b"gamma", gamma=float("inf"))
    for eps in (-1e-3, float("nan"), float("inf")):
        refused(L.ERR_INVALID, b"epsilon", eps=eps)
    refused(L.ERR_INVALID, b"max_sweeps", sweeps=0)
    refused(L.ERR_INVALID, b"scheme", scheme=3)
    refused(L.ERR_INVALID, b"scheme", scheme=-1)
    refused(L.ERR_INVALID, b"size_threshold", size=-1)
    refused(L.ERR_INVALID, b"density_threshold", dens=float("nan"))
    refused(L.ERR_INVALID, b"n_states", S=np.array([0], np.int32))
    refused(L.ERR_INVALID, b"n_actions", A=np.array([0], np.int32))
    refused(L.ERR_UNSUPPORTED, b"4096", S=np.array([4097], np.int32), ptr=np.zeros(4097 * 2 + 1, np.int64),
            mu=np.zeros(4097 * 2, np.float32))
    refused(L.ERR_INVALID, b"row_ptr[0]", ptr=ptr + 1)
    refused(L.ERR_INVALID, b"decreases", ptr=np.array([0, 2, 1, 3, 3], np.int64))
    refused(L.ERR_INVALID, b"ascending", col=np.array([1, 1, 0], np.int32))
    refused(L.ERR_INVALID, b"ascending", col=np.array([2, 0, 1], np.int32))
    refused(L.ERR_INVALID, b"ascending", col=np.array([-1, 0, 1], np.int32))
    for bad in (np.nan, np.inf, -1.0):
        refused(L.ERR_INVALID, b"finite", hp=np.array([2.5, bad, 3.5], np.float32))
    for bad in (0.0, -0.5, np.nan, np.inf):
        refused(L.ERR_INVALID, b"prior[0]", prior=np.array([bad], np.float32))
    bad = mu.copy()
    bad[2] = np.nan
    refused(L.ERR_INVALID, b"mu[2]", mu=bad)
    # an empty layout needs neither col nor hp
    if lib.cmdp_device_count() == 0:   # valid arguments get as far as the device
        assert call() == L.ERR_NO_DEVICE
        assert call(ptr=np.zeros(5, np.int64), col=None, hp=None) == L.ERR_NO_DEVICE
