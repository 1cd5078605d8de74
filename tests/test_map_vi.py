"""Value iteration on the MAP estimate of a Bayesian model (kernel K15), what needs no device: the host definition of the
kernel's prologue (cmdp_psrl_map_rows) against numpy's own MAP estimate bit for bit, the Python packer, the float64
restatement the GPU tests use against the Q the reference recorded (golden G21), and the argument checks."""
import numpy as np
import pytest

import helpers_map_vi as M
from helpers_psrl import bound_episodic
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp

# every branch of numpy's pairwise sum: n < 8, <= 128 with and without a remainder, the recursion
SIZES = [1, 5, 7, 8, 9, 13, 127, 128, 129, 131, 136, 359, 600]


def assert_map_rows(thp, prior, keep=None):
    S, A, _ = thp.shape
    row_ptr, col, hp = dp.map_layout_from_dense(thp, prior, keep)
    rowsum, c, t = dp.psrl_map_rows(row_ptr, col, hp, prior, S, A)
    ref_sum = thp.sum(-1, keepdims=True)
    T = thp / ref_sum
    assert T.dtype == np.float32
    assert np.array_equal(rowsum, ref_sum[:, :, 0])
    # the MAP estimate rebuilt from (c, t) is numpy's, element for element
    dense = np.repeat(c.reshape(S * A, 1), S, axis=1)
    dense[np.repeat(np.arange(S * A), np.diff(row_ptr)), col] = t
    assert np.array_equal(dense.reshape(S, A, S), T)
    return row_ptr, col, hp


@pytest.mark.parametrize("S", SIZES)
def test_map_rows_equal_numpys_map_estimate(S):
    for A, seed in ((1, 0), (3, 1)):
        thp, _, prior = M.tables(S, A, seed=seed)
        row_ptr, _, _ = assert_map_rows(thp, prior)
        assert row_ptr[-1] > 0 or S == 1
    # a row whose layout is the whole row, an empty row, and values far apart in magnitude
    rng = np.random.RandomState(S)
    thp, _, prior = M.tables(S, 2, seed=2)
    thp[0, 0] = (rng.gamma(0.3, size=S) * 50 + 1e-3).astype(np.float32)
    thp[S - 1, 1] = prior
    keep = np.zeros(thp.shape, bool)
    keep[0, 0] = True
    row_ptr, _, _ = assert_map_rows(thp, prior, keep)
    assert row_ptr[1] - row_ptr[0] == S and row_ptr[-1] == row_ptr[-2]


def test_map_rows_on_every_stage_of_g21():
    n = 0
    for i, m, ep, z in M.g21_stages():
        S, A = m["S"], m["A"]
        thp = z["transition_hp"]
        prior = np.float32(1.0 / S) if m["transitions_prior_prms"] is None else np.float32(m["transitions_prior_prms"][0])
        if ep == 0:
            assert (thp == prior).all()
        assert_map_rows(thp, prior)
        assert np.array_equal(M.map_estimate(thp), z["T_map"]) and np.array_equal(z["reward_hp"][:, :, 0], z["R_map"])
        n += 1
    assert n == 12


def test_packer_round_trips():
    thp, mu, prior = M.tables(13, 3, seed=3)
    row_ptr, col, hp = dp.map_layout_from_dense(thp, prior)
    assert (np.diff(row_ptr) >= 0).all() and row_ptr[0] == 0 and len(col) == row_ptr[-1] == (thp != prior).sum()
    for r in range(13 * 3):
        assert (np.diff(col[row_ptr[r]:row_ptr[r + 1]]) > 0).all()
    assert np.array_equal(dp.map_layout_to_dense(row_ptr, col, hp, prior, 13, 3), thp)
    # positions the caller names are kept although they hold the prior
    keep = np.zeros(thp.shape, bool)
    keep[2, 1, :] = True
    p2, c2, h2 = dp.map_layout_from_dense(thp, prior, keep)
    assert p2[2 * 3 + 2] - p2[2 * 3 + 1] == 13 and np.array_equal(dp.map_layout_to_dense(p2, c2, h2, prior, 13, 3), thp)
    # both forms of a problem pack to the same arrays
    a = dp._map_problem((thp, mu, prior))
    b = dp._map_problem((row_ptr, col, hp, prior, mu))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert dp.episodic_value_iteration_map_batch([], 3) == []


def test_restatement_against_the_reference_q():
    """The float64 restatement on G21's tables within bound_episodic(H, qmax, S) of the Q the reference recorded (its BLAS
    product of S terms, float32), and the recorded policy greedy for the restatement up to that bound."""
    for i, m, ep, z in M.g21_stages():
        H, S = m["H"], m["S"]
        Q64, _, _ = M.restatement(z["transition_hp"], z["R_map"], H)
        tol = bound_episodic(H, float(np.abs(Q64).max()), S)
        err = float(np.abs(z["Q"] - Q64).max())
        assert err <= tol, (i, ep, err, tol)
        assert z["policy"].shape == (H + 1, S, m["A"])
        M.check_greedy(z["policy"], Q64, tol)


def test_argument_refusals_without_a_device():
    lib = L.load()
    thp, mu, prior = M.tables(5, 2, seed=0)
    row_ptr, col, hp = dp.map_layout_from_dense(thp, prior)
    S, A = np.array([5], np.int32), np.array([2], np.int32)
    pr, muf = np.array([prior], np.float32), mu.ravel().copy()
    Q, V = np.zeros(4 * 10, np.float32), np.zeros(4 * 5, np.float32)

    def call(count=1, S=S, A=A, H=3, row_ptr=row_ptr, col=col, hp=hp, prior=pr, mu=muf, Q=Q, V=V):
        rc = lib.cmdp_vi_episodic_map(count, L.ptr(S), L.ptr(A), H, L.ptr(row_ptr), L.ptr(col), L.ptr(hp), L.ptr(prior), L.ptr(mu),
                                      L.ptr(Q), L.ptr(V), None, None)
        return rc, lib.cmdp_last_error().decode()

    assert call(count=0)[0] == L.OK
    assert call(count=-1) == (L.ERR_INVALID, "count -1 is negative")
    for k in ("S", "A", "row_ptr", "prior", "mu", "Q", "V", "col", "hp"):
        rc, msg = call(**{k: None})
        assert rc == L.ERR_INVALID and "null argument" in msg, (k, rc, msg)
    assert call(H=0)[0] == L.ERR_INVALID
    assert call(S=np.array([0], np.int32))[0] == L.ERR_INVALID and call(A=np.array([0], np.int32))[0] == L.ERR_INVALID
    rc, msg = call(S=np.array([4097], np.int32))
    assert rc == L.ERR_UNSUPPORTED and "4096" in msg
    bad = row_ptr.copy(); bad[0] = 1
    assert call(row_ptr=bad)[0] == L.ERR_INVALID
    bad = row_ptr.copy(); bad[3] = bad[2] - 1
    rc, msg = call(row_ptr=bad)
    assert rc == L.ERR_INVALID and "decreases" in msg
    r = int(np.flatnonzero(np.diff(row_ptr) >= 1)[0])
    bad = col.copy(); bad[row_ptr[r]] = 5
    assert call(col=bad)[0] == L.ERR_INVALID
    bad = col.copy(); bad[row_ptr[r]] = -1
    assert call(col=bad)[0] == L.ERR_INVALID
    two = np.flatnonzero(np.diff(row_ptr) >= 2)
    if len(two):
        bad = col.copy(); k = row_ptr[two[0]]; bad[k + 1] = bad[k]
        rc, msg = call(col=bad)
        assert rc == L.ERR_INVALID and "ascending" in msg
    bad = hp.copy(); bad[0] = -1.0
    assert call(hp=bad)[0] == L.ERR_INVALID
    bad = hp.copy(); bad[0] = np.nan
    assert call(hp=bad)[0] == L.ERR_INVALID
    for p in (0.0, -1.0, np.inf, np.nan):
        rc, msg = call(prior=np.array([p], np.float32))
        assert rc == L.ERR_INVALID and "prior[0]" in msg, p
    # the host-only definition refuses the same layouts
    z = np.zeros(10, np.float32)
    assert lib.cmdp_psrl_map_rows(0, 2, L.ptr(row_ptr), L.ptr(col), L.ptr(hp), float(prior), L.ptr(z), L.ptr(z), None) == L.ERR_INVALID
    assert lib.cmdp_psrl_map_rows(5, 2, None, L.ptr(col), L.ptr(hp), float(prior), L.ptr(z), L.ptr(z), None) == L.ERR_INVALID
    assert lib.cmdp_psrl_map_rows(5, 2, L.ptr(row_ptr), L.ptr(col), L.ptr(hp), 0.0, L.ptr(z), L.ptr(z), None) == L.ERR_INVALID
    assert lib.cmdp_psrl_map_rows(5, 2, L.ptr(row_ptr), L.ptr(col), L.ptr(hp), float(prior), None, None, None) == L.OK
    # the Python front refuses malformed problems before the library sees them
    with pytest.raises(ValueError):
        dp.episodic_value_iteration_map_batch([(thp, mu, prior)], 0)
    with pytest.raises(ValueError):
        dp.episodic_value_iteration_map_batch([(thp, mu[:, :1], prior)], 3)
    with pytest.raises(ValueError):
        dp.episodic_value_iteration_map_batch([(row_ptr[:-1], col, hp, prior, mu)], 3)
    with pytest.raises(ValueError):
        dp.episodic_value_iteration_map_batch([(thp, mu)], 3)
    with pytest.raises(ValueError):
        dp.psrl_map_rows(row_ptr[:-1], col, hp, prior, 5, 2)
