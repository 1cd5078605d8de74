"""Extended value iteration on the host: the float64 restatement (tests/helpers_evi.py) against the reference's own
outputs (golden G18), the drop-in's refusal without a device, and the argument checks of the batched call."""
import numpy as np
import pytest

from conftest import load_golden
from helpers_evi import bound, evi_f64, random_problem
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp


def g18():
    z, cases = load_golden("G18_extended_vi")
    for i, c in enumerate(cases):
        yield c, tuple(z[f"c{i}_{k}"] for k in ("T", "R", "beta_r", "beta_p")) + (c["r_max"],), z[f"c{i}_Q"], z[f"c{i}_V"]


def check_against_golden(c, Qr, Vr, span, Q, V, sweeps, umax, n_terms):
    """span, Q, V within the bound of the reference's float32 solve (sdot: S roundings per row) plus this solve's, the
    sweep count equal unless the reference's last ptp lies within that bound of epsilon."""
    b = bound(max(sweeps, c["sweeps"]), umax, c["S"]) + bound(sweeps, umax, n_terms)
    assert abs(float(span) - c["span"]) <= b
    assert np.abs(np.asarray(Q, np.float64) - Qr).max() <= b
    assert np.abs(np.asarray(V, np.float64) - Vr).max() <= b
    if abs(c["last_ptp"] - c["epsilon"]) > b:
        assert sweeps == c["sweeps"]


def test_golden_has_the_quirk_cases():
    n_onehot = n_bern = n_uniform = 0
    for c, (T, R, br, bp, rmax), _, _ in g18():
        S, A = R.shape
        pmax = T.max(-1)
        n_onehot += int((pmax + bp[:, :, 0] / 2 >= 1).sum())
        n_bern += bp.shape[2] == S > 1
        n_uniform += int((T == np.float32(1.0 / S)).all(-1).sum())
    assert n_onehot and n_bern and n_uniform
    assert sorted({c["A"] for c, *_ in g18()}) == [2, 3, 4]


@pytest.mark.parametrize("idx", range(14))
def test_restatement_reproduces_the_reference(idx):
    c, prob, Qr, Vr = list(g18())[idx]
    span, Q, V, sweeps, _, umax, _ = evi_f64(*prob, epsilon=c["epsilon"])
    check_against_golden(c, Qr, Vr, span, Q, V, sweeps, umax, 1)


def test_drop_in_raises_without_a_device():
    if L.load().cmdp_device_count() > 0:
        pytest.skip("a GPU is visible; the no-device path cannot be exercised")
    c, prob, _, _ = next(g18())
    with pytest.raises(L.CmdpError) as ei:
        dp.extended_value_iteration(*prob)
    assert ei.value.code == L.ERR_NO_DEVICE


def test_beta_p_shapes_and_argument_checks_on_the_host():
    T, R, br, bp, rmax = random_problem(5, 2, 0, kind="bernstein")
    S, A = R.shape
    p = dp._evi_problem(T, R, br, bp, rmax)
    assert np.array_equal(p[8], bp[:, :, 0].ravel())                      # element 0 of the Bernstein bound
    p1 = dp._evi_problem(T, R, br, bp[:, :, :1], rmax)
    assert np.array_equal(p1[8], p[8])
    p32 = dp._evi_problem(T, R, br.astype(np.float32), bp.astype(np.float32), rmax)
    assert p32[7].dtype == np.float64 and p32[8].dtype == np.float64      # float32 bounds are widened
    # uniform rows travel as one value and no CSR entries
    Tu = T.copy()
    Tu[1, 0] = np.float32(1.0 / S)
    pu = dp._evi_problem(Tu, R, br, bp, rmax)
    r = 1 * A + 0
    assert pu[5][r] == np.float32(1.0 / S) and pu[2][r + 1] == pu[2][r]
    assert (pu[5] > 0).sum() == int(((Tu == Tu[:, :, :1]).all(-1) & (Tu[:, :, 0] > 0)).sum())
    bad = [
        ((T[:, :, :3], R, br, bp, rmax), "T must be"),
        ((T, R[:, :1], br, bp, rmax), "estimated_rewards"),
        ((T, R, br[:1], bp, rmax), "beta_r"),
        ((T, R, br, bp[:, :, :2], rmax), "beta_p"),
        ((-T, R, br, bp, rmax), "probabilities"),
        ((np.where(T > 0, np.nan, T), R, br, bp, rmax), "probabilities"),
    ]
    for args, msg in bad:
        with pytest.raises(ValueError, match=msg):
            dp.extended_value_iteration_batch([args])
    with pytest.raises(ValueError, match="epsilon"):
        dp.extended_value_iteration_batch([(T, R, br, bp, rmax)], epsilon=-1)
    with pytest.raises(ValueError, match="max_sweeps"):
        dp.extended_value_iteration_batch([(T, R, br, bp, rmax)], max_sweeps=0)
    out, sweeps = dp.extended_value_iteration_batch([])
    assert out == [] and len(sweeps) == 0


def test_c_abi_argument_checks():
    """Checked before any device is touched: each refusal names its argument."""
    lib = L.load()
    S, A = 3, 2
    ptr = np.zeros(S * A + 1, np.int64)
    args = dict(n_states=np.array([S], np.int32), n_actions=np.array([A], np.int32), ptr=ptr,
                col=np.zeros(1, np.int32), val=np.zeros(1, np.float32), uni=np.full(S * A, 1 / 3, np.float32),
                R=np.zeros(S * A, np.float32), br=np.zeros(S * A), bp=np.zeros(S * A), rmax=np.ones(1))
    out = [np.zeros(S * A, np.float32), np.zeros(S, np.float32), np.zeros(1), np.zeros(1, np.int64),
           np.zeros(1, np.int32)]

    def call(eps=1e-3, sweeps=10, count=1, **kw):
        a = dict(args, **kw)
        rc = lib.cmdp_extended_vi(count, *[L.ptr(a[k]) for k in ("n_states", "n_actions", "ptr", "col", "val", "uni",
                                                                   "R", "br", "bp", "rmax")], eps, sweeps,
                                  *[L.ptr(o) for o in out])
        return rc, lib.cmdp_last_error().decode()

    assert call(count=-1) == (L.ERR_INVALID, "count -1 is negative")
    assert "epsilon" in call(eps=-1.0)[1] and call(eps=-1.0)[0] == L.ERR_INVALID
    assert "epsilon" in call(eps=float("nan"))[1]
    assert "max_sweeps" in call(sweeps=0)[1]
    assert "n_states[0]" in call(n_states=np.array([0], np.int32))[1]
    assert "n_actions[0]" in call(n_actions=np.array([0], np.int32))[1]
    assert "r_max[0]" in call(rmax=np.array([np.inf]))[1]
    rc, msg = call(n_states=np.array([5000], np.int32))
    assert rc == L.ERR_UNSUPPORTED and "4096" in msg
    # the row form itself (csr_ptr, csr_col, csr_val, rewards, uniform): tests/test_row_form.py, shared with kernel K14
    assert "beta_r[1]" in call(br=np.array([0, np.inf, 0, 0, 0, 0]))[1]
    assert "beta_p0[5]" in call(bp=np.array([0, 0, 0, 0, 0, np.nan]))[1]
    # a row's bounds are checked after its reward and before its uniform value
    nan2 = np.array([0, 0, np.nan, 0, 0, 0])
    assert "rewards[2]" in call(R=nan2.astype(np.float32), br=nan2, bp=nan2)[1]
    assert "beta_r[2]" in call(br=nan2, bp=nan2, uni=np.array([1 / 3, 1 / 3, -0.5, 1 / 3, 1 / 3, 1 / 3], np.float32))[1]
    assert "beta_p0[0]" in call(bp=np.full(S * A, np.nan), uni=np.full(S * A, -0.5, np.float32))[1]
    assert "uniform[0]" in call(bp=np.array([0, 0, 0, 0, 0, np.nan]), uni=np.full(S * A, -0.5, np.float32))[1]
    assert call(count=0)[0] == L.OK
