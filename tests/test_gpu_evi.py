"""Extended value iteration on the device (K10 k_evi through cmdp_extended_vi): the reference's outputs (golden G18),
generated shapes against the float64 restatement, the reference's quirks one case each, max_sweeps per instance,
bit-identical results alone / in a large mixed batch / repeated, and the refusals."""
import numpy as np
import pytest

from helpers_evi import bound, evi_f64, random_problem
from test_evi import check_against_golden, g18
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp

pytestmark = pytest.mark.gpu

MAX_SWEEPS = 3000

# (S, A, density, bound kind, bound scale); S from 1 to the LDS limit, around 64 / 256 / 1024, not powers of two
SHAPES = [
    (1, 1, "sparse", "chernoff", 0.05), (2, 3, "mixed", "bernstein", 0.05), (3, 5, "dense", "chernoff", 0.1),
    (5, 2, "sparse", "bernstein", 0.02), (7, 4, "uniform", "chernoff", 0.3), (13, 1, "mixed", "chernoff", 0.01),
    (31, 3, "mixed", "bernstein", 0.05), (63, 2, "mixed", "chernoff", 0.05), (64, 4, "sparse", "bernstein", 0.1),
    (65, 5, "dense", "chernoff", 0.02), (100, 3, "uniform", "bernstein", 0.05), (127, 1, "dense", "chernoff", 0.5),
    (129, 2, "mixed", "bernstein", 0.2), (200, 4, "sparse", "chernoff", 0.05), (255, 2, "mixed", "chernoff", 0.05),
    (256, 3, "dense", "bernstein", 0.01), (257, 1, "uniform", "chernoff", 0.05), (300, 5, "mixed", "bernstein", 0.1),
    (400, 4, "mixed", "chernoff", 0.02), (511, 2, "sparse", "bernstein", 0.3), (600, 3, "dense", "chernoff", 0.05),
    (784, 3, "mixed", "bernstein", 0.05), (1000, 1, "mixed", "chernoff", 0.05), (1023, 2, "uniform", "bernstein", 0.5),
    (1024, 1, "sparse", "chernoff", 0.05), (1025, 2, "mixed", "chernoff", 0.05), (1500, 1, "dense", "bernstein", 0.02),
    (2047, 1, "mixed", "chernoff", 0.05), (3000, 1, "uniform", "chernoff", 0.3), (4096, 1, "mixed", "chernoff", 0.05),
    (9, 2, "mixed", "chernoff", 5.0), (50, 3, "mixed", "bernstein", 2.0), (17, 2, "sparse", "chernoff", 0.0),
    (40, 5, "mixed", "chernoff", 0.05), (90, 2, "dense", "bernstein", 0.05), (150, 4, "mixed", "chernoff", 0.05),
    (333, 1, "mixed", "bernstein", 0.05), (700, 2, "sparse", "chernoff", 0.05), (2500, 1, "uniform", "chernoff", 0.05),
    (48, 3, "mixed", "chernoff", 0.05),
]


def solve(prob, max_sweeps=MAX_SWEEPS):
    out, sweeps = dp.extended_value_iteration_batch([prob], max_sweeps=max_sweeps)
    return out[0], int(sweeps[0])


def assert_near_restatement(prob, res, sweeps, max_sweeps=MAX_SWEEPS):
    span_r, Q_r, V_r, sw_r, last_ptp, umax, _ = evi_f64(*prob, max_sweeps=max_sweeps)
    b = 2 * bound(max(sweeps, sw_r), umax + 2.0, 1)
    if res is None or span_r is None:
        assert (res is None) == (span_r is None) or abs(last_ptp - 1e-3) <= b, (sweeps, sw_r, last_ptp)
        return
    span, Q, V = res
    assert Q.dtype == np.float32 and V.dtype == np.float32 and isinstance(span, np.float32)
    if abs(last_ptp - 1e-3) > b:
        assert sweeps == sw_r
    assert abs(float(span) - span_r) <= b, (float(span), span_r, b)
    assert np.abs(Q - Q_r).max() <= b
    assert np.abs(V - V_r).max() <= b
    assert np.array_equal(V, Q.max(axis=1))


def test_golden_through_the_drop_in(need_gpu):
    for c, prob, Qr, Vr in g18():
        res = dp.extended_value_iteration(*prob)
        assert res is not None
        span, Q, V = res
        (out,), sweeps = dp.extended_value_iteration_batch([prob])
        assert np.array_equal(out[1], Q) and out[0] == span
        umax_r = evi_f64(*prob)[5]
        check_against_golden(c, Qr, Vr, span, Q, V, int(sweeps[0]), umax_r, 1)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"S{s}_A{a}_{d}_{k}_{x}" for s, a, d, k, x in SHAPES])
def test_generated_shapes_against_float64(need_gpu, shape):
    S, A, density, kind, scale = shape
    prob = random_problem(S, A, seed=S * 7 + A, density=density, kind=kind, scale=scale,
                          r_max=0.8 if S % 3 == 0 else 1.0)  # every third shape caps r_opt at r_max
    res, sweeps = solve(prob)
    assert_near_restatement(prob, res, sweeps)


def test_only_element_0_of_a_bernstein_bound_counts(need_gpu):
    T, R, br, bp, rmax = random_problem(60, 3, 11, kind="bernstein", scale=0.1)
    bp2 = bp.copy()
    bp2[:, :, 1:] = np.random.default_rng(0).random((60, 3, 59))
    a, _ = solve((T, R, br, bp, rmax))
    b, _ = solve((T, R, br, bp2, rmax))
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    bp3 = bp.copy()
    bp3[:, :, 0] *= 3
    c, _ = solve((T, R, br, bp3, rmax))
    assert not np.array_equal(a[1], c[1])


def test_min1_of_one_gives_a_one_hot_row(need_gpu):
    """Bounds of 2 make every row one-hot at the best state: after two sweeps Q = r + float(u1[best] - u1[s])."""
    S, A = 6, 2
    T, R, br, _, _ = random_problem(S, A, 3, density="mixed")
    bp = np.full((S, A, 1), 2.0)
    br = np.zeros((S, A))
    R2 = np.repeat(R[:, :1], A, axis=1)
    (res,), sw = dp.extended_value_iteration_batch([(T, R2, br, bp, 1.0)])
    u1 = R2[:, 0].astype(np.float32)                     # sweep 1: u2 = r (all u1 = 0)
    best = np.argsort(u1, kind="stable")[-1]
    dot = (u1[best].astype(np.float64) - u1.astype(np.float64)).astype(np.float32)
    Q2 = (R2.astype(np.float64) + dot[:, None].astype(np.float64)).astype(np.float32)
    assert sw[0] == 2 and np.array_equal(res[1], Q2)


def test_epsilon_tie_rule_keeps_the_last_action(need_gpu):
    """State 0's two actions lead to the absorbing state 1 with rewards 0.5 and 0.4996: within epsilon, so u2[0] takes
    the LAST action's value and the span is 0.4996, while V[0] = max Q is the true maximum."""
    T = np.zeros((2, 2, 2), np.float32)
    T[0, :, 1] = 1
    T[1, :, 1] = 1
    R = np.array([[0.5, 0.4996], [0, 0]], np.float32)
    zero = np.zeros((2, 2))
    span, Q, V = dp.extended_value_iteration(T, R, zero, zero[:, :, None], 1.0)
    assert span == np.float32(0.4996)
    assert V[0] == np.float32(np.float32(0.5) - np.float32(0.4996))
    R[0] = [0.4996, 0.5]
    span, _, _ = dp.extended_value_iteration(T, R, zero, zero[:, :, None], 1.0)
    assert span == np.float32(0.5)


def test_span_is_taken_from_the_previous_u1(need_gpu):
    """Two self-loops with rewards 1 and 1.0005: ptp(u2 - u1) = 0.0005 < epsilon after the first sweep, and the span is
    ptp(u1) = 0 of the vector that sweep read, not ptp(u2) = 0.0005."""
    T = np.zeros((2, 1, 2), np.float32)
    T[0, 0, 0] = T[1, 0, 1] = 1
    R = np.array([[1.0], [1.0005]], np.float32)
    z = np.zeros((2, 1))
    (res,), sweeps = dp.extended_value_iteration_batch([(T, R, z, z[:, :, None], 2.0)])
    assert sweeps[0] == 1 and res[0] == 0.0
    assert np.array_equal(res[2], R[:, 0])


def test_max_sweeps_fails_only_that_instance(need_gpu):
    T = np.zeros((2, 1, 2), np.float32)  # a 2-cycle with reward on one side never converges
    T[0, 0, 1] = T[1, 0, 0] = 1
    R = np.array([[1.0], [0.0]], np.float32)
    z = np.zeros((2, 1))
    cyc = (T, R, z, z[:, :, None], 1.0)
    ok1 = random_problem(20, 3, 1, scale=0.05)
    ok2 = random_problem(9, 2, 2, kind="bernstein", scale=0.05)
    out, sweeps = dp.extended_value_iteration_batch([ok1, cyc, ok2], max_sweeps=500)
    assert out[1] is None and sweeps[1] == 500
    for i, p in ((0, ok1), (2, ok2)):
        (alone,), sw = dp.extended_value_iteration_batch([p], max_sweeps=500)
        assert sweeps[i] == sw[0] < 500
        assert alone[0] == out[i][0] and np.array_equal(alone[1], out[i][1]) and np.array_equal(alone[2], out[i][2])
    lib = L.load()
    # through the C ABI: the status of the cycle is CMDP_ERR_MAX_ITER and the call succeeds
    p = dp._evi_problem(*cyc)
    Q, V = np.zeros(2, np.float32), np.zeros(2, np.float32)
    span, sw, st = np.zeros(1), np.zeros(1, np.int64), np.zeros(1, np.int32)
    rc = lib.cmdp_extended_vi(1, L.ptr(np.array([2], np.int32)), L.ptr(np.array([1], np.int32)), L.ptr(p[2]),
                              L.ptr(p[3]), L.ptr(p[4]), L.ptr(p[5]), L.ptr(p[6]), L.ptr(p[7]), L.ptr(p[8]),
                              L.ptr(np.ones(1)), 1e-3, 77, L.ptr(Q), L.ptr(V), L.ptr(span), L.ptr(sw), L.ptr(st))
    assert rc == L.OK and st[0] == L.ERR_MAX_ITER and sw[0] == 77 and np.isnan(span[0])


def test_alone_in_a_large_mixed_batch_and_repeated_bit_identical(need_gpu):
    rng = np.random.default_rng(123)
    probs = []
    for i in range(1000):
        S = int(rng.choice([1, 2, 5, 17, 40, 63, 64, 65, 90, 130]))
        probs.append(random_problem(S, int(rng.integers(1, 6)), 5000 + i, density=["sparse", "mixed", "uniform"][i % 3],
                                    kind=["chernoff", "bernstein"][i % 2], scale=0.05))
    probs[500] = random_problem(1500, 1, 77, scale=0.05)
    out, sweeps = dp.extended_value_iteration_batch(probs, max_sweeps=MAX_SWEEPS)
    out2, sweeps2 = dp.extended_value_iteration_batch(probs, max_sweeps=MAX_SWEEPS)
    assert np.array_equal(sweeps, sweeps2)
    for a, b in zip(out, out2):
        assert (a is None) == (b is None)
        if a is not None:
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for i in (0, 1, 2, 333, 500, 998, 999):
        (alone,), sw = dp.extended_value_iteration_batch([probs[i]], max_sweeps=MAX_SWEEPS)
        assert sw[0] == sweeps[i]
        assert (alone is None) == (out[i] is None)
        if alone is not None:
            assert alone[0] == out[i][0] and np.array_equal(alone[1], out[i][1]) and np.array_equal(alone[2], out[i][2])


def test_refusals(need_gpu):
    T = np.full((4097, 1, 4097), np.float32(1 / 4097))
    z = np.zeros((4097, 1))
    with pytest.raises(L.CmdpError) as ei:
        dp.extended_value_iteration(T, z.astype(np.float32), z, z[:, :, None], 1.0)
    assert ei.value.code == L.ERR_UNSUPPORTED and "4096" in str(ei.value)
    lib = L.load()
    one = np.ones(1, np.int32)
    rc = lib.cmdp_extended_vi(1, L.ptr(one), L.ptr(one), L.ptr(np.zeros(2, np.int64)), None, None,
                              L.ptr(np.ones(1, np.float32)), L.ptr(np.zeros(1, np.float32)), L.ptr(np.zeros(1)),
                              L.ptr(np.zeros(1)), L.ptr(np.ones(1)), -1.0, 10, L.ptr(np.zeros(1, np.float32)),
                              L.ptr(np.zeros(1, np.float32)), L.ptr(np.zeros(1)), L.ptr(np.zeros(1, np.int64)),
                              L.ptr(np.zeros(1, np.int32)))
    assert rc == L.ERR_INVALID and b"epsilon" in lib.cmdp_last_error()
