"""The finite-horizon kernels on generated episodic MDPs: K4 `k_episodic<DP_VI | DP_PE>` (backward induction), K6
`k_value_norm` and K5E `k_diam_episodic` (the episodic diameter), on ragged batches with one-, two- and three-state
instances, sizes around the 64-lane and 256-thread strides, explicit zeros, rewards of both signs, an unsorted row, several
starting states with non-dyadic weights, the shortest horizon K5E takes and the largest shapes the two LDS rules admit.
Every element of every instance is held bit for bit against the C oracle and against a float64 reference within a bound
derived from the kernel's operation count (helpers_episodic has generator, references, bounds and checkers).

The CPU tests show that the oracle alone passes every float64 check and that the checkers reject planted errors."""
import functools
import json
import os

import numpy as np
import pytest

import helpers_dp_shapes as H
import helpers_episodic as E

EPS = E.EPS
PE_KINDS = ("dirichlet", "onehot")
RATIOS = {}   # "kernel/batch" -> the worst error / bound seen in this process: reported, never asserted


def _note(kernel, name, value):
    key = f"{kernel}/{name}"
    RATIOS[key] = value if isinstance(value, dict) else max(RATIOS.get(key, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _write_ratios():
    """EPISODIC_SHAPES_JSON=<path> writes what the run recorded (profiles/episodic_shapes.json is one such run)."""
    yield
    path = os.environ.get("EPISODIC_SHAPES_JSON")
    if path and RATIOS:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def _pis(name, kind, Hh=None):
    t = E.batch(name)[0]
    return E.layer_policies(t, int(t["H"]) if Hh is None else Hh, kind, seed=17)


@functools.lru_cache(maxsize=None)
def _ref_k4(name, mode, Hh=None):
    """reference_k4 of a named batch: mode "VI", "dirichlet" or "onehot"; computed once, shared and left unchanged."""
    t = E.batch(name)[0]
    Hh = int(t["H"]) if Hh is None else Hh
    return E.reference_k4(t, Hh, None if mode == "VI" else _pis(name, mode, Hh))


@functools.lru_cache(maxsize=None)
def _ref_k6(name):
    t = E.batch(name)[0]
    V = E.random_values(t, seed=23)
    return V, E.reference_k6(t, V)


def _flat(ref, i):
    return np.concatenate([r[i].ravel() for r in ref])


# ---- the generated batches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.SPECS))
def test_batch_has_the_intended_properties(name):
    """generate_episodic asserts reachability, the mixed reach mask, the backbone weights and the row width while it
    builds; here the shape of every named batch."""
    spec = E.SPECS[name]
    t, (soff, sst, sp) = E.batch(name)
    sizes = np.diff(t["state_off"]).tolist()
    assert sizes == spec["sizes"] and int(t["H"]) == spec["Hh"] and int(t["A"]) == spec["A"]
    assert len(sizes) in (2, 3, 4, 5) and len(set(sizes)) == len(sizes), "ragged"
    row_nnz = np.diff(t["csr_ptr"])
    assert row_nnz.max() == spec["nnz"] and row_nnz.min() == 1
    ptr, col, val = t["csr_ptr"], t["csr_col"], t["csr_val"]
    assert np.allclose(np.add.reduceat(val.astype(np.float64), ptr[:-1]), 1.0, atol=1e-6)
    same_row = np.ones(len(col), bool)
    same_row[ptr[:-1]] = False
    descents = int((np.diff(col)[same_row[1:]] <= 0).sum())
    assert (descents > 0) == bool(spec.get("unsorted_row")), "columns ascend within every row but the reversed one"
    assert bool((val == 0).any()) == bool(spec.get("zeros"))
    lo, hi = {"unit": (0, 1), "neg": (-1, 0), "sym": (-1, 1)}[spec.get("rewards", "unit")]
    assert t["R"].min() >= lo and t["R"].max() <= hi and (t["R"].min() < 0) == (lo < 0) and (t["R"].max() > 0) == (hi > 0)
    assert t["rewards_range"] == (float(lo), float(hi))
    assert sp.dtype == np.float32 and sst.dtype == np.int32 and soff.dtype == np.int64
    for b, S in enumerate(sizes):
        st, w = E.instance_starts((soff, sst, sp), b)
        assert 0 in st and w.tolist() == np.asarray(E.START_WEIGHTS[len(st)], np.float32).tolist()
    assert max(np.diff(soff)) == (2 if name == "h2" else 3), "several starting states, three where an instance has the room"


def test_edge_batches_sit_on_the_lds_limits():
    assert 2 * 4 * E.SPECS["k4_edge"]["sizes"][0] == E.LDS_BUDGET == 160 * 1024
    k = E.SPECS["k5e_edge"]
    assert 4 * k["Hh"] * k["sizes"][0] == E.LDS_BUDGET - 1024
    assert E.k5e_fits(128, 318) and not E.k5e_fits(128, 319)
    st = {n: E.SPECS[n] for n in ("small", "stride")}
    assert any(s < 64 for s in st["stride"]["sizes"]) and any(s > 256 for s in st["stride"]["sizes"])
    assert any(s * 3 < 256 for s in st["stride"]["sizes"]) and {64, 65} <= set(st["small"]["sizes"])


def test_restart_batch_returns_to_the_start_distribution():
    """reference_k5e asserts it while it builds: a quarter of the 300-state instance's targets take longer than H."""
    ref = E.reference_k5e("restart")
    assert (ref[0][0] > E.SPECS["restart"]["Hh"]).mean() >= 0.25


def test_h2_every_state_follows_a_starting_state():
    t, starts = E.batch("h2")
    for b in range(int(t["B"])):
        S, A, csr, _ = H.instance(t, b)
        reach, within = E.reach_layers(S, A, csr, E.instance_starts(starts, b)[0], 2)
        assert reach.shape == (1, S) and within.all()


# ---- the oracle alone stays inside every float64 bound -----------------------------------------------------------------------
@pytest.mark.parametrize("name", E.K4_BATCHES + ("k4_edge",))
def test_oracle_k4_passes_the_float64_check(name):
    t = E.batch(name)[0]
    for mode in ("VI",) + PE_KINDS:
        ref = _ref_k4(name, mode)
        ratio = E.check_k4(t, int(t["H"]), _flat(ref, 0), _flat(ref, 1), ref)
        assert 0 <= ratio <= 1


@pytest.mark.parametrize("name", E.K4_BATCHES)
def test_oracle_k6_passes_the_float64_check(name):
    t = E.batch(name)[0]
    V, ref = _ref_k6(name)
    assert 0 <= E.check_k6(t, np.array([r[0] for r in ref]), ref) <= 1
    assert any(r[0] > 1.0 for r in ref) and all(r[0] == 0 for b, r in enumerate(ref) if np.diff(t["state_off"])[b] == 1)


@pytest.mark.parametrize("name", E.K5E_BATCHES)
def test_oracle_k5e_passes_the_float64_check(name):
    orc = E.oracle_k5e_named(name)
    per, diam = np.concatenate([o[1] for o in orc]), np.array([o[0] for o in orc])
    worst, width, sweeps = E.check_k5e(name, per, diam)
    assert 0 <= worst <= 1 and 1 <= sweeps <= 5000


# ---- the checkers reject planted errors ------------------------------------------------------------------------------------------
def _rejected(fn, *args):
    """The planted error is refused by the oracle comparison alone and by the float64 comparison alone."""
    for parts in (("oracle",), ("f64",)):
        with pytest.raises(AssertionError):
            fn(*args, parts=parts)


def test_check_k4_rejects_planted_errors():
    name = "small"
    t = E.batch(name)[0]
    Hh, A, off = int(t["H"]), int(t["A"]), t["state_off"]
    for mode in ("VI", "dirichlet"):
        ref = _ref_k4(name, mode)
        Q, V = _flat(ref, 0), _flat(ref, 1)
        E.check_k4(t, Hh, Q, V, ref)
        # instances 0 (5 states) and 3 (3 states) trade their first 3 states' worth of results
        q, v = Q.copy(), V.copy()
        a, b = (Hh + 1) * int(off[0]), (Hh + 1) * int(off[3])
        n = (Hh + 1) * 3
        v[a:a + n], v[b:b + n] = V[b:b + n], V[a:a + n]
        q[a * A:(a + n) * A], q[b * A:(b + n) * A] = Q[b * A:(b + n) * A], Q[a * A:(a + n) * A]
        _rejected(E.check_k4, t, Hh, q, v, ref)
        _rejected(E.check_k4, t, Hh, Q, v, ref)
        # Q of the 64-state instance one layer late
        q = Q.copy()
        lo, hi = (Hh + 1) * int(off[2]) * A, (Hh + 1) * int(off[3]) * A
        q[lo:hi] = np.roll(Q[lo:hi].reshape(Hh + 1, -1), 1, axis=0).ravel()
        _rejected(E.check_k4, t, Hh, q, V, ref)
        # one value of one layer moved by twice its bound, Q and V in turn
        bq, bv = ref[4][4], ref[4][5]
        for h in (0, Hh - 1):
            q, v = Q.copy(), V.copy()
            q[(Hh + 1) * int(off[4]) * A + h * 65 * A + 77] += np.float32(2 * bq[h])
            v[(Hh + 1) * int(off[4]) + h * 65 + 64] -= np.float32(2 * bv[h])
            _rejected(E.check_k4, t, Hh, q, V, ref)
            _rejected(E.check_k4, t, Hh, Q, v, ref)
        # a layer H that is not zero
        v = V.copy()
        v[(Hh + 1) * int(off[1]) + Hh] = 1e-30
        _rejected(E.check_k4, t, Hh, Q, v, ref)


def test_check_k6_rejects_planted_errors():
    t = E.batch("stride")[0]
    V, ref = _ref_k6("stride")
    out = np.array([r[0] for r in ref])
    E.check_k6(t, out, ref)
    swapped = out.copy()
    swapped[[0, 2]] = out[[2, 0]]
    _rejected(E.check_k6, t, swapped, ref)
    for b in (0, 3):
        moved = out.copy()
        moved[b] += np.float32(2 * (ref[b][3] - ref[b][1]))
        _rejected(E.check_k6, t, moved, ref)
        moved[b] = out[b] - np.float32(2 * (ref[b][1] - ref[b][2]))
        _rejected(E.check_k6, t, moved, ref)


@pytest.mark.parametrize("name", ("small", "restart"))
def test_check_k5e_rejects_planted_errors(name):
    t = E.batch(name)[0]
    off = t["state_off"]
    orc = E.oracle_k5e_named(name)
    per, diam = np.concatenate([o[1] for o in orc]), np.array([o[0] for o in orc])
    E.check_k5e(name, per, diam)
    # two instances trade results (the first states of the largest two)
    a, b = (int(off[2]), int(off[4])) if name == "small" else (int(off[0]), int(off[1]))
    p = per.copy()
    p[a:a + 40], p[b:b + 40] = per[b:b + 40], per[a:a + 40]
    d = np.array([E.split(t, p, i, 1, False).max() for i in range(int(t["B"]))])
    _rejected(E.check_k5e, name, p, d)
    # one target's value replaced by its neighbour's: every target whose neighbour lies outside its intervals (most do)
    ref = E.reference_k5e(name)
    planted = 0
    for i in range(int(t["B"])):
        for j in range(int(off[i + 1] - off[i]) - 1):
            v = float(per[int(off[i]) + j + 1])
            if per[int(off[i]) + j + 1] == per[int(off[i]) + j]:
                continue
            p = per.copy()
            p[int(off[i]) + j] = per[int(off[i]) + j + 1]
            d = np.array([E.split(t, p, k, 1, False).max() for k in range(int(t["B"]))])
            with pytest.raises(AssertionError):
                E.check_k5e(name, p, d, parts=("oracle",))
            if not any(lo <= v <= hi for _, lo, hi in ref[i][1][j]):
                with pytest.raises(AssertionError):
                    E.check_k5e(name, p, d, parts=("f64",))
                planted += 1
    assert planted >= (int(off[-1]) - int(t["B"])) // 2, planted
    # one value moved by twice the half width of its interval, and a diameter that is not the maximum
    (m, lo, hi) = ref[0][1][3][0]
    p = per.copy()
    p[3] += np.float32(2 * (hi - lo))
    d = np.array([E.split(t, p, k, 1, False).max() for k in range(int(t["B"]))])
    _rejected(E.check_k5e, name, p, d)
    d = diam.copy()
    d[0] = np.nextafter(d[0], np.float32(np.inf))
    _rejected(E.check_k5e, name, per, d)


# ---- on the device ---------------------------------------------------------------------------------------------------------
def _L():
    from colosseum_amd import _lib

    return _lib


def _dp(t):
    from colosseum_amd.batched import BatchedMDP

    return BatchedMDP(tables=t, with_env=False)


def _k4(dp, mode, name=None, Hh=None, pis=None, R=None):
    if mode == "VI":
        return dp.episodic_value_iteration(H=Hh, R=R)
    return dp.episodic_policy_evaluation(_pis(name, mode, Hh) if pis is None else pis, H=Hh, R=R)


def _k5e(dp, Hh, starts, eps=EPS, max_sweeps=1_000_000):
    """cmdp_diameter_episodic with explicit starting arrays (table-built batches carry none): (rc, diameter, per_target)."""
    soff, sst, sp = (np.ascontiguousarray(x, dt) for x, dt in zip(starts, (np.int64, np.int32, np.float32)))
    L = _L()
    per = np.zeros(int(dp.state_off[-1]), np.float32)
    diam = np.zeros(dp.B, np.float32)
    rc = dp._lib.cmdp_diameter_episodic(dp.handle, int(Hh), L.ptr(soff), L.ptr(sst), L.ptr(sp), float(eps), int(max_sweeps),
                                        L.ptr(per), L.ptr(diam))
    return rc, diam, per


def _same(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(E._bits(x), E._bits(y)), what


def _single(t, starts, b):
    """Instance b of a batch as a batch of its own."""
    S, A, (lp, col, val), R = H.instance(t, b)
    st, sp = E.instance_starts(starts, b)
    one = dict(B=1, A=A, H=int(t["H"]), rewards_range=t["rewards_range"], state_off=np.array([0, S], np.int64),
               csr_ptr=lp, csr_col=col.copy(), csr_val=val.copy(), R=R.ravel().copy())
    return one, (np.array([0, len(st)], np.int64), st.copy(), sp.copy())


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.K4_BATCHES)
def test_k4_on_generated_batches(need_gpu, name):
    """Value iteration, and policy evaluation under per-layer Dirichlet and one-hot policies: Q and V of every instance
    and layer (check_k4: the oracle bit for bit, float64 within the bound, layer H exactly zero)."""
    t = E.batch(name)[0]
    dp = _dp(t)
    try:
        for mode in ("VI",) + PE_KINDS:
            Q, V = _k4(dp, mode, name)
            _note("K4-" + mode, name, E.check_k4(t, int(t["H"]), Q, V, _ref_k4(name, mode)))
    finally:
        dp.close()


@pytest.mark.gpu
def test_k4_horizon_argument(need_gpu):
    """H = 3, 12 and 3 again on the H = 7 handle (the result buffers grow in between), and H = 5 on an H = 0 batch."""
    t = E.batch("small")[0]
    for tables, horizons in ((t, (3, 12, 3)), (dict(t, H=0), (5,))):
        dp = _dp(tables)
        try:
            assert dp.H == int(tables["H"])
            first = {}
            for Hh in horizons:
                for mode in ("VI", "dirichlet"):
                    res = _k4(dp, mode, "small", Hh)
                    E.check_k4(t, Hh, *res, _ref_k4("small", mode, Hh))
                    if (Hh, mode) in first:
                        _same(res, first[Hh, mode], f"H = {Hh} {mode} repeated after a longer horizon")
                    first.setdefault((Hh, mode), res)
        finally:
            dp.close()


@pytest.mark.gpu
def test_k4_reward_override(need_gpu):
    """-R and a fresh random R against the oracle run on that R; a call without the override afterwards is unchanged."""
    name = "stride"
    t = E.batch(name)[0]
    Hh = int(t["H"])
    fresh = np.random.default_rng(31).uniform(-2.0, 3.0, len(t["R"])).astype(np.float32)
    dp = _dp(t)
    try:
        for mode in ("VI", "dirichlet"):
            pis = None if mode == "VI" else _pis(name, mode)
            plain = _k4(dp, mode, name)
            for R in (-t["R"], fresh):
                res = _k4(dp, mode, name, R=R)
                E.check_k4(t, Hh, *res, E.reference_k4(t, Hh, pis, R))
                assert not np.array_equal(res[0], plain[0])
            again = _k4(dp, mode, name)
            _same(again, plain, f"{mode} without the override after a call with it")
            E.check_k4(t, Hh, *again, _ref_k4(name, mode))
    finally:
        dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("small", "stride"))
def test_k4_batch_independence(need_gpu, name):
    """Instance b solved alone is bit-equal to its part of the batch result."""
    t, starts = E.batch(name)
    Hh = int(t["H"])
    dp = _dp(t)
    try:
        whole = {mode: _k4(dp, mode, name) for mode in ("VI", "dirichlet")}
    finally:
        dp.close()
    for b in range(int(t["B"])):
        one = _dp(_single(t, starts, b)[0])
        try:
            for mode, (Q, V) in whole.items():
                q, v = _k4(one, mode, pis=None if mode == "VI" else [_pis(name, mode)[b]])
                _same((q, v), (E.split(t, Q, b, Hh + 1, True), E.split(t, V, b, Hh + 1, False)), (name, mode, b))
        finally:
            one.close()


@pytest.mark.gpu
def test_k4_largest_instance_and_refusal(need_gpu):
    """20 480 states (two value layers of 160 KiB) are accepted and correct; 20 481 are refused with CMDP_ERR_UNSUPPORTED,
    for both modes, and the handle goes on working (K6 keeps nothing in LDS)."""
    L = _L()
    name = "k4_edge"
    t = E.batch(name)[0]
    dp = _dp(t)
    try:
        for mode in ("VI", "dirichlet"):
            Q, V = _k4(dp, mode, name)
            _note("K4-" + mode, name, E.check_k4(t, int(t["H"]), Q, V, _ref_k4(name, mode)))
    finally:
        dp.close()
    big = E.with_largest(name, E.K4_MAX_S + 1)[0]
    dp = _dp(big)
    try:
        for mode in ("VI", "dirichlet"):
            with pytest.raises(L.CmdpError) as err:
                _k4(dp, mode, pis=E.layer_policies(big, int(big["H"]), "dirichlet", 17))
            assert err.value.code == L.ERR_UNSUPPORTED
        V = E.random_values(big, seed=29)
        E.check_k6(big, dp.value_norm(V), [(o, None, None, None) for o in E.oracle_k6(big, V)], parts=("oracle",))
    finally:
        dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.K4_BATCHES)
def test_k6_on_generated_batches(need_gpu, name):
    """The value norm of a random V of mixed signs and magnitudes up to 1e3, instance by instance; the other instances'
    V set to 1e30 leaves an instance's value bit-identical; a one-state instance (self-loops only) gives exactly 0."""
    t = E.batch(name)[0]
    off = t["state_off"]
    V, ref = _ref_k6(name)
    assert np.abs(V).max() > 100 and (V < 0).any() and (V > 0).any()
    dp = _dp(t)
    try:
        dp.episodic_value_iteration()   # K6 uploads V into the buffer K4 has just grown to H + 1 layers
        out = dp.value_norm(V)
        _note("K6", name, E.check_k6(t, out, ref))
        ones = [b for b in range(int(t["B"])) if off[b + 1] - off[b] == 1]
        assert bool(ones) == (name != "stride") and all(E._bits(out[b]) == 0 for b in ones)
        for b in range(int(t["B"])):
            W = np.full_like(V, 1e30)
            W[int(off[b]):int(off[b + 1])] = V[int(off[b]):int(off[b + 1])]
            assert E._bits(dp.value_norm(W)[b]) == E._bits(out[b]), (name, b)
    finally:
        dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", E.K5E_BATCHES)
def test_k5e_on_generated_batches(need_gpu, name):
    """per_target of every instance bit-equal to the oracle's, the diameter its float32 maximum, every value in an
    admissible interval of the float64 sweep; a one-state instance and targets that are starting states are among them."""
    t, starts = E.batch(name)
    assert (1 in np.diff(t["state_off"])) == (name in ("small", "h2")), "one-state instances are among those checked"
    assert all(0 in E.instance_starts(starts, b)[0] for b in range(int(t["B"]))), "and targets that are starting states"
    dp = _dp(t)
    try:
        rc, diam, per = _k5e(dp, int(t["H"]), starts)
        assert rc == 0, _L().load().cmdp_last_error()
        worst, width, sweeps = E.check_k5e(name, per, diam)
        _note("K5E", name, dict(worst_ratio=worst, relative_interval_width=width, float64_sweeps=sweeps))
    finally:
        dp.close()


@pytest.mark.gpu
def test_k5e_refusals(need_gpu):
    """319 states at H = 128 (one state more than LDS holds): CMDP_ERR_UNSUPPORTED.  H = 1, an instance without a starting
    state, a starting state out of range: CMDP_ERR_INVALID.  Every refusal comes from the host, before a launch."""
    L = _L()
    t, starts = E.with_largest("k5e_edge", 319)
    dp = _dp(t)
    try:
        assert _k5e(dp, 128, starts)[0] == L.ERR_UNSUPPORTED
        rc, diam, per = _k5e(dp, 127, starts)   # 4 * 127 * 319 fits: the same handle solves a shorter horizon
        assert rc == L.OK
        _same((per,), (np.concatenate([o[1] for o in E.oracle_k5e(t, starts, 127)]),), "H = 127 after the refusal")
    finally:
        dp.close()
    t, (soff, sst, sp) = E.batch("small")
    dp = _dp(t)
    try:
        assert _k5e(dp, 1, (soff, sst, sp))[0] == L.ERR_INVALID
        assert _k5e(dp, 0, (soff, sst, sp))[0] == L.ERR_INVALID
        empty = soff.copy()
        empty[2] = empty[1]   # instance 1 has no starting state; instance 2 takes its entry
        assert _k5e(dp, 7, (empty, sst, sp))[0] == L.ERR_INVALID
        for b, bad in ((0, 5), (4, 65), (2, -1)):   # the instance's own S, and a negative state
            s = sst.copy()
            s[int(soff[b])] = bad
            assert _k5e(dp, 7, (soff, s, sp))[0] == L.ERR_INVALID, (b, bad)
        rc, diam, per = _k5e(dp, 7, (soff, sst, sp))
        assert rc == 0
        E.check_k5e("small", per, diam)
    finally:
        dp.close()


@pytest.mark.gpu
def test_k5e_sweep_limit(need_gpu):
    """max_sweeps = 1 returns the not-converged status (CMDP_ERR_MAX_ITER, which the Python layer raises as
    DynamicProgrammingMaxIterationExceeded) as the oracle does; the next call with the default limit is correct."""
    L = _L()
    t, starts = E.batch("restart")
    assert all(rc == -5 for _, _, rc in E.oracle_k5e(t, starts, max_sweeps=1))
    dp = _dp(t)
    try:
        rc = _k5e(dp, int(t["H"]), starts, max_sweeps=1)[0]
        assert rc == L.ERR_MAX_ITER
        with pytest.raises((L.CmdpError, L.DynamicProgrammingMaxIterationExceeded)):
            L.check(rc)
        rc, diam, per = _k5e(dp, int(t["H"]), starts)
        assert rc == 0
        E.check_k5e("restart", per, diam)
    finally:
        dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("small", "h2"))
def test_k5e_batch_independence(need_gpu, name):
    t, starts = E.batch(name)
    dp = _dp(t)
    try:
        rc, diam, per = _k5e(dp, int(t["H"]), starts)
        assert rc == 0
    finally:
        dp.close()
    for b in range(int(t["B"])):
        one_t, one_s = _single(t, starts, b)
        one = _dp(one_t)
        try:
            rc, d, p = _k5e(one, int(t["H"]), one_s)
            assert rc == 0
            _same((p, d), (E.split(t, per, b, 1, False), diam[b:b + 1]), (name, b))
        finally:
            one.close()


@pytest.mark.gpu
def test_k5e_through_the_env_half(need_gpu):
    """A batch built with its environment half from tables: BatchedMDP.diameter_episodic rebuilds the starting weights as
    differences of the accumulated float64 ones; with the weights 0.2 / 0.3 / 0.5 (and 0.5 / 0.3 / 0.2) the result has the
    bits of the call with the explicit float32 weights, and of the oracle."""
    from colosseum_amd.batched import BatchedMDP, tables_from_models
    from colosseum_amd.mdp import make_model
    from oracle import oracle as O

    models = [make_model("MiniGridEmptyEpisodic", seed=s, size=5, p_rand=0.3, n_starting_states=3) for s in (2, 3)]
    t = tables_from_models(models)
    weights = [np.array([0.2, 0.3, 0.5]), np.array([0.5, 0.3, 0.2])]
    assert np.diff(t["start_off"]).tolist() == [3, 3]
    t["start_cum"] = np.concatenate([np.cumsum(w) for w in weights])
    starts = (np.asarray(t["start_off"], np.int64), np.asarray(t["start_state"], np.int32),
              np.concatenate(weights).astype(np.float32))
    dp = BatchedMDP(tables=t)
    try:
        assert dp.models is None and "start_cum" in dp._keep
        diam, per = dp.diameter_episodic()
        rc, diam2, per2 = _k5e(dp, dp.H, starts)
        assert rc == 0
        _same((diam, per), (diam2, per2), "differences of start_cum against the float32 weights")
        for b, m in enumerate(models):
            od, oper, orc = O.diameter_episodic_csr(m.n_states, m.n_actions, m.H, m.csr(), *E.instance_starts(starts, b))
            assert orc == 0 and np.array_equal(E._bits(dp.split_states(per)[b]), E._bits(oper)) and diam[b] == np.float32(od)
    finally:
        dp.close()
