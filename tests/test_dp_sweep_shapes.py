"""Every compiled discounted sweep kernel against the oracle (bit for bit) and against float64 solutions.

The Jacobi sweeps run on K2 (k_dp_block, CSR in LDS or HBM), K2R (k_dp_reg), K2U (k_dp_regu) or K2W (k_dp_regw), the
Gauss-Seidel sweeps on k_dp_wave_gs; the register-resident families are template instantiations that pick_sweep picks by
the batch's shape (helpers_dp_shapes.select mirrors that choice).  All batches are synthetic, drawn with fixed seeds."""
import ctypes

import numpy as np
import pytest

import helpers_dp_shapes as H

# ---- host-only checks --------------------------------------------------------------------------------------------------
# forced kernels a batch does not fit: (label, A, sizes, nnz, uniq, sorted, forced, mode, automatic choice)
REFUSALS = [
    ("K2U U=8 A=2", 2, [200, 1, 61], 4, 8, True, H.FORCE_K2U, "VI", ("K2R", (2, 4, 1))),
    ("K2U U=8 spt=4", 4, [600, 1, 61], 4, 8, True, H.FORCE_K2U, "VI", ("K2R", (4, 4, 4))),
    ("K2U unsorted", 3, [200, 1, 61], 4, 5, False, H.FORCE_K2U, "PE", ("K2R", (3, 4, 1))),
    ("K2R K=8 spt=4", 3, [800, 1, 61], 8, 9, True, H.FORCE_K2R, "VI", ("K2", "hbm")),
    ("K2W st_w=8", 3, [480, 1, 61], 4, 5, True, H.FORCE_K2W, "VI", ("K2U", (3, 5, 4, 2))),
    ("K2W U=8", 3, [300, 1, 61], 4, 6, True, H.FORCE_K2W, "VI", ("K2R", (3, 4, 2))),
    ("K2W PE (4, 6)", 4, [384, 1, 61], 4, 5, True, H.FORCE_K2W, "PE", ("K2U", (4, 5, 4, 2))),
    ("K2W VI (4, 7)", 4, [448, 1, 61], 4, 5, True, H.FORCE_K2W, "VI", ("K2U", (4, 5, 4, 2))),
    ("K2W PE (4, 7)", 4, [448, 1, 61], 4, 5, True, H.FORCE_K2W, "PE", ("K2U", (4, 5, 4, 2))),
]

# automatic choice on both sides of every band edge: (A, sizes, nnz, uniq, sorted, expected family and key)
EDGES = [
    (3, [256, 1, 90], 4, 5, True, ("K2U", (3, 5, 4, 1))),
    (3, [257, 1, 90], 4, 5, True, ("K2W", (3, 5))),
    (3, [448, 1, 90], 4, 5, True, ("K2W", (3, 7))),
    (3, [449, 1, 90], 4, 5, True, ("K2U", (3, 5, 4, 2))),
    (3, [512, 1, 90], 4, 5, True, ("K2U", (3, 5, 4, 2))),
    (3, [513, 1, 90], 4, 5, True, ("K2U", (3, 5, 4, 4))),
    (3, [1024, 1, 90], 4, 5, True, ("K2U", (3, 5, 4, 4))),
    (3, [1025, 1, 90], 4, 5, True, ("K2", "hbm")),
    (2, [256, 1, 90], 8, 9, True, ("K2R", (2, 8, 1))),
    (2, [257, 1, 90], 8, 9, True, ("K2R", (2, 8, 2))),
    (2, [512, 1, 90], 8, 9, True, ("K2R", (2, 8, 2))),
    (2, [513, 1, 90], 8, 9, True, ("K2", "lds")),
    (4, [200, 1, 61], 4, 9, True, ("K2R", (4, 4, 1))),
    (4, [200, 1, 61], 5, 9, True, ("K2R", (4, 8, 1))),
    (4, [200, 1, 61], 8, 9, True, ("K2R", (4, 8, 1))),
    (4, [200, 1, 61], 9, 9, True, ("K2", "lds")),
    (4, [200, 1, 61], 4, 5, True, ("K2U", (4, 5, 4, 1))),
    (4, [200, 1, 61], 4, 6, True, ("K2U", (4, 8, 4, 1))),
    (4, [200, 1, 61], 4, 8, True, ("K2U", (4, 8, 4, 1))),
    (4, [200, 1, 61], 4, 9, False, ("K2R", (4, 4, 1))),
    (3, [200, 1, 61], 5, 5, True, ("K2U", (3, 5, 8, 1))),
    (3, [200, 1, 61], 5, 6, True, ("K2U", (3, 8, 8, 1))),
    (3, [200, 1, 61], 4, 5, True, ("K2U", (3, 5, 4, 1))),
    (3, [200, 1, 61], 4, 6, True, ("K2R", (3, 4, 1))),
    (3, [200, 1, 61], 8, 8, True, ("K2U", (3, 8, 8, 1))),
    (3, [200, 1, 61], 8, 9, True, ("K2R", (3, 8, 1))),
]
EDGE_IDS = [f"A{c[0]}-S{c[1][0]}-k{c[2]}-u{c[3]}" + ("" if c[4] else "-unsorted") for c in EDGES]


def test_shape_table_is_the_compiled_list():
    """The test's table of register-resident instantiations is exactly what the shape lists of cmdp_dp_plan.h compile: 47 shapes, 93 kernels."""
    assert H.parse_compiled() == H.compiled_cases()
    assert len(H.compiled_cases()) == 93 and len(H.shapes()) == 47


def test_shape_table_parser_sees_one_deleted_case(tmp_path):
    src = open(H.DP_PLAN_H).read()
    p = tmp_path / "cmdp_dp_plan.h"
    for row, lost in ((" X(4, 8, 4, 2)", {("K2U", (4, 8, 4, 2), "VI"), ("K2U", (4, 8, 4, 2), "PE")}),
                      (" X(4, 6, VI)", {("K2W", (4, 6), "VI")})):
        assert src.count(row) == 1
        p.write_text(src.replace(row, ""))
        assert H.compiled_cases() - H.parse_compiled(str(p)) == lost
        assert H.parse_compiled(str(p)) <= H.compiled_cases()


@pytest.mark.parametrize("fam,key", sorted(H.shapes()))
def test_generator_makes_the_intended_shape(fam, key):
    """The batch of every shape has the intended A, max row nnz, distinct successors and max S, and the selection mirror
    sends it to that instantiation when its family is forced."""
    t = H.shape_batch(fam, key, seed=hash(key) % 1000)
    A, nnz, mu, S, _ = st = H.shape_stats(t)
    assert A == key[0] and len(t["state_off"]) == 4 and 1 in np.diff(t["state_off"])
    if fam == "K2W":
        assert (H.k_round(nnz), H.u_round(mu), -(-S // 64)) == (4, 5, key[1])
    elif fam == "K2U":
        assert (H.u_round(mu), H.k_round(nnz), S) == (key[1], key[2], 256 * key[3]) and mu in (5, 8)
    else:
        assert (nnz, S) == (key[1], 256 * key[2])
    for mode in H.shapes()[fam, key]:
        assert H.select(st, mode, 1, H.FORCE_OF[fam]) == (fam, key)
    assert np.allclose(np.add.reduceat(t["csr_val"].astype(np.float64), t["csr_ptr"][:-1]), 1.0, atol=1e-6)


def test_generator_options():
    t = H.generate(3, [40, 1, 7], 3, 6, seed=1, sorted_rows=False, zeros=True, rewards="neg")
    A, nnz, mu, S, _ = H.shape_stats(t)
    assert (A, nnz, mu, S) == (3, 3, 0, 40)
    assert (t["csr_val"] == 0).any() and (t["csr_val"] < 1e-6).any() and (t["csr_val"] == 1).any()
    assert (t["R"] < 0).all()
    t = H.generate(2, [9], 2, 2, seed=2, rewards="equal")
    assert H.shape_stats(t)[:4] == (2, 2, 2, 9) and (t["R"] == 0.5).all()


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_mirror_predicts_forced_refusals(case):
    _, A, sizes, nnz, uniq, srt, forced, mode, auto = case
    st = H.shape_stats(H.generate(A, sizes, nnz, uniq, seed=3, sorted_rows=srt))
    assert H.select(st, mode, 1, forced)[0] == H.UNSUPPORTED
    assert H.select(st, mode, 1, H.AUTO) == auto


@pytest.mark.parametrize("case", EDGES, ids=EDGE_IDS)
def test_mirror_band_edges(case):
    A, sizes, nnz, uniq, srt, want = case
    st = H.shape_stats(H.generate(A, sizes, nnz, uniq, seed=4, sorted_rows=srt))
    assert st[1] == nnz and st[2] == (uniq if srt and st[3] <= 1024 and nnz <= 8 else 0)
    assert H.select(st, "VI", 1, H.AUTO) == want


def test_mirror_lds_limits():
    """K2 keeps Va, Vb and the reduction slots in LDS (8 S + 64 bytes <= 160 KiB); Gauss-Seidel keeps V (4 S)."""
    st = lambda S: (2, 2, 0, S, 4 * S)  # noqa: E731
    assert H.select(st(20472), "VI", 1) == ("K2", "hbm")
    assert H.select(st(20473), "VI", 1)[0] == H.UNSUPPORTED
    assert H.select(st(40960), "VI", 2) == ("GS", None)
    assert H.select(st(40961), "VI", 2)[0] == H.UNSUPPORTED


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _lib():
    from colosseum_amd import _lib as L

    return L


def _batch(t):
    from colosseum_amd.batched import BatchedMDP

    return BatchedMDP(tables=t, with_env=False)


def _kernel(dp):
    L = _lib()
    v = ctypes.c_double()
    L.check(L.load().cmdp_stat(dp.handle, L.STAT_DP_KERNEL, ctypes.byref(v)))
    return int(v.value)


def _run(dp, mode, gamma, eps, scheme, pis=None, max_sweeps=1_000_000, max_abs=None, out=None):
    if mode == "VI":
        return dp.value_iteration(gamma, eps, scheme, max_sweeps, max_abs, out=out)
    return dp.policy_evaluation(np.concatenate([p.ravel() for p in pis]), gamma, eps, scheme, max_sweeps, out=out)


def _oracle(t, mode, gamma, eps, scheme, pis=None, max_sweeps=1_000_000, max_abs=0.0):
    from oracle import oracle as O

    out = []
    for b in range(int(t["B"])):
        S, A, csr, R = H.instance(t, b)
        if mode == "VI":
            out.append(O.vi_discounted(S, A, csr, R, gamma, eps, scheme, max_sweeps, max_abs)[:3])
        else:
            out.append(O.pe_discounted(S, A, csr, R, pis[b], gamma, eps, scheme, max_sweeps)[:3])
    return out


def _assert_oracle(dp, res, ref, what):
    Q, V, sw = res
    for b, (oQ, oV, oit) in enumerate(ref):
        assert oit > 0, (what, b, oit)
        np.testing.assert_array_equal(dp.split_states(V)[b], oV, err_msg=f"{what} V of instance {b}")
        np.testing.assert_array_equal(dp.split_rows(Q)[b].reshape(oQ.shape), oQ, err_msg=f"{what} Q of instance {b}")
        assert sw[b] == oit, (what, b, int(sw[b]), oit)


def _assert_same(res, ref, what):
    for x, y, name in zip(res, ref, "QVs"):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


def _f64_refs(t, gamma, pis):
    """Per instance: (Q*, V*) and (Q^pi, V^pi) for every named policy, float64."""
    refs = []
    for b in range(int(t["B"])):
        S, A, csr, R = H.instance(t, b)
        r = {"VI": H.vi_f64(S, A, csr, R, gamma)}
        for name, p in pis.items():
            r[name] = H.pe_f64(S, A, csr, R, p[b], gamma)
        refs.append(r)
    return refs


def _assert_f64(dp, res, refs, key, gamma, eps, K, what):
    Q, V, _ = res
    for b, r in enumerate(refs):
        Qr, Vr = r[key]
        vmax = max(np.abs(Vr).max(), np.abs(Qr).max())
        bound = H.f64_bound(gamma, eps, K, vmax)
        dv = np.abs(dp.split_states(V)[b] - Vr).max()
        dq = np.abs(dp.split_rows(Q)[b].reshape(Qr.shape) - Qr).max()
        assert dv <= bound, (what, b, key, dv, bound)
        assert dq <= bound + eps, (what, b, key, dq, bound + eps)


EPS = 1e-5
# (mode, gamma, policy): the float64 check runs at gamma = 0.9
RUNS = [("VI", 0.9, None), ("VI", 0.99, None), ("PE", 0.9, "dirichlet"), ("PE", 0.9, "onehot"), ("PE", 0.99, "dirichlet")]


@pytest.mark.gpu
def test_every_sweep_instantiation_equals_oracle_and_float64(need_gpu):
    """For each of the 47 register-resident shapes one ragged batch (the instance that sets the shape at the top of its
    states-per-lane band, a one-state instance, a mid-size one): the forced family runs the instantiation the mirror
    predicts, equals the oracle (Jacobi) bit for bit in Q, V and sweeps, equals the same batch under K2 and through
    page-locked result buffers, and lies within f64_bound of the float64 solution.  K2 (CSR in LDS and in HBM) and the
    Gauss-Seidel kernel are checked the same way (Gauss-Seidel against the oracle's scheme 2) on every K2R batch.
    Finally: every one of the 93 + 4 + 2 kernels ran."""
    L = _lib()
    ran = set()
    for (fam, key), modes in sorted(H.shapes().items()):
        t = H.shape_batch(fam, key, seed=hash(key) % 1000)
        st = H.shape_stats(t)
        K = st[1]
        pis = {k: H.policies(t, k, seed=11) for k in ("dirichlet", "onehot")}
        refs = _f64_refs(t, 0.9, pis)
        wg = H.select(st, "VI", 1, H.WORKGROUP)
        dp = _batch(t)
        try:
            for mode, gamma, pol in RUNS:
                if mode not in modes:
                    continue
                p = pis.get(pol)
                what = f"{fam}{key} {mode} gamma={gamma} {pol or ''}"
                ref = _oracle(t, mode, gamma, EPS, 1, p)
                dp.set_dp_kernel(H.FORCE_OF[fam])
                res = _run(dp, mode, gamma, EPS, L.SCHEME_JACOBI, p)
                assert _kernel(dp) == H.FAMILY_CODE[fam], what
                _assert_oracle(dp, res, ref, what)
                bufs = dp.dp_buffers()
                for x in bufs:
                    x[...] = -7
                _assert_same(_run(dp, mode, gamma, EPS, L.SCHEME_JACOBI, p, out=bufs), res, what + " page-locked")
                ran.add((fam, key, mode))
                dp.set_dp_kernel(L.DP_WORKGROUP)
                _assert_same(_run(dp, mode, gamma, EPS, L.SCHEME_JACOBI, p), res, what + " vs K2")
                assert _kernel(dp) == 1
                ran.add(("K2", wg[1], mode))
                if gamma == 0.9:
                    _assert_f64(dp, res, refs, pol or "VI", gamma, EPS, K, what)
                if fam == "K2R":
                    ref = _oracle(t, mode, gamma, EPS, 2, p)
                    res = _run(dp, mode, gamma, EPS, L.SCHEME_GAUSS_SEIDEL, p)
                    assert _kernel(dp) == H.FAMILY_CODE["GS"]
                    _assert_oracle(dp, res, ref, what + " Gauss-Seidel")
                    ran.add(("GS", None, mode))
                    if gamma == 0.9:
                        _assert_f64(dp, res, refs, pol or "VI", gamma, EPS, K, what + " Gauss-Seidel")
        finally:
            dp.close()
    assert {c for c in ran if c[0] in ("K2R", "K2U", "K2W")} == H.compiled_cases()
    assert {c for c in ran if c[0] == "K2"} == {("K2", w, m) for w in ("lds", "hbm") for m in ("VI", "PE")}
    assert {c for c in ran if c[0] == "GS"} == {("GS", None, m) for m in ("VI", "PE")}
    assert len(ran) == 93 + 4 + 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGES, ids=EDGE_IDS)
def test_band_edges_choose_the_predicted_kernel(need_gpu, case):
    """On both sides of the states-per-lane, non-zeros-per-row and distinct-successor band edges the automatic choice is
    the mirror's, and VI and PE equal the oracle bit for bit (beyond the register limits that is K2)."""
    L = _lib()
    A, sizes, nnz, uniq, srt, want = case
    t = H.generate(A, sizes, nnz, uniq, seed=4, sorted_rows=srt)
    pis = H.policies(t, "dirichlet", seed=5)
    dp = _batch(t)
    try:
        for mode in ("VI", "PE"):
            res = _run(dp, mode, 0.9, EPS, L.SCHEME_JACOBI, pis)
            fam, key = H.select(H.shape_stats(t), mode, 1)
            assert (fam, key) == want
            assert _kernel(dp) == H.FAMILY_CODE[fam]
            _assert_oracle(dp, res, _oracle(t, mode, 0.9, EPS, 1, pis), f"{case} {mode}")
    finally:
        dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_forced_kernel_refusals(need_gpu, case):
    """A forced family the batch does not fit returns CMDP_ERR_UNSUPPORTED from the host; under DP_AUTO the same batch
    runs on the mirror's choice and equals the oracle."""
    L = _lib()
    _, A, sizes, nnz, uniq, srt, forced, mode, auto = case
    t = H.generate(A, sizes, nnz, uniq, seed=3, sorted_rows=srt)
    pis = H.policies(t, "dirichlet", seed=6)
    dp = _batch(t)
    try:
        dp.set_dp_kernel(forced)
        with pytest.raises(L.CmdpError) as e:
            _run(dp, mode, 0.9, EPS, L.SCHEME_JACOBI, pis)
        assert e.value.code == L.ERR_UNSUPPORTED
        dp.set_dp_kernel(L.DP_AUTO)
        res = _run(dp, mode, 0.9, EPS, L.SCHEME_JACOBI, pis)
        assert _kernel(dp) == H.FAMILY_CODE[auto[0]]
        _assert_oracle(dp, res, _oracle(t, mode, 0.9, EPS, 1, pis), case[0])
    finally:
        dp.close()


@pytest.mark.gpu
def test_lds_limits(need_gpu):
    """K2 Jacobi takes S = 20472 (8 S + 64 bytes = 160 KiB of LDS) and refuses 20473; Gauss-Seidel takes 40960 and refuses
    40961.  The refusals are host-side checks."""
    L = _lib()
    for S, scheme in ((20472, L.SCHEME_JACOBI), (40960, L.SCHEME_GAUSS_SEIDEL)):
        t = H.generate(2, [S, 1], 2, 3, seed=S)
        pis = H.policies(t, "onehot", seed=7)
        dp = _batch(t)
        try:
            for mode in ("VI", "PE"):
                res = _run(dp, mode, 0.9, 1e-3, scheme, pis)
                assert _kernel(dp) == (1 if scheme == L.SCHEME_JACOBI else 6)
                _assert_oracle(dp, res, _oracle(t, mode, 0.9, 1e-3, scheme, pis), f"S={S} {mode}")
        finally:
            dp.close()
        t = H.generate(2, [S + 1, 1], 2, 3, seed=S)
        dp = _batch(t)
        try:
            for mode in ("VI", "PE"):
                with pytest.raises(L.CmdpError) as e:
                    _run(dp, mode, 0.9, 1e-3, scheme, H.policies(t, "onehot", seed=7))
                assert e.value.code == L.ERR_UNSUPPORTED
        finally:
            dp.close()


# one small ragged batch per family: (family, forced option, scheme, generator arguments)
FAMILIES = [
    ("K2R", H.FORCE_K2R, 1, (2, [100, 1, 37], 4, 6, False)),
    ("K2U", H.FORCE_K2U, 1, (3, [200, 1, 50], 4, 5, True)),
    ("K2W", H.FORCE_K2W, 1, (3, [300, 1, 70], 4, 5, True)),
    ("K2", H.WORKGROUP, 1, (4, [150, 1, 40], 8, 9, True)),
    ("GS", H.AUTO, 2, (3, [120, 1, 33], 3, 5, True)),
]


def _family_batch(fam, forced, gen, rewards="unit"):
    A, sizes, nnz, uniq, srt = gen
    t = H.generate(A, sizes, nnz, uniq, seed=len(fam) * 31 + A, sorted_rows=srt, rewards=rewards)
    dp = _batch(t)
    dp.set_dp_kernel(forced)
    return t, dp


@pytest.mark.gpu
@pytest.mark.parametrize("fam,forced,scheme,gen", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_sweep_limit(need_gpu, fam, forced, scheme, gen):
    """max_sweeps = n (the oracle's sweep count) converges in exactly n sweeps, max_sweeps = n - 1 raises
    CMDP_ERR_MAX_ITER; for an odd and an even n (the register kernels run two sweeps per loop trip)."""
    L = _lib()
    t, dp = _family_batch(fam, forced, gen)
    pis = H.policies(t, "dirichlet", seed=8)
    try:
        for mode in ("VI", "PE"):
            parities = set()
            for eps in (1e-2, 7e-3, 5e-3, 3e-3, 2e-3, 1e-3, 7e-4, 5e-4, 3e-4):
                ref = _oracle(t, mode, 0.9, eps, scheme, pis)
                n = max(r[2] for r in ref)
                if n % 2 in parities or n < 3:
                    continue
                parities.add(n % 2)
                res = _run(dp, mode, 0.9, eps, scheme, pis, max_sweeps=n)
                assert _kernel(dp) == H.FAMILY_CODE[fam]
                _assert_oracle(dp, res, ref, f"{fam} {mode} max_sweeps={n}")
                with pytest.raises(L.DynamicProgrammingMaxIterationExceeded):
                    _run(dp, mode, 0.9, eps, scheme, pis, max_sweeps=n - 1)
                assert [r[2] for r in _oracle(t, mode, 0.9, eps, scheme, pis, max_sweeps=n - 1)].count(-5) >= 1
                if len(parities) == 2:
                    break
            assert parities == {0, 1}, (fam, mode)
    finally:
        dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fam,forced,scheme,gen", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_max_abs_value(need_gpu, fam, forced, scheme, gen):
    """Negative rewards: |V|, not V, crosses max_abs_value.  CMDP_ERR_MAX_VALUE when every instance crosses it and when
    only one does; a bound that is not crossed returns the oracle's result."""
    L = _lib()
    t, dp = _family_batch(fam, forced, gen, rewards="neg")
    try:
        off = t["state_off"] * t["A"]
        t["R"][off[0]:off[1]] *= 8.0   # the first instance's values are ~8 times the others'
        dp.close()
        dp = _batch(t)
        dp.set_dp_kernel(forced)
        ref = _oracle(t, "VI", 0.9, EPS, scheme)
        vmax = [float(np.abs(r[1]).max()) for r in ref]
        assert vmax[0] > 2 * max(vmax[1:]) and all(r[2] > 0 for r in ref)
        for bound, crossed in ((0.5 * min(vmax), [True, True, True]), (0.5 * (vmax[0] + max(vmax[1:])), [True, False, False])):
            with pytest.raises(L.CmdpError) as e:
                _run(dp, "VI", 0.9, EPS, scheme, max_abs=bound)
            assert e.value.code == L.ERR_MAX_VALUE
            assert [r[2] == -7 for r in _oracle(t, "VI", 0.9, EPS, scheme, max_abs=bound)] == \
                   [c and v > bound for c, v in zip(crossed, vmax)]
        bound = 1.01 * vmax[0]
        res = _run(dp, "VI", 0.9, EPS, scheme, max_abs=bound)
        assert _kernel(dp) == H.FAMILY_CODE[fam]
        _assert_oracle(dp, res, _oracle(t, "VI", 0.9, EPS, scheme, max_abs=bound), f"{fam} max_abs={bound}")
    finally:
        dp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fam,forced,scheme,gen", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_extreme_gamma(need_gpu, fam, forced, scheme, gen):
    """gamma = 0: Q == R exactly after the oracle's number of sweeps; gamma = 0.999 equals the oracle."""
    t, dp = _family_batch(fam, forced, gen)
    pis = H.policies(t, "onehot", seed=9)
    try:
        for mode in ("VI", "PE"):
            ref = _oracle(t, mode, 0.0, EPS, scheme, pis)
            res = _run(dp, mode, 0.0, EPS, scheme, pis)
            assert _kernel(dp) == H.FAMILY_CODE[fam]
            _assert_oracle(dp, res, ref, f"{fam} {mode} gamma=0")
            np.testing.assert_array_equal(res[0], t["R"])
            ref = _oracle(t, mode, 0.999, 1e-3, scheme, pis)
            _assert_oracle(dp, _run(dp, mode, 0.999, 1e-3, scheme, pis), ref, f"{fam} {mode} gamma=0.999")
    finally:
        dp.close()


# ---- discounted_policy_iteration ---------------------------------------------------------------------------------------
def _dense(S, A, succ, seed):
    """T [S, A, S] float32 with `succ` successors per row (Dirichlet), R [S, A] in [0, 1)."""
    rng = np.random.default_rng(seed)
    T = np.zeros((S, A, S), np.float32)
    for s in range(S):
        for a in range(A):
            c = rng.choice(S, size=succ, replace=False)
            T[s, a, c] = rng.dirichlet(np.ones(succ))
    return T, rng.random((S, A)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("S,A,succ", [(20, 2, 20), (120, 3, 9), (300, 4, 5)])
def test_discounted_policy_iteration(need_gpu, monkeypatch, S, A, succ):
    """The drop-in's policy iteration against a host loop with the reference's semantics (seeded np.random.rand start,
    argmax_2d, oracle policy evaluation under discounted_policy_evaluation's scheme rule): the same policies in the same
    order, the same final Q, V and pi; the final V within f64_bound of V*, pi greedy for the float64 Q* wherever the top
    two actions are further apart than twice the Q bound."""
    from colosseum_amd import dynamic_programming as DP
    from colosseum_amd.dp_handle import csr_from_dense
    from oracle import oracle as O

    gamma, eps = 0.9, 1e-5
    T, R = _dense(S, A, succ, seed=S)
    seen = []
    pe = DP.discounted_policy_evaluation

    def spy(T_, R_, pi, gamma_, epsilon_):
        seen.append(np.array(pi, np.float32))
        return pe(T_, R_, pi, gamma_, epsilon_)

    monkeypatch.setattr(DP, "discounted_policy_evaluation", spy)
    np.random.seed(1234 + S)
    Q, V, pi = DP.discounted_policy_iteration(T, R, gamma, eps)

    csr = csr_from_dense(T)
    scheme = 1 if (S > 200 and len(csr[1]) / T.size < 0.2) else 2
    np.random.seed(1234 + S)
    hpi = DP.argmax_2d(np.random.rand(S, A))
    hist = []
    while True:
        hist.append(hpi)
        hQ, hV, it, _ = O.pe_discounted(S, A, csr, R, hpi, gamma, eps, scheme)
        assert it > 0
        new = DP.argmax_2d(hQ)
        if (new != hpi).sum() == 0:
            break
        hpi = new
    assert len(seen) == len(hist) >= 2
    for a, b in zip(seen, hist):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(Q, hQ)
    np.testing.assert_array_equal(V, hV)
    np.testing.assert_array_equal(pi, new)

    Qs, Vs = H.vi_f64(S, A, csr, R, gamma)
    bound = H.f64_bound(gamma, eps, int(np.diff(csr[0]).max()), max(np.abs(Vs).max(), np.abs(Qs).max()))
    assert np.abs(V - Vs).max() <= bound
    top2 = np.sort(Qs, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 2 * (bound + eps)
    assert clear.mean() > 0.5
    np.testing.assert_array_equal(pi.argmax(1)[clear], Qs.argmax(1)[clear])
