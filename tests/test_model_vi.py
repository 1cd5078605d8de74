"""Value iteration on models in the row form (kernel K14), what needs no device: the scheme rule against the oracle's, the
argument checks of cmdp_vi_discounted_model, the Python packer, and the generated fixtures of tests/test_gpu_model_vi.py
(the oracle converges on each; the AUTO-edge batch falls where it is meant to)."""
import numpy as np
import pytest

import helpers_model_vi as H
from colosseum_amd import _lib as L
from colosseum_amd import dynamic_programming as dp
from oracle import oracle as O


def test_scheme_rule_equals_the_oracles_at_the_default_thresholds():
    lib, ol = L.load(), O.lib()
    shapes = [(1, 1), (2, 5), (63, 64), (64, 2), (65, 5), (257, 1), (257, 64), (299, 3), (300, 3), (301, 3), (300, 4), (4096, 64),
              (519, 1), (520, 1), (150, 12)]   # 300 * 3 * 300 and 150 * 12 * 150 equal the threshold; 301 * 3 * 301 and 520^2 exceed it
    n = 0
    for S, A in shapes:
        size = S * A * S
        fifth = size // 5   # nnz / size is exactly 0.2 where 5 divides size
        for nnz in {0, 1, S, S * A, fifth - 1, fifth, fifth + 1, size // 2, size - 1, size}:
            if nnz < 0:
                continue
            got = lib.cmdp_model_vi_scheme(S, A, nnz, H.SIZE_THRESHOLD, H.DENSITY_THRESHOLD)
            assert got == ol.oracle_vi_scheme_rule(S, A, nnz), (S, A, nnz)
            assert got == dp._vi_rule(size, nnz, H.SIZE_THRESHOLD, H.DENSITY_THRESHOLD), (S, A, nnz)
            n += 1
    assert lib.cmdp_model_vi_scheme(300, 3, 10, H.SIZE_THRESHOLD, 0.2) == L.SCHEME_GAUSS_SEIDEL   # equal to the threshold
    assert lib.cmdp_model_vi_scheme(150, 12, 150 * 12 * 150 // 5 - 1, H.SIZE_THRESHOLD, 0.2) == L.SCHEME_GAUSS_SEIDEL
    assert lib.cmdp_model_vi_scheme(520, 1, 520 * 520 // 5 - 1, H.SIZE_THRESHOLD, 0.2) == L.SCHEME_JACOBI     # one above: 270 400
    assert lib.cmdp_model_vi_scheme(520, 1, 520 * 520 // 5, H.SIZE_THRESHOLD, 0.2) == L.SCHEME_GAUSS_SEIDEL   # density exactly 0.2
    assert n > 100


def test_scheme_rule_with_custom_thresholds_equals_the_python_rule():
    lib = L.load()
    rng = np.random.default_rng(5)
    for _ in range(500):
        S, A = int(rng.integers(1, 200)), int(rng.integers(1, 20))
        size = S * A * S
        thr = int(rng.choice([0, size - 1, size, size + 1, int(rng.integers(0, 2 * size + 2))]))
        dens = float(rng.choice([0.0, 0.2, 0.25, 0.5, 1.0, 1.5, float(rng.random())]))
        nnz = int(rng.choice([0, size, int(size * dens), int(size * dens) + 1, max(0, int(size * dens) - 1), int(rng.integers(0, size + 1))]))
        assert lib.cmdp_model_vi_scheme(S, A, nnz, thr, dens) == dp._vi_rule(size, nnz, thr, dens), (S, A, nnz, thr, dens)


def test_argument_checks_without_a_device():
    fx = H.make_fixture(3, 2, "state_0", 1)
    args = H.pack([fx])

    def call(count=1, **kw):
        a = dict(args, **{k: v for k, v in kw.items() if k in args})
        rest = {k: v for k, v in kw.items() if k not in args}
        rest.setdefault("out", dict(Q=np.zeros(6, np.float32), V=np.zeros(3, np.float32), sweeps=np.zeros(1, np.int64),
                                    scheme=np.zeros(1, np.int32), status=np.zeros(1, np.int32)))
        rc, msg, _ = H.call_raw(a, count, **rest)
        return rc, msg

    def invalid(word, **kw):
        rc, msg = call(**kw)
        assert rc == L.ERR_INVALID and word in msg, (kw, rc, msg)

    lib = L.load()
    assert lib.cmdp_vi_discounted_model(0, *[None] * 7, 0.99, 1e-3, 0, 0, 0.2, 10, *[None] * 5) == L.OK
    assert call(count=-1) == (L.ERR_INVALID, "count -1 is negative")
    for k in ("n_states", "n_actions", "ptr", "R"):
        invalid("null argument", **{k: None})
    for k in ("Q", "V", "sweeps", "scheme", "status"):
        out = dict(Q=np.zeros(6, np.float32), V=np.zeros(3, np.float32), sweeps=np.zeros(1, np.int64),
                   scheme=np.zeros(1, np.int32), status=np.zeros(1, np.int32))
        out[k] = None
        invalid("null argument", out=out)
    invalid("n_states[0]", n_states=np.array([0], np.int32))
    invalid("n_actions[0]", n_actions=np.array([0], np.int32))
    # the row form itself (csr_ptr, csr_col, csr_val, rewards, uniform): tests/test_row_form.py, shared with kernel K10
    for v in (np.inf, np.nan):
        invalid("gamma", gamma=v)
        invalid("epsilon", eps=v)
    invalid("epsilon", eps=-1.0)
    invalid("max_sweeps", max_sweeps=0)
    invalid("scheme 3", scheme=3)
    invalid("scheme -1", scheme=-1)
    for k, n, word in (("n_states", 4097, "4096"), ("n_actions", 65, "64")):
        big = dict(args, **{k: np.array([n], np.int32)})
        rows = int(big["n_states"][0]) * int(big["n_actions"][0])
        big.update(ptr=np.zeros(rows + 1, np.int64), uni=np.full(rows, 0.5, np.float32), R=np.zeros(rows, np.float32))
        rc, msg, _ = H.call_raw(big, 1)
        assert rc == L.ERR_UNSUPPORTED and word in msg, msg


def test_python_packer():
    for mix in H.MIXES:
        fx = H.make_fixture(7, 3, mix, 3)
        T, R = fx.dense()
        S, A, ptr, col, val, uni, Rr, nnz = dp._vi_problem(T, R)
        assert (S, A) == (7, 3) and nnz == np.count_nonzero(T) == fx.nnz
        T2 = T.reshape(21, 7)
        full = (T2[:, :1] == T2).all(axis=1) & (T2[:, 0] > 0)
        assert np.array_equal(uni > 0, full) and np.array_equal(uni[full], T2[full, 0])
        assert ((np.diff(ptr) == 0) | ~full).all() and (val > 0).all() and len(col) == ptr[-1] == nnz - 7 * full.sum()
        back = np.zeros_like(T2)
        back[np.repeat(np.arange(21), np.diff(ptr)), col] = val
        back[full] = uni[full, None]
        assert np.array_equal(back, T2) and np.array_equal(Rr, R.ravel())
        for r in range(21):
            assert (np.diff(col[ptr[r]:ptr[r + 1]]) > 0).all()
    T, R = H.make_fixture(4, 2, "no_uniform", 1).dense()
    for bad in ((T[:, :, :3], R), (T[0], R), (T, R[:, :1]), (T, R.ravel()), (-T, R), (np.zeros((0, 2, 0), np.float32), R),
                (np.where(T > 0, np.nan, T), R)):
        with pytest.raises(ValueError):
            dp._vi_problem(*bad)
    for kw in (dict(epsilon=-1), dict(epsilon=np.nan), dict(max_sweeps=0), dict(scheme=3)):
        with pytest.raises(ValueError):
            dp.discounted_value_iteration_batch([(T, R)], **kw)
    assert dp.discounted_value_iteration_batch([])[0] == []
    # the packer the extended solver shares with it
    p = dp._evi_problem(T, R, np.zeros_like(R), np.zeros(R.shape + (1,)), 1.0)
    q = dp._vi_problem(T, R)
    for i in range(7):
        assert np.array_equal(p[i], q[i])


def test_the_oracle_converges_on_every_fixture():
    g = H.grid()
    assert len(g) == len(H.STATES) * len(H.ACTIONS) * len(H.MIXES)
    assert {gm for _, gm in g} == set(H.GAMMAS)
    seen = set()
    for fx, gamma in g:
        for scheme in (L.SCHEME_JACOBI, L.SCHEME_GAUSS_SEIDEL):
            Q, V, it = fx.reference(gamma, scheme)
            assert it >= 1 and np.isfinite(Q).all() and np.isfinite(V).all(), (fx.name, gamma, scheme, it)
            assert not np.signbit(Q[Q == 0]).any()   # no -0: the kernel's wave maximum and fmaxf then agree
        seen.add((fx.rule(), gamma))
    # under AUTO at the default thresholds the grid reaches both schemes
    assert {s for s, _ in seen} == {L.SCHEME_JACOBI, L.SCHEME_GAUSS_SEIDEL}
    # the row form says what the dense CSR says: a full row given as CSR has its entries in val, a uniform row counts S
    for fx, _ in g:
        assert int((fx.val > 0).sum()) + fx.S * int((fx.uni > 0).sum()) == fx.nnz, fx.name


def test_the_auto_edge_batch_falls_on_both_sides_of_both_edges():
    lib = L.load()
    thr, dens = H.EDGE_THRESHOLDS
    batch = H.edge_batch()
    got = []
    for fx, meant in batch:
        assert fx.rule(thr, dens) == meant, fx.name
        assert lib.cmdp_model_vi_scheme(fx.S, fx.A, fx.nnz, thr, dens) == meant, fx.name
        assert fx.reference(0.99, meant)[2] >= 1
        got.append((fx.S * fx.A * fx.S > thr, fx.nnz / (fx.S * fx.A * fx.S) < dens))
    assert set(got) == {(False, True), (True, True), (True, False)}
    assert any(fx.S * fx.A * fx.S == thr for fx, _ in batch) and any(fx.nnz / (fx.S * fx.A * fx.S) == dens for fx, _ in batch)
    assert len({fx.S for fx, _ in batch}) > 2
