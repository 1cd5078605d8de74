"""Every compiled continuous-diameter kernel on generated communicating MDPs: bit for bit against the oracle, within the
derived float32 tolerance of a float64 restatement of the reference's per-target value iteration, and -- through
CMDP_STAT_DIAMETER_KERNEL -- on the template instantiation the host mirror predicts.

k_dp_block<DP_VI, true, .> (CSR in LDS / HBM) and k_dp_wave_gs<DP_VI, true> take the automatic path; the lanes kernels
k_diam_lanes<8>, k_diam_lanes_ell<NW, A, K>, k_diam_tiles<., A, K, .> and k_diam_cluster<CL, A, K, XCD> are reached through
CMDP_OPT_DP_KERNEL, CMDP_OPT_DIAMETER_RELABEL_MIN_STATES and the CMDP_K5C / CMDP_K5S_NW / CMDP_K5C_SCOPE switches, the last
two in child processes because the library reads them once.  helpers_diam has the generator, the references and the mirror."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers_diam as D
import helpers_dp_shapes as H

SHAPE_IDS = [f"A{a}-K{k}" for a, k in D.SHAPES]
EPS = D.EPS


# ---- host-only checks --------------------------------------------------------------------------------------------------
def test_fixed_width_table_is_the_compiled_list(tmp_path):
    """The nine (A, K) pairs of the tests are CMDP_FIXED_WIDTH_SHAPES, and the parser sees one deleted X(P, a, k)."""
    assert D.parse_fixed_width() == D.SHAPES and len(D.SHAPES) == 9
    assert len(D.all_kernels()) == 27 + 54 + 9 + 1 + 2 + 1
    src = open(D.DP_PLAN_H).read()
    p = tmp_path / "cmdp_dp_plan.h"
    for row, lost in ((" X(P, 3, 8)", (3, 8)), (" X(P, 4, 2)", (4, 2))):
        assert src.count(row) == 1
        p.write_text(src.replace(row, ""))
        assert D.parse_fixed_width(str(p)) == [s for s in D.SHAPES if s != lost]


def _row_view(t):
    ptr, col, val = t["csr_ptr"], t["csr_col"], t["csr_val"]
    return ptr, col, val, np.diff(ptr)


@pytest.mark.parametrize("shape", D.SHAPES, ids=SHAPE_IDS)
def test_shape_batch_has_the_intended_properties(shape):
    A, K = shape
    U = D.chunk_states(A, K)
    for key, sizes, nnz in ((("shape", A, K), D.shape_sizes(A, K), D.NNZ[shape]), (("wide", A, K), D.wide_sizes(), D.WIDE_NNZ[shape])):
        t = D.batch(key)
        ptr, col, val, row_nnz = _row_view(t)
        st = H.shape_stats(t)
        assert (st[0], st[1], D.fixed_width_K(st[1])) == (A, nnz, K)
        assert np.diff(t["state_off"]).tolist() == sizes and int(t["H"]) == 0
        assert (row_nnz < nnz).any() and (row_nnz == 1).any() and (row_nnz >= 1).all()
        assert val[val > 0].min() >= np.float32(0.05)
        assert np.allclose(np.add.reduceat(val.astype(np.float64), ptr[:-1]), 1.0, atol=1e-6)
        same_row = np.ones(len(col), bool)
        same_row[ptr[:-1]] = False
        assert np.all(np.diff(col)[same_row[1:]] > 0), "columns ascend within every row"
        self_loops = ring_not_first = ring_sure = 0
        ring_actions = set()
        for b in range(int(t["B"])):
            S, _, (lp, c, v), _ = H.instance(t, b)
            assert D.strongly_connected(S, A, (lp, c, v)), (key, b)
            state = np.repeat(np.arange(S * A) // A, np.diff(lp))
            first = np.zeros(len(c), bool)
            first[lp[:-1]] = True
            ring = (c == (state + 1) % S) & (v > 0)
            assert len(np.unique(state[ring])) == S, "every state has a ring edge"
            self_loops += int(((c == state) & (S > 1)).sum())
            ring_not_first += int((ring & ~first).sum())
            ring_sure += int((ring & (v == 1)).sum())
            ring_actions |= set((np.repeat(np.arange(S * A), np.diff(lp))[ring] % A).tolist())
        assert self_loops and ring_not_first and ring_sure
        assert ring_actions == set(range(A)), "which action carries the ring edge varies: every action does somewhere"
    sizes = D.shape_sizes(A, K)
    assert {1, 2, 64, 65} <= set(sizes) and max(sizes) == 333 and sizes[-1] == 3 and sizes.index(333) < len(sizes) - 1
    assert all(333 % u for u in (U, 64) if u > 1) and (U <= 2 or any(2 < s < U for s in sizes))
    assert len(D.launch_groups(sizes)) == 1 and len(D.launch_groups(sizes, 1)) >= 2 and sum(D.launch_groups(sizes)) <= D.CUS
    assert sum(D.launch_groups(D.wide_sizes())) > D.CUS and len(D.launch_groups(D.wide_sizes())) == 1


def test_every_row_width_occurs():
    assert set(D.NNZ.values()) | set(D.WIDE_NNZ.values()) == set(range(2, 9))
    assert all(D.fixed_width_K(D.NNZ[s]) == s[1] == D.fixed_width_K(D.WIDE_NNZ[s]) for s in D.SHAPES)
    assert (D.batch(("shape", 3, 4))["csr_val"] == 0).any(), "explicit zeros occur"


ALL_BATCHES = [("shape",) + s for s in D.SHAPES] + [("wide",) + s for s in D.SHAPES] + ["hbm", "A5", "nnz9", "limit"]


@pytest.mark.parametrize("key", ALL_BATCHES, ids=str)
def test_every_target_converges_within_5000_float64_sweeps(key):
    """The condition on the inputs: at eps = 1e-3 every target of every generated batch converges in the float64
    restatement within 5 000 sweeps (the reference asserts it while it is built)."""
    D.reference(key)
    assert 1 <= D.SWEEPS64[key, 1, EPS] <= 5000, key


def test_jacobi_f64_agrees_with_exact_hitting_times():
    """The restatement run to eps = 1e-10 against float64 policy iteration with a linear solve per policy: 1e-7 relative
    on every target of two batches."""
    for key in ("A5", "limit"):
        t = D.batch(key)
        for b in range(int(t["B"])):
            S, A, csr, _ = H.instance(t, b)
            traj = D.jacobi_f64(S, A, csr, np.arange(S), 1e-10, 100_000, stop=1.0)
            for scheme2 in ([2] if S <= 70 else []):
                gs = D.jacobi_f64(S, A, csr, np.arange(S), 1e-10, 100_000, scheme=scheme2, stop=1.0)
                np.testing.assert_allclose(gs["r"][-1], traj["r"][-1], rtol=1e-7)
            exact = np.array([D.hitting_f64(S, A, csr, j).max() for j in range(S)])
            np.testing.assert_allclose(traj["r"][-1], exact, rtol=1e-7, atol=0)


@pytest.mark.parametrize("shape", D.SHAPES, ids=SHAPE_IDS)
def test_oracle_alone_passes_the_float64_check(shape):
    """The tolerance accepts a correct float32 implementation: the oracle's Jacobi and Gauss-Seidel results of every
    shape batch lie in an admissible interval, target by target."""
    key = ("shape",) + shape
    for scheme in (1, 2):
        per = np.concatenate([p for _, p in D.oracle(key, scheme)])
        _, E, err, _ = D.check_f64(key, per, scheme)
        assert err <= E


def _jacobi_f32(S, A, csr, target, eps, drop_row=None, absorb=None):
    """The per-target solve in float32 numpy, every product and sum rounded separately and in entry order, as the kernels
    and the oracle run it.  drop_row: that row's last entry is left out; absorb: the state given the absorbing row."""
    ptr, col, val = csr
    absorb = target if absorb is None else absorb
    kmax = int(np.diff(ptr).max())
    pc = np.zeros((S * A, kmax), np.int64)
    pv = np.zeros((S * A, kmax), np.float32)
    for k in range(kmax):
        has = np.diff(ptr) > k
        pc[has, k] = col[ptr[:-1][has] + k]
        pv[has, k] = val[ptr[:-1][has] + k]
    if drop_row is not None:
        pv[drop_row, ptr[drop_row + 1] - ptr[drop_row] - 1] = 0.0   # acc + 0 * V == acc: the entry is gone
    V = np.zeros(S, np.float32)
    for _ in range(5000):
        acc = np.zeros(S * A, np.float32)
        for k in range(kmax):
            acc = acc + pv[:, k] * V[pc[:, k]]
        q = (np.float32(-1.0) + np.float32(1.0) * acc).reshape(S, A)
        Vn = q.max(1)
        Vn[absorb] = V[absorb]
        diff = np.abs(V - Vn).max()
        V = Vn
        if float(diff) < eps:
            return -V.min(), V, q
    raise AssertionError("no convergence")


def test_admissible_rejects_planted_errors():
    """Two targets of a 65-state instance solved by float32 Jacobi in numpy: the unplanted solve equals the oracle bit for
    bit and is accepted; with the last entry of one row dropped (the greedy row of the state farthest from the target),
    and with the absorbing row given to the target's neighbour, the value lies in no admissible interval."""
    key = ("shape", 3, 4)
    t = D.batch(key)
    b = D.shape_sizes(3, 4).index(65)
    S, A, csr, _ = H.instance(t, b)
    ptr, col, val = csr
    planted = 0
    for target in range(S):
        iv = D.reference(key)[b][target]
        good, V, q = _jacobi_f32(S, A, csr, target, EPS)
        assert good == D.oracle(key)[b][1][target] and D.accepts(iv, good)
        s = int(V.argmin())   # the state farthest from the target, and the row it follows
        row = s * A + int(q[s].argmax())
        last = int(ptr[row + 1]) - 1
        if not (ptr[row + 1] - ptr[row] >= 2 and val[last] > 0 and col[last] != target):
            continue   # a one-entry row, or the entry would be an explicit zero or lead to the target
        planted += 1
        dropped = _jacobi_f32(S, A, csr, target, EPS, drop_row=row)[0]
        moved = _jacobi_f32(S, A, csr, target, EPS, absorb=(target + 1) % S)[0]
        assert not D.accepts(iv, dropped), (target, good, dropped)
        assert not D.accepts(iv, moved), (target, good, moved)
        if planted == 2:
            break
    assert planted == 2


def test_mirror_of_the_kernel_choice():
    st = H.shape_stats(D.batch(("shape", 3, 4)))
    assert D.select_diam(st, 1) == D.code(D.K2, 0, 1) and D.select_diam(st, 2) == D.code(D.K3)
    assert D.select_diam(H.shape_stats(D.batch("hbm")), 1) == D.code(D.K2, 0, 0)
    assert D.select_diam(st, 2, D.OPT_K5S) == D.code(D.K3), "the lanes kernels are Jacobi only"
    assert D.select_diam(st, 1, D.OPT_K5S, n_groups=256) == D.code(D.K5S_ELL, 16)
    assert D.select_diam(st, 1, D.OPT_K5S, n_groups=257) == D.code(D.K5S_ELL, 8)
    assert D.select_diam(st, 1, D.OPT_K5S, n_groups=257, env={"CMDP_K5S_NW": "4"}) == D.code(D.K5S_ELL, 4)
    assert D.select_diam(st, 1, D.OPT_K5S, relabel=True, n_groups=257, env={"CMDP_K5C": "0"}) == D.code(D.K5S_ELL, 16)
    assert D.select_diam(st, 1, D.OPT_K5S, relabel=True) == D.code(D.K5C, 16, 1)
    assert D.select_diam(st, 1, D.OPT_K5S, relabel=True, env={"CMDP_K5C": "32", "CMDP_K5C_SCOPE": "agent"}) == D.code(D.K5C, 32, 0)
    assert D.select_diam(st, 1, D.OPT_K5S, relabel=True, cus=304) == D.code(D.K5S_ELL, 16), "304 CUs are no multiple of 128"
    assert D.select_diam(st, 1, D.OPT_K5S_CSR, relabel=True) == D.code(D.K5S_CSR, 8)
    assert D.select_diam(st, 1, D.OPT_K5T, relabel=True) == D.code(D.K5T, 6)
    for key in ("A5", "nnz9"):
        for forced in (D.OPT_K5S, D.OPT_K5S_CSR, D.OPT_K5T):
            assert D.select_diam(H.shape_stats(D.batch(key)), 1, forced, relabel=True) == D.code(D.K5S_CSR, 8)
    assert D.select_diam((2, 2, 0, 20473, 4 * 20473), 1) == D.code(D.K5S_ELL, 16), "beyond the LDS of K2: the lanes kernels"
    assert D.launch_groups([2, 333, 1, 65], 1) == [8, 2] and D.launch_groups([65, 3], 1, 3, 66) == [2]


def _largest_sweep_count(key, eps):
    """The largest per-target sweep count of a batch: the oracle fails below it (bisection over its max_sweeps)."""
    lo, hi = 0, 5000
    while hi - lo > 1:
        mid = (lo + hi) // 2
        try:
            D.oracle(key, 1, eps, mid)
            hi = mid
        except RuntimeError as e:
            assert str(e) == "oracle diameter failed (-5)", e   # the sweep limit and nothing else steers the search
            lo = mid
    return hi


LIMIT_EPS = (1e-3, 2e-3)   # an odd and an even largest sweep count on the "limit" batch


def test_sweep_limit_cases_have_both_parities():
    n = [_largest_sweep_count("limit", e) for e in LIMIT_EPS]
    assert n[0] % 2 == 1 and n[1] % 2 == 0, n


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _lib():
    from colosseum_amd import _lib as L

    return L


def _handle(key):
    from colosseum_amd.batched import BatchedMDP

    return BatchedMDP(tables=D.batch(key), with_env=False)


def _stat(dp, which):
    L = _lib()
    v = ctypes.c_double()
    L.check(L.load().cmdp_stat(dp.handle, which, ctypes.byref(v)))
    return int(v.value)


class _Env:
    """CMDP_* switches the library reads per call: set for the block, restored after it."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)


def _switches():
    return {k: v for k, v in os.environ.items() if k in ("CMDP_K5C", "CMDP_K5S_NW", "CMDP_K5C_SCOPE")}


FINDINGS = {}   # ((A, K) or batch name, scheme) -> the four figures of helpers_diam.check_f64, the largest over the calls


def check_call(dp, key, forced=D.OPT_AUTO, scheme=1, relabel=False, ws_mb=24576):
    """One cmdp_diameter of the handle's current options on batch `key`: per_target and diameter bit-equal to the oracle's
    scheme per instance, every per_target value in an admissible interval of the float64 trajectory, and the statistic
    equal to the mirror's prediction.  Returns the kernel that ran."""
    L = _lib()
    t = D.batch(key)
    st = H.shape_stats(t)
    sizes = np.diff(t["state_off"])
    diam, per = dp.diameter(EPS, scheme)
    for b, (od, oper) in enumerate(D.oracle(key, scheme)):
        np.testing.assert_array_equal(dp.split_states(per)[b], oper, err_msg=f"{key} instance {b}")
        assert diam[b] == np.float32(od), (key, b)
    f = D.check_f64(key, per, scheme)
    name = key[1:] if isinstance(key, tuple) else key
    FINDINGS[name, scheme] = [max(x, y) for x, y in zip(FINDINGS.get((name, scheme), (0, 0.0, 0.0, 0.0)), f)]
    got = _stat(dp, L.STAT_DIAMETER_KERNEL)
    want = D.select_diam(st, scheme, forced, relabel, D.launch_groups(sizes, ws_mb)[-1], env=_switches())
    assert got == want, (key, forced, scheme, relabel, got, want, f"the mirror and the batches assume {D.CUS} compute units")
    return D.kernel_id(got, st[0], D.fixed_width_K(st[1]))


def _check_ranges(dp, key, relabel):
    """Target ranges whose cuts split a group and an instance reassemble to the oracle's full vector."""
    L = _lib()
    t = D.batch(key)
    sizes = np.diff(t["state_off"])
    full = np.concatenate([p for _, p in D.oracle(key)])
    n = len(full)
    cuts = sorted({0, 1, 70, int(t["state_off"][2]) - 30, n // 2, n - 2, n})
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.append(dp.diameter_range(a, b, EPS))
        want = D.select_diam(H.shape_stats(t), 1, D.OPT_K5S, relabel, D.launch_groups(sizes, lo=a, hi=b)[-1], env=_switches())
        assert _stat(dp, L.STAT_DIAMETER_KERNEL) == want, (key, a, b)
    np.testing.assert_array_equal(np.concatenate(parts), full)


RECORD = {}   # what ran in this process -> ("ok", the kernels seen) or ("failed", the exception): every outcome, once


def recorded(fn):
    """Runs fn(*args) at most once per process and keeps the outcome, a failure included: a second call returns the
    stored set or raises the stored exception again.  What has failed -- or faulted, or hung -- is never started twice."""
    @functools.wraps(fn)
    def once(*args):
        name = (fn.__name__,) + args
        if name not in RECORD:
            RECORD[name] = ("failed", RuntimeError(f"{name} was interrupted"))   # (stays if something other than an Exception ends it)
            try:
                RECORD[name] = ("ok", fn(*args))
            except Exception as e:
                RECORD[name] = ("failed", e)
        state, result = RECORD[name]
        if state == "failed":
            raise result
        return result
    return once


@recorded
def run_path(path, A, K):
    """All calls of one path on the batches of shape (A, K); returns the set of kernels that ran."""
    L = _lib()
    key = ("wide" if path == "wide" else "shape", A, K)
    ran = set()
    dp = _handle(key)
    try:
        if path == "auto":      # one workgroup per target (CSR in LDS), one wavefront per target (Gauss-Seidel)
            ran.add(check_call(dp, key))
            ran.add(check_call(dp, key, scheme=2))
        elif path == "ell":     # K5S with fixed-width rows, 16 wavefronts per group
            dp.set_option(L.OPT_DP_KERNEL, D.OPT_K5S)
            ran.add(check_call(dp, key, D.OPT_K5S))
            dp.set_option(L.OPT_DIAMETER_WORKSPACE_MB, 1)   # several launches
            assert len(D.launch_groups(D.shape_sizes(A, K), 1)) >= 2
            ran.add(check_call(dp, key, D.OPT_K5S, ws_mb=1))
            dp.set_option(L.OPT_DIAMETER_WORKSPACE_MB, 24576)
            dp.set_option(L.OPT_DIAMETER_RELABEL_MIN_STATES, 1)   # rows in the locality order, targets through new_of
            with _Env(CMDP_K5C="0"):
                ran.add(check_call(dp, key, D.OPT_K5S, relabel=True))
                if (A, K) == (3, 4):
                    _check_ranges(dp, key, True)
        elif path == "wide":    # more groups than compute units in one launch: 8 wavefronts per group
            dp.set_option(L.OPT_DP_KERNEL, D.OPT_K5S)
            ran.add(check_call(dp, key, D.OPT_K5S))
        elif path == "csr":
            dp.set_option(L.OPT_DP_KERNEL, D.OPT_K5S_CSR)
            ran.add(check_call(dp, key, D.OPT_K5S_CSR))
        elif path == "k5t":
            dp.set_option(L.OPT_DP_KERNEL, D.OPT_K5T)
            ran.add(check_call(dp, key, D.OPT_K5T))
        elif path == "k5c":     # clusters of 8, 16 and 32 workgroups per group
            dp.set_option(L.OPT_DP_KERNEL, D.OPT_K5S)
            dp.set_option(L.OPT_DIAMETER_RELABEL_MIN_STATES, 1)
            for cl in (8, 16, 32):
                with _Env(CMDP_K5C=str(cl)):
                    before = _stat(dp, L.STAT_DIAMETER_CLUSTER_LAUNCHES)
                    ran.add(check_call(dp, key, D.OPT_K5S, relabel=True))
                    assert _stat(dp, L.STAT_DIAMETER_CLUSTER_LAUNCHES) == before + 1
                    assert _stat(dp, L.STAT_DIAMETER_CLUSTER_FALLBACKS) == 0
                    if (A, K, cl) == (2, 2, 16):
                        _check_ranges(dp, key, True)
        else:
            raise ValueError(path)
    finally:
        dp.close()
    return frozenset(ran)


def _scope():
    return "agent" if os.environ.get("CMDP_K5C_SCOPE") == "agent" else "xcd"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", D.SHAPES, ids=SHAPE_IDS)
def test_automatic_path_and_gauss_seidel(need_gpu, shape):
    assert run_path("auto", *shape) == {("K2", "lds"), ("K3",)}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", D.SHAPES, ids=SHAPE_IDS)
def test_fixed_width_lanes_kernel(need_gpu, shape):
    """K5S-ELL with 16 wavefronts per group: one launch, several launches, relabelled rows (and target ranges)."""
    assert run_path("ell", *shape) == {("K5S-ELL", 16) + shape}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", D.SHAPES, ids=SHAPE_IDS)
def test_fixed_width_lanes_kernel_with_more_groups_than_compute_units(need_gpu, shape):
    assert run_path("wide", *shape) == {("K5S-ELL", 8) + shape}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", D.SHAPES, ids=SHAPE_IDS)
def test_generic_csr_walker(need_gpu, shape):
    assert run_path("csr", *shape) == {("K5S-CSR", 8)}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", D.SHAPES, ids=SHAPE_IDS)
def test_tiled_kernel(need_gpu, shape):
    """K5T.  build_tiles refuses only a state with more than 47 distinct successors, which no fixed-width shape has
    (A * K <= 32): every batch of a compiled shape, one-state instances included, is taken."""
    assert run_path("k5t", *shape) == {("K5T", 6) + shape}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", D.SHAPES, ids=SHAPE_IDS)
def test_cluster_kernel(need_gpu, shape):
    assert run_path("k5c", *shape) == {("K5C", cl) + shape + (_scope(),) for cl in (8, 16, 32)}


@recorded
def run_extras():
    L = _lib()
    ran = set()
    dp = _handle("hbm")
    try:
        ran.add(check_call(dp, "hbm"))
    finally:
        dp.close()
    for key in ("A5", "nnz9"):   # no fixed-width shape fits: options 3, 4 and 6 all take the generic walker
        dp = _handle(key)
        try:
            for forced in (D.OPT_K5S_CSR, D.OPT_K5S, D.OPT_K5T):
                dp.set_option(L.OPT_DP_KERNEL, forced)
                dp.set_option(L.OPT_DIAMETER_RELABEL_MIN_STATES, 1 if forced == D.OPT_K5S else 8192)
                ran.add(check_call(dp, key, forced, relabel=forced == D.OPT_K5S))
            assert _stat(dp, L.STAT_DIAMETER_CLUSTER_LAUNCHES) == 0
        finally:
            dp.close()
    return frozenset(ran)


@pytest.mark.gpu
def test_csr_in_hbm_and_batches_without_a_fixed_width_shape(need_gpu):
    assert run_extras() == {("K2", "hbm"), ("K5S-CSR", 8)}


CHILDREN = {"nw4": {"CMDP_K5S_NW": "4"}, "agent": {"CMDP_K5C_SCOPE": "agent"}}


def child(mode):
    """Runs in a fresh process whose environment carries the switch: the same checks over all nine shapes, then one line
    with the kernels that ran."""
    ran = set()
    for shape in D.SHAPES:
        ran |= run_path("ell" if mode == "nw4" else "k5c", *shape)
    print("KERNELS " + json.dumps(sorted(ran)), flush=True)


@recorded
def run_child(mode):
    """One child at a time; a child that exits non-zero, or is killed at the time limit, fails and is not started again."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=dict(os.environ, **CHILDREN[mode]),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [x for x in r.stdout.splitlines() if x.startswith("KERNELS ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return frozenset(tuple(k) for k in json.loads(lines[0][len("KERNELS "):]))


@pytest.mark.gpu
def test_four_wavefronts_per_group_in_a_child_process(need_gpu):
    assert run_child("nw4") == {("K5S-ELL", 4) + s for s in D.SHAPES}


@pytest.mark.gpu
def test_agent_scope_cluster_kernels_in_a_child_process(need_gpu):
    assert run_child("agent") == {("K5C", cl) + s + ("agent",) for s in D.SHAPES for cl in (8, 16, 32)}


LIMIT_PATHS = {"K5S-CSR": (D.OPT_K5S_CSR, False), "K5S-ELL": (D.OPT_K5S, False), "K5T": (D.OPT_K5T, False), "K5C": (D.OPT_K5S, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("eps", LIMIT_EPS)
@pytest.mark.parametrize("path", sorted(LIMIT_PATHS))
def test_sweep_limit(need_gpu, path, eps):
    """max_sweeps equal to the sweeps the slowest target needs returns the oracle's values; one below raises
    DynamicProgrammingMaxIterationExceeded (status -5 of the lanes kernels), for an odd and an even count."""
    L = _lib()
    n = _largest_sweep_count("limit", eps)
    forced, relabel = LIMIT_PATHS[path]
    dp = _handle("limit")
    try:
        dp.set_option(L.OPT_DP_KERNEL, forced)
        if relabel:
            dp.set_option(L.OPT_DIAMETER_RELABEL_MIN_STATES, 1)
        diam, per = dp.diameter(eps, L.SCHEME_JACOBI, max_sweeps=n)
        assert D.FAMILY_NAME[D.decode(_stat(dp, L.STAT_DIAMETER_KERNEL))[0]] == path
        for b, (od, oper) in enumerate(D.oracle("limit", 1, eps)):
            np.testing.assert_array_equal(dp.split_states(per)[b], oper)
            assert diam[b] == np.float32(od)
        with pytest.raises(L.DynamicProgrammingMaxIterationExceeded):
            dp.diameter(eps, L.SCHEME_JACOBI, max_sweeps=n - 1)
    finally:
        dp.close()


def _compute_units():
    """Compute units of the GPUs the kernel driver lists (KFD topology: simd_count / simd_per_cu of every GPU node), as a
    set; empty where the topology cannot be read."""
    import glob

    out = set()
    for path in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
        try:
            p = dict(line.split()[:2] for line in open(path) if len(line.split()) >= 2)
        except OSError:
            continue
        if int(p.get("simd_count", 0)) > 0:
            out.add(int(p["simd_count"]) // max(int(p.get("simd_per_cu", 4)), 1))
    return out


@pytest.mark.gpu
def test_cluster_give_up_backs_off_for_8_then_16_calls(need_gpu):
    """The back-off of K5C -- pick_diameter_cluster's `backing_off` input, diameter_lanes' skip counter and doubling -- call
    by call on one handle, with a barrier time limit of one tick (the designed give-up path): call 1 tries K5C and gives
    up, calls 2-9 do not try, call 10 tries and gives up again, calls 11-26 do not try; with the limit lifted call 27 runs
    K5C.  8 and 16 are the code's max(8, 2 * back-off).  Every call returns the oracle's per-target values bit for bit."""
    L = _lib()
    if _compute_units() != {D.CUS}:
        pytest.skip(f"K5C's default clusters and this test's counts are the {D.CUS}-CU part's")
    key = ("shape", 2, 2)
    want = np.concatenate([p for _, p in D.oracle(key)])
    dp = _handle(key)
    old = os.environ.get("CMDP_K5C_TIMEOUT_TICKS")
    seen, first = [], None
    try:
        dp.set_option(L.OPT_DP_KERNEL, D.OPT_K5S)
        dp.set_option(L.OPT_DIAMETER_RELABEL_MIN_STATES, 1)
        os.environ["CMDP_K5C_TIMEOUT_TICKS"] = "1"
        for call in range(1, 28):
            if call == 27:
                os.environ.pop("CMDP_K5C_TIMEOUT_TICKS")
            _, per = dp.diameter(EPS, L.SCHEME_JACOBI)
            first = per.copy() if first is None else first
            np.testing.assert_array_equal(per, first, err_msg=f"call {call}")
            np.testing.assert_array_equal(per, want, err_msg=f"call {call}")
            seen.append((_stat(dp, L.STAT_DIAMETER_CLUSTER_LAUNCHES), _stat(dp, L.STAT_DIAMETER_CLUSTER_FALLBACKS),
                         _stat(dp, L.STAT_DIAMETER_KERNEL)))
    finally:
        os.environ.pop("CMDP_K5C_TIMEOUT_TICKS", None)
        if old is not None:
            os.environ["CMDP_K5C_TIMEOUT_TICKS"] = old
        dp.close()
    print("\n(launches, fallbacks, kernel) of calls 1 .. 27:", seen)
    assert [(l, f) for l, f, _ in seen] == [(0, 1)] * 9 + [(0, 2)] * 17 + [(1, 2)]
    assert [D.decode(k)[0] for _, _, k in seen[:26]] == [D.K5S_ELL] * 26
    assert seen[26][2] == D.code(D.K5C, 16, 1)


@pytest.mark.gpu
def test_sparse_float64_diameter_on_a_ragged_generated_batch(need_gpu):
    """K5D over several launches: the float64 diameter and the running maximum after every target, bit for bit."""
    from oracle import oracle as O

    L = _lib()
    t = D.batch("k5d")
    dp = _handle("k5d")
    try:
        dp.set_option(L.OPT_DIAMETER_WORKSPACE_MB, 1)
        d, run = dp.diameter_sparse_f64()
        for b in range(int(t["B"])):
            S, A, csr, _ = H.instance(t, b)
            od, orun = O.sparse_diameter_f64(S, A, csr)
            assert d[b] == od and dp.split_states(run)[b].tolist() == orun, b
    finally:
        dp.close()


@pytest.mark.gpu
def test_every_compiled_diameter_kernel_ran(need_gpu):
    """The kernels recorded through the statistic, the two child processes included, are the full compiled set: 27 K5S-ELL,
    54 K5C, 9 K5T, the CSR walker, both workgroup forms and the Gauss-Seidel form.  Starts nothing: it reads the outcomes
    the tests above recorded and fails if a path or a child failed or never ran (run the module's GPU tests together)."""
    assert _scope() == "xcd" and "CMDP_K5S_NW" not in os.environ
    expected = [("run_extras",), ("run_child", "nw4"), ("run_child", "agent")]
    expected += [("run_path", path) + shape for shape in D.SHAPES for path in ("auto", "ell", "wide", "csr", "k5t", "k5c")]
    never = [n for n in expected if n not in RECORD]
    failed = [n for n in expected if n in RECORD and RECORD[n][0] != "ok"]
    assert not never and not failed, f"this test only reads what the tests before it recorded: never ran {never}, failed {failed}"
    ran = set().union(*(RECORD[n][1] for n in expected))
    assert ran == D.all_kernels(), (sorted(D.all_kernels() - ran), sorted(ran - D.all_kernels()))
    print("\n(shape, scheme): float64 sweeps to diff < eps of the slowest target, largest E_m of an admissible sweep, largest "
          "|float32 - float64 r| at the NEAREST admissible sweep, widest union of intervals / value")
    for name, f in sorted(FINDINGS.items(), key=str):
        print(f"{name}: {f[0]} {f[1]:.3e} {f[2]:.3e} {f[3]:.3e}")


if __name__ == "__main__":
    sys.path.insert(0, H.ROOT)
    child(sys.argv[1])
