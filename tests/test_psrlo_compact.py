"""The compact optimistic sample (kernel K19, csrc/cmdp_psrlo_vi.h) as tests/helpers_psrlo_compact.py defines it, held
against the NumPy twin of the reference's optimistic sampling (tests/helpers_psrlo.py, pinned to the reference by golden G23)
without a device.  PSRLOTwin runs on RiverSwim of sizes 4 and 5 -- the twin's own draws, a NumPy walk on the model's dense T --
long enough for rounds that are all simple, mixed and all posterior, and for the chain's `+=` / `-=` pair to run on a non-zero
P_minus with z_k inside the row's layout (the case in which a stored value may drift).  A value that actually changed is
counted and asserted NOT to occur: at these sizes it cannot.  A pair below eta = 10 S visits has a deviation w >= 1/2, so a
non-zero P_minus = P_hat - w comes from two values in [1/2, 1] and lies on their grid of 2^-53, as does summing = 1 - P_minus:
x + summing = 1 and 1 - summing = x are exact (a row has one non-zero P_minus at most: two would need two P_hat > 1/2).  On
every sample the compact form expands to the twin's
T_ext bit for bit, its count is (T_ext != 0).sum(), and the float64 solver on the compact form agrees with the float64 dense
restatement to 1e-12.  The package's own host helpers (dynamic_programming.optimistic_compact_from_dense / optimistic_expand)
are held against the same samples."""
import numpy as np
import pytest

import helpers_psrlo_compact as HC
from helpers_psrlc import GAMMA32, GAUSS_SEIDEL, JACOBI, vi_discounted_f64
from helpers_psrlo import PSRLOTwin
from colosseum_amd import dynamic_programming as dp
from colosseum_amd.agents import optimistic_sampling_scalars
from colosseum_amd.mdp import make_model


def quick_solver(T, R):
    """Any solver drives the twin: Jacobi in float64 to 1e-3, cast as the reference casts."""
    T, R = T.astype(np.float64), R.astype(np.float64)
    V = np.zeros(T.shape[0])
    while True:
        Q = R + GAMMA32 * (T @ V)
        V2 = Q.max(-1)
        if np.abs(V2 - V).max() < 1e-3:
            return Q.astype(np.float32)
        V = V2


def drifted(tw):
    """Whether the reference's `P_minus[:, :, z] += summing; ... -= summing` leaves some non-zero value of a simple row changed
    at some k: the float64 chain of optimistic_sampling (:411-443) on the twin's N, restated."""
    Nsum = tw.N.sum(-1)
    P_hat = tw.N / np.maximum(Nsum[..., None], 1)
    N = np.maximum(tw.N, 1)
    P = P_hat - np.minimum(np.sqrt(3 * P_hat * np.log(4 * tw.S) / N) + 3 * np.log(4 * tw.S) / N, P_hat)
    for z in tw.last_z:
        before = P[:, :, z].copy()
        summing = 1 - P.sum(-1)
        P[:, :, z] += summing
        P[:, :, z] -= summing
        if ((P[:, :, z] != before) & tw.last_simple).any():
            return True
    return False


def run(size, seed, steps, p_lazy=None, **kw):
    m = make_model("RiverSwimContinuous", seed=seed, size=size, p_lazy=p_lazy)
    T_true, R_true = m.dense()
    S, A = m.n_states, m.n_actions
    psi, _, eta, _ = optimistic_sampling_scalars(S, A, 600, **kw)
    tw = PSRLOTwin(seed, S, A, float(m.rewards_range[1]), psi, eta, quick_solver)
    row_ptr, col = HC.layout_from_support(T_true)
    rng = np.random.RandomState(100 + seed)
    seen = dict(kinds=set(), drift=0, z_in_layout=0, nonzero_p_minus=0, samples=0)

    def check():
        c = HC.compact_of_twin(tw, row_ptr, col)
        T = HC.expand(c)
        assert T.dtype == np.float32 and np.array_equal(T, tw.last_T), tw.episode
        assert HC.nonzero_count(c) == int((tw.last_T != 0).sum()), tw.episode
        assert np.array_equal(HC.r_ext(c), tw.last_R_ext)
        n1, n2 = tw.last_n
        seen["kinds"].add("mixed" if n1 and n2 else "all_posterior" if n1 else "all_simple")
        seen["drift"] += bool(n2) and drifted(tw)
        for row in np.flatnonzero(c["simple"]):
            cs = c["col"][row_ptr[row]:row_ptr[row + 1]]
            vals = c["pmk"][:, row_ptr[row]:row_ptr[row + 1]]
            p_minus = (vals != 0) & (cs[None, :] != c["z"][:, None])   # at z_k the position holds the bump, not P_minus
            seen["nonzero_p_minus"] += bool(p_minus.any())
            seen["z_in_layout"] += int(np.isin(c["z"], cs).sum()) if p_minus.any() else 0
        # the package's host helpers: given the sampler's mask and z they build the same arrays, and expand them back
        p = dp.optimistic_compact_from_dense(tw.last_T, psi, row_ptr, col, tw.last_R, simple=c["simple"], z=c["z"])
        for key in ("pmk", "bump", "pidx", "post", "z"):
            assert np.array_equal(p[key], c[key]), (key, tw.episode)
        assert np.array_equal(dp.optimistic_expand(p), tw.last_T)
        assert np.array_equal(dp.optimistic_expand(dp.optimistic_compact_from_dense(tw.last_T, psi, row_ptr, col, tw.last_R)), tw.last_T)
        if seen["samples"] % 6 == 0 or len(seen["kinds"]) > seen.get("kinds_solved", 0):
            seen["kinds_solved"] = len(seen["kinds"])
            for scheme in (JACOBI, GAUSS_SEIDEL):
                Qc, dc, _, _ = HC.vi_compact_f64(c, GAMMA32, scheme, 25)
                Qd, dd, _, _ = vi_discounted_f64(tw.last_T, tw.last_R_ext, GAMMA32, scheme, 25)
                assert np.abs(Qc - Qd).max() <= 1e-12 and abs(dc - dd) <= 1e-12, (scheme, tw.episode)
            V = rng.rand(S).astype(np.float32)
            for row in np.flatnonzero(c["simple"])[:3]:
                s, a = divmod(int(row), A)
                for k in (0, psi - 1):
                    dense = tw.last_T[s, a * psi + k].astype(np.float64) @ V.astype(np.float64)
                    assert abs(HC.simple_row_sum(c, row, k, V) - dense) <= 1e-15 * S
        seen["samples"] += 1

    tw.before_start_interacting()
    check()
    s = 0
    for _ in range(steps):
        a = tw.select_action(s)
        s2 = int(rng.choice(S, p=T_true[s, a].astype(np.float64) / T_true[s, a].astype(np.float64).sum()))
        tw.step_update(s, a, float(R_true[s, a]), s2)
        if tw.is_episode_end(s, a):
            tw.episode_end_update()
            check()
        s = s2
    return seen


def test_riverswim5_defaults_nonzero_p_minus_and_z_inside_the_layout():
    seen = run(5, 0, 600)
    print(seen)
    assert "all_simple" in seen["kinds"]
    assert seen["nonzero_p_minus"] > 0 and seen["z_in_layout"] > 0 and seen["drift"] == 0


def test_riverswim5_lazy_two_successors_per_row():
    """A lazy step gives every pair two successors: layouts of two positions, P_hat < 1, and the chain on non-zero data."""
    seen = run(5, 1, 900, p_lazy=0.1)
    print(seen)
    assert seen["nonzero_p_minus"] > 0 and seen["z_in_layout"] > 0 and seen["drift"] == 0


def test_riverswim4_small_eta_all_three_kinds_of_round():
    seen = run(4, 6, 600, eta_weight=1e-10, max_psi=5)
    print(seen)
    assert seen["kinds"] == {"all_simple", "mixed", "all_posterior"} and seen["drift"] == 0


@pytest.mark.parametrize("size", [4, 5])
def test_mixed_rounds_with_small_eta(size):
    seen = run(size, 3, 300, eta_weight=1e-10, max_psi=7)
    print(seen)
    assert "mixed" in seen["kinds"] and seen["samples"] > 10 and seen["drift"] == 0
