"""Test helper of the MAP-model solve (kernel K15, csrc/cmdp_map_vi.h): tables, the float64 restatement of
`episodic_value_iteration(H, *get_map_estimate())`, its bound and the comparison of two greedy policies up to rounding.

The restatement: the dense float32 MAP estimate exactly as the reference forms it (conjugate_transitions.py
M_DIR.get_map_estimate: hyper_params / hyper_params.sum(-1, keepdims=True), float32) through helpers_psrl.vi_episodic_f64.
The kernel evaluates a row's dot product in the split form c (SV - sum_e V_e) + sum_e t_e V_e in float64 and rounds Q once:
per layer it differs from the exact value by that one rounding, U qmax, plus float64 effects of relative size ~S 2^-53
(the cancellation in SV - sum_e V_e is of values <= S qmax, times c <= 1 / S for a prior-only remainder), which the
(1 + 2^-20) factor of helpers_psrl.bound_episodic(H, qmax, 1) covers.  That bound is used as it is."""
import json
import os

import numpy as np

from helpers_psrl import bound_episodic, moment_tables, vi_episodic_f64

G21 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G21_psrl_map.npz")


def g21():
    z = np.load(G21)
    return z, json.loads(str(z["cases"]))


def g21_stages():
    """(case index, meta, episodes, arrays of the stage) for every recorded stage."""
    z, meta = g21()
    for i, m in enumerate(meta):
        for st in m["stages"]:
            p = f"c{i}_e{st['episodes']}_"
            yield i, m, st["episodes"], {k: z[p + k] for k in ("reward_hp", "transition_hp", "T_map", "R_map", "Q", "policy")}


def tables(S, A, seed=0, n_transitions=None):
    """(transition_hp [S, A, S], mu [S, A], prior) float32: helpers_psrl.moment_tables (prior 1 / S, some rows updated)."""
    thp, rhp = moment_tables(S, A, n_transitions=4 * S if n_transitions is None else n_transitions, seed=seed)
    prior = np.tile([1.0 / S], (1, 1, 1)).astype(np.float32)[0, 0, 0]
    return thp, np.ascontiguousarray(rhp[:, :, 0]), prior


def map_estimate(transition_hp):
    """M_DIR.get_map_estimate as the reference writes it (float32)."""
    thp = np.asarray(transition_hp, np.float32)
    T = thp / thp.sum(-1, keepdims=True)
    assert T.dtype == np.float32
    return T


def restatement(transition_hp, mu, H):
    """(Q64 [H + 1, S, A], V64, bound): float64 value iteration on the float32 MAP estimate and the largest |Q - Q64| the
    kernel may show."""
    Q64, V64, qmax = vi_episodic_f64(H, map_estimate(transition_hp), np.asarray(mu, np.float32))
    return Q64, V64, bound_episodic(H, qmax, 1)


def check_solve(Q, V, transition_hp, mu, H):
    """The kernel's Q and V against the restatement; returns err / bound."""
    Q64, V64, tol = restatement(transition_hp, mu, H)
    assert Q.dtype == np.float32 and Q.shape == Q64.shape
    err = float(np.abs(Q - Q64).max())
    assert err <= tol, (err, tol)
    if V is not None:
        assert np.array_equal(V, Q.max(-1))
        assert float(np.abs(V - V64).max()) <= tol
    assert (Q[H] == 0).all()
    return err / tol


def check_greedy(pi, Q64, tol):
    """`pi` [H + 1, S, A] is one-hot and greedy for Q64 up to rounding at EVERY (h, s): no exclusion."""
    assert pi.shape == Q64.shape and ((pi == 0) | (pi == 1)).all() and (pi.sum(-1) == 1).all()
    chosen = np.take_along_axis(Q64, pi.argmax(-1)[..., None], -1)[..., 0]
    assert (chosen >= Q64.max(-1) - 2 * tol).all(), float((Q64.max(-1) - chosen).max())


def compare_policies(pi_a, pi_b, Q64, tol):
    """Two policies must agree wherever the top two Q64 values of (h, s) differ by more than 2 tol.  Returns the share of
    (h, s) left out (near and exact ties)."""
    top = np.sort(Q64, -1)
    decided = (top[..., -1] - top[..., -2] > 2 * tol) if Q64.shape[-1] > 1 else np.ones(Q64.shape[:2], bool)
    same = (pi_a.argmax(-1) == pi_b.argmax(-1))
    assert same[decided].all(), int((~same & decided).sum())
    return 1.0 - float(decided.mean())


def host_route(transition_hp, reward_hp, H):
    """`BatchedPSRLEpisodic.current_optimal_stochastic_policy` as it stood before the device route: map_estimate(), the
    library's `episodic_value_iteration` on the dense MAP estimate, argmax_3d."""
    from colosseum_amd.dynamic_programming import argmax_3d, episodic_value_iteration

    T, R = map_estimate(transition_hp), np.asarray(reward_hp, np.float32)[:, :, 0]
    return argmax_3d(episodic_value_iteration(int(H), np.ascontiguousarray(T), np.ascontiguousarray(R))[0])


def custom_model(S, A, H, seed, fan):
    """A CustomEpisodic MDP with `fan` successors in two rows of three and one in the others (so the agent's layout has
    rows of one position and, for fan > 64, rows longer than a wavefront), uniform rewards, two start states."""
    from colosseum_amd.mdp import make_model

    rng = np.random.RandomState(seed)
    T = np.zeros((S, A, S))
    for s in range(S):
        for a in range(A):
            k = min(S, fan if (s + a) % 3 else 1)
            T[s, a, rng.choice(S, k, replace=False)] = rng.dirichlet(np.ones(k))
    R = rng.uniform(size=(S, A)).astype(np.float32)
    return make_model("CustomEpisodic", seed=seed, T_0={0: 0.5, S - 1: 0.5}, T=T, R=R, H=H)
