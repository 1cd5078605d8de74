"""K1E's interior rounds (csrc/cmdp_k1e.h): a round of eight full episodes, none of them the segment's first and none
with its last transition, skips the per-chain bookkeeping of the general path.

CPU: the predicate the kernel branches on (exported as cmdp_k1e_round_interior) against the kernel's own definitions of
a chain's first transition and length, by brute force.
GPU: every launch twice -- interior rounds on the short path, and CMDP_K1E_DEBUG=16 (every round on the general path) --
bit-equal to each other and to the CPU oracle, with the number of interior rounds of each launch counted through the
exported predicate."""
import functools
import os

import numpy as np
import pytest

from colosseum_amd import _lib as L
from colosseum_amd.batched import BatchedMDP
from colosseum_amd.mdp import make_model
from oracle import oracle as O

# mirrors of cmdp_k1e.h: wavefronts per workgroup, episodes per round of a wavefront, instances per group, segment length
K1E_NW, K1E_ROUND, K1E_NI, K1E_SEG = 16, 8, 32, 61440
K1E_EPP = K1E_NW * K1E_ROUND


def _max_episodes(n_steps, H):   # k1e_max_episodes
    return (n_steps + 2 * H - 2) // H


def _rounds(n_steps, H):
    """The first episodes e_lo of all rounds the workgroup walks in a segment of n_steps transitions."""
    R = (_max_episodes(n_steps, H) + K1E_EPP - 1) // K1E_EPP   # K1ePlan::n_pass
    return [(w * R + p) * K1E_ROUND for w in range(K1E_NW) for p in range(R)]


def _interior_rounds(B, H, n_steps):
    """Interior rounds of one launch of n_steps transitions on B instances (segments of K1E_SEG, groups of K1E_NI)."""
    lib = L.load()
    total = 0
    for s0 in range(0, n_steps, K1E_SEG):
        n = min(K1E_SEG, n_steps - s0)
        for g0 in range(0, B, K1E_NI):
            nb = min(K1E_NI, B - g0)
            total += sum(lib.cmdp_k1e_round_interior(e_lo, H, n, nb) for e_lo in _rounds(n, H))
    return total


def test_interior_predicate_against_chain_definitions():
    """predicate true => for every in-episode start time h0 and every owner lane, all eight chains of the round are full
    episodes (len_of == H), none is episode 0 and none ends at n_steps (the chain that leaves the instance's state behind);
    and the predicate is not vacuous: a segment of at least 24 episodes of a full group has an interior round."""
    lib = L.load()
    for H in (1, 3, 9, 30, 32, 33, 64):
        h0 = np.arange(H)[:, None]                       # [H, 1]
        for n in list(range(1, 40 * H + 1)) + [61440, 61439]:
            any_true = False
            for e_lo in _rounds(n, H) + [_rounds(n, H)[-1] + K1E_ROUND]:
                got = [lib.cmdp_k1e_round_interior(e_lo, H, n, nb) for nb in (1, 31, 32)]
                assert all(g in (0, 1) for g in got)
                any_true |= got[2] == 1
                if not any(got):
                    continue
                e = e_lo + np.arange(K1E_ROUND)[None, :]   # [1, 8]: the round's episodes (half s, chain c: e_lo + 4 s + c)
                first = np.where(e == 0, 0, e * H - h0)    # first_of
                length = np.where(first < n, np.minimum(np.where(e == 0, H - h0, H), n - first), 0)   # len_of of an owner lane
                assert (e != 0).all(), (H, n, e_lo)
                assert (length == H).all(), (H, n, e_lo)
                assert (first + length != n).all(), (H, n, e_lo)
            if n >= 24 * H:
                assert any_true, (H, n)
    assert lib.cmdp_k1e_round_interior(8, 9, 10_000, 0) == 0   # a group without instances has nothing to walk


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _models(B):
    return tuple(make_model("DeepSeaEpisodic", seed=300 + i, size=9) for i in range(B))


def _keys(B):
    return (np.arange(B) * 104729 + 17).astype(np.uint64)


def _run_k1e(debug, script, models=None, tables=None, keys=None):
    """One handle created with CMDP_K1E_DEBUG = debug (None: unset), the script of ("reset", mask) / ("rollout", n) legs on
    the episode-parallel kernel; returns per rollout leg (last_obs, reward_sum) and at the end visits, state, and a
    131-transition continuation (more than one Philox block: it starts where the transition counters say)."""
    saved = os.environ.pop("CMDP_K1E_DEBUG", None)
    if debug is not None:
        os.environ["CMDP_K1E_DEBUG"] = str(debug)
    try:
        if models is not None:
            env = BatchedMDP(list(models), rng_mode=L.RNG_PHILOX, philox_keys=keys, with_dp=False)
        else:
            env = BatchedMDP(tables=tables, rng_mode=L.RNG_PHILOX, philox_keys=keys)
    finally:
        os.environ.pop("CMDP_K1E_DEBUG", None)
        if saved is not None:
            os.environ["CMDP_K1E_DEBUG"] = saved
    env.set_rollout_kernel(L.ROLLOUT_EPISODE_PARALLEL)
    legs = []
    for op, arg in script:
        if op == "reset":
            env.reset(arg)
        else:
            out = env.rollout(arg)
            assert env.lds_plan()["kernel"] == "k_rollout_epi"
            legs.append((out["last_obs"].copy(), out["reward_sum"].copy()))
    vs, vsa = env.visits()
    cur, h, nr = env.state()
    tail = env.rollout(131)
    env.close()
    return dict(legs=legs, vs=vs, vsa=vsa, cur=cur, h=h, nr=nr, tail=(tail["last_obs"].copy(), tail["reward_sum"].copy()))


def _assert_same(a, b):
    assert len(a["legs"]) == len(b["legs"])
    for (lo_a, rs_a), (lo_b, rs_b) in zip(a["legs"] + [a["tail"]], b["legs"] + [b["tail"]]):
        np.testing.assert_array_equal(lo_a, lo_b)
        np.testing.assert_array_equal(rs_a, rs_b)
    for k in ("vs", "vsa", "cur", "h", "nr"):
        np.testing.assert_array_equal(a[k], b[k])


def _oracle_models(models, keys, script):
    B = len(models)
    n_legs = sum(op == "rollout" for op, _ in script)
    legs = [(np.zeros(B, np.int32), np.zeros(B, np.float64)) for _ in range(n_legs)]
    tail = (np.zeros(B, np.int32), np.zeros(B, np.float64))
    vs, vsa, cur, h, nr = [], [], np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, bool)
    for b, m in enumerate(models):
        e = O.OracleEnv(m, rng_mode=1, philox_key=int(keys[b]))
        k = 0
        for op, arg in script:
            if op == "reset":
                if arg is None or arg[b]:
                    e.reset()
            else:
                r = e.rollout(arg, trace=False)
                legs[k][0][b], legs[k][1][b] = r["last_obs"], r["reward_sum"]
                k += 1
        v = e.visits()
        vs.append(np.asarray(v[0]).ravel())
        vsa.append(np.asarray(v[1]).ravel())
        cur[b], h[b], nr[b] = e.state()
        r = e.rollout(131, trace=False)
        tail[0][b], tail[1][b] = r["last_obs"], r["reward_sum"]
    return dict(legs=legs, vs=np.concatenate(vs), vsa=np.concatenate(vsa), cur=cur, h=h, nr=nr, tail=tail)


_N = 128 * 9 * 2   # the bench's situation scaled down: from reset (h0 = 0), a multiple of H, two rounds per wavefront
_MASK45 = (np.arange(45) % 3 == 0).astype(np.uint8)
_CASES = {
    # name: (B, script, interior rounds expected (None: at least one))
    "bench_like": (64, (("reset", None), ("rollout", _N)), None),
    "last_interior_round_minus_1": (64, (("reset", None), ("rollout", _N - 1)), None),
    "last_interior_round_plus_1": (64, (("reset", None), ("rollout", _N + 1)), None),
    "per_lane_phases": (45, (("reset", None), ("rollout", 13), ("reset", _MASK45), ("rollout", 6_007)), None),
    "two_segments": (33, (("reset", None), ("rollout", 70_000)), None),
    "no_interior_round": (32, (("reset", None), ("rollout", 15 * 9)), 0),
    "single_instance": (1, (("reset", None), ("rollout", _N)), None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(_CASES))
def test_interior_rounds_equal_general_path_and_oracle(need_gpu, case):
    """DeepSeaEpisodic size 9 (H = 9, 45 states): last observation, float64 reward sum, visits_s / visits_sa, state,
    in-episode time and (through a 131-transition continuation) the transition counters, compared with == between the
    interior path, the general path alone (CMDP_K1E_DEBUG=16) and per-instance OracleEnv runs."""
    B, script, expect = _CASES[case]
    models, keys = _models(B), _keys(B)
    assert models[0].H == 9 and models[0].n_states == 45
    # the longest launch of the script decides; every launch is counted
    counts = [_interior_rounds(B, 9, n) for op, n in script if op == "rollout"]
    if expect == 0:
        assert sum(counts) == 0, counts
    else:
        assert max(counts) > 0, counts
    fast = _run_k1e(None, script, models=models, keys=keys)
    general = _run_k1e(16, script, models=models, keys=keys)
    _assert_same(fast, general)
    _assert_same(fast, _oracle_models(models, keys, script))


@pytest.mark.gpu
def test_interior_rounds_two_code_words_per_episode(need_gpu):
    """A horizon above 32 (two code words per episode): DeepSea-20's graph under a horizon of 45, as
    test_lds_resident_rollout_equals_global_kernel_and_oracle builds it; B = 40 (one full group, one ragged), n = 5 000.
    The oracle of a table batch is oracle.batch_rollout (last observation, reward sum, both visit counters); state and
    in-episode time are compared between the two runs, and from reset the in-episode time is n mod H."""
    from colosseum_amd.mdp.fast_batch import deepsea_episodic_tables

    B, n = 40, 5_000
    seeds = np.arange(1000, 1000 + B)
    tables = deepsea_episodic_tables(seeds, 20)
    tables["H"] = 45
    keys = (seeds * 7919).astype(np.uint64)
    script = (("reset", None), ("rollout", n))
    assert _interior_rounds(B, 45, n) > 0
    fast = _run_k1e(None, script, tables=tables, keys=keys)
    general = _run_k1e(16, script, tables=tables, keys=keys)
    _assert_same(fast, general)
    last, rsum, ovs, ovsa = O.batch_rollout(tables, 0, B, n, rng_mode=1, philox_keys=keys, want_visits=True)
    np.testing.assert_array_equal(fast["legs"][0][0], last)
    np.testing.assert_array_equal(fast["legs"][0][1], rsum)
    np.testing.assert_array_equal(fast["vs"], ovs)
    np.testing.assert_array_equal(fast["vsa"], ovsa)
    np.testing.assert_array_equal(fast["h"], np.full(B, n % 45))
    last2, rsum2, _, _ = O.batch_rollout(tables, 0, B, n + 131, rng_mode=1, philox_keys=keys, want_visits=True)
    np.testing.assert_array_equal(fast["tail"][0], last2)   # the continuation ends where one run of n + 131 transitions ends
