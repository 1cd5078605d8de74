"""K1E without count words (csrc/cmdp_k1e.h): the walk stores the 2-bit reward codes of an episode chunk only, and the
reward scan counts the steps per code from the code words itself.

CPU: the two count functions the scan uses (exported as cmdp_k1e_code_counts) against field-by-field counting.
GPU: K1E against the CPU oracle on small batches whose rewards are edited so that both count forms, a scaled minimum
reward other than 0, tie cases and negative rewards (the float64 path) occur; several launches of odd lengths continue
one another, so that the action-bit ring is entered at many wrap positions; every case on the interior path and, with
CMDP_K1E_DEBUG=16, on the general path alone."""
import functools
import os
import types

import numpy as np
import pytest

from colosseum_amd import _lib as L
from colosseum_amd.batched import BatchedMDP
from oracle import oracle as O

K1E_NW, K1E_ROUND, K1E_NI, K1E_SEG = 16, 8, 32, 61440   # mirrors of cmdp_k1e.h
K1E_EPP = K1E_NW * K1E_ROUND


# ---- CPU: the count functions -------------------------------------------------------------------------------------------

def _pack(fields):
    """32 two-bit fields (step j at bits 2 j of the 64-bit word) -> (lo, hi)."""
    f = np.asarray(fields, np.uint64)
    assert f.shape == (32,) and (f < 4).all()
    word = int((f << (2 * np.arange(32, dtype=np.uint64))).sum())
    return word & 0xFFFFFFFF, word >> 32


def _expected(fields):
    f = np.asarray(fields)
    return int((f == 1).sum()) | int((f == 2).sum()) << 11 | int((f == 3).sum()) << 22


def _check(fields, few):
    lib = L.load()
    lo, hi = _pack(fields)
    want = _expected(fields)
    assert lib.cmdp_k1e_code_counts(lo, hi, 0) == want, (fields, "four-code form")
    if few:
        assert not (np.asarray(fields) == 3).any()   # the few form is defined on words without a field equal to 3 only
        assert lib.cmdp_k1e_code_counts(lo, hi, 1) == want, (fields, "few form")


def test_code_counts_all_patterns_of_a_few_fields():
    """every 2-bit pattern of five low fields, and of four fields at the ends of the two halves (steps 0, 15, 16, 31)"""
    for pos in ((0, 1, 2, 3, 4), (0, 15, 16, 31)):
        n = len(pos)
        for v in range(4 ** n):
            fields = np.zeros(32, np.int64)
            fields[list(pos)] = [(v >> (2 * i)) & 3 for i in range(n)]
            _check(fields, few=not (fields == 3).any())
    for c in (1, 2, 3):   # full words of one code: the largest counts
        _check(np.full(32, c), few=c != 3)


def test_code_counts_random_words():
    """4 000 seeded random words with four codes and 4 000 with three (both forms), a third of them partial chunks: the
    fields from a random length on are zero, as the walk leaves them."""
    rng = np.random.RandomState(20260)
    for n_codes in (4, 3):
        for i in range(4000):
            fields = rng.randint(0, n_codes, 32)
            if i % 3 == 0:
                fields[rng.randint(0, 32):] = 0
            _check(fields, few=n_codes == 3)


# ---- GPU ------------------------------------------------------------------------------------------------------------

_B, _SIZE = 33, 9   # one full group of 32 instances and one instance in the next; DeepSea size 9: 45 states, H = 9
# tie cases: added to a sum in [1, 2) (spacing 2^-52) resp. [256, 512) (spacing 2^-44) the value lies exactly half way
# between two representable sums, so ties-to-even looks at the sum itself; a first launch passes through both binades
_TIE, _TIE8 = 2.0 ** -53, 0.75 + 2.0 ** -45
# name: the distinct reward values, code 0 (the value of the first row) first
_VARIANTS = {
    "three_values": (0.0, 0.5, 1.0),
    "four_values": (0.0, 0.5, 1.0, 0.25),
    "minimum_not_zero": (0.125, 0.5, 1.0),
    "tie_case": (0.0, 0.5, _TIE, _TIE8),
    "negative": (0.0, -0.25, 1.0),
}


def _lengths(H):
    """Eight odd launch lengths of at least 300 episodes, no multiple of H."""
    base = 300 * H + 1 + (300 * H) % 2
    return [base + d for d in (0, 142, 300, 298, 6, 502, 216, 406)]


@functools.lru_cache(maxsize=None)
def _tables(variant, H):
    """deepsea_episodic_tables(size 9) with the reward of row r of instance b set to values[(r + 3 b) mod n], and the
    horizon set to H (H = 45: two code words per episode, the second one partial)."""
    from colosseum_amd.mdp.fast_batch import deepsea_episodic_tables

    vals = np.asarray(_VARIANTS[variant], np.float64)
    t = deepsea_episodic_tables(np.arange(500, 500 + _B), _SIZE)
    S = int(t["state_off"][1])
    rows = np.arange(S * 2)[None, :] + 3 * np.arange(_B)[:, None]
    rew = vals[rows % len(vals)].reshape(-1)
    t["sp_reward"] = rew.copy()
    t["sp_rp0"] = rew.copy()
    t["H"] = H
    return t


def _keys():
    return (np.arange(_B) * 15485863 + 29).astype(np.uint64)


def _instance(t, b):
    """Instance b of a table batch as the plain arrays OracleEnv reads."""
    S, A = int(t["state_off"][1]), int(t["A"])
    r0, r1 = b * S * A, (b + 1) * S * A
    rew = np.asarray(t["sp_reward"][r0:r1], np.float64)
    return types.SimpleNamespace(
        sp_ptr=np.asarray(t["sp_ptr"][r0:r1 + 1]) - t["sp_ptr"][r0], sp_next=t["sp_next"][r0:r1], sp_cum=t["sp_cum"][r0:r1],
        sp_rkind=np.zeros(r1 - r0, np.uint8), sp_rp0=rew, sp_rmean=rew, sp_seed=t["sp_seed"][r0:r1],
        start_states=t["start_state"][b:b + 1], start_probs=np.ones(1), start_seed=0, deterministic_rewards=True,
        n_states=S, n_actions=A, H=int(t["H"]), rewards_range=tuple(t["rewards_range"]))


@functools.lru_cache(maxsize=None)
def _oracle(variant, H):
    """Per-instance OracleEnv runs of the launches (computed once per case, shared by both GPU runs): per launch last
    observation and reward sum, at the end visit counters, state and in-episode time, and the rewards met on the way."""
    t, keys, lengths = _tables(variant, H), _keys(), _lengths(H)
    legs = [(np.zeros(_B, np.int32), np.zeros(_B, np.float64)) for _ in lengths]
    vs, vsa, cur, h, seen = [], [], np.zeros(_B, np.int32), np.zeros(_B, np.int32), set()
    for b in range(_B):
        e = O.OracleEnv(_instance(t, b), rng_mode=1, philox_key=int(keys[b]))
        e.reset()
        for k, n in enumerate(lengths):
            r = e.rollout(n, trace=k == 0)
            legs[k][0][b], legs[k][1][b] = r["last_obs"], r["reward_sum"]
            if k == 0:
                seen.update(np.unique(r["rew"]).tolist())
        v = e.visits()
        vs.append(np.asarray(v[0]).ravel())
        vsa.append(np.asarray(v[1]).ravel())
        cur[b], h[b], _ = e.state()
    return dict(legs=legs, vs=np.concatenate(vs), vsa=np.concatenate(vsa), cur=cur, h=h, seen=seen)


def _interior_rounds(B, H, n_steps):
    lib = L.load()
    total = 0
    for s0 in range(0, n_steps, K1E_SEG):
        n = min(K1E_SEG, n_steps - s0)
        R = ((n + 2 * H - 2) // H + K1E_EPP - 1) // K1E_EPP
        for g0 in range(0, B, K1E_NI):
            total += sum(lib.cmdp_k1e_round_interior((w * R + p) * K1E_ROUND, H, n, min(K1E_NI, B - g0))
                         for w in range(K1E_NW) for p in range(R))
    return total


def _run_k1e(debug, tables, keys, lengths):
    saved = os.environ.pop("CMDP_K1E_DEBUG", None)
    if debug is not None:
        os.environ["CMDP_K1E_DEBUG"] = str(debug)
    try:
        env = BatchedMDP(tables=tables, rng_mode=L.RNG_PHILOX, philox_keys=keys)
    finally:
        os.environ.pop("CMDP_K1E_DEBUG", None)
        if saved is not None:
            os.environ["CMDP_K1E_DEBUG"] = saved
    env.set_rollout_kernel(L.ROLLOUT_EPISODE_PARALLEL)
    env.reset()
    legs = []
    for n in lengths:
        out = env.rollout(n)
        assert env.lds_plan()["kernel"] == "k_rollout_epi"
        legs.append((out["last_obs"].copy(), out["reward_sum"].copy()))
    vs, vsa = env.visits()
    cur, h, _ = env.state()
    env.close()
    return dict(legs=legs, vs=vs, vsa=vsa, cur=cur, h=h)


@pytest.mark.gpu
@pytest.mark.parametrize("H", (9, 45))
@pytest.mark.parametrize("variant", list(_VARIANTS))
def test_k1e_code_words_equal_oracle(need_gpu, variant, H):
    """33 instances of DeepSea size 9 with edited rewards, eight launches of odd lengths that continue one another: reward
    sums compared with ==, last observation, visits_s, visits_sa, state and in-episode time with assert_array_equal,
    against per-instance OracleEnv runs (and oracle.batch_rollout for the first launch), on the interior path and with
    CMDP_K1E_DEBUG=16 on the general path."""
    tables, keys, lengths = _tables(variant, H), _keys(), _lengths(H)
    vals = _VARIANTS[variant]
    # the launches: partial first and last episodes, interior and general rounds, >= 8 ring positions at a launch's start
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    assert all(n % 2 == 1 and n % H != 0 and n >= 300 * H for n in lengths)
    assert len(set(int(s) % 512 for s in starts)) >= 8
    assert len(set(int(s) % H for s in starts)) >= 3
    for n in lengths:
        R = ((n + 2 * H - 2) // H + K1E_EPP - 1) // K1E_EPP
        assert 0 < _interior_rounds(_B, H, n) < 2 * K1E_NW * R
    ref = _oracle(variant, H)
    # every reward value occurs on the oracle's trajectories: codes 1, 2 (and 3) are all met
    assert tuple(tables["rewards_range"]) == (0.0, 1.0)   # the scaled reward is the table's value
    assert ref["seen"] == set(vals), (ref["seen"], vals)
    assert len(ref["seen"]) == len(vals) and len(vals) == (4 if variant in ("four_values", "tie_case") else 3)
    if variant == "minimum_not_zero":
        assert min(ref["seen"]) != 0.0
    if variant == "negative":
        assert min(ref["seen"]) < 0.0
    if variant == "tie_case":   # the sums pass through the binades the two values tie in
        assert (ref["legs"][0][1] >= 512.0).all()
    last0, rsum0 = O.batch_rollout(tables, 0, _B, lengths[0], rng_mode=1, philox_keys=keys)
    np.testing.assert_array_equal(ref["legs"][0][0], last0)
    assert (ref["legs"][0][1] == rsum0).all()
    for debug in (None, 16):
        got = _run_k1e(debug, tables, keys, lengths)
        for k, ((g_last, g_sum), (o_last, o_sum)) in enumerate(zip(got["legs"], ref["legs"])):
            assert (g_sum == o_sum).all(), (debug, k, np.flatnonzero(g_sum != o_sum)[:8])
            np.testing.assert_array_equal(g_last, o_last, err_msg=f"debug {debug} launch {k}")
        for name in ("vs", "vsa", "cur", "h"):
            np.testing.assert_array_equal(got[name], ref[name], err_msg=f"debug {debug} {name}")
