"""The single-value path of K1E's reward scan on the GPU (csrc/cmdp_k1e.h, k1r_single inside k_reward_scan): tiles whose
advance fails and that hold one nonzero reward value are resolved from their step counts, beside lanes of the same wavefront
that take the searching slow path -- through BatchedMDP.rollout against per-instance OracleEnv runs: reward sums compared
with ==, last observations, visit counters, state and in-episode time with assert_array_equal.

The batch-wide reward values are (0, 1/900, 1, 2^-53) -- four codes -- and the rows of instance b draw from {0, 1/900}, {0,
1/900, 1}, {0, 1} or {0, 2^-53} (b mod 4): the lanes of one wavefront take the single-value path in integers, the old path
and the float64 loop side by side.  Before the comparison the oracle's reward traces of instances 0 .. 3 go through the
scan's own lane code on the CPU (cmdp_k1e_scan_words_ex), segment by segment as launch_k1e cuts a launch: its counters prove
that every long launch took single-value tiles on instances 0 and 2 and searched words on instance 1.
(The construction is that of test_k1e_scan_paths.py.)"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from colosseum_amd import _lib as L
from colosseum_amd.batched import BatchedMDP
from oracle import oracle as O

K1E_SEG, K1R_T = 61440, 8   # mirrors of cmdp_k1e.h
_SIZE, _BMAX = 9, 65         # DeepSea size 9: 45 states; 65 instances: a second wavefront of the scan with ONE live lane
_VALS = (0.0, 1.0 / 900.0, 1.0, 2.0 ** -53)
_DRAWS = ((0, 1), (0, 1, 2), (0, 2), (0, 3))   # b mod 4: the values (indices into _VALS) the rows of instance b draw from
_MASK = (np.arange(_BMAX) % 3 == 0).astype(np.uint8)
_TRACED = (0, 1, 2, 3)
PLAIN, SLOW, WORD, REBASE, SINGLE, CROSS, FADD = range(7)


def _script(H):
    """("reset", mask or None) / ("rollout", n) legs: the script of test_k1e_scan_paths.py -- short launches whose code words
    end at the boundaries of a tile and of the three rolling tiles, 300 episodes + 1, 70 000 transitions (two segments), a
    launch after a masked reset (two in-episode times within a wavefront) -- and, for H = 30, a launch of 300 whole episodes
    from reset: the pair walk, plain tiles throughout."""
    nch = (H + 31) // 32
    legs = []
    for E in ((7, 8, 9, 25) if nch == 1 else (4, 5, 12, 13)):
        legs += [("reset", None), ("rollout", E * H - 2)]
    legs += [("reset", None), ("rollout", 300 * H + 1)]
    legs += [("reset", None), ("rollout", 70_000)]
    legs += [("reset", None), ("rollout", 13), ("reset", _MASK), ("rollout", 120 * H - 2)]
    assert all(n % H != 0 for op, n in legs if op == "rollout")
    if H == 30:
        legs += [("reset", None), ("rollout", 300 * H)]
    return legs


@functools.lru_cache(maxsize=None)
def _tables(H, B):
    """deepsea_episodic_tables(size 9) with the reward of row r of instance b set to one of the values of its draw, (r + 3 b)
    mod their number, and the horizon set to H; row 0 of instance 0 .. 3 holds the four values, so that every batch has the
    four reward codes; the first 33 instances of the 65 are the 33."""
    from colosseum_amd.mdp.fast_batch import deepsea_episodic_tables

    vals = np.asarray(_VALS, np.float64)
    t = deepsea_episodic_tables(np.arange(900, 900 + B), _SIZE)
    S = int(t["state_off"][1])
    rew = np.zeros((B, S * 2), np.float64)
    for b in range(B):
        draw = np.asarray(_DRAWS[b % 4])
        rew[b] = vals[draw[(np.arange(S * 2) + 3 * b) % len(draw)]]
    assert set(np.unique(rew[:4]).tolist()) == set(_VALS)
    t["sp_reward"] = rew.reshape(-1).copy()
    t["sp_rp0"] = rew.reshape(-1).copy()
    t["H"] = H
    return t


def _keys(B):
    return (np.arange(B) * 15485863 + 43).astype(np.uint64)


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
def _oracle(H):
    """Per-instance OracleEnv runs of the script on the 65 instances (once per horizon, shared by both batch sizes): per launch
    last observation and reward sum; at the end visit counters, state and in-episode time; for the traced instances the
    reward trace and the in-episode time at the start of every launch."""
    t, keys, script = _tables(H, _BMAX), _keys(_BMAX), _script(H)
    n_legs = sum(op == "rollout" for op, _ in script)
    legs = [(np.zeros(_BMAX, np.int32), np.zeros(_BMAX, np.float64)) for _ in range(n_legs)]
    vs, vsa, cur, h, traces = [], [], np.zeros(_BMAX, np.int32), np.zeros(_BMAX, np.int32), {b: [] for b in _TRACED}
    for b in range(_BMAX):
        e = O.OracleEnv(_instance(t, b), rng_mode=1, philox_key=int(keys[b]))
        k = 0
        for op, arg in script:
            if op == "reset":
                if arg is None or arg[b]:
                    e.reset()
            else:
                h0 = int(e.state()[1])
                r = e.rollout(arg, trace=b in traces)
                legs[k][0][b], legs[k][1][b] = r["last_obs"], r["reward_sum"]
                if b in traces:
                    traces[b].append((h0, np.asarray(r["rew"], np.float64).copy()))
                k += 1
        v = e.visits()
        vs.append(np.asarray(v[0]).ravel())
        vsa.append(np.asarray(v[1]).ravel())
        cur[b], h[b], _ = e.state()
    return dict(legs=legs, vs=vs, vsa=vsa, cur=cur, h=h, traces=traces)


def _words(codes, H, h0):
    """the code words of a segment: ceil(H / 32) per episode, the steps of an episode from field 0 of its first word on"""
    n, nch = len(codes), (H + 31) // 32
    g = np.arange(n, dtype=np.int64) + h0
    e = g // H
    j = g % H - np.where(e == 0, h0, 0)
    words = np.zeros(int((h0 + n + H - 1) // H) * nch, np.uint64)
    np.add.at(words, e * nch + j // 32, np.asarray(codes, np.uint64) << (2 * (j % 32)).astype(np.uint64))
    return words


def _lane_stats(rew, H, h0):
    """The launch whose rewards are `rew`, through the scan's lane code segment by segment: (sum, counters, segments)."""
    lib = L.load()
    vals = np.asarray(_VALS, np.float64)
    codes = np.argmin(np.abs(rew[:, None] - vals[None, :]), axis=1)
    assert (vals[codes] == rew).all()   # (the table's rewards are the scaled rewards: rewards_range = (0, 1))
    r = vals.copy()
    total, s = np.zeros(8, np.int64), 0.0
    for p0 in range(0, len(rew), K1E_SEG):
        seg = codes[p0:p0 + K1E_SEG]
        hs = (h0 + p0) % H
        words = _words(seg, H, hs)
        out, stats = C.c_double(), np.zeros(8, np.int32)
        rc = lib.cmdp_k1e_scan_words_ex(words.ctypes.data, len(words), H, hs, len(seg), (H + 31) // 32, len(vals), r.ctypes.data, s,
                                        C.byref(out), stats.ctypes.data)
        assert rc == 0, lib.cmdp_last_error()
        s = out.value
        total += stats
    return s, total, -(-len(rew) // K1E_SEG)


@pytest.mark.gpu
@pytest.mark.parametrize("B", (33, 65))
@pytest.mark.parametrize("H", (9, 30, 45))
def test_k1e_scan_single_value_equals_oracle(need_gpu, H, B):
    tables, keys, script = _tables(H, B), _keys(B), _script(H)
    nch = (H + 31) // 32
    assert tuple(tables["rewards_range"]) == (0.0, 1.0)
    ref = _oracle(H)
    lengths = [n for op, n in script if op == "rollout"]
    # ---- the launches reach the paths they are meant for
    for b, trace in ref["traces"].items():
        for k, (h0, rew) in enumerate(trace):
            s, st, n_seg = _lane_stats(rew, H, h0)
            assert s == ref["legs"][k][1][b], (b, k)
            if len(rew) < 100 * H:
                continue
            if b in (0, 2, 3):   # one nonzero value: every tile that fails its advance is a single-value tile, no word is searched
                assert st[SINGLE] >= 1 and st[SINGLE] == st[SLOW] and st[WORD] == 0, (b, k, st.tolist())
                assert st[FADD] >= 1, (b, k, st.tolist())   # (every launch starts from 0.0: the float64 loop of the first tile)
            if b in (0, 2):      # ... and the sum leaves binades in integers
                assert st[CROSS] >= 1, (b, k, st.tolist())
            if b == 1:           # two nonzero values: the searching path, as before
                assert st[WORD] >= 1 and st[SLOW] > st[SINGLE], (b, k, st.tolist())
            if nch == 1:
                assert st[PLAIN] >= 1, (b, k, st.tolist())
            else:                # chunked episodes have no plain tile: the path is entered from the other branch
                assert st[PLAIN] == 0, (b, k, st.tolist())
    assert lengths[5] > K1E_SEG   # two segments
    # ---- the GPU
    env = BatchedMDP(tables=tables, rng_mode=L.RNG_PHILOX, philox_keys=keys)
    env.set_rollout_kernel(L.ROLLOUT_EPISODE_PARALLEL)
    k = 0
    for op, arg in script:
        if op == "reset":
            env.reset(None if arg is None else arg[:B])
            continue
        out = env.rollout(arg)
        assert env.lds_plan()["kernel"] == "k_rollout_epi"
        if arg % H == 0:
            assert env.k1e_plan()["last_form"] == "pair"   # whole episodes from reset on an even horizon
        o_last, o_sum = ref["legs"][k]
        assert (out["reward_sum"] == o_sum[:B]).all(), (k, arg, np.flatnonzero(out["reward_sum"] != o_sum[:B])[:8])
        np.testing.assert_array_equal(out["last_obs"], o_last[:B], err_msg=f"launch {k}")
        k += 1
    vs, vsa = env.visits()
    cur, h, _ = env.state()
    env.close()
    np.testing.assert_array_equal(vs, np.concatenate(ref["vs"][:B]))
    np.testing.assert_array_equal(vsa, np.concatenate(ref["vsa"][:B]))
    np.testing.assert_array_equal(cur, ref["cur"][:B])
    np.testing.assert_array_equal(h, ref["h"][:B])
