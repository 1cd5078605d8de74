"""K1E's reward scan on the GPU (csrc/cmdp_k1e.h, k_reward_scan): plain tiles (step counts per code and one integer advance),
the slow path behind them, the unpredicated loads and the predicated ones at ragged ends -- through BatchedMDP.rollout
against per-instance OracleEnv runs: reward sums compared with ==, last observations and counters with assert_array_equal.

Before the comparison the oracle's reward trace of an instance, turned into code words, goes through the scan's own lane
code on the CPU (cmdp_k1e_scan_words), segment by segment as launch_k1e cuts a launch: its statistics prove that the launch
takes plain AND slow tiles, so a case cannot pass by never leaving the general path."""
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
_TIE, _TIE8 = 2.0 ** -53, 0.75 + 2.0 ** -45   # tie cases in [1, 2) resp. [256, 512), as in test_k1e_code_words.py
_VARIANTS = {
    "three_values": (0.0, 0.5, 1.0),
    "four_values": (0.0, 0.5, 1.0, 0.25),
    "tie_case": (0.0, 0.5, _TIE, _TIE8),
}
_MASK = (np.arange(_BMAX) % 3 == 0).astype(np.uint8)


def _script(H):
    """("reset", mask or None) / ("rollout", n) legs.  Short launches from reset whose code words end at the boundaries of a
    tile and of the three rolling tiles (W = 7, 8, 9, 25 for one word per episode; 8, 10, 24, 26 for two), 300 episodes + 1,
    70 000 transitions (two segments: the second continues the first's sum), and a launch after a masked reset that leaves
    the lanes of a wavefront at two in-episode times, so that W differs between them.  Every length ends inside an episode
    (no launch takes the pair form, and a segment is K1E_SEG transitions)."""
    nch = (H + 31) // 32
    legs = []
    for E in ((7, 8, 9, 25) if nch == 1 else (4, 5, 12, 13)):
        legs += [("reset", None), ("rollout", E * H - 2)]
    legs += [("reset", None), ("rollout", 300 * H + 1)]
    legs += [("reset", None), ("rollout", 70_000)]
    legs += [("reset", None), ("rollout", 13), ("reset", _MASK), ("rollout", 120 * H - 2)]
    assert all(n % H != 0 for op, n in legs if op == "rollout")
    return legs


@functools.lru_cache(maxsize=None)
def _tables(variant, H, B):
    """deepsea_episodic_tables(size 9) with the reward of row r of instance b set to values[(r + 3 b) mod n] and the horizon
    set to H (H = 45: two code words per episode, the second one partial); the first 33 instances of the 65 are the 33."""
    from colosseum_amd.mdp.fast_batch import deepsea_episodic_tables

    vals = np.asarray(_VARIANTS[variant], np.float64)
    t = deepsea_episodic_tables(np.arange(700, 700 + B), _SIZE)
    S = int(t["state_off"][1])
    rows = np.arange(S * 2)[None, :] + 3 * np.arange(B)[:, None]
    rew = vals[rows % len(vals)].reshape(-1)
    t["sp_reward"] = rew.copy()
    t["sp_rp0"] = rew.copy()
    t["H"] = H
    return t


def _keys(B):
    return (np.arange(B) * 15485863 + 41).astype(np.uint64)


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
    """Per-instance OracleEnv runs of the script on the 65 instances (once per configuration, shared by both batch sizes): per
    launch last observation and reward sum; at the end visit counters, state and in-episode time; for instances 0 and 1 the
    reward trace and the in-episode time at the start of every launch."""
    t, keys, script = _tables(variant, H, _BMAX), _keys(_BMAX), _script(H)
    n_legs = sum(op == "rollout" for op, _ in script)
    legs = [(np.zeros(_BMAX, np.int32), np.zeros(_BMAX, np.float64)) for _ in range(n_legs)]
    vs, vsa, cur, h, traces = [], [], np.zeros(_BMAX, np.int32), np.zeros(_BMAX, np.int32), {0: [], 1: []}
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


def _lane_stats(rew, H, h0, vals):
    """The launch whose rewards are `rew`, through the scan's lane code segment by segment: (sum, statistics, segments)."""
    lib = L.load()
    vals = np.asarray(vals, np.float64)
    codes = np.argmin(np.abs(rew[:, None] - vals[None, :]), axis=1)
    assert (vals[codes] == rew).all()   # (the table's rewards are the scaled rewards: rewards_range = (0, 1))
    r = np.zeros(4, np.float64)
    r[:len(vals)] = vals
    total, s = np.zeros(4, np.int64), 0.0
    for p0 in range(0, len(rew), K1E_SEG):
        seg = codes[p0:p0 + K1E_SEG]
        hs = (h0 + p0) % H
        words = _words(seg, H, hs)
        out, stats = C.c_double(), np.zeros(4, np.int32)
        rc = lib.cmdp_k1e_scan_words(words.ctypes.data, len(words), H, hs, len(seg), (H + 31) // 32, len(vals), r.ctypes.data, s,
                                     C.byref(out), stats.ctypes.data)
        assert rc == 0, lib.cmdp_last_error()
        s = out.value
        total += stats
    return s, total, -(-len(rew) // K1E_SEG)


@pytest.mark.gpu
@pytest.mark.parametrize("B", (33, 65))
@pytest.mark.parametrize("H", (9, 45))
@pytest.mark.parametrize("variant", list(_VARIANTS))
def test_k1e_scan_paths_equal_oracle(need_gpu, variant, H, B):
    tables, keys, script = _tables(variant, H, B), _keys(B), _script(H)
    vals, nch = _VARIANTS[variant], (H + 31) // 32
    assert tuple(tables["rewards_range"]) == (0.0, 1.0)
    ref = _oracle(variant, H)
    lengths = [n for op, n in script if op == "rollout"]
    # ---- the launches reach the paths they are meant for (instance 0; in the last launch instance 1 as well, which starts
    # at another in-episode time and owns one episode more)
    for b, trace in ref["traces"].items():
        for k, (h0, rew) in enumerate(trace):
            s, (plain, slow, word, rebase), n_seg = _lane_stats(rew, H, h0, vals)
            assert s == ref["legs"][k][1][b], (b, k)
            long_enough = len(rew) >= 100 * H
            if nch == 1 and long_enough:
                # (on the host a tile is plain by the lane's own w0: every tile of a segment but its first and the one that
                # holds its last word.  More slow tiles than those two per segment: a plain tile's integer advance failed
                # and the lane went on to the slow path from there)
                assert plain >= 1 and slow > 2 * n_seg and word >= 1, (b, k, plain, slow, word, n_seg)
            elif long_enough:   # chunked episodes have no plain tile
                assert plain == 0 and slow >= 1 and word >= 1, (b, k, plain, slow, word)
    W = [-(-n // H) * nch for n in lengths[:4]]
    assert W == ([7, 8, 9, 25] if nch == 1 else [8, 10, 24, 26])
    assert lengths[5] > K1E_SEG   # two segments
    h_last = [ref["traces"][b][-1][0] for b in (0, 1)]
    assert h_last[0] == 0 and h_last[1] == 13 % H
    assert -(-(h_last[0] + lengths[-1]) // H) != -(-(h_last[1] + lengths[-1]) // H)   # W differs within the wavefront
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
