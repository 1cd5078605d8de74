"""K1E's pair form (csrc/cmdp_k1e_pair.h): launches of whole episodes walked from reset take TWO transitions per LDS atomic,
on a table with one row per (state at an even in-episode time, action pair).

CPU: the host plan (plan_k1e_pair, read through cmdp_k1e_pair_plan_desc: no handle, no device) -- eligibility, the even-time
states recomputed by breadth-first search over the layers of the tables, every pair word; and the count algebra of the fold
(pair counts -> the reference's arrival counts) against the same walk done row by row, in numpy.
GPU: every case asserts the form each launch took, then compares last observation, float64 reward sum, visits_s, visits_sa,
state, in-episode time, reset flags and a 131-transition continuation with == against the CPU oracle and against the same
script on a handle created with CMDP_K1E_PAIR=0."""
import functools
import os

import numpy as np
import pytest

from colosseum_amd import _lib as L
from colosseum_amd.batched import BatchedMDP, k1e_pair_plan_of_tables
from colosseum_amd.mdp import make_model
from colosseum_amd.mdp.fast_batch import deepsea_episodic_tables
from helpers_det import tables as det_tables
from oracle import oracle as O


# ---- the batches ---------------------------------------------------------------------------------------------------------

def _deepsea(size, B, H=None):
    t = deepsea_episodic_tables(np.arange(1000, 1000 + B), size)
    if H is not None:
        t["H"] = H
    return t


def _det_even(B=37):
    """A generated batch (helpers_det): every instance its own graph of 40 states, horizon 12, four reward values, a non-zero
    start state -- and state 5 made absorbing in every instance (both rows lead back to it: self-loops in the fold)."""
    t = det_tables(4242, B, 40, H=12, n_rew=4, permuted=False, start="fixed")
    nxt = t["sp_next"].reshape(B, 40, 2)
    nxt[:, 5, :] = 5
    t["sp_next"] = nxt.reshape(-1)
    return t


@functools.lru_cache(maxsize=None)
def _tables(name):
    return {
        "deepsea30": lambda: _deepsea(30, 3),
        "deepsea8": lambda: _deepsea(8, 40),
        "deepsea2": lambda: _deepsea(2, 5),
        "deepsea20_h44": lambda: _deepsea(20, 33, H=44),
        "deepsea9": lambda: _deepsea(9, 4),
        "det_even": _det_even,
    }[name]()


def _graph(t):
    B, S = int(t["B"]), int(t["state_off"][1])
    return t["sp_next"].reshape(B, S, 2), t["sp_reward"].reshape(B, S, 2), np.asarray(t["start_state"])


def _even_states(nxt, start, H):
    """The states of one instance at even in-episode times t < H, layer by layer (no shortcut: every layer is formed)."""
    layer, E = {int(start)}, set()
    for _ in range(0, H, 2):
        E |= layer
        layer = {int(nxt[int(nxt[s, a0]), a1]) for s in layer for a0 in (0, 1) for a1 in (0, 1)}
    return E


def _codes(t):
    """Reward code of every row: index into the distinct values of the batch in order of first appearance."""
    r = np.asarray(t["sp_reward"], np.float64).view(np.uint64)
    vals, first, inv = np.unique(r, return_index=True, return_inverse=True)
    rank = np.empty(len(vals), np.int64)
    rank[np.argsort(first)] = np.arange(len(vals))
    B, S = int(t["B"]), int(t["state_off"][1])
    return rank[inv].reshape(B, S, 2)


# ---- CPU: the plan -------------------------------------------------------------------------------------------------------

_PLANS = {"deepsea30": (225, 256), "deepsea8": (16, 32), "deepsea2": (1, 32), "deepsea20_h44": (100, 128), "det_even": (None, 64)}


@pytest.mark.parametrize("name", list(_PLANS))
def test_pair_plan_tables(name):
    """ok, n_even, SP2 and LDS bytes of the plan; for a few instances E by breadth-first search, the map and its inverse, and
    every pair word: successor index, both codes, a zero successor field where s'' is not in E."""
    t = _tables(name)
    nxt, _, start = _graph(t)
    codes = _codes(t)
    B, S, H = int(t["B"]), nxt.shape[1], int(t["H"])
    n_even, SP2 = _PLANS[name]
    for b in sorted({0, 1 % B, B // 2, B - 1}):
        p = k1e_pair_plan_of_tables(t, instance=b)
        assert p["ok"] and p["H"] == H and p["SP2"] == SP2 and p["last_form"] is None, p
        assert p["lds_bytes"] <= 160 * 1024 and p["lds_bytes"] > 4 * SP2 * 128
        E = _even_states(nxt[b], start[b], H)
        assert n_even is None or (len(E) == n_even and p["n_even"] == n_even)
        assert len(E) <= p["n_even"] <= SP2 and p["n_even_instance"] == len(E)
        idx, inv, words = p["index"], p["inverse"], p["words"]
        assert {s for s in range(S) if idx[s] >= 0} == E and idx[start[b]] == 0
        assert sorted(idx[idx >= 0].tolist()) == list(range(len(E)))
        np.testing.assert_array_equal(idx[inv], np.arange(len(E)))
        for x, s in enumerate(inv):
            for q in range(4):
                a0, a1 = q & 1, q >> 1
                s1 = nxt[b, s, a0]
                s2 = nxt[b, s1, a1]
                w = int(words[x, q])
                assert w & 3 == codes[b, s, a0] and (w >> 2) & 3 == codes[b, s1, a1] and (w >> 4) & 7 == 0, (b, s, q)
                assert w >> 7 == (idx[s2] if s2 in E else 0), (b, s, q)
    if name == "det_even":
        d = {k: v for k, v in zip(("S", "n_rew"), (S, len(np.unique(t["sp_reward"]))))}
        assert d == {"S": 40, "n_rew": 4} and start[0] != 0 and (nxt[:, 5] == 5).all() and H % 2 == 0


def test_pair_plan_refusals():
    """An odd horizon, more than 256 even-time states (the 512-state batch of tests/test_gpu_rollout_plans.py: 4 SP2 x 128 B
    no longer fit beside the rings), more than four reward values (no K1E at all)."""
    assert not k1e_pair_plan_of_tables(_tables("deepsea9"))["ok"]
    big = det_tables(7, 64, 512, H=40, n_rew=4, permuted=True)
    nxt, _, start = _graph(big)
    assert len(_even_states(nxt[0], start[0], 40)) > 256
    p = k1e_pair_plan_of_tables(big)
    assert not p["ok"] and p["SP2"] == 0 and p["lds_bytes"] == 0
    assert not k1e_pair_plan_of_tables(det_tables(8, 8, 40, H=12, n_rew=5, permuted=False))["ok"]
    small = det_tables(7, 64, 100, H=40, n_rew=4, permuted=True)   # the same generator within the limit: planned
    assert k1e_pair_plan_of_tables(small)["ok"]


# ---- CPU: the count algebra ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["deepsea8", "deepsea20_h44", "det_even"])
def test_pair_count_algebra(name):
    """A few hundred whole episodes of three instances walked with the pair words (random action bits), counted per pair row,
    folded by the fold's rule -- a pair count c at (s, a0, a1) adds c to the arrivals of (s', a0) and of (s'', a1), and every
    reset counts the start state -- equal visits_s / visits_sa of the same walk done row by row as the reference counts it;
    and the code bits shifted in four per pair are the row-by-row reward codes, step j at bits 2 j."""
    t = _tables(name)
    nxt, _, start = _graph(t)
    codes = _codes(t)
    S, H = nxt.shape[1], int(t["H"])
    rng = np.random.default_rng(5)
    for b in (0, 1, int(t["B"]) - 1):
        p = k1e_pair_plan_of_tables(t, instance=b)
        inv, words = p["inverse"], p["words"]
        n_epi = 300
        acts = rng.integers(0, 2, (n_epi, H))
        # row by row, as BaseMDP.step counts: the ARRIVAL state under the action taken; reset counts the start state
        vs, vsa = np.zeros(S, np.int64), np.zeros((S, 2), np.int64)
        ref_codes = np.zeros((n_epi, H), np.int64)
        for e in range(n_epi):
            s = start[b]
            for j in range(H):
                a = acts[e, j]
                ref_codes[e, j] = codes[b, s, a]
                s = nxt[b, s, a]
                vs[s] += 1
                vsa[s, a] += 1
            vs[start[b]] += 1   # the episode ends: reset
        # the pair walk
        cnt = np.zeros((len(inv), 4), np.int64)
        for e in range(n_epi):
            x, cw = 0, 0
            for j in range(0, H, 2):
                q = acts[e, j] | (acts[e, j + 1] << 1)
                w = int(words[x, q])
                cnt[x, q] += 1
                cw |= (w & 15) << (2 * j)
                x = w >> 7
            assert cw == sum(int(c) << (2 * j) for j, c in enumerate(ref_codes[e])), (b, e)
        # the fold
        fs, fsa = np.zeros(S, np.int64), np.zeros((S, 2), np.int64)
        for x, s in enumerate(inv):
            for q in range(4):
                a0, a1 = q & 1, q >> 1
                s1 = nxt[b, s, a0]
                s2 = nxt[b, s1, a1]
                fsa[s1, a0] += cnt[x, q]
                fsa[s2, a1] += cnt[x, q]
        fs = fsa.sum(axis=1)
        fs[start[b]] += n_epi
        np.testing.assert_array_equal(fsa, vsa)
        np.testing.assert_array_equal(fs, vs)


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def _keys(B):
    return (np.arange(B) * 104729 + 17).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _models(size, B):
    return tuple(make_model("DeepSeaEpisodic", seed=300 + i, size=size) for i in range(B))


def _run(script, env_vars, models=None, tables=None, keys=None):
    """One handle created under `env_vars`, the script of ("reset", mask) / ("rollout", n) / ("step", None) / ("visits", None)
    legs on K1E; per rollout leg (last_obs, reward_sum, form of the launch), at the end visits, state and a 131-transition
    continuation."""
    saved = {k: os.environ.pop(k, None) for k in ("CMDP_K1E_PAIR", "CMDP_K1E_DEBUG")}
    os.environ.update(env_vars)
    try:
        if models is not None:
            env = BatchedMDP(list(models), rng_mode=L.RNG_PHILOX, philox_keys=keys, with_dp=False)
        else:
            env = BatchedMDP(tables=tables, rng_mode=L.RNG_PHILOX, philox_keys=keys)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    env.set_rollout_kernel(L.ROLLOUT_EPISODE_PARALLEL)
    assert env.k1e_plan()["last_form"] is None
    legs, forms = [], []
    for op, arg in script:
        if op == "reset":
            env.reset(arg)
        elif op == "step":
            env.step(np.zeros(env.B, np.int32))
        elif op == "visits":
            env.visits()
        else:
            out = env.rollout(arg)
            forms.append(env.k1e_plan()["last_form"])
            legs.append((out["last_obs"].copy(), out["reward_sum"].copy()))
    vs, vsa = env.visits()
    cur, h, nr = env.state()
    tail = env.rollout(131)
    plan = env.k1e_plan()
    env.close()
    return dict(legs=legs, forms=forms, vs=vs, vsa=vsa, cur=cur, h=h, nr=nr, plan=plan,
                tail=(tail["last_obs"].copy(), tail["reward_sum"].copy()))


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
            elif op == "step":
                e.step(0)
            elif op == "rollout":
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


def _check_models(size, B, script, forms):
    models, keys = _models(size, B), _keys(B)
    got = _run(script, {}, models=models, keys=keys)
    assert got["forms"] == list(forms), got["forms"]
    single = _run(script, {"CMDP_K1E_PAIR": "0"}, models=models, keys=keys)
    assert set(single["forms"]) == {"single"} and not single["plan"]["ok"]
    _assert_same(got, single)
    _assert_same(got, _oracle_models(models, keys, script))
    return got


_R = ("reset", None)
_MASK40 = (np.arange(40) % 3 == 0).astype(np.uint8)
_MODEL_CASES = {
    # name: (size, B, script, forms)
    "two_rounds_ragged_group": (8, 40, (_R, ("rollout", 8 * 256)), ["pair"]),
    "last_round_idle_chains": (8, 40, (_R, ("rollout", 8 * 1001)), ["pair"]),
    "one_and_two_episodes": (8, 40, (_R, ("rollout", 8), ("rollout", 16)), ["pair", "pair"]),
    "single_instance": (8, 1, (_R, ("rollout", 8 * 1001)), ["pair"]),
    "one_pair_per_episode": (2, 37, (_R, ("rollout", 2 * 300)), ["pair"]),
    "bench_table_shape": (30, 64, (_R, ("rollout", 30 * 256)), ["pair"]),
    # fallbacks: each takes the single form
    "odd_horizon": (9, 40, (_R, ("rollout", 9 * 256)), ["single"]),
    "not_a_multiple_then_multiple": (8, 40, (_R, ("rollout", 8 * 100 + 3), ("rollout", 8 * 100)), ["single", "single"]),
    "reset_restores": (8, 40, (_R, ("rollout", 8 * 100 + 3), _R, ("rollout", 8 * 100)), ["single", "pair"]),
    "masked_reset": (8, 40, (_R, ("rollout", 8 * 100), ("reset", _MASK40), ("rollout", 8 * 100)), ["pair", "single"]),
    "step_in_between": (8, 40, (_R, ("rollout", 8 * 100), ("step", None), ("rollout", 8 * 100)), ["pair", "single"]),
    # both forms, in both orders, before one visits()
    "mixed_pair_single_pair": (8, 40, (_R, ("rollout", 8 * 300), ("rollout", 8 * 50 + 5), _R, ("rollout", 8 * 200)),
                               ["pair", "single", "pair"]),
    "mixed_single_pair": (8, 40, (_R, ("rollout", 8 * 50 + 5), _R, ("rollout", 8 * 300), ("visits", None), ("rollout", 8 * 40)),
                          ["single", "pair", "pair"]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(_MODEL_CASES))
def test_pair_form_equals_single_form_and_oracle(need_gpu, case):
    size, B, script, forms = _MODEL_CASES[case]
    got = _check_models(size, B, script, forms)
    assert got["plan"]["ok"] == (size % 2 == 0)


@pytest.mark.gpu
def test_debug_16_keeps_the_single_form(need_gpu):
    """Bit 16 of CMDP_K1E_DEBUG keeps its meaning: every round the general way."""
    models, keys = _models(8, 40), _keys(40)
    script = (_R, ("rollout", 8 * 256))
    got = _run(script, {"CMDP_K1E_DEBUG": "16"}, models=models, keys=keys)
    assert got["forms"] == ["single"] and got["plan"]["ok"]
    _assert_same(got, _oracle_models(models, keys, script))


def _check_tables(t, legs_n, forms):
    """A table batch: reset, then the launches legs_n.  The oracle of a table batch is oracle.batch_rollout, one run from reset:
    last observation and visit counters after the launches so far, the reward sum of the first launch."""
    B = int(t["B"])
    keys = (np.arange(B) * 7919 + 3).astype(np.uint64)
    script = (_R,) + tuple(("rollout", n) for n in legs_n)
    got = _run(script, {}, tables=t, keys=keys)
    assert got["forms"] == list(forms), got["forms"]
    single = _run(script, {"CMDP_K1E_PAIR": "0"}, tables=t, keys=keys)
    assert set(single["forms"]) == {"single"}
    _assert_same(got, single)
    total = 0
    for k, n in enumerate(legs_n):
        total += n
        last, rsum, ovs, ovsa = O.batch_rollout(t, 0, B, total, rng_mode=1, philox_keys=keys, want_visits=True)
        np.testing.assert_array_equal(got["legs"][k][0], last)
        if k == 0:
            np.testing.assert_array_equal(got["legs"][k][1], rsum)
    np.testing.assert_array_equal(got["vs"], ovs)
    np.testing.assert_array_equal(got["vsa"], ovsa)
    H = int(t["H"])
    np.testing.assert_array_equal(got["h"], np.full(B, total % H))
    last2, _, _, _ = O.batch_rollout(t, 0, B, total + 131, rng_mode=1, philox_keys=keys, want_visits=True)
    np.testing.assert_array_equal(got["tail"][0], last2)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [44 * 130, 44 * 1500])
def test_pair_form_two_code_words_per_episode(need_gpu, n):
    """DeepSea(20) under a horizon of 44: two code words per episode; 44 x 1500 transitions are two segments, and 61 440 is no
    multiple of 44."""
    _check_tables(_tables("deepsea20_h44"), [n], ["pair"])


@pytest.mark.gpu
def test_pair_form_generated_batch(need_gpu):
    """The generated batch: self-loops in the fold, four reward codes, a non-zero start state; two launches."""
    _check_tables(_tables("det_even"), [12 * 700, 12 * 3], ["pair", "pair"])
