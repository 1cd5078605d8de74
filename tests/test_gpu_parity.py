"""GPU parity tests: the HIP path (through the C ABI of libcmdp.so) against the reference's golden
vectors and against the CPU oracle.  Integer results (states, step types, visit counts, sweep counts)
bit-exact; float rewards bit-exact (deterministic values); value functions within 1e-6 relative
(BASELINE.json north_star), and bit-exact against the oracle which shares the accumulation order."""
import numpy as np
import pytest

from conftest import load_golden
from colosseum_amd import _lib as L
from colosseum_amd.batched import BatchedMDP
from colosseum_amd.mdp import make_model
from oracle import oracle as O

pytestmark = pytest.mark.gpu

VTOL = dict(rtol=1e-6, atol=1e-6)


def _models(cases):
    return [make_model(c["cls"], **c["kwargs"]) for c in cases]


@pytest.mark.parametrize("name", ["G1_deepsea8", "G2_deepsea30"])
def test_trajectories_vs_reference_batched(need_gpu, name):
    """All golden DeepSea cases as ONE batch, driven by the stored action streams."""
    z, cases = load_golden(name)
    models = _models(cases)
    env = BatchedMDP(models, rng_mode=L.RNG_MT_COMPAT, with_dp=False)
    first = env.reset()
    n = len(z["c0_actions"])
    acts = np.stack([z[f"c{i}_actions"] for i in range(len(cases))], 1)
    out = env.rollout(n, acts, trace=True)
    vs, vsa = env.visits()
    for i in range(len(cases)):
        k = f"c{i}_"
        assert first[i] == z[k + "resets"][0]
        np.testing.assert_array_equal(out["obs"][:, i], z[k + "obs"].astype(np.int32))
        np.testing.assert_array_equal(out["rew"][:, i], z[k + "rew"])
        np.testing.assert_array_equal(out["stype"][:, i], z[k + "stype"])
        np.testing.assert_array_equal(env.split_states(vs)[i], z[k + "visits_s"])
        np.testing.assert_array_equal(env.split_rows(vsa)[i].reshape(-1, env.A), z[k + "visits_sa"])
        assert out["reward_sum"][i] == pytest.approx(float(np.sum(z[k + "rew"])), abs=1e-9)
    env.close()


def test_trajectories_stochastic_mt_compat(need_gpu):
    """Stochastic dynamics: per-(s,a) MT19937 streams on the device reproduce the reference draw for draw
    (12 000 steps, crossing the reference's 5000-sample refills).  Ragged: one handle per case."""
    for name in ("G3_stochastic", "G12_families"):
        _check_mt_compat_trajectories(*load_golden(name))


def _check_mt_compat_trajectories(z, cases):
    for i, c in enumerate(cases):
        k = f"c{i}_"
        m = make_model(c["cls"], **c["kwargs"])
        if not m.deterministic_rewards:  # Beta rewards: host sampler, tests/test_rewards.py
            continue
        env = BatchedMDP([m], rng_mode=L.RNG_MT_COMPAT, with_dp=False)
        first = env.reset()
        acts = z[k + "actions"][:, None]
        out = env.rollout(len(acts), acts, trace=True)
        vs, vsa = env.visits()
        assert first[0] == z[k + "resets"][0], c
        np.testing.assert_array_equal(out["obs"][:, 0], z[k + "obs"], err_msg=str(c))
        np.testing.assert_array_equal(out["rew"][:, 0], z[k + "rew"])
        np.testing.assert_array_equal(out["stype"][:, 0], z[k + "stype"])
        np.testing.assert_array_equal(vs, z[k + "visits_s"])
        if k + "visits_sa" in z:
            np.testing.assert_array_equal(vsa.reshape(-1, env.A), z[k + "visits_sa"])
        env.close()


def test_step_api_matches_rollout_and_reference(need_gpu):
    """cmdp_step one call per transition (BaseMDP.step semantics incl. the needs-reset assert)."""
    z, cases = load_golden("G1_deepsea8")
    models = _models(cases)
    env = BatchedMDP(models, with_dp=False)
    with pytest.raises(AssertionError):
        env.step(np.zeros(env.B, np.int32))  # reset pending
    obs = env.reset()
    n = 300
    resets = [1] * env.B
    for t in range(n):
        a = np.array([z[f"c{i}_actions"][t] for i in range(env.B)], np.int32)
        o, r, ty = env.step(a)
        for i in range(env.B):
            k = f"c{i}_"
            assert o[i] == z[k + "obs"][t] and r[i] == z[k + "rew"][t] and ty[i] == z[k + "stype"][t]
        if (ty == 2).any():
            assert (ty == 2).all()  # same horizon
            with pytest.raises(AssertionError):
                env.step(a)
            o2 = env.reset()
            for i in range(env.B):
                assert o2[i] == z[f"c{i}_resets"][resets[i]]
                resets[i] += 1
    with pytest.raises(L.CmdpError):
        env.step(np.full(env.B, 7, np.int32))  # action out of range
    env.close()


def test_step_auto_reset(need_gpu):
    z, cases = load_golden("G1_deepsea8")
    m = make_model(cases[0]["cls"], **cases[0]["kwargs"])
    env = BatchedMDP([m], with_dp=False)
    o, r, ty = env.step([0], auto_reset=True)  # behaves as reset()
    assert ty[0] == 0 and r[0] == 0.0 and o[0] == m.start_states[0]
    for t in range(m.H):
        o, r, ty = env.step([0], auto_reset=True)
    assert ty[0] == 2 and o[0] == -1
    o, r, ty = env.step([1], auto_reset=True)
    assert ty[0] == 0 and o[0] == m.start_states[0]
    env.close()


def test_philox_rollout_vs_oracle(need_gpu):
    """Throughput mode: GPU and CPU oracle share the Philox streams -> bit-exact states/visits/rewards,
    on-device random policy, deterministic (DeepSea) and stochastic (FrozenLake, MiniGrid) dynamics."""
    specs = [("DeepSeaEpisodic", dict(seed=s, size=30)) for s in range(6)]
    models = [make_model(c, **k) for c, k in specs]
    keys = np.array([0x9E3779B97F4A7C15 ^ (i * 0x1000003) for i in range(len(models))], np.uint64)
    env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=keys, with_dp=False)
    env.reset()
    out = env.rollout(5000, None, trace=True)
    out2 = env.rollout(777, None, trace=False)  # counters persist across launches
    vs, vsa = env.visits()
    for i, m in enumerate(models):
        e = O.OracleEnv(m, rng_mode=1, philox_key=int(keys[i]))
        e.reset()
        ref = e.rollout(5000)
        ref2 = e.rollout(777, trace=False)
        np.testing.assert_array_equal(out["obs"][:, i], ref["obs"])
        np.testing.assert_array_equal(out["rew"][:, i], ref["rew"])
        np.testing.assert_array_equal(out["stype"][:, i], ref["stype"])
        assert out["reward_sum"][i] == ref["reward_sum"] and out2["reward_sum"][i] == ref2["reward_sum"]
        assert out2["last_obs"][i] == ref2["last_obs"]
        rvs, rvsa = e.visits()
        np.testing.assert_array_equal(env.split_states(vs)[i], rvs)
        np.testing.assert_array_equal(env.split_rows(vsa)[i].reshape(-1, 2), rvsa)
    env.close()
    for cls, kw in [("FrozenLakeContinuous", dict(seed=3, size=12, p_frozen=0.9, p_rand=0.1)),
                    ("MiniGridEmptyEpisodic", dict(seed=1, size=6, p_rand=0.2, n_starting_states=3)),
                    ("MiniGridRoomsContinuous", dict(seed=2, room_size=3, n_rooms=4, p_lazy=0.2, n_starting_states=2))]:
        m = make_model(cls, **kw)
        env = BatchedMDP([m, m], rng_mode=L.RNG_PHILOX, philox_keys=[11, 12], with_dp=False)
        env.reset()
        out = env.rollout(4000, None, trace=True)
        vs, vsa = env.visits()
        for i in range(2):
            e = O.OracleEnv(m, rng_mode=1, philox_key=11 + i)
            e.reset()
            ref = e.rollout(4000)
            np.testing.assert_array_equal(out["obs"][:, i], ref["obs"], err_msg=cls)
            np.testing.assert_array_equal(out["rew"][:, i], ref["rew"])
            rvs, rvsa = e.visits()
            np.testing.assert_array_equal(env.split_states(vs)[i], rvs)
        assert not np.array_equal(out["obs"][:, 0], out["obs"][:, 1])
        env.close()


def test_lds_resident_rollout_equals_global_kernel_and_oracle(need_gpu):
    """K1L (tables + 16-bit count deltas in LDS) vs the lane-per-instance kernel vs the oracle: 70 000
    transitions (crosses the 32 768-step flush of the 16-bit deltas), ragged batch sizes (B not a multiple of the
    instances-per-workgroup), visits / last observation / reward sums bit-equal."""
    from colosseum_amd.mdp.fast_batch import deepsea_episodic_tables

    # horizon 5 < 8: several episode ends inside one group of 8 transitions; horizon 3: a row is arrived at every twelfth
    # transition, so K1T's 8-bit deltas wrap before its flush period is over (its overflow list is used)
    for size, n2 in ((12, 70_000), (5, 9_000), (3, 9_000)):
        _check_lds_rollout(75, size, 50, n2, expect_k1t=True, k1t_g=50, expect_k1e=True)   # K1T: groups of 50 and 25; K1E: 32 + 32 + 11
    # K1T with both halves of a workgroup in use (100 instances per group, the last group holds 61: half 1 empty)
    _check_lds_rollout(261, 9, 50, 8_000, expect_k1t=True, k1t_g=100, expect_k1e=True)
    # K1U with all four quarters of a workgroup in use (250 per group, the last group holds 97: quarters 2, 3 empty / ragged)
    _check_lds_rollout(597, 7, 50, 4_000, expect_k1t=True, k1t_g=250, expect_k1e=True)
    # horizon 40 > 32: two code words per episode (K1E walks an episode in 32-step chunks)
    _check_lds_rollout(70, 40, 77, 3_001, expect_k1e=False, k1t_g=35)   # 820 states: no room for 32 private tables -- K1E must refuse
    t45 = deepsea_episodic_tables(np.arange(1000, 1070), 20)
    t45["H"] = 45   # DeepSea-20's graph (the bottom row leads back to the start) under a horizon of 45: K1E's second code word
    _check_lds_rollout(70, None, 77, 5_003, tables=t45, expect_k1e=True, k1t_g=35)
    t33 = deepsea_episodic_tables(np.arange(1000, 1033), 9)
    t33["H"] = 64   # exactly two full code words per episode; one full workgroup and one instance in the next
    _check_lds_rollout(33, None, 64, 6_400, tables=t33, expect_k1e=True, k1t_g=20)
    _check_lds_rollout(40, 31, 77, 9_001, expect_k1t=True, k1t_g=40, expect_k1e=True)


def _check_lds_rollout(B, size, n1, n2, tables=None, models=None, expect_k1t=None, k1t_g=128, expect_k1e=None):
    """expect_k1t: True = the shared-table kernel must take the batch, False = it must refuse it, None = either;
    expect_k1e likewise for the episode-parallel kernel."""
    import os

    from colosseum_amd.mdp.fast_batch import deepsea_episodic_tables

    seeds = np.arange(1000, 1000 + B)
    if models is not None:
        from colosseum_amd.batched import tables_from_models
        tables = tables_from_models(models, True, False)
    elif tables is None:
        tables = deepsea_episodic_tables(seeds, size)
    keys = (seeds * 7919).astype(np.uint64)
    res = {}
    # the LDS-resident rollout exists as the fused walker (K1L) and as the wavefront pipeline (K1P); CMDP_K1L_PIPE
    # (read when the handle is created) forces one of them
    # ... and, for two-action batches whose instances are action-permuted copies of one MDP, as the shared-table
    # pipeline K1T (CMDP_K1T_G: instances per workgroup, so that small batches exercise both halves and ragged groups)
    # ... and as K1U, K1T's chain with the trace streamed to HBM and histogrammed by a second kernel (CMDP_K1U_G likewise;
    # a launch longer than 32 768 transitions runs as several segments)
    # ... and, for episodic two-action batches, as the episode-parallel kernel K1E (lane = (instance, episode); a launch
    # longer than 61 440 transitions runs as several segments)
    TMPL = (L.ROLLOUT_LDS_TEMPLATE, L.ROLLOUT_LDS_TEMPLATE_STREAM, L.ROLLOUT_EPISODE_PARALLEL)
    for which, pipe in ((L.ROLLOUT_GLOBAL, None), (L.ROLLOUT_LDS, "0"), (L.ROLLOUT_LDS, "1"), (L.ROLLOUT_LDS_TEMPLATE, "1"),
                        (L.ROLLOUT_LDS_TEMPLATE_STREAM, "1"), (L.ROLLOUT_EPISODE_PARALLEL, "1")):
        saved = os.environ.pop("CMDP_K1L_PIPE", None)
        if pipe is not None:
            os.environ["CMDP_K1L_PIPE"] = pipe
        if which in TMPL:
            os.environ["CMDP_K1T_G"] = str(k1t_g)
            os.environ["CMDP_K1U_G"] = str(k1t_g)
        try:
            env = BatchedMDP(tables=tables, rng_mode=L.RNG_PHILOX, philox_keys=keys)
        finally:
            os.environ.pop("CMDP_K1L_PIPE", None)
            os.environ.pop("CMDP_K1T_G", None)
            os.environ.pop("CMDP_K1U_G", None)
            if saved is not None:
                os.environ["CMDP_K1L_PIPE"] = saved
        env.set_rollout_kernel(which)
        if which == L.ROLLOUT_LDS:
            plan = env.lds_plan()
            assert plan["eligible"] and plan["kernel"] == ("k_rollout_pipe" if pipe == "1" else "k_rollout_lds"), plan
        env.reset()
        try:
            a = env.rollout(n1)  # odd transition count: the next launch starts mid Philox block and mid episode
        except L.CmdpError as e:  # K1T exists for A = 2 and action-permuted copies of one MDP; it must say so otherwise
            assert which in TMPL and e.code == L.ERR_UNSUPPORTED and not (expect_k1e if which == L.ROLLOUT_EPISODE_PARALLEL else expect_k1t), e
            env.close()
            continue
        if which == L.ROLLOUT_EPISODE_PARALLEL:
            plan = env.lds_plan()
            assert expect_k1e is not False and plan["kernel"] == "k_rollout_epi" and plan["instances_per_workgroup"] == 32, plan
        if which == L.ROLLOUT_LDS_TEMPLATE:
            plan = env.lds_plan()
            assert expect_k1t is not False and plan["kernel"] == "k_rollout_tmpl" and plan["instances_per_workgroup"] == min(k1t_g, 128), plan
        if which == L.ROLLOUT_LDS_TEMPLATE_STREAM:
            plan = env.lds_plan()
            assert expect_k1t is not False and plan["kernel"] == "k_rollout_tmpl_stream" and plan["instances_per_workgroup"] == min(k1t_g, 256), plan
        b = env.rollout(n2)
        c = env.rollout(3)   # shorter than one Philox block / one group of 8
        vs, vsa = env.visits()
        res[(which, pipe)] = (a["last_obs"], a["reward_sum"], b["last_obs"], b["reward_sum"], c["last_obs"],
                              c["reward_sum"], vs, vsa, env.state())
        env.close()
    if expect_k1t:
        assert (L.ROLLOUT_LDS_TEMPLATE, "1") in res and (L.ROLLOUT_LDS_TEMPLATE_STREAM, "1") in res
    if expect_k1e:
        assert (L.ROLLOUT_EPISODE_PARALLEL, "1") in res
    g = res[(L.ROLLOUT_GLOBAL, None)]
    for key in ((L.ROLLOUT_LDS, "0"), (L.ROLLOUT_LDS, "1"), (L.ROLLOUT_LDS_TEMPLATE, "1"), (L.ROLLOUT_LDS_TEMPLATE_STREAM, "1"),
                (L.ROLLOUT_EPISODE_PARALLEL, "1")):
        if key not in res:
            continue
        l = res[key]
        for x, y in zip(g[:8], l[:8]):
            np.testing.assert_array_equal(x, y)
        for x, y in zip(g[8], l[8]):
            np.testing.assert_array_equal(x, y)
    l = res[(L.ROLLOUT_LDS, "1")]
    last, rsum, ovs, ovsa = O.batch_rollout(tables, 0, B, n1 + n2 + 3, rng_mode=1, philox_keys=keys, want_visits=True)
    np.testing.assert_array_equal(l[4], last)
    np.testing.assert_array_equal(l[6], ovs)
    np.testing.assert_array_equal(l[7], ovsa)
    # the oracle sums all rewards in one go; the launches' sums are separate partial sums
    np.testing.assert_allclose(l[1] + l[3] + l[5], rsum, rtol=1e-12)


def test_lds_rollout_continuous_and_other_families(need_gpu):
    """K1L / K1P on continuous (no horizon: the per-lane flavour of the walker) and episodic instances of other
    deterministic families, A = 2..5, against the HBM-table kernel and the oracle."""
    B = 70
    for cls, kw, k1t in (("DeepSeaContinuous", dict(size=9), True), ("SimpleGridContinuous", dict(size=7), False),
                         ("MiniGridEmptyEpisodic", dict(size=6), False), ("RiverSwimEpisodic", dict(size=40), None)):
        models = [make_model(cls, seed=1000 + i, **kw) for i in range(B)]
        _check_lds_rollout(B, None, 13, 9_001, models=models, expect_k1t=k1t, k1t_g=40, expect_k1e=False if "Continuous" in cls or cls.startswith("MiniGrid") else None)


def test_lds_rollout_with_per_instance_episode_phase(need_gpu):
    """A masked reset() leaves the instances of a batch at different in-episode times: the LDS walkers then run
    their per-lane flavour (no shared episode clock).  K1L, K1P and the HBM-table kernel against per-instance oracle
    environments: last observation, reward sum, visit counts, state."""
    import os

    B, size = 45, 9
    models = [make_model("DeepSeaEpisodic", seed=300 + i, size=size) for i in range(B)]
    keys = (np.arange(B) * 104729 + 17).astype(np.uint64)
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    n1, n2 = 13, 6_007
    res = {}
    for which, pipe in ((L.ROLLOUT_GLOBAL, None), (L.ROLLOUT_LDS, "0"), (L.ROLLOUT_LDS, "1"), (L.ROLLOUT_LDS_TEMPLATE, "1"),
                        (L.ROLLOUT_LDS_TEMPLATE_STREAM, "1"), (L.ROLLOUT_EPISODE_PARALLEL, "1")):
        saved = os.environ.pop("CMDP_K1L_PIPE", None)
        if pipe is not None:
            os.environ["CMDP_K1L_PIPE"] = pipe
        os.environ["CMDP_K1T_G"] = "30"
        os.environ["CMDP_K1U_G"] = "30"
        try:
            env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=keys, with_dp=False)
        finally:
            os.environ.pop("CMDP_K1L_PIPE", None)
            os.environ.pop("CMDP_K1T_G", None)
            os.environ.pop("CMDP_K1U_G", None)
            if saved is not None:
                os.environ["CMDP_K1L_PIPE"] = saved
        env.set_rollout_kernel(which)
        env.reset()
        env.rollout(n1)
        env.reset(mask)                       # every third instance back to h = 0, the others stay at h = 13 mod H
        assert len(set(env.state()[1].tolist())) > 1
        out = env.rollout(n2)
        vs, vsa = env.visits()
        res[(which, pipe)] = (out["last_obs"], out["reward_sum"], vs, vsa) + tuple(env.state())
        env.close()
    g = res[(L.ROLLOUT_GLOBAL, None)]
    for key in ((L.ROLLOUT_LDS, "0"), (L.ROLLOUT_LDS, "1"), (L.ROLLOUT_LDS_TEMPLATE, "1"), (L.ROLLOUT_LDS_TEMPLATE_STREAM, "1"),
                (L.ROLLOUT_EPISODE_PARALLEL, "1")):
        for x, y in zip(g, res[key]):
            np.testing.assert_array_equal(x, y)
    off = np.concatenate([[0], np.cumsum([m.n_states for m in models])])
    for b in range(B):
        e = O.OracleEnv(models[b], rng_mode=1, philox_key=int(keys[b]))
        e.reset()
        e.rollout(n1, trace=False)
        if mask[b]:
            e.reset()
        r = e.rollout(n2, trace=False)
        assert g[0][b] == r["last_obs"] and g[1][b] == r["reward_sum"], b
        np.testing.assert_array_equal(g[2][off[b]:off[b + 1]], e.visits()[0])


def test_episode_parallel_rollout_interleaved_with_everything_else(need_gpu):
    """K1E keeps DEPARTURE counts in an image of its own and folds them into the visit counters lazily, and its reward scan
    runs on a second stream: every other entry point must see the counters and sums as if each launch had finished on the spot.
    One handle, one oracle environment per instance, the same sequence on both: asynchronous K1E launches, per-step calls,
    masked resets, a launch of the HBM-table kernel, counter read-outs and resets in between -- visit counts (both arrays),
    states, in-episode times, reward sums compared with the oracle after every leg."""
    B, size = 37, 7
    models = [make_model("DeepSeaEpisodic", seed=50 + i, size=size) for i in range(B)]
    keys = (np.arange(B) * 2654435761 + 99).astype(np.uint64)
    env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=keys, with_dp=False)
    assert env.lds_plan()["kernel"] == "k_rollout_epi"
    oes = [O.OracleEnv(m, rng_mode=1, philox_key=int(keys[b])) for b, m in enumerate(models)]
    env.reset()
    for e in oes:
        e.reset()
    off = np.concatenate([[0], np.cumsum([m.n_states for m in models])])

    def check(tag, sums=None, osums=None):
        vs, vsa = env.visits()
        cur, h, _ = env.state()
        for b, e in enumerate(oes):
            rvs, rvsa = e.visits()
            np.testing.assert_array_equal(vs[off[b]:off[b + 1]], rvs, err_msg=tag)
            np.testing.assert_array_equal(vsa[2 * off[b]:2 * off[b + 1]].reshape(-1, 2), rvsa, err_msg=tag)
            oc, oh, _ = e.state()
            assert (cur[b], h[b]) == (oc, oh), (tag, b)
        if sums is not None:
            np.testing.assert_array_equal(sums, osums, err_msg=tag)

    def oracle_rollout(n):
        return np.array([e.rollout(n, trace=False)["reward_sum"] for e in oes])

    # two asynchronous K1E launches back to back (the second starts mid-episode), then a read-out
    env.rollout_async(333)
    env.rollout_async(1001)
    oracle_rollout(333)
    oracle_rollout(1001)
    check("after two async launches")
    # a synchronous launch right behind an asynchronous one: its sums come from the second stream
    env.rollout_async(70)
    out = env.rollout(4321)
    oracle_rollout(70)
    check("sync after async", out["reward_sum"], oracle_rollout(4321))
    # per-step calls (lane-per-instance kernel), with a masked reset in the middle
    for t in range(5):
        acts = (np.arange(B) + t) % 2
        env.step(acts.astype(np.int32), auto_reset=True)
        for b, e in enumerate(oes):
            if e.state()[2]:
                e.reset()
            else:
                e.step(int(acts[b]))
    mask = ((np.arange(B) % 4 == 1) | env.state()[2]).astype(np.uint8)   # every fourth instance + those a step left terminated
    env.reset(mask)
    for b, e in enumerate(oes):
        if mask[b]:
            e.reset()
    check("after steps and a masked reset")
    # K1E from per-lane episode phases, then the HBM-table kernel, then K1E again
    a = env.rollout(777)
    oa = oracle_rollout(777)
    env.set_rollout_kernel(L.ROLLOUT_GLOBAL)
    b_ = env.rollout(500)
    ob = oracle_rollout(500)
    env.set_rollout_kernel(L.ROLLOUT_AUTO)
    env.rollout_async(64)
    oracle_rollout(64)
    check("K1E / K1 / K1E", a["reward_sum"] + b_["reward_sum"], oa + ob)
    # a long asynchronous K1E launch, at once a synchronous one of fewer than 64 transitions (K1): K1 writes the reward
    # sums the K1E scan on the second stream writes too
    env.rollout_async(5000)
    short = env.rollout(10)
    oracle_rollout(5000)
    check("K1 right behind an async K1E", short["reward_sum"], oracle_rollout(10))
    # K1E, the streamed-trace kernel K1U forced on the same handle, K1E again
    env.rollout_async(2000)
    oracle_rollout(2000)
    env.set_rollout_kernel(L.ROLLOUT_LDS_TEMPLATE_STREAM)
    assert env.lds_plan()["kernel"] == "k_rollout_tmpl_stream"
    u = env.rollout(3000)
    ou = oracle_rollout(3000)
    env.set_rollout_kernel(L.ROLLOUT_AUTO)
    e2 = env.rollout(1500)
    oe2 = oracle_rollout(1500)
    check("K1E / K1U / K1E", u["reward_sum"] + e2["reward_sum"], ou + oe2)
    # counters reset while K1E's image holds counts: they must not come back
    env.rollout_async(3000)
    oracle_rollout(3000)
    env.reset_visits()
    for e in oes:
        e.reset_visits()
    env.rollout_async(129)
    oracle_rollout(129)
    check("after reset_visits")
    env.close()


def test_visit_counter_overflow_is_refused_not_wrapped(need_gpu):
    """The device counters are int32 (cmdp_visits widens them); the reference's are Python ints.  A counter restored near
    2^31 (cmdp_set_visits) must make a call that could carry it past 2^31 - 1 fail with CMDP_ERR_OVERFLOW BEFORE anything is
    stepped -- for every rollout kernel, the per-step API and reset -- and the handle stays usable."""
    from colosseum_amd.mdp.fast_batch import deepsea_episodic_tables

    tables = deepsea_episodic_tables(np.arange(40), 6)
    for which in (L.ROLLOUT_AUTO, L.ROLLOUT_GLOBAL, L.ROLLOUT_LDS_TEMPLATE_STREAM):
        env = BatchedMDP(tables=tables, rng_mode=L.RNG_PHILOX, philox_keys=np.arange(40, dtype=np.uint64) + 5)
        env.set_rollout_kernel(which)
        env.reset()
        env.rollout(600)
        vs, vsa = env.visits()
        start = int(tables["start_state"][0])
        vs2 = vs.copy()
        vs2[start] = 2**31 - 1 - 200            # instance 0's start state: 100 more transitions are the most that is safe
        env.set_visits(vs2, vsa)
        before = [a.copy() for a in env.state()]
        with pytest.raises(L.CmdpError) as ei:
            env.rollout(101)
        assert ei.value.code == L.ERR_OVERFLOW
        for a, b in zip(before, env.state()):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(env.visits()[0], vs2)        # nothing was counted
        env.set_rollout_kernel(L.ROLLOUT_LDS_STOCHASTIC)           # refused calls take no room
        for _ in range(3):
            with pytest.raises(L.CmdpError) as ei:
                env.rollout(100)
            assert ei.value.code == L.ERR_UNSUPPORTED
        env.set_rollout_kernel(which)
        env.rollout(100)                                           # this much fits
        vs3, _ = env.visits()
        assert vs3[start] > vs2[start] and vs3.min() >= 0 and vs3[start] <= 2**31 - 1
        with pytest.raises(L.CmdpError) as ei:
            env.step(np.zeros(40, np.int32))
        assert ei.value.code == L.ERR_OVERFLOW
        env.reset_visits()
        env.rollout(5000)                                          # counters cleared: room again
        assert env.visits()[0].reshape(40, -1).sum(1).min() >= 5000
        env.close()
    # a call refused because an instance needs reset takes no room either: every instance at the end of an episode first
    # (cmdp_set_visits resets the bound), then exactly room for the reset (2) and 100 transitions (200)
    env = BatchedMDP(tables=tables, rng_mode=L.RNG_PHILOX, philox_keys=np.arange(40, dtype=np.uint64) + 5)
    env.reset()
    while not env.state()[2].all():
        env.step(np.zeros(40, np.int32), auto_reset=False)
    vs, vsa = env.visits()
    vs2 = vs.copy()
    vs2[int(tables["start_state"][0])] = 2**31 - 1 - 202
    env.set_visits(vs2, vsa)
    with pytest.raises(AssertionError, match="needs reset"):     # (CMDP_ERR_NEEDS_RESET: the reference's AssertionError)
        env.rollout(100)
    env.reset()
    env.rollout(100)
    env.close()
    with pytest.raises(L.CmdpError):                               # values beyond int32 cannot be restored
        env = BatchedMDP(tables=tables, rng_mode=L.RNG_PHILOX)
        bad = np.zeros(int(tables["state_off"][-1]), np.int64)
        bad[3] = 2**31
        env.set_visits(bad, None)


def test_lds_kernel_refused_when_not_eligible(need_gpu):
    m = make_model("FrozenLakeContinuous", seed=0, size=5, p_frozen=0.9)
    env = BatchedMDP([m], rng_mode=L.RNG_PHILOX, with_dp=False)
    env.set_rollout_kernel(L.ROLLOUT_LDS)
    env.reset()
    with pytest.raises(L.CmdpError) as ei:
        env.rollout(100)
    assert ei.value.code == L.ERR_UNSUPPORTED
    env.set_rollout_kernel(L.ROLLOUT_AUTO)
    env.rollout(100)
    env.close()


def test_vi_frozenlake20_vs_reference(need_gpu):
    """Config C3 slice: FrozenLake 20x20 discounted VI; Jacobi (the scheme the reference's rule selects)
    bit-exact incl. sweep counts; Gauss-Seidel within tolerance (the reference's BLAS summation order is
    not reproducible), bit-exact against the oracle."""
    z, cases = load_golden("G4_frozenlake20_vi")
    models = _models(cases)
    dp = BatchedMDP(models, with_env=False)
    for eps, tag in ((1e-3, "e3"), (1e-6, "e6")):
        Q, V, sw = dp.value_iteration(0.99, eps, L.SCHEME_AUTO)
        Qg, Vg, swg = dp.value_iteration(0.99, eps, L.SCHEME_GAUSS_SEIDEL)
        for i, c in enumerate(cases):
            k = f"c{i}_"
            assert c["reference_rule_selects"] == "jacobi"
            np.testing.assert_array_equal(dp.split_states(V)[i], z[k + f"jac_{tag}_V"])
            np.testing.assert_array_equal(dp.split_rows(Q)[i].reshape(-1, 4), z[k + f"jac_{tag}_Q"])
            np.testing.assert_array_equal(dp.split_states(V)[i], z[k + f"disp_{tag}_V"])
            assert sw[i] == c[f"jac_{tag}_sweeps"]
            # Gauss-Seidel: the reference's `T[s] @ V` is BLAS sgemv, whose accumulation order belongs to the BLAS KERNEL of
            # the CPU it runs on.  oracle/gs_blas_experiment.py ran the reference's own function on these very instances
            # under six OpenBLAS kernel families (profiles/r03_gs_blas_kernels.json): two runs of the REFERENCE differ by up
            # to 2.86e-6 (Sandybridge vs Haswell / Zen / SkylakeX), this build's in-order restatement is 1.07e-6 from the
            # Haswell-family runs (the golden's) and 2.74e-6 from the Nehalem / Sandybridge ones -- inside the reference's
            # own spread, which is why the bound here is not the north star's 1e-6
            np.testing.assert_allclose(dp.split_states(Vg)[i], z[k + f"gs_{tag}_V"], rtol=0, atol=2e-6)
            np.testing.assert_allclose(dp.split_rows(Qg)[i].reshape(-1, 4), z[k + f"gs_{tag}_Q"], rtol=0, atol=2e-6)
            assert abs(int(swg[i]) - c[f"gs_{tag}_sweeps"]) <= 1
            m = models[i]
            oQ, oV, oit, _ = O.vi_discounted(m.n_states, 4, m.csr(), m.reward_matrix(), 0.99, eps, 2)
            np.testing.assert_array_equal(dp.split_states(Vg)[i], oV)
            np.testing.assert_array_equal(dp.split_rows(Qg)[i].reshape(-1, 4), oQ)
            assert swg[i] == oit
    pis = [np.ones((m.n_states, 4), np.float32) / 4 for m in models]
    Q, V, sw = dp.policy_evaluation(pis, 0.99, 1e-5, L.SCHEME_JACOBI)
    Qg, Vg, swg = dp.policy_evaluation(pis, 0.99, 1e-5, L.SCHEME_GAUSS_SEIDEL)
    for i, c in enumerate(cases):
        k = f"c{i}_"
        np.testing.assert_array_equal(dp.split_states(V)[i], z[k + "pe_jac_V"])
        np.testing.assert_array_equal(dp.split_rows(Q)[i].reshape(-1, 4), z[k + "pe_jac_Q"])
        assert sw[i] == c["pe_jac_sweeps"]
        np.testing.assert_allclose(dp.split_states(Vg)[i], z[k + "pe_gs_V"], **VTOL)
        assert abs(int(swg[i]) - c["pe_gs_sweeps"]) <= 1
    dp.close()


def test_register_resident_sweeps_equal_workgroup_kernel_and_oracle(need_gpu):
    """K2R (CSR in registers), K2U (its distinct-successor form), K2W (one wavefront per instance) vs K2 (CSR in LDS/HBM)
    vs the oracle on A = 2, 3, 4, ragged batches, VI and PE."""
    batches = [
        [make_model("DeepSeaContinuous", seed=s, size=sz, p_rand=0.2) for s, sz in ((0, 9), (1, 14), (2, 23))],
        [make_model("MiniGridEmptyContinuous", seed=s, size=sz, p_rand=0.1, p_lazy=0.05) for s, sz in ((0, 4), (1, 7), (2, 9))],
        [make_model("FrozenLakeContinuous", seed=s, size=sz, p_frozen=0.9, p_rand=0.1) for s, sz in ((0, 6), (1, 17), (2, 30))],
        [make_model("MiniGridRoomsContinuous", seed=s, room_size=3, n_rooms=4, p_rand=0.3, p_lazy=0.1) for s in (0, 1)],
        # <= 448 states: what K2W takes (5, 6 and 7 states per lane; A = 4, 3, 2)
        [make_model("FrozenLakeContinuous", seed=s, size=sz, p_frozen=0.9, p_rand=0.1) for s, sz in ((3, 5), (4, 18), (5, 16))],
        [make_model("FrozenLakeContinuous", seed=s, size=sz, p_frozen=0.9, p_rand=0.1) for s, sz in ((6, 20), (7, 12))],
        [make_model("FrozenLakeContinuous", seed=s, size=sz, p_frozen=0.95, p_rand=0.1) for s, sz in ((8, 21), (9, 20), (10, 3))],
        [make_model("MiniGridEmptyContinuous", seed=s, size=sz, p_rand=0.1) for s, sz in ((3, 10), (4, 5))],
        [make_model("DeepSeaContinuous", seed=s, size=sz, p_rand=0.2) for s, sz in ((3, 28), (4, 11))],
    ]
    n_k2w = 0
    for models in batches:
        A = models[0].n_actions
        dp = BatchedMDP(models, with_env=False)
        outs = {}
        n_distinct = 0
        for which in (L.DP_WORKGROUP, L.DP_REGISTER, L.DP_REGISTER_DISTINCT, L.DP_REGISTER_WAVEFRONT):
            dp.set_dp_kernel(which)
            pis = [np.random.RandomState(5 + i).dirichlet(np.ones(A), m.n_states).astype(np.float32) for i, m in enumerate(models)]
            try:
                vi = dp.value_iteration(0.99, 1e-5, L.SCHEME_JACOBI)
            except L.CmdpError as e:  # K2U exists for <= 8 distinct successors per state; it must say so otherwise
                assert which in (L.DP_REGISTER_DISTINCT, L.DP_REGISTER_WAVEFRONT) and e.code == L.ERR_UNSUPPORTED
                continue
            try:
                pe = dp.policy_evaluation(pis, 0.95, 1e-6, L.SCHEME_JACOBI)
            except L.CmdpError as e:  # K2W under policy evaluation: four actions fit its registers at five states per lane only
                assert which == L.DP_REGISTER_WAVEFRONT and A == 4 and e.code == L.ERR_UNSUPPORTED
                pe = None
            outs[which] = (vi, pe)
            n_distinct += which == L.DP_REGISTER_DISTINCT
            n_k2w += which == L.DP_REGISTER_WAVEFRONT
        for which in outs:
            for x, y in zip(outs[L.DP_WORKGROUP], outs[which]):
                if y is None:
                    continue
                for u, v in zip(x, y):
                    np.testing.assert_array_equal(u, v)
        n_k2u = locals().get("n_k2u", 0) + n_distinct
        (Q, V, sw), (Qp, Vp, swp) = outs[L.DP_REGISTER]
        for i, m in enumerate(models):
            oQ, oV, oit, _ = O.vi_discounted(m.n_states, A, m.csr(), m.reward_matrix(), 0.99, 1e-5, 1)
            np.testing.assert_array_equal(dp.split_states(V)[i], oV)
            np.testing.assert_array_equal(dp.split_rows(Q)[i].reshape(-1, A), oQ)
            assert sw[i] == oit
            oQ, oV, oit, _ = O.pe_discounted(m.n_states, A, m.csr(), m.reward_matrix(), pis[i], 0.95, 1e-6, 1)
            np.testing.assert_array_equal(dp.split_states(Vp)[i], oV)
            assert swp[i] == oit
        dp.close()
    assert n_k2u >= 2  # the distinct-successor kernel really ran for some of the batches
    assert n_k2w >= 4  # and so did the one-wavefront kernel (5, 6 and 7 states per lane)


def test_episodic_dp_vs_reference(need_gpu):
    for name in ("G1_deepsea8", "G3_stochastic", "G12_families"):
        z, cases = load_golden(name)
        for i, c in enumerate(cases):
            k = f"c{i}_"
            if k + "V_opt" not in z:
                continue
            m = make_model(c["cls"], **c["kwargs"])
            S, A, H = m.n_states, m.n_actions, m.H
            dp = BatchedMDP([m, m], with_env=False)
            Q, V = dp.episodic_value_iteration()
            Qw, Vw = dp.episodic_value_iteration(R=[-m.reward_matrix()] * 2)
            pi = np.ones((H, S, A), np.float32) / A
            Qr, Vr = dp.episodic_policy_evaluation([pi, pi])
            for b in range(2):
                np.testing.assert_allclose(dp.split_states(V, H + 1)[b].reshape(H + 1, S), z[k + "V_opt"], **VTOL)
                np.testing.assert_allclose(dp.split_states(Vr, H + 1)[b].reshape(H + 1, S), z[k + "V_rand"], **VTOL)
                if k + "Q_opt" not in z:  # G12 keeps the value functions only
                    continue
                np.testing.assert_allclose(dp.split_rows(Q, H + 1)[b].reshape(H + 1, S, A), z[k + "Q_opt"], **VTOL)
                np.testing.assert_allclose(dp.split_rows(Qw, H + 1)[b].reshape(H + 1, S, A), z[k + "Q_worst"], **VTOL)
                np.testing.assert_allclose(dp.split_rows(Qr, H + 1)[b].reshape(H + 1, S, A), z[k + "Q_rand"], **VTOL)
            oQ, oV = O.episodic(S, A, H, m.csr(), m.reward_matrix())
            np.testing.assert_array_equal(dp.split_rows(Q, H + 1)[0].reshape(H + 1, S, A), oQ)
            oQr, oVr = O.episodic(S, A, H, m.csr(), m.reward_matrix(), pi)
            np.testing.assert_array_equal(dp.split_states(Vr, H + 1)[1].reshape(H + 1, S), oVr)
            dp.close()


def test_drop_in_dp_functions(need_gpu):
    """The reference's free-function signatures on dense T, R."""
    from colosseum_amd import dynamic_programming as dpf

    z, cases = load_golden("G4_frozenlake20_vi")
    m = make_model(cases[0]["cls"], **cases[0]["kwargs"])
    T, R = m.dense()
    Q, V = dpf.discounted_value_iteration(T, R, 0.99, 1e-6)
    np.testing.assert_array_equal(V, z["c0_disp_e6_V"])
    assert dpf.discounted_value_iteration(T, R, 0.99, 1e-6, max_abs_value=0.5) is None
    with pytest.raises(dpf.DynamicProgrammingMaxIterationExceeded):
        from colosseum_amd.dp_handle import DPBatch, csr_from_dense

        with DPBatch([(m.n_states, 4, csr_from_dense(T), R)]) as h:
            h.value_iteration(0.99, 1e-9, L.SCHEME_JACOBI, 5)
    z1, c1 = load_golden("G1_deepsea8")
    m = make_model(c1[0]["cls"], **c1[0]["kwargs"])
    T, R = m.dense()
    Q, V = dpf.episodic_value_iteration(m.H, T, R)
    np.testing.assert_array_equal(Q, z1["c0_Q_opt"])
    pol = dpf.get_policy_from_q_values(Q[: m.H], True)
    Qp, Vp = dpf.episodic_policy_evaluation(m.H, T, R, pol)
    np.testing.assert_allclose(Vp[0, m.start_states[0]], V[0, m.start_states[0]], **VTOL)


def test_diameter_and_value_norm(need_gpu):
    import json
    import os

    from conftest import GOLDEN

    rows = json.load(open(os.path.join(GOLDEN, "G6_hardness_ref.json")))
    for row in rows:
        if "Episodic" in row["cls"]:
            continue
        m = make_model(row["cls"], **row["kwargs"])
        dp = BatchedMDP([m], with_env=False)
        diam, per = dp.diameter()
        od, oper = O.diameter_continuous(m.n_states, m.n_actions, m.csr())
        np.testing.assert_array_equal(per, oper)
        assert diam[0] == od
        # G-S path, eps = 1e-3: the reference's BLAS summation order can move the stopping sweep by one, i.e.
        # the hitting times by up to ~eps -> absolute tolerance 2*eps; GPU == oracle exactly (above)
        assert diam[0] == pytest.approx(row["diameter"], abs=2e-3), row
        Q, V, _ = dp.value_iteration(0.99, 1e-3)
        vn = dp.value_norm(V)
        assert vn[0] == pytest.approx(row["value_norm"], rel=5e-6, abs=1e-6), row
        assert vn[0] == O.value_norm(m.n_states, m.n_actions, m.csr(), V)
        dp.close()


def test_episodic_diameter(need_gpu):
    """Episodic diameter (time-augmented state space): GPU (every target to diff < eps) vs the oracle's two
    variants (the reference's single-thread order with the running-max early exit, and pure convergence), vs the
    values the reference recomputed here (G6) and the reference's cached values (G5)."""
    import json
    import os

    from conftest import GOLDEN

    rows = [r for r in json.load(open(os.path.join(GOLDEN, "G6_hardness_ref.json"))) if "Episodic" in r["cls"]]
    kat = [r for r in json.load(open(os.path.join(GOLDEN, "G5_hardness_kat.json")))
           if "Episodic" in r["cls"] and r["measure"] == "diameter"]
    seen = set()
    for r in kat:
        key = (r["cls"], json.dumps({k: v for k, v in r["kwargs"].items() if k != "seed"}, sort_keys=True))
        if key not in seen:
            seen.add(key)
            rows.append(dict(cls=r["cls"], kwargs=r["kwargs"], diameter=r["value"], cached=True))
    checked = n_cached = n_tight = 0
    for r in rows:
        m = make_model(r["cls"], **r["kwargs"])
        if m.n_states * m.H > 6000:
            continue
        dp = BatchedMDP([m, m], with_env=False)
        diam, per = dp.diameter_episodic()
        od, oper = O.diameter_episodic(m, use_running_max=False)
        np.testing.assert_array_equal(dp.split_states(per)[0], oper)  # GPU == oracle, target by target
        np.testing.assert_array_equal(dp.split_states(per)[1], oper)
        assert diam[0] == np.float32(od) and diam[1] == diam[0]
        od_ref, _ = O.diameter_episodic(m, use_running_max=True)
        assert abs(od_ref - od) <= 0.01 + 1e-6  # the early exit stops at diff < 0.01
        if r.get("cached"):
            # the authors' files: per-target convergence or the order-dependent early exit, several reference versions
            # (tests/test_gpu_kat_all.py states the two tolerance tiers and runs EVERY cached row)
            assert diam[0] == pytest.approx(r["diameter"], rel=5e-5, abs=5e-2), r
            n_cached += 1
            n_tight += diam[0] == pytest.approx(r["diameter"], rel=5e-6, abs=1e-3)
        else:
            assert diam[0] == pytest.approx(r["diameter"], rel=5e-6, abs=1e-5), r
        checked += 1
        dp.close()
    assert checked >= 12 and n_tight >= 0.9 * n_cached


def test_edge_cases(need_gpu):
    """Zero-length rollouts, a single instance, B not a multiple of anything, many start states, a large sparse
    instance that only the HBM-table kernel can take, masks, repeated resets, bad arguments."""
    m = make_model("DeepSeaEpisodic", seed=0, size=4)
    env = BatchedMDP([m], rng_mode=L.RNG_PHILOX)
    with pytest.raises(AssertionError):
        env.rollout(10)  # reset pending
    o0 = env.reset()
    out = env.rollout(0)
    assert out["last_obs"][0] == o0[0] and out["reward_sum"][0] == 0.0
    vs, vsa = env.visits()
    assert vs.sum() == 1 and vsa.sum() == 0
    env.reset()  # a second reset() visits the start state again (BaseMDP.reset, mdp/base.py:1275-1276)
    assert env.visits()[0][m.start_states[0]] == 2
    cur, h, nr = env.state()
    assert cur[0] == m.start_states[0] and h[0] == 0 and not nr[0]
    env.reset_visits()
    assert env.visits()[0].sum() == 0
    env.close()

    # masked reset: only instance 1 is reset
    ms = [make_model("DeepSeaEpisodic", seed=s, size=4) for s in range(3)]
    env = BatchedMDP(ms, rng_mode=L.RNG_PHILOX, with_dp=False)
    env.reset()
    env.rollout(2)
    env.reset(mask=np.array([0, 1, 0], np.uint8))
    cur, h, nr = env.state()
    assert h.tolist() == [2, 0, 2]
    env.close()

    # 12 start states, stochastic start sampler + stochastic rows, MT_COMPAT vs the oracle over several episodes
    m = make_model("MiniGridEmptyEpisodic", seed=3, size=5, n_starting_states=4, p_rand=0.3)
    env = BatchedMDP([m], rng_mode=L.RNG_MT_COMPAT, with_dp=False)
    e = O.OracleEnv(m, rng_mode=0)
    acts = np.random.RandomState(0).randint(0, 3, 5000).astype(np.int8)
    assert env.reset()[0] == e.reset()
    got = env.rollout(5000, acts[:, None], trace=True)
    ref = e.rollout(5000, acts)
    np.testing.assert_array_equal(got["obs"][:, 0], ref["obs"])
    np.testing.assert_array_equal(env.visits()[0], e.visits()[0])
    env.close()

    # |S| = 11 532: too large for any LDS-resident path; HBM-table rollout + oracle, and DP must refuse loudly or work
    big = make_model("MiniGridRoomsContinuous", seed=0, room_size=13, n_rooms=16, p_lazy=0.1, n_starting_states=2)
    assert big.n_states > 10_000
    env = BatchedMDP([big], rng_mode=L.RNG_PHILOX, philox_keys=[5])
    env.reset()
    got = env.rollout(3000, None, trace=True)
    e = O.OracleEnv(big, rng_mode=1, philox_key=5)
    e.reset()
    ref = e.rollout(3000)
    np.testing.assert_array_equal(got["obs"][:, 0], ref["obs"])
    Q, V, sw = env.value_iteration(0.9, 1e-4, L.SCHEME_JACOBI)  # V ping-pong of 92 KB still fits LDS
    oQ, oV, oit, _ = O.vi_discounted(big.n_states, 3, big.csr(), big.reward_matrix(), 0.9, 1e-4, 1)
    np.testing.assert_array_equal(V, oV)
    assert sw[0] == oit
    env.close()

    with pytest.raises(ValueError):
        BatchedMDP([make_model("DeepSeaEpisodic", seed=0, size=4), make_model("DeepSeaEpisodic", seed=0, size=5)])
    with pytest.raises(L.CmdpError):  # stochastic reward tables are rejected, not silently replaced by their means
        BatchedMDP([make_model("DeepSeaEpisodic", seed=0, size=4, make_reward_stochastic=True)])


def test_dense_row_layout_vs_oracle(need_gpu):
    """CMDP_LAYOUT_DENSE (float32 P[s,a,:] rows in HBM, wavefront prefix-sum CDF lookup): states, visit counts and
    reward sums bit-equal to the oracle's sequential scan of the same rows; deterministic rows give the same
    trajectories as the CSR layout."""
    cases = [
        [make_model("DeepSeaEpisodic", seed=s, size=9) for s in range(5)],
        [make_model("FrozenLakeContinuous", seed=s, size=sz, p_frozen=0.9, p_rand=0.15, p_lazy=0.05) for s, sz in ((0, 5), (1, 9), (2, 17))],
        [make_model("MiniGridEmptyEpisodic", seed=2, size=7, p_rand=0.3, n_starting_states=3)] * 2,
        [make_model("MiniGridRoomsContinuous", seed=1, room_size=4, n_rooms=4, p_lazy=0.2, p_rand=0.1, n_starting_states=2)],
    ]
    for models in cases:
        keys = np.arange(40, 40 + len(models), dtype=np.uint64)
        env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=keys, layout=L.LAYOUT_DENSE)
        env.reset()
        a = env.rollout(1500)
        acts = np.random.RandomState(3).randint(0, models[0].n_actions, (700, len(models))).astype(np.int8)
        b = env.rollout(700, acts)
        vs, vsa = env.visits()
        for i, m in enumerate(models):
            e = O.OracleEnv(m, rng_mode=1, philox_key=int(keys[i]), dense=True)
            e.reset()
            ra = e.rollout(1500, trace=False)
            rb = e.rollout(700, acts[:, i], trace=False)
            assert a["last_obs"][i] == ra["last_obs"] and b["last_obs"][i] == rb["last_obs"], (m.extra["cls_name"], i)
            assert a["reward_sum"][i] == ra["reward_sum"] and b["reward_sum"][i] == rb["reward_sum"]
            ovs, ovsa = e.visits()
            np.testing.assert_array_equal(env.split_states(vs)[i], ovs)
            np.testing.assert_array_equal(env.split_rows(vsa)[i].reshape(-1, m.n_actions), ovsa)
        env.close()
    # deterministic dynamics: dense == CSR layout
    models = cases[0]
    outs = []
    for layout in (L.LAYOUT_CSR, L.LAYOUT_DENSE):
        env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, layout=layout)
        env.reset()
        r = env.rollout(999)
        outs.append((r["last_obs"], r["reward_sum"], env.visits()[1]))
        env.close()
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)
    with pytest.raises(L.CmdpError):
        BatchedMDP(models, rng_mode=L.RNG_MT_COMPAT, layout=L.LAYOUT_DENSE)


def test_suboptimality_gaps_vs_reference(need_gpu):
    import json
    import os

    from conftest import GOLDEN
    from colosseum_amd import hardness

    rows = json.load(open(os.path.join(GOLDEN, "G6_hardness_ref.json")))
    models = [make_model(r["cls"], **r["kwargs"]) for r in rows]
    got = hardness.sum_reciprocals_suboptimality_gaps(models)
    for r, g in zip(rows, got):
        # every term 1/(gap + 0.1) amplifies a value difference by up to 1/0.1^2 = 100: values within 1e-6 (the
        # Gauss-Seidel path is not bit-reproducible against BLAS) => the sum within ~1e-5 relative
        assert g == pytest.approx(r["suboptimal_gaps"], rel=2e-5), r


def test_diameter_lanes_kernel_equals_workgroup_kernel_and_oracle(need_gpu):
    """K5S (64 targets per workgroup, value vectors in HBM -- what instances too large for LDS get, config C5) forced
    on small instances: hitting times bit-equal to the LDS-resident Jacobi kernel and to the oracle; target ranges
    (the multi-GPU split) reassemble to the full vector."""
    ms = [make_model("FrozenLakeContinuous", seed=1, size=9, p_frozen=0.8),
          make_model("MiniGridRoomsContinuous", seed=2, room_size=4, n_rooms=4, p_lazy=0.1),
          make_model("MiniGridRoomsContinuous", seed=5, room_size=6, n_rooms=9, p_lazy=0.05, p_rand=0.1),  # 1 400 states
          make_model("DeepSeaContinuous", seed=3, size=11, p_rand=0.2)]
    ms = [m for m in ms if m.n_actions == ms[0].n_actions] + [m for m in ms if m.n_actions != ms[0].n_actions]
    by_A = {}
    for m in ms:
        by_A.setdefault(m.n_actions, []).append(m)
    for A, group in by_A.items():
        dp = BatchedMDP(group, with_env=False)
        diam0, per0 = dp.diameter(1e-3, L.SCHEME_JACOBI)
        dp.set_option(L.OPT_DP_KERNEL, 3)
        dp.set_option(L.OPT_DIAMETER_WORKSPACE_MB, 1)  # several launches
        diam1, per1 = dp.diameter(1e-3, L.SCHEME_JACOBI)
        np.testing.assert_array_equal(per1, per0)
        np.testing.assert_array_equal(diam1, diam0)
        dp.set_option(L.OPT_DIAMETER_RELABEL_MIN_STATES, 1)  # rows stored in the locality order of the states (C5's default)
        # ... which is also where K5C takes over (clusters of workgroups per target group, one barrier per sweep); then K5S
        # alone (CMDP_K5C=0), then K5C with a barrier time limit of one tick: every cluster gives up and K5S repeats the solve
        import ctypes
        import os

        def stat(which):
            v = ctypes.c_double()
            L.check(L.load().cmdp_stat(dp.handle, which, ctypes.byref(v)))
            return int(v.value)

        # (a give-up is remembered: the call after it does not try the persistent launch again -- back-off of 8 calls --, so the
        # two calls of the last leg count ONE fallback)
        for env, launches, fallbacks in (({}, 2, 0), ({"CMDP_K5C": "0"}, 2, 0), ({"CMDP_K5C_TIMEOUT_TICKS": "1"}, 2, 1)):
            os.environ.update(env)
            try:
                diam2, per2 = dp.diameter(1e-3, L.SCHEME_JACOBI)
                np.testing.assert_array_equal(per2, per0)
                np.testing.assert_array_equal(diam2, diam0)
                np.testing.assert_array_equal(dp.diameter_range(3, len(per0) - 2), per0[3:-2])  # a target range (the multi-GPU split)
            finally:
                for k in env:
                    os.environ.pop(k)
            assert (stat(L.STAT_DIAMETER_CLUSTER_LAUNCHES), stat(L.STAT_DIAMETER_CLUSTER_FALLBACKS)) == (launches, fallbacks), env
        dp.set_option(L.OPT_DIAMETER_RELABEL_MIN_STATES, 1 << 40)
        dp.set_option(L.OPT_DP_KERNEL, 4)  # generic CSR walker instead of the fixed-width-row variant
        np.testing.assert_array_equal(dp.diameter(1e-3, L.SCHEME_JACOBI)[1], per0)
        dp.set_option(L.OPT_DP_KERNEL, 6)  # K5T: value rows of a cluster of states gathered into an LDS tile first (C5's kernel)
        diam6, per6 = dp.diameter(1e-3, L.SCHEME_JACOBI)
        np.testing.assert_array_equal(per6, per0)
        np.testing.assert_array_equal(diam6, diam0)
        dp.set_option(L.OPT_DP_KERNEL, 3)
        off = 0
        for m in group:
            _, oper = O.diameter_continuous(m.n_states, m.n_actions, m.csr(), scheme=1)
            np.testing.assert_array_equal(per1[off:off + m.n_states], oper)
            off += m.n_states
        n = int(dp.state_off[-1])
        cuts = sorted({0, min(5, n), min(64, n), min(70, n), n // 2, n})
        parts = [dp.diameter_range(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
        np.testing.assert_array_equal(np.concatenate(parts), per0)
        dp.close()


def test_lds_resident_stochastic_rollout_equals_hbm_kernel_and_oracle(need_gpu):
    """K1S (sampler tables compressed into patterns / successor sets / 4-bit codes, resident in LDS) on batches with
    stochastic dynamics: final states, float64 reward sums, state and state-action visit counts, in-episode times and
    the Philox counters bit-equal to the lane-per-instance kernel K1 and to the CPU oracle, over several launches of odd
    lengths, multiple start states, episodic and continuous."""
    cases = [
        ("FrozenLakeContinuous", dict(size=8, p_frozen=0.9, p_rand=0.1), 9),
        ("FrozenLakeEpisodic", dict(size=5, p_frozen=0.9, p_rand=0.2, p_lazy=0.1), 20),
        ("MiniGridEmptyEpisodic", dict(size=6, p_rand=0.1, n_starting_states=3), 12),
        ("MiniGridEmptyContinuous", dict(size=8, p_rand=0.05, p_lazy=0.05), 70),   # more instances than fit one workgroup
        ("DeepSeaEpisodic", dict(size=9, p_rand=0.3), 7),                          # rewards depend on the row
        ("MiniGridRoomsContinuous", dict(room_size=3, n_rooms=4, p_lazy=0.1, n_starting_states=2), 5),
    ]
    ran = 0
    for cls, kw, n in cases:
        ms = [make_model(cls, seed=s, **kw) for s in range(n)]
        ms = [m for m in ms if m.n_states == ms[0].n_states and m.H == ms[0].H]
        keys = np.arange(1000, 1000 + len(ms), dtype=np.uint64)
        outs = []
        for kernel in (L.ROLLOUT_LDS_STOCHASTIC, L.ROLLOUT_GLOBAL):
            env = BatchedMDP(ms, rng_mode=L.RNG_PHILOX, philox_keys=keys, with_dp=False)
            if kernel == L.ROLLOUT_LDS_STOCHASTIC:
                assert env.lds_plan()["kernel"] == "k_rollout_stoch", (cls, env.lds_plan())
            env.set_rollout_kernel(kernel)
            env.reset()
            rs = []
            for steps in (1, 63, 700, 9001):   # 9001: several flushes of the 8-bit counters
                r = env.rollout(steps)
                rs.append((r["last_obs"].copy(), r["reward_sum"].copy()))
            vs, vsa = env.visits()
            cur, h, _ = env.state()
            last = env.last_start()
            outs.append((rs, vs, vsa, cur, h, last, env.previous_start))
            env.close()
        (rs1, vs1, vsa1, cur1, h1, l1, p1), (rs0, vs0, vsa0, cur0, h0, l0, p0) = outs
        for (a, b), (c, d) in zip(rs1, rs0):
            np.testing.assert_array_equal(a, c, err_msg=cls)
            np.testing.assert_array_equal(b, d, err_msg=cls)
        for x, y in ((vs1, vs0), (vsa1, vsa0), (cur1, cur0), (h1, h0), (l1, l0), (p1, p0)):
            np.testing.assert_array_equal(x, y, err_msg=cls)
        # and the oracle, instance 0 and the last one
        for i in (0, len(ms) - 1):
            e = O.OracleEnv(ms[i], rng_mode=1, philox_key=int(keys[i]))
            e.reset()
            for steps in (1, 63, 700, 9001):
                e.rollout(steps, trace=False)
            off = int(sum(m.n_states for m in ms[:i]))
            np.testing.assert_array_equal(vs1[off:off + ms[i].n_states], e.visits()[0])
        ran += 1
    assert ran == len(cases)


def test_sparse_float64_diameter_equals_reference(need_gpu):
    """K5D + the host replay of the reference's sequential loop (`cmdp_diameter_sparse_f64`) against the reference's own
    `_get_sparse_diameter` (golden G16) and, on further MDPs incl. a mixed batch, the numpy restatement: float64
    diameters and the running maximum after every target, bit for bit."""
    import json
    import os

    from conftest import GOLDEN
    from colosseum_amd import hardness

    rows = json.load(open(os.path.join(GOLDEN, "G16_sparse_diameter.json")))
    for r in rows:
        m = make_model(r["cls"], **r["kwargs"])
        dp = BatchedMDP([m], with_env=False)
        d, run = dp.diameter_sparse_f64()
        assert d[0] == r["diameter"], (r["cls"], d[0], r["diameter"])
        assert run.tolist() == r["running_max"]
        dp.close()
    ms = [make_model("MiniGridEmptyContinuous", seed=s, size=4 + s, p_rand=0.1) for s in range(3)]  # 64, 100, 144 states
    dp = BatchedMDP(ms, with_env=False)
    dp.set_option(L.OPT_DIAMETER_WORKSPACE_MB, 1)  # several launches
    d, run = dp.diameter_sparse_f64()
    off = 0
    for i, m in enumerate(ms):
        od, orun = O.sparse_diameter_f64(m.n_states, m.n_actions, m.csr())
        assert d[i] == od and run[off:off + m.n_states].tolist() == orun
        off += m.n_states
    dp.close()
    # the dispatch of a single-core reference: above 1000 states the sparse float64 path, below it the per-target one
    big = make_model("MiniGridEmptyContinuous", seed=0, size=16, p_rand=0.1)  # 1024 states
    assert big.n_states > 1000
    got = hardness.diameter([ms[0], big], variant="reference_single_core")
    assert got[0] == hardness.diameter([ms[0]])[0]
    per_target = hardness.diameter([big])[0]
    assert got[1] != per_target and got[1] == pytest.approx(per_target, abs=0.06)  # float64 + early exit vs float32 to eps


def test_greedy_q_policy_rollout(need_gpu):
    """CMDP_POLICY_GREEDY_Q: the device picks the first maximiser of the current Q row.  Feeding the actions it must
    have taken (recomputed on the host from the traced observations) through CMDP_POLICY_HOST_ACTIONS on a fresh handle
    with the same streams reproduces observations, rewards and step types."""
    rng = np.random.default_rng(3)
    for cls, kw in (("FrozenLakeContinuous", dict(seed=3, size=6, p_frozen=0.9, p_rand=0.1)),
                    ("MiniGridEmptyEpisodic", dict(seed=1, size=5, p_rand=0.2, n_starting_states=1)),
                    ("DeepSeaEpisodic", dict(seed=2, size=7))):
        ms = [make_model(cls, **kw)] * 3
        m = ms[0]
        assert len(m.start_states) == 1
        S, A, H = m.n_states, m.n_actions, m.H
        qs = [np.round(rng.random((max(H, 1), S, A)), 1).astype(np.float32) for _ in ms]   # rounding makes ties
        n = 500
        env = BatchedMDP(ms, rng_mode=L.RNG_MT_COMPAT, with_dp=False)
        first = env.reset()
        out = env.rollout(n, greedy_q=[q if H else q[0] for q in qs], trace=True)
        env.close()
        acts = np.zeros((n, len(ms)), np.int8)
        for b in range(len(ms)):
            cur, h = int(first[b]), 0
            for t in range(n):
                acts[t, b] = int(np.argmax(qs[b][h if H else 0, cur]))     # np.argmax = first maximiser
                if out["stype"][t, b] == 2:       # termination: the device reset to the (single) start state
                    cur, h = int(m.start_states[0]), 0
                else:
                    cur, h = int(out["obs"][t, b]), h + 1
        assert len(np.unique(acts)) > 1
        env = BatchedMDP(ms, rng_mode=L.RNG_MT_COMPAT, with_dp=False)
        env.reset()
        ref = env.rollout(n, acts, trace=True)
        env.close()
        np.testing.assert_array_equal(out["obs"], ref["obs"], err_msg=cls)
        np.testing.assert_array_equal(out["rew"], ref["rew"])
        np.testing.assert_array_equal(out["stype"], ref["stype"])


def test_custom_mdp_trajectories_on_device(need_gpu):
    """CustomMDP (golden G13): the device's MT19937 streams reproduce the reference's 4 000-step trajectories."""
    z, cases = load_golden("G13_custom")
    for i, c in enumerate(cases):
        k = f"c{i}_"
        T0 = {int(a): float(b) for a, b in zip(z[k + "in_T0k"], z[k + "in_T0v"])}
        m = make_model(c["cls"], T_0=T0, T=z[k + "in_T"], R=z[k + "in_R"], **c["kwargs"])
        env = BatchedMDP([m], rng_mode=L.RNG_MT_COMPAT, with_dp=False)
        first = env.reset()
        acts = z[k + "actions"][:, None]
        out = env.rollout(len(acts), acts, trace=True)
        vs, vsa = env.visits()
        assert first[0] == z[k + "resets"][0]
        np.testing.assert_array_equal(out["obs"][:, 0], z[k + "obs"])
        np.testing.assert_array_equal(out["rew"][:, 0], z[k + "rew"])
        np.testing.assert_array_equal(out["stype"][:, 0], z[k + "stype"])
        np.testing.assert_array_equal(vs, z[k + "visits_s"])
        np.testing.assert_array_equal(vsa.reshape(-1, env.A), z[k + "visits_sa"])
        env.close()


def test_value_iteration_into_pinned_buffers(need_gpu):
    """`out=` with page-locked result buffers (BatchedMDP.dp_buffers): same bits as the freshly allocated arrays, and the
    buffers are reusable."""
    models = [make_model("FrozenLakeContinuous", seed=s, size=8, p_frozen=0.9, p_rand=0.1) for s in range(5)]
    dp = BatchedMDP(models, with_env=False)
    Q0, V0, sw0 = dp.value_iteration(0.95, 1e-5)
    bufs = dp.dp_buffers()
    for _ in range(2):
        Q, V, sw = dp.value_iteration(0.95, 1e-5, out=bufs)
        assert Q is bufs[0] and V is bufs[1] and sw is bufs[2]
        np.testing.assert_array_equal(Q, Q0)
        np.testing.assert_array_equal(V, V0)
        np.testing.assert_array_equal(sw, sw0)
        Q[:] = -1.0
    dp.close()


def test_dp_results_stored_straight_into_page_locked_buffers(need_gpu):
    """`BatchedMDP.dp_buffers()` hands out page-locked arrays; the register-resident sweep kernels (K2W / K2U / K2R) then store
    Q, V and the sweep counts into them directly (no copy after the kernel).  Same numbers as through pageable arrays, for
    value iteration and policy evaluation, on batches that take each of the three kernels; the LDS / Gauss-Seidel kernels keep
    the copy."""
    cases = [[make_model("FrozenLakeContinuous", seed=s, size=20, p_frozen=0.9, p_rand=0.1) for s in range(6)],   # K2W (400 states)
             [make_model("FrozenLakeContinuous", seed=s, size=12, p_frozen=0.85, p_lazy=0.1) for s in range(5)],  # K2U
             [make_model("DeepSeaContinuous", seed=s, size=14, p_rand=0.2) for s in range(4)],
             [make_model("MiniGridEmptyContinuous", seed=s, size=6, p_rand=0.1) for s in range(3)]]
    kernels = set()
    for ms in cases:
        dp = BatchedMDP(ms, with_env=False)
        for scheme in (L.SCHEME_JACOBI, L.SCHEME_GAUSS_SEIDEL):
            Q0, V0, s0 = dp.value_iteration(0.99, 1e-6, scheme=scheme)
            bufs = dp.dp_buffers()
            for b in bufs:
                b[...] = 0
            Q1, V1, s1 = dp.value_iteration(0.99, 1e-6, scheme=scheme, out=bufs)
            np.testing.assert_array_equal(Q1, Q0)
            np.testing.assert_array_equal(V1, V0)
            np.testing.assert_array_equal(s1, s0)
            if scheme == L.SCHEME_JACOBI:
                import ctypes

                v = ctypes.c_double()
                L.check(L.load().cmdp_stat(dp.handle, L.STAT_DP_KERNEL, ctypes.byref(v)))
                kernels.add(int(v.value))
            pi = np.concatenate([np.full((m.n_states, m.n_actions), 1.0 / m.n_actions, np.float32).ravel() for m in ms])
            P0 = dp.policy_evaluation(pi, 0.99, 1e-6, scheme=scheme)
            for b in bufs:
                b[...] = 0
            P1 = dp.policy_evaluation(pi, 0.99, 1e-6, scheme=scheme, out=bufs)
            for a, b in zip(P0, P1):
                np.testing.assert_array_equal(b, a)
        dp.close()
    assert 7 in kernels and (5 in kernels or 2 in kernels), kernels
