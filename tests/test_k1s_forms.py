"""Every compiled form of the stochastic-dynamics rollout K1S (k_rollout_stoch) on generated batches: bit for bit against
the lane-per-instance kernel K1 and against the CPU oracle, every instance.

plan_k1s chooses among 1 / 2 / 4 walker wavefronts, teams of 16 / 8 / 1 lanes, three sources of the reward code, one or
two shape bytes per row and nine specialised walk loops plus a generic one.  CMDP_K1S_G sets the instances per workgroup
so that small batches reach all of them, and every case first asserts, through the plan query (cmdp_k1s_plan, whose
`form` is computed by the function the kernel's dispatch branches on), that it landed in the form it names.  The same
assertions and the planner's refusal edges run without a GPU through cmdp_k1s_plan_desc at 256 compute units.
helpers_k1s has the generator."""
import functools
import os

import numpy as np
import pytest

import helpers_k1s as K
from colosseum_amd import _lib as L
from colosseum_amd.batched import BatchedMDP, k1s_plan_of_tables
from oracle import oracle as O

KNOBS = ("CMDP_K1L_PIPE", "CMDP_K1T_G", "CMDP_K1U_G", "CMDP_K1S_G", "CMDP_K1L_G", "CMDP_K1T_CH")   # the environment cmdp_create reads
CUS = 256   # the MI355X; the planned G of the knob-less batch holds for it only
GEOMETRY = {1: (1, 1, 16), 2: (2, 1, 16), 3: (2, 2, 16), 5: (4, 2, 16), 16: (4, 4, 16), 17: (4, 5, 8), 32: (4, 8, 8),
            33: (4, 9, 1), 64: (4, 16, 1)}   # G -> walker wavefronts, instances per walker, team
TEAM_G = {16: 3, 8: 20, 1: 40}   # an instances-per-workgroup value for each team size
SOURCE = {"packed": dict(reward_by="state", n_rew=5), "state_table": dict(reward_by="state", n_rew=17),
          "row": dict(reward_by="row", n_rew=5)}
SOURCE_PLAN = {"packed": dict(reward_mode=0, rc_packed=1), "state_table": dict(reward_mode=0, rc_packed=0),
               "row": dict(reward_mode=1, rc_packed=0)}


def _ragged_B(G):
    """2 G + r instances, 0 < r < G: a ragged last workgroup in which some walker wavefronts have no instance"""
    return 3 if G == 1 else 2 * G + max(1, G // 3)


def _cases():
    """name -> (generator arguments, CMDP_K1S_G or None, expected plan fields, extra launches)"""
    c = {}
    # the nine specialised forms: one pattern, one shape byte.  Horizons, start states, actions and the rewards range vary
    # along the way (A = 3 draws its actions from whole Philox words, A = 2 / 4 from packed bits).
    vary = {(16, "packed"): dict(H=0), (16, "state_table"): dict(H=5, n_start=3, rewards_range=(-2.5, 4.0)),
            (16, "row"): dict(H=33, A=3), (8, "packed"): dict(H=7, n_start=2, A=4), (8, "state_table"): dict(H=0, A=3),
            (8, "row"): dict(H=0, rewards_range=(0.3, 1.7)), (1, "packed"): dict(H=0, rewards_range=(-1.0, 2.0)),
            (1, "state_table"): dict(H=40), (1, "row"): dict(H=9, n_start=4)}
    for team, G in TEAM_G.items():
        for i, src in enumerate(SOURCE):
            gen = dict(seed=100 + team + i, B=_ragged_B(G), S=6, entries=(3, 3), succ=3, self_loop=0.2, **SOURCE[src], **vary[team, src])
            c[f"team{team}_{src}"] = (gen, G, dict(form=f"team{team}_{src}", team=team, n_pat=1, shape_bytes=1, U=3, **SOURCE_PLAN[src]), ())
    # the generic form at every team size and reward source: several patterns, rows of up to 16 entries, successor sets of
    # 16 (instances are copies of a few templates: few enough row shapes for one shape byte).  The limits of the format --
    # 64 patterns, 8 start states -- are among them.
    vary = {(16, "packed"): dict(n_pat=64, H=0), (16, "state_table"): dict(n_pat=3, H=6, n_start=8),
            (16, "row"): dict(n_pat=5, H=0, rewards_range=(-2.5, 4.0)), (8, "packed"): dict(n_pat=4, H=11, n_start=8),
            (8, "state_table"): dict(n_pat=64, H=0), (8, "row"): dict(n_pat=2, H=3, n_start=2),
            (1, "packed"): dict(n_pat=3, H=0, rewards_range=(0.3, 1.7)), (1, "state_table"): dict(n_pat=7, H=50),
            (1, "row"): dict(n_pat=64, H=13, n_start=8)}
    for team, G in TEAM_G.items():
        for i, src in enumerate(SOURCE):
            v = vary[team, src]
            gen = dict(seed=200 + team + i, B=_ragged_B(G), S=18, entries=(1, 16), succ=16, templates=3, **SOURCE[src], **v)
            c[f"generic_team{team}_{src}"] = (gen, G, dict(form="generic", team=team, n_pat=v["n_pat"], shape_bytes=1, U=16, **SOURCE_PLAN[src]), ())
    # two shape bytes: more than 256 row shapes in the batch, with one pattern and with several
    c["shape16_one_pattern"] = (dict(seed=301, B=40, S=8, entries=(8, 8), succ=6, n_rew=4, H=0), 20,
                                dict(form="generic", team=8, n_pat=1, shape_bytes=2), ())
    c["shape16_patterns"] = (dict(seed=302, B=40, S=8, entries=(3, 8), succ=6, n_pat=5, n_rew=20, H=10, n_start=2), 3,
                             dict(form="generic", team=16, n_pat=5, shape_bytes=2, rc_packed=0, reward_mode=0), ())
    # group geometry: walker wavefronts and instances per walker, ragged last workgroup
    for G, (nw, gw, team) in GEOMETRY.items():
        gen = dict(seed=400 + G, B=_ragged_B(G), S=4 + G % 3, A=2 + G % 2, entries=(2, 3), succ=3, n_rew=3, H=(0, 12)[G % 2], n_start=1 + G % 3)
        c[f"geometry_G{G}"] = (gen, G, dict(G=G, nw=nw, gw=gw, team=team), ())
    c["geometry_full_groups"] = (dict(seed=450, B=15, S=5, H=4, n_start=2), 5, dict(G=5, nw=4, gw=2, team=16), ())
    # no knob: the planner's own G > 1 (1 100 instances over 256 CUs) -- the knob path and the planned path are one code
    c["planned_G5"] = (dict(seed=460, B=1100, S=5, H=6, n_start=2), None, dict(G=5, nw=4, gw=2, team=16), ())
    # inputs that stress the format
    c["ragged_states"] = (dict(seed=501, B=13, S=[3 + (7 * i) % 9 for i in range(13)], succ=2, entries=(2, 3), n_pat=2, H=5), 5,
                          dict(G=5, form="generic"), ())
    c["ragged_states_row_rewards"] = (dict(seed=502, B=46, S=[4 + i % 5 for i in range(46)], reward_by="row", n_rew=4, H=0), 20,
                                      dict(G=20, form="team8_row"), ())
    c["starts8"] = (dict(seed=503, B=7, S=10, n_start=8, H=3), 3, dict(form="team16_packed"), ())
    c["horizon1"] = (dict(seed=504, B=7, S=6, n_start=3, H=1), 3, dict(form="team16_packed"), ())
    c["horizon2"] = (dict(seed=505, B=46, S=6, n_start=3, H=2), 20, dict(form="team8_packed"), ())
    c["horizon7"] = (dict(seed=506, B=90, S=6, n_start=2, H=7), 40, dict(form="team1_packed"), ())
    # 8-bit counter wraps: almost every transition arrives in state 0, so one row (A = 1) or two (A = 2) collect the whole
    # flush period of 7 680 transitions -- 30 wraps, the capacity of the overflow list -- in a launch of two periods
    c["absorbing_A2"] = (dict(seed=507, B=7, S=4, absorbing=True, H=0), 3, dict(form="team16_packed"), (2 * 7680 + 1,))
    c["absorbing_A1"] = (dict(seed=508, B=46, S=4, A=1, absorbing=True, H=0, reward_by="row", n_rew=3), 20, dict(form="team8_row"), (2 * 7680,))
    return c


CASES = _cases()

# one step past a limit of the format (generator arguments); the at-the-limit batches are in the matrix above
REFUSED = {
    "entries17": dict(seed=601, B=5, S=6, entries=(17, 17), succ=3),
    "successors17": dict(seed=602, B=5, S=19, entries=(9, 16), succ=17),
    "patterns65": dict(seed=603, B=5, S=8, entries=(2, 6), n_pat=65),
    "starts9": dict(seed=604, B=5, S=10, n_start=9, H=4),
    "reward_of_row_and_successor": dict(seed=605, B=5, S=6, reward_by="neither", n_rew=4),
    "rows65536": dict(seed=606, B=1, S=32768, A=2, entries=(2, 2), succ=2),
}
REFUSED_ROLLOUT = ("entries17", "reward_of_row_and_successor")   # ... whose automatic rollout is held against the oracle


@functools.lru_cache(maxsize=None)
def _tables(name):
    gen = CASES[name][0] if name in CASES else REFUSED[name]
    return K.tables(**gen)


@functools.lru_cache(maxsize=None)
def _oracle(name, n_steps):
    t = _tables(name)
    return O.batch_rollout(t, 0, int(t["B"]), n_steps, rng_mode=1, philox_keys=K.keys(int(t["B"])), want_visits=True)


def _launches(name):
    return K.LAUNCHES + tuple(CASES[name][3]) if name in CASES else K.LAUNCHES


def _check_plan(plan, want):
    assert plan["ok"], plan
    assert {k: plan[k] for k in want} == want, plan
    nw, gw, team = plan["nw"], plan["gw"], plan["team"]
    assert (nw, gw, team) == GEOMETRY.get(plan["G"], (nw, gw, team)) and nw * gw >= plan["G"] and gw * team <= 64 and plan["ch"] == 32


# ---- host only: the planner on the bare description ---------------------------------------------------------------------
def test_generator_covers_what_it_claims():
    """Totals other than 1, ties, the limits of the format and the sizes just past them are in the generated tables."""
    d = K.describe(_tables("generic_team16_packed"))
    assert d["entries"] == (1, 16) and d["max_succ"] == 16 and d["n_pat"] == 64 and d["n_rew"] == 5
    assert d["ties"] and len([x for x in d["totals"] if x != 1.0]) >= 2
    assert K.describe(_tables("generic_team16_state_table"))["max_starts"] == 8
    assert K.describe(_tables("team16_state_table"))["n_rew"] == 17
    assert K.describe(_tables("entries17"))["entries"] == (17, 17)
    assert K.describe(_tables("successors17"))["max_succ"] == 17
    assert K.describe(_tables("patterns65"))["n_pat"] == 65
    assert K.describe(_tables("starts9"))["max_starts"] == 9
    t = _tables("rows65536")
    assert int(t["state_off"][-1]) * int(t["A"]) == 65536
    for name in CASES:   # unequal start probabilities wherever there are several starts
        t = _tables(name)
        for b in np.flatnonzero(np.diff(t["start_off"]) > 1)[:3]:
            w = np.diff(np.concatenate([[0.0], t["start_cum"][t["start_off"][b]:t["start_off"][b + 1]]]))
            assert len(set(w.tolist())) == len(w)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_of_description(name):
    """The case lands in the form it names (cmdp_k1s_plan_desc: no handle, no device)."""
    gen, G, want, _ = CASES[name]
    plan = k1s_plan_of_tables(_tables(name), CUS, G or 0)
    _check_plan(plan, want)
    if G:
        assert plan["G"] == G
        assert k1s_plan_of_tables(_tables(name), CUS, 1000)["G"] == 64   # capped by the format (these slots are small)


def test_every_form_is_in_the_matrix():
    plans = {name: k1s_plan_of_tables(_tables(name), CUS, CASES[name][1] or 0) for name in CASES}
    assert {p["form"] for p in plans.values()} == set(L.K1S_FORMS.values()) and len(L.K1S_FORMS) == 10
    generic = {(p["team"], p["reward_mode"], p["rc_packed"]) for p in plans.values() if p["form"] == "generic" and p["shape_bytes"] == 1}
    assert generic >= {(t, m, r) for t in (16, 8, 1) for m, r in ((0, 1), (0, 0), (1, 0))}
    assert {p["n_pat"] == 1 for p in plans.values() if p["shape_bytes"] == 2} == {True, False}
    assert all(p["n_shapes"] > 256 for p in plans.values() if p["shape_bytes"] == 2)
    assert {p["nw"] for p in plans.values()} == {1, 2, 4} and max(p["gw"] for p in plans.values()) == 16


@pytest.mark.parametrize("name", list(REFUSED))
def test_planner_refuses_one_past_the_limit(name):
    plan = k1s_plan_of_tables(_tables(name), CUS, 0)
    assert not plan["ok"] and plan["form"] is None and plan["G"] == 0, plan


def test_plan_of_description_needs_philox_and_refused_deterministic_planners():
    t = _tables("team16_packed")
    assert k1s_plan_of_tables(t, CUS, 0)["ok"] and not k1s_plan_of_tables(t, CUS, 0, rng_mode=L.RNG_MT_COMPAT)["ok"]
    det = K.tables(seed=1, B=4, S=6, entries=(1, 1), succ=2)   # deterministic rows, one start: K1L / K1P take the batch
    assert not k1s_plan_of_tables(det, CUS, 0)["ok"]
    with pytest.raises(L.CmdpError) as e:
        k1s_plan_of_tables(dict(t, sp_next=t["sp_next"] + 6), CUS, 0)
    assert e.value.code == L.ERR_INVALID


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _create(tables, G):
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    if G:
        os.environ["CMDP_K1S_G"] = str(G)
    try:
        return BatchedMDP(tables=tables, rng_mode=L.RNG_PHILOX, philox_keys=K.keys(int(tables["B"])))
    finally:
        os.environ.pop("CMDP_K1S_G", None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def _run(tables, G, which, launches, want=None):
    """The launches back to back on one handle: per launch (last_obs, reward_sum), then visits, state and starts."""
    env = _create(tables, G)
    try:
        env.set_rollout_kernel(which)
        if want is not None:
            plan = env.k1s_plan()
            _check_plan(plan, want)
            assert plan == k1s_plan_of_tables(tables, CUS, G or 0)   # (a 256-CU device)
            assert env.lds_plan()["kernel"] == "k_rollout_stoch" and env.lds_plan()["instances_per_workgroup"] == plan["G"]
        env.reset()
        outs = [env.rollout(n) for n in launches]
        vs, vsa = env.visits()
        cur, h, need_reset = env.state()
        last_start = env.last_start()
        return dict(last=[o["last_obs"] for o in outs], rsum=[o["reward_sum"] for o in outs], vs=vs, vsa=vsa, cur=cur, h=h,
                    need_reset=need_reset, last_start=last_start, previous_start=env.previous_start)
    finally:
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_k1s_equals_k1_and_oracle(need_gpu, name):
    gen, G, want, _ = CASES[name]
    t, launches = _tables(name), _launches(name)
    total = int(sum(launches))
    s = _run(t, G, L.ROLLOUT_LDS_STOCHASTIC, launches, want)
    g = _run(t, G, L.ROLLOUT_GLOBAL, launches)
    for i in range(len(launches)):
        assert np.array_equal(s["last"][i], g["last"][i]), (name, launches[i])
        assert np.array_equal(s["rsum"][i], g["rsum"][i]), (name, launches[i])
    for k in ("vs", "vsa", "cur", "h", "need_reset", "last_start", "previous_start"):
        assert np.array_equal(s[k], g[k]), (name, k)
    last, rsum, vs, vsa = _oracle(name, total)   # every instance
    assert np.array_equal(s["last"][-1], last) and np.array_equal(s["cur"], last)
    assert np.array_equal(s["vs"], vs) and np.array_equal(s["vsa"], vsa)
    assert vs.sum() >= t["B"] * total and vsa.sum() == t["B"] * total
    np.testing.assert_allclose(np.sum(s["rsum"], axis=0), rsum, rtol=1e-12, atol=0)
    one = _run(t, G, L.ROLLOUT_LDS_STOCHASTIC, (total,))   # one launch from reset: the float64 sum in the oracle's order
    assert np.array_equal(one["rsum"][0], rsum) and np.array_equal(one["last"][0], last)
    assert np.array_equal(one["vs"], vs) and np.array_equal(one["vsa"], vsa)
    assert len(np.unique(rsum)) > 1 or t["B"] == 1


def test_absorbing_cases_fill_the_overflow_list():
    """The premise of the counter-wrap cases, from the oracle's visit counts: the rows of state 0 take (nearly) every
    transition, so a flush period of 7 680 transitions wraps the 8-bit counters of an instance 29 or 30 times."""
    for name in ("absorbing_A2", "absorbing_A1"):
        t = _tables(name)
        A, total = int(t["A"]), int(sum(_launches(name)))
        _, _, _, vsa = _oracle(name, total)
        for b in range(int(t["B"])):
            r0 = int(t["state_off"][b]) * A
            assert vsa[r0:r0 + A].sum() >= total - 200


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_batches_fail_when_forced(need_gpu, name):
    t = _tables(name)
    env = _create(t, None)
    try:
        assert not env.k1s_plan()["ok"] and not env.lds_plan()["eligible"]
        env.set_rollout_kernel(L.ROLLOUT_LDS_STOCHASTIC)
        env.reset()
        with pytest.raises(L.CmdpError) as e:
            env.rollout(64)
        assert e.value.code == L.ERR_UNSUPPORTED
    finally:
        env.close()
    if name in REFUSED_ROLLOUT:
        a = _run(t, None, L.ROLLOUT_AUTO, K.LAUNCHES)
        last, rsum, vs, vsa = _oracle(name, int(sum(K.LAUNCHES)))
        assert np.array_equal(a["last"][-1], last) and np.array_equal(a["vs"], vs) and np.array_equal(a["vsa"], vsa)
        np.testing.assert_allclose(np.sum(a["rsum"], axis=0), rsum, rtol=1e-12, atol=0)
