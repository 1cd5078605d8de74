"""The logged loop of the park-and-solve agents on the device: cmdp_psrl_run_logged / cmdp_ucrl2_run_logged (one in-order
driver) against the Python-driven loop of experiment/batched_loop.py, row for row; UCRL2's reuse of the policy of an
unchanged model; the benchmark runner with --agents.

Two agents built the same way on two handles walk the same trajectory (the reference sampler is a host RandomState per
instance, the Philox sampler a pure function of key, episode and tables), so the two routes are compared for identity:
every logged value equal in value and numpy type, `steps_per_second` (wall clock) excepted.

A device batch shares n_actions, the horizon and the rewards range, so the models below run as one device batch per
(n_actions, horizon); where a family allows two sizes at one horizon the batch is ragged."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from colosseum_amd import _lib as L
from colosseum_amd.agents import BatchedPSRLEpisodic, BatchedUCRL2Continuous
from colosseum_amd.batched import BatchedMDP
from colosseum_amd.experiment.batched_loop import BatchedContinuousLoop, BatchedEpisodicLoop
from colosseum_amd.experiment.vector_tracker import n_log_rows
from colosseum_amd.mdp import make_model

pytestmark = pytest.mark.gpu

EPISODIC = [
    [("DeepSeaEpisodic", dict(seed=0, size=3)), ("DeepSeaEpisodic", dict(seed=4, size=3, p_rand=0.2))],
    [("RiverSwimEpisodic", dict(seed=1, size=6)), ("RiverSwimEpisodic", dict(seed=5, size=4, H=6))],   # ragged
    [("SimpleGridEpisodic", dict(seed=2, size=3, n_starting_states=3)), ("SimpleGridEpisodic", dict(seed=6, size=3, n_starting_states=2))],
    [("FrozenLakeEpisodic", dict(seed=3, size=3, p_frozen=.9, p_rand=.1, make_reward_stochastic=True)),
     ("FrozenLakeEpisodic", dict(seed=7, size=3, p_frozen=.8, p_rand=.1, make_reward_stochastic=True))],
]
CONTINUOUS = [
    [("RiverSwimContinuous", dict(seed=0, size=5)), ("DeepSeaContinuous", dict(seed=3, size=4, p_rand=.1))],   # ragged
    [("SimpleGridContinuous", dict(seed=1, size=3, n_starting_states=2)), ("SimpleGridContinuous", dict(seed=6, size=4, n_starting_states=2))],
    [("FrozenLakeContinuous", dict(seed=2, size=3, p_frozen=.9, p_rand=.1)), ("FrozenLakeContinuous", dict(seed=7, size=4, p_frozen=.9, p_rand=.1))],
]
_MODELS = {}


def models_of(batch):
    key = json.dumps(batch, sort_keys=True)
    if key not in _MODELS:
        _MODELS[key] = [make_model(cls, **kw) for cls, kw in batch]
    return _MODELS[key]


def triple(models, agent_cls, setup="mt", T=1000, n_check=10, **kw):
    """(env, agent, loop).  setup "mt": MT19937 transition streams, Beta rewards as their means, PSRL's reference sampler;
    "philox": counter-based streams throughout."""
    beta = any(not m.deterministic_rewards for m in models)
    B = len(models)
    if setup == "mt":
        env = BatchedMDP(models, rng_mode=L.RNG_MT_COMPAT, flags=L.FLAG_REWARD_MEANS if beta else 0)
    else:
        env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=np.arange(B, dtype=np.uint64) * 7919 + 5)
    seeds = [11 + 3 * b for b in range(B)]
    if agent_cls is BatchedPSRLEpisodic:
        agent = agent_cls(env, seeds, optimization_horizon=T, sampler="reference" if setup == "mt" else "philox", **kw)
        loop = BatchedEpisodicLoop(env, agent, n_check)
    else:
        agent = agent_cls(env, seeds, optimization_horizon=T, bound_type_p="bernstein", **kw)
        loop = BatchedContinuousLoop(env, agent, n_check)
    return env, agent, loop


def pair(models, agent_cls, **kw):
    """Two identical (env, agent, loop) triples: the first runs the library's driver, the second the Python-driven loop."""
    a, b = triple(models, agent_cls, **kw), triple(models, agent_cls, **kw)
    b[2].native = False
    return a, b


def close(*triples):
    for env, agent, _ in triples:
        agent.close()
        env.close()


def run_native(loop, T, log_every, max_time=np.inf):
    """The library's driver itself: `loop.run` would fall back to the Python-driven loop on CMDP_ERR_UNSUPPORTED."""
    assert loop.native
    return loop._run_native(T, log_every, max_time)


def assert_rows_equal(la, ra, lb, rb):
    assert len(ra) == len(rb)
    for ta, tb in zip(ra, rb):
        assert len(ta) == len(tb)
        for x, y in zip(ta, tb):
            assert set(x) == set(y)
            for k in x:
                if k != "steps_per_second":
                    assert x[k] == y[k] and type(x[k]) is type(y[k]), (k, x["steps"], x[k], y[k])
    np.testing.assert_array_equal(la.vt.is_training, lb.vt.is_training)
    np.testing.assert_array_equal(la.last_training_step, lb.last_training_step)


def both_routes(batch, agent_cls, T, log_every, max_time=np.inf, **kw):
    """Runs the pair; returns the two triples (open) and the native rows after holding them against the Python-driven ones."""
    a, b = pair(models_of(batch), agent_cls, T=T, **kw)
    rows = run_native(a[2], T, log_every, max_time)
    assert_rows_equal(a[2], rows, b[2], b[2].run(T, log_every, max_time))
    assert all(len(t) == n_log_rows(T, log_every) for t in rows)
    return a, b, rows


SCHEDULES_PSRL = [(600, 50), (601, 50), (40, 1), (300, -1)]   # the last interval short; no step between rows; the final row only
SCHEDULES_UCRL2 = [(400, 40), (401, 40), (30, 1), (200, -1)]


@pytest.mark.parametrize("T,log_every", SCHEDULES_PSRL)
@pytest.mark.parametrize("setup", ["mt", "philox"])
def test_psrl_native_rows_are_the_python_driven_rows(need_gpu, setup, T, log_every):
    for batch in EPISODIC:
        a, b, rows = both_routes(batch, BatchedPSRLEpisodic, T, log_every, setup=setup)
        assert [r["steps"] for r in rows[0]] == ([t for t in range(log_every, T, log_every)] if log_every > 0 else []) + [T - 1]
        np.testing.assert_array_equal(a[1].model()["episode"], b[1].model()["episode"])
        close(a, b)


# Picked on the MI355X: with two rows to check, some instances of the batches turn optimal (two successive rows with a
# normalised regret of ~0 after 0.2 T) well before the end and others never do.
FREEZE_T, FREEZE_EVERY = 1000, 50


def test_psrl_freeze_by_optimality_masks_the_instance_in_both_routes(need_gpu):
    frozen = training = 0
    for batch in EPISODIC:
        a, b, rows = both_routes(batch, BatchedPSRLEpisodic, FREEZE_T, FREEZE_EVERY, setup="mt", n_check=2)
        assert (a[2].last_training_step == -1).all()   # no time limit: whoever stopped training was found optimal
        frozen += int((~a[2].vt.is_training).sum())
        training += int(a[2].vt.is_training.sum())
        # a frozen instance samples nothing: it has drawn fewer posterior samples than its episodes would have asked for
        ep = a[1].model()["episode"]
        np.testing.assert_array_equal(ep, b[1].model()["episode"])
        H = int(a[0].H)
        for i in np.flatnonzero(~a[2].vt.is_training):
            assert ep[i] < 1 + FREEZE_T // H
        close(a, b)
    print(f"frozen by optimality {frozen}, still training {training}")
    assert frozen >= 1 and training >= 1


@pytest.mark.parametrize("T,log_every", SCHEDULES_UCRL2)
def test_ucrl2_native_rows_are_the_python_driven_rows(need_gpu, T, log_every):
    for batch in CONTINUOUS:
        a, b, rows = both_routes(batch, BatchedUCRL2Continuous, T, log_every)
        ma, mb = a[1].model(), b[1].model()
        for k in ("iteration", "episode"):
            np.testing.assert_array_equal(ma[k], mb[k])
        close(a, b)


@pytest.mark.parametrize("which", range(len(CONTINUOUS)))
def test_ucrl2_policy_reuse_changes_no_row_and_skips_solves(need_gpu, which):
    T, log_every = 300, 1
    stats, rows = {}, {}
    for reuse in (True, False):
        a, b = pair(models_of(CONTINUOUS[which]), BatchedUCRL2Continuous, T=T)
        for t in (a, b):
            t[1]._set_policy_reuse(reuse)
        rows[reuse] = run_native(a[2], T, log_every)
        assert_rows_equal(a[2], rows[reuse], b[2], b[2].run(T, log_every))
        stats[reuse] = (a[1].stats(), b[1].stats())
        if reuse:
            keep = (a, b)
        else:
            assert_rows_equal(keep[0][2], rows[True], a[2], rows[False])
            close(a, b, *keep)
    B = len(CONTINUOUS[which])
    for route in (0, 1):
        on, off = stats[True][route], stats[False][route]
        print(f"route {route}: reuse on solved {on['policy_solved']} reused {on['policy_reused']}; off solved {off['policy_solved']}")
        assert off["policy_reused"] == 0 and off["policy_solved"] == on["policy_solved"] + on["policy_reused"]
        assert on["policy_reused"] > 0 and on["policy_solved"] < off["policy_solved"]
        assert off["policy_solved"] <= B * n_log_rows(T, log_every)


def test_ucrl2_plain_calls_reuse_the_policy_of_an_unchanged_model(need_gpu):
    env, agent, _ = triple(models_of(CONTINUOUS[0]), BatchedUCRL2Continuous)
    env2, agent2, _ = triple(models_of(CONTINUOUS[0]), BatchedUCRL2Continuous)
    agent2._set_policy_reuse(False)
    B = env.B
    for e in (env, env2):
        e.reset()
    # Step counts picked on the MI355X: the 40th step of this batch ends an artificial episode of one of its two instances
    # and not of the other, so the request after it solves a strict, non-empty subset of what it is asked for -- the only
    # case in which K14 is launched on a list of instances
    for ag in (agent, agent2):
        ag.run(39)
    first, first2 = agent.average_reward(), agent2.average_reward()
    s0 = agent.stats()
    assert (s0["policy_solved"], s0["policy_reused"]) == (B, 0)
    pi0, ep0 = agent.policy(), agent.model()["episode"].copy()   # the model has not moved: all B reused
    s1 = agent.stats()
    assert (s1["policy_solved"], s1["policy_reused"]) == (B, B)
    for ag in (agent, agent2):
        ag.run(1)
    ep1 = agent.model()["episode"]
    second, second2 = agent.average_reward(), agent2.average_reward()
    s2 = agent.stats()
    moved = int((ep1 != ep0).sum())
    assert 0 < moved < B
    assert s2["policy_solved"] - s1["policy_solved"] == moved and s2["policy_reused"] - s1["policy_reused"] == B - moved
    pi1, pi2 = agent.policy(), agent2.policy()
    for b in range(B):   # the switch changes no bit, whether a stored policy was used or not
        assert first[b] == first2[b] and type(first[b]) is type(first2[b])
        assert second[b] == second2[b] and type(second[b]) is type(second2[b])
        np.testing.assert_array_equal(pi1[b], pi2[b])
        if ep1[b] == ep0[b]:
            np.testing.assert_array_equal(pi1[b], pi0[b])
    assert agent2.stats()["policy_reused"] == 0
    # a mask asks for (and counts) its instances only; an option that may change a solve discards the stored ones
    mask = np.zeros(B, bool)
    mask[0] = True
    s3 = agent.stats()
    np.testing.assert_array_equal(agent.policy(mask)[0], pi1[0])
    s4 = agent.stats()
    assert (s4["policy_solved"] - s3["policy_solved"], s4["policy_reused"] - s3["policy_reused"]) == (0, 1)
    agent._set_policy_size_threshold(300 * 3 * 300)
    agent.policy()
    assert agent.stats()["policy_solved"] - s4["policy_solved"] == B
    close((env, agent, None), (env2, agent2, None))


@pytest.mark.parametrize("agent_cls,batch", [(BatchedPSRLEpisodic, EPISODIC[1]), (BatchedUCRL2Continuous, CONTINUOUS[0])])
def test_time_limit_freezes_every_instance_at_the_first_row(need_gpu, agent_cls, batch):
    T, log_every = 200, 20
    a, b, rows = both_routes(batch, agent_cls, T, log_every, max_time=0.0)
    for t in (a, b):
        assert (t[2].last_training_step == 20).all() and not t[2].vt.is_training.any()
    # nothing was learnt after step 20: the model is that of an identical agent run for steps 0 .. 20
    c = triple(models_of(batch), agent_cls, T=T)
    c[0].reset_visits()
    c[0].reset()
    c[1].run(21)
    ma, mc = a[1].model(), c[1].model()
    np.testing.assert_array_equal(ma["episode"], mc["episode"])
    for k in (("transitions", "rewards") if agent_cls is BatchedPSRLEpisodic else ("N", "P", "estimated_rewards", "iteration")):
        for x, y in zip(ma[k], mc[k]):
            np.testing.assert_array_equal(x, y)
    close(a, b, c)


def _snapshot(env, agent):
    m = agent.model()
    flat = []
    for k in sorted(m):
        flat += [np.asarray(x).copy() for x in (m[k] if isinstance(m[k], list) else [m[k]])]
    return [np.asarray(x).copy() for x in env.state()] + [np.asarray(x).copy() for x in env.visits()] + flat


@pytest.mark.parametrize("agent_cls,batch", [(BatchedPSRLEpisodic, EPISODIC[1]), (BatchedUCRL2Continuous, CONTINUOUS[0])])
def test_refusals_leave_the_agent_untouched(need_gpu, agent_cls, batch):
    T, log_every = 100, 10
    env, agent, loop = triple(models_of(batch), agent_cls, T=T)
    env.reset()
    desc, keep = loop._desc(T, log_every, np.inf)
    before = _snapshot(env, agent)
    with pytest.raises(L.CmdpError) as e:
        agent.run_logged(desc, n_log_rows(T, log_every) + 1)
    assert e.value.code == L.ERR_INVALID and "n_logs" in str(e.value)
    for x, y in zip(before, _snapshot(env, agent)):
        np.testing.assert_array_equal(x, y)
    agent.run(5)
    before = _snapshot(env, agent)
    with pytest.raises(L.CmdpError) as e:
        agent.run_logged(desc, n_log_rows(T, log_every))
    assert e.value.code == L.ERR_INVALID and "already taken" in str(e.value)
    for x, y in zip(before, _snapshot(env, agent)):
        np.testing.assert_array_equal(x, y)
    close((env, agent, loop))


# ---- the runner ---------------------------------------------------------------------------------------------------------
ENV = dict(os.environ)
ENV.pop("RANK", None)
ENV.pop("WORLD_SIZE", None)


def _runner(out, benchmark, agents):
    cmd = [sys.executable, "tools/run_benchmark.py", "--configs-json", os.path.join(GOLDEN, "G11_benchmark_configs.json"), "--benchmark",
           benchmark, "--steps", "300", "--seeds", "1", "--log-every", "50", "--beta-rewards", "philox", "--out", str(out)]
    p = subprocess.run(cmd + (["--agents"] + agents if agents else []), cwd=ROOT, env=ENV, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _csv(folder, ins):
    from colosseum_amd import benchmark as bm

    with open(bm.log_file(str(folder), ins), newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


@pytest.mark.parametrize("benchmark,agents", [("benchmark_episodic_ergodic", ["QLearningEpisodic", "PSRLEpisodic"]),
                                              ("benchmark_continuous_ergodic", ["UCRL2Continuous"])])
def test_runner_writes_reference_layout_logs_for_every_agent(need_gpu, tmp_path, benchmark, agents):
    from colosseum_amd import benchmark as bm

    cfg = json.load(open(os.path.join(GOLDEN, "G11_benchmark_configs.json")))[benchmark]["mdp_configs"]
    s = _runner(tmp_path / "agents", benchmark, agents)
    instances = bm.enumerate_instances(cfg, 1, agents=agents)
    default = bm.enumerate_instances(cfg, 1)
    assert s["instances"] == s["run"] == len(instances) == len(agents) * len(default)
    header = sorted(L.LOG_COLUMNS + ["steps"])
    for ins in instances:
        assert bm.log_file(str(tmp_path / "agents"), ins).endswith(
            os.path.join("logs", f"{ins.mdp_scope}-{ins.mdp_cls}____prms_0-{ins.agent_cls}", "seed0_logs.csv"))
        h, rows = _csv(tmp_path / "agents", ins)
        assert h == header and len(h) == 18 and len(rows) == n_log_rows(300, 50)   # the header of every agent's file
        assert [r[h.index("steps")] for r in rows] == ["50", "100", "150", "200", "250", "299"]
    if default[0].agent_cls not in agents:
        return
    # the Q-learning logs do not depend on which other agents the run holds
    _runner(tmp_path / "default", benchmark, None)
    skip = header.index("steps_per_second")
    for ins in default:
        (h1, r1), (h2, r2) = _csv(tmp_path / "agents", ins), _csv(tmp_path / "default", ins)
        assert h1 == h2 and len(r1) == len(r2)
        for x, y in zip(r1, r2):
            assert [v for i, v in enumerate(x) if i != skip] == [v for i, v in enumerate(y) if i != skip]
