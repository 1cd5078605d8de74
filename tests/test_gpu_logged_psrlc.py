"""The logged loop of the continuous PSRL agents on the device: cmdp_psrlc_run_logged (a third adapter of the in-order driver,
reached through BatchedContinuousLoop) against the Python-driven loop of experiment/batched_loop.py, row for row, for the plain
and the optimistic agent, both samplers, both policy routes, both sample routes and with min_steps_before_new_episode; the
time limit, the freeze by optimality and the refusals; the tuned agent of benchmark.make_psrl_continuous through the loop.

The pattern is tests/test_gpu_logged_agents.py's: two agents built the same way on two handles walk the same trajectory, so
the two routes are compared for identity, `steps_per_second` (wall clock) excepted.  The optimistic agent runs with
max_psi = 4."""
import numpy as np
import pytest

from colosseum_amd import _lib as L
from colosseum_amd import benchmark as bm
from colosseum_amd.agents import BatchedPSRLContinuous, BatchedPSRLContinuousOptimistic
from colosseum_amd.batched import BatchedMDP
from colosseum_amd.experiment.batched_loop import BatchedContinuousLoop
from colosseum_amd.experiment.vector_tracker import n_log_rows
from test_gpu_logged_agents import CONTINUOUS, _snapshot, assert_rows_equal, close, models_of, run_native

pytestmark = pytest.mark.gpu

CLASSES = [BatchedPSRLContinuous, BatchedPSRLContinuousOptimistic]
SCHEDULES = [(400, 40), (401, 40), (30, 1), (200, -1)]   # the last interval short; no step between rows; the final row only
# A round of these agents is a solve of some 10 ms whatever the size, and without the gate a run takes one at most of its
# steps: a case runs ONE batch, the cases of a class and sampler between them all three.  Measured on the MI355X, a run of 400
# steps of the optimistic agent takes 0.5 s on CONTINUOUS[0], 3 s on [2] and 8 s on [1] (five actions, the most rounds), so
# [1] goes to the schedule of 30 steps.
BATCH_OF = {"mt": (0, 2, 1, 0), "philox": (2, 0, 1, 2)}


def triple(models, agent_cls, setup="mt", T=1000, n_check=10, policy_solver=None, min_steps=None, **kw):
    """(env, agent, loop).  setup "mt": MT19937 transition streams, Beta rewards as their means, the reference sampler;
    "philox": counter-based streams throughout."""
    beta = any(not m.deterministic_rewards for m in models)
    B = len(models)
    if setup == "mt":
        env = BatchedMDP(models, rng_mode=L.RNG_MT_COMPAT, flags=L.FLAG_REWARD_MEANS if beta else 0)
    else:
        env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=np.arange(B, dtype=np.uint64) * 7919 + 5)
    seeds = [11 + 3 * b for b in range(B)]
    kw = dict(kw, sampler="reference" if setup == "mt" else "philox")
    if agent_cls is BatchedPSRLContinuous:
        kw.pop("sample_solver", None)
        agent = agent_cls(env, seeds, optimization_horizon=T, no_optimistic_sampling=True, **kw)
    else:
        agent = agent_cls(env, seeds, optimization_horizon=T, max_psi=4, **kw)
    if policy_solver is not None:
        agent.set_policy_solver(policy_solver)
    if min_steps is not None:
        agent.set_min_steps_before_new_episode(min_steps)
    return env, agent, BatchedContinuousLoop(env, agent, n_check)


def pair(models, agent_cls, **kw):
    """Two identical (env, agent, loop) triples: the first runs the library's driver, the second the Python-driven loop."""
    a, b = triple(models, agent_cls, **kw), triple(models, agent_cls, **kw)
    b[2].native = False
    return a, b


def both_routes(batch, agent_cls, T, log_every, max_time=np.inf, **kw):
    """Runs the pair; returns the two triples (open) and the native rows after holding them against the Python-driven ones."""
    a, b = pair(models_of(batch), agent_cls, T=T, **kw)
    rows = run_native(a[2], T, log_every, max_time)
    assert_rows_equal(a[2], rows, b[2], b[2].run(T, log_every, max_time))
    assert all(len(t) == n_log_rows(T, log_every) for t in rows)
    np.testing.assert_array_equal(a[1].model()["episode"], b[1].model()["episode"])
    return a, b, rows


@pytest.mark.parametrize("T,log_every", SCHEDULES)
@pytest.mark.parametrize("setup", ["mt", "philox"])
@pytest.mark.parametrize("agent_cls", CLASSES)
def test_native_rows_are_the_python_driven_rows(need_gpu, agent_cls, setup, T, log_every):
    batch = CONTINUOUS[BATCH_OF[setup][SCHEDULES.index((T, log_every))]]
    a, b, rows = both_routes(batch, agent_cls, T, log_every, setup=setup)
    assert [r["steps"] for r in rows[0]] == ([t for t in range(log_every, T, log_every)] if log_every > 0 else []) + [T - 1]
    assert (a[1].model()["episode"] > 1).all()
    close(a, b)


VARIANTS = [dict(policy_solver="dense"), dict(policy_solver="tables"), dict(sample_solver="dense"), dict(sample_solver="compact"),
            dict(min_steps=7)]


# the sample routes are the optimistic agent's
ROUTE_CASES = [(c, v) for c in CLASSES for v in VARIANTS if c is BatchedPSRLContinuousOptimistic or "sample_solver" not in v]


@pytest.mark.parametrize("agent_cls,variant", ROUTE_CASES,
                         ids=lambda x: x.__name__ if isinstance(x, type) else "-".join(map(str, *x.items())))
def test_native_rows_on_every_route_and_with_the_gate(need_gpu, agent_cls, variant):
    T, log_every = 400, 40
    # the routes on one batch each; the gate, which makes rounds rare, on all three
    for batch in (CONTINUOUS if "min_steps" in variant else [CONTINUOUS[2 * (VARIANTS.index(variant) % 2)]]):
        a, b, rows = both_routes(batch, agent_cls, T, log_every, setup="philox", **variant)
        for t in (a, b):
            if "policy_solver" in variant:
                assert t[1].policy_solver == variant["policy_solver"]
            if "sample_solver" in variant and agent_cls is BatchedPSRLContinuousOptimistic:
                assert t[1].sample_solver == t[1].stats()["sample_solver"] == variant["sample_solver"]
            if "min_steps" in variant:
                g = t[1].episode_gate()
                assert g["min_steps"] == 7 and (g["last_change"][t[2].vt.is_training] > T - 8).all()
                assert (t[1].model()["episode"] <= 1 + T // 7).all()
        np.testing.assert_array_equal(a[1].episode_gate()["last_change"], b[1].episode_gate()["last_change"])
        close(a, b)


@pytest.mark.parametrize("agent_cls", CLASSES)
def test_time_limit_freezes_every_instance_at_the_first_row(need_gpu, agent_cls):
    T, log_every = 200, 20
    batch = CONTINUOUS[0]
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
    for k in ("transitions", "rewards", "N_sa", "nu_k"):
        for x, y in zip(ma[k], mc[k]):
            np.testing.assert_array_equal(x, y)
    close(a, b, c)


# Picked on the MI355X (see the printed counts): with two rows to check and T = 200, some instances of these batches turn
# optimal (two successive rows with a normalised regret of ~0 after 0.2 T) before the end and others never do -- the plain
# agent freezes both instances of CONTINUOUS[0] and the first of [1], the optimistic one the first of [0] and none of [2].
# At T >= 300 either agent freezes all of [0] and [1] and none of [2].
FREEZE_T, FREEZE_EVERY = 200, 20
FREEZE_BATCHES = {BatchedPSRLContinuous: (0, 1), BatchedPSRLContinuousOptimistic: (0, 2)}


@pytest.mark.parametrize("agent_cls", CLASSES)
def test_freeze_by_optimality_masks_the_instance_in_both_routes(need_gpu, agent_cls):
    frozen = training = 0
    for k in FREEZE_BATCHES[agent_cls]:
        a, b, rows = both_routes(CONTINUOUS[k], agent_cls, FREEZE_T, FREEZE_EVERY, setup="mt", n_check=2)
        assert (a[2].last_training_step == -1).all()   # no time limit: whoever stopped training was found optimal
        frozen += int((~a[2].vt.is_training).sum())
        training += int(a[2].vt.is_training.sum())
        close(a, b)
    print(f"{agent_cls.__name__}: frozen by optimality {frozen}, still training {training}")
    assert frozen >= 1 and training >= 1


@pytest.mark.parametrize("agent_cls", CLASSES)
def test_refusals_leave_the_agent_untouched(need_gpu, agent_cls):
    T, log_every = 100, 10
    env, agent, loop = triple(models_of(CONTINUOUS[0]), agent_cls, T=T)
    env.reset()
    desc, keep = loop._desc(T, log_every, np.inf)

    def refused(desc, n_logs, code, text):
        before = _snapshot(env, agent)
        with pytest.raises(L.CmdpError) as e:
            agent._run_logged_native(desc, n_logs)
        assert e.value.code == code and text in str(e.value), str(e.value)
        for x, y in zip(before, _snapshot(env, agent)):
            np.testing.assert_array_equal(x, y)

    refused(desc, n_log_rows(T, log_every) + 1, L.ERR_INVALID, "n_logs")
    big = (1 << 24) + 1
    desc_big, keep_big = loop._desc(big, -1, np.inf)
    refused(desc_big, n_log_rows(big, -1), L.ERR_OVERFLOW, "2^24")
    agent.run(5)
    refused(desc, n_log_rows(T, log_every), L.ERR_INVALID, "already taken")
    # the public call stays refused and names the way
    with pytest.raises(NotImplementedError, match="BatchedContinuousLoop"):
        agent.run_logged(desc, n_log_rows(T, log_every))
    close((env, agent, loop))


# ---- the tuned agent of benchmark.make_psrl_continuous through the loop -----------------------------------------------------
@pytest.mark.parametrize("plain", [False, True])
def test_tuned_agent_with_min_steps_bounds_the_solves(need_gpu, plain):
    T, log_every, m = 120, 40, 30
    models = models_of(CONTINUOUS[0])
    trips = []
    for native in (True, False):
        env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=np.arange(len(models), dtype=np.uint64) * 7919 + 5)
        agent = bm.make_psrl_continuous(env, [0, 1], optimization_horizon=T, sampler="philox", min_steps_before_new_episode=m,
                                        no_optimistic_sampling=plain, **bm.DEFAULT_AGENT_CONFIGS["PSRLContinuous"])
        assert type(agent) is (BatchedPSRLContinuous if plain else BatchedPSRLContinuousOptimistic)
        assert agent.policy_solver == "tables" and agent.min_steps_before_new_episode == m
        assert plain or agent.sample_solver == "compact"
        loop = BatchedContinuousLoop(env, agent)
        loop.native = native
        trips.append((env, agent, loop))
    a, b = trips
    rows = run_native(a[2], T, log_every)
    assert_rows_equal(a[2], rows, b[2], b[2].run(T, log_every))
    assert [r["steps"] for r in rows[0]] == [40, 80, 119]
    for t in trips:
        st = t[1].stats()
        print(f"{type(t[1]).__name__}: {st['solves']} solves in {st['rounds']} rounds")
        assert len(models) <= st["solves"] <= len(models) * (1 + T // m)
    close(a, b)
