"""min_steps_before_new_episode on the device (the gate of k_psrlc_walk<GATE, OPT>, CMDP_PSRLC_OPT_MIN_STEPS): the steps at
which an instance's `episode` advances are those of the gated rule of tests/helpers_psrlc_gate.py -- which
tests/test_psrlc_gate.py holds against the reference's own runs (golden G24) -- fed the device's transitions, and
`last_change` is the rule's; the reference's `ended` flags themselves where the device can follow the reference's trajectory;
splitting a run, freezing an instance, and min_steps = 0 change nothing they should not; the option's refusals.

The batches are the two-instance ragged ones of tests/test_gpu_logged_agents.py (S <= 16); the optimistic agent runs with
max_psi = 4."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from colosseum_amd import _lib as L
from colosseum_amd.agents import BatchedPSRLContinuous, BatchedPSRLContinuousOptimistic
from colosseum_amd.batched import BatchedMDP
from colosseum_amd.mdp import make_model
from helpers_psrlc_gate import gate_schedule
from test_gpu_logged_agents import CONTINUOUS, models_of

pytestmark = pytest.mark.gpu

G24 = os.path.join(ROOT, "tests", "golden", "G24_psrlc_gate.npz")
T = 300
MIN_STEPS = [1, 7, 10_000]
KINDS = ["plain", "optimistic"]


def make(models, kind, sampler, min_steps=None, seeds=None, horizon=T):
    """(env, agent) after the environment's reset.  Sampler "reference": MT19937 transition streams and the reference's own
    draws; "philox": counter-based streams throughout."""
    B = len(models)
    beta = any(not m.deterministic_rewards for m in models)
    if sampler == "reference":
        env = BatchedMDP(models, rng_mode=L.RNG_MT_COMPAT, flags=L.FLAG_REWARD_MEANS if beta else 0)
    else:
        env = BatchedMDP(models, rng_mode=L.RNG_PHILOX, philox_keys=np.arange(B, dtype=np.uint64) * 7919 + 5)
    env.reset()
    seeds = [11 + 3 * b for b in range(B)] if seeds is None else seeds
    if kind == "plain":
        agent = BatchedPSRLContinuous(env, seeds, horizon, sampler=sampler, no_optimistic_sampling=True)
    else:
        agent = BatchedPSRLContinuousOptimistic(env, seeds, horizon, sampler=sampler, max_psi=4)
    if min_steps is not None:
        agent.set_min_steps_before_new_episode(min_steps)
        assert agent.min_steps_before_new_episode == min_steps
    return env, agent


def close(*pairs):
    for env, agent in pairs:
        agent.close()
        env.close()


def pairs_of(out, start, b, k):
    """The (s, a) pairs of instance b's first k steps of a traced call that began in state `start`."""
    s = np.concatenate([[start], out["observations"][:k - 1, b]]) if k else np.zeros(0, np.int64)
    return list(zip(s.tolist(), out["actions"][:k, b].tolist()))


def walk(env, agent, n_steps):
    """Steps every instance at least n_steps, stopping each at its own episode ends (`stop_at_episode_end`: a call returns
    after the instance's next episode_end_update), so that the step of every advance of `episode` is known.  Returns per
    instance the (s, a) pairs and the flags `ended`."""
    B = env.B
    cur = env.state()[0].copy()
    pairs, ended = [[] for _ in range(B)], [[] for _ in range(B)]
    ep = agent.model()["episode"].copy()
    done = np.zeros(B, np.int64)
    while done.min() < n_steps:
        n = int(n_steps - done.min())
        out = agent.run(n, trace=True, stop_at_episode_end=True)
        ep2 = agent.model()["episode"]
        for b in range(B):
            k = int(out["steps_taken"][b])
            assert 1 <= k <= n and ep2[b] - ep[b] in (0, 1), b
            assert ep2[b] != ep[b] or k == n, b   # stopped early only by an episode end
            pairs[b] += pairs_of(out, cur[b], b, k)
            ended[b] += [False] * (k - 1) + [bool(ep2[b] != ep[b])]
            cur[b] = out["observations"][k - 1, b]
        assert np.array_equal(env.state()[0], cur)
        ep = ep2.copy()
        done += out["steps_taken"]
    return pairs, [np.array(e) for e in ended]


@pytest.mark.parametrize("min_steps", MIN_STEPS)
@pytest.mark.parametrize("sampler", ["reference", "philox"])
@pytest.mark.parametrize("kind", KINDS)
def test_episode_advances_where_the_gated_rule_says(need_gpu, kind, sampler, min_steps):
    # m = 1 takes a round at every step, each a solve of some 10 ms: one batch a case there, the four cases between them all
    # three (the optimistic agent's rounds on CONTINUOUS[1], five actions, are the longest: it has them at m = 7 and 10 000)
    first = {("plain", "reference"): 1, ("plain", "philox"): 2, ("optimistic", "reference"): 0, ("optimistic", "philox"): 2}
    for batch in ([CONTINUOUS[first[kind, sampler]]] if min_steps == 1 else CONTINUOUS):
        models = models_of(batch)
        # stopped at every episode end: the step of every advance
        env, agent = make(models, kind, sampler, min_steps)
        pairs, ended = walk(env, agent, T)
        gate = agent.episode_gate()
        assert gate["min_steps"] == min_steps and gate["last_change"].dtype == np.int32
        for b, m in enumerate(models):
            want, rule = gate_schedule(pairs[b], m.n_states, m.n_actions, min_steps)
            assert np.array_equal(ended[b], want), (b, np.flatnonzero(ended[b] != want)[:5])
            assert gate["last_change"][b] == rule.last_change, b
            if min_steps == 1:
                assert not ended[b][0] and ended[b][1] and rule.last_change == len(pairs[b]) - 1
            if min_steps > T:
                assert not ended[b].any() and rule.last_change == 0
            if min_steps == 7:
                assert 1 <= ended[b].sum() <= len(pairs[b]) // 7
        # one call of 300 steps: as many advances as the rule counts on its trace, and the rule's last_change
        env2, agent2 = make(models, kind, sampler, min_steps)
        start = env2.state()[0].copy()
        out = agent2.run(T, trace=True)
        assert (out["steps_taken"] == T).all()
        ep, gate2 = agent2.model()["episode"], agent2.episode_gate()
        for b, m in enumerate(models):
            want, rule = gate_schedule(pairs_of(out, start[b], b, T), m.n_states, m.n_actions, min_steps)
            assert ep[b] == 1 + want.sum() and gate2["last_change"][b] == rule.last_change, b
        assert agent2.stats()["solves"] >= len(models)
        close((env, agent), (env2, agent2))


def test_ended_flags_are_the_references(need_gpu):
    """The reference sampler on MT-compatible streams draws the reference's numbers, so where the rewards are deterministic the
    device walks the reference's trajectory for as long as its Q orders the actions as the reference's does, and G24's `ended`
    flags are the device's."""
    z = np.load(G24)
    meta = json.loads(str(z["cases"]))
    seen = 0
    for i, m in enumerate(meta):
        model = make_model(m["cls"], **m["params"])
        if not model.deterministic_rewards:
            continue
        seen += 1
        env, agent = make([model], "plain" if m["plain"] else "optimistic", "reference", m["min_steps"], seeds=[m["seed"]],
                          horizon=m["T"])
        if not m["plain"]:
            assert agent.psi.tolist() == [m["psi"]] and agent.eta.tolist() == [m["eta"]]
        pairs, ended = walk(env, agent, m["T"])
        steps = z[f"c{i}_steps"]
        mine = np.array(pairs[0][:m["T"]])
        d = np.flatnonzero((mine != steps[:, :2]).any(-1))
        print(f"case {i} ({m['cls']}, plain={m['plain']}, m={m['min_steps']}): {int(ended[0][:m['T']].sum())} episode ends, the "
              f"reference {int(steps[:, 3].sum())}; (s, a) leaves the reference's at step {int(d[0]) if len(d) else None}")
        assert np.array_equal(ended[0][:m["T"]], steps[:, 3].astype(bool)), (i, np.flatnonzero(ended[0][:m["T"]] != steps[:, 3])[:5])
        close((env, agent))
    assert seen >= 6


def tables(env, agent):
    m = agent.model()
    flat = []
    for k in sorted(m):
        flat += [np.asarray(x).copy() for x in (m[k] if isinstance(m[k], list) else [m[k]])]
    flat += [np.asarray(q).copy() for q in agent.last_sample()["Q"]]
    return flat + [np.asarray(x).copy() for x in env.state()] + [agent.episode_gate()["last_change"]]


@pytest.mark.parametrize("sampler", ["reference", "philox"])
@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_of_150_are_one_of_300(need_gpu, kind, sampler):
    models = models_of(CONTINUOUS[0])
    a, b = make(models, kind, sampler, 7), make(models, kind, sampler, 7)
    o1 = a[1].run(T, trace=True)
    o2 = [b[1].run(T // 2, trace=True) for _ in range(2)]
    for k in ("actions", "observations", "rewards"):
        np.testing.assert_array_equal(o1[k], np.concatenate([o[k] for o in o2]))
    np.testing.assert_array_equal(o1["cumulative_reward"], o2[1]["cumulative_reward"])
    for x, y in zip(tables(*a), tables(*b)):
        np.testing.assert_array_equal(x, y)
    assert a[1].episode_gate()["last_change"].max() > T // 2   # the gate's state crossed the call boundary
    close(a, b)


@pytest.mark.parametrize("kind", KINDS)
def test_frozen_instance_never_moves_last_change(need_gpu, kind):
    models = models_of(CONTINUOUS[1])
    env, agent = make(models, kind, "philox", 1)
    agent.run(100, train=[True, False])
    assert agent.episode_gate()["last_change"].tolist() == [99, 0]
    ep = agent.model()["episode"]
    assert ep[0] > 1 and ep[1] == 1
    agent.run(50, train=[False, True])   # the instance's own clock: h is 100 at its first check
    assert agent.episode_gate()["last_change"].tolist() == [99, 149]
    close((env, agent))


@pytest.mark.parametrize("sampler", ["reference", "philox"])
@pytest.mark.parametrize("kind", KINDS)
def test_min_steps_0_is_the_agent_that_never_set_it(need_gpu, kind, sampler):
    models = models_of(CONTINUOUS[2])
    a, b = make(models, kind, sampler, None), make(models, kind, sampler, 0)
    oa, ob = a[1].run(T, trace=True), b[1].run(T, trace=True)
    for k in ("actions", "observations", "rewards", "cumulative_reward"):
        np.testing.assert_array_equal(oa[k], ob[k])
    for x, y in zip(tables(*a), tables(*b)):
        np.testing.assert_array_equal(x, y)
    for t in (a, b):
        g = t[1].episode_gate()
        assert g["min_steps"] == 0 and not g["last_change"].any()
    close(a, b)


@pytest.mark.parametrize("kind", KINDS)
def test_option_refusals(need_gpu, kind):
    env, agent = make(models_of(CONTINUOUS[0]), kind, "philox")
    lib = L.load()
    for bad in (-1, 1 << 31):
        assert lib.cmdp_psrlc_set_option(agent._h, L.PSRLC_OPT_MIN_STEPS, bad) == L.ERR_INVALID
        assert b"min_steps_before_new_episode" in lib.cmdp_last_error()
    agent.set_min_steps_before_new_episode((1 << 31) - 1)
    agent.set_min_steps_before_new_episode(3)
    assert agent.min_steps_before_new_episode == 3
    agent.run(1)
    with pytest.raises(L.CmdpError) as e:
        agent.set_min_steps_before_new_episode(5)
    assert e.value.code == L.ERR_INVALID and "already taken" in str(e.value)
    assert agent.min_steps_before_new_episode == 3
    close((env, agent))
