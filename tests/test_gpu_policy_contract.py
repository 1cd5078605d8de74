"""What cmdp_ucrl2_policy, cmdp_psrl_policy, cmdp_psrl_evaluate and cmdp_psrlc_policy (both routes) do to the caller's
arrays, at the C level: the instances of the mask hold what the unmasked call returns, bit for bit; outside the mask UCRL2
leaves the caller's memory as it found it (pi, Q, sweeps, scheme) and the PSRL agents write zeros; an unmasked call after a
masked one returns the full result again.  Three instances of 4, 9 and 16 states."""
import numpy as np
import pytest

from colosseum_amd import _lib as L
from colosseum_amd.agents import BatchedPSRLContinuous, BatchedPSRLEpisodic, BatchedUCRL2Continuous
from colosseum_amd.batched import BatchedMDP
from colosseum_amd.mdp import make_model

pytestmark = pytest.mark.gpu

SIZES = (4, 9, 16)
SENTINEL = {np.float32: np.float32(-12345.5), np.int64: np.int64(-77), np.int32: np.int32(-77)}
MASKS = [np.array([1, 0, 1], np.uint8), np.zeros(3, np.uint8)]
_MODELS = {}


def models(cls):
    if cls not in _MODELS:
        kw = dict(H=max(SIZES)) if cls.endswith("Episodic") else {}   # a device batch shares the horizon
        _MODELS[cls] = [make_model(cls, seed=3 + i, size=n, **kw) for i, n in enumerate(SIZES)]
    return _MODELS[cls]


def ucrl2(reuse):
    env = BatchedMDP(models("RiverSwimContinuous"), rng_mode=L.RNG_MT_COMPAT)
    agent = BatchedUCRL2Continuous(env, [11, 14, 17], optimization_horizon=1000, bound_type_p="bernstein")
    agent._set_policy_reuse(reuse)
    R, B = int(env.row_off[-1]), env.B
    spans = [(np.float32, env.row_off), (np.float32, env.row_off), (np.int64, np.arange(B + 1)), (np.int32, np.arange(B + 1))]
    return env, agent, agent._lib.cmdp_ucrl2_policy, spans, False


def psrl(entry):
    env = BatchedMDP(models("RiverSwimEpisodic"), rng_mode=L.RNG_MT_COMPAT)
    agent = BatchedPSRLEpisodic(env, [11, 14, 17], optimization_horizon=1000, sampler="philox")
    if entry == "evaluate":
        return env, agent, agent._lib.cmdp_psrl_evaluate, [(np.float32, env.state_off)], True
    layers = (int(env.H) + 1) * np.asarray(env.row_off)
    return env, agent, agent._lib.cmdp_psrl_policy, [(np.float32, layers), (np.float32, layers)], True


def psrlc(route):
    env = BatchedMDP(models("RiverSwimContinuous"), rng_mode=L.RNG_MT_COMPAT)
    agent = BatchedPSRLContinuous(env, [11, 14, 17], optimization_horizon=1000, no_optimistic_sampling=True, sampler="philox")
    agent.set_policy_solver(route)
    B = env.B
    spans = [(np.float32, env.row_off), (np.float32, env.row_off), (np.int64, np.arange(B + 1)), (np.int32, np.arange(B + 1))]
    return env, agent, agent._lib.cmdp_psrlc_policy, spans, True


CASES = {"ucrl2-reuse": lambda: ucrl2(True), "ucrl2-solve": lambda: ucrl2(False), "psrl-policy": lambda: psrl("policy"),
         "psrl-evaluate": lambda: psrl("evaluate"), "psrlc-dense": lambda: psrlc("dense"), "psrlc-tables": lambda: psrlc("tables")}


@pytest.mark.parametrize("case", list(CASES))
def test_caller_arrays_inside_and_outside_the_mask(need_gpu, case):
    env, agent, entry, spans, zeroed = CASES[case]()
    env.reset()
    agent.run(60)

    def call(mask):
        out = [np.full(int(off[-1]), SENTINEL[dt], dt) for dt, off in spans]
        L.check(entry(agent._h, L.ptr(mask), *[L.ptr(x) for x in out]))
        return out

    full = call(None)
    assert (full[0] != SENTINEL[np.float32]).all()   # the unmasked call fills every element
    for mask in MASKS:
        got = call(mask)
        for x, ref, (dt, off) in zip(got, full, spans):
            for b in range(env.B):
                seg = slice(int(off[b]), int(off[b + 1]))
                if mask[b]:
                    assert x[seg].tobytes() == ref[seg].tobytes(), (case, b)
                else:
                    assert (x[seg] == (0 if zeroed else SENTINEL[dt])).all(), (case, b)
    for x, ref in zip(call(None), full):   # a masked call leaves nothing behind that a later unmasked one could return
        assert x.tobytes() == ref.tobytes()
    agent.close()
    env.close()
