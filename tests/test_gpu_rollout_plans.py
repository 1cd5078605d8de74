"""Pins the rollout plan cmdp_create makes for a matrix of batches: for every batch and every CMDP_OPT_ROLLOUT_KERNEL
value, what cmdp_lds_plan reports (eligible, kernel, instances per workgroup, chunk) and the error code of a short
rollout (0: it ran).  Together they fix which of K1L / K1P / K1T / K1U / K1E / K1S each batch is eligible for, the
automatic choice, the forced choices and their refusals, and the instances per workgroup of every plan.

The expected values were observed on an MI355X: the instances per workgroup follow from the batch's rounds of
workgroups over the device's 256 CUs, so they hold for a 256-CU device only."""
import os

import numpy as np
import pytest

from colosseum_amd import _lib as L
from colosseum_amd.batched import BatchedMDP, tables_from_models
from colosseum_amd.mdp import make_model
from colosseum_amd.mdp.fast_batch import deepsea_episodic_tables

pytestmark = pytest.mark.gpu

KERNELS = (0, 2, 3, 4, 5, 6)   # CMDP_OPT_ROLLOUT_KERNEL: automatic and every forced LDS-resident kernel
KNOBS = ("CMDP_K1L_PIPE", "CMDP_K1T_G", "CMDP_K1U_G", "CMDP_K1S_G", "CMDP_K1L_G", "CMDP_K1T_CH")   # the environment cmdp_create reads


def _det(B, S, A=2, H=16, n_rew=2, permuted=True, seed=0):
    """Deterministic tables with one start state.  `permuted`: every instance is a per-state action permutation of the
    first (A = 2: a swap), else each instance draws its own successors and rewards.  S may be a list (ragged)."""
    rng = np.random.default_rng(seed)
    sizes = [S] * B if np.isscalar(S) else list(S)
    base_n = rng.integers(0, sizes[0], (sizes[0], A))
    base_r = rng.integers(0, n_rew, (sizes[0], A))
    base_r.flat[:n_rew] = np.arange(n_rew)   # every reward value occurs
    nxt, rew = [], []
    for b, Sb in enumerate(sizes):
        if permuted:
            swap = (rng.random(Sb) < 0.5) & (b > 0)
            n, r = np.where(swap[:, None], base_n[:, ::-1], base_n), np.where(swap[:, None], base_r[:, ::-1], base_r)
        else:
            n, r = rng.integers(0, Sb, (Sb, A)), rng.integers(0, n_rew, (Sb, A))
        nxt.append(n.reshape(-1))
        rew.append(r.reshape(-1) / max(1, n_rew - 1))
    R = sum(sizes) * A
    return dict(
        B=B, A=A, H=H, rewards_range=(0.0, 1.0),
        state_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
        sp_ptr=np.arange(R + 1, dtype=np.int64), sp_next=np.concatenate(nxt).astype(np.int32),
        sp_cum=np.ones(R), sp_reward=np.concatenate(rew), sp_rkind=np.zeros(R, np.uint8), sp_rp0=np.concatenate(rew),
        sp_rp1=np.zeros(R), sp_seed=np.zeros(R, np.int32), start_off=np.arange(B + 1, dtype=np.int64),
        start_state=np.zeros(B, np.int32), start_cum=np.ones(B), start_seed=np.zeros(B, np.int32))


def _models(cls, B, with_dp=False, **kw):
    return tables_from_models([make_model(cls, seed=100 + i, **kw) for i in range(B)], True, with_dp)


def _batch(name):
    """name -> (tables, BatchedMDP keywords); deepsea<size>_<B> is DeepSeaEpisodic(seed=i, size) for i < B"""
    P = dict(rng_mode=L.RNG_PHILOX)
    if name.startswith("deepsea") and name[7].isdigit():
        size, B = (int(x) for x in name[7:].split("_"))
        return deepsea_episodic_tables(np.arange(B), size), P
    beta = dict(size=10, make_reward_stochastic=True)
    return {
        "deepsea_continuous": lambda: (_models("DeepSeaContinuous", 70, size=9), P),
        "perm_a2": lambda: (_det(200, 100, H=20, n_rew=3), P),
        "nonperm_a2": lambda: (_det(200, 100, H=20, n_rew=3, permuted=False), P),
        "a4": lambda: (_det(100, 50, A=4, n_rew=3, permuted=False), P),
        "rewards5": lambda: (_det(100, 100, n_rew=5), P),
        "rewards300": lambda: (_det(64, 512, n_rew=300), P),
        "states512": lambda: (_det(256, 512, H=40, n_rew=4), P),
        "states513": lambda: (_det(256, 513, H=40, n_rew=4), P),
        "ragged": lambda: (_det(50, [30 + (i % 7) for i in range(50)], permuted=False), P),
        "stochastic": lambda: (_models("DeepSeaEpisodic", 40, size=10, p_rand=0.3), P),
        "mt_compat": lambda: (deepsea_episodic_tables(np.arange(40), 10), dict(rng_mode=L.RNG_MT_COMPAT)),
        "mt_compat_stochastic": lambda: (_models("DeepSeaEpisodic", 40, size=10, p_rand=0.3), dict(rng_mode=L.RNG_MT_COMPAT)),
        "beta": lambda: (_models("DeepSeaEpisodic", 40, **beta), P),
        "beta_means": lambda: (_models("DeepSeaEpisodic", 40, **beta), dict(P, flags=L.FLAG_REWARD_MEANS)),
        "dense": lambda: (_models("FrozenLakeEpisodic", 8, with_dp=True, size=6, p_frozen=0.9), dict(P, layout=L.LAYOUT_DENSE)),
    }[name]()


CREATE_ONLY = {"deepsea30_65536"}   # the bench's batch: plans only, no rollout


def _create(tables, kw, env_vars):
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env_vars or {})
    try:
        return BatchedMDP(tables=tables, **kw)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def observe(name, env_vars=None):
    """{kernel option: (eligible, kernel name, instances per workgroup, chunk, error code of a 64-transition rollout)}"""
    env = _create(*_batch(name), env_vars)
    out = {}
    try:
        for rk in KERNELS:
            env.set_rollout_kernel(rk)
            p = env.lds_plan()
            code = None
            if name not in CREATE_ONLY:
                code = 0
                try:
                    env.reset()
                    env.rollout(64)
                except L.CmdpError as e:
                    code = e.code
            out[rk] = (int(p["eligible"]), p["kernel"], p["instances_per_workgroup"], p["chunk"], code)
    finally:
        env.close()
    return out


def groups_per_cu():
    """K1L (CMDP_K1L_PIPE=0) at one and at two workgroups per CU (CMDP_OPT_LDS_GROUPS_PER_CU), DeepSea-30 x 4096."""
    env = _create(deepsea_episodic_tables(np.arange(4096), 30), dict(rng_mode=L.RNG_PHILOX), {"CMDP_K1L_PIPE": "0"})
    out = {}
    try:
        env.set_rollout_kernel(L.ROLLOUT_LDS)
        out[0] = tuple(env.lds_plan().values())
        for g in (1, 2):
            env.set_option(L.OPT_LDS_GROUPS_PER_CU, g)
            out[g] = tuple(env.lds_plan().values())
    finally:
        env.close()
    return out


NAMES = ["deepsea8_40", "deepsea30_300", "deepsea10_1", "deepsea10_37", "deepsea10_4096", "deepsea30_65536",
         "deepsea_continuous", "perm_a2", "nonperm_a2", "a4", "rewards5", "rewards300", "states512", "states513", "ragged",
         "stochastic", "mt_compat", "mt_compat_stochastic", "beta", "beta_means", "dense"]
# the knobs cmdp_create reads: K1L or K1P forced, K1T / K1U instances per workgroup
ENV_CASES = {"deepsea10_300_pipe0": ("deepsea10_300", {"CMDP_K1L_PIPE": "0"}),
             "deepsea10_300_pipe1": ("deepsea10_300", {"CMDP_K1L_PIPE": "1"}),
             "deepsea10_300_g30": ("deepsea10_300", {"CMDP_K1T_G": "30", "CMDP_K1U_G": "30"})}

EXPECTED = {
    "deepsea8_40": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_tmpl', 1, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 1, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "deepsea30_300": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 2, 64, 0),
        3: (1, 'k_rollout_pipe', 2, 64, -4),
        4: (1, 'k_rollout_tmpl', 2, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 2, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "deepsea10_1": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_tmpl', 1, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 1, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "deepsea10_37": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_tmpl', 1, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 1, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "deepsea10_4096": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 16, 64, 0),
        3: (1, 'k_rollout_pipe', 16, 64, -4),
        4: (1, 'k_rollout_tmpl', 16, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 16, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "deepsea30_65536": {
        0: (1, 'k_rollout_epi', 32, 128, None),
        2: (1, 'k_rollout_pipe', 52, 32, None),
        3: (1, 'k_rollout_pipe', 52, 32, None),
        4: (1, 'k_rollout_tmpl', 128, 32, None),
        5: (1, 'k_rollout_tmpl_stream', 256, 72, None),
        6: (1, 'k_rollout_epi', 32, 128, None),
    },
    "deepsea_continuous": {
        0: (1, 'k_rollout_pipe', 1, 64, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_tmpl', 1, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 1, 72, 0),
        6: (1, 'k_rollout_pipe', 1, 64, -4),
    },
    "perm_a2": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_tmpl', 1, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 1, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "nonperm_a2": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_pipe', 1, 64, -4),
        5: (1, 'k_rollout_pipe', 1, 64, -4),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "a4": {
        0: (1, 'k_rollout_pipe', 1, 64, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_pipe', 1, 64, -4),
        5: (1, 'k_rollout_pipe', 1, 64, -4),
        6: (1, 'k_rollout_pipe', 1, 64, -4),
    },
    "rewards5": {
        0: (1, 'k_rollout_pipe', 1, 64, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_tmpl', 1, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 1, 72, 0),
        6: (1, 'k_rollout_pipe', 1, 64, -4),
    },
    "rewards300": {
        0: (0, 'k_rollout_lds', 0, 0, 0),
        2: (0, 'k_rollout_lds', 0, 0, -4),
        3: (0, 'k_rollout_lds', 0, 0, -4),
        4: (0, 'k_rollout_lds', 0, 0, -4),
        5: (0, 'k_rollout_lds', 0, 0, -4),
        6: (0, 'k_rollout_lds', 0, 0, -4),
    },
    "states512": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_tmpl', 1, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 1, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "states513": {
        0: (1, 'k_rollout_pipe', 1, 64, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_tmpl', 1, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 1, 64, 0),
        6: (1, 'k_rollout_pipe', 1, 64, -4),
    },
    "ragged": {
        0: (1, 'k_rollout_stoch', 1, 32, 0),
        2: (1, 'k_rollout_stoch', 1, 32, -4),
        3: (1, 'k_rollout_stoch', 1, 32, 0),
        4: (1, 'k_rollout_stoch', 1, 32, -4),
        5: (1, 'k_rollout_stoch', 1, 32, -4),
        6: (1, 'k_rollout_stoch', 1, 32, -4),
    },
    "stochastic": {
        0: (1, 'k_rollout_stoch', 1, 32, 0),
        2: (1, 'k_rollout_stoch', 1, 32, -4),
        3: (1, 'k_rollout_stoch', 1, 32, 0),
        4: (1, 'k_rollout_stoch', 1, 32, -4),
        5: (1, 'k_rollout_stoch', 1, 32, -4),
        6: (1, 'k_rollout_stoch', 1, 32, -4),
    },
    "mt_compat": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_tmpl', 1, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 1, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "mt_compat_stochastic": {
        0: (0, 'k_rollout_lds', 0, 0, 0),
        2: (0, 'k_rollout_lds', 0, 0, -4),
        3: (0, 'k_rollout_lds', 0, 0, -4),
        4: (0, 'k_rollout_lds', 0, 0, -4),
        5: (0, 'k_rollout_lds', 0, 0, -4),
        6: (0, 'k_rollout_lds', 0, 0, -4),
    },
    "beta": {
        0: (0, 'k_rollout_lds', 0, 0, 0),
        2: (0, 'k_rollout_lds', 0, 0, -4),
        3: (0, 'k_rollout_lds', 0, 0, -4),
        4: (0, 'k_rollout_lds', 0, 0, -4),
        5: (0, 'k_rollout_lds', 0, 0, -4),
        6: (0, 'k_rollout_lds', 0, 0, -4),
    },
    "beta_means": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 1, 64, 0),
        3: (1, 'k_rollout_pipe', 1, 64, -4),
        4: (1, 'k_rollout_tmpl', 1, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 1, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "dense": {
        0: (0, 'k_rollout_lds', 0, 0, 0),
        2: (0, 'k_rollout_lds', 0, 0, 0),
        3: (0, 'k_rollout_lds', 0, 0, 0),
        4: (0, 'k_rollout_lds', 0, 0, 0),
        5: (0, 'k_rollout_lds', 0, 0, 0),
        6: (0, 'k_rollout_lds', 0, 0, 0),
    },
    "deepsea10_300_pipe0": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_lds', 1, 256, 0),
        3: (1, 'k_rollout_lds', 1, 256, -4),
        4: (1, 'k_rollout_tmpl', 2, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 2, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "deepsea10_300_pipe1": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 2, 64, 0),
        3: (1, 'k_rollout_pipe', 2, 64, -4),
        4: (1, 'k_rollout_tmpl', 2, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 2, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
    "deepsea10_300_g30": {
        0: (1, 'k_rollout_epi', 32, 128, 0),
        2: (1, 'k_rollout_pipe', 2, 64, 0),
        3: (1, 'k_rollout_pipe', 2, 64, -4),
        4: (1, 'k_rollout_tmpl', 30, 64, 0),
        5: (1, 'k_rollout_tmpl_stream', 30, 72, 0),
        6: (1, 'k_rollout_epi', 32, 128, 0),
    },
}

EXPECTED_GROUPS_PER_CU = {0: (True, 'k_rollout_lds', 8, 256), 1: (True, 'k_rollout_lds', 16, 256), 2: (True, 'k_rollout_lds', 8, 256)}


def observe_all():
    res = {n: observe(n) for n in NAMES}
    res.update({k: observe(n, e) for k, (n, e) in ENV_CASES.items()})
    return res


@pytest.mark.parametrize("name", NAMES + list(ENV_CASES))
def test_rollout_plan(need_gpu, name):
    n, e = ENV_CASES.get(name, (name, None))
    assert observe(n, e) == EXPECTED[name]


def test_lds_groups_per_cu(need_gpu):
    assert groups_per_cu() == EXPECTED_GROUPS_PER_CU
