"""Sharded benchmark runner (BASELINE config C4).

The reference enumerates (seed x MDP gin scope x agent gin scope) experiment instances, runs each in its own OS process
(colosseum/experiment/experiment_instances.py:117-223) and meets the results on the filesystem as one CSV per instance
(`<folder>/logs/<mdp_scope>-<MDP>____<agent_scope>-<Agent>/seed<n>_logs.csv`, header = sorted indicator names,
colosseum/utils/acme/csv_logger.py:99, colosseum/experiment/experiment_instance.py:53-82).

Here the same enumeration (seed-major, folder_structuring.py:76-104) is block-partitioned over the ranks (one process per
GPU, `colosseum_amd.sharding`), each rank groups its instances into device batches (same class, horizon and action
count), runs them with agents on the device (`colosseum_amd.agents`, `experiment.batched_loop`) and writes the same CSV
files.  The only communication is the final gather of one summary vector per instance.

Gin files of the benchmark folders only contain `prms_<i>/<Class>.<param> = <literal>` lines; they are parsed with a
regular expression (no gin dependency)."""
import ast
import csv
import os
import re
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _lib as L
from .agents import (BatchedPSRLContinuous, BatchedPSRLContinuousOptimistic, BatchedPSRLEpisodic, BatchedQLearningContinuous,
                     BatchedQLearningEpisodic, BatchedUCRL2Continuous)
from .batched import BatchedMDP
from .experiment.batched_loop import BatchedContinuousLoop, BatchedEpisodicLoop
from .mdp import make_model
from .sharding import shard_range

_GIN_LINE = re.compile(r"^\s*(prms_\d+)/(\w+)\.(\w+)\s*=\s*(.+?)\s*$")

# tuned hyper-parameters shipped with the reference (benchmark/cached_hyperparameters/agent_configs/*.gin)
DEFAULT_AGENT_CONFIGS = {
    "QLearningEpisodic": dict(p=0.05, UCB_type="bernstein", c_1=0.9415278732894797, c_2=0.013873778519317169,
                              min_at=0.07263563483119442),
    "QLearningContinuous": dict(h_weight=0.942, span_approx_weight=0.014, min_at=0.073),
    "PSRLEpisodic": dict(reward_prior_model="N_NIG", transitions_prior_model="M_DIR",
                         rewards_prior_prms=[0.41854463543357456, 1, 1, 1], transitions_prior_prms=[0.32345772625210756]),
    "UCRL2Continuous": dict(bound_type_p="bernstein", alpha_p=0.9883750006754203, alpha_r=0.10294276593728004),
    "PSRLContinuous": dict(reward_prior_model="N_NIG", rewards_prior_prms=[0.23589883401606418, 1, 1, 1],
                           psi_weight=0.016737988780906453, omega_weight=0.1104641036501887, kappa_weight=2.694052439968039,
                           eta_weight=1.3826913305347895e-07),
}


def samples_plainly(n_states: int, n_actions: int) -> bool:
    """Where the reference's PSRLContinuous drops optimistic sampling by itself (posterior_sampling.py:272-275)."""
    return int(n_states) ** 2 * int(n_actions) > 6_000_000


def make_psrl_continuous(env, seeds, optimization_horizon, **kw):
    """The reference's `PSRLContinuous` for a device batch, deciding as its constructor does: `BatchedPSRLContinuous` (plain
    sampling) when `no_optimistic_sampling` is set or every instance has S^2 * A > 6 000 000,
    `BatchedPSRLContinuousOptimistic` when no instance does, ValueError on a batch that mixes the two.  Three keys are not
    constructor keywords and are applied to the new agent: `min_steps_before_new_episode` (default 0), `sample_solver`
    (default "compact") and `policy_solver` (default "tables").  The defaults are the two table-form routes because neither
    T_ext [S, A * psi, S] nor the dense MAP workspace [S, A, S] of a whole batch fits at benchmark sizes; their Q carry the
    same rounding bounds against the reference as the dense routes'.  `DEFAULT_AGENT_CONFIGS["PSRLContinuous"]` holds the
    reference's tuned values for it.  It is not an entry of `DEVICE_AGENTS` yet: the enumeration's tests pin "PSRLContinuous"
    as a name `enumerate_instances` does not know, so `tools/run_benchmark.py --agents` does not offer it."""
    kw = dict(kw)
    min_steps = kw.pop("min_steps_before_new_episode", 0)
    sample_solver = kw.pop("sample_solver", "compact")
    policy_solver = kw.pop("policy_solver", "tables")
    large = [samples_plainly(S, env.A) for S in env.n_states]
    if kw.get("no_optimistic_sampling", False) or all(large):
        kw["no_optimistic_sampling"] = True
        agent = BatchedPSRLContinuous(env, seeds, optimization_horizon, **kw)
    elif any(large):
        raise ValueError("a device batch mixes instances with S^2 * A above and below 6 000 000: the reference samples the "
                         "former plainly and the latter optimistically, which are two agent classes here")
    else:
        agent = BatchedPSRLContinuousOptimistic(env, seeds, optimization_horizon, sample_solver=sample_solver, **kw)
    agent.set_policy_solver(policy_solver)
    if min_steps:
        agent.set_min_steps_before_new_episode(min_steps)
    return agent


# the agents built on the device: class name -> (episodic, agent class, loop class)
DEVICE_AGENTS = {
    "QLearningEpisodic": (True, BatchedQLearningEpisodic, BatchedEpisodicLoop),
    "PSRLEpisodic": (True, BatchedPSRLEpisodic, BatchedEpisodicLoop),
    "QLearningContinuous": (False, BatchedQLearningContinuous, BatchedContinuousLoop),
    "UCRL2Continuous": (False, BatchedUCRL2Continuous, BatchedContinuousLoop),
}
# ... of which these park their instances for a solve: their walk kernels do not park for reward blocks as well, so they
# refuse CMDP_FLAG_REWARD_CACHE handles (the reference's own Beta-reward caches)
_NO_REWARD_CACHE = ("PSRLEpisodic", "UCRL2Continuous")


def parse_gin(text: str) -> Dict[str, Dict[str, Dict[str, Any]]]:
    """{class: {scope: {param: value}}} from `prms_0/DeepSeaEpisodic.size=10` lines."""
    out: Dict[str, Dict[str, Dict[str, Any]]] = {}
    for line in text.splitlines():
        m = _GIN_LINE.match(line)
        if not m:
            continue
        scope, cls, key, val = m.groups()
        out.setdefault(cls, {}).setdefault(scope, {})[key] = ast.literal_eval(val)
    return out


def load_mdp_configs(folder: str) -> Dict[str, Dict[str, Dict[str, Any]]]:
    """All `mdp_configs/*.gin` of a benchmark folder laid out like the reference's."""
    cfg: Dict[str, Dict[str, Dict[str, Any]]] = {}
    d = os.path.join(folder, "mdp_configs")
    for f in sorted(os.listdir(d)):
        if f.endswith(".gin"):
            for cls, scopes in parse_gin(open(os.path.join(d, f)).read()).items():
                cfg.setdefault(cls, {}).update(scopes)
    return cfg


@dataclass
class Instance:
    seed: int
    mdp_cls: str
    mdp_scope: str
    mdp_kwargs: Dict[str, Any]
    agent_cls: str
    agent_scope: str = "prms_0"

    @property
    def label(self) -> str:  # ExperimentInstance.experiment_label
        return f"{self.mdp_scope}-{self.mdp_cls}____{self.agent_scope}-{self.agent_cls}"


def enumerate_instances(mdp_configs: Dict[str, Dict[str, Dict[str, Any]]], n_seeds: int,
                        supported_only: bool = True, agents: Optional[Sequence[str]] = None) -> List[Instance]:
    """Seed-major enumeration of folder_structuring.py:76-104: seed, then MDP class and scope, then agent.  `agents`: class
    names of `DEVICE_AGENTS`, each with its one scope `prms_0`; an agent of the other setting than the MDP class is skipped
    for it.  None: one tabular Q-learning agent per setting."""
    from .mdp.registry import FAMILIES

    if agents is None:
        agents = ("QLearningEpisodic", "QLearningContinuous")
    for a in agents:
        if a not in DEVICE_AGENTS:
            raise KeyError(f"agent {a!r}: one of {sorted(DEVICE_AGENTS)}")
    out = []
    for seed in range(n_seeds):
        for cls, scopes in mdp_configs.items():
            fam = cls.replace("Episodic", "").replace("Continuous", "")
            if fam not in FAMILIES:
                if supported_only:
                    continue
                raise KeyError(cls)
            matching = [a for a in agents if DEVICE_AGENTS[a][0] == cls.endswith("Episodic")]
            for scope in sorted(scopes, key=lambda s: int(s.split("_")[1])):
                for agent in matching:
                    out.append(Instance(seed, cls, scope, dict(scopes[scope]), agent))
    return out


def _build_one(ins: Instance):
    m = make_model(ins.mdp_cls, seed=ins.seed, **ins.mdp_kwargs)
    m.csr()             # the DP views every batch needs, computed where the model is built (a pool of processes), not under
    m.reward_matrix()   # the GIL of the threads that drive the device batches; they travel with the model (small arrays)
    return m


def _build_models(instances: Sequence[Instance], workers: int):
    """Host-side graph construction (Python) for many instances; a fork()ed pool must be used BEFORE the HIP runtime is
    initialised in this process, so `workers > 0` is only honoured then (the caller's responsibility)."""
    if workers and workers > 1 and len(instances) >= 4 * workers:
        import multiprocessing as mp

        with mp.get_context("fork").Pool(workers) as pool:
            return pool.map(_build_one, instances, chunksize=max(1, len(instances) // (workers * 8)))
    return [_build_one(i) for i in instances]


def build_shard_models(instances: Sequence[Instance], rank: int = 0, world: int = 1, workers: int = 0,
                       skip: Optional[Sequence[int]] = None) -> Dict[int, Any]:
    """{global instance index: TabularModel} of this rank's contiguous shard (fork()ed pool: call it before anything
    initialises the HIP runtime or RCCL in this process)."""
    lo, hi = shard_range(len(instances), rank, world)
    skip = set(skip or ())
    mine = [i for i in range(lo, hi) if i not in skip]
    return dict(zip(mine, _build_models([instances[i] for i in mine], workers)))


def _run_group(models, seeds, agent_cls, agent_kwargs, n_steps, log_every, rng_mode, device, max_time=np.inf,
               beta_rewards="reference"):
    L.check(L.load().cmdp_set_device(device))
    env, agent, loop, exact, t0, t1 = _setup_group(models, seeds, agent_cls, agent_kwargs, n_steps, rng_mode, beta_rewards)
    rows = loop.run(n_steps, log_every, max_time)
    t2 = time.time()
    for b, table in enumerate(rows):  # what MDPLoop.run returns first: where the time limit froze training (-1: it did not)
        table.last_training_step = int(loop.last_training_step[b])
    if exact and rows:
        rows[0].reward_cache_stats = env.reward_cache_stats()
    agent.close()
    env.close()
    if rows:
        rows[0].phase_seconds = (t1 - t0, t2 - t1, time.time() - t2)   # tables + baselines + agent | the interaction | release
    return rows


def check_group(agent_cls: str, stochastic: bool, beta_rewards: str):
    """What a device batch refuses before any handle is created.  PSRL and UCRL2 cannot run on the reference's own
    Beta-reward caches; nothing falls back silently to another reward stream."""
    if agent_cls not in DEVICE_AGENTS:
        raise KeyError(f"agent {agent_cls!r}: one of {sorted(DEVICE_AGENTS)}")
    if stochastic and beta_rewards == "reference" and agent_cls in _NO_REWARD_CACHE:
        raise ValueError(f"{agent_cls} on MDPs with stochastic rewards: beta_rewards='reference' needs CMDP_FLAG_REWARD_CACHE "
                         f"handles, which this agent's kernels do not support -- run with --beta-rewards philox "
                         f"(beta_rewards='philox': Beta rewards sampled on the device, distribution-exact)")


def _setup_group(models, seeds, agent_cls, agent_kwargs, n_steps, rng_mode, beta_rewards):
    stochastic = any(not m.deterministic_rewards for m in models)
    check_group(agent_cls, stochastic, beta_rewards)
    # Beta rewards, "reference": the reference's own per-triple caches of 5000 samples from the MDP's numpy stream
    # (CMDP_FLAG_REWARD_CACHE: blocks in HBM, drawn by the library on the host whenever an instance needs one), next to
    # the reference's transition streams -- rows equal the reference's for that seed.  "philox": sampled on the device
    # from counter-based streams (distribution-exact throughput mode; no host work).
    exact = stochastic and beta_rewards == "reference"
    t0 = time.time()
    env = BatchedMDP(models, rng_mode=L.RNG_PHILOX if stochastic and not exact else rng_mode,
                     philox_keys=np.asarray(seeds, np.uint64) * np.uint64(0x9E3779B1) + np.uint64(17),
                     flags=L.FLAG_REWARD_CACHE if exact else (L.FLAG_BETA_GAMMAS if beta_rewards == "philox-gammas" else 0))
    _, make_agent, make_loop = DEVICE_AGENTS[agent_cls]
    kw = dict(agent_kwargs)
    if agent_cls == "PSRLEpisodic":  # the posterior is sampled where the rewards are
        kw.setdefault("sampler", "philox" if stochastic else "reference")
    agent = make_agent(env, seeds, optimization_horizon=n_steps, **kw)
    loop = make_loop(env, agent)
    return env, agent, loop, exact, t0, time.time()


def run_instances(instances: Sequence[Instance], n_steps: int, log_every: int, rank: int = 0, world: int = 1,
                  agent_configs: Optional[Dict[str, Dict[str, Any]]] = None, rng_mode: int = L.RNG_MT_COMPAT,
                  device: int = 0, max_concurrent_groups: int = 6, build_workers: int = 0, progress=None,
                  max_batch: int = 128, models: Optional[Dict[int, Any]] = None, max_time: float = np.inf,
                  skip: Optional[Sequence[int]] = None, beta_rewards: str = "reference", on_group_done=None):
    """Runs this rank's contiguous shard; returns {global instance index: logger rows}.  `models` = the shard's
    models from `build_shard_models` (a caller that must initialise RCCL between the fork()ed build and the first HIP
    call builds them itself).  `max_time`: the experiment's `max_interaction_time_s` (training of an instance is frozen
    once its batch has run that long, agent_mdp_interaction.py:160-177).  `skip`: global indices not to run -- instances
    whose log file already exists (`unfinished_instances`), as the reference's resume does.  `beta_rewards`: "reference"
    (default: the reference's reward caches and streams, rows equal the reference's) or "philox" (device-sampled Beta
    rewards, distribution-exact).  `on_group_done(indices, rows)` is called from the worker thread as soon as a device
    batch has finished (the runner writes that batch's log files then, so an interrupted run resumes from them)."""
    assert beta_rewards in ("reference", "philox", "philox-gammas")
    agent_configs = agent_configs or DEFAULT_AGENT_CONFIGS
    lo, hi = shard_range(len(instances), rank, world)
    skip = set(skip or ())
    mine = [i for i in range(lo, hi) if i not in skip]
    if models is None:
        models = build_shard_models(instances, rank, world, build_workers, skip)
    groups: Dict[tuple, List[int]] = {}
    from .hardness import _vi_rule

    for i in mine:
        m = models[i]
        # continuous baselines use discounted VI under the reference's own scheme rule, which depends on the instance's
        # size and density: one scheme per device batch
        scheme = 0 if m.is_episodic else _vi_rule(m.n_states, m.n_actions, len(m.csr()[1]))
        # deterministic- and Beta-reward instances never share a device batch: in "philox" mode the two run different
        # transition streams (MT_COMPAT / Philox), and what an instance produces must not depend on which other
        # instances the benchmark holds
        # ... nor do the instances of two agents
        groups.setdefault((instances[i].mdp_cls, m.H, m.n_actions, tuple(m.rewards_range), scheme, m.deterministic_rewards,
                           instances[i].agent_cls, instances[i].agent_scope), []).append(i)
    for idx in groups.values():  # refused for the whole run before the first handle is created
        check_group(instances[idx[0]].agent_cls, not models[idx[0]].deterministic_rewards, beta_rewards)
    results: Dict[int, list] = {}

    def work(idx):

        ins = instances[idx[0]]
        t0 = time.time()
        rows = _run_group([models[i] for i in idx], [instances[i].seed for i in idx], ins.agent_cls,
                          agent_configs[ins.agent_cls], n_steps, log_every, rng_mode, device, max_time, beta_rewards)
        if on_group_done:
            on_group_done(idx, rows)
        if progress:
            rcs = getattr(rows[0], "reward_cache_stats", None) if rows else None
            ph = getattr(rows[0], "phase_seconds", None) if rows else None
            progress(f"{ins.label}: {len(idx)} instances, S={models[idx[0]].n_states}, H={models[idx[0]].H}, "
                     f"{time.time() - t0:.1f} s" + (f" (set-up and baselines {ph[0]:.1f} s, interaction {ph[1]:.1f} s, release {ph[2]:.1f} s)" if ph else "")
                     + (f", reward blocks {rcs['fills']} in {rcs['rounds']} rounds, {rcs['round_ms'] / 1e3:.1f} s "
                                                    f"in rounds of which {rcs['fill_ms'] / 1e3:.1f} s drawing" if rcs else ""))
        return idx, rows

    # Device batches are small next to the GPU (20-220 instances: a handful of wavefronts in latency-bound kernels), so a
    # few of them are driven concurrently, one host thread and one HIP stream each; the C calls release the GIL.  This
    # only pays because the per-log host work is short (vector_tracker): with per-instance Python trackers the threads
    # convoyed on the GIL (every one of the ~6 short C calls per log waited a 5 ms switch interval) and ran 10-100x
    # slower than one after the other.  Largest batches first, so that the tail is short.
    # very large batches are split: their per-log kernels are latency-bound per instance, so two halves in flight on two
    # streams finish sooner than one batch (and the longest batch is what bounds the wall time)
    parts = []
    for idx in groups.values():
        n_parts = -(-len(idx) // max(1, max_batch))
        size = -(-len(idx) // n_parts)
        parts += [idx[i:i + size] for i in range(0, len(idx), size)]
    # longest first.  A batch's time is rows x (dependent kernel time per row), which hardly depends on the number of
    # instances: per row the episodic loop evaluates a policy over H x S (state, time) pairs, the continuous one solves a
    # chain of S states (measured on C4: ~1.5 s per 1 000 for either measure)
    def expected(idx):
        m = models[idx[0]]
        return (m.H * m.n_states if m.is_episodic else 6 * m.n_states) * (1.0 + len(idx) / 400.0)

    order = sorted(parts, key=lambda idx: -expected(idx))
    import sys

    old_interval = sys.getswitchinterval()
    sys.setswitchinterval(2e-4)
    try:
        with ThreadPoolExecutor(max_workers=max(1, max_concurrent_groups)) as pool:
            for idx, rows in pool.map(work, order):
                for i, r in zip(idx, rows):
                    results[i] = r
    finally:
        sys.setswitchinterval(old_interval)
    return results


def _write_atomic(path: str, text: str):
    """The log file appears complete or not at all: a run killed mid-write must not leave a truncated file that the
    resume (`unfinished_instances`) would take for a finished instance."""
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, "w", newline="") as f:
        f.write(text)
    os.replace(tmp, path)


def _write_slice(task):
    """Worker of `submit_group_logs` (runs in a spawned process): formats the CSV texts of a slice of one device batch
    and writes them, each file atomically, with the `time_exceeded.txt` ledger lines."""
    from .experiment.vector_tracker import _csv_texts_of_slice

    steps, cols, n, paths, last_steps = task
    for text, path, last in zip(_csv_texts_of_slice((steps, cols, n)), paths, last_steps):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        _write_atomic(path, text)
        if last != -1:  # the ledger run_experiment_instance appends to (experiment_instances.py:218-222)
            with open(os.path.join(os.path.dirname(path), "time_exceeded.txt"), "a") as f:
                f.write(f"last training step at ({last}) for {path}\n")
    return len(paths)


def submit_group_logs(pool, folder: str, instances: Sequence[Instance], idx: Sequence[int], rows, chunk: int = 8):
    """Hands the log files of ONE finished device batch to `pool` (a concurrent.futures executor of spawned processes:
    the float -> text conversion is Python-level work that must not hold the GIL of the threads driving the other
    batches).  Returns the futures.  Files are written as their batch finishes, so an interrupted benchmark resumes from
    what is on disk (the reference writes every instance's file at its own end, experiment_instance.py:53-82)."""
    log = rows[0].log
    fin = log.finalize()
    futs = []
    for b0 in range(0, len(idx), chunk):
        b1 = min(len(idx), b0 + chunk)
        bs = [rows[j].b for j in range(b0, b1)]
        assert bs == list(range(bs[0], bs[0] + len(bs)))
        cols = {n: (v[:, bs[0]:bs[-1] + 1], k if isinstance(k, int) else k[:, bs[0]:bs[-1] + 1]) for n, (v, k) in fin.items()}
        paths = [log_file(folder, instances[idx[j]]) for j in range(b0, b1)]
        lasts = [int(getattr(rows[j], "last_training_step", -1)) for j in range(b0, b1)]
        futs.append(pool.submit(_write_slice, (list(log.steps), cols, b1 - b0, paths, lasts)))
    return futs


def write_csv_logs(folder: str, instances: Sequence[Instance], results: Dict[int, list], workers: int = 0):
    """The reference's on-disk wire format (CSVLogger with add_uid=False; header = sorted keys).  `workers` > 1
    formats the column stores of the device batches in a process pool.  Every file is written atomically."""
    from .experiment.vector_tracker import LogTable, csv_texts_parallel

    logs = {}
    for rows in results.values():
        if isinstance(rows, LogTable):
            logs.setdefault(id(rows.log), rows.log)
    texts = csv_texts_parallel(list(logs.values()), workers) if logs else {}
    for i, rows in results.items():
        ins = instances[i]
        d = os.path.join(folder, "logs", ins.label)
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"seed{ins.seed}_logs.csv")
        if isinstance(rows, LogTable):
            _write_atomic(path, texts[id(rows.log)][rows.b])
        else:
            import io

            buf = io.StringIO(newline="")
            fields = sorted(rows[0].keys())
            w = csv.DictWriter(buf, fieldnames=fields, extrasaction="ignore")
            w.writeheader()
            for r in rows:
                w.writerow({k: np.array(v) for k, v in r.items()})
            _write_atomic(path, buf.getvalue())
        last = getattr(rows, "last_training_step", -1)
        if last != -1:  # the ledger run_experiment_instance appends to (experiment_instances.py:218-222)
            with open(os.path.join(d, "time_exceeded.txt"), "a") as f:
                f.write(f"last training step at ({last}) for {os.path.join(d, f'seed{ins.seed}_logs.csv')}\n")


def log_file(folder: str, ins: Instance) -> str:
    """ExperimentInstance's log file (experiment_instance.py:67-82)."""
    return os.path.join(folder, "logs", ins.label, f"seed{ins.seed}_logs.csv")


def unfinished_instances(folder: str, instances: Sequence[Instance]) -> List[int]:
    """Indices of the instances whose log file does not exist yet: the reference only (re-)creates those
    (`does_log_file_exists`, folder_structuring.py:102), which is how an interrupted benchmark resumes."""
    return [i for i, ins in enumerate(instances) if not os.path.exists(log_file(folder, ins))]


def read_summary(folder: str, ins: Instance) -> np.ndarray:
    """`summary_vector` of an instance from its log file (instances skipped by a resumed run)."""
    with open(log_file(folder, ins), newline="") as f:
        last = list(csv.DictReader(f))[-1]
    return np.array([float(last["steps"]), float(last["normalized_cumulative_regret"]), float(last["cumulative_reward"])])


def summary_vector(rows) -> np.ndarray:
    """What is gathered across ranks at the end: last step, normalized cumulative regret, cumulative reward."""
    last = rows[-1]
    return np.array([last["steps"], last["normalized_cumulative_regret"], last["cumulative_reward"]], np.float64)
