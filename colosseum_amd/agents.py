"""Agents that run on the device next to their environments.

`BatchedQLearningEpisodic` = one reference `QLearningEpisodic` agent (colosseum/agent/agents/episodic/q_learning.py)
per instance of a `BatchedMDP`, advanced by a kernel that fuses select_action -> step -> step_update; Q tables and action
streams are bit-equal to the reference agent driven by the reference's MDPLoop (golden G7)."""
import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from .batched import BatchedMDP


class _DeviceAgent:
    """A handle of the library's: `_PREFIX` names the agent's C functions (`<_PREFIX>_destroy` frees it)."""

    _PREFIX = None

    def _create(self, env, seeds, *args, create="_create"):
        """Loads the library, takes one seed per instance, creates the handle with `<_PREFIX><create>(&h, env, seeds, *args)`
        and ties it to the environment's."""
        self._lib = L.load()
        self.env = env
        seeds = np.ascontiguousarray(seeds, np.int32)
        assert len(seeds) == env.B
        self._h = C.c_void_p()
        L.check(getattr(self._lib, self._PREFIX + create)(C.byref(self._h), env._h, L.ptr(seeds), *args))
        env._register_agent(self)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._lib, self._PREFIX + "_destroy")(self._h)
            self._h = C.c_void_p()

    def run_logged(self, desc, n_logs: int):
        """`MDPLoop.run` for the whole batch in one library call (cmdp_qlearning_run_logged, cmdp_ucrl2_run_logged,
        cmdp_psrl_run_logged): interaction, policy evaluation at every logging step and the reference's indicators, all
        without returning to Python; the agents that park their instances take the rows strictly in order and must not have
        taken a step yet.  `desc` from `vector_tracker.loop_desc`.  Returns (steps [n_logs], values, kinds [n_logs, 17, B],
        last_training_step, is_training)."""
        return self._run_logged_native(desc, n_logs)

    def _run_logged_native(self, desc, n_logs: int):
        """`<_PREFIX>_run_logged`: what `run_logged` returns, and what the batched loops call."""
        B = self.env.B
        steps = np.zeros(n_logs, np.int64)
        values = np.zeros((n_logs, len(L.LOG_COLUMNS), B), np.float64)
        kinds = np.zeros((n_logs, len(L.LOG_COLUMNS), B), np.uint8)
        last = np.zeros(B, np.int64)
        training = np.zeros(B, np.uint8)
        L.check(getattr(self._lib, self._PREFIX + "_run_logged")(self._h, C.byref(desc), int(n_logs), L.ptr(steps), L.ptr(values),
                                                                 L.ptr(kinds), L.ptr(last), L.ptr(training)))
        return steps, values, kinds, last, training.astype(bool)

    def _sa(self, x):
        """A per-row array of the library's -> list of [S, A] per instance."""
        return [y.reshape(-1, self.env.A) for y in self.env.split_rows(x)]

    def _mask(self, mask):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        assert m is None or m.shape == (self.env.B,)
        return m, (range(self.env.B) if m is None else np.flatnonzero(m))

    def _average_reward(self, mask):
        m, sel = self._mask(mask)
        avg, kind = np.zeros(self.env.B, np.float64), np.zeros(self.env.B, np.int32)
        L.check(getattr(self._lib, self._PREFIX + "_average_reward")(self._h, L.ptr(m), L.ptr(avg), L.ptr(kind)))
        return [np.float32(avg[b]) if kind[b] else np.float64(avg[b]) for b in sel]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchedQLearningEpisodic(_DeviceAgent):
    _PREFIX = "cmdp_qlearning"

    def __init__(self, env: BatchedMDP, seeds: Sequence[int], optimization_horizon: int, p: float, c_1: float,
                 c_2: Optional[float] = None, min_at: float = 0.0, UCB_type: str = "hoeffding"):
        ucb = {"hoeffding": 0, "bernstein": 1}[UCB_type.lower()]
        self._create(env, seeds, int(optimization_horizon), float(p), float(c_1), float(c_2 or 0.0), float(min_at), ucb)

    def run(self, n_steps: int, train=True, trace_actions: bool = False):
        """n_steps of select_action -> step -> step_update per instance.  `train`: bool or per-instance mask.
        Returns the running cumulative reward (since creation) and, optionally, the actions [n_steps, B]."""
        n_steps = int(n_steps)
        acts = np.zeros((n_steps, self.env.B), np.int8) if trace_actions else None
        rsum = np.zeros(self.env.B, np.float64)
        mask = None
        if train is not True:
            mask = np.ascontiguousarray(np.broadcast_to(np.asarray(train, bool), (self.env.B,)), np.uint8)
        L.check(self._lib.cmdp_qlearning_run(self._h, n_steps, L.ptr(mask), L.ptr(acts), L.ptr(rsum)))
        return dict(cumulative_reward=rsum, actions=acts)

    def evaluate(self) -> np.ndarray:
        """V[0, :] (concatenated over instances) of the current greedy policies, policy and evaluation on device."""
        V0 = np.zeros(int(self.env.state_off[-1]), np.float32)
        L.check(self._lib.cmdp_qlearning_evaluate(self._h, L.ptr(V0)))
        return V0

    def tables(self):
        """(Q, N): per instance arrays of shape [H, S_b, A]."""
        env = self.env
        n = int(env.H * env.row_off[-1])
        Q = np.zeros(n, np.float32)
        N = np.zeros(n, np.int32)
        L.check(self._lib.cmdp_qlearning_tables(self._h, L.ptr(Q), L.ptr(N)))
        qs = [x.reshape(env.H, -1, env.A) for x in env.split_rows(Q, env.H)]
        ns = [x.reshape(env.H, -1, env.A) for x in env.split_rows(N, env.H)]
        return qs, ns


class BatchedQLearningContinuous(BatchedQLearningEpisodic):
    """One reference `QLearningContinuous` (colosseum/agent/agents/infinite_horizon/q_learning.py) per instance."""

    def __init__(self, env: BatchedMDP, seeds: Sequence[int], optimization_horizon: int, min_at: float = 0.0,
                 confidence: float = 0.95, span_approx_weight: float = 1.0, h_weight: float = 1.0):
        self._create(env, seeds, int(optimization_horizon), float(min_at), float(confidence), float(span_approx_weight),
                     float(h_weight), create="_continuous_create")

    def tables(self):
        env = self.env
        Q = np.zeros(int(env.row_off[-1]), np.float64)  # float64 tables (NEP 50: float32 zeros + numpy float64 H)
        N = np.zeros(int(env.row_off[-1]), np.int32)
        L.check(self._lib.cmdp_qlearning_tables(self._h, L.ptr(Q), L.ptr(N)))
        return self._sa(Q), self._sa(N)

    def evaluate(self):
        raise NotImplementedError("use policy(): continuous regrets come from the stationary distribution")

    def average_reward(self, mask=None) -> list:
        """`get_average_reward` of the current greedy policies from the current states, on the device (kernel K9): a
        list of numpy scalars (np.float32 where the reference's value is one) for the instances selected by `mask`."""
        return self._average_reward(mask)

    def policy(self):
        """argmax_2d greedy policies (RandomState(42) tie-break), per instance [S, A]."""
        pi = np.zeros(int(self.env.row_off[-1]), np.float32)
        L.check(self._lib.cmdp_qlearning_policy(self._h, L.ptr(pi)))
        return self._sa(pi)


class _ParkAndSolveAgent(_DeviceAgent):
    """What the agents that park their instances for a solve share (csrc: ParkAgent): the layout of the model's tables (per
    row the distinct successors), run(), stats().  `_STATS` names the agent's counters."""

    _STATS = ()

    def _fetch_layout(self):
        layout = getattr(self._lib, self._PREFIX + "_layout")
        nz = C.c_int64()
        L.check(layout(self._h, C.byref(nz), None, None))
        self._nz = int(nz.value)
        self._ptr = np.zeros(int(self.env.row_off[-1]) + 1, np.int64)
        self._col = np.zeros(self._nz, np.int32)
        L.check(layout(self._h, None, L.ptr(self._ptr), L.ptr(self._col)))
        # dense position of every layout entry inside its instance's [S * A, S] array
        self._rows = np.repeat(np.arange(len(self._ptr) - 1), np.diff(self._ptr))

    def _run(self, n_steps, train, trace, stop_at_episode_end):
        n_steps, B = int(n_steps), self.env.B
        acts = np.zeros((n_steps, B), np.int8) if trace else None
        obs = np.zeros((n_steps, B), np.int32) if trace else None
        rew = np.zeros((n_steps, B), np.float64) if trace else None
        rsum = np.zeros(B, np.float64)
        taken = np.zeros(B, np.int64)
        mask = None
        if train is not True:
            mask = np.ascontiguousarray(np.broadcast_to(np.asarray(train, bool), (B,)), np.uint8)
        L.check(getattr(self._lib, self._PREFIX + "_run")(self._h, n_steps, int(bool(stop_at_episode_end)), L.ptr(mask),
                                                          L.ptr(acts), L.ptr(obs), L.ptr(rew), L.ptr(rsum), L.ptr(taken)))
        return dict(cumulative_reward=rsum, steps_taken=taken, actions=acts, observations=obs, rewards=rew)

    def _dense(self, values, dtype, fill=None, uniform=None):
        """Layout values as dense [S, A, S] arrays per instance; elsewhere `fill[b]` (default 0), and rows with
        `uniform` > 0 hold that value at every state."""
        env, out = self.env, []
        for b in range(env.B):
            S = int(env.n_states[b])
            r0, r1 = int(env.row_off[b]), int(env.row_off[b + 1])
            z0, z1 = int(self._ptr[r0]), int(self._ptr[r1])
            M = np.full((r1 - r0, S), 0 if fill is None else fill[b], dtype)
            M[self._rows[z0:z1] - r0, self._col[z0:z1]] = values[z0:z1]
            if uniform is not None:
                u = uniform[r0:r1]
                M[u > 0] = u[u > 0, None]
            out.append(M.reshape(S, env.A, S))
        return out

    def _stats(self) -> dict:
        v, out = C.c_double(), {}
        for k, w in self._STATS:
            L.check(self._lib.cmdp_stat(self.env._h, w, C.byref(v)))
            out[k] = float(v.value) if k.endswith("_ms") else int(v.value)
        return out


class _ContinuousModelPolicy:
    """`policy()`, `policy_solve()` and `average_reward()` of the continuous agents that solve a model for their greedy policy:
    UCRL2 its estimated model (ucrl2.py:80-83, kernel K14), PSRL the MAP estimate of its posterior
    (infinite_horizon/posterior_sampling.py:174-178, by the route of `policy_solver`).  Touch nothing the agent acts or
    learns with."""

    def policy(self, mask=None):
        """argmax_2d (RandomState(42) tie-break) of discounted value iteration on the agent's model, on the device, per
        instance [S, A]; with `mask`, for the selected instances only, in their order."""
        m, sel = self._mask(mask)
        pi = np.zeros(int(self.env.row_off[-1]), np.float32)
        L.check(getattr(self._lib, self._PREFIX + "_policy")(self._h, L.ptr(m), L.ptr(pi), None, None, None))
        rows = self._sa(pi)
        return [rows[b] for b in sel]

    def policy_solve(self, mask=None):
        """The solve behind `policy()`: `Q` per instance [S, A] float32, `sweeps` and `scheme` (L.SCHEME_JACOBI /
        L.SCHEME_GAUSS_SEIDEL, the reference's rule on the model) [B]; with `mask`, zeros elsewhere."""
        m, _ = self._mask(mask)
        Q = np.zeros(int(self.env.row_off[-1]), np.float32)
        sweeps, scheme = np.zeros(self.env.B, np.int64), np.zeros(self.env.B, np.int32)
        L.check(getattr(self._lib, self._PREFIX + "_policy")(self._h, L.ptr(m), None, L.ptr(Q), L.ptr(sweeps), L.ptr(scheme)))
        return dict(Q=self._sa(Q), sweeps=sweeps, scheme=scheme)

    def average_reward(self, mask=None) -> list:
        """`get_average_reward` of `policy()` from the environments' current states, on the device (the solve, then kernel
        K9): a list of numpy scalars (np.float32 where the reference's value is one) for the instances selected by `mask`."""
        return self._average_reward(mask)


class BatchedUCRL2Continuous(_ContinuousModelPolicy, _ParkAndSolveAgent):
    """One reference `UCRL2Continuous` (colosseum/agent/agents/infinite_horizon/ucrl2.py) per instance of a continuous
    `BatchedMDP`, driven as `MDPLoop.run` drives it: interaction, counts, confidence bounds, the estimated model and the
    optimistic solves (extended value iteration, kernel K10) stay on the device (kernel K11, csrc/cmdp_ucrl2.h).  The
    keyword names and defaults are the reference's.  `bound_type_rew="bernstein"` is refused: the reference raises
    AttributeError there at its first solve."""

    _PREFIX = "cmdp_ucrl2"
    _STATS = (("rounds", L.STAT_UCRL2_ROUNDS), ("solves", L.STAT_UCRL2_SOLVES), ("unconverged", L.STAT_UCRL2_UNCONVERGED),
              ("round_ms", L.STAT_UCRL2_ROUND_MS), ("wait_ms", L.STAT_UCRL2_WAIT_MS),
              ("policy_kernel_ms", L.STAT_UCRL2_POLICY_KERNEL_MS), ("policy_solved", L.STAT_UCRL2_POLICY_SOLVED),
              ("policy_reused", L.STAT_UCRL2_POLICY_REUSED))
    _BOUNDS = {"_chernoff": L.BOUND_CHERNOFF, "bernstein": L.BOUND_BERNSTEIN}

    def __init__(self, env: BatchedMDP, seeds: Sequence[int], optimization_horizon: int, alpha_r=1.0, alpha_p=1.0,
                 bound_type_p="_chernoff", bound_type_rew="_chernoff", epsilon_greedy=None, boltzmann_temperature=None):
        assert bound_type_p in self._BOUNDS and bound_type_rew in self._BOUNDS  # ucrl2.py:130-131
        actor = L.ACTOR_GREEDY
        if epsilon_greedy is not None:
            actor = L.ACTOR_EPSILON_GREEDY
        elif boltzmann_temperature is not None:
            actor = L.ACTOR_BOLTZMANN
        self._create(env, seeds, int(optimization_horizon), float(alpha_r), float(alpha_p), self._BOUNDS[bound_type_p],
                     self._BOUNDS[bound_type_rew], actor)
        self._fetch_layout()

    def run(self, n_steps: int, train=True, trace: bool = False, stop_at_episode_end: bool = False):
        """n_steps of select_action -> step -> step_update -> (episode_end_update) per instance; with
        `stop_at_episode_end` every instance stops after its next episode_end_update.  Returns `cumulative_reward` (since
        creation), `steps_taken` [B] and, with `trace`, `actions`, `observations` (after the step) and float64 `rewards`,
        each [n_steps, B] with row t of instance b valid for t < steps_taken[b]."""
        return self._run(n_steps, train, trace, stop_at_episode_end)

    def model(self):
        """Per instance the reference agent's tables: dense `N` [S, A, S] int32 and `P` float32, `estimated_rewards`,
        `variance_proxy_reward`, `estimated_holding_times` [S, A] float32, `iteration`, `episode`, `delta`."""
        env = self.env
        R = int(env.row_off[-1])
        N, P = np.zeros(self._nz, np.int32), np.zeros(self._nz, np.float32)
        uni, er, vr, ht = (np.zeros(R, np.float32) for _ in range(4))
        it, ep, delta = np.zeros(env.B, np.int64), np.zeros(env.B, np.int64), np.zeros(env.B, np.float64)
        L.check(self._lib.cmdp_ucrl2_model(self._h, L.ptr(N), L.ptr(P), L.ptr(uni), L.ptr(er), L.ptr(vr), L.ptr(ht), L.ptr(it),
                                           L.ptr(ep), L.ptr(delta)))
        sa = self._sa
        return dict(N=self._dense(N, np.int32), P=self._dense(P, np.float32, uniform=uni), estimated_rewards=sa(er),
                    variance_proxy_reward=sa(vr), estimated_holding_times=sa(ht), iteration=it, episode=ep, delta=delta)

    def last_solve(self):
        """The last optimistic solve of every instance: its inputs `P` [S, A, S], `estimated_rewards`, `beta_r`, `beta_p0`
        (element 0 of beta_p[s, a]) [S, A] and the `Q` [S, A] / `span` the actor holds (those of the last solve that
        converged), `sweeps` and `status` of the last solve."""
        env = self.env
        R = int(env.row_off[-1])
        P, uni, er, Q = np.zeros(self._nz, np.float32), np.zeros(R, np.float32), np.zeros(R, np.float32), np.zeros(R, np.float32)
        br, bp = np.zeros(R, np.float64), np.zeros(R, np.float64)
        span, sweeps, status = np.zeros(env.B, np.float64), np.zeros(env.B, np.int64), np.zeros(env.B, np.int32)
        L.check(self._lib.cmdp_ucrl2_last_solve(self._h, L.ptr(P), L.ptr(uni), L.ptr(er), L.ptr(br), L.ptr(bp), L.ptr(Q),
                                                L.ptr(span), L.ptr(sweeps), L.ptr(status)))
        sa = self._sa
        return dict(P=self._dense(P, np.float32, uniform=uni), estimated_rewards=sa(er), beta_r=sa(br), beta_p0=sa(bp), Q=sa(Q),
                    span=span, sweeps=sweeps, status=status)

    def current_optimal_stochastic_policy(self):
        """ucrl2.py:80-83 per instance: `policy()`."""
        return self.policy()

    def stats(self) -> dict:
        """Rounds of parked instances, instances solved in them, solves that did not converge, host time of the rounds
        (park list, logarithms, enqueue) and time spent waiting for the device in them; `policy_solved` / `policy_reused`:
        instances the policy solve (K14) has run for, and instances that kept their stored policy because their estimated
        model had not changed.  Kept per ENVIRONMENT handle: agents created on the same environment share these counters."""
        return self._stats()

    def _set_policy_size_threshold(self, n: int):
        """Test hook: the size threshold of the scheme rule in the policy solve (the reference's default 300 * 3 * 300)."""
        L.check(self._lib.cmdp_ucrl2_set_option(self._h, L.UCRL2_OPT_POLICY_SIZE_THRESHOLD, int(n)))

    def _set_policy_reuse(self, on: bool):
        """Whether an instance whose `episode` has not moved keeps the policy of its last solve (default) or every
        `policy()` / `average_reward()` / logged row solves again.  The results are identical either way."""
        L.check(self._lib.cmdp_ucrl2_set_option(self._h, L.UCRL2_OPT_POLICY_REUSE, int(bool(on))))

    def _set_max_sweeps(self, n: int):
        """Test hook: the sweeps a solve may take (the not-converged path keeps the previous Q)."""
        L.check(self._lib.cmdp_ucrl2_set_option(self._h, L.UCRL2_OPT_MAX_SWEEPS, int(n)))


class _PosteriorSamplingAgent(_ParkAndSolveAgent):
    """What the two PSRL agents share: the BayesianMDPModel's priors as the library takes them (one N_NIG parameter list and
    one M_DIR prior per instance), the samplers, episode_end_update() and the MAP estimate."""

    _STATS = (("rounds", L.STAT_PSRL_ROUNDS), ("solves", L.STAT_PSRL_SOLVES), ("sample_kernel_ms", L.STAT_PSRL_SAMPLE_KERNEL_MS),
              ("vi_kernel_ms", L.STAT_PSRL_VI_KERNEL_MS), ("reference_ms", L.STAT_PSRL_REFERENCE_MS),
              ("policy_kernel_ms", L.STAT_PSRL_POLICY_KERNEL_MS))
    _SAMPLERS = {"reference": L.PSRL_SAMPLER_REFERENCE, "philox": L.PSRL_SAMPLER_PHILOX}

    def __init__(self, env: BatchedMDP, seeds: Sequence[int], optimization_horizon: int, reward_prior_model=None,
                 transitions_prior_model=None, rewards_prior_prms=None, transitions_prior_prms=None, epsilon_greedy=None,
                 boltzmann_temperature=None, sampler="reference"):
        if sampler not in self._SAMPLERS:
            raise ValueError(f"sampler {sampler!r}: 'reference' or 'philox'")
        if epsilon_greedy is not None or boltzmann_temperature is not None:
            raise NotImplementedError("only the greedy actor is built: epsilon_greedy and boltzmann_temperature must be None")
        name = lambda m: getattr(m, "name", m)  # noqa: E731  (the reference passes enum members)
        if reward_prior_model is not None and name(reward_prior_model) != "N_NIG":
            raise NotImplementedError(f"reward_prior_model {name(reward_prior_model)!r}: only N_NIG is built")
        if transitions_prior_model is not None and name(transitions_prior_model) != "M_DIR":
            raise NotImplementedError(f"transitions_prior_model {name(transitions_prior_model)!r}: only M_DIR is built")
        # bayesian_model.py:48-53: a prior model left None takes the reference's default parameters too
        if reward_prior_model is None:
            rewards_prior_prms = None
        if transitions_prior_model is None:
            transitions_prior_prms = None
        for prms in (rewards_prior_prms, transitions_prior_prms):
            if prms is not None and (isinstance(prms, dict) or type(prms[0]) in (list, tuple, np.ndarray)):
                raise NotImplementedError("per-pair prior lists are not built: give one parameter list for all pairs")
        if rewards_prior_prms is None:
            rewards_prior_prms = [float(env.rewards_range[1]), 1, 1, 1]
        assert len(rewards_prior_prms) == 4 and (transitions_prior_prms is None or len(transitions_prior_prms) == 1)
        # base_conjugate.py:49 `np.tile(...).astype(np.float32)`, then N_NIG.__init__'s "interpretable parameters" transform
        # (conjugate_rewards.py:54-63) with its float32 scalars: (mu, n_mu, n_tau * 0.5, (0.5 * n_tau) / tau)
        mu, n_mu, tau, n_tau = np.tile(rewards_prior_prms, (1, 1, 1)).astype(np.float32)[0, 0]
        hp = np.zeros(4, np.float32)
        hp[:] = (mu, n_mu, n_tau * 0.5, (0.5 * n_tau) / tau)
        rprior = np.ascontiguousarray(np.tile(hp, (env.B, 1)), np.float32)
        if transitions_prior_prms is None:
            tprior = np.array([np.tile([1.0 / int(S)], (1, 1, 1)).astype(np.float32)[0, 0, 0] for S in env.n_states], np.float32)
        else:
            tprior = np.full(env.B, np.tile(transitions_prior_prms, (1, 1, 1)).astype(np.float32)[0, 0, 0], np.float32)
        self._create(env, seeds, int(optimization_horizon), L.ptr(rprior), L.ptr(tprior), self._SAMPLERS[sampler], L.ACTOR_GREEDY)
        self._fetch_layout()

    def _sample_T(self, fetch):
        """The last posterior sample's `T` per instance [S, A, S]: `fetch(T)` fills the library's dense, unpadded array."""
        env = self.env
        sizes = [int(S) * env.A * int(S) for S in env.n_states]
        T = np.zeros(sum(sizes), np.float32)
        fetch(T)
        return [x.reshape(int(S), env.A, int(S)) for x, S in zip(np.split(T, np.cumsum(sizes)[:-1]), env.n_states)]

    def episode_end_update(self):
        """The reference agent's `episode_end_update()` for every instance: a new posterior sample on the tables as they are,
        its solve and the new Q; no step is taken, the environment is not reset."""
        L.check(getattr(self._lib, self._PREFIX + "_episode_end_update")(self._h))

    def map_estimate(self):
        """BayesianMDPModel.get_map_estimate per instance: (hyper_params / hyper_params.sum(-1, keepdims=True),
        hyper_params[:, :, 0])."""
        m = self.model()
        return [(t / t.sum(-1, keepdims=True), r[:, :, 0]) for t, r in zip(m["transitions"], m["rewards"])]

    def current_optimal_stochastic_policy(self):
        """The reference agent's `current_optimal_stochastic_policy` per instance: `policy()`."""
        return self.policy()


class BatchedPSRLEpisodic(_PosteriorSamplingAgent):
    """One reference `PSRLEpisodic` (colosseum/agent/agents/episodic/posterior_sampling.py) per instance of an episodic
    `BatchedMDP`, driven as `MDPLoop.run` drives it: interaction, the N_NIG / M_DIR posterior tables, the posterior sample,
    the solve (k_vi_episodic_dense) and the actor's Q stay on the device (kernel K12, csrc/cmdp_psrl.h).  The keyword
    names and defaults are the reference's.  `sampler="reference"` draws the reference's own numbers (numpy's legacy
    samplers on the host, one RandomState(seed) per conjugate model); `sampler="philox"` draws on the device: the same
    distributions from a counter-based stream, a pure function of (seed, episode, tables).  Per-pair prior lists, the
    N_N reward model and the exploration actors are refused."""

    _PREFIX = "cmdp_psrl"

    def run(self, n_steps: int, train=True, trace: bool = False, stop_at_episode_end: bool = False):
        """n_steps of select_action -> step -> step_update -> (episode_end_update, reset) per instance; with
        `stop_at_episode_end` every instance stops after its next episode_end_update.  Returns `cumulative_reward` (since
        creation), `steps_taken` [B] and, with `trace`, `actions`, `observations` (after the step; -1 at an episode's last
        step) and float64 `rewards`, each [n_steps, B] with row t of instance b valid for t < steps_taken[b]."""
        return self._run(n_steps, train, trace, stop_at_episode_end)

    def model(self):
        """Per instance the reference model's tables: `transitions` dense [S, A, S] float32 (M_DIR.hyper_params) and
        `rewards` [S, A, 4] float32 (N_NIG.hyper_params); `episode` [B]: posterior samples drawn so far."""
        env = self.env
        R = int(env.row_off[-1])
        rp, tp = np.zeros(R * 4, np.float32), np.zeros(self._nz, np.float32)
        prior, ep = np.zeros(env.B, np.float32), np.zeros(env.B, np.int64)
        L.check(self._lib.cmdp_psrl_model(self._h, L.ptr(rp), L.ptr(tp), L.ptr(prior), L.ptr(ep)))
        trans = self._dense(tp, np.float32, fill=prior)
        rew = [x.reshape(-1, env.A, 4) for x in env.split_rows(rp.reshape(R, 4))]
        return dict(transitions=trans, rewards=rew, episode=ep)

    def last_sample(self):
        """The last posterior sample of every instance, `T` [S, A, S] and `R` [S, A] float32, and the `Q` [H + 1, S, A]
        the actor holds (solved on them)."""
        R = int(self.env.row_off[-1])
        Rs, Q = np.zeros(R, np.float32), np.zeros((int(self.env.H) + 1) * R, np.float32)
        Ts = self._sample_T(lambda T: L.check(self._lib.cmdp_psrl_last_sample(self._h, L.ptr(T), L.ptr(Rs), L.ptr(Q))))
        return dict(T=Ts, R=self._sa(Rs), Q=self._layers(Q))

    def _layers(self, x):
        """A per-instance [H + 1][S][A] array of the library's -> list of [H + 1, S, A]."""
        env, H = self.env, int(self.env.H)
        out = []
        for b in range(env.B):
            q0, n = (H + 1) * int(env.row_off[b]), (H + 1) * int(env.n_states[b]) * env.A
            out.append(x[q0:q0 + n].reshape(H + 1, -1, env.A))
        return out

    def policy(self, mask=None):
        """posterior_sampling.py:78-82 on the device: argmax_3d (RandomState(42) tie-break) of episodic value iteration on
        the MAP estimate of the model (kernel K15, no dense array), per instance [H + 1, S, A]; with `mask`, for the
        selected instances only, in their order.  Touches nothing the agent acts or learns with."""
        m, sel = self._mask(mask)
        pi = np.zeros((int(self.env.H) + 1) * int(self.env.row_off[-1]), np.float32)
        L.check(self._lib.cmdp_psrl_policy(self._h, L.ptr(m), L.ptr(pi), None))
        rows = self._layers(pi)
        return [rows[b] for b in sel]

    def policy_solve(self, mask=None):
        """The solve behind `policy()`: `Q` per instance [H + 1, S, A] float32; with `mask`, zeros elsewhere."""
        m, _ = self._mask(mask)
        Q = np.zeros((int(self.env.H) + 1) * int(self.env.row_off[-1]), np.float32)
        L.check(self._lib.cmdp_psrl_policy(self._h, L.ptr(m), None, L.ptr(Q)))
        return dict(Q=self._layers(Q))

    def evaluate(self, mask=None) -> np.ndarray:
        """V[0, :] (concatenated over instances) of `policy()` on the true MDP -- what the episodic regret needs -- solve,
        policy and evaluation on the device; with `mask`, zeros for the other instances."""
        m, _ = self._mask(mask)
        V0 = np.zeros(int(self.env.state_off[-1]), np.float32)
        L.check(self._lib.cmdp_psrl_evaluate(self._h, L.ptr(m), L.ptr(V0)))
        return V0

    def stats(self) -> dict:
        """Rounds of parked instances, instances solved in them, HIP-event times of the last round's sample and solve
        kernels, host time of the reference sampler's draws, HIP-event time of K15 in the last policy() / policy_solve() /
        evaluate().  Kept per ENVIRONMENT handle."""
        return self._stats()


class BatchedPSRLContinuous(_ContinuousModelPolicy, _PosteriorSamplingAgent):
    """One reference `PSRLContinuous` (colosseum/agent/agents/infinite_horizon/posterior_sampling.py) with PLAIN posterior
    sampling -- the reference's own `no_optimistic_sampling=True` path -- per instance of a continuous `BatchedMDP`, driven as
    `MDPLoop.run` drives it: interaction, the N_NIG / M_DIR posterior tables (K12's), the artificial-episode rule, the
    posterior sample, the solve (k_vi_discounted_dense: the reference's Jacobi / Gauss-Seidel rule per sample) and the actor's
    Q stay on the device (kernel K13, csrc/cmdp_psrlc.h).  `policy()` / `policy_solve()` / `average_reward()` solve the MAP
    model by one of two routes, `set_policy_solver("dense" | "tables")`.  The keyword names and defaults are the reference's; the four weights
    and `max_psi` only shape optimistic sampling and are accepted and unused, as on the reference's plain path.  Refused, each
    by name: optimistic sampling (`no_optimistic_sampling=False` unless every instance has S^2 * A > 6 000 000, where the
    reference switches by itself), `truncate_reward_with_max=True`, `min_steps_before_new_episode != 0` as a constructor
    keyword (`set_min_steps_before_new_episode(n)` on the new agent sets it), the exploration actors, and what
    `BatchedPSRLEpisodic` refuses of the priors.  The logged run is `BatchedContinuousLoop`'s; the public `run_logged`
    stays refused."""

    _PREFIX = "cmdp_psrlc"
    _STATS = _PosteriorSamplingAgent._STATS + (("unconverged", L.STAT_PSRL_UNCONVERGED), ("sweeps", L.STAT_PSRL_SWEEPS))

    def __init__(self, env: BatchedMDP, seeds: Sequence[int], optimization_horizon: int, reward_prior_model=None,
                 transitions_prior_model=None, rewards_prior_prms=None, transitions_prior_prms=None, epsilon_greedy=None,
                 boltzmann_temperature=None, psi_weight=1.0, omega_weight=1.0, kappa_weight=1.0, eta_weight=1.0, p=0.05,
                 no_optimistic_sampling=False, truncate_reward_with_max=False, min_steps_before_new_episode=0, max_psi=60,
                 sampler="reference"):
        # posterior_sampling.py:272-275: the reference takes the plain path by itself for large instances
        plain = no_optimistic_sampling or all(int(S) ** 2 * env.A > 6_000_000 for S in env.n_states)
        if not plain:
            raise NotImplementedError("optimistic sampling (psi extended actions) is BatchedPSRLContinuousOptimistic: pass "
                                      "no_optimistic_sampling=True for the reference's plain posterior sampling")
        if truncate_reward_with_max:
            raise NotImplementedError("truncate_reward_with_max=True is not built")
        if min_steps_before_new_episode != 0:
            raise NotImplementedError("min_steps_before_new_episode != 0 at construction is not built: call "
                                      "set_min_steps_before_new_episode(n) on the new agent")
        super().__init__(env, seeds, optimization_horizon, reward_prior_model=reward_prior_model,
                         transitions_prior_model=transitions_prior_model, rewards_prior_prms=rewards_prior_prms,
                         transitions_prior_prms=transitions_prior_prms, epsilon_greedy=epsilon_greedy,
                         boltzmann_temperature=boltzmann_temperature, sampler=sampler)

    def run(self, n_steps: int, train=True, trace: bool = False, stop_at_episode_end: bool = False):
        """n_steps of select_action -> step -> step_update -> (episode_end_update) per instance; the environment is never
        reset.  With `stop_at_episode_end` every instance stops after its next episode_end_update.  Returns as
        `BatchedPSRLEpisodic.run` (observations are never -1)."""
        return self._run(n_steps, train, trace, stop_at_episode_end)

    def run_logged(self, desc, n_logs: int):
        raise NotImplementedError("BatchedPSRLContinuous.run_logged is not built as a public call: the logged run "
                                  "(cmdp_psrlc_run_logged) is reached through BatchedContinuousLoop(env, agent).run")

    def set_min_steps_before_new_episode(self, n: int):
        """The reference's `min_steps_before_new_episode` (posterior_sampling.py:353-355), on a new agent only: with n > 0
        `is_episode_end` evaluates its rule only at a step whose in-run time h (steps since the environment's last reset,
        read before the step) is at least n past `last_change`, and every check that passes moves `last_change` to h.  A run
        of T steps then takes at most T / n artificial episodes per instance.  0 (the default) is the ungated walk.  A
        negative or non-integer n is a ValueError; once an instance has taken a step the library refuses (ERR_INVALID)."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:   # before the handle is touched
            raise ValueError(f"min_steps_before_new_episode {n!r}: an integer >= 0")
        L.check(self._lib.cmdp_psrlc_set_option(self._h, L.PSRLC_OPT_MIN_STEPS, int(n)))

    @property
    def min_steps_before_new_episode(self) -> int:
        return int(self.episode_gate()["min_steps"])

    def episode_gate(self) -> dict:
        """The gate's state: `min_steps` and `last_change` [B] int32 (the reference agent's `last_change`, 0 at creation)."""
        m, lc = C.c_int64(), np.zeros(self.env.B, np.int32)
        L.check(self._lib.cmdp_psrlc_episode_gate(self._h, C.byref(m), L.ptr(lc)))
        return dict(min_steps=int(m.value), last_change=lc)

    def model(self):
        """Per instance the reference's tables: `transitions` dense [S, A, S] float32 (M_DIR.hyper_params), `rewards`
        [S, A, 4] float32 (N_NIG.hyper_params), `N_sa` [S, A] int32 (N.sum(-1)), `nu_k` [S, A] int32 (visits since the last
        episode_end_update); `episode` [B]: posterior samples drawn so far."""
        env = self.env
        R = int(env.row_off[-1])
        rp, tp = np.zeros(R * 4, np.float32), np.zeros(self._nz, np.float32)
        prior, ep = np.zeros(env.B, np.float32), np.zeros(env.B, np.int64)
        nsa, nu = np.zeros(R, np.int32), np.zeros(R, np.int32)
        L.check(self._lib.cmdp_psrlc_model(self._h, L.ptr(rp), L.ptr(tp), L.ptr(prior), L.ptr(nsa), L.ptr(nu), L.ptr(ep)))
        return dict(transitions=self._dense(tp, np.float32, fill=prior),
                    rewards=[x.reshape(-1, env.A, 4) for x in env.split_rows(rp.reshape(R, 4))], N_sa=self._sa(nsa),
                    nu_k=self._sa(nu), episode=ep)

    def last_sample(self):
        """The last posterior sample of every instance, `T` [S, A, S] and `R` [S, A] float32, the `Q` [S, A] the actor holds
        (solved on them), and of that solve `sweeps`, `scheme` (L.SCHEME_JACOBI / L.SCHEME_GAUSS_SEIDEL) and `status`
        (0, or L.ERR_MAX_ITER: Q is then the last sweep's) [B]."""
        env = self.env
        R = int(env.row_off[-1])
        Rs, Q = np.zeros(R, np.float32), np.zeros(R, np.float32)
        sweeps, scheme, status = np.zeros(env.B, np.int64), np.zeros(env.B, np.int32), np.zeros(env.B, np.int32)
        Ts = self._sample_T(lambda T: L.check(self._lib.cmdp_psrlc_last_sample(self._h, L.ptr(T), L.ptr(Rs), L.ptr(Q), L.ptr(sweeps),
                                                                                L.ptr(scheme), L.ptr(status))))
        return dict(T=Ts, R=self._sa(Rs), Q=self._sa(Q), sweeps=sweeps, scheme=scheme, status=status)

    _POLICY_SOLVERS = ("dense", "tables")

    def set_policy_solver(self, route: str):
        """The route behind `policy()` / `policy_solve()` / `average_reward()`.  "dense" (the default): the dense MAP model
        [S, A, S] of every selected instance in a workspace of its own, then the agent's solver k_vi_discounted_dense on it.
        "tables": kernel K17 (csrc/cmdp_map_dvi.h) straight on the posterior tables, O(layout + S) per sweep instead of
        O(S * A * S) and no dense workspace; its Q agrees with the dense route's within the two kernels' rounding bounds and
        the sweep either may stop earlier, not bit for bit.  Anything else is a ValueError."""
        routes = BatchedPSRLContinuous._POLICY_SOLVERS
        if route not in routes:   # before the handle is touched
            raise ValueError(f"policy solver {route!r}: one of {routes}")
        L.check(self._lib.cmdp_psrlc_set_option(self._h, L.PSRLC_OPT_POLICY_SOLVER, routes.index(route)))
        self._policy_solver = route

    @property
    def policy_solver(self) -> str:
        return getattr(self, "_policy_solver", "dense")

    def stats(self) -> dict:
        """As `BatchedPSRLEpisodic.stats`, with `unconverged` (solves that reached the sweep limit; the actor then holds the
        last sweep's Q) and `sweeps` (of the last round's solves, summed)."""
        return self._stats()

    def _set_size_threshold(self, n: int):
        """Test hook: the size threshold of the scheme rule in the agent's solves (the reference's default 300 * 3 * 300)."""
        L.check(self._lib.cmdp_psrlc_set_option(self._h, L.PSRLC_OPT_SIZE_THRESHOLD, int(n)))

    def _set_max_sweeps(self, n: int):
        """Test hook: the sweeps a solve may take (the reference's DP_MAX_ITERATION = 10^6)."""
        L.check(self._lib.cmdp_psrlc_set_option(self._h, L.PSRLC_OPT_MAX_SWEEPS, int(n)))


def optimistic_sampling_scalars(n_states, n_actions, optimization_horizon, p=0.05, psi_weight=1.0, omega_weight=1.0,
                                eta_weight=1.0, max_psi=60):
    """(psi, omega, eta, log(4 S)) of one reference PSRLContinuous (posterior_sampling.py:22-113, :278-307, :426) with the
    reference's own expressions in NumPy."""
    S, A, T = int(n_states), int(n_actions), int(optimization_horizon)
    psi = min(max_psi, max(2, int(psi_weight * (S * np.log(S * A / p)))))
    omega = omega_weight * np.log(T / p)
    eta = max(5, min(10 * S, eta_weight * (np.sqrt(T * S / A) + 12 * omega * S ** 4)))
    return int(psi), float(omega), float(eta), float(np.log(4 * S))


class BatchedPSRLContinuousOptimistic(BatchedPSRLContinuous):
    """One reference `PSRLContinuous` with its DEFAULT, optimistic sampling (Agrawal & Jia: psi extended actions per real
    action) per instance of a continuous `BatchedMDP` (kernel K18, csrc/cmdp_psrlo.h), next to `BatchedPSRLContinuous`, whose
    tables, artificial-episode rule, round driver, solver and MAP policy it shares.  Per instance psi, omega, eta and log(4 S)
    are the reference's expressions (`optimistic_sampling_scalars`).  The walk is greedy on the extended Q [S, A * psi] and
    plays j // psi; the sample is T_ext [S, A * psi, S] with R_ext[s, j] = R[s, j % A], as the reference pairs them.  The
    keyword names and defaults are the reference's.  Refused, each by name: `no_optimistic_sampling=True` and an instance with
    S^2 * A > 6 000 000 (the reference samples plainly there: `BatchedPSRLContinuous`), custom `get_psi` / `get_omega` /
    `get_kappa` / `get_eta`, and what `BatchedPSRLContinuous` refuses.  `sampler="reference"` draws the reference's own
    numbers on the host (a fourth stream, the agent's own RandomState(seed), gives z); `sampler="philox"` draws posterior
    rows, z and rewards on the device, a pure function of (seed, episode, tables).  The sample and its solve take one of two
    routes, `sample_solver="dense" | "compact"` at creation or `set_sample_solver` later.  "dense" (the default) writes T_ext
    and solves it with k_vi_discounted_dense: O(S * A * psi * S) memory and work per sweep.  "compact" (kernel K19,
    csrc/cmdp_psrlo_vi.h) keeps the sample as the sampler leaves it -- per sample the layout values and the value at z_k of the
    simple rows, dense rows only for the posterior rows of the draw -- and solves it there: T_ext is never built, a simple row
    costs its layout length per sweep, and the Q agrees with the dense route's within the two kernels' rounding bounds, not
    bit for bit.  `last_sample()["T"]` is the same T_ext on both routes, bit for bit.  The logged run is
    `BatchedContinuousLoop`'s; the public `run_logged` stays refused."""

    _SAMPLE_SOLVERS = ("dense", "compact")
    _STATS = BatchedPSRLContinuous._STATS + (("sample_bytes", L.STAT_PSRL_SAMPLE_BYTES), ("sample_solver", L.STAT_PSRL_SAMPLE_SOLVER))

    def __init__(self, env: BatchedMDP, seeds: Sequence[int], optimization_horizon: int, reward_prior_model=None,
                 transitions_prior_model=None, rewards_prior_prms=None, transitions_prior_prms=None, epsilon_greedy=None,
                 boltzmann_temperature=None, psi_weight=1.0, omega_weight=1.0, kappa_weight=1.0, eta_weight=1.0, get_psi=None,
                 get_omega=None, get_kappa=None, get_eta=None, p=0.05, no_optimistic_sampling=False,
                 truncate_reward_with_max=False, min_steps_before_new_episode=0, max_psi=60, sampler="reference",
                 sample_solver="dense"):
        if sample_solver not in self._SAMPLE_SOLVERS:
            raise ValueError(f"sample solver {sample_solver!r}: one of {self._SAMPLE_SOLVERS}")
        self._sample_solver = sample_solver
        if no_optimistic_sampling:
            raise NotImplementedError("no_optimistic_sampling=True is BatchedPSRLContinuous: this class builds the reference's "
                                      "optimistic sampling only")
        for b, S in enumerate(env.n_states):
            if int(S) ** 2 * env.A > 6_000_000:
                raise NotImplementedError(f"instance {b}: S^2 * A = {int(S) ** 2 * env.A} > 6 000 000, where the reference samples "
                                          f"plainly by itself: use BatchedPSRLContinuous")
        for name, f in (("get_psi", get_psi), ("get_omega", get_omega), ("get_kappa", get_kappa), ("get_eta", get_eta)):
            if f is not None:
                raise NotImplementedError(f"a custom {name} is not built: the reference's theoretical value is used")
        if truncate_reward_with_max:
            raise NotImplementedError("truncate_reward_with_max=True is not built")
        if min_steps_before_new_episode != 0:
            raise NotImplementedError("min_steps_before_new_episode != 0 at construction is not built: call "
                                      "set_min_steps_before_new_episode(n) on the new agent")
        sc = [optimistic_sampling_scalars(S, env.A, optimization_horizon, p, psi_weight, omega_weight, eta_weight, max_psi)
              for S in env.n_states]
        self.psi = np.array([s[0] for s in sc], np.int32)
        self.omega = np.array([s[1] for s in sc], np.float64)
        self.eta = np.array([s[2] for s in sc], np.float64)
        self._log4s = np.array([s[3] for s in sc], np.float64)
        self._xoff = np.concatenate([[0], np.cumsum(np.asarray(env.n_states, np.int64) * env.A * self.psi)])
        _PosteriorSamplingAgent.__init__(self, env, seeds, optimization_horizon, reward_prior_model=reward_prior_model,
                                         transitions_prior_model=transitions_prior_model, rewards_prior_prms=rewards_prior_prms,
                                         transitions_prior_prms=transitions_prior_prms, epsilon_greedy=epsilon_greedy,
                                         boltzmann_temperature=boltzmann_temperature, sampler=sampler)

    def _create(self, env, seeds, horizon, rprior, tprior, sampler, actor):
        super()._create(env, seeds, horizon, rprior, tprior, L.ptr(self.psi), L.ptr(self.eta), L.ptr(self._log4s), sampler, actor,
                        self._SAMPLE_SOLVERS.index(self._sample_solver), create="_create_optimistic_route")

    def set_sample_solver(self, route: str):
        """The route of the optimistic sample and its solve from the next `episode_end_update` on, internal or external:
        "dense" or "compact" (the class docstring).  Anything else is a ValueError.  Switching an agent created compact to
        dense allocates T_ext then; when it does not fit the call raises and the agent stays compact."""
        routes = self._SAMPLE_SOLVERS
        if route not in routes:   # before the handle is touched
            raise ValueError(f"sample solver {route!r}: one of {routes}")
        L.check(self._lib.cmdp_psrlc_set_option(self._h, L.PSRLC_OPT_SAMPLE_SOLVER, routes.index(route)))
        self._sample_solver = route

    @property
    def sample_solver(self) -> str:
        return self._sample_solver

    def stats(self) -> dict:
        """As `BatchedPSRLContinuous.stats`, with `sample_bytes` (device bytes the sample routes hold: pmk and bump, T_ext and
        its upload once the dense route has run, the posterior blocks of the compact one) and `sample_solver` (the route of
        the last round, whose kernels `sample_kernel_ms` and `vi_kernel_ms` time)."""
        out = self._stats()
        out["sample_solver"] = self._SAMPLE_SOLVERS[out["sample_solver"]]
        return out

    def run_logged(self, desc, n_logs: int):
        raise NotImplementedError("BatchedPSRLContinuousOptimistic.run_logged is not built as a public call: the logged run "
                                  "(cmdp_psrlc_run_logged) is reached through BatchedContinuousLoop(env, agent).run")

    def model(self):
        """As `BatchedPSRLContinuous.model`, with the agent's `N` dense [S, A, S] int32 per instance and `psi`, `eta` [B]."""
        out = super().model()
        N = np.zeros(self._nz, np.int32)
        L.check(self._lib.cmdp_psrlc_counts(self._h, L.ptr(N)))
        out.update(N=self._dense(N, np.int32), psi=self.psi.copy(), eta=self.eta.copy())
        return out

    def _ext(self, x):
        """A per-extended-row array of the library's -> list of [S, A * psi] per instance."""
        return [x[self._xoff[b]:self._xoff[b + 1]].reshape(int(self.env.n_states[b]), -1) for b in range(self.env.B)]

    def last_sample(self):
        """The last optimistic sample of every instance: `T` [S, A * psi, S], `R` [S, A] as N_NIG gave it, `R_ext` and the
        actor's `Q` [S, A * psi], `z` [psi] (reference sampler: -1 where the call drew none), `simple` [S, A] bool, and of the solve `sweeps`,
        `scheme`, `status` [B]."""
        env = self.env
        R, X = int(env.row_off[-1]), int(self._xoff[-1])
        Rs, Rx, Q = np.zeros(R, np.float32), np.zeros(X, np.float32), np.zeros(X, np.float32)
        z, simple = np.zeros(int(self.psi.sum()), np.int32), np.zeros(R, np.uint8)
        sweeps, scheme, status = np.zeros(env.B, np.int64), np.zeros(env.B, np.int32), np.zeros(env.B, np.int32)
        sizes = [int(S) * env.A * int(k) * int(S) for S, k in zip(env.n_states, self.psi)]
        T = np.zeros(sum(sizes), np.float32)
        L.check(self._lib.cmdp_psrlc_last_sample_optimistic(self._h, L.ptr(T), L.ptr(Rs), L.ptr(Rx), L.ptr(Q), L.ptr(z), L.ptr(simple),
                                                            L.ptr(sweeps), L.ptr(scheme), L.ptr(status)))
        Ts = [x.reshape(int(S), -1, int(S)) for x, S in zip(np.split(T, np.cumsum(sizes)[:-1]), env.n_states)]
        return dict(T=Ts, R=self._sa(Rs), R_ext=self._ext(Rx), Q=self._ext(Q), z=np.split(z, np.cumsum(self.psi)[:-1]),
                    simple=[m.astype(bool) for m in self._sa(simple)], sweeps=sweeps, scheme=scheme, status=status)
