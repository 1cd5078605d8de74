"""ctypes binding of libcmdp.so (include/cmdp.h).  Fails loudly when the HIP library is missing:
there is no CPU fallback anywhere in this package."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libcmdp.so")

OK, ERR_INVALID, ERR_HIP, ERR_NEEDS_RESET, ERR_UNSUPPORTED, ERR_MAX_ITER, ERR_NO_DEVICE, ERR_MAX_VALUE, ERR_OVERFLOW = (
    0, -1, -2, -3, -4, -5, -6, -7, -8)
RNG_MT_COMPAT, RNG_PHILOX = 0, 1
POLICY_RANDOM, POLICY_HOST_ACTIONS, POLICY_GREEDY_Q = 0, 1, 2
POLICY_RANDOM_REFERENCE = 3  # RandomActor's stream: RandomState(seed).randint(0, A, .) per instance, generated on the device (K16)
SCHEME_AUTO, SCHEME_JACOBI, SCHEME_GAUSS_SEIDEL = 0, 1, 2
LAYOUT_CSR, LAYOUT_DENSE = 0, 1
FLAG_REWARD_MEANS = 1
FLAG_BETA_GAMMAS = 4   # device-sampled Beta rewards: two gammas for every shape (rounds 1-2 recipe)
FLAG_REWARD_CACHE = 2  # reference-exact per-triple reward caches for batches (csrc/cmdp_reward_cache.h)
OPT_ROLLOUT_KERNEL = 1
OPT_DP_KERNEL = 2
OPT_LDS_GROUPS_PER_CU = 3
OPT_DIAMETER_WORKSPACE_MB = 4
OPT_CHAIN_EXACT_ORDER = 5
OPT_MIXING_PATH = 6
OPT_DIAMETER_RELABEL_MIN_STATES = 7
STAT_DP_KERNEL_MS, STAT_DP_KERNEL, STAT_REWARD_FILLS, STAT_REWARD_ROUNDS, STAT_ROLLOUT_KERNEL_MS, STAT_HIST_KERNEL_MS = 1, 2, 3, 4, 5, 6
STAT_CHAIN_FAST_INSTANCES = 7
STAT_REWARD_FILL_MS, STAT_REWARD_ROUND_MS = 8, 9
STAT_DIAMETER_CLUSTER_LAUNCHES, STAT_DIAMETER_CLUSTER_FALLBACKS = 10, 11
STAT_UCRL2_UNCONVERGED, STAT_UCRL2_ROUNDS, STAT_UCRL2_SOLVES, STAT_UCRL2_ROUND_MS = 12, 13, 14, 15
STAT_UCRL2_WAIT_MS = 16
STAT_PSRL_ROUNDS, STAT_PSRL_SOLVES, STAT_PSRL_SAMPLE_KERNEL_MS, STAT_PSRL_VI_KERNEL_MS, STAT_PSRL_REFERENCE_MS = 17, 18, 19, 20, 21
STAT_DIAMETER_KERNEL = 22  # family * 1000 + n * 10 + flag, see include/cmdp.h
STAT_UCRL2_POLICY_KERNEL_MS = 23
STAT_PSRL_POLICY_KERNEL_MS = 24
STAT_UCRL2_POLICY_SOLVED, STAT_UCRL2_POLICY_REUSED = 25, 26  # instances K14 solved / kept their stored policy
STAT_ACTIONS_KERNEL_MS = 27  # K16 before the last K1E walk under POLICY_RANDOM_REFERENCE
STAT_PSRL_UNCONVERGED, STAT_PSRL_SWEEPS = 28, 29  # continuous PSRL (K13): solves at max_sweeps / sweeps of the last round
STAT_PSRL_SAMPLE_BYTES, STAT_PSRL_SAMPLE_SOLVER = 30, 31  # optimistic PSRL (K18 / K19): bytes of the sample routes / last round's route
PSRLC_OPT_SIZE_THRESHOLD, PSRLC_OPT_MAX_SWEEPS, PSRLC_OPT_POLICY_SOLVER, PSRLC_OPT_SAMPLE_SOLVER = 1, 2, 3, 4
PSRLC_OPT_MIN_STEPS = 5
PSRL_SAMPLER_REFERENCE, PSRL_SAMPLER_PHILOX = 0, 1
PSRL_KEY_HI = 0x5053524C
BOUND_CHERNOFF, BOUND_BERNSTEIN = 0, 1
ACTOR_GREEDY, ACTOR_EPSILON_GREEDY, ACTOR_BOLTZMANN = 0, 1, 2
UCRL2_OPT_MAX_SWEEPS = 1
UCRL2_OPT_POLICY_SIZE_THRESHOLD = 2
UCRL2_OPT_POLICY_REUSE = 3
NOISE_NONE, NOISE_GAUSSIAN, NOISE_GAUSSIAN_CORRELATED, NOISE_STUDENT_T, NOISE_STUDENT_T_CORRELATED = 0, 1, 2, 3, 4
CALIB_LDS_READ, CALIB_LDS_CHAIN, CALIB_LDS_CHAIN_SHARED = 0, 1, 2
DP_AUTO, DP_WORKGROUP, DP_REGISTER = 0, 1, 2
DP_REGISTER_DISTINCT = 5  # K2U: register-resident, gathers deduplicated per state
DP_REGISTER_WAVEFRONT = 7  # K2W: K2U's tables with one wavefront per instance (<= 448 states, <= 5 distinct successors)
ROLLOUT_AUTO, ROLLOUT_GLOBAL, ROLLOUT_LDS, ROLLOUT_LDS_STOCHASTIC = 0, 1, 2, 3
ROLLOUT_LDS_TEMPLATE = 4  # K1T: K1P with one successor table per workgroup (batches of action-permuted copies of one MDP)
ROLLOUT_LDS_TEMPLATE_STREAM = 5  # K1U: K1T with the trace streamed to HBM and histogrammed afterwards (256 instances per CU)
ROLLOUT_EPISODE_PARALLEL = 6  # K1E: lane = (instance, episode): episodic batches with two actions walk their episodes in parallel
# cmdp_k1s_plan / cmdp_k1s_plan_desc: the fields in the order of include/cmdp.h, and the names of `form` (the compiled form of
# K1S's walk loop: generic, or team * 4 + reward source)
K1S_PLAN_FIELDS = ("ok", "G", "nw", "gw", "team", "U", "n_pat", "n_codes", "reward_mode", "rc_packed", "n_shapes", "shape_bytes",
                   "ch", "form")
K1S_REWARD_SOURCES = ("packed", "state_table", "row")
K1S_FORMS = {0: "generic", **{t * 4 + i: f"team{t}_{src}" for t in (16, 8, 1) for i, src in enumerate(K1S_REWARD_SOURCES)}}
# cmdp_det_plan / cmdp_det_plan_desc: the fields of K1L / K1P, K1T and K1U in the order of include/cmdp.h, the names of the two
# `form` fields (what launch_k1lp / launch_k1u branch on) and the order of the knobs cmdp_det_plan_desc takes
DET_PLAN_FIELDS = {
    "k1lp": ("ok", "pipe", "packed", "code_shift", "succ_bits", "n_codes", "ch", "G", "per_cu", "capacity", "slot_bytes", "lds_bytes",
             "form"),
    "k1t": ("ok", "automatic", "ch", "G", "capacity", "slot_bytes", "tmpl_bytes", "lds_bytes"),
    "k1u": ("ok", "automatic", "pack10", "ch", "G", "capacity", "lds_bytes", "hist_lds_bytes", "form"),
}
K1LP_FORMS = {0: "k1l_unpacked", 1: "k1l_packed", 2: "k1p"}
K1U_FORMS = {0: "pack10", 1: "wide"}
# cmdp_k1e_pair_plan / cmdp_k1e_pair_plan_desc: the fields in the order of include/cmdp.h and the names of `last_form`
K1E_PAIR_PLAN_FIELDS = ("ok", "H", "SP2", "n_even", "lds_bytes", "last_form")
K1E_FORMS = {0: None, 1: "single", 2: "pair"}
DET_PLAN_KNOBS = ("pipe", "k1l_G", "k1t_G", "k1u_G", "k1t_ch")   # CMDP_K1L_PIPE, CMDP_K1L_G, CMDP_K1T_G, CMDP_K1U_G, CMDP_K1T_CH

EXPORTS = [
    "cmdp_version", "cmdp_build_id", "cmdp_last_error", "cmdp_device_count", "cmdp_set_device", "cmdp_create", "cmdp_destroy",
    "cmdp_stream", "cmdp_reset", "cmdp_step", "cmdp_rollout", "cmdp_rollout_async", "cmdp_synchronize", "cmdp_stat", "cmdp_calibrate", "cmdp_set_option", "cmdp_lds_plan",
    "cmdp_visits", "cmdp_reset_visits", "cmdp_set_visits", "cmdp_state", "cmdp_last_start", "cmdp_vi_discounted", "cmdp_pe_discounted",
    "cmdp_vi_episodic", "cmdp_pe_episodic", "cmdp_diameter", "cmdp_diameter_episodic", "cmdp_value_norm", "cmdp_gth", "cmdp_qlearning_create", "cmdp_qlearning_destroy", "cmdp_qlearning_run",
    "cmdp_qlearning_tables", "cmdp_qlearning_evaluate", "cmdp_greedy_policy_episodic", "cmdp_qlearning_continuous_create",
    "cmdp_qlearning_policy", "cmdp_qlearning_average_reward", "cmdp_qlearning_run_logged", "cmdp_tracker_replay", "cmdp_average_reward", "cmdp_diameter_range", "cmdp_diameter_sparse_f64", "cmdp_mixing_time", "cmdp_set_observation_table", "cmdp_observe", "cmdp_observe_noise",
    "cmdp_set_reward_streams", "cmdp_legacy_beta", "cmdp_extended_vi",
    "cmdp_ucrl2_create", "cmdp_ucrl2_destroy", "cmdp_ucrl2_run", "cmdp_ucrl2_layout", "cmdp_ucrl2_model", "cmdp_ucrl2_last_solve",
    "cmdp_ucrl2_set_option", "cmdp_ucrl2_policy", "cmdp_ucrl2_average_reward", "cmdp_model_vi_scheme", "cmdp_vi_discounted_model",
    "cmdp_psrl_create", "cmdp_psrl_destroy", "cmdp_psrl_run", "cmdp_psrl_layout", "cmdp_psrl_model", "cmdp_psrl_last_sample",
    "cmdp_psrl_reference_sample", "cmdp_vi_episodic_dense", "cmdp_psrl_episode_end_update", "cmdp_k1e_round_interior",
    "cmdp_k1e_code_counts", "cmdp_k1e_scan_words", "cmdp_k1e_scan_words_ex", "cmdp_k1s_plan", "cmdp_k1s_plan_desc", "cmdp_det_plan", "cmdp_det_plan_desc", "cmdp_chain_plan_desc", "cmdp_chain_choice",
    "cmdp_k1e_pair_plan", "cmdp_k1e_pair_plan_desc",
    "cmdp_psrl_map_rows", "cmdp_vi_episodic_map", "cmdp_psrl_policy", "cmdp_psrl_evaluate",
    "cmdp_ucrl2_run_logged", "cmdp_psrl_run_logged",
    "cmdp_set_action_streams", "cmdp_action_stream_state", "cmdp_set_action_stream_state", "cmdp_mt_randint", "cmdp_mt_action_bits",
    "cmdp_psrlc_create", "cmdp_psrlc_destroy", "cmdp_psrlc_run", "cmdp_psrlc_episode_end_update", "cmdp_psrlc_layout",
    "cmdp_psrlc_model", "cmdp_psrlc_last_sample", "cmdp_psrlc_set_option", "cmdp_psrlc_policy", "cmdp_psrlc_average_reward",
    "cmdp_vi_discounted_dense", "cmdp_vi_discounted_map", "cmdp_vi_discounted_optimistic", "cmdp_psrlc_create_optimistic_route",
    "cmdp_psrlc_create_optimistic", "cmdp_psrlc_last_sample_optimistic", "cmdp_psrlc_counts", "cmdp_psrlo_reference_draw",
    "cmdp_psrlc_run_logged", "cmdp_psrlc_episode_gate",
]


class CmdpDesc(C.Structure):
    _fields_ = [
        ("n_instances", C.c_int32), ("n_actions", C.c_int32), ("horizon", C.c_int32), ("rng_mode", C.c_int32),
        ("layout", C.c_int32), ("flags", C.c_int32),
        ("reward_min", C.c_double), ("reward_max", C.c_double),
        ("state_off", C.c_void_p),
        ("sp_ptr", C.c_void_p), ("sp_next", C.c_void_p), ("sp_cum", C.c_void_p), ("sp_reward", C.c_void_p),
        ("sp_rkind", C.c_void_p), ("sp_rp0", C.c_void_p), ("sp_rp1", C.c_void_p), ("sp_seed", C.c_void_p), ("start_off", C.c_void_p), ("start_state", C.c_void_p),
        ("start_cum", C.c_void_p), ("start_seed", C.c_void_p), ("philox_key", C.c_void_p),
        ("csr_ptr", C.c_void_p), ("csr_col", C.c_void_p), ("csr_val", C.c_void_p), ("R", C.c_void_p),
    ]


class CmdpLoopDesc(C.Structure):
    _fields_ = [
        ("n_steps", C.c_int64), ("log_every", C.c_int64),
        ("n_check", C.c_int32), ("horizon", C.c_int32), ("kmax", C.c_int32), ("reserved", C.c_int32),
        ("max_time", C.c_double),
        ("base_val", C.c_void_p), ("base_kind", C.c_void_p), ("opt0", C.c_void_p), ("worst0", C.c_void_p),
        ("start_pos", C.c_void_p), ("start_prob", C.c_void_p),
    ]


LOG_COLUMNS = [  # CMDP_LOG_COLUMNS: the indicator names in sorted order, without "steps"
    "cumulative_expected_reward", "cumulative_regret", "cumulative_reward", "normalized_cumulative_expected_reward",
    "normalized_cumulative_regret", "normalized_cumulative_reward", "optimal_cumulative_expected_reward",
    "optimal_normalized_cumulative_expected_reward", "random_cumulative_expected_reward", "random_cumulative_regret",
    "random_normalized_cumulative_expected_reward", "random_normalized_cumulative_regret", "steps_per_second",
    "worst_cumulative_expected_reward", "worst_cumulative_regret", "worst_normalized_cumulative_expected_reward",
    "worst_normalized_cumulative_regret",
]


class CmdpError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"libcmdp error {code}: {message}")
        self.code = code


class DynamicProgrammingMaxIterationExceeded(Exception):
    """Same name as the reference's exception (colosseum/dynamic_programming/utils.py:8-9)."""


_lib = None


def source_files():
    """The files libcmdp.so is compiled from, in the order their hash is taken."""
    csrc = os.path.join(HERE, "csrc")
    files = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))]
    files.append(os.path.join(os.path.dirname(HERE), "include", "cmdp.h"))
    return files


def source_hash():
    """SHA-256 over the library's sources: what `cmdp_build_id()` of an up-to-date build returns."""
    import hashlib

    h = hashlib.sha256()
    for f in source_files():
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()


def built_id(path=LIB_PATH):
    """The build id stamped into the library file at `path`, read from the file's bytes (no dlopen: a process that
    rebuilds the library must not have the old image mapped under the same name); None if missing or unstamped."""
    import re

    if not os.path.exists(path):
        return None
    m = re.search(rb"CMDP_BUILD_ID=([0-9a-f]{64})", open(path, "rb").read())
    return m.group(1).decode() if m else None


def load():
    """Returns the loaded library; raises if it has not been built (python __graft_entry__.py / build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                f"(python -c 'import __graft_entry__ as g; g.build()').  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        L.cmdp_build_id.restype = C.c_char_p
        bid, want = L.cmdp_build_id().decode(), source_hash()
        if bid != want and os.environ.get("CMDP_ALLOW_STALE_LIB") != "1":
            raise ImportError(
                f"{LIB_PATH} was built from other sources (build id {bid[:16]}, tree {want[:16]}): rebuild it "
                f"(python -c 'import __graft_entry__ as g; g.build()').")
        vp, i32, i64, f32, f64 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
        L.cmdp_version.restype = C.c_int
        L.cmdp_last_error.restype = C.c_char_p
        L.cmdp_device_count.restype = C.c_int
        L.cmdp_set_device.argtypes = [i32]
        L.cmdp_create.argtypes = [C.POINTER(vp), C.POINTER(CmdpDesc)]
        L.cmdp_destroy.argtypes = [vp]
        L.cmdp_stream.restype = vp
        L.cmdp_stream.argtypes = [vp]
        L.cmdp_reset.argtypes = [vp, vp, vp]
        L.cmdp_step.argtypes = [vp, vp, i32, vp, vp, vp]
        L.cmdp_rollout.argtypes = [vp, i32, vp, i64, vp, vp, vp, vp, vp]
        L.cmdp_rollout_async.argtypes = [vp, i32, i64]
        L.cmdp_synchronize.argtypes = [vp]
        L.cmdp_stat.argtypes = [vp, i32, vp]
        L.cmdp_calibrate.argtypes = [i32, i64, vp]
        L.cmdp_set_option.argtypes = [vp, i32, i64]
        L.cmdp_lds_plan.argtypes = [vp, vp]
        L.cmdp_visits.argtypes = [vp, vp, vp]
        L.cmdp_reset_visits.argtypes = [vp]
        L.cmdp_set_visits.argtypes = [vp, vp, vp]
        L.cmdp_state.argtypes = [vp, vp, vp, vp]
        L.cmdp_last_start.argtypes = [vp, vp, vp]
        L.cmdp_vi_discounted.argtypes = [vp, f32, f64, i32, i64, f64, vp, vp, vp, vp]
        L.cmdp_pe_discounted.argtypes = [vp, vp, f32, f64, i32, i64, vp, vp, vp, vp]
        L.cmdp_vi_episodic.argtypes = [vp, i32, vp, vp, vp]
        L.cmdp_pe_episodic.argtypes = [vp, i32, vp, vp, vp, vp]
        L.cmdp_diameter.argtypes = [vp, f64, i32, i64, vp, vp]
        L.cmdp_diameter_episodic.argtypes = [vp, i32, vp, vp, vp, f64, i64, vp, vp]
        L.cmdp_value_norm.argtypes = [vp, vp, vp]
        L.cmdp_gth.argtypes = [i32, vp, vp, vp]
        L.cmdp_extended_vi.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f64, i64, vp, vp, vp, vp, vp]
        L.cmdp_qlearning_create.argtypes = [C.POINTER(vp), vp, vp, i64, f64, f64, f64, f64, i32]
        L.cmdp_qlearning_destroy.argtypes = [vp]
        L.cmdp_qlearning_run.argtypes = [vp, i64, vp, vp, vp]
        L.cmdp_qlearning_evaluate.argtypes = [vp, vp]
        L.cmdp_qlearning_run_logged.argtypes = [vp, C.POINTER(CmdpLoopDesc), i64, vp, vp, vp, vp, vp]
        L.cmdp_ucrl2_run_logged.argtypes = [vp, C.POINTER(CmdpLoopDesc), i64, vp, vp, vp, vp, vp]
        L.cmdp_psrl_run_logged.argtypes = [vp, C.POINTER(CmdpLoopDesc), i64, vp, vp, vp, vp, vp]
        L.cmdp_tracker_replay.argtypes = [C.POINTER(CmdpLoopDesc), i32, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cmdp_qlearning_continuous_create.argtypes = [C.POINTER(vp), vp, vp, i64, f64, f64, f64, f64]
        L.cmdp_qlearning_policy.argtypes = [vp, vp]
        L.cmdp_qlearning_average_reward.argtypes = [vp, vp, vp, vp]
        L.cmdp_average_reward.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.cmdp_diameter_range.argtypes = [vp, C.c_double, i64, i64, i64, vp]
        L.cmdp_diameter_sparse_f64.argtypes = [vp, C.c_double, i64, vp, vp]
        L.cmdp_mixing_time.argtypes = [vp, vp, vp, C.c_double, i64, vp, vp]
        L.cmdp_set_observation_table.argtypes = [vp, vp, i32, i32]
        L.cmdp_observe.argtypes = [vp, C.c_double, vp]
        L.cmdp_observe_noise.argtypes = [vp, i32, C.c_double, C.c_double, vp, vp]
        L.cmdp_greedy_policy_episodic.argtypes = [vp, i32, i32, vp, vp]
        L.cmdp_qlearning_tables.argtypes = [vp, vp, vp]
        L.cmdp_set_reward_streams.argtypes = [vp, vp, vp, vp, vp]
        L.cmdp_legacy_beta.argtypes = [vp, vp, vp, vp, f64, f64, i64, vp]
        L.cmdp_set_action_streams.argtypes = [vp, vp]
        L.cmdp_action_stream_state.argtypes = [vp, vp, vp]
        L.cmdp_set_action_stream_state.argtypes = [vp, vp, vp]
        L.cmdp_mt_randint.argtypes = [vp, vp, i32, i64, vp]
        L.cmdp_mt_action_bits.argtypes = [vp, vp, i64, i64, vp]
        L.cmdp_ucrl2_create.argtypes = [C.POINTER(vp), vp, vp, i64, f64, f64, i32, i32, i32]
        L.cmdp_ucrl2_destroy.argtypes = [vp]
        L.cmdp_ucrl2_run.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, vp]
        L.cmdp_ucrl2_layout.argtypes = [vp, vp, vp, vp]
        L.cmdp_ucrl2_model.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cmdp_ucrl2_last_solve.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cmdp_ucrl2_set_option.argtypes = [vp, i32, i64]
        L.cmdp_ucrl2_policy.argtypes = [vp, vp, vp, vp, vp, vp]
        L.cmdp_ucrl2_average_reward.argtypes = [vp, vp, vp, vp]
        L.cmdp_model_vi_scheme.argtypes = [i32, i32, i64, i64, f64]
        L.cmdp_vi_discounted_model.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, f32, f64, i32, i64, f64, i64, vp, vp, vp, vp, vp]
        L.cmdp_psrl_create.argtypes = [C.POINTER(vp), vp, vp, i64, vp, vp, i32, i32]
        L.cmdp_psrl_destroy.argtypes = [vp]
        L.cmdp_psrl_run.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, vp]
        L.cmdp_psrl_episode_end_update.argtypes = [vp]
        L.cmdp_psrl_layout.argtypes = [vp, vp, vp, vp]
        L.cmdp_psrl_model.argtypes = [vp, vp, vp, vp, vp]
        L.cmdp_psrl_last_sample.argtypes = [vp, vp, vp, vp]
        L.cmdp_psrl_reference_sample.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp]
        L.cmdp_vi_episodic_dense.argtypes = [i32, vp, vp, i32, vp, vp, vp, vp]
        L.cmdp_psrl_map_rows.argtypes = [i32, i32, vp, vp, vp, f32, vp, vp, vp]
        L.cmdp_vi_episodic_map.argtypes = [i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.cmdp_psrl_policy.argtypes = [vp, vp, vp, vp]
        L.cmdp_psrl_evaluate.argtypes = [vp, vp, vp]
        L.cmdp_psrlc_create.argtypes = [C.POINTER(vp), vp, vp, i64, vp, vp, i32, i32]
        L.cmdp_psrlc_destroy.argtypes = [vp]
        L.cmdp_psrlc_run.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp, vp]
        L.cmdp_psrlc_episode_end_update.argtypes = [vp]
        L.cmdp_psrlc_layout.argtypes = [vp, vp, vp, vp]
        L.cmdp_psrlc_model.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.cmdp_psrlc_last_sample.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.cmdp_psrlc_set_option.argtypes = [vp, i32, i64]
        L.cmdp_psrlc_policy.argtypes = [vp, vp, vp, vp, vp, vp]
        L.cmdp_psrlc_average_reward.argtypes = [vp, vp, vp, vp]
        L.cmdp_psrlc_create_optimistic.argtypes = [C.POINTER(vp), vp, vp, i64, vp, vp, vp, vp, vp, i32, i32]
        L.cmdp_psrlc_last_sample_optimistic.argtypes = [vp] * 10
        L.cmdp_psrlc_create_optimistic_route.argtypes = [C.POINTER(vp), vp, vp, i64, vp, vp, vp, vp, vp, i32, i32, i32]
        L.cmdp_vi_discounted_optimistic.argtypes = [i32] + [vp] * 12 + [f32, f64, i32, i64, f64, i64, vp, vp, vp, vp, vp]
        L.cmdp_psrlc_counts.argtypes = [vp, vp]
        L.cmdp_psrlc_run_logged.argtypes = [vp, C.POINTER(CmdpLoopDesc), i64, vp, vp, vp, vp, vp]
        L.cmdp_psrlc_episode_gate.argtypes = [vp, vp, vp]
        L.cmdp_psrlo_reference_draw.argtypes = [vp] * 12 + [i32, i32, i32, f64, i64, vp, vp, vp, vp, f32] + [vp] * 6
        L.cmdp_vi_discounted_dense.argtypes = [i32, vp, vp, vp, vp, f32, f64, i32, i64, f64, i64, vp, vp, vp, vp, vp]
        L.cmdp_vi_discounted_map.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, f32, f64, i32, i64, f64, i64, vp, vp, vp, vp, vp, vp, vp]
        L.cmdp_k1e_round_interior.argtypes = [i32, i32, i64, i32]
        L.cmdp_k1e_code_counts.argtypes = [C.c_uint32, C.c_uint32, i32]
        L.cmdp_k1e_scan_words.argtypes = [vp, i64, i32, i32, i64, i32, i32, vp, f64, vp, vp]
        L.cmdp_k1e_scan_words_ex.argtypes = [vp, i64, i32, i32, i64, i32, i32, vp, f64, vp, vp]
        L.cmdp_k1s_plan.argtypes = [vp, vp]
        L.cmdp_k1s_plan_desc.argtypes = [C.POINTER(CmdpDesc), i32, i32, vp]
        L.cmdp_det_plan.argtypes = [vp, vp]
        L.cmdp_det_plan_desc.argtypes = [C.POINTER(CmdpDesc), i32, vp, vp]
        L.cmdp_k1e_pair_plan.argtypes = [vp, vp]
        L.cmdp_k1e_pair_plan_desc.argtypes = [C.POINTER(CmdpDesc), i32, i32, vp, vp, vp, vp, vp]
        L.cmdp_chain_plan_desc.argtypes = [C.POINTER(CmdpDesc), vp, vp, vp, vp, i64, vp, vp, vp, vp, vp]
        L.cmdp_chain_choice.argtypes = [i32, i32, i32, i32, i32, vp]
        L.cmdp_k1e_code_counts.restype = C.c_uint32
        _lib = L
    return _lib


def check(rc):
    if rc == OK:
        return
    msg = load().cmdp_last_error().decode()
    if rc == ERR_MAX_ITER:
        raise DynamicProgrammingMaxIterationExceeded(msg)
    if rc == ERR_NEEDS_RESET:
        raise AssertionError(msg)  # the reference raises AssertionError (mdp/base.py:1290)
    raise CmdpError(rc, msg)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def carr(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


_hip = None


def pinned_empty(n, dtype):
    """A page-locked host array (hipHostMalloc) for results that are fetched repeatedly: device-to-host copies into it
    run as one DMA at PCIe rate and touch no fresh pages (a new `np.zeros` costs a page fault per 4 KiB inside the copy).
    Freed when the array is garbage collected."""
    import weakref

    global _hip
    load()  # libcmdp.so has mapped the HIP runtime
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        _hip.hipHostFree.argtypes = [C.c_void_p]
    dt = np.dtype(dtype)
    nbytes = max(1, int(n)) * dt.itemsize
    p = C.c_void_p()
    rc = _hip.hipHostMalloc(C.byref(p), nbytes, 0)
    if rc != 0 or not p.value:
        raise MemoryError(f"hipHostMalloc({nbytes}) failed with {rc}")
    buf = (C.c_char * nbytes).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dt, count=int(n))
    weakref.finalize(buf, _hip.hipHostFree, C.c_void_p(p.value))
    return arr
