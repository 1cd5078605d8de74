/* cmdp.h -- C ABI of libcmdp.so, the MI355X-native batched tabular-MDP engine.
 *
 * The reference (MichelangeloConserva/Colosseum, pure Python + numba) has no FFI of its own; the
 * drop-in boundary is its Python call surface.  Every entry point below names the reference
 * interface it replaces (paths relative to the reference tree).  The library is loaded with
 * ctypes.CDLL by colosseum_amd/_lib.py; INTEGRATION.md shows the binding a reference maintainer
 * would add.
 *
 * Conventions: plain C types only; every function returns 0 (CMDP_OK) or a negative error code and
 * never throws; cmdp_last_error() gives the message of the calling thread's last failure; host
 * buffers are borrowed for the duration of the call; a cmdp_t owns its device memory and one HIP
 * stream, is bound to the device current at cmdp_create time, and is not thread-safe; calls are
 * synchronous on return unless stated otherwise.
 *
 * Batch layout: B independent MDP instances (environment parameterisation x seed), instance b having
 * S_b states and the common A actions.  state_off[b] = sum_{i<b} S_i.  "row" r of instance b is
 * (state_off[b] + s) * A + a for the action a an agent passes to step().  All per-state arrays are
 * the instances' arrays concatenated ([state_off[B]]), all per-row arrays likewise ([state_off[B]*A]).
 */
#ifndef CMDP_H
#define CMDP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMDP_ABI_VERSION 1

enum {
  CMDP_OK = 0,
  CMDP_ERR_INVALID = -1,     /* bad argument (message says which)                                  */
  CMDP_ERR_HIP = -2,         /* a HIP runtime call failed                                           */
  CMDP_ERR_NEEDS_RESET = -3, /* step() on an instance whose episode ended: the reference's
                                `assert not self.necessary_reset`, colosseum/mdp/base.py:1290       */
  CMDP_ERR_UNSUPPORTED = -4, /* feature outside the built scope                                     */
  CMDP_ERR_MAX_ITER = -5,    /* DynamicProgrammingMaxIterationExceeded,
                                colosseum/dynamic_programming/utils.py:8-9                          */
  CMDP_ERR_NO_DEVICE = -6,   /* no HIP device visible                                               */
  CMDP_ERR_MAX_VALUE = -7,   /* |V| exceeded max_abs_value: the reference returns None,
                                colosseum/dynamic_programming/infinite_horizon.py:136-138           */
  CMDP_ERR_OVERFLOW = -8     /* a device visit counter (int32) could wrap during this call: refused before anything is
                                stepped -- read the counters out (cmdp_visits widens them to int64) and
                                cmdp_reset_visits first; the reference's Python ints do not wrap      */
};

/* Random-number discipline of the transition sampler. */
enum {
  /* One CPython MT19937 stream per stochastic (s,a) row and per stochastic start sampler, seeded
     like random.Random(seed) and consumed one random() per sample: reproduces the reference's
     NextStateSampler (colosseum/mdp/utils/custom_samplers.py:49-72) draw for draw. */
  CMDP_RNG_MT_COMPAT = 0,
  /* Philox-4x32-10 keyed by the instance (counter-based, nothing stored per sampler):
     counter (n, domain): domain 0, n = transition index -> 53-bit transition uniform (stochastic rows);
     domain 1, n = reset index -> start-state uniform; domain 2 -> the actions of CMDP_POLICY_RANDOM: this project's OWN
     stream, the throughput stream -- NOT the reference's (RandomActor, colosseum/agent/actors/random.py:34-47, pops
     numpy blocks of 50 000 from RandomState(seed); that stream is CMDP_POLICY_RANDOM_REFERENCE, in either rng_mode): for A in {2, 4, 16, 256} the PACKED form -- block n / apb holds apb = 128 / log2(A)
     actions, action k = n % apb in bits [lg (k % apw), +lg) of word k / apw, apw = 32 / lg (A = 2: 128
     one-bit actions per block, least significant bit of word 0 first); for any other A, block n >> 2,
     word (n & 3), a = (word * A) >> 32. */
  CMDP_RNG_PHILOX = 1
};

/* Action source of cmdp_rollout. */
enum {
  CMDP_POLICY_RANDOM = 0,       /* uniform over A from the instance's Philox stream (config C2)      */
  CMDP_POLICY_HOST_ACTIONS = 1, /* policy_arg = const int8_t actions[n_steps][B]                      */
  CMDP_POLICY_GREEDY_Q = 2,     /* policy_arg = const float Q: per instance [S_b][A] (continuous) or
                                   [H][S_b][A] at H*state_off[b]*A (episodic, row = in-episode time);
                                   the action is the first maximiser of the current row            */
  /* The reference's random agent: instance b takes the actions RandomState(seeds[b]).randint(0, A, .) yields, one after the
     other across calls (RandomActor, colosseum/agent/actors/random.py:34-47: its blocks of 50 000 are consecutive pieces of
     that stream).  Generated on the device from the streams cmdp_set_action_streams seeded (CMDP_ERR_INVALID before that);
     policy_arg is ignored.  CMDP_POLICY_RANDOM is the Philox stream of domain 2 instead: equally distributed, other actions.
     Runs on the episode-parallel kernel K1E when the batch is eligible (automatically from 64 transitions, or
     CMDP_OPT_ROLLOUT_KERNEL 6) and on the lane-per-instance kernel K1 otherwise; CMDP_OPT_ROLLOUT_KERNEL 2-5 are
     CMDP_ERR_UNSUPPORTED with this policy. */
  CMDP_POLICY_RANDOM_REFERENCE = 3
};

/* Sweep scheme of the discounted solvers. */
enum {
  CMDP_SCHEME_AUTO = 0,   /* the reference's own size/density rule,
                             colosseum/dynamic_programming/infinite_horizon.py:25-36,53-64          */
  CMDP_SCHEME_JACOBI = 1, /* _discounted_value_iteration_sparse / _discounted_policy_evaluation_sparse */
  CMDP_SCHEME_GAUSS_SEIDEL = 2 /* _discounted_value_iteration / _discounted_policy_evaluation (numba) */
};

/* Device table layout of the transition sampler. */
enum {
  CMDP_LAYOUT_CSR = 0,   /* per-row successor lists (compact; the default)                           */
  CMDP_LAYOUT_DENSE = 1  /* per-instance dense float32 P[s,a,:] rows streamed from HBM, wavefront
                            prefix-sum CDF lookup: next = min{ j : sum_{i<=j} P[s,a,i] > u*total } in
                            STATE order (not the sampler's creation order), so stochastic rows draw
                            different -- equally distributed -- successors than CMDP_LAYOUT_CSR for the
                            same u.  Philox mode, cmdp_rollout only, needs both halves of the description
                            and S_max*A*4*round_up(S_max,256) bytes per instance.                      */
};

/* cmdp_desc.flags */
enum {
  /* Accept entries with sp_rkind != 0 (stochastic reward distributions) and report sp_reward -- which then holds
     the distribution MEAN -- as the reward of such transitions.  For callers that sample those rewards themselves
     (the reference-exact host sampler of colosseum_amd/mdp/reward_sampler.py) or only need expectations. */
  CMDP_FLAG_REWARD_MEANS = 1,
  /* REFERENCE-EXACT stochastic rewards for a whole batch: BaseMDP.sample_reward (colosseum/mdp/base.py:1187-1207) keeps a
     FIFO cache of 5000 samples per visited (node, action, next_node) triple, drawn from the MDP's single numpy stream
     `self._rng` when the triple is first needed and whenever its cache runs dry, so the draw order follows the
     trajectory.  With this flag the device serves rewards from such caches in HBM; an instance that needs a block it does
     not have parks (its transition committed, the step unfinished), the host draws the block from that instance's own
     stream with numpy's legacy Beta sampler (cmdp_set_reward_streams positions the streams; csrc/cmdp_reward_cache.h)
     and the kernel is relaunched -- inside cmdp_step, cmdp_rollout, cmdp_qlearning_run and cmdp_qlearning_run_logged.
     Needs sp_rp0 / sp_rp1 and the CSR layout; the transition streams are whatever rng_mode says (CMDP_RNG_MT_COMPAT for
     the reference's).  Rollouts run on the lane-per-instance kernel; cmdp_rollout_async is synchronous in this mode. */
  CMDP_FLAG_REWARD_CACHE = 2,
  /* CMDP_RNG_PHILOX with Beta rewards sampled on the device: EVERY Beta(a, b) as Ga / (Ga + Gb) with two Marsaglia-Tsang
     gammas -- the recipe of rounds 1-2.  Without the flag a Beta with a == 1 or b == 1 (nearly every triple of the
     reference's MDP families) is drawn by inverse CDF from one uniform: the same distribution from a tenth of the
     instructions, other numbers.  The flag exists so that earlier runs can be reproduced (csrc/cmdp_device.h philox_beta). */
  CMDP_FLAG_BETA_GAMMAS = 4
};

typedef struct cmdp cmdp_t;

/* Model description handed to cmdp_create.  Either half may be absent (all its pointers NULL):
 * the sampler half is what reset/step/rollout/visits need, the CSR half what the DP entry points
 * need.  Replaces the tables the reference builds in BaseMDP.instantiate_MDP
 * (colosseum/mdp/base.py:463-503) and get_transition_matrix_and_rewards
 * (colosseum/mdp/utils/mdp_creation.py:41-95). */
typedef struct cmdp_desc {
  int32_t n_instances;       /* B >= 1                                                               */
  int32_t n_actions;         /* A >= 1                                                               */
  int32_t horizon;           /* H > 0: episodic (EpisodicMDP.H); 0: continuous                       */
  int32_t rng_mode;          /* CMDP_RNG_*                                                           */
  int32_t layout;            /* CMDP_LAYOUT_*                                                        */
  int32_t flags;             /* CMDP_FLAG_*                                                          */
  double reward_min;         /* BaseMDP.rewards_range, applied as r*(max-min) - min                  */
  double reward_max;         /*   (sic, colosseum/mdp/base.py:1205-1207)                             */
  const int64_t* state_off;  /* [B+1]                                                                */

  /* --- sampler half: NextStateSampler tables in creation order, duplicates kept ---------------- */
  const int64_t* sp_ptr;     /* [R+1] entry offsets, R = state_off[B]*A                              */
  const int32_t* sp_next;    /* [E]   successor state index, local to the instance                   */
  const double*  sp_cum;     /* [E]   itertools.accumulate(probs) within the row                     */
  const double*  sp_reward;  /* [E]   reward of (s,a,s'): the deterministic value (loc)              */
  const uint8_t* sp_rkind;   /* [E]   0 deterministic, 1 Beta(sp_rp0, sp_rp1); NULL = all 0.  Beta entries
                                      need CMDP_FLAG_REWARD_MEANS (report the mean) or CMDP_RNG_PHILOX with
                                      sp_rp0/sp_rp1 (sampled on the device, Philox domain 3)            */
  const double*  sp_rp0;     /* [E]   Beta a (ignored for deterministic entries); may be NULL           */
  const double*  sp_rp1;     /* [E]   Beta b                                                            */
  const int32_t* sp_seed;    /* [R]   seed given to the row's NextStateSampler (MT_COMPAT)           */
  const int64_t* start_off;  /* [B+1]                                                                */
  const int32_t* start_state;/* [NS]  starting states, local index                                   */
  const double*  start_cum;  /* [NS]  accumulated starting probabilities                             */
  const int32_t* start_seed; /* [B]   seed of the start sampler (MT_COMPAT; ignored if one start)    */
  const uint64_t* philox_key;/* [B]   per-instance Philox key (PHILOX)                               */

  /* --- DP half: the non-zeros of the reference's dense float32 T[S,A,S], ascending column ------- */
  const int64_t* csr_ptr;    /* [R+1]                                                                */
  const int32_t* csr_col;    /* [N]   local successor index                                          */
  const float*   csr_val;    /* [N]                                                                  */
  const float*   R;          /* [R]   reward matrix R[s,a]                                           */
} cmdp_desc;

/* ---- library / device -------------------------------------------------------------------------- */
int cmdp_version(void);
/* SHA-256 (hex) over the sources this binary was compiled from (csrc files by name order, then this header), stamped by
   build() through -DCMDP_BUILD_ID; colosseum_amd/_lib.py refuses a library whose id differs from the tree's hash, so a
   stale prebuilt .so cannot pass for the sources next to it.  No reference counterpart. */
const char* cmdp_build_id(void);
const char* cmdp_last_error(void);
/* K1E (csrc/cmdp_k1e.h): 1 when the round of eight episodes e_lo .. e_lo + 7 of a segment of n_steps transitions is INTERIOR
   for a group of n_instances (1 .. 32) instances -- whatever in-episode time in [0, horizon) the segment starts at, all
   eight are walked at full length, none is the segment's first episode and none contains its last transition -- else 0.
   The very predicate k_rollout_epi branches on (such rounds skip the per-chain bookkeeping); needs no handle and no device.
   No reference counterpart. */
int cmdp_k1e_round_interior(int e_lo, int horizon, int64_t n_steps, int n_instances);
/* K1E: the packed step counts n1 | n2 << 11 | n3 << 22 of a 64-bit code word (lo, hi): 32 two-bit reward codes, unused fields
   zero; n_c = fields equal to c.  few != 0: the form k_reward_scan uses for batches with at most three reward codes (valid
   only when no field is 3), else its four-code form.  The very functions the kernel calls; needs no handle and no device.
   No reference counterpart. */
uint32_t cmdp_k1e_code_counts(uint32_t lo, uint32_t hi, int few);
/* K1E: the float64 reward sum of ONE instance over a segment, by the very per-lane code k_reward_scan runs (a wave-uniform
   vote of the kernel is the lane's own predicate here).  words[n_words]: the instance's code words in order -- the segment
   has n_steps transitions and starts h0 steps into an episode of horizon H with nch = ceil(H / 32) words per episode, so
   n_words = ceil((h0 + n_steps) / H) * nch; step j of a chunk at bits 2 j, unused fields zero.  rv[c]: the scaled reward of
   code c < n_codes (<= 4); s0: the sum before the segment.  *sum: s0 + the rewards one by one in float64, in transition
   order.  stats: plain tiles advanced whole, tiles that took the slow path, words added step by step, rebases after them.
   Needs no handle and no device.  No reference counterpart. */
int cmdp_k1e_scan_words(const uint64_t* words, int64_t n_words, int H, int h0, int64_t n_steps, int nch, int n_codes,
                        const double rv[4], double s0, double* sum, int32_t stats[4]);
/* ... with the counters of the scan's SINGLE-VALUE path as well (a tile whose whole advance fails and in which at most one
   code present has a nonzero reward: no code word is searched, see csrc/cmdp_k1e.h, k1r_single).  stats[0..3] as above -- a
   single-value tile counts as a slow tile, its rebases as rebases, and it never counts a word -- stats[4]: tiles resolved on
   the single-value path, stats[5]: the float64 additions it made that left a binade, stats[6]: the additions of its float64
   loop (no integer form, or the value is a tie case), stats[7]: reserved, zero. */
int cmdp_k1e_scan_words_ex(const uint64_t* words, int64_t n_words, int H, int h0, int64_t n_steps, int nch, int n_codes,
                           const double rv[4], double s0, double* sum, int32_t stats[8]);
int cmdp_device_count(void);
int cmdp_set_device(int device);

/* ---- life cycle ------------------------------------------------------------------------------------ */
/* BaseMDP.__init__/instantiate_MDP (colosseum/mdp/base.py:327-503) for B instances at once. */
int cmdp_create(cmdp_t** out, const cmdp_desc* desc);
int cmdp_destroy(cmdp_t* h);
/* Handle's HIP stream (a hipStream_t) so that a caller can time it with HIP events. */
void* cmdp_stream(cmdp_t* h);

/* CMDP_FLAG_REWARD_CACHE: hands over `BaseMDP._rng` (colosseum/mdp/base.py:408) of every instance as
   numpy.random.RandomState.get_state() leaves it after the MDP's construction: mt_key [B][624], mt_pos [B] (0..624),
   has_gauss [B] and cached_gaussian [B] (either may be NULL = 0).  The library continues these streams whenever it
   fills a reward cache.  May be called again to reposition the streams (e.g. a new run on a fresh copy). */
int cmdp_set_reward_streams(cmdp_t* h, const uint32_t* mt_key, const int32_t* mt_pos, const int32_t* has_gauss,
                            const double* cached_gaussian);
/* `RandomState.beta(a, b, n)` on a caller-held stream state (updated in place): numpy's LEGACY sampler
   (numpy/random/src/legacy/legacy-distributions.c: Johnk for a, b <= 1, else Ga / (Ga + Gb) with Marsaglia-Tsang /
   Ahrens-Dieter gammas on the polar Gaussian) -- what scipy.stats.beta(a, b).rvs(n, random_state=rs) draws in
   BaseMDP.sample_reward.  Host only (libm); exists so that the CPU test suite can hold the sampler the reward caches are
   filled with against numpy itself, draw for draw. */
int cmdp_legacy_beta(uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss, double* cached_gaussian, double a, double b,
                     int64_t n, double* out);

/* CMDP_POLICY_RANDOM_REFERENCE: seeds [B]; instance b's action stream becomes numpy.random.RandomState(seeds[b]) as seeding
   leaves it.  Calling it again reseeds. */
int cmdp_set_action_streams(cmdp_t* h, const uint32_t* seeds);
/* The action streams as RandomState.get_state() gives and set_state() takes them: mt_key [B][624], mt_pos [B] (0..624; the
   setter refuses anything else with CMDP_ERR_INVALID).  The setter also creates the streams, like cmdp_set_action_streams. */
int cmdp_action_stream_state(cmdp_t* h, uint32_t* mt_key, int32_t* mt_pos);
int cmdp_set_action_stream_state(cmdp_t* h, const uint32_t* mt_key, const int32_t* mt_pos);
/* `RandomState.randint(0, n_actions, n)` on a caller-held stream state (mt_key [624], *mt_pos; updated in place): out [n].
   n_actions in 1..128 (actions are int8).  Host only, built from the very functions the device generator K16 (csrc/cmdp_actions.h) draws with;
   exists so that the CPU test suite can hold them against numpy itself, action for action. */
int cmdp_mt_randint(uint32_t* mt_key, int32_t* mt_pos, int n_actions, int64_t n, int8_t* out);
/* `RandomState.randint(0, 2, n)` packed as K16 packs it for K1E: action j becomes bit (bit_offset + j) & 31 of word
   (bit_offset + j) >> 5 of out; no other bit of out is changed.  Host only, as cmdp_mt_randint. */
int cmdp_mt_action_bits(uint32_t* mt_key, int32_t* mt_pos, int64_t n, int64_t bit_offset, uint32_t* out);

/* ---- interaction: BaseMDP.reset / BaseMDP.step -------------------------------------------------- */
/* BaseMDP.reset (colosseum/mdp/base.py:1268-1277) on every instance with mask[b] != 0 (all when mask
   is NULL): h = 0, start state sampled, its state-visit count bumped.  obs_out[b] = start state index
   (untouched where masked out); may be NULL. */
int cmdp_reset(cmdp_t* h, const uint8_t* mask, int32_t* obs_out);

/* BaseMDP.step(action, auto_reset) (colosseum/mdp/base.py:1279-1317) on every instance.
   obs[b] = new state index, or -1 when the episode ended (h >= H); step_type: 0 FIRST (an auto-reset
   happened instead of a transition; reward 0), 1 MID, 2 LAST.  With auto_reset == 0 an instance that
   needs a reset makes the call fail with CMDP_ERR_NEEDS_RESET and nothing is modified. */
int cmdp_step(cmdp_t* h, const int32_t* actions, int auto_reset,
              int32_t* obs, double* reward, uint8_t* step_type);

/* The body of MDPLoop.run's loop, env side, fused on the device
   (colosseum/experiment/agent_mdp_interaction.py:238-298): n_steps transitions per instance, each
   episodic termination followed at once by reset() (which is not counted as a step).  Instances must
   have been reset.  last_obs[B], reward_sum[B] (sum of the n_steps rewards) and the three trace
   arrays ([n_steps][B], obs = -1 on termination) may each be NULL. */
int cmdp_rollout(cmdp_t* h, int policy, const void* policy_arg, int64_t n_steps,
                 int32_t* last_obs, double* reward_sum,
                 int32_t* trace_obs, double* trace_reward, uint8_t* trace_type);
/* Same launch without the final synchronisation or any copy-back (for back-to-back timing): CMDP_POLICY_RANDOM or
   CMDP_POLICY_RANDOM_REFERENCE. */
int cmdp_rollout_async(cmdp_t* h, int policy, int64_t n_steps);
int cmdp_synchronize(cmdp_t* h);

/* Measurements taken inside the library (for bench.py's roofline objects; no reference counterpart).
   CMDP_STAT_DP_KERNEL_MS: HIP-event time, on the handle's stream, of the sweep kernel of the last
   cmdp_vi_discounted / cmdp_pe_discounted (kernel only: no upload, no result copy).
   CMDP_STAT_DP_KERNEL: which kernel that was -- 1 K2 (workgroup, CSR in LDS/HBM), 2 K2R, 5 K2U, 7 K2W, 6 K3 (Gauss-Seidel). */
enum { CMDP_STAT_DP_KERNEL_MS = 1, CMDP_STAT_DP_KERNEL = 2,
       CMDP_STAT_REWARD_FILLS = 3,   /* CMDP_FLAG_REWARD_CACHE: blocks of 5000 samples drawn so far                */
       CMDP_STAT_REWARD_ROUNDS = 4,  /* ... and park / fill / relaunch rounds                                        */
       CMDP_STAT_ROLLOUT_KERNEL_MS = 5, /* K1U / K1E: HIP-event time of the rollout kernel (k_rollout_tmpl_stream /
                                           k_rollout_epi) in the last launch of either (last segment)                       */
       CMDP_STAT_HIST_KERNEL_MS = 6,    /* ... and of its second kernel (k_trace_hist / k_reward_scan, the latter on the
                                           second stream unless CMDP_K1E_OVERLAP=0)                                         */
       CMDP_STAT_CHAIN_FAST_INSTANCES = 7 /* instances (evaluated or masked out) the last average-reward call did NOT hand to K9:
                                             those K9F solved (irreducible chain, fill-reducing elimination order); 0 when
                                             that call did not launch K9F (exact order, no plan, K9F beyond the LDS budget) */,
       CMDP_STAT_REWARD_FILL_MS = 8,   /* CMDP_FLAG_REWARD_CACHE: host wall time spent drawing blocks (all host threads together
                                          count once: the time the calling thread waited for the draws)                       */
       CMDP_STAT_REWARD_ROUND_MS = 9   /* ... and wall time of the park rounds as a whole: copy of the park list, draws, install,
                                          up to the relaunch                                                                  */,
       CMDP_STAT_DIAMETER_CLUSTER_LAUNCHES = 10,  /* diameter solves of this handle that ran on K5C (clusters of workgroups per
                                                     group of 64 targets, k_diam_cluster)                                     */
       CMDP_STAT_DIAMETER_CLUSTER_FALLBACKS = 11  /* ... and K5C launches given up because a cluster's workgroups were not all
                                                     resident within the time limit (the targets were then solved by K5S)      */,
       CMDP_STAT_UCRL2_UNCONVERGED = 12, /* UCRL2 agents of this handle: solves that hit max_sweeps (the agent kept its Q)    */
       CMDP_STAT_UCRL2_ROUNDS = 13,      /* ... rounds of parked instances (bounds -> K10 -> model_update, one launch each)   */
       CMDP_STAT_UCRL2_SOLVES = 14,      /* ... instances solved in those rounds (= artificial episodes, the first included)  */
       CMDP_STAT_UCRL2_ROUND_MS = 15     /* ... host wall time from reading a park list to having enqueued its round (and,
                                            with stop_at_episode_end, to the round's completion)                              */,
       CMDP_STAT_UCRL2_WAIT_MS = 16      /* ... host wall time spent waiting for the stream inside cmdp_ucrl2_run's rounds: the
                                            device's share (walk kernel + the previous round's bounds, K10 and update)       */,
       CMDP_STAT_PSRL_ROUNDS = 17,           /* PSRL agents of this handle: rounds of parked instances (sample -> solve -> reset)  */
       CMDP_STAT_PSRL_SOLVES = 18,           /* ... instances solved in those rounds (= episodes, the solve on the prior included) */
       CMDP_STAT_PSRL_SAMPLE_KERNEL_MS = 19, /* ... HIP-event time of the last round's k_psrl_sample (Philox sampler)              */
       CMDP_STAT_PSRL_VI_KERNEL_MS = 20,     /* ... HIP-event time of the last round's k_vi_episodic_dense                         */
       CMDP_STAT_PSRL_REFERENCE_MS = 21      /* ... host wall time spent in the reference sampler's draws, all rounds together     */,
       CMDP_STAT_DIAMETER_KERNEL = 22        /* the kernel of the last cmdp_diameter / cmdp_diameter_range that launched one (0: none
                                                yet), the kernel that produced its results where it returned CMDP_OK.  A call
                                                that fails after its launch (CMDP_ERR_MAX_ITER) sets it too; an empty range
                                                launches nothing and leaves it.  Encoded as family * 1000 + n * 10 + flag:
                                                  1 K2, k_dp_block, one workgroup per target (n = 0; flag 1: CSR in LDS, 0: in HBM)
                                                  2 K3, k_dp_wave_gs, Gauss-Seidel (n = 0, flag = 0)
                                                  3 K5S with fixed-width rows, k_diam_lanes_ell (n = wavefronts per group: 4, 8, 16)
                                                  4 K5S with the generic CSR walker, k_diam_lanes (n = 8)
                                                  5 K5C, k_diam_cluster (n = workgroups per cluster: 8, 16, 32; flag 1: the launch
                                                    that succeeded used XCD-scope barriers, 0: agent-scope barriers)
                                                  6 K5T, k_diam_tiles (n = 6 wavefronts per group)
                                                -- e.g. 3160 = K5S-ELL with 16 wavefronts, 5081 = K5C with clusters of 8 at XCD
                                                scope.  A K5C launch that gave up reports the K5S kernel that solved the targets
                                                instead.  When the workspace limit splits a call into several launches of
                                                different widths, the last launch is reported.  Set on the host; read-only.        */,
       CMDP_STAT_UCRL2_POLICY_KERNEL_MS = 23 /* UCRL2 agents of this handle: HIP-event time of the last K14 launch (the solve of
                                                cmdp_ucrl2_policy / cmdp_ucrl2_average_reward)                                     */,
       CMDP_STAT_PSRL_POLICY_KERNEL_MS = 24  /* PSRL agents of this handle: HIP-event time of the last K15 launch (the solve of
                                                cmdp_psrl_policy / cmdp_psrl_evaluate)                                             */,
       CMDP_STAT_UCRL2_POLICY_SOLVED = 25,   /* UCRL2 agents of this handle: instances K14 has solved for cmdp_ucrl2_policy /
                                                cmdp_ucrl2_average_reward / cmdp_ucrl2_run_logged, all requests together       */
       CMDP_STAT_UCRL2_POLICY_REUSED = 26    /* ... and instances of those requests that kept their stored policy instead
                                                (CMDP_UCRL2_OPT_POLICY_REUSE)                                                     */,
       CMDP_STAT_ACTIONS_KERNEL_MS = 27      /* CMDP_POLICY_RANDOM_REFERENCE on K1E: HIP-event time, on the handle's stream, of K16
                                                (k_mt_actions, the action bits) before the walk CMDP_STAT_ROLLOUT_KERNEL_MS times  */,
       CMDP_STAT_PSRL_UNCONVERGED = 28,      /* continuous PSRL agents of this handle (K13): solves that reached max_sweeps; the
                                                actor then holds the last sweep's Q                                                */
       CMDP_STAT_PSRL_SWEEPS = 29            /* ... sweeps of the last round's solves, summed over its instances                  */,
       CMDP_STAT_PSRL_SAMPLE_BYTES = 30,     /* optimistic PSRL agent of this handle (K18 / K19): device bytes its sample routes hold
                                                -- pmk and bump, T_ext and its upload (dense), the posterior blocks (compact)    */
       CMDP_STAT_PSRL_SAMPLE_SOLVER = 31     /* ... the route of its last round (CMDP_PSRLC_OPT_SAMPLE_SOLVER), whose kernels
                                                CMDP_STAT_PSRL_SAMPLE_KERNEL_MS and CMDP_STAT_PSRL_VI_KERNEL_MS time               */ };
/* The UCRL2 and PSRL statistics belong to the environment handle: agents created on the same handle share them. */
int cmdp_stat(cmdp_t* h, int which, double* out);
/* Latency floor of the LDS-resident rollout kernels, measured on the current device: one wavefront per CU follows
   per-lane uint16 tables in LDS for n_steps dependent reads.  CMDP_CALIB_LDS_READ: the bare dependent ds_read_u16
   (read, mask, address); CMDP_CALIB_LDS_CHAIN: the minimal dependency chain of one deterministic transition (action
   bit, successor read, mask, in-episode step, episode-end select); CMDP_CALIB_LDS_CHAIN_SHARED: the same for the
   shared-table kernel K1T (the state's word pair and its swap bit: two independent reads, the word selected by a bit-field
   extract).  ns_per_step = launch time / n_steps. */
enum { CMDP_CALIB_LDS_READ = 0, CMDP_CALIB_LDS_CHAIN = 1, CMDP_CALIB_LDS_CHAIN_SHARED = 2 };
int cmdp_calibrate(int what, int64_t n_steps, double* ns_per_step);

/* Tuning knobs (never change results).  CMDP_OPT_ROLLOUT_KERNEL: 0 = automatic, 1 = lane-per-instance
   kernel with the tables in HBM, 2 = LDS-resident kernel (fails with CMDP_ERR_UNSUPPORTED when the batch is
   not eligible: deterministic dynamics, one start state, equal state counts <= 65535, <= 256 distinct reward
   values, at least 8 instances per 160 KiB of LDS), 3 = LDS-resident kernel for STOCHASTIC dynamics K1S (Philox mode;
   the sampler tables compressed into shared cumulative-probability patterns and per-state successor sets: <= 16
   entries per row, <= 16 distinct successors per state, <= 64 patterns, rewards a function of the successor or of
   the row, at least 4 instances per 160 KiB of LDS), 4 = the shared-table pipeline K1T (a batch eligible for 2 with two
   actions whose instances are, state by state, the first instance's rows or their swap -- the seeds of a family whose
   structure does not depend on the seed: the workgroup keeps one successor table and a swap bit per state and
   instance, 128 instances per CU at config C2 instead of 52; taken automatically when eligible, 2 keeps K1L / K1P),
   5 = K1U, K1T's chain with the 16-bit trace streamed to HBM and histogrammed by a second kernel instead of 8-bit count
   deltas in LDS: up to 256 instances per CU resident at once (taken automatically when that saves a round of workgroups
   over K1T -- config C2: one round instead of two; 4 keeps K1T),
   6 = K1E, the EPISODE-PARALLEL rollout (a batch eligible for 2 that is episodic, has two actions, at most four distinct
   reward values and at most 512 states per instance): lane = (instance, episode) -- under the random policy the episodes
   of an instance are independent (fixed horizon, one start state: colosseum/mdp/base.py:1268-1277,1310-1317; the action
   of transition n is a function of (key, n)), so a launch is walked as H-step chains, 4 096 of them per CU, against
   private {successor | count} tables in LDS; the float64 reward sums are added in transition order by a second kernel
   from 2-bit reward codes.  Taken automatically when eligible (launches of >= 64 transitions); 5 / 4 / 2 keep the
   chain kernels.
   For 3: the automatic choice takes it while the batch is small enough that
   the HBM-table kernel's rate, which grows with the batch, stays below it -- FrozenLake 20x20: up to ~35 000 instances).
   CMDP_OPT_DP_KERNEL (Jacobi sweeps): 0 = automatic, 1 = workgroup kernel with the CSR in LDS or HBM,
   2 = register-resident CSR kernel (CMDP_ERR_UNSUPPORTED when no compiled shape fits: A in 2..4, <= 8
   non-zeros per row, <= 1024 states), 3 = (cmdp_diameter only) the 64-targets-per-workgroup kernel K5S that is
   otherwise taken when the value vector of an instance does not fit LDS (4 = the same with its generic CSR walker
   instead of the fixed-width-row variant; 6 = its tiled form K5T, which gathers the value rows of a cluster of states
   into LDS first: half the HBM traffic, same bits, not faster -- on request only), 5 = the distinct-successor form K2U of the register-resident kernel (taken
   by default when the A rows of a state share their successors: <= 8 distinct columns per state, rows in ascending
   column order; 2 keeps the per-row form K2R), 7 = K2W, K2U's tables with ONE wavefront per instance and no barrier per
   sweep (taken by default for 257..448 states, <= 5 distinct successors per state, <= 4 non-zeros per row; 5 keeps K2U).
   All forms return identical bits.
   CMDP_OPT_CHAIN_EXACT_ORDER (cmdp_average_reward / cmdp_qlearning_average_reward): 1 = every float64 sum of the GTH
   elimination in the reference's index order and the states eliminated in the reference's order (bit-equal to cmdp_gth
   and the oracle, one serial chain per sum);
   0 (default) = wave butterfly sums and -- for irreducible chains -- a fill-reducing elimination order computed once per
   instance from the MDP's transition graph, several independent pivots per step (kernel K9F): deterministic, within
   ~1e-13 relative of the former (GTH is subtraction-free: any elimination order gives the stationary distribution to
   rounding), 5-8 x faster on chains with hundreds of states.
   CMDP_OPT_DIAMETER_WORKSPACE_MB: HBM the value arrays of K5S may take per launch (default 24576; 512 bytes per
   state per group of 64 targets; more groups in flight = more of the GPU busy).
   CMDP_OPT_DIAMETER_RELABEL_MIN_STATES: K5S stores the rows of instances with at least this many states (default 8192)
   in a locality order of the states (breadth-first clusters of the transition graph) so that the value rows a chunk of
   states gathers were fetched by the chunks before it; row contents and entry order are unchanged, results bit-equal.
   A value above every instance's size keeps the caller's state order.
   CMDP_OPT_MIXING_PATH (cmdp_mixing_time): 0 = automatic (matrix powers when an instance has more than 1024 states or
   a float64 row does not fit LDS), 1 = matrix powers, 2 = one sparse step at a time with the row in LDS.
   CMDP_OPT_LDS_GROUPS_PER_CU: 1 or 2 workgroups of the fused-walker kernel K1L per CU (default: whichever needs
   fewer rounds of workgroups for the batch).  Setting it re-plans the handle onto K1L with the
   balanced number of instances per workgroup for that many groups (the pipeline kernel K1P always runs one workgroup
   per CU); CMDP_ERR_INVALID when the batch is not eligible for the LDS-resident kernels or two groups do not fit. */
enum { CMDP_OPT_ROLLOUT_KERNEL = 1, CMDP_OPT_DP_KERNEL = 2, CMDP_OPT_LDS_GROUPS_PER_CU = 3,
       CMDP_OPT_DIAMETER_WORKSPACE_MB = 4, CMDP_OPT_CHAIN_EXACT_ORDER = 5, CMDP_OPT_MIXING_PATH = 6,
       CMDP_OPT_DIAMETER_RELABEL_MIN_STATES = 7 };
int cmdp_set_option(cmdp_t* h, int option, int64_t value);

/* What the LDS-resident random-policy rollout of this handle is (introspection for benchmarks and tests; no
   reference counterpart): plan[0] = 1 if the batch is eligible for it, plan[1] = 1 for the wavefront-pipeline kernel
   K1P (k_rollout_pipe), 0 for the fused walker K1L (k_rollout_lds), 2 for the stochastic-dynamics kernel K1S
   (k_rollout_stoch), 3 for the shared-table pipeline K1T (k_rollout_tmpl), 4 for its streamed-trace form K1U
   (k_rollout_tmpl_stream + k_trace_hist), plan[2] = instances per workgroup,
   plan[3] = transitions per chunk.  The kernel flavour and chunk length are chosen when the handle is created (fewest
   rounds of workgroups x measured time per transition). */
int cmdp_lds_plan(cmdp_t* h, int32_t plan[4]);

/* The plan of the stochastic-dynamics rollout K1S (csrc/cmdp_k1s.h) that cmdp_create made for this handle (introspection for
   tests; makes no HIP call; no reference counterpart).  out, in this order: ok (1 when the batch is eligible for K1S: every
   other field is 0 otherwise), G (instances per workgroup), nw (walker wavefronts), gw (instances per walker wavefront), team
   (lanes per instance), U (successor-set slots per state), n_pat (cumulative-probability patterns), n_codes (distinct reward
   values), reward_mode (0: the reward is a function of the successor state, 1: of the row), rc_packed (mode 0: the code
   travels in the successor-set entries, no per-state table), n_shapes (row shapes), shape_bytes (1 or 2 per row), ch
   (transitions per chunk), form (the compiled form of the walk loop the kernel's dispatch takes: 0 the generic form, else
   team * 4 + reward source for the nine specialised ones -- one pattern, one shape byte, team 16 / 8 / 1; source 0: packed
   code, 1: per-state table, 2: per row -- computed by the very function the kernel branches on).
   The environment variable CMDP_K1S_G, read by cmdp_create like CMDP_K1T_G and CMDP_K1U_G, sets G to min(LDS capacity, value);
   nw, gw and team follow from G as they do for a planned G. */
#define CMDP_K1S_PLAN_FIELDS 14
int cmdp_k1s_plan(cmdp_t* h, int32_t out[CMDP_K1S_PLAN_FIELDS]);
/* The same for a bare description, without a handle and without a device: what cmdp_create would plan for `desc` on a device
   of `cus` compute units (only the sampler half is read; philox_key and the seeds are not).  instances_per_workgroup: 0 for
   the planned G, else what CMDP_K1S_G would be set to (the environment is not read).  CMDP_ERR_INVALID for a description
   cmdp_create would reject before planning (offsets, successor indices, row lengths). */
int cmdp_k1s_plan_desc(const cmdp_desc* desc, int cus, int instances_per_workgroup, int32_t out[CMDP_K1S_PLAN_FIELDS]);

/* The plans of the deterministic LDS-resident rollouts K1L / K1P, K1T and K1U that cmdp_create made for this handle
   (introspection for tests; makes no HIP call; no reference counterpart).  The fields of a kernel the batch is not eligible
   for are 0.  out, in this order:
     K1L / K1P [0..12]   ok, pipe (1: K1P), packed (reward code in the successor word), code_shift, succ_bits (bits of a row
                         base), n_codes (distinct reward values), ch (transitions per chunk), G (instances per workgroup),
                         per_cu (workgroups per CU of the chosen candidate), capacity (instances per workgroup that fit LDS at
                         that candidate, at most 64), slot_bytes, lds_bytes (of a workgroup of G), form (0: k_rollout_lds<false>,
                         1: k_rollout_lds<true>, 2: k_rollout_pipe)
     K1T [13..20]        ok, automatic (the automatic choice prefers it to K1L / K1P), ch, G, capacity (at most 128), slot_bytes,
                         tmpl_bytes, lds_bytes
     K1U [21..29]        ok, automatic (... prefers it to K1T), pack10, ch, G, capacity (at most 256), lds_bytes (of the chain
                         kernel), hist_lds_bytes (of the histogram kernel, static arrays included), form (0: the PACK10 kernels, 1: the wide trace)
   The two `form` fields are computed by the functions the launchers branch on.
   Environment read by cmdp_create, for tests: CMDP_K1L_G=n sets G of K1L / K1P to min(capacity, n) at the candidate the
   planner chose; CMDP_K1T_CH=64|32|16 plans K1T at that chunk length only (not eligible when it has no room).  Neither
   changes a result. */
#define CMDP_DET_PLAN_FIELDS 30
int cmdp_det_plan(cmdp_t* h, int32_t out[CMDP_DET_PLAN_FIELDS]);
/* The same for a bare description on a device of `cus` compute units, without a handle and without a device (only the
   sampler half is read; the environment is not).  knobs[5] stand for CMDP_K1L_PIPE, CMDP_K1L_G, CMDP_K1T_G, CMDP_K1U_G and
   CMDP_K1T_CH, 0 or -1 each for "planned" (pipe: -1 for planned, 0 K1L only, 1 K1P only); NULL: all planned.
   CMDP_ERR_INVALID as for cmdp_k1s_plan_desc. */
int cmdp_det_plan_desc(const cmdp_desc* desc, int cus, const int32_t knobs[5], int32_t out[CMDP_DET_PLAN_FIELDS]);

/* The PAIR plan of the episode-parallel rollout K1E (csrc/cmdp_k1e_pair.h, plan_k1e_pair in csrc/cmdp_rollout_plan.h) that
   cmdp_create made for this handle (introspection for tests; makes no HIP call; no reference counterpart): the walk of a
   launch of whole episodes from reset takes two transitions per step, on a table with one row per (state at an even in-episode
   time, action pair).  out, in this order: ok (1 when the batch is eligible for K1E, its horizon is even, every instance has at
   most SP2 even-time states and four images of SP2 x 128 B plus the action-bit rings fit LDS -- and CMDP_K1E_PAIR is not 0; the
   next four fields are 0 otherwise), H, SP2 (rows of an image: a power of two >= 32), n_even (the largest number of even-time
   states of an instance), lds_bytes (of a workgroup), last_form (the form the last K1E launch of the handle took: 0 none yet,
   1 single, 2 pair).  A launch takes the pair form when ok, every instance is at its start state with in-episode time 0
   (after an unmasked cmdp_reset, or after rollouts of multiples of H transitions since), n is a multiple of H, the policy is
   random without trace and bit 16 of CMDP_K1E_DEBUG is clear; results are those of the single form.
   The environment variable CMDP_K1E_PAIR, read by cmdp_create, 0: every launch takes the single form. */
#define CMDP_K1E_PAIR_PLAN_FIELDS 6
int cmdp_k1e_pair_plan(cmdp_t* h, int32_t out[CMDP_K1E_PAIR_PLAN_FIELDS]);
/* The same for a bare description on a device of `cus` compute units, without a handle and without a device (only the sampler
   half is read; the environment is not; last_form is 0), and the tables of instance `instance` (each pointer may be NULL;
   nothing is written to them when ok is 0): *n_even its number of even-time states; index [S]: the compact index of every
   state, -1 for a state that is no even-time state (the start state has index 0); inverse [SP2]: the state of every compact
   index, -1 past n_even; words [SP2][4]: the pair words, pair q = a0 | a1 << 1 of row x at words[4 x + q] =
   index(s'') << 7 | code(s, a0) | code(s', a1) << 2 with s' = next(s, a0), s'' = next(s', a1), the successor field 0 where s''
   is no even-time state; rows past n_even are 0.  The reward codes are indices into the distinct reward values in order of
   first appearance over the rows of the batch.  CMDP_ERR_INVALID as for cmdp_k1s_plan_desc. */
int cmdp_k1e_pair_plan_desc(const cmdp_desc* desc, int cus, int instance, int32_t out[CMDP_K1E_PAIR_PLAN_FIELDS], int32_t* n_even,
                            int32_t* index, int32_t* inverse, uint16_t* words);

/* K9F's plan (csrc/cmdp_chain_plan.h; the arrays are ChainFast's of csrc/cmdp_chain.h) for a bare description, without a
   handle and without a device: what the first cmdp_average_reward call on a handle of `desc` uploads (introspection for
   tests; only the DP half is read; no reference counterpart).  The caller sizes the arrays: rank and piv [state_off[B]],
   cptr and rptr [state_off[B] + B] (rptr: the round offsets of the planned instances, packed; the rest is left as it is),
   cbase, rbase and nrounds [B] (nrounds -1: no plan, the instance keeps K9), cand [cand_capacity].  *n_cand receives the
   number of entries of cand; CMDP_ERR_INVALID when cand_capacity is smaller, and for a description cmdp_create would
   reject before planning (offsets, column indices). */
int cmdp_chain_plan_desc(const cmdp_desc* desc, int32_t* rank, int32_t* cptr, int64_t* cbase, uint16_t* cand, int64_t cand_capacity,
                         int64_t* n_cand, int32_t* nrounds, int64_t* rbase, int32_t* rptr, int32_t* piv);
/* Which kernels a cmdp_average_reward call launches for a batch whose largest instance has max_S states and whose longest row
   max_row_nnz entries (host only).  exact_order: CMDP_OPT_CHAIN_EXACT_ORDER; fast_enabled: 0 stands for CMDP_CHAIN_FAST = 0
   (the environment is not read); any_plan: some instance has a K9F plan.  out: the refusal (CMDP_OK, or CMDP_ERR_UNSUPPORTED
   when not even K9 fits LDS), K9's dynamic LDS bytes, 1 if K9F runs first, K9F's LDS bytes. */
int cmdp_chain_choice(int max_S, int max_row_nnz, int exact_order, int fast_enabled, int any_plan, int64_t out[4]);

/* BaseMDP.get_visitation_counts / reset_visitation_counts (colosseum/mdp/base.py:1357-1382).
   state_counts [state_off[B]], sa_counts [state_off[B]*A]; either may be NULL. */
int cmdp_visits(cmdp_t* h, int64_t* state_counts, int64_t* sa_counts);
int cmdp_reset_visits(cmdp_t* h);
/* Restores the counters (e.g. of an earlier run that is being continued: the reference's MDPs are pickled with their
   counts).  Either array may be NULL (left as it is); every value must fit the device's int32 counters.  The device
   counters are int32: the library keeps an upper bound of what any of them can hold (largest restored value + two per
   transition taken since -- an arrival and, at an episode end, the reset) and refuses a call that could carry one past
   2^31 - 1 with CMDP_ERR_OVERFLOW, before anything is stepped. */
int cmdp_set_visits(cmdp_t* h, const int64_t* state_counts, const int64_t* sa_counts);
/* Current state index, in-episode step and needs-reset flag of every instance (BaseMDP.cur_node,
   .h, .necessary_reset); each may be NULL. */
int cmdp_state(cmdp_t* h, int32_t* cur, int32_t* hstep, uint8_t* needs_reset);
/* BaseMDP.last_starting_node as a state index: the state the latest reset() of every instance sampled [B], and
   (nullable) the one the reset before it sampled -- MDPLoop evaluates a log row BEFORE the reset that follows a
   terminating step, while the fused kernels reset at once. */
int cmdp_last_start(cmdp_t* h, int32_t* last_start, int32_t* previous_start);

/* ---- dynamic programming ---------------------------------------------------------------------------- */
/* discounted_value_iteration (colosseum/dynamic_programming/infinite_horizon.py:14-44,121-164).
   R_override ([R] or NULL) replaces the reward matrix (e.g. -R for the worst policy).  Q [R], V
   [state_off[B]], sweeps [B] (sweeps executed, including the converging one); sweeps may be NULL.
   max_abs_value <= 0 disables the bound. */
int cmdp_vi_discounted(cmdp_t* h, float gamma, double epsilon, int scheme, int64_t max_sweeps,
                       double max_abs_value, const float* R_override,
                       float* Q, float* V, int64_t* sweeps);
/* discounted_policy_evaluation (infinite_horizon.py:47-64,167-205); pi [R] float32. */
int cmdp_pe_discounted(cmdp_t* h, const float* pi, float gamma, double epsilon, int scheme,
                       int64_t max_sweeps, const float* R_override,
                       float* Q, float* V, int64_t* sweeps);
/* episodic_value_iteration / episodic_policy_evaluation
   (colosseum/dynamic_programming/finite_horizon.py:11-42).  Q of instance b is [H+1][S_b][A] at
   offset (H+1)*state_off[b]*A, V is [H+1][S_b] at (H+1)*state_off[b]; pi is [H][S_b][A] at
   H*state_off[b]*A. */
int cmdp_vi_episodic(cmdp_t* h, int H, const float* R_override, float* Q, float* V);
int cmdp_pe_episodic(cmdp_t* h, int H, const float* pi, const float* R_override, float* Q, float* V);

/* ---- hardness measures --------------------------------------------------------------------------- */
/* get_diameter, continuous setting (colosseum/hardness/measures/diameter.py:76-106): for every
   target state es the optimal expected hitting time by value iteration with es absorbing, R = -1,
   gamma = 1; diameter[b] = max over targets and start states.  per_target [state_off[B]] may be
   NULL.  scheme as in cmdp_vi_discounted (AUTO = the rule applied to the instance's T). */
int cmdp_diameter(cmdp_t* h, double epsilon, int scheme, int64_t max_sweeps,
                  float* per_target, float* diameter);
/* `_get_sparse_diameter` (colosseum/hardness/measures/diameter.py:382-420): the variant a single-core reference runs
   for continuous MDPs above 1000 states (dispatch :35-39) -- float64 hitting times, targets in index order, and the
   running-maximum early exit `diff < 0.05 and max - 1 < diameter so far`, which makes the value depend on that order.
   The device solves every target to diff < epsilon and logs (diff, max) per sweep; the host replays the reference's
   sequential loop on the logs, so the committed values are the reference's.  diameter [B] float64; running_max
   [state_off[B]] (may be NULL) = the running maximum after each target.  Continuous handles only. */
int cmdp_diameter_sparse_f64(cmdp_t* h, double epsilon, int64_t max_sweeps, double* running_max, double* diameter);
/* The per-target hitting-time solves of cmdp_diameter for the targets [target_lo, target_hi) of the flat state
   space [0, state_off[B]) only (Jacobi scheme, kernel K5S; any instance size): per_target[i] belongs to target
   target_lo + i.  This is how config C5 (one MDP with ~50 000 states) is split over GPUs: every rank takes a
   contiguous range of targets and the diameter is the maximum over all ranks
   (colosseum/hardness/measures/diameter.py:108-124 does the same with a process pool). */
int cmdp_diameter_range(cmdp_t* h, double epsilon, int64_t max_sweeps, int64_t target_lo, int64_t target_hi,
                        float* per_target);
/* get_diameter, episodic setting (colosseum/hardness/measures/diameter.py:193-234,285-318) on the
   time-augmented transition array of get_episodic_transition_matrix_and_rewards
   (colosseum/mdp/utils/mdp_creation.py:98-128), which is never materialised: H, the starting states
   (start_off [B+1], start_state [NS], start_prob [NS] as float32) and the CSR define it.  Every target
   runs to diff < epsilon; the reference's running-maximum early exit (order dependent) is not applied.
   per_target [state_off[B]] may be NULL. */
int cmdp_diameter_episodic(cmdp_t* h, int H, const int64_t* start_off, const int32_t* start_state,
                           const float* start_prob, double epsilon, int64_t max_sweeps,
                           float* per_target, float* diameter);
/* calculate_norm_discounted (colosseum/hardness/measures/value_norm.py:83-87). V [state_off[B]]. */
int cmdp_value_norm(cmdp_t* h, const float* V, float* out);

/* ---- agents on the device --------------------------------------------------------- */
/* Batched tabular Q-learning with UCB exploration for episodic MDPs: one agent per environment instance of `env`,
   reproducing colosseum/agent/agents/episodic/q_learning.py (QLearningEpisodic: QValuesModel.step_update + the
   greedy QValuesActor with its RandomState(seed) tie-break) bit for bit.  seeds [B]; ucb_type 0 = hoeffding,
   1 = bernstein (c_2 required). */
typedef struct cmdp_agent cmdp_agent_t;
int cmdp_qlearning_create(cmdp_agent_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon,
                          double p, double c_1, double c_2, double min_at, int ucb_type);
int cmdp_qlearning_destroy(cmdp_agent_t* a);
/* The continuous-setting agent, colosseum/agent/agents/infinite_horizon/q_learning.py (QLearningContinuous: optimistic
   Q-learning for the average-reward setting) on a continuous environment handle; get_span_approx / get_H are the
   reference defaults.  The returned handle is used with the same cmdp_qlearning_run / _tables / _destroy. */
int cmdp_qlearning_continuous_create(cmdp_agent_t** out, cmdp_t* env, const int32_t* seeds,
                                     int64_t optimization_horizon, double min_at, double confidence,
                                     double span_approx_weight, double h_weight);
/* MDPLoop.run's loop with the agent in it (colosseum/experiment/agent_mdp_interaction.py:238-298): per step
   select_action -> BaseMDP.step -> step_update -> reset() at the end of an episode.  train_mask [B] (NULL = all
   ones): instances with 0 act but do not update, as after MDPLoop froze their training (:284-288).
   cumulative_reward [B] receives `MDPLoop._cumulative_reward`, the running float64 sum of ALL rewards since the agent
   was created (the additions continue across calls in transition order).  actions_trace [n_steps][B] may be NULL. */
int cmdp_qlearning_run(cmdp_agent_t* a, int64_t n_steps, const uint8_t* train_mask, int8_t* actions_trace,
                       double* cumulative_reward);
/* MDPLoop.run as ONE call (colosseum/experiment/agent_mdp_interaction.py:179-302 with its indicator code :304-578 and
   colosseum/experiment/indicators.py:29-45): the interaction of cmdp_qlearning_run, and at every logging step the
   evaluation of the agents' greedy policies on the device (episodic: V[0] by policy evaluation; continuous: average reward
   of the policy's chain from the current state) followed by the reference's 18 performance indicators, computed on the
   host in C++ with the reference's numpy scalar types (csrc/cmdp_tracker.h), the `_is_policy_optimal` freeze of training
   and the wall-clock limit -- one stream synchronisation per logging step, no Python in between.

   desc: n_steps = T, log_every (<= 0: only the final row), n_check = n_log_intervals_to_check_for_agent_optimality,
   max_time (seconds of training for the batch; the reference gives every instance its own process and clock: here all
   instances still training are frozen at the first logging step after max_time - 0.5 s); base_val / base_kind [B][3]: the
   optimal, worst and random average reward of every instance as Python / numpy scalars (kind 0 = Python float, 1 =
   np.float32, 2 = np.float64); episodic
   handles also need horizon, opt0 / worst0 (V*[0] and V_worst[0], flat [state_off[B]]) and the start distribution as
   start_pos / start_prob [B][kmax] (flat state positions in state-index order, probability 0 for padding).
   Outputs for the n_logs = len(range(log_every, T, log_every)) + 1 rows: steps [n_logs]; values / kinds
   [n_logs][CMDP_LOG_COLUMNS][B] -- the columns are the indicator names in sorted order without "steps" (kind 1 =
   np.float32, 2 = np.float64; the values are rounded to 5 decimals in their type, as the logger receives them);
   last_training_step [B] (-1: the time limit was not hit); is_training [B] after the run (these two may be NULL). */
#define CMDP_LOG_COLUMNS 17
typedef struct cmdp_loop_desc {
  int64_t n_steps, log_every;
  int32_t n_check, horizon, kmax, reserved;
  double max_time;
  const double* base_val;
  const int32_t* base_kind;
  const float* opt0;
  const float* worst0;
  const int64_t* start_pos;
  const double* start_prob;
} cmdp_loop_desc;
int cmdp_qlearning_run_logged(cmdp_agent_t* a, const cmdp_loop_desc* desc, int64_t n_logs, int64_t* steps, double* values,
                              uint8_t* kinds, int64_t* last_training_step, uint8_t* is_training);
/* What cmdp_qlearning_run_logged does on the host at every row (csrc/cmdp_logged_loop.h), on caller-supplied inputs
   (host only, no device): per row the step, whether it lies inside the loop (the final row does not run the freeze
   check), the steps since the previous row, cumulative rewards [n_logs][B], and -- episodic: V0 [n_logs][state_off[B]] of
   the policies and the logged episode's start state [n_logs][B] (instance-relative); continuous: avg / avg_kind
   [n_logs][B] (kind != 0: np.float32).  is_training [n_logs][B] receives the flags after every row.
   With log_steps, in_loop and n_since all NULL the rows are those of cmdp_qlearning_run_logged for desc->n_steps and
   desc->log_every, and an n_logs that is not their number is CMDP_ERR_INVALID, as there.  Every row is also held to the
   rule by which the loop starts an interval before the previous row's result is known: inputs that freeze an instance at
   a row the rule lets run ahead fail with CMDP_ERR_HIP.  For tests against the reference's indicator code. */
int cmdp_tracker_replay(const cmdp_loop_desc* desc, int32_t B, int32_t episodic, const int64_t* state_off, int64_t n_logs,
                        const int64_t* log_steps, const uint8_t* in_loop, const int64_t* n_since, const double* cum_reward,
                        const float* V0, const int64_t* start_state, const double* avg, const int32_t* avg_kind,
                        double* values, uint8_t* kinds, uint8_t* is_training);
/* V[0, :] of episodic_policy_evaluation for the agents' current greedy policies
   (BaseAgent.current_optimal_stochastic_policy = argmax_3d(Q), ties by RandomState(42)): what
   MDPLoop._compute_episodic_regret needs.  The environment handle must carry the DP half.  V0 [state_off[B]]. */
int cmdp_qlearning_evaluate(cmdp_agent_t* a, float* V0);
/* argmax_2d (colosseum/dynamic_programming/utils.py:12-25) of the continuous agents' Q tables: one-hot float32
   policies pi [state_off[B]*A] (BaseAgent.current_optimal_stochastic_policy). */
int cmdp_qlearning_policy(cmdp_agent_t* a, float* pi);
/* BaseMDP-side `get_average_reward(T, R, policy, [(state, 1.0)])` (colosseum/mdp/utils/markov_chain.py:12-31, the
   regret of every continuous-setting log row, agent_mdp_interaction.py:518-532) for the agents' current greedy
   policies from the environments' current states, all on the device: recurrent classes in networkx's
   attracting_components order, GTH elimination of the class taken, numpy's summation order.  avg[b] is the value;
   kind[b] = 1 when the reference's result is a numpy float32 (one recurrent class smaller than the chain), else 0
   (float64).  mask [B] selects the instances to evaluate (NULL = all; the others' outputs are left untouched). */
int cmdp_qlearning_average_reward(cmdp_agent_t* a, const uint8_t* mask, double* avg, int32_t* kind);
/* argmax_3d (colosseum/dynamic_programming/utils.py:28-39) of host tables Q [per instance q_layers*S_b*A, q_layers
   >= H]: one-hot float32 policy of the first H layers, pi [per instance H*S_b*A]. */
int cmdp_greedy_policy_episodic(cmdp_t* h, int H, int q_layers, const float* Q, float* pi);
/* Q [B instances concatenated: H*S_b*A float32 each for the episodic agent; S_b*A FLOAT64 each -- pass a double* --
   for the continuous agent, whose tables are float64], N likewise (int32); either may be NULL. */
int cmdp_qlearning_tables(cmdp_agent_t* a, float* Q, int32_t* N);

/* ---- non-tabular observations --------------------------------------------------------------------------------- */
/* EmissionMap.all_observations (colosseum/emission_maps/base.py:56-83) of every instance: float32 feature vectors of
   length F, per instance [S_b][F] at state_off[b]*F, or -- time_indexed, episodic handles -- [H][S_b][F] at
   H*state_off[b]*F.  The table is copied to the device. */
int cmdp_set_observation_table(cmdp_t* h, const float* table, int32_t F, int time_indexed);
/* EmissionMap.get_observation (emission_maps/base.py:110-141) for the current state of every instance: obs [B][F];
   all zeros for an episodic instance that has reached its horizon.  noise_scale > 0 adds scale * N(0,1) per element
   from the instance's Philox stream (throughput mode, CMDP_RNG_PHILOX only; the reference-exact GaussianUncorrelated
   stream is numpy's and stays on the host, colosseum_amd/emission_maps.py). */
int cmdp_observe(cmdp_t* h, double noise_scale, float* obs);
/* The same with any of the reference's four noise classes (the files of colosseum/noises/) in throughput mode: Gaussian
   (scale), Gaussian correlated (y = L z, chol = the lower Cholesky factor L [F][F] of the covariance -- the reference
   draws it from a Wishart distribution once per MDP), Student-t (df) and the multivariate Student-t (chol = factor of
   the shape matrix, df).  Philox mode only; distribution-exact, not stream-exact (the reference-exact streams are
   numpy's / scipy's and stay on the host, colosseum_amd/emission_maps.py: CompatNoise). */
enum { CMDP_NOISE_NONE = 0, CMDP_NOISE_GAUSSIAN = 1, CMDP_NOISE_GAUSSIAN_CORRELATED = 2, CMDP_NOISE_STUDENT_T = 3,
       CMDP_NOISE_STUDENT_T_CORRELATED = 4 };
int cmdp_observe_noise(cmdp_t* h, int kind, double scale, double df, const float* chol, float* obs);

/* ---- Markov chains ------------------------------------------------------------------------------------ */
/* BUILD-DEFINED (the reference has no mixing time): t_mix[b] = smallest t >= 1 with
   max_s TV(P^t(s, .), stationary) <= threshold for the chain P[s, j] = sum_a pi[s, a] T[s, a, j] of instance b, rows
   normalised to sum to one in float64 (float32 probabilities sum to 1 only within ~1e-7, which would leak 1e-2 of mass
   over the 1e5 steps a slow chain needs); pi [state_off[B]*A] float32, NULL = the uniform policy; stationary
   [state_off[B]] float64, e.g. from cmdp_gth on the same normalised chain;
   float64 on the device; -1 when max_steps is reached first (periodic chains never get there).  tv_at [B] (may be
   NULL) receives the total variation at t_mix (or at the last t evaluated).  Parity unpinned by construction.
   Two paths (CMDP_OPT_MIXING_PATH).  Stepping: the S rows of X_t = P^t advance one sparse step at a time, row in LDS
   (S <= ~20 000).  Matrix powers, for large chains (config C5, S = 50 272): X is a dense S x S float64 matrix in HBM
   (20 GB at C5); since max_s TV is non-increasing in t, A_k = P^(2^k) is squared (rocBLAS dgemm) until 2^K is mixed,
   a binary search multiplies the stored powers back in, one dgemm per bit, and the last 2^r steps -- r = the lowest
   power still held when HBM ran out of S x S buffers -- are sparse steps that gather from the row in global memory.
   The two paths round differently (1e-16 relative per product) and return the same t unless the total variation
   crosses the threshold within that distance. */
int cmdp_mixing_time(cmdp_t* h, const float* pi, const double* stationary, double threshold, int64_t max_steps,
                     int64_t* t_mix, double* tv_at);
/* get_average_reward (colosseum/mdp/utils/markov_chain.py:12-31) of deterministic stationary policies: actions
   [state_off[B]] gives the action of every state of every (continuous, horizon 0) instance, start_states [B] the
   instance-relative state the chain starts from.  Outputs as cmdp_qlearning_average_reward; n_classes [B] (may be
   NULL) receives the number of recurrent classes of each chain.  CMDP_ERR_UNSUPPORTED when an instance exceeds the
   kernel's LDS budget (80 bytes per state + 4 per successor). */
int cmdp_average_reward(cmdp_t* h, const int32_t* actions, const int32_t* start_states, const uint8_t* mask, double* avg,
                        int32_t* kind, int32_t* n_classes);
/* _gth_solve_numba (colosseum/mdp/utils/markov_chain.py:139-166): stationary distributions of `count` chains with a
   single recurrent class each, float64 GTH elimination on the current device.  Chain m is the dims[m] x dims[m]
   row-major matrix at mats + sum_{i<m} dims[i]^2 (not modified); its distribution goes to
   out + sum_{i<m} dims[i]. */
int cmdp_gth(int count, const int32_t* dims, const double* mats, double* out);

/* extended_value_iteration (colosseum/dynamic_programming/infinite_horizon.py:67-118, _max_proba at :222-251), the
   optimistic solver of UCRL2, for `count` estimated models at once on the current device; one launch runs every
   instance to convergence or to max_sweeps.  Instance b has n_states[b] <= 4096 states and n_actions[b] actions; its
   S*A rows follow those of the instances before it, its states likewise.  Rows: csr_ptr [n_rows + 1] (csr_ptr[0] = 0)
   into csr_col (instance-relative successors, ascending within a row) and csr_val (float32 T[s, a, col] >= 0);
   uniform [n_rows] (may be NULL): uniform[r] = c > 0 makes row r equal to c at every state and then the row has no
   CSR entries (the estimated model's unvisited pairs, 1/S, without S entries each; a full CSR row of one value is
   detected as well);
   rewards [n_rows] float32 estimated rewards; beta_r [n_rows] and beta_p0 [n_rows] (element 0 of beta_p[s, a], the
   only one the reference reads) float64; r_max [count] float64; epsilon >= 0 as in the reference (1e-3 there);
   max_sweeps >= 1 (10**6 there).  Outputs: Q [n_rows] and V [n_states] float32 of the last sweep, span [count] =
   ptp(u1) of the last sweep's input (NaN when not converged), sweeps [count] sweeps run, status [count] 0 or
   CMDP_ERR_MAX_ITER -- an instance that does not converge does not fail the call.  CMDP_ERR_INVALID names a bad
   argument; CMDP_ERR_UNSUPPORTED when an instance exceeds the LDS budget.  A per-device workspace is reused across calls
   (no allocation in steady state); calls are serialised. */
int cmdp_extended_vi(int count, const int32_t* n_states, const int32_t* n_actions, const int64_t* csr_ptr,
                     const int32_t* csr_col, const float* csr_val, const float* uniform, const float* rewards,
                     const double* beta_r, const double* beta_p0, const double* r_max, double epsilon,
                     int64_t max_sweeps, float* Q, float* V, double* span, int64_t* sweeps, int32_t* status);

/* The rule discounted_value_iteration picks its scheme by (infinite_horizon.py:28-36) as kernel K14 applies it:
   CMDP_SCHEME_JACOBI when n_states * n_actions * n_states > size_threshold and nnz / (n_states * n_actions * n_states) <
   density_threshold, else CMDP_SCHEME_GAUSS_SEIDEL.  Host only: no device is looked for. */
int cmdp_model_vi_scheme(int n_states, int n_actions, int64_t nnz, int64_t size_threshold, double density_threshold);

/* discounted_value_iteration (infinite_horizon.py:14-44) for `count` models in cmdp_extended_vi's row form at once on the
   current device (kernel K14); one launch runs every instance to convergence or to max_sweeps.  n_states[b] <= 4096,
   n_actions[b] <= 64 (else CMDP_ERR_UNSUPPORTED); csr_ptr / csr_col / csr_val / uniform / rewards as for cmdp_extended_vi,
   a uniform row counting as its S entries c in column order.  scheme: CMDP_SCHEME_JACOBI or CMDP_SCHEME_GAUSS_SEIDEL for
   every instance, or CMDP_SCHEME_AUTO: per instance cmdp_model_vi_scheme on nnz = entries with csr_val > 0 plus n_states
   per uniform row (the reference's defaults: size_threshold 300 * 3 * 300, density_threshold 0.2).  Q [n_rows], V [n_states]
   and sweeps [count] are bit for bit those of cmdp_vi_discounted with the same scheme on the CSR of the dense model;
   scheme_used [count] the scheme taken; status [count] 0 or CMDP_ERR_MAX_ITER -- an instance that does not converge does not
   fail the call.  Arguments are checked on the host before a device is looked for.  A per-device workspace is reused across
   calls; calls are serialised. */
int cmdp_vi_discounted_model(int count, const int32_t* n_states, const int32_t* n_actions, const int64_t* csr_ptr,
                             const int32_t* csr_col, const float* csr_val, const float* uniform, const float* rewards,
                             float gamma, double epsilon, int scheme, int64_t size_threshold, double density_threshold,
                             int64_t max_sweeps, float* Q, float* V, int64_t* sweeps, int32_t* scheme_used, int32_t* status);

/* ---- UCRL2 on the device (kernel K11) ------------------------------------------------------------------------- */
/* One UCRL2Continuous (colosseum/agent/agents/infinite_horizon/ucrl2.py:33-357) per instance of a CONTINUOUS environment
   handle on the CSR layout, driven as MDPLoop.run drives it (colosseum/experiment/agent_mdp_interaction.py:224-263):
   interaction, transition counts, confidence bounds, the estimated model and the optimistic solves (K10,
   cmdp_extended_vi's kernel fed from device memory) all stay on the device.  seeds [B] seed the greedy actor's tie-break
   streams (colosseum/agent/actors/Q_values_actor.py:67-88).  bound_type_p / bound_type_rew: CMDP_BOUND_*
   (ucrl2.py:93-94,130-131); bound_type_rew = CMDP_BOUND_BERNSTEIN is refused with CMDP_ERR_UNSUPPORTED: the reference
   raises AttributeError at its first solve (ucrl2.py:268).  actor: CMDP_ACTOR_GREEDY (epsilon_greedy and
   boltzmann_temperature None, ucrl2.py:96-97); the others are CMDP_ERR_UNSUPPORTED, as are episodic handles,
   CMDP_FLAG_REWARD_CACHE handles and instances with more than 4096 states (K10's limit).  Both rng modes; rewards
   deterministic, CMDP_FLAG_REWARD_MEANS or sampled on the device.  Creation performs before_start_interacting
   (ucrl2.py:192-193): the first solve, on the uniform model. */
enum { CMDP_BOUND_CHERNOFF = 0, CMDP_BOUND_BERNSTEIN = 1 };
enum { CMDP_ACTOR_GREEDY = 0, CMDP_ACTOR_EPSILON_GREEDY = 1, CMDP_ACTOR_BOLTZMANN = 2 };
typedef struct cmdp_ucrl2 cmdp_ucrl2_t;
int cmdp_ucrl2_create(cmdp_ucrl2_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon, double alpha_r,
                      double alpha_p, int bound_type_p, int bound_type_rew, int actor);
int cmdp_ucrl2_destroy(cmdp_ucrl2_t* a);
/* MDPLoop.run's loop with the agent in it (agent_mdp_interaction.py:238-263): select_action -> BaseMDP.step -> step_update
   (ucrl2.py:195-211) -> is_episode_end (:169-177) -> episode_end_update (:179-190: the solve on the model BEFORE this
   episode's model_update with the counts that already include it, then model_update :213-238).  An instance whose
   artificial episode ends parks; the parked instances of a round are solved by one K10 launch and resumed.
   stop_at_episode_end = 1: every instance stops after its next episode_end_update or after n_steps, whichever is first
   (steps_taken [B] reports which); 0: n_steps per instance.  train_mask [B] (NULL = all ones): instances with 0 act
   greedily but count nothing and end no episode (MDPLoop froze their training, :284-288).  Traces are [n_steps][B]
   (row t of instance b valid for t < steps_taken[b]): the action, the observation after it and the float64 reward;
   cumulative_reward [B] as in cmdp_qlearning_run.  Every pointer but the agent may be NULL.  The open episodes' trace of
   (pair, reward) is kept in device memory, sized before anything is stepped from the bound 2 * length <= steps so far +
   n_steps + S * A; a call whose trace cannot be allocated, or that could carry an int32 count past 2^31 - 1, is refused
   with CMDP_ERR_OVERFLOW. */
int cmdp_ucrl2_run(cmdp_ucrl2_t* a, int64_t n_steps, int stop_at_episode_end, const uint8_t* train_mask, int8_t* actions_trace,
                   int32_t* obs_trace, double* reward_trace, double* cumulative_reward, int64_t* steps_taken);
/* The model's sparse layout, constant after creation: per row (state_off[b] + s) * A + a the DISTINCT successors the
   environment's row can reach, ascending (K10's CSR): n_positions, row_ptr [R + 1], col [n_positions]; each may be NULL. */
int cmdp_ucrl2_layout(cmdp_ucrl2_t* a, int64_t* n_positions, int64_t* row_ptr, int32_t* col);
/* The agent's tables (ucrl2.py:140-159): N and P per position of the layout (all other elements of the dense arrays are 0,
   except that a row with uniform[r] = c > 0 is c at EVERY state: 1/S before the pair's first model_update);
   estimated_rewards, variance_proxy_reward, estimated_holding_times [R] float32; iteration, episode [B]; delta [B]. */
int cmdp_ucrl2_model(cmdp_ucrl2_t* a, int32_t* N, float* P_val, float* uniform, float* estimated_rewards, float* variance_proxy,
                     float* holding_times, int64_t* iteration, int64_t* episode, double* delta);
/* The last solve_optimistic_model (ucrl2.py:310-357) of every instance: its inputs (P per position, uniform, estimated
   rewards, beta_r and element 0 of beta_p[s, a]: [R] float64) and the Q [R] / span [B] the actor holds -- those of the last
   solve that CONVERGED (ucrl2.py:348-357); sweeps and status [B] are the last solve's (status CMDP_ERR_MAX_ITER: Q and
   span were kept). */
int cmdp_ucrl2_last_solve(cmdp_ucrl2_t* a, float* P_val, float* uniform, float* rewards, double* beta_r, double* beta_p0,
                          float* Q, double* span, int64_t* sweeps, int32_t* status);
/* CMDP_UCRL2_OPT_MAX_SWEEPS: sweeps a solve may take (default 10**6, the reference's DP_MAX_ITERATION); for tests of the
   not-converged path. */
/* CMDP_UCRL2_OPT_POLICY_SIZE_THRESHOLD: the size threshold of the scheme rule in cmdp_ucrl2_policy's solve (default
   300 * 3 * 300, the reference's); a test hook that lets small instances take the Jacobi scheme. */
/* CMDP_UCRL2_OPT_POLICY_REUSE: 1 (default) an instance whose `episode` has not moved since its last converged policy solve
   keeps that solve's Q and greedy policy -- the estimated model changes in model_update only, which ends an episode -- and
   cmdp_ucrl2_policy / cmdp_ucrl2_average_reward / cmdp_ucrl2_run_logged skip K14 for it; 0: every request solves.  The
   results are bit-identical either way.  Setting either of the other two options discards the stored solves. */
enum { CMDP_UCRL2_OPT_MAX_SWEEPS = 1, CMDP_UCRL2_OPT_POLICY_SIZE_THRESHOLD = 2, CMDP_UCRL2_OPT_POLICY_REUSE = 3 };
int cmdp_ucrl2_set_option(cmdp_ucrl2_t* a, int option, int64_t value);
/* UCRL2Continuous.current_optimal_stochastic_policy (ucrl2.py:80-83) of the instances with mask[b] != 0 (NULL: all), on the
   device: kernel K14 on the agent's own tables (gamma 0.99, epsilon 1e-3, the reference's scheme rule), then argmax_2d with
   the RandomState(42) tie-break.  pi [R] one-hot float32, Q [R], sweeps [B], scheme_used [B]; each may be NULL, and what
   belongs to an instance outside the mask is left as it was.  CMDP_ERR_MAX_ITER names an instance whose solve took 10**6
   sweeps (the reference raises there).  The actor's Q and streams, the counts and the environment are not touched. */
int cmdp_ucrl2_policy(cmdp_ucrl2_t* a, const uint8_t* mask, float* pi, float* Q, int64_t* sweeps, int32_t* scheme_used);
/* ... and get_average_reward of that policy from the environments' current states (as cmdp_qlearning_average_reward). */
int cmdp_ucrl2_average_reward(cmdp_ucrl2_t* a, const uint8_t* mask, double* avg, int32_t* kind);
/* MDPLoop.run as one call for the UCRL2 agents: arguments, outputs and rows as cmdp_qlearning_run_logged on a continuous
   handle.  The interaction is cmdp_ucrl2_run's, a row's evaluation cmdp_ucrl2_average_reward's for the instances that
   still need one.  The rows are processed strictly in order on the handle's stream (the agent synchronises in every round of
   parked instances, so no interval starts early).  Refused before anything is reset or stepped: null arguments, an n_logs
   that is not the schedule's, missing baselines, optimal - worst <= 0.0002, a handle without the DP half (all
   CMDP_ERR_INVALID); an instance beyond K9's LDS budget when log_every > 0 (CMDP_ERR_UNSUPPORTED); an agent that has
   already taken steps (CMDP_ERR_INVALID: the reward sums count from creation, MDPLoop's from zero); n_steps beyond what
   cmdp_ucrl2_run would take in one call (CMDP_ERR_OVERFLOW). */
int cmdp_ucrl2_run_logged(cmdp_ucrl2_t* a, const cmdp_loop_desc* desc, int64_t n_logs, int64_t* steps, double* values,
                          uint8_t* kinds, int64_t* last_training_step, uint8_t* is_training);

/* One PSRLEpisodic (colosseum/agent/agents/episodic/posterior_sampling.py with BayesianMDPModel, N_NIG rewards and M_DIR
   transitions) per instance of an EPISODIC environment handle, driven as MDPLoop.run drives it
   (agent_mdp_interaction.py:224-298).  The interaction, the posterior tables, the posterior sample, the solve
   (k_vi_episodic_dense) and the actor's Q stay on the device (K12, csrc/cmdp_psrl.h).  seeds [B] seed the greedy actor's
   tie-break stream, the reference sampler's two RandomState streams and the Philox sampler's key (seed, CMDP_PSRL_KEY_HI).
   reward_prior [B][4]: N_NIG's hyper-parameters (mu, lambda, alpha, beta) float32 AFTER the "interpretable parameters"
   transform of N_NIG.__init__; transition_prior [B]: M_DIR's prior, the same for every element of the instance.
   sampler: CMDP_PSRL_SAMPLER_REFERENCE draws the reference's own numbers on the host (numpy's legacy samplers, one
   RandomState(seed) per conjugate model and instance); CMDP_PSRL_SAMPLER_PHILOX draws on the device (k_psrl_sample:
   distribution-exact, counter-based, a pure function of (key, episode, tables)).  actor: CMDP_ACTOR_GREEDY; the others
   are CMDP_ERR_UNSUPPORTED, as are continuous handles, CMDP_FLAG_REWARD_CACHE handles and instances with more than 4096
   states.  CMDP_ERR_OVERFLOW when the dense workspace of the sampled models (sum of S * A * S float32) cannot be
   allocated.  Creation performs before_start_interacting: the first sample and solve, on the prior. */
enum { CMDP_PSRL_SAMPLER_REFERENCE = 0, CMDP_PSRL_SAMPLER_PHILOX = 1 };
#define CMDP_PSRL_KEY_HI 0x5053524Cu
typedef struct cmdp_psrl cmdp_psrl_t;
int cmdp_psrl_create(cmdp_psrl_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon,
                     const float* reward_prior, const float* transition_prior, int sampler, int actor);
int cmdp_psrl_destroy(cmdp_psrl_t* a);
/* n_steps of select_action -> step -> step_update per instance; an instance whose step was its episode's last gets its
   episode_end_update (sample -> solve -> the new Q) and then the environment's reset().  Arguments and results as
   cmdp_ucrl2_run: stop_at_episode_end stops every instance after its next episode_end_update, steps_taken [B] says where;
   train_mask [B] (NULL: all train) 0 = the instance acts on the Q it holds, updates nothing and samples nothing (the
   environment still resets); traces [n_steps][B] (observation -1 at an episode's last step).  A call that could carry a
   visit counter of the environment past 2^31 - 1, or a float32 transition count past 2^24, is refused with
   CMDP_ERR_OVERFLOW before anything is stepped. */
int cmdp_psrl_run(cmdp_psrl_t* a, int64_t n_steps, int stop_at_episode_end, const uint8_t* train_mask, int8_t* actions_trace,
                  int32_t* obs_trace, double* reward_trace, double* cumulative_reward, int64_t* steps_taken);
/* PSRLEpisodic.episode_end_update() for EVERY instance, outside the loop: a new posterior sample on the tables as they are, its
   solve, the new Q; no step is taken and the environment is not reset (what creation does once on the prior). */
int cmdp_psrl_episode_end_update(cmdp_psrl_t* a);
/* The transition model's sparse layout (as cmdp_ucrl2_layout). */
int cmdp_psrl_layout(cmdp_psrl_t* a, int64_t* n_positions, int64_t* row_ptr, int32_t* col);
/* reward_hp [R][4] float32; transition_hp per position of the layout (every other element of the dense array equals
   transition_prior [B]); episodes [B]: posterior samples drawn so far, the one at creation included.  Each may be NULL. */
int cmdp_psrl_model(cmdp_psrl_t* a, float* reward_hp, float* transition_hp, float* transition_prior, int64_t* episodes);
/* The last posterior sample of every instance: T dense [sum S * A * S], R [R], and the Q [sum (H + 1) * S * A] the actor
   holds (instance b: [H + 1][S][A], layer H zero).  Each may be NULL. */
int cmdp_psrl_last_sample(cmdp_psrl_t* a, float* T, float* R, float* Q);
/* Host only: M_DIR.sample and N_NIG.sample of one instance on two numpy RandomState streams given as `get_state()`
   leaves them (key [624], position, has_gauss, cached_gaussian; updated in place).  Transition hyper-parameters: dense
   [S * A * S], or -- when that is NULL -- a layout (row_ptr [S * A + 1], col ascending, val) over `prior`.  reward_hp
   [S * A][4].  Outputs T [S * A * S] and R [S * A] float32: numpy's numbers, draw for draw. */
int cmdp_psrl_reference_sample(uint32_t* t_key, int32_t* t_pos, int32_t* t_has_gauss, double* t_gauss, uint32_t* r_key,
                               int32_t* r_pos, int32_t* r_has_gauss, double* r_gauss, int n_states, int n_actions,
                               const float* transition_hp_dense, const int64_t* row_ptr, const int32_t* col, const float* val,
                               float prior, const float* reward_hp, float* T, float* R);
/* episodic_value_iteration(H, T, R) (colosseum/dynamic_programming/finite_horizon.py:11-26) on `count` dense float32
   problems: T concatenated [S, A, S] per instance, R [S, A]; Q receives [H + 1][S][A] and V [H + 1][S] per instance, layer H
   zero.  Q[h, s, a] = float(double(R[s, a]) + sum_j double(T[s, a, j]) * double(V[h + 1, j])), the sum in float64 in a fixed
   order.  The kernel the PSRL agent solves with.  CMDP_ERR_UNSUPPORTED beyond 4096 states. */
int cmdp_vi_episodic_dense(int count, const int32_t* n_states, const int32_t* n_actions, int H, const float* T, const float* R,
                           float* Q, float* V);
/* Host only (no HIP call): the MAP estimate of one instance's M_DIR model in table form.  Row r of the dense hyper-parameter
   array holds hp[e] at the ascending columns col[e], e in row_ptr[r] .. row_ptr[r + 1] (row_ptr [S * A + 1] indexes col / hp /
   t directly), and `prior` > 0 at every other state.  rowsum [S * A] = numpy's pairwise float32 sum of the dense row,
   c [S * A] = prior / rowsum, t[e] = hp[e] / rowsum (float32): hyper_params / hyper_params.sum(-1, keepdims=True) bit for
   bit.  Each output may be NULL.  The definition of K15's prologue. */
int cmdp_psrl_map_rows(int n_states, int n_actions, const int64_t* row_ptr, const int32_t* col, const float* hp, float prior,
                       float* rowsum, float* c, float* t);
/* episodic_value_iteration(H, T_map, mu) on `count` MAP models in table form (K15, csrc/cmdp_map_vi.h), one launch, no dense
   array: row_ptr [sum S * A + 1] over the rows of all problems (row_ptr[0] = 0), col instance-relative and ascending within a
   row, hp per position, prior [count], mu [sum S * A].  With T_map as cmdp_psrl_map_rows defines it,
     Q[h, s, a] = float(double(mu[s, a]) + double(c) * (SV - sum_e double(V[h + 1, col_e])) + sum_e double(t_e) * double(V[h + 1, col_e]))
   where SV is the float64 sum of V[h + 1, :] in a fixed order and V[h, s] = max_a Q[h, s, a].  Q receives [H + 1][S][A] and V
   [H + 1][S] per instance, layer H zero; t_layout_out (per position) and c_out (per row) receive T_map and may be NULL.
   CMDP_ERR_UNSUPPORTED beyond 4096 states. */
int cmdp_vi_episodic_map(int count, const int32_t* n_states, const int32_t* n_actions, int H, const int64_t* row_ptr,
                         const int32_t* col, const float* hp, const float* prior, const float* mu, float* Q, float* V,
                         float* t_layout_out, float* c_out);
/* PSRLEpisodic.current_optimal_stochastic_policy (posterior_sampling.py:78-82) for the instances selected by mask [B] (NULL:
   all), on the device from the agent's posterior tables: K15 on the MAP estimate, then argmax_3d (RandomState(42) tie-break)
   over all H + 1 layers.  pi and Q receive [H + 1][S][A] per instance (pi one-hot), zeros for unselected instances; each may
   be NULL.  The actor's Q, the last sample, the posterior tables, the episode counters, both RNG streams and the environment
   are left untouched. */
int cmdp_psrl_policy(cmdp_psrl_t* a, const uint8_t* mask, float* pi, float* Q);
/* V[0, :] of that policy on the TRUE MDP (the handle's episodic policy evaluation), V0 [state_off[B]], zeros for unselected
   instances: what MDPLoop's episodic regret needs.  CMDP_ERR_UNSUPPORTED when the environment handle has no DP half. */
int cmdp_psrl_evaluate(cmdp_psrl_t* a, const uint8_t* mask, float* V0);
/* MDPLoop.run as one call for the PSRL agents: as cmdp_ucrl2_run_logged, on an episodic handle with the episodic baselines of
   cmdp_qlearning_run_logged.  The interaction is cmdp_psrl_run's, a row's evaluation cmdp_psrl_evaluate(a, NULL, .)'s.  The
   same refusals; a handle without the DP half or beyond the evaluation's LDS budget is CMDP_ERR_UNSUPPORTED. */
int cmdp_psrl_run_logged(cmdp_psrl_t* a, const cmdp_loop_desc* desc, int64_t n_logs, int64_t* steps, double* values,
                         uint8_t* kinds, int64_t* last_training_step, uint8_t* is_training);

/* One PSRLContinuous (colosseum/agent/agents/infinite_horizon/posterior_sampling.py) with PLAIN posterior sampling -- the
   reference's no_optimistic_sampling=True path -- per instance of a CONTINUOUS environment handle, driven as MDPLoop.run
   drives it (K13, csrc/cmdp_psrlc.h).  Arguments, samplers and refusals as cmdp_psrl_create (an episodic handle is
   CMDP_ERR_UNSUPPORTED here).  The posterior tables and both samplers are K12's; an artificial episode ends after the step
   with N[s, a].sum() >= 2 * (N[s, a].sum() - nu_k[s, a]); the solve is discounted_value_iteration(T, R) with gamma = 0.99,
   epsilon = 1e-3 and the reference's scheme rule per sample (cmdp_vi_discounted_dense).  Creation performs
   before_start_interacting: the first sample and solve, on the prior.  The statistics are CMDP_STAT_PSRL_*.  Optimistic
   sampling is cmdp_psrlc_create_optimistic's (below); truncate_reward_with_max and min_steps_before_new_episode != 0 are not
   built. */
typedef struct cmdp_psrlc cmdp_psrlc_t;
int cmdp_psrlc_create(cmdp_psrlc_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon,
                      const float* reward_prior, const float* transition_prior, int sampler, int actor);
int cmdp_psrlc_destroy(cmdp_psrlc_t* a);
/* As cmdp_psrl_run, without resets: an instance whose step ended an artificial episode gets its episode_end_update (sample ->
   solve -> the new Q) and walks on from where it stands.  train_mask 0 = the instance acts on the Q it holds, updates nothing
   and never ends an episode.  An instance whose solve reaches max_sweeps keeps the last sweep's Q
   (CMDP_STAT_PSRL_UNCONVERGED). */
int cmdp_psrlc_run(cmdp_psrlc_t* a, int64_t n_steps, int stop_at_episode_end, const uint8_t* train_mask, int8_t* actions_trace,
                   int32_t* obs_trace, double* reward_trace, double* cumulative_reward, int64_t* steps_taken);
/* PSRLContinuous.episode_end_update() for EVERY instance, outside the loop: sample, solve, the new Q, every nu_k back to 0. */
int cmdp_psrlc_episode_end_update(cmdp_psrlc_t* a);
int cmdp_psrlc_layout(cmdp_psrlc_t* a, int64_t* n_positions, int64_t* row_ptr, int32_t* col);
/* As cmdp_psrl_model, with the agent's visit counters per row: n_sa [R] = N[s, a].sum(), nu_k [R] = visits since the last
   episode_end_update.  Each may be NULL. */
int cmdp_psrlc_model(cmdp_psrlc_t* a, float* reward_hp, float* transition_hp, float* transition_prior, int32_t* n_sa,
                     int32_t* nu_k, int64_t* episodes);
/* The last posterior sample of every instance, T dense [sum S * A * S] and R [R], the Q [R] the actor holds, and of its solve
   the sweeps [B], the scheme [B] (CMDP_SCHEME_JACOBI / CMDP_SCHEME_GAUSS_SEIDEL) and the status [B] (0 or CMDP_ERR_MAX_ITER).
   Each may be NULL. */
int cmdp_psrlc_last_sample(cmdp_psrlc_t* a, float* T, float* R, float* Q, int64_t* sweeps, int32_t* scheme, int32_t* status);
/* PSRLContinuous.current_optimal_stochastic_policy (infinite_horizon/posterior_sampling.py:174-178) for the instances selected
   by mask [B] (NULL: all), on the device from the agent's posterior tables: the dense MAP model (T_map as cmdp_psrl_map_rows
   defines it, R_map = mu) in a workspace of its own, cmdp_vi_discounted_dense's kernel on it, then argmax_2d (RandomState(42)
   tie-break).  pi and Q receive [S][A] per instance (pi one-hot), sweeps and scheme [B]; zeros for unselected instances; each
   may be NULL.  CMDP_ERR_MAX_ITER when a solve does not converge.  The actor's Q, the last sample, the posterior tables, the
   counters, both RNG streams and the environment are left untouched. */
int cmdp_psrlc_policy(cmdp_psrlc_t* a, const uint8_t* mask, float* pi, float* Q, int64_t* sweeps, int32_t* scheme);
/* get_average_reward of that policy from the environments' current states (as cmdp_ucrl2_average_reward). */
int cmdp_psrlc_average_reward(cmdp_psrlc_t* a, const uint8_t* mask, double* avg, int32_t* kind);
/* Test hooks: the size threshold of the scheme rule (the reference's default 300 * 3 * 300) and the sweeps a solve may take
   (DP_MAX_ITERATION = 10^6).  CMDP_PSRLC_OPT_POLICY_SOLVER picks the route behind cmdp_psrlc_policy and
   cmdp_psrlc_average_reward: 0 (the default) the dense route described above, 1 the tables route -- K17
   (cmdp_vi_discounted_map's kernel) straight on the posterior tables, which never allocates the dense workspace; any other
   value is CMDP_ERR_INVALID.  Both routes fill the same outputs and CMDP_STAT_PSRL_POLICY_KERNEL_MS. */
/* CMDP_PSRLC_OPT_SAMPLE_SOLVER (optimistic handles; CMDP_ERR_UNSUPPORTED on a plain one, any value but 0 and 1
   CMDP_ERR_INVALID) picks the route of the optimistic sample and its solve from the next episode_end_update on, internal or
   external: 0 (the default) the dense route, T_ext written and cmdp_vi_discounted_dense's kernel on it; 1 the compact route,
   K19 (cmdp_vi_discounted_optimistic's kernel) on the compact sample, T_ext never built.  Switching a handle created compact to
   dense allocates the dense arrays at that moment; when they do not fit it returns CMDP_ERR_OVERFLOW and the handle stays
   compact.  An instance's last sample stays in the form of the round that drew it. */
/* CMDP_PSRLC_OPT_MIN_STEPS (plain and optimistic handles) is the reference's min_steps_before_new_episode
   (posterior_sampling.py:353-355): is_episode_end evaluates its rule only at a step whose in-run time h (steps since the
   environment's last reset, read before the step) is at least that many past last_change, and every check that passes moves
   last_change [B] (0 at creation) to h, whether or not the episode ends; a frozen instance never checks, and no
   episode_end_update touches last_change.  0 (the default) runs the walk kernels compiled without the gate.  A value outside
   [0, 2^31 - 1] is CMDP_ERR_INVALID, and so is any call once an instance has taken a step: the reference fixes the value at
   construction. */
enum { CMDP_PSRLC_OPT_SIZE_THRESHOLD = 1, CMDP_PSRLC_OPT_MAX_SWEEPS = 2, CMDP_PSRLC_OPT_POLICY_SOLVER = 3,
       CMDP_PSRLC_OPT_SAMPLE_SOLVER = 4, CMDP_PSRLC_OPT_MIN_STEPS = 5 };
int cmdp_psrlc_set_option(cmdp_psrlc_t* a, int option, int64_t value);
/* The gate's state: the option's value and last_change [B]; either may be null. */
int cmdp_psrlc_episode_gate(cmdp_psrlc_t* a, int64_t* min_steps, int32_t* last_change);
/* MDPLoop.run as one call for the continuous PSRL agents, plain and optimistic: as cmdp_ucrl2_run_logged.  The interaction is
   cmdp_psrlc_run's, a row's evaluation what cmdp_psrlc_average_reward(a, need, .) enqueues, by the handle's current policy
   route.  The same refusals, with the float32 limit of 2^24 steps of cmdp_psrlc_run; the route's workspace is allocated
   before anything is reset or stepped (the dense route's may be CMDP_ERR_OVERFLOW). */
int cmdp_psrlc_run_logged(cmdp_psrlc_t* a, const cmdp_loop_desc* desc, int64_t n_logs, int64_t* steps, double* values,
                          uint8_t* kinds, int64_t* last_training_step, uint8_t* is_training);
/* The same agent with the reference's OPTIMISTIC sampling (no_optimistic_sampling=False, its default; K18,
   csrc/cmdp_psrlo.h): psi [B] extended actions per real action, eta [B] the visit count below which a row is sampled simply,
   log4s [B] = log(4 S) as the caller's NumPy gives it.  The handle serves every cmdp_psrlc_* entry: the walk acts greedily on
   the extended Q [S][A * psi] and plays j / psi, the sample is T_ext [S, A * psi, S] with R_ext[s, j] = R[s, j % A], the
   solver is cmdp_vi_discounted_dense's on the extended arrays, and the agent's N[s, a, s'] is kept as int32.
   CMDP_PSRL_SAMPLER_REFERENCE draws on the host (the two models' streams and the agent's own RandomState(seed));
   CMDP_PSRL_SAMPLER_PHILOX draws the posterior rows, z and the rewards in k_psrlo_sample, a pure function of (seed, episode,
   tables).  Refused before anything is allocated: S * A * psi * S of an instance reaching 2^32 (CMDP_ERR_UNSUPPORTED) and a
   batch whose extended arrays (with the reference sampler also their upload) exceed the free device memory
   (CMDP_ERR_OVERFLOW; the message names the bytes). */
int cmdp_psrlc_create_optimistic(cmdp_psrlc_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon,
                                 const float* reward_prior, const float* transition_prior, const int32_t* psi, const double* eta,
                                 const double* log4s, int sampler, int actor);
/* cmdp_psrlc_create_optimistic with the sample route chosen at creation: sample_solver 0 is that entry, 1 the compact route
   (K19, csrc/cmdp_psrlo_vi.h; CMDP_PSRLC_OPT_SAMPLE_SOLVER), anything else CMDP_ERR_INVALID.  Created compact, the handle
   allocates neither T_ext nor the reference sampler's T_ext-sized upload, and the memory refusal counts only the extended Q,
   R_ext and bump arrays and the plain-sized workspace.  Per instance the compact sample keeps pmk [psi][nz_b] and bump
   [psi][S * A] and one block of posterior rows [psi][n1_b][S] for the n1_b posterior rows of its last draw; a block only grows,
   to max(need, min(2 * capacity, psi * S * A * S)) floats (to need alone when that much cannot be had), and a round that
   cannot grow one fails with CMDP_ERR_OVERFLOW (the message names the bytes); that instance then holds no sample until a
   later round.  CMDP_STAT_PSRL_SAMPLE_BYTES of a handle that was never dense is therefore
     4 * (max(1, sum_b psi_b * nz_b) + sum_b S_b * A * psi_b) + 8 * B + 4 * sum_b capacity_b.
   The S * A * psi * S < 2^32 refusal stays: the Philox sampler's counters are the dense route's. */
int cmdp_psrlc_create_optimistic_route(cmdp_psrlc_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon,
                                       const float* reward_prior, const float* transition_prior, const int32_t* psi,
                                       const double* eta, const double* log4s, int sampler, int actor, int sample_solver);
/* The last optimistic sample of every instance: T dense [sum S * A * psi * S], R [R] as N_NIG gave it, R_ext and the actor's
   Q [sum S * A * psi], z [sum psi] (reference sampler: -1 where no row was simple and none was drawn), the simple mask [R], and the solve's
   sweeps, scheme and status [B].  Each may be NULL.  CMDP_ERR_UNSUPPORTED on a plain handle, as cmdp_psrlc_last_sample is on
   an optimistic one.  For an instance whose last sample is compact, T is its expansion, produced instance by instance
   through a staging buffer of one instance's size. */
int cmdp_psrlc_last_sample_optimistic(cmdp_psrlc_t* a, float* T, float* R, float* R_ext, float* Q, int32_t* z, uint8_t* simple,
                                      int64_t* sweeps, int32_t* scheme, int32_t* status);
/* The agent's N[s, a, s'] at the positions of cmdp_psrlc_layout (0 elsewhere, for ever); optimistic handles only. */
int cmdp_psrlc_counts(cmdp_psrlc_t* a, int32_t* N);
/* The host half of an optimistic sample with the reference sampler, callable without a device: one optimistic_sampling call's
   draws and the N_NIG sample that follows on three RandomState streams handed over and returned as cmdp_psrl_reference_sample
   does (t: M_DIR's, r: N_NIG's, a: the agent's, which first skips `skip_randn` legacy Gaussians).  n_sa [S * A]; the M_DIR
   hyper-parameters as a layout over `prior`.  Out: simple [S * A]; *n_posterior = n1; posterior [psi][n1][S] the normalised
   posterior rows in row-major order (capacity psi * S * A * S); z [psi], -1 where none is drawn; R [S * A]. */
int cmdp_psrlo_reference_draw(uint32_t* t_key, int32_t* t_pos, int32_t* t_has_gauss, double* t_gauss, uint32_t* r_key,
                              int32_t* r_pos, int32_t* r_has_gauss, double* r_gauss, uint32_t* a_key, int32_t* a_pos,
                              int32_t* a_has_gauss, double* a_gauss, int n_states, int n_actions, int psi, double eta,
                              int64_t skip_randn, const int32_t* n_sa, const int64_t* row_ptr, const int32_t* col, const float* val,
                              float prior, const float* reward_hp, uint8_t* simple, int32_t* n_posterior, float* posterior,
                              int32_t* z, float* R);
/* discounted_value_iteration(T, R) (colosseum/dynamic_programming/infinite_horizon.py:14-44) on `count` dense float32 problems
   in one launch (k_vi_discounted_dense, csrc/cmdp_psrlc.h): T concatenated [S, A, S] per instance, R [S, A]; Q receives [S][A]
   and V [S] per instance.  scheme: CMDP_SCHEME_AUTO applies the reference's rule per instance on its count of non-zero
   elements (cmdp_model_vi_scheme with size_threshold and density_threshold).  Every row sum is taken in float64 in a fixed
   order:
     Gauss-Seidel  Q[s, a] = float(double(R[s, a]) + sum_j double(fl32(gamma * T[s, a, j])) * double(V[j])), V[s] = max_a at once
     Jacobi        Q[s, a] = R[s, a] + gamma * float(sum_j double(T[s, a, j]) * double(V_old[j])) in float32
   from V = 0 until max_s |V_old[s] - V[s]| < epsilon after a sweep.  sweeps [count], scheme_used [count], status [count]: 0,
   or CMDP_ERR_MAX_ITER when max_sweeps were taken (Q and V are then the last sweep's; the call still returns CMDP_OK).
   CMDP_ERR_UNSUPPORTED beyond 4096 states; values of T or R that are not finite are CMDP_ERR_INVALID. */
int cmdp_vi_discounted_dense(int count, const int32_t* n_states, const int32_t* n_actions, const float* T, const float* R,
                             float gamma, double epsilon, int scheme, int64_t size_threshold, double density_threshold,
                             int64_t max_sweeps, float* Q, float* V, int64_t* sweeps, int32_t* scheme_used, int32_t* status);

/* discounted_value_iteration(T_ext, R_ext) on `count` COMPACT optimistic samples in one launch (K19,
   k_vi_discounted_optimistic, csrc/cmdp_psrlo_vi.h), T_ext [S, A * psi, S] never built.  Per problem b with S states, A real
   actions and psi[b] samples, the arrays of all problems concatenated in problem order:
     row_ptr [sum S * A + 1], col   the layout of the real rows (row_ptr[0] = 0; col problem-relative, ascending within a row);
                                    nz_b positions in problem b
     simple  [sum S * A]            1: a simple row, 0: a posterior row
     z       [sum psi]              the bumped column of sample k; in [0, S) when the problem has a simple row, else unread
     pmk     [sum psi * nz_b]       per problem [psi][nz_b]: the value of sample k at layout position e (simple rows' are read)
     bump    [sum S * A * psi]      per problem [psi][S * A]: the value of sample k of a simple row at column z_k
     pidx    [sum S * A]            posterior rows: their index among the problem's n1_b posterior rows in row order; simple
                                    rows: unread
     post    [sum psi * n1_b * S]   per problem [psi][n1_b][S] the dense posterior rows; NULL when no problem has one
     R       [sum S * A]            the real rewards; R_ext[s, j] = R[s, j % A] is computed
   Extended row j = a * psi + k of state s is, for a simple row (s, a), zero except pmk[k][e] at col[e] and bump[k][row] at z_k
   (at z_k the bump stands, once), and post[k][pidx][:] for a posterior row.  A posterior row's sum is
   cmdp_vi_discounted_dense's (same lanes, same order); a simple row's terms are taken in ascending column order and added one
   at a time in float64 to +0, double(fl32(gamma * t)) * double(V[c]) under Gauss-Seidel and double(t) * double(V_old[c])
   under Jacobi, and wrapped up as the dense definition does.  CMDP_SCHEME_AUTO counts the non-zero elements of the expansion
   from the compact form.  The solver's arguments, refusals and outputs (Q [S][A * psi], V [S], sweeps, scheme_used, status)
   are cmdp_vi_discounted_dense's; psi < 1 or A * psi > 2^20, a malformed layout, a pidx out of order, a z outside [0, S) and
   values that are not finite are CMDP_ERR_INVALID, S * A * psi * S >= 2^32 CMDP_ERR_UNSUPPORTED. */
int cmdp_vi_discounted_optimistic(int count, const int32_t* n_states, const int32_t* n_actions, const int32_t* psi,
                                  const int64_t* row_ptr, const int32_t* col, const uint8_t* simple, const int32_t* z,
                                  const float* pmk, const float* bump, const int32_t* pidx, const float* post, const float* R,
                                  float gamma, double epsilon, int scheme, int64_t size_threshold, double density_threshold,
                                  int64_t max_sweeps, float* Q, float* V, int64_t* sweeps, int32_t* scheme_used, int32_t* status);

/* discounted_value_iteration(T_map, mu) on `count` MAP models in table form (K17, csrc/cmdp_map_dvi.h), one launch, no dense
   array.  The problem is cmdp_vi_episodic_map's: row_ptr [sum S * A + 1] over the rows of all problems (row_ptr[0] = 0), col
   instance-relative and ascending within a row, hp per position, prior [count], mu [sum S * A]; the solver's arguments, their
   refusals and the outputs Q [S][A], V [S], sweeps, scheme_used and status are cmdp_vi_discounted_dense's.  With T_map = (t, c)
   as cmdp_psrl_map_rows defines it, sub = sum_e double(V[col_e]) and SV the float64 sum of V in a fixed order:
     Gauss-Seidel  Q[s, a] = float(double(mu) + (double(fl32(gamma c)) * (SV - sub) + sum_e double(fl32(gamma t_e)) * double(V[col_e]))),
                   V[s] = max_a at once, SV = SV + (double(V_new) - double(V[s]))
     Jacobi        Q[s, a] = mu + gamma * float(double(c) * (SV - sub) + sum_e double(t_e) * double(V_old[col_e])) in float32
   from V = 0 until max_s |V_old[s] - V[s]| < epsilon after a sweep; a row whose layout covers every column leaves the c term
   out.  CMDP_SCHEME_AUTO counts the positions with t_e != 0 plus S - len for every row with c != 0: the dense MAP array's
   non-zero elements.  t_layout_out (per position) and c_out (per row) receive T_map and may be NULL.  CMDP_ERR_UNSUPPORTED
   beyond 4096 states; every other null or invalid argument is CMDP_ERR_INVALID, by name. */
int cmdp_vi_discounted_map(int count, const int32_t* n_states, const int32_t* n_actions, const int64_t* row_ptr,
                           const int32_t* col, const float* hp, const float* prior, const float* mu, float gamma, double epsilon,
                           int scheme, int64_t size_threshold, double density_threshold, int64_t max_sweeps, float* Q, float* V,
                           int64_t* sweeps, int32_t* scheme_used, int32_t* status, float* t_layout_out, float* c_out);

#ifdef __cplusplus
}
#endif
#endif /* CMDP_H */
