// cmdp_kernels.h -- HIP kernels of libcmdp (gfx950 / CDNA4).  Included once by cmdp.hip.
//
// K1  k_reset / k_step / k_rollout : agent<->MDP interaction, one lane per instance, tables in HBM/L2
// K2  k_dp_block<...>              : Jacobi sweeps (discounted VI / PE, diameter), one workgroup per
//                                    (instance[, target]); V ping-pong and, when it fits, the CSR in LDS
// K3  k_dp_wave_gs<...>            : Gauss-Seidel sweeps, one wavefront per (instance[, target]), V in LDS
// K4  k_episodic                   : backward induction, one workgroup per instance
// K6  k_value_norm                 : value-norm reduction
// K14 k_vi_model (cmdp_model_vi.h) : discounted VI on estimated models in K10's row form (CSR rows, or one value for a
//                                    row that holds it everywhere), either scheme, one wavefront per instance, every
//                                    sweep in one launch; the serial sums of the uniform rows shared
// K15 k_vi_episodic_map (cmdp_map_vi.h) : episodic VI on the MAP estimate of a Bayesian model from its tables (layout
//                                    positions over a prior), one workgroup per instance, no dense array
//
// No MFMA anywhere: rows have <= ~8 non-zeros; everything is gather / scan / max-reduce.
// Float32 DP arithmetic uses __fmul_rn/__fadd_rn (never contracted into FMA): the reference's
// accumulations round the product and the sum separately.
#pragma once
#include <type_traits>
#include "cmdp_device.h"
#include "cmdp_reward_cache.h"

struct __attribute__((aligned(32))) RowDesc {  // 32 B, one per (instance, state, action): ONE load per transition
  int32_t first;         // first entry of the row, relative to the instance's entry base
  int32_t n;             // number of successors (1 = deterministic shortcut, no draw)
  int32_t next_if_det;   // successor when n == 1
  int32_t mt_slot;       // MT19937 slot of the row's sampler (MT_COMPAT, n > 1), else -1
  double reward_if_det;  // reward of the only successor when n == 1 (saves the dependent entry load)
  double pad;
};

// Visit counters belong to exactly one lane; the add is issued as a no-return atomic so that the wave never
// waits for a counter load (fire and forget; the increments are off the state's dependency chain).
__device__ __forceinline__ void bump(int32_t* p) {
  (void)__hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct EnvTables {
  int32_t B, A, H, rng_mode;
  double rscale, rmin;               // reward = r * rscale - rmin
  int32_t beta_gammas;               // CMDP_FLAG_BETA_GAMMAS
  const int64_t* state_off;          // [B+1]
  const int64_t* entry_base;         // [B]
  const RowDesc* row;                // [R]
  const int32_t* sp_next;            // [E]
  const double* sp_cum;              // [E]
  const double* sp_reward;           // [E]  deterministic value | distribution mean
  const uint8_t* sp_rkind;           // [E]  null: every reward is deterministic; 1 = Beta(sp_rp0, sp_rp1) sampled per transition
  const double* sp_rp0;              // [E]
  const double* sp_rp1;              // [E]
  const int64_t* start_off;          // [B+1]
  const int32_t* start_state;        // [NS]
  const double* start_cum;           // [NS]
  const int32_t* start_slot;         // [B]  MT slot of the start sampler or -1
  const uint2* philox_key;           // [B]
  uint32_t* mt;                      // [n_slots][624]
  int32_t* mt_pos;                   // [n_slots]
  // dynamic state
  int32_t* cur;                      // [B]
  int32_t* hstep;                    // [B]
  uint8_t* need_reset;               // [B]
  unsigned long long* n_trans;       // [B]
  unsigned long long* n_reset;       // [B]
  int32_t* visits_s;                 // [NSTATES]
  int32_t* visits_sa;                // [R]
  int32_t* last_start;               // [B] BaseMDP.last_starting_node (index): state of the latest reset()
  int32_t* prev_start;               // [B] the one before it (MDPLoop logs BEFORE the reset that follows a termination)
};

// ---------------------------------------------------------------------------------------------------
__global__ void k_mt_seed(uint32_t* __restrict__ mt, int32_t* __restrict__ mt_pos, const int32_t* __restrict__ seeds,
                          int64_t n_slots) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slots) return;
  mt_seed_python_int(mt + i * 624, (uint32_t)seeds[i]);
  mt_pos[i] = 0;
}

// random-policy action of transition n (the domain-2 stream of cmdp_device.h: packed when A is 2, 4, 16 or 256)
__device__ __forceinline__ int philox_action(unsigned long long n, uint2 key, int A) {
  uint32_t act[4];
  philox_act4(n >> 2, key, A, philox_act_lg(A), act);
  const int j = (int)(n & 3);
  return (int)((j == 0) ? act[0] : (j == 1) ? act[1] : (j == 2) ? act[2] : act[3]);
}

// BaseMDP.reset (reference colosseum/mdp/base.py:1268-1277) for one instance
__device__ __forceinline__ int32_t env_reset(const EnvTables& t, int b, int64_t soff, uint2 key,
                                             unsigned long long& n_reset) {
  const int64_t lo = t.start_off[b];
  const int n = (int)(t.start_off[b + 1] - lo);
  int idx = 0;
  if (n > 1) {
    double u;
    if (t.rng_mode == 0) {
      const int slot = t.start_slot[b];
      u = mt_random(t.mt + (int64_t)slot * 624, t.mt_pos + slot);
    } else {
      uint32_t w[4];
      philox4x32_10((uint32_t)n_reset, (uint32_t)(n_reset >> 32), 1u, 0u, key.x, key.y, w);
      u = u53(w[0], w[1]);
    }
    idx = choose_index(t.start_cum + lo, n, u);
  }
  n_reset++;
  const int32_t s = t.start_state[lo + idx];
  bump(t.visits_s + soff + s);
  t.prev_start[b] = t.last_start[b];
  t.last_start[b] = s;
  return s;
}

// BaseMDP.step (reference colosseum/mdp/base.py:1293-1317) for one instance, up to (not including) the reward sample:
// action -> successor, visit counts, in-episode time.  Returns the step type (1 MID, 2 LAST); `action` < 0 requests the
// Philox random-policy action; `e` receives the global entry of the transition taken, `rraw` its deterministic reward /
// distribution mean before the range rescale.
// The core takes the row descriptor of (cur, action) by value.  `PAIR`: the two MT19937 words of a draw are fetched together
// (the agent kernels, which also fetch the descriptors of all actions next to the Q row, before the action is known).
template <bool PAIR>
__device__ __forceinline__ int env_transition_desc(const EnvTables& t, int64_t soff, int64_t ebase, uint2 key, int32_t& cur,
                                                   int32_t& h, unsigned long long n, int action, int32_t& obs,
                                                   double& rraw, int64_t& e, const RowDesc d) {
  h += 1;
  int32_t nxt = d.next_if_det;
  rraw = d.reward_if_det;
  e = ebase + d.first;
  if (d.n > 1) {  // NextStateSampler.sample (custom_samplers.py:59-72)
    double u;
    if (t.rng_mode == 0) {
      u = PAIR ? mt_random_pair(t.mt + (int64_t)d.mt_slot * 624, t.mt_pos + d.mt_slot)
               : mt_random(t.mt + (int64_t)d.mt_slot * 624, t.mt_pos + d.mt_slot);
    } else {
      uint32_t w[4];
      philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), 0u, 0u, key.x, key.y, w);
      u = u53(w[0], w[1]);
    }
    e += choose_index(t.sp_cum + e, d.n, u);
    nxt = t.sp_next[e];
    rraw = t.sp_reward[e];
  }
  // visit counts on the arrival node with the action taken at the departure node (base.py:1302-1303)
  bump(t.visits_s + soff + nxt);
  bump(t.visits_sa + (soff + nxt) * t.A + action);
  cur = nxt;
  if (t.H > 0 && h >= t.H) {
    obs = -1;
    return 2;
  }
  obs = nxt;
  return 1;
}

__device__ __forceinline__ int env_transition(const EnvTables& t, int64_t soff, int64_t ebase, uint2 key, int32_t& cur,
                                              int32_t& h, unsigned long long& n_trans, int& action, int32_t& obs,
                                              double& rraw, int64_t& e) {
  const unsigned long long n = n_trans;
  if (action < 0) action = philox_action(n, key, t.A);
  n_trans++;
  const RowDesc d = t.row[(soff + cur) * t.A + action];
  return env_transition_desc<false>(t, soff, ebase, key, cur, h, n, action, obs, rraw, e, d);
}

// The whole step incl. the reward (`sample_reward`, base.py:1187-1207) for handles whose rewards are deterministic or
// sampled on the device.  BETA = false compiles the Beta-reward sampler (Marsaglia-Tsang gammas: log/pow/cos in float64,
// ~100 VGPRs) out of the kernel: handles without stochastic rewards then run at twice the occupancy.
template <bool BETA = true>
__device__ __forceinline__ int env_step(const EnvTables& t, int64_t soff, int64_t ebase, uint2 key, int32_t& cur,
                                        int32_t& h, unsigned long long& n_trans, int action, int32_t& obs,
                                        double& reward) {
  const unsigned long long n = n_trans;
  double rraw;
  int64_t e;
  const int ty = env_transition(t, soff, ebase, key, cur, h, n_trans, action, obs, rraw, e);
  if (BETA && t.sp_rkind && t.sp_rkind[e] == 1) rraw = philox_beta(t.sp_rp0[e], t.sp_rp1[e], n, key, t.beta_gammas);  // throughput mode only
  reward = rraw * t.rscale - t.rmin;  // `r * (max - min) - min`, base.py:1205-1207
  return ty;
}

__global__ void k_reset(EnvTables t, const uint8_t* __restrict__ mask, int32_t* __restrict__ obs_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  if (mask && !mask[b]) return;
  unsigned long long nr = t.n_reset[b];
  const int32_t s = env_reset(t, b, t.state_off[b], t.philox_key ? t.philox_key[b] : make_uint2(0, 0), nr);
  t.n_reset[b] = nr;
  t.cur[b] = s;
  t.hstep[b] = 0;
  t.need_reset[b] = 0;
  if (obs_out) obs_out[b] = s;
}

__global__ void k_any_needs_reset(const uint8_t* __restrict__ need_reset, int B, int32_t* __restrict__ flag) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B && need_reset[b]) atomicOr(flag, 1);
}

__global__ void k_check_actions(const int32_t* __restrict__ actions, int B, int A, int32_t* __restrict__ flag) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B && (actions[b] < 0 || actions[b] >= A)) atomicOr(flag, 2);
}

// RC: reference-exact reward caches (cmdp_reward_cache.h).  A lane whose reward block is missing parks after the
// transition; the relaunch (`resume` != 0) only completes the parked lanes.
template <bool RC>
__global__ void k_step(EnvTables t, const int32_t* __restrict__ actions, int auto_reset, int32_t* __restrict__ obs,
                       double* __restrict__ reward, uint8_t* __restrict__ step_type, RewardCache rc, int resume) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  const int64_t soff = t.state_off[b];
  if (RC && resume) {
    const int32_t pe = rc.pend_e[b];
    if (pe < 0) return;
    double rraw = 0.0;
    if (!rc_fetch(t.sp_rkind, rc, pe, rraw)) {  // cannot happen after an install; parks again rather than inventing a value
      rc_park(rc, b, pe, rc.pend_prev[b], rc.pend_act[b]);
      return;
    }
    rc.pend_e[b] = -1;
    reward[b] = rraw * t.rscale - t.rmin;
    return;
  }
  if (t.need_reset[b]) {  // only reachable with auto_reset (the host pre-checks otherwise): step() == reset()
    unsigned long long nr = t.n_reset[b];
    const int32_t s = env_reset(t, b, soff, t.philox_key ? t.philox_key[b] : make_uint2(0, 0), nr);
    t.n_reset[b] = nr;
    t.cur[b] = s;
    t.hstep[b] = 0;
    t.need_reset[b] = 0;
    obs[b] = s;
    reward[b] = 0.0;
    step_type[b] = 0;
    return;
  }
  int32_t cur = t.cur[b], h = t.hstep[b], o;
  unsigned long long nt = t.n_trans[b];
  double r;
  int ty;
  const uint2 key = t.philox_key ? t.philox_key[b] : make_uint2(0, 0);
  if (RC) {
    const int32_t prev = cur;
    int a = actions[b];
    double rraw;
    int64_t e;
    ty = env_transition(t, soff, t.entry_base[b], key, cur, h, nt, a, o, rraw, e);
    if (rc_fetch(t.sp_rkind, rc, e, rraw)) r = rraw * t.rscale - t.rmin;
    else { rc_park(rc, b, e, prev, a); r = 0.0; }
  } else {
    ty = env_step(t, soff, t.entry_base[b], key, cur, h, nt, actions[b], o, r);
  }
  t.cur[b] = cur;
  t.hstep[b] = h;
  t.n_trans[b] = nt;
  t.need_reset[b] = (ty == 2);
  obs[b] = o;
  reward[b] = r;
  step_type[b] = (uint8_t)ty;
}

// The env side of MDPLoop.run's loop (reference colosseum/experiment/agent_mdp_interaction.py:238-298),
// fused: n_steps transitions per instance, every termination followed at once by reset().
// POLICY 0: on-device uniform random (Philox); 1: host action stream actions[t][B] (int8); 2: greedy in a Q table
// (`qtab`: per instance [S][A], or [H][S][A] indexed by the in-episode time when the handle is episodic), first maximiser.
// RC: reference-exact reward caches -- a lane parks when its block is missing and the relaunch (`resume`) continues it
// where it stopped, first completing the saved step (cmdp_reward_cache.h); `reward_sum` then accumulates across the
// launches of one call (the host zeroes it first).
template <int POLICY, bool TRACE, bool BETA, bool RC = false>
__global__ void __launch_bounds__(256) k_rollout(EnvTables t, const int8_t* __restrict__ actions, int64_t n_steps,
                                                 double* __restrict__ reward_sum, int32_t* __restrict__ last_obs,
                                                 int32_t* __restrict__ tr_obs, double* __restrict__ tr_rew,
                                                 uint8_t* __restrict__ tr_type, const float* __restrict__ qtab = nullptr,
                                                 RewardCache rc = RewardCache{}, int resume = 0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  int64_t s0 = 0;
  bool pending = false;
  if (RC && resume) {
    const long long left = rc.left[b];
    if (left == 0) return;
    s0 = n_steps - left;
    pending = rc.pend_e[b] >= 0;
  }
  const int64_t soff = t.state_off[b], ebase = t.entry_base[b];
  const int64_t S_b = t.state_off[b + 1] - soff;
  const uint2 key = t.philox_key ? t.philox_key[b] : make_uint2(0, 0);
  int32_t cur = t.cur[b], h = t.hstep[b], obs = cur;
  unsigned long long nt = t.n_trans[b], nr = t.n_reset[b];
  double sum = (RC && resume) ? reward_sum[b] : 0.0;
  bool parked = false;
  int64_t s = s0;
  for (; s < n_steps; ++s) {
    double r;
    int ty;
    if (RC) {
      int a = -1;
      int32_t prev = cur;
      double rraw = 0.0;
      int64_t e;
      if (pending) {  // the step this lane parked in: transition committed, reward outstanding
        e = rc.pend_e[b];
        prev = rc.pend_prev[b];
        a = rc.pend_act[b];
        ty = (t.H > 0 && h >= t.H) ? 2 : 1;
        obs = (ty == 2) ? -1 : cur;
        pending = false;
      } else {
        if (POLICY == 1) a = (int)actions[s * t.B + b];
        if (POLICY == 2) {
          const float* q = qtab + ((t.H > 0 ? (int64_t)t.H * soff + (int64_t)h * S_b : soff) + cur) * t.A;
          float best = q[0];
          a = 0;
          for (int k = 1; k < t.A; ++k)
            if (q[k] > best) { best = q[k]; a = k; }
        }
        ty = env_transition(t, soff, ebase, key, cur, h, nt, a, obs, rraw, e);
      }
      if (!rc_fetch(t.sp_rkind, rc, e, rraw)) {
        rc_park(rc, b, e, prev, a);
        parked = true;
        break;
      }
      r = rraw * t.rscale - t.rmin;
    } else {
      int a = -1;
      if (POLICY == 1) a = (int)actions[s * t.B + b];
      if (POLICY == 2) {
        const float* q = qtab + ((t.H > 0 ? (int64_t)t.H * soff + (int64_t)h * S_b : soff) + cur) * t.A;
        float best = q[0];
        a = 0;
        for (int k = 1; k < t.A; ++k)
          if (q[k] > best) { best = q[k]; a = k; }
      }
      ty = env_step<BETA>(t, soff, ebase, key, cur, h, nt, a, obs, r);
    }
    sum += r;
    if (TRACE) {
      if (tr_obs) tr_obs[s * t.B + b] = obs;
      if (tr_rew) tr_rew[s * t.B + b] = r;
      if (tr_type) tr_type[s * t.B + b] = (uint8_t)ty;
    }
    if (ty == 2) {
      cur = env_reset(t, b, soff, key, nr);
      h = 0;
      obs = cur;
    }
  }
  t.cur[b] = cur;
  t.hstep[b] = h;
  t.n_trans[b] = nt;
  t.n_reset[b] = nr;
  if (RC) {
    rc.left[b] = parked ? (long long)(n_steps - s) : 0;
    if (!parked) rc.pend_e[b] = -1;
  }
  if (reward_sum) reward_sum[b] = sum;
  if (last_obs) last_obs[b] = obs;
}

// ---------------------------------------------------------------------------------------------------
// K1L: LDS-resident rollout for batches of small deterministic-dynamics instances (config C2).
//
// The lane-per-instance kernel above moves a whole HBM sector for every 4..32-byte table access
// (measured ~640 B of traffic per 44-byte transition), so it is bound by HBM sector throughput.  Here a
// one-wavefront workgroup stages the tables of G instances into LDS with coalesced loads ONCE per launch
// -- per instance: successor table uint16[S*A] and visit-count deltas [S*A] (packed mode: successor row base with
// the reward code in the upper bits, 8-bit deltas with an overflow list; otherwise a separate uint8[S*A] reward-code
// table and 16-bit deltas) -- walks them for n_steps entirely on chip (one LDS read on the dependency chain per
// transition), then adds the deltas into the HBM counters with coalesced read-modify-writes.
// HBM traffic per launch ~ (2..3 + 12) bytes per table row, independent of n_steps.
// Instances per workgroup, chunk length and workgroups per CU are chosen in cmdp_create (fewest rounds).
// ---------------------------------------------------------------------------------------------------
struct LdsPlan {
  int32_t G;               // instances per workgroup (<= 64)
  int32_t rows_max;        // max S*A over the batch
  int32_t slot_bytes;      // LDS bytes per instance slot
  int32_t off_rcode;       // byte offsets inside a slot
  int32_t off_cnt;
  int32_t off_ovf;         // packed mode: uint16 list of the rows whose 8-bit counter wrapped since the last flush
  int32_t ch;              // transitions per action-ring chunk (multiple of 8)
  int32_t n_codes;         // distinct reward values (<= 256)
  int32_t pipe;            // 1: run as the three-stage wavefront pipeline K1P (packed mode only)
  int32_t code_shift;      // > 0: next16 holds (successor * A) in its low code_shift bits and the reward code above
                           //      them (no rcode table, no multiply on the walker's dependency chain)
  const uint16_t* next16;  // [R] successor of every (deterministic) row
  const uint8_t* rcode;    // [R] index into rvals
  const double* rvals;     // [n_codes]
};

struct LdsPlan;
// dst[j] += delta(j) for j in [0, total): ROWS: delta = 16-bit count of row j; else delta = sum over the A
// counts of state j (+ the resets of its instance when j is the start state).  `per` = rows or states per slot.
template <bool ROWS, bool BYTES, int NT>
__device__ __forceinline__ void flush_counts(int32_t* __restrict__ dst, int total, int per, int A, unsigned char* slots,
                                             const LdsPlan& p, const int32_t* resets, const int32_t* start_states,
                                             int tid);
// `K` independent global loads in flight per thread before any is consumed (memory-level parallelism:
// the staging / flush phases are pure streaming and must not serialise on HBM latency).
#define K1L_UNROLL 8
#define K1L_THREADS 256
#define K1L_OVF 30                      // wrap events an instance can record between two flushes (8-bit counters)
#define K1L_NRV 264                      // reward table entries in LDS: 256 codes + a zero entry (index 256) + pad
#define K1P_ACT_STRIDE(ch) ((ch) + 4)       // K1P ring strides in bytes per instance
#define K1P_TR_STRIDE(ch) (2 * (ch) + 4)
#define K1L_FIXED (K1L_NRV * 8 + 64 * 4 + 64 * 8 + 64 * 8)   // rv2[K1L_NRV] f64, resets[64] i32, keys[64] uint2, ntr[64] u64

// Stages the successor words of a group's `total_rows` rows into the instance slots: 16-byte loads from the
// aligned-down address, K1L_UNROLL of them in flight per thread (the element arrays carry 16 bytes of slack at
// both ends, see cmdp_create).
template <int NT>
__device__ __forceinline__ void k1l_stage_words(const LdsPlan& p, int64_t row00, int total_rows, int rows,
                                                unsigned char* slots, int tid) {
  {
    const uint16_t* src = p.next16 + row00;
    const int head = (int)((reinterpret_cast<uintptr_t>(src) & 15) >> 1);
    const uint4* vsrc = reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(src) - 2 * head);
    const int nchunks = (head + total_rows + 7) >> 3;
    for (int c0 = 0; c0 < nchunks; c0 += NT * K1L_UNROLL) {
      uint4 v[K1L_UNROLL];
#pragma unroll
      for (int k = 0; k < K1L_UNROLL; ++k) {
        const int c = c0 + k * NT + tid;
        if (c < nchunks) v[k] = vsrc[c];
      }
#pragma unroll
      for (int k = 0; k < K1L_UNROLL; ++k) {
        const int c = c0 + k * NT + tid;
        if (c < nchunks) {
          const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
          int j = c * 8 - head;
          int slot = (j > 0) ? j / rows : 0, off = j - slot * rows;
#pragma unroll
          for (int e = 0; e < 8; ++e, ++j, ++off) {
            if (off == rows) { off = 0; ++slot; }
            if (j >= 0 && j < total_rows)
              reinterpret_cast<uint16_t*>(slots + (size_t)slot * p.slot_bytes)[off] = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
          }
        }
      }
    }
  }
}

// Wavefront specialisation: lanes of wavefront 0 walk one instance each; wavefronts 1-3 are the random-policy
// PRODUCERS -- they compute the Philox blocks of the NEXT chunk of p.ch transitions for all G instances into a
// double-buffered LDS ring of action bytes while the walkers consume the current chunk, so the walker's
// instruction stream is only: action byte, successor read (the one LDS load on the dependency chain), 16-bit count
// add, reward add.  The walker is software-pipelined by hand: the bookkeeping of transition s-1 (count add, reward
// table read) and the reward add of transition s-2 are issued while the successor read of transition s is in flight.
template <bool PACKED>
__global__ void __launch_bounds__(K1L_THREADS) k_rollout_lds(EnvTables t, LdsPlan p, int64_t n_steps,
                                                            double* __restrict__ reward_sum,
                                                            int32_t* __restrict__ last_obs) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int g0 = blockIdx.x * p.G;
  const int nb = min(p.G, t.B - g0);
  double* rv2 = reinterpret_cast<double*>(smem);                          // [256] reward value AFTER the range rescale
  int32_t* resets = reinterpret_cast<int32_t*>(smem + K1L_NRV * 8);       // [64]
  uint2* keys = reinterpret_cast<uint2*>(smem + K1L_NRV * 8 + 64 * 4);    // [64]
  unsigned long long* ntr = reinterpret_cast<unsigned long long*>(smem + K1L_NRV * 8 + 64 * 4 + 64 * 8);  // [64] transition counters at launch
  const int CH = p.ch;
  unsigned char* ring = smem + K1L_FIXED;                                 // [2][G][CH] action bytes
  unsigned char* slots = ring + 2 * p.G * CH;
  const int A = t.A, H = t.H;
  // all instances of the batch have the same S (eligibility): the group's rows are one contiguous range
  const int64_t so0 = t.state_off[g0];
  const int S = (int)(t.state_off[g0 + 1] - so0);
  const int rows = S * A;
  const int64_t row00 = so0 * A;
  const int total_rows = nb * rows, total_states = nb * S;
  // `r * (max - min) - min` (base.py:1205-1207) applied once per distinct value: the same two float64 operations
  for (int i = tid; i < p.n_codes; i += K1L_THREADS) rv2[i] = p.rvals[i] * t.rscale - t.rmin;
  if (tid == 0) rv2[256] = 0.0;  // what the walker's software pipeline adds before it holds a real reward
  if (tid < nb) { keys[tid] = t.philox_key[g0 + tid]; ntr[tid] = t.n_trans[g0 + tid]; }
  // ---- stage the tables: 16-byte loads from the aligned-down address, K1L_UNROLL of them in flight per
  //      thread (the element arrays carry 16 bytes of slack at both ends, see cmdp_create) -----------------
  k1l_stage_words<K1L_THREADS>(p, row00, total_rows, rows, slots, tid);
  if (!PACKED) {
    const uint8_t* src = p.rcode + row00;
    const int head = (int)(reinterpret_cast<uintptr_t>(src) & 15);
    const uint4* vsrc = reinterpret_cast<const uint4*>(src - head);
    const int nchunks = (head + total_rows + 15) >> 4;
    for (int c0 = 0; c0 < nchunks; c0 += K1L_THREADS * K1L_UNROLL) {
      uint4 v[K1L_UNROLL];
#pragma unroll
      for (int k = 0; k < K1L_UNROLL; ++k) {
        const int c = c0 + k * K1L_THREADS + tid;
        if (c < nchunks) v[k] = vsrc[c];
      }
#pragma unroll
      for (int k = 0; k < K1L_UNROLL; ++k) {
        const int c = c0 + k * K1L_THREADS + tid;
        if (c < nchunks) {
          const uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
          int j = c * 16 - head;
          int slot = (j > 0) ? j / rows : 0, off = j - slot * rows;
#pragma unroll
          for (int e = 0; e < 16; ++e, ++j, ++off) {
            if (off == rows) { off = 0; ++slot; }
            if (j >= 0 && j < total_rows)
              (slots + (size_t)slot * p.slot_bytes + p.off_rcode)[off] = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
          }
        }
      }
    }
  }
  // count deltas: 16-bit halves of dwords, or (packed mode) bytes incl. the walker's dummy counter behind them
  const int cnt_dwords = PACKED ? (p.rows_max + 4) / 4 : (rows + 1) / 2;
  for (int j = tid; j < nb * cnt_dwords; j += K1L_THREADS) {
    const int slot = j / cnt_dwords, off = j - slot * cnt_dwords;
    reinterpret_cast<uint32_t*>(slots + (size_t)slot * p.slot_bytes + p.off_cnt)[off] = 0u;
  }
  const bool walker = tid < nb;
  const int b = g0 + (walker ? tid : 0);
  const int32_t start = t.start_state[t.start_off[b]];
  const int32_t start_k = PACKED ? start * A : start;
  int32_t cur = PACKED ? t.cur[b] * A : t.cur[b], h = t.hstep[b];
  // every instance of the group has its own transition counter; the producers need all of them
  const unsigned long long nt0 = t.n_trans[b];
  unsigned long long nr = t.n_reset[b];
  double sum = 0.0;
  const unsigned char* base = slots + (size_t)(walker ? tid : 0) * p.slot_bytes;
  const uint16_t* nx = reinterpret_cast<const uint16_t*>(base);
  const uint8_t* rc = base + p.off_rcode;
  uint32_t* cnt = reinterpret_cast<uint32_t*>(const_cast<unsigned char*>(base) + p.off_cnt);
  uint8_t* c8 = const_cast<unsigned char*>(base) + p.off_cnt;                                  // packed mode
  uint16_t* ovf = reinterpret_cast<uint16_t*>(const_cast<unsigned char*>(base) + p.off_ovf);    // packed mode
  int n_ovf = 0;
  __syncthreads();

  // producer: fills ring buffer `buf` with the actions of transitions [first, first + len) of every instance
  const int act_lg = philox_act_lg(A);
  auto produce = [&](int buf, int64_t first, int len) {
    const int ptid = tid - 64;  // 0..191
    const int per_slot = CH / 4 + 1;  // Philox blocks that can overlap a chunk window (unaligned start)
    for (int item = ptid; item < nb * per_slot; item += K1L_THREADS - 64) {
      const int slot = item / per_slot, qi = item - slot * per_slot;
      const unsigned long long n0 = ntr[slot] + (unsigned long long)first;  // first transition of the window (LDS copy:
                                                                            // a global load per item made the producers as slow as the walk)
      const unsigned long long q = (n0 >> 2) + (unsigned long long)qi;
      const uint2 key = keys[slot];
      uint32_t w[4];
      philox_act4(q, key, A, act_lg, w);
      unsigned char* dst = ring + ((size_t)buf * p.G + slot) * CH;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long pos = (long long)(4 * q + j) - (long long)n0;
        if (pos >= 0 && pos < len) dst[pos] = (unsigned char)w[j];
      }
    }
  };

  int64_t done = 0;
  int buf = 0;
  if (n_steps > 0 && tid >= 64) produce(0, 0, (int)min((int64_t)CH, n_steps));
  __syncthreads();
  int since_flush = 0;
  int32_t n_resets = 0, n_resets_total = 0;
  // Software pipeline registers of the walker.  They start at neutral elements so that the steady-state body needs
  // no predicates: +0.0 (x + 0.0 == x), the zero entry of the reward table, and a dummy count dword behind the
  // slot's real counters (never flushed).
  const int dummy_crow = PACKED ? p.rows_max : 2 * ((p.rows_max + 1) / 2);
  int pend_crow = dummy_crow, pend_code = 256;
  double pend_val = 0.0;
  const bool episodic = H > 0;
  const int smask = (1 << p.code_shift) - 1;
  // wave 0 only: lanes beyond the group's instances mirror lane 0 (b = g0), so a plain wave vote works
  const bool uniform_h = episodic && tid < 64 && __all(h == __builtin_amdgcn_readfirstlane(h));
  while (done < n_steps) {
    const int len = (int)min((int64_t)CH, n_steps - done);
    if (tid >= 64) {
      const int64_t nfirst = done + len;
      if (nfirst < n_steps) produce(buf ^ 1, nfirst, (int)min((int64_t)CH, n_steps - nfirst));
    } else if (walker) {
      const unsigned char* acts = ring + ((size_t)buf * p.G + tid) * CH;
      // The walker is bound by the number of instructions it issues per transition (a lone wavefront issues one every
      // 4-8 cycles: ~25 instructions made ~85 ns, against ~35 ns for the bare dependent LDS chain,
      // tools/calib/lds_chase.hip), so the body exists in three flavours chosen per group of 8 transitions:
      //   T0  all walkers share their in-episode time and no episode ends inside the group: no episode logic at all
      //   T1  shared in-episode time, scalar episode-end test
      //   T2  per-lane in-episode time (general case)
      // and the loop over whole groups carries no per-transition bounds test (the ragged tail runs separately).
      int hs = uniform_h ? __builtin_amdgcn_readfirstlane(h) : 0, nres_s = 0;
      auto step = [&](int a, auto mode_tag) {
        constexpr int MODE = decltype(mode_tag)::value;
        // PACKED: `cur` and the table's successor field are ROW BASES (state * A): no multiply on the chain
        const int row = PACKED ? cur + a : cur * A + a;
        const int word = nx[row];  // the one load on the dependency chain
        const int nxt = PACKED ? (word & smask) : word;
        const int code = PACKED ? (word >> p.code_shift) : (int)rc[row];
        // bookkeeping of the two previous transitions while the successor read is in flight
        sum += pend_val;             // rewards are added in transition order: bit-equal to the sequential sum
        pend_val = rv2[pend_code];
        // visit count of the ARRIVAL node under the action taken (base.py:1302-1303)
        if (PACKED) {
          // 8-bit counter, read-modify-write by its only owner (LDS executes a wave's operations in order, so the
          // next transition's read sees this write); a wrap is recorded in the overflow list (a vote + branch instead was
          // slower: it forces the wait for the count read at once).  Half the bytes of the 16-bit form: 40 % more instances fit a CU.
          const int c1 = (int)c8[pend_crow] + 1;
          ovf[n_ovf] = (uint16_t)pend_crow;  // branch-free: the slot behind the last entry is only kept on a wrap
          n_ovf += c1 >> 8;
          c8[pend_crow] = (uint8_t)c1;
        } else {
          atomicAdd(cnt + (pend_crow >> 1), (pend_crow & 1) ? 0x10000u : 1u);  // 16-bit halves of a dword
        }
        pend_crow = PACKED ? nxt + a : nxt * A + a;
        pend_code = code;
        if (MODE == 0) {
          cur = nxt;
        } else if (MODE == 1) {
          ++hs;
          const bool term = hs >= H;  // scalar
          cur = term ? start_k : nxt;
          hs = term ? 0 : hs;
          nres_s += term ? 1 : 0;
        } else {
          ++h;
          const bool term = episodic && h >= H;  // episodic termination followed at once by reset()
          cur = term ? start_k : nxt;
          h = term ? 0 : h;
          n_resets += term ? 1 : 0;
        }
      };
      using T0 = std::integral_constant<int, 0>;
      using T1 = std::integral_constant<int, 1>;
      using T2 = std::integral_constant<int, 2>;
      int s0 = 0;
      for (; s0 + 8 <= len; s0 += 8) {
        const uint2 aw = *reinterpret_cast<const uint2*>(acts + s0);  // eight action bytes, one LDS read
#define K1L_ACT(j) (int)((((j) < 4 ? aw.x : aw.y) >> (8 * ((j) & 3))) & 0xffu)
        if (uniform_h && hs + 8 < H) {
          step(K1L_ACT(0), T0{}); step(K1L_ACT(1), T0{}); step(K1L_ACT(2), T0{}); step(K1L_ACT(3), T0{});
          step(K1L_ACT(4), T0{}); step(K1L_ACT(5), T0{}); step(K1L_ACT(6), T0{}); step(K1L_ACT(7), T0{});
          hs += 8;
        } else if (uniform_h && H >= 8) {
          // exactly one episode ends inside this group, after transition jstar: plain transitions around one reset
          const int jstar = H - hs - 1;
#define K1L_STEP_R(j)                               \
  step(K1L_ACT(j), T0{});                           \
  if (jstar == (j)) { cur = start_k; ++nres_s; }
          K1L_STEP_R(0) K1L_STEP_R(1) K1L_STEP_R(2) K1L_STEP_R(3) K1L_STEP_R(4) K1L_STEP_R(5) K1L_STEP_R(6) K1L_STEP_R(7)
#undef K1L_STEP_R
          hs = 7 - jstar;
        } else if (uniform_h) {
          step(K1L_ACT(0), T1{}); step(K1L_ACT(1), T1{}); step(K1L_ACT(2), T1{}); step(K1L_ACT(3), T1{});
          step(K1L_ACT(4), T1{}); step(K1L_ACT(5), T1{}); step(K1L_ACT(6), T1{}); step(K1L_ACT(7), T1{});
        } else {
          step(K1L_ACT(0), T2{}); step(K1L_ACT(1), T2{}); step(K1L_ACT(2), T2{}); step(K1L_ACT(3), T2{});
          step(K1L_ACT(4), T2{}); step(K1L_ACT(5), T2{}); step(K1L_ACT(6), T2{}); step(K1L_ACT(7), T2{});
        }
#undef K1L_ACT
      }
      for (; s0 < len; ++s0) {  // ragged tail of the launch's last chunk
        const int a = acts[s0];
        if (uniform_h) step(a, T1{}); else step(a, T2{});
      }
      if (uniform_h) { h = hs; n_resets += nres_s; }
    }
    done += len;
    since_flush += len;
    buf ^= 1;
    // 16-bit deltas cannot wrap within 32 768 transitions; 8-bit ones wrap at most once per 256 transitions of their
    // instance, and the overflow list holds K1L_OVF wraps
    const bool flush_now = (since_flush + CH > (PACKED ? 256 * K1L_OVF : 32768)) || done >= n_steps;
    if (flush_now && tid < 64) {
      if (walker) {  // drain the software pipeline before the counters are read
        sum += pend_val;
        sum += rv2[pend_code];
        if (PACKED) {
          int c1 = (int)c8[pend_crow] + 1;
          if (c1 == 256) { ovf[n_ovf++] = (uint16_t)pend_crow; c1 = 0; }
          c8[pend_crow] = (uint8_t)c1;
        } else {
          atomicAdd(cnt + (pend_crow >> 1), (pend_crow & 1) ? 0x10000u : 1u);
        }
        pend_crow = dummy_crow; pend_code = 256; pend_val = 0.0;
        resets[tid] = n_resets;
        n_resets_total += n_resets;
        n_resets = 0;
      }
    }
    __syncthreads();
    if (flush_now) {
      // ---- flush the deltas into the HBM counters: 16-byte read-modify-writes (every counter has exactly one
      //      owner; the partial chunks at the two ends of the group's range go element by element) -----------
      flush_counts<true, PACKED, K1L_THREADS>(t.visits_sa + row00, total_rows, rows, A, slots, p, resets, nullptr, tid);
      flush_counts<false, PACKED, K1L_THREADS>(t.visits_s + so0, total_states, S, A, slots, p, resets, t.start_state + t.start_off[g0], tid);
      __syncthreads();
      if (PACKED && walker) {  // every recorded wrap is worth 256 visits (the dummy counter never gets that far)
        for (int e = 0; e < n_ovf; ++e) {
          const int r = ovf[e];
          if (r < rows) {
            t.visits_sa[row00 + (int64_t)tid * rows + r] += 256;
            t.visits_s[so0 + (int64_t)tid * S + r / A] += 256;
          }
        }
        n_ovf = 0;
      }
      for (int j = tid; j < nb * cnt_dwords; j += K1L_THREADS) {
        const int slot = j / cnt_dwords, off = j - slot * cnt_dwords;
        reinterpret_cast<uint32_t*>(slots + (size_t)slot * p.slot_bytes + p.off_cnt)[off] = 0u;
      }
      since_flush = 0;
      __syncthreads();
    }
  }
  if (walker) {
    if (PACKED) cur /= A;
    t.cur[b] = cur;
    t.hstep[b] = h;
    t.n_trans[b] = nt0 + (unsigned long long)n_steps;
    t.n_reset[b] = nr + (unsigned long long)n_resets_total;
    if (n_resets_total) t.prev_start[b] = t.last_start[b];   // as env_reset at every termination: the start before the latest one is this (only) start state too
    if (reward_sum) reward_sum[b] = sum;
    if (last_obs) last_obs[b] = cur;  // the state after the last transition (the start state after a termination)
  }
}

// ---------------------------------------------------------------------------------------------------
// K1P: the packed LDS rollout as a WAVEFRONT PIPELINE.
//
// K1L's walker is bound by the instructions one wavefront issues per transition (~17; a lone wavefront issues one
// every 4-8 cycles), not by the dependent LDS read.  Here a transition's work is split over the wavefronts of the
// workgroup, one chunk of p.ch transitions apart:
//   wave 0        CHAIN     action byte -> successor word (the dependent LDS read) -> trace entry `word + 2 action`
//                           (= byte offset of the arrival row under the action taken | reward code << code_shift),
//                           stored one transition late so that it queues behind the next read; episode bookkeeping
//   wave 1        COUNTS    8-bit visit counters of the traced rows (+ overflow list), one chunk behind the chain
//   wave 4        REWARDS   adds the traced reward codes' values in transition order (bit-equal to the sequential sum)
//   waves 2,3,6,7 PRODUCERS Philox action bytes of the chunk after the chain's (lane i: instance i; the blocks of a
//                           window are dealt round-robin to the four waves)
//   wave 5        idle (waves w and w + 4 share a SIMD: the chain and the counters keep theirs almost to themselves)
// Lane i of every wave owns instance i of the group.  Rings (actions, trace) are double-buffered; one barrier per chunk.
// The successor field of the table word is the successor's row base as a BYTE offset (2 A s'), so the chain's
// address is one add3.  LDS per instance: slot_bytes + 2 (p.ch + 4) + 2 (2 p.ch + 4); the odd strides keep the
// per-lane rings off each other's banks.
// ---------------------------------------------------------------------------------------------------
#define K1P_THREADS 512
#define K1P_NPROD 4
__global__ void __launch_bounds__(K1P_THREADS) k_rollout_pipe(EnvTables t, LdsPlan p, int64_t n_steps,
                                                             double* __restrict__ reward_sum,
                                                             int32_t* __restrict__ last_obs) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;  // scalar: the role branches are uniform
  const int g0 = blockIdx.x * p.G;
  const int nb = min(p.G, t.B - g0);
  double* rv2 = reinterpret_cast<double*>(smem);
  int32_t* resets = reinterpret_cast<int32_t*>(smem + K1L_NRV * 8);
  const int CH = p.ch;
  const int AS = K1P_ACT_STRIDE(CH), TS = K1P_TR_STRIDE(CH);
  unsigned char* ring = smem + K1L_FIXED;                 // [2][G] action bytes, stride AS
  unsigned char* trace = ring + 2 * p.G * AS;             // [2][G] uint16 trace entries, stride TS bytes
  unsigned char* slots = trace + 2 * p.G * TS;
  const int A = t.A, H = t.H;
  const int64_t so0 = t.state_off[g0];
  const int S = (int)(t.state_off[g0 + 1] - so0);
  const int rows = S * A;
  const int64_t row00 = so0 * A;
  const int total_rows = nb * rows, total_states = nb * S;
  const int cnt_dwords = (p.rows_max + 4) / 4;
  for (int i = tid; i < p.n_codes; i += K1P_THREADS) rv2[i] = p.rvals[i] * t.rscale - t.rmin;
  k1l_stage_words<K1P_THREADS>(p, row00, total_rows, rows, slots, tid);
  for (int j = tid; j < nb * cnt_dwords; j += K1P_THREADS) {
    const int slot = j / cnt_dwords, off = j - slot * cnt_dwords;
    reinterpret_cast<uint32_t*>(slots + (size_t)slot * p.slot_bytes + p.off_cnt)[off] = 0u;
  }
  const bool owner = lane < nb;  // this lane's instance exists
  const int b = g0 + (owner ? lane : 0);
  unsigned char* base = slots + (size_t)(owner ? lane : 0) * p.slot_bytes;
  uint8_t* c8 = base + p.off_cnt;
  uint16_t* ovf = reinterpret_cast<uint16_t*>(base + p.off_ovf);
  const int smask = (1 << p.code_shift) - 1;
  // chain state (wave 0): `cur` is the byte offset of the current state's row base (2 A s)
  const int32_t start_k = t.start_state[t.start_off[b]] * A * 2;
  int32_t cur = t.cur[b] * A * 2, h = t.hstep[b];
  int32_t n_resets = 0, n_resets_total = 0;
  const bool episodic = H > 0;
  const bool uniform_h = episodic && wave == 0 && __all(h == __builtin_amdgcn_readfirstlane(h));
  int n_ovf = 0;     // counts state (wave 1)
  double sum = 0.0;  // rewards state (wave 2)
  // producer state: the lane's key, transition counter and ring row stay in registers
  const uint2 my_key = t.philox_key[b];
  const unsigned long long my_ntr = t.n_trans[b];
  const int act_lg = philox_act_lg(A);
  __syncthreads();

  // actions of transitions [first, first + len) of this lane's instance, Philox blocks pidx, pidx + K1P_NPROD, ...
  auto produce = [&](int buf, int64_t first, int len, int pidx) {
    if (!owner) return;
    const unsigned long long n0 = my_ntr + (unsigned long long)first;
    const int rel0 = (int)(n0 & 3ull);  // the window starts inside a block when the counter is not a multiple of 4
    const unsigned long long q0 = n0 >> 2;
    const int nblk = (rel0 + len + 3) >> 2;
    unsigned char* dst = ring + ((size_t)buf * p.G + lane) * AS;
    for (int qi = pidx; qi < nblk; qi += K1P_NPROD) {
      const unsigned long long q = q0 + (unsigned long long)qi;
      uint32_t act[4];
      philox_act4(q, my_key, A, act_lg, act);
      const int pos0 = 4 * qi - rel0;
      if (rel0 == 0 && pos0 + 4 <= len) {
        *reinterpret_cast<uint32_t*>(dst + pos0) = act[0] | (act[1] << 8) | (act[2] << 16) | (act[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (pos0 + j >= 0 && pos0 + j < len) dst[pos0 + j] = (unsigned char)act[j];
      }
    }
  };

  // chain (wave 0): walks chunk `cb` of `len` transitions
  auto chain_body = [&](int cb, int len) {
    if (!owner || len <= 0) return;
    const unsigned char* acts = ring + ((size_t)cb * p.G + lane) * AS;
    uint16_t* tr = reinterpret_cast<uint16_t*>(trace + ((size_t)cb * p.G + lane) * TS);
    int hs = uniform_h ? __builtin_amdgcn_readfirstlane(h) : 0, nres_s = 0;
    int pend = 0;
    // flavours as in K1L: T0 no episode logic, T1 scalar episode test, T2 per-lane
    auto step = [&](int s, int a, auto mode_tag) {
      constexpr int MODE = decltype(mode_tag)::value;
      const int word = *reinterpret_cast<const uint16_t*>(base + cur + 2 * a);  // the one load on the dependency chain
      // The trace entry of the PREVIOUS transition is stored now, behind this transition's read in the LDS queue:
      // stored in its own transition it sits in front of the next read, on the dependency chain.  (The slot before a
      // chunk's first entry is the padding of the neighbouring ring row.)
      tr[s - 1] = (uint16_t)pend;
      pend = word + 2 * a;  // arrival row under the action taken (base.py:1302-1303) | reward code
      const int nxt = word & smask;
      if (MODE == 0) {
        cur = nxt;
      } else if (MODE == 1) {
        ++hs;
        const bool term = hs >= H;
        cur = term ? start_k : nxt;
        hs = term ? 0 : hs;
        nres_s += term ? 1 : 0;
      } else {
        ++h;
        const bool term = episodic && h >= H;  // episodic termination followed at once by reset()
        cur = term ? start_k : nxt;
        h = term ? 0 : h;
        n_resets += term ? 1 : 0;
      }
    };
    using T0 = std::integral_constant<int, 0>;
    using T1 = std::integral_constant<int, 1>;
    using T2 = std::integral_constant<int, 2>;
    int s0 = 0;
    for (; s0 + 8 <= len; s0 += 8) {
      const uint32_t a_lo = *reinterpret_cast<const uint32_t*>(acts + s0);
      const uint32_t a_hi = *reinterpret_cast<const uint32_t*>(acts + s0 + 4);
#define K1P_ACT(j) (int)((((j) < 4 ? a_lo : a_hi) >> (8 * ((j) & 3))) & 0xffu)
      if (uniform_h && hs + 8 < H) {
        step(s0 + 0, K1P_ACT(0), T0{}); step(s0 + 1, K1P_ACT(1), T0{}); step(s0 + 2, K1P_ACT(2), T0{});
        step(s0 + 3, K1P_ACT(3), T0{}); step(s0 + 4, K1P_ACT(4), T0{}); step(s0 + 5, K1P_ACT(5), T0{});
        step(s0 + 6, K1P_ACT(6), T0{}); step(s0 + 7, K1P_ACT(7), T0{});
        hs += 8;
      } else if (uniform_h && H >= 8) {
        const int jstar = H - hs - 1;  // exactly one episode ends inside this group, after transition jstar
#define K1P_STEP_R(j)                         \
  step(s0 + (j), K1P_ACT(j), T0{});           \
  if (jstar == (j)) { cur = start_k; ++nres_s; }
        K1P_STEP_R(0) K1P_STEP_R(1) K1P_STEP_R(2) K1P_STEP_R(3) K1P_STEP_R(4) K1P_STEP_R(5) K1P_STEP_R(6) K1P_STEP_R(7)
#undef K1P_STEP_R
        hs = 7 - jstar;
      } else if (uniform_h) {
        step(s0 + 0, K1P_ACT(0), T1{}); step(s0 + 1, K1P_ACT(1), T1{}); step(s0 + 2, K1P_ACT(2), T1{});
        step(s0 + 3, K1P_ACT(3), T1{}); step(s0 + 4, K1P_ACT(4), T1{}); step(s0 + 5, K1P_ACT(5), T1{});
        step(s0 + 6, K1P_ACT(6), T1{}); step(s0 + 7, K1P_ACT(7), T1{});
      } else {
        step(s0 + 0, K1P_ACT(0), T2{}); step(s0 + 1, K1P_ACT(1), T2{}); step(s0 + 2, K1P_ACT(2), T2{});
        step(s0 + 3, K1P_ACT(3), T2{}); step(s0 + 4, K1P_ACT(4), T2{}); step(s0 + 5, K1P_ACT(5), T2{});
        step(s0 + 6, K1P_ACT(6), T2{}); step(s0 + 7, K1P_ACT(7), T2{});
      }
#undef K1P_ACT
    }
    for (; s0 < len; ++s0) {  // ragged tail of the launch's last chunk
      const int a = acts[s0];
      if (uniform_h) step(s0, a, T1{}); else step(s0, a, T2{});
    }
    tr[len - 1] = (uint16_t)pend;
    if (uniform_h) { h = hs; n_resets += nres_s; }
  };
  // counts (wave 1): the chunk the chain traced into buffer `tb`
  auto counts_body = [&](int tb, int plen) {
    if (!owner || plen <= 0) return;
    const unsigned char* trb = trace + ((size_t)tb * p.G + lane) * TS;
    // 8-bit counters, read-modify-write by their only owner (LDS executes a wave's operations in order).  Two
    // transitions per round trip: both counter reads are in flight together, and the second takes the first's
    // result when they hit the same row.  A wrap goes to the overflow list, branch-free: the slot behind the
    // last entry is only kept on a wrap.
    auto count2 = [&](int x0, int x1) {
      const int r0 = c8[x0], r1 = c8[x1];
      const int c0 = r0 + 1;
      const int c1 = (x1 == x0 ? (c0 & 255) : r1) + 1;
      ovf[n_ovf] = (uint16_t)x0;
      n_ovf += c0 >> 8;
      ovf[n_ovf] = (uint16_t)x1;
      n_ovf += c1 >> 8;
      c8[x0] = (uint8_t)c0;
      c8[x1] = (uint8_t)c1;
    };
    auto count1 = [&](int x0) {
      const int c0 = (int)c8[x0] + 1;
      ovf[n_ovf] = (uint16_t)x0;
      n_ovf += c0 >> 8;
      c8[x0] = (uint8_t)c0;
    };
    int s0 = 0;
    for (; s0 + 4 <= plen; s0 += 4) {
      const uint32_t e0 = *reinterpret_cast<const uint32_t*>(trb + 2 * s0);
      const uint32_t e1 = *reinterpret_cast<const uint32_t*>(trb + 2 * s0 + 4);
      count2((int)((e0 & (uint32_t)smask) >> 1), (int)(((e0 >> 16) & (uint32_t)smask) >> 1));
      count2((int)((e1 & (uint32_t)smask) >> 1), (int)(((e1 >> 16) & (uint32_t)smask) >> 1));
    }
    for (; s0 < plen; ++s0) count1((int)((reinterpret_cast<const uint16_t*>(trb)[s0] & smask) >> 1));
  };
  // rewards (wave 4)
  auto rewards_body = [&](int tb, int plen) {
    if (!owner || plen <= 0) return;
    const unsigned char* trb = trace + ((size_t)tb * p.G + lane) * TS;
    int s0 = 0;
    for (; s0 + 4 <= plen; s0 += 4) {
      const uint32_t e0 = *reinterpret_cast<const uint32_t*>(trb + 2 * s0);
      const uint32_t e1 = *reinterpret_cast<const uint32_t*>(trb + 2 * s0 + 4);
      const double r0 = rv2[(e0 & 0xffffu) >> p.code_shift], r1 = rv2[e0 >> (16 + p.code_shift)];
      const double r2 = rv2[(e1 & 0xffffu) >> p.code_shift], r3 = rv2[e1 >> (16 + p.code_shift)];
      sum += r0; sum += r1; sum += r2; sum += r3;  // transition order
    }
    for (; s0 < plen; ++s0) sum += rv2[reinterpret_cast<const uint16_t*>(trb)[s0] >> p.code_shift];
  };

  // Wavefronts w and w + 4 of a workgroup share a SIMD (the dispatcher deals them out in a fixed rotation from an
  // arbitrary start, tools/calib/wave_placement.hip): the chain and the counters keep a SIMD to themselves apart from
  // the light reward adder (wave 4; wave 5 idles); the four producers share the other two SIMDs
  const int pidx = wave == 2 ? 0 : wave == 3 ? 1 : wave == 6 ? 2 : wave == 7 ? 3 : -1;
  if (n_steps > 0 && pidx >= 0) produce(0, 0, (int)min((int64_t)CH, n_steps), pidx);
  __syncthreads();
  // Pipeline iteration: the chain walks chunk `cb` (len transitions) while the bookkeepers take the chunk before it
  // (plen) and the producers fill the one after.  Every wave keeps its own copy of these (uniform) counters and runs
  // its own compact loop -- one shared loop dispatching on the role cost ~0.6 us per iteration in far branches.
  int since_flush = 0, cb = 0, len = 0, plen = 0;
  int64_t left = n_steps;  // transitions the chain has not walked yet
  bool last = false, flush_now = false;
  auto begin_iter = [&]() {
    plen = len;
    len = (int)min((int64_t)CH, left);
    left -= len;
  };
  auto end_iter = [&]() {
    since_flush += plen;
    last = len == 0;  // the bookkeepers have just drained the final chunk
    // 8-bit deltas wrap at most once per 256 transitions of their instance; the overflow list holds K1L_OVF wraps
    flush_now = (since_flush + CH > 256 * K1L_OVF) || last;
    cb ^= 1;
  };
  for (;;) {
    if (wave == 0) {
      do {
        begin_iter();
        chain_body(cb, len);
        end_iter();
        if (flush_now && owner) {
          resets[lane] = n_resets;
          n_resets_total += n_resets;
          n_resets = 0;
        }
        __syncthreads();
      } while (!flush_now);
    } else if (wave == 1) {
      do {
        begin_iter();
        counts_body(cb ^ 1, plen);
        end_iter();
        __syncthreads();
      } while (!flush_now);
    } else if (wave == 4) {
      do {
        begin_iter();
        rewards_body(cb ^ 1, plen);
        end_iter();
        __syncthreads();
      } while (!flush_now);
    } else if (pidx >= 0) {
      do {
        begin_iter();
        if (left > 0) produce(cb ^ 1, n_steps - left, (int)min((int64_t)CH, left), pidx);
        end_iter();
        __syncthreads();
      } while (!flush_now);
    } else {
      do {
        begin_iter();
        end_iter();
        __syncthreads();
      } while (!flush_now);
    }
    flush_counts<true, true, K1P_THREADS>(t.visits_sa + row00, total_rows, rows, A, slots, p, resets, nullptr, tid);
    flush_counts<false, true, K1P_THREADS>(t.visits_s + so0, total_states, S, A, slots, p, resets, t.start_state + t.start_off[g0], tid);
    __syncthreads();
    if (wave == 1 && owner) {  // every recorded wrap is worth 256 visits
      for (int e = 0; e < n_ovf; ++e) {
        const int r = ovf[e];
        t.visits_sa[row00 + (int64_t)lane * rows + r] += 256;
        t.visits_s[so0 + (int64_t)lane * S + r / A] += 256;
      }
      n_ovf = 0;
    }
    if (last) break;
    for (int j = tid; j < nb * cnt_dwords; j += K1P_THREADS) {
      const int slot = j / cnt_dwords, off = j - slot * cnt_dwords;
      reinterpret_cast<uint32_t*>(slots + (size_t)slot * p.slot_bytes + p.off_cnt)[off] = 0u;
    }
    since_flush = 0;
    __syncthreads();
  }
  if (wave == 0 && owner) {
    cur /= 2 * A;
    t.cur[b] = cur;
    t.hstep[b] = h;
    t.n_trans[b] = my_ntr + (unsigned long long)n_steps;
    t.n_reset[b] += (unsigned long long)n_resets_total;
    if (n_resets_total) t.prev_start[b] = t.last_start[b];   // (as K1L)
    if (last_obs) last_obs[b] = cur;  // the state after the last transition (the start state after a termination)
  }
  if (wave == 4 && owner && reward_sum) reward_sum[b] = sum;
}

template <bool ROWS, bool BYTES, int NT>
__device__ __forceinline__ void flush_counts(int32_t* __restrict__ dst, int total, int per, int A, unsigned char* slots,
                                             const LdsPlan& p, const int32_t* resets, const int32_t* start_states,
                                             int tid) {
  auto delta = [&](int slot, int off) -> int {
    const unsigned char* cb = slots + (size_t)slot * p.slot_bytes + p.off_cnt;
    const uint16_t* c16 = reinterpret_cast<const uint16_t*>(cb);
    if (ROWS) return BYTES ? (int)cb[off] : (int)c16[off];
    int acc = (off == start_states[slot]) ? resets[slot] : 0;
    for (int a = 0; a < A; ++a) acc += BYTES ? (int)cb[off * A + a] : (int)c16[off * A + a];
    return acc;
  };
  const int head = (int)((reinterpret_cast<uintptr_t>(dst) & 15) >> 2);  // counters before the first aligned chunk
  const int lead = head ? min(4 - head, total) : 0;
  const int nfull = (total - lead) >> 2;
  const int tail0 = lead + 4 * nfull;
  if (tid < lead) {
    const int d = delta(tid / per, tid % per);
    if (d) dst[tid] += d;
  }
  if (tid >= 64 && tid - 64 < total - tail0) {
    const int j = tail0 + tid - 64;
    const int d = delta(j / per, j % per);
    if (d) dst[j] += d;
  }
  int4* vdst = reinterpret_cast<int4*>(dst + lead);
  // (reading only the 16-byte groups whose deltas are nonzero was measured SLOWER: the loads lose their batching)
  for (int c0 = 0; c0 < nfull; c0 += NT * K1L_UNROLL) {
    int4 old[K1L_UNROLL];
#pragma unroll
    for (int k = 0; k < K1L_UNROLL; ++k) {
      const int c = c0 + k * NT + tid;
      if (c < nfull) old[k] = vdst[c];
    }
#pragma unroll
    for (int k = 0; k < K1L_UNROLL; ++k) {
      const int c = c0 + k * NT + tid;
      if (c < nfull) {
        int j = lead + 4 * c;
        int slot = j / per, off = j - slot * per;
        int d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e, ++off) {
          if (off == per) { off = 0; ++slot; }
          d[e] = delta(slot, off);
        }
        if (d[0] | d[1] | d[2] | d[3]) {
          old[k].x += d[0]; old[k].y += d[1]; old[k].z += d[2]; old[k].w += d[3];
          vdst[c] = old[k];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// K1D: dense-row layout (CMDP_LAYOUT_DENSE, the layout BASELINE.json's north star names): every instance
// keeps its float32 P[s,a,:] rows (row stride `spad` floats) in HBM.  One WAVEFRONT per instance: per
// transition the 64 lanes stream the row with 16-byte coalesced loads, form exact float64 partial sums, take a
// wavefront inclusive prefix sum (6 shuffle steps) and pick next = min{ j : cum_j > u * total } with a ballot.
// Algorithmic bytes per transition: 4*S (row) + 28 -- this kernel is genuinely HBM-bound.
// The prefix sums are exact in float64 (probabilities are >= 2^-28, checked at create time), so their
// association does not matter and the result equals the oracle's sequential scan bit for bit.
// ---------------------------------------------------------------------------------------------------
struct DenseArgs {
  const float* P;   // [R][spad]
  int32_t spad;     // multiple of 256
};

// (A DPP row_shr / row_bcast version of this scan was measured 9 % SLOWER in K1D: every DPP move is a dependent VALU
// instruction with hazard wait states, while the ds_bpermute latency below is hidden by the other resident waves.)
__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}

// NV = float4 loads per lane per row (row stride = 256 * NV floats); the row stays in registers between the
// partial-sum pass and the search pass.  The Philox work of a wavefront is spread over its lanes: every 64
// transitions lane j computes the transition uniform of transition base+j and the action block base/4+j, and
// the per-transition values are then broadcast with one shuffle each (values are wave-uniform anyway).
// NI = instances per wavefront.  A transition is one dependent chain -- row address -> 2 KB row from HBM -> scan ->
// successor -- so a wavefront with one instance has ONE row in flight and idles for the HBM latency (16 wavefronts per CU
// x 2 KB = 32 KB in flight per CU, half of what covers the latency at 8 TB/s).  With NI = 2 the wavefront walks two
// instances in one instruction stream, software-pipelined half a transition apart: the row of one is in flight while the
// other's is scanned (`issue` = everything up to the loads, `consume` = everything after).  Per-instance state is
// indexed by compile-time constants only (registers, no scratch).
template <int NV>
struct DenseWalk {
  // persistent
  int b;
  int64_t soff, ebase;
  int S_b;
  uint2 key;
  int32_t cur, h;
  unsigned long long nt, nr, base;
  double sum, u_lane;
  uint32_t acts_lane;
  // in flight between issue and consume
  float4 v[NV];
  RowDesc d;
  double u;
  int a;
};

template <int POLICY, int NV, bool BETA, int NI>
__global__ void __launch_bounds__(256) k_rollout_dense(EnvTables t, DenseArgs dn, const int8_t* __restrict__ actions,
                                                       int64_t n_steps, double* __restrict__ reward_sum,
                                                       int32_t* __restrict__ last_obs) {
  const int lane = threadIdx.x & 63;
  // the instance index and everything derived from it is wave-uniform: readfirstlane tells the compiler, and the walkers'
  // state (current state, counters, keys, offsets, the row descriptor) lives in scalar registers -- VGPRs, which set the
  // occupancy, are left to the row itself and the scan
  const int b0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))) * NI;
  if (b0 >= t.B) return;  // whole wavefronts leave together
  DenseWalk<NV> w[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int b = (b0 + i < t.B) ? b0 + i : b0;  // an odd batch: the last wavefront's second walker stays idle
    w[i].b = b;
    w[i].soff = t.state_off[b];
    w[i].ebase = t.entry_base[b];
    w[i].S_b = (int)(t.state_off[b + 1] - w[i].soff);
    w[i].key = t.philox_key[b];
    w[i].cur = t.cur[b];
    w[i].h = t.hstep[b];
    w[i].nt = t.n_trans[b];
    w[i].nr = t.n_reset[b];
    w[i].base = w[i].nt;
    w[i].sum = 0.0;
    w[i].u_lane = 0.0;
    w[i].acts_lane = 0;
  }
  const bool second_is_real = NI == 1 || b0 + 1 < t.B;

  // everything of a transition up to and including its loads
  auto issue = [&](DenseWalk<NV>& x, int64_t step) {
    const int i = (int)(x.nt - x.base);
    if (i == 0 || i == 64) {  // refill: 64 transitions' worth of random numbers, one Philox block per lane
      x.base = x.nt;
      uint32_t r4[4];
      const unsigned long long n = x.base + (unsigned long long)lane;
      philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), 0u, 0u, x.key.x, x.key.y, r4);
      x.u_lane = u53(r4[0], r4[1]);
      if (POLICY == 0) {
        const unsigned long long q = (x.base >> 2) + (unsigned long long)lane;
        philox_act4(q, x.key, t.A, philox_act_lg(t.A), r4);
        x.acts_lane = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) x.acts_lane |= r4[j] << (8 * j);
      }
    }
    // wave-uniform lane indices: v_readlane (scalar result, no LDS round trip) instead of a shuffle
    const int idx = __builtin_amdgcn_readfirstlane((int)(x.nt - x.base));
    x.u = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x.u_lane), idx),
                           __builtin_amdgcn_readlane(__double2loint(x.u_lane), idx));
    if (POLICY == 1) {
      x.a = (int)actions[step * t.B + x.b];
    } else {
      const int widx = __builtin_amdgcn_readfirstlane((int)((x.nt >> 2) - (x.base >> 2)));
      const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)x.acts_lane, widx);
      x.a = (int)((word >> (8 * (int)(x.nt & 3))) & 0xffu);
    }
    ++x.nt;
    ++x.h;
    const int64_t r = (x.soff + x.cur) * t.A + x.a;
    const float4* row = reinterpret_cast<const float4*>(dn.P + r * dn.spad + (int64_t)lane * (4 * NV));
#pragma unroll
    for (int q = 0; q < NV; ++q)  // the padding behind the last state is all zeros: not fetched
      x.v[q] = (lane * (4 * NV) + 4 * q < x.S_b) ? row[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    x.d = t.row[r];  // independent of the row data: in flight together with it
  };

  // everything after the loads: the successor, the reward, the counters, the episode end
  auto consume = [&](DenseWalk<NV>& x) {
    // exact float64 prefix sums inside the lane (kept in registers), then across the wave
    double cl[4 * NV];
    double part = 0.0;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      part += (double)x.v[q].x; cl[4 * q + 0] = part;
      part += (double)x.v[q].y; cl[4 * q + 1] = part;
      part += (double)x.v[q].z; cl[4 * q + 2] = part;
      part += (double)x.v[q].w; cl[4 * q + 3] = part;
    }
    const double incl = wave_incl_scan(part, lane);
    const double total = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(incl), 63),
                                          __builtin_amdgcn_readlane(__double2loint(incl), 63));
    const double xx = x.u * total;
    const double excl = incl - part;
    // next = min{ j : cum_j > x }.  The cumulative sums are non-decreasing and only grow at non-zero columns, so the
    // first lane whose inclusive total exceeds x holds the column, and inside it the column is the number of its
    // prefix sums that are still <= x (all sums are exact, so excl + cl[i] is the sequential scan's value).
    const unsigned long long m = __ballot(incl > xx);
    int nxt;
    if (m) {
      int cnt = 0;
#pragma unroll
      for (int i = 0; i < 4 * NV; ++i) cnt += (excl + cl[i] <= xx) ? 1 : 0;
      nxt = __builtin_amdgcn_readlane(lane * (4 * NV) + cnt, __ffsll((long long)m) - 1);
    } else {  // u * total rounded up to total: the last non-zero column of the row
      int last_nz = -1;
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const float e[4] = {x.v[q].x, x.v[q].y, x.v[q].z, x.v[q].w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (e[k] != 0.0f) last_nz = lane * (4 * NV) + q * 4 + k;
      }
      const unsigned long long mz = __ballot(last_nz >= 0);
      nxt = __builtin_amdgcn_readfirstlane(__shfl(last_nz, 63 - __clzll((long long)mz), 64));
    }
    // reward of the sampler entry (s, a, nxt)
    const RowDesc d = x.d;
    double rraw = d.reward_if_det;
    int64_t ent = x.ebase + d.first;
    if (d.n > 1) {
      int found = -1;
      for (int k0 = 0; k0 < d.n && found < 0; k0 += 64) {
        const int k = k0 + lane;
        const bool eq = k < d.n && t.sp_next[x.ebase + d.first + k] == nxt;
        const unsigned long long me = __ballot(eq);
        if (me) found = k0 + __ffsll((long long)me) - 1;
      }
      ent += found;
      rraw = t.sp_reward[ent];
    }
    if (BETA && t.sp_rkind && t.sp_rkind[ent] == 1) rraw = philox_beta(t.sp_rp0[ent], t.sp_rp1[ent], x.nt - 1, x.key, t.beta_gammas);
    x.sum += rraw * t.rscale - t.rmin;
    if (lane == 0) {
      bump(t.visits_s + x.soff + nxt);
      bump(t.visits_sa + (x.soff + nxt) * t.A + x.a);
    }
    x.cur = nxt;
    if (t.H > 0 && x.h >= t.H) {
      int32_t s0 = 0;
      unsigned long long nr_lane0 = x.nr;
      if (lane == 0) s0 = env_reset(t, x.b, x.soff, x.key, nr_lane0);
      x.nr += 1;  // what env_reset did to lane 0's copy: the counter itself stays wave-uniform
      x.cur = __builtin_amdgcn_readfirstlane(s0);
      x.h = 0;
    }
  };

  if (n_steps > 0) {
    if constexpr (NI == 1) {
      for (int64_t step = 0; step < n_steps; ++step) {
        issue(w[0], step);
        consume(w[0]);
      }
    } else {
      issue(w[0], 0);
      for (int64_t step = 0; step < n_steps; ++step) {
        if (second_is_real) issue(w[1], step);
        consume(w[0]);
        if (step + 1 < n_steps) issue(w[0], step + 1);
        if (second_is_real) consume(w[1]);
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (i == 0 || second_is_real) {
        const int b = w[i].b;
        t.cur[b] = w[i].cur;
        t.hstep[b] = w[i].h;
        t.n_trans[b] = w[i].nt;
        t.n_reset[b] = w[i].nr;
        if (reward_sum) reward_sum[b] = w[i].sum;
        if (last_obs) last_obs[b] = w[i].cur;
      }
    }
  }
}

// scatter of the CSR non-zeros into the (zero-filled) dense rows
__global__ void k_dense_fill(float* __restrict__ P, int spad, const int64_t* __restrict__ csr_ptr,
                             const int32_t* __restrict__ csr_col, const float* __restrict__ csr_val, int64_t n_rows) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  for (int64_t k = csr_ptr[r]; k < csr_ptr[r + 1]; ++k) P[r * spad + csr_col[k]] = csr_val[k];
}

// ===================================================================================================
// Dynamic programming
// ===================================================================================================
struct DpTables {
  int32_t B, A;
  const int64_t* state_off;  // [B+1]
  const int64_t* csr_ptr;    // [R+1] global offsets
  const int32_t* csr_col;
  const float* csr_val;
  const float* R;            // [R] (already the override when one was given)
  const float* pi;           // [R] or null
  const int64_t* unit_off;   // DIAM: [B+1] prefix of targets (== state_off); else null
  float gamma;
  double eps;
  double max_abs;            // <= 0: off
  int64_t max_sweeps;
  float* Q;                  // [R]        (null for DIAM)
  float* V;                  // [NSTATES]  (null for DIAM)
  int64_t* sweeps;           // [units] or null
  float* per_target;         // DIAM: [NSTATES] = -min V
  int32_t* status;           // [units] 0 ok, -5 max sweeps, -7 max value
};

enum { DP_VI = 0, DP_PE = 1 };

// instance-relative int32 view of the global int64 row-pointer array
struct GPtr {
  const int64_t* p;
  int64_t z;
  __device__ __forceinline__ int operator[](int i) const { return (int)(p[i] - z); }
};

// unit -> (instance, target) for the diameter launches
__device__ __forceinline__ void unit_to_instance(const DpTables& t, int64_t unit, int& b, int& target) {
  if (!t.unit_off) { b = (int)unit; target = -1; return; }
  int lo = 0, hi = t.B;  // largest b with unit_off[b] <= unit
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (t.unit_off[mid] <= unit) lo = mid; else hi = mid;
  }
  b = lo;
  target = (int)(unit - t.unit_off[lo]);
}

// One Bellman backup of state s from value vector Vin.
//   JACOBI VI : q = R + gamma * sum_k val_k * V[col_k]        (infinite_horizon.py:154)
//   otherwise : q = R + sum_k (gamma * val_k) * V[col_k]       (infinite_horizon.py:134,179,200)
// DIAM: target rows are the absorbing row {target: 1} with R = 0, all other rows have R = -1
//       (hardness/measures/diameter.py:85-90).
template <int MODE, bool JACOBI, bool DIAM, bool WRITE_Q, typename PtrT, typename ColT, typename ValT, typename RT>
__device__ __forceinline__ float backup_state(int s, int A, int target, PtrT ptr, ColT col, ValT val, RT Rv,
                                              const float* __restrict__ pi, const float* __restrict__ Vin, float gamma,
                                              float* __restrict__ Qout) {
  float v = 0.0f;
  for (int a = 0; a < A; ++a) {
    const int r = s * A + a;
    float acc = 0.0f;
    float rew;
    if (DIAM && s == target) {
      const float c = (MODE == DP_VI && JACOBI) ? 1.0f : __fmul_rn(gamma, 1.0f);
      acc = __fadd_rn(acc, __fmul_rn(c, Vin[target]));
      rew = 0.0f;
    } else {
      const int lo = ptr[r], hi = ptr[r + 1];
      for (int k = lo; k < hi; ++k) {
        const float c = (MODE == DP_VI && JACOBI) ? val[k] : __fmul_rn(gamma, val[k]);
        acc = __fadd_rn(acc, __fmul_rn(c, Vin[col[k]]));
      }
      rew = DIAM ? -1.0f : Rv[r];
    }
    const float q = (MODE == DP_VI && JACOBI) ? __fadd_rn(rew, __fmul_rn(gamma, acc)) : __fadd_rn(rew, acc);
    if (WRITE_Q) Qout[r] = q;
    if (MODE == DP_VI) {
      v = (a == 0) ? q : fmaxf(v, q);
    } else {
      const float qp = __fmul_rn(q, pi[r]);
      v = (a == 0) ? qp : __fadd_rn(v, qp);
    }
  }
  return v;
}

// K2: Jacobi sweeps, one workgroup per unit.  Dynamic LDS: V ping-pong [2][S], reduction scratch, and
// (CSR_LDS) ptr[S*A+1] (instance-relative int32), col, val, R.
template <int MODE, bool DIAM, bool CSR_LDS>
__global__ void __launch_bounds__(256) k_dp_block(DpTables t) {
  extern __shared__ __align__(16) unsigned char smem[];
  int b, target;
  unit_to_instance(t, blockIdx.x, b, target);
  const int A = t.A;
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int rows = S * A;
  const int64_t row0 = soff * A;
  const int64_t nz0 = t.csr_ptr[row0];
  const int nnz = (int)(t.csr_ptr[row0 + rows] - nz0);
  const int tid = threadIdx.x, nth = blockDim.x, wave = tid >> 6, lane = tid & 63, nwaves = nth >> 6;

  float* Va = reinterpret_cast<float*>(smem);
  float* Vb = Va + S;
  float* red = Vb + S;                 // [2][nwaves][2]
  unsigned char* p = reinterpret_cast<unsigned char*>(red + 4 * nwaves);
  int32_t* lptr = reinterpret_cast<int32_t*>(p);
  int32_t* lcol = lptr + (rows + 1);
  float* lval = reinterpret_cast<float*>(lcol + nnz);
  float* lR = lval + nnz;
  if (CSR_LDS) {
    for (int i = tid; i <= rows; i += nth) lptr[i] = (int32_t)(t.csr_ptr[row0 + i] - nz0);
    for (int i = tid; i < nnz; i += nth) { lcol[i] = t.csr_col[nz0 + i]; lval[i] = t.csr_val[nz0 + i]; }
    if (!DIAM) for (int i = tid; i < rows; i += nth) lR[i] = t.R[row0 + i];
  }
  for (int i = tid; i < S; i += nth) { Va[i] = 0.0f; Vb[i] = 0.0f; }
  __syncthreads();

  const float* pi = (MODE == DP_PE) ? t.pi + row0 : nullptr;
  float* Vold = Va;
  float* Vnew = Vb;
  int64_t it = 0;
  int status = -5;
  while (it < t.max_sweeps) {
    ++it;
    float dmax = 0.0f, vabs = 0.0f;
    for (int s = tid; s < S; s += nth) {
      float v;
      if (CSR_LDS) {
        v = backup_state<MODE, true, DIAM, false>(s, A, target, lptr, lcol, lval, lR, pi, Vold, t.gamma, nullptr);
      } else {
        GPtr gp{t.csr_ptr + row0, nz0};
        v = backup_state<MODE, true, DIAM, false>(s, A, target, gp, t.csr_col + nz0, t.csr_val + nz0, t.R + row0, pi,
                                                  Vold, t.gamma, nullptr);
      }
      Vnew[s] = v;
      dmax = fmaxf(dmax, fabsf(Vold[s] - v));
      vabs = fmaxf(vabs, fabsf(v));
    }
    dmax = wave_max(dmax);
    vabs = wave_max(vabs);
    float* rbuf = red + (it & 1) * 2 * nwaves;
    if (lane == 0) { rbuf[2 * wave] = dmax; rbuf[2 * wave + 1] = vabs; }
    __syncthreads();
    float diff = 0.0f, vmax = 0.0f;
    for (int w = 0; w < nwaves; ++w) { diff = fmaxf(diff, rbuf[2 * w]); vmax = fmaxf(vmax, rbuf[2 * w + 1]); }
    float* tmp = Vold; Vold = Vnew; Vnew = tmp;  // Vold = newest values, Vnew = the vector they were computed from
    if (t.max_abs > 0.0 && (double)vmax > t.max_abs) { status = -7; break; }
    if ((double)diff < t.eps) { status = 0; break; }
  }
  // outputs
  const int64_t unit = blockIdx.x;
  if (tid == 0) {
    t.status[unit] = status;
    if (t.sweeps) t.sweeps[unit] = it;
  }
  if (DIAM) {
    float mn = 3.0e38f;
    for (int s = tid; s < S; s += nth) mn = fminf(mn, Vold[s]);
    mn = wave_min(mn);
    __syncthreads();
    if (lane == 0) red[wave] = mn;
    __syncthreads();
    if (tid == 0) {
      float m = red[0];
      for (int w = 1; w < nwaves; ++w) m = fminf(m, red[w]);
      t.per_target[soff + target] = -m;
    }
  } else {
    // Q of the last sweep is a function of the vector that sweep read (now in Vnew); recomputing it
    // repeats the identical arithmetic.
    for (int s = tid; s < S; s += nth) {
      t.V[soff + s] = Vold[s];
      if (it > 0) {
        if (CSR_LDS) {
          backup_state<MODE, true, false, true>(s, A, -1, lptr, lcol, lval, lR, pi, Vnew, t.gamma, t.Q + row0);
        } else {
          GPtr gp{t.csr_ptr + row0, nz0};
          backup_state<MODE, true, false, true>(s, A, -1, gp, t.csr_col + nz0, t.csr_val + nz0, t.R + row0, pi, Vnew,
                                                t.gamma, t.Q + row0);
        }
      }
    }
  }
}

// K2R: Jacobi sweeps with the instance's CSR held in REGISTERS.  One 256-thread workgroup per instance,
// thread t owns states t, t+256, ... (SPT of them) and keeps the (column, coefficient) pairs of all their
// A x KMAX row entries plus R in VGPRs for the whole solve: a sweep touches LDS only for the V gathers and the
// V write (no CSR traffic at all, no bank-conflicting table walks), one barrier per sweep.  Rows shorter than
// KMAX are padded with (col 0, coefficient +0.0): acc + 0*V[0] == acc exactly, so the padded sum is bit-equal
// to the reference's in-order accumulation.  HBM traffic: the CSR once per solve, Q/V once at the end.
template <int MODE, int A_T, int KMAX, int SPT>
__global__ void __launch_bounds__(256) k_dp_reg(DpTables t) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.x;
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int64_t row0 = soff * A_T;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  constexpr int NW = 4;
  // The two value vectors sit at COMPILE-TIME offsets (0 and VB_OFF) and the sweep body exists once per parity, so a
  // gather is `ds_read_b32 v, col4 offset:<const>`: the byte offsets col*4 live in registers for the whole solve and no
  // address arithmetic is left in the loop.
  constexpr int VB_OFF = SPT * 256 * 4;
  float* red = reinterpret_cast<float*>(smem + 2 * VB_OFF);  // [2][NW][2]

  int32_t col4[SPT][A_T][KMAX];
  float cf[SPT][A_T][KMAX];
  float Rr[SPT][A_T], Pi[SPT][A_T];
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * 256;
#pragma unroll
    for (int a = 0; a < A_T; ++a) {
      const int64_t r = row0 + (int64_t)s * A_T + a;
      int64_t lo = 0, hi = 0;
      if (s < S) { lo = t.csr_ptr[r]; hi = t.csr_ptr[r + 1]; }
      Rr[j][a] = (s < S) ? t.R[r] : 0.0f;
      Pi[j][a] = (MODE == DP_PE && s < S) ? t.pi[r] : 0.0f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const bool in = lo + k < hi;
        col4[j][a][k] = in ? 4 * t.csr_col[lo + k] : 0;
        const float v = in ? t.csr_val[lo + k] : 0.0f;
        // PE (and every non-Jacobi-VI form) multiplies the coefficient by gamma first: `(gamma * T) @ V`
        cf[j][a][k] = (MODE == DP_PE) ? __fmul_rn(t.gamma, v) : v;
      }
    }
  }
  for (int i = tid; i < 2 * SPT * 256; i += 256) reinterpret_cast<float*>(smem)[i] = 0.0f;
  __syncthreads();

  const bool track_abs = t.max_abs > 0.0;
  int64_t it = 0;
  int status = -5;
  // one Jacobi sweep reading the vector at byte offset RD and writing the one at WR; Q rows go to `qout` when given
  auto backup = [&](auto rd_tag, int j, int a) -> float {
    constexpr int RD = decltype(rd_tag)::value;
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      acc = __fadd_rn(acc, __fmul_rn(cf[j][a][k], *reinterpret_cast<const float*>(smem + RD + col4[j][a][k])));
    return (MODE == DP_VI) ? __fadd_rn(Rr[j][a], __fmul_rn(t.gamma, acc)) : __fadd_rn(Rr[j][a], acc);
  };
  auto sweep = [&](auto rd_tag) -> int {
    constexpr int RD = decltype(rd_tag)::value, WR = VB_OFF - RD;
    ++it;
    float dmax = 0.0f, vabs = 0.0f;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tid + j * 256;
      if (s < S) {
        float v = 0.0f;
#pragma unroll
        for (int a = 0; a < A_T; ++a) {
          const float q = backup(rd_tag, j, a);
          if (MODE == DP_VI) {
            v = (a == 0) ? q : fmaxf(v, q);
          } else {
            const float qp = __fmul_rn(q, Pi[j][a]);
            v = (a == 0) ? qp : __fadd_rn(v, qp);
          }
        }
        *reinterpret_cast<float*>(smem + WR + 4 * s) = v;
        dmax = fmaxf(dmax, fabsf(*reinterpret_cast<const float*>(smem + RD + 4 * s) - v));
        if (track_abs) vabs = fmaxf(vabs, fabsf(v));
      }
    }
    dmax = wave_max_lane63(dmax);
    if (track_abs) vabs = wave_max_lane63(vabs);
    float* rbuf = red + (it & 1) * 2 * NW;  // [NW] max|dV| then [NW] max|V|, 16-byte aligned
    if (lane == 63) {
      rbuf[wave] = dmax;
      if (track_abs) rbuf[NW + wave] = vabs;
    }
    __syncthreads();
    const float4 d4 = *reinterpret_cast<const float4*>(rbuf);
    const float diff = fmaxf(fmaxf(d4.x, d4.y), fmaxf(d4.z, d4.w));
    float vmax = 0.0f;
    if (track_abs) {
      const float4 a4 = *reinterpret_cast<const float4*>(rbuf + NW);
      vmax = fmaxf(fmaxf(a4.x, a4.y), fmaxf(a4.z, a4.w));
    }
    if (track_abs && (double)vmax > t.max_abs) return 2;
    if ((double)diff < t.eps) return 1;
    return 0;
  };
  using Even = std::integral_constant<int, 0>;
  using Odd = std::integral_constant<int, VB_OFF>;
  int newest = 0;  // byte offset of the newest vector after the loop
  while (it < t.max_sweeps) {
    int rc = sweep(Even{});  // reads Va (offset 0), writes Vb
    newest = VB_OFF;
    if (rc == 0 && it < t.max_sweeps) {
      rc = sweep(Odd{});     // reads Vb, writes Va
      newest = 0;
    }
    if (rc) { status = (rc == 1) ? 0 : -7; break; }
  }
  if (tid == 0) {
    t.status[b] = status;
    if (t.sweeps) t.sweeps[b] = it;
  }
  // Q of the last sweep = the same arithmetic on the vector that sweep read (the older one)
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * 256;
    if (s < S) {
      t.V[soff + s] = *reinterpret_cast<const float*>(smem + newest + 4 * s);
#pragma unroll
      for (int a = 0; a < A_T; ++a) {
        const float q = (newest == VB_OFF) ? backup(Even{}, j, a) : backup(Odd{}, j, a);
        t.Q[row0 + (int64_t)s * A_T + a] = q;
      }
    }
  }
}

// K2U: K2R with the gathers of a state DEDUPLICATED.  The A rows of a state mostly name the same few successor
// states (grid worlds: the four neighbours and the state itself, whatever the action), so K2R's A x KMAX gathers fetch
// the same <= U values over and over -- and the kernel is bound by exactly that LDS gather traffic.  Here a thread keeps,
// per owned state, the sorted list of its U distinct successor columns and a DENSE A x U coefficient matrix over them
// (both built in registers when the kernel starts); a sweep gathers U values once and every action's expectation is the
// ascending-column sum over all U of them.  The terms a row does not have carry the coefficient +0.0 and leave the
// partial sum unchanged, so the result equals the row's own in-order accumulation (the same argument as K2R's
// padding; values are finite: `max_abs_value` / gamma < 1).  U gathers and 2 A U float operations instead of A x KMAX and
// 2 A KMAX.  Chosen by run_sweeps when the batch's states have <= 8 distinct successors and U <= A KMAX / 2.
// (Packed-FP32 arithmetic, two actions per v_pk_mul_f32 / v_pk_add_f32, was measured 3 % slower: the kernel is bound by
// the latency of its gather -> sum -> reduce -> barrier chain at 4 workgroups per CU, not by VALU throughput.)
// Occupancy: the sweep is a latency chain (gather -> sums -> wave reduce -> barrier), so one more workgroup per CU pays
// for a few spilled registers: measured at C3 (A=4, U=5, SPT=2: 103 VGPRs unconstrained) 4 / 5 / 6 waves per SIMD =
// 2.93 / 2.65 / 2.75 ms.  The cap follows the registers the resident tables need.
#define K2U_WAVES(A, U, SPT) (((SPT) * ((A) * (U) + (U) + (A)) + 30) <= 96 ? 5 : (((SPT) * ((A) * (U) + (U) + (A)) + 30) <= 128 ? 4 : 3))
template <int MODE, int A_T, int U_T, int KMAX, int SPT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(K2U_WAVES(A_T, U_T, SPT), K2U_WAVES(A_T, U_T, SPT))))
k_dp_regu(DpTables t) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.x;
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int64_t row0 = soff * A_T;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  constexpr int NW = 4;
  constexpr int VB_OFF = SPT * 256 * 4;
  constexpr int SENT = 0x7fffffff;
  float* red = reinterpret_cast<float*>(smem + 2 * VB_OFF);  // [2][NW][2]

  // LDS pointers (address space 3) of the distinct successors' values in vector A; the other vector is VB_OFF bytes on,
  // which folds into the instruction's offset field
  typedef const __attribute__((address_space(3))) float* lds_cf;
  typedef __attribute__((address_space(3))) float* lds_f;
  const lds_f vbase = (lds_f)(__attribute__((address_space(3))) unsigned char*)smem;
  lds_cf vp[SPT][U_T];
  float W[SPT][A_T][U_T];
  float Rr[SPT][A_T], Pi[SPT][A_T];
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * 256;
    int32_t ucol[U_T];
#pragma unroll
    for (int u = 0; u < U_T; ++u) ucol[u] = SENT;
    int32_t ecol[A_T][KMAX];
    float ecf[A_T][KMAX];
#pragma unroll
    for (int a = 0; a < A_T; ++a) {
      const int64_t r = row0 + (int64_t)s * A_T + a;
      int64_t lo = 0, hi = 0;
      if (s < S) { lo = t.csr_ptr[r]; hi = t.csr_ptr[r + 1]; }
      Rr[j][a] = (s < S) ? t.R[r] : 0.0f;
      Pi[j][a] = (MODE == DP_PE && s < S) ? t.pi[r] : 0.0f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const bool in = lo + k < hi;
        ecol[a][k] = in ? t.csr_col[lo + k] : SENT;
        const float v = in ? t.csr_val[lo + k] : 0.0f;
        ecf[a][k] = (MODE == DP_PE) ? __fmul_rn(t.gamma, v) : v;
        // sorted insertion without duplicates: the larger of (carried, slot) moves on
        int32_t c = ecol[a][k];
#pragma unroll
        for (int u = 0; u < U_T; ++u) {
          const int32_t cur = ucol[u];
          const bool dup = c == cur;
          const bool less = c < cur;
          ucol[u] = less ? c : cur;
          c = dup ? SENT : (less ? cur : c);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U_T; ++u) {
      vp[j][u] = vbase + (ucol[u] == SENT ? 0 : ucol[u]);
#pragma unroll
      for (int a = 0; a < A_T; ++a) {
        float w = 0.0f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) w = (ecol[a][k] == ucol[u] && ucol[u] != SENT) ? ecf[a][k] : w;
        W[j][a][u] = w;
      }
    }
  }
  for (int i = tid; i < 2 * SPT * 256; i += 256) reinterpret_cast<float*>(smem)[i] = 0.0f;
  __syncthreads();

  const bool track_abs = t.max_abs > 0.0;
  int64_t it = 0;
  int status = -5;
  auto backup_all = [&](auto rd_tag, int j, float (&q)[A_T]) {
    constexpr int RD = decltype(rd_tag)::value;
    float v[U_T];
#pragma unroll
    for (int u = 0; u < U_T; ++u) v[u] = vp[j][u][RD / 4];
#pragma unroll
    for (int a = 0; a < A_T; ++a) {
      float acc = 0.0f;
#pragma unroll
      for (int u = 0; u < U_T; ++u) acc = __fadd_rn(acc, __fmul_rn(W[j][a][u], v[u]));
      q[a] = (MODE == DP_VI) ? __fadd_rn(Rr[j][a], __fmul_rn(t.gamma, acc)) : __fadd_rn(Rr[j][a], acc);
    }
  };
  auto sweep = [&](auto rd_tag) -> int {
    constexpr int RD = decltype(rd_tag)::value, WR = VB_OFF - RD;
    ++it;
    float dmax = 0.0f, vabs = 0.0f;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tid + j * 256;
      if (s < S) {
        float q[A_T];
        backup_all(rd_tag, j, q);
        float v = 0.0f;
        if (MODE == DP_VI) {  // values are never NaN: bare max instructions
          if constexpr (A_T == 2) v = fmax_nn(q[0], q[1]);
          else if constexpr (A_T == 3) v = fmax3_nn(q[0], q[1], q[2]);
          else v = fmax_nn(fmax3_nn(q[0], q[1], q[2]), q[A_T - 1]);
        } else {
#pragma unroll
          for (int a = 0; a < A_T; ++a) {
            const float qp = __fmul_rn(q[a], Pi[j][a]);
            v = (a == 0) ? qp : __fadd_rn(v, qp);
          }
        }
        const float vold = vbase[RD / 4 + s];
        vbase[WR / 4 + s] = v;
        dmax = fmax_abs_nn(dmax, vold - v);
        if (track_abs) vabs = fmax_abs_nn(vabs, v);
      }
    }
    dmax = wave_max_lane63_nn(dmax);
    if (track_abs) vabs = wave_max_lane63_nn(vabs);
    float* rbuf = red + (it & 1) * 2 * NW;
    if (lane == 63) {
      rbuf[wave] = dmax;
      if (track_abs) rbuf[NW + wave] = vabs;
    }
    __syncthreads();
    const float4 d4 = *reinterpret_cast<const float4*>(rbuf);
    const float diff = fmax_nn(fmax3_nn(d4.x, d4.y, d4.z), d4.w);
    float vmax = 0.0f;
    if (track_abs) {
      const float4 a4 = *reinterpret_cast<const float4*>(rbuf + NW);
      vmax = fmax_nn(fmax3_nn(a4.x, a4.y, a4.z), a4.w);
    }
    if (track_abs && (double)vmax > t.max_abs) return 2;
    if ((double)diff < t.eps) return 1;
    return 0;
  };
  using Even = std::integral_constant<int, 0>;
  using Odd = std::integral_constant<int, VB_OFF>;
  int newest = 0;
  while (it < t.max_sweeps) {
    int rc = sweep(Even{});
    newest = VB_OFF;
    if (rc == 0 && it < t.max_sweeps) {
      rc = sweep(Odd{});
      newest = 0;
    }
    if (rc) { status = (rc == 1) ? 0 : -7; break; }
  }
  if (tid == 0) {
    t.status[b] = status;
    if (t.sweeps) t.sweeps[b] = it;
  }
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * 256;
    if (s < S) {
      t.V[soff + s] = vbase[newest / 4 + s];
      float q[A_T];
      if (newest == VB_OFF) backup_all(Even{}, j, q); else backup_all(Odd{}, j, q);
#pragma unroll
      for (int a = 0; a < A_T; ++a) t.Q[row0 + (int64_t)s * A_T + a] = q[a];
    }
  }
}

// K2W: K2U with ONE WAVEFRONT per instance (lane t owns states t, t + 64, ...: up to 7 per lane, 448 states).  K2U's
// sweep ends in a workgroup barrier among the four wavefronts of an instance (SQ counters: 43 % of the wave cycles parked)
// and repeats its per-sweep overhead (reduction, loop, address set-up) in every wavefront.  With the whole instance in one
// wavefront a sweep needs no barrier at all (LDS executes a wavefront's operations in order: the values lane i wrote in
// sweep k are what lane j reads in sweep k + 1) and the max|dV| reduction is DPP + one readlane.  What hides latency
// instead of the other wavefronts is instruction-level parallelism, and the sweep is written for it:
//   * no `s < S` branch -- a lane's states past the instance's last one have all-zero tables (W, R = +0 -> v = +0, |dV| = 0)
//     and LDS slots of their own, so the whole sweep is ONE basic block;
//   * all reads first (the SPT x U gathers and the SPT old values: ~36 ds_read in flight), then the arithmetic, then the
//     writes -- the compiler cannot know that the two value vectors do not alias, a write between reads would fence them;
//   * the A accumulation chains of a state advance side by side (successor-major), so consecutive float instructions are
//     independent (a dependent one issues ~1.7 x later, which nothing covers at two wavefronts per SIMD).
// The price is registers: SPT (A U + U + A) resident table entries per lane (C3: 6 x 29 = 174 of 253 VGPRs), i.e. two
// wavefronts per SIMD.  Same arithmetic in the same order per row: bit-equal to K2U, K2R, K2 and the oracle.
// C3 (4 096 x FrozenLake 20x20): 2.00 ms against K2U's 2.43 ms; 322 VALU wave-instructions per instance-sweep against 419.
// (Round 4: two actions per v_pk_mul_f32 / v_pk_add_f32 -- bit-equal, 144 fewer instructions per sweep -- changed nothing,
// 2.09 ms: at two wavefronts per SIMD a packed instruction issues every 6.1 cycles, a plain float32 one every 4.2
// (tools/calib/valu_int_rate.hip), and the pairs cost register moves.  The SIMDs issue back to back at that rate.)
template <int MODE, int A_T, int U_T, int KMAX, int SPT>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_dp_regw(DpTables t) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.x;
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int64_t row0 = soff * A_T;
  const int tid = threadIdx.x;
  constexpr int NT = 64;
  constexpr int VB_OFF = SPT * NT * 4;
  constexpr int SENT = 0x7fffffff;

  // LDS pointers (address space 3) of the distinct successors' values in vector A; the other vector is VB_OFF bytes on,
  // which folds into the instruction's offset field
  typedef const __attribute__((address_space(3))) float* lds_cf;
  typedef __attribute__((address_space(3))) float* lds_f;
  const lds_f vbase = (lds_f)(__attribute__((address_space(3))) unsigned char*)smem;
  lds_cf vp[SPT][U_T];
  float W[SPT][A_T][U_T];
  float Rr[SPT][A_T], Pi[SPT][A_T];
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * NT;
    int32_t ucol[U_T];
#pragma unroll
    for (int u = 0; u < U_T; ++u) ucol[u] = SENT;
    int32_t ecol[A_T][KMAX];
    float ecf[A_T][KMAX];
#pragma unroll
    for (int a = 0; a < A_T; ++a) {
      const int64_t r = row0 + (int64_t)s * A_T + a;
      int64_t lo = 0, hi = 0;
      if (s < S) { lo = t.csr_ptr[r]; hi = t.csr_ptr[r + 1]; }
      Rr[j][a] = (s < S) ? t.R[r] : 0.0f;
      Pi[j][a] = (MODE == DP_PE && s < S) ? t.pi[r] : 0.0f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const bool in = lo + k < hi;
        ecol[a][k] = in ? t.csr_col[lo + k] : SENT;
        const float v = in ? t.csr_val[lo + k] : 0.0f;
        ecf[a][k] = (MODE == DP_PE) ? __fmul_rn(t.gamma, v) : v;
        // sorted insertion without duplicates: the larger of (carried, slot) moves on
        int32_t c = ecol[a][k];
#pragma unroll
        for (int u = 0; u < U_T; ++u) {
          const int32_t cur = ucol[u];
          const bool dup = c == cur;
          const bool less = c < cur;
          ucol[u] = less ? c : cur;
          c = dup ? SENT : (less ? cur : c);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U_T; ++u) {
      vp[j][u] = vbase + (ucol[u] == SENT ? 0 : ucol[u]);
#pragma unroll
      for (int a = 0; a < A_T; ++a) {
        float w = 0.0f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) w = (ecol[a][k] == ucol[u] && ucol[u] != SENT) ? ecf[a][k] : w;
        W[j][a][u] = w;
      }
    }
  }
  for (int i = tid; i < 2 * SPT * NT; i += NT) reinterpret_cast<float*>(smem)[i] = 0.0f;
  __builtin_amdgcn_wave_barrier();

  const bool track_abs = t.max_abs > 0.0;
  int64_t it = 0;
  int status = -5;
  auto gather = [&](auto rd_tag, int j, float (&v)[U_T]) {
    constexpr int RD = decltype(rd_tag)::value;
#pragma unroll
    for (int u = 0; u < U_T; ++u) v[u] = vp[j][u][RD / 4];
  };
  auto backup_all = [&](int j, const float (&v)[U_T], float (&q)[A_T]) {
    // the A accumulation chains advance side by side (successor-major): consecutive instructions are independent, which
    // matters at two wavefronts per SIMD (a dependent float32 instruction issues ~1.7 x later than an independent one)
    float acc[A_T];
#pragma unroll
    for (int a = 0; a < A_T; ++a) acc[a] = 0.0f;
#pragma unroll
    for (int u = 0; u < U_T; ++u) {
      float p[A_T];
#pragma unroll
      for (int a = 0; a < A_T; ++a) p[a] = __fmul_rn(W[j][a][u], v[u]);
#pragma unroll
      for (int a = 0; a < A_T; ++a) acc[a] = __fadd_rn(acc[a], p[a]);
    }
#pragma unroll
    for (int a = 0; a < A_T; ++a) acc[a] = (MODE == DP_VI) ? __fmul_rn(t.gamma, acc[a]) : acc[a];
#pragma unroll
    for (int a = 0; a < A_T; ++a) q[a] = __fadd_rn(Rr[j][a], acc[a]);
  };
  auto sweep = [&](auto rd_tag) -> int {
    constexpr int RD = decltype(rd_tag)::value, WR = VB_OFF - RD;
    ++it;
    float dmax = 0.0f, vabs = 0.0f;
    // No `s < S` branch: a lane's states past the instance's last one have all-zero tables (W, R = +0 -> v = +0, |dV| = 0)
    // and their own LDS slots, so the sweep is ONE basic block.  All reads come before the first write (the compiler
    // cannot know that the two value vectors do not alias), so the gathers of all SPT states are in flight together.
    float vnew[SPT], vold[SPT], vg[SPT][U_T];
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      gather(rd_tag, j, vg[j]);
      vold[j] = vbase[RD / 4 + tid + j * NT];
    }
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      float q[A_T];
      backup_all(j, vg[j], q);
      float v = 0.0f;
      if (MODE == DP_VI) {  // values are never NaN: bare max instructions
        if constexpr (A_T == 2) v = fmax_nn(q[0], q[1]);
        else if constexpr (A_T == 3) v = fmax3_nn(q[0], q[1], q[2]);
        else v = fmax_nn(fmax3_nn(q[0], q[1], q[2]), q[A_T - 1]);
      } else {
#pragma unroll
        for (int a = 0; a < A_T; ++a) {
          const float qp = __fmul_rn(q[a], Pi[j][a]);
          v = (a == 0) ? qp : __fadd_rn(v, qp);
        }
      }
      vnew[j] = v;
    }
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      vbase[WR / 4 + tid + j * NT] = vnew[j];
      dmax = fmax_abs_nn(dmax, vold[j] - vnew[j]);
      if (track_abs) vabs = fmax_abs_nn(vabs, vnew[j]);
    }
    // lane 63 holds the wave's maximum; every lane needs it (the loop condition is uniform)
    const float diff = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_max_lane63_nn(dmax)), 63));
    float vmax = 0.0f;
    if (track_abs) vmax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_max_lane63_nn(vabs)), 63));
    __builtin_amdgcn_wave_barrier();   // no instruction: keeps this sweep's LDS writes ahead of the next sweep's reads
    if (track_abs && (double)vmax > t.max_abs) return 2;
    if ((double)diff < t.eps) return 1;
    return 0;
  };
  using Even = std::integral_constant<int, 0>;
  using Odd = std::integral_constant<int, VB_OFF>;
  int newest = 0;
  while (it < t.max_sweeps) {
    int rc = sweep(Even{});
    newest = VB_OFF;
    if (rc == 0 && it < t.max_sweeps) {
      rc = sweep(Odd{});
      newest = 0;
    }
    if (rc) { status = (rc == 1) ? 0 : -7; break; }
  }
  if (tid == 0) {
    t.status[b] = status;
    if (t.sweeps) t.sweeps[b] = it;
  }
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * NT;
    if (s < S) {
      t.V[soff + s] = vbase[newest / 4 + s];
      float q[A_T], v[U_T];
      if (newest == VB_OFF) gather(Even{}, j, v); else gather(Odd{}, j, v);
      backup_all(j, v, q);
#pragma unroll
      for (int a = 0; a < A_T; ++a) t.Q[row0 + (int64_t)s * A_T + a] = q[a];
    }
  }
}

// K3: Gauss-Seidel sweeps (numba paths of the reference), one wavefront per unit, V in LDS, states in
// order.  Lane a < A backs up action a of the current state; later states see the updated V.
template <int MODE, bool DIAM>
__global__ void __launch_bounds__(64) k_dp_wave_gs(DpTables t) {
  extern __shared__ __align__(16) unsigned char smem[];
  int b, target;
  unit_to_instance(t, blockIdx.x, b, target);
  const int A = t.A;
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int64_t row0 = soff * A;
  const int lane = threadIdx.x;
  float* V = reinterpret_cast<float*>(smem);
  for (int i = lane; i < S; i += 64) V[i] = 0.0f;
  __syncthreads();
  const int64_t* ptr = t.csr_ptr + row0;
  const int32_t* col = t.csr_col;
  const float* val = t.csr_val;
  const bool active = lane < A;
  int64_t it = 0;
  int status = -5;
  while (it < t.max_sweeps) {
    ++it;
    float dmax = 0.0f;
    bool too_big = false;
    for (int s = 0; s < S; ++s) {
      float q = -3.0e38f, qp = 0.0f;
      if (active) {
        const int r = s * A + lane;
        float acc = 0.0f, rew;
        if (DIAM && s == target) {
          acc = __fadd_rn(acc, __fmul_rn(__fmul_rn(t.gamma, 1.0f), V[target]));
          rew = 0.0f;
        } else {
          const int64_t lo = ptr[r], hi = ptr[r + 1];
          for (int64_t k = lo; k < hi; ++k) acc = __fadd_rn(acc, __fmul_rn(__fmul_rn(t.gamma, val[k]), V[col[k]]));
          rew = DIAM ? -1.0f : t.R[row0 + r];
        }
        q = __fadd_rn(rew, acc);
        if (!DIAM) t.Q[row0 + r] = q;
        if (MODE == DP_PE) qp = __fmul_rn(q, t.pi[row0 + r]);
      }
      float v;
      if (MODE == DP_VI) {
        v = wave_max(q);
      } else {
        v = __shfl(qp, 0, 64);
        for (int a = 1; a < A; ++a) v = __fadd_rn(v, __shfl(qp, a, 64));
      }
      __syncthreads();  // every lane has read V for this state before it changes
      if (lane == 0) {
        const float old = V[s];
        V[s] = v;
        dmax = fmaxf(dmax, fabsf(old - v));
        if (t.max_abs > 0.0 && fabs((double)v) > t.max_abs) too_big = true;
      }
      __syncthreads();
    }
    const float diff = __shfl(dmax, 0, 64);
    if (__shfl((int)too_big, 0, 64)) { status = -7; break; }
    if ((double)diff < t.eps) { status = 0; break; }
  }
  const int64_t unit = blockIdx.x;
  if (lane == 0) {
    t.status[unit] = status;
    if (t.sweeps) t.sweeps[unit] = it;
  }
  if (DIAM) {
    float mn = 3.0e38f;
    for (int i = lane; i < S; i += 64) mn = fminf(mn, V[i]);
    mn = wave_min(mn);
    if (lane == 0) t.per_target[soff + target] = -mn;
  } else {
    for (int i = lane; i < S; i += 64) t.V[soff + i] = V[i];
  }
}

// K4: finite-horizon backward induction (reference colosseum/dynamic_programming/finite_horizon.py:11-42),
// one workgroup per instance; V[h+1] is staged in LDS, Q[h]/V[h] go straight to HBM.
template <int MODE>
__global__ void __launch_bounds__(256) k_episodic(DpTables t, int H, float* __restrict__ Qout, float* __restrict__ Vout) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.x;
  const int A = t.A;
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int64_t row0 = soff * A;
  const int64_t nz0 = t.csr_ptr[row0];
  const int tid = threadIdx.x, nth = blockDim.x;
  float* Va = reinterpret_cast<float*>(smem);
  float* Vb = Va + S;
  float* Q = Qout + (int64_t)(H + 1) * row0;
  float* V = Vout + (int64_t)(H + 1) * soff;
  for (int i = tid; i < S; i += nth) { Va[i] = 0.0f; V[(int64_t)H * S + i] = 0.0f; }
  for (int i = tid; i < S * A; i += nth) Q[(int64_t)H * S * A + i] = 0.0f;
  __syncthreads();
  GPtr gp{t.csr_ptr + row0, nz0};
  float* Vnext = Va;
  float* Vcur = Vb;
  for (int h = H - 1; h >= 0; --h) {
    const float* pi = (MODE == DP_PE) ? t.pi + (int64_t)H * row0 + (int64_t)h * S * A : nullptr;
    float* Qh = Q + (int64_t)h * S * A;
    for (int s = tid; s < S; s += nth) {
      // gamma == 1: `Q[h, s] = R[s] + T[s] @ V[h + 1]`; products 1*val are exact
      const float v = backup_state<MODE, true, false, true>(s, A, -1, gp, t.csr_col + nz0, t.csr_val + nz0, t.R + row0,
                                                            pi, Vnext, 1.0f, Qh);
      Vcur[s] = v;
      V[(int64_t)h * S + s] = v;
    }
    __syncthreads();
    float* tmp = Vnext; Vnext = Vcur; Vcur = tmp;
  }
}

// K5E: episodic diameter on the time-augmented state space (reference colosseum/hardness/measures/diameter.py:
// 285-318 over the T_epi of colosseum/mdp/utils/mdp_creation.py:98-128).  One workgroup per (instance, target);
// ETs[H][S] lives in LDS and is updated in place layer by layer (h = H-1 .. 1, one barrier per layer) exactly in
// the reference's order; every target runs to diff < eps (the reference's second, running-maximum stopping rule
// depends on the order in which targets are visited and is not reproduced -- SURVEY 8e).
struct EpiDiamArgs {
  int32_t H;
  const int64_t* start_off;   // [B+1]
  const int32_t* start_state; // [NS]
  const float* start_prob;    // [NS] float32, as stored in T_epi[H-1]
  const uint8_t* reach;       // per instance [H][S_b] at offset H*state_off[b]: row (h, s) of T_epi is filled
};

__global__ void __launch_bounds__(256) k_diam_episodic(DpTables t, EpiDiamArgs e) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ float red[2][4];
  __shared__ float last_val;
  int b, es;
  unit_to_instance(t, blockIdx.x, b, es);
  const int A = t.A, H = e.H;
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int64_t row0 = soff * A;
  const int64_t* ptr = t.csr_ptr + row0;
  const uint8_t* reach = e.reach + (int64_t)H * soff;
  const int64_t s0 = e.start_off[b];
  const int n_start = (int)(e.start_off[b + 1] - s0);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* ETs = reinterpret_cast<float*>(smem);  // [H][S]
  for (int i = tid; i < H * S; i += 256) ETs[i] = 0.0f;
  __syncthreads();
  int64_t it = 0;
  int status = -5;
  while (it < t.max_sweeps) {
    ++it;
    float dmax = 0.0f;
    if (tid == 0) {  // ETs[-1] = T[-1, 0, 0] @ (1 + ETs[0]): the start distribution row
      float last = 0.0f;
      for (int i = 0; i < n_start; ++i)
        last = __fadd_rn(last, __fmul_rn(e.start_prob[s0 + i], __fadd_rn(1.0f, ETs[e.start_state[s0 + i]])));
      last_val = last;
    }
    __syncthreads();
    {
      const float last = last_val;
      float* El = ETs + (size_t)(H - 1) * S;
      for (int s = tid; s < S; s += 256) {
        dmax = fmaxf(dmax, fabsf(El[s] - last));
        El[s] = last;
      }
    }
    __syncthreads();
    for (int h = H - 1; h >= 1; --h) {
      const float* En = ETs + (size_t)h * S;
      float* Ec = ETs + (size_t)(h - 1) * S;
      for (int j = tid; j < S; j += 256) {
        if (j == es) continue;
        float best = 0.0f;
        if (reach[(size_t)(h - 1) * S + j]) {
          for (int a = 0; a < A; ++a) {
            const int r = j * A + a;
            float acc = 0.0f, p_es = 0.0f;
            for (int64_t k = ptr[r]; k < ptr[r + 1]; ++k) {
              const int c = t.csr_col[k];
              const float v = t.csr_val[k];
              if (c == es) { p_es = v; continue; }
              acc = __fadd_rn(acc, __fmul_rn(v, __fadd_rn(1.0f, En[c])));
            }
            const float cand = __fadd_rn(p_es, acc);
            best = (a == 0) ? cand : fminf(best, cand);
          }
        }
        dmax = fmaxf(dmax, fabsf(Ec[j] - best));
        Ec[j] = best;
      }
      __syncthreads();
    }
    dmax = wave_max(dmax);
    if (lane == 0) red[it & 1][wave] = dmax;
    __syncthreads();
    const float diff = fmaxf(fmaxf(red[it & 1][0], red[it & 1][1]), fmaxf(red[it & 1][2], red[it & 1][3]));
    if ((double)diff < t.eps) { status = 0; break; }
  }
  // cur_diam = max_s min_{h : ETs[h][s] > 0} ETs[h][s]
  float cur = 0.0f;
  for (int s = tid; s < S; s += 256) {
    float mn = 3.0e38f;
    for (int h = 0; h < H; ++h) {
      const float v = ETs[(size_t)h * S + s];
      if (v > 0.0f && v < mn) mn = v;
    }
    cur = fmaxf(cur, mn);
  }
  cur = wave_max(cur);
  __syncthreads();
  if (lane == 0) red[0][wave] = cur;
  __syncthreads();
  if (tid == 0) {
    t.per_target[soff + es] = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    t.status[blockIdx.x] = status;
  }
}

// K6: calculate_norm_discounted (reference colosseum/hardness/measures/value_norm.py:83-87):
//   Ev[j,a] = sum_k T[j,a,k] V[k];  out = max_{i,a} sqrt( sum_j T[i,a,j] (V[j] - Ev[j,a])^2 )
__global__ void __launch_bounds__(256) k_value_norm(DpTables t, const float* __restrict__ V, float* __restrict__ Ev,
                                                    float* __restrict__ out) {
  __shared__ float red[4];
  const int b = blockIdx.x;
  const int A = t.A;
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int rows = S * A;
  const int64_t row0 = soff * A;
  const int tid = threadIdx.x, nth = blockDim.x;
  const float* Vb = V + soff;
  for (int r = tid; r < rows; r += nth) {
    float acc = 0.0f;
    for (int64_t k = t.csr_ptr[row0 + r]; k < t.csr_ptr[row0 + r + 1]; ++k)
      acc = __fadd_rn(acc, __fmul_rn(t.csr_val[k], Vb[t.csr_col[k]]));
    Ev[row0 + r] = acc;
  }
  __syncthreads();  // Ev of this instance was written by this workgroup only
  float best = 0.0f;
  for (int r = tid; r < rows; r += nth) {
    const int a = r % A;
    float acc = 0.0f;
    for (int64_t k = t.csr_ptr[row0 + r]; k < t.csr_ptr[row0 + r + 1]; ++k) {
      const int j = t.csr_col[k];
      const float d = __fsub_rn(Vb[j], Ev[row0 + (int64_t)j * A + a]);
      acc = __fadd_rn(acc, __fmul_rn(t.csr_val[k], __fmul_rn(d, d)));
    }
    best = fmaxf(best, __fsqrt_rn(acc));
  }
  best = wave_max(best);
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    float m = red[0];
    for (int w = 1; w < (nth >> 6); ++w) m = fmaxf(m, red[w]);
    out[b] = m;
  }
}


// ===================================================================================================
// K7: stationary distribution by GTH elimination (reference colosseum/mdp/utils/markov_chain.py:139-166,
// `_gth_solve_numba`), float64, one workgroup per chain (the matrix is a work copy in HBM/L2, n <= a few hundred
// in the benchmark).  Step i: scale = sum_k a[i,k>i] (one lane, index order, as the reference); column i below the
// diagonal is divided by it; the trailing block gets the rank-1 update a[j,k] += a[j,i]*a[i,k] (all threads,
// multiply and add rounded separately).  Back-substitution and the normalisation are index-order sums as well.
// ===================================================================================================
__global__ void __launch_bounds__(256) k_gth(const int64_t* __restrict__ mat_off, const int32_t* __restrict__ dims,
                                             const int64_t* __restrict__ x_off, double* __restrict__ mats,
                                             double* __restrict__ xs) {
  __shared__ double s_scale;
  __shared__ int s_n;
  const int m = blockIdx.x, tid = threadIdx.x;
  const int n = dims[m];
  double* a = mats + mat_off[m];
  double* x = xs + x_off[m];
  if (tid == 0) s_n = n;
  __syncthreads();
  for (int i = 0; i < s_n - 1; ++i) {
    const int nn = s_n;
    if (tid == 0) {
      double sc = 0.0;
      for (int k = i + 1; k < nn; ++k) sc = __dadd_rn(sc, a[(size_t)i * n + k]);
      s_scale = sc;
      if (sc <= 0.0) s_n = i + 1;
    }
    __syncthreads();
    if (s_n != nn) break;
    const double sc = s_scale;
    for (int j = i + 1 + tid; j < nn; j += 256) a[(size_t)j * n + i] = a[(size_t)j * n + i] / sc;
    __syncthreads();
    const int w = nn - i - 1;
    for (int e = tid; e < w * w; e += 256) {
      const int j = i + 1 + e / w, k = i + 1 + e % w;
      a[(size_t)j * n + k] = __dadd_rn(a[(size_t)j * n + k], __dmul_rn(a[(size_t)j * n + i], a[(size_t)i * n + k]));
    }
    __syncthreads();
  }
  __syncthreads();
  const int nn = s_n;
  for (int i = tid; i < n; i += 256) x[i] = 0.0;
  __syncthreads();
  if (tid == 0) {
    x[nn - 1] = 1.0;
    if (nn >= 2) x[nn - 2] = a[(size_t)(nn - 1) * n + (nn - 2)];
    for (int i = nn - 3; i >= 0; --i) {
      double acc = 0.0;
      for (int j = i + 1; j < nn; ++j) acc = __dadd_rn(acc, __dmul_rn(x[j], a[(size_t)j * n + i]));
      x[i] = acc;
    }
    double tot = 0.0;
    for (int i = 0; i < nn; ++i) tot = __dadd_rn(tot, x[i]);
    for (int i = 0; i < nn; ++i) x[i] = x[i] / tot;
  }
}


// ===================================================================================================
// K5S: diameter of LARGE instances (config C5: S ~ 50 000, the value vector of one target no longer fits LDS).
// Same arithmetic as K2 in DIAM mode -- per target es the Jacobi value iteration of
// `_continuous_diam_calculation` (reference colosseum/hardness/measures/diameter.py:76-96) on T_es / R_es with
// gamma = 1, float32 in-order accumulation, stop at max|dV| < eps -- but organised for HBM:
//   * one workgroup solves 64 consecutive targets AT ONCE, lane = target.  All 64 value vectors live interleaved
//     in HBM as V[state][lane] (two copies, Jacobi), so the gather V[col] of every non-zero is one fully
//     coalesced 256-byte row for the whole wave, whatever the column is;
//   * the CSR walk is the same for all 64 targets: row pointers, columns and values are wave-uniform (scalar
//     loads through the constant cache), read once per 64 targets instead of once per target;
//   * the NW waves of the workgroup split the states; max|dV| and min V are lane-private running values, reduced
//     across the waves through LDS once per sweep (one barrier per sweep);
//   * a target that has converged keeps its result (-min V of ITS final sweep) while the others continue.
// Algorithmic HBM bytes per (target, sweep): 4 B read + 4 B written per state (the CSR is shared by 64 targets).
// ===================================================================================================
struct DiamLanesArgs {
  const int32_t* grp_inst;     // [groups] instance of the group
  const int32_t* grp_target0;  // [groups] first target (instance-relative)
  const int32_t* grp_count;    // [groups] targets in the group (<= 64)
  const int64_t* grp_voff;     // [groups] offset of the group's two value arrays in `vbuf` (floats)
  float* vbuf;
};

template <int NW>
__global__ void __launch_bounds__(NW * 64) k_diam_lanes(DpTables t, DiamLanesArgs g) {
  __shared__ float red_d[2][NW][64];
  __shared__ float red_m[2][NW][64];
  const int grp = blockIdx.x;
  const int b = g.grp_inst[grp];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int A = t.A;
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int64_t row0 = soff * A;
  const int64_t* ptr = t.csr_ptr + row0;
  const int target = g.grp_target0[grp] + lane;
  const bool active = lane < g.grp_count[grp];
  float* Vold = g.vbuf + g.grp_voff[grp];
  float* Vnew = Vold + (int64_t)S * 64;
  for (int64_t i = threadIdx.x; i < (int64_t)S * 128; i += NW * 64) Vold[i] = 0.0f;
  __syncthreads();

  bool done = !active;
  float result = 0.0f;
  int status = active ? -5 : 0;
  int64_t it = 0;
  while (it < t.max_sweeps) {
    ++it;
    float dmax = 0.0f, vmin = 3.0e38f;
    for (int s = wave; s < S; s += NW) {
      float v = 0.0f;
      for (int a = 0; a < A; ++a) {
        const int64_t lo = ptr[(int64_t)s * A + a], hi = ptr[(int64_t)s * A + a + 1];
        float acc = 0.0f;
        for (int64_t k = lo; k < hi; ++k)
          acc = __fadd_rn(acc, __fmul_rn(t.csr_val[k], Vold[(int64_t)t.csr_col[k] * 64 + lane]));
        const float q = __fadd_rn(-1.0f, __fmul_rn(t.gamma, acc));
        v = (a == 0) ? q : fmaxf(v, q);
      }
      const float vo = Vold[(int64_t)s * 64 + lane];
      if (s == target) {  // absorbing row {target: 1}, R = 0: every action gives 0 + gamma * (0 + 1 * V[target])
        v = __fadd_rn(0.0f, __fmul_rn(t.gamma, __fadd_rn(0.0f, __fmul_rn(1.0f, vo))));
      }
      Vnew[(int64_t)s * 64 + lane] = v;
      dmax = fmaxf(dmax, fabsf(vo - v));
      vmin = fminf(vmin, v);
    }
    const int par = (int)(it & 1);
    red_d[par][wave][lane] = dmax;
    red_m[par][wave][lane] = vmin;
    __syncthreads();
    float diff = 0.0f, mn = 3.0e38f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      diff = fmaxf(diff, red_d[par][w][lane]);
      mn = fminf(mn, red_m[par][w][lane]);
    }
    float* tmp = Vold; Vold = Vnew; Vnew = tmp;
    if (!done && (double)diff < t.eps) {
      done = true;
      result = -mn;
      status = 0;
    }
    if (__all(done)) break;
  }
  if (wave == 0 && active) {
    t.per_target[soff + target] = result;
    t.status[soff + target] = status;
  }
}


// K5S, fixed-width rows.  The CSR rows are padded to K entries (column = the row's first column, coefficient +0.0:
// acc + 0*V == acc exactly, as in K2R) and stored state-major, so the A*K entries of U = 64/(A*K) consecutive states
// are ONE coalesced 64-lane load; every entry reaches the whole wave as a scalar through v_readlane.  A wave keeps
// U states in flight: all U*A*K gathers (one 256-byte row each) are issued
// before any of them is consumed, and the next chunk's entries are fetched meanwhile -- one memory round trip per U
// states instead of three dependent ones per state.
__global__ void __launch_bounds__(256) k_build_ell(int64_t n_rows, int K, const int64_t* __restrict__ ptr,
                                                   const int32_t* __restrict__ col, const float* __restrict__ val,
                                                   int32_t* __restrict__ ecol, float* __restrict__ eval_) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows + 64 / K + 1) return;  // tail padding so that a 64-entry load past the last state stays inside
  if (r >= n_rows) {
    for (int k = 0; k < K; ++k) { ecol[r * K + k] = 0; eval_[r * K + k] = 0.0f; }
    return;
  }
  const int64_t lo = ptr[r], hi = ptr[r + 1];
  const int32_t c0 = hi > lo ? col[lo] : 0;
  for (int k = 0; k < K; ++k) {
    const bool in = lo + k < hi;
    ecol[r * K + k] = in ? col[lo + k] : c0;
    eval_[r * K + k] = in ? val[lo + k] : 0.0f;
  }
}

// `new_of` (or null): the rows were stored in a locality order of the states (relabel_states in cmdp.hip) -- row n is the
// row of the original state that was relabelled n, its entries in their ORIGINAL (ascending original column) order with
// the column replaced by the successor's new label.  Every sum therefore adds the same terms in the same order and the
// result is bit-equal to the unrelabelled kernel; only the target's label has to be translated.
template <int NW, int A, int K>
__global__ void __launch_bounds__(NW * 64) k_diam_lanes_ell(DpTables t, DiamLanesArgs g, const int32_t* __restrict__ ecol,
                                                           const float* __restrict__ eval_, const int32_t* __restrict__ new_of) {
  constexpr int AK = A * K, U = 64 / AK;
  static_assert(U >= 1, "A*K must not exceed 64");
  __shared__ float red_d[2][NW][64];
  __shared__ float red_m[2][NW][64];
  const int grp = blockIdx.x;
  const int b = g.grp_inst[grp];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int32_t* ec = ecol + soff * AK;
  const float* ev = eval_ + soff * AK;
  const int target = g.grp_target0[grp] + lane;
  const bool active = lane < g.grp_count[grp];
  const int target_row = (new_of && active) ? new_of[soff + target] : target;  // where the target's row and value live
  float* Vold = g.vbuf + g.grp_voff[grp];
  float* Vnew = Vold + (int64_t)S * 64;
  for (int64_t i = threadIdx.x; i < (int64_t)S * 128; i += NW * 64) Vold[i] = 0.0f;
  __syncthreads();
  // chunks of U states are dealt round-robin to the waves: the NW waves of the workgroup walk NW adjacent chunks at
  // the same time, so the value rows neighbouring states share are fetched once and hit in L1/L2 for the others
  const int s_begin = wave * U;
  const int s_end = S;
  constexpr int STRIDE = NW * U;

  bool done = !active;
  float result = 0.0f;
  int status = active ? -5 : 0;
  int64_t it = 0;
  while (it < t.max_sweeps) {
    ++it;
    float dmax = 0.0f, vmin = 3.0e38f;
    if (s_begin < s_end) {
      // entries past the instance's last state belong to the next instance (or the tail padding): column 0 keeps
      // their (discarded) gathers inside this group's value array
      const int sl = lane / AK;
      int ccol = (s_begin + sl < S) ? ec[(int64_t)s_begin * AK + lane] : 0;
      float cval = ev[(int64_t)s_begin * AK + lane];
      for (int s0 = s_begin; s0 < s_end; s0 += STRIDE) {
        const int sn = (s0 + STRIDE < s_end) ? s0 + STRIDE : s0;  // next chunk (re-reads the current one at the very end)
        const int ncol = (sn + sl < S) ? ec[(int64_t)sn * AK + lane] : 0;
        const float nval = ev[(int64_t)sn * AK + lane];
        float x[U * AK], vo[U];
#pragma unroll
        for (int e = 0; e < U * AK; ++e) {
          const int c = __builtin_amdgcn_readlane(ccol, e);
          x[e] = Vold[(int64_t)c * 64 + lane];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int s = (s0 + u < s_end) ? s0 + u : s0;
          vo[u] = Vold[(int64_t)s * 64 + lane];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int s = s0 + u;
          if (s < s_end) {
            float v = 0.0f;
#pragma unroll
            for (int a = 0; a < A; ++a) {
              float acc = 0.0f;
#pragma unroll
              for (int k = 0; k < K; ++k) {
                const int e = (u * A + a) * K + k;
                const float coef = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cval), e));
                acc = __fadd_rn(acc, __fmul_rn(coef, x[e]));
              }
              const float q = __fadd_rn(-1.0f, __fmul_rn(t.gamma, acc));
              v = (a == 0) ? q : fmaxf(v, q);
            }
            if (s == target_row) v = __fadd_rn(0.0f, __fmul_rn(t.gamma, __fadd_rn(0.0f, __fmul_rn(1.0f, vo[u]))));
            Vnew[(int64_t)s * 64 + lane] = v;
            dmax = fmaxf(dmax, fabsf(vo[u] - v));
            vmin = fminf(vmin, v);
          }
        }
        ccol = ncol;
        cval = nval;
      }
    }
    const int par = (int)(it & 1);
    red_d[par][wave][lane] = dmax;
    red_m[par][wave][lane] = vmin;
    __syncthreads();
    float diff = 0.0f, mn = 3.0e38f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      diff = fmaxf(diff, red_d[par][w][lane]);
      mn = fminf(mn, red_m[par][w][lane]);
    }
    float* tmp = Vold; Vold = Vnew; Vnew = tmp;
    if (!done && (double)diff < t.eps) {
      done = true;
      result = -mn;
      status = 0;
    }
    if (__all(done)) break;
  }
  if (wave == 0 && active) {
    t.per_target[soff + target] = result;
    t.status[soff + target] = status;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// K5C (round 3): K5S with a CLUSTER of CL workgroups per group of 64 targets.  K5S keeps one group per CU: thirty-two groups
// per XCD stream 13 MB of value rows each (S = 50 272) through a 4 MB L2, and the rows are re-read 2.3 times.  Here the CL
// workgroups of a cluster sit on the same XCD (workgroups are dealt to the XCDs round-robin, so the members are blockIdx
// = xcd + 8 * (CL * c + m)), share one pair of value arrays and split every sweep between them: 32 / CL streams per L2
// instead of 32, each with CL times the window.  Per sweep the members meet at ONE barrier (a monotone counter per cluster
// in HBM, release / acquire at agent scope; every member then reduces the same CL partial (max |dV|, min V) rows in the
// same order, so all of them take the same decisions and execute the same number of barriers).  The launch is persistent:
// n_clusters * CL workgroups, cluster q solves groups q, q + n_clusters, ...  Arithmetic per target = K5S's, term for term.
// The barrier spins with a wall-clock limit: if the members of a cluster are not all resident (CUs held by another
// kernel), every workgroup leaves through the same exit with `*err` set and the host repeats the launch on K5S.
// ---------------------------------------------------------------------------------------------------------------
// tuning switch of the K5C kernels: the new value rows written with nontemporal stores (they are not read again before the
// next sweep, by which time they have left the L2 anyway)
#ifndef CMDP_K5C_NT_STORE
#define CMDP_K5C_NT_STORE 1
#endif
constexpr bool NT_STORE = CMDP_K5C_NT_STORE != 0;

struct DiamClusterArgs {
  int n_groups, n_clusters;
  int64_t vstride;            // floats per cluster (two value arrays of the largest instance)
  float* cred;                // [n_clusters][2][CL][2][64] partial reductions
  unsigned int* cbar;         // [n_clusters] barrier counters (zero at launch)
  int* err;                   // 1: a barrier timed out; 2: a cluster's workgroups are not on one XCD
  int* xcc;                   // [n_clusters][CL] XCC id of every member (XCD-scope barriers only)
  long long timeout_ticks;    // wall_clock64 ticks (100 MHz)
};

// XCD = true: the members have verified (HW_REG_XCC_ID) that they share an XCD, i.e. one L2.  Stores are complete when
// the L2 has acknowledged them (the vector L1 is write-through), so the release is a wait for the outstanding stores and the
// acquire only drops the wave's L1 lines (`buffer_inv sc0`); the agent-scope pair would write the whole L2 back and
// invalidate it once per sweep.
template <int CL, bool XCD>
__device__ __forceinline__ bool cluster_barrier(unsigned int* bar, unsigned int& epoch, int* err, long long timeout_ticks) {
  // all stores of this workgroup (value rows, partials) before the arrival; the workgroup's arrival is one atomic
  if (XCD) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  ++epoch;
  __shared__ int ok_s;
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned int want = epoch * (unsigned int)CL;
    const long long t0 = (long long)wall_clock64();
    int ok = 1;
    while ((int)(__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want) < 0) {
      __builtin_amdgcn_s_sleep(1);
      if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { ok = 0; break; }
      if ((long long)wall_clock64() - t0 > timeout_ticks) {
        __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0;
        break;
      }
    }
    ok_s = ok;
  }
  __syncthreads();
  if (XCD) asm volatile("buffer_inv sc0" ::: "memory");
  else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return ok_s != 0;
}

template <int CL, int A, int K, bool XCD>
__global__ void __launch_bounds__(1024) k_diam_cluster(DpTables t, DiamLanesArgs g, DiamClusterArgs ca, const int32_t* __restrict__ ecol,
                                                      const float* __restrict__ eval_, const int32_t* __restrict__ new_of) {
  // U states in flight per wavefront: the 64 / AK whose entries one 64-lane load fetches -- at most eight (A = K = 2 would
  // hold sixteen states x four gathered rows in registers: 12 bytes of scratch under the 128-register cap of a 1024-thread
  // workgroup)
  constexpr int NW = 16, AK = A * K, U = (64 / AK > 10) ? 8 : 64 / AK, XCDS = 8;
  static_assert(U >= 1, "A*K must not exceed 64");
  __shared__ float red_d[NW][64];
  __shared__ float red_m[NW][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int xcd = blockIdx.x % XCDS, idx = blockIdx.x / XCDS;
  const int member = idx % CL;
  const int cluster = xcd + XCDS * (idx / CL);
  if (cluster >= ca.n_clusters) return;
  unsigned int* bar = ca.cbar + cluster;
  float* cred = ca.cred + (int64_t)cluster * 2 * CL * 2 * 64;
  float* vbase = g.vbuf + (int64_t)cluster * ca.vstride;
  unsigned int epoch = 0;
  unsigned int sweep_no = 0;   // parity of the partial rows: continues across the cluster's groups
  if (XCD) {
    // the cheap barrier is only right if the members really share an L2: every member publishes its XCC id, all compare
    // after one agent-scope barrier, and a cluster that is spread over XCDs reports it (the host repeats the launch with
    // agent-scope barriers)
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xfu;   // HW_REG_XCC_ID[3:0]
    if (threadIdx.x == 0) __hip_atomic_store(ca.xcc + (int64_t)cluster * CL + member, (int)xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!cluster_barrier<CL, false>(bar, epoch, ca.err, ca.timeout_ticks)) return;
    bool same = true;
    for (int m = 0; m < CL; ++m)
      same = same && __hip_atomic_load(ca.xcc + (int64_t)cluster * CL + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)xcc;
    if (!same) {
      if (threadIdx.x == 0) __hip_atomic_store(ca.err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  }
  constexpr int CW = CL * NW;  // wavefronts of the cluster
  const int cw = member * NW + wave;

  for (int grp = cluster; grp < ca.n_groups; grp += ca.n_clusters) {
    const int b = g.grp_inst[grp];
    const int64_t soff = t.state_off[b];
    const int S = (int)(t.state_off[b + 1] - soff);
    const int32_t* ec = ecol + soff * AK;
    const float* ev = eval_ + soff * AK;
    const int target = g.grp_target0[grp] + lane;
    const bool active = lane < g.grp_count[grp];
    const int target_row = (new_of && active) ? new_of[soff + target] : target;
    float* Vold = vbase;
    float* Vnew = vbase + (int64_t)S * 64;
    // zero both arrays, the members' slices interleaved
    for (int64_t i = (int64_t)member * 1024 + threadIdx.x; i < (int64_t)S * 128; i += (int64_t)CL * 1024) Vold[i] = 0.0f;
    if (!cluster_barrier<CL, XCD>(bar, epoch, ca.err, ca.timeout_ticks)) return;

    const int s_begin = cw * U;
    constexpr int STRIDE = CW * U;
    bool done = !active;
    float result = 0.0f;
    int status = active ? -5 : 0;
    int64_t it = 0;
    while (it < t.max_sweeps) {
      ++it;
      float dmax = 0.0f, vmin = 3.0e38f;
      if (s_begin < S) {
        const int sl = lane / AK;
        int ccol = (s_begin + sl < S) ? ec[(int64_t)s_begin * AK + lane] : 0;
        float cval = ev[(int64_t)s_begin * AK + lane];
        for (int s0 = s_begin; s0 < S; s0 += STRIDE) {
          const int sn = (s0 + STRIDE < S) ? s0 + STRIDE : s0;
          const int ncol = (sn + sl < S) ? ec[(int64_t)sn * AK + lane] : 0;
          const float nval = ev[(int64_t)sn * AK + lane];
          float x[U * AK], vo[U];
#pragma unroll
          for (int e = 0; e < U * AK; ++e) {
            const int c = __builtin_amdgcn_readlane(ccol, e);
            x[e] = Vold[(int64_t)c * 64 + lane];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int s = (s0 + u < S) ? s0 + u : s0;
            vo[u] = Vold[(int64_t)s * 64 + lane];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int s = s0 + u;
            if (s < S) {
              float v = 0.0f;
#pragma unroll
              for (int a = 0; a < A; ++a) {
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                  const int e = (u * A + a) * K + k;
                  const float coef = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cval), e));
                  acc = __fadd_rn(acc, __fmul_rn(coef, x[e]));
                }
                const float q = __fadd_rn(-1.0f, __fmul_rn(t.gamma, acc));
                v = (a == 0) ? q : fmaxf(v, q);
              }
              if (s == target_row) v = __fadd_rn(0.0f, __fmul_rn(t.gamma, __fadd_rn(0.0f, __fmul_rn(1.0f, vo[u]))));
              if (NT_STORE) __builtin_nontemporal_store(v, Vnew + (int64_t)s * 64 + lane); else Vnew[(int64_t)s * 64 + lane] = v;
              dmax = fmaxf(dmax, fabsf(vo[u] - v));
              vmin = fminf(vmin, v);
            }
          }
          ccol = ncol;
          cval = nval;
        }
      }
      // the workgroup's partial row, then the cluster's
      red_d[wave][lane] = dmax;
      red_m[wave][lane] = vmin;
      __syncthreads();
      const int par = (int)(sweep_no & 1u);
      ++sweep_no;
      if (wave == 0) {
        float d = 0.0f, m = 3.0e38f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          d = fmaxf(d, red_d[w][lane]);
          m = fminf(m, red_m[w][lane]);
        }
        float* row = cred + ((int64_t)(par * CL + member) * 2) * 64;
        row[lane] = d;
        row[64 + lane] = m;
      }
      if (!cluster_barrier<CL, XCD>(bar, epoch, ca.err, ca.timeout_ticks)) return;
      float diff = 0.0f, mn = 3.0e38f;
#pragma unroll
      for (int m = 0; m < CL; ++m) {
        const float* row = cred + ((int64_t)(par * CL + m) * 2) * 64;
        diff = fmaxf(diff, __builtin_nontemporal_load(row + lane));
        mn = fminf(mn, __builtin_nontemporal_load(row + 64 + lane));
      }
      float* tmp = Vold; Vold = Vnew; Vnew = tmp;
      if (!done && (double)diff < t.eps) {
        done = true;
        result = -mn;
        status = 0;
      }
      if (__all(done)) break;
    }
    if (member == 0 && wave == 0 && active) {
      t.per_target[soff + target] = result;
      t.status[soff + target] = status;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Calibration of the rollout kernels' latency floor (cmdp_calibrate; no reference counterpart): one wavefront per
// workgroup, every lane follows its own uint16 successor table in LDS for `steps` DEPENDENT reads.
//   CHAIN = 0: ds_read_u16 -> mask -> address, nothing else (the bare dependent LDS read);
//   CHAIN = 1: what a deterministic-dynamics transition cannot avoid on its dependency chain -- action bit into the
//              address, the successor read, the field mask, the in-episode step count and the episode-end select
//              (K1P's chain stage does exactly this plus the trace store, which is off the chain).
//   CHAIN = 2: the same for K1T, whose transition reads the state's word pair AND its swap bit (two independent reads)
//              and selects the word by a bit-field extract.
template <int CHAIN>
__global__ void __launch_bounds__(64) k_calib_lds_chain(int steps, int H, int32_t* __restrict__ sink) {
  extern __shared__ unsigned short calib_tab[];
  constexpr int kPer = 512;  // entries per lane: 64 lanes x 512 x 2 B = 64 KiB
  unsigned x = 12345u + blockIdx.x * 977u + threadIdx.x;
  for (int i = 0; i < kPer; ++i) {
    x = x * 1664525u + 1013904223u;
    calib_tab[threadIdx.x * kPer + i] = (unsigned short)(((x >> 8) % (kPer / 2)) * 2);
  }
  __syncthreads();
  const int base = threadIdx.x * kPer;
  int cur = 0, h = 0;
  for (int s = 0; s < steps; ++s) {
    if (CHAIN == 0) {
      cur = calib_tab[base + cur] & (kPer - 1);
    } else if (CHAIN == 1) {
      const int a = (s * 7 + threadIdx.x) & 1;
      const int nxt = calib_tab[base + cur + a] & (kPer - 2);
      ++h;
      const bool term = h >= H;
      cur = term ? 0 : nxt;
      h = term ? 0 : h;
    } else {
      // K1T's chain: the state's two words (one 32-bit read) and the byte with its swap bit (a second, independent read
      // from the far end of the lane's table), word[a ^ bit] selected by a bit-field extract, the episode-end select.
      // `cur` is the state's byte offset in the word table (4 s, s < 128: the last 32 entries of the lane's table serve as
      // the 16 mask bytes)
      const int a = (s * 7 + threadIdx.x) & 1;
      const unsigned pair = *reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(calib_tab + base) + cur);
      const unsigned mb = reinterpret_cast<const unsigned char*>(calib_tab + base)[960 + (cur >> 5)];
      const unsigned sh = ((mb >> ((cur >> 2) & 7)) << 4) + (unsigned)(a << 4);
      const int nxt = (int)(__builtin_amdgcn_ubfe(pair, sh, 16u) & 0x1fcu);   // a multiple of 4 below 512
      ++h;
      const bool term = h >= H;
      cur = term ? 0 : nxt;
      h = term ? 0 : h;
    }
  }
  sink[blockIdx.x * 64 + threadIdx.x] = cur + h;
}

// ---------------------------------------------------------------------------------------------------------------
// K5T k_diam_tiles: K5S with the value rows a cluster of states needs gathered into LDS first.
//
// K5S reads V[successor][lane] straight from HBM/L2 for every entry of every row: at C5 (S = 50 272, the two value
// arrays of a 64-target group are 25.7 MB) every value row is fetched ~3 times per sweep (PMC: 3.1 x the algorithmic
// reads), because a row's successors are far away in the state numbering and nothing that large stays in L2 with
// hundreds of groups in flight.  Here the states of an instance are cut into CLUSTERS of <= 64 states (breadth-first
// regions of the transition graph, built on the host) whose distinct successors outside the cluster (the "halo") are
// few; a wavefront takes a cluster at a time, gathers the cluster's own rows and its halo rows -- R <= RMAX rows of 256
// bytes -- into its private LDS tile with LDS-DMA loads (global_load_lds_dwordx4: 4 rows per instruction, the source row
// of a lane is arbitrary, the LDS image is linear), and then every gather of the sweep is a conflict-free ds_read_b32.
// Each value row is read from memory (1 + halo/cluster) times per sweep instead of ~3.
//
// The arithmetic is K5S's: every row keeps its entries in ascending ORIGINAL column order (only the index is replaced by
// the position in the tile), float32 with separately rounded multiply and add, so the results are bit-equal to K5S, K2
// and the oracle.
// ---------------------------------------------------------------------------------------------------------------
constexpr int K5T_C = 32;      // state slots per cluster (<= 64: one lane per slot holds the slot's state number)
struct TileArgs {
  const int32_t* inst_c0;      // [B] first cluster of the instance
  const int32_t* inst_ncl;     // [B] clusters of the instance
  const int32_t* cl_n;         // [clusters] states in the cluster (<= K5T_C)
  const int32_t* cl_R;         // [clusters] tile rows (cluster + halo), a multiple of 4
  const int32_t* rows;         // [clusters][RMAX] instance-relative state of every tile row (padding repeats row 0)
  const int32_t* lcol;         // [clusters][K5T_C * A * K] tile row of every entry (+64 entries of tail padding)
  const float* val;            // same shape: coefficients (+0.0 for padding)
};

template <int NW, int A, int K, int RMAX>
__global__ void __launch_bounds__(NW * 64) k_diam_tiles(DpTables t, DiamLanesArgs g, TileArgs ta) {
  constexpr int AK = A * K, U = 64 / AK;
  static_assert(U >= 1 && RMAX % 4 == 0, "shape");
  extern __shared__ float k5t_lds[];             // NW tiles of RMAX x 64 floats
  __shared__ float red_d[2][NW][64];
  __shared__ float red_m[2][NW][64];
  const int grp = blockIdx.x;
  const int b = g.grp_inst[grp];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int target = g.grp_target0[grp] + lane;
  const bool active = lane < g.grp_count[grp];
  float* Vold = g.vbuf + g.grp_voff[grp];
  float* Vnew = Vold + (int64_t)S * 64;
  for (int64_t i = threadIdx.x; i < (int64_t)S * 128; i += NW * 64) Vold[i] = 0.0f;
  __syncthreads();
  float* tile = k5t_lds + (size_t)wave * RMAX * 64;
  const int c0 = ta.inst_c0[b], ncl = ta.inst_ncl[b];

  bool done = !active;
  float result = 0.0f;
  int status = active ? -5 : 0;
  int64_t it = 0;
  while (it < t.max_sweeps) {
    ++it;
    float dmax = 0.0f, vmin = 3.0e38f;
    for (int ci = wave; ci < ncl; ci += NW) {
      const int c = c0 + ci;
      const int n = ta.cl_n[c], R = ta.cl_R[c];
      const int32_t* crow = ta.rows + (int64_t)c * RMAX;
      // every ds_read of the previous cluster has returned before its tile is overwritten
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      // gather: instruction q brings tile rows 4q .. 4q+3, 16 lanes x 16 bytes per row
      int rid[RMAX / 4];   // all row numbers first (the list is padded to RMAX entries), then the gathers back to back
#pragma unroll
      for (int q = 0; q < RMAX / 4; ++q) rid[q] = crow[4 * q + (lane >> 4)];
#pragma unroll
      for (int q = 0; q < RMAX / 4; ++q) {
        if (q < R / 4) {
          const float* src = Vold + (int64_t)rid[q] * 64 + (lane & 15) * 4;
          __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(tile + q * 256), 16, 0, 0);
        }
      }
      const int myrow = crow[lane < n ? lane : 0];   // state of cluster slot `lane` (K5T_C = 64 slots)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const int32_t* ec = ta.lcol + (int64_t)c * K5T_C * AK;
      const float* ev = ta.val + (int64_t)c * K5T_C * AK;
      for (int s0 = 0; s0 < n; s0 += U) {
        const int ccol = ec[s0 * AK + lane];
        const float cval = ev[s0 * AK + lane];
        float x[U * AK], vo[U];
#pragma unroll
        for (int e = 0; e < U * AK; ++e) {
          const int cl = __builtin_amdgcn_readlane(ccol, e);
          x[e] = tile[cl * 64 + lane];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) vo[u] = tile[((s0 + u < n) ? s0 + u : s0) * 64 + lane];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (s0 + u < n) {
            float v = 0.0f;
#pragma unroll
            for (int a = 0; a < A; ++a) {
              float acc = 0.0f;
#pragma unroll
              for (int k = 0; k < K; ++k) {
                const int e = (u * A + a) * K + k;
                const float coef = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cval), e));
                acc = __fadd_rn(acc, __fmul_rn(coef, x[e]));
              }
              const float qv = __fadd_rn(-1.0f, __fmul_rn(t.gamma, acc));
              v = (a == 0) ? qv : fmaxf(v, qv);
            }
            const int s = __builtin_amdgcn_readlane(myrow, s0 + u);
            if (s == target) v = __fadd_rn(0.0f, __fmul_rn(t.gamma, __fadd_rn(0.0f, __fmul_rn(1.0f, vo[u]))));
            Vnew[(int64_t)s * 64 + lane] = v;
            dmax = fmaxf(dmax, fabsf(vo[u] - v));
            vmin = fminf(vmin, v);
          }
        }
      }
    }
    const int par = (int)(it & 1);
    red_d[par][wave][lane] = dmax;
    red_m[par][wave][lane] = vmin;
    __syncthreads();   // also orders this sweep's Vnew stores before the next sweep's gathers (workgroup scope, same CU)
    float diff = 0.0f, mn = 3.0e38f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      diff = fmaxf(diff, red_d[par][w][lane]);
      mn = fminf(mn, red_m[par][w][lane]);
    }
    float* tmp = Vold; Vold = Vnew; Vnew = tmp;
    if (!done && (double)diff < t.eps) {
      done = true;
      result = -mn;
      status = 0;
    }
    if (__all(done)) break;
  }
  if (wave == 0 && active) {
    t.per_target[soff + target] = result;
    t.status[soff + target] = status;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// K5D k_diam_lanes_f64: the reference's SPARSE float64 diameter (`_get_sparse_diameter`,
// colosseum/hardness/measures/diameter.py:382-420 -- what a single-core reference runs for continuous MDPs above 1000
// states).  Per target i: float64 expected hitting times over the other states, Jacobi sweeps
//     ET'[s] = min_a ( T[s,a,i] + sum_{j != i, ascending} float64(T[s,a,j]) * (1 + ET[j]) ),
// diff = max_{s != i} |ET' - ET|.  The reference stops a target at diff < eps OR (diff < 0.05 and max ET' - 1 < the
// running maximum over the targets before it): the second clause makes the result depend on the target ORDER.  The
// sweeps themselves do not depend on it, so the kernel runs every target to diff < eps (lane = target, 64 targets per
// workgroup, value vectors interleaved in HBM as in K5S) and LOGS (diff, max ET') of every sweep from the first one with
// diff < max(eps, 0.05) on; the host then walks the targets in the reference's order and takes, for each, the sweep at
// which the reference would have stopped (cmdp_diameter_sparse_f64).
// ---------------------------------------------------------------------------------------------------------------
struct DiamF64Args {
  const int32_t* grp_inst;
  const int32_t* grp_target0;
  const int32_t* grp_count;
  const int64_t* grp_voff;     // offset of the group's two value arrays in `vbuf` (doubles)
  double* vbuf;
  double* log;                 // [groups][64][log_cap][2]: (diff, max) per logged sweep
  int32_t* log_n;              // [groups][64] logged sweeps (log_cap + 1: the log overflowed)
  int32_t log_cap;
};

template <int NW>
__global__ void __launch_bounds__(NW * 64) k_diam_lanes_f64(DpTables t, DiamF64Args g) {
  __shared__ double red_d[2][NW][64];
  __shared__ double red_m[2][NW][64];
  const int grp = blockIdx.x;
  const int b = g.grp_inst[grp];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int A = t.A;
  const int64_t soff = t.state_off[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int64_t* ptr = t.csr_ptr + soff * A;
  const int target = g.grp_target0[grp] + lane;
  const bool active = lane < g.grp_count[grp];
  double* Eold = g.vbuf + g.grp_voff[grp];
  double* Enew = Eold + (int64_t)S * 64;
  for (int64_t i = threadIdx.x; i < (int64_t)S * 128; i += NW * 64) Eold[i] = 0.0;
  __syncthreads();
  double* mylog = g.log + ((int64_t)grp * 64 + lane) * g.log_cap * 2;
  const double log_thr = t.eps > 0.05 ? t.eps : 0.05;
  bool done = !active;
  int n_logged = 0;
  int64_t it = 0;
  while (it < t.max_sweeps) {
    ++it;
    double dmax = 0.0, emax = -1.0e300;
    for (int s = wave; s < S; s += NW) {
      double v = 0.0;
      for (int a = 0; a < A; ++a) {
        const int64_t lo = ptr[(int64_t)s * A + a], hi = ptr[(int64_t)s * A + a + 1];
        double acc = 0.0, te = 0.0;
        for (int64_t k = lo; k < hi; ++k) {
          const int c = t.csr_col[k];
          const double p = (double)t.csr_val[k];
          const double term = __dmul_rn(p, __dadd_rn(1.0, Eold[(int64_t)c * 64 + lane]));
          if (c == target) te = p;                  // the hit: its column is not part of the sum
          else acc = __dadd_rn(acc, term);
        }
        const double q = __dadd_rn(te, acc);
        v = (a == 0) ? q : fmin(v, q);
      }
      Enew[(int64_t)s * 64 + lane] = v;
      if (s != target) {
        dmax = fmax(dmax, fabs(Eold[(int64_t)s * 64 + lane] - v));
        emax = fmax(emax, v);
      }
    }
    const int par = (int)(it & 1);
    red_d[par][wave][lane] = dmax;
    red_m[par][wave][lane] = emax;
    __syncthreads();
    double diff = 0.0, mx = -1.0e300;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      diff = fmax(diff, red_d[par][w][lane]);
      mx = fmax(mx, red_m[par][w][lane]);
    }
    double* tmp = Eold; Eold = Enew; Enew = tmp;
    if (!done && diff < log_thr) {
      if (wave == 0) {
        if (n_logged < g.log_cap) { mylog[2 * n_logged] = diff; mylog[2 * n_logged + 1] = mx; }
      }
      ++n_logged;
      if (diff < t.eps || n_logged > g.log_cap) done = true;
    }
    if (__all(done)) break;
  }
  if (wave == 0 && active) {
    g.log_n[(int64_t)grp * 64 + lane] = done ? n_logged : -1;   // -1: max_sweeps reached
    t.status[soff + target] = done ? 0 : -5;
  }
}
