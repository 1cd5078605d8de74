// cmdp_psrlc.h -- K13: batched posterior sampling for the continuous setting with PLAIN posterior sampling (the reference's
// own no_optimistic_sampling=True path, which it also takes by itself when S^2 * A > 6 000 000), one reference agent per
// instance,
//   colosseum/agent/agents/infinite_horizon/posterior_sampling.py   (PSRLContinuous)
//   colosseum/agent/mdp_models/bayesian_model.py                    (BayesianMDPModel.step_update, sample)
//   colosseum/dynamic_programming/infinite_horizon.py:14-44         (discounted_value_iteration)
//   colosseum/experiment/agent_mdp_interaction.py:224-298           (MDPLoop.run)
// with the interaction, the posterior tables, the artificial-episode rule, the sample, the solve and the actor's Q on the
// device.  The posterior tables, both samplers (k_psrl_sample, psrl_host::reference_draw) and the release (k_psrl_resume with
// do_reset = 0) are K12's, unchanged (cmdp_psrl.h).
//
// What the reference does on this path:
//   Driving order (MDPLoop.run).  before_start_interacting: one episode_end_update on the prior; then per step select_action
//     -> step -> step_update, then episode_end_update if is_episode_end.  The environment is never reset; in the continuous
//     setting ts_tp1.last() is never true.
//   step_update (:390-409).  N_NIG.update_sa for the one reward (psrl_nnig_update, the arithmetic of K12's walk);
//     M_DIR: hyper_params[s, a, s'] += 1 on EVERY step, there is never a last step; the agent's N[s, a, s'] += 1; s' is
//     appended to episode_transition_data[s, a].  self.M is never read and is not built.
//   is_episode_end (:346-358) with min_steps_before_new_episode = 0.  nu_k = visits of (s, a) since the last
//     episode_end_update, N_tau = N[s, a].sum(), both with the current step; the episode ends iff N_tau >= 2 * (N_tau - nu_k).
//     A first visit always ends an episode.
//   episode_end_update (:360-377).  T = M_DIR.sample(), R = N_NIG.sample(), Q, _ = discounted_value_iteration(T, R) with
//     gamma = 0.99, epsilon = 1e-3; Q is installed in the actor; episode_transition_data is cleared: every nu_k is 0 again.
//   select_action.  Greedy on Q[s, :] with the RandomState(seed) tie-break; extended_action_to_real is the identity here.
//   current_optimal_stochastic_policy (:174-178).  discounted_value_iteration on get_map_estimate(), then
//     get_policy_from_q_values(Q, True).
// The sampled T is not dense in the reference's sense: M_DIR._sample casts the gamma variates to float32, where small shapes
// underflow to exactly 0 (a row of zeros stays the zero row: 0 / (1e-5 + 0)), and discounted_value_iteration picks its scheme
// PER SAMPLE from the count of non-zero elements: Jacobi on sparse.COO(T) when T.size > 300 * 3 * 300 and nnz / T.size < 0.2,
// dense Gauss-Seidel otherwise.  model_vi_scheme (cmdp_model_vi.h) is that rule.
//
// Kernels:
//   k_psrlc_walk            lane per instance: greedy action on Q[s, :], the environment's step, the two model updates, the
//                           visit counters of the row, and PARKS after the step that ends an artificial episode.
//                           n_sa [R] is N[s, a].sum() and is never cleared.  nu [R] carries the episode it was last written in
//                           (stamp [R]) and counts as 0 when that is not the instance's current `episode`: an
//                           episode_end_update, internal or external, resets every nu_k at the cost of one increment.
//                           One template for the whole family, <GATE, OPT>: GATE compiles min_steps_before_new_episode in
//                           (PcGate), OPT is the optimistic agent's walk (K18: PoArgs).  <false, false> is the walk described
//                           here; the host picks the instantiation (cmdp_psrlc_run).
//   k_vi_discounted_dense   workgroup per listed instance, V (and V_old) in LDS; the arithmetic is defined below.
//
// The solver's arithmetic, one definition for the agent and for cmdp_vi_discounted_dense.  A ROW SUM over the columns j of
// row (s, a) is taken in float64: a wavefront owns the row, lane l adds the terms of its own columns in ascending order to
// +0 -- columns 4 l + 256 k + {0, 1, 2, 3} when S % 4 == 0 and the row is 16-byte aligned (16-byte loads), columns l + 64 k
// otherwise -- and the 64 partial sums are added by the xor butterfly 32, 16, 8, 4, 2, 1.  Every term is a product of two
// float32 values and so exact in float64.  V starts at 0.
//   Gauss-Seidel  acc = sum_j double(fl32(gamma * T[s, a, j])) * double(V[j]), V holding this sweep's values of the states
//                 before s;  Q[s, a] = float(double(R[s, a]) + acc);  V[s] = max_a Q[s, a], taken at once
//   Jacobi        tv = float(sum_j double(T[s, a, j]) * double(V_old[j]));  Q[s, a] = R[s, a] + gamma * tv as two float32
//                 operations without contraction;  V[s] = max_a Q[s, a]
//   both stop after the sweep with max_s |V_old[s] - V[s]| < epsilon (float32 difference, compared in float64); at
//   max_sweeps the status is CMDP_ERR_MAX_ITER and Q, V are the last sweep's.
// How many wavefronts share an instance does not enter the definition: WAVES of them (4, or 1 for measurements: ddv_waves in
// cmdp.hip) split a state's rows (Gauss-Seidel: wave w takes the actions w, w + WAVES, ...; one barrier per state) or the
// states (Jacobi: wave w takes the states w, w + WAVES, ...; one barrier per sweep).  Gauss-Seidel is serial over the states but the rows of T do not depend on V:
// a wave issues the loads of its NEXT row (and its reward) before it reduces the current one, so only the reduction, the LDS
// reads of V and the barrier are on the chain from state to state.
#pragma once
#include "cmdp_model_vi.h"
#include "cmdp_psrl.h"
#include "cmdp_map_vi.h"

#define DDV_MAX_WAVES 4
#define DDV_PF 4   // register trips of a prefetched row: 1024 columns with 16-byte loads, 256 without; the rest is loaded in place

struct PcCounters {
  int32_t* n_sa;    // [R] N[s, a].sum(-1)
  int32_t* nu;      // [R] visits in the episode `stamp`
  int32_t* stamp;   // [R] starts at 0; `episode` is >= 1 once the agent exists (the solve on the prior)
};

// min_steps_before_new_episode (posterior_sampling.py:353-355), for the walks compiled with GATE: is_episode_end evaluates its
// rule only when the in-run time h of the step (mdp.h read BEFORE the step: t.hstep at the top of the loop) is at least
// `min_steps` past last_change, and every check that passes moves last_change to h, whether or not the episode ends.  A
// frozen instance never calls is_episode_end; episode_end_update touches neither.  GATE = false is the walk of
// min_steps = 0: it reads and writes no last_change.
struct PcGate {
  int32_t min_steps;
  int32_t* last_change;   // [B] starts at 0
};

// The device arguments of the optimistic agent (K18, cmdp_psrlo.h), defined here because the walk takes them.  Of these the
// walk (OPT = true) reads psi, q_off, N and Qx: its Q has A * psi_b values per state at per-instance offsets, the action played
// is j / psi_b, and the agent's N is counted at the layout's positions.  The plain walk (OPT = false) reads no member; the
// host passes it empty.  The struct is passed whole, not as a view of the four: the kernel-argument layout is part of what the
// register allocator sees, and this one gives every instantiation the counts recorded in DESIGN.md.
struct PoArgs {
  const int32_t* psi;       // [B]
  const double* eta;        // [B]
  const double* log4s;      // [B] numpy's log(4 * S)
  const int64_t* q_off;     // [B] first extended row: R_ext, Q [S][A * psi], bump [psi][S * A]
  const int64_t* tx_off;    // [B] first element of T_ext (a multiple of 4); also of the compact posterior rows
  const int64_t* k_off;     // [B] first of the instance's psi values of z
  const int64_t* pm_off;    // [B] first of the instance's psi * nz_b values of pmk
  int32_t* N;               // [NZ] the agent's N at the layout's positions
  double* pm;               // [NZ] P_minus of the chain
  float* pmk;               // per k the float32 layout values of the simple rows
  float* bump;              // per (k, row) the float32 value at z_k
  int32_t* z;               // [sum psi]
  uint8_t* simple;          // [R]
  const int32_t* pidx;      // [R] index of a posterior row among the instance's posterior rows (reference sampler)
  const int32_t* n1;        // [B] posterior rows of the last draw
  const float* post;        // at tx_off[b]: [psi][n1][S] posterior rows as the host drew them; null: the Philox sampler
  float* Tx;
  float* Rx;                // [sum S * A * psi]
  float* Qx;                // the actor's table
  float* const* pk;         // [B] null: the dense route.  The compact route: the instance's posterior rows [psi][n1][S]; Tx unread
  int pk_from_host;         // compact route: 1 the host has drawn and uploaded the posterior rows (reference sampler; `post`
                            // unread), 0 the kernel draws them (Philox sampler)
};

template <bool GATE, bool OPT>
__global__ void __launch_bounds__(256) k_psrlc_walk(EnvTables t, PsArgs p, PcCounters c, PoArgs o, PcGate gt, int64_t n_steps,
                                                    const uint8_t* __restrict__ train_mask, int8_t* __restrict__ act_trace,
                                                    int32_t* __restrict__ obs_trace, double* __restrict__ rew_trace,
                                                    double* __restrict__ cum_reward) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  long long left = p.call.left[b];
  if (left == 0) return;
  const int64_t soff = t.state_off[b], ebase = t.entry_base[b];
  const int A = t.A;
  int psi = 1;
  if constexpr (OPT) psi = o.psi[b];
  const int AX = A * psi;   // Q values per state
  const uint2 key = t.philox_key ? t.philox_key[b] : make_uint2(0, 0);
  int32_t cur = t.cur[b], h = t.hstep[b];
  unsigned long long nt = t.n_trans[b];
  const float* Q = p.Q + soff * A;
  if constexpr (OPT) Q = o.Qx + o.q_off[b];
  float* RP = p.rp + soff * A * 4;
  uint32_t* mt = p.mt + (int64_t)b * 624;
  int32_t* mtp = p.mt_pos + b;
  const int32_t ep = (int32_t)p.episode[b];
  const bool train = train_mask ? train_mask[b] != 0 : true;   // a frozen instance acts on the Q it holds and never parks
  int32_t lc = 0;
  if (GATE && train) lc = gt.last_change[b];
  double sum = cum_reward[b];
  bool parked = false;
  while (left > 0) {
    const int64_t step = n_steps - left;
    const int32_t h0 = h;
    int action = greedy_action_row(Q + (int64_t)cur * AX, AX, mt, mtp);
    if constexpr (OPT) action /= psi;   // extended_action_to_real
    const int32_t idx = cur * A + action;
    const unsigned long long n0 = nt;
    int32_t obs;
    double rraw;
    int64_t e;
    env_transition(t, soff, ebase, key, cur, h, nt, action, obs, rraw, e);   // continuous: never terminates
    if (t.sp_rkind && t.sp_rkind[e] == 1) rraw = philox_beta(t.sp_rp0[e], t.sp_rp1[e], n0, key, t.beta_gammas);  // throughput mode only
    const double reward = rraw * t.rscale - t.rmin;
    sum += reward;
    if (act_trace) act_trace[step * t.B + b] = (int8_t)action;
    if (obs_trace) obs_trace[step * t.B + b] = obs;
    if (rew_trace) rew_trace[step * t.B + b] = reward;
    --left;
    if (train) {
      psrl_nnig_update(RP + (int64_t)idx * 4, reward);
      const int32_t pos = p.slot[e];
      float* tc = p.tp + pos;   // M_DIR.update_sa: every step
      *tc = __fadd_rn(*tc, 1.0f);
      if constexpr (OPT) o.N[pos] += 1;
      const int64_t r = soff * A + idx;
      const int32_t n_tau = c.n_sa[r] + 1;
      const int32_t nu_k = (c.stamp[r] == ep ? c.nu[r] : 0) + 1;
      c.n_sa[r] = n_tau;
      c.nu[r] = nu_k;
      c.stamp[r] = ep;
      bool checked = true;
      if (GATE) {
        checked = h0 - lc >= gt.min_steps;   // both >= 0: the difference cannot wrap
        if (checked) lc = h0;
      }
      if (checked && n_tau >= 2 * (n_tau - nu_k)) {   // is_episode_end: the round samples, solves and installs Q
        parked = true;
        break;
      }
    }
  }
  t.cur[b] = cur;
  t.hstep[b] = h;
  t.n_trans[b] = nt;
  cum_reward[b] = sum;
  p.call.left[b] = left;
  if (GATE && train) gt.last_change[b] = lc;
  if (parked) p.call.park_list[atomicAdd(p.call.park_count, 1)] = b;
}

// After a round's solve: tally[0] += instances that did not converge, tally[1] (zeroed by the round) += their sweeps
__global__ void __launch_bounds__(256) k_psrlc_tally(const int32_t* __restrict__ list, int count, const int32_t* __restrict__ status,
                                                     const int64_t* __restrict__ sweeps, unsigned long long* __restrict__ tally) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const int b = list[k];
  if (status[b] != 0) atomicAdd(tally, 1ull);
  atomicAdd(tally + 1, (unsigned long long)sweeps[b]);
}

struct DdvArgs {
  const int32_t* list;   // block k solves instance list[k]; null: instance k
  const int32_t* S;      // [count]
  const int32_t* A;      // [count]
  const int64_t* t_off;  // [count] first element of T[S, A, S]
  const int64_t* r_off;  // [count] first row: R, Q [S, A]
  const int64_t* s_off;  // [count] first state: V [S]
  const float* T;
  const float* R;
  float gamma;
  double eps;
  int scheme;            // CMDP_SCHEME_AUTO: model_vi_scheme per instance on its count of non-zero elements
  int64_t size_threshold;
  double density_threshold;
  int64_t max_sweeps;
  float* Q;
  float* V;
  int64_t* sweeps;       // [count]
  int32_t* scheme_used;  // [count]
  int32_t* status;       // [count] 0 or CMDP_ERR_MAX_ITER
};

// Dynamic LDS of a launch whose largest instance has max_S states: V, V_old, then per wave two maxima of the stopping rule,
// two of a state's rows and one count
inline size_t ddv_lds_bytes(int max_S) {
  return (size_t)2 * ((max_S + 3) & ~3) * sizeof(float) + (size_t)DDV_MAX_WAVES * (4 * sizeof(float) + sizeof(long long));
}

// One row of T in flight: its reward and the first DDV_PF trips of every lane
struct DdvRow {
  float4 x[DDV_PF];
  float r;
};

__device__ __forceinline__ void ddv_fetch(DdvRow& d, const float* __restrict__ tr, const float* __restrict__ rr, int S, int lane,
                                          bool vec) {
  d.r = *rr;
#pragma unroll
  for (int k = 0; k < DDV_PF; ++k) {
    d.x[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (vec) {
      const int c = lane * 4 + k * 256;
      if (c < S) d.x[k] = *reinterpret_cast<const float4*>(tr + c);
    } else {
      const int c = lane + k * 64;
      if (c < S) d.x[k].x = tr[c];
    }
  }
}

template <bool GS>
__device__ __forceinline__ double ddv_term(float x, float v, float gamma) {
  return GS ? (double)__fmul_rn(gamma, x) * (double)v : (double)x * (double)v;   // exact products: fused or not, the same sum
}

// The row sum of the header comment; `v` in LDS
template <bool GS>
__device__ __forceinline__ double ddv_dot(const DdvRow& d, const float* __restrict__ tr, const float* v, int S, int lane, bool vec,
                                          float gamma) {
  double acc = 0.0;
  if (vec) {
#pragma unroll
    for (int k = 0; k < DDV_PF; ++k) {
      const int c = lane * 4 + k * 256;
      if (c < S) {
        const float4 w = *reinterpret_cast<const float4*>(v + c);
        acc += ddv_term<GS>(d.x[k].x, w.x, gamma);
        acc += ddv_term<GS>(d.x[k].y, w.y, gamma);
        acc += ddv_term<GS>(d.x[k].z, w.z, gamma);
        acc += ddv_term<GS>(d.x[k].w, w.w, gamma);
      }
    }
    for (int c = lane * 4 + DDV_PF * 256; c < S; c += 256) {
      const float4 x = *reinterpret_cast<const float4*>(tr + c);
      const float4 w = *reinterpret_cast<const float4*>(v + c);
      acc += ddv_term<GS>(x.x, w.x, gamma);
      acc += ddv_term<GS>(x.y, w.y, gamma);
      acc += ddv_term<GS>(x.z, w.z, gamma);
      acc += ddv_term<GS>(x.w, w.w, gamma);
    }
  } else {
#pragma unroll
    for (int k = 0; k < DDV_PF; ++k) {
      const int c = lane + k * 64;
      if (c < S) acc += ddv_term<GS>(d.x[k].x, v[c], gamma);
    }
    for (int c = lane + DDV_PF * 64; c < S; c += 64) acc += ddv_term<GS>(tr[c], v[c], gamma);
  }
  return wave_sum(acc);
}

template <int WAVES>
__global__ void __launch_bounds__(WAVES * 64) k_vi_discounted_dense(DdvArgs g) {
  static_assert(WAVES >= 1 && WAVES <= DDV_MAX_WAVES, "ddv_lds_bytes sizes the per-wave words for DDV_MAX_WAVES");
  extern __shared__ __align__(16) float ddv_lds[];
  constexpr int NT = WAVES * 64;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = g.list ? g.list[blockIdx.x] : blockIdx.x;
  const int S = g.S[b], A = g.A[b];
  const int spad = (S + 3) & ~3;
  float* V = ddv_lds;
  float* W = V + spad;                    // V_old
  float* red = W + spad;                  // [2][DDV_MAX_WAVES] the waves' maxima of |V_old - V|, by the sweep's parity
  float* wq = red + 2 * DDV_MAX_WAVES;    // [2][DDV_MAX_WAVES] the waves' maxima over their rows of a state, by the state's parity
  long long* cnt = reinterpret_cast<long long*>(wq + 2 * DDV_MAX_WAVES);   // [DDV_MAX_WAVES]
  const float* __restrict__ T = g.T + g.t_off[b];
  const float* __restrict__ R = g.R + g.r_off[b];
  float* __restrict__ Q = g.Q + g.r_off[b];
  const float gamma = g.gamma;
  const bool vec = (S & 3) == 0 && (reinterpret_cast<uintptr_t>(T) & 15) == 0;

  // prologue: the rule's count of non-zero elements, one coalesced pass
  int scheme = g.scheme;
  if (scheme == CMDP_SCHEME_AUTO) {
    const int64_t n = (int64_t)S * A * S;
    long long c = 0;
    if (vec) {
      for (int64_t i = (int64_t)tid * 4; i < n; i += NT * 4) {
        const float4 x = *reinterpret_cast<const float4*>(T + i);
        c += (x.x != 0.0f) + (x.y != 0.0f) + (x.z != 0.0f) + (x.w != 0.0f);
      }
    } else {
      for (int64_t i = tid; i < n; i += NT) c += T[i] != 0.0f;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) cnt[wid] = c;
    __syncthreads();
    long long nnz = 0;
    for (int w = 0; w < WAVES; ++w) nnz += cnt[w];
    scheme = model_vi_scheme(S, A, (int64_t)nnz, g.size_threshold, g.density_threshold);
  }
  for (int i = tid; i < spad; i += NT) { V[i] = 0.0f; W[i] = 0.0f; }
  __syncthreads();

  float* Vout = V;
  int64_t sweep = 1;
  bool done = false;
  if (scheme == CMDP_SCHEME_JACOBI) {
    float* Vold = V;
    float* Vnew = W;
    for (;; ++sweep) {
      float d = 0.0f;
      DdvRow cur;
      if (wid < S) ddv_fetch(cur, T + (int64_t)wid * A * S, R + (int64_t)wid * A, S, lane, vec);
      for (int s = wid; s < S; s += WAVES) {
        float vmax = -INFINITY;
        for (int a = 0; a < A; ++a) {
          const int row = s * A + a;
          const int nrow = a + 1 < A ? row + 1 : (s + WAVES) * A;   // this wave's next row
          DdvRow nxt;
          if (nrow < S * A) ddv_fetch(nxt, T + (int64_t)nrow * S, R + nrow, S, lane, vec);
          const float tv = (float)ddv_dot<false>(cur, T + (int64_t)row * S, Vold, S, lane, vec, gamma);
          const float q = __fadd_rn(cur.r, __fmul_rn(gamma, tv));
          if (lane == 0) Q[row] = q;
          vmax = fmaxf(vmax, q);
          if (nrow < S * A) cur = nxt;
        }
        if (lane == 0) Vnew[s] = vmax;
        d = fmaxf(d, fabsf(__fsub_rn(Vold[s], vmax)));
      }
      float* rb = red + (sweep & 1) * DDV_MAX_WAVES;
      if (lane == 0) rb[wid] = d;
      __syncthreads();   // Vnew is whole, and every wave has read Vold
      for (int w = 0; w < WAVES; ++w) d = fmaxf(d, rb[w]);
      float* x = Vold; Vold = Vnew; Vnew = x;
      done = (double)d < g.eps;
      if (done || sweep >= g.max_sweeps) break;
    }
    Vout = Vold;
  } else {
    const int nw = A < WAVES ? A : WAVES;   // waves that own a row of every state
    for (;; ++sweep) {
      for (int i = tid; i < S; i += NT) W[i] = V[i];
      __syncthreads();
      DdvRow cur;
      if (wid < A) ddv_fetch(cur, T + (int64_t)wid * S, R + wid, S, lane, vec);
      for (int s = 0; s < S; ++s) {
        float wmax = -INFINITY;
        for (int a = wid; a < A; a += WAVES) {
          const int row = s * A + a;
          const int nrow = a + WAVES < A ? row + WAVES : (s + 1) * A + wid;   // this wave's next row
          DdvRow nxt;
          if (nrow < S * A) ddv_fetch(nxt, T + (int64_t)nrow * S, R + nrow, S, lane, vec);
          const double acc = ddv_dot<true>(cur, T + (int64_t)row * S, V, S, lane, vec, gamma);
          const float q = (float)__dadd_rn((double)cur.r, acc);
          if (lane == 0) Q[row] = q;
          wmax = fmaxf(wmax, q);
          if (nrow < S * A) cur = nxt;
        }
        float* qb = wq + (s & 1) * DDV_MAX_WAVES;
        if (lane == 0 && wid < A) qb[wid] = wmax;
        __syncthreads();   // every wave has read V for this state; the state's rows are all in qb
        float v = qb[0];
        for (int w = 1; w < nw; ++w) v = fmaxf(v, qb[w]);
        // every wave stores the same V[s] for itself: its own LDS operations stay in order, so it needs no second barrier
        // before it reads V for the next state, and no wave waits for another's store
        if (lane == 0) V[s] = v;
      }
      float d = 0.0f;
      for (int i = tid; i < S; i += NT) d = fmaxf(d, fabsf(__fsub_rn(W[i], V[i])));
      d = wave_max(d);
      float* rb = red + (sweep & 1) * DDV_MAX_WAVES;
      if (lane == 0) rb[wid] = d;
      __syncthreads();   // every thread has read W before the next sweep's copy
      for (int w = 0; w < WAVES; ++w) d = fmaxf(d, rb[w]);
      done = (double)d < g.eps;
      if (done || sweep >= g.max_sweeps) break;
    }
  }
  float* __restrict__ Vg = g.V + g.s_off[b];
  for (int i = tid; i < S; i += NT) Vg[i] = Vout[i];
  if (tid == 0) {
    g.sweeps[b] = sweep;
    g.scheme_used[b] = scheme;
    g.status[b] = done ? 0 : CMDP_ERR_MAX_ITER;
  }
}

// The dense MAP model of the listed instances for the solve behind policy(): get_map_estimate() =
// (hyper_params / hyper_params.sum(-1, keepdims=True), hyper_params[:, :, 0]) by K15's definition (cmdp_map_vi.h,
// cmdp_psrl_map_rows): rowsum = numpy's pairwise float32 sum of the dense row, T_map = hp / rowsum at the layout's positions
// and prior / rowsum elsewhere, as float32 divisions; R_map = mu.  Written into a region of its own, so the last sample stays
// what it was.  A lane per row takes the row sums, then a wavefront per row writes the row once, coalesced.
struct PcMapArgs {
  const int32_t* list;     // block k fills instance list[k]; null: instance k
  const int32_t* S;        // [B]
  const int32_t* A;        // [B]
  const int64_t* r_off;    // [B] first row
  const int64_t* t_off;    // [B] first element of the instance's dense T (a multiple of 4)
  const int64_t* row_ptr;  // [R + 1]
  const int32_t* col;
  const float* hp;         // M_DIR hyper-parameters at the layout's positions
  const float* prior;      // [B]
  const float* rp;         // [R][4] N_NIG hyper-parameters
  float* rowsum;           // [R] scratch
  float* T;                // out: T_map
  float* Rm;               // [R] out: R_map
};

__global__ void __launch_bounds__(MAPVI_THREADS) k_psrlc_map_fill(PcMapArgs g) {
  __shared__ int plan_work[2 * MAPVI_DEPTH + 2];
  __shared__ short plan_run[MAPVI_MAX_RUNS];
  __shared__ signed char plan_merges[MAPVI_MAX_RUNS];
  __shared__ int plan_n;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = g.list ? g.list[blockIdx.x] : blockIdx.x;
  const int S = g.S[b], A = g.A[b];
  const int nrows = S * A;
  const int64_t r0 = g.r_off[b];
  const int64_t* __restrict__ ptr = g.row_ptr + r0;
  const float prior = g.prior[b];
  float* __restrict__ T = g.T + g.t_off[b];
  if (tid == 0) plan_n = mapvi_plan(S, plan_work, plan_run, plan_merges);
  __syncthreads();
  const int n_runs = plan_n;
  for (int row = tid; row < nrows; row += MAPVI_THREADS) {
    MapViRow<float> r{g.col, g.hp, ptr[row], ptr[row + 1], prior};
    g.rowsum[r0 + row] = mapvi_rowsum(r, n_runs, plan_run, plan_merges);
    g.Rm[r0 + row] = g.rp[(r0 + row) * 4];
  }
  __syncthreads();   // the workgroup's row sums are written
  for (int row = wid; row < nrows; row += MAPVI_THREADS / 64) {
    const float rs = g.rowsum[r0 + row];
    const float c = __fdiv_rn(prior, rs);
    const int64_t rb = ptr[row], re = ptr[row + 1];
    for (int j = lane; j < S; j += 64) {
      const int64_t m = psrl_layout_find(g.col, rb, re, j);   // the row's layout positions scattered over the prior
      T[(int64_t)row * S + j] = m >= 0 ? __fdiv_rn(g.hp[m], rs) : c;
    }
  }
}
