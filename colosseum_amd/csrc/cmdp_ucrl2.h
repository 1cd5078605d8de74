// cmdp_ucrl2.h -- K11: batched UCRL2 for the continuous setting, one reference agent per environment instance,
//   colosseum/agent/agents/infinite_horizon/ucrl2.py           (UCRL2Continuous: counts, bounds, model_update)
//   colosseum/experiment/agent_mdp_interaction.py:238-263      (select_action -> step -> step_update -> is_episode_end)
//   colosseum/agent/actors/Q_values_actor.py:67-88             (greedy action, uniform tie-break from RandomState(seed))
// with interaction, counts, confidence bounds, the estimated model and the optimistic solves (K10, cmdp_evi.h) on the
// device.  The model lives in K10's layout: per row the DISTINCT successors of the environment's row in ascending
// order (`row_ptr` / `col`, built once at creation; `slot` maps a sampler entry to its position), the counts `N` and the
// float32 probabilities `val` per position, `uni` = 1/S for a row no model_update has written yet.
//
// Three kernels:
//   k_ucrl2_walk    lane per instance: acts greedily on the Q of the last solve, steps the environment, counts, appends
//                   (row, reward) to the episode's trace in HBM and PARKS when the artificial episode ends
//                   (ucrl2.py:169-177);
//   k_ucrl2_bounds  workgroup per parked instance: beta_r, beta_p[:, :, 0] (float64, ucrl2.py:240-308) from the counts
//                   INCLUDING the episode and the tables BEFORE its model_update (episode_end_update solves first,
//                   ucrl2.py:179-190), and a snapshot of those tables for the solve;
//   k_ucrl2_update  workgroup per parked instance: takes the solve's Q if it converged, then model_update
//                   (ucrl2.py:213-238) from the trace, and releases the instance.
// The only transcendental of the bounds, math.log(log_C * (iteration + 1) / delta), is one or two scalars per instance
// and solve: the host takes them with std::log (what CPython calls) while it reads the park list.
#pragma once
#include "cmdp_agent.h"

#define UCRL2_THREADS 256

struct UcArgs {
  // layout (constant after creation)
  const int64_t* row_ptr;  // [R + 1]
  const int32_t* col;      // [NZ] instance-relative successor, ascending within a row
  const int32_t* slot;     // [E]  environment entry -> position in col / N / val
  // estimated model
  int32_t* N;              // [NZ] self.N[s, a, s']
  int32_t* N_row;          // [R]  self.N[s, a].sum()
  int32_t* nu;             // [R]  visits of the pair in the open artificial episode
  int32_t* kdone;          // [R]  rewards of the pair model_update has consumed (scratch of k_ucrl2_update, 0 between launches)
  float* val;              // [NZ] self.P[s, a, col]
  float* uni;              // [R]  c when self.P[s, a] is c at every state (1/S before the pair's first model_update), else 0
  float* ER;               // [R]  self.estimated_rewards
  float* VR;               // [R]  self.variance_proxy_reward
  float* HT;               // [R]  self.estimated_holding_times
  int64_t* iteration;      // [B]
  int64_t* episode;        // [B]
  double* delta;           // [B]
  // actor
  float* Q;                // [R]  Q of the last solve that converged
  uint32_t* mt;            // [B][624] numpy RandomState(seed)
  int32_t* mt_pos;
  // trace of the open episode, [tr_cap][B]: element i of instance b at i * B + b
  int32_t* tr_row;         // instance-relative row s * A + a
  double* tr_rew;
  int64_t* tr_len;         // [B]
  int64_t tr_cap;
  ParkCall call;           // state of the call
  int32_t* overflow;       // set when a trace would not fit (cannot happen: the host sizes it from the episode bound)
  // the last solve: its inputs (snapshot) and outputs
  float* sv_val; float* sv_uni; float* sv_R;
  double* beta_r; double* beta_p0;
  float* Qs;               // [R] K10's output
  double* span; int64_t* sweeps; int32_t* status;  // [B]
};

// One round of parked instances: park_list[k] = b; the host's scalars and K10's compact per-launch arrays are indexed by k.
struct UcRound {
  const int32_t* list;
  const double* c_r;       // [count] 3.5 * log(2 S A (iteration + 1) / delta)
  const double* c_p;       // [count] chernoff: 14 S * log(2 A (iteration + 1) / delta); bernstein: log(2.0 S A (iteration + 1) / delta)
  const double* delta;     // [count] 1 / sqrt(iteration + 1)
  int32_t bernstein_p;
  double alpha_r, alpha_p, sqrt_alpha_p, r_max;
  // K10's per-instance arguments for this launch
  int32_t* eS; int32_t* eA; int64_t* e_soff; int64_t* e_roff; double* e_rmax;
  const double* e_span; const int64_t* e_sweeps; const int32_t* e_status;
};

__global__ void __launch_bounds__(256) k_ucrl2_walk(EnvTables t, UcArgs u, int64_t n_steps,
                                                    const uint8_t* __restrict__ train_mask, int8_t* __restrict__ act_trace,
                                                    int32_t* __restrict__ obs_trace, double* __restrict__ rew_trace,
                                                    double* __restrict__ cum_reward) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  long long left = u.call.left[b];
  if (left == 0) return;
  const int64_t soff = t.state_off[b], ebase = t.entry_base[b];
  const int A = t.A;
  const uint2 key = t.philox_key ? t.philox_key[b] : make_uint2(0, 0);
  int32_t cur = t.cur[b], h = t.hstep[b];
  unsigned long long nt = t.n_trans[b];
  const float* Q = u.Q + soff * A;
  int32_t* NR = u.N_row + soff * A;
  int32_t* NU = u.nu + soff * A;
  uint32_t* mt = u.mt + (int64_t)b * 624;
  int32_t* mtp = u.mt_pos + b;
  const bool train = train_mask ? train_mask[b] != 0 : true;
  double sum = cum_reward[b];
  int64_t len = u.tr_len[b];
  bool parked = false;
  while (left > 0) {
    const int64_t step = n_steps - left;
    // loads issued as early as their addresses are known (see k_qlearn_episodic): row descriptors of all actions next to
    // the Q row, the pair's counts right after the action, both MT19937 words of the draw together
    constexpr int AM = 4;
    const bool fastA = A <= AM;
    float qv[AM];
    RowDesc rd[AM];
    int action = 0;
    int32_t obs;
    double reward;
    {  // ---- QValuesActor.select_action: greedy with uniform tie-break ----
      const float* qrow = Q + (int64_t)cur * A;
      if (fastA) {
        const RowDesc* rp = t.row + (soff + cur) * A;
#pragma unroll
        for (int a = 0; a < AM; ++a) {
          qv[a] = (a < A) ? qrow[a] : -INFINITY;
          if (a < A) rd[a] = rp[a];
        }
      }
      float qmax;
      int n_tie = 0;
      if (fastA) {
        qmax = qv[0];
#pragma unroll
        for (int a = 1; a < AM; ++a) qmax = fmaxf(qmax, qv[a]);
#pragma unroll
        for (int a = 0; a < AM; ++a) n_tie += (a < A && qv[a] == qmax) ? 1 : 0;
      } else {
        qmax = qrow[0];
        for (int a = 1; a < A; ++a) qmax = fmaxf(qmax, qrow[a]);
        for (int a = 0; a < A; ++a) n_tie += (qrow[a] == qmax) ? 1 : 0;
      }
      const int pick = n_tie > 1 ? tie_break_draw(n_tie, mt, mtp) : 0;
      if (fastA) {
        int k = 0;
#pragma unroll
        for (int a = 0; a < AM; ++a)
          if (a < A && qv[a] == qmax) { if (k == pick) action = a; ++k; }
      } else {
        for (int a = 0, k = 0; a < A; ++a)
          if (qrow[a] == qmax) { if (k == pick) action = a; ++k; }
      }
    }
    const int32_t idx = cur * A + action;
    int32_t n_pre = 0, nu_pre = 0;   // their loads ride under the transition's round trips
    if (train) { n_pre = NR[idx]; nu_pre = NU[idx]; }
    // ---- BaseMDP.step ----
    const unsigned long long n0 = nt;
    double rraw;
    int64_t e;
    if (fastA) {
      RowDesc dsel = rd[0];
#pragma unroll
      for (int a = 1; a < AM; ++a)
        if (a == action) dsel = rd[a];
      env_transition_desc<true>(t, soff, ebase, key, cur, h, n0, action, obs, rraw, e, dsel);
      ++nt;
    } else {
      env_transition(t, soff, ebase, key, cur, h, nt, action, obs, rraw, e);  // continuous: never terminates
    }
    if (t.sp_rkind && t.sp_rkind[e] == 1) rraw = philox_beta(t.sp_rp0[e], t.sp_rp1[e], n0, key, t.beta_gammas);  // throughput mode only
    reward = rraw * t.rscale - t.rmin;
    sum += reward;
    if (act_trace) act_trace[step * t.B + b] = (int8_t)action;
    if (obs_trace) obs_trace[step * t.B + b] = obs;
    if (rew_trace) rew_trace[step * t.B + b] = reward;
    --left;
    if (train) {
      // ---- step_update (ucrl2.py:195-211) and is_episode_end (:169-177), N already holding this visit ----
      if (len >= u.tr_cap) {  // never: the host sized the trace from the bound on an episode's length
        *u.overflow = 1;
        left = 0;
        break;
      }
      bump(u.N + u.slot[e]);
      const int32_t nrow = n_pre + 1, nuv = nu_pre + 1;
      NR[idx] = nrow;
      NU[idx] = nuv;
      u.tr_row[len * t.B + b] = idx;
      u.tr_rew[len * t.B + b] = reward;
      ++len;
      const int32_t rest = nrow - nuv;
      if (nuv >= (rest > 1 ? rest : 1)) {
        parked = true;
        break;
      }
    }
  }
  t.cur[b] = cur;
  t.hstep[b] = h;
  t.n_trans[b] = nt;
  cum_reward[b] = sum;
  u.call.left[b] = left;
  u.tr_len[b] = len;
  if (parked) u.call.park_list[atomicAdd(u.call.park_count, 1)] = b;
}

// beta_r (ucrl2.py:240-259, Chernoff) and element 0 of beta_p[s, a] (:275-308, the only one extended_value_iteration reads)
// of every pair of a parked instance, plus the snapshot K10 solves on.
__global__ void __launch_bounds__(UCRL2_THREADS) k_ucrl2_bounds(UcArgs u, UcRound g, const int64_t* __restrict__ state_off, int A) {
  const int k = blockIdx.x, tid = threadIdx.x;
  const int b = g.list[k];
  const int64_t soff = state_off[b];
  const int S = (int)(state_off[b + 1] - soff);
  const int64_t r0 = soff * A;
  const int nrows = S * A;
  const double cr = g.c_r[k], cp = g.c_p[k];
  for (int i = tid; i < nrows; i += UCRL2_THREADS) {
    const int64_t r = r0 + i;
    const int32_t n = u.N_row[r];
    const double nmax = (double)(n > 1 ? n : 1);
    // alpha_r * (range * np.sqrt(sqrt_C * log / np.maximum(1, N)))
    u.beta_r[r] = g.alpha_r * (g.r_max * sqrt(cr / nmax));
    double bp;
    if (!g.bernstein_p) {
      bp = g.alpha_p * sqrt(cp / nmax);   // range = 1.0
    } else {
      const int64_t rb = u.row_ptr[r], re = u.row_ptr[r + 1];
      const float c = u.uni[r];
      const float p0 = c > 0.0f ? c : ((re > rb && u.col[rb] == 0) ? u.val[rb] : 0.0f);
      const double nm1 = (double)(n - 1 > 1 ? n - 1 : 1);
      const float var_p = __fmul_rn(p0, __fsub_rn(1.0f, p0));        // float32: self.P * (1.0 - self.P)
      const double scale_a = (double)__fmul_rn(14.0f, var_p) / nmax;  // float32 / int64 -> float64
      const double scale_b = 49.0 / (3.0 * nm1);
      bp = g.sqrt_alpha_p * sqrt(scale_a * cp) + g.alpha_p * (scale_b * cp);
    }
    u.beta_p0[r] = bp;
    u.sv_R[r] = u.ER[r];
    u.sv_uni[r] = u.uni[r];
  }
  const int64_t z0 = u.row_ptr[r0], z1 = u.row_ptr[r0 + nrows];
  for (int64_t z = z0 + tid; z < z1; z += UCRL2_THREADS) u.sv_val[z] = u.val[z];
  if (tid == 0) {
    g.eS[k] = S;
    g.eA[k] = A;
    g.e_soff[k] = soff;
    g.e_roff[k] = r0;
    g.e_rmax[k] = g.r_max;
  }
}

// After the solve: `self.Q` and the span change only when the solve converged (ucrl2.py:348-357); then model_update
// (:213-238).  The per-pair recurrence over the episode's rewards is sequential, pairs are independent: thread
// (row mod 256) owns a pair and keeps its three float32 elements in registers while consecutive trace elements name it;
// numpy's promotion per operation (np.float32 element, np.float64 factor -> float64 operation, float32 store).
__global__ void __launch_bounds__(UCRL2_THREADS) k_ucrl2_update(UcArgs u, UcRound g, const int64_t* __restrict__ state_off, int A,
                                                                int B, int stop, int64_t n_steps, int32_t* __restrict__ unconverged) {
  __shared__ int32_t ch_row[UCRL2_THREADS];
  __shared__ double ch_rew[UCRL2_THREADS];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int b = g.list[k];
  const int64_t soff = state_off[b];
  const int S = (int)(state_off[b + 1] - soff);
  const int64_t r0 = soff * A;
  const int nrows = S * A;
  const bool ok = g.e_status[k] == 0;
  if (ok)
    for (int i = tid; i < nrows; i += UCRL2_THREADS) u.Q[r0 + i] = u.Qs[r0 + i];
  const int64_t len = u.tr_len[b];
  int crow = -1, kd = 0;
  float er = 0.0f, vr = 0.0f, ht = 0.0f;
  long long sf = 0;
  for (int64_t base = 0; base < len; base += UCRL2_THREADS) {
    __syncthreads();
    if (base + tid < len) {
      ch_row[tid] = u.tr_row[(base + tid) * B + b];
      ch_rew[tid] = u.tr_rew[(base + tid) * B + b];
    }
    __syncthreads();
    const int m = (int)((len - base) < UCRL2_THREADS ? (len - base) : UCRL2_THREADS);
    for (int j = 0; j < m; ++j) {
      const int r = ch_row[j];
      if ((r & (UCRL2_THREADS - 1)) != tid) continue;
      if (r != crow) {
        if (crow >= 0) { u.ER[r0 + crow] = er; u.VR[r0 + crow] = vr; u.HT[r0 + crow] = ht; u.kdone[r0 + crow] = kd; }
        crow = r;
        er = u.ER[r0 + r]; vr = u.VR[r0 + r]; ht = u.HT[r0 + r]; kd = u.kdone[r0 + r];
        sf = (long long)u.N_row[r0 + r] + kd;   // scale_f = self.N[s, a].sum(), the episode included
      }
      const double rew = ch_rew[j];
      sf += 1;                                   // before it is used
      ++kd;
      const double x = (double)sf / ((double)sf + 1.0);
      const float old = er;
      er = (float)((double)er * x);
      er = (float)((double)er + rew / ((double)sf + 1.0));
      // the reward is a Python float (BaseMDP.sample_reward pops it from a list): `r - np.float32` is a float32 operation
      vr = __fadd_rn(vr, __fmul_rn(__fsub_rn((float)rew, old), __fsub_rn((float)rew, er)));
      ht = (float)((double)ht * x);
      ht = (float)((double)ht + 1.0 / (double)(sf + 1));
    }
  }
  if (crow >= 0) { u.ER[r0 + crow] = er; u.VR[r0 + crow] = vr; u.HT[r0 + crow] = ht; }
  __syncthreads();
  // self.P[s, a] = self.N[s, a] / self.N[s, a].sum() for the pairs of the episode (int -> float64 -> float32 store)
  for (int i = tid; i < nrows; i += UCRL2_THREADS) {
    const int64_t r = r0 + i;
    if (u.nu[r] == 0) continue;
    const double nsum = (double)u.N_row[r];
    const int64_t rb = u.row_ptr[r], re = u.row_ptr[r + 1];
    float v0 = 0.0f;
    bool same = true;
    for (int64_t z = rb; z < re; ++z) {
      const float v = (float)((double)u.N[z] / nsum);
      u.val[z] = v;
      if (z == rb) v0 = v;
      else same = same && v == v0;
    }
    u.uni[r] = (re - rb == S && same && v0 > 0.0f) ? v0 : 0.0f;   // a full row of one value: K10's uniform form
    u.nu[r] = 0;
    u.kdone[r] = 0;
  }
  if (tid == 0) {
    if (ok) u.span[b] = g.e_span[k];
    else atomicAdd(unconverged, 1);
    u.sweeps[b] = g.e_sweeps[k];
    u.status[b] = g.e_status[k];
    u.iteration[b] += len;   // self.iteration += 1 per reward
    u.episode[b] += 1;
    u.delta[b] = g.delta[k];
    u.tr_len[b] = 0;
    park_release(u.call, b, stop, n_steps);
  }
}
