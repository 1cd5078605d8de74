// cmdp_psrl.h -- K12: batched posterior sampling (PSRL) for the episodic setting, one reference agent per instance,
//   colosseum/agent/agents/episodic/posterior_sampling.py      (PSRLEpisodic: sample -> episodic_value_iteration -> Q)
//   colosseum/agent/mdp_models/bayesian_model.py               (BayesianMDPModel.step_update, sample)
//   colosseum/agent/mdp_models/bayesian_models/*.py            (N_NIG rewards, M_DIR transitions)
//   colosseum/experiment/agent_mdp_interaction.py:224-298      (select_action -> step -> step_update -> episode end -> reset)
// with the interaction, the posterior tables, the posterior sample, the solve and the actor's Q on the device.
//
// Model.  N_NIG hyper-parameters (mu, lambda, alpha, beta) float32 per row [R][4]; M_DIR hyper-parameters (prior + counts,
// float32) per position of K11's layout -- per row the DISTINCT successors the environment's row can reach, ascending
// (`row_ptr` / `col`, `slot` maps a sampler entry to its position); every other element of the dense [S, A, S] array
// equals the instance's prior for ever.
//
// Kernels:
//   k_psrl_walk           lane per instance: greedy action on Q[h, s, :] (tie-break stream of RandomState(seed)), the
//                         environment's step, the two model updates, and PARKS at the episode's last step;
//   k_psrl_sample         CMDP_PSRL_SAMPLER_PHILOX: a wavefront per row (s, a) of a parked instance, lanes over columns:
//                         gamma variates on Philox domain 6, the row sum in float64 rounded once, T = r / (1e-5f + sum)
//                         written once, coalesced, into the dense workspace (psrl_dirichlet_row, which K18's sample shares
//                         on domain 8); lane 0 draws the row's reward on domain 7 (psrl_nnig_draw, shared likewise);
//   k_vi_episodic_dense   workgroup per instance: colosseum/dynamic_programming/finite_horizon.py:11-26 on dense float32 T,
//                         V[h + 1] in LDS, a wavefront per state walking its actions, each row T[s, a, :] streamed with
//                         16-byte loads, the dot product accumulated in float64 (exact float32 x float32 products), reduced across the wavefront in a
//                         fixed order and rounded once: Q[h, s, a] = float(double(R[s, a]) + sum);
//   k_psrl_resume         lane per parked instance: the environment's reset(), the episode counter, and the release.
// CMDP_PSRL_SAMPLER_REFERENCE draws on the host instead of k_psrl_sample (psrl_host::reference_draw below: numpy's legacy
// samplers on each instance's two RandomState(seed) streams, glibc's libm, numpy's pairwise float32 sum).
#pragma once
#include "cmdp_agent.h"
#include "cmdp_reward_cache.h"

#define PSRL_SAMPLE_THREADS 256
#define PSRL_VI_THREADS 512
#define PSRL_MAX_STATES 4096

struct PsArgs {
  // layout (constant after creation)
  const int64_t* row_ptr;  // [R + 1]
  const int32_t* col;      // [NZ]
  const int32_t* slot;     // [E]
  // posterior tables
  float* tp;               // [NZ] M_DIR hyper-parameters at the layout's positions
  const float* tprior;     // [B]  ... and everywhere else
  float* rp;               // [R][4] N_NIG hyper-parameters
  int64_t* episode;        // [B] posterior samples drawn so far (the counter of the Philox sampler)
  const uint2* key;        // [B] Philox key of the agent's sampler: (seed, CMDP_PSRL_KEY_HI)
  // the last sample and the actor
  const int64_t* t_off;    // [B] first element of the instance's dense T (a multiple of 4)
  float* T;                // [sum S * A * S, padded]
  float* Rs;               // [R]
  float* Q;                // [(H + 1) * R]: instance b at (H + 1) * state_off[b] * A, [H + 1][S][A]
  float* V;                // [(H + 1) * n_states]
  uint32_t* mt;            // [B][624] numpy RandomState(seed) of the actor
  int32_t* mt_pos;
  ParkCall call;           // state of the call
};

// N_NIG.update_sa for the one-element list [reward] (conjugate_rewards.py:65-82) on the row's (mu, lambda, alpha, beta): n = 1,
// y_bar = np.mean -> float64, np.var of one sample = 0; the unpacked prior values are np.float32 scalars, the results are
// stored as float32.  The walks of K12 and K13 share it.
__device__ __forceinline__ void psrl_nnig_update(float* hp, double reward) {
  const float mu0 = hp[0], l0 = hp[1], a0 = hp[2], b0 = hp[3];
  const float l1 = __fadd_rn(l0, 1.0f);                                       // lambda0 + n
  const double mu1 = ((double)__fmul_rn(l0, mu0) + reward) / (double)l1;      // (lambda0 * mu0 + n * y_bar) / lambda1
  const float a1 = __fadd_rn(a0, 0.5f);                                       // alpha0 + n * 0.5
  const double d = reward - (double)mu0;
  const double pd = __ddiv_rn(__dmul_rn((double)l0, __dmul_rn(d, d)), (double)l1);  // lambda0 * n * (y_bar - mu0)**2 / lambda1
  const double b1 = (double)b0 + 0.5 * pd;                                    // beta0 + 0.5 * (ssq + prior_disc), ssq = 0.0
  hp[0] = (float)mu1; hp[1] = l1; hp[2] = a1; hp[3] = (float)b1;
}

__global__ void __launch_bounds__(256) k_psrl_walk(EnvTables t, PsArgs p, int64_t n_steps, const uint8_t* __restrict__ train_mask,
                                                   int8_t* __restrict__ act_trace, int32_t* __restrict__ obs_trace,
                                                   double* __restrict__ rew_trace, double* __restrict__ cum_reward) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  long long left = p.call.left[b];
  if (left == 0) return;
  const int64_t soff = t.state_off[b], ebase = t.entry_base[b];
  const int S = (int)(t.state_off[b + 1] - soff);
  const int A = t.A, H = t.H;
  const uint2 key = t.philox_key ? t.philox_key[b] : make_uint2(0, 0);
  int32_t cur = t.cur[b], h = t.hstep[b];
  unsigned long long nt = t.n_trans[b], nr = t.n_reset[b];
  const float* Q = p.Q + (int64_t)(H + 1) * soff * A;
  float* RP = p.rp + soff * A * 4;
  uint32_t* mt = p.mt + (int64_t)b * 624;
  int32_t* mtp = p.mt_pos + b;
  const bool train = train_mask ? train_mask[b] != 0 : true;
  double sum = cum_reward[b];
  bool parked = false;
  while (left > 0) {
    const int64_t step = n_steps - left;
    int action = 0;
    {  // ---- QValuesActor.select_action: greedy with uniform tie-break ----
      const float* qrow = Q + ((int64_t)h * S + cur) * A;
      action = greedy_action_row(qrow, A, mt, mtp);
    }
    const int32_t idx = cur * A + action;
    // ---- BaseMDP.step ----
    const unsigned long long n0 = nt;
    int32_t obs;
    double rraw;
    int64_t e;
    const int ty = env_transition(t, soff, ebase, key, cur, h, nt, action, obs, rraw, e);
    if (t.sp_rkind && t.sp_rkind[e] == 1) rraw = philox_beta(t.sp_rp0[e], t.sp_rp1[e], n0, key, t.beta_gammas);  // throughput mode only
    const double reward = rraw * t.rscale - t.rmin;
    sum += reward;
    if (act_trace) act_trace[step * t.B + b] = (int8_t)action;
    if (obs_trace) obs_trace[step * t.B + b] = obs;
    if (rew_trace) rew_trace[step * t.B + b] = reward;
    --left;
    if (train) {
      psrl_nnig_update(RP + (int64_t)idx * 4, reward);
      // ---- M_DIR.update_sa: hyper_params[s, a, s'] += 1 unless the step was the episode's last (bayesian_model.py:90) ----
      if (ty != 2) {
        float* c = p.tp + p.slot[e];
        *c = __fadd_rn(*c, 1.0f);
      }
    }
    if (ty == 2) {
      if (train) {  // is_episode_end: the round samples, solves, installs Q and resets the environment
        parked = true;
        break;
      }
      cur = env_reset(t, b, soff, key, nr);   // a frozen agent (MDPLoop :249-263) acts on: only the environment resets
      h = 0;
    }
  }
  t.cur[b] = cur;
  t.hstep[b] = h;
  t.n_trans[b] = nt;
  t.n_reset[b] = nr;
  cum_reward[b] = sum;
  p.call.left[b] = left;
  if (parked) p.call.park_list[atomicAdd(p.call.park_count, 1)] = b;
}

// The layout position of column j in a row's ascending columns col[rb .. re), or -1: every other element of the dense row holds
// the prior (or, in the optimistic sample's simple rows, zero).  The one lookup of K12, K13 and K18.
__device__ __forceinline__ int64_t psrl_layout_find(const int32_t* __restrict__ col, int64_t rb, int64_t re, int j) {
  int64_t lo = rb, hi = re;
  while (lo < hi) {
    const int64_t m = lo + ((hi - lo) >> 1);
    const int cc = col[m];
    if (cc == j) return m;
    if (cc < j) lo = m + 1; else hi = m;
  }
  return -1;
}

// One row of M_DIR's sample by the Philox sampler, a wavefront per row with its lanes over the columns: the gamma variate of
// column c on Philox domain DOMAIN with n = ep | (base + c), shapes tp at the layout positions [rb, re) over `prior`, cast to
// float32 and kept in the wave's LDS slice `g`; the row sum in float64 rounded once; dst = r / (1e-5f + sum).
template <uint32_t DOMAIN>
__device__ __forceinline__ void psrl_dirichlet_row(const int32_t* __restrict__ col, const float* __restrict__ tp, int64_t rb,
                                                   int64_t re, float prior, int S, int lane, unsigned long long ep, uint32_t base,
                                                   uint2 key, float* g, float* __restrict__ dst) {
  double part = 0.0;
  for (int c = lane; c < S; c += 64) {
    const int64_t m = psrl_layout_find(col, rb, re, c);
    const float shape = m >= 0 ? tp[m] : prior;
    uint32_t draw = 0;
    const float v = (float)philox_gamma((double)shape, ep | (base + (uint32_t)c), key, draw, DOMAIN);
    g[c] = v;
    part += (double)v;
  }
  part = wave_sum(part);
  const float den = __fadd_rn(1e-5f, (float)part);
  for (int c = lane; c < S; c += 64) dst[c] = __fdiv_rn(g[c], den);
}

// N_NIG.sample of one row (conjugate_rewards.py:84-99) by the Philox sampler, domain 7, n = ep | row: tau = gamma(alpha,
// 1 / beta) as float32 (the scale a float32 quotient), var = 1 / (lambda * tau) and its root in float32, mean = normal(mu,
// sqrt(var)) rounded to float32
__device__ __forceinline__ float psrl_nnig_draw(const float* hp, unsigned long long n, uint2 key) {
  uint32_t draw = 0;
  const double ga = philox_gamma((double)hp[2], n, key, draw, 7u);
  const float tau = (float)__dmul_rn((double)__fdiv_rn(1.0f, hp[3]), ga);
  const float sd = __fsqrt_rn(__fdiv_rn(1.0f, __fmul_rn(hp[1], tau)));
  uint32_t w[4];
  philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), 7u, draw, key.x, key.y, w);
  const double z = sqrt(-2.0 * log(1.0 - u53(w[0], w[1]))) * cos(6.283185307179586476925286766559 * u53(w[2], w[3]));
  return (float)__dadd_rn((double)hp[0], __dmul_rn((double)sd, z));
}

// The posterior sample of episode k of the parked instances (Philox sampler; the counter packing is documented in
// cmdp_device.h).  `bpi` = ceil(max rows / 4) blocks per instance: wave `w` of block x takes row 4 (x % bpi) + w of instance
// list[x / bpi].  A lane keeps
// the variates of its own columns (c = lane, lane + 64, ...) in its wave's LDS slice between the draw and the division.
__global__ void __launch_bounds__(PSRL_SAMPLE_THREADS) k_psrl_sample(PsArgs p, const int32_t* __restrict__ list,
                                                                      const int64_t* __restrict__ state_off, int A, int s_max, int bpi) {
  extern __shared__ __align__(16) float ps_lds[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int b = list[blockIdx.x / bpi];
  const int64_t soff = state_off[b];
  const int S = (int)(state_off[b + 1] - soff);
  const int row = (blockIdx.x % bpi) * (PSRL_SAMPLE_THREADS / 64) + wid;
  if (row >= S * A) return;   // wave-uniform; the kernel has no workgroup barrier
  float* g = ps_lds + (size_t)wid * s_max;
  const int64_t r = soff * A + row;
  const int64_t rb = p.row_ptr[r], re = p.row_ptr[r + 1];
  const float prior = p.tprior[b];
  const uint2 key = p.key[b];
  const unsigned long long ep = (unsigned long long)p.episode[b] << 32;
  psrl_dirichlet_row<6u>(p.col, p.tp, rb, re, prior, S, lane, ep, (uint32_t)row * (uint32_t)S, key, g,
                         p.T + p.t_off[b] + (int64_t)row * S);
  if (lane == 0) p.Rs[r] = psrl_nnig_draw(p.rp + r * 4, ep | (uint32_t)row, key);
}

struct DviArgs {
  const int32_t* list;   // block k solves instance list[k]; null: instance k
  const int32_t* S;      // [count]
  const int32_t* A;      // [count]
  const int64_t* t_off;  // [count] first element of T[S, A, S]
  const int64_t* r_off;  // [count] first row: R[S, A]; Q at (H + 1) * r_off
  const int64_t* s_off;  // [count] first state: V at (H + 1) * s_off
  const float* T;
  const float* R;
  float* Q;              // [H + 1][S][A] per instance, layer H zero
  float* V;              // [H + 1][S]
  int H;
};

// Dynamic LDS of a launch whose largest instance has max_S states: the two value layers of k_vi_episodic_dense
inline size_t dense_vi_lds_bytes(int max_S) { return (size_t)2 * ((max_S + 3) & ~3) * sizeof(float); }

__global__ void __launch_bounds__(PSRL_VI_THREADS) k_vi_episodic_dense(DviArgs g) {
  extern __shared__ __align__(16) float dv_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = g.list ? g.list[blockIdx.x] : blockIdx.x;
  const int S = g.S[b], A = g.A[b], H = g.H;
  const int spad = (S + 3) & ~3;
  float* vn = dv_lds;          // V[h + 1]
  float* vc = dv_lds + spad;   // V[h]
  const float* __restrict__ T = g.T + g.t_off[b];
  const float* __restrict__ R = g.R + g.r_off[b];
  float* __restrict__ Q = g.Q + (int64_t)(H + 1) * g.r_off[b];
  float* __restrict__ V = g.V + (int64_t)(H + 1) * g.s_off[b];
  const int nrows = S * A;
  for (int i = tid; i < spad; i += PSRL_VI_THREADS) vn[i] = 0.0f;
  for (int i = tid; i < S; i += PSRL_VI_THREADS) V[(int64_t)H * S + i] = 0.0f;
  for (int i = tid; i < nrows; i += PSRL_VI_THREADS) Q[(int64_t)H * nrows + i] = 0.0f;
  __syncthreads();
  const bool vec = (S & 3) == 0 && (reinterpret_cast<uintptr_t>(T) & 15) == 0;
  for (int h = H - 1; h >= 0; --h) {
    for (int s = wid; s < S; s += PSRL_VI_THREADS / 64) {
      float vmax = -INFINITY;
      for (int a = 0; a < A; ++a) {
        const int row = s * A + a;
        const float* __restrict__ tr = T + (int64_t)row * S;
        double acc = 0.0;   // float32 x float32 products are exact in float64: fused or not, the same sum
        if (vec) {
          for (int c = lane * 4; c < S; c += 256) {
            const float4 x = *reinterpret_cast<const float4*>(tr + c);
            const float4 v = *reinterpret_cast<const float4*>(vn + c);
            acc += (double)x.x * (double)v.x;
            acc += (double)x.y * (double)v.y;
            acc += (double)x.z * (double)v.z;
            acc += (double)x.w * (double)v.w;
          }
        } else {
          for (int c = lane; c < S; c += 64) acc += (double)tr[c] * (double)vn[c];
        }
        acc = wave_sum(acc);
        const float q = (float)__dadd_rn((double)R[row], acc);
        if (lane == 0) Q[(int64_t)h * nrows + row] = q;
        vmax = fmaxf(vmax, q);
      }
      if (lane == 0) {
        vc[s] = vmax;
        V[(int64_t)h * S + s] = vmax;
      }
    }
    __syncthreads();
    float* x = vn; vn = vc; vc = x;
  }
}

// After the solve: the environment's reset() (agent_mdp_interaction.py:295-297; not at creation, where
// before_start_interacting follows the caller's reset), the sample counter, and the release of the instance.
__global__ void __launch_bounds__(256) k_psrl_resume(EnvTables t, PsArgs p, const int32_t* __restrict__ list, int count,
                                                     int do_reset, int stop, int64_t n_steps) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const int b = list[k];
  if (do_reset) {
    unsigned long long nr = t.n_reset[b];
    const int32_t s = env_reset(t, b, t.state_off[b], t.philox_key ? t.philox_key[b] : make_uint2(0, 0), nr);
    t.n_reset[b] = nr;
    t.cur[b] = s;
    t.hstep[b] = 0;
    t.need_reset[b] = 0;
  }
  p.episode[b] += 1;
  park_release(p.call, b, stop, n_steps);
}

// ---- host side: the reference's own posterior sample ----------------------------------------------------------------
namespace psrl_host {

// numpy's pairwise summation of a contiguous float32 run (numpy/core/src/umath/loops_utils.h.src, FLOAT_pairwise_sum)
inline float pairwise_sum_f32(const float* a, int64_t n) {
  if (n < 8) {
    float res = 0.0f;
    for (int64_t i = 0; i < n; ++i) res += a[i];
    return res;
  }
  if (n <= 128) {
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int64_t i;
    for (i = 8; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  int64_t n2 = n / 2;
  n2 -= n2 % 8;
  return pairwise_sum_f32(a, n2) + pairwise_sum_f32(a + n2, n - n2);
}

// One row of M_DIR's sample from the layout positions [z, ze) over `prior`; K18's posterior rows are drawn with it too
inline void reference_draw_row(cmdp_rc::NumpyStream& ts, int S, int64_t z, int64_t ze, const int32_t* col, const float* val,
                               float prior, float* row) {
  for (int c = 0; c < S; ++c) {
    float shape = prior;
    if (z < ze && col[z] == c) shape = val[z++];
    row[c] = (float)ts.standard_gamma((double)shape);
  }
  const float den = 1e-5f + (0.0f + pairwise_sum_f32(row, S));   // 1e-5 + r.sum(-1, keepdims=True), float32
  for (int c = 0; c < S; ++c) row[c] = row[c] / den;
}

// N_NIG.sample of SA rows (conjugate_rewards.py:84-99)
inline void reference_draw_rewards(cmdp_rc::NumpyStream& rs, int SA, const float* rhp, float* R) {
  // tau = rng.gamma(shape=alpha, scale=1.0 / beta).astype(float32): every gamma first, then every normal
  std::vector<float> tau((size_t)SA);
  for (int r = 0; r < SA; ++r) {
    const float scale = 1.0f / rhp[4 * r + 3];
    tau[(size_t)r] = (float)((double)scale * rs.standard_gamma((double)rhp[4 * r + 2]));
  }
  for (int r = 0; r < SA; ++r) {
    const float var = 1.0f / (rhp[4 * r + 1] * tau[(size_t)r]);
    const float sd = std::sqrt(var);
    R[r] = (float)((double)rhp[4 * r] + (double)sd * rs.legacy_gauss());
  }
}

// M_DIR.sample and N_NIG.sample of one instance (conjugate_transitions.py:48-60, conjugate_rewards.py:84-99) on its two
// RandomState streams.  Transition hyper-parameters: `dense` [S * A * S], or (ptr, col, val) over `prior` when null
// (ptr relative to the instance's first row is NOT assumed: ptr[r] indexes col / val directly).
inline void reference_draw(cmdp_rc::NumpyStream& ts, cmdp_rc::NumpyStream& rs, int S, int A, const float* dense,
                           const int64_t* ptr, const int32_t* col, const float* val, float prior, const float* rhp,
                           float* T, float* R) {
  const int SA = S * A;
  for (int r = 0; r < SA; ++r) {
    float* row = T + (int64_t)r * S;
    if (dense) {
      for (int c = 0; c < S; ++c) row[c] = (float)ts.standard_gamma((double)dense[(int64_t)r * S + c]);
      const float den = 1e-5f + (0.0f + pairwise_sum_f32(row, S));
      for (int c = 0; c < S; ++c) row[c] = row[c] / den;
    } else {
      reference_draw_row(ts, S, ptr[r], ptr[r + 1], col, val, prior, row);
    }
  }
  reference_draw_rewards(rs, SA, rhp, R);
}

inline void seed_numpy(cmdp_rc::NumpyStream& s, uint32_t seed) {  // RandomState(seed): init_genrand, position 624
  s.key[0] = seed;
  for (int k = 1; k < 624; ++k) s.key[k] = 1812433253u * (s.key[k - 1] ^ (s.key[k - 1] >> 30)) + (uint32_t)k;
  s.pos = 624;
  s.has_gauss = 0;
  s.gauss = 0.0;
  s.out_valid = false;
}

}  // namespace psrl_host
