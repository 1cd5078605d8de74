// cmdp_psrlo.h -- K18: OPTIMISTIC posterior sampling for the continuous setting (Agrawal & Jia), the reference's default path
// (no_optimistic_sampling=False), one reference agent per instance,
//   colosseum/agent/agents/infinite_horizon/posterior_sampling.py   (PSRLContinuous.optimistic_sampling, episode_end_update)
// next to K13's plain path (cmdp_psrlc.h), whose posterior tables, artificial-episode rule, round driver and solver
// (k_vi_discounted_dense with a per-instance A) it shares unchanged.
//
// What the reference does on this path:
//   Scalars (__init__ :268-307), computed by the caller in NumPy and handed over per instance:
//     psi = min(max_psi, max(2, int(psi_weight * S * log(S * A / p)))),  omega = omega_weight * log(T / p),
//     eta = max(5, min(10 * S, eta_weight * (sqrt(T * S / A) + 12 * omega * S^4)));  kappa and self.M are never read.
//   before_start_interacting.  self._rng.randn(S, A * psi) on the AGENT's RandomState(seed) -- a fourth stream next to the
//     actor's and the two conjugate models'; the Q it gives is replaced at once, what stays is the stream's position (legacy
//     polar Gaussians).  Then one episode_end_update.
//   optimistic_sampling (:411-443), per call.  Nsum = N.sum(-1); a row (s, a) is SIMPLE iff Nsum < eta, else POSTERIOR.
//     Posterior rows, row-major, for every k in range(psi): M_DIR.sample_sa(rows) = standard_gamma(hyper_params[rows],
//       (1, n1, S)) on the transitions model's stream, cast to float32, then r / (1e-5 + r.sum(-1, keepdims=True)).
//     Simple rows, in float64:  P_hat = N / maximum(Nsum, 1),  Nm = maximum(N, 1),  l = log(4 S),
//       P_minus = P_hat - minimum(sqrt(((3 * P_hat) * l) / Nm) + (3 * l) / Nm, P_hat)
//       and for every k:  z = agent_rng.randint(S);  summing = 1 - P_minus.sum(-1) (NumPy's pairwise float64 sum of the dense
//       row);  P_minus[:, :, z] += summing;  Q[k, simple rows] = float32(P_minus[simple rows]);  P_minus[:, :, z] -= summing.
//       The += / -= pair is not exact: a layout value may drift, and summing is taken from the restored row at every k.
//     A call with no simple row draws no z; a call with no posterior row draws no gamma.
//   episode_end_update (:360-377).  T_ext = moveaxis(Q, 0, 2).reshape(S, A * psi, S): extended action j = a * psi + k carries
//     sample k of real action a.  R = N_NIG.sample(), R_ext = tile(R, (1, psi)): R_ext[s, j] = R[s, j % A] -- not j / psi; the
//     reference pairs them this way and so does this file.  discounted_value_iteration(T_ext, R_ext): the scheme rule sees the
//     EXTENDED array.
//   select_action.  Greedy on Q[s, :] of length A * psi with the tie-break over all of it; the real action is j / psi.
//   step_update, is_episode_end, current_optimal_stochastic_policy: as on the plain path; the agent's N[s, a, s'] is kept as
//     int32 at the layout's positions (the float32 hyper-parameters cannot give it back).
//
// Kernels:
//   k_psrlc_walk<GATE, true>  (cmdp_psrlc.h) K13's walk on A * psi_b Q values per state (per-instance offsets): it plays and
//     traces j / psi_b and counts N.  It reads psi, Qx, q_off and N of PoArgs and nothing else of it.
//   k_psrlo_sample  one workgroup per listed instance, fills T_ext [S, A * psi, S] and R_ext [S, A * psi].
//     Phase 1, a lane per row: the flag (double)n_sa < eta, P_minus at the row's layout positions, then the serial chain over k.
//       A non-zero of the dense row sits at a layout position or at z_k, so the pairwise sum is mapvi_rowsum itself
//       (cmdp_map_vi.h) on a float64 row with zero fill.  A z_k outside the layout holds 0 + summing and returns to 0 - exactly.
//       Per k the lane leaves float32(P_minus) of its layout positions (`pmk`) and the float32 value at z_k (`bump`).
//     Phase 2, a wavefront per (row, k): the row of T_ext written once, coalesced (16-byte stores where S % 4 == 0): zeros,
//       the layout positions and z_k for a simple row (psrlo_write_simple); the host's compact upload for a posterior row
//       (psrlo_write_posterior).  k_psrlo_expand (cmdp_psrlo_vi.h) writes its rows with the same two functions.
// The COMPACT route (K19, cmdp_psrlo_vi.h; PoArgs::pk set) stops after Phase 1 for the simple rows: the compact sample of an
//   instance is simple [R], z [psi], pmk [psi][nz_b] and bump [psi][S * A] exactly as Phase 1 leaves them (sample-major, the
//   arrangement Phase 2 reads) and, for the n1_b posterior rows of THIS draw, the packed block pk[b] = [psi][n1_b][S]
//   indexed through pidx -- sample-major, the arrangement psrlo_host::draw produces, so the reference sampler's rows are
//   uploaded as drawn.  k_psrlo_count numbers the posterior rows (pidx, n1) before the block is sized.  With the Philox sampler
//   Phase 2 writes each posterior row's variates into the block: the same counters (domain 8, n = episode << 32 | (j * S + c)
//   with j the row of T_ext) and the same normalisation, so the sample stays the same pure function and its expansion is
//   bit for bit the T_ext of the dense route.  T_ext, and R_ext's pairing, are never written to a T_ext-sized array.
// CMDP_PSRL_SAMPLER_REFERENCE: psrlo_host::draw below draws the gammas, the z and the N_NIG sample on the instance's streams.
// CMDP_PSRL_SAMPLER_PHILOX (`post` null): everything is drawn in the kernel, a pure function of (seed, episode, tables):
//   z_k = (w0 * S) >> 32 of the block (n = episode << 32 | k, domain 9);  the gamma variate of element c of extended row
//   j = row * psi + k on domain 8 with n = episode << 32 | (j * S + c) (S * A * psi * S < 2^32 is checked at creation), the
//   row by k_psrl_sample's own psrl_dirichlet_row: float64 sum rounded once, T = r / (1e-5f + sum);  the reward of a row by
//   psrl_nnig_draw (domain 7).  A wavefront keeps its row's variates in its LDS slice (dynamic LDS: 4 * s_max floats).
#pragma once
#include "cmdp_psrlc.h"

#define PSRLO_THREADS 256

// PoArgs, the optimistic agent's device arguments, is defined in cmdp_psrlc.h: the shared walk takes it.

// The compact route's numbering of the posterior rows of the listed instances, a wavefront per instance: pidx[row] = index of
// a posterior row among the instance's posterior rows (-1 for a simple one), n1[b] their number.  The flag is Phase 1's.
__global__ void __launch_bounds__(64) k_psrlo_count(PcCounters c, const double* __restrict__ eta, const int32_t* __restrict__ list,
                                                    const int64_t* __restrict__ state_off, int A, int32_t* __restrict__ pidx,
                                                    int32_t* __restrict__ n1) {
  const int lane = threadIdx.x;
  const int b = list[blockIdx.x];
  const int64_t r0 = state_off[b] * A;
  const int rows = (int)(state_off[b + 1] - state_off[b]) * A;
  const double e = eta[b];
  int run = 0;
  for (int base = 0; base < rows; base += 64) {
    const int row = base + lane;
    const bool post = row < rows && !((double)c.n_sa[r0 + row] < e);
    const unsigned long long m = __ballot(post);
    if (row < rows) pidx[r0 + row] = post ? run + __popcll(m & ((1ull << lane) - 1ull)) : -1;
    run += __popcll(m);
  }
  if (lane == 0) n1[b] = run;
}

// Extended row (row, k) of a SIMPLE row, written by one wavefront: zeros, the float32 layout values `vk` of sample k at the
// columns of [rb, re), and `bump` at z_k, where it wins over a layout value.  `vec`: 16-byte stores (S % 4 == 0, dst aligned).
__device__ __forceinline__ void psrlo_write_simple(float* __restrict__ dst, const int32_t* __restrict__ col,
                                                   const float* __restrict__ vk, int64_t rb, int64_t re, int zk, float bump, int S,
                                                   int lane, bool vec) {
  auto at = [&](int j) {
    if (j == zk) return bump;
    const int64_t m = psrl_layout_find(col, rb, re, j);
    return m >= 0 ? vk[m] : 0.0f;
  };
  if (vec) {
    for (int j = lane * 4; j < S; j += 256) *reinterpret_cast<float4*>(dst + j) = make_float4(at(j), at(j + 1), at(j + 2), at(j + 3));
  } else {
    for (int j = lane; j < S; j += 64) dst[j] = at(j);
  }
}

// ... and of a POSTERIOR row: the dense row `src` as it was drawn, copied
__device__ __forceinline__ void psrlo_write_posterior(float* __restrict__ dst, const float* __restrict__ src, int S, int lane,
                                                      bool vec) {
  if (vec) {
    for (int j = lane * 4; j < S; j += 256) *reinterpret_cast<float4*>(dst + j) = *reinterpret_cast<const float4*>(src + j);
  } else {
    for (int j = lane; j < S; j += 64) dst[j] = src[j];
  }
}

__global__ void __launch_bounds__(PSRLO_THREADS) k_psrlo_sample(PsArgs p, PcCounters c, PoArgs o, const int32_t* __restrict__ list,
                                                                const int64_t* __restrict__ state_off, int A, int s_max) {
  extern __shared__ __align__(16) float po_lds[];
  __shared__ int plan_work[2 * MAPVI_DEPTH + 2];
  __shared__ short plan_run[MAPVI_MAX_RUNS];
  __shared__ signed char plan_merges[MAPVI_MAX_RUNS];
  __shared__ int plan_n;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = list[blockIdx.x];
  const int64_t soff = state_off[b];
  const int S = (int)(state_off[b + 1] - soff);
  const int rows = S * A, psi = o.psi[b];
  const int64_t r0 = soff * A;
  const int64_t* __restrict__ ptr = p.row_ptr + r0;
  const int64_t nz0 = ptr[0], nzb = ptr[rows] - nz0;
  int32_t* __restrict__ z = o.z + o.k_off[b];
  float* __restrict__ pmk = o.pmk + o.pm_off[b];   // [psi][nzb], indexed by layout position - nz0
  float* __restrict__ bump = o.bump + o.q_off[b];  // [psi][rows]
  if (tid == 0) plan_n = mapvi_plan(S, plan_work, plan_run, plan_merges);
  const bool philox = o.pk ? o.pk_from_host == 0 : o.post == nullptr;
  const uint2 key = p.key[b];
  const unsigned long long ep = (unsigned long long)p.episode[b] << 32;
  if (philox) {
    for (int k = tid; k < psi; k += PSRLO_THREADS) {
      uint32_t w[4];
      philox4x32_10((uint32_t)k, (uint32_t)(ep >> 32), 9u, 0u, key.x, key.y, w);
      z[k] = (int32_t)(((unsigned long long)w[0] * (unsigned long long)S) >> 32);
    }
    for (int row = tid; row < rows; row += PSRLO_THREADS)
      p.Rs[r0 + row] = psrl_nnig_draw(p.rp + (r0 + row) * 4, ep | (uint32_t)row, key);
  }
  __syncthreads();   // the plan, and with the Philox sampler the workgroup's z and rewards
  const int n_runs = plan_n;
  const double eta = o.eta[b], l4 = o.log4s[b];
  const double l3 = __dmul_rn(3.0, l4);
  for (int row = tid; row < rows; row += PSRLO_THREADS) {
    const int32_t nsa = c.n_sa[r0 + row];
    const bool simple = (double)nsa < eta;
    o.simple[r0 + row] = simple ? 1 : 0;
    if (!simple) continue;
    const int64_t rb = ptr[row], re = ptr[row + 1];
    const double den = (double)(nsa > 1 ? nsa : 1);
    for (int64_t e = rb; e < re; ++e) {
      const int32_t n = o.N[e];
      const double ph = __ddiv_rn((double)n, den), nm = (double)(n > 1 ? n : 1);
      const double w = __dadd_rn(__dsqrt_rn(__ddiv_rn(__dmul_rn(__dmul_rn(3.0, ph), l4), nm)), __ddiv_rn(l3, nm));
      o.pm[e] = __dsub_rn(ph, w < ph ? w : ph);
    }
    for (int k = 0; k < psi; ++k) {
      const int zk = z[k];
      MapViRow<double> r{p.col, o.pm, rb, re, 0.0};   // a z outside the layout is 0 whenever the row is summed
      const double summing = __dsub_rn(1.0, __dadd_rn(0.0, mapvi_rowsum(r, n_runs, plan_run, plan_merges)));
      int64_t ez = -1;
      for (int64_t e = rb; e < re; ++e)
        if (p.col[e] == zk) ez = e;
      double at_z = __dadd_rn(0.0, summing);
      if (ez >= 0) {
        at_z = __dadd_rn(o.pm[ez], summing);
        o.pm[ez] = at_z;
      }
      float* __restrict__ out = pmk + (int64_t)k * nzb - nz0;
      for (int64_t e = rb; e < re; ++e) out[e] = (float)o.pm[e];
      bump[(int64_t)k * rows + row] = (float)at_z;
      if (ez >= 0) o.pm[ez] = __dsub_rn(at_z, summing);
    }
  }
  // R_ext[s, j] = R[s, j % A]
  const int AX = A * psi;
  float* __restrict__ Rx = o.Rx + o.q_off[b];
  for (int i = tid; i < rows * psi; i += PSRLO_THREADS) Rx[i] = p.Rs[r0 + (int64_t)(i / AX) * A + (i % AX) % A];
  __syncthreads();   // the workgroup's flags, pmk and bump are written
  const bool compact = o.pk != nullptr;
  if (compact && !philox) return;   // the host has uploaded the posterior rows into the instance's block
  float* __restrict__ T = compact ? o.pk[b] : o.Tx + o.tx_off[b];
  const float* __restrict__ post = philox ? nullptr : o.post + o.tx_off[b];
  const int n1 = o.n1[b];
  const float prior = p.tprior[b];
  float* g = po_lds + (size_t)wid * s_max;   // Philox: the wavefront's variates between the draw and the division
  const bool vec = (S & 3) == 0;   // tx_off is a multiple of 4 elements and so is every row's start
  for (int item = wid; item < rows * psi; item += PSRLO_THREADS / 64) {
    const int row = item / psi, k = item % psi;
    const bool is_simple = o.simple[r0 + row] != 0;
    if (compact && is_simple) continue;
    float* __restrict__ dst = compact ? T + ((int64_t)k * n1 + o.pidx[r0 + row]) * S : T + (int64_t)item * S;
    if (is_simple) {
      psrlo_write_simple(dst, p.col, pmk + (int64_t)k * nzb - nz0, ptr[row], ptr[row + 1], z[k], bump[(int64_t)k * rows + row], S,
                         lane, vec);
    } else if (philox) {
      psrl_dirichlet_row<8u>(p.col, p.tp, ptr[row], ptr[row + 1], prior, S, lane, ep, (uint32_t)item * (uint32_t)S, key, g, dst);
    } else {
      psrlo_write_posterior(dst, post + ((int64_t)k * n1 + o.pidx[r0 + row]) * S, S, lane, vec);
    }
  }
}

// ---- host side: the reference's own draws of one optimistic_sampling call ---------------------------------------------------
namespace psrlo_host {

// RandomState.randint(n) for 1 <= n <= 2^32: masked rejection on 32-bit words; n = 1 draws nothing
inline int32_t randint(cmdp_rc::NumpyStream& s, int n) {
  const uint32_t mx = (uint32_t)(n - 1);
  if (mx == 0) return 0;
  uint32_t mask = mx;
  mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
  uint32_t v;
  do { v = s.next_u32() & mask; } while (v > mx);
  return (int32_t)v;
}

// before_start_interacting's randn(S, A * psi) on the agent's stream: only its position matters
inline void skip_randn(cmdp_rc::NumpyStream& s, int64_t n) {
  for (int64_t i = 0; i < n; ++i) (void)s.legacy_gauss();
}

// One optimistic_sampling call and the N_NIG sample that follows it, on the instance's three streams (`ts` M_DIR's, `rs`
// N_NIG's, `as` the agent's).  n_sa [S * A]; (ptr, col, val) the M_DIR hyper-parameters over `prior`, ptr[r] indexing col /
// val directly.  Out: simple [S * A]; pidx [S * A] the index of a posterior row among the posterior rows, -1 for a simple
// one; post [psi][n1][S] the normalised posterior rows; z [psi], -1 where the reference draws none; R [S * A].  Returns n1.
inline int draw(cmdp_rc::NumpyStream& ts, cmdp_rc::NumpyStream& rs, cmdp_rc::NumpyStream& as, int S, int A, int psi, double eta,
                const int32_t* n_sa, const int64_t* ptr, const int32_t* col, const float* val, float prior, const float* rhp,
                uint8_t* simple, int32_t* pidx, float* post, int32_t* z, float* R) {
  const int SA = S * A;
  int n1 = 0;
  for (int r = 0; r < SA; ++r) {
    simple[r] = (double)n_sa[r] < eta ? 1 : 0;
    pidx[r] = simple[r] ? -1 : n1++;
  }
  const int n2 = SA - n1;
  for (int k = 0; k < psi; ++k) {
    for (int r = 0; r < SA; ++r) {
      if (simple[r]) continue;
      float* row = post + ((int64_t)k * n1 + pidx[r]) * S;
      psrl_host::reference_draw_row(ts, S, ptr[r], ptr[r + 1], col, val, prior, row);
    }
    z[k] = n2 > 0 ? randint(as, S) : -1;
  }
  psrl_host::reference_draw_rewards(rs, SA, rhp, R);
  return n1;
}

}  // namespace psrlo_host
