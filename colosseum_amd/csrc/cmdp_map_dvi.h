// cmdp_map_dvi.h -- K17 k_vi_discounted_map: discounted value iteration (colosseum/dynamic_programming/infinite_horizon.py:
// 14-44) on the MAP estimate of a Bayesian model, straight from the model's tables in K11 / K12's layout.  What
// PSRLContinuous.current_optimal_stochastic_policy solves (infinite_horizon/posterior_sampling.py:174-178), without the
// dense [S, A, S] array that k_psrlc_map_fill writes and k_vi_discounted_dense sweeps (cmdp_psrlc.h).
//
// THE DEFINITION.  The input is K15's table form (cmdp_map_vi.h): per row r = (s, a) the ascending instance-relative columns
// col[e] hold hp[e] for e in row_ptr[r] .. row_ptr[r + 1], `prior` stands at every other state, mu[r] is the reward MAP.
//   prologue, K15's (mapvi_plan / mapvi_rowsum), once per solve and row:
//     rowsum = numpy's pairwise float32 sum of the dense row in column order
//     c      = prior / rowsum          every element of T_map outside the layout
//     t[e]   = hp[e] / rowsum          T_map[s, a, col[e]]       -- float32 divisions: the bits of cmdp_psrl_map_rows, and so
//                                                                   of the array k_psrlc_map_fill writes
// The solver's arithmetic is k_vi_discounted_dense's with the prior's share factored out.  V starts at 0; every float64
// operation is rounded on its own (no contraction); the two sums over e run in layout order from +0; len = the row's number
// of layout positions.  SV(X) is the float64 sum of X[0 .. S): 64 partial sums, partial l adding double(X[l]), double(X[l + 64]),
// ... in ascending order to +0, combined by the xor butterfly 32, 16, 8, 4, 2, 1 (wave_sum; K15's order).
//   Gauss-Seidel  per row, once: gt[e] = fl32(gamma * t[e]), gc = fl32(gamma * c)
//                 per sweep: SV = SV(V), taken afresh, so nothing drifts from sweep to sweep; then per state s in order
//                   per action:  sub = sum_e double(V[col e]);  dot = sum_e double(gt[e]) * double(V[col e])
//                                Q[s, a] = float(double(mu) + (double(gc) * (SV - sub) + dot))
//                   V_new = max_a Q[s, a];  SV = SV + (double(V_new) - double(V[s]));  V[s] = V_new, taken at once
//   Jacobi        per sweep: SV = SV(V_old); per state and action
//                   tv = float(double(c) * (SV - sub) + sum_e double(t[e]) * double(V_old[col e])), sub over V_old
//                   Q[s, a] = R + gamma * tv as two float32 operations;  V[s] = max_a Q[s, a]
//   a row whose layout covers all S columns (len == S) leaves the gc / c term out: Q = float(double(mu) + dot), tv = float(dot)
//   both stop after the sweep with max_s |V_old[s] - V[s]| < epsilon (float32 difference, compared in float64); at
//   max_sweeps the status is CMDP_ERR_MAX_ITER and Q, V are the last sweep's.
//   CMDP_SCHEME_AUTO is model_vi_scheme on nnz = the layout positions with t[e] != 0 plus S - len for every row with c != 0:
//   the count k_vi_discounted_dense takes on the dense MAP array, so scheme_used equals the dense route's.
// How lanes and wavefronts are assigned does not enter the definition.
//
// THE KERNEL.  One wavefront per instance, V (and V_old) in LDS, every instance of a launch to convergence or to max_sweeps
// without a host round trip.  Gauss-Seidel is a dependent chain from state to state; nothing of a row depends on V, so the
// descriptors run ahead of the chain in two stages: the row bounds of state s + 2 and, with the bounds fetched one state
// earlier, mu, c, V[s + 1] and the first MAPDVI_PF (column, t) pairs of state s + 1 are loaded while state s is reduced, and
// are first touched (the products with gamma) after it.  None of these loads stands behind a branch.
// Lane = action of the current state (actions beyond 64 and layout positions beyond MAPDVI_PF are walked in place by their
// lane).  A pair a row does not have is (column S, 0): V[S] is a word that stays +0, and adding +0 to a sum that started at
// +0 changes no bit, so the MAPDVI_PF reads of V need no branch.  On the chain: those LDS reads, the two short sums, the max
// over the actions (DPP moves within the lanes that hold actions, then one readlane) and the SV update, which every lane
// does for itself on the wave-uniform V_new.  The lane that stores V[s] and the lanes that read it next belong to one
// wavefront, whose LDS operations execute in order: no barrier.
// Jacobi: lane = state, actions and layout positions in order, one barrier per sweep.
// An instance whose row bounds, c, mu, t and col fit next to the value arrays in what the launch was given
// (map_dvi_stage_bytes) keeps them in LDS; a larger one reads them from global memory through the same code.
#pragma once
#include <type_traits>

#include "cmdp_model_vi.h"
#include "cmdp_map_vi.h"

#define MAPDVI_THREADS 64
#define MAPDVI_PF 4   // layout positions of a row held in registers one state ahead

struct MapDviArgs {
  const int32_t* list;     // block k solves instance list[k]; null: instance k
  const int32_t* S;        // [count]
  const int32_t* A;        // [count]
  const int64_t* r_off;    // [count] first row: row_ptr, c, mu, Q
  const int64_t* s_off;    // [count] first state: V
  const int64_t* row_ptr;  // [n_rows + 1] into col / hp / t
  const int32_t* col;      // instance-relative, ascending within a row
  const float* hp;         // M_DIR hyper-parameters at the layout's positions
  const float* prior;      // [count] ... and everywhere else
  const float* mu;         // reward MAP of row r at mu[r * mu_stride] (4: the N_NIG table itself)
  int mu_stride;
  float* t;                // [NZ] out: T_map at the layout's positions
  float* c;                // [n_rows] out: T_map elsewhere
  float gamma;
  double eps;
  int scheme;              // CMDP_SCHEME_AUTO: model_vi_scheme per instance
  int64_t size_threshold;
  double density_threshold;
  int64_t max_sweeps;
  float* Q;                // [n_rows]
  float* V;                // [n_states]
  int64_t* sweeps;         // [count]
  int32_t* scheme_used;    // [count]
  int32_t* status;         // [count] 0 or CMDP_ERR_MAX_ITER
  unsigned lds_bytes;      // dynamic LDS of the launch
};

// LDS of one instance: two value arrays of S words and the zero word V[S], and -- staged -- its row bounds (relative to the
// instance's first position), c, mu, t and col
__host__ __device__ inline int map_dvi_vpad(int S) { return (S + 4) & ~3; }
__host__ __device__ inline size_t map_dvi_value_bytes(int S) { return (size_t)2 * map_dvi_vpad(S) * sizeof(float); }
__host__ __device__ inline size_t map_dvi_stage_bytes(int S, int A, int64_t nz) {
  const size_t rows = (size_t)S * A;
  return map_dvi_value_bytes(S) + 4 * (rows + 1) + 8 * rows + 8 * (size_t)nz;
}
// what a launch asks for: every instance's value arrays, and the tables of every instance that stays under `stage_max`
inline size_t map_dvi_lds_bytes(int S, int A, int64_t nz, size_t stage_max) {
  const size_t full = map_dvi_stage_bytes(S, A, nz);
  return full <= stage_max ? full : map_dvi_value_bytes(S);
}

// SV of the header comment; every lane receives the same bits
__device__ __forceinline__ double mapdvi_sv(const float* v, int S, int lane) {
  double sv = 0.0;
  for (int j = lane; j < S; j += 64) sv = __dadd_rn(sv, (double)v[j]);
  return wave_sum(sv);
}

// max over the lanes 0 .. min(A, 64) - 1 (the others hold -inf), wave-uniform.  DPP moves: quad_perm [1,0,3,2], [2,3,0,1],
// row_ror:4, row_ror:8, row_bcast:15, row_bcast:31, as far as A needs them; called by the whole wavefront.
__device__ __forceinline__ float mapdvi_action_max(float q, int A) {
  int x = __float_as_int(q);
#define MAPDVI_DPP_MAX(ctrl) \
  x = __float_as_int(fmaxf(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(x, x, ctrl, 0xf, 0xf, false))))
  MAPDVI_DPP_MAX(0xb1);
  MAPDVI_DPP_MAX(0x4e);
  if (A > 4) {
    MAPDVI_DPP_MAX(0x124);
    MAPDVI_DPP_MAX(0x128);
  }
  if (A > 16) {
    MAPDVI_DPP_MAX(0x142);
    MAPDVI_DPP_MAX(0x143);
    return __int_as_float(__builtin_amdgcn_readlane(x, 63));
  }
#undef MAPDVI_DPP_MAX
  return __int_as_float(__builtin_amdgcn_readlane(x, 0));
}

// The tables of one instance, in LDS (STAGED: bounds relative to the instance's first position) or in global memory
// (bounds as the caller's row_ptr, col and t from the batch's first position)
template <bool STAGED>
struct MapDviTab {
  using Off = typename std::conditional<STAGED, int32_t, int64_t>::type;
  const Off* ptr;      // [rows + 1]
  const int32_t* col;
  const float* t;
  const float* c;      // [rows]
  const float* mu;     // row r at mu[r * mus]
  int mus;
};

// One row in place: sub and dot of the definition over the positions lo .. hi, in layout order from +0
template <bool GS, typename Off>
__device__ __forceinline__ void mapdvi_sums(const int32_t* col, const float* t, Off lo, Off hi, const float* v, float gamma,
                                            double& sub, double& dot) {
  for (Off e = lo; e < hi; ++e) {
    const double x = (double)v[col[e]];
    const float w = GS ? __fmul_rn(gamma, t[e]) : t[e];
    sub = __dadd_rn(sub, x);
    dot = __dadd_rn(dot, __dmul_rn((double)w, x));
  }
}

// double(k) * (SV - sub) + dot, or dot alone for a row whose layout covers every column
__device__ __forceinline__ double mapdvi_inner(float k, double sv, double sub, double dot, bool full) {
  return full ? dot : __dadd_rn(__dmul_rn((double)k, __dsub_rn(sv, sub)), dot);
}

template <bool STAGED>
__device__ __forceinline__ void mapdvi_solve(const MapDviArgs& g, const MapDviTab<STAGED> tb, int S, int A, int scheme, float* V,
                                             float* W, float* __restrict__ Q, int lane, float*& Vout, int64_t& sweep, bool& done) {
  using Off = typename MapDviTab<STAGED>::Off;
  const float gamma = g.gamma;
  Vout = V;
  sweep = 1;
  done = false;
  if (scheme == CMDP_SCHEME_JACOBI) {
    float* Vold = V;
    float* Vnew = W;
    for (;; ++sweep) {
      const double sv = mapdvi_sv(Vold, S, lane);
      float d = 0.0f;
      for (int s = lane; s < S; s += MAPDVI_THREADS) {
        float vmax = -INFINITY;
        for (int a = 0; a < A; ++a) {
          const int r = s * A + a;
          const Off lo = tb.ptr[r], hi = tb.ptr[r + 1];
          double sub = 0.0, dot = 0.0;
          mapdvi_sums<false, Off>(tb.col, tb.t, lo, hi, Vold, gamma, sub, dot);
          const float tv = (float)mapdvi_inner(tb.c[r], sv, sub, dot, hi - lo == (Off)S);
          const float q = __fadd_rn(tb.mu[(int64_t)r * tb.mus], __fmul_rn(gamma, tv));
          Q[r] = q;
          vmax = fmaxf(vmax, q);
        }
        Vnew[s] = vmax;
        d = fmaxf(d, fabsf(__fsub_rn(Vold[s], vmax)));
      }
      d = wave_max(d);
      __syncthreads();   // Vnew is whole, and every lane has read Vold
      float* x = Vold; Vold = Vnew; Vnew = x;
      done = (double)d < g.eps;
      if (done || sweep >= g.max_sweeps) break;
    }
    Vout = Vold;
    return;
  }
  // Every lane walks a row: lane l < A its own action, the others the last action's again (the same words, nothing stored),
  // and the states past the last are the last again, so that no load of the pipeline stands behind a branch -- a load
  // behind one is waited for where it is issued, and then it is no prefetch.
  const bool active = lane < A;
  const int la = active ? lane : A - 1;
  const int rows = S * A;
  const Off end = tb.ptr[rows];
  const bool any = end > tb.ptr[0];   // wave-uniform: the instance has layout positions at all
  const Off last = end - 1;
  for (;; ++sweep) {
    double sv = mapdvi_sv(V, S, lane);
    float dmax = 0.0f;
    // the pipeline's registers: state s (_c: ready for the chain), state s + 1 (_b: its bounds), state s + 2 (_n: loads in flight)
    const int r1 = (S > 1 ? A : 0) + la;
    Off lo_c = tb.ptr[la], hi_c = tb.ptr[la + 1], lo_b = tb.ptr[r1], hi_b = tb.ptr[r1 + 1];
    float mu_c = tb.mu[(int64_t)la * tb.mus], gc_c = __fmul_rn(gamma, tb.c[la]), old_c = V[0];
    int col_c[MAPDVI_PF];
    float gt_c[MAPDVI_PF];
#pragma unroll
    for (int k = 0; k < MAPDVI_PF; ++k) {
      col_c[k] = S;
      gt_c[k] = 0.0f;
      if (lo_c + k < hi_c) { col_c[k] = tb.col[lo_c + k]; gt_c[k] = __fmul_rn(gamma, tb.t[lo_c + k]); }
    }
    for (int s = 0; s < S; ++s) {
      // stage 1: the bounds of state s + 2
      const int rn2 = (s + 2 < S ? s + 2 : S - 1) * A + la;
      const Off lo_n = tb.ptr[rn2], hi_n = tb.ptr[rn2 + 1];
      // stage 2: state s + 1 from the bounds fetched one state ago; positions the row does not have read the instance's
      // last position instead and are replaced after the chain
      const int sn = s + 1 < S ? s + 1 : S - 1;
      const int rn1 = sn * A + la;
      const float mu_n = tb.mu[(int64_t)rn1 * tb.mus], c_n = tb.c[rn1];
      const float old_n = V[sn];   // state s writes V[s] alone
      int col_n[MAPDVI_PF];
      float t_n[MAPDVI_PF];
#pragma unroll
      for (int k = 0; k < MAPDVI_PF; ++k) {
        col_n[k] = S;
        t_n[k] = 0.0f;
        if (any) {
          const Off e = lo_b + k < last ? lo_b + k : last;
          col_n[k] = tb.col[e];
          t_n[k] = tb.t[e];
        }
      }
      // the chain: state s
      double sub = 0.0, dot = 0.0;
#pragma unroll
      for (int k = 0; k < MAPDVI_PF; ++k) {
        const double x = (double)V[col_c[k]];
        sub = __dadd_rn(sub, x);
        dot = __dadd_rn(dot, __dmul_rn((double)gt_c[k], x));
      }
      if (hi_c - lo_c > MAPDVI_PF) mapdvi_sums<true, Off>(tb.col, tb.t, lo_c + MAPDVI_PF, hi_c, V, gamma, sub, dot);
      float q = (float)__dadd_rn((double)mu_c, mapdvi_inner(gc_c, sv, sub, dot, hi_c - lo_c == (Off)S));
      if (active) Q[s * A + lane] = q;
      for (int a = lane + MAPDVI_THREADS; a < A; a += MAPDVI_THREADS) {   // more actions than lanes: in place
        const int r = s * A + a;
        const Off lo = tb.ptr[r], hi = tb.ptr[r + 1];
        double sub2 = 0.0, dot2 = 0.0;
        mapdvi_sums<true, Off>(tb.col, tb.t, lo, hi, V, gamma, sub2, dot2);
        const float q2 = (float)__dadd_rn((double)tb.mu[(int64_t)r * tb.mus],
                                          mapdvi_inner(__fmul_rn(gamma, tb.c[r]), sv, sub2, dot2, hi - lo == (Off)S));
        Q[r] = q2;
        q = fmaxf(q, q2);
      }
      const float v = mapdvi_action_max(active ? q : -INFINITY, A);
      sv = __dadd_rn(sv, __dsub_rn((double)v, (double)old_c));
      if (lane == 0) V[s] = v;
      dmax = fmaxf(dmax, fabsf(__fsub_rn(old_c, v)));
      __builtin_amdgcn_sched_barrier(0);   // what follows consumes the loads of stage 2: after the chain, not before it
      lo_c = lo_b; hi_c = hi_b; lo_b = lo_n; hi_b = hi_n;
      mu_c = mu_n; gc_c = __fmul_rn(gamma, c_n); old_c = old_n;
#pragma unroll
      for (int k = 0; k < MAPDVI_PF; ++k) {
        const bool has = lo_c + k < hi_c;
        col_c[k] = has ? col_n[k] : S;
        gt_c[k] = has ? __fmul_rn(gamma, t_n[k]) : 0.0f;
      }
    }
    done = (double)dmax < g.eps;
    if (done || sweep >= g.max_sweeps) break;
  }
}

__global__ void __launch_bounds__(MAPDVI_THREADS) k_vi_discounted_map(MapDviArgs g) {
  extern __shared__ __align__(16) float mapdvi_lds[];
  __shared__ int plan_work[2 * MAPVI_DEPTH + 2];
  __shared__ short plan_run[MAPVI_MAX_RUNS];
  __shared__ signed char plan_merges[MAPVI_MAX_RUNS];
  __shared__ int plan_n;
  const int lane = threadIdx.x;
  const int b = g.list ? g.list[blockIdx.x] : blockIdx.x;
  const int S = g.S[b], A = g.A[b];
  const int vpad = map_dvi_vpad(S);
  const int rows = S * A;
  float* V = mapdvi_lds;
  float* W = mapdvi_lds + vpad;
  const int64_t r0 = g.r_off[b];
  const int64_t* __restrict__ ptr = g.row_ptr + r0;
  const float prior = g.prior[b];
  float* cmap = g.c + r0;
  const float* mu = g.mu + r0 * g.mu_stride;

  if (lane == 0) plan_n = mapvi_plan(S, plan_work, plan_run, plan_merges);
  __syncthreads();
  const int n_runs = plan_n;
  const int64_t z0 = ptr[0], nz = ptr[rows] - z0;
  const bool staged = map_dvi_stage_bytes(S, A, nz) <= (size_t)g.lds_bytes;
  int32_t* lptr = reinterpret_cast<int32_t*>(mapdvi_lds + 2 * vpad);   // [rows + 1]
  float* lc = reinterpret_cast<float*>(lptr + rows + 1);                // [rows]
  float* lmu = lc + rows;                                               // [rows]
  float* lt = lmu + rows;                                               // [nz]
  int32_t* lcol = reinterpret_cast<int32_t*>(lt + nz);                  // [nz]
  if (staged && lane == 0) lptr[rows] = (int32_t)nz;
  // K15's prologue, a lane per row, and the rule's count of non-zero elements
  long long nnz = 0;
  for (int row = lane; row < rows; row += MAPDVI_THREADS) {
    const int64_t zb = ptr[row], ze = ptr[row + 1];
    MapViRow<float> r{g.col, g.hp, zb, ze, prior};
    const float rowsum = mapvi_rowsum(r, n_runs, plan_run, plan_merges);
    const float c = __fdiv_rn(prior, rowsum);
    cmap[row] = c;
    if (c != 0.0f) nnz += S - (ze - zb);
    if (staged) {
      lptr[row] = (int32_t)(zb - z0);
      lc[row] = c;
      lmu[row] = mu[(int64_t)row * g.mu_stride];
    }
    for (int64_t e = zb; e < ze; ++e) {
      const float t = __fdiv_rn(g.hp[e], rowsum);
      g.t[e] = t;
      nnz += t != 0.0f ? 1 : 0;
      if (staged) {
        lt[e - z0] = t;
        lcol[e - z0] = g.col[e];
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) nnz += __shfl_xor(nnz, o, 64);
  const int scheme = g.scheme == CMDP_SCHEME_AUTO ? model_vi_scheme(S, A, (int64_t)nnz, g.size_threshold, g.density_threshold) : g.scheme;
  for (int i = lane; i < 2 * vpad; i += MAPDVI_THREADS) mapdvi_lds[i] = 0.0f;
  __syncthreads();   // the instance's t and c are written: the solve reads them

  float* Vout;
  int64_t sweep;
  bool done;
  float* __restrict__ Q = g.Q + r0;
  if (staged) {
    const MapDviTab<true> tb{lptr, lcol, lt, lc, lmu, 1};
    mapdvi_solve<true>(g, tb, S, A, scheme, V, W, Q, lane, Vout, sweep, done);
  } else {
    const MapDviTab<false> tb{ptr, g.col, g.t, cmap, mu, g.mu_stride};
    mapdvi_solve<false>(g, tb, S, A, scheme, V, W, Q, lane, Vout, sweep, done);
  }
  float* __restrict__ Vg = g.V + g.s_off[b];
  for (int i = lane; i < S; i += MAPDVI_THREADS) Vg[i] = Vout[i];
  if (lane == 0) {
    g.sweeps[b] = sweep;
    g.scheme_used[b] = scheme;
    g.status[b] = done ? 0 : CMDP_ERR_MAX_ITER;
  }
}
