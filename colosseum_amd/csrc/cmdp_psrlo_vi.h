// cmdp_psrlo_vi.h -- K19: discounted value iteration on the COMPACT optimistic sample (cmdp_psrlo.h), never building
// T_ext [S, A * psi, S].  It is discounted_value_iteration(T_ext, R_ext) of the reference
//   colosseum/dynamic_programming/infinite_horizon.py:14-44
// with T_ext given by the compact sample's expansion (cmdp_psrlo.h: zeros, the layout's values, then z_k) and
// R_ext[s, j] = R[s, j % A] computed, not stored.  Gamma, epsilon, the stop rule, max_sweeps, the outputs (extended Q
// [S][A * psi], V, sweeps, scheme used, status) and the scheme rule are k_vi_discounted_dense's (cmdp_psrlc.h); the rule's
// count of non-zero elements is taken from the compact form and equals (T_ext != 0).sum() of the expansion, so both routes
// pick the same scheme.
//
// The compact sample of one instance (S states, A actions, psi samples, rows = S * A real rows, layout positions
// [ptr[0], ptr[rows]) with nz = ptr[rows] - ptr[0] of them, columns ascending within a row):
//   simple [rows]            1: the row is a SIMPLE row, 0: a POSTERIOR row
//   z      [psi]             the column every simple row's sample k is bumped at (any value when no row is simple)
//   pmk    [psi][nz]         sample-major: float32 value of sample k at layout position e (read for simple rows only)
//   bump   [psi][rows]       sample-major: float32 value of sample k of simple row `row` at column z_k
//   pidx   [rows]            index of a posterior row among the instance's n1 posterior rows, in row order
//   post   [psi][n1][S]      the dense float32 posterior rows, sample-major, as psrlo_host::draw leaves them; the instance's
//                            block starts on a 16-byte boundary
// Expansion (k_psrlo_expand below, Phase 2 of k_psrlo_sample): extended row j = a * psi + k of state s is, for a simple
// row, zero except pmk[k][e] at column col[e] and bump[k][row] at column z_k -- at z_k the bump wins over a layout value --
// and post[k][pidx[row]][:] for a posterior row.
// Non-zero count: per simple (row, k), (bump != 0) + #{e: col[e] != z_k and pmk[k][e] != 0}; per posterior (row, k) the
// non-zeros of its S values.  A z_k inside the layout so counts once.
//
// Arithmetic (one definition for the agent and for cmdp_vi_discounted_optimistic).  V starts at 0.
//   Posterior row  the dense kernel's row sum verbatim (ddv_fetch / ddv_dot of cmdp_psrlc.h): a wavefront owns extended row
//                  (row, k), the same lane-to-column map (16-byte loads when S % 4 == 0), the same xor butterfly.  Its Q
//                  has the bits the dense route gives on the expansion whenever V has.
//   Simple row     lane = sample k of a real row.  The at most len + 1 non-zero positions of the extended row are taken in
//                  ASCENDING COLUMN order (z_k merged into the layout's columns; where z_k is a layout column the value is
//                  the bump, once) and added one at a time in float64 to +0.  Every term is a product of two float32
//                  values and so exact:  double(fl32(gamma * t)) * double(V[c]) under Gauss-Seidel,
//                  double(t) * double(V_old[c]) under Jacobi.  The dense route adds the same terms (and zeros) in another
//                  order, so the two agree within the rounding bound of the float64 sums, not bit for bit.
//   Wrap-up        Gauss-Seidel  Q = float(double(R) + acc), V[s] = max_j Q[s, j] taken at once
//                  Jacobi        Q = R + gamma * float(acc) as two float32 operations without contraction
//   both stop after the sweep with max_s |V_old[s] - V[s]| < epsilon (float32 difference, compared in float64).
// Work split (does not enter the definition): a workgroup of POV_WAVES wavefronts per instance, V and V_old in LDS.  A
// simple real row takes ceil(psi / 64) trips of one wavefront, 64 samples a trip (psi > 64: further trips); a posterior
// real row is psi dense rows dealt to the wavefronts by k.  Gauss-Seidel: per state the wavefront w takes the simple rows
// of actions w, w + POV_WAVES, ...; one barrier per state.  Jacobi: wavefront w takes the states w, w + POV_WAVES, ...; one
// barrier per sweep.  A wavefront loads the descriptor, the first POV_PF layout values of every lane, the bump and z_k of
// its NEXT simple row before it reduces the current one: none of them depends on V, so only the LDS reads of V, the
// float64 chain and the barrier lie between two states.
#pragma once
#include "cmdp_psrlc.h"

#define POV_WAVES 4
#define POV_PF 4   // layout positions of a simple row held in registers ahead of its reduction; the rest is loaded in place

struct PovArgs {
  const int32_t* list;     // block i solves instance list[i]; null: instance i
  const int32_t* S;        // [count]
  const int32_t* A;        // [count] real actions
  const int32_t* psi;      // [count]
  const int64_t* r_off;    // [count] first real row: row_ptr, simple, pidx, R
  const int64_t* s_off;    // [count] first state: V
  const int64_t* q_off;    // [count] first extended row: Q [S][A * psi], bump [psi][rows]
  const int64_t* k_off;    // [count] first of the instance's psi values of z
  const int64_t* pm_off;   // [count] first of the instance's psi * nz values of pmk
  const int64_t* row_ptr;  // ptr[r] indexes col directly
  const int32_t* col;
  const uint8_t* simple;
  const int32_t* pidx;
  const int32_t* n1;       // [count] posterior rows of the instance
  const int32_t* z;
  const float* pmk;
  const float* bump;
  const float* const* post;  // [count] the instance's posterior rows [psi][n1][S], 16-byte aligned; unread when n1 = 0
  const float* R;          // [rows] the real rewards
  float gamma;
  double eps;
  int scheme;
  int64_t size_threshold;
  double density_threshold;
  int64_t max_sweeps;
  float* Q;
  float* V;
  int64_t* sweeps;
  int32_t* scheme_used;
  int32_t* status;
  int desc_rows;           // real rows the launch's LDS has room for behind V and V_old (pov_lds_bytes); 0: none
};

// Dynamic LDS of a launch: k_vi_discounted_dense's (V, V_old, the per-wave words), then -- when the largest instance's real
// rows fit POV_DESC_MAX_BYTES -- every row's flag and range: the sweeps read them from LDS instead of global memory, where a
// flag, then a range, then the values would be three dependent loads on the way from one state to the next
#define POV_DESC_MAX_BYTES (64 * 1024)
inline size_t pov_desc_bytes(int rows) { return ((size_t)rows + 1) * 4 + (((size_t)rows + 15) & ~(size_t)15); }
inline int pov_desc_rows(int max_rows) { return pov_desc_bytes(max_rows) <= POV_DESC_MAX_BYTES ? max_rows : 0; }
__host__ __device__ inline size_t pov_base_bytes(int S) {   // ddv_lds_bytes, rounded up to 16 bytes
  return (((size_t)2 * ((S + 3) & ~3) * sizeof(float) + (size_t)DDV_MAX_WAVES * (4 * sizeof(float) + sizeof(long long))) + 15) & ~(size_t)15;
}
inline size_t pov_lds_bytes(int max_S, int desc_rows) {
  return pov_base_bytes(max_S) + (desc_rows ? pov_desc_bytes(desc_rows) : 0);
}

// A real row's flag and range, from LDS (`lp` set: range relative to the instance's first position) or from global memory
struct PovDesc {
  const uint8_t* sf;
  const int32_t* lp;
  const int64_t* gp;
  int64_t nz0;
  __device__ __forceinline__ bool simple(int row) const { return sf[row] != 0; }
  __device__ __forceinline__ int64_t begin(int row) const { return lp ? nz0 + lp[row] : gp[row]; }
};

// One trip of a simple row in flight: the row's range, and per lane (= sample) what does not depend on V
struct PovRow {
  int64_t rb, re;
  int c[POV_PF];     // the first POV_PF columns (wave-uniform)
  float x[POV_PF];   // ... and the lane's values there
  float bump, r;
  int zk;
};

// The instance's arrays as the lanes index them
struct PovInst {
  PovDesc ptr;             // [rows + 1]
  const int32_t* col;
  const float* pmk;        // pmk[k * nz + e - nz0]: already offset by -nz0
  const float* bump;
  const int32_t* z;
  const float* R;
  int64_t nz;
  int rows, A, psi;
};

__device__ __forceinline__ void pov_fetch(PovRow& d, const PovInst& I, int row, int k) {
  d.rb = I.ptr.begin(row);
  d.re = I.ptr.begin(row + 1);
  const bool on = k < I.psi;
  const float* pk = I.pmk + (int64_t)(on ? k : 0) * I.nz;
#pragma unroll
  for (int i = 0; i < POV_PF; ++i) {
    const int64_t e = d.rb + i;
    d.c[i] = e < d.re ? I.col[e] : 0;
    d.x[i] = on && e < d.re ? pk[e] : 0.0f;
  }
  d.bump = on ? I.bump[(int64_t)k * I.rows + row] : 0.0f;
  d.zk = on ? I.z[k] : 0;
  const int j = (row % I.A) * I.psi + k;   // the extended action; R_ext[s, j] = R[s, j % A]
  d.r = on ? I.R[(row / I.A) * I.A + j % I.A] : 0.0f;
}

// The simple row's sum of the header comment for the lane's sample; `v` in LDS
template <bool GS>
__device__ __forceinline__ double pov_dot(const PovRow& d, const PovInst& I, int k, const float* v, float gamma) {
  double acc = 0.0;
  bool zdone = false;
  const int zk = d.zk;
  const float* pk = I.pmk + (int64_t)k * I.nz;
#pragma unroll
  for (int i = 0; i < POV_PF; ++i) {
    if (d.rb + i < d.re) {
      const int c = d.c[i];
      float x = d.x[i];
      if (!zdone && zk <= c) {
        zdone = true;
        if (zk < c) acc += ddv_term<GS>(d.bump, v[zk], gamma); else x = d.bump;
      }
      acc += ddv_term<GS>(x, v[c], gamma);
    }
  }
  for (int64_t e = d.rb + POV_PF; e < d.re; ++e) {
    const int c = I.col[e];
    float x = pk[e];
    if (!zdone && zk <= c) {
      zdone = true;
      if (zk < c) acc += ddv_term<GS>(d.bump, v[zk], gamma); else x = d.bump;
    }
    acc += ddv_term<GS>(x, v[c], gamma);
  }
  if (!zdone) acc += ddv_term<GS>(d.bump, v[zk], gamma);
  return acc;
}

template <bool GS>
__device__ __forceinline__ float pov_wrap(float r, double acc, float gamma) {
  return GS ? (float)__dadd_rn((double)r, acc) : __fadd_rn(r, __fmul_rn(gamma, (float)acc));
}

// All trips of the simple real row `row`; `d` holds trip 0.  Returns the lane's maximum over its samples.
template <bool GS>
__device__ __forceinline__ float pov_simple_row(PovRow& d, const PovInst& I, int row, int lane, const float* v, float gamma,
                                                float* __restrict__ Q) {
  float m = -INFINITY;
  float* __restrict__ q_row = Q + (int64_t)(row / I.A) * I.A * I.psi + (int64_t)(row % I.A) * I.psi;
  for (int k = lane;; k += 64) {
    if (k < I.psi) {
      const float q = pov_wrap<GS>(d.r, pov_dot<GS>(d, I, k, v, gamma), gamma);
      q_row[k] = q;
      m = fmaxf(m, q);
    }
    if (k - lane + 64 >= I.psi) break;
    pov_fetch(d, I, row, k + 64);
  }
  return m;
}

// Extended row (row, k) of a posterior real row: the dense kernel's row sum and wrap-up
template <bool GS>
__device__ __forceinline__ float pov_posterior(const float* __restrict__ tr, float r, const float* v, int S, int lane, bool vec,
                                               float gamma) {
  DdvRow d;
  ddv_fetch(d, tr, &r, S, lane, vec);
  return pov_wrap<GS>(r, ddv_dot<GS>(d, tr, v, S, lane, vec, gamma), gamma);
}

__global__ void __launch_bounds__(POV_WAVES * 64) k_vi_discounted_optimistic(PovArgs g) {
  static_assert(POV_WAVES <= DDV_MAX_WAVES, "ddv_lds_bytes sizes the per-wave words for DDV_MAX_WAVES");
  extern __shared__ __align__(16) float pov_lds[];
  constexpr int NT = POV_WAVES * 64, WAVES = POV_WAVES;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int b = g.list ? g.list[blockIdx.x] : blockIdx.x;
  const int S = g.S[b], A = g.A[b], psi = g.psi[b];
  const int rows = S * A, AX = A * psi;
  const int spad = (S + 3) & ~3;
  float* V = pov_lds;
  float* W = V + spad;
  float* red = W + spad;
  float* wq = red + 2 * DDV_MAX_WAVES;
  long long* cnt = reinterpret_cast<long long*>(wq + 2 * DDV_MAX_WAVES);
  const int64_t r0 = g.r_off[b];
  const int64_t* __restrict__ ptr = g.row_ptr + r0;
  const int64_t nz0 = ptr[0], nz = ptr[rows] - nz0;
  const int32_t* __restrict__ pidx = g.pidx + r0;
  PovDesc D{g.simple + r0, nullptr, ptr, nz0};
  if (rows <= g.desc_rows) {   // stage the flags and ranges behind the per-wave words
    int32_t* lp = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(pov_lds) + pov_base_bytes(S));
    uint8_t* lf = reinterpret_cast<uint8_t*>(lp + rows + 1);
    for (int i = tid; i <= rows; i += NT) lp[i] = (int32_t)(ptr[i] - nz0);
    for (int i = tid; i < rows; i += NT) lf[i] = g.simple[r0 + i];
    D.sf = lf;
    D.lp = lp;
  }
  __syncthreads();
  const uint8_t* simple = D.sf;   // in LDS when staged
  const int n1 = g.n1[b];
  const float* __restrict__ post = n1 > 0 ? g.post[b] : nullptr;
  const PovInst I{D, g.col, g.pmk + g.pm_off[b] - nz0, g.bump + g.q_off[b], g.z + g.k_off[b], g.R + r0, nz, rows, A, psi};
  float* __restrict__ Q = g.Q + g.q_off[b];
  const float gamma = g.gamma;
  const bool vec = (S & 3) == 0;   // the posterior block is 16-byte aligned and so is every row of it

  int scheme = g.scheme;
  if (scheme == CMDP_SCHEME_AUTO) {   // the count of non-zero elements the expansion would hold
    long long c = 0;
    for (int64_t i = tid; i < (int64_t)rows * psi; i += NT) {
      const int row = (int)(i / psi), k = (int)(i % psi);
      if (!simple[row]) continue;
      const int zk = I.z[k];
      const float* pk = I.pmk + (int64_t)k * nz;
      c += I.bump[(int64_t)k * rows + row] != 0.0f;
      for (int64_t e = ptr[row]; e < ptr[row + 1]; ++e) c += g.col[e] != zk && pk[e] != 0.0f;
    }
    for (int64_t i = tid; i < (int64_t)psi * n1 * S; i += NT) c += post[i] != 0.0f;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) cnt[wid] = c;
    __syncthreads();
    long long nnz = 0;
    for (int w = 0; w < WAVES; ++w) nnz += cnt[w];
    scheme = model_vi_scheme(S, AX, (int64_t)nnz, g.size_threshold, g.density_threshold);
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
      PovRow cur;
      if (wid < S && simple[wid * A]) pov_fetch(cur, I, wid * A, lane);
      for (int s = wid; s < S; s += WAVES) {
        float vmax = -INFINITY;
        for (int a = 0; a < A; ++a) {
          const int row = s * A + a;
          const int nrow = a + 1 < A ? row + 1 : (s + WAVES) * A;   // this wave's next row
          if (simple[row]) {
            // trip 0 of the next row is fetched before this row is reduced only when this row takes one trip: `cur` is
            // the one set of registers of both
            const bool ahead = psi <= 64 && nrow < rows && simple[nrow];
            PovRow nxt;
            if (ahead) pov_fetch(nxt, I, nrow, lane);
            vmax = fmaxf(vmax, pov_simple_row<false>(cur, I, row, lane, Vold, gamma, Q));
            if (ahead) cur = nxt;
            else if (nrow < rows && simple[nrow]) pov_fetch(cur, I, nrow, lane);
          } else {
            for (int k = 0; k < psi; ++k) {
              const int j = a * psi + k;
              const float q = pov_posterior<false>(post + ((int64_t)k * n1 + pidx[row]) * S, I.R[s * A + j % A], Vold, S, lane,
                                                   vec, gamma);
              if (lane == 0) Q[(int64_t)s * AX + j] = q;
              vmax = fmaxf(vmax, q);
            }
            if (nrow < rows && simple[nrow]) pov_fetch(cur, I, nrow, lane);
          }
        }
        vmax = wave_max(vmax);
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
    // this wave's simple rows in the order it meets them: (s, a) for a = wid, wid + WAVES, ... of every state
    auto next_simple = [&](int row) {   // the first simple row of this wave after `row` (rows: none)
      for (;;) {
        const int a = row % A, s = row / A;
        row = a + WAVES < A ? row + WAVES : (s + 1) * A + wid;
        if (wid >= A || row >= rows) return rows;
        if (simple[row]) return row;
      }
    };
    for (;; ++sweep) {
      for (int i = tid; i < S; i += NT) W[i] = V[i];
      __syncthreads();
      PovRow cur;
      int mine = wid < A ? (simple[wid] ? wid : next_simple(wid)) : rows;   // the simple row `cur` holds trip 0 of
      if (mine < rows) pov_fetch(cur, I, mine, lane);
      for (int s = 0; s < S; ++s) {
        float wmax = -INFINITY;
        for (int a = 0; a < A; ++a) {
          const int row = s * A + a;
          if (simple[row]) {
            if (a % WAVES != wid) continue;
            const int nrow = next_simple(row);
            const bool ahead = psi <= 64 && nrow < rows;
            PovRow nxt;
            if (ahead) pov_fetch(nxt, I, nrow, lane);
            wmax = fmaxf(wmax, pov_simple_row<true>(cur, I, row, lane, V, gamma, Q));
            if (ahead) cur = nxt;
            else if (nrow < rows) pov_fetch(cur, I, nrow, lane);
            mine = nrow;
          } else {
            for (int k = wid; k < psi; k += WAVES) {
              const int j = a * psi + k;
              const float q = pov_posterior<true>(post + ((int64_t)k * n1 + pidx[row]) * S, I.R[s * A + j % A], V, S, lane, vec,
                                                  gamma);
              if (lane == 0) Q[(int64_t)s * AX + j] = q;
              wmax = fmaxf(wmax, q);
            }
          }
        }
        wmax = wave_max(wmax);
        float* qb = wq + (s & 1) * DDV_MAX_WAVES;
        if (lane == 0) qb[wid] = wmax;
        __syncthreads();   // every wave has read V for this state; the state's rows are all in qb
        float v = qb[0];
        for (int w = 1; w < WAVES; ++w) v = fmaxf(v, qb[w]);
        if (lane == 0) V[s] = v;   // every wave stores the same V[s] for itself (k_vi_discounted_dense)
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

// The expansion of ONE instance's compact sample into T [S * A * psi][S] (Phase 2's rule of k_psrlo_sample): a wavefront per
// extended row.  `T` holds S * A * psi * S floats.
struct PoxArgs {
  int S, A, psi, n1;
  const int64_t* ptr;      // [rows + 1] the instance's
  const int32_t* col;
  const uint8_t* simple;   // the instance's
  const int32_t* pidx;
  const int32_t* z;
  const float* pmk;        // the instance's, not offset
  const float* bump;
  const float* post;
  float* T;
};

__global__ void __launch_bounds__(256) k_psrlo_expand(PoxArgs g) {
  const int lane = threadIdx.x & 63;
  const int rows = g.S * g.A;
  const int64_t nz0 = g.ptr[0], nz = g.ptr[rows] - nz0;
  const int64_t n_items = (int64_t)rows * g.psi;
  for (int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < n_items; item += (int64_t)gridDim.x * 4) {
    const int row = (int)(item / g.psi), k = (int)(item % g.psi);
    float* __restrict__ dst = g.T + item * g.S;
    if (g.simple[row]) {
      psrlo_write_simple(dst, g.col, g.pmk + (int64_t)k * nz - nz0, g.ptr[row], g.ptr[row + 1], g.z[k],
                         g.bump[(int64_t)k * rows + row], g.S, lane, false);
    } else {
      psrlo_write_posterior(dst, g.post + ((int64_t)k * g.n1 + g.pidx[row]) * g.S, g.S, lane, false);
    }
  }
}
