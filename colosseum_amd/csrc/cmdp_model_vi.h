// cmdp_model_vi.h -- K14 k_vi_model: discounted value iteration (colosseum/dynamic_programming/infinite_horizon.py:14-44,
// 121-164) on models in K10's row form, every instance of a launch to convergence or to max_sweeps without a host round trip.
// What UCRL2Continuous.current_optimal_stochastic_policy solves (ucrl2.py:80-83), straight from the agent's device tables.
// A launch solves the instances of `list`, one workgroup each, as the other batch solvers select theirs (null: all of them).
//
// A row (s, a) is either UNIFORM -- uni[r] = c > 0: T[s, a, j] = c at every state j, its CSR entries (if any) are not read --
// or the CSR row ptr[r] .. ptr[r + 1] with ascending columns.  By this kernel's definition, with every product and every sum
// a separate float32 operation rounded to nearest (no contraction) and every row sum taken one product at a time in column
// order from the accumulator +0:
//   Jacobi        tv = sum_j T[s, a, j] * Vold[j];                Q[s, a] = R[s, a] + gamma * tv;  V[s] = max_a Q[s, a]
//   Gauss-Seidel  acc = sum_j (gamma * T[s, a, j]) * V[j], V holding this sweep's values of the states before s;
//                 Q[s, a] = R[s, a] + acc;  V[s] = max_a Q[s, a] at once
//   both stop after the sweep with max_s |Vold[s] - V[s]| < epsilon (float32 difference, compared in float64).
// A uniform row is the row of S entries c: bit for bit what cmdp_vi_discounted computes on the CSR of the dense model.
// The scheme of an instance is model_vi_scheme (infinite_horizon.py:28-36) on nnz = entries with val > 0 plus S per uniform
// row, taken in the prologue, unless the caller forces one.
//
// One wavefront per instance; V (and Vold for Jacobi) in LDS.  The S-term chain of a uniform row is serial, so it is shared:
// c0 = the c of the instance's first uniform row (UCRL2 has one c, 1 / S; rows with another c stay exact and walk their own
// chain).  The products c0 * Vold[j] (Jacobi) or (gamma * c0) * V[j] (Gauss-Seidel) do not depend on the accumulator: the
// lanes write them to LDS side by side and the chain only adds.
//   Jacobi: every c0 row of a sweep has the same tv -- one chain of S adds per sweep.
//   Gauss-Seidel: the rows of state s with c0 share one chain.  Its part over the states 0 .. s - 1 (already updated) is the
//     accumulator the chain of state s - 1 passed through after s - 1 terms, plus one add of state s - 1's new product: the
//     running prefix P.  Only the suffix over s .. S - 1 is added per state, S^2 / 2 dependent adds per sweep, and only for
//     states that have a c0 row.  The chain is wave-uniform: every lane reads the same LDS words (a broadcast) and holds the
//     same sum, so nothing has to be handed from lane to lane.
// Sparse rows: Jacobi, lane = state, actions in order (as K2); Gauss-Seidel, lane = action of the current state (as K3), the
// next state's row descriptors fetched while the current one is worked on.
#pragma once

#define MVI_THREADS 64
#define MVI_MAX_STATES 4096
#define MVI_MAX_ACTIONS 64

struct ModelViArgs {
  const int32_t* S;          // [count] states
  const int32_t* A;          // [count] actions
  const int64_t* state_off;  // [count] first state (V) of the instance
  const int64_t* row_off;    // [count] first row (Q, R, uni, ptr) of the instance
  const int64_t* ptr;        // [n_rows + 1] row pointers into col / val
  const int32_t* col;        // instance-relative successor, ascending within a row
  const float* val;          // T[s, a, col] >= 0
  const float* uni;          // [n_rows] c when the row is c > 0 at every state (its CSR entries are then not read), else 0
  const float* R;            // [n_rows]
  const int32_t* list;       // block k solves instance list[k]; null: instance k.  The other instances' outputs stay as they are
  float gamma;
  double eps;
  int scheme;                // CMDP_SCHEME_AUTO: model_vi_scheme per instance
  int64_t size_threshold;
  double density_threshold;
  int64_t max_sweeps;
  float* Q;                  // [n_rows]
  float* V;                  // [n_states]
  int64_t* sweeps;           // [count]
  int32_t* scheme_used;      // [count]
  int32_t* status;           // [count] 0 or CMDP_ERR_MAX_ITER
};

// reference infinite_horizon.py:28-36: `T.size > sparse_n_states_threshold and T_sparse.nnz / T.size < sparse_nnz_per_threshold`
__host__ __device__ inline int model_vi_scheme(int S, int A, int64_t nnz, int64_t size_threshold, double density_threshold) {
  const double size = (double)S * (double)A * (double)S;   // exact: at most 2^53
  return (size > (double)size_threshold && (double)nnz / size < density_threshold) ? CMDP_SCHEME_JACOBI : CMDP_SCHEME_GAUSS_SEIDEL;
}

inline size_t model_vi_lds_bytes(int max_S) { return (size_t)((max_S + 3) & ~3) * 3 * sizeof(float); }

// acc + p[j] + p[j + 1] + ... + p[n - 1], one add after the other; p is 16-byte aligned and wave-uniform
__device__ __forceinline__ float mvi_chain(float acc, const float* __restrict__ p, int j, int n) {
  for (; j < n && (j & 3); ++j) acc = __fadd_rn(acc, p[j]);
#pragma unroll 4
  for (; j + 4 <= n; j += 4) {
    const float4 x = *reinterpret_cast<const float4*>(p + j);
    acc = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc, x.x), x.y), x.z), x.w);
  }
  for (; j < n; ++j) acc = __fadd_rn(acc, p[j]);
  return acc;
}

__global__ void __launch_bounds__(MVI_THREADS) k_vi_model(ModelViArgs g) {
  extern __shared__ __align__(16) unsigned char mvi_lds[];
  const int b = g.list ? g.list[blockIdx.x] : blockIdx.x, lane = threadIdx.x;
  const int S = g.S[b], A = g.A[b];
  const int SP = (S + 3) & ~3;
  float* V = reinterpret_cast<float*>(mvi_lds);
  float* W = V + SP;
  float* prod = W + SP;
  const int64_t r0 = g.row_off[b];
  const int64_t* __restrict__ ptr = g.ptr + r0;
  const int32_t* __restrict__ col = g.col;
  const float* __restrict__ val = g.val;
  const float* __restrict__ uni = g.uni + r0;
  const float* __restrict__ R = g.R + r0;
  float* __restrict__ Q = g.Q + r0;
  const int rows = S * A;
  const float gamma = g.gamma;

  // prologue: the first uniform row (its c is the shared one) and, for the rule, nnz as sparse.COO(T).nnz counts it
  int first = rows;
  long long nnz = 0;
  const bool count = g.scheme == CMDP_SCHEME_AUTO;
  for (int r = lane; r < rows; r += MVI_THREADS) {
    if (uni[r] > 0.0f) {
      first = first < r ? first : r;
      nnz += S;
    } else if (count) {
      for (int64_t k = ptr[r], e = ptr[r + 1]; k < e; ++k) nnz += val[k] > 0.0f ? 1 : 0;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int f = __shfl_xor(first, o, 64);
    first = first < f ? first : f;
    nnz += __shfl_xor(nnz, o, 64);
  }
  const float c0 = first < rows ? uni[first] : 0.0f;
  const int scheme = count ? model_vi_scheme(S, A, (int64_t)nnz, g.size_threshold, g.density_threshold) : g.scheme;
  for (int i = lane; i < SP; i += MVI_THREADS) { V[i] = 0.0f; W[i] = 0.0f; prod[i] = 0.0f; }
  __syncthreads();

  float* Vout = V;
  int64_t sweep = 1;
  bool done = false;
  if (scheme == CMDP_SCHEME_JACOBI) {
    float* Vold = V;
    float* Vnew = W;
    for (;; ++sweep) {
      float tv0 = 0.0f;
      if (c0 > 0.0f) {
        for (int i = lane; i < S; i += MVI_THREADS) prod[i] = __fmul_rn(c0, Vold[i]);
        __syncthreads();
        tv0 = mvi_chain(0.0f, prod, 0, S);
      }
      float dmax = 0.0f;
      for (int s = lane; s < S; s += MVI_THREADS) {
        float v = 0.0f;
        for (int a = 0; a < A; ++a) {
          const int r = s * A + a;
          const float u = uni[r];
          float tv = 0.0f;
          if (u > 0.0f) {
            if (u == c0) tv = tv0;
            else
              for (int j = 0; j < S; ++j) tv = __fadd_rn(tv, __fmul_rn(u, Vold[j]));
          } else {
            for (int64_t k = ptr[r], e = ptr[r + 1]; k < e; ++k) tv = __fadd_rn(tv, __fmul_rn(val[k], Vold[col[k]]));
          }
          const float q = __fadd_rn(R[r], __fmul_rn(gamma, tv));
          Q[r] = q;
          v = a == 0 ? q : fmaxf(v, q);
        }
        Vnew[s] = v;
        dmax = fmaxf(dmax, fabsf(__fsub_rn(Vold[s], v)));
      }
      dmax = wave_max(dmax);
      __syncthreads();  // Vnew is whole, and every lane has read Vold and prod
      float* t = Vold; Vold = Vnew; Vnew = t;
      done = (double)dmax < g.eps;
      if (done || sweep >= g.max_sweeps) break;
    }
    Vout = Vold;
  } else {
    const bool active = lane < A;
    const float gc0 = __fmul_rn(gamma, c0);
    for (;; ++sweep) {
      if (c0 > 0.0f)
        for (int i = lane; i < S; i += MVI_THREADS) prod[i] = __fmul_rn(gc0, V[i]);
      __syncthreads();
      float P = 0.0f, dmax = 0.0f;
      float u_n = 0.0f, R_n = 0.0f;
      int64_t lo_n = 0, hi_n = 0;
      if (active) { u_n = uni[lane]; R_n = R[lane]; lo_n = ptr[lane]; hi_n = ptr[lane + 1]; }
      for (int s = 0; s < S; ++s) {
        const float u = u_n, Rr = R_n;
        const int64_t lo = lo_n, hi = hi_n;
        if (active && s + 1 < S) {  // the next state's rows: their loads fly under this state's chain
          const int rn = (s + 1) * A + lane;
          u_n = uni[rn]; R_n = R[rn]; lo_n = ptr[rn]; hi_n = ptr[rn + 1];
        }
        const bool shared = active && u > 0.0f && u == c0;
        float chain = 0.0f;
        if (__ballot(shared) != 0ull) chain = mvi_chain(P, prod, s, S);
        float q = -INFINITY;
        if (active) {
          float acc = 0.0f;
          if (shared) {
            acc = chain;
          } else if (u > 0.0f) {
            const float gu = __fmul_rn(gamma, u);
            for (int j = 0; j < S; ++j) acc = __fadd_rn(acc, __fmul_rn(gu, V[j]));
          } else {
            for (int64_t k = lo; k < hi; ++k) acc = __fadd_rn(acc, __fmul_rn(__fmul_rn(gamma, val[k]), V[col[k]]));
          }
          q = __fadd_rn(Rr, acc);
          Q[s * A + lane] = q;
        }
        const float v = wave_max(q);
        const float old = V[s];
        __syncthreads();  // every lane has read V and prod for this state before they change
        if (lane == 0) { V[s] = v; prod[s] = __fmul_rn(gc0, v); }
        __syncthreads();
        P = __fadd_rn(P, __fmul_rn(gc0, v));
        dmax = fmaxf(dmax, fabsf(__fsub_rn(old, v)));
      }
      done = (double)dmax < g.eps;
      if (done || sweep >= g.max_sweeps) break;
    }
  }
  float* __restrict__ Vg = g.V + g.state_off[b];
  for (int i = lane; i < S; i += MVI_THREADS) Vg[i] = Vout[i];
  if (lane == 0) {
    g.sweeps[b] = sweep;
    g.scheme_used[b] = scheme;
    g.status[b] = done ? 0 : CMDP_ERR_MAX_ITER;
  }
}
