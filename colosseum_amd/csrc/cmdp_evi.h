// cmdp_evi.h -- K10 k_evi: extended value iteration, the optimistic solver of UCRL2
// (colosseum/dynamic_programming/infinite_horizon.py:67-118 with _max_proba at :222-251).
//
// One workgroup per instance runs every sweep of its instance to convergence or to max_sweeps; there is no host round
// trip per sweep.  LDS holds u1 and u2 (float32, as in the reference), the sweep's order as sorted 64-bit keys
// (sortable bits of u1[i] << 32 | i: a bitonic sort of the next power of two >= S keys, so ties in u1 break by ascending
// state index) and every state's rank in that order (uint16).  LDS bytes = 8 P + 10 S for P = 2^ceil(log2 S): 73 728 at
// S = 4096, the largest instance taken.
//
// A thread owns a state and runs its actions in order (the u2 rule "replace when larger OR within epsilon" is sequential
// over the actions).  Per row (s, a), with p = T[s, a] and best = the last state of the order:
//   min1 = min(1.0, double(p[best]) + beta_p0 / 2)                                  (float64, element 0 of the bound)
//   min1 == 1: p2 = one-hot(best) and the dot is u1[best] - u1[s] (0 when best == s): O(1);
//   otherwise p2 = p, p2[best] = float(min1), s = 1 - p[best] + min1, and the nonzeros of p are walked in ascending rank,
//     p2[j] = float(max(0, 1 - s + p_j)), s += max1 - p_j (float64), stopping once s <= 1.  The walk never sorts the
//     row: rows of at most EVI_SELECT_NNZ entries take their next nonzero by selection on the shared ranks, longer rows
//     scan the shared order from the bottom and look their entries up by bisection, and UNIFORM rows (every state, one
//     value c > 0: the estimated model's unvisited pairs; flagged on the host) scan the order with p_j = c.
// The dot product dot(p2 - e_s, u1) is, by this kernel's definition, a float64 sum of exact float32 x float32 products
// rounded once to float32: the row's CSR dot product in column order (c * sum(u1) for a uniform row, the sum taken once
// per sweep in a fixed order), plus (p2_j - p_j) u1_j for every walked state other than s and best, then best's and s's
// own corrections, with p2[s] - 1 rounded to float32 as the reference stores it.  A sweep costs O(nnz + walked) reads
// of its rows instead of O(S^2 A).  The reference's float32 `np.dot` (a BLAS sdot of unspecified order) rounds at every
// addition; this one rounds once.
//   r_opt = min(float(r_max), double(R) + beta_r); v = r_opt + dot (float64); Q = float(v);
//   u2[s] = float(v + u1[s]) at the first action and whenever v + u1[s] > u2[s] or |v + u1[s] - u2[s]| < epsilon;
//   V[s] = max_a Q; stop when ptp(u2 - u1) < epsilon (float32 differences, float32 ptp) and report ptp(u1).
#pragma once

#define EVI_THREADS 256
#define EVI_MAX_STATES 4096
#define EVI_SELECT_NNZ 16

struct EviArgs {
  const int32_t* S;          // [count] states
  const int32_t* A;          // [count] actions
  const int64_t* state_off;  // [count] first state (V) of the instance
  const int64_t* row_off;    // [count] first row (Q, R, beta_r, beta_p0, ptr) of the instance
  const int64_t* ptr;        // [n_rows + 1] CSR row pointers into col / val
  const int32_t* col;        // instance-relative successor, ascending within a row
  const float* val;          // T[s, a, col] > 0 (explicit zeros are skipped)
  const float* uni;          // [n_rows] c when the row is c > 0 at every state, else 0
  const float* R;            // [n_rows] estimated rewards
  const double* beta_r;      // [n_rows]
  const double* beta_p0;     // [n_rows] element 0 of beta_p[s, a]
  const double* r_max;       // [count]
  double eps;
  int64_t max_sweeps;
  float* Q;                  // [n_rows]
  float* V;                  // [n_states]
  double* span;              // [count]
  int64_t* sweeps;           // [count]
  int32_t* status;           // [count] 0 or CMDP_ERR_MAX_ITER
};

// Dynamic LDS of a launch whose largest instance has S states: k_evi's carve-up below (keys, u1, u2, rank)
inline size_t evi_lds_bytes(int S) {
  int P = 1;
  while (P < S) P <<= 1;
  return (size_t)P * 8 + (size_t)S * 10;
}

__device__ __forceinline__ uint32_t evi_sortable(float f) {
  uint32_t b = __float_as_uint(__fadd_rn(f, 0.0f));  // -0 -> +0: argsort sees them equal
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// T[row, j] of a CSR row with ascending columns (0 when absent).
__device__ __forceinline__ float evi_lookup(const int32_t* __restrict__ col, const float* __restrict__ val, int64_t b,
                                            int64_t e, int j) {
  while (b < e) {
    int64_t m = b + ((e - b) >> 1);
    int c = col[m];
    if (c == j) return val[m];
    if (c < j) b = m + 1; else e = m;
  }
  return 0.0f;
}

// One step of the walk (_max_proba's loop body); returns true once s <= 1.
struct EviWalk {
  double sacc, corr;
  float pb2, ps2;
  int s, best;
  __device__ __forceinline__ bool step(int j, float pj, const float* u1) {
    double x = (1.0 - sacc) + (double)pj;
    double m = x > 0.0 ? x : 0.0;
    sacc = sacc + (m - (double)pj);
    float nv = (float)m;
    if (j == best) pb2 = nv;
    else if (j == s) ps2 = nv;
    else corr += ((double)nv - (double)pj) * (double)u1[j];
    return sacc <= 1.0;
  }
};

__global__ void __launch_bounds__(EVI_THREADS) k_evi(EviArgs g) {
  extern __shared__ __align__(16) unsigned char evi_lds[];
  __shared__ double red_d[EVI_THREADS / 64];
  __shared__ float red_f[4][EVI_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int S = g.S[b], A = g.A[b];
  int P = 1;
  while (P < S) P <<= 1;
  uint64_t* keys = reinterpret_cast<uint64_t*>(evi_lds);
  float* u1 = reinterpret_cast<float*>(keys + P);
  float* u2 = u1 + S;
  uint16_t* rank = reinterpret_cast<uint16_t*>(u2 + S);
  const int64_t r0 = g.row_off[b], v0 = g.state_off[b];
  const float rmax = (float)g.r_max[b];
  const double eps = g.eps;
  const int64_t* __restrict__ ptr = g.ptr;
  const int32_t* __restrict__ col = g.col;
  const float* __restrict__ val = g.val;

  for (int i = tid; i < S; i += EVI_THREADS) u1[i] = 0.0f;
  for (int64_t sweep = 1;; ++sweep) {
    // the order of this sweep: argsort(u1), ties by state index (sweep 1: u1 = 0, the identity as in the reference)
    for (int i = tid; i < P; i += EVI_THREADS)
      keys[i] = i < S ? ((uint64_t)evi_sortable(u1[i]) << 32) | (uint32_t)i : ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < P; i += EVI_THREADS) {
          int l = i ^ j;
          if (l > i) {
            uint64_t x = keys[i], y = keys[l];
            if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[l] = x; }
          }
        }
        __syncthreads();
      }
    double part = 0.0;  // sum(u1): thread-strided float64 partial sums, then a fixed butterfly and the waves in order
    for (int i = tid; i < S; i += EVI_THREADS) {
      rank[(uint32_t)keys[i]] = (uint16_t)i;
      part += (double)u1[i];
    }
    part = wave_sum(part);
    if (lane == 0) red_d[wid] = part;
    __syncthreads();
    double sumU = 0.0;
    for (int w = 0; w < EVI_THREADS / 64; ++w) sumU += red_d[w];
    const int best = (int)(uint32_t)keys[S - 1];
    const float ubest = u1[best];

    float dmin = INFINITY, dmax = -INFINITY, umin = INFINITY, umax = -INFINITY;
    for (int s = tid; s < S; s += EVI_THREADS) {
      const float u1s = u1[s];
      float u2s = 0.0f, vmax = 0.0f;
      for (int a = 0; a < A; ++a) {
        const int64_t r = r0 + (int64_t)s * A + a;
        const int64_t rb = ptr[r], re = ptr[r + 1];
        const float c = g.uni[r];
        const float pbest = c > 0.0f ? c : evi_lookup(col, val, rb, re, best);
        double min1 = (double)pbest + g.beta_p0[r] / 2.0;
        min1 = min1 < 1.0 ? min1 : 1.0;
        double D;
        if (min1 == 1.0) {
          D = best == s ? 0.0 : (double)ubest - (double)u1s;
        } else {
          const float ps = c > 0.0f ? c : (s == best ? pbest : evi_lookup(col, val, rb, re, s));
          double base = 0.0;
          if (c > 0.0f) base = (double)c * sumU;
          else
            for (int64_t k = rb; k < re; ++k) base += (double)val[k] * (double)u1[col[k]];
          EviWalk w{1.0 - (double)pbest + min1, 0.0, (float)min1, ps, s, best};
          if (c > 0.0f) {
            for (int k = 0; k < S; ++k)
              if (w.step((int)(uint32_t)keys[k], c, u1)) break;
          } else if (re - rb <= EVI_SELECT_NNZ) {
            int prev = -1;
            for (;;) {
              int nr = S, nj = -1;
              float np_ = 0.0f;
              for (int64_t k = rb; k < re; ++k) {
                const float p = val[k];
                if (!(p > 0.0f)) continue;
                const int j = col[k], rk = rank[j];
                if (rk > prev && rk < nr) { nr = rk; nj = j; np_ = p; }
              }
              if (nj < 0 || w.step(nj, np_, u1)) break;
              prev = nr;
            }
          } else {
            for (int k = 0; k < S; ++k) {
              const int j = (int)(uint32_t)keys[k];
              const float p = evi_lookup(col, val, rb, re, j);
              if (p > 0.0f && w.step(j, p, u1)) break;
            }
          }
          if (s == best) w.ps2 = w.pb2;
          else w.corr += ((double)w.pb2 - (double)pbest) * (double)ubest;
          const float vs = (float)((double)w.ps2 - 1.0);
          w.corr += ((double)vs - (double)ps) * (double)u1s;
          D = base + w.corr;
        }
        const float dot = (float)D;
        double ropt = (double)g.R[r] + g.beta_r[r];
        ropt = ropt < (double)rmax ? ropt : (double)rmax;
        const double v = ropt + (double)dot;
        const float q = (float)v;
        g.Q[r] = q;
        const double wv = v + (double)u1s;
        if (a == 0 || wv > (double)u2s || fabs(wv - (double)u2s) < eps) u2s = (float)wv;
        vmax = (a == 0 || q > vmax) ? q : vmax;
      }
      u2[s] = u2s;
      g.V[v0 + s] = vmax;
      const float d = __fsub_rn(u2s, u1s);
      dmin = fminf(dmin, d); dmax = fmaxf(dmax, d);
      umin = fminf(umin, u1s); umax = fmaxf(umax, u1s);
    }
    // ptp(u2 - u1) and ptp(u1): min / max are exact, so their reduction order does not matter
    for (int o = 32; o > 0; o >>= 1) {
      dmin = fminf(dmin, __shfl_xor(dmin, o, 64)); dmax = fmaxf(dmax, __shfl_xor(dmax, o, 64));
      umin = fminf(umin, __shfl_xor(umin, o, 64)); umax = fmaxf(umax, __shfl_xor(umax, o, 64));
    }
    if (lane == 0) { red_f[0][wid] = dmin; red_f[1][wid] = dmax; red_f[2][wid] = umin; red_f[3][wid] = umax; }
    __syncthreads();
    for (int w = 0; w < EVI_THREADS / 64; ++w) {
      dmin = fminf(dmin, red_f[0][w]); dmax = fmaxf(dmax, red_f[1][w]);
      umin = fminf(umin, red_f[2][w]); umax = fmaxf(umax, red_f[3][w]);
    }
    const bool done = (double)__fsub_rn(dmax, dmin) < eps;
    if (done || sweep >= g.max_sweeps) {
      if (tid == 0) {
        g.span[b] = done ? (double)__fsub_rn(umax, umin) : NAN;
        g.sweeps[b] = sweep;
        g.status[b] = done ? 0 : CMDP_ERR_MAX_ITER;
      }
      return;
    }
    float* t = u1; u1 = u2; u2 = t;
    __syncthreads();  // every thread has read red_f / red_d / keys before the next sweep writes them
  }
}
