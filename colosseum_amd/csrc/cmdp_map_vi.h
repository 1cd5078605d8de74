// cmdp_map_vi.h -- K15 k_vi_episodic_map: episodic value iteration (colosseum/dynamic_programming/finite_horizon.py:11-26) on
// the MAP estimate of a Bayesian model (BayesianMDPModel.get_map_estimate: M_DIR hyper_params / hyper_params.sum(-1), N_NIG
// hyper_params[:, :, 0]), straight from the model's tables in K11 / K12's layout.  What
// PSRLEpisodic.current_optimal_stochastic_policy solves (posterior_sampling.py:78-82), without the dense [S, A, S] array.
//
// A row (s, a) of the transition hyper-parameters holds hp[e] at the ascending columns col[e] of its layout positions
// row_ptr[r] .. row_ptr[r + 1] and the instance's prior at every other state.
//   prologue, once per solve and row:
//     rowsum = numpy's pairwise float32 sum of the dense row in column order (psrl_host::pairwise_sum_f32 restates it)
//     c      = prior / rowsum          every element of T_map outside the layout
//     t[e]   = hp[e] / rowsum          T_map[s, a, col[e]]               -- float32 divisions: bit for bit the reference's T_map
//   layers h = H - 1 .. 0, V[H] = 0:
//     SV        = sum_j double(V[h + 1, j])                              -- one per layer, float64, fixed order
//     dot       = double(c) * (SV - sum_e double(V[h + 1, col[e]])) + sum_e double(t[e]) * double(V[h + 1, col[e]])
//     Q[h, s, a] = float(double(mu[s, a]) + dot);   V[h, s] = max_a Q[h, s, a]
// which is the dense dot product with the prior's share factored out: O(layout + S) work per layer instead of O(S * A * S).
// The two sums over e run in layout order in float64; the products double(t) * double(V) are exact.
//
// One workgroup per instance; V[h + 1] and V[h] in LDS (2 x 16 KB at 4096 states), and next to them the instance's row
// pointers, c, mu, t and col when all of that stays under MAPVI_STAGE_MAX_BYTES (every layer reads them again, each read the
// end of a dependent chain ptr -> col -> V; from HBM that chain, not bandwidth, is the layer's time); larger instances
// read them from global memory through the same code.  Prologue: a lane per row walks the dense
// row once in column order with a cursor into the layout -- the pairwise sum's blocks come in ascending order, so the cursor
// never goes back; the recursion above 128 elements depends on S alone, so one lane flattens it once per workgroup into
// a list of runs and merges (mapvi_plan) and every lane replays that list with its partial sums in registers.
// Layers: every wavefront takes SV itself (the same lanes add the same words in the same order in each of them, so no
// barrier and no broadcast is needed), then a lane per state walks the state's actions and their layout positions; one
// barrier per layer.  Rows of any length are walked by one lane.
#pragma once

#define MAPVI_THREADS 512
#define MAPVI_MAX_STATES 4096
#define MAPVI_DEPTH 7      // splits of numpy's pairwise sum before a run of <= 128 elements is reached: at most 6 up to 4096 elements
#define MAPVI_MAX_RUNS 64  // ... and its runs: at most 33

struct MapViArgs {
  const int32_t* list;     // block k solves instance list[k]; null: instance k
  const int32_t* S;        // [count]
  const int32_t* A;        // [count]
  const int64_t* r_off;    // [count] first row: row_ptr, c, mu; Q at (H + 1) * r_off
  const int64_t* s_off;    // [count] first state: V at (H + 1) * s_off
  const int64_t* row_ptr;  // [n_rows + 1] into col / hp / t
  const int32_t* col;      // instance-relative, ascending within a row
  const float* hp;         // M_DIR hyper-parameters at the layout's positions
  const float* prior;      // [count] ... and everywhere else
  const float* mu;         // reward MAP of row r at mu[r * mu_stride] (4: the N_NIG table itself)
  int mu_stride;
  float* t;                // [NZ] out: T_map at the layout's positions
  float* c;                // [n_rows] out: T_map elsewhere
  float* Q;                // [H + 1][S][A] per instance, layer H zero
  float* V;                // [H + 1][S]
  int H;
  unsigned lds_bytes;      // dynamic LDS of the launch: an instance whose tables fit in it keeps them there (map_vi_stage_bytes)
};

#define MAPVI_STAGE_MAX_BYTES (128u * 1024u)   // of the CU's 160 KB: two staged workgroups of <= 80 KB share a CU

// LDS of one instance: the two value layers, and -- staged -- its row pointers, c, mu, t and col
__host__ __device__ inline size_t map_vi_value_bytes(int S) { return (size_t)2 * ((S + 3) & ~3) * sizeof(float); }
__host__ __device__ inline size_t map_vi_stage_bytes(int S, int A, int64_t nz) {
  const size_t rows = (size_t)S * A;
  return map_vi_value_bytes(S) + 8 * (rows + 1) + 8 * rows + 8 * (size_t)nz;
}
// what a launch asks for: every instance's value layers, and the tables of every instance that stays under the limit
inline size_t map_vi_lds_bytes(int S, int A, int64_t nz) {
  const size_t full = map_vi_stage_bytes(S, A, nz);
  return full <= MAPVI_STAGE_MAX_BYTES ? full : map_vi_value_bytes(S);
}

// the rounded add of numpy's pairwise sums, chosen by the element type
__device__ __forceinline__ float rn_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double rn_add(double a, double b) { return __dadd_rn(a, b); }

// the dense row, read once in ascending column order: val[e] at the layout's columns col[e], e in [z, ze), `fill` elsewhere.
// K15 / K17 and the MAP fill read float32 hyper-parameters over the prior, K18's chain float64 P_minus over 0.
template <typename T>
struct MapViRow {
  typedef T elem;
  const int32_t* col;
  const T* val;
  int64_t z, ze;
  T fill;
  __device__ __forceinline__ T at(int j) {
    if (z < ze && col[z] == j) return val[z++];
    return fill;
  }
};

// FLOAT_pairwise_sum / DOUBLE_pairwise_sum on a run of n <= 128 elements starting at column j0
template <typename Row>
__device__ __forceinline__ typename Row::elem mapvi_run(Row& r, int j0, int n) {
  typedef typename Row::elem T;
  if (n < 8) {
    T res = 0;
    for (int i = 0; i < n; ++i) res = rn_add(res, r.at(j0 + i));
    return res;
  }
  T acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = r.at(j0 + j);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = rn_add(acc[j], r.at(j0 + i + j));
  }
  T res = rn_add(rn_add(rn_add(acc[0], acc[1]), rn_add(acc[2], acc[3])), rn_add(rn_add(acc[4], acc[5]), rn_add(acc[6], acc[7])));
  for (; i < n; ++i) res = rn_add(res, r.at(j0 + i));
  return res;
}

// The recursion of FLOAT_pairwise_sum on n elements as a flat program: its runs of <= 128 elements from left to right and,
// after each run, how many of the partial sums on the stack are merged (top two added, the older one on the left).  A node
// of n > 128 elements splits at n2 = n / 2 rounded down to a multiple of 8.  One lane; `work` holds MAPVI_DEPTH * 2 + 2 words.
__device__ inline int mapvi_plan(int n, int* work, short* run, signed char* merges) {
  constexpr int MERGE = -1;
  int sp = 0, n_runs = 0, cur = n;
  for (;;) {
    while (cur > 128) {
      int n2 = cur / 2;
      n2 -= n2 % 8;
      work[sp++] = MERGE;
      work[sp++] = cur - n2;
      cur = n2;
    }
    run[n_runs] = (short)cur;
    merges[n_runs] = 0;
    ++n_runs;
    for (;;) {
      if (sp == 0) return n_runs;
      const int x = work[--sp];
      if (x != MERGE) { cur = x; break; }
      ++merges[n_runs - 1];
    }
  }
}

// numpy's pairwise sum of the dense row `r` in the row's element type: one lane replays the plan of mapvi_plan with its
// partial sums in registers.  K15's and K17's prologues, the MAP fill of the continuous PSRL agent (cmdp_psrlc.h) and, in
// float64 over zero fill, the P_minus chain of its optimistic sample (cmdp_psrlo.h) share it.
template <typename Row>
__device__ __forceinline__ typename Row::elem mapvi_rowsum(Row& r, int n_runs, const short* plan_run, const signed char* plan_merges) {
  typedef typename Row::elem T;
  T st[MAPVI_DEPTH + 1];   // the partial sums waiting for their right-hand halves, st[0] the newest
#pragma unroll
  for (int k = 0; k <= MAPVI_DEPTH; ++k) st[k] = 0;
  int j0 = 0;
  for (int k = 0; k < n_runs; ++k) {
    const int n = plan_run[k];
    const T x = mapvi_run(r, j0, n);
    j0 += n;
#pragma unroll
    for (int d = MAPVI_DEPTH; d > 0; --d) st[d] = st[d - 1];
    st[0] = x;
    for (int m = plan_merges[k]; m > 0; --m) {
      st[0] = rn_add(st[1], st[0]);
#pragma unroll
      for (int d = 1; d < MAPVI_DEPTH; ++d) st[d] = st[d + 1];
    }
  }
  return st[0];
}

__global__ void __launch_bounds__(MAPVI_THREADS) k_vi_episodic_map(MapViArgs g) {
  extern __shared__ __align__(16) float mapvi_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = g.list ? g.list[blockIdx.x] : blockIdx.x;
  const int S = g.S[b], A = g.A[b], H = g.H;
  const int spad = (S + 3) & ~3;
  float* vn = mapvi_lds;          // V[h + 1]
  float* vc = mapvi_lds + spad;   // V[h]
  const int64_t r0 = g.r_off[b];
  const int64_t* __restrict__ ptr = g.row_ptr + r0;
  const int32_t* __restrict__ col = g.col;
  const float* __restrict__ hp = g.hp;
  float* tmap = g.t;               // written in the prologue, read in the layers
  float* cmap = g.c + r0;
  const float prior = g.prior[b];
  const int mstride = g.mu_stride;
  const float* __restrict__ mu = g.mu + r0 * mstride;
  float* __restrict__ Q = g.Q + (int64_t)(H + 1) * r0;
  float* __restrict__ V = g.V + (int64_t)(H + 1) * g.s_off[b];
  const int nrows = S * A;

  __shared__ int plan_work[2 * MAPVI_DEPTH + 2];
  __shared__ short plan_run[MAPVI_MAX_RUNS];
  __shared__ signed char plan_merges[MAPVI_MAX_RUNS];
  __shared__ int plan_n;
  if (tid == 0) plan_n = mapvi_plan(S, plan_work, plan_run, plan_merges);
  __syncthreads();
  const int n_runs = plan_n;
  // the instance's tables are read again in every layer: from LDS when they fit in what the launch was given
  const int64_t z0 = ptr[0], nz = ptr[nrows] - z0;
  const bool staged = map_vi_stage_bytes(S, A, nz) <= (size_t)g.lds_bytes;
  int64_t* lptr = reinterpret_cast<int64_t*>(mapvi_lds + 2 * spad);   // [nrows + 1], as ptr
  float* lc = reinterpret_cast<float*>(lptr + nrows + 1);             // [nrows]
  float* lmu = lc + nrows;                                             // [nrows]
  float* lt = lmu + nrows;                                             // [nz]
  int32_t* lcol = reinterpret_cast<int32_t*>(lt + nz);                 // [nz]
  if (staged && tid == 0) lptr[nrows] = z0 + nz;
  for (int row = tid; row < nrows; row += MAPVI_THREADS) {
    const int64_t zb = ptr[row], ze = ptr[row + 1];
    MapViRow<float> r{col, hp, zb, ze, prior};
    const float rowsum = mapvi_rowsum(r, n_runs, plan_run, plan_merges);
    const float c = __fdiv_rn(prior, rowsum);
    cmap[row] = c;
    for (int64_t e = zb; e < ze; ++e) tmap[e] = __fdiv_rn(hp[e], rowsum);
    if (staged) {
      lptr[row] = zb;
      lc[row] = c;
      lmu[row] = mu[(int64_t)row * mstride];
      for (int64_t e = zb; e < ze; ++e) {
        lt[e - z0] = __fdiv_rn(hp[e], rowsum);
        lcol[e - z0] = col[e];
      }
    }
  }
  for (int i = tid; i < 2 * spad; i += MAPVI_THREADS) mapvi_lds[i] = 0.0f;
  for (int i = tid; i < S; i += MAPVI_THREADS) V[(int64_t)H * S + i] = 0.0f;
  for (int i = tid; i < nrows; i += MAPVI_THREADS) Q[(int64_t)H * nrows + i] = 0.0f;
  __syncthreads();   // the workgroup's t and c are written

  // one walk for both homes of the tables (generic pointers: LDS or global)
  const int64_t* P = staged ? lptr : ptr;
  const int32_t* C = staged ? lcol : col + z0;
  const float* Tm = staged ? lt : tmap + z0;
  const float* Cm = staged ? lc : cmap;
  const float* Mu = staged ? lmu : mu;
  const int mus = staged ? 1 : mstride;
  for (int h = H - 1; h >= 0; --h) {
    double sv = 0.0;
    for (int j = lane; j < S; j += 64) sv += (double)vn[j];
    sv = wave_sum(sv);
    for (int s = tid; s < S; s += MAPVI_THREADS) {
      float vmax = -INFINITY;
      for (int a = 0; a < A; ++a) {
        const int row = s * A + a;
        double in_v = 0.0, in_tv = 0.0;
        for (int64_t e = P[row] - z0, ze = P[row + 1] - z0; e < ze; ++e) {
          const double v = (double)vn[C[e]];
          in_v += v;
          in_tv += (double)Tm[e] * v;
        }
        const double dot = __dadd_rn(__dmul_rn((double)Cm[row], __dsub_rn(sv, in_v)), in_tv);
        const float q = (float)__dadd_rn((double)Mu[(int64_t)row * mus], dot);
        Q[(int64_t)h * nrows + row] = q;
        vmax = fmaxf(vmax, q);
      }
      vc[s] = vmax;
      V[(int64_t)h * S + s] = vmax;
    }
    __syncthreads();
    float* x = vn; vn = vc; vc = x;
  }
}

// ---- host side: the CPU-testable definition of the prologue ---------------------------------------------------------
namespace map_vi_host {

// rowsum [S * A], c [S * A] and t (indexed as hp) of one instance; row_ptr indexes col / hp / t directly
template <typename PairwiseSum>
inline void map_rows(int S, int A, const int64_t* row_ptr, const int32_t* col, const float* hp, float prior, PairwiseSum&& sum,
                     float* rowsum, float* c, float* t) {
  std::vector<float> dense((size_t)S);
  for (int64_t r = 0; r < (int64_t)S * A; ++r) {
    std::fill(dense.begin(), dense.end(), prior);
    for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e) dense[(size_t)col[e]] = hp[e];
    const float rs = sum(dense.data(), (int64_t)S);
    if (rowsum) rowsum[r] = rs;
    if (c) c[r] = prior / rs;
    if (t)
      for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e) t[e] = hp[e] / rs;
  }
}

// the splits numpy's pairwise sum takes on n elements before every run is <= 128 long
inline int pairwise_depth(int64_t n) {
  if (n <= 128) return 0;
  int64_t n2 = n / 2;
  n2 -= n2 % 8;
  return 1 + std::max(pairwise_depth(n2), pairwise_depth(n - n2));
}

}  // namespace map_vi_host
