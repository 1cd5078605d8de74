// cmdp_dp_plan.h -- host-side choice of the dynamic-programming sweep kernels (K2, K2R, K2U, K2W, K3; K5S / K5T / K5C).
//
// The compiled instantiations of every template family are listed here once, as X-macro lists: the launch switches of
// cmdp.hip and the predicates "is this shape compiled" below expand the same lists.  pick_sweep decides which kernel
// serves a batch of a given shape.  pick_diameter_path / _cluster / _lanes decide the same for a continuous diameter: the
// workgroup kernels (then pick_sweep's) or the lanes kernels, whether a call tries K5C first and with which cluster size,
// and which of K5T / K5S-ELL / K5S-CSR, how wide, takes a launch.  The pickers are pure: the handle's back-off state and
// the counters stay with diameter_lanes of cmdp.hip.  Nothing here makes a HIP call or reads the environment.  Included by
// cmdp.hip after the kernel headers.
#pragma once

namespace { int fail(int code, const char* fmt, ...); }  // cmdp.hip: sets the text of cmdp_last_error, returns `code`

constexpr int kDpBlock = 256;

// CMDP_OPT_DP_KERNEL values (include/cmdp.h documents the numbers)
enum { DP_KERNEL_AUTO = 0, DP_KERNEL_K2 = 1, DP_KERNEL_K2R = 2, DP_KERNEL_K2U = 5, DP_KERNEL_K2W = 7,  // Jacobi sweeps
       // cmdp_diameter only: 64 targets per workgroup; the same with the generic CSR walker; with LDS tiles
       DP_KERNEL_K5S = 3, DP_KERNEL_K5S_CSR = 4, DP_KERNEL_K5T = 6 };

// ---- the compiled shapes, once each ------------------------------------------------------------------------------------
// K = max row nnz rounded up, U = distinct successors per state rounded up, spt = states per lane of a 256-lane workgroup,
// st_w = states per lane of one wavefront.  Every K2R and K2U shape is compiled for value iteration and policy evaluation.
// K2R: X(A, K, spt)
#define CMDP_K2R_SHAPES(X)                                                                  \
  X(2, 4, 1) X(2, 4, 2) X(2, 4, 4) X(3, 4, 1) X(3, 4, 2) X(3, 4, 4) X(4, 4, 1) X(4, 4, 2) X(4, 4, 4) \
  X(2, 8, 1) X(2, 8, 2) X(3, 8, 1) X(3, 8, 2) X(4, 8, 1) X(4, 8, 2)
// K2U: X(A, U, K, spt)
#define CMDP_K2U_SHAPES(X)                                                                  \
  X(2, 5, 4, 1) X(2, 5, 4, 2) X(2, 5, 4, 4) X(2, 5, 8, 1) X(2, 5, 8, 2) X(2, 5, 8, 4)       \
  X(3, 5, 4, 1) X(3, 5, 4, 2) X(3, 5, 4, 4) X(3, 5, 8, 1) X(3, 5, 8, 2) X(3, 5, 8, 4)       \
  X(4, 5, 4, 1) X(4, 5, 4, 2) X(4, 5, 4, 4) X(4, 5, 8, 1) X(4, 5, 8, 2) X(4, 5, 8, 4)       \
  X(3, 8, 8, 1) X(3, 8, 8, 2) X(4, 8, 4, 1) X(4, 8, 4, 2) X(4, 8, 8, 1) X(4, 8, 8, 2)
// K2W (U = 5, K = 4): X(A, st_w, modes), modes VI_PE or VI.  Only instantiations that keep their tables in registers: with
// four actions, seven states per lane -- and six under policy evaluation, which also holds the policy's rows -- spill to
// scratch; those batches take K2U.
#define CMDP_K2W_SHAPES(X)                                                                  \
  X(2, 5, VI_PE) X(2, 6, VI_PE) X(2, 7, VI_PE) X(3, 5, VI_PE) X(3, 6, VI_PE) X(3, 7, VI_PE) \
  X(4, 5, VI_PE) X(4, 6, VI)
// Fixed-width rows of the diameter kernels K5S-ELL, K5T and K5C: X(P, A, K); P is handed through (K5C: the cluster size)
#define CMDP_FIXED_WIDTH_SHAPES(X, P)                                                       \
  X(P, 2, 2) X(P, 2, 4) X(P, 2, 8) X(P, 3, 2) X(P, 3, 4) X(P, 3, 8) X(P, 4, 2) X(P, 4, 4) X(P, 4, 8)

#define CMDP_MODES_VI_PE(mode) true
#define CMDP_MODES_VI(mode) ((mode) == DP_VI)
#define CMDP_K2R_IS(AT, KT, ST) || (A == AT && K == KT && spt == ST)
#define CMDP_K2U_IS(AT, UT, KT, ST) || (A == AT && U == UT && K == KT && spt == ST)
#define CMDP_K2W_IS(AT, ST, MODES) || (A == AT && st_w == ST && CMDP_MODES_##MODES(mode))
#define CMDP_FIXED_WIDTH_IS(P, AT, KT) || (A == AT && K == KT)
inline bool k2r_compiled(int A, int K, int spt) { return false CMDP_K2R_SHAPES(CMDP_K2R_IS); }
inline bool k2u_compiled(int A, int U, int K, int spt) { return false CMDP_K2U_SHAPES(CMDP_K2U_IS); }
inline bool k2w_compiled(int A, int st_w, int mode) { return false CMDP_K2W_SHAPES(CMDP_K2W_IS); }

// Width of the fixed-width rows a batch needs (0: none is compiled), and whether (A, K) is a compiled shape: the nine
// shapes are all of 2 <= A <= 4 with K in {2, 4, 8}.
inline int fixed_width_K(int max_row_nnz) { return max_row_nnz <= 2 ? 2 : (max_row_nnz <= 4 ? 4 : (max_row_nnz <= 8 ? 8 : 0)); }
inline bool fixed_width_compiled(int A, int K) { return false CMDP_FIXED_WIDTH_SHAPES(CMDP_FIXED_WIDTH_IS, _); }

// ---- the sweep kernel of one launch ------------------------------------------------------------------------------------
struct DpShape {  // shape statistics of a batch (cmdp_create)
  int A, max_row_nnz, max_state_unique, max_S;
  int64_t max_inst_nnz;
};

// enumerators = the CMDP_STAT_DP_KERNEL codes
enum SweepFamily { SWEEP_K2 = 1, SWEEP_K2R = 2, SWEEP_K2U = 5, SWEEP_K3 = 6, SWEEP_K2W = 7 };

struct SweepChoice {
  int family;        // SweepFamily
  int A, U, K, spt;  // template key of the register-resident families: K2R (A, K, spt), K2U (A, U, K, spt), K2W (A, spt = st_w)
  size_t lds;        // dynamic LDS bytes
  int block;         // threads per workgroup
  bool csr_lds;      // K2: the CSR lives in LDS (otherwise it is streamed from L2/HBM every sweep)
  bool reg() const { return family == SWEEP_K2R || family == SWEEP_K2U || family == SWEEP_K2W; }
};

// LDS a K2 workgroup needs before any CSR: Va, Vb and the reduction slots
inline size_t k2_value_lds(int max_S) { return 2 * sizeof(float) * (size_t)max_S + sizeof(float) * 4 * (kDpBlock / 64); }

// Which kernel sweeps a batch of shape `s`: `forced` is the handle's CMDP_OPT_DP_KERNEL, `diam` the diameter's solves
// (one per target, workgroup / wavefront kernels only).  CMDP_ERR_UNSUPPORTED when a forced family has no instantiation
// for the shape, or the instance does not fit LDS.
inline int pick_sweep(const DpShape& s, int mode, bool diam, int scheme, int forced, SweepChoice* out) {
  SweepChoice& c = *out = SweepChoice{};
  const int A = c.A = s.A;
  if (scheme == CMDP_SCHEME_JACOBI && !diam && forced != DP_KERNEL_K2) {
    // register-resident CSR (K2R) when the shapes fit one of the compiled instantiations
    const int K = c.K = s.max_row_nnz <= 4 ? 4 : (s.max_row_nnz <= 8 ? 8 : 0);
    const int spt = c.spt = s.max_S <= 256 ? 1 : (s.max_S <= 512 ? 2 : (s.max_S <= 1024 ? 4 : 0));
    c.lds = 2 * sizeof(float) * 256 * (size_t)std::max(spt, 1) + sizeof(float) * 16;  // Va, Vb at fixed offsets
    c.block = 256;
    // K2U when the states' rows share their successors: U gathers instead of A x K (option 5 forces it, 2 forbids it)
    const int U = c.U = s.max_state_unique == 0 ? 0 : (s.max_state_unique <= 5 ? 5 : (s.max_state_unique <= 8 ? 8 : 0));
    const bool want_u = U > 0 && K > 0 && spt > 0 && spt * U <= 20 && forced != DP_KERNEL_K2R &&
                        (forced == DP_KERNEL_K2U || forced == DP_KERNEL_K2W || 2 * U <= A * K);
    if (forced == DP_KERNEL_K2U && !want_u)
      return fail(CMDP_ERR_UNSUPPORTED, "no distinct-successor instantiation (A=%d, %d distinct successors per state, %d states)",
                  A, s.max_state_unique, s.max_S);
    // K2W (one wavefront per instance, 5..7 states per lane): the batches the reference's scheme rule sends to Jacobi
    // sweeps start at ~260 states, and up to 448 the whole instance fits a wavefront's registers.  Option 7 forces it,
    // 5 keeps K2U.
    const int sptw = (s.max_S + 63) / 64;
    const bool want_w = want_u && U == 5 && K == 4 && sptw <= 7 && (forced == DP_KERNEL_K2W || (forced == DP_KERNEL_AUTO && sptw >= 5));
    if (forced == DP_KERNEL_K2W && !want_w)
      return fail(CMDP_ERR_UNSUPPORTED, "no one-wavefront instantiation (A=%d, %d distinct successors per state, %d non-zeros/row, %d states)",
                  A, s.max_state_unique, s.max_row_nnz, s.max_S);
    if (want_w) {
      const int st_w = sptw <= 5 ? 5 : sptw;
      if (k2w_compiled(A, st_w, mode)) {
        c.family = SWEEP_K2W; c.spt = st_w; c.lds = 2 * sizeof(float) * 64 * (size_t)st_w; c.block = 64;
        return CMDP_OK;
      }
      if (forced == DP_KERNEL_K2W)
        return fail(CMDP_ERR_UNSUPPORTED, "no one-wavefront instantiation for A=%d, %d states per lane%s", A, st_w,
                    mode == DP_PE ? " (policy evaluation)" : "");
    }
    if (want_u) {
      if (k2u_compiled(A, U, K, spt)) { c.family = SWEEP_K2U; return CMDP_OK; }
      if (forced == DP_KERNEL_K2U)
        return fail(CMDP_ERR_UNSUPPORTED, "no distinct-successor instantiation for A=%d, U=%d, %d non-zeros/row, %d states", A, U, s.max_row_nnz, s.max_S);
    }
    if (k2r_compiled(A, K, spt)) { c.family = SWEEP_K2R; return CMDP_OK; }
    if (forced == DP_KERNEL_K2R)
      return fail(CMDP_ERR_UNSUPPORTED, "no register-resident instantiation for A=%d, %d non-zeros/row, %d states", A, s.max_row_nnz, s.max_S);
  }
  if (scheme == CMDP_SCHEME_JACOBI) {
    const size_t base = k2_value_lds(s.max_S);
    const size_t csr = sizeof(int32_t) * ((size_t)s.max_S * A + 1) + 8 * (size_t)s.max_inst_nnz + sizeof(float) * (size_t)s.max_S * A;
    if (base > (size_t)kLdsBudget)
      return fail(CMDP_ERR_UNSUPPORTED, "instance with %d states does not fit the LDS-resident sweep (2*4*S > 160 KiB)", s.max_S);
    // CSR in LDS when two workgroups still fit on a CU
    c.family = SWEEP_K2;
    c.csr_lds = base + csr <= (size_t)kLdsBudget / 2;
    c.lds = c.csr_lds ? base + csr : base;
    c.block = kDpBlock;
  } else {
    c.family = SWEEP_K3;
    c.lds = sizeof(float) * (size_t)s.max_S;
    c.block = 64;
    if (c.lds > (size_t)kLdsBudget)
      return fail(CMDP_ERR_UNSUPPORTED, "instance with %d states does not fit the LDS-resident sweep", s.max_S);
  }
  return CMDP_OK;
}

// ---- the kernels of one continuous diameter: pick_diameter_path / _cluster / _lanes ---------------------------------------------------------------
// CMDP_STAT_DIAMETER_KERNEL (include/cmdp.h documents the encoding): family, wavefronts per group or workgroups per
// cluster, and a flag -- K2: the CSR lives in LDS; K5C: the barriers are XCD-scope
enum DiamFamily { DIAM_K2 = 1, DIAM_K3 = 2, DIAM_K5S_ELL = 3, DIAM_K5S_CSR = 4, DIAM_K5C = 5, DIAM_K5T = 6 };
constexpr int diam_code(int family, int n, bool flag) { return family * 1000 + n * 10 + (flag ? 1 : 0); }

constexpr int kK5tRmax = 48;  // tile rows per cluster: 6 wavefronts x 48 rows x 256 B = 72 KiB of LDS, two workgroups per CU
constexpr int kK5tNw = 6;
constexpr int kK5cCluster = 16;  // workgroups per K5C cluster unless CMDP_K5C names another compiled size
#define CMDP_K5C_SIZES(X) X(8) X(16) X(32)
#define CMDP_K5C_IS(CLT) || CL == CLT
inline bool k5c_compiled(int CL, int A, int K) { return (false CMDP_K5C_SIZES(CMDP_K5C_IS)) && fixed_width_compiled(A, K); }

// The CMDP_K5* environment switches (tuning aids), as diam_switches of cmdp.hip read them
struct DiamSwitches {
  int k5c;                  // CMDP_K5C: -1 unset, 0 switches K5C off, CL > 0 chooses the cluster size and overrides the back-off
  int k5s_nw;               // CMDP_K5S_NW: wavefronts per group of K5S-ELL (0: by rule)
  bool agent_scope;         // CMDP_K5C_SCOPE=agent: skip the launch with XCD-scope barriers
  long long timeout_ticks;  // CMDP_K5C_TIMEOUT_TICKS: the barriers' time limit, 100 MHz wall clock (the driver's, no picker reads it)
  int k5s_cluster;          // CMDP_K5S_CLUSTER: states per cluster of the locality order, 0 keeps the caller's order, -1 unset (ensure_ell's)
};

// Path of a cmdp_diameter call: the lanes kernels (64 targets per workgroup, value vectors in HBM) on request, and when
// the value vectors of an instance do not fit the workgroup kernel's LDS; otherwise one workgroup or wavefront per target,
// which pick_sweep(..., diam = true, ...) chooses.  cmdp_diameter_range always takes the lanes.
enum DiamPath { DIAM_PATH_WORKGROUP, DIAM_PATH_LANES };
inline DiamPath pick_diameter_path(const DpShape& s, int scheme, int forced) {
  const bool lanes = scheme == CMDP_SCHEME_JACOBI && (forced == DP_KERNEL_K5S || forced == DP_KERNEL_K5S_CSR || forced == DP_KERNEL_K5T ||
                                                      k2_value_lds(s.max_S) > (size_t)kLdsBudget);
  return lanes ? DIAM_PATH_LANES : DIAM_PATH_WORKGROUP;
}

// K5C (clusters of workgroups per group, k_diam_cluster) for instances large enough for the value rows to overflow the
// L2s: the cluster size a lanes call tries first, 0 for none.  `relabel`: the largest instance reaches
// CMDP_OPT_DIAMETER_RELABEL_MIN_STATES; `backing_off`: an earlier call gave up and the handle still skips (a give-up costs
// every workgroup its 2-second spin).  Only compiled (CL, A, K) are returned.
inline int pick_diameter_cluster(const DpShape& s, int forced, bool relabel, int cus, const DiamSwitches& sw, bool backing_off, bool any_group) {
  const int A = s.A, K = fixed_width_K(s.max_row_nnz), CL = sw.k5c > 0 ? sw.k5c : kK5cCluster;
  const bool wanted = forced != DP_KERNEL_K5S_CSR && forced != DP_KERNEL_K5T && sw.k5c != 0 && cus % (8 * CL) == 0 && relabel &&
                      !backing_off && any_group;
  return wanted && k5c_compiled(CL, A, K) ? CL : 0;
}

// The lanes kernel that solves the groups K5C did not: K5T (value rows gathered into LDS tiles per cluster of states) on
// request only -- at C5 it halves the HBM traffic of K5S and is bit-equal, but runs 2.3 s against 2.05 s, see DESIGN.md;
// K5S over the fixed-width rows when (A, K) is compiled, unless option 4 keeps the generic CSR walker.
inline int lanes_family(const DpShape& s, int forced) {
  if (!fixed_width_compiled(s.A, fixed_width_K(s.max_row_nnz)) || forced == DP_KERNEL_K5S_CSR) return DIAM_K5S_CSR;
  return forced == DP_KERNEL_K5T ? DIAM_K5T : DIAM_K5S_ELL;
}

struct LanesChoice { int family, nw, code; };  // DIAM_K5T / DIAM_K5S_ELL / DIAM_K5S_CSR, wavefronts per group, diam_code(...)

// ... and its width for a launch of `n_groups` groups.  K5S-ELL: 8 wavefronts fill the chip when there are at least two
// groups per CU; with fewer groups than CUs (a rank's share of C5 on an 8-GPU node: 98 groups) the launch lasts as long as
// ONE group, so each group gets 16 -- and 16 with the locality order (`ell_relabelled`: the handle's fixed-width rows are
// stored relabelled, which CMDP_K5S_CLUSTER = 0 prevents): half as many groups share an L2, so a row is still there when
// the next chunk wants it (C5 1.83 -> 1.75 s).
// (two targets per lane -- value rows of 128 floats, the row walk paid once per 128 targets -- measured 2.47 s against
// 1.79 s at C5: the wider rows halve every group's window in L2; not kept)
inline LanesChoice pick_diameter_lanes(const DpShape& s, int forced, bool ell_relabelled, int64_t n_groups, int cus, const DiamSwitches& sw) {
  const int family = lanes_family(s, forced);
  const int ell_nw = sw.k5s_nw ? sw.k5s_nw : ((n_groups <= (int64_t)cus || ell_relabelled) ? 16 : 8);
  const int nw = family == DIAM_K5T ? kK5tNw : (family == DIAM_K5S_ELL && (ell_nw == 16 || ell_nw == 4)) ? ell_nw : 8;
  return {family, nw, diam_code(family, nw, false)};
}
