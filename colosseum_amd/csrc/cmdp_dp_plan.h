// cmdp_dp_plan.h -- host-side choice of the dynamic-programming sweep kernels (K2, K2R, K2U, K2W, K3; K5S / K5T / K5C).
//
// The compiled instantiations of every template family are listed here once, as X-macro lists: the launch switches of
// cmdp.hip and the predicates "is this shape compiled" below expand the same lists.  pick_sweep decides which kernel
// serves a batch of a given shape.  Nothing here makes a HIP call.  Included by cmdp.hip after the kernel headers.
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
