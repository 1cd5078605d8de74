// cmdp.hip -- C ABI (include/cmdp.h) over the HIP kernels of cmdp_kernels.h.  gfx950 only.
#include "../../include/cmdp.h"

#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <cstdlib>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <limits>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

extern char** environ;

#include <new>
#include "cmdp_kernels.h"
#include "cmdp_tracker.h"
#include "cmdp_logged_loop.h"
#include "cmdp_k1s.h"
#include "cmdp_k1t.h"
#include "cmdp_k1u.h"
#include "cmdp_k1e.h"
#include "cmdp_k1e_pair.h"
#include "cmdp_rollout_plan.h"
#include "cmdp_dp_plan.h"
#include "cmdp_agent.h"
#include "cmdp_actions.h"
#include "cmdp_chain.h"
#include "cmdp_chain_plan.h"
#include "cmdp_batch.h"
#include "cmdp_evi.h"
#include "cmdp_model_vi.h"
#include "cmdp_ucrl2.h"
#include "cmdp_psrl.h"
#include "cmdp_psrlc.h"
#include "cmdp_psrlo.h"
#include "cmdp_psrlo_vi.h"
#include "cmdp_map_vi.h"
#include "cmdp_map_dvi.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail(CMDP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// Device buffer that only grows: hipFree (and often hipMalloc) synchronises the WHOLE device, which would serialise
// handles that run concurrently on their own streams (benchmark runner: one host thread per device batch), so steady-state
// calls must not allocate.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;    // logical size of the current contents
  size_t cap = 0;  // allocated elements
  hipError_t alloc(size_t count) {
    if (count <= cap) {
      n = count;
      return hipSuccess;
    }
    release();
    if (count == 0) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
    if (e == hipSuccess) { n = count; cap = count; }
    return e;
  }
  hipError_t upload(const T* src, size_t count, hipStream_t s) {
    hipError_t e = alloc(count);
    if (e != hipSuccess || count == 0) return e;
    return hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s);
  }
  hipError_t download(T* dst, size_t count, hipStream_t s) const {
    return count ? hipMemcpyAsync(dst, p, count * sizeof(T), hipMemcpyDeviceToHost, s) : hipSuccess;
  }
  hipError_t zero(hipStream_t s) { return n ? hipMemsetAsync(p, 0, n * sizeof(T), s) : hipSuccess; }
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(cap, o.cap); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    cap = 0;
  }
  ~DevBuf() { release(); }
};

// Lease of the workspace of a batch solver that takes no environment handle (cmdp_gth, cmdp_extended_vi,
// cmdp_vi_discounted_model, cmdp_vi_episodic_dense, cmdp_vi_episodic_map): the solver's own struct `Ws` of DevBufs and a
// non-blocking stream, one pair per device.  acquire() takes the solver's mutex, refuses when no device is visible, and
// finds or creates the pair of the current device; the mutex is held until the lease goes out of scope, so the calls of one
// solver are serialised.  Every solver names a Ws type of its own and so has its own pool, mutex and streams: host threads
// in different solvers do not wait for each other.  The workspaces are reused across calls (no per-call hipMalloc / hipFree:
// both synchronise the device) and deliberately leaked at exit (a static destructor's hipFree would run while the runtime
// is being torn down).  A pair whose stream cannot be created is not kept: that call fails and the next one tries again.
template <typename Ws>
struct DeviceWorkspace {
  Ws* ws = nullptr;
  hipStream_t st = nullptr;
  std::unique_lock<std::mutex> lock;
  Ws* operator->() const { return ws; }
  int acquire() {
    struct Slot { Ws ws; hipStream_t st = nullptr; };
    static std::mutex mu;
    static std::map<int, Slot*>* all = new std::map<int, Slot*>;
    lock = std::unique_lock<std::mutex>(mu);
    int ndev = 0, dev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(CMDP_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipGetDevice(&dev));
    Slot*& slot = (*all)[dev];
    if (!slot) {
      hipStream_t created = nullptr;
      HIP_TRY(hipStreamCreateWithFlags(&created, hipStreamNonBlocking));
      slot = new Slot;
      slot->st = created;
    }
    ws = &slot->ws;
    st = slot->st;
    return CMDP_OK;
  }
};

// Page-locked host memory for the per-log read-backs of the logged loop.  Only grows, like DevBuf.
template <typename T>
struct PinnedBuf {
  T* p = nullptr;
  size_t cap = 0;
  int alloc(size_t n) {
    if (p && n <= cap) return CMDP_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr, cap = 0;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(T) * std::max<size_t>(n, 1), 0));
    cap = std::max<size_t>(n, 1);
    return CMDP_OK;
  }
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
};

}  // namespace

struct cmdp {
  int device = 0;
  hipStream_t stream = nullptr;
  int B = 0, A = 0, H = 0, rng_mode = 0, layout = 0;
  double rmin = 0, rmax = 1;
  int64_t n_states = 0, n_rows = 0, n_entries = 0, n_csr = 0, n_slots = 0;
  bool has_env = false, has_dp = false;
  bool sample_beta = false;  // Beta rewards drawn on the device (CMDP_RNG_PHILOX without CMDP_FLAG_REWARD_MEANS)
  bool beta_gammas = false;  // CMDP_FLAG_BETA_GAMMAS
  // CMDP_FLAG_REWARD_CACHE: the reference's per-triple caches of 5000 samples from the MDP's own numpy stream
  // (cmdp_reward_cache.h): blocks in HBM, drawn on the host whenever an instance parks
  bool reward_cache = false, rc_streams_set = false;
  std::vector<uint8_t> h_rkind;
  std::vector<double> h_rp0, h_rp1;
  std::vector<int32_t> h_canon;
  std::vector<cmdp_rc::NumpyStream> rc_streams;   // [B] BaseMDP._rng of every instance, where construction left it
  std::vector<double*> rc_blk_h;                  // [E] host mirror of the block pointers
  std::vector<double*> rc_chunks;                 // pool of blocks: chunks of rc_chunk_blocks blocks each
  size_t rc_chunk_blocks = 0, rc_next_block = 0;  // blocks handed out so far
  int rc_cap = 0;                                 // blocks one install pass can stage
  int64_t rc_fills = 0, rc_rounds = 0;            // CMDP_STAT_REWARD_FILLS / _ROUNDS
  double rc_fill_ms = 0.0, rc_round_ms = 0.0;     // CMDP_STAT_REWARD_FILL_MS / _ROUND_MS
  double* rc_stage_h = nullptr;                   // pinned [rc_cap][5000]
  double** rc_dst_h = nullptr;                    // pinned [rc_cap]
  int32_t* rc_ent_h = nullptr;                    // pinned [rc_cap]
  int32_t* rc_list_h = nullptr;                   // pinned [B]
  int32_t* rc_pend_h = nullptr;                   // pinned [B]
  DevBuf<int32_t> d_rc_canon, d_rc_pos, d_rc_pend_e, d_rc_pend_prev, d_rc_pend_act, d_rc_park_count, d_rc_park_list, d_rc_ent;
  DevBuf<double*> d_rc_blk, d_rc_dst;
  DevBuf<long long> d_rc_left;
  DevBuf<double> d_rc_stage;
  RewardCache rcache() {
    RewardCache c{};
    c.canon = d_rc_canon.p; c.blk = d_rc_blk.p; c.pos = d_rc_pos.p; c.pend_e = d_rc_pend_e.p; c.pend_prev = d_rc_pend_prev.p;
    c.pend_act = d_rc_pend_act.p; c.park_count = d_rc_park_count.p; c.park_list = d_rc_park_list.p; c.left = d_rc_left.p;
    return c;
  }
  std::vector<int64_t> state_off;  // host copy
  std::vector<int64_t> csr_nnz;    // per instance
  int max_S = 0;
  int64_t max_inst_nnz = 0;
  int max_row_nnz = 0;
  int max_state_unique = 0;  // distinct successor columns of a state over its A rows (0: not computed / rows unsorted)
  bool known_reset = false;  // every instance is known to be past reset() (cmdp_rollout_async checks once, cmdp_step clears)
  hipEvent_t ev_dp0 = nullptr, ev_dp1 = nullptr;  // around the sweep kernel of the last discounted solve (cmdp_stat)
  hipEvent_t ev_row[2] = {nullptr, nullptr};      // logged loop: policy + state snapshot taken | evaluation of the row complete
  DevBuf<int32_t> d_cur_snap;                     // logged loop: current states at the row (the solve runs beside the next interval)
  int last_dp_kernel = 0;     // CMDP_STAT_DP_KERNEL: 1 K2, 2 K2R, 5 K2U, 7 K2W, 6 K3 (Gauss-Seidel) -- SweepFamily
  PinnedBuf<int32_t> pin_status;   // discounted(): the status words of a solve that stores into page-locked result arrays
  int dp_kernel = 0;  // CMDP_OPT_DP_KERNEL: DP_KERNEL_AUTO .. DP_KERNEL_K2W (cmdp_dp_plan.h; 3, 4, 6: diameter only)

  DevBuf<int64_t> d_state_off, d_entry_base, d_start_off, d_csr_ptr;
  DevBuf<RowDesc> d_row;
  DevBuf<int32_t> d_sp_next, d_start_state, d_start_slot, d_mt_pos, d_cur, d_h, d_visits_s, d_visits_sa, d_csr_col,
      d_flag, d_status, d_i32_scratch, d_last_start, d_prev_start;
  DevBuf<double> d_sp_cum, d_sp_reward, d_start_cum, d_f64_scratch, d_sp_rp0, d_sp_rp1;
  DevBuf<uint8_t> d_sp_rkind;
  DevBuf<uint2> d_key;
  DevBuf<uint32_t> d_mt;
  DevBuf<uint8_t> d_need_reset, d_u8_scratch;
  DevBuf<unsigned long long> d_ntrans, d_nreset;
  DevBuf<float> d_csr_val, d_R, d_Rov, d_pi, d_Q, d_V, d_per_target, d_Ev, d_out;
  DevBuf<int64_t> d_sweeps;
  DevBuf<int8_t> d_actions8;
  // CMDP_POLICY_RANDOM_REFERENCE (cmdp_actions.h): RandomState(seed) of every instance in numpy's representation, the action
  // bits of a K1E segment, and K16's failure flag (raised on the device, read at the next synchronisation)
  DevBuf<uint32_t> d_as_key;
  DevBuf<int32_t> d_as_pos, d_as_fail;
  DevBuf<uint4> d_abits;
  bool as_set = false, as_unchecked = false;
  hipEvent_t ev_as[2] = {nullptr, nullptr};   // around K16 of the last segment of the last K1E launch under that policy
  DevBuf<int32_t> d_tr_obs, d_last_obs;
  DevBuf<double> d_tr_rew, d_rsum;
  DevBuf<uint8_t> d_tr_type, d_mask;
  // LDS-resident rollout of stochastic-dynamics batches (K1S)
  bool k1s_ok = false;
  K1sPlan k1s{};
  size_t k1s_bytes = 0;
  DevBuf<uint4> d_k1s_dict;
  DevBuf<uint8_t> d_k1s_pat, d_k1s_rc;
  DevBuf<uint16_t> d_k1s_sets, d_k1s_shape16;
  DevBuf<double> d_k1s_patterns, d_k1s_rvals;
  // LDS-resident rollout (K1L)
  bool lds_ok = false;
  int lds_G1 = 0, lds_G2 = 0;  // LDS capacity in instances per workgroup at one / two workgroups per CU
  int lds_succ_bits = 0, lds_per_cu = 0;   // (cmdp_det_plan) bits of a row base; workgroups per CU of the chosen candidate
  int tmpl_cap = 0, k1u_cap = 0;           // (cmdp_det_plan) LDS capacity in instances per workgroup of K1T / K1U
  int cus = 256;
  int rollout_kernel = 0;  // CMDP_OPT_ROLLOUT_KERNEL
  LdsPlan lds_plan{};
  size_t lds_bytes = 0;
  bool tmpl_auto = false;
  bool tmpl_ok = false;      // K1T: one shared successor table per workgroup + per-instance action-swap bits
  TmplPlan tmpl_plan{};
  size_t tmpl_lds = 0;
  DevBuf<uint16_t> d_tmpl_words;
  DevBuf<uint8_t> d_swap_bits;
  // K1U: K1T with the trace streamed to HBM and histogrammed by a second kernel (all instances of a CU resident at once)
  bool k1u_ok = false, k1u_auto = false;
  K1uPlan k1u{};
  size_t k1u_lds = 0;
  DevBuf<uint4> d_k1u_trace;
  DevBuf<int32_t> d_k1u_resets;
  // CMDP_STAT_ROLLOUT_KERNEL_MS / _HIST_KERNEL_MS: around the two kernels of the last segment of the last K1U or K1E launch
  // (events 0-1: the rollout kernel; 1-2: the second kernel on the handle's stream, or 3-4 on the second stream: ev_time_aux)
  hipEvent_t ev_time[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool ev_time_aux = false;
  // K1E: the episode-parallel rollout (cmdp_k1e.h): lane = (instance, episode), private {successor | count} tables in LDS
  bool k1e_ok = false;
  K1ePlan k1e{};
  size_t k1e_lds = 0;
  DevBuf<uint32_t> d_etab;
  DevBuf<uint2> d_k1e_codes[2];    // two sets: the reward scan of one segment runs (second stream) under the walk of the next
  DevBuf<int32_t> d_k1e_h0b;       // second seg_h0 buffer
  struct {                         // the second stream: K1E's reward scans (scan of code set i after the walk that wrote it)
    hipStream_t stream = nullptr;
    hipEvent_t walk[2] = {nullptr, nullptr}, scan[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    int64_t seq = 0;               // scans enqueued: the next segment takes set seq & 1
    bool pending = false;          // the handle's stream has not waited for the last scan yet
  } aux;                           // (cmdp_qlearning_run_logged evaluates on the stream too, after bind() has settled it)
  DevBuf<int2> d_k1e_dep;          // departure counts of the K1E launches since the last fold (k_epi_fold)
  DevBuf<int32_t> d_k1e_dep_res, d_vis_ovf;
  int64_t vis_bound = 0;           // upper bound of every device visit counter (int32): CMDP_ERR_OVERFLOW guard
  bool k1e_pending = false;        // d_k1e_dep holds counts the visit counters do not have yet
  int64_t k1e_pending_steps = 0;   // transitions per instance since the last fold (the departure image is int32)
  DevBuf<int32_t> d_k1e_h0;
  // K1E's pair form (cmdp_k1e_pair.h): two transitions per step, for launches of whole episodes walked from reset
  bool k1e_pair_ok = false;        // the batch has a pair plan (plan_k1e_pair) and CMDP_K1E_PAIR is not 0
  int k1e_sp2 = 0, k1e_n_even = 0;
  size_t k1e_pair_lds = 0;
  int k1e_last_form = 0;           // the form the last K1E launch took: 0 none yet, 1 single, 2 pair
  DevBuf<uint32_t> d_ptab;
  DevBuf<uint16_t> d_pinv;
  DevBuf<int2> d_k1e_dep2;         // pair counts of the pair-form launches since the last fold
  // every instance is at its start state with in-episode time 0: set by an unmasked cmdp_reset, kept by a rollout of a
  // multiple of H transitions, cleared by whoever takes the mutable tables (env()) for anything else
  bool at_start = false;
  DevBuf<float> d_gp_q, d_gp_p;  // cmdp_greedy_policy_episodic workspace
  // K5S workspace (large-instance diameter)
  DevBuf<float> d_dl_v, d_ell_val;
  DevBuf<int32_t> d_ell_col, d_ell_newof;
  int ell_K = 0;
  int64_t relabel_min_states = 8192;  // CMDP_OPT_DIAMETER_RELABEL_MIN_STATES
  bool ell_relabelled = false;  // the fixed-width rows are stored in relabel_states' order (d_ell_newof: original -> new label)
  // K5T cluster tables (large-instance diameter with LDS tiles)
  DevBuf<int32_t> d_tl_c0, d_tl_ncl, d_tl_n, d_tl_R, d_tl_rows, d_tl_lcol;
  DevBuf<float> d_tl_val;
  int tile_K = 0;          // K the tables were built for (0: not built)
  double tile_rows_per_state = 0.0;  // tile rows gathered per state and sweep (1 + halo/cluster)
  DevBuf<int32_t> d_dl_inst, d_dl_t0, d_dl_cnt;
  DevBuf<int64_t> d_dl_voff;
  DevBuf<float> d_k5c_red;          // K5C: the clusters' partial reductions
  DevBuf<unsigned int> d_k5c_bar;   // K5C: barrier counters + error flag
  int64_t k5c_launches = 0, k5c_timeouts = 0;
  int k5c_skip = 0, k5c_backoff = 0;   // after a give-up K5C is skipped for `k5c_backoff` calls (8, 16, ... 1024), then tried again
  bool k5c_agent_scope = false;     // K5C: a cluster was found spread over XCDs once -- agent-scope barriers from then on
  int last_diam_kernel = 0;         // CMDP_STAT_DIAMETER_KERNEL: diam_code(...) of the last launch of the last diameter call
  size_t dl_ws_bytes = (size_t)24 << 30;  // value arrays of the target groups in flight per launch
  // observation tables (k_emit)
  DevBuf<float> d_obs_table, d_obs_out, d_obs_chol;
  DevBuf<unsigned long long> d_n_obs;
  int obs_F = 0, obs_time_indexed = 0;
  // cmdp_average_reward workspace (K9)
  int mixing_path = 0;       // CMDP_OPT_MIXING_PATH: 0 auto, 1 matrix powers, 2 stepping
  bool chain_exact = false;  // CMDP_OPT_CHAIN_EXACT_ORDER
  DevBuf<double> d_ch_work, d_ch_avg;
  DevBuf<int64_t> d_ch_off;
  DevBuf<int32_t> d_ch_kind, d_ch_ncls, d_ch_act, d_ch_start, d_ch_idx;
  DevBuf<uint8_t> d_ch_mask;
  // K9F: the plan of every instance (plan_chains of cmdp_chain_plan.h), built at the first average-reward call that wants it
  struct ChainFastState {
    bool built = false, any = false;  // any: some instance has a plan
    bool ran = false;                 // K9F was launched by the last average-reward call (its `slow` flags are that call's)
    DevBuf<int32_t> rank, cptr, nrounds, rptr, piv;
    DevBuf<int64_t> cbase, rbase;
    DevBuf<uint16_t> cand;
    DevBuf<uint8_t> slow;
    ChainFast args() const { return {rank.p, cptr.p, cbase.p, cand.p, nrounds.p, rbase.p, rptr.p, piv.p, slow.p}; }
  } cf;
  // UCRL2 agents on this handle (cmdp_ucrl2_*): CMDP_STAT_UCRL2_*
  // ... their `env` fields: cleared by cmdp_destroy, so that an agent destroyed AFTER its environment (garbage collection
  // picks the order) frees its own memory and touches nothing of the handle
  std::vector<cmdp_t**> uc_backrefs;
  int64_t uc_rounds = 0, uc_solves = 0;
  double uc_round_ms = 0.0, uc_wait_ms = 0.0;
  double uc_policy_ms = 0.0;   // CMDP_STAT_UCRL2_POLICY_KERNEL_MS: the last K14 launch of an agent of this handle
  int64_t uc_policy_solved = 0, uc_policy_reused = 0;   // CMDP_STAT_UCRL2_POLICY_SOLVED / _REUSED: instances, all requests together
  DevBuf<int32_t> d_uc_unconverged;
  // PSRL agents on this handle (cmdp_psrl_*): CMDP_STAT_PSRL_*
  int64_t ps_rounds = 0, ps_solves = 0;
  double ps_sample_ms = 0.0, ps_vi_ms = 0.0, ps_ref_ms = 0.0;
  double ps_policy_ms = 0.0;   // CMDP_STAT_PSRL_POLICY_KERNEL_MS: the last K15 launch of an agent of this handle
  double ps_sample_bytes = 0.0;   // CMDP_STAT_PSRL_SAMPLE_BYTES: what the optimistic agent's sample routes hold (K18 / K19)
  int ps_sample_solver = 0;       // CMDP_STAT_PSRL_SAMPLE_SOLVER: the route of the optimistic agent's last round
  DevBuf<unsigned long long> d_ps_tally;   // continuous PSRL (K13): solves that did not converge, sweeps of the last round
  DevBuf<float> d_dense;  // CMDP_LAYOUT_DENSE: [R][dense_spad]
  int dense_spad = 0;
  DevBuf<uint16_t> d_next16;
  DevBuf<uint8_t> d_rcode;
  DevBuf<double> d_rvals;

  EnvTables env() {
    at_start = false;   // (the kernel that gets these pointers may move an instance: whoever knows better sets the flag again)
    EnvTables t{};
    t.B = B; t.A = A; t.H = H; t.rng_mode = rng_mode;
    t.rscale = rmax - rmin; t.rmin = rmin; t.beta_gammas = beta_gammas ? 1 : 0;
    t.state_off = d_state_off.p; t.entry_base = d_entry_base.p; t.row = d_row.p;
    t.sp_next = d_sp_next.p; t.sp_cum = d_sp_cum.p; t.sp_reward = d_sp_reward.p;
    t.sp_rkind = d_sp_rkind.p; t.sp_rp0 = d_sp_rp0.p; t.sp_rp1 = d_sp_rp1.p;
    t.start_off = d_start_off.p; t.start_state = d_start_state.p; t.start_cum = d_start_cum.p;
    t.start_slot = d_start_slot.p; t.philox_key = d_key.p; t.mt = d_mt.p; t.mt_pos = d_mt_pos.p;
    t.cur = d_cur.p; t.hstep = d_h.p; t.need_reset = d_need_reset.p; t.n_trans = d_ntrans.p; t.n_reset = d_nreset.p;
    t.visits_s = d_visits_s.p; t.visits_sa = d_visits_sa.p; t.last_start = d_last_start.p; t.prev_start = d_prev_start.p;
    return t;
  }
};

namespace {

// The device visit counters are int32.  No counter can grow by more than two per transition (the arrival and, when the
// episode ends there, the reset), so `vis_bound` bounds all of them; a call that could carry one past 2^31 - 1 is refused.
int visits_check(const cmdp_t* h, int64_t n_transitions) {
  if (h->vis_bound + 2 * n_transitions > 0x7fffffffLL)
    return fail(CMDP_ERR_OVERFLOW, "a visit counter (int32 on the device) could wrap: up to %lld counted since the last "
                "cmdp_reset_visits / cmdp_set_visits, %lld more transitions asked for -- read the counters (cmdp_visits) and reset them",
                (long long)h->vis_bound, (long long)n_transitions);
  return CMDP_OK;
}

// ... and the call's transitions are added to the bound once its kernels may have run: after success, or after a HIP error
// (one of several launches can fail); a call refused with any other code has stepped nothing
int visits_commit(cmdp_t* h, int64_t n_transitions, int rc = CMDP_OK) {
  if (rc == CMDP_OK || rc == CMDP_ERR_HIP) h->vis_bound += 2 * n_transitions;
  return rc;
}

inline int grid_for(int64_t n, int block) { return (int)((n + block - 1) / block); }

template <typename K>
int set_lds(K kernel, size_t bytes) {
  if (bytes > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return CMDP_OK;
}

int k1e_fold(cmdp_t* h) {
  if (!h->k1e_pending) return CMDP_OK;
  K1ePlan e = h->k1e;
  e.dep = h->d_k1e_dep.p;
  e.dep_res = h->d_k1e_dep_res.p;
  e.dep2 = h->d_k1e_dep2.p;   // (null: no launch took the pair form)
  const size_t lds = k1e_fold_lds_bytes(e);
  if (int rc = set_lds(k_epi_fold, lds)) return rc;
  const bool at_start = h->at_start;   // (the fold moves no instance)
  hipLaunchKernelGGL(k_epi_fold, dim3(grid_for(h->B, K1E_NI)), dim3(K1E_THREADS), lds, h->stream, h->env(), e, h->d_vis_ovf.p);
  h->at_start = at_start;
  HIP_TRY(hipGetLastError());
  h->k1e_pending = false;
  h->k1e_pending_steps = 0;
  return CMDP_OK;
}

// the handle's stream waits for the reward scan K1E still owes on the second stream: before anything reads the reward sums
int k1e_scan_join(cmdp_t* h) {
  if (h->aux.pending) {
    HIP_TRY(hipStreamWaitEvent(h->stream, h->aux.scan[(h->aux.seq + 1) & 1], 0));
    h->aux.pending = false;
  }
  return CMDP_OK;
}

// ... and also folds the departure counts K1E has accumulated into the visit counters: what every other kernel and every
// read of the counters needs first
int k1e_settle(cmdp_t* h) {
  if (int rc = k1e_scan_join(h)) return rc;
  return k1e_fold(h);
}

int bind(cmdp_t* h, bool settle = true) {
  if (!h) return fail(CMDP_ERR_INVALID, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  return settle ? k1e_settle(h) : CMDP_OK;
}

}  // namespace

// ---- cmdp_create, step by step ----------------------------------------------------------------------------------------
// The description's shape; *max_S: the largest instance.
static int check_desc(const cmdp_desc* d, int* max_S) {
  if (d->n_instances < 1 || d->n_actions < 1 || d->n_actions > 64 || d->horizon < 0)
    return fail(CMDP_ERR_INVALID, "n_instances/n_actions/horizon out of range (1 <= A <= 64)");
  if (d->rng_mode != CMDP_RNG_MT_COMPAT && d->rng_mode != CMDP_RNG_PHILOX) return fail(CMDP_ERR_INVALID, "rng_mode");
  if (d->layout != CMDP_LAYOUT_CSR && d->layout != CMDP_LAYOUT_DENSE) return fail(CMDP_ERR_INVALID, "layout");
  if (d->layout == CMDP_LAYOUT_DENSE && (d->rng_mode != CMDP_RNG_PHILOX || !d->sp_ptr || !d->csr_ptr))
    return fail(CMDP_ERR_INVALID, "CMDP_LAYOUT_DENSE needs CMDP_RNG_PHILOX and both halves of the description "
                                  "(the float32 rows come from the DP half, rewards and starts from the sampler half)");
  if (!d->state_off) return fail(CMDP_ERR_INVALID, "state_off is required");
  const bool has_env = d->sp_ptr != nullptr, has_dp = d->csr_ptr != nullptr;
  if (!has_env && !has_dp) return fail(CMDP_ERR_INVALID, "neither the sampler half nor the DP half is present");
  if (has_env && (!d->sp_next || !d->sp_cum || !d->sp_reward || !d->start_off || !d->start_state || !d->start_cum))
    return fail(CMDP_ERR_INVALID, "sampler half is incomplete");
  if (has_env && d->rng_mode == CMDP_RNG_MT_COMPAT && (!d->sp_seed || !d->start_seed))
    return fail(CMDP_ERR_INVALID, "MT_COMPAT needs sp_seed and start_seed");
  if (has_dp && (!d->csr_col || !d->csr_val || !d->R)) return fail(CMDP_ERR_INVALID, "DP half is incomplete");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(CMDP_ERR_NO_DEVICE, "no HIP device visible");
  if (d->state_off[0] != 0) return fail(CMDP_ERR_INVALID, "state_off[0] != 0");
  *max_S = 0;
  for (int b = 0; b < d->n_instances; ++b) {
    const int64_t S = d->state_off[b + 1] - d->state_off[b];
    if (S < 1 || S > (1 << 28)) return fail(CMDP_ERR_INVALID, "instance %d has %lld states", b, (long long)S);
    *max_S = std::max<int>(*max_S, (int)S);
  }
  return CMDP_OK;
}

// Reward kinds: deterministic values, Beta rewards drawn on the device, or the reference-exact reward caches.
static int upload_rewards(cmdp_t* h, const cmdp_desc* d) {
  hipStream_t st = h->stream;
  const int B = h->B;
  const int64_t R = h->n_rows, E = h->n_entries;
  bool any_beta = false;
  if (d->sp_rkind)
    for (int64_t e = 0; e < E; ++e) {
      if (d->sp_rkind[e] > 1) return fail(CMDP_ERR_UNSUPPORTED, "unknown reward distribution kind at entry %lld", (long long)e);
      any_beta |= d->sp_rkind[e] == 1;
    }
  if ((d->flags & CMDP_FLAG_REWARD_MEANS) && (d->flags & CMDP_FLAG_REWARD_CACHE))
    return fail(CMDP_ERR_INVALID, "CMDP_FLAG_REWARD_MEANS and CMDP_FLAG_REWARD_CACHE exclude each other");
  h->reward_cache = any_beta && (d->flags & CMDP_FLAG_REWARD_CACHE);
  h->sample_beta = any_beta && !(d->flags & (CMDP_FLAG_REWARD_MEANS | CMDP_FLAG_REWARD_CACHE));
  h->beta_gammas = (d->flags & CMDP_FLAG_BETA_GAMMAS) != 0;
  if (h->reward_cache && (!d->sp_rp0 || !d->sp_rp1 || d->layout != CMDP_LAYOUT_CSR))
    return fail(CMDP_ERR_INVALID, "CMDP_FLAG_REWARD_CACHE needs sp_rp0 / sp_rp1 and the CSR layout");
  if (h->reward_cache && E > 0x7fffffffLL) return fail(CMDP_ERR_UNSUPPORTED, "CMDP_FLAG_REWARD_CACHE: more than 2^31 entries");
  if (h->sample_beta && (d->rng_mode != CMDP_RNG_PHILOX || !d->sp_rp0 || !d->sp_rp1))
    return fail(CMDP_ERR_UNSUPPORTED, "Beta rewards are sampled on the device only in CMDP_RNG_PHILOX mode with sp_rp0/"
                                      "sp_rp1; the reference-exact stream is host side (CMDP_FLAG_REWARD_MEANS)");
  if (!h->reward_cache && !h->sample_beta) return CMDP_OK;
  for (int64_t e = 0; e < E; ++e)
    if (d->sp_rkind[e] == 1 && !(d->sp_rp0[e] > 0.0 && d->sp_rp1[e] > 0.0))
      return fail(CMDP_ERR_INVALID, "Beta parameters must be positive (entry %lld)", (long long)e);
  HIP_TRY(h->d_sp_rkind.upload(d->sp_rkind, E, st));
  if (h->sample_beta) {
    HIP_TRY(h->d_sp_rp0.upload(d->sp_rp0, E, st));
    HIP_TRY(h->d_sp_rp1.upload(d->sp_rp1, E, st));
    return CMDP_OK;
  }
  h->h_rkind.assign(d->sp_rkind, d->sp_rkind + E);
  h->h_rp0.assign(d->sp_rp0, d->sp_rp0 + E);
  h->h_rp1.assign(d->sp_rp1, d->sp_rp1 + E);
  // the reference keys its caches by (node, action, next_node): entries of a row that name the same successor
  // (p_rand adds repeated successors) share one cache -- represented by the first of them
  h->h_canon.resize((size_t)E);
  for (int64_t r = 0; r < R; ++r) {
    const int64_t lo = d->sp_ptr[r], hi = d->sp_ptr[r + 1];
    for (int64_t e = lo; e < hi; ++e) {
      int64_t c = e;
      for (int64_t f = lo; f < e; ++f)
        if (d->sp_next[f] == d->sp_next[e]) { c = f; break; }
      h->h_canon[(size_t)e] = (int32_t)c;
    }
  }
  HIP_TRY(h->d_rc_canon.upload(h->h_canon.data(), E, st));
  HIP_TRY(h->d_rc_blk.alloc(E)); HIP_TRY(h->d_rc_blk.zero(st));
  HIP_TRY(h->d_rc_pos.alloc(E)); HIP_TRY(h->d_rc_pos.zero(st));
  HIP_TRY(h->d_rc_pend_e.alloc(B)); HIP_TRY(hipMemsetAsync(h->d_rc_pend_e.p, 0xff, sizeof(int32_t) * B, st));
  HIP_TRY(h->d_rc_pend_prev.alloc(B)); HIP_TRY(h->d_rc_pend_prev.zero(st));
  HIP_TRY(h->d_rc_pend_act.alloc(B)); HIP_TRY(h->d_rc_pend_act.zero(st));
  HIP_TRY(h->d_rc_park_count.alloc(1)); HIP_TRY(h->d_rc_park_count.zero(st));
  HIP_TRY(h->d_rc_park_list.alloc(B));
  HIP_TRY(h->d_rc_left.alloc(B)); HIP_TRY(h->d_rc_left.zero(st));
  h->rc_blk_h.assign((size_t)E, nullptr);
  h->rc_cap = std::min(B, 1024);
  h->rc_chunk_blocks = (size_t)std::max(256, std::min(B * 8, 4096));  // 10 .. 164 MB per chunk
  HIP_TRY(h->d_rc_stage.alloc((size_t)h->rc_cap * CMDP_RC_BLOCK));
  HIP_TRY(h->d_rc_dst.alloc(h->rc_cap));
  HIP_TRY(h->d_rc_ent.alloc(h->rc_cap));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->rc_stage_h), sizeof(double) * (size_t)h->rc_cap * CMDP_RC_BLOCK, 0));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->rc_dst_h), sizeof(double*) * (size_t)h->rc_cap, 0));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->rc_ent_h), sizeof(int32_t) * (size_t)h->rc_cap, 0));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->rc_list_h), sizeof(int32_t) * (size_t)B, 0));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->rc_pend_h), sizeof(int32_t) * (size_t)B, 0));
  return CMDP_OK;
}

// The sampler half: row descriptors, entry bases and MT slots -- validated on the host so that no kernel can index out
// of range -- and the per-instance state.  *rows and *seeds stay with the caller for the rollout plans and the MT streams.
static int upload_sampler(cmdp_t* h, const cmdp_desc* d, std::vector<RowDesc>* rows, std::vector<int32_t>* seeds) {
  hipStream_t st = h->stream;
  const int B = h->B, A = h->A;
  const int64_t NS = h->n_states, R = h->n_rows, E = d->sp_ptr[R];
  h->n_entries = E;
  if (d->sp_ptr[0] != 0) return fail(CMDP_ERR_INVALID, "sp_ptr[0] != 0");
  if (int rc = upload_rewards(h, d)) return rc;
  rows->resize((size_t)R);
  std::vector<int64_t> ebase((size_t)B);
  for (int b = 0; b < B; ++b) {
    const int64_t s0 = d->state_off[b], S = d->state_off[b + 1] - s0;
    const int64_t r0 = s0 * A, r1 = (s0 + S) * A;
    ebase[b] = d->sp_ptr[r0];
    for (int64_t r = r0; r < r1; ++r) {
      const int64_t lo = d->sp_ptr[r], n = d->sp_ptr[r + 1] - lo;
      if (n < 1 || n > 4096 || lo - ebase[b] > 0x7fffffffLL)
        return fail(CMDP_ERR_INVALID, "row %lld has %lld successors", (long long)r, (long long)n);
      for (int64_t e = lo; e < lo + n; ++e) {
        if (d->sp_next[e] < 0 || d->sp_next[e] >= S)
          return fail(CMDP_ERR_INVALID, "successor index out of range at entry %lld", (long long)e);
        if (e > lo && d->sp_cum[e] < d->sp_cum[e - 1])
          return fail(CMDP_ERR_INVALID, "sp_cum not non-decreasing at entry %lld", (long long)e);
      }
      RowDesc rd;
      rd.first = (int32_t)(lo - ebase[b]);
      rd.n = (int32_t)n;
      rd.next_if_det = d->sp_next[lo];
      rd.reward_if_det = d->sp_reward[lo];
      rd.pad = 0.0;
      rd.mt_slot = -1;
      if (n > 1 && d->rng_mode == CMDP_RNG_MT_COMPAT) {
        rd.mt_slot = (int32_t)seeds->size();
        seeds->push_back(d->sp_seed[r]);
      }
      (*rows)[(size_t)r] = rd;
    }
  }
  std::vector<int32_t> start_slot((size_t)B, -1);
  if (d->start_off[0] != 0) return fail(CMDP_ERR_INVALID, "start_off[0] != 0");
  for (int b = 0; b < B; ++b) {
    const int64_t lo = d->start_off[b], n = d->start_off[b + 1] - lo;
    const int64_t S = d->state_off[b + 1] - d->state_off[b];
    if (n < 1) return fail(CMDP_ERR_INVALID, "instance %d has no starting state", b);
    for (int64_t i = lo; i < lo + n; ++i)
      if (d->start_state[i] < 0 || d->start_state[i] >= S)
        return fail(CMDP_ERR_INVALID, "starting state out of range (instance %d)", b);
    if (n > 1 && d->rng_mode == CMDP_RNG_MT_COMPAT) {
      start_slot[b] = (int32_t)seeds->size();
      seeds->push_back(d->start_seed[b]);
    }
  }
  if (seeds->size() > 0x7fffffffULL / 2) return fail(CMDP_ERR_INVALID, "too many MT19937 sampler streams");
  h->n_slots = (int64_t)seeds->size();
  const int64_t NSt = d->start_off[B];
  HIP_TRY(h->d_row.upload(rows->data(), rows->size(), st));
  HIP_TRY(h->d_entry_base.upload(ebase.data(), ebase.size(), st));
  HIP_TRY(h->d_sp_next.upload(d->sp_next, E, st));
  HIP_TRY(h->d_sp_cum.upload(d->sp_cum, E, st));
  HIP_TRY(h->d_sp_reward.upload(d->sp_reward, E, st));
  HIP_TRY(h->d_start_off.upload(d->start_off, B + 1, st));
  HIP_TRY(h->d_start_state.upload(d->start_state, NSt, st));
  HIP_TRY(h->d_start_cum.upload(d->start_cum, NSt, st));
  HIP_TRY(h->d_start_slot.upload(start_slot.data(), B, st));
  std::vector<uint2> keys((size_t)B);
  for (int b = 0; b < B; ++b) {
    const uint64_t k = d->philox_key ? d->philox_key[b] : 0;
    keys[b] = make_uint2((uint32_t)k, (uint32_t)(k >> 32));
  }
  HIP_TRY(h->d_key.upload(keys.data(), B, st));
  HIP_TRY(h->d_cur.alloc(B));
  HIP_TRY(h->d_cur.zero(st));
  HIP_TRY(h->d_last_start.alloc(B));
  HIP_TRY(h->d_last_start.zero(st));
  HIP_TRY(h->d_prev_start.alloc(B));
  HIP_TRY(h->d_prev_start.zero(st));
  HIP_TRY(h->d_h.alloc(B));
  HIP_TRY(h->d_h.zero(st));
  HIP_TRY(h->d_need_reset.alloc(B));
  HIP_TRY(hipMemsetAsync(h->d_need_reset.p, 1, B, st));  // BaseMDP starts with a reset pending
  HIP_TRY(h->d_ntrans.alloc(B));
  HIP_TRY(h->d_ntrans.zero(st));
  HIP_TRY(h->d_nreset.alloc(B));
  HIP_TRY(h->d_nreset.zero(st));
  HIP_TRY(h->d_visits_s.alloc(NS));
  HIP_TRY(h->d_visits_s.zero(st));
  HIP_TRY(h->d_visits_sa.alloc(R));
  HIP_TRY(h->d_visits_sa.zero(st));
  HIP_TRY(hipStreamSynchronize(st));  // keys and start_slot go out of scope
  return CMDP_OK;
}

// K1S: the plan's tables to the device
static int install_k1s(cmdp_t* h, K1sChoice* ks) {
  hipStream_t st = h->stream;
  K1sPlan& p = ks->p;
  if (p.shape_bytes == 1) {
    HIP_TRY(h->d_k1s_pat.upload(ks->shape8.data(), ks->shape8.size(), st));
    p.shape = h->d_k1s_pat.p;
  } else {
    HIP_TRY(h->d_k1s_shape16.upload(ks->shape16.data(), ks->shape16.size(), st));
    p.shape = h->d_k1s_shape16.p;
  }
  HIP_TRY(h->d_k1s_dict.upload(ks->dict.data(), ks->dict.size(), st));
  HIP_TRY(h->d_k1s_sets.upload(ks->sets.data(), ks->sets.size(), st));
  HIP_TRY(h->d_k1s_rc.upload(ks->rc.data(), ks->rc.size(), st));
  HIP_TRY(h->d_k1s_patterns.upload(ks->patterns.data(), ks->patterns.size(), st));
  HIP_TRY(h->d_k1s_rvals.upload(ks->rvals.data(), ks->rvals.size(), st));
  HIP_TRY(hipStreamSynchronize(st));  // the host images die with the caller's scope
  p.dict = h->d_k1s_dict.p; p.sets = h->d_k1s_sets.p; p.rcode = h->d_k1s_rc.p;
  p.patterns = h->d_k1s_patterns.p; p.rvals = h->d_k1s_rvals.p;
  h->k1s = p;
  h->k1s_bytes = ks->bytes;
  h->k1s_ok = true;
  return CMDP_OK;
}

// The LDS-resident rollout kernels the batch is eligible for (cmdp_rollout_plan.h), and the tables they read.
static int install_rollout_plans(cmdp_t* h, const cmdp_desc* d, const std::vector<RowDesc>& rows) {
  hipStream_t st = h->stream;
  const PlanInput in{d, rows.data(), h->B, h->A, h->H, h->max_S, h->cus};
  const PlanKnobs knobs = plan_knobs();
  const bool table_rewards = !h->sample_beta && !h->reward_cache;   // the rewards are the table's values
  DetTables t;
  K1lpChoice lp;
  if (table_rewards && h->n_slots == 0 && det_tables(in, &t)) lp = plan_k1lp(in, t, knobs);
  if (!lp.ok) {
    if (!table_rewards || h->rng_mode != CMDP_RNG_PHILOX || h->layout != CMDP_LAYOUT_CSR) return CMDP_OK;
    K1sChoice ks = plan_k1s(in, knobs);
    return ks.ok ? install_k1s(h, &ks) : CMDP_OK;
  }
  K1tChoice kt = plan_k1t(in, t, lp, knobs);
  const K1uChoice ku = plan_k1u(in, kt, knobs);
  K1eChoice ke = plan_k1e(in, t, knobs);
  k1lp_images(lp.p, h->A, &t);
  HIP_TRY(h->d_next16.upload(t.next16.data(), t.next16.size(), st));
  HIP_TRY(h->d_rcode.upload(t.codes.data(), t.codes.size(), st));
  HIP_TRY(h->d_rvals.upload(t.vals.data(), t.vals.size(), st));
  lp.p.next16 = h->d_next16.p + 8; lp.p.rcode = h->d_rcode.p + 16; lp.p.rvals = h->d_rvals.p;
  h->lds_plan = lp.p;
  h->lds_bytes = k1l_lds_bytes(lp.p, lp.p.G);
  h->lds_G1 = lp.G1;
  h->lds_G2 = lp.G2;
  h->lds_succ_bits = lp.succ_bits;
  h->lds_per_cu = lp.per_cu;
  h->lds_ok = true;
  if (kt.ok) {   // eligible: CMDP_OPT_ROLLOUT_KERNEL 4 may force it, and the automatic choice when it needs fewer rounds x time
    HIP_TRY(h->d_tmpl_words.upload(kt.words.data(), kt.words.size(), st));
    HIP_TRY(h->d_swap_bits.upload(kt.swap_bits.data(), kt.swap_bits.size(), st));
    kt.q.tmpl = h->d_tmpl_words.p; kt.q.swap_bits = h->d_swap_bits.p; kt.q.rvals = h->d_rvals.p;
    h->tmpl_plan = kt.q;
    h->tmpl_lds = k1t_lds_bytes(kt.q, kt.q.G);
    h->tmpl_ok = true;
    h->tmpl_auto = kt.autos;
    h->tmpl_cap = kt.cap;
  }
  if (ku.ok) {
    h->k1u = ku.u;
    h->k1u.tmpl = h->d_tmpl_words.p; h->k1u.swap_bits = h->d_swap_bits.p; h->k1u.rvals = h->d_rvals.p;
    h->k1u_lds = k1u_lds_bytes(ku.u, ku.u.G);
    h->k1u_ok = true;
    h->k1u_auto = ku.autos;
    h->k1u_cap = ku.cap;
  }
  if (ke.ok) {
    HIP_TRY(h->d_etab.upload(ke.etab.data(), ke.etab.size(), st));
    ke.e.etab = h->d_etab.p; ke.e.rvals = h->d_rvals.p;
    if (ke.pair.ok) {
      HIP_TRY(h->d_ptab.upload(ke.pair.ptab.data(), ke.pair.ptab.size(), st));
      HIP_TRY(h->d_pinv.upload(ke.pair.inv.data(), ke.pair.inv.size(), st));
      ke.e.ptab = h->d_ptab.p; ke.e.pinv = h->d_pinv.p;
      h->k1e_pair_ok = knobs.k1e_pair != 0;
      h->k1e_sp2 = ke.pair.SP2;
      h->k1e_n_even = ke.pair.n_even;
      h->k1e_pair_lds = k1e_pair_lds_bytes(ke.e, ke.e.ash2);
    }
    h->k1e = ke.e;
    h->k1e_lds = k1e_lds_bytes(ke.e);
    h->k1e_ok = true;
  }
  HIP_TRY(hipStreamSynchronize(st));  // the host images die with this scope
  return CMDP_OK;
}

// One MT19937 state per sampler stream of CMDP_RNG_MT_COMPAT (rows with several successors, instances with several starts)
static int seed_mt(cmdp_t* h, const std::vector<int32_t>& seeds) {
  if (!h->n_slots) return CMDP_OK;
  hipStream_t st = h->stream;
  DevBuf<int32_t> d_seeds;
  HIP_TRY(d_seeds.upload(seeds.data(), seeds.size(), st));
  HIP_TRY(h->d_mt.alloc((size_t)h->n_slots * 624));
  HIP_TRY(h->d_mt_pos.alloc(h->n_slots));
  hipLaunchKernelGGL(k_mt_seed, dim3(grid_for(h->n_slots, 64)), dim3(64), 0, st, h->d_mt.p, h->d_mt_pos.p,
                     d_seeds.p, h->n_slots);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));  // d_seeds is released at scope exit
  return CMDP_OK;
}

// The DP half: CSR rows, validated, and the shape statistics the DP kernels are chosen by.
static int upload_dp(cmdp_t* h, const cmdp_desc* d) {
  hipStream_t st = h->stream;
  const int B = h->B, A = h->A;
  const int64_t R = h->n_rows;
  if (d->csr_ptr[0] != 0) return fail(CMDP_ERR_INVALID, "csr_ptr[0] != 0");
  const int64_t N = d->csr_ptr[R];
  h->n_csr = N;
  h->csr_nnz.resize(B);
  for (int b = 0; b < B; ++b) {
    const int64_t s0 = d->state_off[b], S = d->state_off[b + 1] - s0;
    const int64_t r0 = s0 * A, r1 = (s0 + S) * A;
    h->csr_nnz[b] = d->csr_ptr[r1] - d->csr_ptr[r0];
    if (h->csr_nnz[b] > 0x7fffffffLL) return fail(CMDP_ERR_INVALID, "instance %d has too many non-zeros", b);
    h->max_inst_nnz = std::max(h->max_inst_nnz, h->csr_nnz[b]);
    for (int64_t r = r0; r < r1; ++r) {
      if (d->csr_ptr[r + 1] < d->csr_ptr[r]) return fail(CMDP_ERR_INVALID, "csr_ptr decreasing at row %lld", (long long)r);
      h->max_row_nnz = std::max<int>(h->max_row_nnz, (int)std::min<int64_t>(d->csr_ptr[r + 1] - d->csr_ptr[r], 1 << 30));
      for (int64_t k = d->csr_ptr[r]; k < d->csr_ptr[r + 1]; ++k)
        if (d->csr_col[k] < 0 || d->csr_col[k] >= S)
          return fail(CMDP_ERR_INVALID, "csr_col out of range at %lld", (long long)k);
    }
  }
  // K2U (k_dp_regu): distinct successor columns per STATE over its A rows, and whether every row lists its columns
  // in strictly ascending order (the dense-over-the-distinct-set sum is the ascending-column sum)
  h->max_state_unique = 0;
  if (A <= 4 && h->max_row_nnz <= 8 && h->max_S <= 1024) {
    bool sorted = true;
    int32_t cols[32];
    for (int64_t s = 0; s < d->state_off[B] && sorted; ++s) {
      int n = 0;
      for (int a = 0; a < A; ++a) {
        const int64_t r = s * A + a;
        for (int64_t k = d->csr_ptr[r]; k < d->csr_ptr[r + 1]; ++k) {
          if (k > d->csr_ptr[r] && d->csr_col[k] <= d->csr_col[k - 1]) sorted = false;
          cols[n++] = d->csr_col[k];
        }
      }
      std::sort(cols, cols + n);
      const int u = (int)(std::unique(cols, cols + n) - cols);
      h->max_state_unique = std::max(h->max_state_unique, u);
    }
    if (!sorted) h->max_state_unique = 0;
  }
  HIP_TRY(h->d_csr_ptr.upload(d->csr_ptr, R + 1, st));
  HIP_TRY(h->d_csr_col.upload(d->csr_col, N, st));
  HIP_TRY(h->d_csr_val.upload(d->csr_val, N, st));
  HIP_TRY(h->d_R.upload(d->R, R, st));
  return CMDP_OK;
}

// CMDP_LAYOUT_DENSE: the float32 rows of the DP half as dense [R][dense_spad] rows.
static int build_dense(cmdp_t* h, const cmdp_desc* d) {
  const int64_t R = h->n_rows;
  // exact float64 prefix sums need every probability to be a multiple of 2^-52 after scaling: p >= 2^-28
  for (int64_t k = 0; k < h->n_csr; ++k)
    if (!(d->csr_val[k] >= 3.7252902984619141e-09f) || d->csr_val[k] > 1.0f)
      return fail(CMDP_ERR_INVALID, "dense layout needs probabilities in [2^-28, 1] (entry %lld)", (long long)k);
  const int nv = (h->max_S + 255) / 256;
  const int allowed[] = {1, 2, 3, 4, 6, 8, 12, 16};
  int pick = 0;
  for (int v : allowed) if (v >= nv) { pick = v; break; }
  if (!pick) return fail(CMDP_ERR_UNSUPPORTED, "dense layout supports at most 4096 states per instance");
  h->dense_spad = pick * 256;
  const size_t n = (size_t)R * h->dense_spad;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (n * sizeof(float) > free_b)
    return fail(CMDP_ERR_INVALID, "dense layout needs %zu MiB, %zu MiB free", n * sizeof(float) >> 20, free_b >> 20);
  HIP_TRY(h->d_dense.alloc(n));
  HIP_TRY(h->d_dense.zero(h->stream));
  hipLaunchKernelGGL(k_dense_fill, dim3(grid_for(R, 256)), dim3(256), 0, h->stream, h->d_dense.p, h->dense_spad,
                     h->d_csr_ptr.p, h->d_csr_col.p, h->d_csr_val.p, R);
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

extern "C" {

int cmdp_version(void) { return CMDP_ABI_VERSION; }
#ifndef CMDP_BUILD_ID
#define CMDP_BUILD_ID "unstamped"
#endif
static const char k_build_id[] = "CMDP_BUILD_ID=" CMDP_BUILD_ID;  /* the tag lets build() read the stamp from the file */
const char* cmdp_build_id(void) { return k_build_id + 14; }

const char* cmdp_last_error(void) { return g_err.c_str(); }

int cmdp_k1e_round_interior(int e_lo, int horizon, int64_t n_steps, int n_instances) {
  return k1e_round_interior(e_lo, horizon, n_steps, n_instances) ? 1 : 0;
}

uint32_t cmdp_k1e_code_counts(uint32_t lo, uint32_t hi, int few) {
  return few ? k1e_code_counts_few(lo, hi) : k1e_code_counts(lo, hi);
}

int cmdp_k1e_scan_words(const uint64_t* words, int64_t n_words, int H, int h0, int64_t n_steps, int nch, int n_codes,
                        const double rv[4], double s0, double* sum, int32_t stats[4]) {
  if (!stats) return fail(CMDP_ERR_INVALID, "cmdp_k1e_scan_words: null argument");
  int32_t all[8];
  const int rc = cmdp_k1e_scan_words_ex(words, n_words, H, h0, n_steps, nch, n_codes, rv, s0, sum, all);
  if (rc != CMDP_OK) return rc;
  for (int i = 0; i < 4; ++i) stats[i] = all[i];
  return CMDP_OK;
}

int cmdp_k1e_scan_words_ex(const uint64_t* words, int64_t n_words, int H, int h0, int64_t n_steps, int nch, int n_codes,
                           const double rv[4], double s0, double* sum, int32_t stats[8]) {
  if (!words || !rv || !sum || !stats) return fail(CMDP_ERR_INVALID, "cmdp_k1e_scan_words: null argument");
  // (a segment: the lane counts its steps in an int)
  if (H < 1 || h0 < 0 || h0 >= H || n_steps < 1 || n_steps >= ((int64_t)1 << 31) || nch != (H + 31) / 32 || n_codes < 1 || n_codes > 4)
    return fail(CMDP_ERR_INVALID, "cmdp_k1e_scan_words: H %d, h0 %d, n_steps %lld, nch %d, n_codes %d", H, h0, (long long)n_steps, nch, n_codes);
  if ((((int64_t)h0 + n_steps + H - 1) / H) * nch != n_words || n_words >= ((int64_t)1 << 31))
    return fail(CMDP_ERR_INVALID, "cmdp_k1e_scan_words: %lld words do not hold %lld steps from in-episode time %d", (long long)n_words,
                (long long)n_steps, h0);
  double r[4];
  for (int c = 0; c < 4; ++c) r[c] = c < n_codes ? rv[c] : 0.0;
  K1rLane L;
  k1r_init(L, r, n_codes, H, nch, h0, n_steps, s0);
  K1rHostLoader ld{words, L.W};
  K1rStats st;
  k1r_scan(L, ld, st);
  *sum = k1r_sum(L);
  for (int i = 0; i < 8; ++i) stats[i] = st.n[i];
  return CMDP_OK;
}

int cmdp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int cmdp_set_device(int device) {
  HIP_TRY(hipSetDevice(device));
  // CMDP_SYNC_MODE = spin | yield | block: how host threads wait in hipStreamSynchronize (tuning aid for hosts with a CPU
  // quota: several threads driving batches concurrently each spin on a core by default)
  if (const char* e = std::getenv("CMDP_SYNC_MODE")) {
    const unsigned f = !std::strcmp(e, "block") ? hipDeviceScheduleBlockingSync
                     : !std::strcmp(e, "yield") ? hipDeviceScheduleYield
                     : !std::strcmp(e, "spin") ? hipDeviceScheduleSpin : hipDeviceScheduleAuto;
    HIP_TRY(hipSetDeviceFlags(f));
  }
  return CMDP_OK;
}

void* cmdp_stream(cmdp_t* h) { return h ? (void*)h->stream : nullptr; }

int cmdp_destroy(cmdp_t* h) {
  if (h && h->ev_dp0) {
    (void)hipEventDestroy(h->ev_dp0);
    (void)hipEventDestroy(h->ev_dp1);
  }
  if (!h) return CMDP_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamDestroy(h->stream);
  }
  for (int i = 0; i < 2; ++i) {
    if (h->aux.walk[i]) (void)hipEventDestroy(h->aux.walk[i]);
    if (h->aux.scan[i]) (void)hipEventDestroy(h->aux.scan[i]);
  }
  if (h->aux.stream) {
    (void)hipStreamSynchronize(h->aux.stream);
    (void)hipStreamDestroy(h->aux.stream);
  }
  for (int i = 0; i < 5; ++i)
    if (h->ev_time[i]) (void)hipEventDestroy(h->ev_time[i]);
  for (int i = 0; i < 2; ++i)
    if (h->ev_row[i]) (void)hipEventDestroy(h->ev_row[i]);
  for (int i = 0; i < 2; ++i)
    if (h->ev_as[i]) (void)hipEventDestroy(h->ev_as[i]);
  for (cmdp_t** back : h->uc_backrefs) *back = nullptr;
  for (double* c : h->rc_chunks) (void)hipFree(c);
  if (h->rc_stage_h) (void)hipHostFree(h->rc_stage_h);
  if (h->rc_dst_h) (void)hipHostFree(h->rc_dst_h);
  if (h->rc_ent_h) (void)hipHostFree(h->rc_ent_h);
  if (h->rc_list_h) (void)hipHostFree(h->rc_list_h);
  if (h->rc_pend_h) (void)hipHostFree(h->rc_pend_h);
  delete h;
  return CMDP_OK;
}

int cmdp_create(cmdp_t** out, const cmdp_desc* d) {
  if (!out || !d) return fail(CMDP_ERR_INVALID, "null argument");
  *out = nullptr;
  int max_S = 0;
  if (int rc = check_desc(d, &max_S)) return rc;
  const int B = d->n_instances, A = d->n_actions;

  cmdp_t* h = new cmdp;
  struct Guard {
    cmdp_t* h;
    ~Guard() { if (h) cmdp_destroy(h); }
  } guard{h};
  HIP_TRY(hipGetDevice(&h->device));
  if (hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || h->cus < 1) h->cus = 256;
  HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  h->B = B; h->A = A; h->H = d->horizon; h->rng_mode = d->rng_mode; h->layout = d->layout;
  h->rmin = d->reward_min; h->rmax = d->reward_max;
  h->n_states = d->state_off[B]; h->n_rows = h->n_states * A; h->max_S = max_S;
  h->has_env = d->sp_ptr != nullptr; h->has_dp = d->csr_ptr != nullptr;
  h->state_off.assign(d->state_off, d->state_off + B + 1);
  HIP_TRY(h->d_state_off.upload(d->state_off, B + 1, h->stream));
  HIP_TRY(h->d_flag.alloc(1));
  if (h->has_env) {
    std::vector<RowDesc> rows;
    std::vector<int32_t> seeds;
    if (int rc = upload_sampler(h, d, &rows, &seeds)) return rc;
    if (int rc = install_rollout_plans(h, d, rows)) return rc;
    if (int rc = seed_mt(h, seeds)) return rc;
  }
  if (h->has_dp) {
    if (int rc = upload_dp(h, d)) return rc;
  }
  if (d->layout == CMDP_LAYOUT_DENSE) {
    if (int rc = build_dense(h, d)) return rc;
  }
  HIP_TRY(hipStreamSynchronize(h->stream));  // host staging vectors go out of scope
  guard.h = nullptr;
  *out = h;
  return CMDP_OK;
}

// ---- interaction --------------------------------------------------------------------------------------
int cmdp_reset(cmdp_t* h, const uint8_t* mask, int32_t* obs_out) {
  if (int rc = bind(h)) return rc;
  if (!h->has_env) return fail(CMDP_ERR_INVALID, "handle was created without the sampler half");
  if (int rc = visits_check(h, 1)) return rc;
  hipStream_t st = h->stream;
  uint8_t* dmask = nullptr;
  if (mask) {
    HIP_TRY(h->d_mask.upload(mask, h->B, st));
    dmask = h->d_mask.p;
  }
  if (obs_out && h->d_last_obs.n < (size_t)h->B) HIP_TRY(h->d_last_obs.alloc(h->B));
  if (obs_out && mask) HIP_TRY(hipMemcpyAsync(h->d_last_obs.p, obs_out, sizeof(int32_t) * h->B, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_reset, dim3(grid_for(h->B, 256)), dim3(256), 0, st, h->env(), dmask,
                     obs_out ? h->d_last_obs.p : nullptr);
  visits_commit(h, 1);
  HIP_TRY(hipGetLastError());
  if (obs_out) HIP_TRY(hipMemcpyAsync(obs_out, h->d_last_obs.p, sizeof(int32_t) * h->B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (!mask) h->known_reset = true;
  h->at_start = !mask;   // (a masked reset leaves the other instances where they are)
  return CMDP_OK;
}

}  // extern "C"
// ---- reference-exact reward caches: the park / fill / relaunch loop (cmdp_reward_cache.h) ------------------------------
// `launch(resume)` enqueues the interaction kernel of the call on the handle's stream (resume 0: every lane starts the
// call's steps; 1: only lanes that parked continue).  Returns when no instance is parked any more; the stream is idle then.
template <typename F>
static int rc_drive(cmdp_t* h, F&& launch) {
  hipStream_t st = h->stream;
  const int B = h->B;
  // refused before anything is stepped: a lane that parks has already committed its transition
  if (!h->rc_streams_set)
    return fail(CMDP_ERR_INVALID, "CMDP_FLAG_REWARD_CACHE: cmdp_set_reward_streams has not been called on this handle");
  HIP_TRY(h->d_rc_park_count.zero(st));
  if (int rc = launch(0)) return rc;
  for (;;) {
    HIP_TRY(hipMemcpyAsync(h->rc_list_h, h->d_rc_park_count.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int count = h->rc_list_h[0];
    if (count == 0) return CMDP_OK;
    const auto t_round = std::chrono::steady_clock::now();
    if (count < 0 || count > B) return fail(CMDP_ERR_HIP, "reward cache: corrupt park count %d", count);
    if (!h->rc_streams_set)
      return fail(CMDP_ERR_INVALID, "CMDP_FLAG_REWARD_CACHE: a Beta reward is needed but cmdp_set_reward_streams was not called");
    HIP_TRY(hipMemcpyAsync(h->rc_list_h, h->d_rc_park_list.p, sizeof(int32_t) * count, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h->rc_pend_h, h->d_rc_pend_e.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->rc_rounds++;
    for (int j0 = 0; j0 < count; j0 += h->rc_cap) {
      const int n = std::min(h->rc_cap, count - j0);
      // one task per parked instance: 5000 draws of its triple's distribution from the instance's own numpy stream
      const std::function<void(int)> fill = [&](int j) {
        const int b = h->rc_list_h[j0 + j];
        const int32_t c = h->h_canon[(size_t)h->rc_pend_h[b]];
        const double pa = h->h_rp0[(size_t)c], pb = h->h_rp1[(size_t)c];
        cmdp_rc::NumpyStream& rs = h->rc_streams[(size_t)b];
        double* out = h->rc_stage_h + (size_t)j * CMDP_RC_BLOCK;
        for (int k = 0; k < CMDP_RC_BLOCK; ++k) out[k] = rs.beta(pa, pb);
      };
      const auto t_fill = std::chrono::steady_clock::now();
      cmdp_rc::Pool::get().parallel_for(n, fill);
      h->rc_fill_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_fill).count();
      for (int j = 0; j < n; ++j) {
        const int b = h->rc_list_h[j0 + j];
        const int32_t c = h->h_canon[(size_t)h->rc_pend_h[b]];
        double* blk = h->rc_blk_h[(size_t)c];
        if (!blk) {  // first fill of the triple: a block of its own from the pool (a refill overwrites it in place)
          const size_t chunk = h->rc_next_block / h->rc_chunk_blocks, slot = h->rc_next_block % h->rc_chunk_blocks;
          if (chunk == h->rc_chunks.size()) {
            double* cp = nullptr;
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&cp), sizeof(double) * h->rc_chunk_blocks * CMDP_RC_BLOCK));
            h->rc_chunks.push_back(cp);
          }
          blk = h->rc_chunks[chunk] + slot * CMDP_RC_BLOCK;
          h->rc_next_block++;
          h->rc_blk_h[(size_t)c] = blk;
        }
        h->rc_dst_h[j] = blk;
        h->rc_ent_h[j] = c;
      }
      h->rc_fills += n;
      HIP_TRY(hipMemcpyAsync(h->d_rc_stage.p, h->rc_stage_h, sizeof(double) * (size_t)n * CMDP_RC_BLOCK, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(h->d_rc_dst.p, h->rc_dst_h, sizeof(double*) * (size_t)n, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(h->d_rc_ent.p, h->rc_ent_h, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_rc_install, dim3(n), dim3(256), 0, st, n, h->d_rc_stage.p, h->d_rc_dst.p, h->d_rc_ent.p, h->rcache());
      HIP_TRY(hipGetLastError());
      if (j0 + n < count) HIP_TRY(hipStreamSynchronize(st));  // the pinned staging area is reused by the next slice
    }
    if (int rc = launch(1)) return rc;
    h->rc_round_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_round).count();
  }
}

extern "C" {
int cmdp_set_reward_streams(cmdp_t* h, const uint32_t* mt_key, const int32_t* mt_pos, const int32_t* has_gauss,
                            const double* cached_gaussian) {
  if (!h || !mt_key || !mt_pos) return fail(CMDP_ERR_INVALID, "null argument");
  const int B = h->B;
  for (int b = 0; b < B; ++b)
    if (mt_pos[b] < 0 || mt_pos[b] > 624) return fail(CMDP_ERR_INVALID, "instance %d: MT19937 position %d outside [0, 624]", b, mt_pos[b]);
  h->rc_streams.resize((size_t)B);
  for (int b = 0; b < B; ++b) {
    cmdp_rc::NumpyStream& rs = h->rc_streams[(size_t)b];
    std::memcpy(rs.key, mt_key + (size_t)b * 624, sizeof rs.key);
    rs.pos = mt_pos[b];
    rs.out_valid = false;
    rs.has_gauss = has_gauss ? has_gauss[b] : 0;
    rs.gauss = cached_gaussian ? cached_gaussian[b] : 0.0;
  }
  if (h->rc_streams_set && h->reward_cache) {
    // repositioned streams = a new run on a fresh copy of every MDP (BaseMDP.sample_reward starts with empty caches,
    // colosseum/mdp/base.py:1187-1207): the blocks installed on the device, their positions and any parked step are dropped;
    // the pool's chunks are handed out again from the start
    if (int rc = bind(h)) return rc;
    hipStream_t st = h->stream;
    HIP_TRY(h->d_rc_blk.zero(st));
    HIP_TRY(h->d_rc_pos.zero(st));
    HIP_TRY(hipMemsetAsync(h->d_rc_pend_e.p, 0xff, sizeof(int32_t) * (size_t)B, st));
    HIP_TRY(h->d_rc_left.zero(st));
    HIP_TRY(h->d_rc_park_count.zero(st));
    HIP_TRY(hipStreamSynchronize(st));
    std::fill(h->rc_blk_h.begin(), h->rc_blk_h.end(), nullptr);
    h->rc_next_block = 0;
  }
  h->rc_streams_set = true;
  return CMDP_OK;
}

int cmdp_legacy_beta(uint32_t* mt_key, int32_t* mt_pos, int32_t* has_gauss, double* cached_gaussian, double a, double b,
                     int64_t n, double* out) {
  if (!mt_key || !mt_pos || !has_gauss || !cached_gaussian || !out || n < 0) return fail(CMDP_ERR_INVALID, "null argument");
  if (!(a > 0.0 && b > 0.0)) return fail(CMDP_ERR_INVALID, "Beta parameters must be positive");
  if (*mt_pos < 0 || *mt_pos > 624) return fail(CMDP_ERR_INVALID, "MT19937 position outside [0, 624]");
  cmdp_rc::NumpyStream rs;
  std::memcpy(rs.key, mt_key, sizeof rs.key);
  rs.pos = *mt_pos; rs.has_gauss = *has_gauss; rs.gauss = *cached_gaussian;
  // several blocks in parallel would not be the reference's stream: one stream, sequential draws
  for (int64_t i = 0; i < n; ++i) out[i] = rs.beta(a, b);
  std::memcpy(mt_key, rs.key, sizeof rs.key);
  *mt_pos = rs.pos; *has_gauss = rs.has_gauss; *cached_gaussian = rs.gauss;
  return CMDP_OK;
}

static int any_needs_reset(cmdp_t* h, bool* any) {
  hipStream_t st = h->stream;
  HIP_TRY(h->d_flag.zero(st));
  hipLaunchKernelGGL(k_any_needs_reset, dim3(grid_for(h->B, 256)), dim3(256), 0, st, h->d_need_reset.p, h->B,
                     h->d_flag.p);
  HIP_TRY(hipGetLastError());
  int32_t f = 0;
  HIP_TRY(hipMemcpyAsync(&f, h->d_flag.p, sizeof f, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *any = f != 0;
  return CMDP_OK;
}

int cmdp_step(cmdp_t* h, const int32_t* actions, int auto_reset, int32_t* obs, double* reward, uint8_t* step_type) {
  if (int rc = bind(h)) return rc;
  if (!h->has_env) return fail(CMDP_ERR_INVALID, "handle was created without the sampler half");
  if (!actions || !obs || !reward || !step_type) return fail(CMDP_ERR_INVALID, "null argument");
  if (h->layout == CMDP_LAYOUT_DENSE) return fail(CMDP_ERR_UNSUPPORTED, "dense layout: use cmdp_rollout");
  if (int rc = visits_check(h, 1)) return rc;
  hipStream_t st = h->stream;
  const int B = h->B;
  if (h->d_i32_scratch.n < (size_t)2 * B) HIP_TRY(h->d_i32_scratch.alloc((size_t)2 * B));
  if (h->d_f64_scratch.n < (size_t)B) HIP_TRY(h->d_f64_scratch.alloc(B));
  if (h->d_u8_scratch.n < (size_t)B) HIP_TRY(h->d_u8_scratch.alloc(B));
  int32_t* d_act = h->d_i32_scratch.p;
  int32_t* d_obs = h->d_i32_scratch.p + B;
  HIP_TRY(hipMemcpyAsync(d_act, actions, sizeof(int32_t) * B, hipMemcpyHostToDevice, st));
  HIP_TRY(h->d_flag.zero(st));
  if (!auto_reset)
    hipLaunchKernelGGL(k_any_needs_reset, dim3(grid_for(B, 256)), dim3(256), 0, st, h->d_need_reset.p, B, h->d_flag.p);
  hipLaunchKernelGGL(k_check_actions, dim3(grid_for(B, 256)), dim3(256), 0, st, d_act, B, h->A, h->d_flag.p);
  HIP_TRY(hipGetLastError());
  int32_t f = 0;
  HIP_TRY(hipMemcpyAsync(&f, h->d_flag.p, sizeof f, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (f & 2) return fail(CMDP_ERR_INVALID, "action out of range [0, %d)", h->A);
  if (f & 1) return fail(CMDP_ERR_NEEDS_RESET, "step() on an instance that needs reset()");
  h->known_reset = false;  // a step may end an episode (LAST): the async rollout re-checks before its next launch
  if (h->reward_cache) {
    if (int rc = visits_commit(h, 1, rc_drive(h, [&](int resume) -> int {
          hipLaunchKernelGGL(k_step<true>, dim3(grid_for(B, 256)), dim3(256), 0, st, h->env(), d_act, auto_reset, d_obs,
                             h->d_f64_scratch.p, h->d_u8_scratch.p, h->rcache(), resume);
          HIP_TRY(hipGetLastError());
          return CMDP_OK;
        })))
      return rc;
  } else {
    hipLaunchKernelGGL(k_step<false>, dim3(grid_for(B, 256)), dim3(256), 0, st, h->env(), d_act, auto_reset, d_obs,
                       h->d_f64_scratch.p, h->d_u8_scratch.p, RewardCache{}, 0);
    visits_commit(h, 1);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(obs, d_obs, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(reward, h->d_f64_scratch.p, sizeof(double) * B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(step_type, h->d_u8_scratch.p, B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

// ---- CMDP_POLICY_RANDOM_REFERENCE: the reference's action streams (cmdp_actions.h) ------------------------------------
static int action_streams_alloc(cmdp_t* h) {
  HIP_TRY(h->d_as_key.alloc((size_t)h->B * MTA_N));
  HIP_TRY(h->d_as_pos.alloc(h->B));
  if (!h->d_as_fail.p) {
    HIP_TRY(h->d_as_fail.alloc(1));
    HIP_TRY(h->d_as_fail.zero(h->stream));
  }
  return CMDP_OK;
}

int cmdp_set_action_streams(cmdp_t* h, const uint32_t* seeds) {
  if (int rc = bind(h, false)) return rc;
  if (!h->has_env) return fail(CMDP_ERR_INVALID, "handle was created without the sampler half");
  if (!seeds) return fail(CMDP_ERR_INVALID, "null argument");
  hipStream_t st = h->stream;
  if (int rc = action_streams_alloc(h)) return rc;
  DevBuf<uint32_t> d_seeds;
  HIP_TRY(d_seeds.upload(seeds, h->B, st));
  // init_genrand, then numpy's position right after seeding: the first draw twists the block
  hipLaunchKernelGGL(k_mt_seed_numpy, dim3(grid_for(h->B, 64)), dim3(64), 0, st, h->d_as_key.p, h->d_as_pos.p, d_seeds.p, h->B);
  hipLaunchKernelGGL(k_fill_i32, dim3(grid_for(h->B, 256)), dim3(256), 0, st, h->d_as_pos.p, MTA_N, (int64_t)h->B);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));   // (the seeds leave scope)
  h->as_set = true;
  return CMDP_OK;
}

int cmdp_set_action_stream_state(cmdp_t* h, const uint32_t* mt_key, const int32_t* mt_pos) {
  if (int rc = bind(h, false)) return rc;
  if (!h->has_env) return fail(CMDP_ERR_INVALID, "handle was created without the sampler half");
  if (!mt_key || !mt_pos) return fail(CMDP_ERR_INVALID, "null argument");
  for (int b = 0; b < h->B; ++b)
    if (mt_pos[b] < 0 || mt_pos[b] > MTA_N) return fail(CMDP_ERR_INVALID, "instance %d: MT19937 position %d outside [0, 624]", b, mt_pos[b]);
  if (int rc = action_streams_alloc(h)) return rc;
  HIP_TRY(hipMemcpyAsync(h->d_as_key.p, mt_key, sizeof(uint32_t) * (size_t)h->B * MTA_N, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_as_pos.p, mt_pos, sizeof(int32_t) * (size_t)h->B, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->as_set = true;
  return CMDP_OK;
}

int cmdp_action_stream_state(cmdp_t* h, uint32_t* mt_key, int32_t* mt_pos) {
  if (int rc = bind(h, false)) return rc;
  if (!mt_key || !mt_pos) return fail(CMDP_ERR_INVALID, "null argument");
  if (!h->as_set) return fail(CMDP_ERR_INVALID, "no action streams: call cmdp_set_action_streams first");
  HIP_TRY(hipMemcpyAsync(mt_key, h->d_as_key.p, sizeof(uint32_t) * (size_t)h->B * MTA_N, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(mt_pos, h->d_as_pos.p, sizeof(int32_t) * (size_t)h->B, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CMDP_OK;
}

int cmdp_mt_randint(uint32_t* mt_key, int32_t* mt_pos, int n_actions, int64_t n, int8_t* out) {
  if (!mt_key || !mt_pos || (!out && n > 0) || n < 0) return fail(CMDP_ERR_INVALID, "null argument");
  if (n_actions < 1 || n_actions > 128) return fail(CMDP_ERR_INVALID, "n_actions outside [1, 128] (actions are int8)");
  if (*mt_pos < 0 || *mt_pos > MTA_N) return fail(CMDP_ERR_INVALID, "MT19937 position outside [0, 624]");
  if (!mta_randint_host(mt_key, mt_pos, n_actions, n, out))
    return fail(CMDP_ERR_HIP, "randint: more than %lld words for %lld actions", mta_word_bound(n), (long long)n);
  return CMDP_OK;
}

int cmdp_mt_action_bits(uint32_t* mt_key, int32_t* mt_pos, int64_t n, int64_t bit_offset, uint32_t* out) {
  if (!mt_key || !mt_pos || (!out && n > 0) || n < 0 || bit_offset < 0) return fail(CMDP_ERR_INVALID, "bad argument");
  if (*mt_pos < 0 || *mt_pos > MTA_N) return fail(CMDP_ERR_INVALID, "MT19937 position outside [0, 624]");
  mta_action_bits_host(mt_key, mt_pos, n, bit_offset, out);
  return CMDP_OK;
}

// K16's byte form: the call's n_steps x B actions into d_actions8, in the layout of CMDP_POLICY_HOST_ACTIONS (every kernel but
// K1E takes them as such).  Once per call: reward-cache handles relaunch the rollout kernel, never this.
static int reference_actions(cmdp_t* h, int64_t n_steps, const int8_t** d_act) {
  if (n_steps > 0x7fffffffLL) return fail(CMDP_ERR_INVALID, "CMDP_POLICY_RANDOM_REFERENCE: more than 2^31 - 1 transitions in one call");
  HIP_TRY(h->d_actions8.alloc((size_t)n_steps * (size_t)h->B));
  if (n_steps > 0) {
    hipLaunchKernelGGL(k_mt_actions<false>, dim3(h->B), dim3(K16_THREADS), 0, h->stream, h->d_as_key.p, h->d_as_pos.p,
                       (const unsigned long long*)nullptr, h->B, h->A, (int)n_steps, 0, (uint4*)nullptr, h->d_actions8.p, h->d_as_fail.p);
    HIP_TRY(hipGetLastError());
    h->as_unchecked = true;
  }
  *d_act = h->d_actions8.p;
  return CMDP_OK;
}

// K16 raises its flag on the device when a draw exceeds its word bound; the host looks after a synchronisation of the stream
static int action_streams_check(cmdp_t* h) {
  if (!h->as_unchecked) return CMDP_OK;
  h->as_unchecked = false;
  int32_t f = 0;
  HIP_TRY(hipMemcpy(&f, h->d_as_fail.p, sizeof f, hipMemcpyDeviceToHost));
  if (!f) return CMDP_OK;
  HIP_TRY(hipMemset(h->d_as_fail.p, 0, sizeof f));
  return fail(CMDP_ERR_HIP, "CMDP_POLICY_RANDOM_REFERENCE: an action stream rejected more words than its bound allows; the "
                            "remaining actions of that launch were 0 (reseed the streams and reset the handle)");
}

// ---- rollout: the kernel a launch takes, then one launcher per kernel -----------------------------------
enum class RolloutKernel { K1, K1_REWARD_CACHE, K1_GREEDY, K1D, K1L, K1P, K1T, K1U, K1E, K1S };

struct RolloutCall {
  int policy;
  const int8_t* actions;   // CMDP_POLICY_HOST_ACTIONS: [n][B]
  const float* q;          // CMDP_POLICY_GREEDY_Q: the Q table
  int64_t n;
  double* rsum;
  int32_t* last;
  int32_t* tobs; double* trew; uint8_t* ttype;   // the trace (only K1 records one)
  int resume;              // reward caches: 1 when only the lanes that parked continue
  bool trace() const { return tobs || trew || ttype; }
};

// No HIP calls.  CMDP_OPT_ROLLOUT_KERNEL forces a kernel (refused when the batch is not eligible); the reward-cache,
// greedy-Q and dense-layout paths ignore it.  Automatically the LDS-resident kernels are taken from 64 transitions on
// (they pay a fixed staging + flush cost per launch), the most specialised eligible one first.
static int pick_rollout(const cmdp_t* h, int policy, bool trace, int64_t n_steps, RolloutKernel* out) {
  using K = RolloutKernel;
  const int rk = h->rollout_kernel;
  const bool dense = h->layout == CMDP_LAYOUT_DENSE, wide = rk == 0 && n_steps >= 64;
  *out = h->reward_cache ? K::K1_REWARD_CACHE : policy == CMDP_POLICY_GREEDY_Q ? K::K1_GREEDY : dense ? K::K1D : K::K1;
  if (*out == K::K1_GREEDY && dense) return fail(CMDP_ERR_UNSUPPORTED, "CMDP_POLICY_GREEDY_Q runs on the CSR layout");
  if (*out == K::K1D && trace) return fail(CMDP_ERR_UNSUPPORTED, "the dense-layout rollout does not record traces");
  if (*out != K::K1) return CMDP_OK;
  // CMDP_POLICY_RANDOM_REFERENCE: K1E consumes K16's bit blocks; the chain kernels K1L / K1P / K1T / K1U / K1S draw Philox only
  const bool ref = policy == CMDP_POLICY_RANDOM_REFERENCE;
  if (ref && rk >= 2 && rk <= 5)
    return fail(CMDP_ERR_UNSUPPORTED, "CMDP_POLICY_RANDOM_REFERENCE runs on the episode-parallel rollout K1E (CMDP_OPT_ROLLOUT_KERNEL 6 or 0) and on "
                                      "the lane-per-instance kernel K1 (1 or 0); kernel %d draws the Philox stream only", rk);
  const bool lds = h->lds_ok && (policy == CMDP_POLICY_RANDOM || ref) && !trace, k1s = h->k1s_ok && policy == CMDP_POLICY_RANDOM && !trace;
  if (rk == 2 && !lds)
    return fail(CMDP_ERR_UNSUPPORTED, "LDS-resident rollout needs deterministic dynamics, one start state, <= 65535 "
                                      "states, <= 256 distinct rewards, the random policy and no trace");
  if (rk == 4 && !(lds && h->tmpl_ok))
    return fail(CMDP_ERR_UNSUPPORTED, "the shared-table rollout K1T needs a batch eligible for K1P with two actions whose instances "
                                      "are per-state action permutations of the first one, the random policy and no trace");
  if (rk == 5 && !(lds && h->k1u_ok))
    return fail(CMDP_ERR_UNSUPPORTED, "the streamed-trace rollout K1U needs a batch eligible for the shared-table rollout K1T (CMDP_OPT_ROLLOUT_KERNEL 4) "
                                      "and room for 64 instances per workgroup");
  if (rk == 6 && !(lds && h->k1e_ok))
    return fail(CMDP_ERR_UNSUPPORTED, "the episode-parallel rollout K1E needs a batch eligible for the LDS-resident kernels (CMDP_OPT_ROLLOUT_KERNEL 2) "
                                      "that is episodic, has two actions, at most four distinct reward values, at most 512 states per instance and a horizon whose action bits for 128 episodes fit LDS");
  if (rk == 3 && !k1s)
    return fail(CMDP_ERR_UNSUPPORTED, "the LDS-resident stochastic rollout K1S needs Philox mode, the random policy, no trace, equal "
                                      "state counts, <= 16 entries per row and <= 16 distinct successors per state, <= 64 "
                                      "cumulative-probability patterns, deterministic rewards that depend on the successor or on "
                                      "the row alone, and room for four instances in LDS");
  // K1S runs G instances per CU at a time however large the batch is (LDS capacity), K1's rate grows with the batch (more
  // wavefronts cover its HBM latency) until bandwidth caps it: K1 ~ B x 2.5e5 / (1 + B / 40 000) transitions/s (measured,
  // profiles/r02_k1_vs_k1s_batch.json).  Round 3 (row-shape dictionary: 2-3 x the instances per CU; four walker
  // wavefronts; specialised, hand-pipelined walker): K1S ~ CUs x G / 320-470 ns -- FrozenLake-20 1.44e10 at 4 096 instances
  // and 1.85e10 at 131 072 (K1: 0.8e9 / 6.6e9), so K1S stays ahead at every batch size measured
  // (profiles/r03_k1s_walkers.txt); the model is kept for batches where few instances fit a CU.
  const double k1_rate = (double)h->B * 2.5e5 / (1.0 + (double)h->B / 4.0e4);
  const double k1s_rate = (double)h->cus * (double)h->k1s.G / 450e-9;
  if (lds && h->k1e_ok && n_steps > 0 && (rk == 6 || wide)) *out = K::K1E;
  else if (ref) *out = K::K1;
  else if (lds && h->k1u_ok && (rk == 5 || (wide && h->k1u_auto))) *out = K::K1U;
  else if (lds && h->tmpl_ok && (rk == 4 || (wide && h->tmpl_auto))) *out = K::K1T;
  else if (lds && (rk == 2 || wide)) *out = h->lds_plan.pipe ? K::K1P : K::K1L;
  else if (k1s && (rk == 3 || (wide && k1_rate < 1.1 * k1s_rate))) *out = K::K1S;
  return CMDP_OK;
}

// K1E / K1U: no device memory for the workspace of a launch's first segment (nothing enqueued yet)
constexpr int kNoWorkspace = 1;

// K1E: per segment of <= K1E_SEG transitions (16-bit counts in the table dwords; the code buffer) the walk kernel, then the
// reward scan over the code words it left in HBM.  The walk accumulates DEPARTURE counts over launches (cmdp_k1e.h), which
// k1e_settle folds into the visit counters before any other kernel or read.
// The form: the pair form (k_rollout_epi<1>, cmdp_k1e_pair.h) when the batch has a pair plan, every instance is at its start
// state with in-episode time 0 (`from_start`: the handle's flag before this call), n is a multiple of H and bit 16 of
// CMDP_K1E_DEBUG ("every round the general way") is clear; its segments are whole episodes.  Else the single form.
static int launch_k1e(cmdp_t* h, const RolloutCall& c, bool from_start) {
  hipStream_t st = h->stream; EnvTables t = h->env();
  if (!h->ev_time[0])   // (timestamps only: no host-visibility cache flush per launch)
    for (int i = 0; i < 5; ++i) HIP_TRY(hipEventCreateWithFlags(&h->ev_time[i], hipEventDisableSystemFence));
  K1ePlan e = h->k1e;
  if (!h->d_k1e_dep.p) {
    const size_t nd = (size_t)grid_for(h->B, K1E_NI) * (size_t)e.gdw;
    HIP_TRY(h->d_k1e_dep.alloc(nd));
    HIP_TRY(h->d_k1e_dep.zero(st));
    HIP_TRY(h->d_k1e_dep_res.alloc(h->B));
    HIP_TRY(h->d_k1e_dep_res.zero(st));
    HIP_TRY(h->d_vis_ovf.alloc(1));
    HIP_TRY(h->d_vis_ovf.zero(st));
  }
  if (h->k1e_pending_steps + c.n > 0x7fff0000LL) { if (int rc = k1e_fold(h)) return rc; }   // the departure image is int32
  e.dep = h->d_k1e_dep.p;
  e.dep_res = h->d_k1e_dep_res.p;
  bool pair = h->k1e_pair_ok && from_start && c.n % e.H == 0 && !(e.debug & 16);
  if (pair && !h->d_k1e_dep2.p) {
    HIP_TRY(h->d_k1e_dep2.alloc((size_t)grid_for(h->B, K1E_NI) * (size_t)e.pgdw));
    HIP_TRY(h->d_k1e_dep2.zero(st));
  }
  e.dep2 = h->d_k1e_dep2.p;
  // The reward scan of a segment runs on the second stream under the walk of the next segment / launch (two sets of code
  // buffers): it is one wavefront per SIMD of sequential sums, the walk fills the rest of the chip (CMDP_K1E_OVERLAP=0: one
  // stream).  cmdp_rollout / cmdp_synchronize / every call that reads the sums waits for it.
  static const int ov_env = std::getenv("CMDP_K1E_OVERLAP") ? std::atoi(std::getenv("CMDP_K1E_OVERLAP")) : 1;
  const bool ov = ov_env != 0;
  if (ov && !h->aux.stream) HIP_TRY(hipStreamCreateWithFlags(&h->aux.stream, hipStreamNonBlocking));
  if (ov && !h->aux.walk[0])
    for (int i = 0; i < 2; ++i) {
      HIP_TRY(hipEventCreateWithFlags(&h->aux.walk[i], hipEventDisableTiming | hipEventDisableSystemFence));
      HIP_TRY(hipEventCreateWithFlags(&h->aux.scan[i], hipEventDisableTiming | hipEventDisableSystemFence));
    }
  if (!ov) { if (int rc = k1e_scan_join(h)) return rc; }
  // segment length: the code words of a segment (8 bytes per episode chunk and instance, two sets) stay within ~1.5 GB
  const int64_t budget_words = std::max<int64_t>(4, (int64_t)((768ll << 20) / (8 * (int64_t)h->B * e.nch)));
  int64_t seg = std::max<int64_t>(e.H, std::min<int64_t>(K1E_SEG, (budget_words - 2) * e.H));
  const int64_t epi_cap = k1e_max_episodes(std::min<int64_t>(c.n, seg), e.H);
  const size_t need = (size_t)epi_cap * (size_t)e.nch * (size_t)h->B;
  if (h->d_k1e_h0.n < (size_t)h->B) HIP_TRY(h->d_k1e_h0.alloc(h->B));
  if (h->d_k1e_h0b.n < (size_t)h->B) HIP_TRY(h->d_k1e_h0b.alloc(h->B));
  // (the pair form stores its code words through 32-bit byte offsets, like the single form's interior rounds)
  pair = pair && need * sizeof(uint2) < ((size_t)1 << 31);
  if (pair) seg -= seg % e.H;   // whole episodes (seg >= H)
  // (the scan's lane keeps its byte offset 8 b in 32 bits for every batch that fits a device: K1rDeviceLoader says what that buys)
  const auto scan = (size_t)h->B * sizeof(uint2) < ((size_t)1 << 31) ? k_reward_scan<true> : k_reward_scan<false>;
  // CMDP_POLICY_RANDOM_REFERENCE: forms 2 / 3 load the action bits K16 makes before each segment's walk (<= 482 blocks of
  // 16 bytes per instance); one buffer, K16 and the walk follow each other on the handle's stream
  const bool ref = c.policy == CMDP_POLICY_RANDOM_REFERENCE;
  if (ref) {
    const size_t nblk_max = (size_t)((std::min<int64_t>(c.n, seg) + 126) >> 7) + 1;
    if (h->d_abits.n < nblk_max * (size_t)h->B) HIP_TRY(h->d_abits.alloc(nblk_max * (size_t)h->B));
    if (!h->ev_as[0])
      for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreateWithFlags(&h->ev_as[i], hipEventDisableSystemFence));
    e.abits = h->d_abits.p;
    if (int rc = pair ? set_lds(k_rollout_epi<3>, h->k1e_pair_lds) : set_lds(k_rollout_epi<2>, h->k1e_lds)) return rc;
  } else if (int rc = pair ? set_lds(k_rollout_epi<1>, h->k1e_pair_lds) : set_lds(k_rollout_epi<0>, h->k1e_lds)) return rc;
  h->k1e_last_form = pair ? 2 : 1;
  for (int64_t s0 = 0; s0 < c.n; s0 += seg) {
    const int64_t n = std::min<int64_t>(seg, c.n - s0);
    const int i = ov ? (int)(h->aux.seq & 1) : 0;
    if (h->d_k1e_codes[i].n < need) {
      if (h->aux.stream) HIP_TRY(hipStreamSynchronize(h->aux.stream));   // a scan may still read the buffer
      if (h->d_k1e_codes[i].alloc(need) != hipSuccess) {
        // no room for the code words (8 bytes per episode chunk and instance): possible before the first segment only (the
        // buffers never shrink)
        (void)hipGetLastError();
        if (s0 > 0) return fail(CMDP_ERR_HIP, "K1E: out of device memory for the code words of a later segment");
        h->d_k1e_codes[i].release();
        return fail(kNoWorkspace, "K1E: out of device memory for %zu code words", need);
      }
    }
    e.codes = h->d_k1e_codes[i].p;
    e.seg_h0 = i ? h->d_k1e_h0b.p : h->d_k1e_h0.p;
    e.n_pass = (int)(((pair ? n / e.H : k1e_max_episodes(n, e.H)) + K1E_EPP - 1) / K1E_EPP);
    // interior rounds: 32-bit byte offsets into codes, and a wavefront's ring starts at a multiple of its own size (the ring
    // address is then formed by OR).  Sixteen rings larger than the tables do not fit the LDS budget, so the rings of every
    // plan are aligned today; were one not, all its rounds would go the general way
    e.fast = !(e.debug & 16) && need * sizeof(uint2) < ((size_t)1 << 31) && k1e_ring_aligned(e);
    if (ov && h->aux.used[i]) HIP_TRY(hipStreamWaitEvent(st, h->aux.scan[i], 0));   // its last scan has read this set
    const bool last = s0 + seg >= c.n;
    if (ref) {   // the segment's action bits, aligned on the instances' transition counters as the walk will read them
      const int nblk = (int)((n + 126) >> 7) + 1;
      if (last) HIP_TRY(hipEventRecord(h->ev_as[0], st));
      hipLaunchKernelGGL(k_mt_actions<true>, dim3(h->B), dim3(K16_THREADS), 0, st, h->d_as_key.p, h->d_as_pos.p, t.n_trans, h->B, h->A,
                         (int)n, nblk, h->d_abits.p, (int8_t*)nullptr, h->d_as_fail.p);
      if (last) HIP_TRY(hipEventRecord(h->ev_as[1], st));
      h->as_unchecked = true;
    }
    if (last) HIP_TRY(hipEventRecord(h->ev_time[0], st));
    // one workgroup per CU (the tables take the CU's LDS), each walking its groups one after the other with the next
    // group's table image in flight under the walk; CMDP_K1E_GRID = workgroups (timing experiments; any value is correct)
    int k1e_grid = std::min(grid_for(h->B, K1E_NI), h->cus);
    if (const char* gs = std::getenv("CMDP_K1E_GRID")) k1e_grid = std::max(1, std::min(grid_for(h->B, K1E_NI), std::atoi(gs)));
    if (ref && pair) hipLaunchKernelGGL(k_rollout_epi<3>, dim3(k1e_grid), dim3(K1E_THREADS), h->k1e_pair_lds, st, t, e, (int)n, c.last);
    else if (ref) hipLaunchKernelGGL(k_rollout_epi<2>, dim3(k1e_grid), dim3(K1E_THREADS), h->k1e_lds, st, t, e, (int)n, c.last);
    else if (pair) hipLaunchKernelGGL(k_rollout_epi<1>, dim3(k1e_grid), dim3(K1E_THREADS), h->k1e_pair_lds, st, t, e, (int)n, c.last);
    else hipLaunchKernelGGL(k_rollout_epi<0>, dim3(k1e_grid), dim3(K1E_THREADS), h->k1e_lds, st, t, e, (int)n, c.last);
    if (last) HIP_TRY(hipEventRecord(h->ev_time[1], st));
    if (ov) {
      HIP_TRY(hipEventRecord(h->aux.walk[i], st));
      HIP_TRY(hipStreamWaitEvent(h->aux.stream, h->aux.walk[i], 0));
      if (last) HIP_TRY(hipEventRecord(h->ev_time[3], h->aux.stream));
      hipLaunchKernelGGL(scan, dim3(grid_for(h->B, K1R_THREADS)), dim3(K1R_THREADS), 0, h->aux.stream, t, e, n, c.rsum, s0 > 0 ? 1 : 0);
      if (last) HIP_TRY(hipEventRecord(h->ev_time[4], h->aux.stream));
      HIP_TRY(hipEventRecord(h->aux.scan[i], h->aux.stream));
      h->aux.used[i] = true;
      h->aux.pending = true;
      h->aux.seq++;
    } else {
      hipLaunchKernelGGL(scan, dim3(grid_for(h->B, K1R_THREADS)), dim3(K1R_THREADS), 0, st, t, e, n, c.rsum, s0 > 0 ? 1 : 0);
      if (last) HIP_TRY(hipEventRecord(h->ev_time[2], st));
    }
  }
  h->ev_time_aux = ov;
  h->k1e_pending = true;
  h->k1e_pending_steps += c.n;
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

// K1U: per segment of <= K1U_SEG transitions the chain kernel (trace -> HBM), then the histogram of that trace
static int launch_k1u(cmdp_t* h, const RolloutCall& c) {
  hipStream_t st = h->stream; EnvTables t = h->env();
  if (!h->ev_time[0])   // (timestamps only: no host-visibility cache flush per launch)
    for (int i = 0; i < 5; ++i) HIP_TRY(hipEventCreateWithFlags(&h->ev_time[i], hipEventDisableSystemFence));
  K1uPlan u = h->k1u;
  const bool pack10 = k1u_form(u) == K1U_FORM_PACK10;
  const int epp = K1U_EPP(pack10);
  const size_t need = (size_t)((std::min<int64_t>(c.n, K1U_SEG) + epp - 1) / epp) * (size_t)h->B;
  const size_t hist_lds = k1h_lds_bytes(h->max_S, 64);
  if (int rc = pack10 ? set_lds(k_rollout_tmpl_stream<true>, h->k1u_lds) : set_lds(k_rollout_tmpl_stream<false>, h->k1u_lds)) return rc;
  if (int rc = pack10 ? set_lds(k_trace_hist<64, 1024, true>, hist_lds) : set_lds(k_trace_hist<64, 1024, false>, hist_lds)) return rc;
  if (h->d_k1u_trace.n < need && h->d_k1u_trace.alloc(need) != hipSuccess) {
    // no room for the trace (16 bytes per 8-12 transitions and instance; every segment of a launch uses the one buffer)
    (void)hipGetLastError();
    h->d_k1u_trace.release();
    return fail(kNoWorkspace, "K1U: out of device memory for a trace of %zu pieces", need);
  }
  if (h->d_k1u_resets.n < (size_t)h->B) HIP_TRY(h->d_k1u_resets.alloc(h->B));
  u.trace = h->d_k1u_trace.p; u.seg_resets = h->d_k1u_resets.p;
  const dim3 rgrid(grid_for(h->B, u.G)), rblock(K1U_THREADS), hgrid(grid_for(h->B, 64)), hblock(1024);
  for (int64_t s0 = 0; s0 < c.n; s0 += K1U_SEG) {
    const int64_t n = std::min<int64_t>(K1U_SEG, c.n - s0);
    const bool last = s0 + K1U_SEG >= c.n;
    if (last) HIP_TRY(hipEventRecord(h->ev_time[0], st));
    if (pack10) hipLaunchKernelGGL(k_rollout_tmpl_stream<true>, rgrid, rblock, h->k1u_lds, st, t, u, n, c.rsum, c.last, s0 > 0 ? 1 : 0);
    else hipLaunchKernelGGL(k_rollout_tmpl_stream<false>, rgrid, rblock, h->k1u_lds, st, t, u, n, c.rsum, c.last, s0 > 0 ? 1 : 0);
    if (last) HIP_TRY(hipEventRecord(h->ev_time[1], st));
    if (pack10) hipLaunchKernelGGL((k_trace_hist<64, 1024, true>), hgrid, hblock, hist_lds, st, t, u.trace, u.seg_resets, n, u.code_shift);
    else hipLaunchKernelGGL((k_trace_hist<64, 1024, false>), hgrid, hblock, hist_lds, st, t, u.trace, u.seg_resets, n, u.code_shift);
    if (last) HIP_TRY(hipEventRecord(h->ev_time[2], st));
  }
  h->ev_time_aux = false;
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

static int launch_k1t(cmdp_t* h, const RolloutCall& c) {
  if (int rc = set_lds(k_rollout_tmpl, h->tmpl_lds)) return rc;
  hipLaunchKernelGGL(k_rollout_tmpl, dim3(grid_for(h->B, h->tmpl_plan.G)), dim3(K1T_THREADS), h->tmpl_lds, h->stream, h->env(),
                     h->tmpl_plan, c.n, c.rsum, c.last);
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

static int launch_k1lp(cmdp_t* h, const RolloutCall& c) {
  hipStream_t st = h->stream; EnvTables t = h->env();
  const dim3 lgrid(grid_for(h->B, h->lds_plan.G)), lblock(K1L_THREADS);
  const int form = k1lp_form(h->lds_plan);
  if (form == K1LP_FORM_PIPE) {
    if (int rc = set_lds(k_rollout_pipe, h->lds_bytes)) return rc;
    hipLaunchKernelGGL(k_rollout_pipe, lgrid, dim3(K1P_THREADS), h->lds_bytes, st, t, h->lds_plan, c.n, c.rsum, c.last);
  } else if (form == K1LP_FORM_PACKED) {
    if (int rc = set_lds(k_rollout_lds<true>, h->lds_bytes)) return rc;
    hipLaunchKernelGGL(k_rollout_lds<true>, lgrid, lblock, h->lds_bytes, st, t, h->lds_plan, c.n, c.rsum, c.last);
  } else {
    if (int rc = set_lds(k_rollout_lds<false>, h->lds_bytes)) return rc;
    hipLaunchKernelGGL(k_rollout_lds<false>, lgrid, lblock, h->lds_bytes, st, t, h->lds_plan, c.n, c.rsum, c.last);
  }
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

static int launch_k1s(cmdp_t* h, const RolloutCall& c) {
  if (int rc = set_lds(k_rollout_stoch, h->k1s_bytes)) return rc;
  hipLaunchKernelGGL(k_rollout_stoch, dim3(grid_for(h->B, h->k1s.G)), dim3(K1S_THREADS), h->k1s_bytes, h->stream, h->env(), h->k1s,
                     c.n, c.rsum, c.last);
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

static int launch_k1d(cmdp_t* h, const RolloutCall& c) {
  hipStream_t st = h->stream; EnvTables t = h->env();
  DenseArgs dn{h->d_dense.p, h->dense_spad};
  // two instances per wavefront (software-pipelined: one row in flight while the other is scanned) when the row fits
  // the registers twice; CMDP_K1D_NI = 1 / 2 overrides (tuning aid)
  static const int ni_env = std::getenv("CMDP_K1D_NI") ? std::atoi(std::getenv("CMDP_K1D_NI")) : 0;
  const int nv = h->dense_spad / 256;
  const int ni = ni_env ? ni_env : (nv <= 4 ? 2 : 1);
  const dim3 dgrid(grid_for(h->B, 4 * ni));
#define DENSE_LAUNCH(P, NV, BT, NI) \
  hipLaunchKernelGGL((k_rollout_dense<P, NV, BT, NI>), dgrid, dim3(256), 0, st, t, dn, c.actions, c.n, c.rsum, c.last)
#define DENSE_CASE(NV, NI)                                                                        \
  if (nv == NV && ni == NI) {                                                                     \
    if (c.policy == CMDP_POLICY_RANDOM) { if (h->sample_beta) DENSE_LAUNCH(0, NV, true, NI); else DENSE_LAUNCH(0, NV, false, NI); } \
    else { if (h->sample_beta) DENSE_LAUNCH(1, NV, true, NI); else DENSE_LAUNCH(1, NV, false, NI); }      \
  } else
  DENSE_CASE(1, 1) DENSE_CASE(2, 1) DENSE_CASE(3, 1) DENSE_CASE(4, 1) DENSE_CASE(6, 1) DENSE_CASE(8, 1) DENSE_CASE(12, 1)
  DENSE_CASE(16, 1) DENSE_CASE(1, 2) DENSE_CASE(2, 2) DENSE_CASE(3, 2) DENSE_CASE(4, 2)
  { return fail(CMDP_ERR_UNSUPPORTED, "dense layout: no kernel for a row stride of %d floats, %d instances per wavefront", h->dense_spad, ni); }
#undef DENSE_CASE
#undef DENSE_LAUNCH
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

// K1, lane = instance, tables in HBM: the reward-cache form (park protocol, every policy), the greedy-Q form, the plain one
static int launch_k1(cmdp_t* h, RolloutKernel k, const RolloutCall& c) {
  hipStream_t st = h->stream; EnvTables t = h->env();
  const dim3 grid(grid_for(h->B, 256)), block(256);
  const bool trace = c.trace(), bt = h->sample_beta;
  if (k == RolloutKernel::K1_REWARD_CACHE) {
    const RewardCache rc = h->rcache();
#define ROLL_RC(P, TR) \
  hipLaunchKernelGGL((k_rollout<P, TR, false, true>), grid, block, 0, st, t, c.actions, c.n, c.rsum, c.last, c.tobs, c.trew, c.ttype, c.q, rc, c.resume)
    if (c.policy == CMDP_POLICY_RANDOM) { if (trace) ROLL_RC(0, true); else ROLL_RC(0, false); }
    else if (c.policy == CMDP_POLICY_HOST_ACTIONS) { if (trace) ROLL_RC(1, true); else ROLL_RC(1, false); }
    else { if (trace) ROLL_RC(2, true); else ROLL_RC(2, false); }
#undef ROLL_RC
  } else if (k == RolloutKernel::K1_GREEDY) {
    if (trace) hipLaunchKernelGGL((k_rollout<2, true, true>), grid, block, 0, st, t, c.actions, c.n, c.rsum, c.last, c.tobs, c.trew, c.ttype, c.q);
    else hipLaunchKernelGGL((k_rollout<2, false, true>), grid, block, 0, st, t, c.actions, c.n, c.rsum, c.last, c.tobs, c.trew, c.ttype, c.q);
  } else {
#define ROLL(P, TR, BT) \
  hipLaunchKernelGGL((k_rollout<P, TR, BT>), grid, block, 0, st, t, c.actions, c.n, c.rsum, c.last, c.tobs, c.trew, c.ttype)
    if (c.policy == CMDP_POLICY_RANDOM) {
      if (trace) { if (bt) ROLL(0, true, true); else ROLL(0, true, false); }
      else { if (bt) ROLL(0, false, true); else ROLL(0, false, false); }
    } else {
      if (trace) { if (bt) ROLL(1, true, true); else ROLL(1, true, false); }
      else { if (bt) ROLL(1, false, true); else ROLL(1, false, false); }
    }
#undef ROLL
  }
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

// Pick, check the visit bound, settle what K1E left on the second stream and in its departure image (every other kernel
// reads and writes the sums and counters itself), launch.  The caller commits the visit bound.
static int launch_rollout(cmdp_t* h, const RolloutCall& c0) {
  using K = RolloutKernel;
  RolloutCall c = c0;
  // whole episodes walked from reset end at reset again, whichever kernel walks them (only K1E's pair form asks)
  const bool from_start = h->at_start, stays = from_start && h->k1e_pair_ok && h->H > 0 && c.n % h->H == 0;
  for (;;) {
    K k = K::K1;
    if (int rc = pick_rollout(h, c.policy, c.trace(), c.n, &k)) return rc;
    if (int rc = visits_check(h, c.n)) return rc;
    if (k != K::K1E) { if (int rc = k1e_settle(h)) return rc; }
    if (k != K::K1E && c.policy == CMDP_POLICY_RANDOM_REFERENCE) {
      // K1E had no workspace (the callers hand every other kernel CMDP_POLICY_HOST_ACTIONS themselves): the byte form now
      if (int rc = reference_actions(h, c.n, &c.actions)) return rc;
      c.policy = CMDP_POLICY_HOST_ACTIONS;
    }
    int rc = CMDP_OK;
    switch (k) {
      case K::K1E: rc = launch_k1e(h, c, from_start); break;
      case K::K1U: rc = launch_k1u(h, c); break;
      case K::K1T: rc = launch_k1t(h, c); break;
      case K::K1L: case K::K1P: rc = launch_k1lp(h, c); break;
      case K::K1S: rc = launch_k1s(h, c); break;
      case K::K1D: rc = launch_k1d(h, c); break;
      default: rc = launch_k1(h, k, c); break;
    }
    if (rc == CMDP_OK) h->at_start = stays;
    if (rc != kNoWorkspace) return rc;
    // the chain kernels need no workspace: this handle takes them from now on, unless K1E / K1U was forced
    (k == K::K1E ? h->k1e_ok : h->k1u_ok) = false;
    if (h->rollout_kernel) return CMDP_ERR_HIP;   // (the launcher has said why)
  }
}

int cmdp_rollout(cmdp_t* h, int policy, const void* policy_arg, int64_t n_steps, int32_t* last_obs, double* reward_sum,
                 int32_t* trace_obs, double* trace_reward, uint8_t* trace_type) {
  if (int rc = bind(h, false)) return rc;   // (launch_rollout settles K1E unless it takes K1E again)
  if (!h->has_env) return fail(CMDP_ERR_INVALID, "handle was created without the sampler half");
  if (n_steps < 0) return fail(CMDP_ERR_INVALID, "n_steps < 0");
  const bool ref = policy == CMDP_POLICY_RANDOM_REFERENCE;
  if (policy != CMDP_POLICY_RANDOM && policy != CMDP_POLICY_HOST_ACTIONS && policy != CMDP_POLICY_GREEDY_Q && !ref)
    return fail(CMDP_ERR_INVALID, "policy");
  if (policy != CMDP_POLICY_RANDOM && !ref && !policy_arg && n_steps > 0) return fail(CMDP_ERR_INVALID, "policy_arg missing");
  if (ref && !h->as_set) return fail(CMDP_ERR_INVALID, "CMDP_POLICY_RANDOM_REFERENCE: cmdp_set_action_streams has not been called on this handle");
  RolloutKernel ref_kernel = RolloutKernel::K1;
  if (ref) { if (int rc = pick_rollout(h, policy, trace_obs || trace_reward || trace_type, n_steps, &ref_kernel)) return rc; }
  bool any = false;
  if (int rc = any_needs_reset(h, &any)) return rc;
  if (any) return fail(CMDP_ERR_NEEDS_RESET, "rollout() on an instance that needs reset()");
  h->known_reset = true;  // the fused loop resets at once after every terminating step
  hipStream_t st = h->stream;
  const int B = h->B;
  const size_t NB = (size_t)n_steps * B;
  const int8_t* d_act = nullptr;
  if (policy == CMDP_POLICY_HOST_ACTIONS) {
    const int8_t* a = static_cast<const int8_t*>(policy_arg);
    for (size_t i = 0; i < NB; ++i)
      if (a[i] < 0 || a[i] >= h->A) return fail(CMDP_ERR_INVALID, "action out of range [0, %d)", h->A);
    HIP_TRY(h->d_actions8.upload(a, NB, st));
    d_act = h->d_actions8.p;
  }
  if (ref && ref_kernel != RolloutKernel::K1E) {
    if (int rc = reference_actions(h, n_steps, &d_act)) return rc;
    policy = CMDP_POLICY_HOST_ACTIONS;
  }
  const float* d_q = nullptr;
  if (policy == CMDP_POLICY_GREEDY_Q) {
    HIP_TRY(h->d_gp_q.upload(static_cast<const float*>(policy_arg), (size_t)(h->H > 0 ? h->H : 1) * h->n_rows, st));
    d_q = h->d_gp_q.p;
  }
  if (h->d_rsum.n < (size_t)B) HIP_TRY(h->d_rsum.alloc(B));
  if (h->d_last_obs.n < (size_t)B) HIP_TRY(h->d_last_obs.alloc(B));
  if (trace_obs && h->d_tr_obs.n < NB) HIP_TRY(h->d_tr_obs.alloc(NB));
  if (trace_reward && h->d_tr_rew.n < NB) HIP_TRY(h->d_tr_rew.alloc(NB));
  if (trace_type && h->d_tr_type.n < NB) HIP_TRY(h->d_tr_type.alloc(NB));
  auto launch = [&](int resume) -> int {
    return launch_rollout(h, {policy, d_act, d_q, n_steps, h->d_rsum.p, h->d_last_obs.p, trace_obs ? h->d_tr_obs.p : nullptr,
                              trace_reward ? h->d_tr_rew.p : nullptr, trace_type ? h->d_tr_type.p : nullptr, resume});
  };
  if (int rc = visits_commit(h, n_steps, h->reward_cache ? rc_drive(h, launch) : launch(0))) return rc;
  if (int rc = k1e_scan_join(h)) return rc;   // (K1E: the sums of the last segment come from the second stream)
  if (last_obs) HIP_TRY(hipMemcpyAsync(last_obs, h->d_last_obs.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
  if (reward_sum) HIP_TRY(hipMemcpyAsync(reward_sum, h->d_rsum.p, sizeof(double) * B, hipMemcpyDeviceToHost, st));
  if (trace_obs) HIP_TRY(hipMemcpyAsync(trace_obs, h->d_tr_obs.p, sizeof(int32_t) * NB, hipMemcpyDeviceToHost, st));
  if (trace_reward) HIP_TRY(hipMemcpyAsync(trace_reward, h->d_tr_rew.p, sizeof(double) * NB, hipMemcpyDeviceToHost, st));
  if (trace_type) HIP_TRY(hipMemcpyAsync(trace_type, h->d_tr_type.p, NB, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return action_streams_check(h);
}

int cmdp_rollout_async(cmdp_t* h, int policy, int64_t n_steps) {
  if (int rc = bind(h, false)) return rc;   // (launch_rollout settles K1E unless it takes K1E again)
  if (!h->has_env) return fail(CMDP_ERR_INVALID, "handle was created without the sampler half");
  const bool ref = policy == CMDP_POLICY_RANDOM_REFERENCE;
  if (policy != CMDP_POLICY_RANDOM && !ref)
    return fail(CMDP_ERR_INVALID, "rollout_async supports CMDP_POLICY_RANDOM and CMDP_POLICY_RANDOM_REFERENCE only");
  if (n_steps < 0) return fail(CMDP_ERR_INVALID, "n_steps < 0");
  if (ref && !h->as_set) return fail(CMDP_ERR_INVALID, "CMDP_POLICY_RANDOM_REFERENCE: cmdp_set_action_streams has not been called on this handle");
  RolloutKernel ref_kernel = RolloutKernel::K1;
  if (ref) { if (int rc = pick_rollout(h, policy, false, n_steps, &ref_kernel)) return rc; }
  if (!h->known_reset) {  // one 4-byte read-back on the first call after create / cmdp_step, none afterwards
    bool any = false;
    if (int rc = any_needs_reset(h, &any)) return rc;
    if (any) return fail(CMDP_ERR_NEEDS_RESET, "rollout_async() on an instance that needs reset()");
    h->known_reset = true;
  }
  if (h->d_rsum.n < (size_t)h->B) HIP_TRY(h->d_rsum.alloc(h->B));
  if (h->d_last_obs.n < (size_t)h->B) HIP_TRY(h->d_last_obs.alloc(h->B));
  const int8_t* d_act = nullptr;
  if (ref && ref_kernel != RolloutKernel::K1E) {
    if (int rc = reference_actions(h, n_steps, &d_act)) return rc;
    policy = CMDP_POLICY_HOST_ACTIONS;
  }
  auto launch = [&](int resume) -> int {
    return launch_rollout(h, {policy, d_act, nullptr, n_steps, h->d_rsum.p, h->d_last_obs.p, nullptr, nullptr, nullptr, resume});
  };
  // (reward caches: the park / fill / relaunch loop needs the host -- synchronous in this mode)
  return visits_commit(h, n_steps, h->reward_cache ? rc_drive(h, launch) : launch(0));
}

int cmdp_set_option(cmdp_t* h, int option, int64_t value) {
  if (!h) return fail(CMDP_ERR_INVALID, "null handle");
  if (option == CMDP_OPT_ROLLOUT_KERNEL && value >= 0 && value <= 6) {
    h->rollout_kernel = (int)value;
    return CMDP_OK;
  }
  if (option == CMDP_OPT_LDS_GROUPS_PER_CU && (value == 1 || value == 2)) {
    if (!h->lds_ok) return fail(CMDP_ERR_INVALID, "the batch is not eligible for the LDS-resident rollout kernels");
    if (h->lds_plan.pipe)
      return fail(CMDP_ERR_UNSUPPORTED, "this handle runs the pipeline kernel K1P, one workgroup per CU by construction "
                  "(its successor table is encoded for K1P at cmdp_create: set CMDP_K1L_PIPE=0 before creating the handle to use K1L)");
    const int cap = value == 1 ? h->lds_G1 : h->lds_G2;
    if (cap < 1) return fail(CMDP_ERR_INVALID, "no room for %lld workgroups per CU", (long long)value);
    h->lds_plan.G = even_groups(h->B, cap, (int64_t)h->cus * value).G;   // (as cmdp_create plans it)
    h->lds_per_cu = (int)value;
    h->lds_bytes = k1l_lds_bytes(h->lds_plan, h->lds_plan.G);
    return CMDP_OK;
  }
  if (option == CMDP_OPT_DP_KERNEL && value >= 0 && value <= 7) {
    h->dp_kernel = (int)value;
    return CMDP_OK;
  }
  if (option == CMDP_OPT_CHAIN_EXACT_ORDER && (value == 0 || value == 1)) {
    h->chain_exact = value == 1;
    return CMDP_OK;
  }
  if (option == CMDP_OPT_MIXING_PATH && value >= 0 && value <= 2) {
    h->mixing_path = (int)value;
    return CMDP_OK;
  }
  if (option == CMDP_OPT_DIAMETER_WORKSPACE_MB && value >= 1) {
    h->dl_ws_bytes = (size_t)value << 20;
    return CMDP_OK;
  }
  if (option == CMDP_OPT_DIAMETER_RELABEL_MIN_STATES && value >= 0) {
    h->relabel_min_states = value;
    h->ell_K = 0;  // the fixed-width rows are rebuilt by the next K5S launch
    return CMDP_OK;
  }
  return fail(CMDP_ERR_INVALID, "unknown option %d / value %lld", option, (long long)value);
}

int cmdp_lds_plan(cmdp_t* h, int32_t plan[4]) {
  if (!h || !plan) return fail(CMDP_ERR_INVALID, "bad argument");
  // what a launch of the random policy without trace and of >= 64 transitions takes; when that is no LDS-resident kernel,
  // the one the batch is eligible for
  RolloutKernel k = RolloutKernel::K1;
  const std::string err = g_err;   // (a forced kernel the batch cannot take is no error of this call)
  if (pick_rollout(h, CMDP_POLICY_RANDOM, false, 64, &k) != CMDP_OK) k = RolloutKernel::K1;
  g_err = err;
  const int32_t k1e[3] = {5, K1E_NI, K1E_EPP}, k1u[3] = {4, h->k1u.G, h->k1u.ch}, k1t[3] = {3, h->tmpl_plan.G, h->tmpl_plan.ch},
                k1lp[3] = {h->lds_plan.pipe, h->lds_plan.G, h->lds_plan.ch}, k1s[3] = {2, h->k1s.G, h->k1s.ch}, none[3] = {0, 0, 0};
  const int32_t* p = k == RolloutKernel::K1E ? k1e : k == RolloutKernel::K1U ? k1u : k == RolloutKernel::K1T ? k1t
                     : h->lds_ok ? k1lp : h->k1s_ok ? k1s : none;   // (K1L / K1P / K1S: the batch's only LDS-resident kernel)
  plan[0] = (h->lds_ok || h->k1s_ok) ? 1 : 0;
  std::copy(p, p + 3, plan + 1);
  return CMDP_OK;
}

// cmdp_k1s_plan / cmdp_k1s_plan_desc: the fields of a K1S plan in the order include/cmdp.h gives
static void k1s_plan_report(bool ok, const K1sPlan& p, int32_t out[CMDP_K1S_PLAN_FIELDS]) {
  std::fill(out, out + CMDP_K1S_PLAN_FIELDS, 0);
  if (!ok) return;
  const int32_t v[CMDP_K1S_PLAN_FIELDS] = {1, p.G, p.nw, p.gw, p.team, p.U, p.n_pat, p.n_codes, p.reward_mode, p.rc_packed, p.n_shapes,
                                           p.shape_bytes, p.ch, k1s_walk_form(p.n_pat, p.shape_bytes, p.team, p.rc_packed, p.reward_mode)};
  std::copy(v, v + CMDP_K1S_PLAN_FIELDS, out);
}

int cmdp_k1e_pair_plan(cmdp_t* h, int32_t out[CMDP_K1E_PAIR_PLAN_FIELDS]) {
  if (!h || !out) return fail(CMDP_ERR_INVALID, "bad argument");
  k1e_pair_plan_report(h->k1e_ok && h->k1e_pair_ok, h->k1e, h->k1e_sp2, h->k1e_n_even, h->k1e_last_form, out);
  return CMDP_OK;
}

int cmdp_k1s_plan(cmdp_t* h, int32_t out[CMDP_K1S_PLAN_FIELDS]) {
  if (!h || !out) return fail(CMDP_ERR_INVALID, "bad argument");
  k1s_plan_report(h->k1s_ok, h->k1s, out);
  return CMDP_OK;
}

// As much of cmdp_create's validation of a bare description as the planners index by, and their input: row descriptors,
// the largest state count, whether any reward is a Beta entry.  `who` names the caller in the message.
static int plan_input_of_desc(const cmdp_desc* d, int cus, const char* who, std::vector<RowDesc>* rows, PlanInput* in, bool* any_beta) {
  if (d->n_instances < 1 || d->n_actions < 1 || !d->state_off || !d->sp_ptr || !d->sp_next || !d->sp_cum || !d->sp_reward ||
      !d->start_off)
    return fail(CMDP_ERR_INVALID, "%s needs the sampler half of the description", who);
  const int B = d->n_instances, A = d->n_actions;
  int max_S = 0;
  if (d->state_off[0] != 0 || d->sp_ptr[0] != 0 || d->start_off[0] != 0) return fail(CMDP_ERR_INVALID, "offsets do not start at 0");
  for (int b = 0; b < B; ++b) {
    const int64_t S = d->state_off[b + 1] - d->state_off[b];
    if (S < 1 || S > (1 << 28)) return fail(CMDP_ERR_INVALID, "instance %d has %lld states", b, (long long)S);
    if (d->start_off[b + 1] - d->start_off[b] < 1) return fail(CMDP_ERR_INVALID, "instance %d has no starting state", b);
    max_S = std::max<int>(max_S, (int)S);
  }
  const int64_t R = d->state_off[B] * A;
  rows->resize((size_t)R);
  *any_beta = false;
  for (int b = 0; b < B; ++b) {
    const int64_t S = d->state_off[b + 1] - d->state_off[b];
    for (int64_t r = d->state_off[b] * A; r < d->state_off[b + 1] * A; ++r) {
      const int64_t lo = d->sp_ptr[r], n = d->sp_ptr[r + 1] - lo;
      if (n < 1 || n > 4096) return fail(CMDP_ERR_INVALID, "row %lld has %lld successors", (long long)r, (long long)n);
      for (int64_t e = lo; e < lo + n; ++e) {
        if (d->sp_next[e] < 0 || d->sp_next[e] >= S) return fail(CMDP_ERR_INVALID, "successor index out of range at entry %lld", (long long)e);
        *any_beta |= d->sp_rkind && d->sp_rkind[e] != 0;
      }
      RowDesc rd{};
      rd.n = (int32_t)n;
      rd.next_if_det = d->sp_next[lo];
      rd.reward_if_det = d->sp_reward[lo];
      (*rows)[(size_t)r] = rd;
    }
  }
  *in = PlanInput{d, rows->data(), B, A, d->horizon, max_S, cus};
  return CMDP_OK;
}

// the rewards are the table's values (install_rollout_plans: neither sampled Beta rewards nor reward caches)
static bool desc_table_rewards(const cmdp_desc* d, bool any_beta) {
  return !any_beta || (d->flags & (CMDP_FLAG_REWARD_MEANS | CMDP_FLAG_REWARD_CACHE)) == CMDP_FLAG_REWARD_MEANS;
}

int cmdp_k1s_plan_desc(const cmdp_desc* d, int cus, int instances_per_workgroup, int32_t out[CMDP_K1S_PLAN_FIELDS]) {
  if (!d || !out || cus < 1 || instances_per_workgroup < 0) return fail(CMDP_ERR_INVALID, "bad argument");
  std::vector<RowDesc> rows;
  PlanInput in{};
  bool any_beta = false;
  if (int rc = plan_input_of_desc(d, cus, "cmdp_k1s_plan_desc", &rows, &in, &any_beta)) return rc;
  // cmdp_create plans K1S for the Philox batches with table rewards that K1L / K1P refuse (install_rollout_plans)
  PlanKnobs knobs;
  knobs.k1s_G = instances_per_workgroup;
  K1sChoice ks;
  const bool table_rewards = desc_table_rewards(d, any_beta);
  DetTables t;
  if (table_rewards && d->rng_mode == CMDP_RNG_PHILOX && d->layout == CMDP_LAYOUT_CSR && !(det_tables(in, &t) && plan_k1lp(in, t, knobs).ok))
    ks = plan_k1s(in, knobs);
  k1s_plan_report(ks.ok, ks.p, out);
  return CMDP_OK;
}

int cmdp_det_plan(cmdp_t* h, int32_t out[CMDP_DET_PLAN_FIELDS]) {
  if (!h || !out) return fail(CMDP_ERR_INVALID, "bad argument");
  DetPlans d;
  d.lds_ok = h->lds_ok; d.lp = h->lds_plan; d.succ_bits = h->lds_succ_bits; d.per_cu = h->lds_per_cu;
  d.lp_cap = h->lds_per_cu == 2 ? h->lds_G2 : h->lds_G1;
  d.tmpl_ok = h->tmpl_ok; d.tmpl_auto = h->tmpl_auto; d.kt = h->tmpl_plan; d.kt_cap = h->tmpl_cap;
  d.k1u_ok = h->k1u_ok; d.k1u_auto = h->k1u_auto; d.ku = h->k1u; d.ku_cap = h->k1u_cap; d.max_S = h->max_S;
  det_plan_report(d, out);
  return CMDP_OK;
}

int cmdp_det_plan_desc(const cmdp_desc* d, int cus, const int32_t knobs_in[5], int32_t out[CMDP_DET_PLAN_FIELDS]) {
  if (!d || !out || cus < 1) return fail(CMDP_ERR_INVALID, "bad argument");
  std::vector<RowDesc> rows;
  PlanInput in{};
  bool any_beta = false;
  if (int rc = plan_input_of_desc(d, cus, "cmdp_det_plan_desc", &rows, &in, &any_beta)) return rc;
  PlanKnobs knobs;
  if (knobs_in) {
    knobs.pipe = knobs_in[0] < 0 ? -1 : knobs_in[0];
    knobs.k1l_G = std::max(0, knobs_in[1]);
    knobs.k1t_G = std::max(0, knobs_in[2]);
    knobs.k1u_G = std::max(0, knobs_in[3]);
    knobs.k1t_ch = std::max(0, knobs_in[4]);
  }
  // as install_rollout_plans (a batch that passes det_tables has no MT19937 slots: its rows and starts draw nothing)
  DetTables t;
  K1lpChoice lp;
  if (desc_table_rewards(d, any_beta) && det_tables(in, &t)) lp = plan_k1lp(in, t, knobs);
  K1tChoice kt;
  K1uChoice ku;
  if (lp.ok) {
    kt = plan_k1t(in, t, lp, knobs);
    ku = plan_k1u(in, kt, knobs);
  }
  det_plan_report(det_plans_of(lp, kt, ku, in.max_S), out);
  return CMDP_OK;
}

int cmdp_k1e_pair_plan_desc(const cmdp_desc* d, int cus, int instance, int32_t out[CMDP_K1E_PAIR_PLAN_FIELDS], int32_t* n_even,
                            int32_t* index, int32_t* inverse, uint16_t* words) {
  if (!d || !out || cus < 1) return fail(CMDP_ERR_INVALID, "bad argument");
  std::vector<RowDesc> rows;
  PlanInput in{};
  bool any_beta = false;
  if (int rc = plan_input_of_desc(d, cus, "cmdp_k1e_pair_plan_desc", &rows, &in, &any_beta)) return rc;
  if (instance < 0 || instance >= in.B) return fail(CMDP_ERR_INVALID, "instance %d of %d", instance, in.B);
  // as install_rollout_plans: K1E is planned for the batches K1L / K1P take
  const PlanKnobs knobs;
  DetTables t;
  K1eChoice ke;
  if (desc_table_rewards(d, any_beta) && d->start_state && det_tables(in, &t) && plan_k1lp(in, t, knobs).ok) ke = plan_k1e(in, t, knobs);
  const K1ePairChoice& pc = ke.pair;
  k1e_pair_plan_report(ke.ok && pc.ok, ke.e, pc.SP2, pc.n_even, 0, out);
  if (n_even) *n_even = 0;
  if (!(ke.ok && pc.ok)) return CMDP_OK;
  const size_t b = (size_t)instance;
  if (n_even) *n_even = pc.n_even_of[b];
  if (index) std::copy(pc.index.begin() + b * in.max_S, pc.index.begin() + (b + 1) * in.max_S, index);
  if (inverse)
    for (int x = 0; x < pc.SP2; ++x) inverse[x] = x < pc.n_even_of[b] ? (int32_t)pc.inv[b * pc.SP2 + x] : -1;
  if (words) std::copy(pc.words.begin() + b * pc.SP2 * 4, pc.words.begin() + (b + 1) * pc.SP2 * 4, words);
  return CMDP_OK;
}

int cmdp_synchronize(cmdp_t* h) {
  if (int rc = bind(h, false)) return rc;   // (the departure image of K1E stays as it is: nothing here reads the counters)
  if (int rc = k1e_scan_join(h)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return action_streams_check(h);
}

int cmdp_stat(cmdp_t* h, int which, double* out) {
  if (int rc = bind(h)) return rc;
  if (!out) return fail(CMDP_ERR_INVALID, "null output");
  if (which == CMDP_STAT_DP_KERNEL_MS) {
    if (!h->ev_dp0) return fail(CMDP_ERR_INVALID, "no discounted solve has run on this handle");
    HIP_TRY(hipEventSynchronize(h->ev_dp1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev_dp0, h->ev_dp1));
    *out = ms;
    return CMDP_OK;
  }
  if (which == CMDP_STAT_DP_KERNEL) {
    *out = h->last_dp_kernel;
    return CMDP_OK;
  }
  if (which == CMDP_STAT_ROLLOUT_KERNEL_MS || which == CMDP_STAT_HIST_KERNEL_MS) {
    if (!h->ev_time[0]) return fail(CMDP_ERR_INVALID, "no streamed-trace (K1U) or episode-parallel (K1E) rollout has run on this handle");
    const bool hist = which == CMDP_STAT_HIST_KERNEL_MS;
    hipEvent_t e0 = hist ? (h->ev_time_aux ? h->ev_time[3] : h->ev_time[1]) : h->ev_time[0];
    hipEvent_t e1 = hist ? (h->ev_time_aux ? h->ev_time[4] : h->ev_time[2]) : h->ev_time[1];
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *out = ms;
    return CMDP_OK;
  }
  if (which == CMDP_STAT_ACTIONS_KERNEL_MS) {
    if (!h->ev_as[0]) return fail(CMDP_ERR_INVALID, "no K1E rollout under CMDP_POLICY_RANDOM_REFERENCE has run on this handle");
    HIP_TRY(hipEventSynchronize(h->ev_as[1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev_as[0], h->ev_as[1]));
    *out = ms;
    return CMDP_OK;
  }
  if (which == CMDP_STAT_CHAIN_FAST_INSTANCES) {
    if (!h->cf.ran) { *out = 0.0; return CMDP_OK; }   // K9 alone: no plan, K9F beyond the LDS budget, exact order
    std::vector<uint8_t> slow((size_t)h->B);
    HIP_TRY(hipMemcpyAsync(slow.data(), h->cf.slow.p, (size_t)h->B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int n = 0;
    for (uint8_t x : slow) n += x == 0;
    *out = (double)n;
    return CMDP_OK;
  }
  if (which == CMDP_STAT_REWARD_FILLS || which == CMDP_STAT_REWARD_ROUNDS) {
    *out = (double)(which == CMDP_STAT_REWARD_FILLS ? h->rc_fills : h->rc_rounds);
    return CMDP_OK;
  }
  if (which == CMDP_STAT_DIAMETER_KERNEL) {
    *out = h->last_diam_kernel;
    return CMDP_OK;
  }
  if (which == CMDP_STAT_DIAMETER_CLUSTER_LAUNCHES || which == CMDP_STAT_DIAMETER_CLUSTER_FALLBACKS) {
    *out = (double)(which == CMDP_STAT_DIAMETER_CLUSTER_LAUNCHES ? h->k5c_launches : h->k5c_timeouts);
    return CMDP_OK;
  }
  if (which == CMDP_STAT_REWARD_FILL_MS || which == CMDP_STAT_REWARD_ROUND_MS) {
    *out = which == CMDP_STAT_REWARD_FILL_MS ? h->rc_fill_ms : h->rc_round_ms;
    return CMDP_OK;
  }
  if (which == CMDP_STAT_UCRL2_WAIT_MS) {
    *out = h->uc_wait_ms;
    return CMDP_OK;
  }
  if (which == CMDP_STAT_UCRL2_ROUNDS || which == CMDP_STAT_UCRL2_SOLVES || which == CMDP_STAT_UCRL2_ROUND_MS) {
    *out = which == CMDP_STAT_UCRL2_ROUNDS ? (double)h->uc_rounds : which == CMDP_STAT_UCRL2_SOLVES ? (double)h->uc_solves : h->uc_round_ms;
    return CMDP_OK;
  }
  if (which >= CMDP_STAT_PSRL_ROUNDS && which <= CMDP_STAT_PSRL_REFERENCE_MS) {
    *out = which == CMDP_STAT_PSRL_ROUNDS ? (double)h->ps_rounds : which == CMDP_STAT_PSRL_SOLVES ? (double)h->ps_solves
           : which == CMDP_STAT_PSRL_SAMPLE_KERNEL_MS ? h->ps_sample_ms : which == CMDP_STAT_PSRL_VI_KERNEL_MS ? h->ps_vi_ms : h->ps_ref_ms;
    return CMDP_OK;
  }
  if (which == CMDP_STAT_UCRL2_POLICY_KERNEL_MS || which == CMDP_STAT_PSRL_POLICY_KERNEL_MS) {
    *out = which == CMDP_STAT_UCRL2_POLICY_KERNEL_MS ? h->uc_policy_ms : h->ps_policy_ms;
    return CMDP_OK;
  }
  if (which == CMDP_STAT_UCRL2_POLICY_SOLVED || which == CMDP_STAT_UCRL2_POLICY_REUSED) {
    *out = (double)(which == CMDP_STAT_UCRL2_POLICY_SOLVED ? h->uc_policy_solved : h->uc_policy_reused);
    return CMDP_OK;
  }
  if (which == CMDP_STAT_PSRL_SAMPLE_BYTES || which == CMDP_STAT_PSRL_SAMPLE_SOLVER) {
    *out = which == CMDP_STAT_PSRL_SAMPLE_BYTES ? h->ps_sample_bytes : (double)h->ps_sample_solver;
    return CMDP_OK;
  }
  if (which == CMDP_STAT_PSRL_UNCONVERGED || which == CMDP_STAT_PSRL_SWEEPS) {
    unsigned long long n[2] = {0, 0};
    if (h->d_ps_tally.p) {
      HIP_TRY(hipMemcpyAsync(n, h->d_ps_tally.p, sizeof n, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
    }
    *out = (double)n[which == CMDP_STAT_PSRL_UNCONVERGED ? 0 : 1];
    return CMDP_OK;
  }
  if (which == CMDP_STAT_UCRL2_UNCONVERGED) {
    int32_t n = 0;
    if (h->d_uc_unconverged.p) {
      HIP_TRY(hipMemcpyAsync(&n, h->d_uc_unconverged.p, sizeof n, hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(hipStreamSynchronize(h->stream));
    }
    *out = (double)n;
    return CMDP_OK;
  }
  return fail(CMDP_ERR_INVALID, "unknown statistic %d", which);
}

int cmdp_calibrate(int what, int64_t n_steps, double* ns_per_step) {
  if (!ns_per_step || n_steps < 1 || n_steps > 10000000) return fail(CMDP_ERR_INVALID, "bad argument");
  if (what != CMDP_CALIB_LDS_READ && what != CMDP_CALIB_LDS_CHAIN && what != CMDP_CALIB_LDS_CHAIN_SHARED)
    return fail(CMDP_ERR_INVALID, "unknown calibration %d", what);
  int dev = 0, cus = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  DevBuf<int32_t> sink;
  HIP_TRY(sink.alloc((size_t)cus * 64));
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  const size_t lds = 64 * 1024;
  for (int rep = 0; rep < 2; ++rep) {  // the first launch warms the code object up
    const int n = rep == 0 ? 1000 : (int)n_steps;
    HIP_TRY(hipEventRecord(e0, nullptr));
    if (what == CMDP_CALIB_LDS_READ) hipLaunchKernelGGL(k_calib_lds_chain<0>, dim3(cus), dim3(64), lds, nullptr, n, 30, sink.p);
    else if (what == CMDP_CALIB_LDS_CHAIN) hipLaunchKernelGGL(k_calib_lds_chain<1>, dim3(cus), dim3(64), lds, nullptr, n, 30, sink.p);
    else hipLaunchKernelGGL(k_calib_lds_chain<2>, dim3(cus), dim3(64), lds, nullptr, n, 30, sink.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e1, nullptr));
    HIP_TRY(hipEventSynchronize(e1));
  }
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *ns_per_step = (double)ms * 1e6 / (double)n_steps;
  return CMDP_OK;
}

int cmdp_visits(cmdp_t* h, int64_t* state_counts, int64_t* sa_counts) {
  if (int rc = bind(h)) return rc;
  if (!h->has_env) return fail(CMDP_ERR_INVALID, "handle was created without the sampler half");
  hipStream_t st = h->stream;
  std::vector<int32_t> tmp;
  if (state_counts) {
    tmp.resize((size_t)h->n_states);
    HIP_TRY(hipMemcpyAsync(tmp.data(), h->d_visits_s.p, sizeof(int32_t) * tmp.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < tmp.size(); ++i) state_counts[i] = tmp[i];
  }
  if (sa_counts) {
    tmp.resize((size_t)h->n_rows);
    HIP_TRY(hipMemcpyAsync(tmp.data(), h->d_visits_sa.p, sizeof(int32_t) * tmp.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = 0; i < tmp.size(); ++i) sa_counts[i] = tmp[i];
  }
  return CMDP_OK;
}

int cmdp_reset_visits(cmdp_t* h) {
  if (int rc = bind(h)) return rc;
  if (!h->has_env) return fail(CMDP_ERR_INVALID, "handle was created without the sampler half");
  HIP_TRY(h->d_visits_s.zero(h->stream));
  HIP_TRY(h->d_visits_sa.zero(h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->vis_bound = 0;
  return CMDP_OK;
}

int cmdp_set_visits(cmdp_t* h, const int64_t* state_counts, const int64_t* sa_counts) {
  if (int rc = bind(h)) return rc;   // (folds what K1E still holds: the restored values replace everything)
  if (!h->has_env) return fail(CMDP_ERR_INVALID, "handle was created without the sampler half");
  hipStream_t st = h->stream;
  int64_t top = 0;
  std::vector<int32_t> tmp;
  for (int which = 0; which < 2; ++which) {
    const int64_t* src = which ? sa_counts : state_counts;
    if (!src) continue;
    const size_t n = (size_t)(which ? h->n_rows : h->n_states);
    tmp.resize(n);
    for (size_t i = 0; i < n; ++i) {
      if (src[i] < 0 || src[i] > 0x7fffffffLL) return fail(CMDP_ERR_INVALID, "visit count %lld at index %zu does not fit the device's int32 counters", (long long)src[i], i);
      tmp[i] = (int32_t)src[i];
      top = std::max(top, src[i]);
    }
    HIP_TRY(hipMemcpyAsync(which ? h->d_visits_sa.p : h->d_visits_s.p, tmp.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  // a counter left as it was keeps its old bound
  h->vis_bound = (state_counts && sa_counts) ? top : std::max(h->vis_bound, top);
  return CMDP_OK;
}

int cmdp_last_start(cmdp_t* h, int32_t* last_start, int32_t* previous_start) {
  if (int rc = bind(h)) return rc;
  if (!h->has_env || !last_start) return fail(CMDP_ERR_INVALID, "bad argument");
  HIP_TRY(hipMemcpyAsync(last_start, h->d_last_start.p, sizeof(int32_t) * h->B, hipMemcpyDeviceToHost, h->stream));
  if (previous_start)
    HIP_TRY(hipMemcpyAsync(previous_start, h->d_prev_start.p, sizeof(int32_t) * h->B, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CMDP_OK;
}

int cmdp_state(cmdp_t* h, int32_t* cur, int32_t* hstep, uint8_t* needs_reset) {
  if (int rc = bind(h)) return rc;
  if (!h->has_env) return fail(CMDP_ERR_INVALID, "handle was created without the sampler half");
  hipStream_t st = h->stream;
  if (cur) HIP_TRY(hipMemcpyAsync(cur, h->d_cur.p, sizeof(int32_t) * h->B, hipMemcpyDeviceToHost, st));
  if (hstep) HIP_TRY(hipMemcpyAsync(hstep, h->d_h.p, sizeof(int32_t) * h->B, hipMemcpyDeviceToHost, st));
  if (needs_reset) HIP_TRY(hipMemcpyAsync(needs_reset, h->d_need_reset.p, h->B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

}  // extern "C"

// ---- dynamic programming ---------------------------------------------------------------------------------
namespace {

// AUTO rules of the reference dispatchers (infinite_horizon.py:28-36 and :60-64), per instance.
int vi_rule(int64_t S, int A, int64_t nnz) {
  const double size = (double)S * A * (double)S;
  return (size > 300.0 * 3 * 300 && (double)nnz / size < 0.2) ? CMDP_SCHEME_JACOBI : CMDP_SCHEME_GAUSS_SEIDEL;
}
int pe_rule(int64_t S, int A, int64_t nnz) {
  const double size = (double)S * A * (double)S;
  return (S > 200 && (double)nnz / size < 0.2) ? CMDP_SCHEME_JACOBI : CMDP_SCHEME_GAUSS_SEIDEL;
}

// One scheme per launch: all instances of a batch must agree under AUTO (they do when they come from
// one parameterisation); otherwise the caller picks the scheme explicitly or splits the batch.
int resolve_scheme(cmdp_t* h, int scheme, bool pe, bool diam, int* out) {
  if (scheme == CMDP_SCHEME_JACOBI || scheme == CMDP_SCHEME_GAUSS_SEIDEL) { *out = scheme; return CMDP_OK; }
  if (scheme != CMDP_SCHEME_AUTO) return fail(CMDP_ERR_INVALID, "scheme");
  int chosen = 0;
  for (int b = 0; b < h->B; ++b) {
    const int64_t S = h->state_off[b + 1] - h->state_off[b];
    int64_t nnz = h->csr_nnz[b];
    if (diam) nnz = std::max<int64_t>(nnz, 1);  // T_es differs from T only by the rows of the target
    const int s = pe ? pe_rule(S, h->A, nnz) : vi_rule(S, h->A, nnz);
    if (chosen == 0) chosen = s;
    else if (chosen != s)
      return fail(CMDP_ERR_INVALID, "CMDP_SCHEME_AUTO selects different schemes inside this batch; pass the scheme "
                                    "explicitly or split the batch");
  }
  *out = chosen;
  return CMDP_OK;
}

DpShape dp_shape(const cmdp_t* h) { return {h->A, h->max_row_nnz, h->max_state_unique, h->max_S, h->max_inst_nnz}; }

// The fields every DP kernel reads: the batch's CSR and its rewards.  The rest is zero; callers set what their kernel needs.
DpTables dp_tables(const cmdp_t* h) {
  DpTables t{};
  t.B = h->B; t.A = h->A; t.state_off = h->d_state_off.p; t.csr_ptr = h->d_csr_ptr.p; t.csr_col = h->d_csr_col.p;
  t.csr_val = h->d_csr_val.p; t.R = h->d_R.p;
  return t;
}

// Host copy of the batch's CSR for the planners that run on the host (`val` may be null); returns after the copies have landed
int fetch_csr(cmdp_t* h, std::vector<int64_t>* ptr, std::vector<int32_t>* col, std::vector<float>* val) {
  hipStream_t st = h->stream;
  ptr->resize((size_t)h->n_rows + 1);
  col->resize((size_t)h->n_csr);
  if (val) val->resize((size_t)h->n_csr);
  HIP_TRY(hipMemcpyAsync(ptr->data(), h->d_csr_ptr.p, sizeof(int64_t) * ptr->size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(col->data(), h->d_csr_col.p, sizeof(int32_t) * col->size(), hipMemcpyDeviceToHost, st));
  if (val) HIP_TRY(hipMemcpyAsync(val->data(), h->d_csr_val.p, sizeof(float) * val->size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

// Device aliases of page-locked result arrays (discounted): the register-resident kernels touch Q, V and the sweep counts
// exactly once, when an instance has converged, so they store into the caller's arrays directly (BatchedMDP.dp_buffers) --
// the results of the instances that converge early cross PCIe under the sweeps of the rest, and no copy follows the kernel
struct ZeroCopy {
  float *Q = nullptr, *V = nullptr;  // both or neither
  int64_t* sweeps = nullptr;         // null: the caller's counts are pageable (or not asked for)
  int32_t* status = nullptr;
  bool used = false;                 // run_sweeps: the kernel stored through these
};

// Launches the sweep kernel for `units` work items (instances, or (instance,target) pairs).
int run_sweeps(cmdp_t* h, int mode, bool diam, int scheme, DpTables t, int64_t units, ZeroCopy* zc = nullptr) {
  hipStream_t st = h->stream;
  if (units > 0x7fffffffLL) return fail(CMDP_ERR_INVALID, "too many work items");
  SweepChoice c{};
  if (int rc = pick_sweep(dp_shape(h), mode, diam, scheme, h->dp_kernel, &c)) return rc;
  if (zc && zc->V && c.reg()) {   // (the workgroup / wavefront kernels keep their working values in the device arrays)
    t.Q = zc->Q; t.V = zc->V; t.status = zc->status;
    if (zc->sweeps) t.sweeps = zc->sweeps;
    zc->used = true;
  }
  // every sweep kernel takes the tables alone; K2 and K3 may claim more than 64 KiB of LDS
  auto launch = [&](void (*kernel)(DpTables)) -> int {
    if (int rc = set_lds(kernel, c.lds)) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)units), dim3(c.block), c.lds, st, t);
    return CMDP_OK;
  };
#define BOTH_MODES(NAME, ...) (mode == DP_VI ? launch(NAME<DP_VI, __VA_ARGS__>) : launch(NAME<DP_PE, __VA_ARGS__>))
#define DIAM_MODES(NAME, ...)                                                                                   \
  (diam ? launch(NAME<DP_VI, true, ##__VA_ARGS__>) : mode == DP_VI ? launch(NAME<DP_VI, false, ##__VA_ARGS__>) \
                                                                   : launch(NAME<DP_PE, false, ##__VA_ARGS__>))
#define K2W_VI_PE(AT, ST) BOTH_MODES(k_dp_regw, AT, 5, 4, ST)
#define K2W_VI(AT, ST) launch(k_dp_regw<DP_VI, AT, 5, 4, ST>)
#define K2W_CASE(AT, ST, MODES) c.A == AT && c.spt == ST ? K2W_##MODES(AT, ST) :
#define K2U_CASE(AT, UT, KT, ST) c.A == AT && c.U == UT && c.K == KT && c.spt == ST ? BOTH_MODES(k_dp_regu, AT, UT, KT, ST) :
#define K2R_CASE(AT, KT, ST) c.A == AT && c.K == KT && c.spt == ST ? BOTH_MODES(k_dp_reg, AT, KT, ST) :
  int rc = CMDP_OK;   // (pick_sweep chose a compiled shape: the last alternative of a list is never taken)
  switch (c.family) {
    case SWEEP_K2W: rc = CMDP_K2W_SHAPES(K2W_CASE) CMDP_OK; break;
    case SWEEP_K2U: rc = CMDP_K2U_SHAPES(K2U_CASE) CMDP_OK; break;
    case SWEEP_K2R: rc = CMDP_K2R_SHAPES(K2R_CASE) CMDP_OK; break;
    case SWEEP_K2: rc = c.csr_lds ? DIAM_MODES(k_dp_block, true) : DIAM_MODES(k_dp_block, false); break;
    default: rc = DIAM_MODES(k_dp_wave_gs); break;
  }
#undef K2R_CASE
#undef K2U_CASE
#undef K2W_CASE
#undef K2W_VI
#undef K2W_VI_PE
#undef DIAM_MODES
#undef BOTH_MODES
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  h->last_dp_kernel = c.family;
  if (diam) h->last_diam_kernel = c.family == SWEEP_K2 ? diam_code(DIAM_K2, 0, c.csr_lds) : diam_code(DIAM_K3, 0, 0);
  return CMDP_OK;
}

// Waits for the stream and scans the status words of `units` work items: those in d_status, or `pinned` ones that the
// kernel stored into page-locked host memory (nothing left to copy)
int check_status(cmdp_t* h, int64_t units, const int32_t* pinned = nullptr) {
  std::vector<int32_t> copy(pinned ? 0 : (size_t)units);
  if (!pinned) HIP_TRY(hipMemcpyAsync(copy.data(), h->d_status.p, sizeof(int32_t) * units, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const int32_t* status = pinned ? pinned : copy.data();
  for (int64_t u = 0; u < units; ++u) {
    if (status[u] == CMDP_ERR_MAX_ITER) return fail(CMDP_ERR_MAX_ITER, "work item %lld did not converge within max_sweeps", (long long)u);
    if (status[u] == CMDP_ERR_MAX_VALUE) return fail(CMDP_ERR_MAX_VALUE, "work item %lld exceeded max_abs_value", (long long)u);
  }
  return CMDP_OK;
}

// ---- what the per-target entry points (cmdp_diameter, _range, _sparse_f64, _episodic) share ---------------------------------
// First of all; each entry point's own argument checks follow it, in the order its callers have always seen them fail
int diam_check(cmdp_t* h) {
  if (int rc = bind(h)) return rc;
  if (!h->has_dp) return fail(CMDP_ERR_INVALID, "handle was created without the DP half");
  return CMDP_OK;
}

// ... after the checks: one result and one status word per state of the batch, and the tables of a per-target solve
// (gamma 1 in the continuous setting; the episodic kernel reads none and has always been handed 0)
int diam_tables(cmdp_t* h, float gamma, double eps, int64_t max_sweeps, DpTables* out) {
  const int64_t NS = h->n_states;
  if (h->d_per_target.n < (size_t)NS) HIP_TRY(h->d_per_target.alloc(NS));
  if (h->d_status.n < (size_t)NS) HIP_TRY(h->d_status.alloc(NS));
  DpTables& t = *out = dp_tables(h);
  t.unit_off = h->d_state_off.p; t.gamma = gamma; t.eps = eps; t.max_sweeps = max_sweeps;
  t.per_target = h->d_per_target.p; t.status = h->d_status.p;
  return CMDP_OK;
}

// ... after the kernels: the status of every target, and per instance the maximum over its targets starting from `start`
// (the reference's `diameter = 0` of the continuous setting, diameter.py:99-105, and `-np.inf` of the episodic, :203)
int diam_finish(cmdp_t* h, float start, float* per_target, float* diameter) {
  const int64_t NS = h->n_states;
  std::vector<float> per((size_t)NS);
  HIP_TRY(hipMemcpyAsync(per.data(), h->d_per_target.p, sizeof(float) * NS, hipMemcpyDeviceToHost, h->stream));
  if (int rc = check_status(h, NS)) return rc;  // synchronises
  for (int b = 0; b < h->B; ++b) {
    float dmax = start;
    for (int64_t s = h->state_off[b]; s < h->state_off[b + 1]; ++s) dmax = std::max(dmax, per[(size_t)s]);
    diameter[b] = dmax;
  }
  if (per_target) std::memcpy(per_target, per.data(), sizeof(float) * NS);
  return CMDP_OK;
}

int discounted(cmdp_t* h, int mode, const float* pi, float gamma, double eps, int scheme, int64_t max_sweeps,
               double max_abs, const float* R_override, float* Q, float* V, int64_t* sweeps) {
  if (int rc = bind(h)) return rc;
  if (!h->has_dp) return fail(CMDP_ERR_INVALID, "handle was created without the DP half");
  if (!Q || !V) return fail(CMDP_ERR_INVALID, "null output");
  if (mode == DP_PE && !pi) return fail(CMDP_ERR_INVALID, "pi is required");
  if (max_sweeps < 1) return fail(CMDP_ERR_INVALID, "max_sweeps < 1");
  int sch = 0;
  if (int rc = resolve_scheme(h, scheme, mode == DP_PE, false, &sch)) return rc;
  hipStream_t st = h->stream;
  const int64_t R = h->n_rows, NS = h->n_states;
  if (R_override) HIP_TRY(h->d_Rov.upload(R_override, R, st));
  if (pi) HIP_TRY(h->d_pi.upload(pi, R, st));
  if (h->d_Q.n < (size_t)R) HIP_TRY(h->d_Q.alloc(R));
  if (h->d_V.n < (size_t)NS) HIP_TRY(h->d_V.alloc(NS));
  if (h->d_sweeps.n < (size_t)h->B) HIP_TRY(h->d_sweeps.alloc(h->B));
  if (h->d_status.n < (size_t)h->B) HIP_TRY(h->d_status.alloc(h->B));
  DpTables t = dp_tables(h);
  if (R_override) t.R = h->d_Rov.p;
  t.pi = pi ? h->d_pi.p : nullptr;
  t.gamma = gamma; t.eps = eps; t.max_abs = max_abs; t.max_sweeps = max_sweeps;
  t.Q = h->d_Q.p; t.V = h->d_V.p; t.sweeps = h->d_sweeps.p; t.status = h->d_status.p;
  if (!h->ev_dp0) {
    HIP_TRY(hipEventCreate(&h->ev_dp0));
    HIP_TRY(hipEventCreate(&h->ev_dp1));
  }
  // device-visible aliases of page-locked result arrays (null for pageable memory)
  auto alias = [](void* p) -> void* {
    hipPointerAttribute_t a{};
    if (p && hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost && a.devicePointer) return a.devicePointer;
    (void)hipGetLastError();   // pageable memory is reported as an error by some runtime versions
    return nullptr;
  };
  static const bool zc_env = !(std::getenv("CMDP_DP_ZERO_COPY") && std::atoi(std::getenv("CMDP_DP_ZERO_COPY")) == 0);
  ZeroCopy zc;
  zc.Q = zc_env ? static_cast<float*>(alias(Q)) : nullptr;
  zc.V = zc.Q ? static_cast<float*>(alias(V)) : nullptr;
  if (!zc.V) zc.Q = nullptr;
  if (zc.V) {
    if (sweeps) zc.sweeps = static_cast<int64_t*>(alias(sweeps));
    if (int rc = h->pin_status.alloc((size_t)h->B)) return rc;
    zc.status = h->pin_status.p;
  }
  HIP_TRY(hipEventRecord(h->ev_dp0, st));
  if (int rc = run_sweeps(h, mode, false, sch, t, h->B, &zc)) return rc;
  HIP_TRY(hipEventRecord(h->ev_dp1, st));
  if (!zc.used) {
    HIP_TRY(hipMemcpyAsync(Q, h->d_Q.p, sizeof(float) * R, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(V, h->d_V.p, sizeof(float) * NS, hipMemcpyDeviceToHost, st));
  }
  if (sweeps && !(zc.used && zc.sweeps)) HIP_TRY(hipMemcpyAsync(sweeps, h->d_sweeps.p, sizeof(int64_t) * h->B, hipMemcpyDeviceToHost, st));
  return check_status(h, h->B, zc.used ? zc.status : nullptr);
}

int episodic(cmdp_t* h, int mode, int H, const float* pi, const float* R_override, float* Q, float* V) {
  if (int rc = bind(h)) return rc;
  if (!h->has_dp) return fail(CMDP_ERR_INVALID, "handle was created without the DP half");
  if (!Q || !V || H < 1) return fail(CMDP_ERR_INVALID, "bad argument");
  if (mode == DP_PE && !pi) return fail(CMDP_ERR_INVALID, "pi is required");
  hipStream_t st = h->stream;
  const int64_t R = h->n_rows, NS = h->n_states;
  const size_t lds = 2 * sizeof(float) * (size_t)h->max_S;
  if (lds > (size_t)kLdsBudget) return fail(CMDP_ERR_UNSUPPORTED, "instance with %d states does not fit LDS", h->max_S);
  if (R_override) HIP_TRY(h->d_Rov.upload(R_override, R, st));
  if (pi) HIP_TRY(h->d_pi.upload(pi, (size_t)H * R, st));
  const size_t nq = (size_t)(H + 1) * R, nv = (size_t)(H + 1) * NS;
  if (h->d_Q.n < nq) HIP_TRY(h->d_Q.alloc(nq));
  if (h->d_V.n < nv) HIP_TRY(h->d_V.alloc(nv));
  DpTables t = dp_tables(h);
  if (R_override) t.R = h->d_Rov.p;
  t.pi = pi ? h->d_pi.p : nullptr;
  const dim3 grid(h->B), block(kDpBlock);
  if (mode == DP_VI) {
    if (int rc = set_lds(k_episodic<DP_VI>, lds)) return rc;
    hipLaunchKernelGGL((k_episodic<DP_VI>), grid, block, lds, st, t, H, h->d_Q.p, h->d_V.p);
  } else {
    if (int rc = set_lds(k_episodic<DP_PE>, lds)) return rc;
    hipLaunchKernelGGL((k_episodic<DP_PE>), grid, block, lds, st, t, H, h->d_Q.p, h->d_V.p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(Q, h->d_Q.p, sizeof(float) * nq, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(V, h->d_V.p, sizeof(float) * nv, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

}  // namespace

extern "C" {

int cmdp_vi_discounted(cmdp_t* h, float gamma, double epsilon, int scheme, int64_t max_sweeps, double max_abs_value,
                       const float* R_override, float* Q, float* V, int64_t* sweeps) {
  return discounted(h, DP_VI, nullptr, gamma, epsilon, scheme, max_sweeps, max_abs_value, R_override, Q, V, sweeps);
}

int cmdp_pe_discounted(cmdp_t* h, const float* pi, float gamma, double epsilon, int scheme, int64_t max_sweeps,
                       const float* R_override, float* Q, float* V, int64_t* sweeps) {
  return discounted(h, DP_PE, pi, gamma, epsilon, scheme, max_sweeps, 0.0, R_override, Q, V, sweeps);
}

int cmdp_vi_episodic(cmdp_t* h, int H, const float* R_override, float* Q, float* V) {
  return episodic(h, DP_VI, H, nullptr, R_override, Q, V);
}

int cmdp_pe_episodic(cmdp_t* h, int H, const float* pi, const float* R_override, float* Q, float* V) {
  return episodic(h, DP_PE, H, pi, R_override, Q, V);
}

// K5S reads a state's value row and its successors' rows once per sweep and target group; with the builder's state
// numbering (depth-first over the grid) a state's successors sit thousands of rows away and every one of them is a fresh
// HBM fetch (PMC: 3.1 x the algorithmic reads at C5).  relabel_states orders the states of every large instance in
// breadth-first clusters of the undirected transition graph (grow a cluster from a seed until it has `cluster` states,
// seed the next one from the frontier it left) so that the rows a chunk of states gathers were fetched by the chunks just
// before it, and build_ell_relabelled stores the fixed-width rows in that order: row n = the row of original state
// orig_of[n], entries in their original order, columns translated.  Sums and stopping rule see the same numbers in the
// same order -- results are bit-equal -- only the memory the gathers touch moves.
constexpr int kK5sCluster = 80;          // states per cluster (8 wavefronts x 10 states = what a workgroup walks at a time at C5)

static void relabel_states(int S, int A, const int64_t* ptr, const int32_t* col, int cluster, std::vector<int32_t>& order) {
  // undirected adjacency (CSR) of the instance's transition graph
  std::vector<int32_t> deg((size_t)S + 1, 0);
  auto each_edge = [&](auto&& f) {
    for (int s = 0; s < S; ++s)
      for (int64_t k = ptr[(int64_t)s * A]; k < ptr[(int64_t)(s + 1) * A]; ++k)
        if (col[k] != s) f(s, col[k]);
  };
  each_edge([&](int s, int w) { ++deg[(size_t)s + 1]; ++deg[(size_t)w + 1]; });
  std::vector<int64_t> off((size_t)S + 1, 0);
  for (int s = 0; s < S; ++s) off[(size_t)s + 1] = off[(size_t)s] + deg[(size_t)s + 1];
  std::vector<int32_t> adj((size_t)off[(size_t)S]);
  std::vector<int64_t> fill(off.begin(), off.end() - 1);
  each_edge([&](int s, int w) { adj[(size_t)fill[(size_t)s]++] = w; adj[(size_t)fill[(size_t)w]++] = s; });
  order.clear();
  order.reserve((size_t)S);
  std::vector<char> seen((size_t)S, 0), placed((size_t)S, 0);
  std::vector<int32_t> pending, queue;
  size_t pending_pos = 0;
  int next_unplaced = 0;
  while ((int)order.size() < S) {
    int seed = -1;
    while (pending_pos < pending.size()) {
      const int c = pending[pending_pos++];
      if (!placed[(size_t)c] && !seen[(size_t)c]) { seed = c; break; }
    }
    if (seed < 0) {
      while (placed[(size_t)next_unplaced]) ++next_unplaced;
      seed = next_unplaced;
    }
    queue.clear();
    queue.push_back(seed);
    seen[(size_t)seed] = 1;
    size_t head = 0;
    int cnt = 0;
    while (head < queue.size() && cnt < cluster) {
      const int v = queue[head++];
      order.push_back(v);
      placed[(size_t)v] = 1;
      ++cnt;
      for (int64_t k = off[(size_t)v]; k < off[(size_t)v + 1]; ++k) {
        const int w = adj[(size_t)k];
        if (!seen[(size_t)w]) { seen[(size_t)w] = 1; queue.push_back(w); }
      }
    }
    for (; head < queue.size(); ++head) {  // the frontier left over seeds the next clusters
      seen[(size_t)queue[head]] = 0;
      pending.push_back(queue[head]);
    }
  }
}

static int build_ell_relabelled(cmdp_t* h, int K, int cluster) {
  hipStream_t st = h->stream;
  const int A = h->A;
  const int64_t NR = h->n_rows, NS = h->n_states;
  std::vector<int64_t> ptr;
  std::vector<int32_t> col;
  std::vector<float> val;
  if (int rc = fetch_csr(h, &ptr, &col, &val)) return rc;
  const size_t rows_p = (size_t)NR + 64 / K + 1;  // tail padding, as k_build_ell
  std::vector<int32_t> ecol(rows_p * K, 0), new_of((size_t)NS);
  std::vector<float> eval_(rows_p * K, 0.0f);
  std::vector<int32_t> order;
  for (int b = 0; b < h->B; ++b) {
    const int64_t so = h->state_off[b];
    const int S = (int)(h->state_off[b + 1] - so);
    // the instance's rows start at ptr[so * A]; relabel_states wants pointers relative to the instance's first row
    if (S >= h->relabel_min_states) {   // default 8192: below, the 2 x S x 256 B value arrays of a group sit in L2 anyway
      relabel_states(S, A, ptr.data() + so * A, col.data(), cluster, order);
    } else {
      order.resize((size_t)S);
      for (int s = 0; s < S; ++s) order[(size_t)s] = s;
    }
    for (int n = 0; n < S; ++n) new_of[(size_t)(so + order[(size_t)n])] = n;
    for (int n = 0; n < S; ++n) {
      for (int a = 0; a < A; ++a) {
        const int64_t ro = (so + order[(size_t)n]) * A + a, rn = (so + n) * A + a;
        const int64_t lo = ptr[(size_t)ro], hi = ptr[(size_t)ro + 1];
        if (hi - lo > K) return fail(CMDP_ERR_INVALID, "row %lld has more than %d non-zeros", (long long)ro, K);
        const int32_t c0 = hi > lo ? new_of[(size_t)(so + col[(size_t)lo])] : 0;
        for (int k = 0; k < K; ++k) {
          const bool in = lo + k < hi;
          ecol[(size_t)rn * K + k] = in ? new_of[(size_t)(so + col[(size_t)(lo + k)])] : c0;
          eval_[(size_t)rn * K + k] = in ? val[(size_t)(lo + k)] : 0.0f;
        }
      }
    }
  }
  HIP_TRY(h->d_ell_col.upload(ecol.data(), ecol.size(), st));
  HIP_TRY(h->d_ell_val.upload(eval_.data(), eval_.size(), st));
  HIP_TRY(h->d_ell_newof.upload(new_of.data(), new_of.size(), st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

// Host side of K5T: cuts every instance into clusters of <= K5T_C states whose rows (own + distinct outside successors)
// fit a tile, and writes the per-cluster row lists and the rows' entries re-indexed to tile positions (original column
// order kept).  Breadth-first region growing over the undirected transition graph keeps the halo small on grid worlds.
static int build_tiles(cmdp_t* h, int K) {
  hipStream_t st = h->stream;
  const int A = h->A;
  std::vector<int64_t> ptr;
  std::vector<int32_t> col;
  std::vector<float> val;
  if (int rc = fetch_csr(h, &ptr, &col, &val)) return rc;
  std::vector<int32_t> c0v, nclv, cl_n, cl_R, rows, lcol;
  std::vector<float> lval;
  int64_t total_rows = 0, total_states = 0;
  for (int b = 0; b < h->B; ++b) {
    const int64_t so = h->state_off[b];
    const int S = (int)(h->state_off[b + 1] - so);
    // distinct successors of every state (directed: what a sweep gathers), and undirected neighbours for the growth
    std::vector<std::vector<int32_t>> succ((size_t)S), nbr((size_t)S);
    for (int s = 0; s < S; ++s) {
      auto& v = succ[(size_t)s];
      for (int64_t r = (so + s) * A; r < (so + s + 1) * A; ++r)
        for (int64_t k = ptr[r]; k < ptr[r + 1]; ++k) v.push_back(col[k]);
      std::sort(v.begin(), v.end());
      v.erase(std::unique(v.begin(), v.end()), v.end());
    }
    for (int s = 0; s < S; ++s)
      for (int32_t w : succ[(size_t)s])
        if (w != s) { nbr[(size_t)s].push_back(w); nbr[(size_t)w].push_back(s); }
    std::vector<char> assigned((size_t)S, 0);
    std::vector<int32_t> mark((size_t)S, -1);   // cluster id while the state is in the cluster or its halo
    std::vector<char> inside((size_t)S, 0);
    std::vector<int32_t> local((size_t)S, -1);
    c0v.push_back((int32_t)cl_n.size());
    int next_seed = 0;
    std::vector<int32_t> seeds;                 // frontier left over by finished clusters: grow next to them
    size_t seed_pos = 0;
    int n_clusters = 0;
    while (true) {
      int seed = -1;
      while (seed_pos < seeds.size()) {
        const int c = seeds[seed_pos++];
        if (!assigned[(size_t)c]) { seed = c; break; }
      }
      if (seed < 0) {
        while (next_seed < S && assigned[(size_t)next_seed]) ++next_seed;
        if (next_seed == S) break;
        seed = next_seed;
      }
      const int cid = n_clusters++;
      std::vector<int32_t> members, halo, queue;
      int n_halo = 0;
      auto try_add = [&](int v) -> bool {
        // rows the tile would hold with v inside: members + 1, halo - (v was halo) + (new outside successors of v)
        int add = 0;
        for (int32_t w : succ[(size_t)v])
          if (w != v && !(inside[(size_t)w]) && mark[(size_t)w] != cid) ++add;
        const int was_halo = (mark[(size_t)v] == cid && !inside[(size_t)v]) ? 1 : 0;
        if ((int)members.size() + 1 + n_halo - was_halo + add > kK5tRmax) return false;
        if (was_halo) --n_halo;
        inside[(size_t)v] = 1;
        mark[(size_t)v] = cid;
        members.push_back(v);
        for (int32_t w : succ[(size_t)v])
          if (w != v && !inside[(size_t)w] && mark[(size_t)w] != cid) { mark[(size_t)w] = cid; halo.push_back(w); ++n_halo; }
        return true;
      };
      // Greedy growth: of the states adjacent to the cluster, take the one with the most neighbours already inside
      // (ties: first found) -- compact blobs with a small halo that also fill the gaps between earlier clusters.
      // `local` doubles as the score of a frontier state while the cluster grows (-1: not on the frontier).
      std::vector<int32_t> frontier{seed};
      local[(size_t)seed] = 0;
      while (!frontier.empty() && (int)members.size() < K5T_C) {
        size_t best = 0;
        for (size_t i = 1; i < frontier.size(); ++i)
          if (local[(size_t)frontier[i]] > local[(size_t)frontier[best]]) best = i;
        const int v = frontier[best];
        frontier[best] = frontier.back();
        frontier.pop_back();
        if (!try_add(v)) { queue.push_back(v); continue; }   // does not fit the tile: left for a later cluster
        assigned[(size_t)v] = 1;
        queue.push_back(v);
        for (int32_t w : nbr[(size_t)v]) {
          if (assigned[(size_t)w]) continue;
          if (local[(size_t)w] < 0) { local[(size_t)w] = 0; frontier.push_back(w); }
          if (local[(size_t)w] >= 0) ++local[(size_t)w];
        }
      }
      for (int32_t w : frontier) queue.push_back(w);
      for (size_t i = 0; i < queue.size(); ++i) {   // reset the scores; unassigned leftovers seed later clusters
        local[(size_t)queue[i]] = -1;
        if (!assigned[(size_t)queue[i]]) seeds.push_back(queue[i]);
      }
      if (members.empty()) {  // a single state whose own successors exceed a tile: K5T cannot take this instance
        return fail(CMDP_ERR_UNSUPPORTED, "state %d of instance %d has more than %d distinct successors: no tile holds its row",
                    seed, b, kK5tRmax - 1);
      }
      // tile rows: members, then the halo states that are still outside (a halo state may have joined later)
      std::vector<int32_t> trow(members);
      for (int32_t w : halo)
        if (!inside[(size_t)w]) trow.push_back(w);
      for (size_t i = 0; i < trow.size(); ++i) local[(size_t)trow[i]] = (int32_t)i;
      const int R = (int)((trow.size() + 3) / 4 * 4);
      cl_n.push_back((int32_t)members.size());
      cl_R.push_back(R);
      total_rows += (int64_t)trow.size();
      total_states += (int64_t)members.size();
      for (int i = 0; i < kK5tRmax; ++i) rows.push_back(i < (int)trow.size() ? trow[(size_t)i] : trow[0]);
      for (int u = 0; u < K5T_C; ++u)
        for (int a = 0; a < A; ++a) {
          int64_t lo = 0, hi = 0;
          if (u < (int)members.size()) {
            const int64_t r = (so + members[(size_t)u]) * A + a;
            lo = ptr[r]; hi = ptr[r + 1];
          }
          for (int k = 0; k < K; ++k) {
            const bool in = lo + k < hi;
            lcol.push_back(in ? local[(size_t)col[lo + k]] : (hi > lo ? local[(size_t)col[lo]] : 0));
            lval.push_back(in ? val[lo + k] : 0.0f);
          }
        }
      for (int32_t v : members) inside[(size_t)v] = 0;
      for (size_t i = 0; i < trow.size(); ++i) local[(size_t)trow[i]] = -1;
    }
    nclv.push_back(n_clusters);
  }
  for (int i = 0; i < 64; ++i) { lcol.push_back(0); lval.push_back(0.0f); }  // a 64-entry load past the last cluster
  HIP_TRY(h->d_tl_c0.upload(c0v.data(), c0v.size(), st));
  HIP_TRY(h->d_tl_ncl.upload(nclv.data(), nclv.size(), st));
  HIP_TRY(h->d_tl_n.upload(cl_n.data(), cl_n.size(), st));
  HIP_TRY(h->d_tl_R.upload(cl_R.data(), cl_R.size(), st));
  HIP_TRY(h->d_tl_rows.upload(rows.data(), rows.size(), st));
  HIP_TRY(h->d_tl_lcol.upload(lcol.data(), lcol.size(), st));
  HIP_TRY(h->d_tl_val.upload(lval.data(), lval.size(), st));
  HIP_TRY(hipStreamSynchronize(st));
  h->tile_K = K;
  h->tile_rows_per_state = total_states ? (double)total_rows / (double)total_states : 0.0;
  if (std::getenv("CMDP_K5T_DEBUG"))
    std::fprintf(stderr, "[K5T] %zu clusters, %.1f states and %.1f tile rows per cluster (%.3f rows gathered per state)\n",
                 cl_n.size(), (double)total_states / cl_n.size(), (double)total_rows / cl_n.size(), h->tile_rows_per_state);
  return CMDP_OK;
}

// Groups of 64 consecutive targets of one instance for the lanes kernels (K5S / K5T / K5C, K5D), and their packing into launches
struct DiamGroups {
  std::vector<int32_t> inst, t0, cnt;
  std::vector<int64_t> elems;  // value-array elements of a group: 2 x S x 64
  std::vector<int64_t> voff;   // of the launch `next` returned last: every group's offset into the workspace, in elements

  // the targets [lo, hi) of the flat state space
  DiamGroups(const std::vector<int64_t>& state_off, int64_t lo, int64_t hi) {
    const int64_t GW = 64;
    for (size_t b = 0; b + 1 < state_off.size(); ++b) {
      const int64_t so = state_off[b], S = state_off[b + 1] - so;
      const int64_t a = std::max(lo, so) - so, z = std::min(hi, so + S) - so;
      for (int64_t x = a; x < z; x += GW) {
        inst.push_back((int32_t)b);
        t0.push_back((int32_t)x);
        cnt.push_back((int32_t)std::min(GW, z - x));
        elems.push_back(2 * S * GW);
      }
    }
  }

  // The launch that starts at group g0: groups while their value arrays (`elem_bytes` per element) and `group_bytes` more
  // per group fit `ws_cap` bytes, and at least one.  Returns its end g1, fills voff and the launch's elements.
  size_t next(size_t g0, size_t elem_bytes, size_t group_bytes, size_t ws_cap, size_t* launch_elems) {
    size_t g1 = g0, total = 0;
    voff.clear();
    while (g1 < inst.size() && (g1 == g0 || (total + (size_t)elems[g1]) * elem_bytes + (g1 - g0 + 1) * group_bytes <= ws_cap)) {
      voff.push_back((int64_t)total);
      total += (size_t)elems[g1];
      ++g1;
    }
    *launch_elems = total;
    return g1;
  }
};

// The CMDP_K5* switches (tuning aids), read nowhere else.  CMDP_K5C and CMDP_K5C_TIMEOUT_TICKS on every call: the tests
// switch them inside one process (one tick drives the fall-back from K5C to K5S).  The others once per process.
static DiamSwitches diam_switches() {
  auto num = [](const char* name, long long unset) { const char* e = std::getenv(name); return e ? std::atoll(e) : unset; };
  static const bool agent = [] { const char* e = std::getenv("CMDP_K5C_SCOPE"); return e && !std::strcmp(e, "agent"); }();
  static const int nw = (int)num("CMDP_K5S_NW", 0), cluster = (int)num("CMDP_K5S_CLUSTER", -1);
  // 2 s of the 100 MHz wall clock unless CMDP_K5C_TIMEOUT_TICKS says otherwise
  return {(int)num("CMDP_K5C", -1), nw, agent, num("CMDP_K5C_TIMEOUT_TICKS", 200000000LL), cluster};
}

// fixed-width rows of the K5S family (k_build_ell / build_ell_relabelled), built once per handle and width
static int ensure_ell(cmdp_t* h, int K, const DiamSwitches& sw) {
  if (h->ell_K != K) {
    const int cluster = sw.k5s_cluster >= 0 ? sw.k5s_cluster : kK5sCluster;
    if (cluster > 0 && h->max_S >= h->relabel_min_states) {
      if (int rc = build_ell_relabelled(h, K, cluster)) return rc;
      h->ell_relabelled = true;
    } else {
      const size_t rows_p = (size_t)h->n_rows + 64 / K + 1;
      HIP_TRY(h->d_ell_col.alloc(rows_p * K));
      HIP_TRY(h->d_ell_val.alloc(rows_p * K));
      hipLaunchKernelGGL(k_build_ell, dim3(grid_for((int64_t)rows_p, 256)), dim3(256), 0, h->stream, h->n_rows, K,
                         h->d_csr_ptr.p, h->d_csr_col.p, h->d_csr_val.p, h->d_ell_col.p, h->d_ell_val.p);
      HIP_TRY(hipGetLastError());
      h->ell_relabelled = false;
    }
    h->ell_K = K;
  }
  return CMDP_OK;
}

// The compiled lanes kernels by template key; all instantiations of a family share a signature.  The pickers of
// cmdp_dp_plan.h return listed keys only: the closing `return nullptr` of a table is never taken.
static auto ell_kernel(int nw, int A, int K) -> void (*)(DpTables, DiamLanesArgs, const int32_t*, const float*, const int32_t*) {
#define ELL_ROW(NW, AT, KT) if (nw == NW && A == AT && K == KT) return k_diam_lanes_ell<NW, AT, KT>;
  CMDP_FIXED_WIDTH_SHAPES(ELL_ROW, 4) CMDP_FIXED_WIDTH_SHAPES(ELL_ROW, 8) CMDP_FIXED_WIDTH_SHAPES(ELL_ROW, 16)
#undef ELL_ROW
  return nullptr;
}

static auto cluster_kernel(int CL, int A, int K, bool xcd)
    -> void (*)(DpTables, DiamLanesArgs, DiamClusterArgs, const int32_t*, const float*, const int32_t*) {
#define K5C_ROW(CLT, AT, KT) \
  if (CL == CLT && A == AT && K == KT) return xcd ? k_diam_cluster<CLT, AT, KT, true> : k_diam_cluster<CLT, AT, KT, false>;
#define K5C_SIZE(CLT) CMDP_FIXED_WIDTH_SHAPES(K5C_ROW, CLT)
  CMDP_K5C_SIZES(K5C_SIZE)
#undef K5C_SIZE
#undef K5C_ROW
  return nullptr;
}

static auto tiles_kernel(int A, int K) -> void (*)(DpTables, DiamLanesArgs, TileArgs) {
#define TILE_ROW(P, AT, KT) if (A == AT && K == KT) return k_diam_tiles<kK5tNw, AT, KT, kK5tRmax>;
  CMDP_FIXED_WIDTH_SHAPES(TILE_ROW, _)
#undef TILE_ROW
  return nullptr;
}

// Lanes driver: the targets [unit_lo, unit_hi) of the flat state space in groups of 64 consecutive targets of one
// instance.  First the cluster attempt -- K5C, every group in one persistent launch --, then, where that was not tried or
// gave up, as many groups per launch of the picked lanes kernel as the value-array workspace allows.
static int diameter_lanes(cmdp_t* h, DpTables t, int64_t unit_lo, int64_t unit_hi) {
  hipStream_t st = h->stream;
  const DpShape shape = dp_shape(h);
  const int A = h->A, K = fixed_width_K(h->max_row_nnz);
  const DiamSwitches sw = diam_switches();
  // (a give-up costs every workgroup its 2-second spin: on a GPU that other streams / ranks keep busy the persistent launch is
  // not tried again at once -- the back-off doubles with every consecutive give-up; CMDP_K5C > 0 overrides it)
  const bool backing_off = h->k5c_skip > 0 && sw.k5c <= 0;
  if (backing_off) h->k5c_skip--;
  DiamGroups gr(h->state_off, unit_lo, unit_hi);
  const size_t G = gr.inst.size();
  if (const int CL = pick_diameter_cluster(shape, h->dp_kernel, h->max_S >= h->relabel_min_states, h->cus, sw, backing_off, G > 0)) {
    if (int rc = ensure_ell(h, K, sw)) return rc;
    const int n_clusters = h->cus / CL;
    DiamClusterArgs ca{};
    ca.n_groups = (int)G; ca.n_clusters = n_clusters; ca.vstride = 2 * (int64_t)h->max_S * 64;
    const size_t vfloats = (size_t)n_clusters * (size_t)ca.vstride;
    if (h->d_dl_v.n < vfloats) {
      if (hipError_t e = h->d_dl_v.alloc(vfloats); e != hipSuccess)
        return fail(CMDP_ERR_HIP, "K5C workspace of %zu bytes: %s", vfloats * sizeof(float), hipGetErrorString(e));
    }
    HIP_TRY(h->d_k5c_red.alloc((size_t)n_clusters * 2 * CL * 2 * 64));
    HIP_TRY(h->d_k5c_bar.alloc((size_t)n_clusters + 1 + (size_t)n_clusters * CL));
    HIP_TRY(h->d_dl_inst.upload(gr.inst.data(), G, st));
    HIP_TRY(h->d_dl_t0.upload(gr.t0.data(), G, st));
    HIP_TRY(h->d_dl_cnt.upload(gr.cnt.data(), G, st));
    ca.cred = h->d_k5c_red.p; ca.cbar = h->d_k5c_bar.p; ca.err = reinterpret_cast<int*>(h->d_k5c_bar.p + n_clusters);
    ca.xcc = ca.err + 1;
    ca.timeout_ticks = sw.timeout_ticks;
    DiamLanesArgs g{h->d_dl_inst.p, h->d_dl_t0.p, h->d_dl_cnt.p, nullptr, h->d_dl_v.p};
    const int32_t* new_of = h->ell_relabelled ? h->d_ell_newof.p : nullptr;
    const unsigned grid = (unsigned)(n_clusters * CL);
    // first with the XCD-scope barriers (the members verify that they share an XCD); a cluster spread over XCDs makes the
    // launch end with err = 2 and it is repeated with agent-scope barriers; CMDP_K5C_SCOPE = agent skips the first form
    for (int pass = (sw.agent_scope || h->k5c_agent_scope) ? 1 : 0; pass < 2; ++pass) {
      HIP_TRY(h->d_k5c_bar.zero(st));   // counters, error flag, XCC ids
      hipLaunchKernelGGL(cluster_kernel(CL, A, K, pass == 0), dim3(grid), dim3(1024), 0, st, t, g, ca, h->d_ell_col.p, h->d_ell_val.p, new_of);
      HIP_TRY(hipGetLastError());
      int err = 0;
      HIP_TRY(hipMemcpyAsync(&err, ca.err, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (!err) {
        h->k5c_launches++;
        h->k5c_backoff = 0;
        h->last_diam_kernel = diam_code(DIAM_K5C, CL, pass == 0);
        return CMDP_OK;
      }
      if (err == 2 && pass == 0) { h->k5c_agent_scope = true; continue; }   // this device does not deal workgroups as assumed
      h->k5c_timeouts++;   // a cluster's workgroups were not all resident: the groups are solved again, one workgroup each
      h->k5c_backoff = std::min(1024, std::max(8, 2 * h->k5c_backoff));
      h->k5c_skip = h->k5c_backoff;
      break;
    }
  }
  // the workspace is also bounded by what the device has free right now (other handles / ranks sharing the GPU):
  // 80 % of the free bytes plus what this handle already holds for the purpose; fewer groups per launch, same results
  size_t ws_cap = h->dl_ws_bytes;
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
      ws_cap = std::min(ws_cap, h->d_dl_v.n * sizeof(float) + free_b / 5 * 4);
  }
  const int family = lanes_family(shape, h->dp_kernel);
  for (size_t g0 = 0, g1 = 0; g0 < G; g0 = g1) {
    size_t floats = 0;
    g1 = gr.next(g0, sizeof(float), 0, ws_cap, &floats);
    const size_t n = g1 - g0;
    if (h->d_dl_v.n < floats) {
      if (hipError_t e = h->d_dl_v.alloc(floats); e != hipSuccess)
        return fail(CMDP_ERR_HIP, "K5S workspace of %zu bytes: %s", floats * sizeof(float), hipGetErrorString(e));
    }
    HIP_TRY(h->d_dl_inst.upload(gr.inst.data() + g0, n, st));
    HIP_TRY(h->d_dl_t0.upload(gr.t0.data() + g0, n, st));
    HIP_TRY(h->d_dl_cnt.upload(gr.cnt.data() + g0, n, st));
    HIP_TRY(h->d_dl_voff.upload(gr.voff.data(), n, st));
    DiamLanesArgs g{h->d_dl_inst.p, h->d_dl_t0.p, h->d_dl_cnt.p, h->d_dl_voff.p, h->d_dl_v.p};
    // the tables of the family, built once per handle and width (build_tiles refuses a state whose own successors exceed a tile)
    if (family == DIAM_K5T && h->tile_K != K)
      if (int rc = build_tiles(h, K)) return rc;
    if (family == DIAM_K5S_ELL)
      if (int rc = ensure_ell(h, K, sw)) return rc;
    const LanesChoice c = pick_diameter_lanes(shape, h->dp_kernel, h->ell_relabelled, (int64_t)n, h->cus, sw);
    const dim3 grid((unsigned)n), block(c.nw * 64);
    if (c.family == DIAM_K5T) {
      TileArgs ta{h->d_tl_c0.p, h->d_tl_ncl.p, h->d_tl_n.p, h->d_tl_R.p, h->d_tl_rows.p, h->d_tl_lcol.p, h->d_tl_val.p};
      const size_t lds = sizeof(float) * 64 * (size_t)kK5tRmax * kK5tNw;
      const auto kernel = tiles_kernel(A, K);
      if (int rc = set_lds(kernel, lds)) return rc;
      hipLaunchKernelGGL(kernel, grid, block, lds, st, t, g, ta);
    } else if (c.family == DIAM_K5S_ELL) {
      const int32_t* new_of = h->ell_relabelled ? h->d_ell_newof.p : nullptr;
      hipLaunchKernelGGL(ell_kernel(c.nw, A, K), grid, block, 0, st, t, g, h->d_ell_col.p, h->d_ell_val.p, new_of);
    } else hipLaunchKernelGGL(k_diam_lanes<8>, grid, block, 0, st, t, g);
    HIP_TRY(hipGetLastError());
    h->last_diam_kernel = c.code;
    HIP_TRY(hipStreamSynchronize(st));  // the next launch overwrites gr.voff, which the upload may still be staging
  }
  return CMDP_OK;
}

int cmdp_diameter(cmdp_t* h, double epsilon, int scheme, int64_t max_sweeps, float* per_target, float* diameter) {
  if (int rc = diam_check(h)) return rc;
  if (!diameter) return fail(CMDP_ERR_INVALID, "null output");
  if (max_sweeps < 1) return fail(CMDP_ERR_INVALID, "max_sweeps < 1");
  int sch = 0;
  if (int rc = resolve_scheme(h, scheme, false, true, &sch)) return rc;
  DpTables t{};
  if (int rc = diam_tables(h, 1.0f, epsilon, max_sweeps, &t)) return rc;
  if (pick_diameter_path(dp_shape(h), sch, h->dp_kernel) == DIAM_PATH_LANES) {
    if (int rc = diameter_lanes(h, t, 0, h->n_states)) return rc;
  } else if (int rc = run_sweeps(h, DP_VI, true, sch, t, h->n_states)) return rc;
  return diam_finish(h, 0.0f, per_target, diameter);
}

int cmdp_diameter_sparse_f64(cmdp_t* h, double epsilon, int64_t max_sweeps, double* running_max, double* diameter) {
  if (int rc = diam_check(h)) return rc;
  if (!diameter) return fail(CMDP_ERR_INVALID, "null output");
  if (max_sweeps < 1) return fail(CMDP_ERR_INVALID, "max_sweeps < 1");
  if (h->H != 0) return fail(CMDP_ERR_INVALID, "the sparse float64 diameter is the continuous setting's (horizon 0)");
  hipStream_t st = h->stream;
  const int64_t NS = h->n_states;
  if (h->d_status.n < (size_t)NS) HIP_TRY(h->d_status.alloc(NS));
  DpTables t = dp_tables(h);
  t.eps = epsilon; t.max_sweeps = max_sweeps; t.status = h->d_status.p;
  constexpr int kLogCap = 2048;  // sweeps between diff < 0.05 and diff < eps that can be logged per target
  DiamGroups gr(h->state_off, 0, NS);
  const size_t G = gr.inst.size();
  size_t ws_cap = h->dl_ws_bytes;
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) ws_cap = std::min(ws_cap, free_b / 5 * 3);
  }
  std::vector<double> log_host;
  std::vector<int32_t> logn_host;
  std::vector<double> run((size_t)NS, 0.0);
  std::vector<double> D((size_t)h->B, -std::numeric_limits<double>::infinity());
  DevBuf<double> d_v, d_log;
  DevBuf<int32_t> d_logn, d_inst, d_t0, d_cnt;
  DevBuf<int64_t> d_voff;
  for (size_t g0 = 0, g1 = 0; g0 < G; g0 = g1) {
    size_t doubles = 0;
    g1 = gr.next(g0, sizeof(double), (size_t)64 * kLogCap * 16, ws_cap, &doubles);   // a group's value arrays and its log
    const size_t n = g1 - g0;
    if (d_v.n < doubles) HIP_TRY(d_v.alloc(doubles));
    if (d_log.n < n * 64 * kLogCap * 2) HIP_TRY(d_log.alloc(n * 64 * kLogCap * 2));
    if (d_logn.n < n * 64) HIP_TRY(d_logn.alloc(n * 64));
    HIP_TRY(d_inst.upload(gr.inst.data() + g0, n, st));
    HIP_TRY(d_t0.upload(gr.t0.data() + g0, n, st));
    HIP_TRY(d_cnt.upload(gr.cnt.data() + g0, n, st));
    HIP_TRY(d_voff.upload(gr.voff.data(), n, st));
    DiamF64Args g{d_inst.p, d_t0.p, d_cnt.p, d_voff.p, d_v.p, d_log.p, d_logn.p, kLogCap};
    hipLaunchKernelGGL(k_diam_lanes_f64<8>, dim3((unsigned)n), dim3(512), 0, st, t, g);
    HIP_TRY(hipGetLastError());
    log_host.resize(n * 64 * kLogCap * 2);
    logn_host.resize(n * 64);
    HIP_TRY(hipMemcpyAsync(logn_host.data(), d_logn.p, sizeof(int32_t) * n * 64, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(log_host.data(), d_log.p, sizeof(double) * log_host.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the reference's loop over the targets, in its order: the first logged sweep at which it would have stopped
    for (size_t gi = 0; gi < n; ++gi) {
      const int b = gr.inst[g0 + gi];
      for (int l = 0; l < gr.cnt[g0 + gi]; ++l) {
        const int32_t nl = logn_host[gi * 64 + l];
        if (nl < 0) return fail(CMDP_ERR_MAX_ITER, "target %d of instance %d did not converge within max_sweeps", gr.t0[g0 + gi] + l, b);
        if (nl > kLogCap)
          return fail(CMDP_ERR_UNSUPPORTED, "target %d of instance %d needs more than %d sweeps between diff < 0.05 and diff < eps",
                      gr.t0[g0 + gi] + l, b, kLogCap);
        const double* lg = log_host.data() + (gi * 64 + l) * (size_t)kLogCap * 2;
        double mx = lg[2 * (nl - 1) + 1];
        for (int32_t j = 0; j < nl; ++j) {
          const double diff = lg[2 * j], m = lg[2 * j + 1];
          if (diff < epsilon || (diff < 0.05 && m - 1 < D[(size_t)b])) { mx = m; break; }
        }
        D[(size_t)b] = std::max(D[(size_t)b], mx);
        run[(size_t)(h->state_off[b] + gr.t0[g0 + gi] + l)] = D[(size_t)b];
      }
    }
  }
  for (int b = 0; b < h->B; ++b) diameter[b] = D[(size_t)b];
  if (running_max) std::memcpy(running_max, run.data(), sizeof(double) * (size_t)NS);
  return CMDP_OK;
}

int cmdp_diameter_range(cmdp_t* h, double epsilon, int64_t max_sweeps, int64_t target_lo, int64_t target_hi,
                        float* per_target) {
  if (int rc = diam_check(h)) return rc;
  if (!per_target) return fail(CMDP_ERR_INVALID, "null output");
  if (max_sweeps < 1) return fail(CMDP_ERR_INVALID, "max_sweeps < 1");
  const int64_t NS = h->n_states;
  if (target_lo < 0 || target_hi > NS || target_lo > target_hi) return fail(CMDP_ERR_INVALID, "target range outside [0, %lld]", (long long)NS);
  if (target_lo == target_hi) return CMDP_OK;
  hipStream_t st = h->stream;
  DpTables t{};
  if (int rc = diam_tables(h, 1.0f, epsilon, max_sweeps, &t)) return rc;
  HIP_TRY(hipMemsetAsync(h->d_status.p, 0, sizeof(int32_t) * NS, st));
  if (int rc = diameter_lanes(h, t, target_lo, target_hi)) return rc;
  HIP_TRY(hipMemcpyAsync(per_target, h->d_per_target.p + target_lo, sizeof(float) * (target_hi - target_lo),
                         hipMemcpyDeviceToHost, st));
  return check_status(h, NS);
}

int cmdp_diameter_episodic(cmdp_t* h, int H, const int64_t* start_off, const int32_t* start_state,
                           const float* start_prob, double epsilon, int64_t max_sweeps, float* per_target,
                           float* diameter) {
  if (int rc = diam_check(h)) return rc;
  if (!diameter || !start_off || !start_state || !start_prob) return fail(CMDP_ERR_INVALID, "null argument");
  if (H < 2 || max_sweeps < 1) return fail(CMDP_ERR_INVALID, "H < 2 or max_sweeps < 1");
  const int B = h->B, A = h->A;
  const int64_t NS = h->n_states;
  const size_t lds = sizeof(float) * (size_t)H * h->max_S;
  if (lds > (size_t)kLdsBudget - 1024)
    return fail(CMDP_ERR_UNSUPPORTED, "H*S = %d*%d floats do not fit the LDS-resident episodic sweep", H, h->max_S);
  if (start_off[0] != 0) return fail(CMDP_ERR_INVALID, "start_off[0] != 0");
  // rows of T_epi that are filled (mdp_creation.py:118-125): layer 0 = starting states, layer h = states with
  // incoming mass in layer h-1, for h <= H-2; layer H-1 is the return to the starting states
  std::vector<int64_t> ptr;
  std::vector<int32_t> col;
  hipStream_t st = h->stream;
  if (int rc = fetch_csr(h, &ptr, &col, nullptr)) return rc;
  std::vector<uint8_t> reach((size_t)H * NS, 0);
  for (int b = 0; b < B; ++b) {
    const int64_t so = h->state_off[b], S = h->state_off[b + 1] - so;
    uint8_t* rb = reach.data() + (size_t)H * so;
    if (start_off[b + 1] <= start_off[b]) return fail(CMDP_ERR_INVALID, "instance %d has no starting state", b);
    for (int64_t i = start_off[b]; i < start_off[b + 1]; ++i) {
      if (start_state[i] < 0 || start_state[i] >= S) return fail(CMDP_ERR_INVALID, "starting state out of range");
      rb[start_state[i]] = 1;
    }
    for (int hh = 1; hh <= H - 2; ++hh)
      for (int64_t s = 0; s < S; ++s)
        if (rb[(size_t)(hh - 1) * S + s])
          for (int a = 0; a < A; ++a) {
            const int64_t r = (so + s) * A + a;
            for (int64_t k = ptr[r]; k < ptr[r + 1]; ++k) rb[(size_t)hh * S + col[k]] = 1;
          }
  }
  DevBuf<uint8_t> d_reach;
  DevBuf<int64_t> d_soff;
  DevBuf<int32_t> d_sstate;
  DevBuf<float> d_sprob;
  HIP_TRY(d_reach.upload(reach.data(), reach.size(), st));
  HIP_TRY(d_soff.upload(start_off, B + 1, st));
  HIP_TRY(d_sstate.upload(start_state, start_off[B], st));
  HIP_TRY(d_sprob.upload(start_prob, start_off[B], st));
  DpTables t{};
  if (int rc = diam_tables(h, 0.0f, epsilon, max_sweeps, &t)) return rc;
  EpiDiamArgs e{H, d_soff.p, d_sstate.p, d_sprob.p, d_reach.p};
  if (int rc = set_lds(k_diam_episodic, lds)) return rc;
  hipLaunchKernelGGL(k_diam_episodic, dim3((unsigned)NS), dim3(256), lds, st, t, e);
  HIP_TRY(hipGetLastError());
  return diam_finish(h, -INFINITY, per_target, diameter);  // synchronises before the upload buffers above die
}

// ---- device agents -----------------------------------------------------------------------------------------
}  // extern "C"

// What every device agent's create and getters do to a buffer `a->buf`, with `a`, `st` / `h` in scope
#define AGENT_ZERO(buf, n) HIP_TRY(a->buf.alloc((size_t)(n))); HIP_TRY(a->buf.zero(st))
#define AGENT_FETCH(dst, buf, n) \
  if (dst) HIP_TRY(hipMemcpyAsync(dst, a->buf.p, sizeof(*a->buf.p) * (size_t)(n), hipMemcpyDeviceToHost, h->stream))

namespace {

// ---- what every device agent is (Q-learning, UCRL2, PSRL) ------------------------------------------------------------------
struct AgentBase {
  cmdp_t* env = nullptr;     // null once the environment handle has been destroyed (agent_attach)
  DevBuf<uint32_t> d_mt;     // the actor's MT19937 stream of every instance (seed_actor)
  DevBuf<int32_t> d_mtpos;
  DevBuf<double> d_rsum;     // MDPLoop._cumulative_reward per instance
  DevBuf<int8_t> d_act;      // [n_steps][B] action trace of the last call that asked for one
  DevBuf<uint8_t> d_mask;    // training mask of the call
};

// The actor's stream of every instance, numpy RandomState(seeds[b]), on the device; returns once the seeds have been read
int seed_actor(AgentBase* a, const int32_t* seeds) {
  cmdp_t* env = a->env;
  const int B = env->B;
  HIP_TRY(a->d_mt.alloc((size_t)B * 624));
  HIP_TRY(a->d_mtpos.alloc(B));
  std::vector<uint32_t> useeds((size_t)B);
  for (int b = 0; b < B; ++b) useeds[b] = (uint32_t)seeds[b];
  DevBuf<uint32_t> d_seeds;
  HIP_TRY(d_seeds.upload(useeds.data(), B, env->stream));
  hipLaunchKernelGGL(k_mt_seed_numpy, dim3(grid_for(B, 64)), dim3(64), 0, env->stream, a->d_mt.p, a->d_mtpos.p, d_seeds.p, B);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(env->stream));
  return CMDP_OK;
}

int agent_check_actor(int actor) {
  if (actor != CMDP_ACTOR_GREEDY)
    return fail(CMDP_ERR_UNSUPPORTED, "only the greedy actor is built: epsilon-greedy and Boltzmann exploration are not");
  return CMDP_OK;
}

// The environment handle clears `env` of the agents attached to it when it is destroyed first (garbage collection picks
// the order): such an agent frees its own memory and touches nothing of the handle, and every entry point refuses it at
// bind(a->env) with "null handle"
template <typename T>
int agent_attach(std::unique_ptr<T>& a, T** out) {
  a->env->uc_backrefs.push_back(&a->env);
  *out = a.release();
  return CMDP_OK;
}

template <typename T>
int agent_destroy(T* a) {
  if (!a) return CMDP_OK;
  if (a->env) {   // null once the environment handle has been destroyed (its stream was drained then)
    (void)hipSetDevice(a->env->device);
    (void)hipStreamSynchronize(a->env->stream);
    auto& v = a->env->uc_backrefs;
    v.erase(std::remove(v.begin(), v.end(), &a->env), v.end());
  }
  delete a;
  return CMDP_OK;
}

// What a run() call of any agent refuses before anything is stepped
int agent_run_check(AgentBase* a, int64_t n_steps) {
  if (!a) return fail(CMDP_ERR_INVALID, "null agent");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  if (n_steps < 0) return fail(CMDP_ERR_INVALID, "n_steps < 0");
  bool any = false;
  if (int rc = any_needs_reset(h, &any)) return rc;
  if (any) return fail(CMDP_ERR_NEEDS_RESET, "the environment needs reset() before the agent can run");
  return visits_check(h, n_steps);
}

// ... and what it puts on the device first: room for the action trace of `NB` = n_steps x B actions when the caller wants
// one, and the training mask (*dmask stays null without one: every instance trains)
int agent_stage_run(AgentBase* a, size_t NB, bool trace, const uint8_t* train_mask, const uint8_t** dmask) {
  if (trace && a->d_act.n < NB) HIP_TRY(a->d_act.alloc(NB));
  *dmask = nullptr;
  if (train_mask) {
    HIP_TRY(a->d_mask.upload(train_mask, a->env->B, a->env->stream));
    *dmask = a->d_mask.p;
  }
  return CMDP_OK;
}

// The policy stage of an agent that solves a model for its greedy policy (UCRL2: K14; PSRL: K15; continuous PSRL: K13 on the
// dense MAP model or K17): everything policy(), policy_solve(), evaluate(), average_reward() and a logged row share.
// Allocated by the first request.  `layers` is 1 for the continuous agents and H + 1 for the episodic one.
struct PolicyStage {
  int layers = 0;
  DevBuf<float> d_Q, d_V, d_pi;         // [layers][rows], [layers][states], [layers][rows] one-hot
  DevBuf<int64_t> d_sweeps;             // [B], iterative solvers only -- as d_scheme and d_status
  DevBuf<int32_t> d_scheme, d_status, d_list;
  std::vector<int32_t> asked, todo, status;   // the request: instances the caller wants back, instances to solve; their status
  hipEvent_t ev[2] = {nullptr, nullptr};      // around the solve
  ~PolicyStage() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// ---- agents that park their instances for a solve (UCRL2: K11, PSRL: K12) -------------------------------------------------
// A walk kernel steps every instance until it has taken the call's steps or its (artificial) episode ends; the instances
// that parked are solved in one round of kernels, released, and walked again.
struct ParkAgent : AgentBase {
  int64_t nz = 0;                      // positions of the model's layout
  std::vector<int64_t> steps_total;    // [B] transitions taken since creation: bounds the model's counts
  DevBuf<int64_t> d_row_ptr, d_taken;  // layout: d_row_ptr, d_col, d_slot (build_model_layout)
  DevBuf<int32_t> d_col, d_slot, d_park, d_obs;
  DevBuf<long long> d_left;
  DevBuf<double> d_rew;
  PinnedBuf<int32_t> pin_park;         // [2 + B]: park count, overflow flag (UCRL2 only), park list
  // a read-back of the agent's own, enqueued after the park list's of every walk (UCRL2: `iteration`)
  void* walk_dst = nullptr;
  const void* walk_src = nullptr;
  size_t walk_bytes = 0;
  PolicyStage pol;

  ParkCall call() const { return ParkCall{d_left.p, d_taken.p, d_park.p, d_park.p + 2}; }
};

// What both agents ask of the environment handle (after bind); `other_setting` is the refusal of a handle of the setting
// the agent is not built for and may print the horizon
int park_check_env(cmdp_t* env, bool episodic, const char* other_setting, const char* name, const char* solver, int max_states) {
  if (!env->has_env) return fail(CMDP_ERR_INVALID, "the environment handle was created without the sampler half");
  if (episodic ? env->H <= 0 : env->H != 0) return fail(CMDP_ERR_UNSUPPORTED, other_setting, env->H);
  if (env->layout != CMDP_LAYOUT_CSR) return fail(CMDP_ERR_UNSUPPORTED, "agents run on the CSR layout");
  if (env->reward_cache) return fail(CMDP_ERR_UNSUPPORTED, "CMDP_FLAG_REWARD_CACHE handles are not supported by the %s agent: "
                                     "its walk kernel does not park for reward blocks", name);
  if (env->max_S > max_states)
    return fail(CMDP_ERR_UNSUPPORTED, "an instance has %d states: %s takes at most %d", env->max_S, solver, max_states);
  return CMDP_OK;
}

// The model's layout from the sampler's tables: per row the distinct successors in ascending order (`ptr` / `col`, K10's
// layout), every sampler entry mapped to its position (`slot`).  Uploaded into the agent; `ptr` and `col` stay with the caller.
int build_model_layout(ParkAgent* a, std::vector<int64_t>& ptr, std::vector<int32_t>& col) {
  cmdp_t* env = a->env;
  const int B = env->B, A = env->A;
  const int64_t R = env->n_rows, E = env->n_entries;
  hipStream_t st = env->stream;
  std::vector<RowDesc> rows((size_t)R);
  std::vector<int32_t> nxt((size_t)E);
  std::vector<int64_t> ebase((size_t)B);
  HIP_TRY(hipMemcpyAsync(rows.data(), env->d_row.p, sizeof(RowDesc) * R, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(nxt.data(), env->d_sp_next.p, sizeof(int32_t) * E, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(ebase.data(), env->d_entry_base.p, sizeof(int64_t) * B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ptr.assign((size_t)R + 1, 0);
  col.clear();
  std::vector<int32_t> slot((size_t)E, 0), tmp;
  for (int b = 0; b < B; ++b)
    for (int64_t r = env->state_off[b] * A; r < env->state_off[b + 1] * A; ++r) {
      const int64_t lo = ebase[b] + rows[(size_t)r].first, n = rows[(size_t)r].n;
      tmp.assign(nxt.begin() + lo, nxt.begin() + lo + n);
      std::sort(tmp.begin(), tmp.end());
      tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
      const int64_t z0 = (int64_t)col.size();
      for (int64_t e = lo; e < lo + n; ++e)
        slot[(size_t)e] = (int32_t)(z0 + (std::lower_bound(tmp.begin(), tmp.end(), nxt[(size_t)e]) - tmp.begin()));
      col.insert(col.end(), tmp.begin(), tmp.end());
      ptr[(size_t)r + 1] = (int64_t)col.size();
    }
  if ((int64_t)col.size() > 0x7fffffffLL) return fail(CMDP_ERR_UNSUPPORTED, "more than 2^31 successor positions");
  a->nz = (int64_t)col.size();
  HIP_TRY(a->d_row_ptr.upload(ptr.data(), ptr.size(), st));
  HIP_TRY(a->d_col.upload(col.data(), col.size(), st));
  HIP_TRY(a->d_slot.upload(slot.data(), slot.size(), st));
  HIP_TRY(hipStreamSynchronize(st));   // `slot` dies here
  return CMDP_OK;
}

int park_layout(ParkAgent* a, int64_t* n_positions, int64_t* row_ptr, int32_t* col) {
  if (!a) return fail(CMDP_ERR_INVALID, "null agent");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  if (n_positions) *n_positions = a->nz;
  AGENT_FETCH(row_ptr, d_row_ptr, h->n_rows + 1);
  AGENT_FETCH(col, d_col, a->nz);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CMDP_OK;
}

// What every create allocates for the calls to come: their state, the cumulative reward, the actor's stream
int park_alloc(ParkAgent* a, const int32_t* seeds) {
  const int B = a->env->B;
  hipStream_t st = a->env->stream;
  a->steps_total.assign((size_t)B, 0);
  AGENT_ZERO(d_left, B); AGENT_ZERO(d_taken, B); AGENT_ZERO(d_park, B + 2); AGENT_ZERO(d_rsum, B);
  if (int rc = a->pin_park.alloc((size_t)B + 2)) return rc;
  return seed_actor(a, seeds);
}

// Parks every instance: the list of a round that solves the whole batch (before_start_interacting, episode_end_update)
int park_all(ParkAgent* a) {
  const int B = a->env->B;
  a->pin_park.p[0] = B; a->pin_park.p[1] = 0;
  for (int b = 0; b < B; ++b) a->pin_park.p[2 + b] = b;
  HIP_TRY(hipMemcpyAsync(a->d_park.p, a->pin_park.p, sizeof(int32_t) * (B + 2), hipMemcpyHostToDevice, a->env->stream));
  return CMDP_OK;
}

// What a run() call refuses before anything is stepped.  `limit_text` prints the instance, its steps so far and n_steps.
int park_run_check(ParkAgent* a, int64_t n_steps, int64_t limit, const char* limit_text) {
  if (int rc = agent_run_check(a, n_steps)) return rc;
  for (int b = 0; b < a->env->B; ++b)
    if (a->steps_total[b] + n_steps > limit)
      return fail(CMDP_ERR_OVERFLOW, limit_text, b, (long long)a->steps_total[b], (long long)n_steps);
  return CMDP_OK;
}

// One run() call after park_run_check.  `walk(mask, actions, observations, rewards)` enqueues the agent's walk kernel on the
// device buffers of the traces the caller asked for; `after_walk()` runs right after the synchronisation that follows it,
// on what the walk left in pinned memory (not CMDP_OK: the call ends with that code); `round(count)` enqueues the solve and
// the release of the `count` instances of pin_park's list, sorted and on the device at d_park + 2.  With `round_ms` the
// call waits for the round it stops after, so that the two intervals are the device's and the host's share.
template <typename Walk, typename AfterWalk, typename Round>
int park_run(ParkAgent* a, int64_t n_steps, int stop_at_episode_end, const uint8_t* train_mask, int8_t* actions_trace,
             int32_t* obs_trace, double* reward_trace, double* cumulative_reward, int64_t* steps_taken, Walk&& walk,
             AfterWalk&& after_walk, Round&& round, double* wait_ms = nullptr, double* round_ms = nullptr) {
  using clk = std::chrono::steady_clock;
  const auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  cmdp_t* h = a->env;
  const int B = h->B;
  hipStream_t st = h->stream;
  const size_t NB = (size_t)n_steps * B;
  if (obs_trace && a->d_obs.n < NB) HIP_TRY(a->d_obs.alloc(NB));
  if (reward_trace && a->d_rew.n < NB) HIP_TRY(a->d_rew.alloc(NB));
  const uint8_t* dmask = nullptr;
  if (int rc = agent_stage_run(a, NB, actions_trace != nullptr, train_mask, &dmask)) return rc;
  std::vector<long long> left((size_t)B, (long long)n_steps);
  std::vector<int64_t> taken((size_t)B, n_steps);
  HIP_TRY(hipMemcpyAsync(a->d_left.p, left.data(), sizeof(long long) * B, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(a->d_taken.p, taken.data(), sizeof(int64_t) * B, hipMemcpyHostToDevice, st));
  int rc = CMDP_OK;
  while (n_steps > 0) {
    HIP_TRY(hipMemsetAsync(a->d_park.p, 0, sizeof(int32_t) * 2, st));
    walk(dmask, actions_trace ? a->d_act.p : nullptr, obs_trace ? a->d_obs.p : nullptr, reward_trace ? a->d_rew.p : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(a->pin_park.p, a->d_park.p, sizeof(int32_t) * (B + 2), hipMemcpyDeviceToHost, st));
    if (a->walk_bytes) HIP_TRY(hipMemcpyAsync(a->walk_dst, a->walk_src, a->walk_bytes, hipMemcpyDeviceToHost, st));
    const auto w0 = clk::now();
    HIP_TRY(hipStreamSynchronize(st));   // the device's share: the previous round's kernels and this walk
    if (wait_ms) *wait_ms += ms_since(w0);
    if ((rc = after_walk())) break;
    const int count = a->pin_park.p[0];
    if (count == 0) break;
    const auto t0 = clk::now();
    std::sort(a->pin_park.p + 2, a->pin_park.p + 2 + count);   // the order instances parked in is not deterministic
    HIP_TRY(hipMemcpyAsync(a->d_park.p + 2, a->pin_park.p + 2, sizeof(int32_t) * count, hipMemcpyHostToDevice, st));
    if ((rc = round(count))) break;
    if (stop_at_episode_end && round_ms) HIP_TRY(hipStreamSynchronize(st));
    if (round_ms) *round_ms += ms_since(t0);
    if (stop_at_episode_end) break;   // every instance either finished its steps or has just been stopped
  }
  if (rc == CMDP_OK && n_steps > 0) {
    HIP_TRY(hipMemcpyAsync(taken.data(), a->d_taken.p, sizeof(int64_t) * B, hipMemcpyDeviceToHost, st));
    if (actions_trace) HIP_TRY(hipMemcpyAsync(actions_trace, a->d_act.p, NB, hipMemcpyDeviceToHost, st));
    if (obs_trace) HIP_TRY(hipMemcpyAsync(obs_trace, a->d_obs.p, sizeof(int32_t) * NB, hipMemcpyDeviceToHost, st));
    if (reward_trace) HIP_TRY(hipMemcpyAsync(reward_trace, a->d_rew.p, sizeof(double) * NB, hipMemcpyDeviceToHost, st));
  }
  if (cumulative_reward) HIP_TRY(hipMemcpyAsync(cumulative_reward, a->d_rsum.p, sizeof(double) * B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) {
    a->steps_total[b] += rc == CMDP_OK ? taken[b] : n_steps;
    if (steps_taken) steps_taken[b] = taken[b];
  }
  return visits_commit(h, n_steps, rc);
}

// A request to the policy stage begins here: the stage's buffers (first request), then `asked` = the instances of the host
// mask (null: all) and `todo` = `asked`, which the agent may narrow before policy_stage (UCRL2 drops unchanged models).
int policy_select(ParkAgent* a, int layers, bool iterative, const uint8_t* mask) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const int B = h->B;
  PolicyStage& p = a->pol;
  if (!p.layers) {
    const size_t nq = (size_t)layers * h->n_rows;
    AGENT_ZERO(pol.d_Q, nq); AGENT_ZERO(pol.d_V, (size_t)layers * h->n_states); AGENT_ZERO(pol.d_pi, nq);
    if (iterative) { AGENT_ZERO(pol.d_sweeps, B); AGENT_ZERO(pol.d_scheme, B); AGENT_ZERO(pol.d_status, B); }
    HIP_TRY(p.d_list.alloc((size_t)B));
    for (hipEvent_t& e : p.ev) HIP_TRY(hipEventCreate(&e));
    p.layers = layers;
  }
  p.asked.clear();
  for (int b = 0; b < B; ++b)
    if (!mask || mask[b]) p.asked.push_back(b);
  p.todo = p.asked;
  return CMDP_OK;
}

// Enqueues the request: `solve(list, count)` launches the agent's solver for the `count` instances of `todo` (list: on the
// device, null when that is the whole batch) into d_Q / d_V / d_sweeps / d_scheme / d_status; then the greedy policy of the
// first `pi_layers` layers of Q into d_pi (0: no policy wanted), for every instance -- an instance outside `todo` gets the
// policy of the Q it was last solved to -- and the status's read-back.  With nothing to solve the stage holds what it held.
// `todo` is read by the upload: it stays as it is until policy_finish.
template <typename Solve>
int policy_stage(ParkAgent* a, int pi_layers, Solve&& solve) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const int B = h->B;
  PolicyStage& p = a->pol;
  const int count = (int)p.todo.size();
  if (count == 0) return CMDP_OK;
  const int32_t* list = nullptr;
  if (count < B) {
    HIP_TRY(p.d_list.upload(p.todo.data(), (size_t)count, st));
    list = p.d_list.p;
  }
  HIP_TRY(hipEventRecord(p.ev[0], st));
  if (int rc = solve(list, count)) return rc;
  HIP_TRY(hipEventRecord(p.ev[1], st));
  if (pi_layers > 0) {
    hipLaunchKernelGGL(k_greedy_policy_episodic<float>, dim3(B), dim3(64), 0, st, B, h->A, pi_layers, p.layers, h->d_state_off.p,
                       p.d_Q.p, p.d_pi.p);
    HIP_TRY(hipGetLastError());
  }
  p.status.assign((size_t)B, 0);
  if (p.d_status.p) HIP_TRY(hipMemcpyAsync(p.status.data(), p.d_status.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
  return CMDP_OK;
}

// Waits for the stream -- the request and whatever the caller enqueued behind it -- leaves the solve's time in *ms and fails
// on the first instance of `todo` that hit its sweep limit (iterative solvers; `model` and `max_sweeps` are for that text)
int policy_finish(ParkAgent* a, double* ms, const char* model, long long max_sweeps) {
  PolicyStage& p = a->pol;
  HIP_TRY(hipStreamSynchronize(a->env->stream));
  if (p.todo.empty()) return CMDP_OK;
  float t = 0.0f;
  HIP_TRY(hipEventElapsedTime(&t, p.ev[0], p.ev[1]));
  *ms = (double)t;
  for (int32_t b : p.todo)
    if (p.status[(size_t)b] != 0)
      return fail(CMDP_ERR_MAX_ITER, "discounted value iteration on the %s model of instance %d did not converge in %lld sweeps",
                  model, (int)b, max_sweeps);
  return CMDP_OK;
}

// The segments of the instances in `asked` of a per-instance device array into the caller's (null: nothing).  `per_state`
// elements per state of the instance, 0: one element per instance.  Outside `asked` the caller's memory is zeroed
// (`zero_outside`) or left as it is.  Enqueued: the caller waits for the stream.
template <typename T>
int policy_fetch(ParkAgent* a, T* dst, const T* src, int64_t per_state, bool zero_outside) {
  if (!dst) return CMDP_OK;
  cmdp_t* h = a->env;
  const std::vector<int32_t>& asked = a->pol.asked;
  auto first = [&](int b) { return per_state ? per_state * h->state_off[b] : (int64_t)b; };
  const bool all = (int)asked.size() == h->B;
  if (!all && zero_outside) std::memset(dst, 0, sizeof(T) * (size_t)first(h->B));
  for (size_t i = 0; i < asked.size();) {   // one copy per run of neighbours
    size_t j = i;
    while (j + 1 < asked.size() && asked[j + 1] == asked[j] + 1) ++j;
    const int64_t lo = first(asked[i]), hi = first(asked[j] + 1);
    HIP_TRY(hipMemcpyAsync(dst + lo, src + lo, sizeof(T) * (size_t)(hi - lo), hipMemcpyDeviceToHost, h->stream));
    i = j + 1;
  }
  return CMDP_OK;
}

}  // namespace

struct cmdp_agent : AgentBase {
  bool continuous = false;
  QlArgs args{};
  QlcArgs cargs{};
  DevBuf<double> d_Hh, d_gamma, d_Qc, d_Qmainc, d_Vc;  // continuous agent: float64 tables
  DevBuf<double> d_ilog, d_s7;
  DevBuf<int64_t> d_qoff, d_voff;
  DevBuf<int32_t> d_N;
  DevBuf<float> d_Q, d_V, d_mu, d_sigma, d_beta;
  DevBuf<float> d_pi;      // greedy policy [H][S][A]
  DevBuf<float> d_v0;      // packed V[0, :] of the evaluated greedy policies
  int64_t n_q = 0, n_v = 0;
};

// What the two creates ask of their arguments before the hyper-parameters, and the new agent
static int ql_create_begin(cmdp_agent_t** out, cmdp_t* env, const int32_t* seeds, bool continuous, std::unique_ptr<cmdp_agent>* guard) {
  if (!out || !env || !seeds) return fail(CMDP_ERR_INVALID, "null argument");
  *out = nullptr;
  if (int rc = bind(env)) return rc;
  if (!env->has_env || (continuous ? env->H != 0 : env->H < 1))
    return fail(CMDP_ERR_INVALID, continuous ? "the continuous Q-learning agent needs a continuous environment handle"
                                             : "the episodic Q-learning agent needs an episodic environment handle");
  if (env->layout != CMDP_LAYOUT_CSR) return fail(CMDP_ERR_UNSUPPORTED, "agents run on the CSR layout");
  guard->reset(new cmdp_agent);
  (*guard)->env = env;
  (*guard)->continuous = continuous;
  return CMDP_OK;
}

// ... and what both end with: the reward sums, the actor's stream (synchronises: the creates' staging vectors die after
// it), the back-reference
static int ql_create_end(std::unique_ptr<cmdp_agent>& guard, const int32_t* seeds, cmdp_agent_t** out) {
  cmdp_agent* a = guard.get();
  hipStream_t st = a->env->stream;
  AGENT_ZERO(d_rsum, a->env->B);
  if (int rc = seed_actor(a, seeds)) return rc;
  a->args.mt = a->cargs.mt = a->d_mt.p;
  a->args.mt_pos = a->cargs.mt_pos = a->d_mtpos.p;
  return agent_attach(guard, out);
}

// the greedy policy of the agent's Q tables into a->d_pi, [H][S][A] (continuous: H = 1), on the handle's stream
static int ql_enqueue_greedy(cmdp_agent_t* a) {
  cmdp_t* h = a->env;
  if (a->d_pi.n < (size_t)a->n_q) HIP_TRY(a->d_pi.alloc(a->n_q));
  if (a->continuous)
    hipLaunchKernelGGL(k_greedy_policy_episodic<double>, dim3(h->B), dim3(64), 0, h->stream, h->B, h->A, 1, 1,
                       h->d_state_off.p, a->d_Qc.p, a->d_pi.p);
  else
    hipLaunchKernelGGL(k_greedy_policy_episodic<float>, dim3(h->B), dim3(64), 0, h->stream, h->B, h->A, h->H, h->H,
                       h->d_state_off.p, a->d_Q.p, a->d_pi.p);
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

extern "C" {

int cmdp_qlearning_create(cmdp_agent_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon, double p,
                          double c_1, double c_2, double min_at, int ucb_type) {
  std::unique_ptr<cmdp_agent> guard;
  if (int rc = ql_create_begin(out, env, seeds, false, &guard)) return rc;
  if (!(p > 0 && p < 1) || !(c_1 > 0) || !(min_at >= 0 && min_at < 0.99) || (ucb_type != 0 && ucb_type != 1) ||
      (ucb_type == 1 && !(c_2 > 0)) || optimization_horizon < 1)
    return fail(CMDP_ERR_INVALID, "hyper-parameters out of range (0<p<1, c_1>0, 0<=min_at<0.99, bernstein needs c_2>0)");
  const int B = env->B, A = env->A, H = env->H;
  cmdp_agent_t* a = guard.get();
  hipStream_t st = env->stream;
  std::vector<double> ilog((size_t)B), s7((size_t)B);
  std::vector<int64_t> qoff((size_t)B), voff((size_t)B);
  for (int b = 0; b < B; ++b) {
    const int64_t S = env->state_off[b + 1] - env->state_off[b];
    // self.i = np.log(n_states * n_actions * optimization_horizon / p): integer product, one division, one log
    ilog[b] = std::log((double)(S * A * optimization_horizon) / p);
    s7[b] = std::sqrt(std::pow((double)H, 7) * (double)S * (double)A);
    qoff[b] = (int64_t)H * env->state_off[b] * A;
    voff[b] = (int64_t)(H + 1) * env->state_off[b];
  }
  a->n_q = (int64_t)H * env->n_states * A;
  a->n_v = (int64_t)(H + 1) * env->n_states;
  HIP_TRY(a->d_ilog.upload(ilog.data(), B, st));
  HIP_TRY(a->d_s7.upload(s7.data(), B, st));
  HIP_TRY(a->d_qoff.upload(qoff.data(), B, st));
  HIP_TRY(a->d_voff.upload(voff.data(), B, st));
  HIP_TRY(a->d_N.alloc(a->n_q));
  HIP_TRY(a->d_Q.alloc(a->n_q));
  AGENT_ZERO(d_V, a->n_v); AGENT_ZERO(d_mu, a->n_q); AGENT_ZERO(d_sigma, a->n_q); AGENT_ZERO(d_beta, a->n_q);
  hipLaunchKernelGGL(k_fill_i32, dim3(grid_for(a->n_q, 256)), dim3(256), 0, st, a->d_N.p, 1, a->n_q);
  hipLaunchKernelGGL(k_fill_f32, dim3(grid_for(a->n_q, 256)), dim3(256), 0, st, a->d_Q.p, (float)H, a->n_q);
  QlArgs& q = a->args;
  q.H = H; q.ucb = ucb_type; q.c1 = c_1; q.c2 = c_2; q.min_at = min_at; q.H3 = (double)H * H * H;
  q.i_log = a->d_ilog.p; q.sqrtH7SA = a->d_s7.p; q.q_off = a->d_qoff.p; q.v_off = a->d_voff.p;
  q.N = a->d_N.p; q.Q = a->d_Q.p; q.V = a->d_V.p; q.mu = a->d_mu.p; q.sigma = a->d_sigma.p; q.beta = a->d_beta.p;
  return ql_create_end(guard, seeds, out);
}

int cmdp_qlearning_continuous_create(cmdp_agent_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon,
                                     double min_at, double confidence, double span_approx_weight, double h_weight) {
  std::unique_ptr<cmdp_agent> guard;
  if (int rc = ql_create_begin(out, env, seeds, true, &guard)) return rc;
  if (!(min_at >= 0 && min_at < 0.99) || !(confidence > 0 && confidence < 1) || !(span_approx_weight > 0) || !(h_weight > 0) ||
      optimization_horizon < 1)
    return fail(CMDP_ERR_INVALID, "hyper-parameters out of range");
  const int B = env->B, A = env->A;
  cmdp_agent_t* a = guard.get();
  hipStream_t st = env->stream;
  const double T = (double)optimization_horizon;
  std::vector<double> Hh((size_t)B), gm((size_t)B);
  std::vector<int64_t> qoff((size_t)B);
  for (int b = 0; b < B; ++b) {
    const double S = (double)(env->state_off[b + 1] - env->state_off[b]);
    // get_H (q_learning.py:19-44): min(sqrt(span * T / S / A), (T / S / A / log(4 T / confidence)) ** 0.333)
    const double h1 = std::sqrt(span_approx_weight * T / S / A);
    const double h2 = std::pow(T / S / A / std::log(4 * T / confidence), 0.333);
    Hh[b] = h_weight * std::min(h1, h2);
    gm[b] = 1 - 1 / Hh[b];
    qoff[b] = env->state_off[b] * A;
  }
  a->n_q = env->n_rows;
  a->n_v = env->n_states;
  HIP_TRY(a->d_Hh.upload(Hh.data(), B, st));
  HIP_TRY(a->d_gamma.upload(gm.data(), B, st));
  HIP_TRY(a->d_qoff.upload(qoff.data(), B, st));
  AGENT_ZERO(d_N, a->n_q);
  HIP_TRY(a->d_Qc.alloc(a->n_q));
  HIP_TRY(a->d_Qmainc.alloc(a->n_q));
  HIP_TRY(a->d_Vc.alloc(a->n_v));
  // Q, Q_main, V start at H: `np.zeros(float32) + np.float64` is float64 under NEP 50
  std::vector<double> q0((size_t)a->n_q), v0((size_t)a->n_v);
  for (int b = 0; b < B; ++b) {
    for (int64_t r = env->state_off[b] * A; r < env->state_off[b + 1] * A; ++r) q0[(size_t)r] = Hh[b];
    for (int64_t s2 = env->state_off[b]; s2 < env->state_off[b + 1]; ++s2) v0[(size_t)s2] = Hh[b];
  }
  HIP_TRY(hipMemcpyAsync(a->d_Qc.p, q0.data(), sizeof(double) * a->n_q, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(a->d_Qmainc.p, q0.data(), sizeof(double) * a->n_q, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(a->d_Vc.p, v0.data(), sizeof(double) * a->n_v, hipMemcpyHostToDevice, st));
  QlcArgs& q = a->cargs;
  q.min_at = min_at > 0.009 ? min_at : 0.0;
  q.four_span = 4 * span_approx_weight;
  q.log_term = std::log(2 * T / confidence);
  q.Hh = a->d_Hh.p; q.gamma = a->d_gamma.p; q.q_off = a->d_qoff.p;
  q.N = a->d_N.p; q.Q = a->d_Qc.p; q.Qmain = a->d_Qmainc.p; q.V = a->d_Vc.p;
  return ql_create_end(guard, seeds, out);
}

int cmdp_qlearning_policy(cmdp_agent_t* a, float* pi) {
  if (!a || !pi) return fail(CMDP_ERR_INVALID, "null argument");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  if (!a->continuous) return fail(CMDP_ERR_INVALID, "cmdp_qlearning_policy is for the continuous agent; use cmdp_qlearning_evaluate");
  hipStream_t st = h->stream;
  if (int rc = ql_enqueue_greedy(a)) return rc;
  HIP_TRY(hipMemcpyAsync(pi, a->d_pi.p, sizeof(float) * a->n_q, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

static_assert(kChainMaxCand == K9F_MAXC && kChainRoundWidth == 16 && kChainLdsBudget == kLdsBudget,
              "cmdp_chain_plan.h plans for another kernel than cmdp_chain.h compiles and chain_launch launches");

// CMDP_CHAIN_FAST = 0 keeps K9 alone; CMDP_CHAIN_DEBUG prints K9's phase times.  Read nowhere else, once per process.
struct ChainSwitches { bool fast, debug; };
static ChainSwitches chain_switches() {
  static const ChainSwitches sw = {std::getenv("CMDP_CHAIN_FAST") ? std::atoi(std::getenv("CMDP_CHAIN_FAST")) != 0 : true,
                                   std::getenv("CMDP_CHAIN_DEBUG") != nullptr};
  return sw;
}

// K9F's plan (plan_chains of cmdp_chain_plan.h) on the device, built once per handle
static int ensure_chain_plan(cmdp_t* h) {
  auto& cf = h->cf;
  if (cf.built) return CMDP_OK;
  cf.built = true;
  hipStream_t st = h->stream;
  std::vector<int64_t> ptr;
  std::vector<int32_t> col;
  std::vector<float> val;
  if (int rc = fetch_csr(h, &ptr, &col, &val)) return rc;
  const ChainPlan p = plan_chains(h->B, h->A, h->state_off.data(), ptr.data(), col.data(), val.data());
  cf.any = p.any;
  if (!p.any) return CMDP_OK;
  HIP_TRY(cf.rank.upload(p.rank.data(), p.rank.size(), st));
  HIP_TRY(cf.cptr.upload(p.cptr.data(), p.cptr.size(), st));
  HIP_TRY(cf.nrounds.upload(p.nrounds.data(), p.nrounds.size(), st));
  HIP_TRY(cf.rptr.upload(p.rptr.data(), p.rptr.size(), st));
  HIP_TRY(cf.piv.upload(p.piv.data(), p.piv.size(), st));
  HIP_TRY(cf.cbase.upload(p.cbase.data(), p.cbase.size(), st));
  HIP_TRY(cf.rbase.upload(p.rbase.data(), p.rbase.size(), st));
  HIP_TRY(cf.cand.upload(p.cand.data(), p.cand.size(), st));
  HIP_TRY(cf.slow.alloc(h->B));
  HIP_TRY(hipStreamSynchronize(st));   // `p` is a local
  return CMDP_OK;
}

// K9's workspace, allocated by the first average-reward call: an S x S work matrix and index matrix per instance, the results
static int ensure_chain_workspace(cmdp_t* h, hipStream_t st) {
  const int B = h->B;
  if (h->d_ch_off.n >= (size_t)B + 1) return CMDP_OK;
  std::vector<int64_t> off(B + 1, 0);
  for (int b = 0; b < B; ++b) {
    const int64_t S = h->state_off[b + 1] - h->state_off[b];
    off[b + 1] = off[b] + S * S;
  }
  HIP_TRY(h->d_ch_off.upload(off.data(), off.size(), st));
  HIP_TRY(hipStreamSynchronize(st));  // `off` is a local
  HIP_TRY(h->d_ch_work.alloc((size_t)off[B]));
  HIP_TRY(h->d_ch_idx.alloc((size_t)off[B]));
  HIP_TRY(h->d_ch_avg.alloc(B));
  HIP_TRY(h->d_ch_kind.alloc(B));
  HIP_TRY(h->d_ch_ncls.alloc(B));
  return CMDP_OK;
}

// CMDP_CHAIN_DEBUG: K9's phase times from the clock words the kernel left in `d_dbg`
static int report_chain_phases(int B, const long long* d_dbg, hipStream_t st) {
  std::vector<long long> t((size_t)B * 8);
  HIP_TRY(hipMemcpyAsync(t.data(), d_dbg, sizeof(long long) * t.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  double ph[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < 7; ++k) ph[k] = std::max(ph[k], (double)(t[(size_t)b * 8 + k + 1] - t[(size_t)b * 8 + k]) / 100.0);
  std::fprintf(stderr, "[K9 us, max over instances] A %.0f  B(tarjan) %.0f  C %.0f  D %.0f  E(gth) %.0f  F(backsub) %.0f  sum %.0f\n",
               ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[6]);
  return CMDP_OK;
}

// K9 launch shared by cmdp_average_reward / cmdp_qlearning_average_reward: policy either as device one-hot rows
// (`d_pi`) or device actions (`d_act`); start states on the device.
// `mask_on_device`: `mask` is already a device pointer (the logged loop keeps its need-mask there)
// `copy_back` false: `avg` / `kind` (when given) are DEVICE-ACCESSIBLE buffers (page-locked host memory in the logged loop) the
// kernels write directly -- no copy kernel per row; nothing is synchronised.
static int chain_launch(cmdp_t* h, const float* d_pi, const int32_t* d_act, const int32_t* d_start, const uint8_t* mask,
                        double* avg, int32_t* kind, int32_t* n_classes, bool mask_on_device = false, bool copy_back = true,
                        hipStream_t on_stream = nullptr) {
  if (!h->has_dp) return fail(CMDP_ERR_INVALID, "the handle was created without the DP half (CSR transition matrices)");
  if (h->H != 0) return fail(CMDP_ERR_INVALID, "average rewards are defined for continuous instances (horizon 0)");
  const ChainSwitches sw = chain_switches();
  // the LDS formulas of cmdp_chain.h (16 wavefronts: the k_chain_fast<16> launched below)
  const size_t k9_lds = chain_lds_bytes(h->max_S, h->max_row_nnz), fast_lds = chain_fast_lds_bytes(h->max_S, h->max_row_nnz, 16);
  // the plan is built by the first call that K9F is not switched off for, whether K9F then fits LDS or not; a call that
  // pick_chain refuses builds none
  if (!h->chain_exact && sw.fast && k9_lds <= (size_t)kLdsBudget)
    if (int rc = ensure_chain_plan(h)) return rc;
  const ChainChoice k = pick_chain(h->max_S, h->max_row_nnz, k9_lds, fast_lds, h->chain_exact, sw.fast, h->cf.any);
  if (k.refusal) return k.refusal;
  hipStream_t st = on_stream ? on_stream : h->stream;   // the logged loop runs the solve beside the agents' next interval
  const int B = h->B;
  if (int rc = ensure_chain_workspace(h, st)) return rc;
  const uint8_t* dmask = nullptr;
  if (mask && mask_on_device) {
    dmask = mask;
  } else if (mask) {
    HIP_TRY(h->d_ch_mask.upload(mask, B, st));
    dmask = h->d_ch_mask.p;
  }
  ChainArgs c{};
  c.B = B; c.A = h->A; c.max_deg = h->max_row_nnz;
  c.state_off = h->d_state_off.p; c.csr_ptr = h->d_csr_ptr.p; c.csr_col = h->d_csr_col.p; c.csr_val = h->d_csr_val.p;
  c.R = h->d_R.p; c.pi = d_pi; c.act = d_act; c.start = d_start; c.mask = dmask;
  c.work_off = h->d_ch_off.p; c.work = h->d_ch_work.p; c.work_idx = h->d_ch_idx.p;
  c.avg = (!copy_back && avg) ? avg : h->d_ch_avg.p;
  c.kind = (!copy_back && kind) ? kind : h->d_ch_kind.p;
  c.n_classes = h->d_ch_ncls.p;
  if (k.k9_lds > 64 * 1024) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_chain_average_reward<16, false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.k9_lds));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_chain_average_reward<16, true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.k9_lds));
  }
  DevBuf<long long> d_dbg;
  if (sw.debug) {
    HIP_TRY(d_dbg.alloc((size_t)B * 8));
    HIP_TRY(d_dbg.zero(st));
    c.dbg = d_dbg.p;
  }
  // K9F first; it flags the instances it leaves to K9, which then runs under that mask
  h->cf.ran = false;
  if (k.fast) {
    if (int rc = set_lds(k_chain_fast<16>, k.fast_lds)) return rc;
    hipLaunchKernelGGL((k_chain_fast<16>), dim3(B), dim3(1024), k.fast_lds, st, c, h->cf.args());
    c.mask = h->cf.slow.p;
    h->cf.ran = true;
  }
  if (h->chain_exact) hipLaunchKernelGGL((k_chain_average_reward<16, true>), dim3(B), dim3(1024), k.k9_lds, st, c);
  else hipLaunchKernelGGL((k_chain_average_reward<16, false>), dim3(B), dim3(1024), k.k9_lds, st, c);
  if (sw.debug)
    if (int rc = report_chain_phases(B, d_dbg.p, st)) return rc;
  HIP_TRY(hipGetLastError());
  if (!copy_back) return CMDP_OK;  // the caller reads d_ch_avg / d_ch_kind itself
  HIP_TRY(hipMemcpyAsync(avg, h->d_ch_avg.p, sizeof(double) * B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(kind, h->d_ch_kind.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
  if (n_classes) HIP_TRY(hipMemcpyAsync(n_classes, h->d_ch_ncls.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

int cmdp_average_reward(cmdp_t* h, const int32_t* actions, const int32_t* start_states, const uint8_t* mask, double* avg,
                        int32_t* kind, int32_t* n_classes) {
  if (int rc = bind(h)) return rc;
  if (!actions || !start_states || !avg || !kind) return fail(CMDP_ERR_INVALID, "null argument");
  for (int b = 0; b < h->B; ++b) {
    const int64_t S = h->state_off[b + 1] - h->state_off[b];
    if (start_states[b] < 0 || start_states[b] >= S) return fail(CMDP_ERR_INVALID, "start state of instance %d out of range", b);
    if (mask && !mask[b]) continue;
    for (int64_t s = h->state_off[b]; s < h->state_off[b + 1]; ++s)
      if (actions[s] < 0 || actions[s] >= h->A) return fail(CMDP_ERR_INVALID, "action of state %lld out of range", (long long)s);
  }
  hipStream_t st = h->stream;
  HIP_TRY(h->d_ch_act.upload(actions, (size_t)h->n_states, st));
  HIP_TRY(h->d_ch_start.upload(start_states, (size_t)h->B, st));
  return chain_launch(h, nullptr, h->d_ch_act.p, h->d_ch_start.p, mask, avg, kind, n_classes);
}

int cmdp_qlearning_average_reward(cmdp_agent_t* a, const uint8_t* mask, double* avg, int32_t* kind) {
  if (!a || !avg || !kind) return fail(CMDP_ERR_INVALID, "null argument");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  if (!a->continuous) return fail(CMDP_ERR_INVALID, "cmdp_qlearning_average_reward is for the continuous agent");
  if (int rc = ql_enqueue_greedy(a)) return rc;
  return chain_launch(h, a->d_pi.p, nullptr, h->d_cur.p, mask, avg, kind, nullptr);
}

// cmdp_chain_plan_desc / cmdp_chain_choice: the planner and the picker of cmdp_chain_plan.h without a handle or a device
int cmdp_chain_plan_desc(const cmdp_desc* d, int32_t* rank, int32_t* cptr, int64_t* cbase, uint16_t* cand, int64_t cand_capacity,
                         int64_t* n_cand, int32_t* nrounds, int64_t* rbase, int32_t* rptr, int32_t* piv) {
  if (!d || !rank || !cptr || !cbase || !cand || !n_cand || !nrounds || !rbase || !rptr || !piv || cand_capacity < 0)
    return fail(CMDP_ERR_INVALID, "bad argument");
  if (d->n_instances < 1 || d->n_actions < 1 || !d->state_off || !d->csr_ptr || !d->csr_col || !d->csr_val)
    return fail(CMDP_ERR_INVALID, "cmdp_chain_plan_desc needs the DP half of the description");
  // as much of cmdp_create's validation as the planner indexes by
  const int B = d->n_instances, A = d->n_actions;
  if (d->state_off[0] != 0 || d->csr_ptr[0] != 0) return fail(CMDP_ERR_INVALID, "offsets do not start at 0");
  for (int b = 0; b < B; ++b) {
    const int64_t S = d->state_off[b + 1] - d->state_off[b];
    if (S < 1 || S > (1 << 28)) return fail(CMDP_ERR_INVALID, "instance %d has %lld states", b, (long long)S);
    for (int64_t r = d->state_off[b] * A; r < d->state_off[b + 1] * A; ++r) {
      if (d->csr_ptr[r + 1] < d->csr_ptr[r]) return fail(CMDP_ERR_INVALID, "csr_ptr decreasing at row %lld", (long long)r);
      for (int64_t k = d->csr_ptr[r]; k < d->csr_ptr[r + 1]; ++k)
        if (d->csr_col[k] < 0 || d->csr_col[k] >= S) return fail(CMDP_ERR_INVALID, "csr_col out of range at %lld", (long long)k);
    }
  }
  const ChainPlan p = plan_chains(B, A, d->state_off, d->csr_ptr, d->csr_col, d->csr_val);
  *n_cand = (int64_t)p.cand.size();
  if (*n_cand > cand_capacity) return fail(CMDP_ERR_INVALID, "the plan has %lld candidates, room for %lld", (long long)*n_cand, (long long)cand_capacity);
  std::copy(p.rank.begin(), p.rank.end(), rank);
  std::copy(p.cptr.begin(), p.cptr.end(), cptr);
  std::copy(p.cbase.begin(), p.cbase.end(), cbase);
  std::copy(p.cand.begin(), p.cand.end(), cand);
  std::copy(p.nrounds.begin(), p.nrounds.end(), nrounds);
  std::copy(p.rbase.begin(), p.rbase.end(), rbase);
  std::copy(p.rptr.begin(), p.rptr.end(), rptr);
  std::copy(p.piv.begin(), p.piv.end(), piv);
  return CMDP_OK;
}

int cmdp_chain_choice(int max_S, int max_row_nnz, int exact_order, int fast_enabled, int any_plan, int64_t out[4]) {
  if (!out || max_S < 1 || max_row_nnz < 1) return fail(CMDP_ERR_INVALID, "bad argument");
  const ChainChoice k = pick_chain(max_S, max_row_nnz, chain_lds_bytes(max_S, max_row_nnz), chain_fast_lds_bytes(max_S, max_row_nnz, kChainRoundWidth),
                                   exact_order != 0, fast_enabled != 0, any_plan != 0);
  const int64_t v[4] = {k.refusal, (int64_t)k.k9_lds, k.fast, (int64_t)k.fast_lds};
  std::copy(v, v + 4, out);
  return CMDP_OK;
}

int cmdp_set_observation_table(cmdp_t* h, const float* table, int32_t F, int time_indexed) {
  if (int rc = bind(h)) return rc;
  if (!h->has_env) return fail(CMDP_ERR_INVALID, "handle was created without the sampler half");
  if (!table || F < 1) return fail(CMDP_ERR_INVALID, "null table or F < 1");
  if (time_indexed && h->H < 1) return fail(CMDP_ERR_INVALID, "a time-indexed table needs an episodic handle");
  hipStream_t st = h->stream;
  const size_t n = (size_t)(time_indexed ? h->H : 1) * (size_t)h->n_states * (size_t)F;
  HIP_TRY(h->d_obs_table.upload(table, n, st));
  HIP_TRY(h->d_obs_out.alloc((size_t)h->B * F));
  HIP_TRY(h->d_n_obs.alloc((size_t)h->B));
  HIP_TRY(h->d_n_obs.zero(st));
  HIP_TRY(hipStreamSynchronize(st));
  h->obs_F = F;
  h->obs_time_indexed = time_indexed ? 1 : 0;
  return CMDP_OK;
}

int cmdp_observe_noise(cmdp_t* h, int kind, double scale, double df, const float* chol, float* obs) {
  if (int rc = bind(h)) return rc;
  if (!obs) return fail(CMDP_ERR_INVALID, "null output");
  if (h->obs_F < 1) return fail(CMDP_ERR_INVALID, "no observation table: call cmdp_set_observation_table first");
  if (kind < CMDP_NOISE_NONE || kind > CMDP_NOISE_STUDENT_T_CORRELATED) return fail(CMDP_ERR_INVALID, "unknown noise kind %d", kind);
  const bool noisy = kind >= CMDP_NOISE_GAUSSIAN_CORRELATED || (kind == CMDP_NOISE_GAUSSIAN && scale > 0.0);
  if (noisy && h->rng_mode != CMDP_RNG_PHILOX)
    return fail(CMDP_ERR_UNSUPPORTED, "device noise needs CMDP_RNG_PHILOX (the reference-exact noise stream is host side)");
  const bool correlated = kind == CMDP_NOISE_GAUSSIAN_CORRELATED || kind == CMDP_NOISE_STUDENT_T_CORRELATED;
  if (correlated && !chol) return fail(CMDP_ERR_INVALID, "correlated noise needs the Cholesky factor");
  if ((kind == CMDP_NOISE_STUDENT_T || kind == CMDP_NOISE_STUDENT_T_CORRELATED) && !(df > 0.0))
    return fail(CMDP_ERR_INVALID, "Student-t noise needs df > 0");
  const size_t lds = correlated ? sizeof(double) * (size_t)h->obs_F : 0;
  if (lds > (size_t)kLdsBudget - 1024) return fail(CMDP_ERR_UNSUPPORTED, "observations of %d elements: the normals do not fit LDS", h->obs_F);
  hipStream_t st = h->stream;
  if (correlated) HIP_TRY(h->d_obs_chol.upload(chol, (size_t)h->obs_F * h->obs_F, st));
  EmitArgs e{};
  e.B = h->B; e.F = h->obs_F; e.H = h->H; e.time_indexed = h->obs_time_indexed;
  e.state_off = h->d_state_off.p; e.table = h->d_obs_table.p; e.cur = h->d_cur.p; e.hstep = h->d_h.p;
  e.key = h->d_key.p; e.n_obs = h->d_n_obs.p; e.scale = scale; e.kind = kind; e.df = df;
  e.chol = correlated ? h->d_obs_chol.p : nullptr; e.out = h->d_obs_out.p;
  if (int rc = set_lds(k_emit, lds)) return rc;
  hipLaunchKernelGGL(k_emit, dim3(h->B), dim3(256), lds, st, e);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(obs, h->d_obs_out.p, sizeof(float) * (size_t)h->B * h->obs_F, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

int cmdp_observe(cmdp_t* h, double noise_scale, float* obs) {
  return cmdp_observe_noise(h, noise_scale > 0.0 ? CMDP_NOISE_GAUSSIAN : CMDP_NOISE_NONE, noise_scale, 0.0, nullptr, obs);
}

}  // extern "C"

// Mixing time of one instance by matrix powers (see cmdp.h).  d(t) = max_s TV(P^t(s, .), pi) is non-increasing in t, so:
// square A_k = P^(2^k) until d(2^K) <= threshold (then t_mix lies in (2^(K-1), 2^K]), walk back down multiplying the
// stored powers in (binary search on t, one dgemm per bit), and finish the last 2^r steps -- r = the lowest power still
// held when HBM ran out of S x S buffers -- with sparse steps.
static int mixing_time_dense(cmdp_t* h, int b, const int64_t* d_cptr, const int32_t* d_crow, const double* d_cval,
                             const double* d_stat, double threshold, int64_t max_steps, int64_t* t_mix, double* tv_at) {
  hipStream_t st = h->stream;
  const int64_t so = h->state_off[b];
  const int S = (int)(h->state_off[b + 1] - so);
  const size_t bytes = sizeof(double) * (size_t)S * (size_t)S;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  int cap = (int)std::min<size_t>(24, (free_b / 10 * 9) / bytes);
  if (const char* e = std::getenv("CMDP_MIX_MAX_BUFFERS")) cap = std::min(cap, std::atoi(e));  // tests: force the sparse tail
  if (cap < 3)
    return fail(CMDP_ERR_UNSUPPORTED, "mixing time of %d states needs three %zu-byte matrices, %zu bytes are free", S, bytes, free_b);
  std::vector<DevBuf<double>> pool((size_t)cap);
  std::vector<int> free_list;
  for (int i = 0; i < cap; ++i) free_list.push_back(i);
  auto take = [&](int* idx) -> int {
    *idx = free_list.back();
    free_list.pop_back();
    if (!pool[(size_t)*idx].p) {
      if (hipError_t e = pool[(size_t)*idx].alloc((size_t)S * S); e != hipSuccess)
        return fail(CMDP_ERR_HIP, "mixing-time matrix of %zu bytes: %s", bytes, hipGetErrorString(e));
    }
    return CMDP_OK;
  };
  DevBuf<unsigned long long> d_tv;
  HIP_TRY(d_tv.alloc(1));
  MixDense m{S, so, d_cptr, d_crow, d_cval, d_stat, d_tv.p};
  // the total-variation word a kernel leaves in d_tv (the bits of a double, raised by atomic max): cleared, `launch`, read
  auto tv_after = [&](auto launch, double* out) -> int {
    HIP_TRY(d_tv.zero(st));
    launch();
    HIP_TRY(hipGetLastError());
    unsigned long long bits = 0;
    HIP_TRY(hipMemcpyAsync(&bits, d_tv.p, sizeof bits, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(out, &bits, sizeof(double));
    return CMDP_OK;
  };
  auto tv_of = [&](const double* X, double* out) -> int {
    return tv_after([&] { hipLaunchKernelGGL(k_mixd_tv, dim3((unsigned)S), dim3(256), 0, st, m, X); }, out);
  };
  rocblas_handle blas = nullptr;
  if (rocblas_create_handle(&blas) != rocblas_status_success) return fail(CMDP_ERR_HIP, "rocblas_create_handle failed");
  struct BlasGuard { rocblas_handle h; ~BlasGuard() { rocblas_destroy_handle(h); } } guard{blas};
  if (rocblas_set_stream(blas, st) != rocblas_status_success) return fail(CMDP_ERR_HIP, "rocblas_set_stream failed");
  // row-major Z = X * Y  <=>  column-major Z^T = Y^T * X^T
  auto matmul = [&](const double* X, const double* Y, double* Z) -> int {
    const double one = 1.0, zero = 0.0;
    if (rocblas_dgemm(blas, rocblas_operation_none, rocblas_operation_none, S, S, S, &one, Y, S, X, S, &zero, Z, S) !=
        rocblas_status_success)
      return fail(CMDP_ERR_HIP, "rocblas_dgemm failed");
    return CMDP_OK;
  };
  *t_mix = -1;
  if (tv_at) *tv_at = 0.0;
  std::vector<int> power;  // power[i] = pool index of A_(r+i)
  int r = 0, idx = 0;
  if (int rc = take(&idx)) return rc;
  HIP_TRY(hipMemsetAsync(pool[(size_t)idx].p, 0, bytes, st));
  hipLaunchKernelGGL(k_mixd_build, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, m, pool[(size_t)idx].p);
  HIP_TRY(hipGetLastError());
  power.push_back(idx);
  double d = 0.0;
  if (int rc = tv_of(pool[(size_t)idx].p, &d)) return rc;
  if (tv_at) *tv_at = d;
  if (d <= threshold) {
    *t_mix = 1;
    return CMDP_OK;
  }
  // ---- doubling: A_(K) = A_(K-1)^2 until mixed ------------------------------------------------------------------
  int K = 0;  // the newest power is A_K, t = 2^K, not mixed
  while (true) {
    if (((int64_t)1 << K) >= max_steps) return CMDP_OK;  // not mixed at 2^K >= max_steps: -1
    if (free_list.empty()) {  // drop the lowest power: the final stretch of sparse steps doubles
      free_list.push_back(power.front());
      power.erase(power.begin());
      ++r;
    }
    if (int rc = take(&idx)) return rc;
    const double* prev = pool[(size_t)power.back()].p;
    if (int rc = matmul(prev, prev, pool[(size_t)idx].p)) return rc;
    power.push_back(idx);
    ++K;
    if (int rc = tv_of(pool[(size_t)idx].p, &d)) return rc;
    if (std::getenv("CMDP_MIX_DEBUG")) std::fprintf(stderr, "[mixing] t = 2^%d: max TV %.6g (%d powers held from 2^%d)\n", K, d, (int)power.size(), r);
    if (d <= threshold) break;
    if (tv_at) *tv_at = d;
  }
  // ---- binary search on t: cur = P^lo (not mixed), lo + 2^k' mixed for the current k' ----------------------------------
  int64_t lo = (int64_t)1 << (K - 1);
  int cand = power.back();              // A_K: mixed, its buffer is scratch from here on
  int cur = power[power.size() - 2];    // A_(K-1)
  double d_hi = d;                      // TV at the smallest t known to be mixed
  for (int k = K - 2; k >= r; --k) {
    const double* Ak = pool[(size_t)power[(size_t)(k - r)]].p;
    if (int rc = matmul(pool[(size_t)cur].p, Ak, pool[(size_t)cand].p)) return rc;
    if (int rc = tv_of(pool[(size_t)cand].p, &d)) return rc;
    if (d > threshold) {
      std::swap(cur, cand);  // A_(K-1)'s buffer becomes scratch: no lower step multiplies by it again
      lo += (int64_t)1 << k;
      if (tv_at) *tv_at = d;
    } else {
      d_hi = d;
    }
  }
  // ---- the last 2^r steps one at a time ---------------------------------------------------------------------------------
  const int64_t last = (int64_t)1 << r;
  for (int64_t i = 1; i <= last; ++i) {
    if (i == last) {  // lo + 2^r is known to be mixed
      d = d_hi;
    } else {
      const auto step = [&] { hipLaunchKernelGGL(k_mixd_step, dim3((unsigned)S), dim3(256), 0, st, m, pool[(size_t)cur].p, pool[(size_t)cand].p); };
      if (int rc = tv_after(step, &d)) return rc;
      std::swap(cur, cand);
    }
    if (d <= threshold) {
      if (lo + i <= max_steps) {
        *t_mix = lo + i;
        if (tv_at) *tv_at = d;
      }
      return CMDP_OK;
    }
    if (tv_at) *tv_at = d;
  }
  return fail(CMDP_ERR_HIP, "mixing-time search lost its bracket (total variation is not monotone?)");
}

extern "C" {

int cmdp_mixing_time(cmdp_t* h, const float* pi, const double* stationary, double threshold, int64_t max_steps,
                     int64_t* t_mix, double* tv_at) {
  if (int rc = bind(h)) return rc;
  if (!h->has_dp) return fail(CMDP_ERR_INVALID, "handle was created without the DP half");
  if (!stationary || !t_mix) return fail(CMDP_ERR_INVALID, "null argument");
  if (!(threshold > 0.0) || max_steps < 1) return fail(CMDP_ERR_INVALID, "threshold <= 0 or max_steps < 1");
  MixingPath path;
  if (int rc = pick_mixing_path(h->mixing_path, h->max_S, &path)) return rc;
  hipStream_t st = h->stream;
  const int B = h->B;
  const int64_t NS = h->n_states;
  std::vector<int64_t> ptr;
  std::vector<int32_t> col;
  std::vector<float> val;
  if (int rc = fetch_csr(h, &ptr, &col, &val)) return rc;
  const PolicyCsc csc = policy_chain_csc(B, h->A, h->state_off.data(), ptr.data(), col.data(), val.data(), pi);
  constexpr int CH = 256;
  DevBuf<int64_t> d_cptr, d_xoff;
  DevBuf<int32_t> d_crow;
  DevBuf<double> d_cval, d_stat, d_X, d_Xn;
  DevBuf<unsigned long long> d_dl;
  HIP_TRY(d_cptr.upload(csc.cptr.data(), csc.cptr.size(), st));
  HIP_TRY(d_xoff.upload(csc.xoff.data(), csc.xoff.size(), st));
  HIP_TRY(d_crow.upload(csc.crow.data(), csc.crow.size(), st));
  HIP_TRY(d_cval.upload(csc.cval.data(), csc.cval.size(), st));
  HIP_TRY(d_stat.upload(stationary, (size_t)NS, st));
  if (path == MIXING_POWERS) {
    for (int b = 0; b < B; ++b)
      if (int rc = mixing_time_dense(h, b, d_cptr.p, d_crow.p, d_cval.p, d_stat.p, threshold, max_steps, t_mix + b,
                                     tv_at ? tv_at + b : nullptr))
        return rc;
    return CMDP_OK;
  }
  HIP_TRY(d_X.alloc((size_t)csc.xoff[B]));
  HIP_TRY(d_Xn.alloc((size_t)csc.xoff[B]));
  HIP_TRY(d_dl.alloc((size_t)B * CH));
  MixArgs m{};
  m.B = B; m.state_off = h->d_state_off.p; m.x_off = d_xoff.p; m.csc_ptr = d_cptr.p; m.csc_row = d_crow.p;
  m.csc_val = d_cval.p; m.stationary = d_stat.p; m.X = d_X.p; m.Xnew = d_Xn.p; m.dlist = d_dl.p; m.chunk = CH;
  hipLaunchKernelGGL(k_mix_init, dim3((unsigned)NS), dim3(256), 0, st, m);
  HIP_TRY(hipGetLastError());
  const size_t lds = sizeof(double) * (size_t)h->max_S;
  if (int rc = set_lds(k_mix_step, lds)) return rc;
  std::vector<unsigned long long> dl((size_t)B * CH);
  std::vector<char> found((size_t)B, 0);
  for (int b = 0; b < B; ++b) { t_mix[b] = -1; if (tv_at) tv_at[b] = 0.0; }
  int remaining = B;
  for (int64_t t0 = 0; t0 < max_steps && remaining > 0; t0 += CH) {
    const int n = (int)std::min<int64_t>(CH, max_steps - t0);
    HIP_TRY(hipMemsetAsync(d_dl.p, 0, sizeof(unsigned long long) * dl.size(), st));
    for (int k = 0; k < n; ++k) {
      m.k = k;
      hipLaunchKernelGGL(k_mix_step, dim3((unsigned)NS), dim3(256), lds, st, m);
      std::swap(m.X, m.Xnew);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dl.data(), d_dl.p, sizeof(unsigned long long) * dl.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) {
      if (found[b]) continue;
      for (int k = 0; k < n; ++k) {
        double tv;
        std::memcpy(&tv, &dl[(size_t)b * CH + k], sizeof(double));
        if (tv <= threshold) {
          t_mix[b] = t0 + k + 1;  // X after (t0 + k + 1) steps
          if (tv_at) tv_at[b] = tv;
          found[b] = 1;
          --remaining;
          break;
        }
        if (tv_at) tv_at[b] = tv;
      }
    }
  }
  return CMDP_OK;
}

int cmdp_qlearning_destroy(cmdp_agent_t* a) { return agent_destroy(a); }

// the interaction kernel of `n_steps` steps on the handle's stream (no synchronisation, no copies)
static int ql_launch(cmdp_agent_t* a, int64_t n_steps, const uint8_t* dmask, int8_t* d_actions, int resume, double* cum_host) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const dim3 grid(grid_for(h->B, 256)), block(256);
  const RewardCache rc = h->rcache();
#define QL_LAUNCH(K, ARGS) hipLaunchKernelGGL(K, grid, block, 0, st, h->env(), ARGS, n_steps, dmask, d_actions, a->d_rsum.p, rc, resume, cum_host)
  if (h->reward_cache) {
    if (a->continuous) QL_LAUNCH(k_qlearn_continuous<true>, a->cargs);
    else if (a->args.ucb == 0) QL_LAUNCH((k_qlearn_episodic<0, true>), a->args);
    else QL_LAUNCH((k_qlearn_episodic<1, true>), a->args);
  } else {
    if (a->continuous) QL_LAUNCH(k_qlearn_continuous<false>, a->cargs);
    else if (a->args.ucb == 0) QL_LAUNCH((k_qlearn_episodic<0, false>), a->args);
    else QL_LAUNCH((k_qlearn_episodic<1, false>), a->args);
  }
#undef QL_LAUNCH
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}
// With reference-exact reward caches the call returns with the stream idle (instances park, the host fills their blocks,
// the kernel is relaunched); otherwise nothing is synchronised.
// `cum_host` (nullable): page-locked host array that receives the running reward sums at the end of the launch.
static int ql_enqueue_run(cmdp_agent_t* a, int64_t n_steps, const uint8_t* dmask, int8_t* d_actions, double* cum_host = nullptr) {
  if (int rc = visits_check(a->env, n_steps)) return rc;
  auto launch = [&](int resume) -> int { return ql_launch(a, n_steps, dmask, d_actions, resume, cum_host); };
  return visits_commit(a->env, n_steps, a->env->reward_cache ? rc_drive(a->env, launch) : launch(0));
}

int cmdp_qlearning_run(cmdp_agent_t* a, int64_t n_steps, const uint8_t* train_mask, int8_t* actions_trace,
                       double* reward_sum) {
  if (int rc = agent_run_check(a, n_steps)) return rc;
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const size_t NB = (size_t)n_steps * h->B;
  const uint8_t* dmask = nullptr;
  if (int rc = agent_stage_run(a, NB, actions_trace != nullptr, train_mask, &dmask)) return rc;
  if (int rc = ql_enqueue_run(a, n_steps, dmask, actions_trace ? a->d_act.p : nullptr)) return rc;
  if (actions_trace) HIP_TRY(hipMemcpyAsync(actions_trace, a->d_act.p, NB, hipMemcpyDeviceToHost, st));
  if (reward_sum) HIP_TRY(hipMemcpyAsync(reward_sum, a->d_rsum.p, sizeof(double) * h->B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

// What the value of a policy on the true episodic MDP asks of the handle; `dp_code` / `dp_text`: the entry point's refusal of
// a handle without the DP half
static int episodic_value_check(cmdp_t* h, int dp_code, const char* dp_text) {
  if (!h->has_dp) return fail(dp_code, "%s", dp_text);
  if (2 * sizeof(float) * (size_t)h->max_S > (size_t)kLdsBudget)
    return fail(CMDP_ERR_UNSUPPORTED, "instance with %d states does not fit LDS", h->max_S);
  return CMDP_OK;
}

// One-hot policy `pi` [H][S][A] per instance (device) -> episodic policy evaluation on the true MDP -> V[0, :] packed into
// `v0` (device-accessible); `snap` (nullable, device-accessible [3][B]) receives last_start | prev_start | hstep from the
// same gather.  After episodic_value_check; no synchronisation.
static int enqueue_episodic_value(cmdp_t* h, const float* pi, float* v0, int32_t* snap) {
  hipStream_t st = h->stream;
  const int H = h->H;
  const size_t lds = 2 * sizeof(float) * (size_t)h->max_S;
  const size_t nq = (size_t)(H + 1) * h->n_rows, nv = (size_t)(H + 1) * h->n_states;
  if (h->d_Q.n < nq) HIP_TRY(h->d_Q.alloc(nq));
  if (h->d_V.n < nv) HIP_TRY(h->d_V.alloc(nv));
  DpTables t = dp_tables(h);
  t.pi = pi;
  if (int rc = set_lds(k_episodic<DP_PE>, lds)) return rc;
  hipLaunchKernelGGL((k_episodic<DP_PE>), dim3(h->B), dim3(kDpBlock), lds, st, t, H, h->d_Q.p, h->d_V.p);
  HIP_TRY(hipGetLastError());
  // V[0, :] of instance b sits at (H+1)*state_off[b]: pack
  hipLaunchKernelGGL(k_gather_v0, dim3(h->B), dim3(256), 0, st, h->B, H, h->d_state_off.p, h->d_V.p, v0, h->d_last_start.p,
                     h->d_prev_start.p, h->d_h.p, snap);
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

// greedy policy of the agents' Q tables -> its value -> V[0, :] packed into `v0_out` (null: a->d_v0); no synchronisation
static int ql_enqueue_evaluate(cmdp_agent_t* a, float* v0_out = nullptr, int32_t* snap = nullptr) {
  cmdp_t* h = a->env;
  if (a->continuous) return fail(CMDP_ERR_INVALID, "cmdp_qlearning_evaluate is for the episodic agent; use cmdp_qlearning_policy");
  if (int rc = episodic_value_check(h, CMDP_ERR_INVALID, "the environment handle was created without the DP half")) return rc;
  if (int rc = ql_enqueue_greedy(a)) return rc;
  if (a->d_v0.n < (size_t)h->n_states) HIP_TRY(a->d_v0.alloc(h->n_states));
  return enqueue_episodic_value(h, a->d_pi.p, v0_out ? v0_out : a->d_v0.p, snap);
}

int cmdp_qlearning_evaluate(cmdp_agent_t* a, float* V0) {
  if (!a || !V0) return fail(CMDP_ERR_INVALID, "null argument");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  if (int rc = ql_enqueue_evaluate(a)) return rc;
  HIP_TRY(hipMemcpyAsync(V0, a->d_v0.p, sizeof(float) * (size_t)h->n_states, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CMDP_OK;
}

// ---- the logged loop: cmdp_logged_loop.h has its rows, its run-ahead rule and a row's host work; here is the device --------
// The switches of the logged loop, read nowhere else and once per process.
// CMDP_LOGGED_PIPELINE = 0 | 1 decides whether rows that cannot change the training mask run ahead; unset: on, except under
// rocprofv3 (its tool library in LD_PRELOAD or its ROCPROF* variables in the environment), whose queue interception faults
// on a stream that never drains.
// CMDP_LOGGED_DRAIN_EVERY = n: the stream is drained completely every n rows (0: never).  Only for runs under rocprofv3,
// whose queue interception faulted in hipLaunchKernel's argument copy once a stream stayed busy long enough for the
// runtime's kernel-argument pool to wrap (ROCm 7.2; the same run outside the profiler is fine).
// CMDP_LOGGED_DEBUG (set): where the host thread's time went (stderr, one line per call).
static const cmdp_tracker::LoggedSwitches& logged_switches() {
  static const cmdp_tracker::LoggedSwitches sw = [] {
    cmdp_tracker::LoggedSwitches s{true, false, 0, std::getenv("CMDP_LOGGED_DEBUG") != nullptr};
    if (const char* e = std::getenv("CMDP_LOGGED_PIPELINE")) {
      s.pipeline = std::atoi(e) != 0;
    } else {
      const char* pre = std::getenv("LD_PRELOAD");
      if (pre && std::strstr(pre, "rocprof")) s.pipeline = false;
      for (char** ev = environ; ev && *ev; ++ev)
        if (!std::strncmp(*ev, "ROCPROF", 7)) s.pipeline = false;
    }
    const char* sync = std::getenv("CMDP_SYNC_MODE");
    s.blocking_sync = sync && !std::strcmp(sync, "block");
    if (const char* e = std::getenv("CMDP_LOGGED_DRAIN_EVERY")) s.drain_every = std::atoi(e);
    return s;
  }();
  return sw;
}

// the rows of (n_steps, log_every), for a caller whose arrays hold n_logs rows
static int logged_plan(const cmdp_loop_desc* d, int64_t n_logs, std::vector<cmdp_tracker::LoggedRow>* rows) {
  if (d->n_steps < 1) return fail(CMDP_ERR_INVALID, "n_steps < 1");
  cmdp_tracker::plan_logged_rows(d->n_steps, d->log_every, rows);
  if (n_logs != (int64_t)rows->size())
    return fail(CMDP_ERR_INVALID, "n_logs must be %lld for %lld steps logged every %lld", (long long)rows->size(), (long long)d->n_steps,
                (long long)d->log_every);
  return CMDP_OK;
}

// The rows' host work alone, on inputs given by the caller (no device involved): what cmdp_qlearning_run_logged does with
// the values it reads back at every logging step.  Exists so that the CPU test suite can hold the C++ tracker against the
// reference's own indicator code (golden G15), and the schedule and the run-ahead rule against the rows: `ahead` is decided
// as the driver decides it with a clock that never runs out, so log_row's check meets every freeze of the inputs.
int cmdp_tracker_replay(const cmdp_loop_desc* d, int32_t B, int32_t episodic, const int64_t* state_off, int64_t n_logs,
                        const int64_t* log_steps, const uint8_t* in_loop, const int64_t* n_since, const double* cum_reward,
                        const float* V0, const int64_t* start_state, const double* avg, const int32_t* avg_kind,
                        double* values, uint8_t* kinds, uint8_t* is_training) {
  using namespace cmdp_tracker;
  if (!d || !cum_reward || !values || !kinds) return fail(CMDP_ERR_INVALID, "null argument");
  std::vector<LoggedRow> rows;
  if (!log_steps && !in_loop && !n_since) {
    if (int rc = logged_plan(d, n_logs, &rows)) return rc;
  } else {
    if (!log_steps || !in_loop || !n_since) return fail(CMDP_ERR_INVALID, "null argument");
    for (int64_t i = 0; i < n_logs; ++i) rows.push_back(LoggedRow{log_steps[i], 0, n_since[i], in_loop[i] != 0});
  }
  std::vector<uint8_t> mask((size_t)B), need((size_t)B);
  // last_start | prev_start | hstep, never 0: `start_state` already names the start of the logged episode
  std::vector<int32_t> snap((size_t)3 * B, 1);
  LoggedRun run;
  run.init(B, episodic != 0, d->n_steps, d, d->horizon, state_off, mask.data(), nullptr);
  const int64_t NS = episodic ? state_off[B] : 0;
  for (int64_t i = 0; i < n_logs; ++i) {
    const LoggedRow& r = rows[(size_t)i];
    RowReadback in{cum_reward + (size_t)i * B, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (episodic) {
      for (int b = 0; b < B; ++b) snap[(size_t)b] = (int32_t)start_state[(size_t)i * B + b];
      in.v0 = V0 + (size_t)i * NS;
      in.snap = snap.data();
    } else {
      continuous_need(run.tr, need.data());
      in.need = need.data();
      in.avg = avg + (size_t)i * B;
      in.akind = avg_kind + (size_t)i * B;
    }
    const bool ahead = i + 1 < n_logs && !row_may_freeze(run.tr, episodic != 0, r.t, d->n_steps);
    bool changed = false;
    if (int rc = log_row(run, r, in, 0.0, std::numeric_limits<double>::infinity(), ahead, values + (size_t)i * N_COLUMNS * B,
                         kinds + (size_t)i * N_COLUMNS * B, &changed))
      return rc;
    if (is_training)
      for (int b = 0; b < B; ++b) is_training[(size_t)i * B + b] = run.tr.inst[(size_t)b].training ? 1 : 0;
  }
  return CMDP_OK;
}

int cmdp_greedy_policy_episodic(cmdp_t* h, int H, int q_layers, const float* Q, float* pi) {
  if (int rc = bind(h)) return rc;
  if (!Q || !pi || H < 1 || q_layers < H) return fail(CMDP_ERR_INVALID, "bad argument");
  hipStream_t st = h->stream;
  DevBuf<float>&d_q = h->d_gp_q, &d_p = h->d_gp_p;
  HIP_TRY(d_q.upload(Q, (size_t)q_layers * h->n_rows, st));
  HIP_TRY(d_p.alloc((size_t)H * h->n_rows));
  hipLaunchKernelGGL(k_greedy_policy_episodic<float>, dim3(h->B), dim3(64), 0, st, h->B, h->A, H, q_layers,
                     h->d_state_off.p, d_q.p, d_p.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(pi, d_p.p, sizeof(float) * (size_t)H * h->n_rows, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

int cmdp_qlearning_tables(cmdp_agent_t* a, float* Q, int32_t* N) {
  if (!a) return fail(CMDP_ERR_INVALID, "null agent");
  if (int rc = bind(a->env)) return rc;
  hipStream_t st = a->env->stream;
  if (Q && a->continuous)  // the continuous agent's tables are float64: Q is read as `double*` here
    HIP_TRY(hipMemcpyAsync(Q, a->d_Qc.p, sizeof(double) * a->n_q, hipMemcpyDeviceToHost, st));
  else if (Q) HIP_TRY(hipMemcpyAsync(Q, a->d_Q.p, sizeof(float) * a->n_q, hipMemcpyDeviceToHost, st));
  if (N) HIP_TRY(hipMemcpyAsync(N, a->d_N.p, sizeof(int32_t) * a->n_q, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

int cmdp_gth(int count, const int32_t* dims, const double* mats, double* out) {
  if (count < 0 || (count > 0 && (!dims || !mats || !out))) return fail(CMDP_ERR_INVALID, "bad argument");
  if (count == 0) return CMDP_OK;
  std::vector<int64_t> moff((size_t)count), xoff((size_t)count);
  int64_t mt = 0, xt = 0;
  for (int m = 0; m < count; ++m) {
    if (dims[m] < 1 || dims[m] > 46340) return fail(CMDP_ERR_INVALID, "chain %d has dimension %d", m, dims[m]);
    moff[m] = mt; xoff[m] = xt;
    mt += (int64_t)dims[m] * dims[m];
    xt += dims[m];
  }
  struct Ws { DevBuf<int64_t> moff, xoff; DevBuf<int32_t> dims; DevBuf<double> mats, x; };
  DeviceWorkspace<Ws> ws;
  if (int rc = ws.acquire()) return rc;
  hipStream_t st = ws.st;
  HIP_TRY(ws->moff.upload(moff.data(), count, st));
  HIP_TRY(ws->xoff.upload(xoff.data(), count, st));
  HIP_TRY(ws->dims.upload(dims, count, st));
  HIP_TRY(ws->mats.upload(mats, (size_t)mt, st));
  HIP_TRY(ws->x.alloc((size_t)xt));
  hipLaunchKernelGGL(k_gth, dim3(count), dim3(256), 0, st, ws->moff.p, ws->dims.p, ws->xoff.p, ws->mats.p, ws->x.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(ws->x.download(out, (size_t)xt, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

// K10's launch on device-resident arguments: what cmdp_extended_vi does after its uploads and what the UCRL2 agent
// (cmdp_ucrl2_*) does for the instances of a round, block k solving the k-th entry of the per-launch arrays
static int evi_launch(const EviArgs& a, int count, size_t lds, hipStream_t st) {
  if (int rc = set_lds(k_evi, lds)) return rc;
  hipLaunchKernelGGL(k_evi, dim3(count), dim3(EVI_THREADS), lds, st, a);
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

int cmdp_extended_vi(int count, const int32_t* n_states, const int32_t* n_actions, const int64_t* csr_ptr,
                     const int32_t* csr_col, const float* csr_val, const float* uniform, const float* rewards,
                     const double* beta_r, const double* beta_p0, const double* r_max, double epsilon,
                     int64_t max_sweeps, float* Q, float* V, double* span, int64_t* sweeps, int32_t* status) {
  if (count < 0) return fail(CMDP_ERR_INVALID, "count %d is negative", count);
  if (count == 0) return CMDP_OK;
  if (!n_states || !n_actions || !csr_ptr || !rewards || !beta_r || !beta_p0 || !r_max || !Q || !V || !span ||
      !sweeps || !status)
    return fail(CMDP_ERR_INVALID, "null argument");
  if (!(epsilon >= 0.0) || !std::isfinite(epsilon)) return fail(CMDP_ERR_INVALID, "epsilon %g is not a finite value >= 0", epsilon);
  if (max_sweeps < 1) return fail(CMDP_ERR_INVALID, "max_sweeps %lld < 1", (long long)max_sweeps);
  BatchLayout L;
  if (int rc = L.build(count, n_states, n_actions,
                       {EVI_MAX_STATES, "instance %d has %d states: extended value iteration keeps u1, u2 and the order in "
                                        "LDS for at most %d states"}))
    return rc;
  for (int b = 0; b < count; ++b)
    if (!std::isfinite(r_max[b])) return fail(CMDP_ERR_INVALID, "r_max[%d] is not finite", b);
  std::vector<float> uni;
  if (int rc = check_row_form(L, {csr_ptr, csr_col, csr_val, uniform, rewards}, &uni, [&](int64_t r) -> int {
        if (!std::isfinite(beta_r[r])) return fail(CMDP_ERR_INVALID, "beta_r[%lld] is not finite", (long long)r);
        if (!std::isfinite(beta_p0[r])) return fail(CMDP_ERR_INVALID, "beta_p0[%lld] is not finite", (long long)r);
        return CMDP_OK;
      }))
    return rc;
  const int64_t ns = L.ns, nr = L.nr, nnz = csr_ptr[nr];
  struct Ws {
    DevBuf<int32_t> S, A, col, status;
    DevBuf<int64_t> soff, roff, ptr, sweeps;
    DevBuf<float> val, uni, R, Q, V;
    DevBuf<double> beta_r, beta_p0, r_max, span;
  };
  DeviceWorkspace<Ws> ws;
  if (int rc = ws.acquire()) return rc;
  hipStream_t st = ws.st;
  HIP_TRY(ws->S.upload(n_states, count, st));
  HIP_TRY(ws->A.upload(n_actions, count, st));
  HIP_TRY(ws->soff.upload(L.soff.data(), L.soff.size(), st));
  HIP_TRY(ws->roff.upload(L.roff.data(), count, st));
  HIP_TRY(ws->ptr.upload(csr_ptr, (size_t)nr + 1, st));
  HIP_TRY(ws->col.upload(csr_col, (size_t)nnz, st));
  HIP_TRY(ws->val.upload(csr_val, (size_t)nnz, st));
  HIP_TRY(ws->uni.upload(uni.data(), (size_t)nr, st));
  HIP_TRY(ws->R.upload(rewards, (size_t)nr, st));
  HIP_TRY(ws->beta_r.upload(beta_r, (size_t)nr, st));
  HIP_TRY(ws->beta_p0.upload(beta_p0, (size_t)nr, st));
  HIP_TRY(ws->r_max.upload(r_max, count, st));
  HIP_TRY(ws->Q.alloc((size_t)nr));
  HIP_TRY(ws->V.alloc((size_t)ns));
  HIP_TRY(ws->span.alloc(count));
  HIP_TRY(ws->sweeps.alloc(count));
  HIP_TRY(ws->status.alloc(count));
  EviArgs a{ws->S.p, ws->A.p, ws->soff.p, ws->roff.p, ws->ptr.p, ws->col.p, ws->val.p, ws->uni.p, ws->R.p,
            ws->beta_r.p, ws->beta_p0.p, ws->r_max.p, epsilon, max_sweeps, ws->Q.p, ws->V.p, ws->span.p,
            ws->sweeps.p, ws->status.p};
  if (int rc = evi_launch(a, count, evi_lds_bytes(L.max_S), st)) return rc;
  HIP_TRY(ws->Q.download(Q, (size_t)nr, st));
  HIP_TRY(ws->V.download(V, (size_t)ns, st));
  HIP_TRY(ws->span.download(span, count, st));
  HIP_TRY(ws->sweeps.download(sweeps, count, st));
  HIP_TRY(ws->status.download(status, count, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

// K14's launch on device-resident arguments: what cmdp_vi_discounted_model does after its uploads and what the UCRL2 agent
// does for its policy (cmdp_ucrl2_policy), block k solving instance list[k] (null: k)
static int mvi_launch(const ModelViArgs& a, int count, int max_S, hipStream_t st) {
  const size_t lds = model_vi_lds_bytes(max_S);
  if (int rc = set_lds(k_vi_model, lds)) return rc;
  hipLaunchKernelGGL(k_vi_model, dim3(count), dim3(MVI_THREADS), lds, st, a);
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

int cmdp_model_vi_scheme(int n_states, int n_actions, int64_t nnz, int64_t size_threshold, double density_threshold) {
  return model_vi_scheme(n_states, n_actions, nnz, size_threshold, density_threshold);
}

int cmdp_vi_discounted_model(int count, const int32_t* n_states, const int32_t* n_actions, const int64_t* csr_ptr,
                             const int32_t* csr_col, const float* csr_val, const float* uniform, const float* rewards,
                             float gamma, double epsilon, int scheme, int64_t size_threshold, double density_threshold,
                             int64_t max_sweeps, float* Q, float* V, int64_t* sweeps, int32_t* scheme_used, int32_t* status) {
  if (count < 0) return fail(CMDP_ERR_INVALID, "count %d is negative", count);
  if (count == 0) return CMDP_OK;
  if (!n_states || !n_actions || !csr_ptr || !rewards || !Q || !V || !sweeps || !scheme_used || !status)
    return fail(CMDP_ERR_INVALID, "null argument");
  if (!std::isfinite(gamma)) return fail(CMDP_ERR_INVALID, "gamma %g is not finite", (double)gamma);
  if (!(epsilon >= 0.0) || !std::isfinite(epsilon)) return fail(CMDP_ERR_INVALID, "epsilon %g is not a finite value >= 0", epsilon);
  if (max_sweeps < 1) return fail(CMDP_ERR_INVALID, "max_sweeps %lld < 1", (long long)max_sweeps);
  if (scheme != CMDP_SCHEME_AUTO && scheme != CMDP_SCHEME_JACOBI && scheme != CMDP_SCHEME_GAUSS_SEIDEL)
    return fail(CMDP_ERR_INVALID, "scheme %d: CMDP_SCHEME_AUTO, CMDP_SCHEME_JACOBI or CMDP_SCHEME_GAUSS_SEIDEL", scheme);
  if (std::isnan(density_threshold)) return fail(CMDP_ERR_INVALID, "density_threshold is not a number");
  BatchLayout L;
  if (int rc = L.build(count, n_states, n_actions,
                       {MVI_MAX_STATES, "instance %d has %d states: value iteration on a model keeps V, Vold and the shared "
                                        "products in LDS for at most %d states",
                        MVI_MAX_ACTIONS, "instance %d has %d actions: a wavefront takes the rows of a state, at most %d"}))
    return rc;
  std::vector<float> uni;
  if (int rc = check_row_form(L, {csr_ptr, csr_col, csr_val, uniform, rewards}, &uni, [](int64_t) -> int { return CMDP_OK; }))
    return rc;
  const int64_t ns = L.ns, nr = L.nr, nnz = csr_ptr[nr];
  struct Ws {
    DevBuf<int32_t> S, A, col, scheme, status;
    DevBuf<int64_t> soff, roff, ptr, sweeps;
    DevBuf<float> val, uni, R, Q, V;
  };
  DeviceWorkspace<Ws> ws;
  if (int rc = ws.acquire()) return rc;
  hipStream_t st = ws.st;
  HIP_TRY(ws->S.upload(n_states, count, st));
  HIP_TRY(ws->A.upload(n_actions, count, st));
  HIP_TRY(ws->soff.upload(L.soff.data(), L.soff.size(), st));
  HIP_TRY(ws->roff.upload(L.roff.data(), count, st));
  HIP_TRY(ws->ptr.upload(csr_ptr, (size_t)nr + 1, st));
  HIP_TRY(ws->col.upload(csr_col, (size_t)nnz, st));
  HIP_TRY(ws->val.upload(csr_val, (size_t)nnz, st));
  HIP_TRY(ws->uni.upload(uni.data(), (size_t)nr, st));
  HIP_TRY(ws->R.upload(rewards, (size_t)nr, st));
  HIP_TRY(ws->Q.alloc((size_t)nr));
  HIP_TRY(ws->V.alloc((size_t)ns));
  HIP_TRY(ws->sweeps.alloc(count));
  HIP_TRY(ws->scheme.alloc(count));
  HIP_TRY(ws->status.alloc(count));
  ModelViArgs a{ws->S.p, ws->A.p, ws->soff.p, ws->roff.p, ws->ptr.p, ws->col.p, ws->val.p, ws->uni.p, ws->R.p, nullptr,
                gamma, epsilon, scheme, size_threshold, density_threshold, max_sweeps, ws->Q.p, ws->V.p, ws->sweeps.p,
                ws->scheme.p, ws->status.p};
  if (int rc = mvi_launch(a, count, L.max_S, st)) return rc;
  HIP_TRY(ws->Q.download(Q, (size_t)nr, st));
  HIP_TRY(ws->V.download(V, (size_t)ns, st));
  HIP_TRY(ws->sweeps.download(sweeps, count, st));
  HIP_TRY(ws->scheme.download(scheme_used, count, st));
  HIP_TRY(ws->status.download(status, count, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

int cmdp_value_norm(cmdp_t* h, const float* V, float* out) {
  if (int rc = bind(h)) return rc;
  if (!h->has_dp) return fail(CMDP_ERR_INVALID, "handle was created without the DP half");
  if (!V || !out) return fail(CMDP_ERR_INVALID, "null argument");
  hipStream_t st = h->stream;
  HIP_TRY(h->d_V.upload(V, h->n_states, st));
  if (h->d_Ev.n < (size_t)h->n_rows) HIP_TRY(h->d_Ev.alloc(h->n_rows));
  if (h->d_out.n < (size_t)h->B) HIP_TRY(h->d_out.alloc(h->B));
  const DpTables t = dp_tables(h);
  hipLaunchKernelGGL(k_value_norm, dim3(h->B), dim3(256), 0, st, t, h->d_V.p, h->d_Ev.p, h->d_out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, h->d_out.p, sizeof(float) * h->B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

}  // extern "C"

// ---- UCRL2 on the device (K11, cmdp_ucrl2.h) ------------------------------------------------------------------------
struct cmdp_ucrl2 : ParkAgent {
  int bernstein_p = 0;
  double alpha_r = 1.0, alpha_p = 1.0;
  int64_t max_sweeps = 1000000;        // DP_MAX_ITERATION of the reference; CMDP_UCRL2_OPT_MAX_SWEEPS
  size_t evi_lds = 0;
  UcArgs args{};
  DevBuf<int64_t> d_iteration, d_episode, d_tr_len, d_sweeps, d_e_soff, d_e_roff, d_e_sweeps;
  DevBuf<int32_t> d_N, d_N_row, d_nu, d_kdone, d_tr_row, d_status, d_eS, d_eA, d_e_status;
  DevBuf<float> d_val, d_uni, d_ER, d_VR, d_HT, d_Q, d_sv_val, d_sv_uni, d_sv_R, d_Qs, d_V;
  DevBuf<double> d_delta, d_tr_rew, d_beta_r, d_beta_p0, d_span, d_e_rmax, d_e_span, d_host;
  PinnedBuf<int64_t> pin_iter;   // [B]
  PinnedBuf<double> pin_host;    // [3][B]: the round's scalars per parked instance
  // the policy solve (K14 through the policy stage): its per-instance arguments, uploaded by the first request
  int64_t policy_size_threshold = 300 * 3 * 300;   // CMDP_UCRL2_OPT_POLICY_SIZE_THRESHOLD
  DevBuf<int32_t> d_pS, d_pA;
  DevBuf<int64_t> d_p_roff;
  // The estimated model changes in model_update only, which ends an artificial episode: while `episode` stands, the solve
  // and its greedy policy are what they were.  p_stamp[b]: `episode` of instance b when the stage's Q and policy were last
  // computed for it by a solve that converged (-1: never, or invalidated by an option).  CMDP_UCRL2_OPT_POLICY_REUSE
  // switches it.
  bool policy_reuse = true;
  std::vector<int64_t> p_stamp, p_episode;   // [B]
};

namespace {

// bounds -> solve -> model_update for the `count` instances of pin_park's list (already on the device, d_park + 2),
// whose `iteration` the host holds in pin_iter: episode_end_update (ucrl2.py:179-190) for all of them, enqueued
int ucrl2_round(cmdp_ucrl2_t* a, int count, int stop, int64_t n_steps) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const int B = h->B, A = h->A;
  double* hv = a->pin_host.p;
  for (int k = 0; k < count; ++k) {
    const int b = a->pin_park.p[2 + k];
    const int64_t S = h->state_off[b + 1] - h->state_off[b];
    const int64_t it = a->pin_iter.p[b];
    const double delta = 1 / std::sqrt((double)(it + 1));   // self.delta = 1 / math.sqrt(self.iteration + 1)
    // math.log(log_C * (it + 1) / delta): an exact integer product, one division, one log (_chernoff, ucrl2.py:22-24)
    hv[k] = 3.5 * std::log((double)(2 * S * A * (it + 1)) / delta);
    if (a->bernstein_p) hv[B + k] = std::log(2.0 * (double)S * (double)A * (double)(it + 1) / delta);  // ucrl2.py:299
    else hv[B + k] = (double)(14 * S) * std::log((double)(2 * A * (it + 1)) / delta);
    hv[2 * B + k] = delta;
  }
  HIP_TRY(hipMemcpyAsync(a->d_host.p, hv, sizeof(double) * 3 * B, hipMemcpyHostToDevice, st));
  UcRound g{};
  g.list = a->d_park.p + 2;
  g.c_r = a->d_host.p; g.c_p = a->d_host.p + B; g.delta = a->d_host.p + 2 * B;
  g.bernstein_p = a->bernstein_p;
  g.alpha_r = a->alpha_r; g.alpha_p = a->alpha_p; g.sqrt_alpha_p = std::sqrt(a->alpha_p); g.r_max = h->rmax;
  g.eS = a->d_eS.p; g.eA = a->d_eA.p; g.e_soff = a->d_e_soff.p; g.e_roff = a->d_e_roff.p; g.e_rmax = a->d_e_rmax.p;
  g.e_span = a->d_e_span.p; g.e_sweeps = a->d_e_sweeps.p; g.e_status = a->d_e_status.p;
  hipLaunchKernelGGL(k_ucrl2_bounds, dim3(count), dim3(UCRL2_THREADS), 0, st, a->args, g, h->d_state_off.p, A);
  HIP_TRY(hipGetLastError());
  EviArgs e{a->d_eS.p, a->d_eA.p, a->d_e_soff.p, a->d_e_roff.p, a->d_row_ptr.p, a->d_col.p, a->d_sv_val.p, a->d_sv_uni.p,
            a->d_sv_R.p, a->d_beta_r.p, a->d_beta_p0.p, a->d_e_rmax.p, 1e-3, a->max_sweeps, a->d_Qs.p, a->d_V.p,
            a->d_e_span.p, a->d_e_sweeps.p, a->d_e_status.p};
  if (int rc = evi_launch(e, count, a->evi_lds, st)) return rc;
  hipLaunchKernelGGL(k_ucrl2_update, dim3(count), dim3(UCRL2_THREADS), 0, st, a->args, g, h->d_state_off.p, A, B, stop, n_steps,
                     h->d_uc_unconverged.p);
  HIP_TRY(hipGetLastError());
  h->uc_rounds += 1;
  h->uc_solves += count;
  return CMDP_OK;
}

// The open episodes' trace, [cap][B].  An artificial episode ends once a pair's visits reach max(1, its visits before the
// episode), so it is at most as long as all steps before it plus S * A, and it is part of the T steps taken in all:
// 2 * length <= T + S * A.  The buffer is sized for that with T = steps so far + the call's n_steps.
int ucrl2_ensure_trace(cmdp_ucrl2_t* a, int64_t n_steps) {
  cmdp_t* h = a->env;
  const int B = h->B;
  int64_t need = 1;
  for (int b = 0; b < B; ++b) {
    const int64_t SA = (h->state_off[b + 1] - h->state_off[b]) * h->A;
    need = std::max(need, (a->steps_total[b] + n_steps + SA + 1) / 2 + 1);
  }
  if (need <= a->args.tr_cap) return CMDP_OK;
  const int64_t cap = std::max(need, 2 * a->args.tr_cap);
  DevBuf<int32_t> nrow;
  DevBuf<double> nrew;
  if (cap > (int64_t)1 << 40 || nrow.alloc((size_t)cap * B) != hipSuccess || nrew.alloc((size_t)cap * B) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CMDP_ERR_OVERFLOW, "the trace of the open artificial episodes cannot be held: the steps so far, the %lld asked "
                "for and S * A bound an episode by %lld transitions, %lld bytes for the batch -- nothing was stepped; ask for "
                "fewer steps per call", (long long)n_steps, (long long)need, (long long)(cap * B * 12));
  }
  if (a->args.tr_cap > 0) {  // the open episodes are a prefix of the rows
    HIP_TRY(hipMemcpyAsync(nrow.p, a->d_tr_row.p, sizeof(int32_t) * a->args.tr_cap * B, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(nrew.p, a->d_tr_rew.p, sizeof(double) * a->args.tr_cap * B, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  a->d_tr_row.swap(nrow);
  a->d_tr_rew.swap(nrew);
  a->args.tr_row = a->d_tr_row.p;
  a->args.tr_rew = a->d_tr_rew.p;
  a->args.tr_cap = cap;
  return CMDP_OK;
}

}  // namespace

extern "C" {

int cmdp_ucrl2_create(cmdp_ucrl2_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon, double alpha_r,
                      double alpha_p, int bound_type_p, int bound_type_rew, int actor) {
  if (!out) return fail(CMDP_ERR_INVALID, "null output");
  *out = nullptr;
  if ((bound_type_p != CMDP_BOUND_CHERNOFF && bound_type_p != CMDP_BOUND_BERNSTEIN) ||
      (bound_type_rew != CMDP_BOUND_CHERNOFF && bound_type_rew != CMDP_BOUND_BERNSTEIN))
    return fail(CMDP_ERR_INVALID, "bound type %d / %d: CMDP_BOUND_CHERNOFF or CMDP_BOUND_BERNSTEIN (the reference asserts the same)",
                bound_type_p, bound_type_rew);
  if (bound_type_rew == CMDP_BOUND_BERNSTEIN)
    return fail(CMDP_ERR_UNSUPPORTED, "bound_type_rew = bernstein: the reference raises AttributeError at its first solve "
                "(ucrl2.py:268 reads self.r_max, which does not exist), so there is nothing to reproduce");
  if (int rc = agent_check_actor(actor)) return rc;
  if (!env || !seeds) return fail(CMDP_ERR_INVALID, "null argument (environment handle or seeds)");
  if (!(alpha_r > 0) || !(alpha_p > 0) || !std::isfinite(alpha_r) || !std::isfinite(alpha_p) || optimization_horizon < 1)
    return fail(CMDP_ERR_INVALID, "hyper-parameters out of range (alpha_r > 0, alpha_p > 0, optimization_horizon >= 1)");
  if (int rc = bind(env)) return rc;
  if (int rc = park_check_env(env, false, "UCRL2 is the continuous setting's agent (the reference has no episodic UCRL2): the "
                              "environment handle is episodic, horizon %d", "UCRL2", "extended value iteration (K10)", EVI_MAX_STATES))
    return rc;
  const int B = env->B, A = env->A;
  const int64_t R = env->n_rows;
  hipStream_t st = env->stream;
  cmdp_ucrl2_t* a = new cmdp_ucrl2;
  std::unique_ptr<cmdp_ucrl2> guard(a);
  a->env = env;
  a->bernstein_p = bound_type_p == CMDP_BOUND_BERNSTEIN;
  a->alpha_r = alpha_r;
  a->alpha_p = alpha_p;
  std::vector<int64_t> ptr;
  std::vector<int32_t> col;
  if (int rc = build_model_layout(a, ptr, col)) return rc;
  const int64_t NZ = a->nz;
  a->evi_lds = evi_lds_bytes(env->max_S);
  // tables as UCRL2Continuous.__init__ leaves them (ucrl2.py:140-159)
  std::vector<float> uni((size_t)R), er((size_t)R, (float)env->rmax), ht((size_t)R, 1.0f);
  for (int b = 0; b < B; ++b) {
    const float c = 1.0f / (float)(env->state_off[b + 1] - env->state_off[b]);   // np.ones(float32) / n_states
    for (int64_t r = env->state_off[b] * A; r < env->state_off[b + 1] * A; ++r) uni[(size_t)r] = c;
  }
  HIP_TRY(a->d_uni.upload(uni.data(), R, st));
  HIP_TRY(a->d_ER.upload(er.data(), R, st));
  HIP_TRY(a->d_HT.upload(ht.data(), R, st));
  AGENT_ZERO(d_VR, R); AGENT_ZERO(d_N, NZ); AGENT_ZERO(d_val, NZ); AGENT_ZERO(d_N_row, R); AGENT_ZERO(d_nu, R);
  AGENT_ZERO(d_kdone, R); AGENT_ZERO(d_iteration, B); AGENT_ZERO(d_episode, B); AGENT_ZERO(d_delta, B); AGENT_ZERO(d_Q, R);
  AGENT_ZERO(d_tr_len, B); AGENT_ZERO(d_sv_val, NZ); AGENT_ZERO(d_sv_uni, R); AGENT_ZERO(d_sv_R, R); AGENT_ZERO(d_beta_r, R);
  AGENT_ZERO(d_beta_p0, R); AGENT_ZERO(d_Qs, R); AGENT_ZERO(d_V, env->n_states); AGENT_ZERO(d_span, B); AGENT_ZERO(d_sweeps, B);
  AGENT_ZERO(d_status, B); AGENT_ZERO(d_eS, B); AGENT_ZERO(d_eA, B); AGENT_ZERO(d_e_soff, B); AGENT_ZERO(d_e_roff, B);
  AGENT_ZERO(d_e_rmax, B); AGENT_ZERO(d_e_span, B); AGENT_ZERO(d_e_sweeps, B); AGENT_ZERO(d_e_status, B);
  AGENT_ZERO(d_host, 3 * (size_t)B);
  if (!env->d_uc_unconverged.p) { HIP_TRY(env->d_uc_unconverged.alloc(1)); HIP_TRY(env->d_uc_unconverged.zero(st)); }
  if (int rc = park_alloc(a, seeds)) return rc;
  if (int rc = a->pin_iter.alloc(B)) return rc;
  if (int rc = a->pin_host.alloc(3 * (size_t)B)) return rc;
  a->walk_dst = a->pin_iter.p; a->walk_src = a->d_iteration.p; a->walk_bytes = sizeof(int64_t) * B;
  UcArgs& u = a->args;
  u.row_ptr = a->d_row_ptr.p; u.col = a->d_col.p; u.slot = a->d_slot.p;
  u.N = a->d_N.p; u.N_row = a->d_N_row.p; u.nu = a->d_nu.p; u.kdone = a->d_kdone.p;
  u.val = a->d_val.p; u.uni = a->d_uni.p; u.ER = a->d_ER.p; u.VR = a->d_VR.p; u.HT = a->d_HT.p;
  u.iteration = a->d_iteration.p; u.episode = a->d_episode.p; u.delta = a->d_delta.p;
  u.Q = a->d_Q.p; u.mt = a->d_mt.p; u.mt_pos = a->d_mtpos.p;
  u.tr_row = nullptr; u.tr_rew = nullptr; u.tr_len = a->d_tr_len.p; u.tr_cap = 0;
  u.call = a->call(); u.overflow = a->d_park.p + 1;
  u.sv_val = a->d_sv_val.p; u.sv_uni = a->d_sv_uni.p; u.sv_R = a->d_sv_R.p; u.beta_r = a->d_beta_r.p; u.beta_p0 = a->d_beta_p0.p;
  u.Qs = a->d_Qs.p; u.span = a->d_span.p; u.sweeps = a->d_sweeps.p; u.status = a->d_status.p;
  // before_start_interacting (ucrl2.py:192-193): one episode_end_update without data -- every instance, one solve
  for (int b = 0; b < B; ++b) a->pin_iter.p[b] = 0;
  if (int rc = park_all(a)) return rc;
  if (int rc = ucrl2_round(a, B, 0, 0)) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return agent_attach(guard, out);
}

int cmdp_ucrl2_destroy(cmdp_ucrl2_t* a) { return agent_destroy(a); }

int cmdp_ucrl2_set_option(cmdp_ucrl2_t* a, int option, int64_t value) {
  if (!a || !a->env) return fail(CMDP_ERR_INVALID, "null agent, or its environment handle has been destroyed");
  if (option == CMDP_UCRL2_OPT_MAX_SWEEPS) {
    if (value < 1) return fail(CMDP_ERR_INVALID, "max_sweeps %lld < 1", (long long)value);
    a->max_sweeps = value;
    std::fill(a->p_stamp.begin(), a->p_stamp.end(), -1);   // an option may change what a solve returns: none is reused
    return CMDP_OK;
  }
  if (option == CMDP_UCRL2_OPT_POLICY_SIZE_THRESHOLD) {
    a->policy_size_threshold = value;
    std::fill(a->p_stamp.begin(), a->p_stamp.end(), -1);
    return CMDP_OK;
  }
  if (option == CMDP_UCRL2_OPT_POLICY_REUSE) {
    if (value != 0 && value != 1) return fail(CMDP_ERR_INVALID, "policy_reuse %lld: 0 or 1", (long long)value);
    a->policy_reuse = value != 0;
    return CMDP_OK;
  }
  return fail(CMDP_ERR_INVALID, "unknown option %d", option);
}

int cmdp_ucrl2_run(cmdp_ucrl2_t* a, int64_t n_steps, int stop_at_episode_end, const uint8_t* train_mask, int8_t* actions_trace,
                   int32_t* obs_trace, double* reward_trace, double* cumulative_reward, int64_t* steps_taken) {
  if (int rc = park_run_check(a, n_steps, 0x7fffffffLL, "a transition count of the model (int32, as the reference's N) could wrap: "
                              "instance %d has taken %lld steps, %lld more asked for")) return rc;
  if (int rc = ucrl2_ensure_trace(a, n_steps)) return rc;
  cmdp_t* h = a->env;
  const int stop = stop_at_episode_end ? 1 : 0;
  return park_run(
      a, n_steps, stop, train_mask, actions_trace, obs_trace, reward_trace, cumulative_reward, steps_taken,
      [&](const uint8_t* dmask, int8_t* act, int32_t* obs, double* rew) {
        hipLaunchKernelGGL(k_ucrl2_walk, dim3(grid_for(h->B, 256)), dim3(256), 0, h->stream, h->env(), a->args, n_steps, dmask, act,
                           obs, rew, a->d_rsum.p);
      },
      [&]() -> int {
        if (!a->pin_park.p[1]) return CMDP_OK;
        return fail(CMDP_ERR_OVERFLOW, "an artificial episode outgrew its trace buffer: the bound the buffer is sized from does "
                    "not hold (a defect of the library); the instance's last transition was taken and not counted, destroy the agent");
      },
      [&](int count) { return ucrl2_round(a, count, stop, n_steps); }, &h->uc_wait_ms, &h->uc_round_ms);
}

// discounted_value_iteration(self.P, self.estimated_rewards) (K14) and argmax_2d of its Q for the instances of `mask` whose
// model has changed since their stored solve, through the policy stage: fails when one hit max_sweeps, as the reference
// raises.  Reads nothing but the model and writes nothing of the agent's but the stage.
static int ucrl2_policy_solve(cmdp_ucrl2_t* a, const uint8_t* mask) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const int B = h->B;
  if (h->A > MVI_MAX_ACTIONS)
    return fail(CMDP_ERR_UNSUPPORTED, "%d actions: value iteration on a model (K14) takes at most %d", h->A, MVI_MAX_ACTIONS);
  if (!a->d_pS.p) {
    std::vector<int32_t> S((size_t)B), A((size_t)B, h->A);
    std::vector<int64_t> roff((size_t)B);
    for (int b = 0; b < B; ++b) {
      S[b] = (int32_t)(h->state_off[b + 1] - h->state_off[b]);
      roff[b] = h->state_off[b] * h->A;
    }
    HIP_TRY(a->d_pA.upload(A.data(), B, st));
    HIP_TRY(a->d_p_roff.upload(roff.data(), B, st));
    a->p_stamp.assign((size_t)B, -1);
    a->p_episode.assign((size_t)B, 0);
    HIP_TRY(a->d_pS.upload(S.data(), B, st));
    HIP_TRY(hipStreamSynchronize(st));  // the vectors are locals
  }
  if (int rc = policy_select(a, 1, true, mask)) return rc;
  PolicyStage& p = a->pol;
  HIP_TRY(hipMemcpyAsync(a->p_episode.data(), a->d_episode.p, sizeof(int64_t) * B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (a->policy_reuse)
    p.todo.erase(std::remove_if(p.todo.begin(), p.todo.end(), [&](int32_t b) { return a->p_stamp[(size_t)b] == a->p_episode[(size_t)b]; }),
                 p.todo.end());
  h->uc_policy_solved += (int64_t)p.todo.size();
  h->uc_policy_reused += (int64_t)(p.asked.size() - p.todo.size());
  int rc = policy_stage(a, 1, [&](const int32_t* list, int count) {
    ModelViArgs g{a->d_pS.p, a->d_pA.p, h->d_state_off.p, a->d_p_roff.p, a->d_row_ptr.p, a->d_col.p, a->d_val.p, a->d_uni.p,
                  a->d_ER.p, list, 0.99f, 1e-3, CMDP_SCHEME_AUTO, a->policy_size_threshold, 0.2, 1000000, p.d_Q.p, p.d_V.p,
                  p.d_sweeps.p, p.d_scheme.p, p.d_status.p};
    return mvi_launch(g, count, h->max_S, st);
  });
  if (rc == CMDP_OK) rc = policy_finish(a, &h->uc_policy_ms, "estimated", 1000000);
  if (rc == CMDP_OK || rc == CMDP_ERR_MAX_ITER)   // a solve that hit max_sweeps is never reused: the next request solves (and fails) again
    for (int32_t b : p.todo) a->p_stamp[(size_t)b] = p.status[(size_t)b] == 0 ? a->p_episode[(size_t)b] : -1;
  return rc;
}

int cmdp_ucrl2_policy(cmdp_ucrl2_t* a, const uint8_t* mask, float* pi, float* Q, int64_t* sweeps, int32_t* scheme_used) {
  if (!a || !a->env) return fail(CMDP_ERR_INVALID, "null agent, or its environment handle has been destroyed");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  if (int rc = ucrl2_policy_solve(a, mask)) return rc;
  // the instances of the mask only: what the call leaves of the others is what it found
  if (int rc = policy_fetch(a, pi, a->pol.d_pi.p, h->A, false)) return rc;
  if (int rc = policy_fetch(a, Q, a->pol.d_Q.p, h->A, false)) return rc;
  if (int rc = policy_fetch(a, sweeps, a->pol.d_sweeps.p, 0, false)) return rc;
  if (int rc = policy_fetch(a, scheme_used, a->pol.d_scheme.p, 0, false)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CMDP_OK;
}

int cmdp_ucrl2_average_reward(cmdp_ucrl2_t* a, const uint8_t* mask, double* avg, int32_t* kind) {
  if (!a || !a->env || !avg || !kind) return fail(CMDP_ERR_INVALID, "null argument, or the agent's environment handle has been destroyed");
  if (int rc = bind(a->env)) return rc;
  if (int rc = ucrl2_policy_solve(a, mask)) return rc;
  return chain_launch(a->env, a->pol.d_pi.p, nullptr, a->env->d_cur.p, mask, avg, kind, nullptr);
}

int cmdp_ucrl2_layout(cmdp_ucrl2_t* a, int64_t* n_positions, int64_t* row_ptr, int32_t* col) {
  return park_layout(a, n_positions, row_ptr, col);
}

int cmdp_ucrl2_model(cmdp_ucrl2_t* a, int32_t* N, float* P_val, float* uniform, float* estimated_rewards, float* variance_proxy,
                     float* holding_times, int64_t* iteration, int64_t* episode, double* delta) {
  if (!a) return fail(CMDP_ERR_INVALID, "null agent");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  const int64_t R = h->n_rows;
  AGENT_FETCH(N, d_N, a->nz); AGENT_FETCH(P_val, d_val, a->nz); AGENT_FETCH(uniform, d_uni, R);
  AGENT_FETCH(estimated_rewards, d_ER, R); AGENT_FETCH(variance_proxy, d_VR, R); AGENT_FETCH(holding_times, d_HT, R);
  AGENT_FETCH(iteration, d_iteration, h->B); AGENT_FETCH(episode, d_episode, h->B); AGENT_FETCH(delta, d_delta, h->B);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CMDP_OK;
}

int cmdp_ucrl2_last_solve(cmdp_ucrl2_t* a, float* P_val, float* uniform, float* rewards, double* beta_r, double* beta_p0, float* Q,
                          double* span, int64_t* sweeps, int32_t* status) {
  if (!a) return fail(CMDP_ERR_INVALID, "null agent");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  const int64_t R = h->n_rows;
  AGENT_FETCH(P_val, d_sv_val, a->nz); AGENT_FETCH(uniform, d_sv_uni, R); AGENT_FETCH(rewards, d_sv_R, R);
  AGENT_FETCH(beta_r, d_beta_r, R); AGENT_FETCH(beta_p0, d_beta_p0, R); AGENT_FETCH(Q, d_Q, R);
  AGENT_FETCH(span, d_span, h->B); AGENT_FETCH(sweeps, d_sweeps, h->B); AGENT_FETCH(status, d_status, h->B);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CMDP_OK;
}

}  // extern "C"

// ---- PSRL on the device (K12, cmdp_psrl.h) --------------------------------------------------------------------------
struct cmdp_psrl : ParkAgent {
  int sampler = CMDP_PSRL_SAMPLER_REFERENCE;
  int64_t t_total = 0;
  size_t sample_lds = 0, vi_lds = 0;
  std::vector<int64_t> h_toff, h_ptr;  // [B] padded offsets of the dense T; the layout (reference sampler)
  std::vector<int32_t> h_col;
  std::vector<float> h_prior, h_tp, h_rp, h_T, h_R;
  std::vector<cmdp_rc::NumpyStream> ts, rs;   // [B] RandomState(seed) of M_DIR and of N_NIG (reference sampler)
  PsArgs args{};
  DevBuf<int64_t> d_episode, d_toff, d_roff;
  DevBuf<int32_t> d_S, d_A;
  DevBuf<float> d_tp, d_tprior, d_rp, d_T, d_Rs, d_Q, d_V;
  DevBuf<uint2> d_key;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // around k_psrl_sample and k_vi_episodic_dense of the last round
  bool ev_sample = false, ev_vi = false;
  // the MAP model of the policy solve (K15, K17; the rest is the policy stage's), allocated by the first request
  DevBuf<float> d_mapt, d_mapc, d_mv0;
  size_t map_lds = 0;   // dynamic LDS of a K15 launch on this batch
  ~cmdp_psrl() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

// K12's solver on device-resident arguments: what cmdp_vi_episodic_dense does after its uploads and what the PSRL agent
// does for the instances of a round
int dvi_launch(const DviArgs& g, int count, size_t lds, hipStream_t st) {
  if (int rc = set_lds(k_vi_episodic_dense, lds)) return rc;
  hipLaunchKernelGGL(k_vi_episodic_dense, dim3(count), dim3(PSRL_VI_THREADS), lds, st, g);
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

// K15's launch on device-resident arguments: what cmdp_vi_episodic_map does after its uploads and what the PSRL agent does
// for its MAP policy (cmdp_psrl_policy / cmdp_psrl_evaluate)
int mapvi_launch(MapViArgs g, int count, int max_S, size_t lds, hipStream_t st) {
  if (max_S > MAPVI_MAX_STATES)
    return fail(CMDP_ERR_UNSUPPORTED, "%d states: value iteration on a MAP model (K15) keeps two value layers in LDS for at most %d",
                max_S, MAPVI_MAX_STATES);
  if (count == 0) return CMDP_OK;
  g.lds_bytes = (unsigned)lds;   // the largest map_vi_lds_bytes of the launch's instances
  if (int rc = set_lds(k_vi_episodic_map, lds)) return rc;
  hipLaunchKernelGGL(k_vi_episodic_map, dim3(count), dim3(MAPVI_THREADS), lds, st, g);
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

// episodic_value_iteration(H, *get_map_estimate()) (K15) for the instances of `mask` over the agent's posterior tables, and
// argmax_3d of the first `pi_layers` layers of its Q (0: none), enqueued on the policy stage: the caller enqueues what it
// wants behind it and ends with psrl_policy_finish.  Reads nothing but the model and writes nothing of the agent's but the
// stage and the MAP model's buffers.
int psrl_policy_solve(cmdp_psrl_t* a, const uint8_t* mask, int pi_layers) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const int B = h->B, H = h->H;
  if (!a->d_mapc.p) {
    HIP_TRY(a->d_mapt.alloc((size_t)a->nz));
    HIP_TRY(a->d_mv0.alloc((size_t)h->n_states));
    a->map_lds = 0;
    for (int b = 0; b < B; ++b) {
      const int64_t s0 = h->state_off[b], s1 = h->state_off[b + 1];
      a->map_lds = std::max(a->map_lds, map_vi_lds_bytes((int)(s1 - s0), h->A, a->h_ptr[(size_t)(s1 * h->A)] - a->h_ptr[(size_t)(s0 * h->A)]));
    }
    HIP_TRY(a->d_mapc.alloc((size_t)h->n_rows));
  }
  if (int rc = policy_select(a, H + 1, false, mask)) return rc;
  PolicyStage& p = a->pol;
  return policy_stage(a, pi_layers, [&](const int32_t* list, int count) {
    MapViArgs g{list, a->d_S.p, a->d_A.p, a->d_roff.p, h->d_state_off.p, a->d_row_ptr.p, a->d_col.p, a->d_tp.p, a->d_tprior.p,
                a->d_rp.p, 4, a->d_mapt.p, a->d_mapc.p, p.d_Q.p, p.d_V.p, H, 0};
    return mapvi_launch(g, count, h->max_S, a->map_lds, st);
  });
}

int psrl_policy_finish(cmdp_psrl_t* a) { return policy_finish(a, &a->env->ps_policy_ms, "MAP", 0); }

void psrl_times(cmdp_psrl_t* a) {   // after a stream synchronisation: the last round's kernel times
  float ms = 0.0f;
  if (a->ev_sample && hipEventElapsedTime(&ms, a->ev[0], a->ev[1]) == hipSuccess) a->env->ps_sample_ms = ms;
  if (a->ev_vi && hipEventElapsedTime(&ms, a->ev[2], a->ev[3]) == hipSuccess) a->env->ps_vi_ms = ms;
  (void)hipGetLastError();
}

// The posterior sample of the `count` instances of pin_park's list (already on the device at d_park + 2) into d_T / d_Rs:
// what a round of the episodic and of the continuous agent begins with
int psrl_sample(cmdp_psrl_t* a, int count) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const int A = h->A;
  const int32_t* list = a->d_park.p + 2;
  if (a->sampler == CMDP_PSRL_SAMPLER_PHILOX) {
    const int bpi = grid_for((int64_t)h->max_S * A, PSRL_SAMPLE_THREADS / 64);
    HIP_TRY(hipEventRecord(a->ev[0], st));
    if (int rc = set_lds(k_psrl_sample, a->sample_lds)) return rc;
    hipLaunchKernelGGL(k_psrl_sample, dim3((unsigned)((int64_t)bpi * count)), dim3(PSRL_SAMPLE_THREADS), a->sample_lds, st,
                       a->args, list, h->d_state_off.p, A, h->max_S, bpi);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(a->ev[1], st));
    a->ev_sample = true;
  } else {
    HIP_TRY(hipMemcpyAsync(a->h_tp.data(), a->d_tp.p, sizeof(float) * a->nz, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(a->h_rp.data(), a->d_rp.p, sizeof(float) * 4 * h->n_rows, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t* hl = a->pin_park.p + 2;
    cmdp_rc::Pool::get().parallel_for(count, [&](int k) {   // one stream pair per instance: sequential inside, parallel across
      const int b = hl[k];
      const int64_t soff = h->state_off[b];
      const int S = (int)(h->state_off[b + 1] - soff);
      psrl_host::reference_draw(a->ts[b], a->rs[b], S, A, nullptr, a->h_ptr.data() + soff * A, a->h_col.data(), a->h_tp.data(),
                                a->h_prior[b], a->h_rp.data() + soff * A * 4, a->h_T.data() + a->h_toff[b],
                                a->h_R.data() + soff * A);
    });
    h->ps_ref_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int k = 0; k < count; ++k) {
      const int b = hl[k];
      const int64_t soff = h->state_off[b], S = h->state_off[b + 1] - soff;
      HIP_TRY(hipMemcpyAsync(a->d_T.p + a->h_toff[b], a->h_T.data() + a->h_toff[b], sizeof(float) * S * A * S, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(a->d_Rs.p + soff * A, a->h_R.data() + soff * A, sizeof(float) * S * A, hipMemcpyHostToDevice, st));
    }
  }
  return CMDP_OK;
}

// sample -> solve (straight into the actor's Q) -> reset -> release for the `count` instances of pin_park's list (already on
// the device at d_park + 2)
int psrl_round(cmdp_psrl_t* a, int count, int do_reset, int stop, int64_t n_steps) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const int32_t* list = a->d_park.p + 2;
  if (int rc = psrl_sample(a, count)) return rc;
  DviArgs g{list, a->d_S.p, a->d_A.p, a->d_toff.p, a->d_roff.p, h->d_state_off.p, a->d_T.p, a->d_Rs.p, a->d_Q.p, a->d_V.p, h->H};
  HIP_TRY(hipEventRecord(a->ev[2], st));
  if (int rc = dvi_launch(g, count, a->vi_lds, st)) return rc;
  HIP_TRY(hipEventRecord(a->ev[3], st));
  a->ev_vi = true;
  hipLaunchKernelGGL(k_psrl_resume, dim3(grid_for(count, 256)), dim3(256), 0, st, h->env(), a->args, list, count, do_reset, stop,
                     n_steps);
  HIP_TRY(hipGetLastError());
  h->ps_rounds += 1;
  h->ps_solves += count;
  return CMDP_OK;
}

// What the creates of both PSRL agents (K12 episodic, K13 continuous) refuse of their arguments, up to binding the handle
int psrl_create_check(cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon, const float* reward_prior,
                      const float* transition_prior, int sampler, int actor) {
  if (sampler != CMDP_PSRL_SAMPLER_REFERENCE && sampler != CMDP_PSRL_SAMPLER_PHILOX)
    return fail(CMDP_ERR_INVALID, "sampler %d: CMDP_PSRL_SAMPLER_REFERENCE or CMDP_PSRL_SAMPLER_PHILOX", sampler);
  if (int rc = agent_check_actor(actor)) return rc;
  if (!env || !seeds || !reward_prior || !transition_prior)
    return fail(CMDP_ERR_INVALID, "null argument (environment handle, seeds or priors)");
  if (optimization_horizon < 1) return fail(CMDP_ERR_INVALID, "optimization_horizon < 1");
  return bind(env);
}

// ... and what both build after park_check_env: the priors' checks, the model's layout, the posterior tables, the dense
// workspace of the sample, the actor's Q ([H + 1] layers; continuous: one) and stream, the samplers' state.  a->env and
// a->sampler are set.
int psrl_build(cmdp_psrl_t* a, const int32_t* seeds, const float* reward_prior, const float* transition_prior) {
  cmdp_t* env = a->env;
  const int sampler = a->sampler;
  const int B = env->B, A = env->A, H = env->H;
  const int64_t R = env->n_rows;
  if ((int64_t)env->max_S * A * env->max_S > 0xffffffffLL)
    return fail(CMDP_ERR_UNSUPPORTED, "S * A * S of an instance exceeds 2^32: the Philox counter holds row * S + column in 32 bits");
  for (int b = 0; b < B; ++b) {
    const float* rp = reward_prior + 4 * b;
    if (!(transition_prior[b] > 0.0f) || !std::isfinite(transition_prior[b]))
      return fail(CMDP_ERR_INVALID, "transition_prior[%d] = %g is not a finite value > 0", b, (double)transition_prior[b]);
    if (!std::isfinite(rp[0]) || !(rp[1] > 0.0f) || !(rp[2] > 0.0f) || !(rp[3] > 0.0f) || !std::isfinite(rp[1]) || !std::isfinite(rp[2]) ||
        !std::isfinite(rp[3]))
      return fail(CMDP_ERR_INVALID, "reward_prior[%d]: mu finite, lambda, alpha and beta finite and > 0", b);
  }
  hipStream_t st = env->stream;
  if (int rc = build_model_layout(a, a->h_ptr, a->h_col)) return rc;
  const int64_t NZ = a->nz;
  std::vector<float> tp((size_t)NZ);   // the prior at every position of the instance's rows
  for (int b = 0; b < B; ++b)
    std::fill(tp.begin() + a->h_ptr[(size_t)(env->state_off[b] * A)], tp.begin() + a->h_ptr[(size_t)(env->state_off[b + 1] * A)],
              transition_prior[b]);
  std::vector<int32_t> hS((size_t)B), hA((size_t)B, A);
  std::vector<int64_t> roff((size_t)B);
  std::vector<float> rp((size_t)R * 4);
  std::vector<uint2> keys((size_t)B);
  a->h_toff.assign((size_t)B, 0);
  a->h_prior.assign(transition_prior, transition_prior + B);
  int64_t tt = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t soff = env->state_off[b], S = env->state_off[b + 1] - soff;
    hS[b] = (int32_t)S;
    roff[b] = soff * A;
    a->h_toff[b] = tt;
    tt += (S * A * S + 3) & ~(int64_t)3;   // every instance's T starts on a 16-byte boundary
    for (int64_t r = soff * A; r < (soff + S) * A; ++r) std::memcpy(&rp[(size_t)r * 4], reward_prior + 4 * b, 4 * sizeof(float));
    keys[b] = make_uint2((uint32_t)seeds[b], CMDP_PSRL_KEY_HI);
  }
  a->t_total = tt;
  a->sample_lds = (size_t)(PSRL_SAMPLE_THREADS / 64) * env->max_S * sizeof(float);
  a->vi_lds = dense_vi_lds_bytes(env->max_S);
  if (tt > (int64_t)1 << 40 || a->d_T.alloc((size_t)tt) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CMDP_ERR_OVERFLOW, "the dense workspace of the sampled transition models cannot be allocated: %lld bytes for the "
                "batch (sum of S * A * S float32) -- create smaller batches", (long long)(tt * 4));
  }
  HIP_TRY(a->d_T.zero(st));
  HIP_TRY(a->d_tp.upload(tp.data(), tp.size(), st));
  HIP_TRY(a->d_tprior.upload(transition_prior, B, st));
  HIP_TRY(a->d_rp.upload(rp.data(), rp.size(), st));
  HIP_TRY(a->d_toff.upload(a->h_toff.data(), B, st));
  HIP_TRY(a->d_roff.upload(roff.data(), B, st));
  HIP_TRY(a->d_S.upload(hS.data(), B, st));
  HIP_TRY(a->d_A.upload(hA.data(), B, st));
  HIP_TRY(a->d_key.upload(keys.data(), B, st));
  AGENT_ZERO(d_episode, B); AGENT_ZERO(d_Rs, R); AGENT_ZERO(d_Q, (size_t)(H + 1) * R); AGENT_ZERO(d_V, (size_t)(H + 1) * env->n_states);
  if (int rc = park_alloc(a, seeds)) return rc;
  for (hipEvent_t& e : a->ev) HIP_TRY(hipEventCreate(&e));
  if (sampler == CMDP_PSRL_SAMPLER_REFERENCE) {
    a->ts.resize((size_t)B);
    a->rs.resize((size_t)B);
    for (int b = 0; b < B; ++b) { psrl_host::seed_numpy(a->ts[b], (uint32_t)seeds[b]); psrl_host::seed_numpy(a->rs[b], (uint32_t)seeds[b]); }
    try {
      a->h_tp.resize((size_t)NZ); a->h_rp.resize((size_t)R * 4); a->h_T.resize((size_t)tt); a->h_R.resize((size_t)R);
    } catch (const std::bad_alloc&) {
      return fail(CMDP_ERR_OVERFLOW, "the host staging of the reference sampler's dense models cannot be allocated: %lld bytes "
                  "for the batch -- create smaller batches", (long long)(tt * 4));
    }
  }
  PsArgs& p = a->args;
  p.row_ptr = a->d_row_ptr.p; p.col = a->d_col.p; p.slot = a->d_slot.p;
  p.tp = a->d_tp.p; p.tprior = a->d_tprior.p; p.rp = a->d_rp.p; p.episode = a->d_episode.p; p.key = a->d_key.p;
  p.t_off = a->d_toff.p; p.T = a->d_T.p; p.Rs = a->d_Rs.p; p.Q = a->d_Q.p; p.V = a->d_V.p;
  p.mt = a->d_mt.p; p.mt_pos = a->d_mtpos.p;
  p.call = a->call();
  return CMDP_OK;
}

}  // namespace

extern "C" {

int cmdp_psrl_create(cmdp_psrl_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon,
                     const float* reward_prior, const float* transition_prior, int sampler, int actor) {
  if (!out) return fail(CMDP_ERR_INVALID, "null output");
  *out = nullptr;
  if (int rc = psrl_create_check(env, seeds, optimization_horizon, reward_prior, transition_prior, sampler, actor)) return rc;
  if (int rc = park_check_env(env, true, "PSRLEpisodic is the episodic setting's agent: the environment handle is continuous "
                              "(cmdp_psrlc_create builds PSRLContinuous with plain posterior sampling)", "PSRL",
                              "the dense solver (K12)", PSRL_MAX_STATES)) return rc;
  cmdp_psrl_t* a = new cmdp_psrl;
  std::unique_ptr<cmdp_psrl> guard(a);
  a->env = env;
  a->sampler = sampler;
  if (int rc = psrl_build(a, seeds, reward_prior, transition_prior)) return rc;
  // before_start_interacting (posterior_sampling.py:146-147): one episode_end_update on the prior -- every instance
  if (int rc = park_all(a)) return rc;
  if (int rc = psrl_round(a, env->B, 0, 0, 0)) return rc;
  HIP_TRY(hipStreamSynchronize(env->stream));
  psrl_times(a);
  return agent_attach(guard, out);
}

int cmdp_psrl_destroy(cmdp_psrl_t* a) { return agent_destroy(a); }

int cmdp_psrl_run(cmdp_psrl_t* a, int64_t n_steps, int stop_at_episode_end, const uint8_t* train_mask, int8_t* actions_trace,
                  int32_t* obs_trace, double* reward_trace, double* cumulative_reward, int64_t* steps_taken) {
  if (int rc = park_run_check(a, n_steps, 1LL << 24, "a transition count of the model (float32, as the reference's "
                              "hyper-parameters) would stop counting at 2^24: instance %d has taken %lld steps, %lld more asked for"))
    return rc;
  cmdp_t* h = a->env;
  const int stop = stop_at_episode_end ? 1 : 0;
  const int rc = park_run(
      a, n_steps, stop, train_mask, actions_trace, obs_trace, reward_trace, cumulative_reward, steps_taken,
      [&](const uint8_t* dmask, int8_t* act, int32_t* obs, double* rew) {
        hipLaunchKernelGGL(k_psrl_walk, dim3(grid_for(h->B, 256)), dim3(256), 0, h->stream, h->env(), a->args, n_steps, dmask, act,
                           obs, rew, a->d_rsum.p);
      },
      [&]() -> int { psrl_times(a); return CMDP_OK; }, [&](int count) { return psrl_round(a, count, 1, stop, n_steps); });
  psrl_times(a);   // after the call's last synchronisation
  return rc;
}

int cmdp_psrl_episode_end_update(cmdp_psrl_t* a) {
  if (!a) return fail(CMDP_ERR_INVALID, "null agent");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  if (int rc = park_all(a)) return rc;
  if (int rc = psrl_round(a, h->B, 0, 0, 0)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  psrl_times(a);
  return CMDP_OK;
}

int cmdp_psrl_layout(cmdp_psrl_t* a, int64_t* n_positions, int64_t* row_ptr, int32_t* col) {
  return park_layout(a, n_positions, row_ptr, col);
}

int cmdp_psrl_model(cmdp_psrl_t* a, float* reward_hp, float* transition_hp, float* transition_prior, int64_t* episodes) {
  if (!a) return fail(CMDP_ERR_INVALID, "null agent");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  AGENT_FETCH(reward_hp, d_rp, 4 * h->n_rows); AGENT_FETCH(transition_hp, d_tp, a->nz); AGENT_FETCH(episodes, d_episode, h->B);
  if (transition_prior) std::memcpy(transition_prior, a->h_prior.data(), sizeof(float) * h->B);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CMDP_OK;
}

int cmdp_psrl_last_sample(cmdp_psrl_t* a, float* T, float* R, float* Q) {
  if (!a) return fail(CMDP_ERR_INVALID, "null agent");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  hipStream_t st = h->stream;
  if (T) {
    int64_t o = 0;
    for (int b = 0; b < h->B; ++b) {   // the workspace pads every instance to 16 bytes; the caller's array is dense
      const int64_t S = h->state_off[b + 1] - h->state_off[b], n = S * h->A * S;
      HIP_TRY(hipMemcpyAsync(T + o, a->d_T.p + a->h_toff[b], sizeof(float) * n, hipMemcpyDeviceToHost, st));
      o += n;
    }
  }
  AGENT_FETCH(R, d_Rs, h->n_rows); AGENT_FETCH(Q, d_Q, (h->H + 1) * h->n_rows);
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

int cmdp_psrl_reference_sample(uint32_t* t_key, int32_t* t_pos, int32_t* t_has_gauss, double* t_gauss, uint32_t* r_key,
                               int32_t* r_pos, int32_t* r_has_gauss, double* r_gauss, int n_states, int n_actions,
                               const float* transition_hp_dense, const int64_t* row_ptr, const int32_t* col, const float* val,
                               float prior, const float* reward_hp, float* T, float* R) {
  if (!t_key || !t_pos || !t_has_gauss || !t_gauss || !r_key || !r_pos || !r_has_gauss || !r_gauss || !reward_hp || !T || !R)
    return fail(CMDP_ERR_INVALID, "null argument");
  if (n_states < 1 || n_actions < 1) return fail(CMDP_ERR_INVALID, "n_states and n_actions must be >= 1");
  if (!transition_hp_dense && (!row_ptr || !col || !val || !(prior > 0.0f)))
    return fail(CMDP_ERR_INVALID, "transition hyper-parameters: a dense array, or a layout (row_ptr, col, val) and a prior > 0");
  if (*t_pos < 0 || *t_pos > 624 || *r_pos < 0 || *r_pos > 624) return fail(CMDP_ERR_INVALID, "MT19937 position outside [0, 624]");
  const int64_t SA = (int64_t)n_states * n_actions;
  if (transition_hp_dense) {
    for (int64_t i = 0; i < SA * n_states; ++i)
      if (!(transition_hp_dense[i] >= 0.0f)) return fail(CMDP_ERR_INVALID, "transition hyper-parameter %lld is negative or NaN", (long long)i);
  } else {
    for (int64_t r = 0; r < SA; ++r) {
      if (row_ptr[r + 1] < row_ptr[r]) return fail(CMDP_ERR_INVALID, "row_ptr decreases at row %lld", (long long)r);
      for (int64_t z = row_ptr[r]; z < row_ptr[r + 1]; ++z)
        if (col[z] < 0 || col[z] >= n_states || (z > row_ptr[r] && col[z] <= col[z - 1]) || !(val[z] >= 0.0f))
          return fail(CMDP_ERR_INVALID, "row %lld of the layout: columns ascending within [0, %d), values >= 0", (long long)r, n_states);
    }
  }
  for (int64_t r = 0; r < SA; ++r)
    if (!(reward_hp[4 * r + 1] > 0.0f) || !(reward_hp[4 * r + 2] > 0.0f) || !(reward_hp[4 * r + 3] > 0.0f))
      return fail(CMDP_ERR_INVALID, "reward hyper-parameters of row %lld: lambda, alpha and beta must be > 0", (long long)r);
  cmdp_rc::NumpyStream ts, rs;
  std::memcpy(ts.key, t_key, sizeof ts.key);
  ts.pos = *t_pos; ts.has_gauss = *t_has_gauss; ts.gauss = *t_gauss;
  std::memcpy(rs.key, r_key, sizeof rs.key);
  rs.pos = *r_pos; rs.has_gauss = *r_has_gauss; rs.gauss = *r_gauss;
  psrl_host::reference_draw(ts, rs, n_states, n_actions, transition_hp_dense, row_ptr, col, val, prior, reward_hp, T, R);
  std::memcpy(t_key, ts.key, sizeof ts.key);
  *t_pos = ts.pos; *t_has_gauss = ts.has_gauss; *t_gauss = ts.gauss;
  std::memcpy(r_key, rs.key, sizeof rs.key);
  *r_pos = rs.pos; *r_has_gauss = rs.has_gauss; *r_gauss = rs.gauss;
  return CMDP_OK;
}

int cmdp_vi_episodic_dense(int count, const int32_t* n_states, const int32_t* n_actions, int H, const float* T, const float* R,
                           float* Q, float* V) {
  if (count < 0) return fail(CMDP_ERR_INVALID, "count %d is negative", count);
  if (count == 0) return CMDP_OK;
  if (!n_states || !n_actions || !T || !R || !Q || !V) return fail(CMDP_ERR_INVALID, "null argument");
  if (H < 1) return fail(CMDP_ERR_INVALID, "H %d < 1", H);
  BatchLayout L;
  if (int rc = L.build(count, n_states, n_actions,
                       {PSRL_MAX_STATES, "instance %d has %d states: the dense episodic solver keeps two value layers in LDS for at "
                                         "most %d states"}))
    return rc;
  const int64_t ns = L.ns, nr = L.nr;
  std::vector<int64_t> toff((size_t)count), tsrc((size_t)count);   // T[S, A, S] of an instance: padded on the device, packed in T
  int64_t nt = 0, nsrc = 0;
  for (int b = 0; b < count; ++b) {
    toff[b] = nt; tsrc[b] = nsrc;
    nsrc += L.rows(b) * n_states[b];
    nt += (L.rows(b) * n_states[b] + 3) & ~(int64_t)3;
  }
  struct Ws {
    DevBuf<int32_t> S, A;
    DevBuf<int64_t> soff, roff, toff;
    DevBuf<float> T, R, Q, V;
  };
  DeviceWorkspace<Ws> ws;
  if (int rc = ws.acquire()) return rc;
  hipStream_t st = ws.st;
  HIP_TRY(ws->S.upload(n_states, count, st));
  HIP_TRY(ws->A.upload(n_actions, count, st));
  HIP_TRY(ws->soff.upload(L.soff.data(), L.soff.size(), st));
  HIP_TRY(ws->roff.upload(L.roff.data(), count, st));
  HIP_TRY(ws->toff.upload(toff.data(), count, st));
  if (ws->T.alloc((size_t)nt) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CMDP_ERR_OVERFLOW, "the dense transition models cannot be held on the device: %lld bytes", (long long)(nt * 4));
  }
  for (int b = 0; b < count; ++b)
    HIP_TRY(hipMemcpyAsync(ws->T.p + toff[b], T + tsrc[b], sizeof(float) * (size_t)(L.rows(b) * n_states[b]), hipMemcpyHostToDevice, st));
  HIP_TRY(ws->R.upload(R, (size_t)nr, st));
  HIP_TRY(ws->Q.alloc((size_t)(H + 1) * nr));
  HIP_TRY(ws->V.alloc((size_t)(H + 1) * ns));
  DviArgs g{nullptr, ws->S.p, ws->A.p, ws->toff.p, ws->roff.p, ws->soff.p, ws->T.p, ws->R.p, ws->Q.p, ws->V.p, H};
  if (int rc = dvi_launch(g, count, dense_vi_lds_bytes(L.max_S), st)) return rc;
  HIP_TRY(ws->Q.download(Q, (size_t)(H + 1) * nr, st));
  HIP_TRY(ws->V.download(V, (size_t)(H + 1) * ns, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

// ---- the MAP model's solve (K15, cmdp_map_vi.h) -----------------------------------------------------------------------
static int map_check_layout(int b, int64_t S, int64_t A, const int64_t* row_ptr, const int32_t* col, const float* hp, float prior) {
  if (!(prior > 0.0f) || !std::isfinite(prior)) return fail(CMDP_ERR_INVALID, "prior[%d] = %g is not a finite value > 0", b, (double)prior);
  for (int64_t r = 0; r < S * A; ++r) {
    if (row_ptr[r + 1] < row_ptr[r]) return fail(CMDP_ERR_INVALID, "instance %d: row_ptr decreases at row %lld", b, (long long)r);
    for (int64_t z = row_ptr[r]; z < row_ptr[r + 1]; ++z)
      if (col[z] < 0 || col[z] >= S || (z > row_ptr[r] && col[z] <= col[z - 1]) || !(hp[z] >= 0.0f) || !std::isfinite(hp[z]))
        return fail(CMDP_ERR_INVALID, "instance %d, row %lld of the layout: columns ascending within [0, %d), values finite and >= 0",
                    b, (long long)r, (int)S);
  }
  return CMDP_OK;
}

int cmdp_psrl_map_rows(int n_states, int n_actions, const int64_t* row_ptr, const int32_t* col, const float* hp, float prior,
                       float* rowsum, float* c, float* t) {
  if (n_states < 1 || n_actions < 1) return fail(CMDP_ERR_INVALID, "n_states and n_actions must be >= 1");
  if (!row_ptr || (row_ptr[(int64_t)n_states * n_actions] > row_ptr[0] && (!col || !hp))) return fail(CMDP_ERR_INVALID, "null argument");
  if (int rc = map_check_layout(0, n_states, n_actions, row_ptr, col, hp, prior)) return rc;
  map_vi_host::map_rows(n_states, n_actions, row_ptr, col, hp, prior, psrl_host::pairwise_sum_f32, rowsum, c, t);
  return CMDP_OK;
}

int cmdp_vi_episodic_map(int count, const int32_t* n_states, const int32_t* n_actions, int H, const int64_t* row_ptr,
                         const int32_t* col, const float* hp, const float* prior, const float* mu, float* Q, float* V,
                         float* t_layout_out, float* c_out) {
  if (count < 0) return fail(CMDP_ERR_INVALID, "count %d is negative", count);
  if (count == 0) return CMDP_OK;
  if (!n_states || !n_actions || !row_ptr || !prior || !mu || !Q || !V) return fail(CMDP_ERR_INVALID, "null argument");
  if (H < 1) return fail(CMDP_ERR_INVALID, "H %d < 1", H);
  BatchLayout L;
  if (int rc = L.build(count, n_states, n_actions,
                       {MAPVI_MAX_STATES, "instance %d has %d states: value iteration on a MAP model (K15) keeps two value layers in "
                                          "LDS for at most %d states"}))
    return rc;
  const int64_t ns = L.ns, nr = L.nr;
  if (row_ptr[0] != 0) return fail(CMDP_ERR_INVALID, "row_ptr[0] = %lld, not 0", (long long)row_ptr[0]);
  const int64_t nz = row_ptr[nr];
  if (nz > 0 && (!col || !hp)) return fail(CMDP_ERR_INVALID, "null argument");
  size_t lds = 0;
  for (int b = 0; b < count; ++b) {
    const int64_t* ptr = row_ptr + L.roff[b];
    if (int rc = map_check_layout(b, n_states[b], n_actions[b], ptr, col, hp, prior[b])) return rc;
    lds = std::max(lds, map_vi_lds_bytes(n_states[b], n_actions[b], ptr[L.rows(b)] - ptr[0]));
  }
  struct Ws {
    DevBuf<int32_t> S, A, col;
    DevBuf<int64_t> soff, roff, ptr;
    DevBuf<float> hp, prior, mu, t, c, Q, V;
  };
  DeviceWorkspace<Ws> ws;
  if (int rc = ws.acquire()) return rc;
  hipStream_t st = ws.st;
  HIP_TRY(ws->S.upload(n_states, count, st));
  HIP_TRY(ws->A.upload(n_actions, count, st));
  HIP_TRY(ws->soff.upload(L.soff.data(), L.soff.size(), st));
  HIP_TRY(ws->roff.upload(L.roff.data(), count, st));
  HIP_TRY(ws->ptr.upload(row_ptr, (size_t)nr + 1, st));
  HIP_TRY(ws->col.upload(col, (size_t)nz, st));
  HIP_TRY(ws->hp.upload(hp, (size_t)nz, st));
  HIP_TRY(ws->prior.upload(prior, count, st));
  HIP_TRY(ws->mu.upload(mu, (size_t)nr, st));
  HIP_TRY(ws->t.alloc((size_t)nz));
  HIP_TRY(ws->c.alloc((size_t)nr));
  HIP_TRY(ws->Q.alloc((size_t)(H + 1) * nr));
  HIP_TRY(ws->V.alloc((size_t)(H + 1) * ns));
  MapViArgs g{nullptr, ws->S.p, ws->A.p, ws->roff.p, ws->soff.p, ws->ptr.p, ws->col.p, ws->hp.p, ws->prior.p, ws->mu.p, 1,
              ws->t.p, ws->c.p, ws->Q.p, ws->V.p, H, 0};
  if (int rc = mapvi_launch(g, count, L.max_S, lds, st)) return rc;
  HIP_TRY(ws->Q.download(Q, (size_t)(H + 1) * nr, st));
  HIP_TRY(ws->V.download(V, (size_t)(H + 1) * ns, st));
  if (t_layout_out) HIP_TRY(ws->t.download(t_layout_out, (size_t)nz, st));
  if (c_out) HIP_TRY(ws->c.download(c_out, (size_t)nr, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

int cmdp_psrl_policy(cmdp_psrl_t* a, const uint8_t* mask, float* pi, float* Q) {
  if (!a || !a->env) return fail(CMDP_ERR_INVALID, "null agent, or its environment handle has been destroyed");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  // get_policy_from_q_values(Q, True) = argmax_3d over all H + 1 layers (posterior_sampling.py:82)
  if (int rc = psrl_policy_solve(a, mask, pi ? h->H + 1 : 0)) return rc;
  const int64_t per_state = (int64_t)(h->H + 1) * h->A;
  if (int rc = policy_fetch(a, pi, a->pol.d_pi.p, per_state, true)) return rc;
  if (int rc = policy_fetch(a, Q, a->pol.d_Q.p, per_state, true)) return rc;
  return psrl_policy_finish(a);
}

}  // extern "C"

// What the evaluation of the MAP policy on the true MDP refuses (after bind)
static int psrl_evaluate_check(cmdp_t* h) {
  return episodic_value_check(h, CMDP_ERR_UNSUPPORTED, "cmdp_psrl_evaluate evaluates the policy on the true MDP: the environment "
                              "handle was created without the DP half (CSR transition matrices)");
}

// K15 -> greedy policy of the first H layers (the same draws of argmax_3d's tie-break stream, laid out as the evaluation reads
// them) -> its value on the true MDP: V[0, :] packed into `v0` (device-accessible; null: a->d_mv0), `snap` as
// enqueue_episodic_value's.  All enqueued: the caller ends with psrl_policy_finish.
static int psrl_enqueue_evaluate(cmdp_psrl_t* a, const uint8_t* mask, float* v0, int32_t* snap) {
  if (int rc = psrl_evaluate_check(a->env)) return rc;
  if (int rc = psrl_policy_solve(a, mask, a->env->H)) return rc;
  return enqueue_episodic_value(a->env, a->pol.d_pi.p, v0 ? v0 : a->d_mv0.p, snap);
}

extern "C" {

int cmdp_psrl_evaluate(cmdp_psrl_t* a, const uint8_t* mask, float* V0) {
  if (!a || !a->env || !V0) return fail(CMDP_ERR_INVALID, "null argument, or the agent's environment handle has been destroyed");
  if (int rc = bind(a->env)) return rc;
  if (int rc = psrl_enqueue_evaluate(a, mask, nullptr, nullptr)) return rc;
  if (int rc = policy_fetch(a, V0, a->d_mv0.p, 1, true)) return rc;
  return psrl_policy_finish(a);
}

}  // extern "C"

// ---- PSRL for the continuous setting, plain posterior sampling (K13, cmdp_psrlc.h) ---------------------------------------
// The posterior tables, the samplers and their state are the episodic agent's (psrl_build, psrl_sample); H = 0 here, so its Q
// and V are the one layer [S][A] / [S] the actor and the solver share.
struct cmdp_psrlc : cmdp_psrl {
  int64_t size_threshold = 300 * 3 * 300;   // the reference's defaults (infinite_horizon.py:20-21)
  double density_threshold = 0.2;
  int64_t max_sweeps = 1000000;             // DP_MAX_ITERATION of the reference
  int policy_solver = 0;                    // CMDP_PSRLC_OPT_POLICY_SOLVER: 0 the dense route, 1 the tables route (K17)
  PcCounters cnt{};
  DevBuf<int32_t> d_nsa, d_nu, d_stamp, d_scheme, d_status;
  DevBuf<int64_t> d_sweeps;
  // the dense route of the MAP-policy solve alone, allocated by its first request: the dense MAP model.  The tables route
  // keeps T_map in d_mapt [NZ] and d_mapc [R] of the base instead.
  DevBuf<float> d_Tmap, d_Rmap, d_mrs;
  bool optimistic = false;                  // the handle is a cmdp_psrlo (K18): its round, walk and destroy are dispatched on it
  // CMDP_PSRLC_OPT_MIN_STEPS: the reference's min_steps_before_new_episode.  0 runs the walks compiled without the gate;
  // d_lastchg [B] exists from the first value > 0
  int32_t min_steps = 0;
  DevBuf<int32_t> d_lastchg;
};

// ---- ... with optimistic sampling (K18, cmdp_psrlo.h): the extended sample, the extended Q of the actor, the agent's N ------
struct cmdp_psrlo : cmdp_psrlc {
  std::vector<int32_t> h_psi;
  std::vector<double> h_eta;
  std::vector<int64_t> h_qoff, h_txoff, h_koff, h_pmoff;   // [B] offsets of the extended arrays (cmdp_psrlo.h: PoArgs)
  int64_t q_total = 0, tx_total = 0, k_total = 0;
  PoArgs po{};
  DevBuf<int32_t> d_psi, d_N, d_z, d_pidx, d_n1, d_Ax;
  DevBuf<double> d_eta, d_log4s, d_pm;
  DevBuf<int64_t> d_qoff, d_txoff, d_koff, d_pmoff;
  DevBuf<float> d_pmk, d_bump, d_Tx, d_Rx, d_Qx, d_post;
  DevBuf<uint8_t> d_simple;
  // reference sampler: the agent's own RandomState(seed) and the host staging of a round's draws
  std::vector<cmdp_rc::NumpyStream> as;
  std::vector<int32_t> h_nsa, h_z, h_pidx, h_n1;
  std::vector<uint8_t> h_simple;
  std::vector<float> h_post;
  // the sample routes (CMDP_PSRLC_OPT_SAMPLE_SOLVER): 0 dense (d_Tx, d_post, h_post), 1 compact (K19, cmdp_psrlo_vi.h).  A
  // route's arrays exist from the first round that takes it; an instance's last sample stays in the form of its round.
  int sample_solver = 0;
  bool has_dense = false, has_compact = false;
  std::vector<uint8_t> h_route;            // [B] the route of the instance's last sample; 2: none (psrlo_grow failed)
  std::vector<DevBuf<float>> pk;           // [B] compact: the posterior rows [psi][n1][S] of the last draw, grown on demand
  std::vector<float*> h_pkptr;             // [B] their addresses, and on the device
  DevBuf<float*> d_pkptr;
  std::vector<std::vector<float>> h_pk;    // [B] reference sampler: the host staging of the same rows
  DevBuf<float> d_stage;                   // one instance's expansion, for cmdp_psrlc_last_sample_optimistic
};

namespace {

// Host-only picker of k_vi_discounted_dense's form: how many wavefronts share an instance.  The results do not depend on it
// (cmdp_psrlc.h); CMDP_DDV_WAVES=1 forces the single wavefront for measurements.
int ddv_waves() {
  const char* e = std::getenv("CMDP_DDV_WAVES");
  return e && e[0] == '1' && e[1] == '\0' ? 1 : DDV_MAX_WAVES;
}

// K13's solver on device-resident arguments: what cmdp_vi_discounted_dense does after its uploads and what the continuous
// PSRL agent does for the instances of a round
int ddv_launch(const DdvArgs& g, int count, int max_S, hipStream_t st) {
  if (count == 0) return CMDP_OK;
  const size_t lds = ddv_lds_bytes(max_S);
  if (ddv_waves() == 1) {
    if (int rc = set_lds(k_vi_discounted_dense<1>, lds)) return rc;
    hipLaunchKernelGGL(k_vi_discounted_dense<1>, dim3(count), dim3(64), lds, st, g);
  } else {
    if (int rc = set_lds(k_vi_discounted_dense<DDV_MAX_WAVES>, lds)) return rc;
    hipLaunchKernelGGL(k_vi_discounted_dense<DDV_MAX_WAVES>, dim3(count), dim3(DDV_MAX_WAVES * 64), lds, st, g);
  }
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

// PSRLContinuous calls discounted_value_iteration(T, R) with nothing else (posterior_sampling.py:177, :374): the defaults of
// colosseum/dynamic_programming/infinite_horizon.py:17-18
constexpr float PSRLC_GAMMA = 0.99f;
constexpr double PSRLC_EPSILON = 1e-3;

// K13's solver as the agent calls it, for a round's sample and for the dense MAP model alike: the handle's plain layout, the
// reference's gamma and epsilon, the scheme by the rule at the handle's thresholds
DdvArgs psrlc_ddv_args(const cmdp_psrlc* a, const int32_t* list, const float* T, const float* R, float* Q, float* V, int64_t* sweeps,
                       int32_t* scheme, int32_t* status) {
  return DdvArgs{list, a->d_S.p, a->d_A.p, a->d_toff.p, a->d_roff.p, a->env->d_state_off.p, T, R, PSRLC_GAMMA, PSRLC_EPSILON,
                 CMDP_SCHEME_AUTO, a->size_threshold, a->density_threshold, a->max_sweeps, Q, V, sweeps, scheme, status};
}

// Host-only picker of k_vi_discounted_map's form and launch geometry (one wavefront per instance, `count` workgroups).  An
// instance may keep its tables in LDS next to its value arrays when they take at most MAPDVI_STAGE_MAX_BYTES (two such
// workgroups share a CU's 160 KB); `staged` is the launch's dynamic LDS in that form, `plain` with every instance's tables
// left in global memory.  The staged form is taken when all its workgroups are resident at once: a launch that would need
// a second round of workgroups keeps the tables in global memory, where the CU holds every instance of the launch.  The
// results do not depend on the form (cmdp_map_dvi.h); CMDP_MAPDVI_STAGE=0 / 1 forces one of them, for measurements.
constexpr size_t MAPDVI_STAGE_MAX_BYTES = (size_t)80 * 1024;
size_t mapdvi_pick_lds(int count, int cus, size_t staged, size_t plain) {
  const char* e = std::getenv("CMDP_MAPDVI_STAGE");
  if (e && (e[0] == '0' || e[0] == '1') && e[1] == '\0') return e[0] == '1' ? staged : plain;
  const size_t per_cu = (size_t)kLdsBudget / std::max<size_t>(staged, 1);
  return (size_t)count <= (size_t)std::max(cus, 1) * per_cu ? staged : plain;
}

// K17's launch on device-resident arguments: what cmdp_vi_discounted_map does after its uploads and what the continuous PSRL
// agent does for its MAP policy on the tables route.  One wavefront per instance; `lds` is the largest map_dvi_lds_bytes of
// the launch's instances.
int mapdvi_launch(MapDviArgs g, int count, int max_S, size_t lds, hipStream_t st) {
  if (max_S > MAPVI_MAX_STATES)
    return fail(CMDP_ERR_UNSUPPORTED, "%d states: value iteration on a MAP model (K17) keeps V and V_old in LDS for at most %d",
                max_S, MAPVI_MAX_STATES);
  if (count == 0) return CMDP_OK;
  g.lds_bytes = (unsigned)lds;
  if (int rc = set_lds(k_vi_discounted_map, lds)) return rc;
  hipLaunchKernelGGL(k_vi_discounted_map, dim3(count), dim3(MAPDVI_THREADS), lds, st, g);
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

// What the sample routes of an optimistic agent hold on the device (CMDP_STAT_PSRL_SAMPLE_BYTES): pmk and bump, which both
// routes fill; T_ext and the reference sampler's upload of the dense route; the posterior blocks and their address table of
// the compact one
void psrlo_account(cmdp_psrlo* a) {
  size_t n = 4 * (a->d_pmk.cap + a->d_bump.cap + a->d_Tx.cap + a->d_post.cap) + sizeof(float*) * a->d_pkptr.cap;
  for (const DevBuf<float>& d : a->pk) n += 4 * d.cap;
  a->env->ps_sample_bytes = (double)n;
}

// The arrays of sample route `route`, at the first round that takes it.  CMDP_ERR_OVERFLOW when the dense route's do not fit.
int psrlo_ensure_route(cmdp_psrlo* a, int route) {
  cmdp_t* h = a->env;
  const bool reference = a->sampler == CMDP_PSRL_SAMPLER_REFERENCE;
  if (route == 0 && !a->has_dense) {
    const long long need = (long long)a->tx_total * (reference ? 2 : 1) * 4;
    if (a->d_Tx.alloc((size_t)a->tx_total) != hipSuccess || (reference && a->d_post.alloc((size_t)a->tx_total) != hipSuccess)) {
      (void)hipGetLastError();
      a->d_Tx.release(); a->d_post.release();
      return fail(CMDP_ERR_OVERFLOW, "the extended samples of the batch cannot be allocated: %lld bytes", need);
    }
    HIP_TRY(a->d_Tx.zero(h->stream));
    if (reference) {
      try {
        a->h_post.resize((size_t)a->tx_total);
      } catch (const std::bad_alloc&) {
        a->d_Tx.release(); a->d_post.release();
        return fail(CMDP_ERR_OVERFLOW, "the host staging of the reference sampler's posterior rows cannot be allocated: %lld bytes",
                    (long long)a->tx_total * 4);
      }
    }
    a->po.post = a->d_post.p;
    a->po.Tx = a->d_Tx.p;
    a->has_dense = true;
  }
  if (route == 1 && !a->has_compact) {
    a->pk = std::vector<DevBuf<float>>((size_t)h->B);
    a->h_pkptr.assign((size_t)h->B, nullptr);
    a->h_pk.resize((size_t)h->B);
    HIP_TRY(a->d_pkptr.upload(a->h_pkptr.data(), (size_t)h->B, h->stream));
    a->has_compact = true;
  }
  psrlo_account(a);
  return CMDP_OK;
}

// The compact route's block of instance b for n1 posterior rows: psi * n1 * S floats.  It only grows, to
// max(need, min(2 * capacity, psi * S * A * S)) floats (to `need` alone when that much cannot be had) -- never to the worst
// case ahead of need, which is T_ext itself.
int psrlo_grow(cmdp_psrlo* a, int b, int n1, bool* moved) {
  cmdp_t* h = a->env;
  const size_t S = (size_t)(h->state_off[b + 1] - h->state_off[b]), psi = (size_t)a->h_psi[b];
  const size_t need = psi * (size_t)n1 * S, worst = psi * S * (size_t)h->A * S;
  DevBuf<float>& d = a->pk[(size_t)b];
  if (need <= d.cap) return CMDP_OK;
  // the new block is allocated before the old one is given up, first at the growth step and then at the need alone.  When
  // neither fits the round fails; the row numbering of the new draw may already be on the device, so the instance counts as
  // holding no sample (route 2) until a later round draws one
  const size_t want = std::max(need, std::min(2 * d.cap, worst));
  DevBuf<float> fresh;
  if (fresh.alloc(want) != hipSuccess) {
    (void)hipGetLastError();
    if (want == need || fresh.alloc(need) != hipSuccess) {
      (void)hipGetLastError();
      a->h_route[(size_t)b] = 2;
      return fail(CMDP_ERR_OVERFLOW, "the %d posterior rows of instance %d's optimistic sample cannot be held on the device: %zu "
                  "bytes", n1, b, need * 4);
    }
  }
  d.swap(fresh);   // `fresh` now holds the old block and frees it
  a->h_pkptr[(size_t)b] = d.p;
  *moved = true;
  return CMDP_OK;
}

// The reference sampler's half of an optimistic sample: the host draws each listed instance's posterior rows, z and rewards
// (psrlo_host::draw) and uploads them compactly -- on the dense route into d_post at the instance's T_ext offset, on the
// compact route into the instance's own block, sized to this draw's posterior rows
int psrlo_reference_draws(cmdp_psrlo* a, int count, bool compact) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const int A = h->A;
  HIP_TRY(hipMemcpyAsync(a->h_tp.data(), a->d_tp.p, sizeof(float) * a->nz, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(a->h_rp.data(), a->d_rp.p, sizeof(float) * 4 * h->n_rows, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(a->h_nsa.data(), a->d_nsa.p, sizeof(int32_t) * h->n_rows, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int32_t* hl = a->pin_park.p + 2;
  if (compact) {
    bool moved = false;
    int rc = CMDP_OK;
    for (int k = 0; k < count && !rc; ++k) {
      const int b = hl[k];
      const int64_t r0 = h->state_off[b] * A, S = h->state_off[b + 1] - h->state_off[b];
      int n1 = 0;
      for (int64_t r = r0; r < r0 + S * A; ++r) n1 += !((double)a->h_nsa[(size_t)r] < a->h_eta[b]);
      rc = psrlo_grow(a, b, n1, &moved);
      if (!rc) {
        try {
          a->h_pk[(size_t)b].resize((size_t)a->h_psi[b] * n1 * S);
        } catch (const std::bad_alloc&) {
          rc = fail(CMDP_ERR_OVERFLOW, "the host staging of instance %d's posterior rows cannot be allocated: %lld bytes", b,
                    (long long)a->h_psi[b] * n1 * S * 4);
        }
      }
    }
    if (moved) HIP_TRY(a->d_pkptr.upload(a->h_pkptr.data(), (size_t)h->B, st));
    if (rc) return rc;
  }
  const auto t0 = std::chrono::steady_clock::now();
  cmdp_rc::Pool::get().parallel_for(count, [&](int k) {
    const int b = hl[k];
    const int64_t r0 = h->state_off[b] * A;
    const int S = (int)(h->state_off[b + 1] - h->state_off[b]);
    a->h_n1[b] = psrlo_host::draw(a->ts[b], a->rs[b], a->as[b], S, A, a->h_psi[b], a->h_eta[b], a->h_nsa.data() + r0,
                                  a->h_ptr.data() + r0, a->h_col.data(), a->h_tp.data(), a->h_prior[b], a->h_rp.data() + r0 * 4,
                                  a->h_simple.data() + r0, a->h_pidx.data() + r0,
                                  compact ? a->h_pk[(size_t)b].data() : a->h_post.data() + a->h_txoff[b],
                                  a->h_z.data() + a->h_koff[b], a->h_R.data() + r0);
  });
  h->ps_ref_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (int k = 0; k < count; ++k) {
    const int b = hl[k];
    const int64_t r0 = h->state_off[b] * A, S = h->state_off[b + 1] - h->state_off[b], rows = S * A;
    const int64_t np = (int64_t)a->h_psi[b] * a->h_n1[b] * S;
    float* dst = compact ? a->pk[(size_t)b].p : a->d_post.p + a->h_txoff[b];
    const float* src = compact ? a->h_pk[(size_t)b].data() : a->h_post.data() + a->h_txoff[b];
    if (np) HIP_TRY(hipMemcpyAsync(dst, src, sizeof(float) * np, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a->d_z.p + a->h_koff[b], a->h_z.data() + a->h_koff[b], sizeof(int32_t) * a->h_psi[b], hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a->d_pidx.p + r0, a->h_pidx.data() + r0, sizeof(int32_t) * rows, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a->d_Rs.p + r0, a->h_R.data() + r0, sizeof(float) * rows, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemcpyAsync(a->d_n1.p, a->h_n1.data(), sizeof(int32_t) * h->B, hipMemcpyHostToDevice, st));
  return CMDP_OK;
}

// The compact route with the Philox sampler: k_psrlo_count numbers the listed instances' posterior rows, the host reads the
// counts and sizes the blocks the sample kernel will fill
int psrlo_size_blocks(cmdp_psrlo* a, int count) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  hipLaunchKernelGGL(k_psrlo_count, dim3(count), dim3(64), 0, st, a->cnt, a->d_eta.p, a->d_park.p + 2, h->d_state_off.p, h->A,
                     a->d_pidx.p, a->d_n1.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(a->h_n1.data(), a->d_n1.p, sizeof(int32_t) * h->B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int32_t* hl = a->pin_park.p + 2;
  bool moved = false;
  int rc = CMDP_OK;
  for (int k = 0; k < count && !rc; ++k) rc = psrlo_grow(a, hl[k], a->h_n1[hl[k]], &moved);
  if (moved) HIP_TRY(a->d_pkptr.upload(a->h_pkptr.data(), (size_t)h->B, st));
  return rc;
}

// The optimistic sample (K18) of the `count` instances of pin_park's list, by the handle's sample route: k_psrlo_sample after
// the host's draws with the reference sampler; with the Philox sampler the kernel draws everything itself.  The dense route
// fills d_Tx / d_Rx, the compact one (K19) leaves the compact sample of cmdp_psrlo_vi.h.
int psrlo_sample(cmdp_psrlo* a, int count) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const int A = h->A;
  const int32_t* list = a->d_park.p + 2;
  const bool compact = a->sample_solver == 1;
  if (int rc = psrlo_ensure_route(a, a->sample_solver)) return rc;
  if (a->sampler == CMDP_PSRL_SAMPLER_REFERENCE) {
    if (int rc = psrlo_reference_draws(a, count, compact)) return rc;
  } else if (compact) {
    if (int rc = psrlo_size_blocks(a, count)) return rc;
  }
  PoArgs po = a->po;
  if (compact) {
    po.pk = a->d_pkptr.p;
    po.pk_from_host = a->sampler == CMDP_PSRL_SAMPLER_REFERENCE ? 1 : 0;
  }
  HIP_TRY(hipEventRecord(a->ev[0], st));
  if (int rc = set_lds(k_psrlo_sample, a->sample_lds)) return rc;
  hipLaunchKernelGGL(k_psrlo_sample, dim3(count), dim3(PSRLO_THREADS), a->sample_lds, st, a->args, a->cnt, po, list,
                     h->d_state_off.p, A, h->max_S);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(a->ev[1], st));
  a->ev_sample = true;
  for (int k = 0; k < count; ++k) a->h_route[(size_t)a->pin_park.p[2 + k]] = (uint8_t)a->sample_solver;
  h->ps_sample_solver = a->sample_solver;
  psrlo_account(a);
  return CMDP_OK;
}

// K19's launch on device-resident arguments: what cmdp_vi_discounted_optimistic does after its uploads and what the optimistic
// agent does for the instances of a round on the compact route
int pov_launch(PovArgs g, int count, int max_S, int max_rows, hipStream_t st) {
  if (count == 0) return CMDP_OK;
  // Host-only picker of where the sweeps read the row flags and ranges: LDS when they fit, else global memory.  The results
  // do not depend on it (cmdp_psrlo_vi.h); CMDP_POV_DESC=0 forces global memory, for measurements and the tests.
  const char* e = std::getenv("CMDP_POV_DESC");
  g.desc_rows = e && e[0] == '0' && e[1] == '\0' ? 0 : pov_desc_rows(max_rows);
  const size_t lds = pov_lds_bytes(max_S, g.desc_rows);
  if (int rc = set_lds(k_vi_discounted_optimistic, lds)) return rc;
  hipLaunchKernelGGL(k_vi_discounted_optimistic, dim3(count), dim3(POV_WAVES * 64), lds, st, g);
  HIP_TRY(hipGetLastError());
  return CMDP_OK;
}

// sample -> solve (straight into the actor's Q) -> tally -> release for the `count` instances of pin_park's list (already on
// the device at d_park + 2).  The environment is not reset.  An instance that does not converge keeps the last sweep's Q.
int psrlc_round(cmdp_psrlc_t* a, int count, int stop, int64_t n_steps) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const int32_t* list = a->d_park.p + 2;
  cmdp_psrlo* o = a->optimistic ? static_cast<cmdp_psrlo*>(a) : nullptr;
  if (int rc = o ? psrlo_sample(o, count) : psrl_sample(a, count)) return rc;
  DdvArgs g = psrlc_ddv_args(a, list, a->d_T.p, a->d_Rs.p, a->d_Q.p, a->d_V.p, a->d_sweeps.p, a->d_scheme.p, a->d_status.p);
  if (o) {   // the same solver on the extended arrays: A * psi actions per instance, Q straight into the actor's extended table
    g.A = o->d_Ax.p; g.t_off = o->d_txoff.p; g.r_off = o->d_qoff.p;
    g.T = o->d_Tx.p; g.R = o->d_Rx.p; g.Q = o->d_Qx.p;
  }
  HIP_TRY(hipEventRecord(a->ev[2], st));
  if (o && o->sample_solver == 1) {   // K19 on the compact sample: the same outputs, T_ext never built
    PovArgs v{list, a->d_S.p, a->d_A.p, o->d_psi.p, a->d_roff.p, h->d_state_off.p, o->d_qoff.p, o->d_koff.p, o->d_pmoff.p,
              a->d_row_ptr.p, a->d_col.p, o->d_simple.p, o->d_pidx.p, o->d_n1.p, o->d_z.p, o->d_pmk.p, o->d_bump.p, o->d_pkptr.p,
              a->d_Rs.p, PSRLC_GAMMA, PSRLC_EPSILON, CMDP_SCHEME_AUTO, a->size_threshold, a->density_threshold, a->max_sweeps,
              o->d_Qx.p, a->d_V.p, a->d_sweeps.p, a->d_scheme.p, a->d_status.p, 0};
    if (int rc = pov_launch(v, count, h->max_S, h->max_S * h->A, st)) return rc;
  } else if (int rc = ddv_launch(g, count, h->max_S, st)) {
    return rc;
  }
  HIP_TRY(hipEventRecord(a->ev[3], st));
  a->ev_vi = true;
  HIP_TRY(hipMemsetAsync(h->d_ps_tally.p + 1, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_psrlc_tally, dim3(grid_for(count, 256)), dim3(256), 0, st, list, count, a->d_status.p, a->d_sweeps.p,
                     h->d_ps_tally.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_psrl_resume, dim3(grid_for(count, 256)), dim3(256), 0, st, h->env(), a->args, list, count, 0, stop, n_steps);
  HIP_TRY(hipGetLastError());
  h->ps_rounds += 1;
  h->ps_solves += count;
  return CMDP_OK;
}

int psrlc_bind(cmdp_psrlc_t* a) {
  if (!a) return fail(CMDP_ERR_INVALID, "null agent");
  return bind(a->env);
}

// What both creates of the continuous agent build: K12's tables and samplers, the counters of the artificial-episode rule,
// the solve's outputs and the handle's tally
int psrlc_build(cmdp_psrlc_t* a, const int32_t* seeds, const float* reward_prior, const float* transition_prior) {
  if (int rc = psrl_build(a, seeds, reward_prior, transition_prior)) return rc;
  cmdp_t* env = a->env;
  hipStream_t st = env->stream;
  const int B = env->B;
  const int64_t R = env->n_rows;
  AGENT_ZERO(d_nsa, R); AGENT_ZERO(d_nu, R); AGENT_ZERO(d_stamp, R);
  AGENT_ZERO(d_scheme, B); AGENT_ZERO(d_status, B); AGENT_ZERO(d_sweeps, B);
  a->cnt = PcCounters{a->d_nsa.p, a->d_nu.p, a->d_stamp.p};
  if (!env->d_ps_tally.p) {
    HIP_TRY(env->d_ps_tally.alloc(2));
    HIP_TRY(env->d_ps_tally.zero(st));
  }
  return CMDP_OK;
}

// What both creates refuse before they build anything, in this order: K12's arguments, the optimistic create's own arrays
// (`optimistic_args` false: one of psi, eta, log4s is null; the plain create passes true), then the environment handle
int psrlc_create_check(cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon, const float* reward_prior,
                       const float* transition_prior, int sampler, int actor, bool optimistic_args) {
  if (int rc = psrl_create_check(env, seeds, optimization_horizon, reward_prior, transition_prior, sampler, actor)) return rc;
  if (!optimistic_args) return fail(CMDP_ERR_INVALID, "null argument (psi, eta or log4s)");
  return park_check_env(env, false, "PSRLContinuous is the continuous setting's agent: the environment handle is episodic "
                        "(horizon %d; cmdp_psrl_create builds PSRLEpisodic)", "PSRLContinuous", "the dense solver (K13)",
                        PSRL_MAX_STATES);
}

// An episode_end_update of every instance, outside a run: before_start_interacting's on the prior
// (infinite_horizon/posterior_sampling.py:379-383) and cmdp_psrlc_episode_end_update's.  Park all, one round, and the round's
// kernel times once the stream has drained.
int psrlc_update_all(cmdp_psrlc_t* a) {
  if (int rc = park_all(a)) return rc;
  if (int rc = psrlc_round(a, a->env->B, 0, 0)) return rc;
  HIP_TRY(hipStreamSynchronize(a->env->stream));
  psrl_times(a);
  return CMDP_OK;
}

}  // namespace

extern "C" {

int cmdp_psrlc_create(cmdp_psrlc_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon,
                      const float* reward_prior, const float* transition_prior, int sampler, int actor) {
  if (!out) return fail(CMDP_ERR_INVALID, "null output");
  *out = nullptr;
  if (int rc = psrlc_create_check(env, seeds, optimization_horizon, reward_prior, transition_prior, sampler, actor, true)) return rc;
  cmdp_psrlc_t* a = new cmdp_psrlc;
  std::unique_ptr<cmdp_psrlc> guard(a);
  a->env = env;
  a->sampler = sampler;
  if (int rc = psrlc_build(a, seeds, reward_prior, transition_prior)) return rc;
  if (int rc = psrlc_update_all(a)) return rc;   // before_start_interacting: one episode_end_update on the prior
  return agent_attach(guard, out);
}

int cmdp_psrlc_create_optimistic_route(cmdp_psrlc_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon,
                                       const float* reward_prior, const float* transition_prior, const int32_t* psi,
                                       const double* eta, const double* log4s, int sampler, int actor, int sample_solver) {
  if (!out) return fail(CMDP_ERR_INVALID, "null output");
  *out = nullptr;
  if (sample_solver != 0 && sample_solver != 1)
    return fail(CMDP_ERR_INVALID, "sample solver %d: 0 (the dense route) or 1 (the compact route, K19)", sample_solver);
  if (int rc = psrlc_create_check(env, seeds, optimization_horizon, reward_prior, transition_prior, sampler, actor,
                                  psi && eta && log4s)) return rc;
  const int B = env->B, A = env->A;
  std::unique_ptr<cmdp_psrlo> guard(new cmdp_psrlo);
  cmdp_psrlo* a = guard.get();
  a->env = env;
  a->sampler = sampler;
  a->optimistic = true;
  a->h_psi.assign(psi, psi + B);
  a->h_eta.assign(eta, eta + B);
  a->h_qoff.assign((size_t)B, 0); a->h_txoff.assign((size_t)B, 0); a->h_koff.assign((size_t)B, 0); a->h_pmoff.assign((size_t)B, 0);
  std::vector<int32_t> hAx((size_t)B);
  for (int b = 0; b < B; ++b) {
    const int64_t S = env->state_off[b + 1] - env->state_off[b];
    if (psi[b] < 1 || (int64_t)psi[b] * A > 1 << 20)
      return fail(CMDP_ERR_INVALID, "psi[%d] = %d: at least 1, and at most 2^20 extended actions", b, psi[b]);
    if (!(eta[b] > 0.0) || !std::isfinite(eta[b])) return fail(CMDP_ERR_INVALID, "eta[%d] = %g is not a finite value > 0", b, eta[b]);
    if (!std::isfinite(log4s[b])) return fail(CMDP_ERR_INVALID, "log4s[%d] is not finite", b);
    const int64_t n = S * A * psi[b] * S;
    if (n >= (int64_t)1 << 32)
      return fail(CMDP_ERR_UNSUPPORTED, "instance %d: S * A * psi * S = %lld reaches 2^32 (%lld bytes for its extended sample): the "
                  "dense optimistic sample is not built for it", b, (long long)n, (long long)(n * 4));
    hAx[b] = A * psi[b];
    a->h_qoff[b] = a->q_total; a->h_txoff[b] = a->tx_total; a->h_koff[b] = a->k_total;
    a->q_total += S * A * psi[b];
    a->tx_total += (n + 3) & ~(int64_t)3;   // every instance's T_ext starts on a 16-byte boundary
    a->k_total += psi[b];
  }
  // the extended sample is psi times K13's, and the reference sampler's compact upload may be as large again; with them the
  // bump, R_ext and Q arrays and K13's plain-sized sample workspace, which psrl_build allocates: refuse before anything is
  // allocated (what is left out is per layout position, psi * 4 + 12 bytes each: small next to these)
  const bool reference = sampler == CMDP_PSRL_SAMPLER_REFERENCE;
  long long plain = 0;
  for (int b = 0; b < B; ++b) {
    const long long S = env->state_off[b + 1] - env->state_off[b];
    plain += (S * A * S + 3) & ~3LL;
  }
  // the compact route (K19) allocates neither T_ext nor its upload: its posterior blocks grow with the draws
  const bool dense = sample_solver == 0;
  const long long need = ((dense ? (long long)a->tx_total * (reference ? 2 : 1) : 0) + 3 * (long long)a->q_total + plain) * 4;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if ((unsigned long long)need > free_b)
    return fail(CMDP_ERR_OVERFLOW, dense ? "the extended samples T_ext [S, A * psi, S] of the batch and their upload take %lld bytes, "
                "%zu bytes of device memory are free -- create smaller batches or lower max_psi"
                : "the extended Q, R_ext and bump arrays of the batch take %lld bytes, %zu bytes of device memory are free -- "
                "create smaller batches or lower max_psi", need, free_b);
  a->sample_solver = sample_solver;
  a->h_route.assign((size_t)B, (uint8_t)sample_solver);
  a->h_n1.assign((size_t)B, 0);
  if (int rc = psrlc_build(a, seeds, reward_prior, transition_prior)) return rc;
  hipStream_t st = env->stream;
  const int64_t R = env->n_rows, NZ = a->nz;
  int64_t pm_total = 0;
  for (int b = 0; b < B; ++b) {
    a->h_pmoff[b] = pm_total;
    pm_total += (int64_t)psi[b] * (a->h_ptr[(size_t)(env->state_off[b + 1] * A)] - a->h_ptr[(size_t)(env->state_off[b] * A)]);
  }
  if (dense)
    if (int rc = psrlo_ensure_route(a, 0)) return rc;
  HIP_TRY(a->d_psi.upload(psi, B, st)); HIP_TRY(a->d_eta.upload(eta, B, st)); HIP_TRY(a->d_log4s.upload(log4s, B, st));
  HIP_TRY(a->d_Ax.upload(hAx.data(), B, st));
  HIP_TRY(a->d_qoff.upload(a->h_qoff.data(), B, st)); HIP_TRY(a->d_txoff.upload(a->h_txoff.data(), B, st));
  HIP_TRY(a->d_koff.upload(a->h_koff.data(), B, st)); HIP_TRY(a->d_pmoff.upload(a->h_pmoff.data(), B, st));
  AGENT_ZERO(d_N, NZ); AGENT_ZERO(d_pm, NZ); AGENT_ZERO(d_pmk, std::max<int64_t>(pm_total, 1)); AGENT_ZERO(d_bump, a->q_total);
  AGENT_ZERO(d_z, a->k_total); AGENT_ZERO(d_simple, R); AGENT_ZERO(d_pidx, R); AGENT_ZERO(d_n1, B);
  AGENT_ZERO(d_Rx, a->q_total); AGENT_ZERO(d_Qx, a->q_total);
  a->po = PoArgs{a->d_psi.p, a->d_eta.p, a->d_log4s.p, a->d_qoff.p, a->d_txoff.p, a->d_koff.p, a->d_pmoff.p, a->d_N.p, a->d_pm.p,
                 a->d_pmk.p, a->d_bump.p, a->d_z.p, a->d_simple.p, a->d_pidx.p, a->d_n1.p, a->d_post.p, a->d_Tx.p, a->d_Rx.p,
                 a->d_Qx.p};
  if (reference) {
    try {
      a->h_nsa.resize((size_t)R); a->h_z.resize((size_t)a->k_total); a->h_pidx.resize((size_t)R);
      a->h_simple.resize((size_t)R);
    } catch (const std::bad_alloc&) {
      return fail(CMDP_ERR_OVERFLOW, "the host staging of the reference sampler's draws cannot be allocated: %lld bytes",
                  (long long)R * 9 + (long long)a->k_total * 4);
    }
    // before_start_interacting: randn(S, A * psi) on the agent's own RandomState(seed)
    a->as.resize((size_t)B);
    for (int b = 0; b < B; ++b) {
      psrl_host::seed_numpy(a->as[b], (uint32_t)seeds[b]);
      psrlo_host::skip_randn(a->as[b], (b + 1 < B ? a->h_qoff[b + 1] : a->q_total) - a->h_qoff[b]);
    }
  }
  if (int rc = psrlc_update_all(a)) return rc;   // ... then one episode_end_update on the prior
  cmdp_psrlo* attached = nullptr;
  const int rc = agent_attach(guard, &attached);
  *out = attached;
  return rc;
}

int cmdp_psrlc_create_optimistic(cmdp_psrlc_t** out, cmdp_t* env, const int32_t* seeds, int64_t optimization_horizon,
                                 const float* reward_prior, const float* transition_prior, const int32_t* psi, const double* eta,
                                 const double* log4s, int sampler, int actor) {
  return cmdp_psrlc_create_optimistic_route(out, env, seeds, optimization_horizon, reward_prior, transition_prior, psi, eta, log4s,
                                            sampler, actor, 0);
}

int cmdp_psrlc_destroy(cmdp_psrlc_t* a) {
  if (a && a->optimistic) return agent_destroy(static_cast<cmdp_psrlo*>(a));
  return agent_destroy(a);
}

int cmdp_psrlc_run(cmdp_psrlc_t* a, int64_t n_steps, int stop_at_episode_end, const uint8_t* train_mask, int8_t* actions_trace,
                   int32_t* obs_trace, double* reward_trace, double* cumulative_reward, int64_t* steps_taken) {
  if (int rc = park_run_check(a, n_steps, 1LL << 24, "a transition count of the model (float32, as the reference's "
                              "hyper-parameters) would stop counting at 2^24: instance %d has taken %lld steps, %lld more asked for"))
    return rc;
  cmdp_t* h = a->env;
  const int stop = stop_at_episode_end ? 1 : 0;
  const int rc = park_run(
      a, n_steps, stop, train_mask, actions_trace, obs_trace, reward_trace, cumulative_reward, steps_taken,
      [&](const uint8_t* dmask, int8_t* act, int32_t* obs, double* rew) {
        // host-only picker of the walk's form: min_steps = 0 runs the kernels without the gate, which touch no last_change
        const bool gate = a->min_steps > 0;
        const PcGate gt{a->min_steps, a->d_lastchg.p};
        const PoArgs ow = a->optimistic ? static_cast<cmdp_psrlo*>(a)->po : PoArgs{};   // the plain walk reads none of it
        auto launch = [&](auto walk) {
          hipLaunchKernelGGL(walk, dim3(grid_for(h->B, 256)), dim3(256), 0, h->stream, h->env(), a->args, a->cnt, ow, gt, n_steps,
                             dmask, act, obs, rew, a->d_rsum.p);
        };
        if (a->optimistic) gate ? launch(k_psrlc_walk<true, true>) : launch(k_psrlc_walk<false, true>);
        else gate ? launch(k_psrlc_walk<true, false>) : launch(k_psrlc_walk<false, false>);
      },
      [&]() -> int { psrl_times(a); return CMDP_OK; }, [&](int count) { return psrlc_round(a, count, stop, n_steps); });
  psrl_times(a);   // after the call's last synchronisation
  return rc;
}

int cmdp_psrlc_episode_end_update(cmdp_psrlc_t* a) {
  if (int rc = psrlc_bind(a)) return rc;
  return psrlc_update_all(a);
}

int cmdp_psrlc_layout(cmdp_psrlc_t* a, int64_t* n_positions, int64_t* row_ptr, int32_t* col) {
  return park_layout(a, n_positions, row_ptr, col);
}

int cmdp_psrlc_set_option(cmdp_psrlc_t* a, int option, int64_t value) {
  if (int rc = psrlc_bind(a)) return rc;
  if (option == CMDP_PSRLC_OPT_SIZE_THRESHOLD) {
    if (value < 0) return fail(CMDP_ERR_INVALID, "the size threshold of the scheme rule must be >= 0");
    a->size_threshold = value;
    return CMDP_OK;
  }
  if (option == CMDP_PSRLC_OPT_MAX_SWEEPS) {
    if (value < 1) return fail(CMDP_ERR_INVALID, "max_sweeps %lld < 1", (long long)value);
    a->max_sweeps = value;
    return CMDP_OK;
  }
  if (option == CMDP_PSRLC_OPT_POLICY_SOLVER) {
    if (value != 0 && value != 1)
      return fail(CMDP_ERR_INVALID, "policy solver %lld: 0 (the dense route) or 1 (the tables route, K17)", (long long)value);
    a->policy_solver = (int)value;
    return CMDP_OK;
  }
  if (option == CMDP_PSRLC_OPT_SAMPLE_SOLVER) {
    if (!a->optimistic)
      return fail(CMDP_ERR_UNSUPPORTED, "the handle samples plainly: the sample solver is the optimistic agent's option");
    if (value != 0 && value != 1)
      return fail(CMDP_ERR_INVALID, "sample solver %lld: 0 (the dense route) or 1 (the compact route, K19)", (long long)value);
    cmdp_psrlo* o = static_cast<cmdp_psrlo*>(a);
    if (int rc = psrlo_ensure_route(o, (int)value)) return rc;   // the dense arrays may not fit: the handle stays as it is
    o->sample_solver = (int)value;
    return CMDP_OK;
  }
  if (option == CMDP_PSRLC_OPT_MIN_STEPS) {
    if (value < 0 || value > 0x7fffffffLL)
      return fail(CMDP_ERR_INVALID, "min_steps_before_new_episode %lld: at least 0 and at most 2^31 - 1", (long long)value);
    cmdp_t* h = a->env;
    for (int b = 0; b < h->B; ++b)   // the reference fixes it at construction
      if (a->steps_total[(size_t)b] != 0)
        return fail(CMDP_ERR_INVALID, "instance %d has already taken %lld steps: min_steps_before_new_episode is set on a new "
                    "agent", b, (long long)a->steps_total[(size_t)b]);
    if (value > 0 && !a->d_lastchg.p) {
      hipStream_t st = h->stream;
      AGENT_ZERO(d_lastchg, h->B);
    }
    a->min_steps = (int32_t)value;
    return CMDP_OK;
  }
  return fail(CMDP_ERR_INVALID, "unknown option %d", option);
}

int cmdp_psrlc_episode_gate(cmdp_psrlc_t* a, int64_t* min_steps, int32_t* last_change) {
  if (int rc = psrlc_bind(a)) return rc;
  cmdp_t* h = a->env;
  if (min_steps) *min_steps = a->min_steps;
  if (last_change) {
    std::memset(last_change, 0, sizeof(int32_t) * (size_t)h->B);   // no value > 0 yet: nothing has moved it
    if (a->d_lastchg.p) {
      AGENT_FETCH(last_change, d_lastchg, h->B);
      HIP_TRY(hipStreamSynchronize(h->stream));
    }
  }
  return CMDP_OK;
}

int cmdp_psrlc_model(cmdp_psrlc_t* a, float* reward_hp, float* transition_hp, float* transition_prior, int32_t* n_sa,
                     int32_t* nu_k, int64_t* episodes) {
  if (int rc = psrlc_bind(a)) return rc;
  cmdp_t* h = a->env;
  const int64_t R = h->n_rows;
  std::vector<int32_t> stamp(nu_k ? (size_t)R : 0);
  std::vector<int64_t> ep((size_t)h->B);
  AGENT_FETCH(reward_hp, d_rp, 4 * R); AGENT_FETCH(transition_hp, d_tp, a->nz); AGENT_FETCH(n_sa, d_nsa, R); AGENT_FETCH(nu_k, d_nu, R);
  if (nu_k) HIP_TRY(hipMemcpyAsync(stamp.data(), a->d_stamp.p, sizeof(int32_t) * R, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(ep.data(), a->d_episode.p, sizeof(int64_t) * h->B, hipMemcpyDeviceToHost, h->stream));
  if (transition_prior) std::memcpy(transition_prior, a->h_prior.data(), sizeof(float) * h->B);
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (nu_k)   // a count written in an earlier episode is 0 now (cmdp_psrlc.h)
    for (int b = 0; b < h->B; ++b)
      for (int64_t r = h->state_off[b] * h->A; r < h->state_off[b + 1] * h->A; ++r)
        if (stamp[(size_t)r] != (int32_t)ep[b]) nu_k[r] = 0;
  if (episodes) std::memcpy(episodes, ep.data(), sizeof(int64_t) * h->B);
  return CMDP_OK;
}

int cmdp_psrlc_last_sample_optimistic(cmdp_psrlc_t* a, float* T, float* R, float* R_ext, float* Q, int32_t* z, uint8_t* simple,
                                      int64_t* sweeps, int32_t* scheme, int32_t* status) {
  if (int rc = psrlc_bind(a)) return rc;
  if (!a->optimistic) return fail(CMDP_ERR_UNSUPPORTED, "the handle samples plainly: cmdp_psrlc_last_sample returns its sample");
  cmdp_psrlo* o = static_cast<cmdp_psrlo*>(a);
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  bool staged = false;
  if (T) {
    int64_t at = 0;
    for (int b = 0; b < h->B; ++b) {   // the workspace pads every instance to 16 bytes; the caller's array is dense
      const int64_t S = h->state_off[b + 1] - h->state_off[b], n = S * h->A * o->h_psi[b] * S;
      if (o->h_route[(size_t)b] == 2)
        return fail(CMDP_ERR_INVALID, "instance %d holds no sample: its last round could not allocate its posterior rows", b);
      if (o->h_route[(size_t)b] == 1) {
        // a compact sample (K19): its expansion, instance by instance through a staging buffer of one instance's size
        const int64_t r0 = h->state_off[b] * h->A;
        const int n1 = o->h_n1[(size_t)b];
        if (o->d_stage.alloc((size_t)n) != hipSuccess) {
          (void)hipGetLastError();
          return fail(CMDP_ERR_OVERFLOW, "the staging buffer of one instance's expansion cannot be allocated: %lld bytes",
                      (long long)n * 4);
        }
        PoxArgs x{(int)S, h->A, o->h_psi[b], n1, a->d_row_ptr.p + r0, a->d_col.p, o->d_simple.p + r0, o->d_pidx.p + r0,
                  o->d_z.p + o->h_koff[b], o->d_pmk.p + o->h_pmoff[b], o->d_bump.p + o->h_qoff[b], o->pk[(size_t)b].p, o->d_stage.p};
        const int64_t items = S * h->A * o->h_psi[b];
        hipLaunchKernelGGL(k_psrlo_expand, dim3((unsigned)std::min<int64_t>((items + 3) / 4, 4096)), dim3(256), 0, st, x);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(T + at, o->d_stage.p, sizeof(float) * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));   // the next instance reuses (and may reallocate) the staging buffer
        staged = true;
      } else {
        HIP_TRY(hipMemcpyAsync(T + at, o->d_Tx.p + o->h_txoff[b], sizeof(float) * n, hipMemcpyDeviceToHost, st));
      }
      at += n;
    }
  }
  if (R_ext) HIP_TRY(hipMemcpyAsync(R_ext, o->d_Rx.p, sizeof(float) * o->q_total, hipMemcpyDeviceToHost, st));
  if (Q) HIP_TRY(hipMemcpyAsync(Q, o->d_Qx.p, sizeof(float) * o->q_total, hipMemcpyDeviceToHost, st));
  if (z) HIP_TRY(hipMemcpyAsync(z, o->d_z.p, sizeof(int32_t) * o->k_total, hipMemcpyDeviceToHost, st));
  if (simple) HIP_TRY(hipMemcpyAsync(simple, o->d_simple.p, (size_t)h->n_rows, hipMemcpyDeviceToHost, st));
  AGENT_FETCH(R, d_Rs, h->n_rows); AGENT_FETCH(sweeps, d_sweeps, h->B);
  AGENT_FETCH(scheme, d_scheme, h->B); AGENT_FETCH(status, d_status, h->B);
  HIP_TRY(hipStreamSynchronize(st));
  if (staged) o->d_stage.release();   // an instance's T_ext: not kept between calls
  return CMDP_OK;
}

int cmdp_psrlc_counts(cmdp_psrlc_t* a, int32_t* N) {
  if (int rc = psrlc_bind(a)) return rc;
  if (!a->optimistic) return fail(CMDP_ERR_UNSUPPORTED, "the handle samples plainly: it keeps N.sum(-1) only (cmdp_psrlc_model)");
  if (!N) return fail(CMDP_ERR_INVALID, "null argument");
  cmdp_t* h = a->env;
  HIP_TRY(hipMemcpyAsync(N, static_cast<cmdp_psrlo*>(a)->d_N.p, sizeof(int32_t) * a->nz, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CMDP_OK;
}

int cmdp_psrlo_reference_draw(uint32_t* t_key, int32_t* t_pos, int32_t* t_has_gauss, double* t_gauss, uint32_t* r_key,
                              int32_t* r_pos, int32_t* r_has_gauss, double* r_gauss, uint32_t* a_key, int32_t* a_pos,
                              int32_t* a_has_gauss, double* a_gauss, int n_states, int n_actions, int psi, double eta,
                              int64_t skip_randn, const int32_t* n_sa, const int64_t* row_ptr, const int32_t* col, const float* val,
                              float prior, const float* reward_hp, uint8_t* simple, int32_t* n_posterior, float* posterior,
                              int32_t* z, float* R) {
  if (!t_key || !t_pos || !t_has_gauss || !t_gauss || !r_key || !r_pos || !r_has_gauss || !r_gauss || !a_key || !a_pos ||
      !a_has_gauss || !a_gauss || !n_sa || !row_ptr || !col || !val || !reward_hp || !simple || !n_posterior || !posterior || !z || !R)
    return fail(CMDP_ERR_INVALID, "null argument");
  if (n_states < 1 || n_actions < 1 || psi < 1) return fail(CMDP_ERR_INVALID, "n_states, n_actions and psi must be >= 1");
  if (!(prior > 0.0f) || !(eta > 0.0) || skip_randn < 0) return fail(CMDP_ERR_INVALID, "prior and eta must be > 0, skip_randn >= 0");
  if (*t_pos < 0 || *t_pos > 624 || *r_pos < 0 || *r_pos > 624 || *a_pos < 0 || *a_pos > 624)
    return fail(CMDP_ERR_INVALID, "MT19937 position outside [0, 624]");
  const int64_t SA = (int64_t)n_states * n_actions;
  for (int64_t r = 0; r < SA; ++r) {
    if (row_ptr[r + 1] < row_ptr[r]) return fail(CMDP_ERR_INVALID, "row_ptr decreases at row %lld", (long long)r);
    for (int64_t q = row_ptr[r]; q < row_ptr[r + 1]; ++q)
      if (col[q] < 0 || col[q] >= n_states || (q > row_ptr[r] && col[q] <= col[q - 1]) || !(val[q] >= 0.0f))
        return fail(CMDP_ERR_INVALID, "row %lld of the layout: columns ascending within [0, %d), values >= 0", (long long)r, n_states);
    if (!(reward_hp[4 * r + 1] > 0.0f) || !(reward_hp[4 * r + 2] > 0.0f) || !(reward_hp[4 * r + 3] > 0.0f))
      return fail(CMDP_ERR_INVALID, "reward hyper-parameters of row %lld: lambda, alpha and beta must be > 0", (long long)r);
  }
  cmdp_rc::NumpyStream s[3];
  uint32_t* keys[3] = {t_key, r_key, a_key};
  int32_t* pos[3] = {t_pos, r_pos, a_pos};
  int32_t* has[3] = {t_has_gauss, r_has_gauss, a_has_gauss};
  double* gs[3] = {t_gauss, r_gauss, a_gauss};
  for (int i = 0; i < 3; ++i) {
    std::memcpy(s[i].key, keys[i], sizeof s[i].key);
    s[i].pos = *pos[i]; s[i].has_gauss = *has[i]; s[i].gauss = *gs[i];
  }
  psrlo_host::skip_randn(s[2], skip_randn);
  std::vector<int32_t> pidx((size_t)SA);
  *n_posterior = psrlo_host::draw(s[0], s[1], s[2], n_states, n_actions, psi, eta, n_sa, row_ptr, col, val, prior, reward_hp, simple,
                                  pidx.data(), posterior, z, R);
  for (int i = 0; i < 3; ++i) {
    std::memcpy(keys[i], s[i].key, sizeof s[i].key);
    *pos[i] = s[i].pos; *has[i] = s[i].has_gauss; *gs[i] = s[i].gauss;
  }
  return CMDP_OK;
}

int cmdp_psrlc_last_sample(cmdp_psrlc_t* a, float* T, float* R, float* Q, int64_t* sweeps, int32_t* scheme, int32_t* status) {
  if (int rc = psrlc_bind(a)) return rc;
  if (a->optimistic)   // never extended data into a plain-sized buffer
    return fail(CMDP_ERR_UNSUPPORTED, "the handle samples optimistically: cmdp_psrlc_last_sample_optimistic returns its extended sample");
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  if (T) {
    int64_t o = 0;
    for (int b = 0; b < h->B; ++b) {   // the workspace pads every instance to 16 bytes; the caller's array is dense
      const int64_t S = h->state_off[b + 1] - h->state_off[b], n = S * h->A * S;
      HIP_TRY(hipMemcpyAsync(T + o, a->d_T.p + a->h_toff[b], sizeof(float) * n, hipMemcpyDeviceToHost, st));
      o += n;
    }
  }
  AGENT_FETCH(R, d_Rs, h->n_rows); AGENT_FETCH(Q, d_Q, h->n_rows); AGENT_FETCH(sweeps, d_sweeps, h->B);
  AGENT_FETCH(scheme, d_scheme, h->B); AGENT_FETCH(status, d_status, h->B);
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

// discounted_value_iteration(*get_map_estimate()) and argmax_2d for the instances of `mask`, through the policy stage.  The
// dense route: the dense MAP model into d_Tmap / d_Rmap (k_psrlc_map_fill), K13's solver on it.  The tables route
// (CMDP_PSRLC_OPT_POLICY_SOLVER = 1): K17 straight on the posterior tables, no dense workspace.  Reads nothing but the model
// and writes nothing of the agent's but the stage and the MAP model's buffers: the last sample and the actor's Q stay what
// they were.  CMDP_ERR_MAX_ITER when an instance did not converge.
// The workspace of the handle's current policy route, at the route's first request.  CMDP_ERR_OVERFLOW when the dense MAP
// models do not fit.
static int psrlc_policy_workspace(cmdp_psrlc_t* a) {
  const int64_t R = a->env->n_rows;
  const bool tables = a->policy_solver == 1;
  if (!tables && !a->d_mrs.p) {
    if (a->d_Tmap.alloc((size_t)a->t_total) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CMDP_ERR_OVERFLOW, "the dense workspace of the MAP models cannot be allocated: %lld bytes for the batch",
                  (long long)(a->t_total * 4));
    }
    HIP_TRY(a->d_Rmap.alloc((size_t)R)); HIP_TRY(a->d_mrs.alloc((size_t)R));
  }
  if (tables && !a->d_mapc.p) {
    HIP_TRY(a->d_mapt.alloc((size_t)a->nz)); HIP_TRY(a->d_mapc.alloc((size_t)R));
  }
  return CMDP_OK;
}

static int psrlc_policy_solve(cmdp_psrlc_t* a, const uint8_t* mask) {
  cmdp_t* h = a->env;
  hipStream_t st = h->stream;
  const int B = h->B;
  const bool tables = a->policy_solver == 1;
  if (int rc = psrlc_policy_workspace(a)) return rc;
  if (int rc = policy_select(a, 1, true, mask)) return rc;
  PolicyStage& p = a->pol;
  const int rc = policy_stage(a, 1, [&](const int32_t* list, int count) -> int {
    if (tables) {
      size_t staged = 0, plain = 0;   // dynamic LDS of a K17 launch on this batch, by the picker's form
      for (int b = 0; b < B; ++b) {
        const int64_t s0 = h->state_off[b], s1 = h->state_off[b + 1];
        staged = std::max(staged, map_dvi_lds_bytes((int)(s1 - s0), h->A, a->h_ptr[(size_t)(s1 * h->A)] - a->h_ptr[(size_t)(s0 * h->A)],
                                                    MAPDVI_STAGE_MAX_BYTES));
        plain = std::max(plain, map_dvi_value_bytes((int)(s1 - s0)));
      }
      MapDviArgs g{list, a->d_S.p, a->d_A.p, a->d_roff.p, h->d_state_off.p, a->d_row_ptr.p, a->d_col.p, a->d_tp.p, a->d_tprior.p,
                   a->d_rp.p, 4, a->d_mapt.p, a->d_mapc.p, PSRLC_GAMMA, PSRLC_EPSILON, CMDP_SCHEME_AUTO, a->size_threshold,
                   a->density_threshold, a->max_sweeps, p.d_Q.p, p.d_V.p, p.d_sweeps.p, p.d_scheme.p, p.d_status.p, 0};
      return mapdvi_launch(g, count, h->max_S, mapdvi_pick_lds(count, h->cus, staged, plain), st);
    }
    PcMapArgs m{list, a->d_S.p, a->d_A.p, a->d_roff.p, a->d_toff.p, a->d_row_ptr.p, a->d_col.p, a->d_tp.p, a->d_tprior.p, a->d_rp.p,
                a->d_mrs.p, a->d_Tmap.p, a->d_Rmap.p};
    hipLaunchKernelGGL(k_psrlc_map_fill, dim3(count), dim3(MAPVI_THREADS), 0, st, m);
    HIP_TRY(hipGetLastError());
    return ddv_launch(psrlc_ddv_args(a, list, a->d_Tmap.p, a->d_Rmap.p, p.d_Q.p, p.d_V.p, p.d_sweeps.p, p.d_scheme.p, p.d_status.p),
                      count, h->max_S, st);
  });
  return rc ? rc : policy_finish(a, &h->ps_policy_ms, "MAP", (long long)a->max_sweeps);
}

int cmdp_psrlc_policy(cmdp_psrlc_t* a, const uint8_t* mask, float* pi, float* Q, int64_t* sweeps, int32_t* scheme) {
  if (!a || !a->env) return fail(CMDP_ERR_INVALID, "null agent, or its environment handle has been destroyed");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  if (int rc = psrlc_policy_solve(a, mask)) return rc;
  if (int rc = policy_fetch(a, pi, a->pol.d_pi.p, h->A, true)) return rc;
  if (int rc = policy_fetch(a, Q, a->pol.d_Q.p, h->A, true)) return rc;
  if (int rc = policy_fetch(a, sweeps, a->pol.d_sweeps.p, 0, true)) return rc;
  if (int rc = policy_fetch(a, scheme, a->pol.d_scheme.p, 0, true)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CMDP_OK;
}

int cmdp_psrlc_average_reward(cmdp_psrlc_t* a, const uint8_t* mask, double* avg, int32_t* kind) {
  if (!a || !a->env || !avg || !kind) return fail(CMDP_ERR_INVALID, "null argument, or the agent's environment handle has been destroyed");
  if (int rc = bind(a->env)) return rc;
  if (int rc = psrlc_policy_solve(a, mask)) return rc;
  return chain_launch(a->env, a->pol.d_pi.p, nullptr, a->env->d_cur.p, mask, avg, kind, nullptr);
}

int cmdp_vi_discounted_dense(int count, const int32_t* n_states, const int32_t* n_actions, const float* T, const float* R,
                             float gamma, double epsilon, int scheme, int64_t size_threshold, double density_threshold,
                             int64_t max_sweeps, float* Q, float* V, int64_t* sweeps, int32_t* scheme_used, int32_t* status) {
  if (count < 0) return fail(CMDP_ERR_INVALID, "count %d is negative", count);
  if (count == 0) return CMDP_OK;
  if (!n_states || !n_actions || !T || !R || !Q || !V || !sweeps || !scheme_used || !status)
    return fail(CMDP_ERR_INVALID, "null argument");
  if (!std::isfinite(gamma)) return fail(CMDP_ERR_INVALID, "gamma %g is not finite", (double)gamma);
  if (!(epsilon >= 0.0) || !std::isfinite(epsilon)) return fail(CMDP_ERR_INVALID, "epsilon %g is not a finite value >= 0", epsilon);
  if (max_sweeps < 1) return fail(CMDP_ERR_INVALID, "max_sweeps %lld < 1", (long long)max_sweeps);
  if (scheme != CMDP_SCHEME_AUTO && scheme != CMDP_SCHEME_JACOBI && scheme != CMDP_SCHEME_GAUSS_SEIDEL)
    return fail(CMDP_ERR_INVALID, "scheme %d: CMDP_SCHEME_AUTO, CMDP_SCHEME_JACOBI or CMDP_SCHEME_GAUSS_SEIDEL", scheme);
  if (size_threshold < 0) return fail(CMDP_ERR_INVALID, "size_threshold %lld is negative", (long long)size_threshold);
  if (std::isnan(density_threshold)) return fail(CMDP_ERR_INVALID, "density_threshold is not a number");
  BatchLayout L;
  if (int rc = L.build(count, n_states, n_actions,
                       {PSRL_MAX_STATES, "instance %d has %d states: the dense discounted solver keeps V and V_old in LDS for at "
                                         "most %d states"}))
    return rc;
  const int64_t ns = L.ns, nr = L.nr;
  std::vector<int64_t> toff((size_t)count), tsrc((size_t)count);   // T[S, A, S] of an instance: padded on the device, packed in T
  int64_t nt = 0, nsrc = 0;
  for (int b = 0; b < count; ++b) {
    toff[b] = nt; tsrc[b] = nsrc;
    nsrc += L.rows(b) * n_states[b];
    nt += (L.rows(b) * n_states[b] + 3) & ~(int64_t)3;
  }
  for (int64_t i = 0; i < nsrc; ++i)   // a value that is not finite would keep a solve sweeping to max_sweeps
    if (!std::isfinite(T[i])) return fail(CMDP_ERR_INVALID, "T[%lld] is not finite", (long long)i);
  for (int64_t i = 0; i < nr; ++i)
    if (!std::isfinite(R[i])) return fail(CMDP_ERR_INVALID, "R[%lld] is not finite", (long long)i);
  struct Ws {
    DevBuf<int32_t> S, A, scheme, status;
    DevBuf<int64_t> soff, roff, toff, sweeps;
    DevBuf<float> T, R, Q, V;
  };
  DeviceWorkspace<Ws> ws;
  if (int rc = ws.acquire()) return rc;
  hipStream_t st = ws.st;
  HIP_TRY(ws->S.upload(n_states, count, st));
  HIP_TRY(ws->A.upload(n_actions, count, st));
  HIP_TRY(ws->soff.upload(L.soff.data(), L.soff.size(), st));
  HIP_TRY(ws->roff.upload(L.roff.data(), count, st));
  HIP_TRY(ws->toff.upload(toff.data(), count, st));
  if (ws->T.alloc((size_t)nt) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CMDP_ERR_OVERFLOW, "the dense transition models cannot be held on the device: %lld bytes", (long long)(nt * 4));
  }
  for (int b = 0; b < count; ++b)
    HIP_TRY(hipMemcpyAsync(ws->T.p + toff[b], T + tsrc[b], sizeof(float) * (size_t)(L.rows(b) * n_states[b]), hipMemcpyHostToDevice, st));
  HIP_TRY(ws->R.upload(R, (size_t)nr, st));
  HIP_TRY(ws->Q.alloc((size_t)nr));
  HIP_TRY(ws->V.alloc((size_t)ns));
  HIP_TRY(ws->sweeps.alloc(count));
  HIP_TRY(ws->scheme.alloc(count));
  HIP_TRY(ws->status.alloc(count));
  DdvArgs g{nullptr, ws->S.p, ws->A.p, ws->toff.p, ws->roff.p, ws->soff.p, ws->T.p, ws->R.p, gamma, epsilon, scheme, size_threshold,
            density_threshold, max_sweeps, ws->Q.p, ws->V.p, ws->sweeps.p, ws->scheme.p, ws->status.p};
  if (int rc = ddv_launch(g, count, L.max_S, st)) return rc;
  HIP_TRY(ws->Q.download(Q, (size_t)nr, st));
  HIP_TRY(ws->V.download(V, (size_t)ns, st));
  HIP_TRY(ws->sweeps.download(sweeps, count, st));
  HIP_TRY(ws->scheme.download(scheme_used, count, st));
  HIP_TRY(ws->status.download(status, count, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

int cmdp_vi_discounted_optimistic(int count, const int32_t* n_states, const int32_t* n_actions, const int32_t* psi,
                                  const int64_t* row_ptr, const int32_t* col, const uint8_t* simple, const int32_t* z,
                                  const float* pmk, const float* bump, const int32_t* pidx, const float* post, const float* R,
                                  float gamma, double epsilon, int scheme, int64_t size_threshold, double density_threshold,
                                  int64_t max_sweeps, float* Q, float* V, int64_t* sweeps, int32_t* scheme_used, int32_t* status) {
  if (count < 0) return fail(CMDP_ERR_INVALID, "count %d is negative", count);
  if (count == 0) return CMDP_OK;
  const std::pair<const void*, const char*> needed[] = {{n_states, "n_states"}, {n_actions, "n_actions"}, {psi, "psi"},
      {row_ptr, "row_ptr"}, {simple, "simple"}, {z, "z"}, {bump, "bump"}, {pidx, "pidx"}, {R, "R"}, {Q, "Q"}, {V, "V"},
      {sweeps, "sweeps"}, {scheme_used, "scheme_used"}, {status, "status"}};
  for (const auto& n : needed)
    if (!n.first) return fail(CMDP_ERR_INVALID, "%s is null", n.second);
  if (!std::isfinite(gamma)) return fail(CMDP_ERR_INVALID, "gamma %g is not finite", (double)gamma);
  if (!(epsilon >= 0.0) || !std::isfinite(epsilon)) return fail(CMDP_ERR_INVALID, "epsilon %g is not a finite value >= 0", epsilon);
  if (max_sweeps < 1) return fail(CMDP_ERR_INVALID, "max_sweeps %lld < 1", (long long)max_sweeps);
  if (scheme != CMDP_SCHEME_AUTO && scheme != CMDP_SCHEME_JACOBI && scheme != CMDP_SCHEME_GAUSS_SEIDEL)
    return fail(CMDP_ERR_INVALID, "scheme %d: CMDP_SCHEME_AUTO, CMDP_SCHEME_JACOBI or CMDP_SCHEME_GAUSS_SEIDEL", scheme);
  if (size_threshold < 0) return fail(CMDP_ERR_INVALID, "size_threshold %lld is negative", (long long)size_threshold);
  if (std::isnan(density_threshold)) return fail(CMDP_ERR_INVALID, "density_threshold is not a number");
  BatchLayout L;
  if (int rc = L.build(count, n_states, n_actions,
                       {PSRL_MAX_STATES, "instance %d has %d states: the optimistic discounted solver (K19) keeps V and V_old in LDS "
                                         "for at most %d states"}))
    return rc;
  const int64_t ns = L.ns, nr = L.nr;
  if (row_ptr[0] != 0) return fail(CMDP_ERR_INVALID, "row_ptr[0] = %lld, not 0", (long long)row_ptr[0]);
  for (int64_t r = 0; r < nr; ++r)
    if (row_ptr[r + 1] < row_ptr[r]) return fail(CMDP_ERR_INVALID, "row_ptr decreases at row %lld", (long long)r);
  const int64_t nz = row_ptr[nr];
  if (nz > 0 && (!col || !pmk)) return fail(CMDP_ERR_INVALID, "null col / pmk");
  // where the instances start in z, pmk, bump / Q and post; the blocks of post are padded to 16 bytes on the device
  std::vector<int64_t> koff((size_t)count), pmoff((size_t)count), qoff((size_t)count), psrc((size_t)count), pdst((size_t)count);
  std::vector<int32_t> n1((size_t)count, 0);
  int64_t nk = 0, npm = 0, nq = 0, nps = 0, npd = 0;
  for (int b = 0; b < count; ++b) {
    const int S = n_states[b], A = n_actions[b];
    if (psi[b] < 1 || (int64_t)psi[b] * A > 1 << 20)
      return fail(CMDP_ERR_INVALID, "psi[%d] = %d: at least 1, and at most 2^20 extended actions", b, psi[b]);
    if ((int64_t)S * A * psi[b] * S >= (int64_t)1 << 32)
      return fail(CMDP_ERR_UNSUPPORTED, "instance %d: S * A * psi * S reaches 2^32", b);
    koff[b] = nk; pmoff[b] = npm; qoff[b] = nq; psrc[b] = nps; pdst[b] = npd;
    const int64_t r0 = L.roff[b], rows = L.rows(b), nzb = row_ptr[r0 + rows] - row_ptr[r0];
    bool any_simple = false;
    for (int64_t r = r0; r < r0 + rows; ++r) {
      for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e)
        if (col[e] < 0 || col[e] >= S || (e > row_ptr[r] && col[e] <= col[e - 1]))
          return fail(CMDP_ERR_INVALID, "col of row %lld is not ascending within [0, %d)", (long long)r, S);
      if (!std::isfinite(R[r])) return fail(CMDP_ERR_INVALID, "R[%lld] is not finite", (long long)r);
      if (simple[r]) {
        any_simple = true;
      } else {
        if (pidx[r] != n1[b])
          return fail(CMDP_ERR_INVALID, "pidx[%lld] = %d: posterior row %d of instance %d in row order", (long long)r, pidx[r], n1[b], b);
        ++n1[b];
      }
    }
    for (int k = 0; k < psi[b]; ++k) {
      if (any_simple && (z[nk + k] < 0 || z[nk + k] >= S))
        return fail(CMDP_ERR_INVALID, "z[%lld] = %d is not a state of instance %d", (long long)(nk + k), z[nk + k], b);
      for (int64_t e = 0; e < nzb; ++e)
        if (!std::isfinite(pmk[npm + k * nzb + e])) return fail(CMDP_ERR_INVALID, "pmk[%lld] is not finite", (long long)(npm + k * nzb + e));
      for (int64_t r = 0; r < rows; ++r)
        if (!std::isfinite(bump[nq + k * rows + r])) return fail(CMDP_ERR_INVALID, "bump[%lld] is not finite", (long long)(nq + k * rows + r));
    }
    const int64_t np = (int64_t)psi[b] * n1[b] * S;
    if (np > 0 && !post) return fail(CMDP_ERR_INVALID, "post is null and instance %d has posterior rows", b);
    for (int64_t i = 0; i < np; ++i)
      if (!std::isfinite(post[nps + i])) return fail(CMDP_ERR_INVALID, "post[%lld] is not finite", (long long)(nps + i));
    nk += psi[b]; npm += psi[b] * nzb; nq += psi[b] * rows; nps += np; npd += (np + 3) & ~(int64_t)3;
  }
  struct Ws {
    DevBuf<int32_t> S, A, psi, col, pidx, n1, z, scheme, status;
    DevBuf<int64_t> soff, roff, qoff, koff, pmoff, ptr, sweeps;
    DevBuf<uint8_t> simple;
    DevBuf<float> pmk, bump, post, R, Q, V;
    DevBuf<float*> pp;
  };
  DeviceWorkspace<Ws> ws;
  if (int rc = ws.acquire()) return rc;
  hipStream_t st = ws.st;
  HIP_TRY(ws->S.upload(n_states, count, st)); HIP_TRY(ws->A.upload(n_actions, count, st)); HIP_TRY(ws->psi.upload(psi, count, st));
  HIP_TRY(ws->soff.upload(L.soff.data(), L.soff.size(), st)); HIP_TRY(ws->roff.upload(L.roff.data(), count, st));
  HIP_TRY(ws->qoff.upload(qoff.data(), count, st)); HIP_TRY(ws->koff.upload(koff.data(), count, st));
  HIP_TRY(ws->pmoff.upload(pmoff.data(), count, st)); HIP_TRY(ws->ptr.upload(row_ptr, (size_t)nr + 1, st));
  HIP_TRY(ws->col.upload(col, (size_t)nz, st)); HIP_TRY(ws->simple.upload(simple, (size_t)nr, st));
  HIP_TRY(ws->pidx.upload(pidx, (size_t)nr, st)); HIP_TRY(ws->n1.upload(n1.data(), count, st));
  HIP_TRY(ws->z.upload(z, (size_t)nk, st)); HIP_TRY(ws->pmk.upload(pmk, (size_t)npm, st));
  HIP_TRY(ws->bump.upload(bump, (size_t)nq, st)); HIP_TRY(ws->R.upload(R, (size_t)nr, st));
  if (ws->post.alloc((size_t)npd) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CMDP_ERR_OVERFLOW, "the posterior rows cannot be held on the device: %lld bytes", (long long)(npd * 4));
  }
  std::vector<float*> pp((size_t)count, nullptr);
  for (int b = 0; b < count; ++b) {
    const int64_t np = (int64_t)psi[b] * n1[b] * n_states[b];
    if (!np) continue;
    pp[b] = ws->post.p + pdst[b];
    HIP_TRY(hipMemcpyAsync(pp[b], post + psrc[b], sizeof(float) * (size_t)np, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(ws->pp.upload(pp.data(), count, st));
  HIP_TRY(ws->Q.alloc((size_t)nq)); HIP_TRY(ws->V.alloc((size_t)ns));
  HIP_TRY(ws->sweeps.alloc(count)); HIP_TRY(ws->scheme.alloc(count)); HIP_TRY(ws->status.alloc(count));
  PovArgs g{nullptr, ws->S.p, ws->A.p, ws->psi.p, ws->roff.p, ws->soff.p, ws->qoff.p, ws->koff.p, ws->pmoff.p, ws->ptr.p, ws->col.p,
            ws->simple.p, ws->pidx.p, ws->n1.p, ws->z.p, ws->pmk.p, ws->bump.p, ws->pp.p, ws->R.p, gamma, epsilon, scheme,
            size_threshold, density_threshold, max_sweeps, ws->Q.p, ws->V.p, ws->sweeps.p, ws->scheme.p, ws->status.p, 0};
  int max_rows = 0;
  for (int b = 0; b < count; ++b) max_rows = std::max(max_rows, (int)L.rows(b));
  if (int rc = pov_launch(g, count, L.max_S, max_rows, st)) return rc;
  HIP_TRY(ws->Q.download(Q, (size_t)nq, st));
  HIP_TRY(ws->V.download(V, (size_t)ns, st));
  HIP_TRY(ws->sweeps.download(sweeps, count, st));
  HIP_TRY(ws->scheme.download(scheme_used, count, st));
  HIP_TRY(ws->status.download(status, count, st));
  HIP_TRY(hipStreamSynchronize(st));   // `pp` is read by the upload until here
  return CMDP_OK;
}

int cmdp_vi_discounted_map(int count, const int32_t* n_states, const int32_t* n_actions, const int64_t* row_ptr,
                           const int32_t* col, const float* hp, const float* prior, const float* mu, float gamma, double epsilon,
                           int scheme, int64_t size_threshold, double density_threshold, int64_t max_sweeps, float* Q, float* V,
                           int64_t* sweeps, int32_t* scheme_used, int32_t* status, float* t_layout_out, float* c_out) {
  if (count < 0) return fail(CMDP_ERR_INVALID, "count %d is negative", count);
  if (count == 0) return CMDP_OK;
  const std::pair<const void*, const char*> needed[] = {{n_states, "n_states"}, {n_actions, "n_actions"}, {row_ptr, "row_ptr"},
      {prior, "prior"}, {mu, "mu"}, {Q, "Q"}, {V, "V"}, {sweeps, "sweeps"}, {scheme_used, "scheme_used"}, {status, "status"}};
  for (const auto& n : needed)
    if (!n.first) return fail(CMDP_ERR_INVALID, "%s is null", n.second);
  if (!std::isfinite(gamma)) return fail(CMDP_ERR_INVALID, "gamma %g is not finite", (double)gamma);
  if (!(epsilon >= 0.0) || !std::isfinite(epsilon)) return fail(CMDP_ERR_INVALID, "epsilon %g is not a finite value >= 0", epsilon);
  if (max_sweeps < 1) return fail(CMDP_ERR_INVALID, "max_sweeps %lld < 1", (long long)max_sweeps);
  if (scheme != CMDP_SCHEME_AUTO && scheme != CMDP_SCHEME_JACOBI && scheme != CMDP_SCHEME_GAUSS_SEIDEL)
    return fail(CMDP_ERR_INVALID, "scheme %d: CMDP_SCHEME_AUTO, CMDP_SCHEME_JACOBI or CMDP_SCHEME_GAUSS_SEIDEL", scheme);
  if (size_threshold < 0) return fail(CMDP_ERR_INVALID, "size_threshold %lld is negative", (long long)size_threshold);
  if (std::isnan(density_threshold)) return fail(CMDP_ERR_INVALID, "density_threshold is not a number");
  BatchLayout L;
  if (int rc = L.build(count, n_states, n_actions,
                       {MAPVI_MAX_STATES, "instance %d has %d states: value iteration on a MAP model (K17) keeps V and V_old in LDS "
                                          "for at most %d states"}))
    return rc;
  const int64_t ns = L.ns, nr = L.nr;
  if (row_ptr[0] != 0) return fail(CMDP_ERR_INVALID, "row_ptr[0] = %lld, not 0", (long long)row_ptr[0]);
  for (int64_t r = 0; r < nr; ++r)
    if (row_ptr[r + 1] < row_ptr[r]) return fail(CMDP_ERR_INVALID, "row_ptr decreases at row %lld", (long long)r);
  const int64_t nz = row_ptr[nr];
  if (nz > 0 && !col) return fail(CMDP_ERR_INVALID, "col is null");
  if (nz > 0 && !hp) return fail(CMDP_ERR_INVALID, "hp is null");
  size_t staged = 0, plain = 0;
  for (int b = 0; b < count; ++b) {
    const int64_t* ptr = row_ptr + L.roff[b];
    if (int rc = map_check_layout(b, n_states[b], n_actions[b], ptr, col, hp, prior[b])) return rc;
    staged = std::max(staged, map_dvi_lds_bytes(n_states[b], n_actions[b], ptr[L.rows(b)] - ptr[0], MAPDVI_STAGE_MAX_BYTES));
    plain = std::max(plain, map_dvi_value_bytes(n_states[b]));
  }
  for (int64_t i = 0; i < nr; ++i)   // a value that is not finite would keep a solve sweeping to max_sweeps
    if (!std::isfinite(mu[i])) return fail(CMDP_ERR_INVALID, "mu[%lld] is not finite", (long long)i);
  struct Ws {
    DevBuf<int32_t> S, A, col, scheme, status;
    DevBuf<int64_t> soff, roff, ptr, sweeps;
    DevBuf<float> hp, prior, mu, t, c, Q, V;
  };
  DeviceWorkspace<Ws> ws;
  if (int rc = ws.acquire()) return rc;
  hipStream_t st = ws.st;
  HIP_TRY(ws->S.upload(n_states, count, st));
  HIP_TRY(ws->A.upload(n_actions, count, st));
  HIP_TRY(ws->soff.upload(L.soff.data(), L.soff.size(), st));
  HIP_TRY(ws->roff.upload(L.roff.data(), count, st));
  HIP_TRY(ws->ptr.upload(row_ptr, (size_t)nr + 1, st));
  HIP_TRY(ws->col.upload(col, (size_t)nz, st));
  HIP_TRY(ws->hp.upload(hp, (size_t)nz, st));
  HIP_TRY(ws->prior.upload(prior, count, st));
  HIP_TRY(ws->mu.upload(mu, (size_t)nr, st));
  HIP_TRY(ws->t.alloc((size_t)nz));
  HIP_TRY(ws->c.alloc((size_t)nr));
  HIP_TRY(ws->Q.alloc((size_t)nr));
  HIP_TRY(ws->V.alloc((size_t)ns));
  HIP_TRY(ws->sweeps.alloc(count));
  HIP_TRY(ws->scheme.alloc(count));
  HIP_TRY(ws->status.alloc(count));
  MapDviArgs g{nullptr, ws->S.p, ws->A.p, ws->roff.p, ws->soff.p, ws->ptr.p, ws->col.p, ws->hp.p, ws->prior.p, ws->mu.p, 1,
               ws->t.p, ws->c.p, gamma, epsilon, scheme, size_threshold, density_threshold, max_sweeps, ws->Q.p, ws->V.p,
               ws->sweeps.p, ws->scheme.p, ws->status.p, 0};
  int dev = 0, cus = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  if (int rc = mapdvi_launch(g, count, L.max_S, mapdvi_pick_lds(count, cus, staged, plain), st)) return rc;
  HIP_TRY(ws->Q.download(Q, (size_t)nr, st));
  HIP_TRY(ws->V.download(V, (size_t)ns, st));
  HIP_TRY(ws->sweeps.download(sweeps, count, st));
  HIP_TRY(ws->scheme.download(scheme_used, count, st));
  HIP_TRY(ws->status.download(status, count, st));
  if (t_layout_out) HIP_TRY(ws->t.download(t_layout_out, (size_t)nz, st));
  if (c_out) HIP_TRY(ws->c.download(c_out, (size_t)nr, st));
  HIP_TRY(hipStreamSynchronize(st));
  return CMDP_OK;
}

}  // extern "C"

// ---- the logged loop's driver -------------------------------------------------------------------------------------------------
// MDPLoop.run for the batch on the rows, the tracker and log_row of cmdp_logged_loop.h: interval, step t, evaluation, log_row,
// the next interval -- which is enqueued BEFORE the host waits for the row when the agent allows it and the row cannot change
// the training mask (row_may_freeze, limit_within_reach); the results are the same either way (tests/test_gpu_mdploop.py
// holds both against the step-by-step loop).  The agent's adapter supplies:
//   ahead                      may rows run ahead at all?  Not for the agents that park: park_run synchronises in every round
//   pre(switches)              the agent's own refusals and allocations for the whole of desc->n_steps; steps nothing
//   run(n, mask, cum)          n steps under the training mask (page-locked); `cum` (page-locked, nullable) receives the reward
//                              sums after them, by the time the stream has run them
//   evaluate(buffers, &done)   the row's evaluation into page-locked memory; `done`: the stream it ends on, if not the handle's
namespace {

struct RowBuffers {
  // `cum` twice: the next interval's kernel may already be writing its sums while the host reads this row's
  PinnedBuf<double> cum[2], avg;
  PinnedBuf<float> v0;
  PinnedBuf<int32_t> snap, akind;
  PinnedBuf<uint8_t> mask, need;
  int alloc(int B, size_t n_states) {
    if (int rc = cum[0].alloc(B)) return rc;
    if (int rc = cum[1].alloc(B)) return rc;
    if (int rc = avg.alloc(B)) return rc;
    if (int rc = v0.alloc(n_states)) return rc;
    if (int rc = snap.alloc((size_t)3 * B)) return rc;
    if (int rc = akind.alloc(B)) return rc;
    if (int rc = mask.alloc(B)) return rc;
    if (int rc = need.alloc(B)) return rc;
    for (int b = 0; b < B; ++b) cum[0].p[b] = cum[1].p[b] = 0.0;
    return CMDP_OK;
  }
};

template <typename Adapter>
int run_logged(AgentBase* a, bool episodic, Adapter&& ad, const cmdp_loop_desc* d, int64_t n_logs, int64_t* steps, double* values,
               uint8_t* kinds, int64_t* last_training_step, uint8_t* is_training) {
  using namespace cmdp_tracker;
  using clk = std::chrono::steady_clock;
  if (!a || !d || !steps || !values || !kinds) return fail(CMDP_ERR_INVALID, "null argument");
  cmdp_t* h = a->env;
  if (int rc = bind(h)) return rc;
  const int B = h->B;
  const int64_t T = d->n_steps;
  hipStream_t st = h->stream;
  // everything below is refused before anything is reset or stepped: a caller that falls back to another loop must find the
  // agent untouched
  std::vector<LoggedRow> plan;
  if (int rc = logged_plan(d, n_logs, &plan)) return rc;
  if (int rc = check_logged_baselines(d, B, episodic)) return rc;
  if (!episodic && !h->has_dp) return fail(CMDP_ERR_INVALID, "the handle was created without the DP half (CSR transition matrices)");
  if (!episodic && d->log_every > 0 && chain_lds_bytes(h->max_S, h->max_row_nnz) > (size_t)kLdsBudget)
    return fail(CMDP_ERR_UNSUPPORTED, "instance with %d states (max %d successors per row) exceeds the LDS budget of K9",
                h->max_S, h->max_row_nnz);
  const LoggedSwitches& sw = logged_switches();
  if (int rc = ad.pre(sw)) return rc;
  RowBuffers buf;
  if (int rc = buf.alloc(B, (size_t)h->n_states)) return rc;
  for (int i = 0; i < 2; ++i)
    if (!h->ev_row[i])
      HIP_TRY(hipEventCreateWithFlags(&h->ev_row[i], hipEventDisableTiming | (sw.blocking_sync ? hipEventBlockingSync : 0)));
  LoggedRun run;
  run.init(B, episodic, T, d, h->H, h->state_off.data(), buf.mask.p, last_training_step);
  // MDPLoop.run: visitation counts cleared, environment reset (agent_mdp_interaction.py:219-224)
  if (int rc = cmdp_reset_visits(h)) return rc;
  if (int rc = cmdp_reset(h, nullptr, nullptr)) return rc;
  const auto t_start = clk::now();
  auto secs = [](clk::time_point a0, clk::time_point a1) { return std::chrono::duration<double>(a1 - a0).count(); };
  auto elapsed = [&]() { return secs(t_start, clk::now()); };
  // the steps of row i: those whose reward sums it logs, then -- inside the loop -- step t itself
  auto enqueue_interval = [&](size_t i) -> int {
    const LoggedRow& r = plan[i];
    double* c = buf.cum[i & 1].p;
    if (r.n_run > 0) {
      if (int rc = ad.run(r.n_run, buf.mask.p, c)) return rc;
    } else {   // no step since the previous row's own: its sums
      HIP_TRY(hipMemcpyAsync(c, a->d_rsum.p, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    }
    return r.in_loop ? ad.run(1, buf.mask.p, nullptr) : CMDP_OK;
  };

  const size_t n_rows = plan.size();
  double longest_row = 0.0, last_row_done = elapsed();
  double t_enq = 0.0, t_wait = 0.0, t_host = 0.0;   // the debug line's
  int64_t n_ahead = 0;
  if (int rc = enqueue_interval(0)) return rc;
  for (size_t i = 0; i < n_rows; ++i) {
    const LoggedRow& r = plan[i];
    const auto c0 = clk::now();
    if (!episodic) continuous_need(run.tr, buf.need.p);
    hipStream_t done = st;
    if (int rc = ad.evaluate(buf, &done)) return rc;
    HIP_TRY(hipEventRecord(h->ev_row[1], done));   // the row's end
    const bool drain = sw.drain_every > 0 && (i + 1) % (size_t)sw.drain_every == 0;
    const bool ahead = ad.ahead && sw.pipeline && i + 1 < n_rows && !drain &&
                       !limit_within_reach(d->max_time - elapsed(), longest_row, run.limit_passed_while_ahead) &&
                       !row_may_freeze(run.tr, episodic, r.t, T);
    if (ahead)
      if (int rc = enqueue_interval(i + 1)) return rc;
    n_ahead += ahead;
    const auto c1 = clk::now();
    HIP_TRY(hipEventSynchronize(h->ev_row[1]));
    const auto c2 = clk::now();
    {
      const double e = elapsed();
      longest_row = std::max(longest_row, e - last_row_done);
      last_row_done = e;
    }
    t_enq += secs(c0, c1);
    t_wait += secs(c1, c2);
    steps[i] = r.t;
    const double sps = (double)r.t / std::max(elapsed(), 1e-9);
    const RowReadback in{buf.cum[i & 1].p, buf.v0.p, buf.snap.p, buf.need.p, buf.avg.p, buf.akind.p};
    bool changed = false;   // run() reads the mask from buf.mask at every call
    if (int rc = log_row(run, r, in, sps, d->max_time - elapsed(), ahead, values + i * N_COLUMNS * B, kinds + i * N_COLUMNS * B, &changed))
      return rc;
    const auto c3 = clk::now();
    t_host += secs(c2, c3);
    if (!r.in_loop) break;
    if (!ahead) {
      if (drain) HIP_TRY(hipStreamSynchronize(st));
      if (int rc = enqueue_interval(i + 1)) return rc;
      t_enq += secs(c3, clk::now());
    }
  }
  HIP_TRY(hipStreamSynchronize(st));
  if (sw.debug)
    std::fprintf(stderr, "[logged loop] %d instances, %zu rows (%lld with the next interval started early): enqueue %.2f s, waiting for the device %.2f s, "
                 "host row work %.2f s\n", B, n_rows, (long long)n_ahead, t_enq, t_wait, t_host);
  if (is_training)
    for (int b = 0; b < B; ++b) is_training[b] = run.tr.inst[(size_t)b].training ? 1 : 0;
  return CMDP_OK;
}

// Q-learning: everything is enqueued.  Two things overlap with the evaluation of row i and with the host's work on it: the
// agents' NEXT interval (same stream) and, for the continuous agent, the stationary-distribution solve itself (second stream,
// on a snapshot of the policy and of the current states).  Everything a row reads comes back WITHOUT copy kernels: the
// kernels write into page-locked host memory directly (V[0, :], the start states and in-episode times, the average rewards
// and their kinds, the reward sums) and read the evaluation mask from it.
struct QlLogged {
  static constexpr bool ahead = true;
  cmdp_agent_t* a;
  cmdp_t* h = a->env;
  hipStream_t sx = nullptr;        // the continuous solve's: the second stream when rows run ahead
  std::vector<uint8_t> on_device;  // the training mask a->d_mask holds: uploaded only when it has changed

  int pre(const cmdp_tracker::LoggedSwitches& sw) {
    const int B = h->B;
    sx = h->stream;
    if (a->d_mask.n < (size_t)B) HIP_TRY(a->d_mask.alloc(B));
    if (h->d_ch_mask.n < (size_t)B) HIP_TRY(h->d_ch_mask.alloc(B));
    if (a->continuous && sw.pipeline) {
      if (!h->aux.stream) HIP_TRY(hipStreamCreateWithFlags(&h->aux.stream, hipStreamNonBlocking));
      sx = h->aux.stream;
      if (h->d_cur_snap.n < (size_t)B) HIP_TRY(h->d_cur_snap.alloc(B));
    }
    return CMDP_OK;
  }

  int run(int64_t n, const uint8_t* mask, double* cum) {   // the kernel leaves the sums in `cum` itself
    if (on_device.empty() || std::memcmp(on_device.data(), mask, on_device.size()) != 0) {
      on_device.assign(mask, mask + h->B);
      HIP_TRY(hipMemcpyAsync(a->d_mask.p, mask, h->B, hipMemcpyHostToDevice, h->stream));
    }
    return ql_enqueue_run(a, n, a->d_mask.p, nullptr, cum);
  }

  int evaluate(RowBuffers& buf, hipStream_t* done) {
    const int B = h->B;
    hipStream_t st = h->stream;
    if (!a->continuous) return ql_enqueue_evaluate(a, buf.v0.p, buf.snap.p);
    bool any = false;
    for (int b = 0; b < B; ++b) any = any || buf.need.p[b];
    if (!any) return CMDP_OK;
    if (int rc = ql_enqueue_greedy(a)) return rc;
    const int32_t* start = h->d_cur.p;
    if (sx != st) {
      HIP_TRY(hipMemcpyAsync(h->d_cur_snap.p, h->d_cur.p, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, st));
      start = h->d_cur_snap.p;
      HIP_TRY(hipEventRecord(h->ev_row[0], st));
      HIP_TRY(hipStreamWaitEvent(sx, h->ev_row[0], 0));
    }
    *done = sx;
    return chain_launch(h, a->d_pi.p, nullptr, start, buf.need.p, buf.avg.p, buf.akind.p, nullptr, true, false, sx);
  }
};

// What the agents that park refuse of a logged run of T steps besides their own: an agent that has taken steps, and what
// every run() call of the loop would check, once for all of the run's steps (the counters start from the driver's reset)
int park_logged_check(ParkAgent* a, int64_t T, int64_t step_limit, const char* limit_text) {
  // MDPLoop._cumulative_reward starts at zero with the run; the agent's sums count from its creation
  for (int b = 0; b < a->env->B; ++b)
    if (a->steps_total[(size_t)b] != 0)
      return fail(CMDP_ERR_INVALID, "instance %d has already taken %lld steps: a logged run starts from a new agent", b,
                  (long long)a->steps_total[(size_t)b]);
  if (T > step_limit) return fail(CMDP_ERR_OVERFLOW, limit_text, 0, 0LL, (long long)T);
  if (2 + 2 * T > 0x7fffffffLL)
    return fail(CMDP_ERR_OVERFLOW, "a visit counter (int32 on the device) could wrap in a run of %lld steps", (long long)T);
  return CMDP_OK;
}

struct Ucrl2Logged {
  static constexpr bool ahead = false;
  cmdp_ucrl2_t* a;
  const cmdp_loop_desc* d;
  int pre(const cmdp_tracker::LoggedSwitches&) {
    if (int rc = park_logged_check(a, d->n_steps, 0x7fffffffLL, "a transition count of the model (int32, as the reference's N) "
                                   "could wrap: instance %d has taken %lld steps, %lld asked for")) return rc;
    return ucrl2_ensure_trace(a, d->n_steps);
  }
  int run(int64_t n, const uint8_t* mask, double* cum) { return cmdp_ucrl2_run(a, n, 0, mask, nullptr, nullptr, nullptr, cum, nullptr); }
  int evaluate(RowBuffers& buf, hipStream_t*) {
    cmdp_t* h = a->env;
    bool any = false;
    for (int b = 0; b < h->B; ++b) any = any || buf.need.p[b];
    if (!any) return CMDP_OK;
    // cmdp_ucrl2_average_reward(a, need, .): K14 where the model has changed, then the chain kernels on the stored policies
    if (int rc = ucrl2_policy_solve(a, buf.need.p)) return rc;
    return chain_launch(h, a->pol.d_pi.p, nullptr, h->d_cur.p, buf.need.p, buf.avg.p, buf.akind.p, nullptr, true, false);
  }
};

struct PsrlLogged {
  static constexpr bool ahead = false;
  cmdp_psrl_t* a;
  const cmdp_loop_desc* d;
  int pre(const cmdp_tracker::LoggedSwitches&) {
    if (int rc = park_logged_check(a, d->n_steps, 1LL << 24, "a transition count of the model (float32, as the reference's "
                                   "hyper-parameters) would stop counting at 2^24: instance %d has taken %lld steps, %lld asked for"))
      return rc;
    return psrl_evaluate_check(a->env);
  }
  int run(int64_t n, const uint8_t* mask, double* cum) { return cmdp_psrl_run(a, n, 0, mask, nullptr, nullptr, nullptr, cum, nullptr); }
  // what cmdp_psrl_evaluate(a, NULL, .) enqueues; the gather writes V[0, :] and the start states straight into the row's memory
  int evaluate(RowBuffers& buf, hipStream_t*) {
    if (int rc = psrl_enqueue_evaluate(a, nullptr, buf.v0.p, buf.snap.p)) return rc;
    return psrl_policy_finish(a);
  }
};

// The continuous PSRL agents, plain and optimistic (K13, K18): the rows' evaluation is what cmdp_psrlc_average_reward(a, need, .)
// enqueues, by the handle's current policy route
struct PsrlcLogged {
  static constexpr bool ahead = false;
  cmdp_psrlc_t* a;
  const cmdp_loop_desc* d;
  int pre(const cmdp_tracker::LoggedSwitches&) {
    if (int rc = park_logged_check(a, d->n_steps, 1LL << 24, "a transition count of the model (float32, as the reference's "
                                   "hyper-parameters) would stop counting at 2^24: instance %d has taken %lld steps, %lld asked for"))
      return rc;
    // everything the rows allocate, now: the route's workspace (the dense MAP models may not fit) and the policy stage
    if (a->policy_solver == 1 && a->env->max_S > MAPVI_MAX_STATES)
      return fail(CMDP_ERR_UNSUPPORTED, "%d states: value iteration on a MAP model (K17) keeps V and V_old in LDS for at most %d",
                  a->env->max_S, MAPVI_MAX_STATES);
    if (int rc = psrlc_policy_workspace(a)) return rc;
    return policy_select(a, 1, true, nullptr);
  }
  int run(int64_t n, const uint8_t* mask, double* cum) { return cmdp_psrlc_run(a, n, 0, mask, nullptr, nullptr, nullptr, cum, nullptr); }
  int evaluate(RowBuffers& buf, hipStream_t*) {
    cmdp_t* h = a->env;
    bool any = false;
    for (int b = 0; b < h->B; ++b) any = any || buf.need.p[b];
    if (!any) return CMDP_OK;
    if (int rc = psrlc_policy_solve(a, buf.need.p)) return rc;
    return chain_launch(h, a->pol.d_pi.p, nullptr, h->d_cur.p, buf.need.p, buf.avg.p, buf.akind.p, nullptr, true, false);
  }
};

}  // namespace

extern "C" {

int cmdp_qlearning_run_logged(cmdp_agent_t* a, const cmdp_loop_desc* d, int64_t n_logs, int64_t* steps, double* values,
                              uint8_t* kinds, int64_t* last_training_step, uint8_t* is_training) {
  if (!a) return fail(CMDP_ERR_INVALID, "null argument");
  const int rc = run_logged(a, !a->continuous, QlLogged{a}, d, n_logs, steps, values, kinds, last_training_step, is_training);
  if (rc == CMDP_OK) a->env->known_reset = true;   // the interaction kernels reset at once after every terminating step
  return rc;
}

int cmdp_ucrl2_run_logged(cmdp_ucrl2_t* a, const cmdp_loop_desc* d, int64_t n_logs, int64_t* steps, double* values, uint8_t* kinds,
                          int64_t* last_training_step, uint8_t* is_training) {
  return run_logged(a, false, Ucrl2Logged{a, d}, d, n_logs, steps, values, kinds, last_training_step, is_training);
}

int cmdp_psrl_run_logged(cmdp_psrl_t* a, const cmdp_loop_desc* d, int64_t n_logs, int64_t* steps, double* values, uint8_t* kinds,
                         int64_t* last_training_step, uint8_t* is_training) {
  return run_logged(a, true, PsrlLogged{a, d}, d, n_logs, steps, values, kinds, last_training_step, is_training);
}

int cmdp_psrlc_run_logged(cmdp_psrlc_t* a, const cmdp_loop_desc* d, int64_t n_logs, int64_t* steps, double* values, uint8_t* kinds,
                          int64_t* last_training_step, uint8_t* is_training) {
  return run_logged(a, false, PsrlcLogged{a, d}, d, n_logs, steps, values, kinds, last_training_step, is_training);
}

}  // extern "C"
