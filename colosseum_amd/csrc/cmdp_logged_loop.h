// cmdp_logged_loop.h -- host side of the logged interaction loop that is not indicator arithmetic: the rows of a run
// (MDPLoop.run's schedule), the rule that lets the next interval start before a row's result is known, and what a row does
// on the host once its evaluation has come back (log_row).  run_logged of cmdp.hip -- the one driver behind
// cmdp_qlearning_run_logged, cmdp_ucrl2_run_logged and cmdp_psrl_run_logged -- drives the device around these;
// cmdp_tracker_replay runs the same rows on inputs given by the caller, which is how the CPU test suite reaches this code.
// Nothing here makes a HIP call, reads the environment or looks at a clock: times are handed in.  Included by cmdp.hip
// after cmdp_tracker.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/cmdp.h"
#include "cmdp_tracker.h"

namespace { int fail(int code, const char* fmt, ...); }  // cmdp.hip: sets the text of cmdp_last_error, returns `code`

namespace cmdp_tracker {

// The rows of the run.  Row i: `n_run` steps whose reward sums the row logs (the reference reads `_cumulative_reward` at
// step t BEFORE adding that step's reward), then -- inside the loop -- step t itself, whose update the logged policy
// already contains; then the evaluation of the agents' greedy policies.  log_every == 1 leaves no step between two rows:
// the sum through step t-1 is then what the previous row's single step left.
struct LoggedRow { int64_t t, n_run, n_since; bool in_loop; };

// T >= 1; log_every <= 0: only the final row.  The Python twin is vector_tracker.log_schedule.
inline void plan_logged_rows(int64_t T, int64_t log_every, std::vector<LoggedRow>* rows) {
  rows->clear();
  int64_t done = 0, n_since = 0;
  if (log_every > 0)
    for (int64_t tl = log_every; tl < T; tl += log_every) {
      if (tl - done > 0) n_since += tl - done;
      rows->push_back(LoggedRow{tl, tl - done, n_since, true});
      done = tl + 1;
      n_since = 1;
    }
  if (T - done > 0) n_since += T - done;
  rows->push_back(LoggedRow{T - 1, T - done, n_since, false});
}

// CMDP_LOGGED_PIPELINE, CMDP_SYNC_MODE=block, CMDP_LOGGED_DRAIN_EVERY, CMDP_LOGGED_DEBUG (logged_switches of cmdp.hip reads them)
struct LoggedSwitches {
  bool pipeline;       // rows that cannot change the training mask have their next interval enqueued before the host waits
  bool blocking_sync;  // the row events are created with hipEventBlockingSync
  int drain_every;     // the stream is drained completely every n rows (0: never)
  bool debug;          // one line on stderr per call: where the host thread's time went
};

// ---- may the next interval start before row `r`'s result is known? ------------------------------------------------------
// The next interval needs its training mask before the row's result is known.  The mask changes in two ways only: (a) an
// instance freezes -- `after_log` requires the last n_check normalised regrets, this row's included, to be ~0 and t > 0.2 T,
// so a row whose n_check - 1 predecessors are not all ~0 cannot freeze anything, and the host knows that BEFORE the row;
// (b) the time limit -- rows closer than a few seconds to it are not run ahead.  A row for which either answers true is
// processed in order.

// (a), the tracker's part
inline bool row_may_freeze(const Tracker& tr, bool episodic, int64_t t, int64_t T) {
  const double atol = episodic ? 1e-4 : 1e-5;
  for (int b = 0; b < tr.B; ++b) {
    const Instance& x = tr.inst[(size_t)b];
    if (!episodic && !x.training && !x.cached) return true;   // the cached evaluation is taken at this row: `need` changes
    if (x.training && may_freeze(x, tr.n_check, t, T, atol)) return true;
  }
  return false;
}

// (b), the clock's part.  "Within reach" follows the longest row seen so far (a park round of the reward caches, a throttled
// host, sixteen batches sharing the GPU can make one row take seconds).
inline bool limit_within_reach(double time_left, double longest_row, bool limit_passed_while_ahead) {
  return limit_passed_while_ahead || time_left < std::max(5.5, 3.0 * longest_row);
}

// ---- one row on the host ------------------------------------------------------------------------------------------------
// What survives from row to row besides the tracker.  `mask` is the caller's memory (the driver uploads it from there) and
// starts all ones; `last_training_step` may be null.
struct LoggedRun {
  Tracker tr;
  bool episodic = false;
  int64_t T = 0;
  EpisodicInputs ein;                      // episodic
  const int64_t* state_off = nullptr;      // episodic: [B] first flat state of every instance
  uint8_t* mask = nullptr;                 // [B] who trains in the interval after the row
  int64_t* last_training_step = nullptr;   // [B] the row at which the time limit froze the instance
  bool limit_passed_while_ahead = false;
  std::vector<int64_t> start_abs;

  void init(int B, bool episodic_, int64_t T_, const cmdp_loop_desc* d, int horizon, const int64_t* state_off_, uint8_t* mask_,
            int64_t* last_training_step_) {
    tr.init(B, d->n_check, d->base_val, d->base_kind);
    episodic = episodic_;
    T = T_;
    ein = EpisodicInputs{horizon, d->opt0, d->worst0, d->start_pos, d->start_prob, d->kmax};
    state_off = state_off_;
    mask = mask_;
    last_training_step = last_training_step_;
    start_abs.assign((size_t)B, 0);
    for (int b = 0; b < B; ++b) {
      mask[b] = 1;
      if (last_training_step) last_training_step[b] = -1;
    }
  }
};

// What the evaluation of a row brought back.  snap [3][B]: last_start | prev_start | hstep.
struct RowReadback {
  const double* cum;       // [B] reward sums through step t - 1
  const float* v0;         // episodic: V[0, :] of the greedy policies, flat
  const int32_t* snap;     // episodic
  const uint8_t* need;     // continuous: continuous_need before the row
  const double* avg;       // continuous: average rewards of the instances with need
  const int32_t* akind;    // continuous: != 0 np.float32
};

// The row's indicators into val / knd [N_COLUMNS][B], then -- inside the loop -- the time-limit freeze and the mask of the next
// interval; *changed: it differs from the previous one.  `time_left`: seconds to max_time; `ahead`: the next interval is
// already running on the old mask.
inline int log_row(LoggedRun& run, const LoggedRow& r, const RowReadback& in, double steps_per_second, double time_left, bool ahead,
                   double* val, uint8_t* knd, bool* changed) {
  Tracker& tr = run.tr;
  const int B = tr.B;
  *changed = false;
  if (run.episodic) {
    // the reference logs step t before the reset that follows a termination: if step t ended an episode (in-episode
    // time back at 0), its `last_starting_node` is still the start of the episode that ended
    for (int b = 0; b < B; ++b)
      run.start_abs[(size_t)b] = run.state_off[b] + ((in.snap[2 * B + b] == 0 && r.in_loop) ? in.snap[B + b] : in.snap[b]);
    episodic_update(tr, run.ein, r.t, run.T, in.v0, run.start_abs.data(), in.cum, r.n_since, r.in_loop, steps_per_second, val, knd);
  } else {
    continuous_update(tr, r.t, run.T, in.need, in.avg, in.akind, in.cum, r.n_since, r.in_loop, steps_per_second, val, knd);
  }
  if (!r.in_loop) return CMDP_OK;
  // `_limit_exceeded` (agent_mdp_interaction.py:172-177) for the batch.  Should the limit pass on a row whose successor is
  // already running (a row far longer than any before it), the freeze is recorded at the next row -- which then runs in order
  bool out_of_time = time_left < 0.5;
  if (out_of_time && ahead) { run.limit_passed_while_ahead = true; out_of_time = false; }
  for (int b = 0; b < B; ++b) {
    if (out_of_time && tr.inst[(size_t)b].training) {
      tr.inst[(size_t)b].training = false;
      if (run.last_training_step) run.last_training_step[b] = r.t;
    }
    const uint8_t m = tr.inst[(size_t)b].training ? 1 : 0;
    *changed = *changed || m != run.mask[b];
    run.mask[b] = m;
  }
  if (*changed && ahead)   // cannot happen (see row_may_freeze); a wrong row must not be returned silently
    return fail(CMDP_ERR_HIP, "logged loop: the training mask changed at step %lld although the next interval was already running",
                (long long)r.t);
  return CMDP_OK;
}

// ---- what the driver refuses of a description ------------------------------------------------------------------------------
// The agents that park their instances for a solve synchronise in every round of a run, so there is nothing to start early:
// for them the driver never runs ahead and walks the rows strictly in order -- interval, step t, evaluation, log_row with
// `ahead` false, the next interval's mask -- with neither the second stream nor LoggedSwitches.pipeline playing a part.

// Before anything is reset or stepped: the baselines a row needs, and the continuous setting's `optimal - worst > 0.0002`
// (agent_mdp_interaction.py:379-382)
inline int check_logged_baselines(const cmdp_loop_desc* d, int B, bool episodic) {
  if (!d->base_val || !d->base_kind) return fail(CMDP_ERR_INVALID, "baseline average rewards missing");
  if (episodic && (!d->opt0 || !d->worst0 || !d->start_pos || !d->start_prob || d->kmax < 1))
    return fail(CMDP_ERR_INVALID, "episodic baselines missing");
  if (!episodic)
    for (int b = 0; b < B; ++b)
      if (!(d->base_val[3 * b] - d->base_val[3 * b + 1] > 0.0002))
        return fail(CMDP_ERR_INVALID, "instance %d: optimal and worst average reward are closer than 0.0002", b);
  return CMDP_OK;
}

}  // namespace cmdp_tracker
