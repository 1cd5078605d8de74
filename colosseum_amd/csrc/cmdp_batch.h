// cmdp_batch.h -- host side of the batch solvers that take no environment handle: cmdp_extended_vi (K10),
// cmdp_vi_discounted_model (K14), cmdp_vi_episodic_dense (K12's solver) and cmdp_vi_episodic_map (K15).
//
// BatchLayout is where the instances of a ragged batch start in the concatenated per-state and per-row arrays, and the
// refusals every solver makes of an instance's size.  check_row_form is the one check of the row form K10 and K14 read
// (CSR rows, or one value for a row that holds it at every state) and the fill of the per-row uniform values the kernels
// are given.  Nothing here makes a HIP call: every refusal below comes before the device is touched, so the argument
// checks of the entry points run on a machine without one.  Included by cmdp.hip.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/cmdp.h"

namespace { int fail(int code, const char* fmt, ...); }  // cmdp.hip: sets the text of cmdp_last_error, returns `code`

// What a solver takes of one instance.  The texts are printf formats over (instance, its states or actions, the cap).
struct BatchCaps {
  int max_states;
  const char* states_text;
  int max_actions = 0;  // 0: any number of actions
  const char* actions_text = nullptr;
};

struct BatchLayout {  // filled by one call of build()
  int count = 0;
  const int32_t* S = nullptr;  // [count] the caller's n_states / n_actions
  const int32_t* A = nullptr;
  std::vector<int64_t> soff;   // [count + 1] first state of the instance; the last entry is ns
  std::vector<int64_t> roff;   // [count] first row (s, a) of the instance
  int64_t ns = 0, nr = 0;      // states and rows of the batch
  int max_S = 0;

  int64_t rows(int b) const { return (int64_t)S[b] * A[b]; }

  int build(int n, const int32_t* n_states, const int32_t* n_actions, const BatchCaps& caps) {
    count = n, S = n_states, A = n_actions;
    soff.assign((size_t)n + 1, 0);
    roff.assign((size_t)n, 0);
    for (int b = 0; b < n; ++b) {
      if (S[b] < 1) return fail(CMDP_ERR_INVALID, "n_states[%d] = %d < 1", b, S[b]);
      if (A[b] < 1) return fail(CMDP_ERR_INVALID, "n_actions[%d] = %d < 1", b, A[b]);
      if (S[b] > caps.max_states) return fail(CMDP_ERR_UNSUPPORTED, caps.states_text, b, S[b], caps.max_states);
      if (caps.max_actions && A[b] > caps.max_actions) return fail(CMDP_ERR_UNSUPPORTED, caps.actions_text, b, A[b], caps.max_actions);
      soff[b] = ns, roff[b] = nr;
      ns += S[b];
      nr += rows(b);
      max_S = std::max(max_S, S[b]);
    }
    soff[n] = ns;
    return CMDP_OK;
  }
};

// The models of a batch in the row form, concatenated: row r of instance b is the global row roff[b] + r.
struct RowForm {
  const int64_t* ptr;      // [nr + 1] from 0, never decreasing
  const int32_t* col;      // instance-relative, ascending within a row
  const float* val;        // finite, >= 0
  const float* uniform;    // [nr] or null: c > 0 on a row without entries that holds c at every state, else 0
  const float* rewards;    // [nr] finite
};

// Refuses a malformed row form and leaves in `uni` [nr] what the kernels read as ModelViArgs::uni / EviArgs::uni.
// row_check(r) is the solver's own check of global row r (CMDP_OK, or its refusal), run after the row's reward.
template <typename RowCheck>
int check_row_form(const BatchLayout& L, const RowForm& m, std::vector<float>* uni, RowCheck&& row_check) {
  if (m.ptr[0] != 0) return fail(CMDP_ERR_INVALID, "csr_ptr[0] = %lld, not 0", (long long)m.ptr[0]);
  for (int64_t r = 0; r < L.nr; ++r)
    if (m.ptr[r + 1] < m.ptr[r]) return fail(CMDP_ERR_INVALID, "csr_ptr decreases at row %lld", (long long)r);
  if (m.ptr[L.nr] > 0 && (!m.col || !m.val)) return fail(CMDP_ERR_INVALID, "null csr_col / csr_val");
  uni->assign((size_t)L.nr, 0.0f);
  for (int b = 0; b < L.count; ++b) {
    const int S = L.S[b];
    for (int64_t r = L.roff[b]; r < L.roff[b] + L.rows(b); ++r) {
      const int64_t rb = m.ptr[r], re = m.ptr[r + 1];
      for (int64_t k = rb; k < re; ++k) {
        if (m.col[k] < 0 || m.col[k] >= S || (k > rb && m.col[k] <= m.col[k - 1]))
          return fail(CMDP_ERR_INVALID, "csr_col of row %lld is not ascending within [0, %d)", (long long)r, S);
        if (!(m.val[k] >= 0.0f) || !std::isfinite(m.val[k]))
          return fail(CMDP_ERR_INVALID, "csr_val[%lld] = %g is not a finite probability >= 0", (long long)k, (double)m.val[k]);
      }
      if (!std::isfinite(m.rewards[r])) return fail(CMDP_ERR_INVALID, "rewards[%lld] is not finite", (long long)r);
      if (int rc = row_check(r)) return rc;
      if (m.uniform && m.uniform[r] != 0.0f) {
        if (!(m.uniform[r] > 0.0f) || !std::isfinite(m.uniform[r]) || re != rb)
          return fail(CMDP_ERR_INVALID, "uniform[%lld] = %g: must be finite > 0 on a row without CSR entries",
                      (long long)r, (double)m.uniform[r]);
        (*uni)[(size_t)r] = m.uniform[r];
      } else if (re - rb == S && m.val[rb] > 0.0f) {  // a full row of one value is taken as uniform too
        bool same = true;
        for (int64_t k = rb + 1; k < re && same; ++k) same = m.val[k] == m.val[rb];
        if (same) (*uni)[(size_t)r] = m.val[rb];
      }
    }
  }
  return CMDP_OK;
}
