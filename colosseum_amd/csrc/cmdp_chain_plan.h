// cmdp_chain_plan.h -- host side of the Markov-chain family (K9, K9F, the mixing time; kernels in cmdp_chain.h).
//
// plan_chains builds K9F's plan, the eight arrays k_chain_fast takes on trust: per instance a minimum-degree elimination
// order of the transition graph, every pivot's candidate list in the filled graph, and rounds of pivots whose rank-1
// updates touch disjoint entries (chain_elim_graph, min_degree_order, schedule_rounds; the K9F comment of cmdp_chain.h says
// what the kernel relies on).  pick_chain decides which of K9 and K9F an average-reward call launches and with how much
// LDS, pick_mixing_path whether a mixing time steps X or takes matrix powers, policy_chain_csc builds the float64 chain of
// a policy that both mixing-time drivers read.  All of it is pure: the handle, the uploads and the launches stay with
// cmdp.hip, which also reads CMDP_CHAIN_FAST (chain_switches) and evaluates the two LDS formulas of cmdp_chain.h.  Nothing
// here makes a HIP call or reads the environment.  Included by cmdp.hip after include/cmdp.h (the error codes).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace { int fail(int code, const char* fmt, ...); }  // cmdp.hip: sets the text of cmdp_last_error, returns `code`

// cmdp.hip holds these against K9F_MAXC, the <16> it launches and kLdsBudget
constexpr int kChainMaxCand = 128;           // candidates a pivot of a planned instance may have
constexpr int kChainRoundWidth = 16;         // pivots per round = wavefronts of k_chain_fast's workgroup
constexpr int kChainLdsBudget = 160 * 1024;  // bytes of LDS one workgroup may claim

// ---- K9F's plan ----------------------------------------------------------------------------------------------------------
// Rows of bitsets over the S states (or positions) of one instance
struct ChainBits {
  int S, nwd;
  std::vector<uint64_t> w;
  explicit ChainBits(int S_) : S(S_), nwd((S_ + 63) / 64), w((size_t)S_ * ((S_ + 63) / 64), 0) {}
  uint64_t* row(int u) { return &w[(size_t)u * nwd]; }
  const uint64_t* row(int u) const { return &w[(size_t)u * nwd]; }
  void set(int u, int v) { row(u)[v >> 6] |= 1ull << (v & 63); }
  int count(int u) const {
    int n = 0;
    for (int k = 0; k < nwd; ++k) n += __builtin_popcountll(row(u)[k]);
    return n;
  }
  int common(int u, int v) const {
    int n = 0;
    for (int k = 0; k < nwd; ++k) n += __builtin_popcountll(row(u)[k] & row(v)[k]);
    return n;
  }
};

// The elimination graph of the instance whose states start at `so`: its transition graph over all actions (positive
// entries, no self-loops), symmetrised
inline ChainBits chain_elim_graph(int S, int A, int64_t so, const int64_t* csr_ptr, const int32_t* csr_col, const float* csr_val) {
  ChainBits g(S);
  for (int s = 0; s < S; ++s)
    for (int a = 0; a < A; ++a) {
      const int64_t r = (so + s) * A + a;
      for (int64_t k = csr_ptr[r]; k < csr_ptr[r + 1]; ++k)
        if (csr_val[k] > 0.0f && csr_col[k] != s) { g.set(s, csr_col[k]); g.set(csr_col[k], s); }
    }
  return g;
}

// Minimum-degree elimination of `g` (consumed): the live state of lowest degree goes next, its neighbours become a clique.
// rank[s] = position of state s; cands[i] = the neighbours of pivot i when it goes, as positions (all above i), ascending.
// false = no plan: a pivot has more than kChainMaxCand candidates.
inline bool min_degree_order(ChainBits g, std::vector<int>* rank, std::vector<std::vector<int>>* cands) {
  const int S = g.S;
  std::vector<int> degree((size_t)S);
  std::vector<char> alive((size_t)S, 1);
  for (int u = 0; u < S; ++u) degree[(size_t)u] = g.count(u);
  rank->assign((size_t)S, -1);
  cands->assign((size_t)S, {});
  for (int step = 0; step < S; ++step) {
    int v = -1;
    for (int u = 0; u < S; ++u)
      if (alive[(size_t)u] && (v < 0 || degree[(size_t)u] < degree[(size_t)v])) v = u;   // ties: the smallest state
    (*rank)[(size_t)v] = step;
    alive[(size_t)v] = 0;
    std::vector<int>& nb = (*cands)[(size_t)step];
    const uint64_t* gv = g.row(v);
    for (int k = 0; k < g.nwd; ++k)
      for (uint64_t x = gv[k]; x; x &= x - 1) nb.push_back(64 * k + __builtin_ctzll(x));
    if (step < S - 1 && (int)nb.size() > kChainMaxCand) return false;
    for (int u : nb) {   // the neighbours become a clique; v leaves the graph
      uint64_t* gu = g.row(u);
      for (int k = 0; k < g.nwd; ++k) gu[k] |= gv[k];
      gu[u >> 6] &= ~(1ull << (u & 63));
      gu[v >> 6] &= ~(1ull << (v & 63));
      degree[(size_t)u] = g.count(u);
    }
  }
  for (std::vector<int>& nb : *cands) {
    for (int& x : nb) x = (*rank)[(size_t)x];
    std::sort(nb.begin(), nb.end());
  }
  return true;
}

// Rounds of up to kChainRoundWidth pivots: a pivot is ready once every lower pivot that lists it is done; of the ready
// ones, lowest position first, a round takes those that share at most one candidate with each pivot it already holds
// (two pivots of a round are then not each other's candidates either: a pivot is ready only after the pivots that list
// it).  The last position is no pivot and must not become ready: `x < S - 1` keeps it out.  Its last lister need not go in
// the last round (a transition graph of several components: the one that holds positions S - 2 and S - 1 can finish rounds
// before another), and without the guard it would take the place of a pivot that is then never scheduled.  Writes the
// S - 1 pivots in schedule order to `piv` and appends round -> first slot (rounds + 1 entries) to `rptr`; returns the
// number of rounds, -1 when a round stays empty.
inline int schedule_rounds(const std::vector<std::vector<int>>& cands, int32_t* piv, std::vector<int32_t>* rptr) {
  const int S = (int)cands.size();
  ChainBits cb(S);
  std::vector<int> pending((size_t)S, 0), ready;
  for (int i = 0; i < S; ++i)
    for (int x : cands[(size_t)i]) { cb.set(i, x); pending[(size_t)x]++; }
  for (int i = 0; i < S - 1; ++i)
    if (!pending[(size_t)i]) ready.push_back(i);
  int filled = 0, nr = 0;
  while (filled < S - 1) {
    std::sort(ready.begin(), ready.end());
    std::vector<int> rnd, rest;
    for (int p : ready) {
      bool fits = (int)rnd.size() < kChainRoundWidth;
      for (size_t q = 0; fits && q < rnd.size(); ++q) fits = cb.common(p, rnd[q]) <= 1;
      (fits ? rnd : rest).push_back(p);
    }
    // cannot trigger: the lowest pivot not yet scheduled has every lower pivot done, so it is ready, and the first ready
    // pivot meets an empty round, which it fits
    if (rnd.empty()) return -1;
    rptr->push_back(filled);
    for (int p : rnd) {
      piv[filled++] = p;
      for (int x : cands[(size_t)p])
        if (--pending[(size_t)x] == 0 && x < S - 1) rest.push_back(x);
    }
    ready.swap(rest);
    ++nr;
  }
  rptr->push_back(filled);
  return nr;
}

// The arrays of ChainFast (cmdp_chain.h), as they are uploaded
struct ChainPlan {
  std::vector<int32_t> rank, cptr, nrounds, rptr, piv;
  std::vector<int64_t> cbase, rbase;
  std::vector<uint16_t> cand;
  bool any = false;   // some instance has a plan
  ChainPlan(int64_t NS, int B) : rank((size_t)NS, -1), cptr((size_t)NS + B, 0), nrounds((size_t)B, -1), piv((size_t)NS, 0), cbase((size_t)B, 0), rbase((size_t)B, 0) {}
};

// The plan of every instance of a batch.  Instances without one (a pivot with more than kChainMaxCand candidates, fewer
// than 2 or more than 65 535 states) have nrounds = -1 and keep K9; they take no room in `cand` and `rptr`.
inline ChainPlan plan_chains(int B, int A, const int64_t* state_off, const int64_t* csr_ptr, const int32_t* csr_col, const float* csr_val) {
  ChainPlan p(state_off[B], B);
  std::vector<int> rank;
  std::vector<std::vector<int>> cands;
  for (int b = 0; b < B; ++b) {
    const int64_t so = state_off[b];
    const int S = (int)(state_off[b + 1] - so);
    p.cbase[(size_t)b] = (int64_t)p.cand.size();
    p.rbase[(size_t)b] = (int64_t)p.rptr.size();
    if (S < 2 || S > 65535) continue;
    if (!min_degree_order(chain_elim_graph(S, A, so, csr_ptr, csr_col, csr_val), &rank, &cands)) continue;
    const int nr = schedule_rounds(cands, p.piv.data() + so, &p.rptr);
    if (nr < 0) { p.rptr.resize((size_t)p.rbase[(size_t)b]); continue; }
    p.nrounds[(size_t)b] = nr;
    std::copy(rank.begin(), rank.end(), p.rank.begin() + so);
    int32_t* cp = p.cptr.data() + so + b;
    for (int i = 0; i < S; ++i) {
      for (int x : cands[(size_t)i]) p.cand.push_back((uint16_t)x);
      cp[i + 1] = cp[i] + (int)cands[(size_t)i].size();
    }
    p.any = true;
  }
  if (p.any && p.cand.empty()) p.cand.push_back(0);   // (no upload is empty)
  if (p.any && p.rptr.empty()) p.rptr.push_back(0);
  return p;
}

// ---- the kernels of one average-reward call ------------------------------------------------------------------------------
struct ChainChoice {
  int refusal;      // CMDP_OK, or CMDP_ERR_UNSUPPORTED: not even K9 fits
  size_t k9_lds;    // dynamic LDS bytes of k_chain_average_reward
  bool fast;        // k_chain_fast runs first and flags the instances it leaves to K9
  size_t fast_lds;  // ... with this much LDS
};

// k9_lds / fast_lds: chain_lds_bytes / chain_fast_lds_bytes of the batch.  K9F (irreducible chains, fill-reducing order,
// rounds of independent pivots) runs first unless the reference's summation order is asked for (CMDP_OPT_CHAIN_EXACT_ORDER),
// CMDP_CHAIN_FAST = 0 switches it off (`fast_enabled`), no instance has a plan, or it does not fit LDS.
inline ChainChoice pick_chain(int max_S, int max_row_nnz, size_t k9_lds, size_t fast_lds, bool exact_order, bool fast_enabled, bool any_plan) {
  ChainChoice c{CMDP_OK, k9_lds, false, fast_lds};
  if (k9_lds > (size_t)kChainLdsBudget)
    c.refusal = fail(CMDP_ERR_UNSUPPORTED, "instance with %d states (max %d successors per row) exceeds the LDS budget of K9", max_S, max_row_nnz);
  else
    c.fast = !exact_order && fast_enabled && any_plan && fast_lds <= (size_t)kChainLdsBudget;
  return c;
}

// ---- the mixing time ------------------------------------------------------------------------------------------------------
// CMDP_OPT_MIXING_PATH: 0 auto, 1 matrix powers, 2 stepping.  Stepping keeps a float64 row of X in LDS; auto takes the
// powers when that does not fit and above 1024 states.
enum MixingPath { MIXING_STEPPING, MIXING_POWERS };
inline int pick_mixing_path(int option, int max_S, MixingPath* out) {
  const bool fits_lds = sizeof(double) * (size_t)max_S <= (size_t)kChainLdsBudget - 1024;
  if (option == 2 && !fits_lds)
    return fail(CMDP_ERR_UNSUPPORTED, "a row of X (%d states, float64) does not fit LDS: the stepping path cannot run", max_S);
  *out = option == 1 || (option == 0 && (!fits_lds || max_S > 1024)) ? MIXING_POWERS : MIXING_STEPPING;
  return CMDP_OK;
}

// The chain of a policy as the mixing-time kernels read it: P[s, j] = sum_a pi[s, a] * T[s, a, j] (float64, actions in
// order; pi null: uniform), rows normalised, as CSC with the predecessors of a state in index order.  xoff: start of every
// instance's S x S block of X.
struct PolicyCsc {
  std::vector<int64_t> cptr, xoff;
  std::vector<int32_t> crow;
  std::vector<double> cval;
};
inline PolicyCsc policy_chain_csc(int B, int A, const int64_t* state_off, const int64_t* ptr, const int32_t* col, const float* val, const float* pi) {
  const int64_t NS = state_off[B];
  PolicyCsc c;
  c.cptr.assign((size_t)NS + 1, 0);
  c.xoff.assign((size_t)B + 1, 0);
  std::vector<std::vector<std::pair<int32_t, double>>> incoming((size_t)NS);
  std::vector<double> rowacc;
  std::vector<int32_t> touched;
  for (int b = 0; b < B; ++b) {
    const int64_t so = state_off[b], S = state_off[b + 1] - so;
    c.xoff[b + 1] = c.xoff[b] + S * S;
    rowacc.assign((size_t)S, 0.0);
    for (int64_t s = 0; s < S; ++s) {
      touched.clear();
      for (int a = 0; a < A; ++a) {
        const int64_t r = (so + s) * A + a;
        const double w = pi ? (double)pi[r] : 1.0 / A;
        if (w == 0.0) continue;
        for (int64_t k = ptr[r]; k < ptr[r + 1]; ++k) {
          if (rowacc[col[k]] == 0.0) touched.push_back(col[k]);
          rowacc[col[k]] += w * (double)val[k];
        }
      }
      // the float32 probabilities of a row sum to 1 only within ~1e-7: without this, X_t would lose or gain that much
      // mass per step (1e-2 over the 1e5 steps a slow chain needs).  The chain is DEFINED with normalised rows.
      double rowsum = 0.0;
      for (int32_t j : touched) rowsum += rowacc[j];
      for (int32_t j : touched) {
        if (rowacc[j] != 0.0) incoming[(size_t)(so + j)].push_back({(int32_t)s, rowacc[j] / rowsum});
        rowacc[j] = 0.0;
      }
    }
  }
  for (int64_t j = 0; j < NS; ++j) {
    c.cptr[j + 1] = c.cptr[j] + (int64_t)incoming[j].size();
    for (auto& e : incoming[j]) { c.crow.push_back(e.first); c.cval.push_back(e.second); }  // s ascending by construction
  }
  return c;
}
