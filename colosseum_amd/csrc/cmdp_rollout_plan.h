// cmdp_rollout_plan.h -- host-side planning of the LDS-resident rollout kernels (K1L / K1P, K1T, K1U, K1E, K1S).
//
// One function per kernel family.  Each takes plain host data of a validated batch description and returns a plan plus
// the host images the plan's kernel reads, or "not eligible" (ok == false).  None makes a HIP call: cmdp_create uploads
// the images and wires the device pointers into the plans.  pick_rollout chooses among the eligible plans per launch.
// Included by cmdp.hip after the kernel headers.
#pragma once

constexpr int kLdsBudget = 160 * 1024;  // bytes of LDS one workgroup may claim on gfx950

// dynamic LDS of a K1L / K1P workgroup of g instances
inline size_t k1l_lds_bytes(const LdsPlan& p, int g) {
  const int rings = p.pipe ? 2 * K1P_ACT_STRIDE(p.ch) + 2 * K1P_TR_STRIDE(p.ch) : 2 * p.ch;
  return (size_t)K1L_FIXED + (size_t)g * (size_t)(p.slot_bytes + rings);
}

// The rounds of workgroups a batch of B instances needs at `cap` instances per workgroup and `slots` resident workgroups,
// and the fewest instances per workgroup that still need that many rounds: evens out the last round and keeps LDS bank
// conflicts down (53 instead of 52 lanes per walker measured +1.2 % at C2).
struct EvenGroups {
  int64_t rounds;
  int G;
};
inline EvenGroups even_groups(int64_t B, int cap, int64_t slots) {
  const int64_t wgs = (B + cap - 1) / cap, rounds = (wgs + slots - 1) / slots;
  return {rounds, (int)std::min<int64_t>(cap, std::max<int64_t>(1, (B + rounds * slots - 1) / (rounds * slots)))};
}

struct PlanInput {
  const cmdp_desc* d;    // the sampler half: sp_ptr, sp_next, sp_cum, sp_reward, sp_rkind, state_off, start_off
  const RowDesc* rows;   // [R] validated row descriptors
  int B, A, H, max_S;
  int cus;               // compute units of the device
};

// Environment read when a handle is created (tests and tools/stress_k1t.py)
struct PlanKnobs {
  int pipe = -1;               // CMDP_K1L_PIPE: 0 plans K1L only, 1 K1P only
  int k1t_G = 0, k1u_G = 0;    // CMDP_K1T_G / CMDP_K1U_G: instances per workgroup (0: planned)
  int k1s_G = 0;               // CMDP_K1S_G: likewise for K1S (walker wavefronts and team size follow from it)
  int k1l_G = 0;               // CMDP_K1L_G: likewise for K1L / K1P, at the candidate the planner chose
  int k1t_ch = 0;              // CMDP_K1T_CH: 64 | 32 | 16 plans K1T at that chunk length only (0: planned)
  int k1t_debug = 0, k1e_debug = 0;   // CMDP_K1T_DEBUG / CMDP_K1E_DEBUG: stages switched off (timing experiments only)
  int k1e_pair = 1;            // CMDP_K1E_PAIR: 0 keeps every K1E launch in the single form (results unchanged)
};
inline PlanKnobs plan_knobs() {
  auto num = [](const char* name, int unset) { const char* e = std::getenv(name); return e ? std::atoi(e) : unset; };
  PlanKnobs k;
  k.pipe = num("CMDP_K1L_PIPE", -1);
  k.k1t_G = std::getenv("CMDP_K1T_G") ? std::max(1, num("CMDP_K1T_G", 0)) : 0;
  k.k1u_G = std::getenv("CMDP_K1U_G") ? std::max(1, num("CMDP_K1U_G", 0)) : 0;
  k.k1s_G = std::getenv("CMDP_K1S_G") ? std::max(1, num("CMDP_K1S_G", 0)) : 0;
  k.k1l_G = std::getenv("CMDP_K1L_G") ? std::max(1, num("CMDP_K1L_G", 0)) : 0;
  k.k1t_ch = std::max(0, num("CMDP_K1T_CH", 0));
  k.k1t_debug = num("CMDP_K1T_DEBUG", 0);
  k.k1e_debug = num("CMDP_K1E_DEBUG", 0);
  k.k1e_pair = num("CMDP_K1E_PAIR", 1);
  return k;
}

// Codes of n reward values v(i): indices into *vals, the distinct values in order of first appearance.  false when there
// are more than 256.
template <class V, class C>
inline bool reward_codes(int64_t n, V v, std::vector<double>* vals, std::vector<C>* codes) {
  std::unordered_map<uint64_t, int> code_of;
  codes->resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const double x = v(i);
    uint64_t bits;
    std::memcpy(&bits, &x, sizeof bits);
    auto it = code_of.find(bits);
    if (it == code_of.end()) {
      if (vals->size() == 256) return false;
      it = code_of.emplace(bits, (int)vals->size()).first;
      vals->push_back(x);
    }
    (*codes)[(size_t)i] = (C)it->second;
  }
  return true;
}

// ---- deterministic batches: the tables K1L / K1P, K1T, K1U and K1E are built from -----------------------------------
struct DetTables {
  std::vector<double> vals;       // distinct reward values, in order of first appearance
  std::vector<uint8_t> codes;     // [R] reward code of every row
  std::vector<uint16_t> next16;   // [R] successor of every row
};

// Uniform S <= 65535, deterministic rows, one start state per instance and <= 256 distinct rewards.  The caller has
// checked that there are no MT19937 slots and that the rewards are the table's values (no Beta, no reward cache).
inline bool det_tables(const PlanInput& in, DetTables* t) {
  const int64_t* so = in.d->state_off;
  const int64_t R = so[in.B] * in.A;
  if (in.max_S > 65535) return false;
  for (int b = 0; b < in.B; ++b)
    if (so[b + 1] - so[b] != in.max_S || in.d->start_off[b + 1] - in.d->start_off[b] != 1) return false;
  for (int64_t r = 0; r < R; ++r)
    if (in.rows[r].n != 1) return false;
  t->next16.resize((size_t)R);
  for (int64_t r = 0; r < R; ++r) t->next16[(size_t)r] = (uint16_t)in.rows[r].next_if_det;
  return reward_codes(R, [&](int64_t r) { return in.rows[r].reward_if_det; }, &t->vals, &t->codes);
}

// ---- K1L / K1P -----------------------------------------------------------------------------------------------------
struct K1lpChoice {
  bool ok = false;
  LdsPlan p{};
  double cost = -1.0;    // rounds x time per transition of the chosen candidate
  int G1 = 0, G2 = 0;    // LDS capacity in instances per workgroup at one / two workgroups per CU
  int per_cu = 0;        // workgroups per CU of the chosen candidate
  int succ_bits = 1;     // bits of a row base (successor * A)
  bool pipe_ok = false;  // the packed words have room for K1P's byte offsets (one more bit)
};

inline K1lpChoice plan_k1lp(const PlanInput& in, const DetTables& t, const PlanKnobs& k) {
  K1lpChoice c;
  LdsPlan& p = c.p;
  const int rows_max = in.max_S * in.A;
  p.rows_max = rows_max;
  // reward code in the upper bits of the successor word when both fit 16 bits: one table and one LDS read less
  // (the successor is stored as its row base, successor * A)
  int bits_c = 0;
  while ((1 << c.succ_bits) < rows_max) ++c.succ_bits;
  while ((1 << bits_c) < (int)t.vals.size()) ++bits_c;
  p.code_shift = (c.succ_bits + bits_c <= 16) ? c.succ_bits : 0;
  c.pipe_ok = c.succ_bits + 1 + bits_c <= 16;
  p.off_rcode = (rows_max * 2 + 3) & ~3;
  if (p.code_shift) {  // packed: successor words, 8-bit count deltas (+ the walker's dummy counter), overflow list
    p.off_cnt = p.off_rcode;
    p.off_ovf = p.off_cnt + ((rows_max + 4 + 3) & ~3);
    p.slot_bytes = p.off_ovf + ((2 * K1L_OVF + 3) & ~3);
  } else {
    p.off_cnt = p.off_rcode + ((rows_max + 3) & ~3);
    p.off_ovf = 0;
    p.slot_bytes = p.off_cnt + (((rows_max + 1) / 2) * 4) + 4;  // + the walker's dummy count dword
  }
  // The walk is bound by the latency of one transition times the number of "rounds" of workgroups the batch needs
  // (instances resident per CU are limited by LDS capacity).  Choose the action-ring chunk length and the workgroups per
  // CU (two overlap one group's staging / flush with the other's walk, one holds a few more instances) that need the
  // fewest rounds; ties go to the longer chunk (fewer barriers), then to two per CU.
  // Packed tables can also run as the wavefront pipeline K1P: ~0.62x the time per transition plus one barrier per chunk
  // (measured at C2: 53 / 56 / 62 ns per transition at ch = 64 / 32 / 16 against K1L's 82), for 6 ch + 16 bytes of
  // rings per instance instead of 2 ch.
  struct Cand { int pipe, ch; };
  const Cand cands[] = {{0, 256}, {0, 128}, {0, 112}, {0, 64}, {1, 64}, {1, 32}, {1, 16}};
  for (const Cand& cd : cands) {
    if ((cd.pipe && !c.pipe_ok) || (k.pipe >= 0 && cd.pipe != k.pipe)) continue;
    const int pi = p.slot_bytes + (cd.pipe ? 2 * K1P_ACT_STRIDE(cd.ch) + 2 * K1P_TR_STRIDE(cd.ch) : 2 * cd.ch);
    const int g1 = std::min<int>(64, (kLdsBudget - K1L_FIXED) / pi);
    // K1P: one workgroup per CU.  Two (26 + 26 instances at C2) need <= 128 VGPRs to be co-resident at all (it has
    // 145: the "1.8x slower" of the first trial was simply one resident group at a time); forced to 128 it spills, and
    // two resident groups gain nothing -- they run in lockstep, so their flushes coincide, and a CU holds the same 52
    // instances either way.
    const int g2 = cd.pipe ? 0 : std::min<int>(64, (kLdsBudget / 2 - K1L_FIXED) / pi);
    for (int per_cu : {2, 1}) {
      const int g = per_cu == 2 ? g2 : g1;
      if (g < (per_cu == 2 ? 12 : 8)) continue;
      const EvenGroups eg = even_groups(in.B, g, (int64_t)in.cus * per_cu);
      const double per_step = cd.pipe ? 0.62 * (1.0 + 3.5 / cd.ch) : 1.0 + 2.0 / cd.ch;
      const double cost = (double)eg.rounds * per_step;
      if (c.cost >= 0 && cost >= c.cost) continue;
      c.cost = cost;
      p.ch = cd.ch;
      p.pipe = cd.pipe;
      p.G = k.k1l_G ? std::min(g, k.k1l_G) : eg.G;
      c.G1 = g1;
      c.G2 = g2;
      c.per_cu = per_cu;
    }
  }
  c.ok = c.cost >= 0;
  if (p.pipe) p.code_shift = c.succ_bits + 1;
  p.n_codes = (int)t.vals.size();
  return c;
}

// The K1L / K1P images of the tables (after every other planner has read them): packed successor words, and 16 bytes
// of slack in front of and behind both element arrays -- the staging loads are 16-byte wide from the aligned-down
// address of a group's first element.
inline void k1lp_images(const LdsPlan& p, int A, DetTables* t) {
  if (p.code_shift)
    for (size_t r = 0; r < t->next16.size(); ++r)
      t->next16[r] = (uint16_t)((t->next16[r] * A * (p.pipe ? 2 : 1)) | (t->codes[r] << p.code_shift));
  t->next16.insert(t->next16.begin(), 8, 0);
  t->next16.insert(t->next16.end(), 8, 0);
  t->codes.insert(t->codes.begin(), 16, 0);
  t->codes.insert(t->codes.end(), 16, 0);
}

// ---- K1T (cmdp_k1t.h) ----------------------------------------------------------------------------------------------
// When every instance's packed words are, state by state, instance 0's words or their swap (A = 2; seeds of a family
// whose structure does not depend on the seed only permute the actions), the workgroup keeps ONE table and a swap bit per
// state and instance: 2-3 x the instances per CU.  K1T packs its own words -- successor row base as a byte offset |
// reward code above it, K1P's format -- whichever of K1L / K1P was planned: small instances plan onto two K1L workgroups
// per CU, and K1T still beats that.
struct K1tChoice {
  bool ok = false;
  bool autos = false;               // the automatic choice: fewer rounds x time than K1L / K1P
  TmplPlan q{};
  int cap = 0;                      // LDS capacity in instances per workgroup at the chosen chunk length
  std::vector<uint16_t> words;      // [tmpl_bytes / 2] the template: instance 0's words
  std::vector<uint8_t> swap_bits;   // [B][mask_bytes]
};

inline K1tChoice plan_k1t(const PlanInput& in, const DetTables& t, const K1lpChoice& lp, const PlanKnobs& k) {
  K1tChoice c;
  if (!lp.ok || !lp.pipe_ok || in.A != 2) return c;
  const int S = in.max_S, rws = S * 2, cs = lp.succ_bits + 1;
  TmplPlan& q = c.q;
  q.rows = rws;
  q.tmpl_bytes = (rws * 2 + 15) & ~15;
  q.mask_bytes = ((S + 7) / 8 + 3) & ~3;
  q.off_cnt = q.mask_bytes;
  q.off_ovf = q.off_cnt + ((rws + 4 + 3) & ~3);
  // two spare entries: the counts wavefront stores ovf[n_ovf] unconditionally before it knows whether a counter
  // wrapped (branch-free), so with the list full the store must still land inside the instance's own slot
  q.slot_bytes = q.off_ovf + ((2 * (K1T_OVF + 2) + 3) & ~3);
  if (((q.slot_bytes / 4) & 1) == 0) q.slot_bytes += 4;   // odd dword stride: the lanes' slots start on different banks
  q.n_codes = lp.p.n_codes;
  q.code_shift = cs;
  q.debug = k.k1t_debug;
  if (q.debug) std::fprintf(stderr, "libcmdp: CMDP_K1T_DEBUG=%d switches stages of k_rollout_tmpl off -- results are INVALID (timing experiments only)\n", q.debug);
  auto word = [&](int64_t r) { return (uint16_t)((t.next16[(size_t)r] * 4) | (t.codes[(size_t)r] << cs)); };
  c.swap_bits.assign((size_t)in.B * q.mask_bytes, 0);
  for (int b = 0; b < in.B; ++b)
    for (int s = 0; s < S; ++s) {
      const int64_t r = (int64_t)b * rws + 2 * s;
      const uint16_t w0 = word(r), w1 = word(r + 1), t0 = word(2 * s), t1 = word(2 * s + 1);
      if (w0 == t0 && w1 == t1) continue;
      if (w0 != t1 || w1 != t0) return c;   // not an action permutation of instance 0
      c.swap_bits[(size_t)b * q.mask_bytes + (s >> 3)] |= (uint8_t)(1u << (s & 7));
    }
  // chunk length and instances per workgroup: fewest rounds x time per transition (K1T's chain carries ~4 more dependent
  // instructions than K1P's: ~1.3 x its time per transition), as for K1L / K1P
  double best = -1.0;
  for (int ch : {64, 32, 16}) {
    if (k.k1t_ch && ch != k.k1t_ch) continue;
    const int per = q.slot_bytes + 2 * K1P_ACT_STRIDE(ch) + 2 * K1P_TR_STRIDE(ch);
    const int cap = std::min<int>(128, (kLdsBudget - K1T_FIXED - q.tmpl_bytes) / per);
    if (cap < 16) continue;
    const EvenGroups eg = even_groups(in.B, cap, in.cus);
    const double cost = (double)eg.rounds * 1.3 * 0.62 * (1.0 + 3.5 / ch);
    if (best >= 0 && cost >= best) continue;
    best = cost;
    q.ch = ch;
    q.G = k.k1t_G ? std::min(cap, k.k1t_G) : eg.G;
    c.cap = cap;
  }
  if (best < 0) return c;
  c.ok = true;
  c.autos = best < lp.cost;
  c.words.resize((size_t)q.tmpl_bytes / 2, 0);
  for (int r = 0; r < rws; ++r) c.words[(size_t)r] = word(r);
  return c;
}

// ---- K1U (cmdp_k1u.h) ----------------------------------------------------------------------------------------------
// K1T's chain with the visit counts histogrammed from an HBM trace: an instance keeps only its swap bits and the rings in
// LDS, up to 256 instances per workgroup.  Taken automatically when that saves a round of workgroups over K1T (config C2:
// one round of 256 instead of two of 128); otherwise the histogram pass is pure overhead and K1T stays.  (The histogram
// of one launch under the chain of the next, on a second stream, was measured at C2 and LOST: co-resident, the chain
// kernel slows from 2.2 to 3.0 ms -- the histogram's LDS atomics sit in the same in-order LDS pipeline as the chain's
// dependent reads -- 3.25 ms per step against 3.00 one after the other; the two kernels run on the handle's stream.)
struct K1uChoice {
  bool ok = false, autos = false;
  K1uPlan u{};
  int cap = 0;   // LDS capacity in instances per workgroup
};

inline K1uChoice plan_k1u(const PlanInput& in, const K1tChoice& kt, const PlanKnobs& k) {
  K1uChoice c;
  if (!kt.ok) return c;
  const TmplPlan& q = kt.q;
  K1uPlan& u = c.u;
  u.rows = q.rows; u.tmpl_bytes = q.tmpl_bytes; u.mask_bytes = q.mask_bytes;
  u.slot_bytes = q.mask_bytes + ((((q.mask_bytes / 4) & 1) == 0) ? 4 : 0);
  u.n_codes = q.n_codes; u.code_shift = q.code_shift;
  u.pack10 = u.rows <= 1024 ? 1 : 0;
  // chunk length: one barrier per chunk (measured at C2: 2.20 ms per launch at 32 transitions, 2.06 ms at 64)
  u.ch = u.pack10 ? 72 : 64;
  const int per = u.slot_bytes + 2 * K1P_ACT_STRIDE(u.ch) + 2 * K1P_TR_STRIDE(u.ch);
  const int cap = std::min<int>(256, (kLdsBudget - K1U_FIXED - u.tmpl_bytes) / per);
  // (the histogram kernel's workgroup: its counters and its static arrays -- without the latter 638 and 639 states were
  // planned and every launch of theirs failed)
  if (cap < 64 || k1h_lds_bytes(in.max_S, 64) + K1H_STATIC_BYTES(64) > (size_t)kLdsBudget) return c;
  const EvenGroups eg = even_groups(in.B, cap, in.cus);
  u.G = k.k1u_G ? std::min(cap, k.k1u_G) : eg.G;
  c.cap = cap;
  c.ok = true;
  c.autos = kt.autos && eg.rounds < even_groups(in.B, q.G, in.cus).rounds;
  return c;
}

// ---- K1E (cmdp_k1e.h) ----------------------------------------------------------------------------------------------
// Episodic batches with two actions and at most four distinct rewards walk their EPISODES in parallel (private
// {successor word | count} tables of 32 instances per workgroup): throughput- instead of latency-bound, and the tables
// need not be action-permuted copies of one MDP.  It reads the K1L / K1P reward values: plan it only when they exist.
// The PAIR plan of a K1E batch with an even horizon (cmdp_k1e_pair.h): one table row per (even-time state s, actions a0 a1).
// E is the set of states an instance can be in at an even in-episode time t < H: breadth-first search from its start state
// over both actions, two transitions a hop, fewer than H / 2 hops (a state is expanded once, at the hop it is first found
// at: what a later occurrence reaches within the horizon the first one reaches too).  The states of E get compact indices
// in the order they are found, so the start state has index 0.  Pair q = a0 | a1 << 1 of the state with index x:
//   word = index(s'') << 7 | code(s, a0) | code(s', a1) << 2,   s' = next(s, a0), s'' = next(s', a1);
// the successor field is 0 where s'' is not in E (only after the last pair of an episode: never followed).  Shifting the four
// code bits of pair j in at bits 4 j gives the code-word layout of the single walk (step j at bits 2 j).
struct K1ePairChoice {
  bool ok = false;
  int SP2 = 0;                    // rows of an image: a power of two >= 32 and >= every instance's |E|
  int ash2 = 0;                   // log2 of an image's bytes: 7 + log2(SP2)
  int n_even = 0;                 // the largest |E|
  int pgdw = 0;                   // dwords of a group's image in HBM: 2 * SP2 * 32
  std::vector<int32_t> n_even_of; // [B] |E|
  std::vector<int32_t> index;     // [B][S] compact index of a state, -1 outside E
  std::vector<uint16_t> inv;      // [B][SP2] state of a compact index (0 past |E|)
  std::vector<uint16_t> words;    // [B][SP2][4] the pair words, q = a0 | a1 << 1
  std::vector<uint32_t> ptab;     // [group of 32][pgdw]: dword (a1 * SP2 + x) * 32 + i = word(x, a0 = 0, a1) | word(x, 1, a1) << 16
};

struct K1eChoice {
  bool ok = false;
  K1ePlan e{};
  std::vector<uint32_t> etab;   // [group of 32][gdw]
  K1ePairChoice pair;           // e.ash2 / e.pgdw are set when pair.ok
};

// LDS of the pair form: four images of SP2 rows x 32 instances x 4 B, then the single form's rings
inline size_t k1e_pair_lds_bytes(const K1ePlan& e, int ash2) { return ((size_t)4 << ash2) + k1e_ring_bytes(e); }

inline K1ePairChoice plan_k1e_pair(const PlanInput& in, const DetTables& t, const K1ePlan& e) {
  K1ePairChoice c;
  if (in.H <= 0 || (in.H & 1)) return c;
  const int S = in.max_S, B = in.B, hops = in.H / 2;
  c.n_even_of.assign((size_t)B, 0);
  c.index.assign((size_t)B * S, -1);
  std::vector<int32_t> order, depth;
  std::vector<std::vector<int32_t>> found((size_t)B);
  for (int b = 0; b < B; ++b) {
    int32_t* idx = c.index.data() + (size_t)b * S;
    const int32_t s0 = in.d->start_state[in.d->start_off[b]];
    if (s0 < 0 || s0 >= S) return c;
    order.assign(1, s0);
    depth.assign(1, 0);
    idx[s0] = 0;
    for (size_t k = 0; k < order.size(); ++k) {
      if (depth[k] + 1 >= hops) continue;   // its successors are past the last even time below H
      for (int q = 0; q < 4; ++q) {
        const int32_t s1 = t.next16[(size_t)2 * ((size_t)b * S + order[k]) + (q & 1)];
        const int32_t s2 = t.next16[(size_t)2 * ((size_t)b * S + s1) + (q >> 1)];
        if (idx[s2] < 0) {
          idx[s2] = (int32_t)order.size();
          order.push_back(s2);
          depth.push_back(depth[k] + 1);
        }
      }
    }
    c.n_even_of[(size_t)b] = (int32_t)order.size();
    c.n_even = std::max(c.n_even, (int)order.size());
    found[(size_t)b] = order;
  }
  c.SP2 = 32;
  c.ash2 = 12;
  while (c.SP2 < c.n_even) { c.SP2 <<= 1; ++c.ash2; }
  // the successor field of a 16-bit word is bits 15:7 (K1E_SMASK): at most 512 rows
  if (c.SP2 > 512 || k1e_pair_lds_bytes(e, c.ash2) > (size_t)kLdsBudget) return c;
  if (((size_t)4 << c.ash2) % ((size_t)e.ring_blocks * 512) != 0) return c;   // the rings are aligned as k1e_ring_aligned requires
  c.pgdw = 2 * c.SP2 * K1E_NI;
  const int64_t groups = ((int64_t)B + K1E_NI - 1) / K1E_NI;
  c.inv.assign((size_t)B * c.SP2, 0);
  c.words.assign((size_t)B * c.SP2 * 4, 0);
  c.ptab.assign((size_t)groups * (size_t)c.pgdw, 0u);
  for (int b = 0; b < B; ++b) {
    const int32_t* idx = c.index.data() + (size_t)b * S;
    const std::vector<int32_t>& ord = found[(size_t)b];
    uint32_t* img = c.ptab.data() + (size_t)(b / K1E_NI) * (size_t)c.pgdw + (size_t)(b % K1E_NI);
    for (size_t x = 0; x < ord.size(); ++x) {
      c.inv[(size_t)b * c.SP2 + x] = (uint16_t)ord[x];
      uint16_t* w = c.words.data() + ((size_t)b * c.SP2 + x) * 4;
      for (int q = 0; q < 4; ++q) {
        const size_t r1 = (size_t)2 * ((size_t)b * S + ord[x]) + (q & 1);
        const size_t r2 = (size_t)2 * ((size_t)b * S + t.next16[r1]) + (q >> 1);
        const int32_t x2 = idx[t.next16[r2]];
        w[q] = (uint16_t)(((uint32_t)(x2 < 0 ? 0 : x2) << 7) | t.codes[r1] | ((uint32_t)t.codes[r2] << 2));
      }
      for (int a1 = 0; a1 < 2; ++a1)
        img[((size_t)a1 * c.SP2 + x) * K1E_NI] = (uint32_t)w[2 * a1] | ((uint32_t)w[2 * a1 + 1] << 16);
    }
  }
  c.ok = true;
  return c;
}

inline K1eChoice plan_k1e(const PlanInput& in, const DetTables& t, const PlanKnobs& k) {
  K1eChoice c;
  if (in.A != 2 || in.H <= 0 || in.H >= (1 << 14) || t.vals.size() > 4) return c;
  const int S = in.max_S;
  K1ePlan& e = c.e;
  e.S = S;
  e.H = in.H;
  e.n_codes = (int)t.vals.size();
  e.nch = (in.H + 31) / 32;
  // a wavefront's ring: the blocks the eight episodes of a round can touch (cmdp_k1e.h)
  const int64_t round_bits = (int64_t)2 * K1E_EPL * in.H;
  int rb = 2;
  while (rb < (round_bits + 126) / 128 + 1) rb <<= 1;
  e.ring_blocks = rb;
  e.ash = 12;   // (at least 32 padded states: an action's image then holds whole rounds of the workgroup's 1024 lanes)
  while ((1 << (e.ash - 7)) < S) ++e.ash;   // action stride: states padded to a power of two, 128 B per state
  e.debug = k.k1e_debug;
  // (bit 16 only sends the interior rounds the general way: results stay valid)
  if (e.debug & 15) std::fprintf(stderr, "libcmdp: CMDP_K1E_DEBUG=%d switches phases of k_rollout_epi off -- results are INVALID (timing experiments only)\n", e.debug);
  e.gdw = (int32_t)((((int64_t)S * K1E_NI + K1E_THREADS - 1) / K1E_THREADS) * K1E_THREADS);   // a group's image: whole rounds of the workgroup's loads
  if (S > 512 || k1e_lds_bytes(e) > (size_t)kLdsBudget) return c;
  // interleaved by instance like the LDS image: [group of 32][state][instance in group]
  const int64_t groups = ((int64_t)in.B + K1E_NI - 1) / K1E_NI;
  c.etab.assign((size_t)groups * (size_t)e.gdw, 0u);
  auto word = [&](int64_t r) { return ((uint32_t)t.next16[(size_t)r] << 7) | t.codes[(size_t)r]; };
  for (int64_t b = 0; b < in.B; ++b)
    for (int s = 0; s < S; ++s) {
      const int64_t r = 2 * (b * S + s);
      c.etab[(size_t)(b / K1E_NI) * (size_t)e.gdw + (size_t)s * K1E_NI + (size_t)(b % K1E_NI)] = word(r) | (word(r + 1) << 16);
    }
  c.ok = true;
  c.pair = plan_k1e_pair(in, t, e);
  if (c.pair.ok) { e.ash2 = c.pair.ash2; e.pgdw = c.pair.pgdw; }
  return c;
}

// cmdp_k1e_pair_plan / cmdp_k1e_pair_plan_desc: the fields in the order include/cmdp.h gives (last_form: 0 no K1E launch yet,
// 1 the single form, 2 the pair form); all 0 but last_form when the batch has no pair plan
inline void k1e_pair_plan_report(bool ok, const K1ePlan& e, int SP2, int n_even, int last_form, int32_t out[CMDP_K1E_PAIR_PLAN_FIELDS]) {
  std::fill(out, out + CMDP_K1E_PAIR_PLAN_FIELDS, 0);
  out[5] = last_form;
  if (!ok) return;
  const int32_t v[5] = {1, e.H, SP2, n_even, (int32_t)k1e_pair_lds_bytes(e, e.ash2)};
  std::copy(v, v + 5, out);
}
static_assert(CMDP_K1E_PAIR_PLAN_FIELDS == 6, "k1e_pair_plan_report writes 6 fields");

// ---- K1S (cmdp_k1s.h) ----------------------------------------------------------------------------------------------
// Compresses the sampler tables of a batch with stochastic dynamics into shared cumulative-probability patterns,
// per-state successor sets and 4-bit entry codes, and sizes the LDS plan.  Not eligible (the batch then takes K1)
// whenever a limit of the format is exceeded.  The caller has checked Philox mode, the CSR layout and that the rewards
// are the table's values.
struct K1sChoice {
  bool ok = false;
  K1sPlan p{};
  size_t bytes = 0;                         // LDS of a workgroup
  std::vector<uint8_t> shape8;              // [R] shape of every row, when shape_bytes == 1
  std::vector<uint16_t> shape16;            // ... when shape_bytes == 2
  std::vector<uint4> dict;                  // [n_shapes]
  std::vector<uint16_t> sets;               // [NS][U]
  std::vector<uint8_t> rc;                  // [NS] or [R]
  std::vector<double> patterns, rvals;
};

inline K1sChoice plan_k1s(const PlanInput& in, const PlanKnobs& knobs) {
  K1sChoice c;
  const cmdp_desc* d = in.d;
  const int B = in.B, A = in.A;
  const int64_t S0 = in.max_S;   // slots are sized for the largest instance
  if (S0 * A >= 65536 || S0 < 1) return c;
  const int64_t NS = d->state_off[B], R = NS * A, E = d->sp_ptr[R];
  if (d->sp_rkind)
    for (int64_t e = 0; e < E; ++e)
      if (d->sp_rkind[e] != 0) return c;   // reward means of Beta entries: K1 reports them
  std::vector<int> ecode;   // reward code of every entry
  if (!reward_codes(E, [&](int64_t e) { return d->sp_reward[e]; }, &c.rvals, &ecode)) return c;
  // cumulative-probability pattern of a row (entries lo .. lo + n) -> id; -1 when 64 are taken
  std::map<std::vector<uint64_t>, int> pat_of;
  auto pattern_id = [&](int64_t lo, int n) {
    std::vector<uint64_t> key((size_t)n);
    std::memcpy(key.data(), d->sp_cum + lo, sizeof(double) * (size_t)n);
    auto it = pat_of.find(key);
    if (it != pat_of.end()) return it->second;
    if (pat_of.size() == 64) return -1;
    for (int k = 0; k < K1S_MAXE; ++k)
      c.patterns.push_back(k < n - 1 ? d->sp_cum[lo + k] : std::numeric_limits<double>::infinity());
    c.patterns.push_back(d->sp_cum[lo + n - 1]);
    return pat_of.emplace(key, (int)pat_of.size()).first->second;
  };
  // slot of successor nx in a state's successor set; -1 when 16 are taken
  auto slot_of = [](std::vector<int32_t>& set, int32_t nx) {
    for (size_t j = 0; j < set.size(); ++j)
      if (set[j] == nx) return (int)j;
    if (set.size() == 16) return -1;
    set.push_back(nx);
    return (int)set.size() - 1;
  };
  // is the reward a function of the successor state alone / of the row alone?
  bool by_state = true, by_row = true;
  auto note = [](int& slot, int code, bool& same) {
    if (slot < 0) slot = code;
    else if (slot != code) same = false;
  };
  std::vector<std::vector<int32_t>> sets((size_t)NS);
  std::vector<unsigned long long> words((size_t)R, 0);
  std::vector<uint8_t> pat_ids((size_t)R, 0);
  std::vector<int> rc_state((size_t)NS, -1), rc_row((size_t)R, -1);
  int U = 1;
  for (int b = 0; b < B; ++b) {
    const int64_t so = d->state_off[b];
    for (int64_t r = so * A; r < d->state_off[b + 1] * A; ++r) {
      const int64_t lo = d->sp_ptr[r];
      const int n = (int)(d->sp_ptr[r + 1] - lo);
      if (n < 1 || n > K1S_MAXE) return c;
      const int pat = pattern_id(lo, n);
      if (pat < 0) return c;
      auto& set = sets[(size_t)(r / A)];
      unsigned long long word = 0;
      for (int k = 0; k < n; ++k) {
        const int32_t nx = d->sp_next[lo + k];
        const int idx = slot_of(set, nx);
        if (idx < 0) return c;
        word |= (unsigned long long)idx << (4 * k);
        note(rc_state[(size_t)(so + nx)], ecode[(size_t)(lo + k)], by_state);
        note(rc_row[(size_t)r], ecode[(size_t)(lo + k)], by_row);
      }
      words[(size_t)r] = word;
      pat_ids[(size_t)r] = (uint8_t)pat;
      U = std::max(U, (int)set.size());
    }
    if (d->start_off[b + 1] - d->start_off[b] > K1S_MAXSTART) return c;
  }
  if (!by_state && !by_row) return c;
  // row shapes: (pattern, word) -- and, when the reward is a function of the row rather than of the successor state, the
  // row's reward code, so that the shape's dictionary entry carries it
  std::map<std::tuple<int, unsigned long long, int>, int> shape_of;
  std::vector<uint16_t> shape((size_t)R, 0);
  for (int64_t r = 0; r < R; ++r) {
    const int rcd = by_state ? 0 : std::max(0, rc_row[(size_t)r]);
    const auto key = std::make_tuple((int)pat_ids[(size_t)r], words[(size_t)r], rcd);
    auto sh = shape_of.find(key);
    if (sh == shape_of.end()) {
      if (c.dict.size() == 65535) return c;
      sh = shape_of.emplace(key, (int)c.dict.size()).first;
      c.dict.push_back(make_uint4((uint32_t)words[(size_t)r], (uint32_t)(words[(size_t)r] >> 32), (uint32_t)pat_ids[(size_t)r], (uint32_t)rcd));
    }
    shape[(size_t)r] = (uint16_t)sh->second;
  }
  K1sPlan& p = c.p;
  p.S = (int)S0; p.rows = (int)S0 * A; p.U = U; p.n_pat = (int)pat_of.size(); p.n_codes = (int)c.rvals.size();
  p.reward_mode = by_state ? 0 : 1;
  p.ch = 32;
  p.n_shapes = (int)c.dict.size();
  p.shape_bytes = p.n_shapes <= 256 ? 1 : 2;
  auto up8 = [](int x) { return (x + 7) & ~7; };
  p.off_cnt = up8(p.rows * p.shape_bytes);
  p.off_ovf = up8(p.off_cnt + p.rows);
  p.off_sets = up8(p.off_ovf + 2 * (K1S_OVF + 2));
  // reward code of the arrival state in the top four bits of its successor-set entries (no separate look-up on the walk)
  // when both fit sixteen bits; per-row codes travel in the shape's dictionary entry: no per-instance code table then
  p.rc_packed = (by_state && S0 <= 4096 && c.rvals.size() <= 16) ? 1 : 0;
  p.off_rc = up8(p.off_sets + 2 * p.S * U);
  p.off_start = up8(p.off_rc + ((by_state && !p.rc_packed) ? p.S : 0));
  p.slot_bytes = up8(p.off_start + 48 + 8 * K1S_MAXSTART + 4 * K1S_MAXSTART);
  const size_t fixed = k1s_fixed_bytes(p.n_pat, p.n_shapes) + 64;
  const size_t per = (size_t)p.slot_bytes + k1s_ring_bytes(p.ch);
  if (fixed + 4 * per > (size_t)kLdsBudget) return c;   // fewer than four instances per CU: not worth it
  const int cap = (int)std::min<size_t>(64, ((size_t)kLdsBudget - fixed) / per);
  p.G = knobs.k1s_G ? std::min(cap, knobs.k1s_G) : even_groups(B, cap, in.cus).G;
  // walker wavefronts and lanes per instance in them.  Round 2 (ONE walker wavefront; FrozenLake-20 / MiniGrid-8 /
  // DeepSea-20 with p_rand, G = 8 / 11 / 22): teams of 8 (two entries per lane, two ballots) +19 %; teams of 4 (four
  // ballots) -3 %; of 2 -31 % against a lane per instance counting its 16 entries itself -- so teams only where a lane
  // gets at most two entries.  With up to four walker wavefronts a wavefront has a quarter of the instances and its teams
  // are larger.
  p.nw = p.G >= 4 ? 4 : (p.G >= 2 ? 2 : 1);
  p.gw = (p.G + p.nw - 1) / p.nw;
  p.team = p.gw <= 4 ? 16 : (p.gw <= 8 ? 8 : 1);
  c.sets.assign((size_t)NS * U, 0);
  for (int b = 0; b < B; ++b) {
    const int64_t so = d->state_off[b];
    for (int64_t s = so; s < d->state_off[b + 1]; ++s)
      for (size_t j = 0; j < sets[(size_t)s].size(); ++j) {
        const int32_t nx = sets[(size_t)s][j];
        const int code = p.rc_packed ? std::max(0, rc_state[(size_t)(so + nx)]) : 0;
        c.sets[(size_t)s * U + j] = (uint16_t)(nx | (code << 12));
      }
  }
  c.rc.resize(by_state ? (size_t)NS : (size_t)R);
  for (size_t i = 0; i < c.rc.size(); ++i) c.rc[i] = (uint8_t)std::max(0, by_state ? rc_state[i] : rc_row[i]);
  if (p.shape_bytes == 1) c.shape8.assign(shape.begin(), shape.end());
  else c.shape16 = std::move(shape);
  c.bytes = fixed + (size_t)p.G * per + 16;
  c.ok = true;
  return c;
}

// ---- cmdp_det_plan / cmdp_det_plan_desc: the plans of the deterministic kernels, as tests read them ----------------
// The compiled form a launch takes.  launch_k1lp / launch_k1u branch on these very functions, and the plan report names
// what they return.
enum { K1LP_FORM_UNPACKED = 0, K1LP_FORM_PACKED = 1, K1LP_FORM_PIPE = 2 };
inline int k1lp_form(const LdsPlan& p) { return p.pipe ? K1LP_FORM_PIPE : (p.code_shift ? K1LP_FORM_PACKED : K1LP_FORM_UNPACKED); }
enum { K1U_FORM_PACK10 = 0, K1U_FORM_WIDE = 1 };
inline int k1u_form(const K1uPlan& u) { return u.pack10 ? K1U_FORM_PACK10 : K1U_FORM_WIDE; }

struct DetPlans {
  bool lds_ok = false, tmpl_ok = false, tmpl_auto = false, k1u_ok = false, k1u_auto = false;
  LdsPlan lp{};
  int succ_bits = 0, per_cu = 0, lp_cap = 0;   // of the chosen K1L / K1P candidate
  TmplPlan kt{};
  int kt_cap = 0;
  K1uPlan ku{};
  int ku_cap = 0, max_S = 0;
};

inline DetPlans det_plans_of(const K1lpChoice& lp, const K1tChoice& kt, const K1uChoice& ku, int max_S) {
  DetPlans d;
  d.lds_ok = lp.ok; d.lp = lp.p; d.succ_bits = lp.succ_bits; d.per_cu = lp.per_cu; d.lp_cap = lp.per_cu == 2 ? lp.G2 : lp.G1;
  d.tmpl_ok = kt.ok; d.tmpl_auto = kt.autos; d.kt = kt.q; d.kt_cap = kt.cap;
  d.k1u_ok = ku.ok; d.k1u_auto = ku.autos; d.ku = ku.u; d.ku_cap = ku.cap; d.max_S = max_S;
  return d;
}

// the fields in the order include/cmdp.h gives; those of a kernel the batch is not eligible for are 0
inline void det_plan_report(const DetPlans& d, int32_t out[CMDP_DET_PLAN_FIELDS]) {
  std::fill(out, out + CMDP_DET_PLAN_FIELDS, 0);
  if (d.lds_ok) {
    const LdsPlan& p = d.lp;
    const int32_t v[13] = {1, p.pipe, p.code_shift ? 1 : 0, p.code_shift, d.succ_bits, p.n_codes, p.ch, p.G, d.per_cu, d.lp_cap,
                           p.slot_bytes, (int32_t)k1l_lds_bytes(p, p.G), k1lp_form(p)};
    std::copy(v, v + 13, out);
  }
  if (d.lds_ok && d.tmpl_ok) {
    const TmplPlan& q = d.kt;
    const int32_t v[8] = {1, d.tmpl_auto ? 1 : 0, q.ch, q.G, d.kt_cap, q.slot_bytes, q.tmpl_bytes, (int32_t)k1t_lds_bytes(q, q.G)};
    std::copy(v, v + 8, out + 13);
  }
  if (d.lds_ok && d.k1u_ok) {
    const K1uPlan& u = d.ku;
    const int32_t v[9] = {1, d.k1u_auto ? 1 : 0, u.pack10, u.ch, u.G, d.ku_cap, (int32_t)k1u_lds_bytes(u, u.G),
                          (int32_t)(k1h_lds_bytes(d.max_S, 64) + K1H_STATIC_BYTES(64)), k1u_form(u)};
    std::copy(v, v + 9, out + 21);
  }
}
static_assert(CMDP_DET_PLAN_FIELDS == 30, "det_plan_report writes 13 + 8 + 9 fields");
