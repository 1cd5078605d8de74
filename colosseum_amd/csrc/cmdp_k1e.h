// cmdp_k1e.h -- K1E k_rollout_epi + k_reward_scan: the EPISODE-PARALLEL random-policy rollout (round 4; config C2's kernel).
//
// Every rollout kernel before this one (K1 .. K1U) walks ONE dependent chain per instance, so a launch is
// (resident chains) x (transitions) x (latency of a chain's dependent LDS read) and the chip idles behind that latency
// (K1U: VALU issue 46 %, LDS pipe 36 %, HBM 16 %).  Under the random policy the episodes of an episodic instance are
// INDEPENDENT of each other:
//   * reset() returns to a start state that depends on nothing the episode did (reference colosseum/mdp/base.py:1268-1277;
//     eligible batches have one start state),
//   * an episode lasts exactly H steps (`h >= H`, base.py:1310-1317),
//   * the action of transition n is a pure function of (instance key, n): the counter-based Philox stream of domain 2
//     (reference RandomActor, colosseum/agent/actors/random.py:34-47, is a seeded stream as well).
// So transition n0 + e H + j of an instance can be walked without its predecessors: lane = (instance, episode), a chain is
// H steps long, and a launch of 65 536 x 30 000 transitions is 65.5 M independent chains of 30 instead of 65 536 of 30 000.
// The kernel is then bound by THROUGHPUT, not by latency -- of two pipes at once (tools/calib/lds_atomic_rate.hip,
// tools/calib/valu_int_rate.hip; profiles/r04_lds_atomic_rate.txt): a wave64 ds_add_rtn_u32 occupies a CU's LDS pipe for 4.3
// cycles (a ds_read_b32 for 1.1), the step's integer VOP3 instructions a SIMD for 4.4-4.8 cycles each; the step alone, in a
// loop that does nothing else, runs at 22.4 cycles per wave-transition per SIMD (5.6 per CU).
//
// k_rollout_epi -- ONE 1024-thread workgroup per CU, each owning groups of NI = 32 instances one after the other:
//   LDS   every instance of the group has a PRIVATE table of S x 2 dwords {visit count : 16 | successor word : 16}, and the 32
//         tables are INTERLEAVED dword by dword: row (s, a) of instance i lives at byte a * 2^ASH + s * 128 + 4 i.  The 32
//         lanes of an LDS lane group are the 32 instances, so lane i only ever touches bank i: every access of the walk is
//         bank-conflict-free whatever the states are (a slot per instance measured 76 % of the LDS cycles as conflicts: 32
//         random dwords over 32 banks collide 3.5-fold), and no two lanes ever add to the same dword.  The successor word
//         is s' << 7 | reward code: the address of the next row is ONE v_and_or_b32, (word & 0xff80) | (action << ASH | 4 i).
//   step  v_add_co (next action bit -> VCC) . v_cndmask (the lane's base in that action's image) . v_and_or (address) .
//         ds_add_rtn_u32 . v_alignbit (reward code into the episode's code word): the returning atomic IS the table read -- it
//         counts the row the chain LEAVES and hands back its successor word: 4 VALU + 1 LDS instruction per transition,
//         spelled out in inline asm (left alone the compiler picks v_bfe . v_and . v_lshlrev . v_or3, five with the
//         v_alignbit; v_bfe . v_lshl_or . v_and_or is four but two of them VOP3 where v_add_co . v_cndmask are VOP2: 25.2 /
//         22.4 / 20.9 cycles per wave-transition per SIMD in isolation).  An idle chain (no episode left for it) walks from
//         state 0 under action 0 and adds ZERO.
//   lanes lane = (instance l & 31, half l >> 5).  Wavefront w owns a CONTIGUOUS range of the segment's episodes and walks it
//         eight at a time (a round): half s, chain c in {0 .. 3} walks episode 8 (R w + r) + 4 s + c -- four independent
//         chains per lane, their atomics issued together.
//   bits  the action bits of a round come from the wavefront's OWN ring of Philox blocks in LDS (interleaved like the
//         tables): lanes 0-31 make one block of their instance, lanes 32-63 the next; consecutive rounds continue in the
//         stream, so every block is made once.  A chain fetches its 32 bits with one funnel shift.  Every bit of every block
//         is used (cmdp_device.h: the packed domain-2 stream): 0.8 VALU instructions per transition instead of the 25 a whole
//         block per four one-bit actions cost K1U.  LDS operations of one wavefront are performed in order, so the walk of a
//         group needs NO workgroup barrier (a ring shared by the workgroup needed two per 128 episodes: 0.04 ms of 0.6).
//   inner a round whose eight episodes are all full, none the segment's first and none with its last transition (123 of a
//         wavefront's 125 working rounds at 30 000 transitions of H = 30) is INTERIOR (k1e_round_interior, wave-uniform, SALU):
//         it takes a path of its own that asks nothing per chain -- constant start word and count, the four chains' bit
//         windows fetched by eight ring reads behind ONE wait (a wavefront's ring starts at a multiple of its own size --
//         k1e_ring_aligned, checked by the host -- so a ring address is one v_and_or_b32, and chain c's stream position is
//         chain 0's plus a scalar: 7 VALU instructions per chain), the code words stored unpredicated through scalar bases
//         and one 32-bit lane offset, no partial episode, no last transition.  At H = 30 per lane and round: bit fetch 29,
//         step loops 480, code words 15 and 4 stores, entry and clearing 22, plus the round's Philox block.  Every other
//         round takes the general path; CMDP_K1E_DEBUG=16 sends all of them there (results unchanged).
//   next  the table image of the workgroup's NEXT group is loaded into registers during the last round of the walk (and the
//         instance scalars under the flush): the staging's HBM round trips run under the walk.
//   flush the table dwords hold DEPARTURE counts; they are added to a launch-spanning departure image in HBM (layout of the
//         LDS image) by returnless 64-bit atomics -- no read-modify-write round trip, the workgroup goes on at once.  The
//         reference counts the ARRIVAL state under the action taken (base.py:1302-1303): a linear function of the departure
//         counts, formed by k_epi_fold when somebody needs the counters.
//   out   the reward codes of an episode (2 bits per step) go to HBM, 8 bytes per (episode, 32-step chunk), layout
//         codes[episode][chunk][instance], and nothing else: the walk is bound by VALU issue, and the steps per code, which
//         only make a tile of the scan cheap, are counted by the scan (the walk once stored them next to the codes: 9 VALU
//         instructions and a 4-byte store per word).  State, in-episode time and the Philox counters are advanced as if the
//         transitions had been taken one by one.
//   bytes LDS per workgroup at DeepSea(30): 131 072 B of tables + 16 x 2 048 B of rings = 163 840 B, the whole CU.  HBM per
//         launch of 65 536 x 30 000 transitions: 122 MB table image in, 524 MB code words out (8 B per episode chunk and
//         instance), 488 MB departure image.
//   pair  k_rollout_epi<1> (cmdp_k1e_pair.h) is a second form of this walk for launches of WHOLE EPISODES WALKED FROM RESET on a
//         batch with an even horizon: one table row per (state at an even in-episode time, action pair), so one step -- one
//         address, one returning atomic, one v_alignbit -- covers TWO transitions.  It writes the same code words and leaves the
//         same state; its counts go to a second departure image, which k_epi_fold folds with this one's.  launch_k1e (cmdp.hip)
//         chooses per launch; everything else takes the form below, k_rollout_epi<0>.
// k_reward_scan -- lane = instance: the float64 reward sum in TRANSITION ORDER from the code words (bit-equal to the
//         oracle's and every other kernel's sequential sum).  It loads the code words in tiles of eight, three tiles in
//         registers.  A PLAIN tile (eight whole single-chunk episodes for every lane of the wavefront: 106 of a wavefront's
//         125 at C2) costs the step counts per code of its eight words, accumulated straight into registers, and one integer
//         advance.  A lane whose advance fails (its sum leaves a binade inside the tile: ~8 tiles per lane at C2) in a tile
//         where only ONE nonzero reward value occurs -- sparse rewards: every such tile of C2 -- takes the single-value path
//         (k1r_single): the order of the steps does not matter then, so the tile's counts are enough, no word is searched.
//         Any other tile, and a lane that fails with two nonzero values present, forms the packed step counts n1 | n2 << 11 |
//         n3 << 22 of each word (k1e_code_counts_few for at most three reward codes, k1e_code_counts for four: one
//         wave-uniform branch per tile) and their prefix sums -- in a plain tile only when some lane of the wavefront needs
//         them; the words a lane has to add step by step are already in its registers.  The lane's arithmetic is
//         __host__ __device__ (K1rLane, k1r_scan) and exported as cmdp_k1e_scan_words / cmdp_k1e_scan_words_ex.
//         No LDS at all and <= 128 VGPRs: k_rollout_epi holds every byte of the CU's LDS and 4 x 96 VGPRs per SIMD, and a
//         wavefront of the scan still fits beside it.
// Results: visit counts, final states, in-episode times, Philox counters and reward sums bit-equal to K1 / K1T / K1U and the
// CPU oracle (tests/test_gpu_parity.py, tests/test_gpu_fullsize.py, tools/stress_k1t.py k1e, tools/fuzz_parity.py).
#pragma once

#define K1E_THREADS 1024
#define K1E_NW (K1E_THREADS / 64)
#define K1E_NI 32                          // instances per workgroup: the 32 lanes of an LDS lane group, one bank each
#define K1E_EPL 4                          // chains (episodes) per lane
#define K1E_EPP (K1E_NW * 2 * K1E_EPL)     // episodes of one instance per round of the whole workgroup (128)
#define K1E_SEG 61440                      // transitions per segment (< 65 536: the 16-bit counts in the table dwords)
#define K1E_SMASK 0xff80u                  // the state field of a successor word (s' << 7; reward code in bits 1:0)

struct K1ePlan {
  int32_t S, H;
  int32_t ash;               // log2 of the action stride in bytes: 7 + log2(SP), SP = states padded to a power of two
  int32_t ring_blocks;       // power of two: Philox blocks of an instance in ONE WAVEFRONT's action-bit ring (the blocks of the eight
                             // episodes the wavefront walks at a time, plus one)
  int32_t n_codes;           // <= 4 distinct reward values (2-bit codes)
  int32_t nch;               // 32-step chunks per episode, ceil(H / 32)
  int32_t n_pass;            // rounds per wavefront in this segment: ceil(episodes / 128)
  int32_t gdw;               // dwords of a group's table image in HBM: S * 32 rounded up to whole rounds of 1024 (the workgroup's
                             // loads and returnless adds need no bounds test; the padding is zero and stays zero)
  int32_t debug;             // CMDP_K1E_DEBUG (timing experiments, results INVALID): 1 no walk, 2 no flush, 4 no Philox, 8 no code stores;
                             // 16 no round is interior (every round takes the general path; results VALID)
  int32_t fast;              // interior rounds take the short path (k1e_round_interior): set per launch, when bit 16 of `debug` is
                             // clear, every byte offset into codes stays below 2^31 (32-bit lane offsets) and the rings are
                             // aligned (k1e_ring_aligned)
  const uint32_t* etab;      // [group of 32 instances][gdw >= S * 32]: one dword per state, successor words of action 0 (low half)
                             // and 1 (high half), s' << 7 | code; interleaved by instance like the LDS image
  const double* rvals;       // [n_codes]
  uint2* codes;              // [episode][chunk][B] 2-bit reward codes of the chunk's steps, step j at bits 2 j
  int32_t* seg_h0;           // [B] in-episode time at the start of the segment (k_reward_scan decodes the episodes with it)
  int2* dep;                 // [group][gdw] DEPARTURE counts (action 0, action 1) accumulated over launches, interleaved like
                             // the LDS image; k_epi_fold turns them into the reference's arrival counts when they are needed
  int32_t* dep_res;          // [B] episode resets not yet added to visits_s of the start state
  // ---- the pair form (cmdp_k1e_pair.h); ash2 == 0: the batch has no pair plan ----
  int32_t ash2;              // log2 of an image's bytes in the pair table: 7 + log2(SP2), SP2 = even-time states padded to a power of two
  int32_t pgdw;              // dwords of a group's pair image in HBM: 2 * SP2 * 32 (whole rounds of the workgroup's 1024 lanes)
  const uint32_t* ptab;      // [group of 32 instances][pgdw]: dword (a1 * SP2 + x) * 32 + i = pair words (a0 = 0 | a0 = 1 << 16) of row x
  const uint16_t* pinv;      // [B][SP2] the state of compact index x
  int2* dep2;                // [group][pgdw] pair counts accumulated over launches, in ptab's layout (a0 = 0, a0 = 1); null in a fold
                             // when no launch of the handle took the pair form
  // ---- forms 2 and 3: the action bits of the segment, made by K16 ----
  const uint4* abits;        // [block relative to the segment's first][B]: bit (n_trans + j) & 127 of block ((n_trans & 127) + j) >> 7
};

// LDS: tables (2 actions x SP states x 32 instances x 4 B) | one ring per wavefront (ring_blocks x 4 dwords x 32 instances)
__host__ __device__ inline size_t k1e_tab_bytes(const K1ePlan& p) { return (size_t)2 << p.ash; }
__host__ __device__ inline size_t k1e_ring_bytes(const K1ePlan& p) { return (size_t)K1E_NW * (size_t)p.ring_blocks * 512; }
__host__ __device__ inline size_t k1e_lds_bytes(const K1ePlan& p) { return k1e_tab_bytes(p) + k1e_ring_bytes(p); }
__host__ __device__ inline size_t k1e_fold_lds_bytes(const K1ePlan& p) { return (size_t)2 * K1E_NI * (size_t)p.S * 4; }
__host__ __device__ inline int64_t k1e_max_episodes(int64_t n_steps, int H) { return (n_steps + 2 * (int64_t)H - 2) / H; }
// Does every wavefront's ring start at a multiple of its own size (ring_blocks x 512 B)?  The rings follow the tables, both are
// powers of two and the dynamic LDS starts at byte 0 (the kernel has no static LDS), so: when a ring is no larger than the
// tables.  The lane's bank offset 4 i lies below bit 7, under every ring dword's address bits: an interior round then forms
// a ring address as (128 d & ring mask) | (ring base + 4 i) -- one v_and_or_b32 -- where the general path masks and adds.
__host__ __device__ inline bool k1e_ring_aligned(const K1ePlan& p) { return k1e_tab_bytes(p) % ((size_t)p.ring_blocks * 512) == 0; }

// Is the round of eight episodes e_lo .. e_lo + 7 of a segment of n_steps transitions INTERIOR -- whatever the in-episode
// time h0 in [0, H) the segment starts at, every one of the eight is walked at full length H, none is episode 0 of the
// segment (which starts from the instance's current state, h0 steps in) and none contains transition n_steps - 1 (whose
// chain leaves the instance's state behind)?  Episode e > 0 covers transitions [e H - h0, (e + 1) H - h0): the last of the
// round ends at (e_lo + 8) H - h0 <= (e_lo + 8) H, which has to stay BELOW n_steps.  Wave-uniform inputs only (the
// kernel evaluates it in SALU); nb = instances of the group (lanes that own none are masked off as a whole, so a ragged group
// has interior rounds too).  Exported as cmdp_k1e_round_interior: the tests check the function the kernel uses.
__host__ __device__ inline bool k1e_round_interior(int e_lo, int H, int64_t n_steps, int nb) {
  return nb > 0 && H > 0 && e_lo >= 2 * K1E_EPL && ((int64_t)e_lo + 2 * K1E_EPL) * (int64_t)H < n_steps;
}

// steps of a code word (2-bit fields, unused fields zero) with code 1, 2, 3: n1 | n2 << 11 | n3 << 22 (11-bit fields: the
// packed words of a tile of the scan add up without carries into the neighbouring field).  k_reward_scan forms them from
// the code words it loads -- the walk stores no counts.  Exported as cmdp_k1e_code_counts: the tests check the functions
// the kernel uses.
// (at most three reward codes -- DeepSea: no field is 3, so every set bit is a step of code 1 or 2 and the 0xaaaaaaaa planes
// hold the steps of code 2: n1 + n2 = all bits, in the accumulating form of v_bcnt_u32_b32, and n1 | n2 << 11 =
// (n1 + n2) + 2047 n2 -- six or seven instructions per word)
__host__ __device__ __forceinline__ uint32_t k1e_code_counts_few(uint32_t lo, uint32_t hi) {
  const uint32_t n12 = (uint32_t)__builtin_popcount(lo) + (uint32_t)__builtin_popcount(hi);
  const uint32_t n2 = (uint32_t)__builtin_popcount(lo & 0xaaaaaaaau) + (uint32_t)__builtin_popcount(hi & 0xaaaaaaaau);
  return n12 + 2047u * n2;
}
__host__ __device__ __forceinline__ uint32_t k1e_code_counts(uint32_t lo, uint32_t hi) {
  const uint32_t l0 = lo & 0x55555555u, l1 = (lo >> 1) & 0x55555555u;
  const uint32_t h0 = hi & 0x55555555u, h1 = (hi >> 1) & 0x55555555u;
  const uint32_t n3 = (uint32_t)__builtin_popcount(l0 & l1) + (uint32_t)__builtin_popcount(h0 & h1);
  const uint32_t n1 = (uint32_t)__builtin_popcount(l0 & ~l1) + (uint32_t)__builtin_popcount(h0 & ~h1);
  const uint32_t n2 = (uint32_t)__builtin_popcount(~l0 & l1) + (uint32_t)__builtin_popcount(~h0 & h1);
  return n1 | (n2 << 11) | (n3 << 22);
}

typedef __attribute__((address_space(3))) uint32_t* k1e_lds_u32;

// what a workgroup needs of a group of 32 instances before it can walk it: the table image (<= 16 dwords per thread) and the
// lane's instance scalars.  A workgroup owns SEVERAL groups, one after the other, and loads the next group's set during the
// last pass of the walk of the current one: the HBM round trips of the staging run under the walk
// (the table image itself travels in ONE plain local array of sixteen, indexed by constants only: scalars after SROA -- a
// struct that is copied as a whole ends up in scratch, a 16-wide vector value is spilled as a whole.  The staging is the only
// reader and comes before the walk, so the last pass loads the next image into the very registers the staging has emptied)
struct K1eGroupRegs {
  uint32_t key_x, key_y, ntr_lo, ntr_hi;
  uint32_t hcs;   // in-episode time << 18 | current state << 9 | start state (S <= 512, H < 2^14: one register instead of three)
};

// FORM 0: the single form, below -- one transition per step, any segment.  FORM 1: the pair form (cmdp_k1e_pair.h, a
// specialisation of its own) -- two transitions per step, segments of whole episodes walked from reset.
// FORM 2 and 3: the same two walks with the action bits of CMDP_POLICY_RANDOM_REFERENCE -- `produce` loads the four dwords of
// a block from p.abits (K16, cmdp_actions.h) where forms 0 and 1 make the Philox block; nothing else differs.
template <int FORM>
__global__ void __launch_bounds__(K1E_THREADS) __attribute__((amdgpu_waves_per_eu(5, 5))) k_rollout_epi(EnvTables t, K1ePlan p, int n_steps,
                                                            int32_t* __restrict__ last_obs) {
  extern __shared__ __align__(16) unsigned char smem[];
  // (the reward scan of the previous launch shares the SIMDs with this kernel: the walk takes the issue slots first, the scan
  // -- one latency-bound wavefront per SIMD with a whole launch to finish in -- what is left.  Not when a workgroup has a
  // single group to walk: the launch is then shorter than the scan, and the scan is what the step waits for)
  if ((t.B + K1E_NI - 1) / K1E_NI > (int)gridDim.x) __builtin_amdgcn_s_setprio(3);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int inst = lane & (K1E_NI - 1), sub = lane >> 5;
  const int H = p.H;
  const int n_groups = (t.B + K1E_NI - 1) / K1E_NI;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;   // 0: no static LDS here
  const uint32_t tab_bytes = 2u << p.ash;
  const uint32_t a_words = (1u << p.ash) >> 2;           // dwords between the two actions' images
  uint32_t* tab = reinterpret_cast<uint32_t*>(smem);
  const uint32_t RD = (uint32_t)p.ring_blocks * 4u;      // ring dwords per instance
  uint32_t* ring = reinterpret_cast<uint32_t*>(smem + tab_bytes) + (size_t)wave * RD * K1E_NI;   // this wavefront's ring
  const uint32_t lbase = lds0 + 4u * (uint32_t)inst;     // the lane's bank
  const uint32_t lbase1 = lbase | (1u << p.ash);         // ... in the image of action 1
  const int nch = p.nch;
  const uint32_t ash = (uint32_t)p.ash;
  const int nj = p.gdw / K1E_THREADS;                     // rounds of the workgroup over a group's image (<= 16)

  // the loads of group g (k = s * 32 + i of the interleaved HBM image: coalesced; S <= 512: at most 16 dwords per thread)
  // (the empty asm statements pin the address arithmetic to this place: hoisted out of the pass loop -- the group is invariant
  // there -- sixteen 64-bit addresses would sit in registers under the whole walk)
  auto fetch_table = [&](int g, uint32_t (&pair)[16]) {
    const uint32_t* src = p.etab + (size_t)g * (size_t)p.gdw;
    uint32_t tid_o = (uint32_t)tid;
    int nj_o = nj;   // (pinned too: the sixteen tests j < nj, kept for staging, fetch and flush alike, cost 32 SGPRs under the walk)
    asm volatile("" : "+s"(src), "+v"(tid_o), "+s"(nj_o));
    // (uniform base + 32-bit lane offset: no 64-bit address per load)
#pragma unroll
    for (int j = 0; j < 16; ++j)
      pair[j] = j < nj_o ? __builtin_nontemporal_load(&src[tid_o + (uint32_t)(j * K1E_THREADS)]) : 0u;
  };
  auto fetch_scalars = [&](int g, K1eGroupRegs& r) {
    int bb = min(g * K1E_NI + inst, t.B - 1);   // (lanes past the batch repeat its last instance; they own nothing)
    asm volatile("" : "+v"(bb));
    const uint2 kk = t.philox_key[bb];
    const unsigned long long nn = t.n_trans[bb];
    r.key_x = kk.x; r.key_y = kk.y;
    r.ntr_lo = (uint32_t)nn; r.ntr_hi = (uint32_t)(nn >> 32);
    r.hcs = ((uint32_t)t.hstep[bb] << 18) | ((uint32_t)t.cur[bb] << 9) | (uint32_t)t.start_state[t.start_off[bb]];
  };

  K1eGroupRegs cur_regs;
  uint32_t cur_pair[16];
  fetch_table(blockIdx.x, cur_pair);
  fetch_scalars(blockIdx.x, cur_regs);

  for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const int g0 = g * K1E_NI;
    const int nb = min(K1E_NI, t.B - g0);
    const bool owner = inst < nb;
    const int b = g0 + (owner ? inst : 0);
    const bool more = g + (int)gridDim.x < n_groups;
    // ---- stage: {count 0 | successor word} from the registers the previous group's last pass (or the prologue) filled ----
    int nj_s = nj;
    asm volatile("" : "+s"(nj_s));   // (as in fetch_table: the tests j < nj are made here, not kept under the walk)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t k = (uint32_t)tid + (uint32_t)(j * K1E_THREADS);
      if (j < nj_s) {   // (gdw <= 2^ash / 4: the padding of the image lands in the padding of the LDS table)
        tab[k] = cur_pair[j] & 0xffffu;
        tab[a_words + k] = cur_pair[j] >> 16;
      }
    }
    __syncthreads();   // the image is complete before any wavefront walks it
    const uint2 key = make_uint2(cur_regs.key_x, cur_regs.key_y);
    const unsigned long long ntr = (unsigned long long)cur_regs.ntr_lo | ((unsigned long long)cur_regs.ntr_hi << 32);
    const uint32_t ntr_lo = (uint32_t)ntr;
    const int h0 = (int)(cur_regs.hcs >> 18);
    const int32_t cur0 = (int32_t)((cur_regs.hcs >> 9) & 511u);
    const int32_t start = (int32_t)(cur_regs.hcs & 511u);
    const unsigned long long blk0 = ntr >> 7;               // first Philox block of the segment
    const int off0 = (int)(ntr & 127ull);

    // The action bits.  A wavefront walks a CONTIGUOUS range of the segment's episodes, eight at a time (a round), and makes
    // the Philox blocks of a round itself, into its own ring: lanes 0-31 one block of their instance, lanes 32-63 the next.
    // Consecutive rounds continue in the stream, so every block is made once (but for the two at the ends of a wavefront's
    // range) -- and the walk needs NO workgroup barrier: LDS operations of one wavefront are performed in order.
    // ring dword d of the instance lives at ring[d * 32 + inst]: the stores and the chains' fetches stay in bank i
    int next_blk = 0;   // first block (relative to blk0) of this wavefront's range not made yet
    auto produce = [&](int e_lo) {   // e_lo: the round's first episode (wave-uniform)
      if (!owner) return;
      const int tlo = e_lo == 0 ? 0 : e_lo * H - h0;
      const int thi = min(n_steps, (e_lo + 2 * K1E_EPL) * H - h0);
      if (tlo >= thi) return;
      const int blo = (off0 + tlo) >> 7, bhi = (off0 + thi - 1) >> 7;
      int sub_o = sub;
      asm volatile("" : "+v"(sub_o));   // (as in fetch_group: nothing of this loop's 64-bit arithmetic is worth a register pair across the walk)
      for (int rb = max(blo, next_blk) + sub_o; rb <= bhi; rb += 2) {
        const unsigned long long blk = blk0 + (unsigned long long)rb;
        uint32_t w[4];
        if constexpr (FORM == 2) {   // the reference's stream: K16 has left the segment's blocks in HBM (cmdp_actions.h)
          const uint4 v = p.abits[(size_t)rb * (size_t)t.B + (size_t)b];
          w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
          philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), 2u, 0u, key.x, key.y, w);
        }
        const uint32_t d0 = ((uint32_t)blk & ((uint32_t)p.ring_blocks - 1u)) << 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) ring[(size_t)(d0 + j) * K1E_NI + inst] = w[j];
      }
      next_blk = bhi + 1;
    };
    // the 32 action bits from transition `rel` of the segment on
    auto fetch_bits = [&](int rel) -> uint32_t {
      const uint32_t a0 = ntr_lo + (uint32_t)rel;
      const uint32_t di = (a0 >> 5) & (RD - 1u);
      const uint32_t d0 = ring[di * K1E_NI + inst], d1 = ring[((di + 1u) & (RD - 1u)) * K1E_NI + inst];
      return __builtin_amdgcn_alignbit(d1, d0, a0 & 31u);
    };

    // The step loops of an INTERIOR round (below): the general path's `steps` and its two loops, word for word, on the interior
    // path's own registers.  (One pair of lambdas shared by both paths compiles, but the general path then keeps five values
    // more across the walk and the kernel no longer fits 96 VGPRs without scratch.)
    auto steps_int = [&](uint32_t (&bits)[K1E_EPL], uint32_t (&w)[K1E_EPL], uint32_t addv, uint32_t (&cw)[K1E_EPL]) {
      uint32_t ra[K1E_EPL];
#pragma unroll
      for (int c = 0; c < K1E_EPL; ++c) {
        uint32_t ax;
        asm("v_add_co_u32 %0, vcc, %0, %0\n\tv_cndmask_b32 %1, %2, %3, vcc" : "+v"(bits[c]), "=v"(ax) : "v"(lbase), "v"(lbase1) : "vcc");
        asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(ra[c]) : "v"(w[c]), "s"(K1E_SMASK), "v"(ax));
      }
#pragma unroll
      for (int c = 0; c < K1E_EPL; ++c)
        w[c] = __hip_atomic_fetch_add((k1e_lds_u32)(uintptr_t)ra[c], addv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
      for (int c = 0; c < K1E_EPL; ++c) cw[c] = __builtin_amdgcn_alignbit(w[c], cw[c], 2u);
    };
    // the L (<= 32, wave-uniform) steps of a chunk: the first L0 = min(L, 16) reward codes into clo, the others into chi
    auto walk_int = [&](int L0, int L, uint32_t (&bits)[K1E_EPL], uint32_t (&w)[K1E_EPL], uint32_t addv,
                        uint32_t (&clo)[K1E_EPL], uint32_t (&chi)[K1E_EPL]) {
      int j = 0;
      for (; j + 1 < L0; j += 2) { steps_int(bits, w, addv, clo); steps_int(bits, w, addv, clo); }
      if (j < L0) steps_int(bits, w, addv, clo);
      j = 16;
      for (; j + 1 < L; j += 2) { steps_int(bits, w, addv, chi); steps_int(bits, w, addv, chi); }
      if (j < L) steps_int(bits, w, addv, chi);
    };
    // this wavefront's ring as LDS byte addresses: dword d of the lane's instance at lbase + ring_sbase + (128 d & ring_mask)
    const uint32_t ring_sbase = tab_bytes + (uint32_t)wave * RD * (4u * K1E_NI);
    const uint32_t ring_mask = (RD - 1u) << 7;

    const int R = p.n_pass;   // rounds per wavefront: wavefront w owns episodes [8 R w, 8 R (w + 1)) of the segment
    for (int pass = 0; pass < R; ++pass) {
      const int e_lo = (wave * R + pass) * 2 * K1E_EPL;
      if (!(p.debug & 4)) produce(e_lo);
      // the next group's table image and scalars: in flight under the whole of this wavefront's last round
      if (pass == R - 1 && more) fetch_table(g + (int)gridDim.x, cur_pair);
      __builtin_amdgcn_wave_barrier();
      // ---- an INTERIOR round (k1e_round_interior: eight full episodes, none the segment's first, none with its last
      // transition -- 123 of a wavefront group's 125 working rounds at 30 000 transitions of H = 30): what the general path
      // below asks per chain and lane is known for the whole wavefront.  Every chain starts from the start state and counts,
      // the four chains' first transitions are H apart, the code / count words go out unpredicated through a uniform base and
      // ONE 32-bit lane offset, and there is neither a partial episode nor a last transition to look for ----
      if (p.fast && k1e_round_interior(e_lo, H, n_steps, nb)) {
        if (owner && !(p.debug & 1)) {
          // (pinned to the round like fetch_table's addresses: hoisted out of the pass loop -- the group is invariant there --
          // the lane's parts of the stream position, the ring address and the word index would sit in registers under the
          // whole walk, where the next group's table image needs them)
          int e0 = sub * K1E_EPL;
          uint32_t ring_base = ring_sbase;
          asm volatile("" : "+v"(e0), "+s"(ring_base));
          e0 += e_lo;
          const uint32_t ring_lane = lbase + ring_base;          // (a multiple of the ring's size + 4 i: p.fast)
          const uint32_t a00 = ntr_lo + (uint32_t)(e0 * H - h0);   // chain 0's first transition, as a stream position
          const uint32_t o00 = a00 << 2;                            // ... and as 128 x its ring dword (+ bits below 7, masked off)
          uint32_t addv = 0x10000u, hcs = cur_regs.hcs;   // every chain counts ...
          asm volatile("" : "+v"(addv), "+v"(hcs));
          uint32_t w[K1E_EPL];
#pragma unroll
          for (int c = 0; c < K1E_EPL; ++c) w[c] = (hcs & 511u) << 7;   // ... and starts from the start state
          for (int ch = 0; ch < nch; ++ch) {
            const int L = __builtin_amdgcn_readfirstlane(min(32, H - 32 * ch));
            // all eight ring reads of the four chains, then ONE wait (ring dword d at ring_lane | (128 d & ring_mask)).
            // Chain c's position is chain 0's plus a wave-uniform c H + 32 ch: per chain two additions of a scalar and two
            // v_and_or_b32 for the addresses, one addition for the funnel shift (a0 mod 32: the chunk drops out)
            uint32_t d0[K1E_EPL], d1[K1E_EPL], bits[K1E_EPL], clo[K1E_EPL], chi[K1E_EPL];
#pragma unroll
            for (int c = 0; c < K1E_EPL; ++c) {
              const uint32_t so = (uint32_t)__builtin_amdgcn_readfirstlane(4 * (c * H + 32 * ch));
              d0[c] = *(k1e_lds_u32)(uintptr_t)(((o00 + so) & ring_mask) | ring_lane);
              d1[c] = *(k1e_lds_u32)(uintptr_t)(((o00 + (so + 128u)) & ring_mask) | ring_lane);
            }
#pragma unroll
            for (int c = 0; c < K1E_EPL; ++c) {
              bits[c] = __builtin_bitreverse32(__builtin_amdgcn_alignbit(d1[c], d0[c], a00 + (uint32_t)(c * H)));
              clo[c] = 0u; chi[c] = 0u;
            }
            const int L0 = __builtin_amdgcn_readfirstlane(min(L, 16));
            walk_int(L0, L, bits, w, addv, clo, chi);
            if (!(p.debug & 8)) {
              const uint32_t wi = ((uint32_t)e0 * (uint32_t)nch + (uint32_t)ch) * (uint32_t)t.B + (uint32_t)b;
              const uint32_t o8 = wi << 3;                               // (< 2^31: p.fast)
              const uint32_t cstride = (uint32_t)nch * (uint32_t)t.B;   // words between two consecutive episodes
#pragma unroll
              for (int c = 0; c < K1E_EPL; ++c) {
                const uint32_t lo = L0 < 16 ? clo[c] >> (32 - 2 * L0) : clo[c];
                const uint32_t hi = L > 16 ? (L < 32 ? chi[c] >> (32 - 2 * (L - 16)) : chi[c]) : 0u;
                typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                u32x2 v;
                v.x = lo; v.y = hi;
                // (the uniform bases pinned to scalar registers: regrouped as (base + lane offset) + chain offset they cost two
                // 64-bit vector additions per chain)
                typedef __attribute__((address_space(1))) unsigned char* k1e_glb_u8;   // (global, not flat, stores)
                k1e_glb_u8 cb = (k1e_glb_u8)(uintptr_t)p.codes + (size_t)((uint32_t)c * cstride) * 8;
                asm volatile("" : "+s"(cb));
                __builtin_nontemporal_store(v, (__attribute__((address_space(1))) u32x2*)(cb + (size_t)o8));
              }
            }
          }
        }
        __builtin_amdgcn_wave_barrier();
        continue;
      }
      // ---- the lane's chains of this round (everything relative to the segment fits an int: n_steps <= K1E_SEG) ----
      // (first transition, length and kind of chain c are recomputed where they are needed, not kept in registers across
      // the walk: the next group's table image waits in registers under the last pass)
      const int e0 = e_lo + sub * K1E_EPL;
      auto first_of = [&](int c) -> int { return e0 + c == 0 ? 0 : (e0 + c) * H - h0; };
      auto len_of = [&](int c) -> int {
        const int f = first_of(c);
        return owner && f < n_steps ? min(e0 + c == 0 ? H - h0 : H, n_steps - f) : 0;
      };
      auto full_of = [&](int c) -> bool { return len_of(c) == H; };
      auto valid_of = [&](int c) -> bool { return owner && first_of(c) < n_steps; };
      uint32_t w[K1E_EPL], addv[K1E_EPL];
#pragma unroll
      for (int c = 0; c < K1E_EPL; ++c) {
        // a chain that is not walked at full length in the fast loop idles: it follows action 0 from state 0 and ADDS ZERO
        w[c] = full_of(c) ? ((uint32_t)(e0 + c == 0 ? cur0 : start) << 7) : 0u;
        addv[c] = full_of(c) ? 0x10000u : 0u;
      }
      bool any_full = false;
#pragma unroll
      for (int c = 0; c < K1E_EPL; ++c) any_full |= full_of(c);

      // ---- fast loop: full episodes, uniform trip counts; lanes without any full chain are masked off as a whole ----
      if (any_full && !(p.debug & 1)) {
        for (int ch = 0; ch < nch; ++ch) {
          const int L = __builtin_amdgcn_readfirstlane(min(32, H - 32 * ch));
          uint32_t bits[K1E_EPL], clo[K1E_EPL], chi[K1E_EPL];
#pragma unroll
          for (int c = 0; c < K1E_EPL; ++c) {
            const uint32_t fb = fetch_bits(first_of(c) + 32 * ch);
            bits[c] = full_of(c) ? __builtin_bitreverse32(fb) : 0u;
            clo[c] = 0u; chi[c] = 0u;
          }
          // one step of all the lane's chains: the atomics of all chains are issued before the first is waited for
          auto steps = [&](uint32_t (&cw)[K1E_EPL]) {
            uint32_t ra[K1E_EPL];
#pragma unroll
            for (int c = 0; c < K1E_EPL; ++c) {
              // (spelled out: left to itself the compiler may pick v_bfe . v_and (literal) . v_lshlrev . v_or3 -- five VALU
              // instructions per transition with the code word's v_alignbit instead of four)
              // (the action bits are consumed from the TOP of the bit-reversed window: v_add_co_u32 shifts the next one into VCC,
              // v_cndmask_b32 picks the lane's base in that action's image -- two VOP2 instructions where v_bfe_u32 .
              // v_lshl_or_b32 are two VOP3 ones: 20.9 instead of 22.4 cycles per wave-transition in isolation,
              // tools/calib/lds_atomic_rate.hip)
              uint32_t ax;
              asm("v_add_co_u32 %0, vcc, %0, %0\n\tv_cndmask_b32 %1, %2, %3, vcc" : "+v"(bits[c]), "=v"(ax) : "v"(lbase), "v"(lbase1) : "vcc");
              asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(ra[c]) : "v"(w[c]), "s"(K1E_SMASK), "v"(ax));
            }
#pragma unroll
            for (int c = 0; c < K1E_EPL; ++c)   // counts the row the chain leaves, returns {old count | successor word}
              w[c] = __hip_atomic_fetch_add((k1e_lds_u32)(uintptr_t)ra[c], addv[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
            for (int c = 0; c < K1E_EPL; ++c) cw[c] = __builtin_amdgcn_alignbit(w[c], cw[c], 2u);
          };
          const int L0 = __builtin_amdgcn_readfirstlane(min(L, 16));   // (wave-uniform by construction: keep the loop control scalar)
          {
            int j = 0;
            for (; j + 1 < L0; j += 2) { steps(clo); steps(clo); }
            if (j < L0) steps(clo);
            j = 16;
            for (; j + 1 < L; j += 2) { steps(chi); steps(chi); }
            if (j < L) steps(chi);
          }
          if (!(p.debug & 8)) {
            uint32_t wi = ((uint32_t)e0 * (uint32_t)nch + (uint32_t)ch) * (uint32_t)t.B + (uint32_t)b;
#pragma unroll
            for (int c = 0; c < K1E_EPL; ++c) {
              if (full_of(c)) {
                const uint32_t lo = L0 < 16 ? clo[c] >> (32 - 2 * L0) : clo[c];
                const uint32_t hi = L > 16 ? (L < 32 ? chi[c] >> (32 - 2 * (L - 16)) : chi[c]) : 0u;
                typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                u32x2 v;
                v.x = lo; v.y = hi;
                __builtin_nontemporal_store(v, reinterpret_cast<u32x2*>(p.codes) + wi);
              }
              wi += (uint32_t)nch * (uint32_t)t.B;
            }
          }
        }
      }
      // ---- slow loop: the partial episodes at the two ends of the segment (per-lane lengths) ----
#pragma unroll
      for (int c = 0; c < K1E_EPL; ++c) {
        if (valid_of(c) && !full_of(c)) {
          const int len_c = len_of(c), first_c = first_of(c);
          uint32_t ws = (uint32_t)((e0 + c) == 0 ? cur0 : start) << 7;
          for (int j0 = 0; j0 < len_c; j0 += 32) {
            const int L = min(32, len_c - j0);
            const uint32_t bits = fetch_bits(first_c + j0);
            uint32_t lo = 0u, hi = 0u;
            for (int j = 0; j < L; ++j) {
              const uint32_t a = (bits >> j) & 1u;
              const uint32_t ra = (ws & K1E_SMASK) | ((a << ash) | lbase);
              ws = __hip_atomic_fetch_add((k1e_lds_u32)(uintptr_t)ra, 0x10000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              if (j < 16) lo |= (ws & 3u) << (2 * j); else hi |= (ws & 3u) << (2 * (j - 16));
            }
            const uint32_t wi = ((uint32_t)(e0 + c) * (uint32_t)nch + (uint32_t)(j0 >> 5)) * (uint32_t)t.B + (uint32_t)b;
            p.codes[wi] = make_uint2(lo, hi);
          }
          w[c] = ws;
        }
      }
      // ---- the chain that takes the segment's last transition leaves the instance's state behind ----
#pragma unroll
      for (int c = 0; c < K1E_EPL; ++c) {
        if (valid_of(c) && first_of(c) + len_of(c) == n_steps) {
          const int hend = ((e0 + c) == 0 ? h0 : 0) + len_of(c);
          const bool term = hend >= H;
          const int32_t cur = term ? start : (int32_t)((w[c] & K1E_SMASK) >> 7);
          int b_o = b;
          asm volatile("" : "+v"(b_o));   // (as in fetch_table: hoisted out of the pass loop the three 64-bit addresses sit under the whole walk)
          t.cur[b_o] = cur;
          t.hstep[b_o] = term ? 0 : hend;
          if (last_obs) last_obs[b_o] = cur;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();   // every wavefront has walked its range: the counts are final

    if (wave == 0 && sub == 0 && owner) {
      const unsigned long long resets = (unsigned long long)(((int64_t)h0 + n_steps) / H);
      t.n_trans[b] = ntr + (unsigned long long)n_steps;
      t.n_reset[b] += resets;
      if (resets) t.prev_start[b] = t.last_start[b];   // (as K1L: env_reset's bookkeeping of the one start state)
      p.seg_h0[b] = h0;
      if (!(p.debug & 2)) p.dep_res[b] += (int32_t)resets;   // episode resets: they count the start state (k_epi_fold)
    }
    // ---- flush.  The table dwords hold DEPARTURE counts (row (s, a) left); they are added to the launch-spanning departure
    // image in HBM, which has the layout of the LDS image: a straight coalesced, conflict-free pass.  The reference's ARRIVAL
    // counts (base.py:1302-1303) are a linear function of them, formed by k_epi_fold when somebody needs the counters.
    // No read-modify-write round trip: the two counts of an entry are added by ONE returnless 64-bit atomic -- action 0 in
    // the low half, action 1 in the high half; the host's overflow guard keeps every count below 2^31, so the low half never
    // carries into the high one -- executed in L2 behind the workgroup's back while it walks its next group ----
    if (!(p.debug & 2)) {
      typedef __attribute__((address_space(1))) unsigned long long* k1e_glb_u64;
      unsigned long long* dep = reinterpret_cast<unsigned long long*>(p.dep) + (size_t)g * (size_t)p.gdw;
      uint32_t tid_o = (uint32_t)tid;
      int nj_f = nj;
      asm volatile("" : "+s"(dep), "+v"(tid_o), "+s"(nj_f));   // (as in fetch_group: no hoisted 64-bit offsets)
      const k1e_glb_u64 gdep = (k1e_glb_u64)(uintptr_t)dep;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t k = tid_o + (uint32_t)(j * K1E_THREADS);
        if (j < nj_f) {
          const uint32_t c0 = tab[k] >> 16, c1 = tab[a_words + k] >> 16;
          if (c0 | c1)
            __hip_atomic_fetch_add(gdep + k, (unsigned long long)c0 | ((unsigned long long)c1 << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    if (!more) break;
    // (the next group's instance scalars: five more registers than the walk has to spare -- this group's are dead now, and the
    // round trip runs under the flush's LDS reads and the barrier)
    fetch_scalars(g + (int)gridDim.x, cur_regs);
    __syncthreads();   // the counts are read: the next group's image may overwrite them
  }
}

// Departure counts -> the reference's visit counters.  BaseMDP.step counts the ARRIVAL node under the action taken
// (colosseum/mdp/base.py:1302-1303): visits_sa[s'][a] += sum of the departures of the rows (s, a) whose successor is s',
// visits_s[s'] += both actions' arrivals (+ the resets, which count the start state: base.py:1268-1277).  One workgroup per
// group of 32 instances; arrival images [action][instance][state] in LDS filled by atomics, then coalesced read-modify-writes
// (a wavefront per instance); the departure image is cleared.  Counters saturate at INT32_MAX and raise *overflow.
__global__ void __launch_bounds__(K1E_THREADS) k_epi_fold(EnvTables t, K1ePlan p, int32_t* __restrict__ overflow) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint32_t* arr0 = reinterpret_cast<uint32_t*>(smem);
  const int S = p.S;
  uint32_t* arr1 = arr0 + (size_t)K1E_NI * S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g0 = blockIdx.x * K1E_NI;
  const int nb = min(K1E_NI, t.B - g0);
  for (int k = tid; k < 2 * K1E_NI * S; k += K1E_THREADS) arr0[k] = 0u;
  __syncthreads();
  int2* dep = p.dep + (size_t)blockIdx.x * (size_t)p.gdw;
  const uint32_t* et = p.etab + (size_t)blockIdx.x * (size_t)p.gdw;
  for (int k = tid; k < S * K1E_NI; k += K1E_THREADS) {   // k = s * 32 + i
    const int2 c = dep[k];
    if (c.x | c.y) {
      const uint32_t pair = et[k];
      const int i = k & 31;
      if (c.x) atomicAdd(&arr0[i * S + (int)((pair & K1E_SMASK) >> 7)], (uint32_t)c.x);
      if (c.y) atomicAdd(&arr1[i * S + (int)(((pair >> 16) & K1E_SMASK) >> 7)], (uint32_t)c.y);
      dep[k] = make_int2(0, 0);
    }
  }
  // the pair image (cmdp_k1e_pair.h), when a launch of the handle took the pair form: dword k = (a1 * SP2 + x) * 32 + i holds
  // the counts of the pairs (a0 = 0, a1) and (a0 = 1, a1) of the even-time state s with compact index x.  A pair count c adds
  // c to the arrivals of (s', a0) and of (s'', a1), s' = next(s, a0), s'' = next(s', a1)
  if (p.dep2) {
    int2* dep2 = p.dep2 + (size_t)blockIdx.x * (size_t)p.pgdw;
    const int i_words = (1 << p.ash2) >> 2, SP2 = i_words >> 5;
    for (int k = tid; k < p.pgdw; k += K1E_THREADS) {
      const int2 c = dep2[k];
      if (c.x | c.y) {   // (lanes past the batch never count)
        const int i = k & 31, a1 = k >= i_words ? 1 : 0, x = (k - a1 * i_words) >> 5;
        const int s = (int)p.pinv[(size_t)(g0 + i) * SP2 + x];
        const uint32_t w1 = et[s * K1E_NI + i];
#pragma unroll
        for (int a0 = 0; a0 < 2; ++a0) {
          const uint32_t cnt = (uint32_t)(a0 ? c.y : c.x);
          if (cnt) {
            const int s1 = (int)(((w1 >> (16 * a0)) & K1E_SMASK) >> 7);
            const int s2 = (int)(((et[s1 * K1E_NI + i] >> (16 * a1)) & K1E_SMASK) >> 7);
            atomicAdd(&(a0 ? arr1 : arr0)[i * S + s1], cnt);
            atomicAdd(&(a1 ? arr1 : arr0)[i * S + s2], cnt);
          }
        }
        dep2[k] = make_int2(0, 0);
      }
    }
  }
  __syncthreads();
  const int64_t so0 = t.state_off[g0];
  bool ovf = false;
  auto sat_add = [&](int32_t old, uint32_t add) -> int32_t {
    const int64_t v = (int64_t)old + (int64_t)add;
    if (v > 0x7fffffffLL) { ovf = true; return 0x7fffffff; }
    return (int32_t)v;
  };
  for (int i = wave; i < nb; i += K1E_NW) {
    const int bi = g0 + i;
    const int32_t s_start = t.start_state[t.start_off[bi]];
    const uint32_t n_res = (uint32_t)p.dep_res[bi];
    const int64_t gs0 = so0 + (int64_t)i * S;
    for (int s = lane; s < S; s += 64) {
      const uint32_t c0 = arr0[i * S + s], c1 = arr1[i * S + s];
      const uint32_t add_s = c0 + c1 + (s == s_start ? n_res : 0u);
      if (add_s) t.visits_s[gs0 + s] = sat_add(t.visits_s[gs0 + s], add_s);
      if (c0 | c1) {
        int2* sa = reinterpret_cast<int2*>(t.visits_sa + (gs0 + s) * 2);
        int2 v = *sa;
        v.x = sat_add(v.x, c0);
        v.y = sat_add(v.y, c1);
        *sa = v;
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) p.dep_res[bi] = 0;
  }
  if (ovf) atomicOr(overflow, 1);
}

// The float64 reward sums of a segment, in TRANSITION ORDER: lane = instance.  The sum is sequential by definition (float64
// addition does not associate and the oracle adds reward by reward), but almost all of it can be done EXACTLY in integers:
// while the running sum S stays inside one binade [2^k, 2^(k+1)) its spacing is u = 2^(k-52), S = m u with an integer m, and
// for a reward v >= 0 the IEEE sum is fl(S + v) = (m + q) u with q = round-to-nearest(v / u) -- an integer that depends on v
// and k only -- unless v / u lies exactly half way between two integers (ties-to-even then looks at m).  Integer addition
// associates, so an episode chunk with n_c steps of reward code c advances m by sum_c n_c q_c, whatever the order: valid
// as long as no code present is a tie case in this binade and m stays below 2^53 (q >= 0: every partial sum then stayed in
// the binade too).  Otherwise -- a binade is crossed (~15 times per 30 000 transitions), S is zero or subnormal, a reward is
// negative or a tie case -- the chunk is added step by step in float64, exactly as the oracle does, and (k, m, q) are
// re-derived from the result.  An episode's code word holds the 2-bit reward codes of its steps, step j of a 32-step
// chunk at bits 2 j of the 64-bit word (unused fields zero).
//
// The lane's arithmetic -- its state (K1rLane), rebase, both forms of advance, the counts of a plain tile, the slow path
// and the episode / chunk bookkeeping -- is __host__ __device__ code: the kernel instantiates k1r_scan with a loader of
// global memory, cmdp_k1e_scan_words (cmdp.hip) with one of a host array, so the tests check on the CPU the very
// functions the kernel runs.  A wave-uniform vote of the kernel is the lane's own predicate on the host.
// element `i` (run-time, per lane) of a register array of 8: a select tree instead of an LDS round trip -- the reward scan
// keeps NO tile in LDS, so that its wavefronts fit beside k_rollout_epi's workgroups (whose tables take the CU's LDS)
typedef uint32_t k1r_u32x8 __attribute__((ext_vector_type(8)));   // (a vector value, not an array: it cannot end up in scratch)
__host__ __device__ __forceinline__ uint32_t k1r_sel8(const k1r_u32x8 a, int i) {
  const bool i0 = (i & 1) != 0, i1 = (i & 2) != 0, i2 = (i & 4) != 0;
  const uint32_t b0 = i0 ? a[1] : a[0], b1 = i0 ? a[3] : a[2], b2 = i0 ? a[5] : a[4], b3 = i0 ? a[7] : a[6];
  const uint32_t c0 = i1 ? b1 : b0, c1 = i1 ? b3 : b2;
  return i2 ? c1 : c0;
}

// ... and halfword `i` of a register array of 4 (the prefix sums of a tile's steps, <= 256, two to a register)
typedef uint32_t k1r_u32x4 __attribute__((ext_vector_type(4)));
__host__ __device__ __forceinline__ uint32_t k1r_sel8h(const k1r_u32x4 a, int i) {
  const bool i1 = (i & 2) != 0, i2 = (i & 4) != 0;
  const uint32_t b0 = i1 ? a[1] : a[0], b1 = i1 ? a[3] : a[2];
  return ((i2 ? b1 : b0) >> ((i & 1) << 4)) & 0xffffu;
}

#define K1R_THREADS 64
// The scan loads the CODE words (8 B) and counts the steps per code itself: the walk is bound by VALU issue and the scan --
// one wavefront per SIMD, hidden under the next walk -- takes the slots the walk leaves, so it is priced by its instruction
// count.  THREE tiles of EIGHT words: while one is summed, two are in flight (128 B per lane), and the tile being summed
// stays in registers for the step-by-step path.
//   plain a tile of single-chunk episodes that is neither the lane's first nor its last, for every lane of the wavefront
//         (one vote), holds 8 H steps: the steps per code of its eight words are accumulated straight into two or three
//         registers (v_bcnt_u32_b32 adds to its second operand) and ONE integer advance follows -- no packed word, no
//         prefix sums.  A lane whose advance fails takes the single-value path (k1r_single) when at most one nonzero reward
//         value occurs in the tile; otherwise it forms the packed prefix sums then, from the words still in its registers,
//         and takes the slow path under exec.
//   loads when the eight words of a tile exist for every lane of the wavefront (one vote) they are loaded unpredicated;
//         otherwise word by word under a test against W, unloaded words zero.  Either way the address is the word's scalar
//         base (advanced in SALU) plus the lane's 8 b: in the loop one v_lshl_add_u64 per load (K1rDeviceLoader).
#define K1R_T 8    // code words per tile
#define K1R_D 3    // tiles in registers: one being summed, the others' loads in flight
#if defined(__HIP_DEVICE_COMPILE__)
#define K1R_ALL(x) (__all(x) != 0)   // every lane of the wavefront ...
#define K1R_ANY(x) (__any(x) != 0)   // some lane of the wavefront ...
#else
#define K1R_ALL(x) (x)               // ... the lane itself on the host
#define K1R_ANY(x) (x)
#endif

// which paths a scan took (cmdp_k1e_scan_words reports them: the tests prove with them that their inputs reach every path);
// the kernel counts nothing
struct K1rNoStats {
  __host__ __device__ __forceinline__ void plain() {}
  __host__ __device__ __forceinline__ void slow() {}
  __host__ __device__ __forceinline__ void word() {}
  __host__ __device__ __forceinline__ void rebase() {}
  __host__ __device__ __forceinline__ void single() {}
  __host__ __device__ __forceinline__ void cross() {}
  __host__ __device__ __forceinline__ void fadd() {}
};
struct K1rStats {
  // plain tiles advanced whole, tiles on the slow path (the single-value ones among them), words added step by step, rebases
  // (after a word, or on the single-value path); then the single-value path alone (k1r_single): tiles it resolved, crossing
  // additions it made, additions of its float64 loop; one reserved
  int32_t n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  void plain() { ++n[0]; }
  void slow() { ++n[1]; }
  void word() { ++n[2]; }
  void rebase() { ++n[3]; }
  void single() { ++n[4]; }
  void cross() { ++n[5]; }
  void fadd() { ++n[6]; }
};

struct K1rLane {
  // the rewards by code (codes >= n_codes: 0.0): value, mantissa with the hidden bit, biased exponent (zero / subnormal: 0)
  double rv[4];
  unsigned long long mv[4];
  int eb[4];
  bool bulk_allowed;   // no reward is negative (or huge): the integer form may be used at all
  int n_codes, H, nch;
  int W;               // code words of the lane's instance in this segment, in order (< 2^31)
  // the sum: while !kvalid `m` holds the bits of the float64 sum S, else the integer form S = m * 2^(kb - 1075) with
  // 2^52 <= m < 2^53 (kb = biased exponent) -- one register pair for both; q[c] = round(rv[c] / spacing) as (low, high)
  // halves; `tie`: codes whose presence forces the float64 path (a tie case in this binade, a subnormal reward, a reward
  // at or above 2^(k+1))
  bool kvalid;
  int kb;
  unsigned long long m;
  uint32_t qlo[4], qhi[4];
  uint32_t tie;
  // episode / chunk bookkeeping of the next word to be laid out
  int ch;
  int e_len;          // steps of the current episode inside this segment
  int ep_left;        // ... not yet covered by earlier chunks
  int tot_left;       // steps from the current episode's first one on (a segment: < 2^31)
};

// (k, m, q, tie) from the float64 sum in L.m (!kvalid).  q is derived for the codes c < n_codes only (wave-uniform): the
// others stay 0 as k1r_init left them
__host__ __device__ __forceinline__ void k1r_rebase(K1rLane& L) {
  const unsigned long long M52 = (1ull << 52) - 1ull, B52 = 1ull << 52;
  L.kvalid = false;
  const unsigned long long sb = L.m;
  const double S = __builtin_bit_cast(double, sb);
  if (!L.bulk_allowed || !(S >= 2.2250738585072014e-308) || !(S < 1.0e300)) return;
  L.kb = (int)(sb >> 52);
  L.m = (sb & M52) | B52;
  L.tie = 0u;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c < L.n_codes) {
      unsigned long long qq = 0ull;
      if (L.rv[c] != 0.0) {
        const int d = L.kb - L.eb[c];
        if (L.eb[c] == 0 || d < 0) L.tie |= 1u << c;   // subnormal reward, or v >= 2^(k+1): the sum would leave the binade
        else if (d == 0) qq = L.mv[c];
        else if (d < 55) {
          const unsigned long long half = 1ull << (d - 1), rem = L.mv[c] & ((1ull << d) - 1ull);
          qq = (L.mv[c] >> d) + (rem > half ? 1ull : 0ull);
          if (rem == half) L.tie |= 1u << c;
        }
      }
      L.qlo[c] = (uint32_t)qq;
      L.qhi[c] = (uint32_t)(qq >> 32);
    }
  }
  L.kvalid = true;
}

// the lane at the start of a segment of n_steps transitions that begins h0 steps into an episode, its sum at S0
__host__ __device__ __forceinline__ void k1r_init(K1rLane& L, const double (&rv)[4], int n_codes, int H, int nch, int h0,
                                                  int64_t n_steps, double S0) {
  const unsigned long long M52 = (1ull << 52) - 1ull, B52 = 1ull << 52;
  L.n_codes = n_codes; L.H = H; L.nch = nch;
  L.bulk_allowed = true;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    L.rv[c] = rv[c];
    L.bulk_allowed = L.bulk_allowed && rv[c] >= 0.0 && rv[c] < 1.0e300;
    const unsigned long long vb = __builtin_bit_cast(unsigned long long, rv[c]);
    L.eb[c] = (int)(vb >> 52) & 0x7ff;
    L.mv[c] = (vb & M52) | B52;
    L.qlo[c] = 0u; L.qhi[c] = 0u;
  }
  const int64_t E = ((int64_t)h0 + n_steps + H - 1) / H;
  L.W = (int)(E * nch);
  L.m = __builtin_bit_cast(unsigned long long, S0);
  L.kvalid = false; L.kb = 0; L.tie = 0u;
  L.ch = 0;
  L.e_len = (int)((int64_t)(H - h0) < n_steps ? (int64_t)(H - h0) : n_steps);
  L.ep_left = L.e_len;
  L.tot_left = (int)n_steps;
  k1r_rebase(L);
}

// m + the advance of `steps` (<= 512) transitions of which n1, n2, n3 have reward code 1, 2, 3; true = the whole of it stays
// in the integer form
__host__ __device__ __forceinline__ bool k1r_advance(const K1rLane& L, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t steps,
                                                     unsigned long long& m2) {
  const uint32_t n0 = steps - n1 - n2 - n3;
  const uint32_t present = (n0 ? 1u : 0u) | (n1 ? 2u : 0u) | (n2 ? 4u : 0u) | (n3 ? 8u : 0u);
  unsigned long long lo64 = (unsigned long long)n0 * L.qlo[0];
  lo64 += (unsigned long long)n1 * L.qlo[1];
  lo64 += (unsigned long long)n2 * L.qlo[2];
  lo64 += (unsigned long long)n3 * L.qlo[3];
  const uint32_t hi32 = n0 * L.qhi[0] + n1 * L.qhi[1] + n2 * L.qhi[2] + n3 * L.qhi[3];   // <= 512 * 2^22
  m2 = L.m + lo64 + ((unsigned long long)hi32 << 32);
  return L.kvalid && (present & L.tie) == 0u && m2 < (1ull << 53);
}
// ... with the packed counts nw = n1 | n2 << 11 | n3 << 22 (k1e_code_counts) of the slow path's prefix sums
__host__ __device__ __forceinline__ bool k1r_advance(const K1rLane& L, uint32_t nw, uint32_t steps, unsigned long long& m2) {
  return k1r_advance(L, nw & 0x7ffu, (nw >> 11) & 0x7ffu, nw >> 22, steps, m2);
}
// the float64 sum (its bits) of the integer form
__host__ __device__ __forceinline__ unsigned long long k1r_compose(const K1rLane& L) {
  return ((unsigned long long)L.kb << 52) | (L.m & ((1ull << 52) - 1ull));
}
__host__ __device__ __forceinline__ double k1r_sum(const K1rLane& L) {
  return __builtin_bit_cast(double, L.kvalid ? k1r_compose(L) : L.m);
}

// The steps per code of a whole tile, accumulated over its eight words (popcount + accumulator is one v_bcnt_u32_b32).
// At most three codes: no field is 3, so all set bits are n1 + n2 and the odd planes hold n2; the odd plane of the low half
// and -- shifted down -- that of the high half are merged into one word before they are counted (one v_lshrrev, one v_bfi).
__host__ __device__ __forceinline__ void k1r_tile_counts_few(const k1r_u32x8& clo, const k1r_u32x8& chi, uint32_t& n1, uint32_t& n2) {
  uint32_t n12 = 0u, c2 = 0u;
#pragma unroll
  for (int k = 0; k < K1R_T; ++k) {
    n12 += (uint32_t)__builtin_popcount(clo[k]);
    n12 += (uint32_t)__builtin_popcount(chi[k]);
    c2 += (uint32_t)__builtin_popcount((clo[k] & 0xaaaaaaaau) | ((chi[k] >> 1) & 0x55555555u));
  }
  n1 = n12 - c2; n2 = c2;
}
// Four codes: all set bits are n1 + n2 + 2 n3, the odd planes n2 + n3, and a third plane (both bits of a field) n3.
__host__ __device__ __forceinline__ void k1r_tile_counts(const k1r_u32x8& clo, const k1r_u32x8& chi, uint32_t& n1, uint32_t& n2,
                                                         uint32_t& n3) {
  uint32_t all = 0u, odd = 0u, c3 = 0u;
#pragma unroll
  for (int k = 0; k < K1R_T; ++k) {
    all += (uint32_t)__builtin_popcount(clo[k]);
    all += (uint32_t)__builtin_popcount(chi[k]);
    odd += (uint32_t)__builtin_popcount((clo[k] & 0xaaaaaaaau) | ((chi[k] >> 1) & 0x55555555u));
    const uint32_t l3 = clo[k] & (clo[k] >> 1), h3 = chi[k] & (chi[k] >> 1);   // (bit 2 j: field j is 3; odd bits: anything)
    c3 += (uint32_t)__builtin_popcount((l3 & 0x55555555u) | ((h3 << 1) & 0xaaaaaaaau));
  }
  n3 = c3; n2 = odd - c3; n1 = all - odd - c3;
}

// The SINGLE-VALUE path of a tile whose whole advance has failed for this lane: among the codes present in the tile (n_c > 0
// of the tile's totals) at most ONE has a nonzero reward v.  The order of the tile's steps then does not matter -- adding
// +0.0 leaves the sum as it is (it is never -0.0) and every other addition is the same number -- so the sum after the tile is
// "v added na times", wherever the na steps sit: no code word, no prefix sum and no search enters.  (Sparse rewards: DeepSea
// under the random policy -- the goal reward needs H right moves -- FrozenLake, MiniGrid; every crossing tile of C2.)
//   integer form  the largest j <= na with m + j q < 2^53: a float32 quotient of room = 2^53 - 1 - m and q, cut at na, gives
//                 an estimate, integer comparisons DECIDE.  Two conversions and a division are each within 2^-24 of their
//                 result, na <= 256: a quotient below 2^20 is estimated to within 1/4, a larger one is cut at na like the
//                 true one.  So the estimate is off by one at the most, and one step down (m + j q does not fit) or up (one
//                 more fits) makes it exact.  j == na: done.  Else the ONE float64 addition that leaves the binade, as the
//                 oracle makes it, a rebase, and the rest of the steps again.  (A float64 quotient and fix-up LOOPS cost the
//                 kernel its last registers: 8 to 20 B of scratch.)
//   float64 loop  no integer form (the sum is zero or subnormal: the first tile of a launch from 0.0) or v is a tie case in
//                 this binade (k1r_rebase: subnormal v and v >= 2^(k+1) too): v is added na times, one addition per trip,
//                 and ONE rebase follows.
// false: the lane is not eligible (a negative reward, two nonzero values present) and goes on to k1r_slow, nothing changed.
template <class ST>
__host__ __device__ __forceinline__ bool k1r_single(K1rLane& L, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t steps, ST& st) {
  const uint32_t n0 = steps - n1 - n2 - n3;
  // (every member of the lane's arrays is read into a value of its own before it is selected: a select between two loads
  // becomes a load through a selected address, and the lane would live in scratch)
  const double rv0 = L.rv[0], rv1 = L.rv[1], rv2 = L.rv[2], rv3 = L.rv[3];
  const bool a0 = (n0 != 0u) & (rv0 != 0.0), a1 = (n1 != 0u) & (rv1 != 0.0), a2 = (n2 != 0u) & (rv2 != 0.0),
             a3 = (n3 != 0u) & (rv3 != 0.0);
  if (!L.bulk_allowed || (int)a0 + (int)a1 + (int)a2 + (int)a3 > 1) return false;
  st.slow();
  st.single();
  // the active code (none: every step adds +0.0), its count and value by selects -- the lane's arrays stay in registers
  uint32_t na = a3 ? n3 : (a2 ? n2 : (a1 ? n1 : (a0 ? n0 : 0u)));
  const double v = a3 ? rv3 : (a2 ? rv2 : (a1 ? rv1 : rv0));
  const uint32_t abit = a3 ? 8u : (a2 ? 4u : (a1 ? 2u : 1u));
  const unsigned long long LIM = 1ull << 53;
  while (na) {
    double S;
    if (!L.kvalid || (L.tie & abit) != 0u) {
      S = __builtin_bit_cast(double, L.kvalid ? k1r_compose(L) : L.m);
      for (uint32_t i = 0; i < na; ++i) { S += v; st.fadd(); }
      na = 0u;
    } else {
      const uint32_t ql0 = L.qlo[0], ql1 = L.qlo[1], ql2 = L.qlo[2], ql3 = L.qlo[3];
      const uint32_t qh0 = L.qhi[0], qh1 = L.qhi[1], qh2 = L.qhi[2], qh3 = L.qhi[3];
      const uint32_t ql = a3 ? ql3 : (a2 ? ql2 : (a1 ? ql1 : ql0));
      const uint32_t qh = a3 ? qh3 : (a2 ? qh2 : (a1 ? qh1 : qh0));   // (< 2^21: j qh fits 32 bits)
      const unsigned long long q = (unsigned long long)ql | ((unsigned long long)qh << 32);
      uint32_t j = na;
      if (q) {
        const float e = (float)(LIM - 1ull - L.m) / (float)q, en = (float)na;
        j = (uint32_t)(e < en ? e : en);
      }
      unsigned long long t = L.m + (unsigned long long)j * ql + ((unsigned long long)(j * qh) << 32);   // (j q < 2^61)
      if (j > 0u && t >= LIM) { --j; t -= q; }          // (the estimate is off by one at the most, see above)
      else if (j < na && t + q < LIM) { ++j; t += q; }
      L.m = t;
      if (j == na) break;
      S = __builtin_bit_cast(double, k1r_compose(L)) + v;   // addition j + 1 leaves the binade
      st.cross();
      na -= j + 1u;
    }
    L.m = __builtin_bit_cast(unsigned long long, S);
    k1r_rebase(L);
    st.rebase();
  }
  return true;
}

// The slow path of a tile whose whole advance has failed for this lane: the first word that does not advance (binary
// search over the prefix sums P of packed counts and SP of steps; SP holds two sums to a register), everything before it
// in one piece, that word in float64 step by step exactly as the oracle adds, then the rest of the tile again.  The search
// is valid because advancing is monotone: q >= 0, and a code that forces the float64 path stays present in every longer prefix.
template <class ST>
__host__ __device__ __forceinline__ void k1r_slow(K1rLane& L, const k1r_u32x8& clo, const k1r_u32x8& chi, const k1r_u32x8& P,
                                                  const k1r_u32x4& SP, ST& st) {
  const uint32_t Pt = P[K1R_T - 1], St = SP[K1R_T / 2 - 1] >> 16;
  const double rv0 = L.rv[0], rv1 = L.rv[1], rv2 = L.rv[2], rv3 = L.rv[3];
  unsigned long long m2;
  uint32_t base_n = 0u, base_s = 0u;
  int from = 0;
  for (;;) {   // (here the advance of the words from `from` on is known to fail: the caller's, or the test at the bottom)
    int lo = from, hi = K1R_T - 1;
#pragma unroll
    for (int it = 0; it < 3; ++it) {   // 2^3 = K1R_T
      const int mid = (lo + hi) >> 1;
      const bool ok = k1r_advance(L, k1r_sel8(P, mid) - base_n, k1r_sel8h(SP, mid) - base_s, m2);
      if (lo < hi) { if (ok) lo = mid + 1; else hi = mid; }
    }
    const int k = lo;
    const uint32_t Sk1 = k > 0 ? k1r_sel8h(SP, k - 1) : 0u;
    if (k > from && k1r_advance(L, k1r_sel8(P, k - 1) - base_n, Sk1 - base_s, m2)) L.m = m2;
    const uint32_t Sk = k1r_sel8h(SP, k);
    const uint32_t Lw = Sk - Sk1;
    if (Lw) {
      st.word();
      // (the word is in registers: the tile is reloaded only when it is done)
      const uint32_t cx = k1r_sel8(clo, k), cy = k1r_sel8(chi, k);
      double S = __builtin_bit_cast(double, L.kvalid ? k1r_compose(L) : L.m);
      // (step by step exactly as the oracle adds, but for the steps whose reward is +0.0 -- x + 0.0 == x, the sum is never
      // -0.0 -- which are skipped: the scaled minimum reward is 0, half of DeepSea's steps.  The reward of a code by a
      // select on four registers: the scan owns no LDS at all, k_rollout_epi may hold every byte of the CU's.  One wavefront
      // per SIMD issues an instruction every ~8 cycles, so this path is priced by its instruction count)
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const uint32_t cw = half ? cy : cx;
        const int Lh = (int)Lw - 16 * half;
        if (Lh > 0) {
          const uint32_t vm = Lh >= 16 ? 0x55555555u : ((1u << (2 * Lh)) - 1u) & 0x55555555u;
          const uint32_t b0 = cw & vm, b1 = (cw >> 1) & vm;
          uint32_t nz = 0u;
          if (rv0 != 0.0) nz |= vm & ~(b0 | b1);
          if (rv1 != 0.0) nz |= b0 & ~b1;
          if (rv2 != 0.0) nz |= b1 & ~b0;
          if (rv3 != 0.0) nz |= b0 & b1;
          while (nz) {
            const uint32_t pos = (uint32_t)__builtin_ctz(nz);
            nz &= nz - 1u;
            const uint32_t cd = cw >> pos;
            const bool c0 = (cd & 1u) != 0u, c1 = (cd & 2u) != 0u;
            const double lo2 = c0 ? rv1 : rv0, hi2 = c0 ? rv3 : rv2;
            S += c1 ? hi2 : lo2;
          }
        }
      }
      L.m = __builtin_bit_cast(unsigned long long, S);
      k1r_rebase(L);
      st.rebase();
    }
    base_n = k1r_sel8(P, k);
    base_s = Sk;
    from = k + 1;
    if (from >= K1R_T) break;
    if (k1r_advance(L, Pt - base_n, St - base_s, m2)) { L.m = m2; break; }
  }
}

// The tile of code words w0 .. w0 + K1R_T - 1 (low and high halves; past the lane's end: zero).
template <class ST>
__host__ __device__ __forceinline__ void k1r_tile(K1rLane& L, const k1r_u32x8& clo, const k1r_u32x8& chi, const int w0, ST& st) {
  const int H = L.H;
  const bool few = L.n_codes <= 3;   // (wave-uniform: no field of a code word is 3)
  unsigned long long m2;
  k1r_u32x8 P;
  k1r_u32x4 SP;   // (prefix sums of steps, SP[k] in halfword k & 1 of register k >> 1)
  // plain tiles -- interior ones of single-chunk episodes, for all lanes: every word holds H steps
  const bool plain = L.nch == 1 && K1R_ALL(w0 >= 1 && w0 + K1R_T <= L.W - 1);
  uint32_t n1, n2, n3, steps;   // the tile's totals
  bool whole;
  if (plain) {
    steps = (uint32_t)(K1R_T * H);
    if (few) {
      k1r_tile_counts_few(clo, chi, n1, n2);
      n3 = 0u;
      whole = k1r_advance(L, n1, n2, 0u, steps, m2);
    } else {
      k1r_tile_counts(clo, chi, n1, n2, n3);
      whole = k1r_advance(L, n1, n2, n3, steps, m2);
    }
    L.tot_left -= K1R_T * H;   // eight full episodes on: the next one may be the segment's last, partial one
    L.e_len = H < L.tot_left ? H : L.tot_left;
    L.ep_left = L.e_len;
    if (whole) st.plain();
  } else {
    // the first and the last tile, chunked episodes, ragged ends: the packed counts of the tile's words and their prefix
    // sums; 0 steps for a chunk a partial episode does not reach or a word past the end
    uint32_t acc = 0u, sacc = 0u;
#pragma unroll
    for (int k = 0; k < K1R_T; ++k) {
      const int Lk = (w0 + k < L.W) ? (L.ep_left < 0 ? 0 : (L.ep_left < 32 ? L.ep_left : 32)) : 0;
      const uint32_t rn = few ? k1e_code_counts_few(clo[k], chi[k]) : k1e_code_counts(clo[k], chi[k]);
      acc += Lk > 0 ? rn : 0u;
      sacc += (uint32_t)Lk;
      P[k] = acc;
      if (k & 1) SP[k >> 1] |= sacc << 16; else SP[k >> 1] = sacc;
      L.ep_left -= 32;
      if (++L.ch == L.nch) {
        L.ch = 0;
        L.tot_left -= L.e_len;
        L.e_len = H < L.tot_left ? H : L.tot_left;
        L.ep_left = L.e_len;
      }
    }
    n1 = acc & 0x7ffu; n2 = (acc >> 11) & 0x7ffu; n3 = acc >> 22;
    steps = sacc;
    whole = k1r_advance(L, n1, n2, n3, steps, m2);
  }
  if (whole) { L.m = m2; return; }
  // A lane whose advance fails takes the single-value path when it may (every crossing tile of C2).  Only when some lane of
  // the wavefront goes on to k1r_slow are the packed counts and the prefix vectors of a plain tile formed, from the words
  // still in registers
  const bool done = k1r_single(L, n1, n2, n3, steps, st);
  if (!K1R_ANY(!done)) return;
  if (done) return;
  if (plain) {
    uint32_t acc = 0u;
#pragma unroll
    for (int k = 0; k < K1R_T; ++k) {
      acc += few ? k1e_code_counts_few(clo[k], chi[k]) : k1e_code_counts(clo[k], chi[k]);
      P[k] = acc;
    }
#pragma unroll
    for (int k = 0; k < K1R_T; k += 2) SP[k >> 1] = (uint32_t)((k + 1) * H) | ((uint32_t)((k + 2) * H) << 16);
  }
  st.slow();
  k1r_slow(L, clo, chi, P, SP, st);
}

// The scan of a lane: three tiles of code words (A, B, C in turn); a tile's registers take the words K1R_D tiles on as soon
// as it is summed.  LD::fetch(clo, chi, w0) loads the words w0 .. w0 + K1R_T - 1 (past the end: zero, not loaded).
template <class LD, class ST>
__host__ __device__ __forceinline__ void k1r_scan(K1rLane& L, LD& ld, ST& st) {
  k1r_u32x8 loA, hiA, loB, hiB, loC, hiC;
  ld.fetch(loA, hiA, 0);
  ld.fetch(loB, hiB, K1R_T);
  ld.fetch(loC, hiC, 2 * K1R_T);
  const int W = L.W;
  for (int w0 = 0; w0 < W; w0 += K1R_D * K1R_T) {
    k1r_tile(L, loA, hiA, w0, st);
    ld.fetch(loA, hiA, w0 + K1R_D * K1R_T);
    if (w0 + K1R_T < W) {
      k1r_tile(L, loB, hiB, w0 + K1R_T, st);
      ld.fetch(loB, hiB, w0 + (K1R_D + 1) * K1R_T);
    }
    if (w0 + 2 * K1R_T < W) {
      k1r_tile(L, loC, hiC, w0 + 2 * K1R_T, st);
      ld.fetch(loC, hiC, w0 + (K1R_D + 2) * K1R_T);
    }
  }
}

// the words of ONE instance in a host array (cmdp_k1e_scan_words)
struct K1rHostLoader {
  const uint64_t* words;
  int W;
  void fetch(k1r_u32x8& clo, k1r_u32x8& chi, const int w0) const {
    for (int k = 0; k < K1R_T; ++k) {
      const uint64_t v = w0 + k < W ? words[w0 + k] : 0ull;
      clo[k] = (uint32_t)v; chi[k] = (uint32_t)(v >> 32);
    }
  }
};

// codes[word][instance] in global memory: word w of the lane's instance b lies B words after word w - 1
typedef uint32_t k1r_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) unsigned char* k1r_glb_u8;
template <bool OFF32>   // 8 B < 2^31: the lane keeps its byte offset 8 b, else b
struct K1rDeviceLoader {
  k1r_glb_u8 codes;    // (wave-uniform)
  uint32_t lane_off;   // OFF32: 8 b, the lane's byte offset from a word's base; else b
  int B, W;
  // The address of word w0 + k: the word's base, pinned to a scalar register pair (s_mov / s_add_u32 / s_addc_u32 per load),
  // plus the lane's offset.  What the compiler makes of it for gfx950: only the loads before the loop take the form "scalar
  // base + 32-bit vector offset"; every load inside the loop is one v_lshl_add_u64 of the base and the pair (8 b, 0), which
  // stays in two registers across the scan, and a load through the 64-bit vector address -- with OFF32 and without.  So the
  // pins and OFF32 do NOT buy the scalar-base form where the time goes.  They stay for what was measured: the same loader
  // written plainly (base + k stride + 8 b, one kernel, no pin; 126 VGPRs, 7 % less SALU in the code) ran the scan alone in
  // 0.187 ms against 0.160 ms for this form and 0.173 ms for the parent, and the step slower than the parent
  // (profiles/k1e_scan_lean.json, "plain_loader").  Why the plain form is slower was not found.
  __device__ __forceinline__ const __attribute__((address_space(1))) k1r_u32x2* word(k1r_glb_u8 base, size_t stride, int k) const {
    k1r_glb_u8 wb = base + (size_t)k * stride;
    asm volatile("" : "+s"(wb));
    if constexpr (OFF32) return (const __attribute__((address_space(1))) k1r_u32x2*)(wb + (size_t)lane_off);
    else {
      uint32_t bo = lane_off;
      asm volatile("" : "+v"(bo));   // (the 64-bit lane offset formed at the load, not kept in a register pair across the scan)
      return (const __attribute__((address_space(1))) k1r_u32x2*)(wb + (size_t)bo * 8);
    }
  }
  __device__ __forceinline__ int instance() const { return (int)(OFF32 ? lane_off >> 3 : lane_off); }
  __device__ __forceinline__ void fetch(k1r_u32x8& clo, k1r_u32x8& chi, const int w0) const {
    const size_t stride = (size_t)(uint32_t)__builtin_amdgcn_readfirstlane(B) * 8;
    const uint64_t a0 = (uint64_t)(uintptr_t)codes + (size_t)w0 * stride;
    const k1r_glb_u8 base = (k1r_glb_u8)(uintptr_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a0) |
                                                    ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a0 >> 32)) << 32));
    if (__all(w0 + K1R_T <= W)) {
      // every lane of the wavefront owns all eight words: no test, no zeroing -- for seven of them: the compiler merges the
      // eighth load into the tested path below (two zeroed registers, an exec branch whose test holds).  A scheduling barrier
      // at the end of this branch keeps it apart; that was built with the plain loader only (above) and not measured alone
#pragma unroll
      for (int k = 0; k < K1R_T; ++k) {
        const k1r_u32x2 v = __builtin_nontemporal_load(word(base, stride, k));
        clo[k] = v.x; chi[k] = v.y;
      }
      return;
    }
#pragma unroll
    for (int k = 0; k < K1R_T; ++k) {
      k1r_u32x2 v = {0u, 0u};
      if (w0 + k < W) v = __builtin_nontemporal_load(word(base, stride, k));
      clo[k] = v.x; chi[k] = v.y;
    }
  }
};

// (<= 128 VGPRs and NO LDS: a wavefront of the scan fits on every SIMD beside k_rollout_epi's workgroup -- 4 x 96 VGPRs
// per SIMD, 163 840 B of LDS per CU -- so that the scan of one segment runs under the walk of the next)
// OFF32: 8 B < 2^31 (launch_k1e)
template <bool OFF32>
__global__ void __launch_bounds__(K1R_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) k_reward_scan(EnvTables t, K1ePlan p, int64_t n_steps,
                                                            double* __restrict__ reward_sum, int accumulate) {
  const int lane = threadIdx.x;
  const int b = min(blockIdx.x * K1R_THREADS + lane, t.B - 1);   // (lanes past the batch repeat its last instance, unstored)
  const bool mine = blockIdx.x * K1R_THREADS + lane < t.B;
  double rv[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) rv[c] = c < p.n_codes ? p.rvals[c] * t.rscale - t.rmin : 0.0;
  K1rLane L;
  k1r_init(L, rv, p.n_codes, p.H, p.nch, p.seg_h0[b], n_steps, accumulate ? reward_sum[b] : 0.0);
  K1rDeviceLoader<OFF32> ld;
  ld.codes = (k1r_glb_u8)(uintptr_t)p.codes;
  ld.lane_off = OFF32 ? (uint32_t)b * 8u : (uint32_t)b;
  ld.B = t.B; ld.W = L.W;
  K1rNoStats st;
  k1r_scan(L, ld, st);
  // (b again, from the one register the loader keeps of it, and pinned: the address of reward_sum[b] formed here, not kept in a
  // register pair from the load above across the whole scan)
  int bs = ld.instance();
  asm volatile("" : "+v"(bs));
  if (mine) reward_sum[bs] = k1r_sum(L);
}
