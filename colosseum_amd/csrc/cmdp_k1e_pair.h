// cmdp_k1e_pair.h -- k_rollout_epi<1> and <3>: the PAIR form of K1E's walk (cmdp_k1e.h), two transitions per LDS atomic.
//
// The single form's step is one address, one returning LDS atomic and one reward code per transition, and both of its pipes
// are close to full (VALU ~17, LDS 4 x 4.3 = 17 of 20.9 cycles per wave-transition per SIMD).  The dynamics of a K1E batch are
// deterministic, so a row "state s, then action a0, then action a1" has ONE successor and TWO reward codes: an episode of
// even length walked from its start state is a chain of H / 2 such rows, and one step per PAIR halves the atomics per
// transition and takes 4 VALU instructions per two transitions instead of 8 (tools/calib/lds_atomic_rate.hip, part 4;
// profiles/k1e_pair_step.txt: 10.5 cycles per transition per SIMD in isolation against 20.9).
//
// The launcher takes this form only for launches that consist of WHOLE EPISODES WALKED FROM RESET (every instance at its
// start state with in-episode time 0, n a multiple of H, H even; launch_k1e in cmdp.hip), so the kernel has no general path:
// every round is what the single form's interior round is.  Everything else keeps k_rollout_epi<0>.
//   table  E = the states an instance can be in at an even in-episode time (plan_k1e_pair, cmdp_rollout_plan.h), compact index
//          x, start state = index 0.  FOUR images (pair q = a0 | a1 << 1) of SP2 rows x 32 instances, interleaved by instance
//          like the single form's two: row (x, q) of instance i at byte q * 2^ash2 + x * 128 + 4 i, SP2 = |E| padded to a power
//          of two (DeepSea(30): |E| = 225, SP2 = 256, 4 x 32 KB = the 128 KB of the single form's two images of 512).  Dword =
//          {pair count : 16 | word : 16}, word = x'' << 7 | code(s, a0) | code(s', a1) << 2.
//   step   the bit window of a chunk is the single form's (32 action bits from the wavefront's Philox ring), consumed from the
//          BOTTOM, a0 first then a1: v_and_or_b32 ((window << ash2) & 3 << ash2 | lane base: image offset and bank) .
//          v_bfi_b32 (the row bits of the word under the state mask) . v_lshrrev_b32 (window >>= 2, VOP2) . ds_add_rtn_u32
//          (counts the pair row, returns the next word) . v_alignbit_b32 (w, cw, 4: both codes).  Pair j of a half chunk lands
//          at bits 4 j of the code word: step j at bits 2 j, the layout k_reward_scan reads -- the scan does not change.
//   rounds as in the single form (wavefront w owns a contiguous range of the segment's episodes, eight a round, four chains a
//          lane).  The segment's last round may have fewer than eight episodes: its idle chains walk from index 0 adding
//          ZERO, and their code stores are predicated (the round body is compiled twice).
//   flush  the four counts of (x, instance) go to a second departure image in the HBM layout of the table (two dwords per
//          (x, instance): pairs (0, a1), (1, a1) for a1 = 0, 1) by two returnless 64-bit atomics.  k_epi_fold turns them into
//          arrivals: a pair count c at (s, a0, a1) adds c to the arrivals of (s', a0) and of (s'', a1).  A count stays below
//          2^16: a segment has at most K1E_SEG / 2 pair steps per instance.
//   end    every instance is back at its start state with in-episode time 0; cur, hstep, last_obs, n_trans, n_reset,
//          prev_start, seg_h0 (= 0) and dep_res are written as the single form writes them for that case.
// Staging, the per-wavefront Philox rings, produce, the fetch of the next group's image under the last round, the two barriers
// per group and the code stores through scalar bases are the single form's.
#pragma once

#include <type_traits>

// The kernel's text is cmdp_k1e_pair_body.h, compiled once per bit source
#define K1E_PAIR_FORM 1
#include "cmdp_k1e_pair_body.h"
#undef K1E_PAIR_FORM
#define K1E_PAIR_FORM 3
#include "cmdp_k1e_pair_body.h"
#undef K1E_PAIR_FORM
