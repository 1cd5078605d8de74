// cmdp_actions.h -- K16 k_mt_actions: the reference's random policy, generated on the device.
//
// The reference's RandomActor (colosseum/agent/actors/random.py:34-47) draws RandomState(seed).randint(0, A, 50 000) blocks
// and pops them in order.  Consecutive randint calls continue one word stream, so the blocks are simply the stream:
//   action = the instance's next raw MT19937 word, tempered and masked with the smallest 2^k - 1 >= A - 1; a word whose
//   masked value exceeds A - 1 is rejected (one word per attempt); A = 1 draws nothing.
// The state of an instance is numpy's own representation (RandomState.get_state()): key[624] AFTER the block twist and pos in
// 0 .. 624, pos = 624 right after seeding (the next draw twists first).  The agents' mt_next_word (cmdp_device.h) twists word
// by word and keeps a different representation of the same stream; the two are not mixed.
//
// k_mt_actions -- one wavefront (a 64-thread workgroup) per instance, the 624 words in LDS (2.5 KB):
//   twist   word k needs the OLD k, k + 1 and, for k < 227, the old k + 397; from 227 on the NEW k - 227, and word 623 the new
//           0 and 396.  Sixty-four words at a time in ascending order meet all of that: a chunk reads before it writes, the
//           word after it is still old, and k - 227 lies in an earlier chunk (227 >= 64).  Ten chunks per block of 624.
//   draw    64 words per pass -- for a block that will be consumed whole, the chunk just twisted, still in its register --
//           temper in the lane, then
//           BITS (A = 2: action = word & 1, no rejection): a wave ballot yields 64 actions at once; they are appended to a
//             64-bit accumulator that starts at bit n_trans[b] & 127 and leave as 128-bit blocks abits[block][B] -- the action
//             of the launch's j-th transition is bit (n_trans[b] + j) & 127 of block ((n_trans[b] & 127) + j) >> 7, least
//             significant bit of word 0 first: exactly how K1E addresses its ring (blk0, off0 in cmdp_k1e.h);
//           BYTES (any A <= 64): accepted words are compacted by ballot and prefix count into int8 actions[n][B], the layout
//             of CMDP_POLICY_HOST_ACTIONS.
//   end     exactly n actions; key and pos are left where numpy's would be, so the next launch continues the stream.
//   bound   acceptance is at least 1/2, so a launch that has consumed more than mta_word_bound(n) words stops, fills the
//           rest with action 0 and raises *fail (read by the host at its next synchronisation): no unbounded spin.
// The twist of one word, the tempering, the mask and the accept test are shared with the host twins cmdp_mt_randint /
// cmdp_mt_action_bits (include/cmdp.h), which the CPU tests hold against numpy itself.
#pragma once

#define MTA_N 624
#define MTA_M 397
#define K16_THREADS 64

// word k of the next block from (old k, k + 1, and k + 397 -- or the new k - 227)
__host__ __device__ __forceinline__ uint32_t mta_twist(uint32_t k0, uint32_t k1, uint32_t km) {
  const uint32_t y = (k0 & 0x80000000u) | (k1 & 0x7fffffffu);
  return km ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
__host__ __device__ __forceinline__ uint32_t mta_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}
// smallest 2^k - 1 >= mx (mx = A - 1)
__host__ __device__ __forceinline__ uint32_t mta_mask(uint32_t mx) {
  uint32_t m = mx;
  m |= m >> 1; m |= m >> 2; m |= m >> 4; m |= m >> 8; m |= m >> 16;
  return m;
}
// the attempt made with one tempered word: its masked value, accepted when it does not exceed mx
__host__ __device__ __forceinline__ bool mta_accept(uint32_t word, uint32_t mask, uint32_t mx, uint32_t* v) {
  *v = word & mask;
  return *v <= mx;
}
// words a draw of n actions may consume before it is failed (expected: at most 2 n)
__host__ __device__ __forceinline__ long long mta_word_bound(long long n) { return 8 * n + 4096; }

// ---- host twins: the state of one stream, updated in place ----
inline void mta_twist_block(uint32_t* key) {
  for (int k = 0; k < MTA_N; ++k)
    key[k] = mta_twist(key[k], key[k + 1 == MTA_N ? 0 : k + 1], key[k < MTA_N - MTA_M ? k + MTA_M : k - (MTA_N - MTA_M)]);
}
inline uint32_t mta_next_word(uint32_t* key, int32_t* pos) {
  if (*pos >= MTA_N) { mta_twist_block(key); *pos = 0; }
  return mta_temper(key[(*pos)++]);
}
// RandomState.randint(0, A, n); false when the word bound is exceeded (the state is where the draw stopped)
inline bool mta_randint_host(uint32_t* key, int32_t* pos, int A, long long n, int8_t* out) {
  if (A == 1) { for (long long j = 0; j < n; ++j) out[j] = 0; return true; }
  const uint32_t mx = (uint32_t)A - 1u, mask = mta_mask(mx);
  const long long bound = mta_word_bound(n);
  long long used = 0;
  for (long long j = 0; j < n; ++j) {
    uint32_t v;
    do {
      if (used++ > bound) return false;
    } while (!mta_accept(mta_next_word(key, pos), mask, mx, &v));
    out[j] = (int8_t)v;
  }
  return true;
}
// RandomState.randint(0, 2, n) packed: action j at bit (bit_offset + j) & 31 of word (bit_offset + j) >> 5; no other bit of
// `out` is changed
inline void mta_action_bits_host(uint32_t* key, int32_t* pos, long long n, long long bit_offset, uint32_t* out) {
  for (long long j = 0; j < n; ++j) {
    const long long q = bit_offset + j;
    const uint32_t bit = 1u << (q & 31);
    if (mta_next_word(key, pos) & 1u) out[q >> 5] |= bit; else out[q >> 5] &= ~bit;
  }
}

// ---- K16 ----
template <bool BITS>
__global__ void __launch_bounds__(K16_THREADS) k_mt_actions(uint32_t* __restrict__ key_all, int32_t* __restrict__ pos_all,
                                                            const unsigned long long* __restrict__ n_trans, int B, int A, int n,
                                                            int nblk, uint4* __restrict__ abits, int8_t* __restrict__ actions,
                                                            int32_t* __restrict__ fail) {
  __shared__ uint32_t key[MTA_N];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  uint32_t* gk = key_all + (size_t)b * MTA_N;
  for (int k = lane; k < MTA_N; k += K16_THREADS) key[k] = gk[k];
  int pos = __builtin_amdgcn_readfirstlane(pos_all[b]);
  __syncthreads();
  // each(c, nv): what the caller does with the lane's new word c + lane of every chunk (0 past the block's end)
  auto twist = [&](auto&& each) {
    // (unrolled: which neighbour a chunk reads -- k + 397 or k - 227, the wrap of k + 1 -- is then known per chunk)
#pragma unroll
    for (int c = 0; c < MTA_N; c += K16_THREADS) {
      const int k = c + lane;
      uint32_t nv = 0u;
      if (k < MTA_N) nv = mta_twist(key[k], key[k + 1 == MTA_N ? 0 : k + 1], key[k < MTA_N - MTA_M ? k + MTA_M : k - (MTA_N - MTA_M)]);
      __syncthreads();   // the chunk has read before it writes
      if (k < MTA_N) key[k] = nv;
      __syncthreads();
      each(c, nv);
    }
  };
  auto nothing = [](int, uint32_t) {};
  if constexpr (BITS) {
    // 64-bit word w of the instance: half w & 1 of block w >> 1
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(abits) + 2 * (size_t)b;
    const int n_words = 2 * nblk;
    auto put = [&](int w, unsigned long long v) {
      if (w < n_words) dst[(size_t)(w >> 1) * 2 * (size_t)B + (size_t)(w & 1)] = v;
    };
    const int off0 = (int)(n_trans[b] & 127ull);
    unsigned long long acc = 0ull;
    int nacc = off0 & 63, widx = off0 >> 6;
    if (widx == 1 && lane == 0) put(0, 0ull);
    // the next k (<= 64) actions, bit j of bal the j-th, join the accumulator; a full word leaves
    auto append = [&](unsigned long long bal, int k) {
      const unsigned long long lo = acc | (bal << nacc), hi = nacc ? bal >> (64 - nacc) : 0ull;
      const int tot = nacc + k;
      if (tot >= 64) {
        if (lane == 0) put(widx, lo);
        ++widx; acc = hi; nacc = tot - 64;
      } else {
        acc = lo; nacc = tot;
      }
    };
    int produced = 0;
    while (produced < n) {
      if (pos >= MTA_N) {
        if (n - produced >= MTA_N) {
          // the whole block will be consumed: every chunk is tempered and balloted as it is twisted, from the register that
          // holds the new word -- no second pass over LDS (all but the two ends of a launch)
          twist([&](int c, uint32_t nv) {
            const int k = min(K16_THREADS, MTA_N - c);
            append(__builtin_amdgcn_ballot_w64(lane < k && (mta_temper(nv) & 1u) != 0u), k);
          });
          produced += MTA_N;   // (pos stays 624: the block is used up)
          continue;
        }
        twist(nothing);
        pos = 0;
      }
      const int k = min(K16_THREADS, min(MTA_N - pos, n - produced));
      append(__builtin_amdgcn_ballot_w64(lane < k && (mta_temper(key[pos + lane]) & 1u) != 0u), k);
      pos += k; produced += k;
    }
    if (nacc > 0) {
      if (lane == 0) put(widx, acc);
      ++widx;
    }
    for (int w = widx + lane; w < n_words; w += K16_THREADS) put(w, 0ull);   // whole blocks: the walk loads all four dwords
  } else {
    int8_t* dst = actions + b;
    if (A == 1) {
      for (int j = lane; j < n; j += K16_THREADS) dst[(size_t)j * (size_t)B] = 0;
      return;   // (nothing drawn: the state stays)
    }
    const uint32_t mx = (uint32_t)A - 1u, mask = mta_mask(mx);
    const long long bound = mta_word_bound(n);
    long long used = 0;
    int produced = 0;
    while (produced < n) {
      if (used > bound) {
        if (lane == 0) atomicOr(fail, 1);
        for (int j = produced + lane; j < n; j += K16_THREADS) dst[(size_t)j * (size_t)B] = 0;
        break;
      }
      if (pos >= MTA_N) { twist(nothing); pos = 0; }
      const int k = min(K16_THREADS, MTA_N - pos);
      uint32_t v = 0u;
      const bool ok = lane < k && mta_accept(mta_temper(key[pos + lane]), mask, mx, &v);
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(ok);
      const int pre = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
      const int cnt = __builtin_popcountll(bal), need = n - produced;
      if (ok && pre < need) dst[(size_t)(produced + pre) * (size_t)B] = (int8_t)v;
      if (cnt >= need) {   // the word of the last action taken ends the draw: the words after it stay in the stream
        const unsigned long long last = __builtin_amdgcn_ballot_w64(ok && pre == need - 1);
        const int used_here = __builtin_ctzll(last) + 1;
        pos += used_here; used += used_here; produced = n;
      } else {
        pos += k; used += k; produced += cnt;
      }
    }
  }
  __syncthreads();
  for (int k = lane; k < MTA_N; k += K16_THREADS) gk[k] = key[k];
  if (lane == 0) pos_all[b] = pos;
}
