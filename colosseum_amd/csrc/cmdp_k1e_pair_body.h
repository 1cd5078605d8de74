// cmdp_k1e_pair_body.h -- the text of K1E's pair kernel, included by cmdp_k1e_pair.h once per K1E_PAIR_FORM: 1 (the action bits
// are the Philox stream's) and 3 (they come from p.abits: CMDP_POLICY_RANDOM_REFERENCE, K16 of cmdp_actions.h).  Only
// `produce` differs.  Two specialisations of one text, not one function called by two kernels: form 1 is then compiled from
// exactly the tokens it always had, whatever form 3 needs.
template <>
__global__ void __launch_bounds__(K1E_THREADS) __attribute__((amdgpu_waves_per_eu(5, 5))) k_rollout_epi<K1E_PAIR_FORM>(EnvTables t, K1ePlan p, int n_steps,
                                                                                                       int32_t* __restrict__ last_obs) {
  extern __shared__ __align__(16) unsigned char smem[];
  // (as the single form: the walk takes the issue slots first, the reward scan of the previous launch what is left)
  if ((t.B + K1E_NI - 1) / K1E_NI > (int)gridDim.x) __builtin_amdgcn_s_setprio(3);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int inst = lane & (K1E_NI - 1), sub = lane >> 5;
  const int H = p.H;
  const int n_ep = n_steps / H;                           // the segment: n_ep whole episodes from the start state
  const int n_groups = (t.B + K1E_NI - 1) / K1E_NI;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;   // 0: no static LDS here
  const uint32_t ash2 = (uint32_t)p.ash2;
  const uint32_t tab_bytes = 4u << ash2;
  const uint32_t i_words = (1u << ash2) >> 2;             // dwords of one image
  uint32_t* tab = reinterpret_cast<uint32_t*>(smem);
  const uint32_t RD = (uint32_t)p.ring_blocks * 4u;      // ring dwords per instance
  uint32_t* ring = reinterpret_cast<uint32_t*>(smem + tab_bytes) + (size_t)wave * RD * K1E_NI;   // this wavefront's ring
  const uint32_t lbase = lds0 + 4u * (uint32_t)inst;     // the lane's bank
  const uint32_t smask = (1u << ash2) - 128u;             // the row field of a word: (SP2 - 1) << 7
  const uint32_t qmask = 3u << ash2;                      // the image of a pair
  const int nch = p.nch;
  const int nj = p.pgdw / K1E_THREADS;                    // rounds of the workgroup over a group's image (<= 16)

  // the loads of group g (k = (a1 * SP2 + x) * 32 + i of the interleaved HBM image: coalesced; at most 16 dwords per thread)
  auto fetch_table = [&](int g, uint32_t (&pair)[16]) {
    const uint32_t* src = p.ptab + (size_t)g * (size_t)p.pgdw;
    uint32_t tid_o = (uint32_t)tid;
    int nj_o = nj;
    asm volatile("" : "+s"(src), "+v"(tid_o), "+s"(nj_o));
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
    r.hcs = (uint32_t)t.start_state[t.start_off[bb]];   // (in-episode time 0 and current state = start state: the launcher's condition)
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
    // ---- stage: {count 0 | pair word}; dword k of the HBM image holds the words of pairs (0, a1) and (1, a1), a1 = k >= i_words ----
    // (an image is whole rounds of the workgroup's 1024 lanes, so a1 is uniform per round j: a scalar offset.  Pinned to this
    // place like the tests j < nj: hoisted out of the group loop, thirty-two LDS addresses would sit in registers under the walk)
    int nj_s = nj;
    uint32_t tid_s = (uint32_t)tid, iw_s = i_words;
    asm volatile("" : "+s"(nj_s), "+v"(tid_s), "+s"(iw_s));
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j < nj_s) {   // (pgdw = 2 i_words: k + a1 * i_words + i_words < 4 i_words)
        const uint32_t k0 = tid_s + ((uint32_t)(j * K1E_THREADS) + ((uint32_t)(j * K1E_THREADS) >= iw_s ? iw_s : 0u));
        tab[k0] = cur_pair[j] & 0xffffu;
        tab[k0 + iw_s] = cur_pair[j] >> 16;
      }
    }
    __syncthreads();   // the image is complete before any wavefront walks it
    const uint2 key = make_uint2(cur_regs.key_x, cur_regs.key_y);
    const unsigned long long ntr = (unsigned long long)cur_regs.ntr_lo | ((unsigned long long)cur_regs.ntr_hi << 32);
    const uint32_t ntr_lo = (uint32_t)ntr;
    const int32_t start = (int32_t)cur_regs.hcs;
    const unsigned long long blk0 = ntr >> 7;               // first Philox block of the segment
    const int off0 = (int)(ntr & 127ull);

    // the action bits: the single form's rings (cmdp_k1e.h), in-episode time 0 at the start of the segment
    int next_blk = 0;   // first block (relative to blk0) of this wavefront's range not made yet
    auto produce = [&](int e_lo) {   // e_lo: the round's first episode (wave-uniform)
      if (!owner) return;
      const int tlo = e_lo * H;
      const int thi = min(n_steps, (e_lo + 2 * K1E_EPL) * H);
      if (tlo >= thi) return;
      const int blo = (off0 + tlo) >> 7, bhi = (off0 + thi - 1) >> 7;
      int sub_o = sub;
      asm volatile("" : "+v"(sub_o));
      for (int rb = max(blo, next_blk) + sub_o; rb <= bhi; rb += 2) {
        const unsigned long long blk = blk0 + (unsigned long long)rb;
        uint32_t w[4];
#if K1E_PAIR_FORM == 3
        (void)key;
        const uint4 v = p.abits[(size_t)rb * (size_t)t.B + (size_t)b];
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#else
        philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), 2u, 0u, key.x, key.y, w);
#endif
        const uint32_t d0 = ((uint32_t)blk & ((uint32_t)p.ring_blocks - 1u)) << 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) ring[(size_t)(d0 + j) * K1E_NI + inst] = w[j];
      }
      next_blk = bhi + 1;
    };

    // one pair step of all the lane's chains: the atomics of all chains are issued before the first is waited for
    auto steps = [&](uint32_t (&wh)[K1E_EPL], uint32_t (&w)[K1E_EPL], const uint32_t (&addv)[K1E_EPL], uint32_t (&cw)[K1E_EPL]) {
      uint32_t ra[K1E_EPL];
#pragma unroll
      for (int c = 0; c < K1E_EPL; ++c) {
        uint32_t tq;
        asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(tq) : "v"(wh[c]), "s"(qmask), "v"(lbase));
        asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(ra[c]) : "s"(smask), "v"(w[c]), "v"(tq));
        wh[c] >>= 2;
      }
#pragma unroll
      for (int c = 0; c < K1E_EPL; ++c)   // counts the pair row the chain leaves, returns {old count | next pair word}
        w[c] = __hip_atomic_fetch_add((k1e_lds_u32)(uintptr_t)ra[c], addv[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
      for (int c = 0; c < K1E_EPL; ++c) cw[c] = __builtin_amdgcn_alignbit(w[c], cw[c], 4u);
    };
    auto walk = [&](int n, uint32_t (&wh)[K1E_EPL], uint32_t (&w)[K1E_EPL], const uint32_t (&addv)[K1E_EPL], uint32_t (&cw)[K1E_EPL]) {
      int j = 0;
      for (; j + 1 < n; j += 2) { steps(wh, w, addv, cw); steps(wh, w, addv, cw); }
      if (j < n) steps(wh, w, addv, cw);
    };
    // this wavefront's ring as LDS byte addresses: dword d of the lane's instance at lbase + ring_sbase + (128 d & ring_mask)
    const uint32_t ring_sbase = tab_bytes + (uint32_t)wave * RD * (4u * K1E_NI);
    const uint32_t ring_mask = (RD - 1u) << 7;

    // a round of eight episodes e_lo .. e_lo + 7; RAGGED: some of them are past the segment's last one (e >= n_ep)
    auto round = [&](int e_lo, auto ragged) {
      constexpr bool RAGGED = decltype(ragged)::value;
      int e0 = sub * K1E_EPL;
      uint32_t ring_base = ring_sbase;
      asm volatile("" : "+v"(e0), "+s"(ring_base));   // (pinned to the round, as in the single form's interior round)
      e0 += e_lo;
      const uint32_t ring_lane = lbase + ring_base;          // (a multiple of the ring's size + 4 i: the plan's condition)
      const uint32_t a00 = ntr_lo + (uint32_t)(e0 * H);      // chain 0's first transition, as a stream position
      const uint32_t o00 = a00 << 2;                          // ... and as 128 x its ring dword (+ bits below 7, masked off)
      uint32_t addv[K1E_EPL], w[K1E_EPL];
      uint32_t one = 0x10000u;
      asm volatile("" : "+v"(one));
#pragma unroll
      for (int c = 0; c < K1E_EPL; ++c) {
        addv[c] = RAGGED ? (e0 + c < n_ep ? 0x10000u : 0u) : one;   // an idle chain adds zero
        w[c] = 0u;                                                    // every chain starts from the start state: index 0
      }
      for (int ch = 0; ch < nch; ++ch) {
        const int P = __builtin_amdgcn_readfirstlane(min(32, H - 32 * ch) >> 1);   // pairs of the chunk (H is even)
        uint32_t d0[K1E_EPL], d1[K1E_EPL], bits[K1E_EPL], wh[K1E_EPL], clo[K1E_EPL], chi[K1E_EPL];
#pragma unroll
        for (int c = 0; c < K1E_EPL; ++c) {
          const uint32_t so = (uint32_t)__builtin_amdgcn_readfirstlane(4 * (c * H + 32 * ch));
          d0[c] = *(k1e_lds_u32)(uintptr_t)(((o00 + so) & ring_mask) | ring_lane);
          d1[c] = *(k1e_lds_u32)(uintptr_t)(((o00 + (so + 128u)) & ring_mask) | ring_lane);
        }
#pragma unroll
        for (int c = 0; c < K1E_EPL; ++c) {
          bits[c] = __builtin_amdgcn_alignbit(d1[c], d0[c], a00 + (uint32_t)(c * H));   // transition j of the chunk at bit j
          wh[c] = bits[c] << ash2;                                                        // its pair at bits ash2 + 1 : ash2
          clo[c] = 0u; chi[c] = 0u;
        }
        const int P0 = __builtin_amdgcn_readfirstlane(min(P, 8));
        walk(P0, wh, w, addv, clo);
        if (P > 8) {
#pragma unroll
          for (int c = 0; c < K1E_EPL; ++c) wh[c] = bits[c] >> (16u - ash2);   // (ash2 <= 15) transition 16 at bit ash2
          walk(P - 8, wh, w, addv, chi);
        }
        if (!(p.debug & 8)) {
          const uint32_t wi = ((uint32_t)e0 * (uint32_t)nch + (uint32_t)ch) * (uint32_t)t.B + (uint32_t)b;
          const uint32_t o8 = wi << 3;                               // (< 2^31: the launcher's condition)
          const uint32_t cstride = (uint32_t)nch * (uint32_t)t.B;   // words between two consecutive episodes
#pragma unroll
          for (int c = 0; c < K1E_EPL; ++c) {
            const uint32_t lo = P0 < 8 ? clo[c] >> (32 - 4 * P0) : clo[c];
            const uint32_t hi = P > 8 ? (P < 16 ? chi[c] >> (32 - 4 * (P - 8)) : chi[c]) : 0u;
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            u32x2 v;
            v.x = lo; v.y = hi;
            typedef __attribute__((address_space(1))) unsigned char* k1e_glb_u8;   // (global, not flat, stores)
            k1e_glb_u8 cb = (k1e_glb_u8)(uintptr_t)p.codes + (size_t)((uint32_t)c * cstride) * 8;
            asm volatile("" : "+s"(cb));
            if (!RAGGED || e0 + c < n_ep)
              __builtin_nontemporal_store(v, (__attribute__((address_space(1))) u32x2*)(cb + (size_t)o8));
          }
        }
      }
    };

    const int R = p.n_pass;   // rounds per wavefront: wavefront w owns episodes [8 R w, 8 R (w + 1)) of the segment
    for (int pass = 0; pass < R; ++pass) {
      const int e_lo = (wave * R + pass) * 2 * K1E_EPL;
      if (!(p.debug & 4)) produce(e_lo);
      // the next group's table image: in flight under the whole of this wavefront's last round
      if (pass == R - 1 && more) fetch_table(g + (int)gridDim.x, cur_pair);
      __builtin_amdgcn_wave_barrier();
      if (owner && !(p.debug & 1)) {
        if (e_lo + 2 * K1E_EPL <= n_ep) round(e_lo, std::false_type{});
        else if (e_lo < n_ep) round(e_lo, std::true_type{});
      }
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();   // every wavefront has walked its range: the counts are final

    if (wave == 0 && sub == 0 && owner) {
      const unsigned long long resets = (unsigned long long)n_ep;
      t.n_trans[b] = ntr + (unsigned long long)n_steps;
      t.n_reset[b] += resets;
      if (resets) {
        t.prev_start[b] = t.last_start[b];   // (as K1L: env_reset's bookkeeping of the one start state)
        t.cur[b] = start;                     // the last transition ended an episode
        t.hstep[b] = 0;
        if (last_obs) last_obs[b] = start;
      }
      p.seg_h0[b] = 0;
      if (!(p.debug & 2)) p.dep_res[b] += (int32_t)resets;   // episode resets: they count the start state (k_epi_fold)
    }
    // ---- flush: the pair counts to the pair image in HBM (the table's layout), one returnless 64-bit atomic per dword of it:
    // pair (0, a1) in the low half, (1, a1) in the high half; the host's overflow guard keeps every count below 2^31 ----
    if (!(p.debug & 2)) {
      typedef __attribute__((address_space(1))) unsigned long long* k1e_glb_u64;
      unsigned long long* dep = reinterpret_cast<unsigned long long*>(p.dep2) + (size_t)g * (size_t)p.pgdw;
      uint32_t tid_o = (uint32_t)tid;
      int nj_f = nj;
      uint32_t iw_f = i_words;
      asm volatile("" : "+s"(dep), "+v"(tid_o), "+s"(nj_f), "+s"(iw_f));
      const k1e_glb_u64 gdep = (k1e_glb_u64)(uintptr_t)dep;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t k = tid_o + (uint32_t)(j * K1E_THREADS);
        if (j < nj_f) {
          const uint32_t k0 = k + ((uint32_t)(j * K1E_THREADS) >= iw_f ? iw_f : 0u);
          const uint32_t c0 = tab[k0] >> 16, c1 = tab[k0 + iw_f] >> 16;
          if (c0 | c1)
            __hip_atomic_fetch_add(gdep + k, (unsigned long long)c0 | ((unsigned long long)c1 << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
    if (!more) break;
    fetch_scalars(g + (int)gridDim.x, cur_regs);
    __syncthreads();   // the counts are read: the next group's image may overwrite them
  }
}
