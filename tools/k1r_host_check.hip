// k1r_host_check -- the reward scan's lane code (csrc/cmdp_k1e.h: K1rLane, k1r_scan, k1r_single, k1r_slow) as a stand-alone
// HOST program: random segments of code words against a plain float64 loop in transition order, compared bit for bit.  It
// exists to be built with the host sanitizers (nothing of it runs on a GPU, nothing is loaded into another process):
//   mkdir -p build && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Icolosseum_amd/csrc -o build/k1r_host_check tools/k1r_host_check.hip
//   build/k1r_host_check [segments = 20000] [seed = 1]
// Exit status 0: every sum equal; the counters of the paths taken are printed.
#include "../include/cmdp.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "cmdp_kernels.h"
#include "cmdp_k1e.h"

namespace {
struct RewardSet {
  int n;
  double v[4], p[4];
};
const double V900 = 1.0 / 900.0;
const RewardSet kSets[] = {
    {2, {0.0, V900}, {0.5, 0.5}},
    {3, {0.0, V900, 1.0}, {0.5, 0.5, 0.0}},
    {1, {0.125}, {1.0}},
    {4, {0.0, 0.0, 0.0, V900}, {0.25, 0.25, 0.25, 0.25}},
    {3, {0.0, V900, 1.0}, {0.499, 0.499, 0.002}},
    {3, {0.0, 0.5, 1.0}, {0.5, 0.3, 0.2}},
    {4, {0.0, 0.5, 1.0, 0.25}, {0.4, 0.2, 0.2, 0.2}},
    {4, {0.0, 0.5, 0x1p-53, 0.75 + 0x1p-45}, {0.4, 0.2, 0.2, 0.2}},
    {2, {0.0, 0.25}, {0.5, 0.5}},
    {2, {0.0, 0x1p-53}, {0.5, 0.5}},
    {2, {0.0, 5e-324}, {0.5, 0.5}},
    {2, {0.0, -0.25}, {0.5, 0.5}},
    {2, {0.0, 1.0}, {0.7, 0.3}},
};
const int kHorizons[] = {1, 2, 3, 5, 9, 17, 30, 31, 32, 33, 45, 64, 70};
}  // namespace

int main(int argc, char** argv) {
  const long n_seg = argc > 1 ? std::atol(argv[1]) : 20000;
  std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1ull);
  auto below = [&](uint64_t n) { return (uint64_t)(rng() % n); };
  long long total[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long bad = 0;
  for (long it = 0; it < n_seg; ++it) {
    const RewardSet& rs = kSets[below(sizeof(kSets) / sizeof(kSets[0]))];
    const int H = kHorizons[below(sizeof(kHorizons) / sizeof(kHorizons[0]))];
    const int nch = (H + 31) / 32, h0 = (int)below((uint64_t)H);
    const int64_t n_steps = 1 + (int64_t)below((uint64_t)(70 * H));
    const double starts[] = {0.0, 1.3125, std::nextafter(2.0, 0.0), 600.0 * (double)below(1u << 20) / (double)(1u << 20), 0x1p40 + 0.5,
                             1e-3, 0x1p53 * V900 - 40.0 * V900, 0x1p51 - 1.25, 0x1p60};
    const double s0 = starts[below(sizeof(starts) / sizeof(starts[0]))];
    const int64_t E = ((int64_t)h0 + n_steps + H - 1) / H;
    std::vector<uint64_t> words((size_t)(E * nch), 0ull);
    double want = s0;
    for (int64_t t = 0; t < n_steps; ++t) {
      const double u = (double)(rng() >> 11) * 0x1p-53;
      int c = 0;
      double acc = rs.p[0];
      while (c + 1 < rs.n && u >= acc) acc += rs.p[++c];
      while (rs.p[c] == 0.0) --c;
      const int64_t g = t + h0, e = g / H, j = g % H - (e == 0 ? h0 : 0);
      words[(size_t)(e * nch + j / 32)] |= (uint64_t)c << (2 * (j % 32));
      want += rs.v[c];
    }
    double r[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < rs.n; ++c) r[c] = rs.v[c];
    K1rLane L;
    k1r_init(L, r, rs.n, H, nch, h0, n_steps, s0);
    if (L.W != (int)words.size()) { std::printf("segment %ld: %d words expected, %zu made\n", it, L.W, words.size()); return 2; }
    K1rHostLoader ld{words.data(), L.W};
    K1rStats st;
    k1r_scan(L, ld, st);
    const double got = k1r_sum(L);
    if (std::memcmp(&got, &want, sizeof got) != 0 && !(got == want)) {
      if (++bad <= 10) std::printf("MISMATCH segment %ld: H %d h0 %d steps %lld set %d s0 %a: %a != %a\n", it, H, h0, (long long)n_steps,
                                   (int)(&rs - kSets), s0, got, want);
    }
    for (int i = 0; i < 8; ++i) total[i] += st.n[i];
  }
  std::printf("%ld segments, %ld mismatches; plain %lld slow %lld word %lld rebase %lld | single %lld cross %lld fadd %lld\n", n_seg, bad,
              total[0], total[1], total[2], total[3], total[4], total[5], total[6]);
  return bad ? 1 : 0;
}
