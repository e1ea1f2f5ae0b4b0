// Host check of the leaf carry's arithmetic (jda_amd/csrc/kernels.h: carry_bits / carry_rounds / carry_fits / carry_pack /
// carry_unpack), the functions k_filter0 packs with and k_finish unpacks with: whole 64-lane queue entries of random
// leaves, written round by round as k_filter0 does and read cart by cart as k_finish does.  tests/test_finish_carry.py
// builds and runs it; no device is needed.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "kernels.h"

int main() {
  using namespace jda;
  const int leaf_ns[] = {2, 4, 8, 16, 32}, Ks[] = {64, 100, 540, 682, 2000};
  uint64_t rng = 0x9e3779b97f4a7c15ull;
  auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 32); };
  int bad = 0;
  for (int leaf_n : leaf_ns)
    for (int K : Ks) {
      const int bits = carry_bits(leaf_n), rounds = carry_rounds(K);
      const bool fits = carry_fits(leaf_n, K);
      std::printf("leaf_n %d K %d fits %d\n", leaf_n, K, fits ? 1 : 0);
      if ((1 << bits) < leaf_n || (bits > 0 && (1 << (bits - 1)) >= leaf_n) || rounds * 64 < K || (rounds - 1) * 64 >= K) bad++;
      if (fits != (bits * rounds <= 32)) bad++;
      if (!fits) continue;
      // every first round a window can start at (k_filter0: kbeg & ~63), lanes past cart K - 1 repeat that cart's leaf
      for (int r0 = 0; r0 < rounds; r0++) {
        std::vector<int> leaf(K);
        for (int k = 0; k < K; k++) leaf[k] = (int)(next() % (uint32_t)leaf_n);
        uint32_t word[64] = {0};
        for (int r = r0; r < rounds; r++)
          for (int lane = 0; lane < 64; lane++) {
            const int k = r * 64 + lane < K ? r * 64 + lane : K - 1;
            word[lane] = carry_pack(word[lane], leaf[k], bits, r);
          }
        for (int k = r0 * 64; k < K; k++)
          if (carry_unpack(word[k & 63], bits, k >> 6) != leaf[k]) bad++;
      }
    }
  if (bad) { std::printf("carry FAILED: %d\n", bad); return 1; }
  std::printf("carry ok\n");
  return 0;
}
