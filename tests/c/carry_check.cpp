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
  // the word's edge (tests/test_finish_launches.py, carry_*): bits * rounds == 32 puts the last round's leaf in the top bits,
  // bit 31 included; 3 x 10 = 30 leaves two bits unused; one cart more and the model does not carry.  The LARGEST leaf in
  // every round: every bit of the word set, every round read back.
  const int edge[][3] = {{4, 1024, 1}, {4, 1025, 0}, {16, 512, 1}, {16, 513, 0}, {256, 256, 1}, {256, 257, 0}, {8, 640, 1}, {8, 641, 0}};
  for (const auto& e : edge) {
    const int leaf_n = e[0], K = e[1], bits = carry_bits(leaf_n), rounds = carry_rounds(K);
    std::printf("edge leaf_n %d K %d bits %d fits %d\n", leaf_n, K, bits * rounds, carry_fits(leaf_n, K) ? 1 : 0);
    if (carry_fits(leaf_n, K) != (e[2] != 0)) bad++;
    if (!e[2]) continue;
    uint32_t word = 0;
    for (int r = 0; r < rounds; r++) word = carry_pack(word, leaf_n - 1, bits, r);
    if (bits * rounds == 32 && word != 0xffffffffu) bad++;
    if (bits * rounds == 30 && word != 0x3fffffffu) bad++;
    for (int r = 0; r < rounds; r++) if (carry_unpack(word, bits, r) != leaf_n - 1) bad++;
    // ... and a lone top-round leaf with its top bit set comes back from a word that is otherwise zero
    const uint32_t top = carry_pack(0u, leaf_n / 2, bits, rounds - 1);
    if (carry_unpack(top, bits, rounds - 1) != leaf_n / 2 || (bits * rounds == 32 && top != 0x80000000u)) bad++;
  }
  if (bad) { std::printf("carry FAILED: %d\n", bad); return 1; }
  std::printf("carry ok\n");
  return 0;
}
