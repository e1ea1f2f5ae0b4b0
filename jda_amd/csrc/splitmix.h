// The counter-based SplitMix64 generator of include/jda.h, for host and device: the initial-shape shift of the mining
// entries (k_mine.hip) and the feature pool of jdaGenFeaturePoolCpp (train.cpp) draw from it.
#pragma once
#include <cstdint>

namespace jda {

constexpr uint64_t kGoldenGamma = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ uint64_t splitmix_draw(uint64_t seed, uint64_t c) {   // draw c = 0, 1, ... under `seed`
  return splitmix64(seed + (c + 1) * kGoldenGamma);
}
__host__ __device__ __forceinline__ double splitmix_unit(uint64_t z) { return (double)(z >> 11) * 0x1.0p-53; }   // [0, 1): the top 53 bits

}  // namespace jda
