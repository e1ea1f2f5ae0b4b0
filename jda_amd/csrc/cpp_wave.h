// The wave-per-sample form of the dialect-CPP sample-set kernels, once, for k_lbf.hip (a stage's close), k_reval.hip
// (Validate on a resident set) and, for the cart descent, k_mine.hip: one wave per sample, the sample's state in the wave's own
// slice of LDS or -- where a slice does not fit -- in global memory, the same arithmetic on the same values.  Here: the
// slice's layout for device and host, the patch copy into it, Cart::Forward on the split node of cpp_patch.h,
// GenDeltaShape's sum, the similarity transform of a sample (stp_calc_uniform, finish_common.h) on its walk and its sum, and
// the launch of such a kernel (wave_lds_sync / wave_global_sync: kernels_common.h).  k_mine.hip
// uses cart_forward alone; k_reval.hip everything but wave_stage_bytes (it keeps a plain loop of its own).
#pragma once
#include "cpp_patch.h"
#include "finish_common.h"

namespace jda {

namespace {

// A wave's slice of LDS: the shape [dim] doubles at 0, the leaf indicators [K] ints at `lbf`, then -- with_patches -- the
// sample's pbytes patch bytes at `pat` (+ 3: wave_stage_bytes keeps the source's offset inside a dword); every part
// starts on a 16-byte boundary.  The kernels carve their pointers from it, the host takes `bytes`.
struct WaveSlice {
  long long lbf, pat, bytes;
  static __host__ __device__ long long align16(long long v) { return (v + 15) & ~15ll; }
  __host__ __device__ WaveSlice(int dim, int K, long long pbytes, bool with_patches)
      : lbf(align16((long long)dim * 8)), pat(lbf + align16((long long)K * 4)), bytes(pat + (with_patches ? align16(pbytes + 3) : 0)) {}
};

// n bytes global -> LDS by one wave, dwords where the source allows: dst keeps the source's offset inside a dword, so
// the body is aligned on both sides; the head and the tail (at most three bytes each) go bytewise.  Four loads of a lane
// are in flight before its first store.
__device__ __forceinline__ uint8_t* wave_stage_bytes(uint8_t* lds, const uint8_t* __restrict__ src, int n, int lane) {
  const int sh = (int)((uintptr_t)src & 3);
  uint8_t* dst = lds + sh;
  const int head = min(n, (4 - sh) & 3);
  const int body = (n - head) >> 2, tail = n - head - 4 * body;
  if (lane < head) dst[lane] = src[lane];
  const uint32_t* s4 = (const uint32_t*)(src + head);
  uint32_t* d4 = (uint32_t*)(dst + head);
  for (int d0 = 0; d0 < body; d0 += 64 * 4) {
    uint32_t v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { const int d = d0 + u * 64 + lane; if (d < body) v[u] = s4[d]; }
#pragma unroll
    for (int u = 0; u < 4; u++) { const int d = d0 + u * 64 + lane; if (d < body) d4[d] = v[u]; }
  }
  if (lane < tail) dst[head + 4 * body + lane] = src[head + 4 * body + lane];
  return dst;
}

// Cart::Forward (cart.cpp:392-404) of one cart for one lane on the dialect-CPP split node: D - 1 levels down from the root,
// the leaf's index within the cart comes back.  node_at(d, node) loads the record of node `node` on level d -- 1-based, its
// children 2 node and 2 node + 1 -- from wherever the caller keeps its carts (and checks that load in the bounds build);
// offsets(nd) may replace the record's offsets before they are used (k_mine_walk's similarity transform, data.cpp:33-34).
// The landmark ids are checked here, with the shape reads they guard: in the bounds build k_mine_walk has that check too.
struct OffsetsAsStored { __device__ __forceinline__ void operator()(NodeD&) const {} };
template <typename NodeAt, typename Offsets = OffsetsAsStored>
__device__ __forceinline__ int cart_forward(const PatchSet& pat, const double* sh, int D, [[maybe_unused]] int dim,
                                            const NodeAt& node_at, const Offsets& offsets = Offsets{}) {
  int node = 1;
  for (int d = 0; d < D - 1; d++) {
    NodeD nd = node_at(d, node);
    offsets(nd);
    JDA_BC(Bc(0, dim), nd.lm1x2, 2, kBcLandmark); JDA_BC(Bc(0, dim), nd.lm2x2, 2, kBcLandmark);
    const int v = pat.feature(nd, sh[nd.lm1x2], sh[nd.lm1x2 + 1], sh[nd.lm2x2], sh[nd.lm2x2 + 1]);
    node = (v <= nd.th) ? 2 * node : 2 * node + 1;       // cart.cpp:398-401
  }
  return node - (1 << (D - 1));
}

// GenDeltaShape (btcart.cpp:407-424) for shape coordinate j: from 0., + wt[lbf[k]][j] for k = 0 .. K - 1 IN CART ORDER (the
// order decides bits).  A weight row is dim contiguous doubles read across the wave (lane = coordinate); its index is in
// lbf before the add chain starts, so the loads of eight rows are in flight per add.  rows: wt's rows (the bounds build).
__device__ __forceinline__ double gen_delta(const int* lbf, const double* wt, int dim, int K, int j,
                                            [[maybe_unused]] long long rows) {
  double delta = 0.;                                     // Mat_<double>::zeros, btcart.cpp:410
  for (int k0 = 0; k0 < K; k0 += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int r = lbf[min(k0 + u, K - 1)];
      JDA_BC(Bc(0, rows), r, 1, kBcWRow);
      v[u] = wt[(size_t)r * dim + j];
    }
#pragma unroll
    for (int u = 0; u < 8; u++)
      if (k0 + u < K) delta += v[u];                     // btcart.cpp:414-420
  }
  return delta;
}

// stp_mc.Apply on GenDeltaShape's sum (btcart.cpp:422, data.cpp:116-126) with lane = coordinate: `mine` is delta[j], its
// partner delta[j ^ 1] sits in the neighbouring lane (dim is even: both in the same round; every lane of the wave calls this).
__device__ __forceinline__ double stp_apply_lane(const Stp<double>& p, double mine, int j) {
  const double other = __shfl_xor(mine, 1, 64);
  return (j & 1) ? p.scale * (p.r10 * other + p.r11 * mine) : p.scale * (p.r00 * mine + p.r01 * other);   // data.hpp:42-45
}

// How many samples (waves) of a workgroup get a slice of wave_bytes within lds_budget -- the LDS bytes a workgroup may
// take, at most the CU's 160 KB -- up to max_waves; none: the kernel runs from global memory with max_waves waves.
inline WaveLaunch plan_wave_slices(long long wave_bytes, int max_waves, int lds_budget) {
  const long long budget = std::min<long long>(std::max(0, lds_budget), 160 * 1024);
  const int waves = (int)std::min<long long>(max_waves, budget / wave_bytes);
  return waves >= 1 ? WaveLaunch{1, waves, (int)(waves * wave_bytes)} : WaveLaunch{0, max_waves, 0};
}

// Launches the planned form over n samples: `lds` with its slices (dynamic LDS, told to the runtime above 48 KB) or `global`.
template <typename Args>
hipError_t launch_wave_slices(void (*lds)(Args), void (*global)(Args), const Args& a, int n, const WaveLaunch& how, hipStream_t stream) {
  void (*kernel)(Args) = how.lds ? lds : global;
  if (how.lds_bytes > 48 * 1024)
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, how.lds_bytes);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + how.waves - 1) / how.waves)), dim3(64 * how.waves), how.lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace

}  // namespace jda
