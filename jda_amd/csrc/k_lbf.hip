// HIP kernel of dialect CPP's stage close for gfx950 (reference src/jda/btcart.cpp:255-292, 390-424): BoostCart::GenLBF --
// every cart of a stage walked over every sample that is still alive -- and GenDeltaShape with the shape update, as one
// pass over a resident sample set.
//   k_lbf   wave = sample.  The sample's o / h / q bytes, its 2L shape doubles and its row of K leaf indicators live in
//           the wave's own slice of LDS (LDS = true), or stay in global memory where a slice does not fit (LDS = false;
//           the same arithmetic on the same values).
//           phase 1  lane = cart, k = lane, lane + 64, ...: Cart::Forward (cart.cpp:392-404) on the dialect-CPP split node
//                    of cpp_patch.h with the identity STParameter -> lbf[k] = k * leafNum + leaf
//           phase 2  lane = shape coordinate, j = lane, lane + 64, ... < 2L: delta[j] from 0, + w[lbf[k]][j] for
//                    k = 0 .. K - 1 IN CART ORDER (the order decides bits), then shape[j] + delta[j] -- the order and form
//                    of k_mine.hip's regression.  A weight row is 2L contiguous doubles read across the wave; its index
//                    sits in LDS before the add chain starts, so the loads of eight carts are in flight per add.
// Whole waves only: no workgroup barrier, a wave synchronises with itself.  No atomics, no log(), fp64 add only.
#include "cpp_patch.h"

namespace jda {

namespace {

__device__ __forceinline__ int lbf_align16(int v) { return (v + 15) & ~15; }

// This wave's writes to global memory before its later reads of them by OTHER lanes of the same wave (LDS = false).
__device__ __forceinline__ void wave_global_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// n bytes global -> LDS by one wave, dwords where the source allows: dst keeps the source's offset inside a dword, so
// the body is aligned on both sides; the head and the tail (at most three bytes each) go bytewise.
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

}  // namespace

template <bool LDS>
__global__ __launch_bounds__(64 * kLbfWaves) void k_lbf(LbfArgs a, int wave_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lbf_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (i >= a.n) return;                                  // (whole waves; no workgroup barrier below)
  const int K = a.K, dim = a.dim;
  const int leaf_n = 1 << (a.D - 1);
  const int pbytes = a.os * a.os + a.hs * a.hs + a.qs * a.qs;
  const double* sh_g = a.shapes + (size_t)i * dim;
  int* lbf_g = a.lbf + (size_t)i * K;
  // the wave's slice: shape [dim] doubles, lbf [K] ints, patches (pbytes + 3) bytes
  double* sh_l = (double*)(lbf_lds + (size_t)wave * wave_bytes);
  int* lbf_l = (int*)((unsigned char*)sh_l + lbf_align16(dim * 8));
  const double* sh = sh_g;
  const int* lbf = lbf_g;
  if (LDS) { sh = sh_l; lbf = lbf_l; }

  if (a.walk) {
    const uint8_t* pat_g = a.patches + (size_t)i * pbytes;
    const uint8_t* pat_p = pat_g;
    if (LDS) {
      pat_p = wave_stage_bytes((uint8_t*)lbf_l + lbf_align16(K * 4), pat_g, pbytes, lane);
      for (int j = lane; j < dim; j += 64) sh_l[j] = sh_g[j];
      wave_lds_sync();
    }
    const PatchSet pat{pat_p, a.os, a.hs, a.qs};
    // ---- phase 1: lane = cart.  Node `node` (1-based, children 2 node and 2 node + 1) of cart k sits level-major in
    //      the table: level d = floor(log2 node) starts at K * (2^d - 1), there cart k's 2^d nodes back to back -- the
    //      roots of the 64 carts of a round are 64 neighbouring records
    [[maybe_unused]] const long long nodes_n = (long long)K * (leaf_n - 1);
    for (int k = lane; k < K; k += 64) {
      int node = 1;
      for (int d = 0; d < a.D - 1; d++) {
        const long long at = (long long)K * ((1 << d) - 1) + (long long)k * (1 << d) + (node - (1 << d));
        JDA_BC(Bc(0, nodes_n), at, 1, kBcNodeTable);
        const LbfNode nd = a.nodes[at];
        JDA_BC(Bc(0, dim), nd.lm1x2, 2, kBcLandmark); JDA_BC(Bc(0, dim), nd.lm2x2, 2, kBcLandmark);
        const int v = pat.feature(nd, sh[nd.lm1x2], sh[nd.lm1x2 + 1], sh[nd.lm2x2], sh[nd.lm2x2 + 1]);
        node = (v <= nd.th) ? 2 * node : 2 * node + 1;   // cart.cpp:398-401
      }
      const int idx = k * leaf_n + (node - leaf_n);      // btcart.cpp:400-403
      lbf_g[k] = idx;
      if (LDS) lbf_l[k] = idx;
    }
  } else if (LDS) {
    for (int k = lane; k < K; k += 64) lbf_l[k] = lbf_g[k];
  }
  if (!a.w) return;
  if (LDS) wave_lds_sync(); else if (a.walk) wave_global_sync();

  // ---- phase 2: lane = shape coordinate; eight rows in flight, added strictly in cart order
  [[maybe_unused]] const long long rows = (long long)K * leaf_n;
  double* out = a.out_shapes + (size_t)i * dim;
  for (int j = lane; j < dim; j += 64) {
    double delta = 0.;                                   // Mat_<double>::zeros, btcart.cpp:410
    for (int k0 = 0; k0 < K; k0 += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int r = lbf[min(k0 + u, K - 1)];
        JDA_BC(Bc(0, rows), r, 1, kBcWRow);
        v[u] = a.w[(size_t)r * dim + j];
      }
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (k0 + u < K) delta += v[u];                   // btcart.cpp:414-420
    }
    out[j] = sh_g[j] + delta;                            // btcart.cpp:287, 291
  }
}

hipError_t launch_lbf(const LbfArgs& a, int lds_budget, LbfLaunch* how, hipStream_t stream) {
  if (how) *how = LbfLaunch{0, kLbfWaves, 0};
  if (a.n <= 0) return hipSuccess;
  if (a.K < 1 || a.D < 1 || a.D > 20 || a.dim < 2) return hipErrorInvalidValue;
  const long long pbytes = (long long)a.os * a.os + (long long)a.hs * a.hs + (long long)a.qs * a.qs;
  const long long wave_bytes = (((long long)a.dim * 8 + 15) & ~15ll) + (((long long)a.K * 4 + 15) & ~15ll) +
                               (a.walk ? ((pbytes + 3 + 15) & ~15ll) : 0);
  const long long budget = std::min<long long>(std::max(0, lds_budget), 160 * 1024);
  const int waves = (int)std::min<long long>(kLbfWaves, budget / wave_bytes);
  if (waves >= 1) {
    const int total = (int)(waves * wave_bytes);
    if (total > 48 * 1024)
      (void)hipFuncSetAttribute((const void*)k_lbf<true>, hipFuncAttributeMaxDynamicSharedMemorySize, total);
    hipLaunchKernelGGL(k_lbf<true>, dim3((unsigned)((a.n + waves - 1) / waves)), dim3(64 * waves), total, stream, a, (int)wave_bytes);
    if (how) *how = LbfLaunch{1, waves, total};
  } else {
    hipLaunchKernelGGL(k_lbf<false>, dim3((unsigned)((a.n + kLbfWaves - 1) / kLbfWaves)), dim3(64 * kLbfWaves), 0, stream, a, 0);
  }
  return hipGetLastError();
}

JDA_BC_READER(k_lbf)

}  // namespace jda
