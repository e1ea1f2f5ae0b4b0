// HIP kernel of dialect CPP's stage close for gfx950 (reference src/jda/btcart.cpp:255-292, 390-424): BoostCart::GenLBF --
// every cart of a stage walked over every sample that is still alive -- and GenDeltaShape with the shape update, as one
// pass over a resident sample set.
//   k_lbf   wave = sample, the form of cpp_wave.h.  The sample's o / h / q bytes, its 2L shape doubles and its row of K leaf
//           indicators live in the wave's own slice of LDS (LDS = true: WaveSlice), or stay in global memory where a slice
//           does not fit (LDS = false; the same arithmetic on the same values).
//           phase 1  lane = cart, k = lane, lane + 64, ...: cart_forward on the stage's level-major node table with the
//                    identity STParameter -> lbf[k] = k * leafNum + leaf
//           phase 2  lane = shape coordinate, j = lane, lane + 64, ... < 2L: gen_delta -- the K rows of w in cart order, the
//                    order of k_mine.hip's regression -- then shape[j] + delta[j]
//           ST = true (train_similarity, include/jda.h): once the shape is readable every lane runs STParameter::Calc(shape,
//           mean_shape) (btcart.cpp:399; stp_calc_uniform: no scratch, the parameter is wave-uniform); phase 1 applies it to the
//           node's offsets, phase 2 to the sum (btcart.cpp:422) before the add.  ST = false is the code it was.
// Whole waves only: no workgroup barrier, a wave synchronises with itself.  No atomics, no log(), fp64 add only.
#include "cpp_wave.h"

namespace jda {

template <bool LDS, bool ST>
__global__ __launch_bounds__(64 * kSampleWaves) void k_lbf(LbfArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lbf_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (i >= a.n) return;                                  // (whole waves; no workgroup barrier below)
  const int K = a.K, dim = a.dim;
  const int leaf_n = 1 << (a.D - 1);
  const int pbytes = a.os * a.os + a.hs * a.hs + a.qs * a.qs;
  const double* sh_g = a.shapes + (size_t)i * dim;
  int* lbf_g = a.lbf + (size_t)i * K;
  const WaveSlice slice(dim, K, pbytes, a.walk != 0);
  unsigned char* mine = lbf_lds + (size_t)wave * slice.bytes;
  double* sh_l = (double*)mine;
  int* lbf_l = (int*)(mine + slice.lbf);
  const double* sh = sh_g;
  const int* lbf = lbf_g;
  if (LDS) { sh = sh_l; lbf = lbf_l; }
  [[maybe_unused]] Stp<double> stp;

  if (a.walk) {
    const uint8_t* pat_g = a.patches + (size_t)i * pbytes;
    const uint8_t* pat_p = pat_g;
    if (LDS) {
      pat_p = wave_stage_bytes(mine + slice.pat, pat_g, pbytes, lane);
      for (int j = lane; j < dim; j += 64) sh_l[j] = sh_g[j];
      wave_lds_sync();
    }
    const PatchSet pat{pat_p, a.os, a.hs, a.qs};
    if (ST) stp = stp_calc_uniform([&](int c) { return sh[c]; }, a.mean, dim >> 1);      // btcart.cpp:399
    // ---- phase 1: lane = cart.  Node `node` of cart k sits level-major in the table (kernels.h: lbf_node_at): level d
    //      starts at K * (2^d - 1), there cart k's 2^d nodes back to back -- the roots of the 64 carts of a round are 64
    //      neighbouring records
    [[maybe_unused]] const long long nodes_n = (long long)K * (leaf_n - 1);
    for (int k = lane; k < K; k += 64) {
      const int leaf = cart_forward(pat, sh, a.D, dim, [&](int d, int node) {
        const long long at = (long long)K * ((1 << d) - 1) + (long long)k * (1 << d) + (node - (1 << d));
        JDA_BC(Bc(0, nodes_n), at, 1, kBcNodeTable);
        return a.nodes[at];
      }, [&](NodeD& nd) { if (ST) stp_apply_offsets(stp, nd); });
      const int idx = k * leaf_n + leaf;                 // btcart.cpp:400-403
      lbf_g[k] = idx;
      if (LDS) lbf_l[k] = idx;
    }
  } else {
    if (LDS) for (int k = lane; k < K; k += 64) lbf_l[k] = lbf_g[k];
    if (ST && a.w) stp = stp_calc_uniform([&](int c) { return sh_g[c]; }, a.mean, dim >> 1);   // (nothing was walked: the shape is not in the slice)
  }
  if (!a.w) return;
  if (LDS) wave_lds_sync(); else if (a.walk) wave_global_sync();

  // ---- phase 2: lane = shape coordinate
  double* out = a.out_shapes + (size_t)i * dim;
  if (ST) {
    for (int j0 = 0; j0 < dim; j0 += 64) {               // (whole rounds: a coordinate's partner is a lane of this round)
      const int j = j0 + lane;
      const double delta = stp_apply_lane(stp, j < dim ? gen_delta(lbf, a.w, dim, K, j, (long long)K * leaf_n) : 0., j);   // btcart.cpp:422
      if (j < dim) out[j] = sh_g[j] + delta;
    }
    return;
  }
  for (int j = lane; j < dim; j += 64)
    out[j] = sh_g[j] + gen_delta(lbf, a.w, dim, K, j, (long long)K * leaf_n);   // btcart.cpp:287, 291
}

hipError_t launch_lbf(const LbfArgs& a, int lds_budget, WaveLaunch* how, hipStream_t stream) {
  *how = WaveLaunch{0, kSampleWaves, 0};
  if (a.n <= 0) return hipSuccess;
  if (a.K < 1 || a.D < 1 || a.D > 20 || a.dim < 2) return hipErrorInvalidValue;
  const long long pbytes = (long long)a.os * a.os + (long long)a.hs * a.hs + (long long)a.qs * a.qs;
  *how = plan_wave_slices(WaveSlice(a.dim, a.K, pbytes, a.walk != 0).bytes, kSampleWaves, lds_budget);
  if (a.mean) return launch_wave_slices(k_lbf<true, true>, k_lbf<false, true>, a, a.n, *how, stream);
  return launch_wave_slices(k_lbf<true, false>, k_lbf<false, false>, a, a.n, *how, stream);
}

JDA_BC_READER(k_lbf)

}  // namespace jda
