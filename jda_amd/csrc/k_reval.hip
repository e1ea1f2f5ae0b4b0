// HIP kernel of dialect CPP's Validate on a resident sample set for gfx950 (reference src/jda/cascador.cpp:166-211;
// jdaValidateSamplesCpp, reval.cpp): every record's stored o / h / q patches through the model as it stands, from the
// record's own start shape.
//   k_reval  wave = sample, the form of cpp_wave.h, which k_lbf.hip uses for one stage.  The sample's
//            patch bytes, its 2L shape doubles and a stage's K leaf indicators live in the wave's own slice of LDS (LDS = true:
//            WaveSlice), or in global memory where a slice does not fit (LDS = false: the same arithmetic on the same values;
//            the shape lives in the output array, the indicators in a scratch row).  Per stage:
//            walk     lane = cart, 64 carts at a time: cart_forward on the mining tables' cart-major heap with the
//                     identity STParameter; the lane keeps its cart's leaf score, mean, std and threshold
//            replay   the score chain of those 64 carts IN CART ORDER, the non-associative chain of Validate:
//                     score += leaf; score = (score - mean) / std -- one fp64 add, one subtract and one IEEE division per
//                     cart, the operands handed from the cart's lane to the whole wave by v_readlane; lane l keeps the
//                     score as it stood after cart l
//            reject   `score < th` per lane, one ballot: the first set bit is the first failing cart -- it fixes carts_n,
//                     the score where the walk stopped and the shape as it stood.  A NaN score fails no comparison.
//            regress  a sample that passed the stage: lane = shape coordinate, gen_delta -- w[lbf[k]][j] for k = 0 .. K-1
//                     in cart order (btcart.cpp:407-424) -- then shape += delta
//            The partial stage of a snapshot runs its `part` carts and no regression (cascador.cpp:198-209).
//            ST = true (train_similarity, include/jda.h): at the start of every full stage every lane runs STParameter::Calc(shape
//            as it stands, mean_shape) (cascador.cpp:180; stp_calc_uniform: no scratch, wave-uniform); the walk applies it to the
//            node's offsets, the regression to the sum before the add (btcart.cpp:422).  The partial stage walks with the stage
//            before's parameter, the first stage with STParameter's default -- as k_mine_walk.  ST = false is the code it was.
// Whole waves only: no workgroup barrier, no atomics, no spinning, nothing between waves.  The model's tables are the
// mining tables, patched in place between launches (model_grow.cpp): every read of them has a lane-dependent address --
// lane = cart in the walk, lane = coordinate in the regression -- so they are vector loads; nothing of them is read
// through the scalar cache.
#include <limits>

#include "cpp_wave.h"

namespace jda {

namespace {

// n bytes global -> LDS by one wave, wave_stage_bytes' contract (cpp_wave.h) as a plain loop: k_reval keeps its own copy,
// because with the batched one reval_bench's complete model measured slower than before (profiles/cpp_wave_ab.json).
__device__ __forceinline__ uint8_t* reval_stage_bytes(uint8_t* lds, const uint8_t* __restrict__ src, int n, int lane) {
  const int sh = (int)((uintptr_t)src & 3);
  uint8_t* dst = lds + sh;
  const int head = min(n, (4 - sh) & 3);
  const int body = (n - head) >> 2, tail = n - head - 4 * body;
  if (lane < head) dst[lane] = src[lane];
  const uint32_t* s4 = (const uint32_t*)(src + head);
  uint32_t* d4 = (uint32_t*)(dst + head);
  for (int d = lane; d < body; d += 64) d4[d] = s4[d];
  if (lane < tail) dst[head + 4 * body + lane] = src[head + 4 * body + lane];
  return dst;
}

}  // namespace

template <bool LDS, bool ST>
__global__ __launch_bounds__(64 * kSampleWaves) void k_reval(RevalArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char reval_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
  if (i >= a.n) return;                                  // (whole waves; no workgroup barrier below)
  JDA_BC(Bc(0, a.n), i, 1, kBcQueue);
  const MineModel& m = a.m;
  const int K = m.K, dim = m.dim, leaf_n = m.leaf_n, node_n = m.node_n;
  const int pbytes = a.os * a.os + a.hs * a.hs + a.qs * a.qs;
  const uint8_t* pat_g = a.patches + (size_t)i * pbytes;
  const double* start = a.start + (size_t)i * dim;
  double* sh_g = a.shape + (size_t)i * dim;
  int* lbf_g = a.lbf + (size_t)i * K;
  const WaveSlice slice(dim, K, pbytes, true);
  unsigned char* mine_l = reval_lds + (size_t)wave * slice.bytes;
  double* sh_l = (double*)mine_l;
  int* lbf_l = (int*)(mine_l + slice.lbf);
  double* sh = sh_g;
  int* lbf = lbf_g;
  const uint8_t* pat_p = pat_g;
  if (LDS) {
    sh = sh_l; lbf = lbf_l;
    pat_p = reval_stage_bytes(mine_l + slice.pat, pat_g, pbytes, lane);
  }
  for (int j = lane; j < dim; j += 64) sh[j] = start[j];
  if (LDS) wave_lds_sync(); else wave_global_sync();
  const PatchSet pat{pat_p, a.os, a.hs, a.qs};

  double score = 0.;                                     // wave-uniform: every lane runs the same chain
  int nn = 0;
  bool is_face = true;
  const int stages = m.full + (m.part > 0 ? 1 : 0);
  [[maybe_unused]] Stp<double> stp;
  [[maybe_unused]] bool apply = false;                   // (false: STParameter's default, the offsets as stored)
  [[maybe_unused]] const long long nodes_all = (long long)m.T * K * node_n, leaves_all = (long long)m.T * K * leaf_n;
  for (int t = 0; t < stages && is_face; t++) {
    const bool partial = t == m.full;                    // the stage in training: `part` carts, no regression
    const int Kt = partial ? m.part : K;
    if (ST && !partial) { stp = stp_calc_uniform([&](int c) { return sh[c]; }, m.mean, dim >> 1); apply = true; }   // cascador.cpp:180
    for (int k0 = 0; k0 < Kt && is_face; k0 += 64) {
      const int k = k0 + lane;
      const bool active = k < Kt;
      double lf = 0., mu = 0., sd = 1., th = -std::numeric_limits<double>::infinity();
      if (active) {
        const size_t ck = (size_t)t * K + k;
        const int leaf = cart_forward(pat, sh, m.D, dim, [&](int, int node) {   // (heap node `node`, 1-based, is record node - 1)
          JDA_BC(Bc(0, nodes_all), (long long)(ck * node_n + node - 1), 1, kBcNodeTable);
          return m.nodes[ck * node_n + node - 1];
        }, [&](NodeD& nd) { if (ST && apply) stp_apply_offsets(stp, nd); });
        JDA_BC(Bc(0, leaves_all), (long long)(ck * leaf_n + leaf), 1, kBcNodeTable);
        lbf[k] = k * leaf_n + leaf;                      // cascador.cpp:192
        lf = m.leaf[ck * leaf_n + leaf]; mu = m.cmean[ck]; sd = m.cstd[ck]; th = m.cth[ck];
      }
      const int cnt = min(64, Kt - k0);
      double mine = 0.;
      for (int l = 0; l < cnt; l++) {                    // cascador.cpp:185-186, in cart order
        score = score + rl(lf, l);
        score = (score - rl(mu, l)) / rl(sd, l);
        if (lane == l) mine = score;
      }
      const unsigned long long failed = __ballot(active && mine < th);      // cascador.cpp:188
      if (failed) {
        const int first = __ffsll((long long)failed) - 1;
        score = rl(mine, first);
        nn += first + 1;
        is_face = false;
      } else {
        nn += cnt;
      }
    }
    if (!is_face || partial) break;
    if (LDS) wave_lds_sync(); else wave_global_sync();  // the stage's indicators, written by their carts' lanes
    // ---- GenDeltaShape (btcart.cpp:407-424) and shape += delta (cascador.cpp:196): lane = coordinate, rows in cart order
    const double* wt = m.w + (size_t)t * K * leaf_n * dim;
    if (ST) {
      for (int j0 = 0; j0 < dim; j0 += 64) {             // (whole rounds: a coordinate's partner is a lane of this round)
        const int j = j0 + lane;
        const double delta = stp_apply_lane(stp, j < dim ? gen_delta(lbf, wt, dim, K, j, (long long)K * leaf_n) : 0., j);
        if (j < dim) sh[j] = sh[j] + delta;
      }
    } else {
      for (int j = lane; j < dim; j += 64)               // (coordinate j is read and written by this lane alone)
        sh[j] = sh[j] + gen_delta(lbf, wt, dim, K, j, (long long)K * leaf_n);
    }
    if (LDS) wave_lds_sync(); else wave_global_sync();  // the next stage's walk reads every coordinate
  }
  if (LDS) for (int j = lane; j < dim; j += 64) sh_g[j] = sh_l[j];
  if (lane == 0) { a.face[i] = is_face ? 1 : 0; a.carts_n[i] = nn; a.score[i] = score; }
}

hipError_t launch_reval(const RevalArgs& a, int lds_budget, WaveLaunch* how, hipStream_t stream) {
  *how = WaveLaunch{0, kSampleWaves, 0};
  if (a.n <= 0) return hipSuccess;
  if (a.m.K < 1 || a.m.D < 1 || a.m.D > 20 || a.m.dim < 2) return hipErrorInvalidValue;
  const long long pbytes = (long long)a.os * a.os + (long long)a.hs * a.hs + (long long)a.qs * a.qs;
  *how = plan_wave_slices(WaveSlice(a.m.dim, a.m.K, pbytes, true).bytes, kSampleWaves, lds_budget);
  if (a.st) return launch_wave_slices(k_reval<true, true>, k_reval<false, true>, a, a.n, *how, stream);
  return launch_wave_slices(k_reval<true, false>, k_reval<false, false>, a, a.n, *how, stream);
}

JDA_BC_READER(k_reval)

}  // namespace jda
