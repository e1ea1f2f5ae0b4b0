// HIP kernels of dialect CPP's CART training for gfx950 (reference src/jda/cart.cpp:41-350, Cart::Train / SplitNode /
// SplitNodeWithClassification / SplitNodeWithRegression, and DataSet::CalcFeatureValues, data.cpp:148-173):
//   k_train_transpose  shapes [n][2L] -> [2L][n]
//   k_stp_mean / k_stp DataSet::CalcSTParameters (data.cpp:131-146): the mean shape's side of STParameter::Calc once per call,
//                      then lane = sample over the transposed shapes -> stp_mc (and stp_cm) as five planes [5][n]
//   k_train_values     lane = sample of a node's list, loop over a tile of the pool: Feature::CalcFeatureValue (data.cpp:18-58)
//                      with the identity STParameter (ST = false) or the sample's own stp_mc (ST = true: train_similarity,
//                      include/jda.h) -> 16-bit values [feature][position in the list]
//   k_train_hist       wave = feature: the 511-bin count histogram and the weighted one, every bin's weights added in
//                      list order (cart.cpp:199-208) -- the order decides bits
//   k_train_var        lane = feature: the order statistic from the counts (cart.cpp:314-320), then the eight sums of
//                      the left / right residuals in list order (cart.cpp:321-334)
// No log() here: the entropy sweep and the leaf scores are host work on these kernels' outputs (train.cpp).
#include "cpp_patch.h"
#include "finish_common.h"

namespace jda {

// =============================================================================
// k_train_transpose
// =============================================================================

__global__ __launch_bounds__(256) void k_train_transpose(const double* __restrict__ in, int n, int dim, double* __restrict__ out) {
  const size_t total = (size_t)n * dim;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t j = e / n, i = e - j * n;             // out[j][i], writes coalesced
    out[e] = in[i * dim + j];
  }
}

hipError_t launch_train_transpose(const double* in, int n, int dim, double* out, hipStream_t stream) {
  if (n <= 0 || dim <= 0) return hipSuccess;
  const size_t total = (size_t)n * dim;
  const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_train_transpose, dim3(grid), dim3(256), 0, stream, in, n, dim, out);
  return hipGetLastError();
}

// =============================================================================
// k_train_values: lane = sample, blockIdx.y = tile of kTrainFeatTile pool features
// =============================================================================

constexpr int kTrainFeatTile = 64;

template <bool ST>
__global__ __launch_bounds__(256) void k_train_values(TrainSet set, const int* __restrict__ list, int count,
                                                      const TrainFeat* __restrict__ pool, int F, short* __restrict__ out,
                                                      size_t stride) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const int s = list ? list[j] : j;
  const PatchSet pat{set.patches + (size_t)s * (size_t)(set.os * set.os + set.hs * set.hs + set.qs * set.qs), set.os, set.hs, set.qs};
  const double* sh = set.shapes_t + s;
  const size_t n = (size_t)set.n;
  Stp<double> stp;
  if (ST) {                                             // the sample's own stp_mc, once (k_stp's planes)
    JDA_BC(Bc(0, set.n), s, 1, kBcQueue);
    stp.scale = set.stp[s]; stp.r00 = set.stp[n + s]; stp.r01 = set.stp[2 * n + s]; stp.r10 = set.stp[3 * n + s]; stp.r11 = set.stp[4 * n + s];
  }
  const int f0 = blockIdx.y * kTrainFeatTile, f1 = min(F, f0 + kTrainFeatTile);
  for (int f = f0; f < f1; f++) {
    TrainFeat ft = pool[f];                             // wave-uniform: scalar loads
    if (ST) stp_apply_offsets(stp, ft);                 // data.cpp:41-42
    out[(size_t)f * stride + j] = (short)pat.feature(ft, sh[(size_t)(2 * ft.lm1) * n], sh[(size_t)(2 * ft.lm1 + 1) * n],
                                                     sh[(size_t)(2 * ft.lm2) * n], sh[(size_t)(2 * ft.lm2 + 1) * n]);
  }
}

hipError_t launch_train_values(const TrainSet& set, const int* list, int count, const TrainFeat* pool, int F, short* out,
                               size_t stride, hipStream_t stream) {
  if (count <= 0 || F <= 0) return hipSuccess;
  const dim3 grid((count + 255) / 256, (F + kTrainFeatTile - 1) / kTrainFeatTile);
  if (set.stp) hipLaunchKernelGGL(k_train_values<true>, grid, dim3(256), 0, stream, set, list, count, pool, F, out, stride);
  else hipLaunchKernelGGL(k_train_values<false>, grid, dim3(256), 0, stream, set, list, count, pool, F, out, stride);
  return hipGetLastError();
}

// =============================================================================
// k_stp_mean, k_stp: DataSet::CalcSTParameters
// =============================================================================
// The mean shape's side of STParameter::Calc is the same for every sample: one wave forms it once per call -- every lane the
// same chain, on the device, so that sqrt and the division are the ones the samples' side uses -- and leaves
// ms[0 .. 4) = centre x, centre y, cv::norm, its reciprocal and ms[4 + i] = coordinate i centred and normalised.
__global__ __launch_bounds__(64) void k_stp_mean(const double* __restrict__ mean, int L, double* __restrict__ ms) {
  const int lane = threadIdx.x;
  const StpSide b = stp_side([&](int i) { return mean[i]; }, L);
  if (lane == 0) { ms[0] = b.cx; ms[1] = b.cy; ms[2] = b.scale; ms[3] = b.inv; }
  for (int l = lane; l < L; l += 64) { ms[4 + 2 * l] = stp_unit(mean[2 * l], b.cx, b.inv); ms[5 + 2 * l] = stp_unit(mean[2 * l + 1], b.cy, b.inv); }
}

// lane = sample i over shapes_t [2L][n] (coalesced): stp_mc = Calc(shape, mean_shape) and stp_cm = Calc(mean_shape, shape)
// (data.cpp:134-135) as planes [5][n] -- scale, rot00, rot01, rot10, rot11 -- either may be null.  The centred values are
// recomputed, not stored: no scratch.  stp_cm is a second pair of add chains in the same pass, not derived from stp_mc:
// negating the sine turns a +0. into a -0. where Calc gives +0. (a shape that equals the mean shape; tests/test_train_st_host.py).
__global__ __launch_bounds__(256) void k_stp(const double* __restrict__ shapes_t, int n, int L, const double* __restrict__ ms,
                                             double* __restrict__ stp_mc, double* __restrict__ stp_cm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t N = (size_t)n;
  const auto s = [&](int c) {
    JDA_BC(Bc(0, (long long)2 * L * n), (size_t)c * N + i, 1, kBcLandmark);
    return shapes_t[(size_t)c * N + i];
  };
  const StpSide a = stp_side(s, L);
  Stp<double> mc, cm;
  stp_rot<true>([&](int l, double* x, double* y) { *x = stp_unit(s(2 * l), a.cx, a.inv); *y = stp_unit(s(2 * l + 1), a.cy, a.inv); }, a.scale,
                [&](int l, double* x, double* y) { *x = ms[4 + 2 * l]; *y = ms[5 + 2 * l]; }, ms[2], L, &mc, &cm);
  if (stp_mc) { stp_mc[i] = mc.scale; stp_mc[N + i] = mc.r00; stp_mc[2 * N + i] = mc.r01; stp_mc[3 * N + i] = mc.r10; stp_mc[4 * N + i] = mc.r11; }
  if (stp_cm) { stp_cm[i] = cm.scale; stp_cm[N + i] = cm.r00; stp_cm[2 * N + i] = cm.r01; stp_cm[3 * N + i] = cm.r10; stp_cm[4 * N + i] = cm.r11; }
}

hipError_t launch_stp(const double* shapes_t, int n, int L, const double* mean, double* ms, double* stp_mc, double* stp_cm,
                      hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (L < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_stp_mean, dim3(1), dim3(64), 0, stream, mean, L, ms);
  hipLaunchKernelGGL(k_stp, dim3((n + 255) / 256), dim3(256), 0, stream, shapes_t, n, L, (const double*)ms, stp_mc, stp_cm);
  return hipGetLastError();
}

// =============================================================================
// k_train_hist: wave = feature
// =============================================================================
// A batch of 64 list entries per step, lane = entry.  Bins of different values are independent, so the entries of a
// batch that fall into DIFFERENT bins are added at once; entries of the SAME bin are added one per round in lane order
// (rank = number of lower lanes with the same value), and batches follow each other in list order: every bin receives
// its weights in exactly the order of cart.cpp:199-208.  The bins live in the wave's own LDS rows; the LDS executes one
// wave's instructions in order, and the accesses are volatile so that the compiler keeps them in program order too.

constexpr int kTrainHistWaves = 4;

__global__ __launch_bounds__(64 * kTrainHistWaves) void k_train_hist(const short* __restrict__ values, size_t stride, int F,
                                                                      const int* __restrict__ list, int count,
                                                                      const double* __restrict__ weights,
                                                                      double* __restrict__ out_w, int* __restrict__ out_c) {
  __shared__ double bins_w[kTrainHistWaves][512];
  __shared__ int bins_c[kTrainHistWaves][512];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f = blockIdx.x * kTrainHistWaves + wave;
  if (f >= F) return;                                  // (whole waves; no workgroup barrier below)
  volatile double* bw = bins_w[wave];
  volatile int* bc = bins_c[wave];
  for (int i = lane; i < 512; i += 64) { bw[i] = 0.; bc[i] = 0; }
  const short* row = values + (size_t)f * stride;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int j0 = 0; j0 < count; j0 += 64) {
    const int j = j0 + lane;
    const bool active = j < count;
    const int b = active ? (((int)row[j] + 255) & 511) : 0;
    const double w = (active && weights) ? weights[list ? list[j] : j] : 0.;
    unsigned long long same = __ballot(active);
#pragma unroll
    for (int bit = 0; bit < 9; bit++) {
      const bool one = (b >> bit) & 1;
      const unsigned long long m = __ballot(active && one);
      same &= one ? m : ~m;
    }
    const int rank = __popcll(same & lt);
    bool pending = active;
    for (int r = 0; __ballot(pending) != 0ull; r++) {
      if (pending && rank == r) {
        if (weights) bw[b] = bw[b] + w;
        bc[b] = bc[b] + 1;
        pending = false;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  for (int i = lane; i < kTrainBins; i += 64) {
    if (weights) out_w[(size_t)f * kTrainBins + i] = bw[i];
    out_c[(size_t)f * kTrainBins + i] = bc[i];
  }
}

hipError_t launch_train_hist(const short* values, size_t stride, int F, const int* list, int count, const double* weights,
                             double* out_w, int* out_c, hipStream_t stream) {
  if (F <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_train_hist, dim3((F + kTrainHistWaves - 1) / kTrainHistWaves), dim3(64 * kTrainHistWaves), 0, stream, values,
                     stride, F, list, count, weights, out_w, out_c);
  return hipGetLastError();
}

// =============================================================================
// k_train_var: lane = feature, one wave per 64 features
// =============================================================================
// The value matrix is [feature][position]: a lane walking its own row would touch one cache line per lane and step.
// A 64 x 64 tile is read row by row (lanes along positions, 128 contiguous bytes per row) into LDS and walked from
// there, lane = row.  Rows are padded to 66 entries (33 dwords): lane f reads dword 33 f + jj / 2, distinct banks.

__global__ __launch_bounds__(64) void k_train_var(const short* __restrict__ values, size_t stride, int F,
                                                  const int* __restrict__ list, int count, const double* __restrict__ residual,
                                                  const uint8_t* __restrict__ has_gt, const int* __restrict__ counts,
                                                  const int* __restrict__ kidx, TrainVar* __restrict__ out) {
  __shared__ short tile[64][66];
  const int lane = threadIdx.x;
  const int f0 = blockIdx.x * 64;
  const int f = f0 + lane;
  const bool mine = f < F;
  // sorted_values[k] (cart.cpp:314-320): the smallest value whose cumulative count exceeds k
  int th = 255;
  if (mine) {
    const int k = kidx[f];
    const int* cnt = counts + (size_t)f * kTrainBins;
    int cum = 0;
    for (int b = 0; b < kTrainBins; b++) {
      cum += cnt[b];
      if (cum > k) { th = b - 255; break; }
    }
  }
  double lx = 0., lxx = 0., ly = 0., lyy = 0., rx = 0., rxx = 0., ry = 0., ryy = 0.;
  int nl = 0, nr = 0;
  const int rows = min(64, F - f0);
  for (int j0 = 0; j0 < count; j0 += 64) {
    const int cols = min(64, count - j0);
    __syncthreads();
    for (int r = 0; r < rows; r++)
      if (lane < cols) tile[r][lane] = values[(size_t)(f0 + r) * stride + j0 + lane];
    __syncthreads();
    if (mine) {
      for (int jj = 0; jj < cols; jj++) {
        const int s = list ? list[j0 + jj] : j0 + jj;      // wave-uniform
        if (has_gt && !has_gt[s]) continue;                // cart.cpp:323-325
        const double x = residual[2 * (size_t)s], y = residual[2 * (size_t)s + 1];
        if ((int)tile[lane][jj] <= th) { lx += x; lxx += x * x; ly += y; lyy += y * y; nl++; }
        else { rx += x; rxx += x * x; ry += y; ryy += y * y; nr++; }
      }
    }
  }
  if (mine) {
    TrainVar v;
    v.s[0] = lx; v.s[1] = lxx; v.s[2] = ly; v.s[3] = lyy; v.s[4] = rx; v.s[5] = rxx; v.s[6] = ry; v.s[7] = ryy;
    v.n_left = nl; v.n_right = nr; v.th = th; v.pad = 0;
    out[f] = v;
  }
}

hipError_t launch_train_var(const short* values, size_t stride, int F, const int* list, int count, const double* residual,
                            const uint8_t* has_gt, const int* counts, const int* kidx, TrainVar* out, hipStream_t stream) {
  if (F <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_train_var, dim3((F + 63) / 64), dim3(64), 0, stream, values, stride, F, list, count, residual, has_gt,
                     counts, kidx, out);
  return hipGetLastError();
}

JDA_BC_READER(k_train)

}  // namespace jda
