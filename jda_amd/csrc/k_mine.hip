// HIP kernels of dialect CPP's Validate on caller crops and of the hard-negative mining walk for gfx950 (reference
// src/jda/data.cpp:885-1065, NegGenerator::NextImage / ParallelMining, and JoinCascador::Validate, cascador.cpp:166-211):
//   k_mine_scan     lane = window of the enumeration: the first carts of stage 0 with every pixel computed on demand from
//                   the background image (chain 0: crop -> o, o -> h, o -> q, each a cv::resize(INTER_LINEAR) pixel)
//   k_mine_items    survivor ordinals -> crops
//   k_mine_patches  workgroup = crop: its o / h / q patches, built once (what MoreNegSamples stores, data.cpp:510-520)
//   k_mine_walk     lane = crop: Validate, literally, on the patches (fp64, snapshot loop bounds, similarity transform,
//                   initial shape shift)
//   k_mine_sum      reject lengths of a range of windows (NegGenerator's carts_n / nega_n, data.cpp:1001-1004)
#include "cpp_wave.h"
#include "finish_common.h"
#include "splitmix.h"

namespace jda {

namespace {

// Pixels of a crop of a transformed background image (data.cpp:930-963 by coordinate remapping: transpose first, then
// mirror the stored image's x / y).
struct Crop {
  const uint8_t* img; int W, H, tf, cx, cy;
  Bc bc;
  __device__ __forceinline__ int operator()(int x, int y) const {
    int u = cx + x, v = cy + y;
    if (tf & kMineSwap) { const int t = u; u = v; v = t; }
    if (tf & kMineFlipX) u = W - 1 - u;
    if (tf & kMineFlipY) v = H - 1 - v;
    JDA_BC_ADDR(bc, img + (size_t)v * W + u, 1, kBcScanPixGlb);
    return img[(size_t)v * W + u];
  }
};

__device__ __forceinline__ Crop make_crop(const uint8_t* base, const MineImg& im, int x, int y) {
  Crop c;
  c.img = base + im.off; c.W = im.w; c.H = im.h; c.tf = im.tf; c.cx = x; c.cy = y;
  c.bc = Bc((long long)(uintptr_t)c.img, (long long)(uintptr_t)c.img + (long long)im.w * im.h);   // (empty in the product build)
  return c;
}

// The initial shape's global shift (RandomShape, data.cpp:225-236) of the crop with key `key`: draws 2 key (x) and
// 2 key + 1 (y) of the counter-based generator (include/jda.h, splitmix.h), mapped like cv::RNG::uniform(a, b): a + (b - a) * u.
__device__ __forceinline__ void mine_shift(const MineSizes& z, unsigned long long key, double* dx, double* dy) {
  if (z.shift == 0.) { *dx = 0.; *dy = 0.; return; }
  const double a = -z.shift, b = z.shift;
  *dx = a + (b - a) * splitmix_unit(splitmix_draw(z.seed, 2ull * key));
  *dy = a + (b - a) * splitmix_unit(splitmix_draw(z.seed, 2ull * key + 1ull));
}

// segment of ordinal o: the last one whose first <= o
__device__ __forceinline__ int find_seg(const MineSeg* segs, int n, unsigned long long o) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].first <= o) lo = mid; else hi = mid - 1;
  }
  return lo;
}

}  // namespace

// =============================================================================
// k_mine_scan: lane = window, stage 0's first carts straight from the background image
// =============================================================================

__global__ __launch_bounds__(256) void k_mine_scan(MineModel m, MineSizes z, const uint8_t* __restrict__ base,
                                                   const MineImg* __restrict__ imgs, const MineSeg* __restrict__ segs,
                                                   int n_segs, unsigned long long lo, unsigned long long hi, int carts0,
                                                   int* __restrict__ status, unsigned long long* __restrict__ surv,
                                                   unsigned* __restrict__ n_surv) {
  const unsigned long long o = lo + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= hi) return;
  const MineSeg sg = segs[find_seg(segs, n_segs, o)];
  const int wi = (int)(o - sg.first);
  const int wy = wi / sg.nx, wx = wi - wy * sg.nx;
  const Crop crop = make_crop(base, imgs[sg.image], wx * sg.step, wy * sg.step);
  const CvResize ro = cv_resize_make(sg.win, sg.win, z.os, z.os);
  const CvResize rh = cv_resize_make(z.os, z.os, z.hs, z.hs), rq = cv_resize_make(z.os, z.os, z.qs, z.qs);
  const Resized<Crop> opx{crop, ro};
  double dx, dy;
  mine_shift(z, o, &dx, &dy);
  double score = 0.;
  int k = 0;
  for (; k < carts0; k++) {
    const NodeD* cart = m.nodes + (size_t)k * m.node_n;
    int node = 0;
    for (int d = 0; d < m.D - 1; d++) {
      const NodeD nd = cart[node];
      // stage 0: every landmark of the shape is mean + (dx, dy)
      const FeatXY c = feature_xy(nd.scale == 0 ? z.os : (nd.scale == 1 ? z.hs : z.qs), m.mean[nd.lm1x2] + dx, m.mean[nd.lm1x2 + 1] + dy,
                                  nd.o1x, nd.o1y, m.mean[nd.lm2x2] + dx, m.mean[nd.lm2x2 + 1] + dy, nd.o2x, nd.o2y);
      // ... and an h / q pixel is a resize of o pixels, themselves made on demand
      const int v = nd.scale == 0 ? feature_diff(opx, c) : feature_diff(Resized<Resized<Crop>>{opx, nd.scale == 1 ? rh : rq}, c);
      node = (v <= nd.th) ? 2 * node + 1 : 2 * node + 2;
    }
    const int idx = node - m.node_n;
    score += m.leaf[(size_t)k * m.leaf_n + idx];
    score = (score - m.cmean[k]) / m.cstd[k];
    if (score < m.cth[k]) break;
  }
  if (k < carts0) {
    status[o - lo] = k + 1;
  } else {
    status[o - lo] = 0;
    surv[atomicAdd(n_surv, 1u)] = o;
  }
}

hipError_t launch_mine_scan(const MineModel& m, const MineSizes& z, const uint8_t* base, const MineImg* imgs,
                            const MineSeg* segs, int n_segs, unsigned long long lo, unsigned long long hi, int carts0,
                            int* status, unsigned long long* surv, unsigned* n_surv, hipStream_t stream, MineLaunch* how) {
  if (how) *how = MineLaunch{false, kMineKScan, 0u, false};
  if (hi <= lo) return hipSuccess;
  const unsigned long long n = hi - lo;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_mine_scan, dim3(grid), dim3(256), 0, stream, m, z, base, imgs, segs, n_segs, lo,
                     hi, carts0, status, surv, n_surv);
  if (how) { how->launched = true; how->grid = grid; }
  return hipGetLastError();
}

// =============================================================================
// k_mine_items: ordinals -> crops
// =============================================================================

__global__ __launch_bounds__(256) void k_mine_items(const MineSeg* __restrict__ segs, int n_segs,
                                                    const unsigned long long* __restrict__ ords, int n,
                                                    MineItem* __restrict__ items) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long o = ords[i];
  const MineSeg sg = segs[find_seg(segs, n_segs, o)];
  const int wi = (int)(o - sg.first);
  const int wy = wi / sg.nx, wx = wi - wy * sg.nx;
  MineItem it;
  it.image = sg.image; it.x = wx * sg.step; it.y = wy * sg.step; it.w = sg.win; it.h = sg.win; it.pad = 0; it.key = o;
  items[i] = it;
}

hipError_t launch_mine_items(const MineSeg* segs, int n_segs, const unsigned long long* ords, int n, MineItem* items,
                             hipStream_t stream, MineLaunch* how) {
  if (how) *how = MineLaunch{false, kMineKItems, 0u, false};
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_mine_items, dim3(grid), dim3(256), 0, stream, segs, n_segs, ords, n, items);
  if (how) { how->launched = true; how->grid = grid; }
  return hipGetLastError();
}

// =============================================================================
// k_mine_patches: workgroup = crop, its o / h / q patches
// =============================================================================

constexpr int kMinePatchMax = 128;      // largest patch side (the o patch is staged in LDS)

__global__ __launch_bounds__(256) void k_mine_patches(MineSizes z, const uint8_t* __restrict__ base,
                                                      const MineImg* __restrict__ imgs, const MineItem* __restrict__ items,
                                                      uint8_t* __restrict__ patches, int pbytes) {
  __shared__ uint8_t o_lds[kMinePatchMax * kMinePatchMax];
  const MineItem it = items[blockIdx.x];
  const Crop crop = make_crop(base, imgs[it.image], it.x, it.y);
  uint8_t* out = patches + (size_t)blockIdx.x * pbytes;
  const CvResize ro = cv_resize_make(it.w, it.h, z.os, z.os);
  for (int e = threadIdx.x; e < z.os * z.os; e += blockDim.x) {
    const int y = e / z.os, x = e - y * z.os;
    const uint8_t v = (uint8_t)cv_resize_px(crop, ro, x, y);
    o_lds[e] = v;
    out[e] = v;
  }
  __syncthreads();
  auto lds_px = [&](int x, int y) {
    JDA_BC(Bc(0, (long long)z.os * z.os), y * z.os + x, 1, kBcFinishTile);
    return (int)o_lds[y * z.os + x];
  };
  for (int s = 1; s <= 2; s++) {
    const int ds = s == 1 ? z.hs : z.qs;
    uint8_t* dst = out + z.os * z.os + (s == 2 ? z.hs * z.hs : 0);
    // chain 0 (mining, data.cpp:987-990): from the o patch; chain 1 (detectSingleScale, cascador.cpp:243-245): from the crop
    const CvResize r = z.mode == 0 ? cv_resize_make(z.os, z.os, ds, ds) : cv_resize_make(it.w, it.h, ds, ds);
    for (int e = threadIdx.x; e < ds * ds; e += blockDim.x) {
      const int y = e / ds, x = e - y * ds;
      dst[e] = (uint8_t)(z.mode == 0 ? cv_resize_px(lds_px, r, x, y) : cv_resize_px(crop, r, x, y));
    }
  }
}

hipError_t launch_mine_patches(const MineSizes& z, const uint8_t* base, const MineImg* imgs, const MineItem* items, int n,
                               uint8_t* patches, int pbytes, hipStream_t stream, MineLaunch* how) {
  if (how) *how = MineLaunch{false, kMineKPatches, 0u, false};
  if (n <= 0) return hipSuccess;
  if (z.os > kMinePatchMax || z.hs > kMinePatchMax || z.qs > kMinePatchMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mine_patches, dim3(n), dim3(256), 0, stream, z, base, imgs, items, patches, pbytes);
  if (how) { how->launched = true; how->grid = (unsigned)n; }
  return hipGetLastError();
}

// =============================================================================
// k_mine_walk: lane = crop, JoinCascador::Validate on its patches
// =============================================================================

__global__ __launch_bounds__(64) void k_mine_walk(MineModel m, MineSizes z, const MineItem* __restrict__ items, int n,
                                                  const uint8_t* __restrict__ patches, int pbytes, int similarity,
                                                  uint8_t* __restrict__ face, int* __restrict__ carts_n,
                                                  double* __restrict__ score_out, double* __restrict__ shape_out,
                                                  int* __restrict__ lbf_ws, double* __restrict__ t1_ws, double* __restrict__ t2_ws,
                                                  const double* __restrict__ init) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int dim = m.dim, K = m.K;
  const PatchSet pat{patches + (size_t)i * pbytes, z.os, z.hs, z.qs};
  double* sh = shape_out + (size_t)i * dim;
  int* lbf = lbf_ws + (size_t)i * K;
  double* t1 = t1_ws + (size_t)i * dim;
  double* t2 = t2_ws + (size_t)i * dim;
  if (init) {                                           // a resident sample's own start shape (jdaValidateSamplesCpp, form 1)
    for (int j = 0; j < dim; j++) sh[j] = init[(size_t)i * dim + j];
  } else {
    double dx, dy;
    mine_shift(z, items[i].key, &dx, &dy);
    for (int j = 0; j < dim; j++) sh[j] = m.mean[j] + ((j & 1) ? dy : dx);    // RandomShape, data.cpp:231-234
  }
  Stp<double> stp; stp.scale = 1.; stp.r00 = 1.; stp.r01 = 0.; stp.r10 = 0.; stp.r11 = 1.;
  bool apply = false;
  double score = 0.;
  int nn = 0;
  // one cart: cart_forward (cpp_wave.h) on the cart-major heap -> leaf index; false = rejected
  auto cart = [&](int t, int k, int* leaf) -> bool {
    const size_t ck = (size_t)t * K + k;
    const NodeD* nodes = m.nodes + ck * m.node_n;
    *leaf = cart_forward(pat, sh, m.D, dim, [&](int, int node) { return nodes[node - 1]; }, [&](NodeD& nd) {
      if (!apply) return;                               // stp_mc.Apply on both offsets, data.cpp:33-34
      double ax, ay, bx, by;
      stp_apply<double>(stp, nd.o1x, nd.o1y, &ax, &ay);
      stp_apply<double>(stp, nd.o2x, nd.o2y, &bx, &by);
      nd.o1x = ax; nd.o1y = ay; nd.o2x = bx; nd.o2y = by;
    });
    score += m.leaf[ck * m.leaf_n + *leaf];
    score = (score - m.cmean[ck]) / m.cstd[ck];
    nn++;
    return !(score < m.cth[ck]);
  };
  bool is_face = true;
  for (int t = 0; t < m.full && is_face; t++) {
    if (similarity) { stp = stp_calc(sh, m.mean, m.L, t1, t2); apply = true; }    // cascador.cpp:180
    for (int k = 0; k < K; k++) {
      int leaf;
      if (!cart(t, k, &leaf)) { is_face = false; break; }
      lbf[k] = k * m.leaf_n + leaf;
    }
    if (!is_face) break;
    // GenDeltaShape (btcart.cpp:407-424): rows summed from zero in cart order, Apply, then shape += delta
    const double* wt = m.w + (size_t)t * K * m.leaf_n * dim;
    for (int j = 0; j < dim; j += 2) {
      double ex = 0., ey = 0.;
      for (int k = 0; k < K; k++) {
        JDA_BC(Bc(0, (long long)K * m.leaf_n), lbf[k], 1, kBcWRow);
        const double* row = wt + (size_t)lbf[k] * dim;
        ex += row[j]; ey += row[j + 1];
      }
      if (similarity) { double ax, ay; stp_apply<double>(stp, ex, ey, &ax, &ay); ex = ax; ey = ay; }
      t1[j] = ex; t1[j + 1] = ey;
    }
    for (int j = 0; j < dim; j++) sh[j] = sh[j] + t1[j];
  }
  // a trainer snapshot: carts [0, part) of the stage in training, no regression, the last stage's parameter (cascador.cpp:198-209)
  for (int k = 0; k < m.part && is_face; k++) {
    int leaf;
    if (!cart(m.full, k, &leaf)) is_face = false;
  }
  if (face) face[i] = is_face ? 1 : 0;
  if (carts_n) carts_n[i] = nn;
  if (score_out) score_out[i] = score;
}

hipError_t launch_mine_walk(const MineModel& m, const MineSizes& z, const MineItem* items, int n, const uint8_t* patches,
                            int pbytes, int similarity, uint8_t* face, int* carts_n, double* score, double* shape, int* lbf,
                            double* t1, double* t2, hipStream_t stream, const double* init, MineLaunch* how) {
  if (how) *how = MineLaunch{false, kMineKWalk, 0u, false};
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((n + 63) / 64);
  hipLaunchKernelGGL(k_mine_walk, dim3(grid), dim3(64), 0, stream, m, z, items, n, patches, pbytes, similarity, face,
                     carts_n, score, shape, lbf, t1, t2, init);
  if (how) { how->launched = true; how->grid = grid; }
  return hipGetLastError();
}

// =============================================================================
// k_mine_sum: reject lengths of a range of windows
// =============================================================================

__global__ __launch_bounds__(256) void k_mine_sum(const int* __restrict__ status, unsigned long long n,
                                                  unsigned long long* __restrict__ out) {
  unsigned long long cnt = 0, sum = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (unsigned long long)gridDim.x * blockDim.x) {
    const int s = status[i];
    if (s > 0) { cnt++; sum += (unsigned long long)s; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off, 64);
    sum += __shfl_down(sum, off, 64);
  }
  if ((threadIdx.x & 63) == 0 && (cnt | sum)) { atomicAdd(&out[0], cnt); atomicAdd(&out[1], sum); }
}

hipError_t launch_mine_sum(const int* status, unsigned long long n, unsigned long long* out, hipStream_t stream,
                           MineLaunch* how) {
  if (how) *how = MineLaunch{false, kMineKSum, 0u, false};
  if (n == 0) return hipSuccess;
  const unsigned grid = (unsigned)std::min<unsigned long long>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(k_mine_sum, dim3(grid), dim3(256), 0, stream, status, n, out);
  // saturated: fewer lanes than windows, so the kernel's stride loop turns again for some lane
  if (how) { how->launched = true; how->grid = grid; how->saturated = n > (unsigned long long)grid * 256; }
  return hipGetLastError();
}

JDA_BC_READER(k_mine)

}  // namespace jda
