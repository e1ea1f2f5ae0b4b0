// HIP kernels of dialect CPP's Validate on caller crops and of the hard-negative mining walk for gfx950 (reference
// src/jda/data.cpp:885-1065, NegGenerator::NextImage / ParallelMining, and JoinCascador::Validate, cascador.cpp:166-211):
//   k_mine_scan     lane = window of the enumeration: the first carts of stage 0 with every pixel computed on demand from
//                   the background image (chain 0: crop -> o, o -> h, o -> q, each a cv::resize(INTER_LINEAR) pixel)
//   k_mine_items    survivor ordinals -> crops
//   k_mine_patches  workgroup = crop: its o / h / q patches, built once (what MoreNegSamples stores, data.cpp:510-520)
//   k_mine_walk     lane = crop: Validate, literally, on the patches (fp64, snapshot loop bounds, similarity transform,
//                   initial shape shift)
//   k_mine_sum      reject lengths of a range of windows (NegGenerator's carts_n / nega_n, data.cpp:1001-1004)
#include "finish_common.h"

namespace jda {

namespace {

// One output pixel of cv::resize(INTER_LINEAR, 8UC1) of an sw x sh source whose pixels `f(x, y)` returns: the same
// operations as resize_cv_pixel (k_misc.hip), with the source behind a function so that it can itself be a resize.
struct Rs { double sx, sy; int sw, sh, area, ident; };

__device__ __forceinline__ Rs rs_make(int sw, int sh, int dw, int dh) {     // launch_resize_cv's parameters
  Rs r;
  r.sw = sw; r.sh = sh;
  const double inv_sx = (double)dw / sw, inv_sy = (double)dh / sh;
  r.sx = 1. / inv_sx; r.sy = 1. / inv_sy;
  r.area = (fabs(r.sx - 2.) < 2.220446049250313e-16 && fabs(r.sy - 2.) < 2.220446049250313e-16) ? 1 : 0;
  r.ident = (sw == dw && sh == dh) ? 1 : 0;     // (the bilinear formula then returns the source pixel itself)
  return r;
}

template <typename F>
__device__ __forceinline__ int cv_px(const F& f, const Rs& r, int dx, int dy) {
  if (r.ident) return f(dx, dy);
  if (r.area) return (f(2 * dx, 2 * dy) + f(2 * dx + 1, 2 * dy) + f(2 * dx, 2 * dy + 1) + f(2 * dx + 1, 2 * dy + 1) + 2) >> 2;
  float fx = (float)(((double)dx + 0.5) * r.sx - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { fx = 0.f; sx = 0; }
  const bool edge = sx + 1 >= r.sw;
  if (sx >= r.sw - 1) { fx = 0.f; sx = r.sw - 1; }
  float fy = (float)(((double)dy + 0.5) * r.sy - 0.5);
  const int sy = (int)floorf(fy);
  fy -= (float)sy;
  auto sat_short = [](float v) { int i = __float2int_rn(v); return i < -32768 ? -32768 : (i > 32767 ? 32767 : i); };
  const int a0 = sat_short((1.f - fx) * 2048.f), a1 = sat_short(fx * 2048.f);
  const int b0 = sat_short((1.f - fy) * 2048.f), b1 = sat_short(fy * 2048.f);
  const int y0 = min(max(sy, 0), r.sh - 1), y1 = min(max(sy + 1, 0), r.sh - 1);
  int r0, r1;
  if (!edge) { r0 = f(sx, y0) * a0 + f(sx + 1, y0) * a1; r1 = f(sx, y1) * a0 + f(sx + 1, y1) * a1; }
  else { r0 = f(sx, y0) * 2048; r1 = f(sx, y1) * 2048; }
  return ((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2) & 0xff;
}

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

// The initial shape's global shift (RandomShape, data.cpp:225-236) of the crop with key `key`: draw c of the
// counter-based generator (include/jda.h: SplitMix64 of seed + (c + 1) * golden gamma, top 53 bits), c = 2 key for x
// and 2 key + 1 for y, mapped like cv::RNG::uniform(a, b): a + (b - a) * u.
__device__ __forceinline__ double mine_draw(unsigned long long seed, unsigned long long c, double a, double b) {
  unsigned long long z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const double u = (double)(z >> 11) * 0x1.0p-53;
  return a + (b - a) * u;
}

__device__ __forceinline__ void mine_shift(const MineSizes& z, unsigned long long key, double* dx, double* dy) {
  if (z.shift == 0.) { *dx = 0.; *dy = 0.; return; }
  *dx = mine_draw(z.seed, 2ull * key, -z.shift, z.shift);
  *dy = mine_draw(z.seed, 2ull * key + 1ull, -z.shift, z.shift);
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

__device__ __forceinline__ int coord_cpp(double s, double o, int pw) {   // data.cpp:40-51, common.hpp:227-232
  return clamp_win(DialectCPP::coord(s, o, pw), pw);
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
  const Rs ro = rs_make(sg.win, sg.win, z.os, z.os);
  const Rs rh = rs_make(z.os, z.os, z.hs, z.hs), rq = rs_make(z.os, z.os, z.qs, z.qs);
  auto opx = [&](int x, int y) { return cv_px(crop, ro, x, y); };
  double dx, dy;
  mine_shift(z, o, &dx, &dy);
  double score = 0.;
  int k = 0;
  for (; k < carts0; k++) {
    const NodeD* cart = m.nodes + (size_t)k * m.node_n;
    int node = 0;
    for (int d = 0; d < m.D - 1; d++) {
      const NodeD nd = cart[node];
      const int pw = nd.scale == 0 ? z.os : (nd.scale == 1 ? z.hs : z.qs);
      // stage 0: every landmark of the shape is mean + (dx, dy)
      const int x1 = coord_cpp(m.mean[nd.lm1x2] + dx, nd.o1x, pw), y1 = coord_cpp(m.mean[nd.lm1x2 + 1] + dy, nd.o1y, pw);
      const int x2 = coord_cpp(m.mean[nd.lm2x2] + dx, nd.o2x, pw), y2 = coord_cpp(m.mean[nd.lm2x2 + 1] + dy, nd.o2y, pw);
      int a, b;
      if (nd.scale == 0) { a = opx(x1, y1); b = opx(x2, y2); }
      else {
        const Rs& r = nd.scale == 1 ? rh : rq;
        a = cv_px(opx, r, x1, y1); b = cv_px(opx, r, x2, y2);
      }
      node = (a - b <= nd.th) ? 2 * node + 1 : 2 * node + 2;
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
                            int* status, unsigned long long* surv, unsigned* n_surv, hipStream_t stream) {
  if (hi <= lo) return hipSuccess;
  const unsigned long long n = hi - lo;
  hipLaunchKernelGGL(k_mine_scan, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m, z, base, imgs, segs, n_segs, lo,
                     hi, carts0, status, surv, n_surv);
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
                             hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_mine_items, dim3((n + 255) / 256), dim3(256), 0, stream, segs, n_segs, ords, n, items);
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
  const Rs ro = rs_make(it.w, it.h, z.os, z.os);
  for (int e = threadIdx.x; e < z.os * z.os; e += blockDim.x) {
    const int y = e / z.os, x = e - y * z.os;
    const uint8_t v = (uint8_t)cv_px(crop, ro, x, y);
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
    const Rs r = z.mode == 0 ? rs_make(z.os, z.os, ds, ds) : rs_make(it.w, it.h, ds, ds);
    for (int e = threadIdx.x; e < ds * ds; e += blockDim.x) {
      const int y = e / ds, x = e - y * ds;
      dst[e] = (uint8_t)(z.mode == 0 ? cv_px(lds_px, r, x, y) : cv_px(crop, r, x, y));
    }
  }
}

hipError_t launch_mine_patches(const MineSizes& z, const uint8_t* base, const MineImg* imgs, const MineItem* items, int n,
                               uint8_t* patches, int pbytes, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (z.os > kMinePatchMax || z.hs > kMinePatchMax || z.qs > kMinePatchMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mine_patches, dim3(n), dim3(256), 0, stream, z, base, imgs, items, patches, pbytes);
  return hipGetLastError();
}

// =============================================================================
// k_mine_walk: lane = crop, JoinCascador::Validate on its patches
// =============================================================================

__global__ __launch_bounds__(64) void k_mine_walk(MineModel m, MineSizes z, const MineItem* __restrict__ items, int n,
                                                  const uint8_t* __restrict__ patches, int pbytes, int similarity,
                                                  uint8_t* __restrict__ face, int* __restrict__ carts_n,
                                                  double* __restrict__ score_out, double* __restrict__ shape_out,
                                                  int* __restrict__ lbf_ws, double* __restrict__ t1_ws, double* __restrict__ t2_ws) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int dim = m.dim, K = m.K;
  const uint8_t* pat = patches + (size_t)i * pbytes;
  const uint8_t* pimg[3] = {pat, pat + z.os * z.os, pat + z.os * z.os + z.hs * z.hs};
  const int pside[3] = {z.os, z.hs, z.qs};
  double* sh = shape_out + (size_t)i * dim;
  int* lbf = lbf_ws + (size_t)i * K;
  double* t1 = t1_ws + (size_t)i * dim;
  double* t2 = t2_ws + (size_t)i * dim;
  double dx, dy;
  mine_shift(z, items[i].key, &dx, &dy);
  for (int j = 0; j < dim; j++) sh[j] = m.mean[j] + ((j & 1) ? dy : dx);      // RandomShape, data.cpp:231-234
  Stp<double> stp; stp.scale = 1.; stp.r00 = 1.; stp.r01 = 0.; stp.r10 = 0.; stp.r11 = 1.;
  bool apply = false;
  double score = 0.;
  int nn = 0;
  // one cart: Cart::Forward (cart.cpp:392-404) -> leaf index; false = rejected
  auto cart = [&](int t, int k, int* leaf) -> bool {
    const size_t ck = (size_t)t * K + k;
    const NodeD* nodes = m.nodes + ck * m.node_n;
    int node = 0;
    for (int d = 0; d < m.D - 1; d++) {
      NodeD nd = nodes[node];
      if (apply) {                                      // stp_mc.Apply on both offsets, data.cpp:33-34
        double ax, ay, bx, by;
        stp_apply<double>(stp, nd.o1x, nd.o1y, &ax, &ay);
        stp_apply<double>(stp, nd.o2x, nd.o2y, &bx, &by);
        nd.o1x = ax; nd.o1y = ay; nd.o2x = bx; nd.o2y = by;
      }
      const int s = nd.scale == 1 ? 1 : (nd.scale == 2 ? 2 : 0);
      const int pw = pside[s];
      const int x1 = coord_cpp(sh[nd.lm1x2], nd.o1x, pw), y1 = coord_cpp(sh[nd.lm1x2 + 1], nd.o1y, pw);
      const int x2 = coord_cpp(sh[nd.lm2x2], nd.o2x, pw), y2 = coord_cpp(sh[nd.lm2x2 + 1], nd.o2y, pw);
      JDA_BC(Bc(0, (long long)pw * pw), y1 * pw + x1, 1, kBcFinishPix);
      JDA_BC(Bc(0, (long long)pw * pw), y2 * pw + x2, 1, kBcFinishPix);
      const int v = (int)pimg[s][y1 * pw + x1] - (int)pimg[s][y2 * pw + x2];
      node = (v <= nd.th) ? 2 * node + 1 : 2 * node + 2;
    }
    *leaf = node - m.node_n;
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
                            double* t1, double* t2, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_mine_walk, dim3((n + 63) / 64), dim3(64), 0, stream, m, z, items, n, patches, pbytes, similarity, face,
                     carts_n, score, shape, lbf, t1, t2);
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

hipError_t launch_mine_sum(const int* status, unsigned long long n, unsigned long long* out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const unsigned grid = (unsigned)std::min<unsigned long long>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(k_mine_sum, dim3(grid), dim3(256), 0, stream, status, n, out);
  return hipGetLastError();
}

JDA_BC_READER(k_mine)

}  // namespace jda
