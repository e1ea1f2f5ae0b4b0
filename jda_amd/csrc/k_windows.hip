// HIP kernel of dialect C's window body on CALLER-GIVEN windows for gfx950 (reference c/jda.c:340-414 and 471-472;
// jdaValidateWindows / jdaValidateWindowsDevice, windows.cpp): the work list is the caller's (frame, x, y, size) list, not a
// scan plan's -- no grid, no minimum size, no NMS.
//   k_windows  wave = window (one-wave workgroups, grid-stride over the list), k_finish's form on k_finish's stage body
//              (stage_body.h).  The shape (2L floats) and the stage's K chosen weight rows live in the workgroup's LDS, and -- windows
//              up to WinArgs::tile_win pixels of a single-scale model -- the window's own pixels (load_window_tile); larger
//              windows and multi-scale models read their pixels from the frame and the half / quarter images.  Per stage:
//              walk     lane = cart, 64 carts a round: walk_stage (stage_body.h) on the level-major node tables, from cart 0
//                       of stage 0 -- no queue, no hand-off, no stage-0 hoist table
//              replay   the score chain of those carts IN CART ORDER (c/jda.c:396-397): one fp32 add per cart and, where the
//                       cart normalises, one subtract and one IEEE division ((s - 0) / 1 is s, bit for bit, so the carts with
//                       (mean, std) = (0, 1) skip them); the operands go from the cart's lane to the whole wave by v_readlane,
//                       lane l keeps the score as it stood after cart l
//              reject   `score < th` per lane, one ballot: the first set bit is the first failing cart (c/jda.c:399) -- it fixes
//                       carts_n, the score where the walk stopped, the hash and the shape as it stood
//              regress  a window that passed the stage: lane = shape coordinate, the K rows added in cart order
//                       (c/jda.c:404-411; add_rows)
//              Results go out by window index -- the caller's order, no atomics, nothing between waves.
// No inline assembly, no scratch (the row batch of the regression is a fixed-size register array).
#include "stage_body.h"

namespace jda {

namespace {

constexpr int kWinRowBatch = 16;       // weight rows in flight per lane in the regression

// LDS of a workgroup without the pixel tile: shape [dim_pad] floats, lbf [K rounded up to 4] row offsets
__host__ __device__ inline size_t windows_lds_base(int dim, int K) {
  return (((size_t)((dim + 1) & ~1) * sizeof(float) + (size_t)((K + 3) & ~3) * 4) + 15) & ~(size_t)15;
}

}  // namespace

template <bool MULTI>
__global__ __launch_bounds__(64) void k_windows(DevModelT<float> m, WinArgs a, float inv_sqrt2) {
  using DL = DialectC;
  extern __shared__ __attribute__((aligned(16))) unsigned char win_lds[];
  const int lane = threadIdx.x;
  const int T = m.T, K = m.K, node_n = m.node_n, leaf_n = m.leaf_n, dim = m.dim, w_pitch = m.w_pitch;
  const int dim_pad = (dim + 1) & ~1;
  float* sh = (float*)win_lds;                               // current shape [dim_pad]
  uint32_t* lbf = (uint32_t*)(sh + dim_pad);                 // weight row (in elements) chosen by every cart of the stage [K]
  uint8_t* tile = win_lds + windows_lds_base(dim, K);        // the window's pixels (tile_win > 0)
  const Stp<float> stp{1.f, 1.f, 0.f, 0.f, 1.f};             // (dialect C has no similarity transform: never applied)
  [[maybe_unused]] const Bc bc_frames((long long)(uintptr_t)a.frames,
                                      (long long)(uintptr_t)(a.frames + (size_t)(a.n_frames - 1) * a.frame_stride + (size_t)a.width * a.height));
  [[maybe_unused]] const Bc bc_lm(0, (long long)K * node_n), bc_deep(0, (long long)K * lm_deep_per_cart(m));
  [[maybe_unused]] const Bc bc_carts(0, (long long)T * K), bc_leaves(0, (long long)T * K * leaf_n);

  for (long long i = blockIdx.x; i < a.n; i += gridDim.x) {
    JDA_BC(Bc(0, a.n), i, 1, kBcWinList);
    const int4 wd = a.windows[i];                            // (frame, x, y, size), validated by the host
    const int frame = wd.x, x = wd.y, y = wd.z, win = wd.w;
    JDA_BC(Bc(0, a.n_frames), frame, 1, kBcWinList);
    View v0{}, v1{}, v2{};
    v0.img = a.frames + (size_t)frame * a.frame_stride; v0.w = a.width; v0.h = a.height; v0.ox = x; v0.oy = y; v0.pw = win;
    if (MULTI) {
      v1.img = a.half + (size_t)frame * a.half_stride; v1.w = a.hw; v1.h = a.hh;
      v2.img = a.quarter + (size_t)frame * a.quarter_stride; v2.w = a.qw; v2.h = a.qh;
      views_c(x, y, win, inv_sqrt2, &v1, &v2);
    }
#ifdef JDA_BOUNDS_CHECK
    v0.bc = bc_frames;
    if (MULTI) {
      v1.bc = Bc((long long)(uintptr_t)a.half, (long long)(uintptr_t)(a.half + (size_t)(a.n_frames - 1) * a.half_stride + (size_t)a.hw * a.hh));
      v2.bc = Bc((long long)(uintptr_t)a.quarter, (long long)(uintptr_t)(a.quarter + (size_t)(a.n_frames - 1) * a.quarter_stride + (size_t)a.qw * a.qh));
    }
#endif
    const WinPix px = win_pix(v0, win, !MULTI && win <= a.tile_win, tile);
    __syncthreads();                                         // the previous window's readers are done with sh, lbf and the tile
    if (!MULTI && px.use_tile) load_window_tile(px.wbase, px.pitch, win, px.tile, px.tpitch, lane, 64, px.bc);
    for (int d = lane; d < dim; d += 64) sh[d] = m.mean_shape[d];          // c/jda.c:361
    __syncthreads();

    float score = 0.f;                                       // wave-uniform: every lane runs the same chain
    unsigned hash = kFnvSeed;
    bool alive = true;
    int carts_n = 0;
    for (int t = 0; t < T && alive; t++) {
      const StageTables<DL> s = stage_tables<DL>(m, t);
      const size_t c0 = (size_t)t * K;                       // the stage's cart records, read from the model's base (stage_body.h says why)
      for (int k0 = 0; k0 < K && alive; k0 += 64) {
        // ---- walk: lane = cart (lanes past cart K - 1 repeat it and are not used)
        int kk[1], lf[1];
        kk[0] = min(k0 + lane, K - 1);
        walk_stage<DL, 1, MULTI, false>(s, nullptr, px, m, kk, sh, win, v0, v1, v2, stp, false, lf, bc_lm, bc_deep);
        const int k = k0 + lane;
        const bool active = k < K;
        float ls = 0.f, thk = 0.f, mk = 0.f, sk = 1.f;
        bool nrm = false;
        if (active) {
          JDA_BC(bc_carts, (long long)(c0 + k), 1, kBcNodeTable);
          JDA_BC(bc_leaves, (long long)((c0 + k) * leaf_n + lf[0]), 1, kBcNodeTable);
          lbf[k] = (uint32_t)(k * leaf_n + lf[0]) * (uint32_t)w_pitch;       // c/jda.c:400, as the row's offset
          ls = m.leaf[(c0 + k) * leaf_n + lf[0]];
          thk = m.cth[c0 + k];
          nrm = m.cnorm[c0 + k] != 0;
          if (nrm) { mk = m.cmean[c0 + k]; sk = m.cstd[c0 + k]; }
        }
        // ---- replay, in cart order (c/jda.c:396-397)
        const int cnt = min(64, K - k0);
        const unsigned long long normmask = __ballot(nrm);
        float mine = 0.f;
        for (int l = 0; l < cnt; l++) {
          score = score + rl(ls, l);
          if ((normmask >> l) & 1ull) score = (score - rl(mk, l)) / rl(sk, l);
          if (lane == l) mine = score;
        }
        // ---- reject (c/jda.c:399): the first failing cart.  A NaN score fails no comparison.
        const unsigned long long failed = __ballot(active && mine < thk);
        int last = cnt - 1;                                  // last cart of the round that was evaluated
        if (failed) {
          last = __ffsll((long long)failed) - 1;
          score = rl(mine, last);
          alive = false;
          carts_n = t * K + k0 + last + 1;
        }
        if (a.hash != nullptr)
          for (int l = 0; l <= last; l++) hash = fnv_step(hash, rl(lf[0], l));
      }
      if (!alive) break;
      __syncthreads();                                       // the stage's rows, written by their carts' lanes
      // ---- regression (c/jda.c:404-411): lane = coordinate, rows in cart order
      for (int d = lane; d < dim; d += 64)                   // (coordinate d is read and written by this lane alone)
        sh[d] = add_rows<float, kWinRowBatch>(s.w_rows + d, lbf, K, sh[d], Bc(0, (long long)K * leaf_n * w_pitch), d);
      __syncthreads();                                       // the next stage's walk reads every coordinate
    }
    if (alive) carts_n = T * K;

    // ---- results, by window index
    JDA_BC(Bc(0, a.n), i, 1, kBcWinOut);
    if (lane == 0) {
      if (a.face) a.face[i] = (alive && !(score < a.th)) ? 1 : 0;             // c/jda.c:414
      if (a.score) a.score[i] = score;
      if (a.carts_n) a.carts_n[i] = carts_n;
      if (a.hash) a.hash[i] = hash;
    }
    const float fx = (float)x, fy = (float)y, fs = (float)win;
    for (int d = lane; d < dim; d += 64) {
      JDA_BC(Bc(0, (long long)a.n * dim), i * dim + d, 1, kBcWinOut);
      const float v = sh[d];
      if (a.shapes) a.shapes[(size_t)i * dim + d] = v;
      if (a.landmarks) {                                     // c/jda.c:471-472: a multiply, then an add
        const float p = v * fs;
        a.landmarks[(size_t)i * dim + d] = p + ((d & 1) ? fy : fx);
      }
    }
  }
}

int windows_tile_limit(int dim, int K) {
  const size_t base = windows_lds_base(dim, K);
  int tile_win = 0;
  for (int tw = 1; tw <= 255; tw++)
    if (base + finish_tile_bytes(tw) <= kFinishLdsPerGroup) tile_win = tw;
  return tile_win;
}

hipError_t launch_windows(const DevModelT<float>& m, const WinArgs& a, hipStream_t stream) {
  if (a.n <= 0) return hipSuccess;
  if (m.K < 1 || m.D < 1 || m.D > 20 || m.dim < 2 || a.n_frames < 1) return hipErrorInvalidValue;
  const bool multi = a.half != nullptr;
  const int tile_win = multi ? 0 : std::max(0, std::min(a.tile_win, windows_tile_limit(m.dim, m.K)));
  WinArgs b = a;
  b.tile_win = tile_win;
  const size_t lds = windows_lds_base(m.dim, m.K) + finish_tile_bytes(tile_win);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  const float r = 1.f / sqrtf(2.f);                          // c/jda.c:341
  // one window per workgroup while the list is short enough (the dispatcher balances the very uneven walks), grid-stride beyond
  const unsigned blocks = (unsigned)std::min<long long>(a.n, 1 << 20);
  auto go = [&](auto kern) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64), lds, stream, m, b, r);
  };
  if (multi) go(k_windows<true>); else go(k_windows<false>);
  return hipGetLastError();
}

JDA_BC_READER(k_windows)

}  // namespace jda
