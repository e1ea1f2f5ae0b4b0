// One stage of the cascade for one window after the scan, what k_finish (k_finish.hip, wave = window) and k_windows
// (k_windows.hip, caller-given windows) share and must agree on bit for bit: the stage's tables in the model (StageTables),
// the resolved stage-0 table of a window size (s0_table_for, k_filter0 too), the choice of walk (WinPix, walk_stage), the
// regression's ordered adds (add_rows), dialect CPP's delta transform (stp_delta) and the end of a window's walk
// (wave_slot, finish_window).
// The loops over rounds of carts, the replay of the score chain and the queues are each kernel's own.  Two things are NOT
// shared because the gfx950 code says no (profiles/finish_shared_isa.txt has every piece against the parent):
//   * k_finish_wide (k_wide.hip) keeps its whole stage body written out: every piece tried in it put an s_waitcnt
//     vmcnt(0) more into the walk blocks of one instantiation or another, and its double-buffered adds as one template
//     cost it a quarter of its waves;
//   * k_windows reads a cart's leaf score, threshold and normalisation from the model's base (m.leaf[(c0 + k) * ..]), not
//     through StageTables: through it both instantiations start their walk loops on a vmcnt(0) the parent does not have.
#pragma once
#include "finish_common.h"

namespace jda {

namespace {

// Records per cart in DevModelT::lm_deep: the nodes below the level-major levels (kernels.h: lm_deep_index).
template <typename Real>
__device__ __forceinline__ int lm_deep_per_cart(const DevModelT<Real>& m) { return m.node_n - ((1 << min(m.lm_split, m.D - 1)) - 1); }

// Stage t's tables in the model: node records (level-major and deep), leaf scores, the carts' thresholds and
// normalisations, weight rows tight (w, dim apart) and padded (w_rows, w_pitch apart).
template <typename DL>
struct StageTables {
  using Real = typename DL::Real;
  const NodeOff<Real>* n_off; const uint2* n_meta; const typename DL::Node* n_deep; int n_split;
  const Real* leaf; const Real* cth; const Real* cmean; const Real* cstd; const uint8_t* cnorm;
  const Real* w; const Real* w_rows;
};
template <typename DL>
__device__ __forceinline__ StageTables<DL> stage_tables(const DevModelT<typename DL::Real>& m, int t) {
  using Real = typename DL::Real;
  const size_t c0 = (size_t)t * m.K;                  // the stage's first cart
  StageTables<DL> s;
  s.n_off = (const NodeOff<Real>*)m.lm_off + c0 * m.node_n;
  s.n_meta = m.lm_meta + c0 * m.node_n;
  s.n_split = m.lm_split;
  s.n_deep = (const typename DL::Node*)m.lm_deep + c0 * lm_deep_per_cart(m);
  s.leaf = m.leaf + c0 * m.leaf_n;
  s.cth = m.cth + c0; s.cmean = m.cmean + c0; s.cstd = m.cstd + c0; s.cnorm = m.cnorm + c0;
  s.w = m.w + c0 * m.leaf_n * m.dim;
  s.w_rows = m.w_rows + c0 * m.leaf_n * m.w_pitch;
  return s;
}

// The resolved stage-0 table of the level whose windows are `win` pixels: lane = level, one ballot.  need_tiled: only a
// level the scan covers (DevLevel::tiled) has one -- k_filter0 passes false, the host launches it only when every level
// has.  Null: no such level.
__device__ __forceinline__ const S0Node* s0_table_for(const DevPlan* __restrict__ plan, const S0Node* __restrict__ s0_table, int win,
                                                      int lane, bool need_tiled) {
  const bool hit = lane < plan->n_levels && plan->lv[lane].win == win;
  const unsigned long long mh = __ballot(hit);
  if (!mh) return nullptr;
  const DevLevel lv = plan->lv[__ffsll((long long)mh) - 1];
  return !need_tiled || lv.tiled ? s0_table + lv.s0_table : nullptr;
}

// Where a window's full-scale pixels are read: the frame (wbase: the window's origin, pitch: the frame's width) or the
// window's own copy in LDS (load_window_tile), when use_tile.
struct WinPix {
  const uint8_t* wbase; int pitch;
  uint8_t* tile; int tpitch; bool use_tile;
  Bc bc;                                              // bounds-check build: the range the frames lie in
};
__device__ __forceinline__ WinPix win_pix(const View& v0, int win, bool use_tile, uint8_t* tile) {
  WinPix p;
  p.wbase = v0.img + (size_t)v0.oy * v0.w + v0.ox; p.pitch = v0.w;
  p.tile = tile; p.tpitch = (win + 3) & ~3; p.use_tile = use_tile;
  p.bc = v0.bc;
  return p;
}

// The walks of G carts of a stage, by the one of four forms that fits: from the resolved stage-0 table (s0 non-null:
// stage 0 of a window whose level has one) or the stage's node tables, pixels from the LDS tile or the frame.
template <typename DL, int G, bool MULTI, bool ST>
__device__ __forceinline__ void walk_stage(const StageTables<DL>& s, const S0Node* __restrict__ s0, const WinPix& px,
                                           const DevModelT<typename DL::Real>& m, const int* kk, const typename DL::Real* sh, int win,
                                           const View& v0, const View& v1, const View& v2, const Stp<typename DL::Real>& stp,
                                           bool apply_st, int* lf, const Bc& bc_lm = Bc(), const Bc& bc_deep = Bc()) {
  if (s0 && px.use_tile) walk_carts_s0<G, true>(s0, m.K, kk, m.D, m.node_n, px.tile, px.tpitch, lf, Bc(0, (long long)px.tpitch * win));
  else if (s0) walk_carts_s0<G, false>(s0, m.K, kk, m.D, m.node_n, px.wbase, px.pitch, lf, px.bc);
  else if (!MULTI && px.use_tile) walk_carts<DL, G, MULTI, ST, true>(s.n_off, s.n_meta, m.K, kk, m.D, m.node_n, sh, win, v0, v1, v2, stp, apply_st, lf, px.tile, px.tpitch, s.n_deep, s.n_split, bc_lm, bc_deep);
  else walk_carts<DL, G, MULTI, ST>(s.n_off, s.n_meta, m.K, kk, m.D, m.node_n, sh, win, v0, v1, v2, stp, apply_st, lf, nullptr, 0, s.n_deep, s.n_split, bc_lm, bc_deep);
}

// The regression of one shape coordinate (c/jda.c:404-411; col: the coordinate's column of the stage's weight rows, lbf[k]:
// the row cart k chose): acc + row 0 + row 1 + .. + row K-1, STRICTLY in cart order -- the order of the adds is the
// specification.  RB row loads in flight, then RB ordered adds, then the tail one by one.  STREAM: non-temporal loads (a
// template parameter: as a run-time branch the optimiser merges the two forms of the load and drops the hint).
// bc, d (bounds-check build): the stage's rows and the coordinate.
template <typename Real, int RB, bool STREAM = false>
__device__ __forceinline__ Real add_rows(const Real* __restrict__ col, const uint32_t* lbf, int K, Real acc,
                                         [[maybe_unused]] const Bc& bc, [[maybe_unused]] int d) {
  int k = 0;
  for (; k + RB <= K; k += RB) {
    Real r[RB];
#pragma unroll
    for (int u = 0; u < RB; u++) { JDA_BC(bc, (long long)lbf[k + u] + d, 1, kBcWRow); r[u] = STREAM ? __builtin_nontemporal_load(col + lbf[k + u]) : col[lbf[k + u]]; }
#pragma unroll
    for (int u = 0; u < RB; u++) acc = acc + r[u];
  }
  for (; k < K; k++) { JDA_BC(bc, (long long)lbf[k] + d, 1, kBcWRow); acc = acc + col[lbf[k]]; }
  return acc;
}

// Dialect CPP: stp_mc.Apply(delta, delta) (btcart.cpp:422, data.hpp:42-45) on the (dx, dy) pair held by lanes d, d ^ 1 (the
// same wave: dim is even); with the identity parameter this is the literal 1*(1*x+0*y) / 1*(0*x+1*y).  Every lane of the
// wave calls it, whether it holds a coordinate or not.
template <typename Real>
__device__ __forceinline__ Real stp_delta(const Stp<Real>& stp, Real acc, int d) {
  const Real other = __shfl_xor(acc, 1);
  return (d & 1) ? stp.scale * (stp.r10 * other + stp.r11 * acc) : stp.scale * (stp.r00 * acc + stp.r01 * other);
}

// The next slot of a queue for a wave: lane 0 counts, every lane gets it.
__device__ __forceinline__ unsigned wave_slot(unsigned long long* counter, int lane) {
  unsigned o = 0;
  if (lane == 0) o = (unsigned)atomicAdd(counter, 1ull);
  return (unsigned)__shfl((int)o, 0);
}

// A window's walk is over (rejected, or past the last stage): its trace record, the final cut (c/jda.c:414), and for a
// detection the slot of the list and the copy of its shape.  By the nt threads tid = 0..nt-1 that hold the window; slot():
// the list's next slot, the same value in every thread (wave_slot, or LDS and a barrier).
template <bool TRACE, typename Real, typename Slot>
__device__ __forceinline__ void finish_window(const WorkT<Real>& w, uint32_t gid, bool alive, int carts_n, Real score, unsigned hash,
                                              bool cut, const Real* sh, int dim, int tid, int nt, const Slot& slot) {
  if (TRACE) {
    if (tid == 0) { w.tr_carts[gid] = carts_n; w.tr_score[gid] = score; w.tr_hash[gid] = hash; }
    for (int d = tid; d < dim; d += nt) w.tr_shape[(size_t)gid * dim + d] = sh[d];
  }
  if (alive && !cut) {
    const unsigned o = slot();
    if (o < w.cap_m) {
      if (tid == 0) { w.out_gid[o] = gid; w.out_score[o] = score; }
      for (int d = tid; d < dim; d += nt) w.out_shape[(size_t)o * dim + d] = sh[d];
    }
  }
}

}  // namespace

}  // namespace jda
