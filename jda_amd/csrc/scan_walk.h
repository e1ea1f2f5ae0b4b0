// Stage 0 over resolved nodes (S0Node), what k_scan (k_scan_impl.h, closed tiles) and k_scan_p (k_scan_p.hip,
// persistent) share and must agree on bit for bit: the tree walks (s0_left, scan_tree, scan_trees), the record the
// score step reads (ThNorm), a tile's geometry (tile_geo) and the hand-off record (handoff_write).
// The score recurrence, the batch replay, the survivor compaction and the fetch of a ragged block are still spelled out
// in both kernels; what was measured of sharing them is in profiles/scan_shared_isa.txt.
// Reference loop being replaced: c/jda.c:357-402 (stage 0: every window still holds the mean shape, so the
// feature offsets are resolved per (node, level) by k_prep_stage0).
#pragma once
#include "kernels_common.h"

namespace jda {

namespace {

// Feature test of one resolved stage-0 node for the window at `base`: true = go left
// (feature <= threshold, c/jda.c:391-393).  WIDE: the 21-bit packing (S0Node).
// bc: what `pix + index` may touch -- indices inside the LDS tile, or (global-pixel mode) addresses inside the frames
template <bool WIDE>
__device__ __forceinline__ bool s0_left(const S0Node r, const uint8_t* __restrict__ pix, int base, const Bc& bc = Bc(), bool bc_addr = false) {
  if (!WIDE) {
    JDA_BC(bc, base + (int)(r.lo & 0xffffu), 1, kBcScanPixLds); JDA_BC(bc, base + (int)(r.lo >> 16), 1, kBcScanPixLds);
    const int a = pix[base + (int)(r.lo & 0xffffu)];
    const int b = pix[base + (int)(r.lo >> 16)];
    return a - b <= (int)r.hi;
  }
  const uint32_t o1 = r.lo & 0x1fffffu;
  const uint32_t o2 = __builtin_amdgcn_alignbit(r.hi, r.lo, 21) & 0x1fffffu;
#ifdef JDA_BOUNDS_CHECK
  if (bc_addr) { JDA_BC_ADDR(bc, pix + base + (int)o1, 1, kBcScanPixGlb); JDA_BC_ADDR(bc, pix + base + (int)o2, 1, kBcScanPixGlb); }
  else { JDA_BC(bc, base + (int)o1, 1, kBcScanPixLds); JDA_BC(bc, base + (int)o2, 1, kBcScanPixLds); }
#endif
  const int a = pix[base + (int)o1];
  const int b = pix[base + (int)o2];
  return a - b + 256 <= (int)(r.hi >> 10);
}

// One cart of stage 0 for one window -> node index reached below the last split level:
// D-1 dependent (node record, 2 pixels) reads.  The node table is in LDS; pixels come
// from the LDS tile or from the frame through L1/L2.
// (Testing the root and both children at once -- 2 dependent round trips instead of 3,
// 8 pixel reads instead of 6 -- was measured 15 % SLOWER: the kernel is sensitive to LDS
// instruction count, see DESIGN.md.)
template <int DEPTH, bool WIDE>
__device__ __forceinline__ int scan_tree(const S0Node* __restrict__ tbl, const uint8_t* __restrict__ pix,
                                         int base, int depth_rt, const Bc& bc = Bc(), bool bc_addr = false) {
  int node = 0;
  const int levels = DEPTH > 0 ? DEPTH - 1 : depth_rt - 1;
#pragma unroll
  for (int d = 0; d < levels; d++) {
    const S0Node r = tbl[node];
    node = 2 * node + (s0_left<WIDE>(r, pix, base, bc, bc_addr) ? 1 : 2);
  }
  return node;
}

// N trees in lockstep, written level-major: the N node records of a level first, then the 2N pixels, then the N
// compares.  scan_tree called N times leaves the interleaving of the N independent chains to the instruction
// scheduler, which does it for the uniform-batch instantiation and -- two VGPRs of pressure later -- walks the trees
// one after the other in the RAGGED one (every LDS read followed by lgkmcnt(0): phases 30-60 % slower, stamps and ISA
// in profiles/r03_ragged_scan.txt).  Same reads, same compares.
template <int DEPTH, bool WIDE, int N>
__device__ __forceinline__ void scan_trees(const S0Node* __restrict__ t_nodes, int k, int node_n,
                                           const uint8_t* __restrict__ pix, int base, int depth_rt, int* lf,
                                           int kstride = 1, int kmax = 0x7fffffff, const Bc& bc = Bc(), bool bc_addr = false) {
  int node[N];
#pragma unroll
  for (int u = 0; u < N; u++) node[u] = 0;
  const int levels = DEPTH > 0 ? DEPTH - 1 : depth_rt - 1;
#pragma unroll
  for (int d = 0; d < levels; d++) {
    S0Node r[N];
#pragma unroll
    for (int u = 0; u < N; u++) r[u] = t_nodes[min(k + u * kstride, kmax) * node_n + node[u]];
    int a[N], b[N];
#pragma unroll
    for (int u = 0; u < N; u++) {
      if (!WIDE) {
        JDA_BC(bc, base + (int)(r[u].lo & 0xffffu), 1, kBcScanPixLds); JDA_BC(bc, base + (int)(r[u].lo >> 16), 1, kBcScanPixLds);
        a[u] = pix[base + (int)(r[u].lo & 0xffffu)];
        b[u] = pix[base + (int)(r[u].lo >> 16)];
      } else {
        const uint32_t o1 = r[u].lo & 0x1fffffu;
        const uint32_t o2 = __builtin_amdgcn_alignbit(r[u].hi, r[u].lo, 21) & 0x1fffffu;
#ifdef JDA_BOUNDS_CHECK
        if (bc_addr) { JDA_BC_ADDR(bc, pix + base + (int)o1, 1, kBcScanPixGlb); JDA_BC_ADDR(bc, pix + base + (int)o2, 1, kBcScanPixGlb); }
        else { JDA_BC(bc, base + (int)o1, 1, kBcScanPixLds); JDA_BC(bc, base + (int)o2, 1, kBcScanPixLds); }
#endif
        a[u] = pix[base + (int)o1];
        b[u] = pix[base + (int)o2];
      }
    }
#pragma unroll
    for (int u = 0; u < N; u++) {
      const bool left = WIDE ? (a[u] - b[u] + 256 <= (int)(r[u].hi >> 10)) : (a[u] - b[u] <= (int)r[u].hi);
      node[u] = 2 * node[u] + (left ? 1 : 2);
    }
  }
#pragma unroll
  for (int u = 0; u < N; u++) lf[u] = node[u] - node_n;
}

// First half of CartPar: all a cart's score step needs where the cart does not normalise (the common case)
template <typename Real>
struct ThNorm { Real th, norm; };

// Tile `trel` of a grid of nx x ny windows cut into tiles of tw x th: its first window, its windows (edge tiles are
// smaller), its origin and its extent in pixels.
struct TileGeo { int wx0, wy0, twe, the, x0, y0, pw, ph; };
__device__ __forceinline__ TileGeo tile_geo(int trel, int tiles_x, int tw, int th, int nx, int ny, int step, int win) {
  TileGeo g;
  const int ty = trel / tiles_x, tx = trel - ty * tiles_x;
  g.wx0 = tx * tw; g.wy0 = ty * th;
  g.twe = min(tw, nx - g.wx0); g.the = min(th, ny - g.wy0);
  g.x0 = g.wx0 * step; g.y0 = g.wy0 * step;
  g.pw = win + (g.twe - 1) * step; g.ph = win + (g.the - 1) * step;
  return g;
}

// One window that is alive after cart K - 1 of stage 0 -> entry `slot` of the hand-off queue (k_filter0 / k_finish
// continue at cart K) or, to_mid (K = all of stage 0), of the mid queue as k_filter0 leaves it -- without stage-0
// leaves (m_k0 = K: k_finish(survivors) walks them all).  (wx, wy): the window in its level's grid.  false: the queue
// is full (the counters keep counting: Pass::recover_overflow).
template <typename Real>
__device__ __forceinline__ bool handoff_write(const WorkT<Real>& w, unsigned slot, bool to_mid, uint32_t gid, Real score, int K,
                                              int wx, int wy, int step, int win, int frame) {
  if (slot >= (to_mid ? w.cap_m : w.cap_q)) return false;
  JDA_BC(Bc(0, to_mid ? w.cap_m : w.cap_q), slot, 1, kBcQueue);
  const uint32_t xy = (uint32_t)(wx * step) | ((uint32_t)(wy * step) << 16);
  const uint32_t wf = (uint32_t)win | ((uint32_t)frame << 16);
  if (to_mid) {
    w.m_gid[slot] = gid; w.m_score[slot] = score; w.m_xy[slot] = xy; w.m_wf[slot] = wf; w.m_k0[slot] = (uint32_t)K;
  } else {
    w.q_gid[slot] = gid; w.q_score[slot] = score; w.q_kstart[slot] = (uint32_t)K; w.q_xy[slot] = xy; w.q_wf[slot] = wf;
  }
  return true;
}

}  // namespace

}  // namespace jda
