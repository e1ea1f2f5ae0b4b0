// HIP kernel for gfx950 that packs frames to gray like k_pack.hip AND turns them by one of the eight orientations on the way
// (include/jda.h, "frames in any orientation"): a phone's sensor rows with their "rotate 90 degrees to display" tag, a
// mirrored front camera, a video decoder that leaves the rotation to the consumer.
//   turned pixel (u, v) = rectangle pixel (x, y):  (x, y) = swap ? (v, u) : (u, v);  x = w-1-x if flipX;  y = h-1-y if flipY
//   k_turn    ONE launch for a ragged set.  A workgroup takes one tile of one image -- at most 64 x 64 pixels of the TURNED
//             image, found through block_img (an item per workgroup, made by the host) and the image record's `first`.  A
//             transposing orientation cannot be read in rows and written in rows without staging, so the tile goes through LDS:
//             - in: the tile's source region (again at most 64 x 64: its rows are the tile's columns under a swap) is read row
//               by row, a lane taking 4 consecutive pixels: its 4 * bpp bytes as aligned dwords -- bpp of them, and one more
//               where the first pixel does not start a dword -- funnelled by the lane's own shift (v_alignbyte_b32) and turned
//               into gray by two v_dot4_u32_u8 per pixel, exactly as k_pack does (pack_pixel.h).  Every dword read holds a byte
//               of a pixel of the region's row: a source that ends with its allocation is safe.  The last, partial group of a
//               region row reads pixel by pixel, byte loads.  The 4 gray bytes are one ds_write_b32;
//             - the LDS tile has rows of kTurnPitch = 68 bytes (17 dwords); lanes l and l + 16 write rows 16 apart, lanes of
//               one read instruction are dealt so that they meet 32 different banks or one dword;
//             - out: a lane takes the 16 bytes at a 16-byte boundary of dst inside one turned row of the tile, gathers them
//               from LDS along the row (mirror: backwards) or down the column (swap), and makes one 16-byte store.  Tile
//               columns are laid from dst's alignment (TurnImg::off), so where the turned width is a multiple of 16 nothing
//               else is left; elsewhere the at most 15 bytes in front of a row segment's first boundary and behind its last
//               are one byte store each, in a pass of their own that such tiles alone run.
//             All offsets are 64-bit.  No atomics, no inline assembly, no scratch; 4352 bytes of LDS.
#include "pack_pixel.h"

namespace jda {

namespace {

constexpr int kTurnLds = kTurnTile * kTurnPitch;

// 16 bytes of the LDS tile from index i on, STEP bytes apart
template <int STEP>
__device__ __forceinline__ pack_u32x4 turn_read16(const uint8_t* tile, int i) {
  JDA_BC(Bc(0, kTurnLds), STEP > 0 ? i : i + 15 * STEP, 15 * (STEP > 0 ? STEP : -STEP) + 1, kBcPackSrc);
  uint32_t q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 16; k++) q[k >> 2] |= (uint32_t)tile[i + k * STEP] << (8 * (k & 3));
  return pack_u32x4{q[0], q[1], q[2], q[3]};
}

// A tile of an image, as every lane of its workgroup sees it
struct TurnTile {
  int swap, fx, fy;
  int tw, th;            // the tile: turned columns [u0, u0 + tw), turned rows [v0, v0 + th)
  int sw, sh;            // its source region: sw x sh pixels, LDS row ry = source row sy0 + ry
  // LDS index of the tile's pixel (du, dv)
  __device__ __forceinline__ int at(int du, int dv) const {
    const int rx = swap ? dv : du, ry = swap ? du : dv;
    return (fy ? sh - 1 - ry : ry) * kTurnPitch + (fx ? sw - 1 - rx : rx);
  }
};

}  // namespace

__global__ __launch_bounds__(kTurnBlock) void k_turn(TurnArgs a) {
  __shared__ uint32_t tile4[kTurnLds / 4];
  const uint8_t* tile = (const uint8_t*)tile4;
  const long long b = blockIdx.x;
  if (b >= a.total) return;
  const int i = a.block_img[b];
  if (i < 0 || i >= a.n) return;                                   // (the host made the list: never taken)
  const TurnImg im = a.imgs[i];
  const long long tl = b - im.first;
  if (tl < 0 || tl >= (long long)im.ntu * im.ntv) {                // (the prefix sums cover [0, total): never taken)
#ifdef JDA_BOUNDS_CHECK
    jda_bc_fail(kBcPackDst, __LINE__);
#endif
    return;
  }
  const int tv = (int)(tl / im.ntu), tu = (int)(tl - (long long)tv * im.ntu);
  TurnTile t;
  t.swap = im.tf & kMineSwap; t.fx = im.tf & kMineFlipX; t.fy = im.tf & kMineFlipY;
  const int TW = t.swap ? im.h : im.w, TH = t.swap ? im.w : im.h;
  const int u0 = max(0, kTurnTile * tu - im.off), v0 = kTurnTile * tv;
  t.tw = min(TW, kTurnTile * tu - im.off + kTurnTile) - u0;
  t.th = min(kTurnTile, TH - v0);
  t.sw = t.swap ? t.th : t.tw; t.sh = t.swap ? t.tw : t.th;
  const int xa = t.swap ? v0 : u0, ya = t.swap ? u0 : v0;
  const int sx0 = t.fx ? im.w - xa - t.sw : xa, sy0 = t.fy ? im.h - ya - t.sh : ya;
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, h2 = lane >> 5;

  // ---- in: source rows -> gray -> LDS.  A lane: pixels [4 q, 4 q + 4) of a region row; lanes l and l + 16 are 16 rows apart
  {
    const int q = lane & 15, hf = (lane >> 4) & 1;
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const int idx = p * 8 + wv * 2 + h2, row = hf * 16 + (idx & 15) + 32 * (idx >> 4);
      if (row >= t.sh || 4 * q >= t.sw) continue;
      const pack_src_t rowp = (pack_src_t)im.src + (long long)(sy0 + row) * im.pitch;
      [[maybe_unused]] const Bc bc_row((long long)(uintptr_t)rowp, (long long)(uintptr_t)rowp + (long long)im.w * im.bpp);
      const pack_src_t s = rowp + (long long)(sx0 + 4 * q) * im.bpp;
      uint32_t o = 0u;
      if (4 * q + 4 <= t.sw) {
        if (im.bpp == 1) pack_row<1, 4>(s, 0u, 0u, bc_row, &o);
        else if (im.bpp == 3) pack_row<3, 4>(s, im.w_lo, im.w_hi, bc_row, &o);
        else pack_row<4, 4>(s, im.w_lo, im.w_hi, bc_row, &o);
      } else {
        for (int k = 0; 4 * q + k < t.sw; k++) o |= pack_pixel(s + k * im.bpp, im.bpp, im.w_lo, im.w_hi, bc_row) << (8 * k);
      }
      JDA_BC(Bc(0, kTurnLds), row * kTurnPitch + 4 * q, 4, kBcPackDst);
      tile4[row * (kTurnPitch / 4) + q] = o;
    }
  }
  __syncthreads();

  // ---- out: LDS -> 16-byte stores.  A lane: unit s (the s-th run of 16 bytes at a 16-byte boundary of dst) of turned row dv
  const pack_dst_t dst = (pack_dst_t)im.dst;
  [[maybe_unused]] const Bc bc_dst((long long)(uintptr_t)im.dst, (long long)(uintptr_t)im.dst + (long long)TW * TH);
  {
    const int g = wv * 2 + h2, l = lane & 31;
    // (the 32 lanes of one LDS read: swap -- 16 rows x 2 units; otherwise rows {r .. r + 3, r + 16 .. r + 19} x 4 units)
    const int s = t.swap ? (l & 1) + 2 * (g >> 2) : l & 3;
    const int dv = t.swap ? (l >> 1) + 16 * (g & 3) : 4 * (g & 3) + 32 * (g >> 2) + ((l >> 2) & 3) + 16 * (l >> 4);
    if (dv < t.th) {
      const long long p0 = (long long)(v0 + dv) * TW + u0;           // the row segment's first byte in dst
      const int head = min(t.tw, (int)((0 - ((uintptr_t)im.dst + (uintptr_t)p0)) & 15));
      const int du = head + 16 * s;
      if (du + 16 <= t.tw) {
        const int at = t.at(du, dv);
        pack_u32x4 o;
        if (t.swap) o = t.fy ? turn_read16<-kTurnPitch>(tile, at) : turn_read16<kTurnPitch>(tile, at);
        else o = t.fx ? turn_read16<-1>(tile, at) : turn_read16<1>(tile, at);
        JDA_BC_ADDR(bc_dst, dst + p0 + du, 16, kBcPackDst);
        *(pack_dst16_t)(dst + p0 + du) = o;                          // 16-byte aligned: head is the segment's distance to its first boundary
      }
    }
  }
  // ---- the bytes in front of a row segment's first boundary and behind its last: none where every row segment of the tile
  //      begins and ends at a boundary (uniform for the workgroup)
  const uintptr_t a0 = (uintptr_t)im.dst + (uintptr_t)((long long)v0 * TW + u0);
  if ((TW & 15) == 0 && (a0 & 15) == 0 && (t.tw & 15) == 0) return;
  for (int e = tid; e < t.th * 32; e += kTurnBlock) {                // 32 slots a row: 16 in front, 16 behind
    const int dv = e >> 5, j = e & 31;
    const long long p0 = (long long)(v0 + dv) * TW + u0;
    const int head = min(t.tw, (int)((0 - ((uintptr_t)im.dst + (uintptr_t)p0)) & 15));
    const int body = ((t.tw - head) >> 4) << 4, tail = t.tw - head - body;
    int du = -1;
    if (j < 16) { if (j < head) du = j; }
    else if (j - 16 < tail) du = head + body + (j - 16);
    if (du < 0) continue;
    const int at = t.at(du, dv);
    JDA_BC(Bc(0, kTurnLds), at, 1, kBcPackSrc);
    JDA_BC_ADDR(bc_dst, dst + p0 + du, 1, kBcPackDst);
    dst[p0 + du] = tile[at];
  }
}

hipError_t launch_turn(const TurnArgs& a, hipStream_t stream) { return launch_tiles<k_turn>(a, stream); }

JDA_BC_READER(k_turn)

}  // namespace jda
