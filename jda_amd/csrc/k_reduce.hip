// HIP kernel for gfx950 that packs frames to gray like k_pack.hip, REDUCES them by an integer factor f in 1..8 -- every f x f
// block of gray pixels becomes its mean, rounded to nearest, halves up -- and turns the reduced image by one of the eight
// orientations like k_turn.hip, in one pass (include/jda.h, "frames larger than the faces need"): a 1080p or 4K camera frame
// need not be scanned at full resolution for faces of 100 pixels and more.
//   reduced pixel (i, j) = (S + f*f/2) / (f*f),  S = the sum of the grays at columns [i f, i f + f), rows [j f, j f + f)
//   turned pixel (u, v)  = reduced pixel (x, y):  (x, y) = swap ? (v, u) : (u, v);  x = rw-1-x if flipX;  y = rh-1-y if flipY
//   k_reduce  ONE launch for a ragged set.  A workgroup takes one tile of one image -- at most 64 x 64 pixels of the TURNED
//             REDUCED image, found through block_img and the image record's `first` exactly as in k_turn -- and stages it in
//             LDS at kTurnPitch:
//             - in: a lane takes 4 consecutive reduced pixels of one row of the tile's region of the reduced image: for each of
//               the f source rows it reads the 4 f source pixels, 4 at a time, with pack_row<BPP, 4> (aligned dwords, the
//               lane's own funnel shift, two v_dot4_u32_u8 per colour pixel: pack_pixel.h), adds the four gray bytes of every
//               read to the block sums they belong to -- one v_dot4_u32_u8 with a 0 / 1 byte mask per (read, block) --, divides
//               once per block and writes the four bytes as one ds_write_b32.  The factor is a template parameter (uniform for
//               the workgroup, a switch): masks and the divisor are constants, the division is the compiler's exact multiply
//               and shift.  The source rows are a loop, the f reads of a row are unrolled: f loads in flight.  Every dword
//               read holds a byte of a pixel that takes part: a source that ends with its allocation is safe.  The last,
//               partial group of a region row goes pixel by pixel, byte loads;
//             - out: k_turn's, a second copy of it (sharing it through a header changed k_turn's registers and code: DESIGN.md
//               section 23): a lane takes the 16 bytes at a 16-byte boundary of dst inside one turned row of the tile, gathers
//               them from LDS along the row (mirror: backwards) or down the column (swap) and makes one 16-byte store; heads
//               and tails of row segments are one byte store each, in a pass that only tiles with such bytes run.
//             All offsets are 64-bit.  No atomics, no inline assembly, no scratch; 4352 bytes of LDS.
#include "pack_pixel.h"

namespace jda {

namespace {

constexpr int kReduceLds = kTurnTile * kTurnPitch;

// 16 bytes of the LDS tile from index i on, STEP bytes apart
template <int STEP>
__device__ __forceinline__ pack_u32x4 reduce_read16(const uint8_t* tile, int i) {
  JDA_BC(Bc(0, kReduceLds), STEP > 0 ? i : i + 15 * STEP, 15 * (STEP > 0 ? STEP : -STEP) + 1, kBcPackSrc);
  uint32_t q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 16; k++) q[k >> 2] |= (uint32_t)tile[i + k * STEP] << (8 * (k & 3));
  return pack_u32x4{q[0], q[1], q[2], q[3]};
}

// A tile of an image, as every lane of its workgroup sees it
struct ReduceTile {
  int swap, fx, fy;
  int tw, th;            // the tile: turned columns [u0, u0 + tw), turned rows [v0, v0 + th)
  int sw, sh;            // its region of the reduced image: sw x sh pixels, LDS row ry = reduced row sy0 + ry
  // LDS index of the tile's pixel (du, dv)
  __device__ __forceinline__ int at(int du, int dv) const {
    const int rx = swap ? dv : du, ry = swap ? du : dv;
    return (fy ? sh - 1 - ry : ry) * kTurnPitch + (fx ? sw - 1 - rx : rx);
  }
};

// The gray bytes of 4 source pixels (o, pixels 4 c .. 4 c + 3 of a lane's 4 F) added to the sums of the blocks they fall in
template <int F>
__device__ __forceinline__ void reduce_add(uint32_t o, int c, uint32_t* S) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint32_t m = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) if ((4 * c + k) / F == i) m |= 1u << (8 * k);
    if (m) S[i] = __builtin_amdgcn_udot4(o, m, S[i], false);       // (c, i, k are constants once unrolled)
  }
}

// (S + F*F/2) / (F*F): exact for every S (unsigned division by a constant)
template <int F>
__device__ __forceinline__ uint32_t reduce_mean(uint32_t S) { return (S + (uint32_t)(F * F / 2)) / (uint32_t)(F * F); }

// n (1..4) consecutive reduced pixels -> their bytes in one dword.  row0: the first of their F source rows (the rectangle's
// first participating byte of it), x: their first source pixel's byte in it, row_bytes: the bytes of a row that take part.
template <int F, int BPP>
__device__ __forceinline__ uint32_t reduce_group(pack_src_t row0, long long pitch, long long x, long long row_bytes, int n, uint32_t w_lo,
                                                 uint32_t w_hi) {
  uint32_t S[4] = {0u, 0u, 0u, 0u};
  if (n == 4) {
#pragma unroll 1
    for (int r = 0; r < F; r++) {
      const pack_src_t rp = row0 + r * pitch;
      [[maybe_unused]] const Bc bc_row((long long)(uintptr_t)rp, (long long)(uintptr_t)rp + row_bytes);
      uint32_t o[F];
#pragma unroll
      for (int c = 0; c < F; c++) pack_row<BPP, 4>(rp + x + 4 * c * BPP, w_lo, w_hi, bc_row, &o[c]);
#pragma unroll
      for (int c = 0; c < F; c++) reduce_add<F>(o[c], c, S);
    }
  } else {
#pragma unroll 1
    for (int r = 0; r < F; r++) {
      const pack_src_t rp = row0 + r * pitch;
      [[maybe_unused]] const Bc bc_row((long long)(uintptr_t)rp, (long long)(uintptr_t)rp + row_bytes);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        if (k >= n) break;
#pragma unroll 1
        for (int c = 0; c < F; c++) S[k] += pack_pixel(rp + x + (k * F + c) * BPP, BPP, w_lo, w_hi, bc_row);
      }
    }
  }
  return reduce_mean<F>(S[0]) | (reduce_mean<F>(S[1]) << 8) | (reduce_mean<F>(S[2]) << 16) | (reduce_mean<F>(S[3]) << 24);
}

// ---- in: source rows -> gray -> block means -> LDS.  A lane: reduced pixels [4 q, 4 q + 4) of a region row; lanes l and l + 16
//      are 16 rows apart
template <int F>
__device__ __forceinline__ void reduce_in(const TurnImg& im, const ReduceTile& t, int sx0, int sy0, uint32_t* tile4, int tid) {
  const int lane = tid & 63, wv = tid >> 6, h2 = lane >> 5;
  const int q = lane & 15, hf = (lane >> 4) & 1;
  const long long row_bytes = (long long)im.w * F * im.bpp;
#pragma unroll 1
  for (int p = 0; p < 4; p++) {
    const int idx = p * 8 + wv * 2 + h2, row = hf * 16 + (idx & 15) + 32 * (idx >> 4);
    if (row >= t.sh || 4 * q >= t.sw) continue;
    const pack_src_t row0 = (pack_src_t)im.src + (long long)(sy0 + row) * F * im.pitch;
    const long long x = (long long)(sx0 + 4 * q) * F * im.bpp;
    const int n = min(4, t.sw - 4 * q);
    uint32_t o;
    if (im.bpp == 1) o = reduce_group<F, 1>(row0, im.pitch, x, row_bytes, n, 0u, 0u);
    else if (im.bpp == 3) o = reduce_group<F, 3>(row0, im.pitch, x, row_bytes, n, im.w_lo, im.w_hi);
    else o = reduce_group<F, 4>(row0, im.pitch, x, row_bytes, n, im.w_lo, im.w_hi);
    JDA_BC(Bc(0, kReduceLds), row * kTurnPitch + 4 * q, 4, kBcPackDst);
    tile4[row * (kTurnPitch / 4) + q] = o;
  }
}

}  // namespace

__global__ __launch_bounds__(kTurnBlock) void k_reduce(TurnArgs a) {
  __shared__ uint32_t tile4[kReduceLds / 4];
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
  // (im.w x im.h is the REDUCED rectangle: from here to the way in, and again behind it, this is k_turn)
  const int tv = (int)(tl / im.ntu), tu = (int)(tl - (long long)tv * im.ntu);
  ReduceTile t;
  t.swap = im.tf & kMineSwap; t.fx = im.tf & kMineFlipX; t.fy = im.tf & kMineFlipY;
  const int TW = t.swap ? im.h : im.w, TH = t.swap ? im.w : im.h;
  const int u0 = max(0, kTurnTile * tu - im.off), v0 = kTurnTile * tv;
  t.tw = min(TW, kTurnTile * tu - im.off + kTurnTile) - u0;
  t.th = min(kTurnTile, TH - v0);
  t.sw = t.swap ? t.th : t.tw; t.sh = t.swap ? t.tw : t.th;
  const int xa = t.swap ? v0 : u0, ya = t.swap ? u0 : v0;
  const int sx0 = t.fx ? im.w - xa - t.sw : xa, sy0 = t.fy ? im.h - ya - t.sh : ya;
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, h2 = lane >> 5;

  switch (im.f) {                                                  // uniform for the workgroup
    case 1: reduce_in<1>(im, t, sx0, sy0, tile4, tid); break;
    case 2: reduce_in<2>(im, t, sx0, sy0, tile4, tid); break;
    case 3: reduce_in<3>(im, t, sx0, sy0, tile4, tid); break;
    case 4: reduce_in<4>(im, t, sx0, sy0, tile4, tid); break;
    case 5: reduce_in<5>(im, t, sx0, sy0, tile4, tid); break;
    case 6: reduce_in<6>(im, t, sx0, sy0, tile4, tid); break;
    case 7: reduce_in<7>(im, t, sx0, sy0, tile4, tid); break;
    case 8: reduce_in<8>(im, t, sx0, sy0, tile4, tid); break;
    default: return;                                               // (the host refuses every other factor: never taken)
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
        if (t.swap) o = t.fy ? reduce_read16<-kTurnPitch>(tile, at) : reduce_read16<kTurnPitch>(tile, at);
        else o = t.fx ? reduce_read16<-1>(tile, at) : reduce_read16<1>(tile, at);
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
    JDA_BC(Bc(0, kReduceLds), at, 1, kBcPackSrc);
    JDA_BC_ADDR(bc_dst, dst + p0 + du, 1, kBcPackDst);
    dst[p0 + du] = tile[at];
  }
}

hipError_t launch_reduce(const TurnArgs& a, hipStream_t stream) { return launch_tiles<k_reduce>(a, stream); }

JDA_BC_READER(k_reduce)

}  // namespace jda
