// HIP kernel for gfx950 that packs frames to gray like k_pack.hip and writes every image ROTATED by its own angle (include/jda.h,
// "frames whose faces are rolled"): a head rolled by 30 - 60 degrees, a tilted phone, a ceiling camera.  The plan (c, s, tw, th)
// comes from the host (jdaRotationPlan); everything here is the header's definition, in fp64 with one operation per step
// (-ffp-contract=off) up to a coordinate's rounding to 1/1024 pixel and in integers from there on:
//   turned pixel (u, v):  du = u - cu, dv = v - cv;  sx = (c du + s dv) + cx;  sy = (c dv - s du) + cy
//                         0 unless sx > -1 && sx < w && sy > -1 && sy < h;  X = floor(sx 1024 + 0.5), x0 = X >> 10, fx = X & 1023
//                         (y alike); four gray taps, 0 outside the rectangle, Q10 x Q10 weights in u32;  (sum + 2^19) >> 20
//   k_rotate  ONE launch for a ragged set.  A workgroup takes one tile of one image -- at most 64 x 64 pixels of the TURNED
//             image, found through block_img and the image record's `first` exactly as in k_turn:
//             - box: the tile's four corners go through the map; the columns floor(min sx - 1/1024) .. floor(max sx + 1/1024)
//               + 1 and the rows alike hold every tap of every pixel of the tile that passes the test (DESIGN.md section 24:
//               the proof) and are at most kRotBox x kRotBox;
//             - in: a lane takes 4 consecutive columns of one row of the box: inside the rectangle it reads them with
//               pack_row<BPP, 4> (aligned dwords, the lane's own funnel shift, two v_dot4_u32_u8 per colour pixel:
//               pack_pixel.h), across the rectangle's left and right edges pixel by pixel with pack_pixel, zeros outside
//               -- every source pixel becomes gray ONCE -- and writes the four bytes as one ds_write_b32 at kRotPitch.
//               Every dword read holds a byte of a pixel of the rectangle's row: a source that ends with its allocation is safe;
//             - out: a lane takes the dword at a 4-byte boundary of dst number (lane & 15) of a turned row of the tile, rows
//               lane >> 4, + 16, + 32, + 48: a wave stores 4 runs of 64 consecutive bytes.  Every pixel is the map in fp64,
//               computed from (u, v) itself -- no incremental stepping, which would change bits -- and four ds_read_u8 from
//               the box.  The bytes in front of a row segment's first boundary and behind its last are one byte store each.
//             All offsets are 64-bit.  No atomics, no inline assembly, no scratch; 8832 bytes of LDS.
#include "pack_pixel.h"

namespace jda {

namespace {

constexpr int kRotLds = kRotBox * kRotPitch;
constexpr int kRotGroups = kRotPitch / 4;        // dwords of a box row
static_assert(kRotBox <= kRotPitch && kRotPitch % 4 == 0, "a box row fits its pitch, in whole dwords");

typedef __attribute__((address_space(1))) uint32_t* rot_dst4_t;

// The plan's map and the tile's box, as every lane of the workgroup sees them
struct RotTile {
  double c, s, cu, cv, cx, cy;
  double wd, hd;         // the rectangle's w and h
  int bx0, by0, bw, bh;  // the box: source columns [bx0, bx0 + bw), rows [by0, by0 + bh); LDS byte (y - by0) * kRotPitch + (x - bx0)
  __device__ __forceinline__ void at(int u, int v, double* sx, double* sy) const {
    const double du = (double)u - cu, dv = (double)v - cv;
    const double a = c * du, b = s * dv;
    *sx = (a + b) + cx;
    const double e = c * dv, f = s * du;
    *sy = (e - f) + cy;
  }
};

// turned pixel (u, v) from the box
__device__ __forceinline__ uint32_t rot_pixel(const RotTile& t, const uint8_t* box, int u, int v) {
  double sx, sy;
  t.at(u, v, &sx, &sy);
  if (!(sx > -1.0 && sx < t.wd && sy > -1.0 && sy < t.hd)) return 0u;
  const int X = (int)floor(sx * 1024.0 + 0.5), Y = (int)floor(sy * 1024.0 + 0.5);   // (|X| < 2^27: a rectangle is at most 65536 a side)
  const int x0 = X >> 10, y0 = Y >> 10;
  const uint32_t fx = (uint32_t)(X & 1023), fy = (uint32_t)(Y & 1023);
  const int bx = x0 - t.bx0, by = y0 - t.by0;
#ifdef JDA_BOUNDS_CHECK
  if (bx < 0 || bx + 1 >= t.bw || by < 0 || by + 1 >= t.bh) { jda_bc_fail(kBcPackSrc, __LINE__); return 0u; }   // the covering proof, checked
#endif
  const int i = by * kRotPitch + bx;
  JDA_BC(Bc(0, kRotLds), i, kRotPitch + 2, kBcPackSrc);
  const uint32_t t00 = box[i], t10 = box[i + 1], t01 = box[i + kRotPitch], t11 = box[i + kRotPitch + 1];
  const uint32_t gx = 1024u - fx, gy = 1024u - fy;
  const uint32_t sum = t00 * (gx * gy) + t10 * (fx * gy) + t01 * (gx * fy) + t11 * (fx * fy);
  return (sum + (1u << 19)) >> 20;
}

// 4 consecutive columns from x of source row y -> their gray bytes in one dword, 0 where outside the rectangle
template <int BPP>
__device__ __forceinline__ uint32_t rot_group(const RotImg& im, int x, int y) {
  if (y < 0 || y >= im.h || x + 4 <= 0 || x >= im.w) return 0u;
  const pack_src_t rp = (pack_src_t)im.src + (long long)y * im.pitch;
  [[maybe_unused]] const Bc bc_row((long long)(uintptr_t)rp, (long long)(uintptr_t)rp + (long long)im.w * BPP);
  uint32_t o = 0u;
  if (x >= 0 && x + 4 <= im.w) {
    pack_row<BPP, 4>(rp + (long long)x * BPP, im.w_lo, im.w_hi, bc_row, &o);
  } else {
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
      const int xx = x + k;
      if (xx >= 0 && xx < im.w) o |= pack_pixel(rp + (long long)xx * BPP, BPP, im.w_lo, im.w_hi, bc_row) << (8 * k);
    }
  }
  return o;
}

}  // namespace

__global__ __launch_bounds__(kTurnBlock) void k_rotate(RotArgs a) {
  __shared__ uint32_t box4[kRotLds / 4];
  const uint8_t* box = (const uint8_t*)box4;
  const long long b = blockIdx.x;
  if (b >= a.total) return;
  const int i = a.block_img[b];
  if (i < 0 || i >= a.n) return;                                   // (the host made the list: never taken)
  const RotImg im = a.imgs[i];
  const long long tl = b - im.first;
  if (tl < 0 || tl >= (long long)im.ntu * im.ntv) {                // (the prefix sums cover [0, total): never taken)
#ifdef JDA_BOUNDS_CHECK
    jda_bc_fail(kBcPackDst, __LINE__);
#endif
    return;
  }
  // the tile: turned columns [u0, u0 + ntw), turned rows [v0, v0 + nth)
  const int tv = (int)(tl / im.ntu), tu = (int)(tl - (long long)tv * im.ntu);
  const int TW = im.tw, TH = im.th;
  const int u0 = max(0, kTurnTile * tu - im.off), v0 = kTurnTile * tv;
  const int ntw = min(TW, kTurnTile * tu - im.off + kTurnTile) - u0;
  const int nth = min(kTurnTile, TH - v0);
  const int tid = (int)threadIdx.x;

  RotTile t;
  t.c = im.c; t.s = im.s;
  t.cu = (double)(TW - 1) / 2; t.cv = (double)(TH - 1) / 2; t.cx = (double)(im.w - 1) / 2; t.cy = (double)(im.h - 1) / 2;
  t.wd = (double)im.w; t.hd = (double)im.h;
  {
    // the map is affine: over the tile sx and sy take their extremes at its corners
    double x00, y00, x10, y10, x01, y01, x11, y11;
    t.at(u0, v0, &x00, &y00); t.at(u0 + ntw - 1, v0, &x10, &y10);
    t.at(u0, v0 + nth - 1, &x01, &y01); t.at(u0 + ntw - 1, v0 + nth - 1, &x11, &y11);
    const double xlo = fmin(fmin(x00, x10), fmin(x01, x11)), xhi = fmax(fmax(x00, x10), fmax(x01, x11));
    const double ylo = fmin(fmin(y00, y10), fmin(y01, y11)), yhi = fmax(fmax(y00, y10), fmax(y01, y11));
    t.bx0 = (int)floor(xlo - 1.0 / 1024); t.by0 = (int)floor(ylo - 1.0 / 1024);
    t.bw = (int)floor(xhi + 1.0 / 1024) + 1 - t.bx0 + 1; t.bh = (int)floor(yhi + 1.0 / 1024) + 1 - t.by0 + 1;
  }
  if (t.bw > kRotBox || t.bh > kRotBox) {                          // (63 (|c| + |s|) + 3 < 93: never taken)
#ifdef JDA_BOUNDS_CHECK
    jda_bc_fail(kBcPackSrc, __LINE__);
#endif
    return;
  }

  // ---- in: source rows -> gray -> LDS.  Item e: dword e % 24 of box row e / 24; consecutive lanes write consecutive dwords
  for (int e = tid; e < t.bh * kRotGroups; e += kTurnBlock) {
    const int row = e / kRotGroups, q = e - row * kRotGroups;
    if (4 * q >= t.bw) continue;
    const int x = t.bx0 + 4 * q, y = t.by0 + row;
    uint32_t o;
    if (im.bpp == 1) o = rot_group<1>(im, x, y);
    else if (im.bpp == 3) o = rot_group<3>(im, x, y);
    else o = rot_group<4>(im, x, y);
    JDA_BC(Bc(0, kRotLds), e * 4, 4, kBcPackDst);
    box4[e] = o;
  }
  __syncthreads();

  // ---- out: LDS -> dword stores.  A lane: dword j of the row segments dv, dv + 16, dv + 32, dv + 48
  const pack_dst_t dst = (pack_dst_t)im.dst;
  [[maybe_unused]] const Bc bc_dst((long long)(uintptr_t)im.dst, (long long)(uintptr_t)im.dst + (long long)TW * TH);
  const int j = tid & 15;
#pragma unroll 1
  for (int dv = tid >> 4; dv < nth; dv += 16) {
    const int v = v0 + dv;
    const long long p0 = (long long)v * TW + u0;                     // the row segment's first byte in dst
    const int head = min(ntw, (int)((0 - ((uintptr_t)im.dst + (uintptr_t)p0)) & 3));
    if (j == 0) {
#pragma unroll 1
      for (int k = 0; k < head; k++) {
        JDA_BC_ADDR(bc_dst, dst + p0 + k, 1, kBcPackDst);
        dst[p0 + k] = (uint8_t)rot_pixel(t, box, u0 + k, v);
      }
    }
    const int du = head + 4 * j;                                     // (head + 64 >= ntw: 16 lanes cover the segment)
    if (du + 4 <= ntw) {
      uint32_t o = 0u;
#pragma unroll
      for (int k = 0; k < 4; k++) o |= rot_pixel(t, box, u0 + du + k, v) << (8 * k);
      JDA_BC_ADDR(bc_dst, dst + p0 + du, 4, kBcPackDst);
      *(rot_dst4_t)(dst + p0 + du) = o;                              // 4-byte aligned: head is the segment's distance to its first boundary
    } else {
#pragma unroll 1
      for (int k = du; k < ntw; k++) {
        JDA_BC_ADDR(bc_dst, dst + p0 + k, 1, kBcPackDst);
        dst[p0 + k] = (uint8_t)rot_pixel(t, box, u0 + k, v);
      }
    }
  }
}

hipError_t launch_rotate(const RotArgs& a, hipStream_t stream) { return launch_tiles<k_rotate>(a, stream); }

JDA_BC_READER(k_rotate)

}  // namespace jda
