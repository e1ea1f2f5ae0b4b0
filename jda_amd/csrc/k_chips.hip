// HIP kernel for gfx950 that cuts upright face chips out of the source images (include/jda.h, "faces as they leave"): a chip
// pixel is the mean of n x n bilinear samples of the source, taken where the face's similarity transform (fitted on the host,
// chips.cpp) puts the sub-pixel centres.  Coordinates are fp64 (no contraction: the build's -ffp-contract=off), everything
// behind the rounding of a coordinate to 1/1024 pixel is integer, so the chip equals the host form's to the byte.
//   k_chips   ONE launch for a ragged set of faces.  All chips of a call have one size and lie back to back, so the call's
//             output is one run of bytes, dealt in units (kernels.h: ChipArgs) whatever the chips' size: lane = unit; a unit
//             below nq is the 16 bytes at a 16-byte boundary of dst, ONE 16-byte store; the bytes in front of the first
//             boundary and behind the last (at most 15 each per call) are one byte store each.  A 45-byte chip begins anywhere
//             inside a unit: a lane finds the face, row, column and channel of its first byte by division and walks on from
//             there, pixel by pixel, into the next row and the next face (whose record it then loads).  A 24 x 24 chip fills
//             its lanes like a 224 x 224 one.
//             - a pixel that the unit holds a byte of is computed whole (its 1 or 3 channels share coordinates and taps);
//               a BGR24 unit computes 6 or 7 pixels for its 5 1/3;
//             - taps are byte loads straight through L1 (the four taps of a sample share one or two cache lines, neighbouring
//               lanes are neighbouring chip pixels): a tap outside the image, or one whose weight is 0, is not read, alpha
//               is never read, so a source that ends with its allocation is safe;
//             - all offsets are 64-bit.  No LDS, no atomics, no inline assembly, no scratch.
#include "pack_pixel.h"   // the pack_*_t typedefs, pack_unit, pack_divmod: shared with k_pack.hip

namespace jda {

namespace {

// One tap of weight wgt at (x, y) into the CC channel sums: nothing outside the image.  gray: the chip is gray (CC == 1), a
// colour tap goes through the Q14 formula first; swap: chip and source differ in their channel order.
template <int CC>
__device__ __forceinline__ void chip_tap(const ChipImg& im, bool swap, long long x, long long y, uint32_t wgt, uint32_t acc[CC]) {
  if (wgt == 0u || x < 0 || y < 0 || x >= im.width || y >= im.height) return;
  const pack_src_t row = (pack_src_t)im.data + y * im.pitch;
  [[maybe_unused]] const Bc bc_row((long long)(uintptr_t)row, (long long)(uintptr_t)row + (long long)im.width * im.bpp);
  const pack_src_t p = row + x * im.bpp;
  JDA_BC_ADDR(bc_row, p, im.bpp == 1 ? 1 : 3, kBcChipSrc);
  if (im.bpp == 1) {
    const uint32_t g = p[0];
#pragma unroll
    for (int c = 0; c < CC; c++) acc[c] += wgt * g;
    return;
  }
  const uint32_t b0 = p[0], b1 = p[1], b2 = p[2];
  if constexpr (CC == 1) {
    const uint32_t w0 = im.rgb ? kGrayR : kGrayB, w2 = im.rgb ? kGrayB : kGrayR;
    acc[0] += wgt * ((b0 * w0 + b1 * kGrayG + b2 * w2 + 8192u) >> 14);
  } else {
    acc[0] += wgt * (swap ? b2 : b0);
    acc[1] += wgt * b1;
    acc[2] += wgt * (swap ? b0 : b2);
  }
}

// chip pixel (u, v) of a face -> its CC channel values (include/jda.h: the order of every operation)
template <int CC>
__device__ __forceinline__ void chip_pixel(const ChipFace& fc, const ChipImg& im, bool swap, int u, int v, uint32_t out[CC]) {
  uint32_t acc[CC];
#pragma unroll
  for (int c = 0; c < CC; c++) acc[c] = 0u;
  const int n = fc.n;
  const double W = (double)im.width, H = (double)im.height, n2 = (double)(2 * n);
  for (int j = 0; j < n; j++) {
    const double cv = (double)v + (double)((2 * j + 1) - n) / n2;
    for (int i = 0; i < n; i++) {
      const double cu = (double)u + (double)((2 * i + 1) - n) / n2;
      const double sx = (fc.m[0] * cu + fc.m[1] * cv) + fc.m[2];
      const double sy = (fc.m[3] * cu + fc.m[4] * cv) + fc.m[5];
      if (!(sx > -1.0 && sx < W && sy > -1.0 && sy < H)) continue;
      const long long X = (long long)__builtin_floor(sx * 1024.0 + 0.5), Y = (long long)__builtin_floor(sy * 1024.0 + 0.5);
      const long long x0 = X >> 10, y0 = Y >> 10;
      const uint32_t fx = (uint32_t)(X & 1023), fy = (uint32_t)(Y & 1023);
      chip_tap<CC>(im, swap, x0, y0, (1024u - fx) * (1024u - fy), acc);
      chip_tap<CC>(im, swap, x0 + 1, y0, fx * (1024u - fy), acc);
      chip_tap<CC>(im, swap, x0, y0 + 1, (1024u - fx) * fy, acc);
      chip_tap<CC>(im, swap, x0 + 1, y0 + 1, fx * fy, acc);
    }
  }
  const uint32_t nn = (uint32_t)(n * n);
#pragma unroll
  for (int c = 0; c < CC; c++) out[c] = ((acc[c] + nn * (1u << 19)) >> 20) / nn;
}

}  // namespace

__global__ __launch_bounds__(kChipBlock) void k_chips(ChipArgs a) {
  const long long g = (long long)blockIdx.x * kChipBlock + (int)threadIdx.x;
  if (g >= a.nq + a.head + a.tail) return;
  [[maybe_unused]] const Bc bc_dst((long long)(uintptr_t)a.dst, (long long)(uintptr_t)a.dst + a.bytes);
  // the unit's first byte of the call's output and its length
  long long p0; int len;
  pack_unit(g, a.nq, a.head, &p0, &len);
  // ... is byte c0 of pixel (u, v) of face f; a chip is below 2^26 pixels, the call's output below 2^32 bytes divides in 32 bits
  const uint32_t chip_bytes = (uint32_t)a.cw * (uint32_t)a.ch * (uint32_t)a.cbpp;
  const pack_qr fr = pack_divmod(p0, chip_bytes);
  long long f = fr.q; const uint32_t r = fr.r;
  const uint32_t pix = r / (uint32_t)a.cbpp;
  int c0 = (int)(r - pix * (uint32_t)a.cbpp);
  int v = (int)(pix / (uint32_t)a.cw), u = (int)(pix - (uint32_t)v * (uint32_t)a.cw);

  unsigned long long lo = 0ull, hi = 0ull;                         // the unit's bytes 0..7 and 8..15
  long long f_have = -1;
  ChipFace fc{}; ChipImg im{}; bool swap = false;
  for (int k = 0; k < len;) {
    if (f != f_have) {
      if (f >= a.n_faces) {                                        // (bytes = n_faces * chip_bytes: never taken)
#ifdef JDA_BOUNDS_CHECK
        jda_bc_fail(kBcChipDst, __LINE__);
#endif
        return;
      }
      fc = a.faces[f];                                             // (kernel-argument pointers: global_ loads)
      if (fc.image < 0 || fc.image >= a.n_images) {                // (the host made the records: never taken)
#ifdef JDA_BOUNDS_CHECK
        jda_bc_fail(kBcChipSrc, __LINE__);
#endif
        return;
      }
      im = a.imgs[fc.image];
      swap = im.bpp > 1 && (im.rgb != 0) != (a.crgb != 0);
      f_have = f;
    }
    uint32_t px[3] = {0u, 0u, 0u};
    if (a.cbpp == 1) chip_pixel<1>(fc, im, swap, u, v, px);
    else chip_pixel<3>(fc, im, swap, u, v, px);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (c >= c0 && c < a.cbpp && k < len) {
        if (k < 8) lo |= (unsigned long long)px[c] << (8 * k); else hi |= (unsigned long long)px[c] << (8 * (k - 8));
        k++;
      }
    }
    c0 = 0;
    if (++u == a.cw) { u = 0; if (++v == a.ch) { v = 0; f++; } }
  }
  if (len == 16) {
    JDA_BC_ADDR(bc_dst, a.dst + p0, 16, kBcChipDst);
    *(pack_dst16_t)(a.dst + p0) = pack_u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};   // 16-byte aligned: head is dst's distance to its first boundary
  } else {
    JDA_BC_ADDR(bc_dst, a.dst + p0, 1, kBcChipDst);
    ((pack_dst_t)a.dst)[p0] = (uint8_t)lo;
  }
}

hipError_t launch_chips(const ChipArgs& a, hipStream_t stream) {
  if (a.n_faces <= 0 || a.bytes <= 0) return hipSuccess;
  if (!a.faces || !a.imgs || !a.dst || a.n_images <= 0 || a.cw < 1 || a.ch < 1 || (a.cbpp != 1 && a.cbpp != 3)) return hipErrorInvalidValue;
  if (a.head < 0 || a.head > 15 || a.tail < 0 || a.tail > 15 || a.nq < 0 || a.head + (a.nq << 4) + a.tail != a.bytes) return hipErrorInvalidValue;
  if (a.bytes != (long long)a.n_faces * a.cw * a.ch * a.cbpp || (a.nq > 0 && (((uintptr_t)a.dst + (uintptr_t)a.head) & 15) != 0)) return hipErrorInvalidValue;
  const long long total = a.nq + a.head + a.tail;
  const long long groups = (total + kChipBlock - 1) / kChipBlock;
  if (groups > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_chips, dim3((unsigned)groups), dim3(kChipBlock), 0, stream, a);
  return hipGetLastError();
}

JDA_BC_READER(k_chips)

}  // namespace jda
