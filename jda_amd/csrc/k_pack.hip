// HIP kernel for gfx950 that turns frames as they arrive -- interleaved BGR / RGB / BGRA / RGBA or 8-bit gray, any row pitch,
// any rectangle -- into the dense 8-bit gray images every detect / validate / mining / positives entry takes (include/jda.h,
// "frames as they arrive"; what the reference's callers do with cvtColor(..., CV_BGR2GRAY) just before the line this library
// replaces: src/live.cpp:32, src/test.cpp:40 and 134, src/jda/data.cpp:621).
//   gray = (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14        integer, OpenCV 2.4's 8-bit form
//   k_pack    ONE launch for a ragged set.  An image's dense output is dealt in units (kernels.h: PackImg), not per row: a
//             48-pixel-wide face crop fills its lanes like a frame does.  lane = unit; a workgroup takes kPackBlock *
//             kPackRounds consecutive units of the launch and finds the image of its first one in block_img (an item per
//             workgroup, made by the host); a lane walks on from there through the image records, whose `first` is the
//             prefix sum of the units.  All offsets are 64-bit.
//             - the destination decides the shape: a unit below nq is the 16 bytes at a 16-byte boundary of dst, one
//               16-byte store; the bytes in front of the first boundary and behind the last are one byte store each;
//             - a 16-byte unit whose pixels lie in one source row reads its 16 * bpp bytes as aligned dwords -- 4 * bpp of
//               them, and one more where the first pixel does not start a dword -- and funnels every dword out of two
//               neighbours by the lane's own shift (v_alignbyte_b32); BGR24 pixels are cut out of the realigned dwords the
//               same way.  Every dword read holds a byte of a pixel of the unit: a source that ends with its allocation is safe;
//             - a unit that straddles source rows (and the single bytes) reads pixel by pixel, byte loads;
//             - the weights are split into their low and high bytes, so a pixel is two v_dot4_u32_u8 on the dword that holds
//               it: the byte that is alpha, or the next pixel's, meets a zero weight.  GRAY8 is the same kernel without it.
//             No LDS, no atomics, no inline assembly, no scratch.
#include "pack_pixel.h"   // pack_row, pack_pixel, pack_unit, pack_divmod, the pack_*_t typedefs: shared with k_turn.hip, k_reduce.hip and k_chips.hip

namespace jda {

__global__ __launch_bounds__(kPackBlock) void k_pack(PackArgs a) {
  const long long base = (long long)blockIdx.x * (kPackBlock * kPackRounds);
  int i = a.block_img[blockIdx.x];
  if (i < 0 || i >= a.n) return;                                   // (the host made the list: never taken)
  PackImg im = a.imgs[i];
  for (int r = 0; r < kPackRounds; r++) {
    const long long g = base + r * kPackBlock + (int)threadIdx.x;
    if (g >= a.total) break;
    while (g >= im.first + im.nq + im.head + im.tail && i + 1 < a.n) im = a.imgs[++i];
    const long long u = g - im.first;
    if (u < 0 || u >= im.nq + im.head + im.tail) {                 // (the prefix sums cover [0, total): never taken)
#ifdef JDA_BOUNDS_CHECK
      jda_bc_fail(kBcPackDst, __LINE__);
#endif
      break;
    }
    const long long npix = (long long)im.w * im.h;
    [[maybe_unused]] const Bc bc_dst((long long)(uintptr_t)im.dst, (long long)(uintptr_t)im.dst + npix);
    [[maybe_unused]] const Bc bc_src((long long)(uintptr_t)im.src, (long long)(uintptr_t)im.src + (long long)(im.h - 1) * im.pitch + (long long)im.w * im.bpp);
    long long p0; int len;
    pack_unit(u, im.nq, im.head, &p0, &len);
    const pack_qr yx = pack_divmod(p0, (uint32_t)im.w);            // the unit's first pixel: row y, column x
    const long long y = yx.q; int x = (int)yx.r;
    if (len == 16) {
      uint32_t q[4] = {0u, 0u, 0u, 0u};
      if (x + 16 <= im.w) {
        const pack_src_t row = (pack_src_t)im.src + y * im.pitch;
        [[maybe_unused]] const Bc bc_row((long long)(uintptr_t)row, (long long)(uintptr_t)row + (long long)im.w * im.bpp);
        const pack_src_t s = row + (long long)x * im.bpp;
        if (im.bpp == 1) pack_row<1, 16>(s, 0u, 0u, bc_row, q);
        else if (im.bpp == 3) pack_row<3, 16>(s, im.w_lo, im.w_hi, bc_row, q);
        else pack_row<4, 16>(s, im.w_lo, im.w_hi, bc_row, q);
      } else {
        pack_src_t row = (pack_src_t)im.src + y * im.pitch;
        pack_src_t s = row + (long long)x * im.bpp;
#pragma unroll
        for (int k = 0; k < 16; k++) {
          q[k >> 2] |= pack_pixel(s, im.bpp, im.w_lo, im.w_hi, bc_src) << (8 * (k & 3));
          s += im.bpp;
          if (++x == im.w) { x = 0; row += im.pitch; s = row; }
        }
      }
      JDA_BC_ADDR(bc_dst, im.dst + p0, 16, kBcPackDst);
      *(pack_dst16_t)(im.dst + p0) = pack_u32x4{q[0], q[1], q[2], q[3]};   // 16-byte aligned: head is dst's distance to its first boundary
    } else {
      const uint32_t v = pack_pixel((pack_src_t)im.src + y * im.pitch + (long long)x * im.bpp, im.bpp, im.w_lo, im.w_hi, bc_src);
      JDA_BC_ADDR(bc_dst, im.dst + p0, 1, kBcPackDst);
      ((pack_dst_t)im.dst)[p0] = (uint8_t)v;
    }
  }
}

hipError_t launch_pack(const PackArgs& a, hipStream_t stream) {
  if (a.n <= 0 || a.total <= 0) return hipSuccess;
  if (!a.imgs || !a.block_img) return hipErrorInvalidValue;
  constexpr long long per = (long long)kPackBlock * kPackRounds;
  const long long groups = (a.total + per - 1) / per;
  if (groups > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pack, dim3((unsigned)groups), dim3(kPackBlock), 0, stream, a);
  return hipGetLastError();
}

JDA_BC_READER(k_pack)

}  // namespace jda
