// The pixel arithmetic k_pack.hip and k_turn.hip share (include/jda.h, "frames as they arrive"): the Q14 gray value of a colour
// pixel as two v_dot4_u32_u8, one pixel by byte loads, the address-space typedefs of the image records' pointers and the
// bounds-check of a run of aligned dwords.  Device code only; every name lives in the including translation unit.
#pragma once
#include "kernels_common.h"

namespace jda {

namespace {

typedef uint32_t pack_u32x4 __attribute__((ext_vector_type(4)));
typedef pack_u32x4 pack_u32x4_a4 __attribute__((aligned(4)));          // four dwords at a dword-aligned address
// (the image records hand out plain pointers; said to be global memory, they are read and written with global_, not flat_, instructions)
typedef const __attribute__((address_space(1))) uint8_t* pack_src_t;
typedef __attribute__((address_space(1))) uint8_t* pack_dst_t;
typedef const __attribute__((address_space(1))) uint32_t* pack_src4_t;
typedef const __attribute__((address_space(1))) pack_u32x4_a4* pack_src16_t;
typedef __attribute__((address_space(1))) pack_u32x4* pack_dst16_t;

#ifdef JDA_BOUNDS_CHECK
// n aligned dwords from p: each must hold a byte of bc (the bytes the rectangle takes of one source row)
#define JDA_BC_PACK_DWORDS(bc, p, n) do { for (int k_ = 0; k_ < (n); k_++) { const long long q_ = (long long)(uintptr_t)(p) + 4 * k_; \
    if (q_ + 4 <= (bc).lo || q_ >= (bc).hi) jda_bc_fail(kBcPackSrc, __LINE__); } } while (0)
#else
#define JDA_BC_PACK_DWORDS(bc, p, n) do { } while (0)
#endif

// the gray value of the pixel in the low bytes of px (weights: PackImg::w_lo / w_hi)
__device__ __forceinline__ uint32_t pack_gray(uint32_t px, uint32_t w_lo, uint32_t w_hi) {
  const uint32_t hi = __builtin_amdgcn_udot4(px, w_hi, 0u, false);
  return __builtin_amdgcn_udot4(px, w_lo, (hi << 8) + 8192u, false) >> 14;
}

// one pixel, byte loads (alpha is not read)
__device__ __forceinline__ uint32_t pack_pixel(pack_src_t p, int bpp, uint32_t w_lo, uint32_t w_hi, const Bc& bc_src) {
  JDA_BC_ADDR(bc_src, p, bpp == 1 ? 1 : 3, kBcPackSrc);
  if (bpp == 1) return p[0];
  return pack_gray((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16), w_lo, w_hi);
}

}  // namespace

}  // namespace jda
