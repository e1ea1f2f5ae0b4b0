// What k_pack.hip, k_turn.hip, k_reduce.hip, k_rotate.hip and k_chips.hip share (include/jda.h, "frames as they arrive"): the address-space typedefs of the
// records' pointers, the Q14 gray value of a colour pixel as two v_dot4_u32_u8, one pixel by byte loads, a run of pixels of one
// source row by aligned vector loads (pack_row), the bounds-check of such a run, the units a destination is dealt in, and the
// tile kernels' launcher (launch_tiles, the only host code).  Every name lives in the including translation unit.
#pragma once
#include "kernels_common.h"

namespace jda {

namespace {

typedef uint32_t pack_u32x4 __attribute__((ext_vector_type(4)));
typedef pack_u32x4 pack_u32x4_a4 __attribute__((aligned(4)));          // four dwords at a dword-aligned address
typedef uint32_t pack_u32x3 __attribute__((ext_vector_type(3)));
typedef pack_u32x3 pack_u32x3_a4 __attribute__((aligned(4)));          // three
// (the records hand out plain pointers; said to be global memory, they are read and written with global_, not flat_, instructions)
typedef const __attribute__((address_space(1))) uint8_t* pack_src_t;
typedef __attribute__((address_space(1))) uint8_t* pack_dst_t;
typedef const __attribute__((address_space(1))) uint32_t* pack_src4_t;
typedef const __attribute__((address_space(1))) pack_u32x3_a4* pack_src12_t;
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

// NPIX pixels (a multiple of 4) of one source row from a (any alignment) -> their gray bytes, o[NPIX / 4].
// Their NPIX * BPP bytes are read as aligned dwords by the widest loads their number allows -- and one more dword only where
// the first pixel does not start one -- funnelled by the lane's own shift (v_alignbyte_b32); BGR24 pixels are cut out of the
// realigned dwords the same way.  Every dword read holds a byte of a pixel of the run: a source that ends with its allocation
// is safe.
template <int BPP, int NPIX>
__device__ __forceinline__ void pack_row(pack_src_t a, uint32_t w_lo, uint32_t w_hi, const Bc& bc_row, uint32_t* o) {
  constexpr int ND = NPIX * BPP / 4;                               // dwords that NPIX pixels fill
  static_assert(NPIX % 4 == 0 && (ND % 4 == 0 || ND == 3 || ND == 1), "whole dwords, loaded as x4, as one x3 or as one dword");
  const uint32_t sh = (uint32_t)((uintptr_t)a & 3);
  const pack_src4_t s4 = (pack_src4_t)(a - sh);                    // dword aligned
  JDA_BC_PACK_DWORDS(bc_row, s4, sh ? ND + 1 : ND);
  uint32_t d[ND + 1];
  if constexpr (ND % 4 == 0) {
#pragma unroll
    for (int k = 0; k < ND; k += 4) {
      const pack_u32x4 v = *(pack_src16_t)(s4 + k);
      d[k] = v.x; d[k + 1] = v.y; d[k + 2] = v.z; d[k + 3] = v.w;
    }
  } else if constexpr (ND == 3) {
    const pack_u32x3 v = *(pack_src12_t)s4;
    d[0] = v.x; d[1] = v.y; d[2] = v.z;
  } else {
    d[0] = s4[0];
  }
  d[ND] = sh ? s4[ND] : 0u;                                        // (holds a byte of the last pixel only then)
  uint32_t t[ND + 1];                                              // the NPIX * BPP bytes from a on
#pragma unroll
  for (int k = 0; k < ND; k++) t[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
  t[ND] = 0u;
  if constexpr (BPP == 1) {
#pragma unroll
    for (int k = 0; k < ND; k++) o[k] = t[k];
  } else {
#pragma unroll
    for (int k = 0; k < NPIX / 4; k++) o[k] = 0u;
#pragma unroll
    for (int k = 0; k < NPIX; k++) {
      constexpr int B = BPP;
      const int j = (B * k) >> 2, off = (B * k) & 3;               // the pixel's dword and its byte in it (constants once unrolled)
      const uint32_t px = off ? __builtin_amdgcn_alignbyte(t[j + 1], t[j], (uint32_t)off) : t[j];
      o[k >> 2] |= pack_gray(px, w_lo, w_hi) << (8 * (k & 3));
    }
  }
}

// Unit u of a destination dealt as nq runs of 16 bytes from its first 16-byte boundary on, then one unit per byte in front of
// that boundary (head) and behind the last run (kernels.h: PackImg, ChipArgs) -> its first byte *p0 and its length, 16 or 1
__device__ __forceinline__ void pack_unit(long long u, long long nq, int head, long long* p0, int* len) {
  if (u < nq) { *p0 = head + (u << 4); *len = 16; }
  else { const long long e = u - nq; *p0 = e < head ? e : (nq << 4) + e; *len = 1; }   // [0, head): in front, [head, head + tail): behind
}

// p = q * d + r; a p below 2^32 divides in 32 bits
struct pack_qr { long long q; uint32_t r; };
__device__ __forceinline__ pack_qr pack_divmod(long long p, uint32_t d) {
  if (p <= 0xffffffffll) { const uint32_t q = (uint32_t)p / d; return {q, (uint32_t)p - q * d}; }
  const long long q = p / (long long)d;
  return {q, (uint32_t)(p - q * (long long)d)};
}

// Host side, the one launcher of the tile kernels (k_turn, k_reduce, k_rotate): a workgroup per tile
template <auto Kernel, typename Img>
hipError_t launch_tiles(const FrameArgs<Img>& a, hipStream_t stream) {
  if (a.n <= 0 || a.total <= 0) return hipSuccess;
  if (!a.imgs || !a.block_img) return hipErrorInvalidValue;
  if (a.total > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(Kernel, dim3((unsigned)a.total), dim3(kTurnBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

}  // namespace jda
