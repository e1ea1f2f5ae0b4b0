// HIP kernel for gfx950 that moves a dialect-CPP sample set into a new order (reference src/jda/data.cpp:319-410: the
// Swap of _QSort_, Remove and MoreNegSamples exchange or append cv::Mat headers; here a sample is P = o*o + h*h + q*q
// bytes of a dense array that k_train_values and k_lbf read in place, so the bytes move).
//   k_gather  wave = destination record, kGatherWaves records per workgroup and round of a grid-stride loop; everything
//             about a record is wave-uniform and lives in SGPRs.  Record addresses are base + r * P with any base and
//             any P (3 .. 49,152): source and destination are misaligned independently.
//             - the destination decides the shape: head = the bytes up to its first 16-byte boundary (at most 15) and
//               tail = the bytes after its last one (at most 15) are byte stores, one lane each; the middle is
//               16-byte stores, lane = one store, consecutive lanes consecutive addresses (1 KiB per wave instruction);
//             - a store's 16 bytes start at source offset sh = (source address & 3) inside an aligned dword: sh == 0
//               takes four aligned dwords as they are, otherwise five are read and every output dword is funnelled out
//               of two neighbours (v_alignbyte_b32).  Every dword read holds at least one byte of the record, so no
//               read leaves the aligned dwords that the record itself touches (an aligned dword never crosses a page).
//             No LDS, no atomics, no scratch; offsets are 64-bit (2 * 10^5 records of 49,152 B are above 4 GB).
#include "kernels_common.h"

namespace jda {

namespace {

typedef uint32_t gather_u32x4 __attribute__((ext_vector_type(4)));
typedef gather_u32x4 gather_u32x4_a4 __attribute__((aligned(4)));      // four dwords at a dword-aligned address

#ifdef JDA_BOUNDS_CHECK
// n aligned dwords from p: each must hold a byte of bc (the record's segment)
#define JDA_BC_GATHER_DWORDS(bc, p, n) do { for (int k_ = 0; k_ < (n); k_++) { const long long q_ = (long long)(uintptr_t)(p) + 4 * k_; \
    if (q_ + 4 <= (bc).lo || q_ >= (bc).hi) jda_bc_fail(kBcGatherSrc, __LINE__); } } while (0)
#else
#define JDA_BC_GATHER_DWORDS(bc, p, n) do { } while (0)
#endif

}  // namespace

__global__ __launch_bounds__(64 * kGatherWaves) void k_gather(GatherArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long stride = (long long)gridDim.x * kGatherWaves;
  const int P = a.P;
  [[maybe_unused]] const Bc bc_dst((long long)(uintptr_t)a.dst, (long long)(uintptr_t)a.dst + a.dst_n * P);
  for (long long w = (long long)blockIdx.x * kGatherWaves + wave; w < a.n_items; w += stride) {
    const GatherItem it = a.items[w];
    const int di = __builtin_amdgcn_readfirstlane(it.dst), si = __builtin_amdgcn_readfirstlane(it.src);
    // the source record's segment (selects, not an indexed copy of the table: nothing goes to scratch)
    const uint8_t* sbase = nullptr;
    long long sfirst = 0;
    [[maybe_unused]] long long sn = 0;
#pragma unroll
    for (int s = 0; s < kGatherSegs; s++) {
      const bool in = s < a.n_segs && si >= a.seg[s].first && si < a.seg[s].first + a.seg[s].n;
      sbase = in ? a.seg[s].base : sbase; sfirst = in ? a.seg[s].first : sfirst; sn = in ? a.seg[s].n : sn;
    }
    const bool ok = sbase != nullptr && di >= a.dst_first && di < a.dst_first + a.dst_n;
#ifdef JDA_BOUNDS_CHECK
    if (!ok && lane == 0) jda_bc_fail(sbase ? kBcGatherDst : kBcGatherSrc, __LINE__);
#endif
    if (!ok) continue;                                   // (the host validated every index: never taken)
    [[maybe_unused]] const Bc bc_src((long long)(uintptr_t)sbase, (long long)(uintptr_t)sbase + sn * P);
    const uint8_t* __restrict__ s = sbase + (size_t)(si - sfirst) * (size_t)P;
    uint8_t* __restrict__ d = a.dst + (size_t)(di - a.dst_first) * (size_t)P;

    const int head = min(P, (int)((0 - (uintptr_t)d) & 15));
    const int nq = (P - head) >> 4, tail = P - head - (nq << 4);
    if (lane < head) {
      JDA_BC_ADDR(bc_src, s + lane, 1, kBcGatherSrc); JDA_BC_ADDR(bc_dst, d + lane, 1, kBcGatherDst);
      d[lane] = s[lane];
    }
    if (lane < tail) {
      const int o = head + (nq << 4) + lane;
      JDA_BC_ADDR(bc_src, s + o, 1, kBcGatherSrc); JDA_BC_ADDR(bc_dst, d + o, 1, kBcGatherDst);
      d[o] = s[o];
    }
    const int sh = (int)((uintptr_t)(s + head) & 3);
    const uint32_t* __restrict__ s4 = (const uint32_t*)(s + head - sh);       // dword aligned
    gather_u32x4* __restrict__ d16 = (gather_u32x4*)(d + head);               // 16-byte aligned
    if (sh == 0) {
      for (int q = lane; q < nq; q += 64) {
        JDA_BC_GATHER_DWORDS(bc_src, s4 + 4 * q, 4); JDA_BC_ADDR(bc_dst, d16 + q, 16, kBcGatherDst);
        d16[q] = *(const gather_u32x4_a4*)(s4 + 4 * q);
      }
    } else {
      for (int q = lane; q < nq; q += 64) {
        JDA_BC_GATHER_DWORDS(bc_src, s4 + 4 * q, 5); JDA_BC_ADDR(bc_dst, d16 + q, 16, kBcGatherDst);
        const gather_u32x4 v = *(const gather_u32x4_a4*)(s4 + 4 * q);
        const uint32_t e = s4[4 * q + 4];
        gather_u32x4 o;                                  // ({hi, lo} >> 8 sh): the four bytes from offset sh of lo
        o.x = __builtin_amdgcn_alignbyte(v.y, v.x, (uint32_t)sh);
        o.y = __builtin_amdgcn_alignbyte(v.z, v.y, (uint32_t)sh);
        o.z = __builtin_amdgcn_alignbyte(v.w, v.z, (uint32_t)sh);
        o.w = __builtin_amdgcn_alignbyte(e, v.w, (uint32_t)sh);
        d16[q] = o;
      }
    }
  }
}

hipError_t launch_gather(const GatherArgs& a, hipStream_t stream) {
  if (a.n_items <= 0) return hipSuccess;
  if (a.n_segs < 1 || a.n_segs > kGatherSegs || a.P < 3 || a.P > 3 * 128 * 128 || !a.items || !a.dst || a.dst_n < 1) return hipErrorInvalidValue;
  // enough workgroups to fill the device several times over; the rest of the records come round in the grid-stride loop
  const long long groups = std::min<long long>((a.n_items + kGatherWaves - 1) / kGatherWaves, 256 * 16);
  hipLaunchKernelGGL(k_gather, dim3((unsigned)groups), dim3(64 * kGatherWaves), 0, stream, a);
  return hipGetLastError();
}

JDA_BC_READER(k_gather)

}  // namespace jda
