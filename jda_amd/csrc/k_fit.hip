// HIP kernel of dialect CPP's global regression for gfx950 (reference src/jda/btcart.cpp:328-388: one liblinear
// L2R_L2LOSS_SVR_DUAL problem per shape coordinate over the stage's leaf indicators), the fit include/jda.h defines to the
// bit under "a stage's global regression".
//   k_fit   ONE LAUNCH = ONE EPOCH of every coordinate that has not stopped.  Dual coordinate descent is serial over the
//           samples of a problem: the parallelism is the 2L problems -- one wave each, in a workgroup of its own -- and what
//           a wave can do inside one sample.  No barrier, no atomics, no communication between waves, no spin: a wave walks
//           its n_rows samples and ends.
//           state   beta [2L][n_rows], the weights transposed [2L][f] and four words per coordinate (FitState) live in
//                   global memory between launches; a wave whose `done` word is set returns at once, so launches queued
//                   past a coordinate's stop change nothing.  All of it is read AND written by this kernel launch after
//                   launch: it is reached by vector loads and stores only (lane-dependent addresses, agent-scope loads
//                   for the state words), never through the scalar cache.
//           column  the coordinate's column w_j (f doubles) sits in LDS for the epoch (LDS = true), or stays in global
//                   memory where it does not fit (LDS = false: the same body on the same values, the wave's writes ordered
//                   before its next reads by wave_global_sync, kernels_common.h).
//           sample  lanes = carts: lane c gathers w_j[lbf[i][k]] for k = c, c + 64, .. and keeps the values; their sum in
//                   ascending k is the partial sum p[c] of the contract, the six steps h = 32 .. 1 are cross-lane adds in
//                   the contract's pairing (h = 32, 16 through the LDS crossbar, h = 8 .. 1 by DPP row shifts); G, the
//                   violation, d (a true IEEE division) and beta are wave-uniform; the scatter writes value + d back from
//                   the registers the gather filled -- K distinct addresses, one per cart.  A wave's LDS operations
//                   complete in order, so the next sample sees these writes without a fence.
//           loads   index -> row of lbf -> y, beta are dependent loads that do not depend on w: 64 indices are loaded per
//                   wave at a time (lane = position), two batches ahead; the y and beta of a batch are gathered one batch
//                   ahead (within an epoch every sample occurs once, so beta may be read early) and handed out by
//                   v_readlane; the rows of lbf of the next kFitPrefetch samples are in registers.  New betas are collected
//                   in the batch's register (a select on the lane) and stored once per batch.
// fp64 add, multiply, divide only; -ffp-contract=off; no scratch.
#include "kernels_common.h"

namespace jda {

namespace {

// lane c <- lane (c + h) & 63, through the LDS crossbar (no LDS memory is touched)
__device__ __forceinline__ double fit_from_above(double v, int lane, int h) {
  const int at = ((lane + h) & 63) << 2;
  const int lo = __builtin_amdgcn_ds_bpermute(at, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(at, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
// lane c <- lane c + H of the same row of 16 lanes (row_shl:H); a lane with no such lane keeps its own value
template <int H>
__device__ __forceinline__ double fit_row_above(double v) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), 0x100 + H, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), 0x100 + H, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// The contract's six steps on the 64 partial sums: after step h, lanes c < h hold p[c] + p[c + h]; the other lanes hold
// values no later step reads.
__device__ __forceinline__ double fit_reduce(double p, int lane) {
  p = p + fit_from_above(p, lane, 32);
  p = p + fit_from_above(p, lane, 16);
  p = p + fit_row_above<8>(p);
  p = p + fit_row_above<4>(p);
  p = p + fit_row_above<2>(p);
  p = p + fit_row_above<1>(p);
  return rl(p, 0);
}


__device__ __forceinline__ int fit_load_int(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double fit_load_double(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// the row of lbf of sample i as the lanes hold it: lane c's entries k = c, c + 64, ..
template <int NR>
__device__ __forceinline__ void fit_load_row(int (&row)[NR], const int* __restrict__ lbf, int i, int K, int lane) {
  const int* __restrict__ p = lbf + (size_t)i * K;
#pragma unroll
  for (int r = 0; r < NR; r++)                           // (a lane past K holds the row's LAST entry, a valid index it gathers from
    row[r] = p[min(lane + 64 * r, K - 1)];               // and never adds or writes: nothing here waits for the loaded value)
}

// The coordinate-independent part of one sample step: G, the violation and d from y, beta and dot (all wave-uniform).
struct FitStep { double d, violation; };
__device__ __forceinline__ FitStep fit_scalar(double y, double b, double dot, double lambda, double H) {
  double G = -y + lambda * b;
  G = G + dot;
  FitStep o;
  o.violation = b == 0. ? (G < 0. ? -G : (G > 0. ? G : 0.)) : fabs(G);
  const double Hb = H * b;
  o.d = G < Hb ? -G / H : (G > Hb ? -G / H : -b);
  return o;
}

}  // namespace

template <bool LDS, int NR>
__global__ __launch_bounds__(64) void k_fit(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fit_lds[];
  constexpr int PF = kFitPrefetch;
  static_assert(PF == 4, "the sample loop below is written out for four steps per round");
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x;
  FitState* st = a.state + j;
  if (fit_load_int(&st->done) != 0) return;              // this coordinate has stopped (wave-uniform: one word)
  const int n = a.n_rows, K = a.K, f = a.f;
  const double lambda = a.lambda, H = a.H;
  double* wg = a.w + (size_t)j * f;
  double* bj = a.beta + (size_t)j * n;
  const double* __restrict__ yj = a.y + (size_t)j * n;
  const int* __restrict__ index = a.index;
  [[maybe_unused]] const Bc bc_n(0, n), bc_f(0, f);
  double* wl = wg;
  if constexpr (LDS) {
    wl = (double*)fit_lds;
    for (int k = lane; k < f; k += 64) wl[k] = wg[k];
    wave_lds_sync();
  }

  // batch A = the 64 samples being stepped, B = the next 64, C = the 64 after them (indices only)
  int iA = lane < n ? index[lane] : 0;
  int iB = 64 + lane < n ? index[64 + lane] : 0;
  if (lane < n) JDA_BC(bc_n, iA, 1, kBcFitSample);
  if (64 + lane < n) JDA_BC(bc_n, iB, 1, kBcFitSample);
  double yA = 0., bA = 0.;
  if (lane < n) { yA = yj[iA]; bA = bj[iA]; }
  [[maybe_unused]] int rows[PF][NR > 0 ? NR : 1];
  if constexpr (NR > 0) {
#pragma unroll
    for (int u = 0; u < PF; u++) fit_load_row<NR>(rows[u], a.lbf, rl(iA, min(u, n - 1)), K, lane);
  }

  double gnorm = 0.;
  int base = 0;
  double yB = 0., bB = 0.;
  // One sample: position s0 + U of the batch at `base`; its row of lbf is in rows[U].
  auto step = [&](auto U, int s0) __attribute__((always_inline)) {
    constexpr int u = decltype(U)::value;
    const int s = s0 + u;
    const double y = rl(yA, s), b = rl(bA, s);
    if constexpr (NR > 0) {
      int cur[NR];
#pragma unroll
      for (int r = 0; r < NR; r++) cur[r] = rows[u][r];
      // the sample PF steps on takes this one's registers (past the end: this sample's row again, never used) --
      // unconditional, so that the loop carries the loads' own registers and waits for them only where they are used
      const int sp = base + s + PF < n ? s + PF : s;
      fit_load_row<NR>(rows[u], a.lbf, sp < 64 ? rl(iA, sp) : rl(iB, sp - 64), K, lane);
      double v[NR];
      double p = 0.;
#pragma unroll
      for (int r = 0; r < NR; r++) {                     // the gather: all reads in flight together
        JDA_BC(bc_f, cur[r], 1, kBcFitWeight);
        v[r] = wl[cur[r]];
      }
#pragma unroll
      for (int r = 0; r < NR; r++) {
        const double t = p + v[r];
        p = lane + 64 * r < K ? t : p;
      }
      const FitStep o = fit_scalar(y, b, fit_reduce(p, lane), lambda, H);
      gnorm += o.violation;
      if (fabs(o.d) < 1.0e-12) return;
      const double nb = b + o.d;
      const double d = nb - b;
      bA = lane == s ? nb : bA;
      if (d != 0.) {
#pragma unroll
        for (int r = 0; r < NR; r++)
          if (lane + 64 * r < K) wl[cur[r]] = v[r] + d;
        if constexpr (LDS) wave_lds_sync(); else wave_global_sync();
      }
    } else {                                             // K above 64 * kFitMaxRounds: the row is read where it is used
      const int* __restrict__ row = a.lbf + (size_t)rl(iA, s) * K;
      double p = 0.;
      for (int k = lane; k < K; k += 64) {
        const int at = row[k];
        JDA_BC(bc_f, at, 1, kBcFitWeight);
        p = p + wl[at];
      }
      const FitStep o = fit_scalar(y, b, fit_reduce(p, lane), lambda, H);
      gnorm += o.violation;
      if (fabs(o.d) < 1.0e-12) return;
      const double nb = b + o.d;
      const double d = nb - b;
      bA = lane == s ? nb : bA;
      if (d != 0.) {
        for (int k = lane; k < K; k += 64) { const int at = row[k]; wl[at] = wl[at] + d; }
        if constexpr (LDS) wave_lds_sync(); else wave_global_sync();
      }
    }
  };
  for (; base < n; base += 64) {
    const int iC = (long long)base + 128 + lane < n ? index[base + 128 + lane] : 0;
    if ((long long)base + 128 + lane < n) JDA_BC(bc_n, iC, 1, kBcFitSample);
    yB = 0.; bB = 0.;
    if ((long long)base + 64 + lane < n) { yB = yj[iB]; bB = bj[iB]; }
    const int cnt = min(64, n - base);
    int s0 = 0;
    for (; s0 + PF <= cnt; s0 += PF) {                   // whole rounds: straight-line, no test per sample
      step(std::integral_constant<int, 0>{}, s0); step(std::integral_constant<int, 1>{}, s0);
      step(std::integral_constant<int, 2>{}, s0); step(std::integral_constant<int, 3>{}, s0);
    }
    if (s0 < cnt) step(std::integral_constant<int, 0>{}, s0);                 // the set's last samples
    if (s0 + 1 < cnt) step(std::integral_constant<int, 1>{}, s0);
    if (s0 + 2 < cnt) step(std::integral_constant<int, 2>{}, s0);
    if ((long long)base + lane < n) bj[iA] = bA;         // the batch's betas, one store per batch
    iA = iB; yA = yB; bA = bB; iB = iC;
  }

  if constexpr (LDS) {
    wave_lds_sync();
    for (int k = lane; k < f; k += 64) wg[k] = wl[k];
  }
  if (lane == 0) {                                       // the device decides convergence; the host only stops launching
    const int iter = fit_load_int(&st->iters);
    const double init = iter == 0 ? gnorm : fit_load_double(&st->gnorm_init);
    if (iter == 0) st->gnorm_init = gnorm;
    st->gnorm_last = gnorm;
    st->iters = iter + 1;
    if (gnorm <= a.eps * init) st->done = 1;
  }
}

namespace {

// prepare: only what a launch of the chosen instantiation needs set beforehand (dynamic LDS above 48 KB), once per call
template <bool LDS>
hipError_t fit_launch_rounds(const FitArgs& a, int rounds, int lds_bytes, bool prepare, hipStream_t stream) {
  const dim3 grid((unsigned)a.dim), block(64);
#define JDA_FIT_CASE(NR) do { \
    if (prepare) return LDS && lds_bytes > 48 * 1024 ? hipFuncSetAttribute((const void*)k_fit<LDS, NR>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) : hipSuccess; \
    hipLaunchKernelGGL((k_fit<LDS, NR>), grid, block, LDS ? lds_bytes : 0, stream, a); } while (0)
  if (rounds <= 1) JDA_FIT_CASE(1);
  else if (rounds <= 2) JDA_FIT_CASE(2);
  else if (rounds <= 4) JDA_FIT_CASE(4);
  else if (rounds <= 9) JDA_FIT_CASE(9);
  else if (rounds <= kFitMaxRounds) JDA_FIT_CASE(kFitMaxRounds);
  else JDA_FIT_CASE(0);
#undef JDA_FIT_CASE
  return hipGetLastError();
}

hipError_t fit_dispatch(const FitArgs& a, const FitLaunch& how, bool prepare, hipStream_t stream) {
  if (a.n_rows <= 0 || a.dim <= 0) return hipSuccess;
  if (a.K < 1 || a.f < a.K) return hipErrorInvalidValue;
  const int rounds = (a.K + 63) / 64;
  return how.lds ? fit_launch_rounds<true>(a, rounds, how.lds_bytes, prepare, stream) : fit_launch_rounds<false>(a, rounds, 0, prepare, stream);
}

}  // namespace

hipError_t plan_fit(const FitArgs& a, int lds_budget, FitLaunch* how) {
  *how = FitLaunch{0, 0};
  const long long bytes = (((long long)a.f * 8) + 15) & ~15ll;
  if (bytes <= std::min<long long>(std::max(0, lds_budget), 160 * 1024)) *how = FitLaunch{1, (int)bytes};
  return fit_dispatch(a, *how, true, nullptr);
}

hipError_t launch_fit(const FitArgs& a, const FitLaunch& how, hipStream_t stream) { return fit_dispatch(a, how, false, stream); }

JDA_BC_READER(k_fit)

}  // namespace jda
