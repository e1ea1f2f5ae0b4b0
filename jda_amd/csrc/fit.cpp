// libjda.so, host side: a stage's global regression of dialect CPP (jdaGlobalRegressionCpp, jdaFitShuffleCpp; reference
// src/jda/btcart.cpp:328-388 with liblinear's solve_l2r_l1l2_svr as include/jda.h restates it) on the kernel of k_fit.hip.
// The host validates, gathers the used rows of lbf and transposes the used residual columns on upload, then runs the
// epochs: per epoch the serial shuffle on the host, the order into one of fit_ahead + 1 rotating buffers, one launch, and
// an asynchronous copy of the coordinates' state words.  The device decides convergence; the host decides when to stop
// launching, from the copy of epoch e - fit_ahead.
#include <climits>
#include <cmath>

#include "detect.h"
#include "splitmix.h"

namespace jda {

namespace {

struct FitCall {
  Cascador* c;
  const int* lbf; const double* residual;
  int n, K;
  const int* rows; int n_rows;
  const jdaFitParamsCpp* params;
  double* w; int* out_iters; double* out_gnorm1;
  jdaFitStatsCpp* stats;
  int leaf_n, dim;
  long long f;
  double t0;                  // when the call began (call_ms covers the validation too)
};

void shuffle_epoch(int* index, int n, uint64_t seed, int iter) {
  const uint64_t base = splitmix64(seed + ((uint64_t)iter + 1) * kGoldenGamma);
  for (int s = 0; s < n; s++) {
    const uint64_t r = splitmix64(base + ((uint64_t)s + 1) * kGoldenGamma);
    const int t = s + (int)(r % (uint64_t)(n - s));
    std::swap(index[s], index[t]);
  }
}

// Everything that can be refused, before the device is touched.  *empty: nothing to fit (w is zeroed).
bool check_call(FitCall& x, bool* empty) {
  *empty = false;
  Cascador* c = x.c;
  if (!c) { fail("bad arguments"); return false; }
  if (x.K <= 0) { fail("K must be positive"); return false; }
  if (!x.rows) x.n_rows = x.n;                           // NULL: all n rows in order, n_rows is not read
  if (x.n < 0 || x.n_rows < 0) { fail("n and n_rows must not be negative"); return false; }
  if (!x.w) { fail("w must be given"); return false; }
  const int D = c->hm.D;
  if (D < 1 || D > 20) { fail("tree_depth outside [1, 20]"); return false; }
  if (c->hm.L < 1) { fail("the cascador has no landmarks"); return false; }
  x.leaf_n = 1 << (D - 1); x.dim = 2 * c->hm.L;
  x.f = (long long)x.K * x.leaf_n;
  if (x.f > INT_MAX) { fail("K * leafNum does not fit an int index"); return false; }
  if (x.n_rows > (1 << 30)) { fail("n_rows above 2^30"); return false; }
  if (x.n_rows == 0) { *empty = true; return true; }
  if (!x.lbf || !x.residual) { fail("lbf and residual must be given"); return false; }
  const int n = x.n, K = x.K, nr = x.n_rows, dim = x.dim;
  const long long leaf_n = x.leaf_n;
  const int blocks = (nr + 1023) / 1024;
  std::atomic<long long> bad_row{-1}, bad_lbf{-1}, bad_res{-1};
  parallel_for(blocks, [&](int b) {
    const int s1 = std::min(nr, (b + 1) * 1024);
    for (int s = b * 1024; s < s1; s++) {
      const long long i = x.rows ? x.rows[s] : s;
      long long none = -1;
      if (i < 0 || i >= n) { bad_row.compare_exchange_strong(none, s); return; }
      const int* row = x.lbf + (size_t)i * K;
      for (int k = 0; k < K; k++) {
        const long long leaf = (long long)row[k] - (long long)k * leaf_n;
        if (leaf < 0 || leaf >= leaf_n) { bad_lbf.compare_exchange_strong(none, i * K + k); return; }
      }
      const double* res = x.residual + (size_t)i * dim;
      for (int j = 0; j < dim; j++)
        if (!std::isfinite(res[j])) { bad_res.compare_exchange_strong(none, i * dim + j); return; }
    }
  }, blocks < 8);
  if (bad_row.load() >= 0) { fail("rows[" + std::to_string(bad_row.load()) + "] is outside [0, n)"); return false; }
  if (bad_lbf.load() >= 0) {
    const long long at = bad_lbf.load();
    fail("lbf[" + std::to_string(at) + "] is not a leaf of cart " + std::to_string(at % K)); return false;
  }
  if (bad_res.load() >= 0) { fail("residual[" + std::to_string(bad_res.load()) + "] is not finite"); return false; }
  return true;
}

// Events and pinned memory of one call, released on every way out (after the stream has drained: the buffers are the
// targets of asynchronous copies).
struct FitHost {
  hipStream_t st = nullptr;
  std::vector<hipEvent_t> ev;
  HostPinned idx, state;
  ~FitHost() {
    if (st) (void)hipStreamSynchronize(st);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    idx.release(); state.release();
  }
};

bool run_call(FitCall& x) {
  const double t0 = x.t0;
  Cascador* c = x.c;
  const int nr = x.n_rows, K = x.K, dim = x.dim, f = (int)x.f;
  const jdaFitParamsCpp* pr = x.params;
  const double C = pr && pr->C > 0. ? pr->C : 1. / (double)nr;                // btcart.cpp:363
  const double eps = pr && pr->eps > 0. ? pr->eps : 0.0001;                   // btcart.cpp:365
  const int max_iter = pr && pr->max_iter > 0 ? pr->max_iter : 1000;
  const uint64_t seed = pr ? pr->seed : 0;
  const double lambda = 0.5 / C;
  const double H = (double)K + lambda;
  const int ahead = (int)std::min<long long>(64, std::max<long long>(0, c->kn.fit_ahead));
  const int nb = ahead + 1;
  double shuffle_ms = 0, upload_ms = 0, device_ms = 0;

  // everything the call keeps on the device is held against workspace_mb: the used rows of lbf, y and beta, the transposed
  // weights, the state words and the rotating orders (each array starts on a 256-byte boundary)
  const size_t lbf_bytes = (size_t)nr * K * sizeof(int);
  const size_t need = lbf_bytes + 2 * (size_t)dim * nr * sizeof(double) + (size_t)dim * f * sizeof(double) + (size_t)dim * sizeof(FitState) +
                      (size_t)nb * nr * sizeof(int) + 7 * 256;
  const size_t budget = (size_t)std::max<long long>(1, c->kn.workspace_mb) << 20;
  if (need > budget) {
    fail("the problem's device arrays (" + std::to_string((need + (1 << 20) - 1) >> 20) + " MB, " + std::to_string((lbf_bytes + (1 << 20) - 1) >> 20) +
         " MB of them the used rows of lbf) do not fit workspace_mb = " + std::to_string(c->kn.workspace_mb) +
         ": the fit is one serial pass over all of them per epoch, chunks would be uploaded again every epoch");
    return false;
  }

  // the problem as the kernel reads it: the used rows of lbf in order, the used residual columns transposed
  const int* lbf_src = x.lbf;
  std::vector<int> lbf_rows;
  if (x.rows) {
    lbf_rows.resize((size_t)nr * K);
    parallel_for((nr + 1023) / 1024, [&](int b) {
      const int s1 = std::min(nr, (b + 1) * 1024);
      for (int s = b * 1024; s < s1; s++) std::memcpy(&lbf_rows[(size_t)s * K], x.lbf + (size_t)x.rows[s] * K, (size_t)K * sizeof(int));
    }, nr < 8192);
    lbf_src = lbf_rows.data();
  }
  std::vector<double> y_t((size_t)dim * nr);
  parallel_for(dim, [&](int j) {
    double* out = &y_t[(size_t)j * nr];
    for (int s = 0; s < nr; s++) out[s] = x.residual[(size_t)(x.rows ? x.rows[s] : s) * dim + j];
  }, (long long)dim * nr < 65536);

  OneLane one(c);
  if (!one.open()) return false;
  FitHost h;
  h.st = one.stream;
  hipStream_t st = one.stream;

  CallBuf buf;
  int* d_lbf; double* d_y; double* d_beta; double* d_w; FitState* d_state; int* d_index;
  if (!carve_into(buf, [&](Carver& cv) {
        d_lbf = cv.take<int>((size_t)nr * K);
        d_y = cv.take<double>((size_t)dim * nr);
        d_beta = cv.take<double>((size_t)dim * nr);
        d_w = cv.take<double>((size_t)dim * f);
        d_state = cv.take<FitState>((size_t)dim);
        d_index = cv.take<int>((size_t)nb * nr);
      })) return false;
  if (!h.idx.reserve((size_t)nb * nr * sizeof(int)) || !h.state.reserve((size_t)nb * dim * sizeof(FitState))) return false;
  int* p_idx = (int*)h.idx.p;
  FitState* p_state = (FitState*)h.state.p;
  h.ev.assign((size_t)3 * nb, nullptr);                                       // per buffer: launch begin, launch end, state copied
  for (int b = 0; b < nb; b++) {
    JDA_HIP(hipEventCreate(&h.ev[3 * b])); JDA_HIP(hipEventCreate(&h.ev[3 * b + 1]));
    JDA_HIP(hipEventCreateWithFlags(&h.ev[3 * b + 2], hipEventDisableTiming));
  }

  double t = now_ms();
  JDA_HIP(hipMemcpyAsync(d_lbf, lbf_src, lbf_bytes, hipMemcpyHostToDevice, st));
  JDA_HIP(hipMemcpyAsync(d_y, y_t.data(), y_t.size() * sizeof(double), hipMemcpyHostToDevice, st));
  JDA_HIP(hipMemsetAsync(d_beta, 0, (size_t)dim * nr * sizeof(double), st));
  JDA_HIP(hipMemsetAsync(d_w, 0, (size_t)dim * f * sizeof(double), st));
  JDA_HIP(hipMemsetAsync(d_state, 0, (size_t)dim * sizeof(FitState), st));
  JDA_HIP(hipStreamSynchronize(st));
  upload_ms += now_ms() - t;

  const long long lds_kb = std::min<long long>(160, std::max<long long>(0, c->kn.fit_lds_kb));
  const long long col_bytes = (long long)f * 8;
  // LDS is handed out in granules: the column fits where its granules fit the option's, and the CU's
  const long long granules = (col_bytes + kLdsGranule - 1) / kLdsGranule;
  const bool fits = granules <= lds_kb * 1024 / kLdsGranule && lds_wgs_per_cu(col_bytes) >= 1;
  const int lds_budget = fits ? 160 * 1024 : 0;

  FitArgs a{};
  a.lbf = d_lbf; a.y = d_y; a.beta = d_beta; a.w = d_w; a.state = d_state;
  a.n_rows = nr; a.K = K; a.f = f; a.dim = dim; a.lambda = lambda; a.H = H; a.eps = eps;
  FitLaunch how{0, 0};
  JDA_HIP(plan_fit(a, lds_budget, &how));
  std::vector<int> index((size_t)nr);
  std::iota(index.begin(), index.end(), 0);
  int launched = 0, collected = 0;
  bool all_done = false;
  // the state copy of epoch q has landed: its launch's time, and whether every coordinate has stopped
  auto collect = [&](int q) -> bool {
    const int b = q % nb;
    JDA_HIP(hipEventSynchronize(h.ev[3 * b + 2]));
    float ms = 0;
    JDA_HIP(hipEventElapsedTime(&ms, h.ev[3 * b], h.ev[3 * b + 1]));
    device_ms += ms;
    const FitState* s = p_state + (size_t)b * dim;
    bool done = true;
    for (int j = 0; j < dim; j++) done = done && s[j].done != 0;
    all_done = done;
    return true;
  };
  for (int e = 0; e < max_iter && !all_done; e++) {
    t = now_ms();
    shuffle_epoch(index.data(), nr, seed, e);
    shuffle_ms += now_ms() - t;
    const int b = e % nb;                                                     // (its last user, epoch e - nb, has been collected)
    t = now_ms();
    std::memcpy(p_idx + (size_t)b * nr, index.data(), (size_t)nr * sizeof(int));
    a.index = d_index + (size_t)b * nr;
    JDA_HIP(hipMemcpyAsync(d_index + (size_t)b * nr, p_idx + (size_t)b * nr, (size_t)nr * sizeof(int), hipMemcpyHostToDevice, st));
    upload_ms += now_ms() - t;
    JDA_HIP(hipEventRecord(h.ev[3 * b], st));
    JDA_HIP(launch_fit(a, how, st));
    JDA_HIP(hipEventRecord(h.ev[3 * b + 1], st));
    JDA_HIP(hipMemcpyAsync(p_state + (size_t)b * dim, d_state, (size_t)dim * sizeof(FitState), hipMemcpyDeviceToHost, st));
    JDA_HIP(hipEventRecord(h.ev[3 * b + 2], st));
    launched++;
    if (e >= ahead) { if (!collect(collected)) return false; collected++; }
  }
  while (collected < launched) { if (!collect(collected)) return false; collected++; }

  // results: the last state copy is the final state (launches past a coordinate's stop are no-ops)
  std::vector<double> w_t((size_t)dim * f);
  JDA_HIP(hipMemcpyAsync(w_t.data(), d_w, w_t.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  JDA_HIP(hipStreamSynchronize(st));
  const FitState* fin = p_state + (size_t)((launched - 1) % nb) * dim;
  parallel_for((f + 4095) / 4096, [&](int b) {
    const int k1 = std::min(f, (b + 1) * 4096);
    for (int k = b * 4096; k < k1; k++)
      for (int j = 0; j < dim; j++) x.w[(size_t)k * dim + j] = w_t[(size_t)j * f + k];
  }, (long long)dim * f < 65536);
  for (int j = 0; j < dim; j++) {
    if (x.out_iters) x.out_iters[j] = fin[j].iters;
    if (x.out_gnorm1) { x.out_gnorm1[j] = fin[j].gnorm_init; x.out_gnorm1[dim + j] = fin[j].gnorm_last; }
  }
  if (x.stats) {
    jdaFitStatsCpp& o = *x.stats;
    o.call_ms = now_ms() - t0; o.shuffle_ms = shuffle_ms; o.upload_ms = upload_ms; o.device_ms = device_ms;
    o.epochs_launched = launched; o.lds_path = how.lds; o.lds_bytes = how.lds_bytes;
  }
  return true;
}

}  // namespace

int fit_entry(void* cascador, const int* lbf, const double* residual, int n, int K, const int* rows, int n_rows,
              const jdaFitParamsCpp* params, double* w, int* out_iters, double* out_gnorm1, jdaFitStatsCpp* stats) {
  if (stats) std::memset(stats, 0, sizeof *stats);
  FitCall x{(Cascador*)cascador, lbf, residual, n, K, rows, n_rows, params, w, out_iters, out_gnorm1, stats, 0, 0, 0, now_ms()};
  bool empty = false;
  if (!check_call(x, &empty)) return -1;
  if (empty) {
    std::fill(w, w + (size_t)x.f * x.dim, 0.);
    if (out_iters) std::fill(out_iters, out_iters + x.dim, 0);
    if (out_gnorm1) std::fill(out_gnorm1, out_gnorm1 + 2 * (size_t)x.dim, 0.);
    return 0;
  }
  return run_call(x) ? 0 : -1;
}

int fit_shuffle(int* index, int n, uint64_t seed, int iter) {
  if (n < 0 || iter < 0 || (n > 0 && !index)) { fail("bad arguments"); return -1; }
  shuffle_epoch(index, n, seed, iter);
  return 0;
}

}  // namespace jda
