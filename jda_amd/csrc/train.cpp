// libjda.so, host side: training one CART of dialect CPP (jdaCalcFeatureValuesCpp, jdaSplitNodeCpp, jdaTrainCartCpp,
// jdaGenFeaturePoolCpp; reference src/jda/cart.cpp:41-390, data.cpp:148-173) on the kernels of k_train.hip.
// The device evaluates the pool on the samples and makes the ordered sums; everything that calls log() -- the entropy
// sweep of cart.cpp:210-238 and the leaf scores of cart.cpp:63-89 -- runs here on the host C library, because the
// device's fp64 log is another function and a last-bit difference flips a strict `<`.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "detect.h"
#include "splitmix.h"

namespace jda {

// (declared in detect.h: stage.cpp checks its sample sets and carts the same way)
bool check_set(const jdaSamplesCpp* s, const char* name, bool need_weights) {
  if (!s) { fail(std::string(name) + ": null sample set"); return false; }
  if (s->n < 0) { fail(std::string(name) + ": negative n"); return false; }
  if (s->n > 0 && (!s->patches || !s->shapes || (need_weights && !s->weights))) {
    fail(std::string(name) + ": patches, shapes and weights must be given for a non-empty set"); return false;
  }
  return true;
}

bool check_pool(const jdaFeatureCpp* pool, size_t count, int L) {
  for (size_t i = 0; i < count; i++) {
    const jdaFeatureCpp& f = pool[i];
    if (f.scale < 0 || f.scale > 2) { fail("feature " + std::to_string(i) + ": scale must be 0, 1 or 2"); return false; }
    if (f.landmark_id1 < 0 || f.landmark_id1 >= L || f.landmark_id2 < 0 || f.landmark_id2 >= L) {
      fail("feature " + std::to_string(i) + ": landmark id outside [0, " + std::to_string(L) + ")"); return false;
    }
  }
  return true;
}

namespace {

static_assert(sizeof(TrainFeat) == sizeof(jdaFeatureCpp), "TrainFeat is jdaFeatureCpp's layout");

constexpr double kEsp = 2.2e-16;          // Config::esp, common.cpp:143

// A caller's sample set on the device.
struct DevSet {
  TrainSet ts{};
  const double* weights = nullptr;        // device
  const double* residual = nullptr;
  const uint8_t* has_gt = nullptr;
  const jdaSamplesCpp* host = nullptr;
  CallBuf buf;
};

// mean != nullptr (train_similarity): the cascador's mean shape [2L] -- every sample's stp_mc = STParameter::Calc(its shape,
// mean), DataSet::CalcSTParameters (data.cpp:131-146), is made after the transpose (k_stp) and the values kernel applies it.
bool upload_set(const jdaSamplesCpp* s, int L, int os, int hs, int qs, DevSet* d, hipStream_t st, const double* mean = nullptr) {
  d->host = s;
  const size_t n = (size_t)s->n, dim = 2 * (size_t)L, pt = (size_t)os * os + (size_t)hs * hs + (size_t)qs * qs;
  d->ts.n = s->n; d->ts.os = os; d->ts.hs = hs; d->ts.qs = qs;
  if (n == 0) return true;
  uint8_t* pa; double* raw; double* tr; double* w; double* res; uint8_t* gt;
  double* ms = nullptr; double* stp = nullptr;
  if (!carve_into(d->buf, [&](Carver& cv) {
        if (mean) { ms = cv.take<double>(4 + 2 * dim); stp = cv.take<double>(5 * n); }
        pa = s->patches_on_device ? nullptr : cv.take<uint8_t>(n * pt);
        raw = cv.take<double>(n * dim); tr = cv.take<double>(n * dim);
        w = s->weights ? cv.take<double>(n) : nullptr;
        res = s->residual ? cv.take<double>(2 * n) : nullptr;
        gt = s->has_gt ? cv.take<uint8_t>(n) : nullptr;
      })) return false;
  if (pa) JDA_HIP(hipMemcpyAsync(pa, s->patches, n * pt, hipMemcpyHostToDevice, st));
  JDA_HIP(hipMemcpyAsync(raw, s->shapes, n * dim * sizeof(double), hipMemcpyHostToDevice, st));
  if (w) JDA_HIP(hipMemcpyAsync(w, s->weights, n * sizeof(double), hipMemcpyHostToDevice, st));
  if (res) JDA_HIP(hipMemcpyAsync(res, s->residual, 2 * n * sizeof(double), hipMemcpyHostToDevice, st));
  if (gt) JDA_HIP(hipMemcpyAsync(gt, s->has_gt, n, hipMemcpyHostToDevice, st));
  JDA_HIP(launch_train_transpose(raw, s->n, (int)dim, tr, st));
  if (mean) {                             // (ms: the mean shape as stored at [4 + dim, 4 + 2 dim), its side of Calc in front)
    JDA_HIP(hipMemcpyAsync(ms + 4 + dim, mean, dim * sizeof(double), hipMemcpyHostToDevice, st));
    JDA_HIP(launch_stp(tr, s->n, L, ms + 4 + dim, ms, stp, nullptr, st));
  }
  JDA_HIP(hipStreamSynchronize(st));      // (the host arrays are the caller's: done with them before anything else)
  d->ts.patches = pa ? pa : s->patches;
  d->ts.shapes_t = tr; d->ts.stp = stp; d->weights = w; d->residual = res; d->has_gt = gt;
  return true;
}

// ---- the two host-side criteria ---------------------------------------------------------------------------------------

inline bool is_zero(double v) { return std::abs(v) < 1e-9; }                 // cart.cpp:18-21

inline double calc_entropy(double p) {                                        // cart.cpp:169-174
  if (is_zero(p) || is_zero(1. - p)) return 0;
  volatile double two = 2.;                 // (the C library's log at run time, never a compile-time constant)
  double entropy = -(p) * std::log(p) - (1. - p) * std::log(1. - p);
  entropy /= std::log(two);
  return entropy;
}

// cart.cpp:210-240 for one feature, from its four histograms and the two totals (both summed in sample order).
void sweep_entropy(const double* wp, const double* wn, const int* p_n, const int* n_n, double wp_r, double wn_r, int pos_n,
                   int neg_n, double* es, int* ths) {
  double wp_l = 0, wn_l = 0;
  int current_p = 0, current_n = 0;
  const double w = wp_r + wn_r;
  int threshold_ = -256;
  double entropy = calc_entropy(wp_r / w);
  for (int th = -255; th <= 255; th++) {
    const int idx = th + 255;
    wp_l += wp[idx]; wn_l += wn[idx];
    wp_r -= wp[idx]; wn_r -= wn[idx];
    current_p += p_n[idx]; current_n += n_n[idx];
    const double p_ratio = double(current_p) / pos_n;
    const double n_ratio = double(current_n) / neg_n;
    if (p_ratio < 0.1 || p_ratio > 0.9) continue;
    if (n_ratio < 0.1 || n_ratio > 0.9) continue;
    const double w_l = wp_l + wn_l, w_r = wp_r + wn_r;
    const double e = (w_l / w) * calc_entropy(wp_l / w_l) + (w_r / w) * calc_entropy(wp_r / w_r);
    if (e < entropy) { entropy = e; threshold_ = th; }
  }
  *es = entropy; *ths = threshold_;
}

// calcVariance (cart.cpp:259-266) from the ordered sums: cv::mean as sum * (1. / n) -- the form recalled from OpenCV's
// mean.cpp, unchecked (include/jda.h).
inline double variance_of(double s1, double s2, int n) {
  if (n == 0) return 0.;
  const double inv = 1. / (double)n;
  const double m1 = s1 * inv, m2 = s2 * inv;
  return m2 - m1 * m1;
}

// ---- one call's device state --------------------------------------------------------------------------------------------

struct Ctx {
  Cascador* c;
  OneLane one;
  hipStream_t st = nullptr;
  int L = 0;
  DevSet pos, neg;
  CallBuf work;
  int F = 0, Fc = 0;
  size_t stride_p = 0, stride_n = 0;
  TrainFeat* d_pool = nullptr; int* d_list_p = nullptr; int* d_list_n = nullptr; int* d_kidx = nullptr; TrainVar* d_var = nullptr;
  short* d_vals_p = nullptr; short* d_vals_n = nullptr;
  double* d_hw_p = nullptr; double* d_hw_n = nullptr; int* d_hc_p = nullptr; int* d_hc_n = nullptr;
  std::vector<double> hw_p, hw_n;
  std::vector<int> hc_p, hc_n, kidx;
  std::vector<TrainVar> var;
  std::vector<TrainFeat> pool;
  std::vector<short> row;
  double device_ms = 0, sweep_ms = 0, partition_ms = 0;
  long long evals = 0;
  int chunks = 0;

  explicit Ctx(Cascador* c_) : c(c_), one(c_) {}

  // The call's lane, both sample sets on the device (neg may be empty) and the workspace for pools of F features.
  bool open(const jdaSamplesCpp* p, const jdaSamplesCpp* n, int os, int hs, int qs, int F_) {
    if (!one.open()) return false;
    st = one.stream; L = c->hm.L;
    const double* mean = train_similarity(c) ? c->hm.mean_shape.data() : nullptr;
    return upload_set(p, L, os, hs, qs, &pos, st, mean) && upload_set(n, L, os, hs, qs, &neg, st, mean) && reserve(F_);
  }

  void carve(Carver& cv) {
    const size_t np = (size_t)pos.ts.n, nn = (size_t)neg.ts.n;
    d_pool = cv.take<TrainFeat>(F); d_list_p = cv.take<int>(std::max<size_t>(np, 1)); d_list_n = cv.take<int>(std::max<size_t>(nn, 1));
    d_kidx = cv.take<int>(F); d_var = cv.take<TrainVar>(Fc);
    d_vals_p = cv.take<short>((size_t)Fc * stride_p); d_vals_n = cv.take<short>((size_t)Fc * stride_n);
    d_hw_p = cv.take<double>((size_t)Fc * kTrainBins); d_hw_n = cv.take<double>((size_t)Fc * kTrainBins);
    d_hc_p = cv.take<int>((size_t)Fc * kTrainBins); d_hc_n = cv.take<int>((size_t)Fc * kTrainBins);
  }

  // Workspace for pools of F features: the value matrices and histograms of one feature chunk within workspace_mb.
  bool reserve(int F_) {
    F = F_;
    const size_t np = (size_t)pos.ts.n, nn = (size_t)neg.ts.n;
    stride_p = std::max<size_t>(8, (np + 7) & ~(size_t)7); stride_n = std::max<size_t>(8, (nn + 7) & ~(size_t)7);
    const size_t budget = (size_t)std::max<long long>(1, c->kn.workspace_mb) << 20;
    const size_t fixed = (size_t)F * (sizeof(TrainFeat) + 4) + (np + nn) * 4 + 4096;
    const size_t per = (stride_p + stride_n) * 2 + 2 * (size_t)kTrainBins * 12 + sizeof(TrainVar) + 1024;
    const size_t room = budget / 2 > fixed ? budget / 2 - fixed : 0;
    Fc = (int)std::max<size_t>(1, std::min<size_t>((size_t)F, room / per));
    if (!carve_into(work, [&](Carver& cv) { carve(cv); })) return false;
    hw_p.resize((size_t)Fc * kTrainBins); hw_n.resize((size_t)Fc * kTrainBins);
    hc_p.resize((size_t)Fc * kTrainBins); hc_n.resize((size_t)Fc * kTrainBins);
    var.resize(Fc); kidx.resize(F); pool.resize(F);
    return true;
  }

  bool upload_pool(const jdaFeatureCpp* p) {
    std::memcpy(pool.data(), p, (size_t)F * sizeof(TrainFeat));
    for (TrainFeat& f : pool) f.pad = 0;
    JDA_HIP(hipMemcpyAsync(d_pool, pool.data(), (size_t)F * sizeof(TrainFeat), hipMemcpyHostToDevice, st));
    return true;
  }
};

// ---- SplitNode's choice (cart.cpp:99-115, 176-350) over the lists pl / nl (ascending sample indices) --------------------

// Copies one chunk's device buffers into the caller's jdaSplitSumsCpp (jdaSplitNodeSumsCpp): features [f0, f0 + fc), after the
// chunk's hipStreamSynchronize.  The histograms of mode 1 and the TrainVar rows are already on the host by then; the value
// matrices (and mode 0's count histogram) are fetched here.
bool sink_chunk(Ctx& x, jdaSplitSumsCpp* k, int mode, int f0, int fc, int pos_n, int neg_n) {
  const size_t hb = (size_t)fc * kTrainBins, ho = (size_t)f0 * kTrainBins;
  auto values = [&](const short* dev, size_t stride, int count, short* out) -> bool {
    if (!out || !count) return true;
    x.row.resize((size_t)fc * stride);
    JDA_HIP(hipMemcpyAsync(x.row.data(), dev, (size_t)fc * stride * sizeof(short), hipMemcpyDeviceToHost, x.st));
    JDA_HIP(hipStreamSynchronize(x.st));
    for (int i = 0; i < fc; i++)
      std::memcpy(out + (size_t)(f0 + i) * count, x.row.data() + (size_t)i * stride, (size_t)count * sizeof(short));
    return true;
  };
  if (!values(x.d_vals_p, x.stride_p, pos_n, k->pos_values)) return false;
  if (mode == 1) {
    if (!values(x.d_vals_n, x.stride_n, neg_n, k->neg_values)) return false;
    if (k->pos_hist_w) std::memcpy(k->pos_hist_w + ho, x.hw_p.data(), hb * sizeof(double));
    if (k->neg_hist_w) std::memcpy(k->neg_hist_w + ho, x.hw_n.data(), hb * sizeof(double));
    if (k->pos_hist_c) std::memcpy(k->pos_hist_c + ho, x.hc_p.data(), hb * sizeof(int));
    if (k->neg_hist_c) std::memcpy(k->neg_hist_c + ho, x.hc_n.data(), hb * sizeof(int));
  } else {
    if (k->pos_hist_c) {
      JDA_HIP(hipMemcpyAsync(k->pos_hist_c + ho, x.d_hc_p, hb * sizeof(int), hipMemcpyDeviceToHost, x.st));
      JDA_HIP(hipStreamSynchronize(x.st));
    }
    for (int i = 0; i < fc; i++) {
      const TrainVar& v = x.var[i];
      if (k->var_sums) std::memcpy(k->var_sums + 8 * (size_t)(f0 + i), v.s, sizeof v.s);
      if (k->var_n_left) k->var_n_left[f0 + i] = v.n_left;
      if (k->var_n_right) k->var_n_right[f0 + i] = v.n_right;
      if (k->var_th) k->var_th[f0 + i] = v.th;
    }
  }
  return true;
}

// sink != nullptr: every chunk's raw device outputs are copied out as well (sink_chunk).
bool split_node(Ctx& x, const std::vector<int>& pl, const std::vector<int>& nl, const jdaFeatureCpp* pool, int mode, const double* u,
                int* feature_idx, int* threshold, double* best, double* criterion, int* thresholds, jdaSplitSumsCpp* sink = nullptr) {
  const int F = x.F, pos_n = (int)pl.size(), neg_n = (int)nl.size();
  std::vector<double> es(F, 0.);
  std::vector<int> ths(F, -256);
  *feature_idx = 0; *threshold = -256; *best = 0.;
  auto finish = [&]() {
    if (criterion) std::memcpy(criterion, es.data(), (size_t)F * sizeof(double));
    if (thresholds) std::memcpy(thresholds, ths.data(), (size_t)F * sizeof(int));
  };
  if (mode == 0 && pos_n == 0) { finish(); return true; }                   // cart.cpp:299-301
  const double* hwp = x.pos.host->weights; const double* hwn = x.neg.host->weights;
  double wp_tot = 0, wn_tot = 0;
  if (mode == 1) {                                                            // wp_r / wn_r, cart.cpp:199-208: sample order
    for (int j = 0; j < pos_n; j++) wp_tot += hwp[pl[j]];
    for (int j = 0; j < neg_n; j++) wn_tot += hwn[nl[j]];
  } else {
    if (!x.pos.residual) { fail("a regression split needs pos->residual"); return false; }
    if (!u) { fail("a regression split needs one u per pool feature"); return false; }
    for (int f = 0; f < F; f++) {
      if (!(u[f] >= 0.) || !(u[f] < 1.)) { fail("u must lie in [0, 1) (the reference draws it from [0.1, 0.9))"); return false; }
      x.kidx[f] = std::min(pos_n - 1, (int)((double)pos_n * u[f]));           // int(pos_n*rng.uniform(0.1, 0.9)), cart.cpp:320
    }
    JDA_HIP(hipMemcpyAsync(x.d_kidx, x.kidx.data(), (size_t)F * sizeof(int), hipMemcpyHostToDevice, x.st));
  }
  if (!x.upload_pool(pool)) return false;
  if (pos_n) JDA_HIP(hipMemcpyAsync(x.d_list_p, pl.data(), (size_t)pos_n * sizeof(int), hipMemcpyHostToDevice, x.st));
  if (neg_n && mode == 1) JDA_HIP(hipMemcpyAsync(x.d_list_n, nl.data(), (size_t)neg_n * sizeof(int), hipMemcpyHostToDevice, x.st));
  for (int f0 = 0; f0 < F; f0 += x.Fc) {
    const int fc = std::min(x.Fc, F - f0);
    const size_t hb = (size_t)fc * kTrainBins;
    const double t0 = now_ms();
    JDA_HIP(launch_train_values(x.pos.ts, x.d_list_p, pos_n, x.d_pool + f0, fc, x.d_vals_p, x.stride_p, x.st));
    x.evals += (long long)fc * pos_n;
    if (mode == 1) {
      JDA_HIP(launch_train_values(x.neg.ts, x.d_list_n, neg_n, x.d_pool + f0, fc, x.d_vals_n, x.stride_n, x.st));
      x.evals += (long long)fc * neg_n;
      JDA_HIP(launch_train_hist(x.d_vals_p, x.stride_p, fc, x.d_list_p, pos_n, x.pos.weights ? x.pos.weights : x.d_hw_p, x.d_hw_p, x.d_hc_p, x.st));
      JDA_HIP(launch_train_hist(x.d_vals_n, x.stride_n, fc, x.d_list_n, neg_n, x.neg.weights ? x.neg.weights : x.d_hw_n, x.d_hw_n, x.d_hc_n, x.st));
      JDA_HIP(hipMemcpyAsync(x.hw_p.data(), x.d_hw_p, hb * sizeof(double), hipMemcpyDeviceToHost, x.st));
      JDA_HIP(hipMemcpyAsync(x.hw_n.data(), x.d_hw_n, hb * sizeof(double), hipMemcpyDeviceToHost, x.st));
      JDA_HIP(hipMemcpyAsync(x.hc_p.data(), x.d_hc_p, hb * sizeof(int), hipMemcpyDeviceToHost, x.st));
      JDA_HIP(hipMemcpyAsync(x.hc_n.data(), x.d_hc_n, hb * sizeof(int), hipMemcpyDeviceToHost, x.st));
      JDA_HIP(hipStreamSynchronize(x.st));
      const double t1 = now_ms();
      parallel_for(fc, [&](int i) {
        const size_t o = (size_t)i * kTrainBins;
        sweep_entropy(x.hw_p.data() + o, x.hw_n.data() + o, x.hc_p.data() + o, x.hc_n.data() + o, wp_tot, wn_tot, pos_n, neg_n,
                      &es[f0 + i], &ths[f0 + i]);
      });
      x.device_ms += t1 - t0; x.sweep_ms += now_ms() - t1;
    } else {
      JDA_HIP(launch_train_hist(x.d_vals_p, x.stride_p, fc, x.d_list_p, pos_n, nullptr, x.d_hw_p, x.d_hc_p, x.st));
      JDA_HIP(launch_train_var(x.d_vals_p, x.stride_p, fc, x.d_list_p, pos_n, x.pos.residual, x.pos.has_gt, x.d_hc_p, x.d_kidx + f0,
                               x.d_var, x.st));
      JDA_HIP(hipMemcpyAsync(x.var.data(), x.d_var, (size_t)fc * sizeof(TrainVar), hipMemcpyDeviceToHost, x.st));
      JDA_HIP(hipStreamSynchronize(x.st));
      const double t1 = now_ms();
      for (int i = 0; i < fc; i++) {                                          // cart.cpp:335-338
        const TrainVar& v = x.var[i];
        es[f0 + i] = (variance_of(v.s[0], v.s[1], v.n_left) + variance_of(v.s[2], v.s[3], v.n_left)) * (double)v.n_left +
                     (variance_of(v.s[4], v.s[5], v.n_right) + variance_of(v.s[6], v.s[7], v.n_right)) * (double)v.n_right;
        ths[f0 + i] = v.th;
      }
      x.device_ms += t1 - t0; x.sweep_ms += now_ms() - t1;
    }
    if (sink && !sink_chunk(x, sink, mode, f0, fc, pos_n, neg_n)) return false;
    x.chunks++;
  }
  double mn = std::numeric_limits<double>::max();                              // cart.cpp:243-250, 341-348
  for (int i = 0; i < F; i++)
    if (es[i] < mn) { mn = es[i]; *threshold = ths[i]; *feature_idx = i; }
  *best = es[*feature_idx];
  finish();
  return true;
}

// Values of ONE pool feature on a list -> host (the partition of cart.cpp:120-150).
bool feature_row(Ctx& x, const DevSet& set, const int* d_list, int count, int f, short* d_vals, std::vector<short>* out) {
  out->resize(count);
  if (!count) return true;
  JDA_HIP(launch_train_values(set.ts, d_list, count, x.d_pool + f, 1, d_vals, (size_t)((count + 7) & ~7), x.st));
  JDA_HIP(hipMemcpyAsync(out->data(), d_vals, (size_t)count * sizeof(short), hipMemcpyDeviceToHost, x.st));
  JDA_HIP(hipStreamSynchronize(x.st));
  x.evals += count;
  return true;
}

bool begin(Cascador* c, int os, int hs, int qs, const char* fn) {
  if (!c) { fail("bad arguments"); return false; }
  if (!check_patch_sizes(os, hs, qs)) return false;
  if (c->similarity && !c->kn.train_similarity) {                            // (refused unless the caller opted in: include/jda.h)
    fail(std::string(fn) + ": refused with jdaSetSimilarityTransform(1): the reference's CalcFeatureValues indexes the per-sample "
         "transform by the feature index (data.cpp:168), there is no behaviour to reproduce");
    return false;
  }
  return true;
}

// counter-based draws of jdaGenFeaturePoolCpp (include/jda.h): draw d = 1, 2, ... of feature i under (seed, key)
struct PoolRng {
  uint64_t base, d = 0;
  PoolRng(uint64_t seed, uint64_t key, uint64_t feature) : base(splitmix_draw(splitmix_draw(seed, key), feature)) {}
  uint64_t next() { return splitmix_draw(base, d++); }
  double unit() { return splitmix_unit(next()); }
  double uniform(double a, double b) { return a + (b - a) * unit(); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

}  // namespace
}  // namespace jda

using namespace jda;

extern "C" {

int jdaGenFeaturePoolCpp(int F, int landmark_n, double radius, int multi_scale, uint64_t seed, uint64_t key,
                         jdaFeatureCpp* out_features, double* out_u) try {
  g_err.clear();
  if (F < 0 || landmark_n < 1 || !std::isfinite(radius) || (F > 0 && !out_features)) { fail("bad arguments"); return -1; }
  for (int i = 0; i < F; i++) {
    PoolRng rng(seed, key, (uint64_t)i);
    double x1 = 1., y1 = 1., x2 = 1., y2 = 1.;
    while (x1 * x1 + y1 * y1 > 1. || x2 * x2 + y2 * y2 > 1.) {               // cart.cpp:364-367
      x1 = rng.uniform(-1., 1.); y1 = rng.uniform(-1., 1.);
      x2 = rng.uniform(-1., 1.); y2 = rng.uniform(-1., 1.);
    }
    jdaFeatureCpp& f = out_features[i];
    std::memset(&f, 0, sizeof f);
    f.scale = rng.below(3);                                                   // cart.cpp:369-378
    if (!multi_scale) f.scale = 0;                                            // cart.cpp:381
    f.landmark_id1 = rng.below(landmark_n);
    f.landmark_id2 = rng.below(landmark_n);
    f.offset1_x = x1 * radius; f.offset1_y = y1 * radius;
    f.offset2_x = x2 * radius; f.offset2_y = y2 * radius;
    if (out_u) out_u[i] = rng.uniform(0.1, 0.9);                              // cart.cpp:320
  }
  return 0;
} JDA_ABI_CATCH(-1)

int jdaCalcSTParametersCpp(void* cascador, const double* shapes, int n, double* stp_mc, double* stp_cm) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || n < 0 || (n > 0 && !shapes)) { fail("bad arguments"); return -1; }
  if (n == 0 || (!stp_mc && !stp_cm)) return 0;
  if (!c->similarity) {                                                       // STParameter's default, data.cpp:68-70
    for (double* out : {stp_mc, stp_cm})
      for (int i = 0; out && i < n; i++) { double* p = out + 5 * (size_t)i; p[0] = 1.; p[1] = 1.; p[2] = 0.; p[3] = 0.; p[4] = 1.; }
    return 0;
  }
  const int L = c->hm.L;
  const size_t N = (size_t)n, dim = 2 * (size_t)L;
  OneLane one(c);
  CallBuf buf;
  auto body = [&]() -> bool {
    if (!one.open()) return false;
    hipStream_t st = one.stream;
    double* raw; double* tr; double* ms; double* mc; double* cm;
    if (!carve_into(buf, [&](Carver& cv) {
          raw = cv.take<double>(N * dim); tr = cv.take<double>(N * dim); ms = cv.take<double>(4 + 2 * dim);
          mc = stp_mc ? cv.take<double>(5 * N) : nullptr; cm = stp_cm ? cv.take<double>(5 * N) : nullptr;
        })) return false;
    JDA_HIP(hipMemcpyAsync(raw, shapes, N * dim * sizeof(double), hipMemcpyHostToDevice, st));
    JDA_HIP(hipMemcpyAsync(ms + 4 + dim, c->hm.mean_shape.data(), dim * sizeof(double), hipMemcpyHostToDevice, st));
    JDA_HIP(launch_train_transpose(raw, n, (int)dim, tr, st));
    JDA_HIP(launch_stp(tr, n, L, ms + 4 + dim, ms, mc, cm, st));
    std::vector<double> planes(5 * N);
    for (int which = 0; which < 2; which++) {                                 // planes [5][n] -> rows of (scale, rot00, rot01, rot10, rot11)
      const double* dev = which ? cm : mc;
      double* out = which ? stp_cm : stp_mc;
      if (!out) continue;
      JDA_HIP(hipMemcpyAsync(planes.data(), dev, 5 * N * sizeof(double), hipMemcpyDeviceToHost, st));
      JDA_HIP(hipStreamSynchronize(st));
      for (size_t i = 0; i < N; i++)
        for (int k = 0; k < 5; k++) out[5 * i + k] = planes[(size_t)k * N + i];
    }
    return true;
  };
  return body() ? 0 : -1;
} JDA_ABI_CATCH_SYNC(-1)

int jdaCalcFeatureValuesCpp(void* cascador, const jdaSamplesCpp* samples, int origin_size, int half_size, int quarter_size,
                            const jdaFeatureCpp* pool, int F, int* out) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!begin(c, origin_size, half_size, quarter_size, __func__)) return -1;
  if (F < 0 || (F > 0 && !pool)) { fail("bad arguments"); return -1; }
  if (!check_set(samples, "samples", false) || !check_pool(pool, (size_t)F, c->hm.L)) return -1;
  if (F == 0 || samples->n == 0) return 0;
  if (!out) { fail("bad arguments"); return -1; }
  Ctx x(c);
  jdaSamplesCpp none{};
  auto body = [&]() -> bool {
    if (!x.open(samples, &none, origin_size, half_size, quarter_size, F) || !x.upload_pool(pool)) return false;
    const int n = samples->n;
    std::vector<short> h((size_t)x.Fc * x.stride_p);
    for (int f0 = 0; f0 < F; f0 += x.Fc) {
      const int fc = std::min(x.Fc, F - f0);
      JDA_HIP(launch_train_values(x.pos.ts, nullptr, n, x.d_pool + f0, fc, x.d_vals_p, x.stride_p, x.st));
      JDA_HIP(hipMemcpyAsync(h.data(), x.d_vals_p, (size_t)fc * x.stride_p * sizeof(short), hipMemcpyDeviceToHost, x.st));
      JDA_HIP(hipStreamSynchronize(x.st));
      for (int i = 0; i < fc; i++)
        for (int j = 0; j < n; j++) out[(size_t)(f0 + i) * n + j] = h[(size_t)i * x.stride_p + j];
    }
    return true;
  };
  return body() ? 0 : -1;
} JDA_ABI_CATCH_SYNC(-1)

int jdaSplitNodeCpp(void* cascador, const jdaSamplesCpp* pos, const jdaSamplesCpp* neg, int origin_size, int half_size,
                    int quarter_size, const jdaFeatureCpp* pool, int F, int mode, const double* u, int* feature_idx,
                    int* threshold, double* criterion, int* thresholds) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!begin(c, origin_size, half_size, quarter_size, __func__)) return -1;
  if (F < 1 || !pool || (mode != 0 && mode != 1) || !feature_idx || !threshold) { fail("bad arguments"); return -1; }
  if (!check_set(pos, "pos", true) || !check_set(neg, "neg", true) || !check_pool(pool, (size_t)F, c->hm.L)) return -1;
  Ctx x(c);
  auto body = [&]() -> bool {
    if (!x.open(pos, neg, origin_size, half_size, quarter_size, F)) return false;
    std::vector<int> pl(pos->n), nl(neg->n);
    std::iota(pl.begin(), pl.end(), 0); std::iota(nl.begin(), nl.end(), 0);
    double best;
    return split_node(x, pl, nl, pool, mode, u, feature_idx, threshold, &best, criterion, thresholds);
  };
  return body() ? 0 : -1;
} JDA_ABI_CATCH_SYNC(-1)

int jdaSplitNodeSumsCpp(void* cascador, const jdaSamplesCpp* pos, const jdaSamplesCpp* neg, int origin_size, int half_size,
                        int quarter_size, const jdaFeatureCpp* pool, int F, int mode, const double* u, const int* pos_list,
                        int pos_list_n, const int* neg_list, int neg_list_n, int* feature_idx, int* threshold, double* criterion,
                        int* thresholds, jdaSplitSumsCpp* sums) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!begin(c, origin_size, half_size, quarter_size, __func__)) return -1;
  if (F < 1 || !pool || (mode != 0 && mode != 1) || !feature_idx || !threshold) { fail("bad arguments"); return -1; }
  if (!check_set(pos, "pos", true) || !check_set(neg, "neg", true) || !check_pool(pool, (size_t)F, c->hm.L)) return -1;
  std::vector<int> pl, nl;
  auto take = [](const int* list, int count, int n, const char* name, std::vector<int>* out) -> bool {
    if (!list) { out->resize(n); std::iota(out->begin(), out->end(), 0); return true; }
    if (count < 0) { fail(std::string(name) + ": negative count"); return false; }
    for (int j = 0; j < count; j++)
      if (list[j] < 0 || list[j] >= n || (j > 0 && list[j] <= list[j - 1])) {
        fail(std::string(name) + ": entry " + std::to_string(j) + " is outside [0, n) or not above the entry before it "
             "(a node's list is strictly ascending)");
        return false;
      }
    out->assign(list, list + count);
    return true;
  };
  if (!take(pos_list, pos_list_n, pos->n, "pos_list", &pl) || !take(neg_list, neg_list_n, neg->n, "neg_list", &nl)) return -1;
  if (sums) {
    const size_t P = pl.size(), N = nl.size(), hb = (size_t)F * kTrainBins;
    auto zero = [](auto* p, size_t count) { if (p && count) std::memset(p, 0, count * sizeof *p); };
    zero(sums->pos_values, (size_t)F * P); zero(sums->neg_values, (size_t)F * N);
    zero(sums->pos_hist_w, hb); zero(sums->neg_hist_w, hb); zero(sums->pos_hist_c, hb); zero(sums->neg_hist_c, hb);
    zero(sums->var_sums, 8 * (size_t)F); zero(sums->var_n_left, F); zero(sums->var_n_right, F); zero(sums->var_th, F);
    sums->chunks = 0;
  }
  Ctx x(c);
  auto body = [&]() -> bool {
    if (!x.open(pos, neg, origin_size, half_size, quarter_size, F)) return false;
    double best;
    if (!split_node(x, pl, nl, pool, mode, u, feature_idx, threshold, &best, criterion, thresholds, sums)) return false;
    if (sums) sums->chunks = x.chunks;
    return true;
  };
  return body() ? 0 : -1;
} JDA_ABI_CATCH_SYNC(-1)

int jdaTrainCartCpp(void* cascador, const jdaSamplesCpp* pos, const jdaSamplesCpp* neg, int origin_size, int half_size,
                    int quarter_size, const jdaFeatureCpp* pools, int F, const int* modes, const double* us,
                    jdaFeatureCpp* out_features, int* out_thresholds, double* out_scores, int* pos_leaf, int* neg_leaf,
                    jdaTrainStatsCpp* stats) try {
  g_err.clear();
  const double t0 = now_ms();
  Cascador* c = (Cascador*)cascador;
  if (!begin(c, origin_size, half_size, quarter_size, __func__)) return -1;
  const int D = c->hm.D;
  if (D < 1 || D > 20) { fail("tree_depth outside [1, 20]"); return -1; }
  const int half = 1 << (D - 1), inner = half - 1;                          // nodes_n / 2 leaves; internal nodes 1 .. half - 1
  if (F < 1 || (inner > 0 && (!pools || !modes))) { fail("bad arguments"); return -1; }
  if (!check_set(pos, "pos", true) || !check_set(neg, "neg", true) || !check_pool(pools, (size_t)inner * F, c->hm.L)) return -1;
  bool any_reg = false;
  for (int i = 0; i < inner; i++) {
    if (modes[i] != 0 && modes[i] != 1) { fail("modes must be 0 (regression) or 1 (classification)"); return -1; }
    any_reg |= modes[i] == 0;
  }
  if (any_reg && !us) { fail("regression nodes need us"); return -1; }
  if (any_reg && pos->n > 0 && !pos->residual) { fail("regression nodes need pos->residual"); return -1; }
  Ctx x(c);
  jdaTrainNodeCpp* ns = stats ? stats->nodes : nullptr;
  double setup_ms = 0;
  auto body = [&]() -> bool {
    if (!x.open(pos, neg, origin_size, half_size, quarter_size, F)) return false;
    setup_ms = now_ms() - t0;
    // the lists of every node, level by level; a node's children keep ascending sample order (cart.cpp:120-150)
    std::vector<std::vector<int>> pl(2 * (size_t)half), nl(2 * (size_t)half);
    pl[1].resize(pos->n); nl[1].resize(neg->n);
    std::iota(pl[1].begin(), pl[1].end(), 0); std::iota(nl[1].begin(), nl[1].end(), 0);
    std::vector<short> row;
    for (int node = 1; node < half; node++) {
      const jdaFeatureCpp* pool = pools + (size_t)(node - 1) * F;
      int fi = 0, th = -256;
      double best = 0;
      if (!split_node(x, pl[node], nl[node], pool, modes[node - 1], us ? us + (size_t)(node - 1) * F : nullptr, &fi, &th, &best,
                      nullptr, nullptr)) return false;
      if (out_features) out_features[node - 1] = pool[fi];
      if (out_thresholds) out_thresholds[node - 1] = th;
      if (ns) {
        jdaTrainNodeCpp& s = ns[node - 1];
        s.pos_n = (int)pl[node].size(); s.neg_n = (int)nl[node].size(); s.feature_idx = fi; s.threshold = th;
        s.mode = modes[node - 1]; s.pad = 0; s.criterion = best;
      }
      const double tp = now_ms();
      // (a regression node with no positives returns before the pool is uploaded: upload it for the partition)
      if (modes[node - 1] == 0 && pl[node].empty() && !x.upload_pool(pool)) return false;
      for (int cls = 0; cls < 2; cls++) {
        std::vector<int>& src = cls ? nl[node] : pl[node];
        std::vector<int>& left = cls ? nl[2 * node] : pl[2 * node];
        std::vector<int>& right = cls ? nl[2 * node + 1] : pl[2 * node + 1];
        int* d_list = cls ? x.d_list_n : x.d_list_p;
        if (!src.empty()) JDA_HIP(hipMemcpyAsync(d_list, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice, x.st));
        if (!feature_row(x, cls ? x.neg : x.pos, d_list, (int)src.size(), fi, cls ? x.d_vals_n : x.d_vals_p, &row)) return false;
        for (size_t j = 0; j < src.size(); j++) (row[j] <= th ? left : right).push_back(src[j]);
        std::vector<int>().swap(src);
      }
      x.partition_ms += now_ms() - tp;
    }
    for (int leaf = 0; leaf < half; leaf++) {                                 // cart.cpp:63-89
      double pos_w = kEsp, neg_w = kEsp;
      for (int s : pl[half + leaf]) { pos_w += pos->weights[s]; if (pos_leaf) pos_leaf[s] = leaf; }
      for (int s : nl[half + leaf]) { neg_w += neg->weights[s]; if (neg_leaf) neg_leaf[s] = leaf; }
      if (out_scores) out_scores[leaf] = 0.5 * (std::log(pos_w) - std::log(neg_w));
    }
    return true;
  };
  if (!body()) return -1;
  if (stats) {
    stats->call_ms = now_ms() - t0; stats->setup_ms = setup_ms; stats->device_ms = x.device_ms; stats->sweep_ms = x.sweep_ms;
    stats->partition_ms = x.partition_ms; stats->feature_evals = x.evals; stats->feature_chunks = x.chunks;
  }
  return 0;
} JDA_ABI_CATCH_SYNC(-1)

}  // extern "C"
