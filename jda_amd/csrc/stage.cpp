// libjda.so, host side: closing a training stage of dialect CPP (jdaGenLbfCpp, jdaStageUpdateShapesCpp, jdaMeanErrorCpp;
// reference src/jda/btcart.cpp:255-292, 390-424, common.cpp:41-77) on the kernel of k_lbf.hip.  The samples go through the
// device in chunks that fit the cascador's workspace_mb; the stage's carts (as a level-major node table) and weights are
// uploaded once per call.  Nothing here fits or writes a model: liblinear's part stays with the caller.
#include <climits>
#include <cmath>

#include "detect.h"

namespace jda {

namespace {

struct StageCall {
  Cascador* c;
  const jdaSamplesCpp* s;
  int os, hs, qs;
  const jdaStageCartsCpp* carts;
  int K;
  const double* w;            // null: indicators only
  const int* lbf_in;          // null: walk the carts
  double* out_shapes;
  int* out_lbf;
  jdaStageStatsCpp* stats;
};

// Everything that can be refused, before the device is touched.  *empty: nothing to do.
bool check_call(StageCall& x, const char* fn, bool* empty) {
  *empty = false;
  Cascador* c = x.c;
  if (!c) { fail("bad arguments"); return false; }
  if (!check_patch_sizes(x.os, x.hs, x.qs)) return false;
  if (c->similarity && !c->kn.train_similarity) {        // (refused unless the caller opted in: include/jda.h)
    fail(std::string(fn) + ": refused with jdaSetSimilarityTransform(1): the training entries refuse with it on (data.cpp:168), "
         "so a sample set for this entry cannot exist");
    return false;
  }
  if (!check_set(x.s, "samples", false)) return false;
  const bool walk = x.lbf_in == nullptr;
  if (walk && !x.carts) { fail("carts must be given where the entry walks them"); return false; }
  x.K = x.carts ? x.carts->K : c->hm.K;
  if (x.K <= 0) { fail("K must be positive"); return false; }
  const int D = c->hm.D;
  if (D < 1 || D > 20) { fail("tree_depth outside [1, 20]"); return false; }
  const long long leaf_n = 1ll << (D - 1), inner = leaf_n - 1;
  if ((long long)x.K * leaf_n > INT_MAX) { fail("K * leafNum does not fit an int index"); return false; }
  if (walk && inner > 0) {
    if (!x.carts->features || !x.carts->thresholds) { fail("carts: features and thresholds must be given"); return false; }
    if (!check_pool(x.carts->features, (size_t)x.K * (size_t)inner, c->hm.L)) return false;
  }
  if (x.s->n == 0) { *empty = true; return true; }
  if (x.out_shapes) {
    if (!x.w) { fail("w must be given"); return false; }
  } else if (!x.out_lbf) {
    fail("bad arguments: no output array"); return false;
  }
  if (x.lbf_in) {                                        // 0 <= lbf_in[i*K + k] - k*leafNum < leafNum
    const int n = x.s->n, K = x.K, blocks = (n + 4095) / 4096;
    std::atomic<long long> bad{-1};
    parallel_for(blocks, [&](int b) {
      const int i1 = std::min(n, (b + 1) * 4096);
      for (int i = b * 4096; i < i1; i++) {
        const int* row = x.lbf_in + (size_t)i * K;
        for (int k = 0; k < K; k++) {
          const long long leaf = (long long)row[k] - (long long)k * leaf_n;
          if (leaf < 0 || leaf >= leaf_n) { long long none = -1; bad.compare_exchange_strong(none, (long long)i * K + k); return; }
        }
      }
    }, blocks < 8);
    if (bad.load() >= 0) {
      const long long at = bad.load();
      fail("lbf_in[" + std::to_string(at) + "] is not a leaf of cart " + std::to_string(at % K)); return false;
    }
  }
  return true;
}

bool run_call(StageCall& x) {
  const double t0 = now_ms();
  Cascador* c = x.c;
  const jdaSamplesCpp* s = x.s;
  const int n = s->n, K = x.K, D = c->hm.D, L = c->hm.L, dim = 2 * L;
  const int leaf_n = 1 << (D - 1), inner = leaf_n - 1;
  const bool walk = x.lbf_in == nullptr, update = x.out_shapes != nullptr;
  const bool st_on = train_similarity(c);                // every sample under STParameter::Calc(its shape, mean_shape), btcart.cpp:399, 422
  const size_t pbytes = (size_t)x.os * x.os + (size_t)x.hs * x.hs + (size_t)x.qs * x.qs;
  const bool host_patches = walk && !s->patches_on_device;
  double upload_ms = 0, device_ms = 0, download_ms = 0;

  OneLane one(c);
  if (!one.open()) return false;
  hipStream_t st = one.stream;

  // the stage's carts, level-major (kernels.h: lbf_node_at), and its weights
  std::vector<NodeD> nodes;
  if (walk && inner > 0) {
    nodes.resize((size_t)K * inner);
    for (int k = 0; k < K; k++)
      for (int d = 0; d < D - 1; d++)
        for (int i = 1 << d; i < (2 << d); i++) {
          const size_t src = (size_t)k * inner + (i - 1);
          const jdaFeatureCpp& f = x.carts->features[src];
          NodeD& nd = nodes[lbf_node_at(K, k, i, d)];
          nd.scale = f.scale; nd.lm1x2 = 2 * f.landmark_id1; nd.lm2x2 = 2 * f.landmark_id2; nd.th = x.carts->thresholds[src];
          nd.o1x = f.offset1_x; nd.o1y = f.offset1_y; nd.o2x = f.offset2_x; nd.o2y = f.offset2_y;
        }
  }
  const size_t w_count = update ? (size_t)K * leaf_n * dim : 0;
  const size_t fixed = nodes.size() * sizeof(NodeD) + w_count * sizeof(double) + 4096;
  const size_t per = (size_t)dim * 8 * (update ? 2 : 1) + (size_t)K * 4 + (host_patches ? pbytes : 0) + 64;
  const size_t budget = (size_t)std::max<long long>(1, c->kn.workspace_mb) << 20;
  const size_t room = budget > fixed ? budget - fixed : 0;
  const int nc = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, room / per));

  CallBuf buf;
  NodeD* d_nodes; double* d_w; double* d_sh; double* d_out; int* d_lbf; uint8_t* d_pat; double* d_mean = nullptr;
  if (!carve_into(buf, [&](Carver& cv) {
        if (st_on) d_mean = cv.take<double>(dim);
        d_nodes = cv.take<NodeD>(std::max<size_t>(nodes.size(), 1));
        d_w = update ? cv.take<double>(w_count) : nullptr;
        d_sh = cv.take<double>((size_t)nc * dim);
        d_out = update ? cv.take<double>((size_t)nc * dim) : nullptr;
        d_lbf = cv.take<int>((size_t)nc * K);
        d_pat = host_patches ? cv.take<uint8_t>((size_t)nc * pbytes) : nullptr;
      })) return false;
  EvTimer timer;
  if (!timer.open(x.stats)) return false;

  double t = now_ms();
  if (!nodes.empty()) JDA_HIP(hipMemcpyAsync(d_nodes, nodes.data(), nodes.size() * sizeof(NodeD), hipMemcpyHostToDevice, st));
  if (update) JDA_HIP(hipMemcpyAsync(d_w, x.w, w_count * sizeof(double), hipMemcpyHostToDevice, st));
  if (st_on) JDA_HIP(hipMemcpyAsync(d_mean, c->hm.mean_shape.data(), (size_t)dim * sizeof(double), hipMemcpyHostToDevice, st));
  JDA_HIP(hipStreamSynchronize(st));
  upload_ms += now_ms() - t;

  const int lds_budget = (int)std::min<long long>(160, std::max<long long>(0, c->kn.lbf_lds_kb)) * 1024;
  WaveLaunch how{0, kSampleWaves, 0};
  int chunks = 0;
  for (int i0 = 0; i0 < n; i0 += nc, chunks++) {
    const int cn = std::min(nc, n - i0);
    t = now_ms();
    JDA_HIP(hipMemcpyAsync(d_sh, s->shapes + (size_t)i0 * dim, (size_t)cn * dim * sizeof(double), hipMemcpyHostToDevice, st));
    if (host_patches) JDA_HIP(hipMemcpyAsync(d_pat, s->patches + (size_t)i0 * pbytes, (size_t)cn * pbytes, hipMemcpyHostToDevice, st));
    if (!walk) JDA_HIP(hipMemcpyAsync(d_lbf, x.lbf_in + (size_t)i0 * K, (size_t)cn * K * sizeof(int), hipMemcpyHostToDevice, st));
    JDA_HIP(hipStreamSynchronize(st));
    upload_ms += now_ms() - t;
    LbfArgs a{};
    a.patches = walk ? (host_patches ? d_pat : s->patches + (size_t)i0 * pbytes) : nullptr;
    a.shapes = d_sh; a.nodes = d_nodes; a.w = d_w; a.lbf = d_lbf; a.out_shapes = d_out;
    a.n = cn; a.K = K; a.D = D; a.dim = dim; a.os = x.os; a.hs = x.hs; a.qs = x.qs; a.walk = walk ? 1 : 0;
    a.mean = d_mean;
    if (!timer.begin(st)) return false;
    JDA_HIP(launch_lbf(a, lds_budget, &how, st));
    if (!timer.end(st)) return false;
    JDA_HIP(hipStreamSynchronize(st));
    if (!timer.add(&device_ms)) return false;
    t = now_ms();
    if (update) JDA_HIP(hipMemcpyAsync(x.out_shapes + (size_t)i0 * dim, d_out, (size_t)cn * dim * sizeof(double), hipMemcpyDeviceToHost, st));
    if (x.out_lbf) JDA_HIP(hipMemcpyAsync(x.out_lbf + (size_t)i0 * K, d_lbf, (size_t)cn * K * sizeof(int), hipMemcpyDeviceToHost, st));
    JDA_HIP(hipStreamSynchronize(st));
    download_ms += now_ms() - t;
  }
  if (x.stats) {
    jdaStageStatsCpp& o = *x.stats;
    o.call_ms = now_ms() - t0; o.upload_ms = upload_ms; o.device_ms = device_ms; o.download_ms = download_ms;
    o.chunks = chunks; o.lds_path = how.lds; o.waves_per_group = how.waves; o.lds_bytes = how.lds_bytes;
  }
  return true;
}

int stage_entry(StageCall& x, const char* fn) {
  if (x.stats) std::memset(x.stats, 0, sizeof *x.stats);
  bool empty = false;
  if (!check_call(x, fn, &empty)) return -1;
  if (empty) return 0;
  return run_call(x) ? 0 : -1;
}

}  // namespace
}  // namespace jda

using namespace jda;

extern "C" {

int jdaGenLbfCpp(void* cascador, const jdaSamplesCpp* samples, int origin_size, int half_size, int quarter_size,
                 const jdaStageCartsCpp* carts, int* lbf) try {
  g_err.clear();
  if (!carts) { fail("bad arguments"); return -1; }
  StageCall x{(Cascador*)cascador, samples, origin_size, half_size, quarter_size, carts, 0, nullptr, nullptr, nullptr, lbf, nullptr};
  return stage_entry(x, __func__);
} JDA_ABI_CATCH_SYNC(-1)

int jdaStageUpdateShapesCpp(void* cascador, const jdaSamplesCpp* samples, int origin_size, int half_size, int quarter_size,
                            const jdaStageCartsCpp* carts, const double* w, const int* lbf_in, double* out_shapes, int* out_lbf,
                            jdaStageStatsCpp* stats) try {
  g_err.clear();
  if (!out_shapes && samples && samples->n > 0) { fail("bad arguments: out_shapes is null"); return -1; }
  StageCall x{(Cascador*)cascador, samples, origin_size, half_size, quarter_size, carts, 0, w, lbf_in, out_shapes, out_lbf, stats};
  return stage_entry(x, __func__);
} JDA_ABI_CATCH_SYNC(-1)

int jdaMeanErrorCpp(const double* gt_shapes, const double* cur_shapes, int n, int L, const int* left_pupils, int n_left,
                    const int* right_pupils, int n_right, double* out) try {
  g_err.clear();
  if (n < 0 || L < 1 || !left_pupils || !right_pupils || n_left < 1 || n_right < 1 || !out || (n > 0 && (!gt_shapes || !cur_shapes))) {
    fail("bad arguments"); return -1;
  }
  for (int j = 0; j < n_left; j++) if (left_pupils[j] < 0 || left_pupils[j] >= L) { fail("left pupil id outside [0, L)"); return -1; }
  for (int j = 0; j < n_right; j++) if (right_pupils[j] < 0 || right_pupils[j] >= L) { fail("right pupil id outside [0, L)"); return -1; }
  const size_t dim = 2 * (size_t)L;
  double e = 0.;
  for (int i = 0; i < n; i++) {                                               // common.cpp:48-74
    const double* gt = gt_shapes + (size_t)i * dim;
    const double* cur = cur_shapes + (size_t)i * dim;
    double left_x = 0., left_y = 0., right_x = 0., right_y = 0.;
    for (int j = 0; j < n_left; j++) { left_x += gt[2 * left_pupils[j]]; left_y += gt[2 * left_pupils[j] + 1]; }
    left_x /= (double)n_left; left_y /= (double)n_left;
    for (int j = 0; j < n_right; j++) { right_x += gt[2 * right_pupils[j]]; right_y += gt[2 * right_pupils[j] + 1]; }
    right_x /= (double)n_right; right_y /= (double)n_right;
    const double dx = left_x - right_x, dy = left_y - right_y;
    const double pupil_dis = std::sqrt(dx * dx + dy * dy);
    double e_ = 0.;
    for (int j = 0; j < L; j++) {
      const double ex = gt[2 * j] - cur[2 * j], ey = gt[2 * j + 1] - cur[2 * j + 1];
      e_ += std::sqrt(ex * ex + ey * ey);
    }
    e += e_ / pupil_dis;
  }
  e /= (double)((long long)L * n);                                            // common.cpp:75
  *out = e;
  return 0;
} JDA_ABI_CATCH(-1)

}  // extern "C"
