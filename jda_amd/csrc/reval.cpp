// libjda.so, host side: JoinCascador::Validate (reference src/jda/cascador.cpp:166-211) on every record of a resident sample
// set (jdaValidateSamplesCpp), on the kernel of k_reval.hip (option reval_form 0, a wave per sample) or on k_mine_walk over the
// same records (reval_form 1, a lane per sample: identical bits, kept for A/B and as an independent check).  The model is the
// one the mining entries walk -- the mining tables with Validate's own loop bounds, patched in place while a model grows
// (mine.cpp, model_grow.cpp) -- the patches are read as stored (nothing is resized) and sample i starts from samples->shapes[i].
// The samples go through the device in chunks that fit the cascador's workspace_mb; device-resident patches are read in place.
#include "detect.h"

namespace jda {

int reval_entry(Cascador* c, const jdaSamplesCpp* s, int os, int hs, int qs, unsigned char* is_face, double* score, int* carts_n,
                double* shape, jdaStageStatsCpp* stats) {
  const double t0 = now_ms();
  const char* fn = "jdaValidateSamplesCpp";
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (!c) { fail("bad arguments"); return -1; }
  if (!check_patch_sizes(os, hs, qs)) return -1;
  if (c->similarity && !c->kn.train_similarity) {        // (refused unless the caller opted in: include/jda.h)
    fail(std::string(fn) + ": refused with jdaSetSimilarityTransform(1): the training entries refuse with it on (data.cpp:168), "
         "so a sample set for this entry cannot exist");
    return -1;
  }
  if (!check_set(s, "samples", false)) return -1;
  const int n = s->n;
  if (n == 0) return 0;
  MineModel m;
  if (!mine_model(c, &m)) return -1;
  const int K = m.K, dim = m.dim;
  const size_t pbytes = (size_t)os * os + (size_t)hs * hs + (size_t)qs * qs;
  const bool host_patches = !s->patches_on_device;
  const bool lane_form = c->kn.reval_form == 1;
  const int st_on = train_similarity(c) ? 1 : 0;         // cascador.cpp:180: every full stage under Calc(shape as it stands, mean_shape)
  double upload_ms = 0, device_ms = 0, download_ms = 0;

  OneLane one(c);
  if (!one.open()) return -1;
  hipStream_t st = one.stream;

  // per sample: start shape and shape, the stage's indicators, the three outputs, host patches; form 1: k_mine_walk's t1, t2
  const size_t per = (size_t)dim * 8 * (lane_form ? 4 : 2) + (size_t)K * 4 + 8 + 4 + 1 + (host_patches ? pbytes : 0) + 64;
  const size_t budget = (size_t)std::max<long long>(1, c->kn.workspace_mb) << 20;
  const int nc = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n, budget / per, (size_t)1 << 22}));

  CallBuf buf;
  double* d_start; double* d_shape; double* d_t1 = nullptr; double* d_t2 = nullptr; int* d_lbf; double* d_score; int* d_carts;
  uint8_t* d_face; uint8_t* d_pat = nullptr;
  auto body = [&]() -> bool {
    if (!carve_into(buf, [&](Carver& cv) {
          d_start = cv.take<double>((size_t)nc * dim); d_shape = cv.take<double>((size_t)nc * dim);
          if (lane_form) { d_t1 = cv.take<double>((size_t)nc * dim); d_t2 = cv.take<double>((size_t)nc * dim); }
          d_lbf = cv.take<int>((size_t)nc * K); d_score = cv.take<double>(nc); d_carts = cv.take<int>(nc);
          d_face = cv.take<uint8_t>(nc);
          if (host_patches) d_pat = cv.take<uint8_t>((size_t)nc * pbytes);
        })) return false;
    EvTimer timer;
    if (!timer.open(stats)) return false;
    const int lds_budget = (int)std::min<long long>(160, std::max<long long>(0, c->kn.reval_lds_kb)) * 1024;
    WaveLaunch how{0, lane_form ? 1 : kSampleWaves, 0};
    std::vector<uint8_t> f(nc);
    int chunks = 0;
    for (int i0 = 0; i0 < n; i0 += nc, chunks++) {
      const int cn = std::min(nc, n - i0);
      double t = now_ms();
      JDA_HIP(hipMemcpyAsync(d_start, s->shapes + (size_t)i0 * dim, (size_t)cn * dim * sizeof(double), hipMemcpyHostToDevice, st));
      if (host_patches) JDA_HIP(hipMemcpyAsync(d_pat, s->patches + (size_t)i0 * pbytes, (size_t)cn * pbytes, hipMemcpyHostToDevice, st));
      JDA_HIP(hipStreamSynchronize(st));
      upload_ms += now_ms() - t;
      const uint8_t* pat = host_patches ? d_pat : s->patches + (size_t)i0 * pbytes;
      if (!timer.begin(st)) return false;
      if (lane_form) {
        const MineSizes z{os, hs, qs, 0, 0., 0ull};
        JDA_HIP(launch_mine_walk(m, z, nullptr, cn, pat, (int)pbytes, st_on, d_face, d_carts, d_score, d_shape, d_lbf, d_t1, d_t2, st, d_start));
      } else {
        RevalArgs a{};
        a.m = m; a.patches = pat; a.start = d_start; a.face = d_face; a.carts_n = d_carts; a.score = d_score; a.shape = d_shape;
        a.lbf = d_lbf; a.n = cn; a.os = os; a.hs = hs; a.qs = qs; a.st = st_on;
        JDA_HIP(launch_reval(a, lds_budget, &how, st));
      }
      if (!timer.end(st)) return false;
      JDA_HIP(hipStreamSynchronize(st));
      if (!timer.add(&device_ms)) return false;
      t = now_ms();
      if (is_face) JDA_HIP(hipMemcpyAsync(is_face + i0, d_face, cn, hipMemcpyDeviceToHost, st));
      if (score) JDA_HIP(hipMemcpyAsync(score + i0, d_score, (size_t)cn * sizeof(double), hipMemcpyDeviceToHost, st));
      if (carts_n) JDA_HIP(hipMemcpyAsync(carts_n + i0, d_carts, (size_t)cn * sizeof(int), hipMemcpyDeviceToHost, st));
      if (shape) JDA_HIP(hipMemcpyAsync(shape + (size_t)i0 * dim, d_shape, (size_t)cn * dim * sizeof(double), hipMemcpyDeviceToHost, st));
      JDA_HIP(hipStreamSynchronize(st));
      download_ms += now_ms() - t;
    }
    if (stats) {
      stats->call_ms = now_ms() - t0; stats->upload_ms = upload_ms; stats->device_ms = device_ms; stats->download_ms = download_ms;
      stats->chunks = chunks; stats->lds_path = how.lds; stats->waves_per_group = how.waves; stats->lds_bytes = how.lds_bytes;
    }
    return true;
  };
  return body() ? 0 : -1;
}

}  // namespace jda
