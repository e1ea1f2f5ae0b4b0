// libjda.so, host side: dialect C's window body (reference c/jda.c:340-414, relocation 471-472) on windows the CALLER names --
// jdaValidateWindows (frames in host memory) and jdaValidateWindowsDevice (frames resident on the device) -- on the kernel of
// k_windows.hip.  Everything is validated before anything is launched; the model is the fp32 copy every dialect-C entry walks
// (a double file narrows like c/jda.c:509-552, a trainer snapshot runs T x K like c/jda.c:499-505); the half / quarter images
// are jdaBuildPyramid's, built by the same resize kernel and only for a model that has a split node with scale != 0.  The call
// runs on one lane of the cascador's pool; the window list goes through the device in chunks that fit the cascador's
// workspace_mb, one launch and one copy-back per chunk.
#include "detect.h"

namespace jda {

int windows_entry(Cascador* c, const char* fn, const unsigned char* const* host_frames, const uint8_t* d_frames, size_t stride, int n,
                  int width, int height, const int* windows, int n_windows, float th, const WindowsOut& out) {
  LaneCall call(c);
  const std::string who = std::string(fn) + ": ";
  if (!c) { fail(who + "null cascador"); return -1; }
  if (n < 0 || n_windows < 0) { fail(who + "negative number of frames or windows"); return -1; }
  if (n_windows == 0) return 0;
  if (!windows) { fail(who + "null window list"); return -1; }
  if (n > 0 && !host_frames && !d_frames) { fail(who + "null frames"); return -1; }
  for (int i = 0; host_frames && i < n; i++)
    if (!host_frames[i]) { fail(who + "null frame pointer (frame " + std::to_string(i) + ")"); return -1; }
  // the frame sizes the other dialect-C entries refuse (plan.cpp: plan_dialect_c, plans.cpp: get_plan)
  if (width <= 0 || height <= 0) { fail(who + "frame has no pixels"); return -1; }
  if (width > 65535 || height > 65535) { fail(who + "frames wider or taller than 65535 pixels are not supported"); return -1; }
  const size_t fbytes = (size_t)width * height;
  if (!host_frames && stride < fbytes) { fail(who + "frame_stride smaller than a frame"); return -1; }
  for (int i = 0; i < n_windows; i++) {
    const int* q = windows + 4 * (size_t)i;
    if (q[0] < 0 || q[0] >= n || q[3] < 1 || q[1] < 0 || q[2] < 0 || (long long)q[1] + q[3] > width || (long long)q[2] + q[3] > height) {
      fail(who + "window " + std::to_string(i) + " (frame, x, y, size) = (" + std::to_string(q[0]) + ", " + std::to_string(q[1]) + ", " +
           std::to_string(q[2]) + ", " + std::to_string(q[3]) + ") does not lie inside one of the " + std::to_string(n) + " frames of " +
           std::to_string(width) + " x " + std::to_string(height));
      return -1;
    }
  }
  const float r = 1.f / sqrtf(2.f);                                // c/jda.c:450-456
  const int hw = (int)((float)width * r), hh = (int)((float)height * r), qw = width / 2, qh = height / 2;
  bool multi = false;
  {
    std::unique_lock<std::mutex> lk(c->mu);
    multi = c->hm.multi_scale();                                   // (caches its answer in the model on first use: under the mutex)
    if (multi && (hw < 1 || hh < 1 || qw < 1 || qh < 1)) { fail(who + "frame too small for the half / quarter images a multi-scale model reads"); return -1; }
    if (!ensure_device(c) || !upload_model<float>(c)) return -1;
  }
  const DevModelT<float> m = c->mf.m;
  const int dim = m.dim;
  if (!call.open()) return -1;
  Lane* ln = call.lane;
  const hipStream_t st = call.st;

  long long faces = 0, nf_carts = 0;
  auto body = [&]() -> bool {
    if (host_frames) {
      if (!stage_frames(ln, host_frames, n, fbytes, &stride)) return false;
      d_frames = (const uint8_t*)ln->frames.p;
    }
    WinArgs a{};
    a.frames = d_frames; a.frame_stride = stride; a.n_frames = n; a.width = width; a.height = height; a.th = th;
    if (multi) {                                                   // jdaImageResize, c/jda.c:203-230, 450-457
      const size_t hs = ((size_t)hw * hh + 255) & ~(size_t)255, qs = ((size_t)qw * qh + 255) & ~(size_t)255;
      if (!ln->pyr.reserve((hs + qs) * (size_t)n + 512)) return false;
      uint8_t* hbuf = (uint8_t*)ln->pyr.p;
      uint8_t* qbuf = hbuf + hs * (size_t)n;
      for (int f0 = 0; f0 < n; f0 += 32768) {                      // (a launch takes its frames in the grid's z)
        const int nf = std::min(32768, n - f0);
        JDA_HIP(launch_resize(d_frames + (size_t)f0 * stride, stride, nf, width, height, hbuf + (size_t)f0 * hs, hs, hw, hh,
                              (float)(width - 1) / hw, (float)(height - 1) / hh, st));
        JDA_HIP(launch_resize(d_frames + (size_t)f0 * stride, stride, nf, width, height, qbuf + (size_t)f0 * qs, qs, qw, qh,
                              (float)(width - 1) / qw, (float)(height - 1) / qh, st));
      }
      a.half = hbuf; a.half_stride = hs; a.hw = hw; a.hh = hh;
      a.quarter = qbuf; a.quarter_stride = qs; a.qw = qw; a.qh = qh;
    }
    const int limit = multi ? 0 : windows_tile_limit(dim, m.K);
    a.tile_win = c->kn.windows_tile < 0 ? limit : (int)std::min<long long>(c->kn.windows_tile, limit);

    // per window: its four ints, the four scalars, shape and landmarks
    const size_t per = 16 + 1 + 4 + 4 + 4 + (size_t)dim * 4 * 2 + 64;
    const size_t budget = (size_t)std::max<long long>(1, c->kn.workspace_mb) << 20;
    const int nc = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n_windows, budget / per, (size_t)1 << 22}));
    int4* d_win; uint8_t* d_face; float* d_score; int* d_carts; uint32_t* d_hash; float* d_shapes; float* d_lm;
    if (!carve_into(ln->win, [&](Carver& cv) {
          d_win = cv.take<int4>(nc); d_face = cv.take<uint8_t>(nc); d_score = cv.take<float>(nc); d_carts = cv.take<int>(nc);
          d_hash = cv.take<uint32_t>(nc); d_shapes = cv.take<float>((size_t)nc * dim); d_lm = cv.take<float>((size_t)nc * dim);
        })) return false;
    std::vector<uint8_t> f(nc);
    std::vector<int> cn(nc);
    for (int i0 = 0; i0 < n_windows; i0 += nc) {
      const int cnw = std::min(nc, n_windows - i0);
      JDA_HIP(hipMemcpyAsync(d_win, windows + 4 * (size_t)i0, (size_t)cnw * sizeof(int4), hipMemcpyHostToDevice, st));
      a.windows = d_win; a.n = cnw;
      // (face and carts_n always: the statistics count them; the rest only where the caller takes it)
      a.face = d_face; a.carts_n = d_carts; a.score = out.score ? d_score : nullptr; a.hash = out.path_hash ? d_hash : nullptr;
      a.shapes = out.shapes ? d_shapes : nullptr; a.landmarks = out.landmarks ? d_lm : nullptr;
      if (!call.begin()) return false;
      JDA_HIP(launch_windows(m, a, st));
      if (!call.end()) return false;
      JDA_HIP(hipMemcpyAsync(f.data(), d_face, cnw, hipMemcpyDeviceToHost, st));
      JDA_HIP(hipMemcpyAsync(cn.data(), d_carts, (size_t)cnw * sizeof(int), hipMemcpyDeviceToHost, st));
      if (out.score) JDA_HIP(hipMemcpyAsync(out.score + i0, d_score, (size_t)cnw * sizeof(float), hipMemcpyDeviceToHost, st));
      if (out.path_hash) JDA_HIP(hipMemcpyAsync(out.path_hash + i0, d_hash, (size_t)cnw * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      if (out.shapes) JDA_HIP(hipMemcpyAsync(out.shapes + (size_t)i0 * dim, d_shapes, (size_t)cnw * dim * sizeof(float), hipMemcpyDeviceToHost, st));
      if (out.landmarks) JDA_HIP(hipMemcpyAsync(out.landmarks + (size_t)i0 * dim, d_lm, (size_t)cnw * dim * sizeof(float), hipMemcpyDeviceToHost, st));
      if (!call.sync()) return false;
      for (int i = 0; i < cnw; i++) {
        if (out.is_face) out.is_face[i0 + i] = f[i];
        if (out.carts_n) out.carts_n[i0 + i] = cn[i];
        if (f[i]) faces++; else nf_carts += cn[i];
      }
    }
    return true;
  };
  if (!call.run(out.stats != nullptr, body)) return -1;
  if (jdaStats* stats = out.stats) {     // as jdaValidateCpp fills them (mine.cpp), and the kernels' device time
    std::memset(stats, 0, sizeof *stats);
    stats->patch_n = n_windows; stats->face_patch_n = faces; stats->nonface_patch_n = n_windows - faces;
    stats->cart_gothrough_n = nf_carts;
    stats->average_cart_n = stats->nonface_patch_n ? (double)nf_carts / stats->nonface_patch_n : 0.;
    stats->gpu_ms = call.device_ms;
    stats->call_ms = call.call_ms();
  }
  return 0;
}

}  // namespace jda
