// libjda.so, host side: dialect CPP (the fp64 `src/jda` path), detect method 1 -- the growing window of
// detectMultiScale1 (reference src/jda/cascador.cpp:310-376) followed by Detect's NMS and relocation (431-477) -- on a
// batch of equally sized frames, in host memory or resident on the device.
#include "detect.h"

namespace jda {

int detect_cpp_device(Cascador* c, const uint8_t* d_frames, size_t stride, int n, int width, int height, const CppCall& call,
                      jdaStats* stats, jdaResultD* out, const unsigned char* const* host_frames) {
  const double t_call = now_ms();
  if (!c || !out || n < 0 || (!d_frames && !host_frames && n > 0)) { fail("bad arguments"); return -1; }
  OutGuard<DialectCpp> guard(out, n, c->hm.L);
  if (!cpp_model_complete(c)) return -1;
  ScanPlan sp; std::string err;
  if (!plan_dialect_cpp(width, height, call.minimum_size, call.step, call.factor, &sp, &err)) { fail(err); return -1; }
  if (!host_frames && stride < (size_t)width * height) { fail("frame_stride smaller than a frame"); return -1; }
  unsigned long long fb; std::memcpy(&fb, &call.factor, 8);
  PlanKey key{width, height, JDA_DIALECT_CPP, call.minimum_size, call.step, c->similarity, fb};
  PlanEntry* pe = nullptr;
  if (!begin_call<double>(c, key, sp, JDA_DIALECT_CPP, &pe)) return -1;
  PlanPin pin{c, pe};
  LaneSet lanes(c);
  HostFrames host;
  if (host_frames) {
    if (!lanes.take(1) || !stage_frames(lanes.v[0], host_frames, n, (size_t)width * height, &stride, true)) return -1;
    d_frames = (const uint8_t*)lanes.v[0]->frames.p;
    host.ptrs = host_frames; host.fbytes = (size_t)width * height;
  }
  RawDets<double> dets;
  RunStats rs;
  rs.timed = stats != nullptr;
  if (!run_device<double>(c, lanes, pe, d_frames, stride, n, false, 0.0, nullptr, &dets, nullptr, &rs, host)) return -1;
  const double post_ms = post_frames<DialectCpp>(sp.levels, FrameSet{n, sp.windows, sp.width, sp.height}, dets, c->hm.L, call.nms != 0, call.overlap,
                                                 Sink<DialectCpp>{out});
  fill_stats(stats, rs, sp.windows * n, c->hm.T, c->hm.K, post_ms);
  if (stats) stats->call_ms = now_ms() - t_call;
  guard.keep = true;
  return 0;
}

}  // namespace jda
