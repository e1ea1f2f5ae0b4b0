// libjda.so, host side: a call's frames over its lanes (run_device), and the shared opening of an entry (begin_call).
#pragma once
#include "pass.h"

namespace jda {

// test hook: JDA_TEST_WPF_SCALE pretends every frame has that many times more windows (the gid-overflow guard
// is otherwise only reachable with thousands of 4K frames)
inline bool jda_gid_overflow(const Knobs& kn, long long n, long long wpf) {
  const long long scale = std::max<long long>(1, kn.test_wpf_scale);
  return (double)n * (double)wpf * (double)scale > 4294967295.0;
}

// The queue capacities of a pass over `windows` windows on plan pe, from the plan's remembered fractions (read under c->mu);
// *dense: the plan's last pass kept most windows alive -- the pass will run k_stage and needs the per-window state.
inline QueueCaps plan_queue_caps(Cascador* c, PlanEntry* pe, size_t windows, bool trace, bool* dense) {
  std::lock_guard<std::mutex> lk(c->mu);
  *dense = c->kn.dense == 2 || (c->kn.dense != 0 && pe->dense_hint);
  // (k_enqueue puts every window of a level without a scan tile into the hand-off queue: the worst case is the common one)
  const bool full = trace || *dense || !pe->fast_scan || pe->any_untiled;
  return queue_caps(c->kn, windows, pe->pred_tail, pe->pred_mid, pe->pred_out, full);
}

// Frames of a call that are still in host memory: run_device copies them sub-batch by sub-batch into the staging buffer
// of the call's first lane (the copies of one sub-batch then overlap the kernels of the other lane).
struct HostFrames {
  const unsigned char* const* ptrs = nullptr;
  size_t fbytes = 0;
  // dialect C: the passes may post-process their frames on the device (RawDets::p_*), with these NMS settings
  bool device_post = false, nms = true;
  float nms_overlap = 0.3f;
  // dialect CPP, method 0 on a multi-scale model: per-window patches of these sides instead of half / quarter images
  int patch_hs = 0, patch_qs = 0;
};

// Runs the device pipeline over n frames in device memory (d_frames; with host.ptrs set they are copied there first,
// sub-batch by sub-batch).  `lanes` holds the call's first lane; a large batch takes a second one from the pool and
// is split into sub-batches that alternate between the two (streams with their own workspace), see Pass.
// A pass that fails half way (an allocation, a launch, a detection list beyond its capacity) leaves work queued on the
// lanes' streams: kernels that still read the caller's frames, copies out of the caller's host memory, writes into
// the lanes' pinned buffers.  The lanes go back to the pool and the caller may free its frames as soon as this
// returns, so everything queued is waited for first.
template <typename Real>
bool run_device(Cascador* c, LaneSet& lanes_held, PlanEntry* pe, const uint8_t* d_frames, size_t stride, int n, bool apply_th, Real th,
                hipStream_t user_stream, RawDets<Real>* dets, const TraceOut<Real>* trace, RunStats* rs, HostFrames host = HostFrames());

struct PlanPin {           // unpins on scope exit
  Cascador* c; PlanEntry* pe;
  ~PlanPin() { unpin_plan(c, pe); }
};

// The shared part of an entry, under c->mu: device, the model of dialect Real on the device, the plan (pinned).
template <typename Real>
bool begin_call(Cascador* c, const PlanKey& key, const ScanPlan& sp, int dialect, PlanEntry** pe);

}  // namespace jda
