// libjda.so, host side: detections of a batch -> per-frame results or rows (sort back into scan order is done by the pass;
// here: the worker pool of the per-frame post-processing, the driver over the frames of a batch -- the result format
// itself is results.h -- and the statistics block).  Reference: c/jda.c:237-316, 414-440.
#include "detect.h"

namespace jda {

// Host post-processing pool: a few persistent workers for the per-frame NMS + result assembly of
// a batch (0.9 us per frame, 0.22 ms per 256-frame batch when done by the calling thread alone;
// starting threads per call would cost more than that).  One job at a time; a caller that finds
// the pool busy (other cascadors on other threads) does its own work serially.
class PostPool {
 public:
  static PostPool& get() { static PostPool p; return p; }
  // A batch call announces its post-processing job ahead of time (when it starts its GPU work):
  // the workers wake up now and spin until the job arrives or `ms` have passed.
  void prewake(int n, double ms) {
    if (ms <= 0 || n < 64 || !ready_.load(std::memory_order_acquire)) return;     // off by default: measured neutral to slightly negative
    { std::lock_guard<std::mutex> lk(mu_); armed_until_.store(now_ms() + ms); }
    cv_.notify_all();
  }
  // heavy: the items are expensive (many detections per frame), worth spreading even a few of them
  void run(int n, const std::function<void(int)>& fn, bool heavy) {
    // a heavy job (thousands of detections: the per-frame NMS is quadratic) starts the workers if nobody did
    if (heavy && n >= 2 && auto_ && !ready_.load(std::memory_order_acquire)) {
      std::lock_guard<std::mutex> lk(spawn_mu_);
      if (!ready_.load(std::memory_order_acquire)) {
        const unsigned hwc = std::thread::hardware_concurrency();
        const int nw = (int)std::min<unsigned>(6, hwc > 2 ? hwc / 2 : 0);
        spawn(nw);
        if (!workers_.empty()) ready_.store(true, std::memory_order_release); else auto_ = false;
      }
    }
    const bool use = !ready_.load(std::memory_order_acquire) ? false : (heavy ? n >= 2 : n >= 64);
    if (!use || !job_mu_.try_lock()) { for (int i = 0; i < n; i++) fn(i); return; }
    auto job = std::make_shared<Job>();
    job->chunk = heavy ? 1 : 8;
    job->fn = &fn; job->n = n; job->chunks = (n + job->chunk - 1) / job->chunk;
    { std::lock_guard<std::mutex> lk(mu_); job_ = job; gen_.fetch_add(1, std::memory_order_release); }
    cv_.notify_all();
    work(*job);
    while (job->done.load(std::memory_order_acquire) < job->chunks) std::this_thread::yield();
    { std::lock_guard<std::mutex> lk(mu_); job_.reset(); armed_until_.store(0.0); }
    job_mu_.unlock();
    // an item threw on a worker (an allocation inside fn): it was caught there -- an exception that leaves a std::thread
    // body ends the process -- and is raised again here, on the caller's thread, where the C ABI's barrier turns it
    // into the entry's error value
    if (job->threw.load(std::memory_order_acquire)) throw std::bad_alloc();
  }

 private:
  struct Job {
    const std::function<void(int)>* fn = nullptr;   // valid until every chunk is done (run() waits for that)
    int n = 0, chunks = 0, chunk = 8;
    std::atomic<int> next{0}, done{0};
    std::atomic<bool> threw{false};
  };
  static void work(Job& j) {
    for (int c; (c = j.next.fetch_add(1)) < j.chunks;) {
      const int e = std::min(j.n, (c + 1) * j.chunk);
      try { for (int i = c * j.chunk; i < e; i++) (*j.fn)(i); }
      catch (...) { j.threw.store(true, std::memory_order_release); }
      j.done.fetch_add(1, std::memory_order_release);
    }
  }
  PostPool() {
    // Off by default: typically 0.22 -> 0.08 ms per 256-frame batch with 6 workers, but 1 run in ~50 on the
    // shared GPU boxes had a worker descheduled in mid-chunk (a multi-millisecond stall of the whole call);
    // the serial path is deterministic.  Opt in with JDA_POST_THREADS=6 on a quiet host.
    // JDA_POST_THREADS: -1 (default) = workers only for heavy jobs, started by the first one; 0 = never; n = n workers
    // from the start, for light jobs too (see above)
    const long long want = env_ll("JDA_POST_THREADS", -1);
    auto_ = want < 0;
    const unsigned hwc = std::thread::hardware_concurrency();
    const int nw = (int)std::max<long long>(0, std::min<long long>(want, hwc > 1 ? hwc - 1 : 0));
    spawn(nw);
    ready_.store(!workers_.empty());
  }
  // (a thread that cannot be started is not an error: the job runs on fewer workers, or serially on the caller)
  void spawn(int nw) {
    for (int i = 0; i < nw; i++) {
      try { workers_.emplace_back([this]() { loop(); }); }
      catch (const std::system_error&) { break; }
    }
  }
  ~PostPool() {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }
  void loop() {
    unsigned long long seen = 0;
    for (;;) {
      std::shared_ptr<Job> job;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&]() { return stop_ || gen_.load() != seen || now_ms() < armed_until_.load(); });
        if (stop_) return;
      }
      // armed (a batch call is in flight): stay awake until its job arrives -- a sleeping worker
      // can take longer to wake than the whole 0.2 ms job lasts
      while (gen_.load(std::memory_order_acquire) == seen && now_ms() < armed_until_.load(std::memory_order_relaxed))
        std::this_thread::yield();
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (stop_) return;
        if (gen_.load() == seen) continue;       // the arming ran out without a job
        seen = gen_.load();
        job = job_;               // may already be gone (a late wake-up): nothing to do then
      }
      if (job) work(*job);        // a finished job hands out no chunk, so its fn is never called late
    }
  }
  std::mutex mu_, job_mu_, spawn_mu_;
  bool auto_ = false;
  std::atomic<bool> ready_{false};        // workers exist
  std::condition_variable cv_;
  std::shared_ptr<Job> job_;
  std::atomic<unsigned long long> gen_{0};
  std::atomic<double> armed_until_{0.0};
  bool stop_ = false;
  std::vector<std::thread> workers_;
};

void parallel_for(int n, const std::function<void(int)>& fn, bool small_job) {
  PostPool::get().run(n, fn, !small_job);
}

void fill_stats(jdaStats* st, const RunStats& rs, long long patch_n, int T, int K, double host_ms) {
  if (!st) return;
  std::memset(st, 0, sizeof(*st));
  st->patch_n = patch_n;
  st->face_patch_n = rs.out;
  st->nonface_patch_n = patch_n - rs.out;
  st->cart_total_n = rs.carts;
  st->cart_gothrough_n = rs.carts - rs.out * (long long)T * K;   // faces walked all T*K carts
  for (int t = 0; t < T && t < 16; t++) st->stage_done_n[t] = rs.stage_done[t];
  st->average_cart_n = st->nonface_patch_n > 0 ? (double)st->cart_gothrough_n / (double)st->nonface_patch_n : 0.0;
  st->gpu_ms = rs.gpu_ms; st->scan_ms = rs.scan_ms; st->host_ms = host_ms;
  st->scan_cart_n = rs.carts_scan; st->scan_patch_n = rs.win_scan; st->scan_launches = rs.scan_launches;
  st->handoff_n = rs.tail;
  st->dense_passes = rs.dense_passes;
  st->scan_fallbacks = rs.scan_fallbacks;
  st->ws_regrows = rs.ws_regrows;
  st->post_passes = rs.post_passes; st->post_declined = rs.post_declined;
  st->scan_lds_ms = rs.scan_lds_ms; st->scan_lds_cart_n = rs.carts_scan - rs.carts_scan_glb;
}

// The statistics block of a per-image call back into the sums fill_stats made it from (the ragged job's per-image fallback)
RunStats run_stats_of(const jdaStats& st) {
  RunStats rs;
  rs.carts = st.cart_total_n; rs.out = st.face_patch_n;
  for (int t = 0; t < 16 && t < kMaxStages; t++) rs.stage_done[t] = st.stage_done_n[t];
  rs.gpu_ms = st.gpu_ms; rs.scan_ms = st.scan_ms;
  rs.carts_scan = st.scan_cart_n; rs.win_scan = st.scan_patch_n; rs.scan_launches = st.scan_launches;
  rs.tail = st.handoff_n;
  rs.dense_passes = st.dense_passes;
  rs.scan_fallbacks = st.scan_fallbacks;
  rs.ws_regrows = st.ws_regrows;
  rs.post_passes = st.post_passes; rs.post_declined = st.post_declined;
  rs.scan_lds_ms = st.scan_lds_ms; rs.carts_scan_glb = st.scan_cart_n - st.scan_lds_cart_n;
  return rs;
}

RunStats& operator+=(RunStats& a, const RunStats& b) {
  a.carts += b.carts; a.out += b.out; a.carts_scan += b.carts_scan; a.carts_scan_glb += b.carts_scan_glb;
  a.win_scan += b.win_scan; a.tail += b.tail; a.gpu_ms += b.gpu_ms; a.scan_ms += b.scan_ms; a.scan_lds_ms += b.scan_lds_ms;
  a.scan_launches += b.scan_launches; a.dense_passes += b.dense_passes; a.scan_fallbacks += b.scan_fallbacks; a.ws_regrows += b.ws_regrows;
  a.post_passes += b.post_passes; a.post_declined += b.post_declined;
  for (int t = 0; t < kMaxStages; t++) a.stage_done[t] += b.stage_done[t];
  return a;
}

template <class D>
double post_frames(const std::vector<Level>& levels, const FrameSet& fs, const RawDets<typename D::Real>& dets, int L, bool nms,
                   double overlap, const Sink<D>& sink) {
  using Real = typename D::Real;
  const double t0 = now_ms();
  const int n = fs.n, dim = 2 * L;
  const size_t nd = dets.gid.size();
  std::vector<size_t> first((size_t)n + 1);          // frame f's candidates: [first[f], first[f + 1])
  {
    size_t i = 0;
    for (int f = 0; f < n; f++) {
      first[f] = i;
      while (i < nd && (long long)dets.gid[i] < fs.gid0(f + 1)) i++;
    }
    first[n] = i;
  }
  // frames whose pass was post-processed on the device (k_post, dialect C): kept detections, relocated, in scan order,
  // rows [p_first[f], p_first[f] + p_n[f]) of p_bb (x, y, size) / p_sc / p_sh
  const bool some_posted = dets.p_n.size() == (size_t)n;
  auto posted = [&](int f) { return some_posted && dets.p_n[f] >= 0; };
  // window boxes of frame f's candidates, in scan order
  auto decode = [&](int f, int* b) {
    GidWalk walk(levels, fs.w(f), fs.h(f), (uint32_t)fs.gid0(f));
    for (size_t i = first[f]; i < first[f + 1]; i++, b += D::box) walk.box<D>(dets.gid[i], b);
  };
  if (!sink.rows) {
    parallel_for(n, [&](int f) {
      typename D::Result& r = sink.out[f];
      if (posted(f)) {
        const size_t k = (size_t)dets.p_n[f], r0 = (size_t)dets.p_first[f];
        alloc<D>(&r, k, L);
        if (k) {
          std::memcpy(D::boxes(r), &dets.p_bb[r0 * D::box], k * D::box * sizeof(int));
          std::memcpy(r.scores, &dets.p_sc[r0], k * sizeof(Real));
          std::memcpy(r.shapes, &dets.p_sh[r0 * dim], k * dim * sizeof(Real));
        }
        return;
      }
      const size_t a = first[f], cnt = first[f + 1] - a;
      static thread_local std::vector<int> boxes;          // per-frame scratch, grown once per thread
      boxes.resize(cnt * D::box);
      decode(f, boxes.data());
      emit<D>(boxes.data(), dets.score.data() + a, dets.shape.data() + a * dim, (int)cnt, L, nms, overlap, &r);
    }, nd < 6000);
    return now_ms() - t0;
  }
  // rows, no result structs in between (a 2,845-image dialect-CPP job keeps 15 MB of rows).  A frame's picks (NMS) go
  // where its candidates are; pick_frame returns how many rows it has, write_frame writes them from o on.
  std::vector<int> boxes(nd * D::box), picks(nd);
  auto pick_frame = [&](int f) -> size_t {
    if (posted(f)) return (size_t)dets.p_n[f];
    const size_t a = first[f], cnt = first[f + 1] - a;
    static thread_local std::vector<int> keep;
    decode(f, boxes.data() + a * D::box);
    pick<D>(boxes.data() + a * D::box, dets.score.data() + a, (int)cnt, nms, overlap, &keep);
    std::copy(keep.begin(), keep.end(), picks.begin() + a);
    return keep.size();
  };
  const size_t rw = (size_t)D::head + dim;
  auto write_frame = [&](int f, Real* o, size_t k) {
    const int frame = sink.frame_offset + f;
    if (posted(f)) {
      for (size_t j = (size_t)dets.p_first[f]; j < (size_t)dets.p_first[f] + k; j++)
        o = write_row<D>(o, frame, &dets.p_bb[j * D::box], dets.p_sc[j], &dets.p_sh[j * dim], dim);
      return;
    }
    const size_t a = first[f];
    write_rows<D>(o, frame, boxes.data() + a * D::box, dets.score.data() + a, dets.shape.data() + a * dim, picks.data() + a, k, L);
  };
  if (!D::parallel_rows) {             // frame after frame on the calling thread, rows appended
    for (int f = 0; f < n; f++) {
      const size_t k = pick_frame(f);
      write_frame(f, sink.rows->grow(k * rw), k);
    }
    return now_ms() - t0;
  }
  // NMS per frame in parallel, then every frame's rows written in place, in parallel
  std::vector<size_t> row0((size_t)n + 1, 0);
  parallel_for(n, [&](int f) { row0[(size_t)f + 1] = pick_frame(f); }, nd < 6000);
  for (int f = 0; f < n; f++) row0[(size_t)f + 1] += row0[f];
  Real* base = sink.rows->grow(row0[n] * rw);
  parallel_for(n, [&](int f) { write_frame(f, base + row0[f] * rw, row0[(size_t)f + 1] - row0[f]); }, row0[n] < 2000);
  return now_ms() - t0;
}
template double post_frames<DialectC>(const std::vector<Level>&, const FrameSet&, const RawDets<float>&, int, bool, double, const Sink<DialectC>&);
template double post_frames<DialectCpp>(const std::vector<Level>&, const FrameSet&, const RawDets<double>&, int, bool, double, const Sink<DialectCpp>&);

}  // namespace jda
