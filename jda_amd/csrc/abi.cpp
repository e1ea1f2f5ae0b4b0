// libjda.so: the extern "C" entry points of include/jda.h (reference interface: c/jda.h:18-68) and of the batch,
// trace and dialect-CPP extensions, on top of detect.cpp / tickets.cpp / ragged.cpp.
#include "detect.h"
#include "frames.h"

// =============================================================================
// C ABI
// =============================================================================

using namespace jda;

namespace {
// test hook (option test_throw; tests/test_abi.py): 1 = std::bad_alloc, 2 = std::runtime_error inside the entry
void maybe_throw(const Cascador* c) {
  if (c->kn.test_throw == 1) throw std::bad_alloc();
  if (c->kn.test_throw == 2) throw std::runtime_error("injected by test_throw");
}
// rows of a job -> the caller: the buffer itself, not a copy
template <class D>
int rows_out(Cascador* c, int rc, RowsOut<typename D::Real>& v, typename D::Real** rows, int* n_rows) {
  *rows = nullptr; *n_rows = 0;
  if (rc != 0) return rc;
  *n_rows = (int)(v.n / ((size_t)D::head + c->hm.dim()));
  *rows = v.release();
  if (!*rows) { *n_rows = 0; fail("out of memory for the detection rows"); return -1; }
  return 0;
}
// One launch report (host.h: LaunchLog) -> the caller's array.
template <int N>
int launch_report(const char* who, void* cascador, std::atomic<long long> (LaunchLog::*report)[N], long long* counts) {
  Cascador* c = (Cascador*)cascador;
  if (!c || !counts) { fail(std::string(who) + ": null cascador or counts"); return -1; }
  LaunchLog::copy_out(c->log.*report, counts);
  return 0;
}
}  // namespace

extern "C" {

const char* jdaGetLastError(void) { return g_err.c_str(); }

static void* create_impl(const char* path, int real_bytes) {
  Cascador* c = nullptr;
  try {
    g_err.clear();
    c = new Cascador();
    c->kn.load();
    std::string err;
    if (!load_model(path, real_bytes, &c->hm, &err)) {
      g_err = err;   // reference returns NULL silently (c/jda.c:487-488); keep the reason retrievable
      delete c;
      return nullptr;
    }
    return c;
  } catch (...) {      // malloc failure: NULL like the reference (c/jda.c:489-493)
    abi_exception("jdaCascadorCreate", false);
    delete c;
    return nullptr;
  }
}

void* jdaCascadorCreateDouble(const char* model) { return create_impl(model, 8); }
void* jdaCascadorCreateFloat(const char* model) { return create_impl(model, 4); }
void* jdaCascadorCreate(const char* model) { return create_impl(model, 0); }

void jdaCascadorSerializeTo(void* cascador, const char* model) try {
  if (!cascador) return;
  (void)save_model_f32(((Cascador*)cascador)->hm, model);
} JDA_ABI_CATCH_VOID

void* jdaCascadorCreateTrainingCpp(int T, int K, int landmark_n, int tree_depth, const double* mean_shape) {
  try {
    g_err.clear();
    return grow_create(T, K, landmark_n, tree_depth, mean_shape);
  } catch (...) {      // the tables of a big model did not fit: NULL like jdaCascadorCreate
    abi_exception("jdaCascadorCreateTrainingCpp", false);
    return nullptr;
  }
}

int jdaModelStatusCpp(void* cascador, int* stage, int* cart) try {
  g_err.clear();
  return grow_status((Cascador*)cascador, stage, cart);
} JDA_ABI_CATCH(-1)

int jdaModelPutCartCpp(void* cascador, int k, const jdaFeatureCpp* features, const int* thresholds, const double* leaf_scores,
                       double th, double mean, double std) try {
  g_err.clear();
  return grow_put_cart((Cascador*)cascador, k, features, thresholds, leaf_scores, th, mean, std);
} JDA_ABI_CATCH(-1)

int jdaModelCloseStageCpp(void* cascador, const double* w) try {
  g_err.clear();
  return grow_close_stage((Cascador*)cascador, w);
} JDA_ABI_CATCH(-1)

int jdaValidateSamplesCpp(void* cascador, const jdaSamplesCpp* samples, int origin_size, int half_size, int quarter_size,
                          unsigned char* is_face, double* score, int* carts_n, double* shape, jdaStageStatsCpp* stats) try {
  g_err.clear();
  return reval_entry((Cascador*)cascador, samples, origin_size, half_size, quarter_size, is_face, score, carts_n, shape, stats);
} JDA_ABI_CATCH_SYNC(-1)

int jdaCascadorSerializeToCpp(void* cascador, const char* path) try {
  g_err.clear();
  return grow_serialize((Cascador*)cascador, path);
} JDA_ABI_CATCH(-1)

void jdaCascadorRelease(void* cascador) try {
  Cascador* c = (Cascador*)cascador;
  if (!c) return;
  // Submitted batches nobody waited for are drained here (their helper threads joined, their streams synchronised by
  // Lane::destroy).  A call still running on another thread is the caller's error, as with the reference, whose
  // release frees what jdaDetect reads (c/jda.c:718-720); such a call is given ten seconds to return before the
  // lanes go -- a race at shutdown then ends in a late but orderly release instead of a use-after-free.
  for (int i = 0; c->pending && i < kTickets; i++) c->pending[i].join_issuer();
  {
    std::unique_lock<std::mutex> lk(c->mu);
    for (int i = 0; c->pending && i < kTickets; i++)
      if (c->pending[i].active && c->pending[i].lane) { c->pending[i].lane->busy = false; c->pending[i].active = false; }
    c->lane_cv.wait_for(lk, std::chrono::seconds(10), [&]() {
      for (auto& l : c->lanes) if (l->busy) return false;
      return true;
    });
  }
  if (c->dev_init) {
    (void)hipSetDevice(c->device);
    for (auto& l : c->lanes) l->destroy();
    c->streams.destroy();        // (aux, the upload stream and the lanes' streams are the pool's)
    c->aux = c->h2d = nullptr;
    for (auto& kv : c->plans) { if (kv.second.dp) (void)hipFree(kv.second.dp); if (kv.second.table) (void)hipFree(kv.second.table); }
    for (auto& b : c->plan_pool) { if (b.dp) (void)hipFree(b.dp); if (b.table) (void)hipFree(b.table); }
    c->mf.buf.release(); c->md.buf.release(); c->mine_buf.release();
  }
  delete[] c->pending;
  delete c;
} JDA_ABI_CATCH_VOID

int jdaCascadorInfo(void* cascador, jdaModelInfo* info) try {
  if (!cascador || !info) return -1;
  const HostModel& h = ((Cascador*)cascador)->hm;
  info->T = h.T; info->K = h.K; info->landmark_n = h.L; info->tree_depth = h.D;
  info->multi_scale = h.multi_scale() ? 1 : 0; info->source_real_bytes = h.real_bytes;
  return 0;
} JDA_ABI_CATCH(-1)

int jdaSetSimilarityTransform(void* cascador, int on) try {
  Cascador* c = (Cascador*)cascador;
  if (!c) return -1;
  std::lock_guard<std::mutex> lock(c->mu);
  for (auto& l : c->lanes)
    if (l->busy) { fail("jdaSetSimilarityTransform while a call is running on this cascador"); return -1; }
  on = on ? 1 : 0;
  if (c->similarity != on) {
    c->similarity = on;
    c->md.ready = false;          // the fp64 node table depends on it (stage-0 offsets carry the transform)
  }
  return 0;
} JDA_ABI_CATCH(-1)

int jdaSetDevice(void* cascador, int device) try {
  Cascador* c = (Cascador*)cascador;
  if (!c) return -1;
  std::lock_guard<std::mutex> lock(c->mu);
  if (c->dev_init && c->device != device) { fail("jdaSetDevice after first use"); return -1; }
  c->device = device;
  return 0;
} JDA_ABI_CATCH(-1)

int jdaSetOption(void* cascador, const char* key, long long value) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !key) { fail("jdaSetOption: null cascador or key"); return -1; }
  std::lock_guard<std::mutex> lock(c->mu);
  for (auto& l : c->lanes)
    if (l->busy) { fail("jdaSetOption while a call is running or a submitted batch is pending on this cascador"); return -1; }
  for (auto& kv : c->plans)
    if (kv.second.pins) { fail("jdaSetOption while a call is running on this cascador"); return -1; }
  if (!c->kn.set(key, value)) { fail(std::string("jdaSetOption: unknown option or value out of range: '") + key + "'"); return -1; }
  // scan plans (tile shapes, table chunking) depend on the knobs: rebuild them on next use (no lane is busy, so
  // nothing runs on the old ones)
  for (auto& kv : c->plans) c->plan_pool.push_back({kv.second.dp, kv.second.table, kv.second.table_cap});
  c->plans.clear();
  return 0;
} JDA_ABI_CATCH(-1)

long long jdaGetOption(void* cascador, const char* key) try {
  Cascador* c = (Cascador*)cascador;
  long long v = 0;
  if (c && key && std::strncmp(key, "hwq_", 4) == 0 && std::strcmp(key, "hwq_place") != 0) {
    // read-only: what the stream pool found (host.h: StreamPool) -- hardware queues known, streams created, probes run,
    // and the most main streams of busy-or-free lanes that share one queue
    std::lock_guard<std::mutex> lk(c->streams.mu);
    if (std::strcmp(key, "hwq_queues") == 0) return (long long)c->streams.rep.size();
    if (std::strcmp(key, "hwq_streams") == 0) return c->streams.created;
    if (std::strcmp(key, "hwq_probes") == 0) return c->streams.probes;
    if (std::strcmp(key, "hwq_max_mains") == 0) { int m = 0; for (int x : c->streams.mains) m = std::max(m, x); return m; }
  }
  // read-only: the largest window side k_windows walks from an LDS copy of the window's pixels with this model (0: none)
  if (c && key && std::strcmp(key, "windows_tile_limit") == 0) {
    std::lock_guard<std::mutex> lk(c->mu);             // (multi_scale() caches its answer in the model on first use)
    return c->hm.multi_scale() ? 0 : windows_tile_limit(c->hm.dim(), c->hm.K);
  }
  if (c && key && std::strncmp(key, "mem_", 4) == 0) {
    // read-only: what the cascador holds on the device -- bytes of its model tables (both dialects' and the mining tables) and
    // of its lanes' buffers, all grow-only, and the plan buffers in the plan map and the pool together (a test of "nothing
    // leaks" compares them across rounds)
    std::lock_guard<std::mutex> lk(c->mu);
    if (std::strcmp(key, "mem_device_bytes") == 0) {
      size_t b = c->mf.buf.bytes + c->md.buf.bytes + c->mine_buf.bytes;
      for (auto& l : c->lanes) b += l->ws.bytes + l->frames.bytes + l->pyr.bytes + l->win.bytes + l->rag_frames.bytes + l->rag_raw.bytes + l->rag_tab.bytes;
      return (long long)b;
    }
    if (std::strcmp(key, "mem_plan_buffers") == 0) return (long long)(c->plans.size() + c->plan_pool.size());
  }
  if (!c || !key || !c->kn.get(key, &v)) { fail("jdaGetOption: unknown option"); return -1; }
  return v;
} JDA_ABI_CATCH(-1)

int jdaFinishForms(void* cascador, long long counts[JDA_FINISH_FORM_N]) try {
  return launch_report("jdaFinishForms", cascador, &LaunchLog::finish_forms, counts);
} JDA_ABI_CATCH(-1)

int jdaScanForms(void* cascador, long long counts[JDA_SCAN_FORM_N]) try {
  return launch_report("jdaScanForms", cascador, &LaunchLog::scan_forms, counts);
} JDA_ABI_CATCH(-1)

int jdaFinishLaunches(void* cascador, long long counts[JDA_FINISH_LAUNCH_N]) try {
  return launch_report("jdaFinishLaunches", cascador, &LaunchLog::finish_launches, counts);
} JDA_ABI_CATCH(-1)

int jdaFinishTileWin(void* cascador, int dialect) try {
  Cascador* c = (Cascador*)cascador;
  if (!c || (dialect != JDA_DIALECT_C && dialect != JDA_DIALECT_CPP)) { fail("jdaFinishTileWin: null cascador or unknown dialect"); return -1; }
  std::lock_guard<std::mutex> lk(c->mu);             // (multi_scale() caches its answer in the model on first use)
  const int real_bytes = dialect == JDA_DIALECT_C ? 4 : 8;
  // (what launch_finish decides with fin_tile = -1: the same function on the same model -- dialect CPP's DevModelT::similarity
  // is nonzero exactly where the cascador's is)
  return finish_tile_win(c->hm.dim(), c->hm.K, real_bytes, finish_st(real_bytes, c->similarity), c->hm.multi_scale(), -1);
} JDA_ABI_CATCH(-1)

int jdaStageLaunches(void* cascador, long long counts[JDA_STAGE_LAUNCH_N]) try {
  return launch_report("jdaStageLaunches", cascador, &LaunchLog::stage_launches, counts);
} JDA_ABI_CATCH(-1)

int jdaMineLaunches(void* cascador, long long counts[JDA_MINE_LAUNCH_N]) try {
  return launch_report("jdaMineLaunches", cascador, &LaunchLog::mine_launches, counts);
} JDA_ABI_CATCH(-1)

int jdaStageLaunchFor(void* cascador, int dialect, int trace, int win, int step, int* lds_bytes) try {
  Cascador* c = (Cascador*)cascador;
  if (!c || (dialect != JDA_DIALECT_C && dialect != JDA_DIALECT_CPP) || win < 1 || step < 1) {
    fail("jdaStageLaunchFor: null cascador, unknown dialect, or a window or step below 1"); return -1;
  }
  std::lock_guard<std::mutex> lk(c->mu);             // (multi_scale() caches its answer in the model on first use)
  // (what Pass::dense_ok and launch_stage would decide: their functions, on the same model and the same constants, without a device)
  const int real_bytes = dialect == JDA_DIALECT_C ? 4 : 8, lds_max = (int)Knobs::dense_lds_max;
  int pix_cap = 0;
  if (c->hm.multi_scale() || (dialect == JDA_DIALECT_CPP && c->similarity) ||
      !stage_model_ok(c->hm.dim(), c->hm.node_n(), c->hm.leaf_n(), real_bytes, (int)Knobs::dense_pix, lds_max, &pix_cap)) return -1;
  const StageChoice sc = stage_choice(win, step, c->hm.dim(), c->hm.node_n(), c->hm.leaf_n(), c->hm.K, real_bytes, pix_cap, lds_max);
  if (sc.chunk == 0) return -1;
  if (lds_bytes) *lds_bytes = sc.lds_bytes;
  return stage_launch_key(dialect, trace != 0, sc);
} JDA_ABI_CATCH(-1)

int jdaCountWindows(int width, int height, float scale, int min_size, int max_size,
                    long long* n_windows, int* n_levels) try {
  ScanPlan sp; std::string err;
  if (!plan_dialect_c(width, height, scale, min_size, max_size, &sp, &err)) { g_err = err; return -1; }
  if (n_windows) *n_windows = sp.windows;
  if (n_levels) *n_levels = (int)sp.levels.size();
  return 0;
} JDA_ABI_CATCH(-1)

void jdaDetectOptionsInit(jdaDetectOptions* opt) try {
  if (!opt) return;
  std::memset(opt, 0, sizeof(*opt));
  opt->dialect = JDA_DIALECT_C; opt->nms = 1; opt->nms_overlap = 0.3f; opt->cpp_step = 5;
} JDA_ABI_CATCH_VOID

int jdaDetectBatchDevice(void* cascador, const unsigned char* d_frames, size_t frame_stride, int n,
                         int width, int height, float scale, float step, int min_size, int max_size,
                         float th, const jdaDetectOptions* opt, jdaResult* out) try {
  (void)step;  // ignored like the reference (c/jda.c:333)
  g_err.clear();
  if (opt && opt->dialect != JDA_DIALECT_C) { fail("jdaDetectBatchDevice runs dialect C; use jdaDetectBatchCpp"); return -1; }
  if (!cascador) { fail("null cascador"); return -1; }
  return detect_c_device((Cascador*)cascador, d_frames, frame_stride, n, width, height, scale, min_size, max_size, th, opt, out);
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchSubmit(void* cascador, const unsigned char* d_frames, size_t frame_stride, int n,
                         int width, int height, float scale, float step, int min_size, int max_size,
                         float th, const jdaDetectOptions* opt) try {
  (void)step;
  g_err.clear();
  if (opt && opt->dialect != JDA_DIALECT_C) { fail("jdaDetectBatchSubmit runs dialect C"); return -1; }
  if (!cascador) { fail("null cascador"); return -1; }
  Cascador* c = (Cascador*)cascador;
  return submit_c_device(c, d_frames, frame_stride, n, width, height, scale, min_size, max_size, th, opt);
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchSubmitHost(void* cascador, const unsigned char* const* frames, int n, int width, int height,
                             float scale, float step, int min_size, int max_size, float th,
                             const jdaDetectOptions* opt) try {
  (void)step;
  g_err.clear();
  if (opt && opt->dialect != JDA_DIALECT_C) { fail("jdaDetectBatchSubmitHost runs dialect C"); return -1; }
  if (!cascador || !frames) { fail("null cascador or frames"); return -1; }
  if (width <= 0 || height <= 0) { fail("frame has no pixels"); return -1; }
  Cascador* c = (Cascador*)cascador;
  return submit_c_device(c, nullptr, 0, n, width, height, scale, min_size, max_size, th, opt, frames);
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchWait(void* cascador, int ticket, jdaStats* stats, jdaResult* out) try {
  g_err.clear();
  if (!cascador) { fail("null cascador"); return -1; }
  Cascador* c = (Cascador*)cascador;
  return wait_c_device(c, ticket, stats, out);
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatch(void* cascador, const unsigned char* const* frames, int n, int width, int height,
                   float scale, float step, int min_size, int max_size, float th,
                   const jdaDetectOptions* opt, jdaResult* out) try {
  (void)step;
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !frames || !out || n < 0) { fail("bad arguments"); return -1; }
  if (width <= 0 || height <= 0) { fail("frame has no pixels"); return -1; }
  for (int i = 0; i < n; i++) if (!frames[i]) { fail("null frame pointer"); return -1; }
  maybe_throw(c);
  return detect_c_device(c, nullptr, 0, n, width, height, scale, min_size, max_size, th, opt, out, frames);
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchRagged(void* cascador, const unsigned char* const* images, const int* widths, const int* heights, int n,
                         float scale, float step, int min_size, int max_size, float th,
                         const jdaDetectOptions* opt, jdaResult* out) try {
  (void)step;
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !images || !widths || !heights || !out || n < 0) { fail("bad arguments"); return -1; }
  if (opt && opt->dialect != JDA_DIALECT_C) { fail("jdaDetectBatchRagged runs dialect C"); return -1; }
  return detect_ragged(c, images, nullptr, nullptr, widths, heights, n, scale, min_size, max_size, th, opt, Sink<DialectC>{out});
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchRaggedDevice(void* cascador, const unsigned char* d_base, const size_t* offsets, const int* widths,
                               const int* heights, int n, float scale, float step, int min_size, int max_size, float th,
                               const jdaDetectOptions* opt, jdaResult* out) try {
  (void)step;
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !d_base || !offsets || !widths || !heights || !out || n < 0) { fail("bad arguments"); return -1; }
  if (opt && opt->dialect != JDA_DIALECT_C) { fail("jdaDetectBatchRaggedDevice runs dialect C"); return -1; }
  return detect_ragged(c, nullptr, d_base, offsets, widths, heights, n, scale, min_size, max_size, th, opt, Sink<DialectC>{out});
} JDA_ABI_CATCH_SYNC(-1)


int jdaDetectBatchRaggedRows(void* cascador, const unsigned char* const* images, const int* widths, const int* heights, int n,
                             float scale, float step, int min_size, int max_size, float th, const jdaDetectOptions* opt,
                             int frame_offset, float** rows, int* n_rows) try {
  (void)step;
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !images || !widths || !heights || !rows || !n_rows || n < 0) { fail("bad arguments"); return -1; }
  if (opt && opt->dialect != JDA_DIALECT_C) { fail("jdaDetectBatchRaggedRows runs dialect C"); return -1; }
  RowsOut<float> v;
  const int rc = detect_ragged(c, images, nullptr, nullptr, widths, heights, n, scale, min_size, max_size, th, opt, Sink<DialectC>{nullptr, &v, frame_offset});
  return rows_out<DialectC>(c, rc, v, rows, n_rows);
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchRaggedDeviceRows(void* cascador, const unsigned char* d_base, const size_t* offsets, const int* widths,
                                   const int* heights, int n, float scale, float step, int min_size, int max_size, float th,
                                   const jdaDetectOptions* opt, int frame_offset, float** rows, int* n_rows) try {
  (void)step;
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !d_base || !offsets || !widths || !heights || !rows || !n_rows || n < 0) { fail("bad arguments"); return -1; }
  if (opt && opt->dialect != JDA_DIALECT_C) { fail("jdaDetectBatchRaggedDeviceRows runs dialect C"); return -1; }
  RowsOut<float> v;
  const int rc = detect_ragged(c, nullptr, d_base, offsets, widths, heights, n, scale, min_size, max_size, th, opt, Sink<DialectC>{nullptr, &v, frame_offset});
  return rows_out<DialectC>(c, rc, v, rows, n_rows);
} JDA_ABI_CATCH_SYNC(-1)

void jdaRowsRelease(float* rows) { std::free(rows); }

jdaResult jdaDetect(void* cascador, unsigned char* data, int width, int height,
                    float scale, float step, int min_size, int max_size, float th) {
  Cascador* c = (Cascador*)cascador;
  jdaResult r;
  blank<DialectC>(&r, c ? c->hm.L : 0);
  try {
    if (!c || !data) { fail("jdaDetect: null cascador or image"); return empty_result<DialectC>(r.landmark_n); }
    const unsigned char* frames[1] = {data};
    if (jdaDetectBatch(cascador, frames, 1, width, height, scale, step, min_size, max_size, th, nullptr, &r) != 0)
      return empty_result<DialectC>(c->hm.L);        // (r is blank: a failed call leaves nothing allocated)
    return r;
  } catch (...) {      // (jdaDetectBatch has its own barrier; what is left is the error string and empty_result; r is blank)
    abi_exception("jdaDetect", false);
    return r;
  }
}

void jdaResultRelease(jdaResult result) { release<DialectC>(&result); }

int jdaTraceBatch(void* cascador, const unsigned char* const* frames, int n, int width, int height,
                  float scale, int min_size, int max_size, int* carts_n, float* score,
                  unsigned int* path_hash, float* shapes) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !frames || n < 0) { fail("bad arguments"); return -1; }
  ScanPlan sp; std::string err;
  if (!plan_dialect_c(width, height, scale, min_size, max_size, &sp, &err)) { fail(err); return -1; }
  unsigned sb; std::memcpy(&sb, &scale, 4);
  PlanKey key{width, height, JDA_DIALECT_C, (int)sb, std::max(min_size, 24), max_size <= 0 ? -1 : max_size, 0ull};
  PlanEntry* pe = nullptr;
  if (!begin_call<float>(c, key, sp, JDA_DIALECT_C, &pe)) return -1;
  PlanPin pin{c, pe};
  LaneSet lanes(c);
  size_t stride = 0;
  if (!lanes.take(1) || !stage_frames(lanes.v[0], frames, n, (size_t)width * height, &stride, true)) return -1;
  TraceOut<float> tr{carts_n, score, path_hash, shapes};
  RunStats rs;
  if (!run_device<float>(c, lanes, pe, (const uint8_t*)lanes.v[0]->frames.p, stride, n, false, 0.f, nullptr, nullptr, &tr, &rs,
                         HostFrames{frames, (size_t)width * height})) return -1;
  return 0;
} JDA_ABI_CATCH_SYNC(-1)

int jdaValidateWindows(void* cascador, const unsigned char* const* frames, int n, int width, int height, const int* windows,
                       int n_windows, float th, unsigned char* is_face, float* score, int* carts_n, unsigned int* path_hash,
                       float* shapes, float* landmarks, jdaStats* stats) try {
  g_err.clear();
  return windows_entry((Cascador*)cascador, "jdaValidateWindows", frames, nullptr, 0, n, width, height, windows, n_windows, th,
                       WindowsOut{is_face, score, carts_n, path_hash, shapes, landmarks, stats});
} JDA_ABI_CATCH_SYNC(-1)

int jdaValidateWindowsDevice(void* cascador, const unsigned char* d_frames, size_t frame_stride, int n, int width, int height,
                             const int* windows, int n_windows, float th, unsigned char* is_face, float* score, int* carts_n,
                             unsigned int* path_hash, float* shapes, float* landmarks, jdaStats* stats) try {
  g_err.clear();
  return windows_entry((Cascador*)cascador, "jdaValidateWindowsDevice", nullptr, d_frames, frame_stride, n, width, height, windows,
                       n_windows, th, WindowsOut{is_face, score, carts_n, path_hash, shapes, landmarks, stats});
} JDA_ABI_CATCH_SYNC(-1)

int jdaPackGray(const jdaPixels* images, int n, unsigned char* dst, const size_t* dst_offsets) try {
  g_err.clear();
  return frames_host(FrameSpec::pack(), images, n, dst, dst_offsets);
} JDA_ABI_CATCH(-1)

int jdaPackGrayDevice(void* cascador, const jdaPixels* images, int n, unsigned char* d_dst, const size_t* dst_offsets,
                      void* hip_stream, jdaPackStats* stats) try {
  g_err.clear();
  return frames_device((Cascador*)cascador, FrameSpec::pack(), images, n, d_dst, dst_offsets, (hipStream_t)hip_stream, stats);
} JDA_ABI_CATCH_SYNC(-1)

int jdaOrientSize(int w, int h, int orient, int* tw, int* th) try {
  g_err.clear();
  return orient_size(w, h, orient, tw, th);
} JDA_ABI_CATCH(-1)

int jdaPackGrayOriented(const jdaPixels* images, const int* orients, int n, unsigned char* dst, const size_t* dst_offsets) try {
  g_err.clear();
  return frames_host(FrameSpec::turn(orients), images, n, dst, dst_offsets);
} JDA_ABI_CATCH(-1)

int jdaPackGrayOrientedDevice(void* cascador, const jdaPixels* images, const int* orients, int n, unsigned char* d_dst,
                              const size_t* dst_offsets, void* hip_stream, jdaPackStats* stats) try {
  g_err.clear();
  return frames_device((Cascador*)cascador, FrameSpec::turn(orients), images, n, d_dst, dst_offsets, (hipStream_t)hip_stream, stats);
} JDA_ABI_CATCH_SYNC(-1)

int jdaOrientBack(const jdaPixels* images, const int* orients, int n_images, const int* face_image, int n_faces, int* boxes,
                  int box_ints, void* landmarks, int real_bytes, int landmark_n, const int* left, const int* right, int sym_n) try {
  g_err.clear();
  return frames_back(FrameSpec::turn(orients), BackCall{images, n_images, face_image, n_faces, boxes, box_ints, landmarks, real_bytes,
                                                       landmark_n, left, right, sym_n});
} JDA_ABI_CATCH(-1)

int jdaReduceSize(int w, int h, int factor, int orient, int* rw, int* rh) try {
  g_err.clear();
  return reduce_size(w, h, factor, orient, rw, rh);
} JDA_ABI_CATCH(-1)

int jdaPackGrayReduced(const jdaPixels* images, const int* factors, const int* orients, int n, unsigned char* dst,
                       const size_t* dst_offsets) try {
  g_err.clear();
  return frames_host(FrameSpec::reduce(factors, orients), images, n, dst, dst_offsets);
} JDA_ABI_CATCH(-1)

int jdaPackGrayReducedDevice(void* cascador, const jdaPixels* images, const int* factors, const int* orients, int n,
                             unsigned char* d_dst, const size_t* dst_offsets, void* hip_stream, jdaPackStats* stats) try {
  g_err.clear();
  return frames_device((Cascador*)cascador, FrameSpec::reduce(factors, orients), images, n, d_dst, dst_offsets, (hipStream_t)hip_stream, stats);
} JDA_ABI_CATCH_SYNC(-1)

int jdaReduceBack(const jdaPixels* images, const int* factors, const int* orients, int n_images, const int* face_image, int n_faces,
                  int* boxes, int box_ints, void* landmarks, int real_bytes, int landmark_n, const int* left, const int* right,
                  int sym_n) try {
  g_err.clear();
  return frames_back(FrameSpec::reduce(factors, orients), BackCall{images, n_images, face_image, n_faces, boxes, box_ints, landmarks,
                                                                   real_bytes, landmark_n, left, right, sym_n});
} JDA_ABI_CATCH(-1)

int jdaRotationPlan(int w, int h, double degrees, jdaRotation* rot) try {
  g_err.clear();
  return rotation_plan("jdaRotationPlan: ", w, h, degrees, rot) ? 0 : -1;
} JDA_ABI_CATCH(-1)

int jdaPackGrayRotated(const jdaPixels* images, const double* degrees, int n, unsigned char* dst, const size_t* dst_offsets) try {
  g_err.clear();
  return frames_host(FrameSpec::rotate(degrees), images, n, dst, dst_offsets);
} JDA_ABI_CATCH(-1)

int jdaPackGrayRotatedDevice(void* cascador, const jdaPixels* images, const double* degrees, int n, unsigned char* d_dst,
                             const size_t* dst_offsets, void* hip_stream, jdaPackStats* stats) try {
  g_err.clear();
  return frames_device((Cascador*)cascador, FrameSpec::rotate(degrees), images, n, d_dst, dst_offsets, (hipStream_t)hip_stream, stats);
} JDA_ABI_CATCH_SYNC(-1)

int jdaRotateBack(const jdaPixels* images, const double* degrees, int n_images, const int* face_image, int n_faces, int* boxes,
                  int box_ints, void* landmarks, int real_bytes, int landmark_n) try {
  g_err.clear();
  return frames_back(FrameSpec::rotate(degrees), BackCall{images, n_images, face_image, n_faces, boxes, box_ints, landmarks, real_bytes,
                                                          landmark_n, nullptr, nullptr, 0});
} JDA_ABI_CATCH(-1)

int jdaFaceChips(const jdaPixels* images, int n_images, const int* face_image, const void* landmarks, int real_bytes, int n_faces,
                 int landmark_n, const double* tmpl, const unsigned char* use, int chip_w, int chip_h, int chip_format, int supersample,
                 unsigned char* dst, double* matrices) try {
  g_err.clear();
  return chips_host(ChipsCall{images, n_images, face_image, landmarks, real_bytes, n_faces, landmark_n, tmpl, use, chip_w, chip_h,
                              chip_format, supersample, dst, matrices});
} JDA_ABI_CATCH(-1)

int jdaFaceChipsDevice(void* cascador, const jdaPixels* images, int n_images, const int* face_image, const void* landmarks,
                       int real_bytes, int n_faces, int landmark_n, const double* tmpl, const unsigned char* use, int chip_w,
                       int chip_h, int chip_format, int supersample, unsigned char* d_dst, double* matrices, void* hip_stream,
                       jdaChipStats* stats) try {
  g_err.clear();
  return chips_device((Cascador*)cascador, ChipsCall{images, n_images, face_image, landmarks, real_bytes, n_faces, landmark_n, tmpl, use,
                                                     chip_w, chip_h, chip_format, supersample, d_dst, matrices},
                      (hipStream_t)hip_stream, stats);
} JDA_ABI_CATCH_SYNC(-1)

int jdaCascadorMeanShape(void* cascador, double* mean_shape) try {
  g_err.clear();
  if (!cascador || !mean_shape) { fail("jdaCascadorMeanShape: null cascador or mean_shape"); return -1; }
  const HostModel& h = ((Cascador*)cascador)->hm;
  std::memcpy(mean_shape, h.mean_shape.data(), h.mean_shape.size() * sizeof(double));
  return 0;
} JDA_ABI_CATCH(-1)

int jdaBuildPyramid(void* cascador, const unsigned char* data, int width, int height,
                    unsigned char* half, int* hw, int* hh, unsigned char* quarter, int* qw, int* qh) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !data || width <= 0 || height <= 0) { fail("bad arguments"); return -1; }
  const float r = 1.f / sqrtf(2.f);
  const int w1 = (int)((float)width * r), h1 = (int)((float)height * r), w2 = width / 2, h2 = height / 2;
  if (hw) *hw = w1; if (hh) *hh = h1; if (qw) *qw = w2; if (qh) *qh = h2;
  if (!half && !quarter) return 0;
  OneLane one_lane(c);
  if (!one_lane.open()) return -1;
  Lane* ln = one_lane.lane;
  const unsigned char* frames[1] = {data};
  size_t stride = 0;
  if (!stage_frames(ln, frames, 1, (size_t)width * height, &stride)) return -1;
  auto one = [&](unsigned char* dst, int dw, int dh) -> bool {
    if (!dst || dw < 1 || dh < 1) return true;
    if (!ln->pyr.reserve((size_t)dw * dh + 256)) return false;
    JDA_HIP(launch_resize((const uint8_t*)ln->frames.p, stride, 1, width, height, (uint8_t*)ln->pyr.p,
                          (size_t)dw * dh, dw, dh, (float)(width - 1) / dw, (float)(height - 1) / dh, ln->stream));
    JDA_HIP(hipMemcpyAsync(dst, ln->pyr.p, (size_t)dw * dh, hipMemcpyDeviceToHost, ln->stream));
    JDA_HIP(hipStreamSynchronize(ln->stream));
    return true;
  };
  if (!one(half, w1, h1) || !one(quarter, w2, h2)) return -1;
  return 0;
} JDA_ABI_CATCH_SYNC(-1)

int jdaTraceBatchCpp(void* cascador, const unsigned char* const* frames, int n, int width, int height,
                     int minimum_size, int step, double factor, int* carts_n, double* score,
                     unsigned int* path_hash, double* shapes) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !frames || n < 0) { fail("bad arguments"); return -1; }
  if (!cpp_model_complete(c)) return -1;
  ScanPlan sp; std::string err;
  if (!plan_dialect_cpp(width, height, minimum_size, step, factor, &sp, &err)) { fail(err); return -1; }
  unsigned long long fb; std::memcpy(&fb, &factor, 8);
  PlanKey key{width, height, JDA_DIALECT_CPP, minimum_size, step, c->similarity, fb};
  PlanEntry* pe = nullptr;
  if (!begin_call<double>(c, key, sp, JDA_DIALECT_CPP, &pe)) return -1;
  PlanPin pin{c, pe};
  LaneSet lanes(c);
  size_t stride = 0;
  if (!lanes.take(1) || !stage_frames(lanes.v[0], frames, n, (size_t)width * height, &stride, true)) return -1;
  TraceOut<double> tr{carts_n, score, path_hash, shapes};
  RunStats rs;
  if (!run_device<double>(c, lanes, pe, (const uint8_t*)lanes.v[0]->frames.p, stride, n, false, 0.0, nullptr, nullptr, &tr, &rs,
                          HostFrames{frames, (size_t)width * height})) return -1;
  return 0;
} JDA_ABI_CATCH_SYNC(-1)

int jdaResizeCv(void* cascador, const unsigned char* data, int width, int height, unsigned char* out, int ow, int oh) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !data || !out || width <= 0 || height <= 0 || ow <= 0 || oh <= 0) { fail("bad arguments"); return -1; }
  OneLane one_lane(c);
  if (!one_lane.open()) return -1;
  Lane* ln = one_lane.lane;
  const unsigned char* frames[1] = {data};
  size_t stride = 0;
  if (!stage_frames(ln, frames, 1, (size_t)width * height, &stride)) return -1;
  auto run = [&]() -> bool {
    if (!ln->pyr.reserve((size_t)ow * oh + 256)) return false;
    JDA_HIP(launch_resize_cv((const uint8_t*)ln->frames.p, stride, 1, width, height, (uint8_t*)ln->pyr.p,
                             (size_t)ow * oh, ow, oh, ln->stream));
    JDA_HIP(hipMemcpyAsync(out, ln->pyr.p, (size_t)ow * oh, hipMemcpyDeviceToHost, ln->stream));
    JDA_HIP(hipStreamSynchronize(ln->stream));
    return true;
  };
  return run() ? 0 : -1;
} JDA_ABI_CATCH_SYNC(-1)

static int detect_cpp_pyramid_impl(void* cascador, const unsigned char* const* frames, int n, int width, int height,
                                   int origin_size, int half_size, int quarter_size, int step, double factor, double overlap, int nms,
                                   jdaStats* stats, jdaResultD* out) {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !frames || !out || n < 0) { fail("bad arguments"); return -1; }
  const int L = c->hm.L, dim = c->hm.dim();
  OutGuard<DialectCpp> guard(out, n, L);
  if (origin_size < 1 || step < 1 || !(factor > 1.0)) { fail("origin_size/step must be positive and factor > 1"); return -1; }
  const bool multi = c->hm.multi_scale();
  if (multi && (half_size < 1 || quarter_size < 1 || half_size > 4096 || quarter_size > 4096)) {
    fail("method 0 on a model with scale != 0 split nodes needs the config's half_size and quarter_size: jdaDetectBatchCppPyramidMS "
         "(jdaDetectBatchCppPyramid serves scale==0 models)");
    return -1;
  }
  if (!cpp_model_complete(c)) return -1;
  OneLane one_lane(c);
  if (!one_lane.open()) return -1;
  Lane* ln = one_lane.lane;
  size_t stride0 = 0;
  if (!stage_frames(ln, frames, n, (size_t)width * height, &stride0)) return -1;

  // per frame, level after level in scan order: rects (already scaled back), scores, normalised shapes
  struct Cands { std::vector<int> rc; std::vector<double> sc, sh; };
  std::vector<Cands> per_frame(n);
  RunStats rs_total;
  long long patch_total = 0;
  // level images ping-pong inside one buffer; level 0 is the staged input
  CallBuf levels;
  const size_t lvl_stride = ((size_t)width * height + 255) & ~(size_t)255;
  auto body = [&]() -> bool {
    if (!levels.reserve(2 * lvl_stride * (size_t)std::max(n, 1))) return false;
    const uint8_t* cur = (const uint8_t*)ln->frames.p;
    size_t cur_stride = stride0;
    int w = width, h = height, li = 0;
    double scale = 1.;
    while (w >= origin_size && h >= origin_size) {               // cascador.cpp:283
      ScanPlan sp; std::string err;
      if (!plan_single_level(w, h, origin_size, step, &sp, &err)) { fail(err); return false; }
      PlanKey key{w, h, 2 /* method 0 level */, origin_size, step, c->similarity, 0ull};
      PlanEntry* pe = nullptr;
      if (!begin_call<double>(c, key, sp, JDA_DIALECT_CPP, &pe)) return false;
      PlanPin pin{c, pe};
      RawDets<double> dets;
      RunStats rs;
      HostFrames hf;
      if (multi) { hf.patch_hs = half_size; hf.patch_qs = quarter_size; }
      // (levels after the first read `cur`, which the resize below wrote on ln->stream: handing that stream in as the
      // caller's stream makes run_device order every lane it uses behind it -- also a lane it only takes now, when the
      // pool had none to spare for an earlier level -- and lane 0 keeps running on ln->stream)
      if (!run_device<double>(c, one_lane.set, pe, cur, cur_stride, n, false, 0.0, li > 0 ? ln->stream : nullptr, &dets, nullptr, &rs, hf))
        return false;
      rs_total += rs;
      patch_total += sp.windows * n;
      for (size_t i = 0; i < dets.gid.size(); i++) {
        const WinRef wr = locate(sp, dets.gid[i]);
        Cands& cf = per_frame[wr.frame];
        for (int v : {wr.x, wr.y, wr.win, wr.win}) cf.rc.push_back((int)(v * scale));   // cascador.cpp:292-294
        cf.sc.push_back(dets.score[i]);
        cf.sh.insert(cf.sh.end(), dets.shape.begin() + i * dim, dets.shape.begin() + (i + 1) * dim);
      }
      scale *= factor;                                            // cascador.cpp:299
      const int nw = (int)(w / factor), nh = (int)(h / factor);   // cascador.cpp:300-301
      if (nw < 1 || nh < 1) break;
      uint8_t* nxt = (uint8_t*)levels.p + (size_t)(li & 1) * lvl_stride * (size_t)n;
      JDA_HIP(launch_resize_cv(cur, cur_stride, n, w, h, nxt, lvl_stride, nw, nh, ln->stream));   // cascador.cpp:302
      cur = nxt; cur_stride = lvl_stride; w = nw; h = nh; li++;
    }
    return true;
  };
  const bool ok = body();
  levels.release();
  if (!ok) return -1;

  const double t0 = now_ms();
  size_t total = 0;
  for (auto& v : per_frame) total += v.sc.size();
  parallel_for(n, [&](int f) {
    const Cands& cf = per_frame[f];
    emit<DialectCpp>(cf.rc.data(), cf.sc.data(), cf.sh.data(), (int)cf.sc.size(), L, nms != 0, overlap, &out[f]);
  }, total < 6000);
  fill_stats(stats, rs_total, patch_total, c->hm.T, c->hm.K, now_ms() - t0);
  guard.keep = true;
  return 0;
}

int jdaDetectBatchCppPyramid(void* cascador, const unsigned char* const* frames, int n, int width, int height,
                             int origin_size, int step, double factor, double overlap, int nms,
                             jdaStats* stats, jdaResultD* out) try {
  return detect_cpp_pyramid_impl(cascador, frames, n, width, height, origin_size, 0, 0, step, factor, overlap, nms, stats, out);
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchCppPyramidMS(void* cascador, const unsigned char* const* frames, int n, int width, int height,
                               int origin_size, int half_size, int quarter_size, int step, double factor, double overlap, int nms,
                               jdaStats* stats, jdaResultD* out) try {
  return detect_cpp_pyramid_impl(cascador, frames, n, width, height, origin_size, half_size, quarter_size, step, factor, overlap, nms, stats, out);
} JDA_ABI_CATCH_SYNC(-1)

int jdaNmsC(const int* bboxes, const float* scores, int n, float overlap, unsigned char* keep) try {
  if (n < 0 || (n > 0 && (!bboxes || !scores || !keep))) return -1;
  std::vector<int> k = nms_dialect_c(bboxes, scores, n, overlap);
  std::memset(keep, 0, (size_t)n);
  for (int i : k) keep[i] = 1;
  return (int)k.size();
} JDA_ABI_CATCH(-1)

int jdaNmsCpp(const int* rects, const double* scores, int n, double overlap, int* picked) try {
  if (n < 0 || (n > 0 && (!rects || !scores || !picked))) return -1;
  std::vector<int> k = nms_dialect_cpp(rects, scores, n, overlap);
  std::copy(k.begin(), k.end(), picked);
  return (int)k.size();
} JDA_ABI_CATCH(-1)

int jdaResultsPack(const jdaResult* results, int n, int frame_offset, float* rows, int capacity_rows) try {
  return results && n >= 0 ? (int)pack<DialectC>(results, n, frame_offset, rows, capacity_rows) : -1;
} JDA_ABI_CATCH(-1)

void jdaResultsRelease(jdaResult* results, int n) {
  for (int i = 0; results && i < n; i++) release<DialectC>(results + i);
}

// Tile plan of a dialect-C call without touching a device (tests, tools): per level 10 ints
// {win, step, nx, ny, mode, tw, th, pitch, tiles_x, tiles_y}.  Returns the number of levels.
int jdaDebugPlanTiles(void* cascador, int width, int height, float scale, int min_size, int max_size, int* out, int cap_levels) try {
  Cascador* c = (Cascador*)cascador;
  if (!c) return -1;
  ScanPlan sp; std::string err;
  if (!plan_dialect_c(width, height, scale, min_size, max_size, &sp, &err)) { fail(err); return -1; }
  if ((int)sp.levels.size() > kMaxLevels) return -1;
  PlanEntry pe;
  bool s0_plain = true;
  const size_t n0 = (size_t)c->hm.K * c->hm.node_n();
  for (size_t i = 0; i < n0; i++) s0_plain = s0_plain && c->hm.nodes[i].scale == 0;
  assign_tiles(sp, c->hm, c->kn, s0_plain, 4, &pe);
  for (int i = 0; i < pe.hp.n_levels && i < cap_levels && out; i++) {
    const DevLevel& d = pe.hp.lv[i];
    const int v[10] = {d.win, d.step, d.nx, d.ny, d.tiled, d.tw, d.th, d.pitch, d.tiles_x, d.tiles_y};
    std::memcpy(out + 10 * i, v, sizeof v);
  }
  return pe.hp.n_levels;
} JDA_ABI_CATCH(-1)

long long jdaModelStreamBytes(int T, int K, int landmark_n, int tree_depth, int real_bytes) {
  return model_stream_bytes(T, K, landmark_n, tree_depth, real_bytes);
}

#ifdef JDA_BOUNDS_CHECK
namespace jda {
void jda_bc_read_k_scan(unsigned long long*); void jda_bc_read_k_scan_d(unsigned long long*); void jda_bc_read_k_scan_r(unsigned long long*);
void jda_bc_read_k_scan_dr(unsigned long long*); void jda_bc_read_k_scan_p(unsigned long long*); void jda_bc_read_k_finish(unsigned long long*);
void jda_bc_read_k_wide(unsigned long long*); void jda_bc_read_k_stage(unsigned long long*); void jda_bc_read_k_mine(unsigned long long*); void jda_bc_read_k_train(unsigned long long*); void jda_bc_read_k_lbf(unsigned long long*);
void jda_bc_read_k_gather(unsigned long long*); void jda_bc_read_k_faces(unsigned long long*); void jda_bc_read_k_fit(unsigned long long*); void jda_bc_read_k_reval(unsigned long long*); void jda_bc_read_k_windows(unsigned long long*); void jda_bc_read_k_pack(unsigned long long*); void jda_bc_read_k_chips(unsigned long long*); void jda_bc_read_k_turn(unsigned long long*); void jda_bc_read_k_reduce(unsigned long long*); void jda_bc_read_k_rotate(unsigned long long*);
}
// bounds-check build only (libjda_bounds.so): per translation unit {first violation: site << 32 | source line, violations}
// since the last call -- out[16]; returns the total number of violations (kernels_common.h: Bc)
__attribute__((visibility("default"))) long long jdaDebugBoundsReport(unsigned long long* out) {
  (void)hipDeviceSynchronize();
  void (*rd[8])(unsigned long long*) = {jda_bc_read_k_scan, jda_bc_read_k_scan_d, jda_bc_read_k_scan_r, jda_bc_read_k_scan_dr,
                                        jda_bc_read_k_scan_p, jda_bc_read_k_finish, jda_bc_read_k_wide, jda_bc_read_k_stage};
  long long total = 0;
  for (int i = 0; i < 8; i++) { unsigned long long v[2] = {0, 0}; rd[i](v); if (out) { out[2 * i] = v[0]; out[2 * i + 1] = v[1]; } total += (long long)v[1]; }
  // k_mine's, k_train's, k_lbf's, k_gather's, k_faces', k_fit's, k_reval's, k_windows', k_pack's, k_chips', k_turn's, k_reduce's and k_rotate's words ride in k_finish's slot (out keeps its 16 words); the line is the source line of the check, in the .hip file, cpp_patch.h or cpp_wave.h
  const struct { void (*rd)(unsigned long long*); const char* tu; } more[13] = {{jda_bc_read_k_mine, "k_mine"}, {jda_bc_read_k_train, "k_train"}, {jda_bc_read_k_lbf, "k_lbf"},
                                                                                {jda_bc_read_k_gather, "k_gather"}, {jda_bc_read_k_faces, "k_faces"}, {jda_bc_read_k_fit, "k_fit"}, {jda_bc_read_k_reval, "k_reval"},
                                                                                {jda_bc_read_k_windows, "k_windows"}, {jda_bc_read_k_pack, "k_pack"}, {jda_bc_read_k_chips, "k_chips"}, {jda_bc_read_k_turn, "k_turn"}, {jda_bc_read_k_reduce, "k_reduce"}, {jda_bc_read_k_rotate, "k_rotate"}};
  for (const auto& t : more) {
    unsigned long long v[2] = {0, 0};
    t.rd(v);
    if (!v[1]) continue;
    std::fprintf(stderr, "libjda: bounds check: %s: %llu violation(s), first at site %llu line %llu (of the .hip file, cpp_patch.h or cpp_wave.h)\n", t.tu, v[1], v[0] >> 32, v[0] & 0xffffffffull);
    if (out) { if (!out[11]) out[10] = v[0]; out[11] += v[1]; }
    total += (long long)v[1];
  }
  return total;
}
#endif

#ifdef JDA_SCAN_TIMING
// timing build only: shader-clock stamps of the k_scan workgroups of the last float pass
__attribute__((visibility("default"))) int jdaDebugScanTiming(void* cascador, unsigned long long* out) {
  Cascador* c = (Cascador*)cascador;
  if (!c || c->lanes.empty()) return -1;
  const unsigned long long* dbg = c->lanes[0]->real_bytes == 8 ? c->lanes[0]->wd.dbg : c->lanes[0]->wf.dbg;
  if (!dbg) return -1;
  return hipMemcpy(out, dbg, sizeof(unsigned long long) * 65536 * 32, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

void jdaResultDRelease(jdaResultD result) { release<DialectCpp>(&result); }

int jdaDetectBatchCpp(void* cascador, const unsigned char* const* frames, int n, int width, int height,
                      int minimum_size, int step, double factor, double overlap, int nms,
                      jdaStats* stats, jdaResultD* out) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !frames || !out || n < 0) { fail("bad arguments"); return -1; }
  if (width <= 0 || height <= 0) { fail("frame has no pixels"); return -1; }
  for (int i = 0; i < n; i++) if (!frames[i]) { fail("null frame pointer"); return -1; }
  return detect_cpp_device(c, nullptr, 0, n, width, height, CppCall{minimum_size, step, factor, overlap, nms}, stats, out, frames);
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchCppDevice(void* cascador, const unsigned char* d_frames, size_t frame_stride, int n, int width, int height,
                            int minimum_size, int step, double factor, double overlap, int nms,
                            jdaStats* stats, jdaResultD* out) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !d_frames || !out || n < 0) { fail("bad arguments"); return -1; }
  return detect_cpp_device(c, d_frames, frame_stride, n, width, height, CppCall{minimum_size, step, factor, overlap, nms}, stats, out);
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchCppRagged(void* cascador, const unsigned char* const* images, const int* widths, const int* heights, int n,
                            int minimum_size, int step, double factor, double overlap, int nms,
                            jdaStats* stats, jdaResultD* out) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !images || !widths || !heights || !out || n < 0) { fail("bad arguments"); return -1; }
  return detect_ragged_cpp(c, images, nullptr, nullptr, widths, heights, n, CppCall{minimum_size, step, factor, overlap, nms}, stats, Sink<DialectCpp>{out});
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchCppRaggedDevice(void* cascador, const unsigned char* d_base, const size_t* offsets, const int* widths,
                                  const int* heights, int n, int minimum_size, int step, double factor, double overlap, int nms,
                                  jdaStats* stats, jdaResultD* out) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !d_base || !offsets || !widths || !heights || !out || n < 0) { fail("bad arguments"); return -1; }
  return detect_ragged_cpp(c, nullptr, d_base, offsets, widths, heights, n, CppCall{minimum_size, step, factor, overlap, nms}, stats, Sink<DialectCpp>{out});
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchCppRaggedRows(void* cascador, const unsigned char* const* images, const int* widths, const int* heights, int n,
                                int minimum_size, int step, double factor, double overlap, int nms, jdaStats* stats,
                                int frame_offset, double** rows, int* n_rows) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !images || !widths || !heights || !rows || !n_rows || n < 0) { fail("bad arguments"); return -1; }
  RowsOut<double> v;
  const int rc = detect_ragged_cpp(c, images, nullptr, nullptr, widths, heights, n, CppCall{minimum_size, step, factor, overlap, nms}, stats,
                                 Sink<DialectCpp>{nullptr, &v, frame_offset});
  return rows_out<DialectCpp>(c, rc, v, rows, n_rows);
} JDA_ABI_CATCH_SYNC(-1)

int jdaDetectBatchCppRaggedDeviceRows(void* cascador, const unsigned char* d_base, const size_t* offsets, const int* widths,
                                      const int* heights, int n, int minimum_size, int step, double factor, double overlap, int nms,
                                      jdaStats* stats, int frame_offset, double** rows, int* n_rows) try {
  g_err.clear();
  Cascador* c = (Cascador*)cascador;
  if (!c || !d_base || !offsets || !widths || !heights || !rows || !n_rows || n < 0) { fail("bad arguments"); return -1; }
  RowsOut<double> v;
  const int rc = detect_ragged_cpp(c, nullptr, d_base, offsets, widths, heights, n, CppCall{minimum_size, step, factor, overlap, nms}, stats,
                                 Sink<DialectCpp>{nullptr, &v, frame_offset});
  return rows_out<DialectCpp>(c, rc, v, rows, n_rows);
} JDA_ABI_CATCH_SYNC(-1)

void jdaRowsDRelease(double* rows) { std::free(rows); }

int jdaGlobalRegressionCpp(void* cascador, const int* lbf, const double* residual, int n, int K, const int* rows, int n_rows,
                           const jdaFitParamsCpp* params, double* w, int* out_iters, double* out_gnorm1, jdaFitStatsCpp* stats) try {
  g_err.clear();
  return fit_entry(cascador, lbf, residual, n, K, rows, n_rows, params, w, out_iters, out_gnorm1, stats);
} JDA_ABI_CATCH_SYNC(-1)

int jdaFitShuffleCpp(int* index, int n, uint64_t seed, int iter) try {
  g_err.clear();
  return fit_shuffle(index, n, seed, iter);
} JDA_ABI_CATCH(-1)

int jdaResultsDPack(const jdaResultD* results, int n, int frame_offset, double* rows, int capacity_rows) try {
  return results && n >= 0 ? (int)pack<DialectCpp>(results, n, frame_offset, rows, capacity_rows) : -1;
} JDA_ABI_CATCH(-1)

void jdaResultsDRelease(jdaResultD* results, int n) {
  for (int i = 0; results && i < n; i++) release<DialectCpp>(results + i);
}

}  // extern "C"
