// libjda.so, host side: the model in training (include/jda.h, "Dialect CPP: the model in training").  A cascador whose
// model starts as JoinCascador::JoinCascador() leaves it (reference src/jda/cascador.cpp:17-29) and grows in place: a cart
// of the stage in training is appended or replaced (BoostCart::Train, btcart.cpp:146-253), a stage is closed with its
// regression weights (btcart.cpp:255-292), the trainer's f64 file is written (cascador.cpp:79-124).
//
// The invariant: after any sequence of these calls the cascador behaves in every entry as one created from the file
// grow_serialize would write at that moment (at (s, K - 1), where nothing is written, from that content with header
// (s, K - 1)).  What keeps it:
//   * the host model is the only truth; the status lives in HostModel::hdr_stage / hdr_cart, where a loaded file has it
//   * the detect tables of both dialects (Cascador::mf, md) and the scan plans depend on the whole model (padding of the
//     carts Validate does not run, stage-0 tables, fast_scan): they are invalidated like jdaSetSimilarityTransform and
//     jdaSetOption invalidate them and rebuilt by the next detect call; the queue-size hints start over as well
//   * the mining tables (Cascador::mine_m, mine_buf) ARE the file layout plus Validate's loop bounds: they are patched in
//     place -- a cart's ranges, a stage's w, `full` / `part` -- never freed or carved again
//   * HostModel::multi_cache is reset
//   * the lanes forget how their workspaces are carved (not the allocations): queue lengths are part of what ws_regrows counts
// The patch is a handful of blocking copies issued AFTER Cascador::mu is released, from bytes staged while it was held: the
// entries refuse while a call runs or a ticket is pending, so no kernel reads the tables meanwhile; a call started on
// another thread while a mutating entry runs is the caller's error, as with jdaSetOption.
#include "detect.h"

namespace jda {

namespace {

// Status the reference's loader accepts (cascador.cpp:138-141); (T + 1, -1) is the C library's float convention and
// means "complete" as well.
bool status_ok(const HostModel& h) {
  if ((h.hdr_stage == h.T || h.hdr_stage == h.T + 1) && h.hdr_cart == -1) return true;
  return h.hdr_stage >= 0 && h.hdr_stage < h.T && h.hdr_cart >= -1 && h.hdr_cart < h.K;
}

std::string status_str(const HostModel& h) { return "(stage " + std::to_string(h.hdr_stage) + ", cart " + std::to_string(h.hdr_cart) + ")"; }

// caller holds c->mu
bool can_mutate_locked(Cascador* c, const char* fn) {
  const HostModel& h = c->hm;
  if (h.real_bytes != 8) { fail(std::string(fn) + ": the model was read from an f32 file; only a training cascador or a trainer (f64) snapshot can grow"); return false; }
  if (!status_ok(h)) { fail(std::string(fn) + ": the model carries an impossible training status " + status_str(h)); return false; }
  for (auto& l : c->lanes)
    if (l->busy) { fail(std::string(fn) + " while a call is running or a submitted batch is pending on this cascador"); return false; }
  for (auto& kv : c->plans)
    if (kv.second.pins) { fail(std::string(fn) + " while a call is running on this cascador"); return false; }
  return true;
}

// caller holds c->mu; no lane is busy and no plan pinned, so nothing runs on what is dropped here
void invalidate_locked(Cascador* c) {
  c->mf.ready = false; c->md.ready = false;
  for (auto& kv : c->plans) c->plan_pool.push_back({kv.second.dp, kv.second.table, kv.second.table_cap});
  c->plans.clear();
  c->pred_tail = c->pred_out = -1; c->last_dense = false;
  c->hm.multi_cache = -1;
  // The lanes forget how their workspaces are carved, not the allocations: the next pass carves the queues it asks for, as on
  // a fresh cascador, instead of inheriting longer ones -- a pass that would overflow there (ws_regrows) overflows here too.
  for (auto& l : c->lanes) {
    l->cap = 0; l->cap_q = 0; l->cap_m = 0; l->trace = false; l->dense_ws = false; l->dim = 0; l->real_bytes = 0;
    l->wf = WorkT<float>{}; l->wd = WorkT<double>{};
  }
}

void set_mine_bounds(const HostModel& h, MineModel* m) {          // mine.cpp: mine_model
  const bool snapshot = h.hdr_stage >= 0 && h.hdr_stage < h.T;
  m->full = snapshot ? h.hdr_stage : h.T;
  m->part = snapshot ? std::min(h.K, std::max(0, h.hdr_cart + 1)) : 0;
}

// What a put or a close copies into the mining tables, staged under c->mu: the copies themselves read nothing of the cascador.
struct MinePatch {
  bool on = false; int device = -1; MineModel m{};
  std::vector<NodeD> nodes; std::vector<double> leaf, w; double th = 0., mean = 0., stddev = 1.;
};

// outside c->mu.  Makes the cascador's device current for the calling thread, as every device entry does (ensure_device).
// A failed copy leaves the tables to be rebuilt -- into the same allocation -- by the next call that needs them.
template <typename Fn>
void patch_mine(Cascador* c, const MinePatch& p, Fn&& copies) {
  if (!p.on) return;
  bool ok = hipSetDevice(p.device) == hipSuccess && copies(p.m);
  if (!ok) {
    (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(c->mu);
    c->mine_ready = false;
  }
}

bool h2d(const void* dst, const void* src, size_t bytes) {
  return bytes == 0 || hipMemcpy(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice) == hipSuccess;
}

}  // namespace

Cascador* grow_create(int T, int K, int L, int D, const double* mean_shape) {
  if (!model_dims_ok(T, K, L, D)) {
    fail("jdaCascadorCreateTrainingCpp: implausible dimensions (T in [1, 16], K in [1, 2^20], landmark_n in [1, 4096], tree_depth in [2, 12])");
    return nullptr;
  }
  if (!mean_shape) { fail("jdaCascadorCreateTrainingCpp: null mean_shape"); return nullptr; }
  std::unique_ptr<Cascador> c(new Cascador());
  c->kn.load();
  HostModel& h = c->hm;
  h.T = T; h.K = K; h.L = L; h.D = D;
  h.hdr_stage = 0; h.hdr_cart = -1;                       // cascador.cpp:23-24
  h.real_bytes = 8;
  const size_t carts = (size_t)h.carts();
  const int node_n = h.node_n(), leaf_n = h.leaf_n(), dim = h.dim();
  h.mean_shape.assign(mean_shape, mean_shape + dim);
  // Cart::Cart (cart.cpp:23-37): Feature() is scale ORIGIN, both landmark ids 0, offsets 0. (common.hpp:76-81), thresholds
  // and scores 0, mean 0., std 1.; `th` is left uninitialised there and is 0. here.  BoostCart::BoostCart (btcart.cpp:104-116):
  // w is zeros.
  h.nodes.assign(carts * node_n, SplitNode{0, 0, 0, {0., 0., 0., 0.}, 0});
  h.leaf_score.assign(carts * leaf_n, 0.);
  h.cart_th.assign(carts, 0.); h.cart_mean.assign(carts, 0.); h.cart_std.assign(carts, 1.);
  h.w.assign(carts * leaf_n * dim, 0.);
  return c.release();
}

int grow_status(Cascador* c, int* stage, int* cart) {
  if (!c) { fail("jdaModelStatusCpp: null cascador"); return -1; }
  std::lock_guard<std::mutex> lk(c->mu);
  if (stage) *stage = c->hm.hdr_stage;
  if (cart) *cart = c->hm.hdr_cart;
  return 0;
}

int grow_put_cart(Cascador* c, int k, const jdaFeatureCpp* features, const int* thresholds, const double* leaf_scores, double th,
                  double mean, double stddev) {
  const char* fn = "jdaModelPutCartCpp";
  if (!c) { fail(std::string(fn) + ": null cascador"); return -1; }
  MinePatch mp;
  size_t ci = 0;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    if (!can_mutate_locked(c, fn)) return -1;
    HostModel& h = c->hm;
    const int node_n = h.node_n(), leaf_n = h.leaf_n();
    if (h.hdr_stage >= h.T) { fail(std::string(fn) + ": the model is complete " + status_str(h)); return -1; }
    const bool append = k == h.hdr_cart + 1 && k < h.K, replace = k == h.hdr_cart && k >= 0;
    if (!append && !replace) {
      fail(std::string(fn) + ": cart " + std::to_string(k) + " can be neither appended nor replaced at status " + status_str(h) +
           " (K = " + std::to_string(h.K) + ")");
      return -1;
    }
    if (!features || !thresholds || !leaf_scores) { fail(std::string(fn) + ": null features, thresholds or leaf_scores"); return -1; }
    if (!std::isfinite(stddev) || stddev == 0.) { fail(std::string(fn) + ": std must be finite and not 0"); return -1; }
    for (int i = 0; i < node_n; i++) {
      const jdaFeatureCpp& f = features[i];
      if (f.scale < 0 || f.scale > 2 || f.landmark_id1 < 0 || f.landmark_id1 >= h.L || f.landmark_id2 < 0 || f.landmark_id2 >= h.L) {
        fail(std::string(fn) + ": node " + std::to_string(i + 1) + " has a scale outside 0..2 or a landmark id outside [0, L)");
        return -1;
      }
    }
    ci = (size_t)h.hdr_stage * h.K + k;
    for (int i = 0; i < node_n; i++) {                    // slot i is node i + 1: the order Cart::SerializeTo writes (cart.cpp:431-441)
      const jdaFeatureCpp& f = features[i];
      h.nodes[ci * node_n + i] = SplitNode{f.scale, f.landmark_id1, f.landmark_id2, {f.offset1_x, f.offset1_y, f.offset2_x, f.offset2_y}, thresholds[i]};
    }
    std::copy(leaf_scores, leaf_scores + leaf_n, h.leaf_score.begin() + ci * leaf_n);
    h.cart_th[ci] = th; h.cart_mean[ci] = mean; h.cart_std[ci] = stddev;
    h.hdr_cart = k;
    // (A replace leaves the status as it is and still drops both detect tables and every plan: the cart's nodes are in them.
    // A restart loop that never detects pays only the return of its -- then empty -- plan map to the pool.)
    invalidate_locked(c);
    if (c->mine_ready) {
      set_mine_bounds(h, &c->mine_m);
      mp.on = true; mp.device = c->device; mp.m = c->mine_m;
      mp.nodes.resize(node_n);
      for (int i = 0; i < node_n; i++) {
        const SplitNode& s = h.nodes[ci * node_n + i];
        mp.nodes[i] = NodeD{s.scale, 2 * s.lm1, 2 * s.lm2, s.th, s.off[0], s.off[1], s.off[2], s.off[3]};
      }
      mp.leaf.assign(leaf_scores, leaf_scores + leaf_n);
      mp.th = th; mp.mean = mean; mp.stddev = stddev;
    }
  }
  patch_mine(c, mp, [&](const MineModel& m) {
    return h2d(m.nodes + ci * m.node_n, mp.nodes.data(), mp.nodes.size() * sizeof(NodeD)) &&
           h2d(m.leaf + ci * m.leaf_n, mp.leaf.data(), mp.leaf.size() * 8) && h2d(m.cth + ci, &mp.th, 8) &&
           h2d(m.cmean + ci, &mp.mean, 8) && h2d(m.cstd + ci, &mp.stddev, 8);
  });
  return 0;
}

int grow_close_stage(Cascador* c, const double* w) {
  const char* fn = "jdaModelCloseStageCpp";
  if (!c) { fail(std::string(fn) + ": null cascador"); return -1; }
  MinePatch mp;
  size_t at = 0, cnt = 0;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    if (!can_mutate_locked(c, fn)) return -1;
    HostModel& h = c->hm;
    if (h.hdr_stage >= h.T) { fail(std::string(fn) + ": the model is complete " + status_str(h)); return -1; }
    if (h.hdr_cart != h.K - 1) {
      fail(std::string(fn) + ": the stage in training has " + std::to_string(h.hdr_cart + 1) + " of its " + std::to_string(h.K) + " carts " + status_str(h));
      return -1;
    }
    if (!w) { fail(std::string(fn) + ": null w"); return -1; }
    cnt = (size_t)h.K * h.leaf_n() * h.dim();
    at = (size_t)h.hdr_stage * cnt;
    std::copy(w, w + cnt, h.w.begin() + at);
    h.hdr_stage += 1; h.hdr_cart = -1;                    // after stage T - 1: (T, -1), the complete model (cascador.cpp:93-98)
    invalidate_locked(c);
    if (c->mine_ready) {
      set_mine_bounds(h, &c->mine_m);
      mp.on = true; mp.device = c->device; mp.m = c->mine_m;
      mp.w.assign(w, w + cnt);
    }
  }
  patch_mine(c, mp, [&](const MineModel& m) { return h2d(m.w + at, mp.w.data(), cnt * 8); });
  return 0;
}

int grow_serialize(Cascador* c, const char* path) {
  const char* fn = "jdaCascadorSerializeToCpp";
  if (!c || !path) { fail(std::string(fn) + ": null cascador or path"); return -1; }
  std::lock_guard<std::mutex> lk(c->mu);
  const HostModel& h = c->hm;
  if (h.real_bytes != 8) { fail(std::string(fn) + ": the model was read from an f32 file (jdaCascadorSerializeTo writes that layout)"); return -1; }
  if (!status_ok(h)) { fail(std::string(fn) + ": the model carries an impossible training status " + status_str(h)); return -1; }
  if (h.hdr_stage < h.T && h.hdr_cart == h.K - 1) {
    // JoinCascador::SerializeTo would write (stage + 1, -1) here (cascador.cpp:93-98): a regression that was never fit.
    // The reference never writes in this state either (btcart.cpp:243: kk != K).
    fail(std::string(fn) + ": every cart of the stage in training is written but the stage is not closed " + status_str(h) +
         ": call jdaModelCloseStageCpp first");
    return -1;
  }
  if (!save_model_f64(h, path)) { fail(std::string(fn) + ": cannot write " + path); return -1; }
  return 0;
}

}  // namespace jda
