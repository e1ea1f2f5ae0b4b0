// libjda.so, host side: dialect CPP's Validate on caller crops (jdaValidateCpp*) and the hard-negative mining walk
// (jdaMineNegativesCpp*, reference src/jda/data.cpp:885-1065), on the kernels of k_mine.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "detect.h"

namespace jda {

namespace {

// NextImage's levels of one (transformed) W x H image (data.cpp:915-925): none unless W, H > origin_size; win starts at
// origin_size, a level is the full grid of windows `step` apart (x and y from 0 while x + win <= W, y + win <= H), the
// next level's win is the int of win * factor (State::win_size is an int), and the walk stops at win >= W || win >= H.
struct MineLevel { int win, nx, ny; };
bool mine_levels(int W, int H, int os, int step, double factor, std::vector<MineLevel>* out, std::string* err) {
  out->clear();
  if (os < 1 || step < 1 || !(factor > 1.0)) { *err = "origin_size and step must be positive and factor > 1"; return false; }
  if (W <= os || H <= os) return true;                    // data.cpp:921
  int win = os;
  while (true) {
    out->push_back({win, (W - win) / step + 1, (H - win) / step + 1});
    const double g = (double)win * factor;
    if (!(g < 2147483647.0)) break;
    const int nw = (int)g;                                // s.win_size *= s.factor (int)
    if (nw >= W || nw >= H) break;                        // data.cpp:906
    if (nw <= win) { *err = "factor does not grow the window (the reference's walk would not end)"; return false; }
    win = nw;
  }
  return true;
}

}  // namespace

// The mining tables of the model as it stands (built on first use, patched in place by model_grow.cpp); also reval.cpp's.
bool mine_model(Cascador* c, MineModel* out) {
  if (!cpp_model_complete(c)) return false;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!ensure_device(c)) return false;
  if (!c->mine_ready) {
    const HostModel& h = c->hm;
    const size_t carts = (size_t)h.carts();
    const int node_n = h.node_n(), leaf_n = h.leaf_n(), dim = h.dim();
    std::vector<NodeD> nodes(carts * node_n);
    for (size_t i = 0; i < nodes.size(); i++) {
      const SplitNode& s = h.nodes[i];
      NodeD& d = nodes[i];
      d.scale = s.scale; d.lm1x2 = 2 * s.lm1; d.lm2x2 = 2 * s.lm2; d.th = s.th;
      d.o1x = s.off[0]; d.o1y = s.off[1]; d.o2x = s.off[2]; d.o2y = s.off[3];
    }
    NodeD* dn; double* dl; double* dth; double* dmu; double* dsd; double* dw; double* dms;
    if (!carve_into(c->mine_buf, [&](Carver& cv) {
          dn = cv.take<NodeD>(nodes.size());
          dl = cv.take<double>(h.leaf_score.size());
          dth = cv.take<double>(carts); dmu = cv.take<double>(carts); dsd = cv.take<double>(carts);
          dw = cv.take<double>(h.w.size());
          dms = cv.take<double>(dim);
        })) return false;
    MineModel& m = c->mine_m;
    auto up = [&](const void* src, size_t bytes, void* dst) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess; };
    if (!up(nodes.data(), nodes.size() * sizeof(NodeD), dn) || !up(h.leaf_score.data(), h.leaf_score.size() * 8, dl) ||
        !up(h.cart_th.data(), carts * 8, dth) || !up(h.cart_mean.data(), carts * 8, dmu) || !up(h.cart_std.data(), carts * 8, dsd) ||
        !up(h.w.data(), h.w.size() * 8, dw) || !up(h.mean_shape.data(), dim * 8, dms)) {
      fail("model upload failed");
      return false;
    }
    m.T = h.T; m.K = h.K; m.L = h.L; m.D = h.D; m.node_n = node_n; m.leaf_n = leaf_n; m.dim = dim;
    // Validate's loop bounds (cascador.cpp:177-209): a trainer snapshot runs stages [0, s) and carts [0, c] of stage s
    const bool snapshot = h.hdr_stage >= 0 && h.hdr_stage < h.T;
    m.full = snapshot ? h.hdr_stage : h.T;
    m.part = snapshot ? std::min(h.K, std::max(0, h.hdr_cart + 1)) : 0;
    m.nodes = dn; m.leaf = dl; m.cth = dth; m.cmean = dmu; m.cstd = dsd; m.w = dw; m.mean = dms;
    c->mine_ready = true;
  }
  *out = c->mine_m;
  return true;
}

namespace {

bool check_sizes(int os, int hs, int qs, int mode, double shift) {
  if (!check_patch_sizes(os, hs, qs)) return false;
  if (mode != 0 && mode != 1) { fail("resize_mode must be 0 (mining chain) or 1 (detectSingleScale chain)"); return false; }
  if (!(shift >= 0.) || !std::isfinite(shift)) { fail("shift_size must be finite and >= 0"); return false; }
  return true;
}

int pbytes_of(const MineSizes& z) { return ((z.os * z.os + z.hs * z.hs + z.qs * z.qs) + 15) & ~15; }
int ptight_of(const MineSizes& z) { return z.os * z.os + z.hs * z.hs + z.qs * z.qs; }

// Per-crop scratch of the walk: patches, shape, two similarity buffers, the K leaf rows of a stage, item, outputs.
size_t item_bytes(const MineModel& m, const MineSizes& z) {
  return (size_t)pbytes_of(z) + 3 * (size_t)m.dim * 8 + (size_t)m.K * 4 + sizeof(MineItem) + 8 + 8 + 4 + 1;
}

struct WalkBufs {
  MineItem* items; uint8_t* patches; double* shape; double* t1; double* t2; int* lbf; double* score; int* carts; uint8_t* face;
  unsigned long long* ords;
  void carve(Carver& cv, const MineModel& m, const MineSizes& z, size_t cap) {
    items = cv.take<MineItem>(cap); patches = cv.take<uint8_t>(cap * pbytes_of(z));
    shape = cv.take<double>(cap * m.dim); t1 = cv.take<double>(cap * m.dim); t2 = cv.take<double>(cap * m.dim);
    lbf = cv.take<int>(cap * m.K); score = cv.take<double>(cap); carts = cv.take<int>(cap); face = cv.take<uint8_t>(cap);
    ords = cv.take<unsigned long long>(cap);
  }
};

// crops that a batch of the walk takes at once, within the call's workspace budget
size_t walk_cap(Cascador* c, const MineModel& m, const MineSizes& z, size_t want) {
  const size_t budget = (size_t)std::max<long long>(64, c->kn.workspace_mb) << 20;
  const size_t per = item_bytes(m, z);
  return std::max<size_t>(1, std::min<size_t>({want, (size_t)65536, budget / 2 / per}));
}

bool upload_imgs(const std::vector<MineImg>& imgs, CallBuf* buf, hipStream_t st) {
  if (!buf->reserve(std::max<size_t>(1, imgs.size()) * sizeof(MineImg) + 256)) return false;
  JDA_HIP(hipMemcpyAsync(buf->p, imgs.data(), imgs.size() * sizeof(MineImg), hipMemcpyHostToDevice, st));
  return true;
}

// Host images -> one device buffer (each image at a 256-byte aligned offset).
bool stage_images(const unsigned char* const* images, const int* widths, const int* heights, int n, CallBuf* buf,
                  std::vector<size_t>* offs, hipStream_t st) {
  offs->resize(n);
  size_t total = 0;
  for (int i = 0; i < n; i++) {
    if (!images[i] || widths[i] < 1 || heights[i] < 1) { fail("null image or empty size"); return false; }
    (*offs)[i] = total;
    total += ((size_t)widths[i] * heights[i] + 255) & ~(size_t)255;
  }
  if (!buf->reserve(std::max<size_t>(total, 256))) return false;
  for (int i = 0; i < n; i++)
    JDA_HIP(hipMemcpyAsync((uint8_t*)buf->p + (*offs)[i], images[i], (size_t)widths[i] * heights[i], hipMemcpyHostToDevice, st));
  JDA_HIP(hipStreamSynchronize(st));
  return true;
}

// The caller's images on the device, and what the four device entries are called with.
struct ImageSet { const uint8_t* d_base; const size_t* offsets; const int* widths; const int* heights; int n; };
struct ValidateArgs {
  ImageSet im; const int* crops; int n_crops; int os, hs, qs, mode; double shift; unsigned long long seed;
  unsigned char* is_face; double* score; int* carts_n; double* shape; jdaStats* stats;
};
struct MineArgs {
  ImageSet im; const int* steps; const double* factors; const int* transforms; int os, hs, qs; long long start; int size;
  double shift; unsigned long long seed; int* hits; double* score; double* shape; unsigned char* patches; jdaMineStats* stats;
};

// The nb items in b.items through k_mine_patches and k_mine_walk; face, carts and (score_h given) score queued back to the
// host.  The caller queues what else it wants back and waits for the stream.  Counts the batch and its two launches.
bool walk_batch(Cascador* c, const MineModel& m, const MineSizes& z, const uint8_t* d_base, const CallBuf& imgs, const WalkBufs& b,
                int nb, uint8_t* face_h, int* carts_h, double* score_h, hipStream_t st) {
  MineLaunch how;
  JDA_HIP(launch_mine_patches(z, d_base, (const MineImg*)imgs.p, b.items, nb, b.patches, pbytes_of(z), st, &how));
  c->log.count(how);
  JDA_HIP(launch_mine_walk(m, z, b.items, nb, b.patches, pbytes_of(z), c->similarity, b.face, b.carts, b.score, b.shape, b.lbf,
                           b.t1, b.t2, st, nullptr, &how));
  c->log.count(how);
  c->log.count_mine_batch(nb);
  JDA_HIP(hipMemcpyAsync(face_h, b.face, nb, hipMemcpyDeviceToHost, st));
  JDA_HIP(hipMemcpyAsync(carts_h, b.carts, nb * sizeof(int), hipMemcpyDeviceToHost, st));
  if (score_h) JDA_HIP(hipMemcpyAsync(score_h, b.score, nb * sizeof(double), hipMemcpyDeviceToHost, st));
  return true;
}

// ---- Validate on caller crops -------------------------------------------------------------------------------------

int validate_device(Cascador* c, const ValidateArgs& a) {
  const double t0 = now_ms();
  const ImageSet& im = a.im;
  const int n_crops = a.n_crops;
  if (!c || im.n < 0 || n_crops < 0 || (n_crops > 0 && (!a.crops || !im.d_base || !im.offsets || !im.widths || !im.heights))) {
    fail("bad arguments"); return -1;
  }
  if (!check_sizes(a.os, a.hs, a.qs, a.mode, a.shift)) return -1;
  std::vector<MineImg> imgs(im.n);
  for (int i = 0; i < im.n; i++) {
    if (im.widths[i] < 1 || im.heights[i] < 1) { fail("image " + std::to_string(i) + " has an empty size"); return -1; }
    imgs[i] = MineImg{(unsigned long long)im.offsets[i], im.widths[i], im.heights[i], 0, 0};
  }
  std::vector<MineItem> items(n_crops);
  for (int i = 0; i < n_crops; i++) {
    const int* q = a.crops + 5 * i;
    if (q[0] < 0 || q[0] >= im.n || q[3] < 1 || q[4] < 1 || q[1] < 0 || q[2] < 0 ||
        (long long)q[1] + q[3] > im.widths[q[0]] || (long long)q[2] + q[4] > im.heights[q[0]]) {
      fail("crop " + std::to_string(i) + " (image, x, y, w, h) = (" + std::to_string(q[0]) + ", " + std::to_string(q[1]) + ", " +
           std::to_string(q[2]) + ", " + std::to_string(q[3]) + ", " + std::to_string(q[4]) + ") does not lie inside its image");
      return -1;
    }
    items[i] = MineItem{q[0], q[1], q[2], q[3], q[4], 0, (unsigned long long)i};
  }
  MineModel m;
  if (!mine_model(c, &m)) return -1;
  const MineSizes z{a.os, a.hs, a.qs, a.mode, a.shift, a.seed};
  OneLane one(c);
  if (!one.open()) return -1;
  const hipStream_t st = one.stream;
  const int dim = m.dim;
  long long faces = 0, nf_carts = 0;
  CallBuf ib, wb;
  auto body = [&]() -> bool {
    if (!upload_imgs(imgs, &ib, st)) return false;
    const size_t cap = walk_cap(c, m, z, (size_t)std::max(1, n_crops));
    c->log.set_mine_cap((long long)cap);
    WalkBufs b;
    if (!carve_into(wb, [&](Carver& cv) { b.carve(cv, m, z, cap); })) return false;
    std::vector<uint8_t> f(cap);
    std::vector<int> cn(cap);
    for (int at = 0; at < n_crops; at += (int)cap) {
      const int nb = (int)std::min<size_t>(cap, (size_t)(n_crops - at));
      JDA_HIP(hipMemcpyAsync(b.items, items.data() + at, nb * sizeof(MineItem), hipMemcpyHostToDevice, st));
      if (!walk_batch(c, m, z, im.d_base, ib, b, nb, f.data(), cn.data(), a.score ? a.score + at : nullptr, st)) return false;
      if (a.shape) JDA_HIP(hipMemcpyAsync(a.shape + (size_t)at * dim, b.shape, (size_t)nb * dim * sizeof(double), hipMemcpyDeviceToHost, st));
      JDA_HIP(hipStreamSynchronize(st));
      for (int i = 0; i < nb; i++) {
        if (a.is_face) a.is_face[at + i] = f[i];
        if (a.carts_n) a.carts_n[at + i] = cn[i];
        if (f[i]) faces++; else nf_carts += cn[i];
      }
    }
    return true;
  };
  if (!body()) return -1;
  if (jdaStats* stats = a.stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->patch_n = n_crops; stats->face_patch_n = faces; stats->nonface_patch_n = n_crops - faces;
    stats->cart_gothrough_n = nf_carts;
    stats->average_cart_n = stats->nonface_patch_n ? (double)nf_carts / stats->nonface_patch_n : 0.;
    stats->call_ms = now_ms() - t0;
  }
  return 0;
}

// ---- the mining walk ----------------------------------------------------------------------------------------------

int mine_device(Cascador* c, const MineArgs& a) {
  const double t0 = now_ms();
  const ImageSet& im = a.im;
  jdaMineStats* stats = a.stats;
  const int size = a.size;
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (!c || im.n < 0 || size < 0 || a.start < 0 ||
      (im.n > 0 && (!im.d_base || !im.offsets || !im.widths || !im.heights || !a.steps || !a.factors || !a.transforms))) {
    fail("bad arguments"); return -1;
  }
  if (!check_sizes(a.os, a.hs, a.qs, 0, a.shift)) return -1;
  // the enumeration: (image, level) segments in NextImage's order
  std::vector<MineImg> imgs(im.n);
  std::vector<MineSeg> segs;
  unsigned long long total = 0;
  std::vector<MineLevel> lv;
  for (int i = 0; i < im.n; i++) {
    if (im.widths[i] < 1 || im.heights[i] < 1) { fail("image " + std::to_string(i) + " has an empty size"); return -1; }
    if (a.transforms[i] < 0 || a.transforms[i] > 7) { fail("transform must be in 0..7"); return -1; }
    const int tf = kTf[a.transforms[i]];
    imgs[i] = MineImg{(unsigned long long)im.offsets[i], im.widths[i], im.heights[i], tf, 0};
    const int W = (tf & kMineSwap) ? im.heights[i] : im.widths[i], H = (tf & kMineSwap) ? im.widths[i] : im.heights[i];
    std::string err;
    if (!mine_levels(W, H, a.os, a.steps[i], a.factors[i], &lv, &err)) { fail("image " + std::to_string(i) + ": " + err); return -1; }
    for (const MineLevel& l : lv) {
      segs.push_back(MineSeg{total, i, l.win, a.steps[i], l.nx});
      total += (unsigned long long)l.nx * l.ny;
    }
  }
  const unsigned long long begin = std::min<unsigned long long>((unsigned long long)a.start, total);
  unsigned long long lo = begin;
  long long n_hits = 0, nega = 0, carts = 0;
  if (size > 0 && begin < total) {
    MineModel m;
    if (!mine_model(c, &m)) return -1;
    const MineSizes z{a.os, a.hs, a.qs, 0, a.shift, a.seed};
    OneLane one(c);
    if (!one.open()) return -1;
    const hipStream_t st = one.stream;
    const int dim = m.dim, pb = pbytes_of(z), pt = ptight_of(z);
    // the scan's share of stage 0: Validate's first carts, pixels on demand.  With the similarity transform every window
    // goes to the walk (its stage-0 parameter depends on the window's own shifted shape).
    const int stage0 = m.full > 0 ? m.K : m.part;
    const int carts0 = c->similarity ? 0 : std::min(stage0, (int)std::max<long long>(1, c->kn.handoff));
    const size_t budget = (size_t)std::max<long long>(64, c->kn.workspace_mb) << 20;
    const unsigned long long chunk = std::max<unsigned long long>(
        64, std::min<unsigned long long>((unsigned long long)std::max<long long>(1, c->kn.mine_chunk_windows), budget / 4 / 12));
    CallBuf ib, sb, wb;
    auto body = [&]() -> bool {
      if (!upload_imgs(imgs, &ib, st)) return false;
      MineSeg* d_segs; int* d_status; unsigned long long* d_surv; unsigned* d_nsurv; unsigned long long* d_sum;
      if (!carve_into(sb, [&](Carver& cv) {
            d_segs = cv.take<MineSeg>(segs.size()); d_status = cv.take<int>(chunk); d_surv = cv.take<unsigned long long>(chunk);
            d_nsurv = cv.take<unsigned>(4); d_sum = cv.take<unsigned long long>(2);
          })) return false;
      JDA_HIP(hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(MineSeg), hipMemcpyHostToDevice, st));
      const size_t cap = walk_cap(c, m, z, 65536);
      c->log.set_mine_cap((long long)cap);
      WalkBufs b;
      if (!carve_into(wb, [&](Carver& cv) { b.carve(cv, m, z, cap); })) return false;
      std::vector<unsigned long long> surv;
      std::vector<uint8_t> f(cap);
      std::vector<int> cn(cap);
      std::vector<double> sc(cap);
      std::vector<MineItem> it(cap);
      std::vector<double> sh_h;
      std::vector<uint8_t> pa_h;
      while (lo < total && n_hits < size) {
        const unsigned long long hi = std::min(total, lo + chunk);
        JDA_HIP(hipMemsetAsync(d_nsurv, 0, 4 * sizeof(unsigned), st));
        JDA_HIP(hipMemsetAsync(d_sum, 0, 2 * sizeof(unsigned long long), st));
        MineLaunch how;
        JDA_HIP(launch_mine_scan(m, z, im.d_base, (const MineImg*)ib.p, d_segs, (int)segs.size(), lo, hi, carts0, d_status, d_surv,
                                 d_nsurv, st, &how));
        c->log.count(how);
        c->log.count_mine_chunk();
        unsigned ns = 0;
        JDA_HIP(hipMemcpyAsync(&ns, d_nsurv, sizeof ns, hipMemcpyDeviceToHost, st));
        JDA_HIP(hipStreamSynchronize(st));
        surv.resize(ns);
        if (ns) {
          JDA_HIP(hipMemcpyAsync(surv.data(), d_surv, ns * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
          JDA_HIP(hipStreamSynchronize(st));
          std::sort(surv.begin(), surv.end());              // enumeration order
        }
        unsigned long long cut = hi;                         // one past the last window this chunk contributes
        long long walk_nega = 0, walk_carts = 0;
        for (size_t at = 0; at < surv.size() && n_hits < size; at += cap) {
          const int nb = (int)std::min<size_t>(cap, surv.size() - at);
          JDA_HIP(hipMemcpyAsync(b.ords, surv.data() + at, nb * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
          JDA_HIP(launch_mine_items(d_segs, (int)segs.size(), b.ords, nb, b.items, st, &how));
          c->log.count(how);
          if (!walk_batch(c, m, z, im.d_base, ib, b, nb, f.data(), cn.data(), sc.data(), st)) return false;
          JDA_HIP(hipMemcpyAsync(it.data(), b.items, nb * sizeof(MineItem), hipMemcpyDeviceToHost, st));
          JDA_HIP(hipStreamSynchronize(st));
          // the batch's faces in order: their rows now, their shapes and patch bytes in one copy each below
          std::vector<int> take;
          for (int i = 0; i < nb && n_hits + (long long)take.size() < size; i++) {
            if (!f[i]) { walk_nega++; walk_carts += cn[i]; continue; }
            take.push_back(i);
            if (n_hits + (long long)take.size() == size) cut = surv[at + i] + 1;
          }
          if (take.empty()) continue;
          const int last = take.back() + 1;             // faces lie in the batch's first `last` entries
          if (a.shape) { sh_h.resize((size_t)last * dim); JDA_HIP(hipMemcpyAsync(sh_h.data(), b.shape, sh_h.size() * sizeof(double), hipMemcpyDeviceToHost, st)); }
          if (a.patches) { pa_h.resize((size_t)last * pb); JDA_HIP(hipMemcpyAsync(pa_h.data(), b.patches, pa_h.size(), hipMemcpyDeviceToHost, st)); }
          JDA_HIP(hipStreamSynchronize(st));
          for (int i : take) {
            const long long h = n_hits++;
            if (a.hits) { int* r = a.hits + 4 * h; r[0] = it[i].image; r[1] = it[i].x; r[2] = it[i].y; r[3] = it[i].w; }
            if (a.score) a.score[h] = sc[i];
            if (a.shape) std::memcpy(a.shape + (size_t)h * dim, sh_h.data() + (size_t)i * dim, dim * sizeof(double));
            if (a.patches) std::memcpy(a.patches + (size_t)h * pt, pa_h.data() + (size_t)i * pb, pt);
          }
        }
        // reject lengths of the windows the scan rejected in [lo, cut), plus the walk's rejects (all below cut)
        unsigned long long sum[2] = {0, 0};
        JDA_HIP(launch_mine_sum(d_status, cut - lo, d_sum, st, &how));
        c->log.count(how);
        JDA_HIP(hipMemcpyAsync(sum, d_sum, sizeof sum, hipMemcpyDeviceToHost, st));
        JDA_HIP(hipStreamSynchronize(st));
        c->log.count_mine_rejects((long long)sum[0], walk_nega);
        nega += (long long)sum[0] + walk_nega;
        carts += (long long)sum[1] + walk_carts;
        lo = cut;
      }
      return true;
    };
    if (!body()) return -1;
  }
  if (stats) {
    stats->windows = (long long)(lo - begin); stats->hits = n_hits; stats->nega_n = nega; stats->carts_n = carts;
    stats->next_start = (long long)lo; stats->total_windows = (long long)total; stats->call_ms = now_ms() - t0;
  }
  return (int)n_hits;
}

// The host entries' first step: the images to the device (the device is made current here), base and offsets into `im`.
struct Staged { CallBuf buf; std::vector<size_t> offs; };
bool stage(Cascador* c, const unsigned char* const* images, ImageSet* im, Staged* st) {
  if (!c || im->n < 0 || (im->n > 0 && (!images || !im->widths || !im->heights))) { fail("bad arguments"); return false; }
  if (!begin_device(c) || !stage_images(images, im->widths, im->heights, im->n, &st->buf, &st->offs, nullptr)) return false;
  im->d_base = (const uint8_t*)st->buf.p; im->offsets = st->offs.data();
  return true;
}

}  // namespace
}  // namespace jda

using namespace jda;

extern "C" {

int jdaMineWindows(int w, int h, int origin_size, int step, double factor, long long* n, int* levels) try {
  std::vector<MineLevel> lv;
  std::string err;
  if (!mine_levels(w, h, origin_size, step, factor, &lv, &err)) { fail(err); return -1; }
  long long t = 0;
  for (const MineLevel& l : lv) t += (long long)l.nx * l.ny;
  if (n) *n = t;
  if (levels) *levels = (int)lv.size();
  return 0;
} JDA_ABI_CATCH(-1)

long long jdaMineWindowList(int w, int h, int origin_size, int step, double factor, int* xyw, long long cap) try {
  std::vector<MineLevel> lv;
  std::string err;
  if (!mine_levels(w, h, origin_size, step, factor, &lv, &err)) { fail(err); return -1; }
  long long t = 0;
  for (const MineLevel& l : lv)
    for (int y = 0; y < l.ny; y++)
      for (int x = 0; x < l.nx; x++, t++)
        if (xyw && t < cap) { xyw[3 * t] = x * step; xyw[3 * t + 1] = y * step; xyw[3 * t + 2] = l.win; }
  return t;
} JDA_ABI_CATCH(-1)

int jdaValidateCpp(void* cascador, const unsigned char* const* images, const int* widths, const int* heights, int n_images,
                   const int* crops, int n_crops, int origin_size, int half_size, int quarter_size, int resize_mode,
                   double shift_size, uint64_t seed, unsigned char* is_face, double* score, int* carts_n, double* shape,
                   jdaStats* stats) try {
  g_err.clear();
  ValidateArgs a{{nullptr, nullptr, widths, heights, n_images}, crops, n_crops, origin_size, half_size, quarter_size, resize_mode,
                 shift_size, seed, is_face, score, carts_n, shape, stats};
  Staged st;
  return stage((Cascador*)cascador, images, &a.im, &st) ? validate_device((Cascador*)cascador, a) : -1;
} JDA_ABI_CATCH_SYNC(-1)

int jdaValidateCppDevice(void* cascador, const unsigned char* d_base, const size_t* offsets, const int* widths, const int* heights,
                         int n_images, const int* crops, int n_crops, int origin_size, int half_size, int quarter_size,
                         int resize_mode, double shift_size, uint64_t seed, unsigned char* is_face, double* score, int* carts_n,
                         double* shape, jdaStats* stats) try {
  g_err.clear();
  return validate_device((Cascador*)cascador, ValidateArgs{{d_base, offsets, widths, heights, n_images}, crops, n_crops, origin_size,
                                                           half_size, quarter_size, resize_mode, shift_size, seed, is_face, score,
                                                           carts_n, shape, stats});
} JDA_ABI_CATCH_SYNC(-1)

int jdaMineNegativesCpp(void* cascador, const unsigned char* const* images, const int* widths, const int* heights, int n_images,
                        const int* steps, const double* factors, const int* transforms, int origin_size, int half_size,
                        int quarter_size, long long start, int size, double shift_size, uint64_t seed, int* hits, double* score,
                        double* shape, unsigned char* patches, jdaMineStats* stats) try {
  g_err.clear();
  MineArgs a{{nullptr, nullptr, widths, heights, n_images}, steps, factors, transforms, origin_size, half_size, quarter_size, start, size,
             shift_size, seed, hits, score, shape, patches, stats};
  Staged st;
  return stage((Cascador*)cascador, images, &a.im, &st) ? mine_device((Cascador*)cascador, a) : -1;
} JDA_ABI_CATCH_SYNC(-1)

int jdaMineNegativesCppDevice(void* cascador, const unsigned char* d_base, const size_t* offsets, const int* widths,
                              const int* heights, int n_images, const int* steps, const double* factors, const int* transforms,
                              int origin_size, int half_size, int quarter_size, long long start, int size, double shift_size,
                              uint64_t seed, int* hits, double* score, double* shape, unsigned char* patches,
                              jdaMineStats* stats) try {
  g_err.clear();
  return mine_device((Cascador*)cascador, MineArgs{{d_base, offsets, widths, heights, n_images}, steps, factors, transforms, origin_size,
                                                   half_size, quarter_size, start, size, shift_size, seed, hits, score, shape,
                                                   patches, stats});
} JDA_ABI_CATCH_SYNC(-1)

}  // extern "C"
