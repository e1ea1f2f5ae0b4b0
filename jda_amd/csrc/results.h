// libjda.so, host side: the result format of both dialects in one place -- the jdaResult / jdaResultD structs (how they
// are allocated, blanked and released), the row layout [frame, box..., score, shape...] of the *Rows entries and of
// jdaResults[D]Pack, the window of a gid, and NMS + relocation of one image's candidates (post.cpp).  Host-only and free
// of HIP, so that a plain C++ compiler can test it (tests/test_results.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <numeric>
#include <vector>

#include "../../include/jda.h"
#include "plan.h"
#include "post.h"

namespace jda {

// ---- the two dialects ----
// Dialect C (c/jda.c): float, jdaResult, boxes (x, y, size), rows of 5 + 2L floats.
struct DialectC {
  using Real = float; using Result = jdaResult;
  static constexpr int box = 3, head = 5;         // ints per box; row elements in front of the shape
  static constexpr bool parallel_rows = false;    // a job's rows are few and mostly k_post's: written on the calling thread
  static int*& boxes(Result& r) { return r.bboxes; }
  static const int* boxes(const Result& r) { return r.bboxes; }
  static void window(int x, int y, int win, int* b) { b[0] = x; b[1] = y; b[2] = win; }
  static void nms(const int* b, const Real* s, int n, double overlap, std::vector<int>* keep) {
    nms_dialect_c_into(b, s, n, (float)overlap, keep);                                     // c/jda.c:237-316
  }
  static void relocate(Real* shape, int L, const int* b) { relocate_dialect_c(shape, L, b[0], b[1], b[2]); }   // c/jda.c:465-474
};
// Dialect CPP (src/jda): double, jdaResultD, rects (x, y, w, h), rows of 6 + 2L doubles.
struct DialectCpp {
  using Real = double; using Result = jdaResultD;
  static constexpr int box = 4, head = 6;
  static constexpr bool parallel_rows = true;     // (no device post: NMS per image on the pool's workers)
  static int*& boxes(Result& r) { return r.rects; }
  static const int* boxes(const Result& r) { return r.rects; }
  static void window(int x, int y, int win, int* b) { b[0] = x; b[1] = y; b[2] = win; b[3] = win; }   // Rect roi_o, cascador.cpp:339
  static void nms(const int* b, const Real* s, int n, double overlap, std::vector<int>* keep) {
    *keep = nms_dialect_cpp(b, s, n, overlap);                                             // cascador.cpp:387-429
  }
  static void relocate(Real* shape, int L, const int* b) { relocate_dialect_cpp(shape, L, b[0], b[1], b[2], b[3]); }   // cascador.cpp:462-474
};

// ---- result structs ----
// Nothing allocated: what every entry hands back for a frame it did not fill.
template <class D>
void blank(typename D::Result* r, int L) {
  r->n = 0; r->landmark_n = L;
  D::boxes(*r) = nullptr; r->shapes = nullptr; r->scores = nullptr;
}
template <class D>
void release(typename D::Result* r) {
  std::free(D::boxes(*r)); std::free(r->shapes); std::free(r->scores);
  blank<D>(r, r->landmark_n);
}
// The three arrays of n detections (never NULL, even for n = 0).  Throws std::bad_alloc with nothing allocated.
template <class D>
void alloc(typename D::Result* r, size_t n, int L) {
  using Real = typename D::Real;
  blank<D>(r, L);
  D::boxes(*r) = (int*)std::malloc(std::max<size_t>(1, n * D::box) * sizeof(int));
  r->scores = (Real*)std::malloc(std::max<size_t>(1, n) * sizeof(Real));
  r->shapes = (Real*)std::malloc(std::max<size_t>(1, n * 2 * L) * sizeof(Real));
  if (!D::boxes(*r) || !r->scores || !r->shapes) { release<D>(r); throw std::bad_alloc(); }
  r->n = (int)n;
}
template <class D>
typename D::Result empty_result(int L) {
  typename D::Result r;
  alloc<D>(&r, 0, L);
  return r;
}

// out[0, n) blank from here on, and blank again on the way out of the entry unless `keep` is set: an entry that fails --
// an error return or an exception -- hands back nothing the caller would have to free.
template <class D>
struct OutGuard {
  typename D::Result* out; int n; bool keep = false;
  OutGuard(typename D::Result* out_, int n_, int L) : out(out_), n(n_) { for (int i = 0; i < n; i++) blank<D>(out + i, L); }
  ~OutGuard() { if (!keep) for (int i = 0; i < n; i++) release<D>(out + i); }
  OutGuard(const OutGuard&) = delete; OutGuard& operator=(const OutGuard&) = delete;
};

// ---- NMS, relocation ----
// The candidates that stay, in output order: NMS (c/jda.c:237-316, cascador.cpp:444-446) or, with NMS off, every one of
// them in scan order (cascador.cpp:447-451).
template <class D>
void pick(const int* boxes, const typename D::Real* scores, int n, bool nms, double overlap, std::vector<int>* keep) {
  if (nms) D::nms(boxes, scores, n, overlap, keep);
  else { keep->resize((size_t)n); std::iota(keep->begin(), keep->end(), 0); }
}

// The result of one image from its n candidates in scan order: boxes (D::box ints each), scores, window-normalised
// shapes (2L each) -> NMS, then the kept ones copied and relocated.
template <class D>
void emit(const int* boxes, const typename D::Real* scores, const typename D::Real* shapes, int n, int L, bool nms, double overlap,
          typename D::Result* out) {
  using Real = typename D::Real;
  const int dim = 2 * L;
  static thread_local std::vector<int> keep;           // per-image scratch, grown once per thread
  pick<D>(boxes, scores, n, nms, overlap, &keep);
  alloc<D>(out, keep.size(), L);
  for (size_t i = 0; i < keep.size(); i++) {
    const int k = keep[i];
    std::memcpy(D::boxes(*out) + D::box * i, boxes + D::box * k, D::box * sizeof(int));
    out->scores[i] = scores[k];
    Real* sh = out->shapes + i * dim;
    std::memcpy(sh, shapes + (size_t)k * dim, dim * sizeof(Real));
    D::relocate(sh, L, boxes + D::box * k);
  }
}

// ---- rows ----
// One row [frame, box..., score, shape...] (D::head + dim elements); returns where the next one starts.  The only writer
// of the row layout.
template <class D>
typename D::Real* write_row(typename D::Real* o, int frame, const int* box, typename D::Real score, const typename D::Real* shape, int dim) {
  using Real = typename D::Real;
  o[0] = (Real)frame;
  for (int q = 0; q < D::box; q++) o[1 + q] = (Real)box[q];
  o[1 + D::box] = score;
  std::memcpy(o + D::head, shape, (size_t)dim * sizeof(Real));
  return o + D::head + dim;
}
// The rows of one image straight from its candidates (as emit() would keep them): the picked ones, relocated in place.
template <class D>
typename D::Real* write_rows(typename D::Real* o, int frame, const int* boxes, const typename D::Real* scores,
                             const typename D::Real* shapes, const int* picked, size_t n_picked, int L) {
  const int dim = 2 * L;
  for (size_t i = 0; i < n_picked; i++) {
    const int k = picked[i];
    typename D::Real* row = o;
    o = write_row<D>(o, frame, boxes + D::box * k, scores[k], shapes + (size_t)k * dim, dim);
    D::relocate(row + D::head, L, boxes + D::box * k);
  }
  return o;
}
// The rows of n results, frame_offset + i for results[i] (jdaResults[D]Pack): the number of rows, written to `rows` unless
// that is NULL; -1 (nothing written) when they are more than capacity_rows.
template <class D>
long long pack(const typename D::Result* results, int n, int frame_offset, typename D::Real* rows, long long capacity_rows) {
  long long total = 0;
  for (int i = 0; i < n; i++) total += results[i].n;
  if (!rows) return total;
  if (total > capacity_rows) return -1;
  for (int i = 0; i < n; i++) {
    const typename D::Result& r = results[i];
    const int dim = 2 * r.landmark_n;
    for (int j = 0; j < r.n; j++) rows = write_row<D>(rows, frame_offset + i, D::boxes(r) + D::box * j, r.scores[j], r.shapes + (size_t)j * dim, dim);
  }
  return total;
}

// Detection rows of a job, grown with realloc and handed to the caller as they are (jdaRowsRelease / jdaRowsDRelease = free).
template <typename T>
struct RowsOut {
  T* p = nullptr; size_t n = 0, cap = 0;          // n, cap in elements
  T* grow(size_t add) {                            // room for `add` more elements; returns where they start
    if (n + add > cap) {
      size_t nc = std::max<size_t>(std::max<size_t>(cap * 2, n + add), 1024);
      T* q = (T*)std::realloc(p, nc * sizeof(T));
      if (!q) throw std::bad_alloc();
      p = q; cap = nc;
    }
    T* at = p + n; n += add;
    return at;
  }
  T* release() { T* q = p ? p : (T*)std::malloc(sizeof(T)); p = nullptr; n = cap = 0; return q; }   // (never NULL on success)
  ~RowsOut() { std::free(p); }
  RowsOut() = default; RowsOut(const RowsOut&) = delete; RowsOut& operator=(const RowsOut&) = delete;
};

// Where the post-processing of a batch puts its frames: one result each (out[f]), or rows appended to *rows with frame
// index frame_offset + f.
template <class D>
struct Sink {
  typename D::Result* out = nullptr;
  RowsOut<typename D::Real>* rows = nullptr; int frame_offset = 0;
};

// ---- the window of a gid ----
// The frames of a batch: frame f's windows are the gids [gid0(f), gid0(f + 1)), its size w(f) x h(f).  A uniform batch
// (every frame `windows` windows of width x height) or, with the tables set, a ragged one.
struct FrameSet {
  int n = 0;
  long long windows = 0; int width = 0, height = 0;
  const uint32_t* gid_first = nullptr; const int* widths = nullptr; const int* heights = nullptr;   // n + 1, n, n
  long long gid0(int f) const { return gid_first ? (long long)gid_first[f] : (long long)f * windows; }
  int w(int f) const { return widths ? widths[f] : width; }
  int h(int f) const { return heights ? heights[f] : height; }
};

// The windows of one frame from its gids in ascending order: the levels' grids are those of c/jda.c:335-336 and
// cascador.cpp:333 for this frame's size, walked once.
class GidWalk {
 public:
  GidWalk(const std::vector<Level>& levels, int W, int H, uint32_t gid_first) : lv_(levels.data()), W_(W), H_(H), base_(gid_first) {}
  // (x, y, win) of gid g; g >= every gid asked for before
  void at(uint32_t g, int* x, int* y, int* win) {
    while (g >= base_ + (uint32_t)cnt_) {
      base_ += (uint32_t)cnt_;
      const Level& d = lv_[++l_];
      nx_ = (W_ - d.win) / d.step + 1;
      cnt_ = nx_ * ((H_ - d.win) / d.step + 1);
    }
    const uint32_t rel = g - base_;
    const Level& d = lv_[l_];
    *x = (int)(rel % (uint32_t)nx_) * d.step; *y = (int)(rel / (uint32_t)nx_) * d.step; *win = d.win;
  }
  template <class D>
  void box(uint32_t g, int* b) { int x, y, win; at(g, &x, &y, &win); D::window(x, y, win, b); }

 private:
  const Level* lv_; int W_, H_;
  uint32_t base_; int l_ = -1, nx_ = 1, cnt_ = 0;
};

// Frame and window of a gid of a uniform batch by a search through the levels (the method-0 pyramid, whose candidates
// are gathered level by level).
struct WinRef { int frame, x, y, win; };
inline WinRef locate(const ScanPlan& sp, uint32_t gid) {
  WinRef r;
  r.frame = (int)(gid / (uint32_t)sp.windows);
  const long long wid = gid - (long long)r.frame * sp.windows;
  size_t l = 0;
  for (size_t i = 1; i < sp.levels.size(); i++)
    if (wid >= sp.levels[i].base) l = i;
  const Level& lv = sp.levels[l];
  const long long rel = wid - lv.base;
  r.y = (int)(rel / lv.nx) * lv.step;
  r.x = (int)(rel % lv.nx) * lv.step;
  r.win = lv.win;
  return r;
}

}  // namespace jda
