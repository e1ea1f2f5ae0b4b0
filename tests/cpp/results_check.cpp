// Host check of the result module (jda_amd/csrc/results.h, no GPU), both dialects, on seeded random inputs:
//  - GidWalk's windows equal a brute-force enumeration of (level, y, x) -- for uniform plans (plan_dialect_c,
//    plan_dialect_cpp, plan_single_level, whose nx / ny must be the walk's grid formula) and for ragged images that take
//    a prefix of one level list -- and equal locate()'s for uniform plans;
//  - rows written straight from candidates (pick + write_rows) equal the rows pack() makes of emit()'s results;
//  - emit() with NMS off keeps every candidate, in order.
// Prints the number of failed checks.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "results.h"

using namespace jda;

static int bad = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      if (bad < 20) std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
      bad++;                                                            \
    }                                                                   \
  } while (0)

struct Win { int x, y, win; };

// every window of a W x H frame over the levels [0, nl), in scan order (level, y, x)
static std::vector<Win> enumerate(const std::vector<Level>& lv, int nl, int W, int H) {
  std::vector<Win> v;
  for (int l = 0; l < nl; l++)
    for (int y = 0; y + lv[l].win <= H; y += lv[l].step)
      for (int x = 0; x + lv[l].win <= W; x += lv[l].step) v.push_back({x, y, lv[l].win});
  return v;
}

// a sorted random subset of [0, n)
static std::vector<uint32_t> some(std::mt19937& rng, long long n, double p) {
  std::vector<uint32_t> v;
  std::bernoulli_distribution take(p);
  for (long long g = 0; g < n; g++) if (take(rng)) v.push_back((uint32_t)g);
  return v;
}

static void check_uniform(std::mt19937& rng, const ScanPlan& sp) {
  for (const Level& lv : sp.levels) {
    CHECK(lv.nx == (sp.width - lv.win) / lv.step + 1);
    CHECK(lv.ny == (sp.height - lv.win) / lv.step + 1);
  }
  const std::vector<Win> all = enumerate(sp.levels, (int)sp.levels.size(), sp.width, sp.height);
  CHECK((long long)all.size() == sp.windows);
  const int frames = 3;
  const std::vector<uint32_t> gids = some(rng, frames * sp.windows, 0.05);
  size_t i = 0;
  for (int f = 0; f < frames; f++) {
    const FrameSet fs{frames, sp.windows, sp.width, sp.height};
    GidWalk walk(sp.levels, fs.w(f), fs.h(f), (uint32_t)fs.gid0(f));
    for (; i < gids.size() && (long long)gids[i] < fs.gid0(f + 1); i++) {
      int x, y, win;
      walk.at(gids[i], &x, &y, &win);
      const Win& want = all[(size_t)(gids[i] - fs.gid0(f))];
      CHECK(x == want.x && y == want.y && win == want.win);
      const WinRef r = locate(sp, gids[i]);
      CHECK(r.frame == f && r.x == x && r.y == y && r.win == win);
    }
  }
  CHECK(i == gids.size());
}

static void check_ragged(std::mt19937& rng, const std::vector<Level>& lv) {
  const int n = 1 + (int)(rng() % 6);
  std::vector<int> w(n), h(n);
  std::vector<uint32_t> first(n + 1, 0);
  std::vector<std::vector<Win>> all(n);
  const int top = lv.back().win + 40;
  for (int i = 0; i < n; i++) {
    w[i] = 1 + (int)(rng() % top); h[i] = 1 + (int)(rng() % top);
    int nl = 0;                                     // the prefix of the levels that fits the image
    while (nl < (int)lv.size() && lv[nl].win <= std::min(w[i], h[i])) nl++;
    all[i] = enumerate(lv, nl, w[i], h[i]);
    first[i + 1] = first[i] + (uint32_t)all[i].size();
  }
  FrameSet fs;
  fs.n = n; fs.gid_first = first.data(); fs.widths = w.data(); fs.heights = h.data();
  const std::vector<uint32_t> gids = some(rng, first[n], 0.1);
  size_t i = 0;
  for (int f = 0; f < n; f++) {
    GidWalk walk(lv, fs.w(f), fs.h(f), (uint32_t)fs.gid0(f));
    for (; i < gids.size() && (long long)gids[i] < fs.gid0(f + 1); i++) {
      int b[4];
      walk.box<DialectCpp>(gids[i], b);
      const Win& want = all[f][gids[i] - first[f]];
      CHECK(b[0] == want.x && b[1] == want.y && b[2] == want.win && b[3] == want.win);
    }
  }
  CHECK(i == gids.size());
}

template <class D>
static void check_emit_and_rows(std::mt19937& rng) {
  using Real = typename D::Real;
  const int n_img = 1 + (int)(rng() % 4), L = 1 + (int)(rng() % 5), dim = 2 * L;
  const bool nms = rng() % 4 != 0;
  const double overlap = 0.3;
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::vector<typename D::Result> res(n_img);
  std::vector<Real> direct;
  for (int f = 0; f < n_img; f++) {
    const int n = (int)(rng() % 40);
    std::vector<int> boxes((size_t)n * D::box);
    std::vector<Real> scores(n), shapes((size_t)n * dim);
    for (int k = 0; k < n; k++) {
      int x = (int)(rng() % 80), y = (int)(rng() % 80), win = 24 + (int)(rng() % 40);
      D::window(x, y, win, &boxes[(size_t)k * D::box]);
      scores[k] = (Real)(rng() % 8 == 0 ? 1.0 : u(rng) * 4.0 - 2.0);      // (ties, too)
      for (int q = 0; q < dim; q++) shapes[(size_t)k * dim + q] = (Real)u(rng);
    }
    emit<D>(boxes.data(), scores.data(), shapes.data(), n, L, nms, overlap, &res[f]);
    CHECK(res[f].landmark_n == L && D::boxes(res[f]) && res[f].scores && res[f].shapes);
    std::vector<int> keep;
    pick<D>(boxes.data(), scores.data(), n, nms, overlap, &keep);
    CHECK((int)keep.size() == res[f].n);
    const size_t at = direct.size();
    direct.resize(at + keep.size() * (D::head + dim));
    Real* end = write_rows<D>(direct.data() + at, 7 + f, boxes.data(), scores.data(), shapes.data(), keep.data(), keep.size(), L);
    CHECK(end == direct.data() + direct.size());
    if (!nms) {                                     // every candidate, in scan order, relocated
      CHECK(res[f].n == n);
      for (int k = 0; k < n && k < res[f].n; k++) {
        CHECK(std::memcmp(D::boxes(res[f]) + (size_t)k * D::box, &boxes[(size_t)k * D::box], D::box * sizeof(int)) == 0);
        CHECK(res[f].scores[k] == scores[k]);
        std::vector<Real> sh(shapes.begin() + (size_t)k * dim, shapes.begin() + (size_t)(k + 1) * dim);
        D::relocate(sh.data(), L, &boxes[(size_t)k * D::box]);
        CHECK(std::memcmp(res[f].shapes + (size_t)k * dim, sh.data(), dim * sizeof(Real)) == 0);
      }
    }
  }
  const long long rows = pack<D>(res.data(), n_img, 7, nullptr, 0);
  std::vector<Real> packed((size_t)rows * (D::head + dim));
  if (rows > 0) CHECK(pack<D>(res.data(), n_img, 7, packed.data(), rows - 1) == -1);
  CHECK(pack<D>(res.data(), n_img, 7, packed.data(), rows) == rows);
  CHECK(packed.size() == direct.size() && std::memcmp(packed.data(), direct.data(), packed.size() * sizeof(Real)) == 0);
  for (auto& r : res) {
    release<D>(&r);
    CHECK(r.n == 0 && !D::boxes(r) && !r.scores && !r.shapes && r.landmark_n == L);
  }
}

int main() {
  std::mt19937 rng(20261016);
  for (int it = 0; it < 200; it++) {
    const int W = 1 + (int)(rng() % 400), H = 1 + (int)(rng() % 400);
    ScanPlan sp;
    std::string err;
    const float scales[] = {1.1f, 1.25f, 1.5f, 2.0f};
    if (plan_dialect_c(W, H, scales[rng() % 4], (int)(rng() % 60), rng() % 3 ? -1 : 24 + (int)(rng() % 200), &sp, &err) && !sp.levels.empty()) {
      check_uniform(rng, sp);
      check_ragged(rng, sp.levels);
    }
    if (plan_dialect_cpp(W, H, 12 + (int)(rng() % 30), 1 + (int)(rng() % 8), 1.1 + 0.1 * (rng() % 5), &sp, &err) && !sp.levels.empty()) {
      check_uniform(rng, sp);
      check_ragged(rng, sp.levels);
    }
    if (plan_single_level(W, H, 12 + (int)(rng() % 40), 1 + (int)(rng() % 8), &sp, &err)) check_uniform(rng, sp);
    check_emit_and_rows<DialectC>(rng);
    check_emit_and_rows<DialectCpp>(rng);
  }
  std::printf("%d\n", bad);
  return bad != 0;
}
