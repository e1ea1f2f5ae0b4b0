// Patch numerics of dialect CPP, once, for k_misc.hip (pyramid and ROI resizes), k_mine.hip (Validate on crops, mining),
// k_train.hip (feature pool values), k_faces.hip (the positive set's patches) and, through cpp_wave.h, k_lbf.hip and
// k_reval.hip (a stage's / the model's carts over the sample set): one pixel of cv::resize(INTER_LINEAR), the split-node
// feature on o / h / q patches.
#pragma once
#include "kernels_common.h"

namespace jda {

namespace {

// cv::resize(INTER_LINEAR) for 8-bit single-channel images as dialect CPP uses it for the half / quarter images
// (cascador.cpp:329-331), the method-0 pyramid (cascador.cpp:300-303) and the trainer's patches (data.cpp:510-520,
// 987-990): 11-bit fixed-point bilinear of OpenCV's 2.4/3.x imgwarp.cpp, with its routing of an exact 2x2 down-scale to
// the box average.  PARITY UNPINNED (no OpenCV here to compare with); bit-exact against the oracle's restatement of the
// same algorithm.
struct CvResize { double sx, sy; int sw, sh, area, ident; };

__host__ __device__ __forceinline__ CvResize cv_resize_make(int sw, int sh, int dw, int dh) {
  CvResize r;
  r.sw = sw; r.sh = sh;
  const double inv_sx = (double)dw / sw, inv_sy = (double)dh / sh;
  r.sx = 1. / inv_sx; r.sy = 1. / inv_sy;
  r.area = (fabs(r.sx - 2.) < 2.220446049250313e-16 && fabs(r.sy - 2.) < 2.220446049250313e-16) ? 1 : 0;
  r.ident = (sw == dw && sh == dh) ? 1 : 0;     // (the bilinear formula then returns the source pixel itself)
  return r;
}

// Row y of a pixel source as a source of its own, `row(x)`: whatever `f(x, y)` computes from y alone is then formed once
// for the taps of a row (Pitched below: the row pointer).
template <typename F>
struct RowOf { const F& f; int y; __device__ __forceinline__ int operator()(int x) const { return f(x, y); } };
template <typename F>
__device__ __forceinline__ RowOf<F> row_of(const F& f, int y) { return RowOf<F>{f, y}; }

// One output pixel (dx, dy) of the resize of an sw x sh source whose pixels `f(x, y)` returns: a pitched image, a crop
// of a transformed background, a patch in LDS, or itself a resize.
template <typename F>
__device__ __forceinline__ int cv_resize_px(const F& f, const CvResize& r, int dx, int dy) {
  if (r.ident) return f(dx, dy);
  if (r.area) {
    const auto t0 = row_of(f, 2 * dy), t1 = row_of(f, 2 * dy + 1);
    return (t0(2 * dx) + t0(2 * dx + 1) + t1(2 * dx) + t1(2 * dx + 1) + 2) >> 2;
  }
  float fx = (float)(((double)dx + 0.5) * r.sx - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { fx = 0.f; sx = 0; }
  const bool edge = sx + 1 >= r.sw;            // dx >= xmax in OpenCV's loop
  if (sx >= r.sw - 1) { fx = 0.f; sx = r.sw - 1; }
  float fy = (float)(((double)dy + 0.5) * r.sy - 0.5);
  const int sy = (int)floorf(fy);
  fy -= (float)sy;
  auto sat_short = [](float v) { int i = __float2int_rn(v); return i < -32768 ? -32768 : (i > 32767 ? 32767 : i); };
  const int a0 = sat_short((1.f - fx) * 2048.f), a1 = sat_short(fx * 2048.f);
  const int b0 = sat_short((1.f - fy) * 2048.f), b1 = sat_short(fy * 2048.f);
  const int y0 = min(max(sy, 0), r.sh - 1), y1 = min(max(sy + 1, 0), r.sh - 1);
  const auto s0 = row_of(f, y0), s1 = row_of(f, y1);
  int r0, r1;
  if (!edge) { r0 = s0(sx) * a0 + s0(sx + 1) * a1; r1 = s1(sx) * a0 + s1(sx + 1) * a1; }
  else { r0 = s0(sx) * 2048; r1 = s1(sx) * 2048; }
  return ((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2) & 0xff;
}

// ... as a pixel source itself: pixel (x, y) of the resize r of the source f
template <typename F>
struct Resized { const F& f; const CvResize& r; __device__ __forceinline__ int operator()(int x, int y) const { return cv_resize_px(f, r, x, y); } };

// pixels of an image whose rows are `pitch` bytes apart
struct Pitched { const uint8_t* s; int pitch; __device__ __forceinline__ int operator()(int x, int y) const { return s[(size_t)y * pitch + x]; } };
struct PitchedRow { const uint8_t* s; __device__ __forceinline__ int operator()(int x) const { return s[x]; } };
__device__ __forceinline__ PitchedRow row_of(const Pitched& f, int y) { return PitchedRow{f.s + (size_t)y * f.pitch}; }

// A landmark coordinate plus a feature offset as a pixel of a patch of side pw (data.cpp:40-54, common.hpp:227-232).
__device__ __forceinline__ int coord_cpp(double s, double o, int pw) { return clamp_win(DialectCPP::coord(s, o, pw), pw); }

// Feature::CalcFeatureValue (data.cpp:18-58) inside a patch of side pw: the pixel of landmark (l1x, l1y) with offset
// (o1x, o1y) and that of landmark (l2x, l2y) with offset (o2x, o2y) ...
struct FeatXY { int x1, y1, x2, y2; };
__device__ __forceinline__ FeatXY feature_xy(int pw, double l1x, double l1y, double o1x, double o1y, double l2x, double l2y,
                                             double o2x, double o2y) {
  return FeatXY{coord_cpp(l1x, o1x, pw), coord_cpp(l1y, o1y, pw), coord_cpp(l2x, o2x, pw), coord_cpp(l2y, o2y, pw)};
}
// ... and their difference, the patch's pixels behind `px(x, y)`
template <typename F>
__device__ __forceinline__ int feature_diff(const F& px, const FeatXY& c) { return px(c.x1, c.y1) - px(c.x2, c.y2); }

// A sample's stored patches, o then h then q, tight (what MoreNegSamples keeps, data.cpp:510-520); scale is 0, 1 or 2
// (model.cpp and train.cpp refuse anything else).
struct PatchSet {
  const uint8_t* o; int os, hs, qs;
  template <typename Feat>       // NodeD-like: scale, o1x, o1y, o2x, o2y
  __device__ __forceinline__ int feature(const Feat& ft, double l1x, double l1y, double l2x, double l2y) const {
    // (from locals: a conditional on the members themselves keeps the whole struct in memory -- LDS, with this compiler)
    const int so = os, sh = hs, sq = qs, o2 = so * so, h2 = sh * sh;
    const int pw = ft.scale == 0 ? so : (ft.scale == 1 ? sh : sq);
    const uint8_t* p = o + (ft.scale == 0 ? 0 : (ft.scale == 1 ? o2 : o2 + h2));
    auto px = [&](int x, int y) {
      JDA_BC(Bc(0, (long long)pw * pw), y * pw + x, 1, kBcFinishPix);
      return (int)p[y * pw + x];
    };
    return feature_diff(px, feature_xy(pw, l1x, l1y, ft.o1x, ft.o1y, l2x, l2y, ft.o2x, ft.o2y));
  }
};

}  // namespace

}  // namespace jda
