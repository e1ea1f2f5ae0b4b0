// libjda.so, host side: frames whose faces are rolled (include/jda.h) -- jdaRotationPlan; the definition of jdaPackGrayRotated,
// plain loops over host memory (the device form is k_rotate.hip); and one face of jdaRotateBack, which takes what a detect call
// returned on rotated rectangles back into the source images.  The call path -- what is refused, the device entry, the way
// back's checks -- is frames.cpp's.  The plan is the only place that asks libm: host form, device form and way back take
// c, s, tw, th from it.
#include "frames.h"

#include <cmath>

namespace jda {

namespace {

constexpr double kRotMaxDegrees = 36000.0;
constexpr double kRotPi180 = 3.14159265358979323846 / 180.0;

// The plan's map: turned (u, v) -> the rectangle's (sx, sy).  One operation per step (-ffp-contract=off).
struct RotMap {
  double c, s, cu, cv, cx, cy;
  explicit RotMap(double c_, double s_, int w, int h, int tw, int th)
      : c(c_), s(s_), cu((double)(tw - 1) / 2), cv((double)(th - 1) / 2), cx((double)(w - 1) / 2), cy((double)(h - 1) / 2) {}
  void at(double u, double v, double* sx, double* sy) const {
    const double du = u - cu, dv = v - cv;
    const double a = c * du, b = s * dv;
    *sx = (a + b) + cx;
    const double e = c * dv, f = s * du;
    *sy = (e - f) + cy;
  }
};

template <class Real>
void back_landmarks(Real* lm, int L, const RotMap& m, const FrameOne& r) {
  for (int i = 0; i < L; i++) {
    double x, y;
    m.at((double)lm[2 * i], (double)lm[2 * i + 1], &x, &y);
    x = x + (double)r.x;
    y = y + (double)r.y;
    lm[2 * i] = (Real)x; lm[2 * i + 1] = (Real)y;
  }
}

}  // namespace

bool rotation_plan(const std::string& who, int w, int h, double degrees, jdaRotation* rot) {
  if (!rot) { fail(who + "null rot"); return false; }
  if (!std::isfinite(degrees) || std::fabs(degrees) > kRotMaxDegrees) {
    fail(who + "angle " + std::to_string(degrees) + " degrees (finite, at most 36000 either way)");
    return false;
  }
  if (w < 1 || h < 1) { fail(who + "w x h = " + std::to_string(w) + " x " + std::to_string(h) + ": a rectangle has at least one pixel"); return false; }
  double c, s;
  if (std::fmod(degrees, 90.0) == 0.0) {
    static const double tc[4] = {1.0, 0.0, -1.0, 0.0}, ts[4] = {0.0, 1.0, 0.0, -1.0};
    const int k = (int)((((long long)(degrees / 90.0)) % 4 + 4) % 4);   // (a multiple of 90 up to 36000 divides exactly)
    c = tc[k]; s = ts[k];
  } else {
    const double a = degrees * kRotPi180;
    c = std::cos(a); s = std::sin(a);
  }
  const double ac = std::fabs(c), as = std::fabs(s);
  const double w1 = (double)w * ac, w2 = (double)h * as, h1 = (double)w * as, h2 = (double)h * ac;
  const double ew = std::ceil((w1 + w2) - 1.0 / 1024), eh = std::ceil((h1 + h2) - 1.0 / 1024);
  if (ew > 2147483647.0 || eh > 2147483647.0) { fail(who + "the rotated size of " + std::to_string(w) + " x " + std::to_string(h) + " does not fit an int"); return false; }
  rot->c = c; rot->s = s; rot->w = w; rot->h = h;
  rot->tw = std::max(1, (int)ew); rot->th = std::max(1, (int)eh);
  return true;
}

void rotate_write(const std::vector<FrameOne>& v) {
  for (const FrameOne& o : v) {
    int wt[3] = {0, 0, 0};
    if (o.bpp > 1) pack_weights(o.format, wt);
    auto tap = [&](long long x, long long y) -> uint32_t {           // gray, rounded per tap; 0 outside the rectangle, which is never read
      if (x < 0 || x >= o.w || y < 0 || y >= o.h) return 0u;
      return gray_of(o.src + y * o.pitch + x * o.bpp, o.bpp, wt);
    };
    const RotMap m(o.c, o.s, o.w, o.h, o.tw, o.th);
    uint8_t* d = o.dst;
    for (int tv = 0; tv < o.th; tv++) {
      for (int tu = 0; tu < o.tw; tu++) {
        double sx, sy;
        m.at((double)tu, (double)tv, &sx, &sy);
        uint32_t out = 0;
        if (sx > -1.0 && sx < (double)o.w && sy > -1.0 && sy < (double)o.h) {
          const long long X = (long long)std::floor(sx * 1024 + 0.5), Y = (long long)std::floor(sy * 1024 + 0.5);
          const long long x0 = X >> 10, y0 = Y >> 10;
          const uint32_t fx = (uint32_t)(X & 1023), fy = (uint32_t)(Y & 1023);
          const uint32_t sum = tap(x0, y0) * ((1024 - fx) * (1024 - fy)) + tap(x0 + 1, y0) * (fx * (1024 - fy)) + tap(x0, y0 + 1) * ((1024 - fx) * fy) +
                               tap(x0 + 1, y0 + 1) * (fx * fy);
          out = (sum + (1u << 19)) >> 20;
        }
        *d++ = (uint8_t)out;
      }
    }
  }
}

void rotate_back_face(const BackCall& k, int f, const FrameOne& r) {
  const RotMap m(r.c, r.s, r.w, r.h, r.tw, r.th);
  if (k.boxes) {
    int* b = k.boxes + (size_t)f * k.box_ints;
    const int bw = b[2], bh = k.box_ints == 4 ? b[3] : b[2];
    const double hw = (double)(bw - 1) / 2, hh = (double)(bh - 1) / 2;
    double mx, my;
    m.at((double)b[0] + hw, (double)b[1] + hh, &mx, &my);
    b[0] = (int)std::floor((mx - hw) + 0.5) + r.x;
    b[1] = (int)std::floor((my - hh) + 0.5) + r.y;
  }
  if (k.landmarks) {
    if (k.real_bytes == 4) back_landmarks((float*)k.landmarks + (size_t)f * 2 * k.landmark_n, k.landmark_n, m, r);
    else back_landmarks((double*)k.landmarks + (size_t)f * 2 * k.landmark_n, k.landmark_n, m, r);
  }
}

}  // namespace jda
