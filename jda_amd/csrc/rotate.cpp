// libjda.so, host side: frames whose faces are rolled (include/jda.h) -- jdaRotationPlan; jdaPackGrayRotated, plain loops over
// the definition in host memory; jdaPackGrayRotatedDevice on the kernel of k_rotate.hip; jdaRotateBack, which takes what a
// detect call returned on rotated rectangles back into the source images.  The pack entries refuse what pack.cpp's refuse
// (check_pack, shared, with the angles) and with every angle a multiple of 90 they ARE turn.cpp's; the way back is turn.cpp's
// orient_back with an angle per image.  The device form builds the image table and the item list (a tile per workgroup: the
// tiles of turn.cpp, of the rotated image), puts them into its lane's grow-only buffer and makes one launch.  The plan is
// the only place that asks libm: host form, device form and way back take c, s, tw, th from it.
#include "detect.h"

#include <cmath>

namespace jda {

namespace {

constexpr double kRotMaxDegrees = 36000.0;
constexpr double kRotPi180 = 3.14159265358979323846 / 180.0;

bool check_rotated(const std::string& who, const jdaPixels* images, const double* degrees, int n, unsigned char* dst, const size_t* dst_offsets,
                   std::vector<PackOne>* v) {
  return check_pack(who, images, nullptr, false, n, dst, dst_offsets, v, nullptr, false, degrees, true);
}

// every angle a multiple of 90: the images as turn.cpp takes them (orientation 0 / 1 / 2 / 3 by the plan's exact table)
bool all_quarter_turns(std::vector<PackOne>* v) {
  for (const PackOne& o : *v) if (!((o.c == 0.0 && std::fabs(o.s) == 1.0) || (o.s == 0.0 && std::fabs(o.c) == 1.0))) return false;
  for (PackOne& o : *v) o.tf = kTf[o.c == 1.0 ? 0 : o.s == 1.0 ? 1 : o.c == -1.0 ? 2 : 3];
  return true;
}

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
void back_landmarks(Real* lm, int L, const RotMap& m, const PixelsOne& r) {
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

int rotation_plan(int w, int h, double degrees, jdaRotation* rot) { return rotation_plan("jdaRotationPlan: ", w, h, degrees, rot) ? 0 : -1; }

int rotate_host(const jdaPixels* images, const double* degrees, int n, unsigned char* dst, const size_t* dst_offsets) {
  std::vector<PackOne> v;
  if (!check_rotated("jdaPackGrayRotated: ", images, degrees, n, dst, dst_offsets, &v)) return -1;
  if (all_quarter_turns(&v)) { turn_write(v); return 0; }           // jdaPackGrayOriented's bytes
  for (const PackOne& o : v) {
    int wt[3] = {0, 0, 0};
    if (o.bpp > 1) pack_weights(o.format, wt);
    auto tap = [&](long long x, long long y) -> uint32_t {           // gray, rounded per tap; 0 outside the rectangle, which is never read
      if (x < 0 || x >= o.w || y < 0 || y >= o.h) return 0u;
      const uint8_t* p = o.src + y * o.pitch + x * o.bpp;
      return o.bpp == 1 ? p[0] : (uint32_t)((p[0] * wt[0] + p[1] * wt[1] + p[2] * wt[2] + 8192) >> 14);
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
  return 0;
}

int rotate_device(Cascador* c, const jdaPixels* images, const double* degrees, int n, unsigned char* d_dst, const size_t* dst_offsets,
                  hipStream_t user_stream, jdaPackStats* stats) {
  LaneCall call(c);
  const std::string who = "jdaPackGrayRotatedDevice: ";
  if (!c) { fail(who + "null cascador"); return -1; }
  std::vector<PackOne> v;
  if (!check_rotated(who, images, degrees, n, d_dst, dst_offsets, &v)) return -1;
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (n == 0) return 0;
  if (all_quarter_turns(&v)) return turn_launch(call, who, v, user_stream, stats);   // the same bytes

  std::vector<RotImg> tab;
  std::vector<int> block_img;
  long long total;
  if (!turn_tiles(who, v, &tab, &block_img, &total)) return -1;
  if (!call.open(user_stream)) return -1;
  const hipStream_t st = call.st;
  auto body = [&]() -> bool {
    RotImg* d_tab; int* d_blk;
    if (!call.upload(tab, block_img, &d_tab, &d_blk) || !call.begin()) return false;
    RotArgs a{d_tab, d_blk, n, total};
    JDA_HIP(launch_rotate(a, st));
    return call.end() && call.sync();
  };
  if (!call.run(stats != nullptr, body)) return -1;
  if (stats) {
    long long pixels = 0, bytes_in = 0;
    for (const PackOne& o : v) { pixels += o.npix; bytes_in += (long long)o.w * o.h * o.bpp; }
    stats->pixels = pixels; stats->bytes_in = bytes_in; stats->bytes_out = pixels; stats->launches = 1;
    stats->device_ms = call.device_ms; stats->call_ms = call.call_ms();
  }
  return 0;
}

void rotate_back_face(const OrientBackCall& k, int f, const PixelsOne& r, const jdaRotation& rot) {
  const RotMap m(rot.c, rot.s, rot.w, rot.h, rot.tw, rot.th);
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

int rotate_back(const OrientBackCall& k, const double* degrees) {
  const std::string who = "jdaRotateBack: ";
  if (k.n_faces > 0 && !degrees) { fail(who + "null degrees"); return -1; }
  return orient_back(who, k, nullptr, k.n_faces > 0 ? degrees : nullptr);
}

}  // namespace jda
