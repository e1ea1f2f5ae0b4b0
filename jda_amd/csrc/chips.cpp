// libjda.so, host side: faces as they leave (include/jda.h) -- the fit of a face's similarity transform, jdaFaceChips, the
// definition in plain loops over host memory, and jdaFaceChipsDevice on the kernel of k_chips.hip.  Both validate everything
// and fit every face before a byte is written or anything is launched; the device form puts the face and image records into
// its lane's grow-only buffer and makes one launch for all faces.  The model is read for its mean shape only.
#include "frames.h"

namespace jda {

namespace {

struct ChipsPlan {                    // a validated call
  std::vector<ChipImg> imgs;          // the WHOLE images
  std::vector<ChipFace> faces;
  int cbpp = 0, crgb = 0;
  long long chip_bytes = 0, bytes = 0, taps = 0;
};

// include/jda.h, "the fit": every operation in the header's order (the build compiles without contraction)
bool fit_face(const std::string& face, const void* landmarks, int real_bytes, long long f, int L, const double* tmpl, const unsigned char* use,
              double rect_x, double rect_y, double M[6]) {
  auto P = [&](int k) { return real_bytes == 4 ? (double)((const float*)landmarks)[f * 2 * L + k] : ((const double*)landmarks)[f * 2 * L + k]; };
  int m = 0;
  double sum_qx = 0., sum_qy = 0., sum_px = 0., sum_py = 0.;
  for (int i = 0; i < L; i++) {
    if (use && !use[i]) continue;
    const double qx = tmpl[2 * i], qy = tmpl[2 * i + 1], px = P(2 * i), py = P(2 * i + 1);
    if (!std::isfinite(qx) || !std::isfinite(qy)) { fail(face + "template point " + std::to_string(i) + " is not finite"); return false; }
    if (!std::isfinite(px) || !std::isfinite(py)) { fail(face + "landmark " + std::to_string(i) + " is not finite"); return false; }
    sum_qx = sum_qx + qx; sum_qy = sum_qy + qy; sum_px = sum_px + px; sum_py = sum_py + py;
    m++;
  }
  if (m < 2) { fail(face + "a similarity needs at least 2 landmarks, " + std::to_string(m) + " are used"); return false; }
  const double md = (double)m;
  const double mqx = sum_qx / md, mqy = sum_qy / md, mpx = sum_px / md, mpy = sum_py / md;
  double den = 0., sa = 0., sb = 0.;
  for (int i = 0; i < L; i++) {
    if (use && !use[i]) continue;
    const double cqx = tmpl[2 * i] - mqx, cqy = tmpl[2 * i + 1] - mqy, cpx = P(2 * i) - mpx, cpy = P(2 * i + 1) - mpy;
    den = den + (cqx * cqx + cqy * cqy);
    sa = sa + (cqx * cpx + cqy * cpy);
    sb = sb + (cqx * cpy - cqy * cpx);
  }
  if (den == 0.) { fail(face + "the used template points coincide (den == 0)"); return false; }
  const double a = sa / den, b = sb / den;
  M[0] = a; M[1] = -b; M[2] = (mpx - (a * mqx - b * mqy)) + rect_x;
  M[3] = b; M[4] = a; M[5] = (mpy - (b * mqx + a * mqy)) + rect_y;
  return true;
}

int auto_n(double a, double b) {
  const double s2 = a * a + b * b;
  return s2 <= 1. ? 1 : s2 <= 4. ? 2 : s2 <= 9. ? 3 : 4;
}

// Everything jdaFaceChips / jdaFaceChipsDevice refuse (include/jda.h) except a missing template; on success the records.
bool check_chips(const std::string& who, const ChipsCall& c, const double* tmpl, ChipsPlan* out) {
  if (!c.images) { fail(who + "null images"); return false; }
  if (!c.face_image) { fail(who + "null face_image"); return false; }
  if (!c.landmarks) { fail(who + "null landmarks"); return false; }
  if (!c.dst) { fail(who + "null destination"); return false; }
  if (c.n_images < 0) { fail(who + "negative number of images (n_images = " + std::to_string(c.n_images) + ")"); return false; }
  if (c.landmark_n < 1) { fail(who + "landmark_n = " + std::to_string(c.landmark_n) + ": at least 1"); return false; }
  if (c.real_bytes != 4 && c.real_bytes != 8) { fail(who + "real_bytes = " + std::to_string(c.real_bytes) + ": 4 (float landmarks) or 8 (double)"); return false; }
  if (c.chip_format != JDA_PIX_GRAY8 && c.chip_format != JDA_PIX_BGR24 && c.chip_format != JDA_PIX_RGB24) {
    fail(who + "unknown chip format " + std::to_string(c.chip_format) + " (JDA_PIX_GRAY8, JDA_PIX_BGR24 or JDA_PIX_RGB24)");
    return false;
  }
  if (c.chip_w < 1 || c.chip_w > 4096 || c.chip_h < 1 || c.chip_h > 4096) {
    fail(who + "chip_w x chip_h = " + std::to_string(c.chip_w) + " x " + std::to_string(c.chip_h) + ": each in 1..4096");
    return false;
  }
  if (c.supersample < 0 || c.supersample > 4) { fail(who + "supersample = " + std::to_string(c.supersample) + ": 0 (by the face's scale) or 1..4"); return false; }
  out->cbpp = pixels_bpp(c.chip_format); out->crgb = c.chip_format == JDA_PIX_RGB24;
  out->chip_bytes = (long long)c.chip_w * c.chip_h * out->cbpp;
  out->bytes = out->chip_bytes * c.n_faces;
  std::vector<PixelsOne> px((size_t)c.n_images);
  out->imgs.resize((size_t)c.n_images);
  const uintptr_t d0 = (uintptr_t)c.dst, d1 = d0 + (uintptr_t)out->bytes;
  for (int i = 0; i < c.n_images; i++) {
    const std::string img = who + "image " + std::to_string(i) + ": ";
    if (!check_pixels(img, c.images[i], &px[(size_t)i])) return false;
    const jdaPixels& p = c.images[i];
    const uintptr_t s0 = (uintptr_t)p.data, s1 = s0 + (uintptr_t)((long long)(p.height - 1) * p.pitch + (long long)p.width * px[(size_t)i].bpp);
    if (d0 < s1 && s0 < d1) { fail(img + "the destination (" + std::to_string(out->bytes) + " bytes) overlaps the image's bytes"); return false; }
    ChipImg& t = out->imgs[(size_t)i];
    t.data = p.data; t.pitch = p.pitch; t.width = p.width; t.height = p.height; t.bpp = px[(size_t)i].bpp;
    t.rgb = p.format == JDA_PIX_RGB24 || p.format == JDA_PIX_RGBA32;
  }
  out->faces.resize((size_t)c.n_faces);
  out->taps = 0;
  for (int f = 0; f < c.n_faces; f++) {
    const std::string face = who + "face " + std::to_string(f) + ": ";
    const int im = c.face_image[f];
    if (im < 0 || im >= c.n_images) { fail(face + "face_image = " + std::to_string(im) + " is outside [0, " + std::to_string(c.n_images) + ")"); return false; }
    ChipFace& r = out->faces[(size_t)f];
    if (!fit_face(face, c.landmarks, c.real_bytes, f, c.landmark_n, tmpl, c.use, (double)px[(size_t)im].x, (double)px[(size_t)im].y, r.m)) return false;
    r.image = im;
    r.n = c.supersample ? c.supersample : auto_n(r.m[0], r.m[3]);
    out->taps += (long long)c.chip_w * c.chip_h * r.n * r.n * 4;
  }
  return true;
}

// counts first: n_faces == 0 touches nothing, not even a NULL pointer
int check_counts(const std::string& who, const ChipsCall& c) {
  if (c.n_faces < 0) { fail(who + "negative number of faces (n_faces = " + std::to_string(c.n_faces) + ")"); return -1; }
  return c.n_faces == 0 ? 0 : 1;
}

// one tap of the definition into the chip's channel sums
inline void host_tap(const ChipImg& im, int cc, bool swap, long long x, long long y, uint32_t wgt, uint32_t acc[3]) {
  if (x < 0 || y < 0 || x >= im.width || y >= im.height) return;
  const uint8_t* p = im.data + y * im.pitch + x * im.bpp;
  if (im.bpp == 1) { for (int c = 0; c < cc; c++) acc[c] += wgt * p[0]; return; }
  if (cc == 1) {
    int w[3];
    pack_weights(im.rgb ? JDA_PIX_RGB24 : JDA_PIX_BGR24, w);
    acc[0] += wgt * (uint32_t)gray_of(p, im.bpp, w);
    return;
  }
  acc[0] += wgt * p[swap ? 2 : 0]; acc[1] += wgt * p[1]; acc[2] += wgt * p[swap ? 0 : 2];
}

void matrices_out(const ChipsPlan& pl, double* matrices) {
  if (!matrices) return;
  for (size_t f = 0; f < pl.faces.size(); f++) std::memcpy(matrices + 6 * f, pl.faces[f].m, sizeof(double) * 6);
}

}  // namespace

int chips_host(const ChipsCall& call) {
  const std::string who = "jdaFaceChips: ";
  const int k = check_counts(who, call);
  if (k <= 0) return k;
  if (!call.tmpl) { fail(who + "null template"); return -1; }
  ChipsPlan pl;
  if (!check_chips(who, call, call.tmpl, &pl)) return -1;
  matrices_out(pl, call.matrices);
  uint8_t* d = call.dst;
  for (const ChipFace& fc : pl.faces) {
    const ChipImg& im = pl.imgs[(size_t)fc.image];
    const bool swap = im.bpp > 1 && (im.rgb != 0) != (pl.crgb != 0);
    const int n = fc.n;
    const uint32_t nn = (uint32_t)(n * n);
    const double W = (double)im.width, H = (double)im.height;
    for (int v = 0; v < call.chip_h; v++) {
      for (int u = 0; u < call.chip_w; u++) {
        uint32_t acc[3] = {0u, 0u, 0u};
        for (int j = 0; j < n; j++) {
          const double cv = (double)v + (double)((2 * j + 1) - n) / (double)(2 * n);
          for (int i = 0; i < n; i++) {
            const double cu = (double)u + (double)((2 * i + 1) - n) / (double)(2 * n);
            const double sx = (fc.m[0] * cu + fc.m[1] * cv) + fc.m[2];
            const double sy = (fc.m[3] * cu + fc.m[4] * cv) + fc.m[5];
            if (!(sx > -1.0 && sx < W && sy > -1.0 && sy < H)) continue;
            const long long X = (long long)std::floor(sx * 1024.0 + 0.5), Y = (long long)std::floor(sy * 1024.0 + 0.5);
            const long long x0 = X >> 10, y0 = Y >> 10;
            const uint32_t fx = (uint32_t)(X & 1023), fy = (uint32_t)(Y & 1023);
            host_tap(im, pl.cbpp, swap, x0, y0, (1024u - fx) * (1024u - fy), acc);
            host_tap(im, pl.cbpp, swap, x0 + 1, y0, fx * (1024u - fy), acc);
            host_tap(im, pl.cbpp, swap, x0, y0 + 1, (1024u - fx) * fy, acc);
            host_tap(im, pl.cbpp, swap, x0 + 1, y0 + 1, fx * fy, acc);
          }
        }
        for (int c = 0; c < pl.cbpp; c++) *d++ = (uint8_t)(((acc[c] + nn * (1u << 19)) >> 20) / nn);
      }
    }
  }
  return 0;
}

int chips_device(Cascador* c, const ChipsCall& call, hipStream_t user_stream, jdaChipStats* stats) {
  LaneCall lc(c);
  const std::string who = "jdaFaceChipsDevice: ";
  if (!c) { fail(who + "null cascador"); return -1; }
  const int k = check_counts(who, call);
  if (k < 0) return -1;
  if (k == 0) { if (stats) std::memset(stats, 0, sizeof *stats); return 0; }
  // the template: the caller's, or the model's mean shape at the chip's size
  std::vector<double> own;
  const double* tmpl = call.tmpl;
  if (!tmpl) {
    if (call.landmark_n != c->hm.L) {
      fail(who + "landmark_n = " + std::to_string(call.landmark_n) + " but the model has " + std::to_string(c->hm.L) + " landmarks (the default template is its mean shape)");
      return -1;
    }
    own.resize((size_t)2 * c->hm.L);
    for (int i = 0; i < c->hm.L; i++) { own[2 * i] = c->hm.mean_shape[2 * i] * (double)call.chip_w; own[2 * i + 1] = c->hm.mean_shape[2 * i + 1] * (double)call.chip_h; }
    tmpl = own.data();
  }
  ChipsPlan pl;
  if (!check_chips(who, call, tmpl, &pl)) return -1;
  if (stats) std::memset(stats, 0, sizeof *stats);

  ChipArgs a{};
  const DstUnits u = dst_units(call.dst, pl.bytes);
  a.dst = call.dst; a.bytes = pl.bytes; a.head = u.head; a.nq = u.nq; a.tail = u.tail;
  a.n_faces = call.n_faces; a.n_images = call.n_images; a.cw = call.chip_w; a.ch = call.chip_h; a.cbpp = pl.cbpp; a.crgb = pl.crgb;
  if ((u.total() + kChipBlock - 1) / kChipBlock > 0x7fffffffll) { fail(who + "too many chip bytes for one launch (" + std::to_string(pl.bytes) + ")"); return -1; }

  if (!lc.launch_one(user_stream, stats != nullptr, pl.faces, pl.imgs, "launch_chips(a, st)", [&](ChipFace* d_faces, ChipImg* d_imgs, hipStream_t st) {
        a.faces = d_faces; a.imgs = d_imgs;
        return launch_chips(a, st);
      })) return -1;
  matrices_out(pl, call.matrices);
  if (stats) {
    stats->faces = call.n_faces; stats->chip_bytes = pl.bytes; stats->taps = pl.taps; stats->launches = 1;
    stats->device_ms = lc.device_ms; stats->call_ms = lc.call_ms();
  }
  return 0;
}

}  // namespace jda
