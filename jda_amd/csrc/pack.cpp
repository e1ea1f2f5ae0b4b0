// libjda.so, host side: frames as they arrive (include/jda.h) -- jdaPackGray, a plain loop over host memory, and
// jdaPackGrayDevice on the kernel of k_pack.hip.  Both validate everything before a byte is written or anything is launched;
// the device form builds the image table and the item list of the launch, puts them into its lane's grow-only buffer and
// makes one launch for all images.  No model is read.  What the entries refuse about ONE image (check_pixels) is shared with
// chips.cpp, what they refuse about a call (check_pack) with turn.cpp and reduce.cpp.
#include "detect.h"

namespace jda {

namespace {

// Does [d0, d1) touch a byte the rectangle takes of any source row?  Row y takes [s + y * pitch, s + y * pitch + L).
bool touches_rows(const PackOne& s, uintptr_t d0, uintptr_t d1) {
  const long long L = (long long)s.w * s.bpp, s0 = (long long)(uintptr_t)s.src, a = (long long)d0, b = (long long)d1;
  // the first row that ends behind a
  long long y = 0;
  if (a - L - s0 >= 0) y = (a - L - s0) / s.pitch + 1;
  return y < s.h && s0 + y * s.pitch < b;
}

}  // namespace

// Everything jdaPackGray / jdaPackGrayDevice refuse (include/jda.h); on success one PackOne per image.  With orients (turn.cpp)
// an orientation outside 0..7 is refused like an unknown format; a turned image takes the same w * h bytes of dst.  With
// reduced (reduce.cpp) factors are needed, a factor outside 1..kReduceMax or above w or h is refused the same way, and image
// i takes (w / f) * (h / f) bytes of dst: npix, which every overlap check below reads.  With rotated (rotate.cpp) degrees are
// needed, an angle the plan refuses or a turned side above kRotMaxSide is refused the same way, and image i takes tw * th bytes.
bool check_pack(const std::string& who, const jdaPixels* images, const int* orients, bool turned, int n, unsigned char* dst,
                const size_t* dst_offsets, std::vector<PackOne>* out, const int* factors, bool reduced, const double* degrees, bool rotated) {
  if (n < 0) { fail(who + "negative number of images (n = " + std::to_string(n) + ")"); return false; }
  if (n == 0) return true;
  if (!images) { fail(who + "null images"); return false; }
  if (!dst) { fail(who + "null destination"); return false; }
  if (turned && !orients) { fail(who + "null orients"); return false; }
  if (reduced && !factors) { fail(who + "null factors"); return false; }
  if (rotated && !degrees) { fail(who + "null degrees"); return false; }
  if (!dst_offsets) { fail(who + "null dst_offsets"); return false; }
  out->resize((size_t)n);
  for (int i = 0; i < n; i++) {
    PixelsOne r;
    if (!check_pixels(who + "image " + std::to_string(i) + ": ", images[i], &r)) return false;
    PackOne& o = (*out)[(size_t)i];
    o.src = r.src;
    o.dst = dst + dst_offsets[i];
    o.pitch = r.pitch; o.npix = (long long)r.w * r.h; o.w = r.w; o.h = r.h; o.bpp = r.bpp; o.format = r.format; o.tf = 0; o.f = 1;
    o.c = o.s = 0; o.tw = o.th = 0;
    if (turned) {
      if (orients[i] < 0 || orients[i] > 7) { fail(who + "image " + std::to_string(i) + ": unknown orientation " + std::to_string(orients[i]) + " (0..7)"); return false; }
      o.tf = kTf[orients[i]];
    }
    if (reduced) {
      const int f = factors[i];
      if (f < 1 || f > kReduceMax) { fail(who + "image " + std::to_string(i) + ": factor " + std::to_string(f) + " (1.." + std::to_string(kReduceMax) + ")"); return false; }
      if (r.w < f || r.h < f) {
        fail(who + "image " + std::to_string(i) + ": a rectangle of " + std::to_string(r.w) + " x " + std::to_string(r.h) + " reduced by factor " + std::to_string(f) + " has no pixel");
        return false;
      }
      o.f = f; o.npix = (long long)(r.w / f) * (r.h / f);
    }
    if (rotated) {
      jdaRotation rot;
      if (!rotation_plan(who + "image " + std::to_string(i) + ": ", r.w, r.h, degrees[i], &rot)) return false;
      if (rot.tw > kRotMaxSide || rot.th > kRotMaxSide) {
        fail(who + "image " + std::to_string(i) + ": a rectangle of " + std::to_string(r.w) + " x " + std::to_string(r.h) + " rotated by " + std::to_string(degrees[i]) +
             " degrees is " + std::to_string(rot.tw) + " x " + std::to_string(rot.th) + " (at most " + std::to_string(kRotMaxSide) + " a side)");
        return false;
      }
      o.c = rot.c; o.s = rot.s; o.tw = rot.tw; o.th = rot.th; o.npix = (long long)rot.tw * rot.th;
    }
  }
  // two destination images that overlap: neighbours in address order
  std::vector<int> by_dst((size_t)n);
  std::iota(by_dst.begin(), by_dst.end(), 0);
  std::sort(by_dst.begin(), by_dst.end(), [&](int a, int b) { return (*out)[a].dst < (*out)[b].dst || ((*out)[a].dst == (*out)[b].dst && a < b); });
  for (int k = 0; k + 1 < n; k++) {
    const PackOne& a = (*out)[by_dst[k]]; const PackOne& b = (*out)[by_dst[k + 1]];
    if ((uintptr_t)a.dst + (uintptr_t)a.npix > (uintptr_t)b.dst) {
      const int i = std::min(by_dst[k], by_dst[k + 1]), j = std::max(by_dst[k], by_dst[k + 1]);
      fail(who + "the destinations of image " + std::to_string(i) + " (offset " + std::to_string(dst_offsets[i]) + ", " + std::to_string((*out)[i].npix) + " bytes) and image " +
           std::to_string(j) + " (offset " + std::to_string(dst_offsets[j]) + ", " + std::to_string((*out)[j].npix) + " bytes) overlap");
      return false;
    }
  }
  // a destination image that overlaps source rows: the sources by their first byte, with the running maximum of their last;
  // a destination looks back from the last source that begins in front of its end for as long as one may still reach it
  std::vector<int> by_src((size_t)n);
  std::iota(by_src.begin(), by_src.end(), 0);
  auto lo = [&](int i) { return (uintptr_t)(*out)[i].src; };
  auto hi = [&](int i) { const PackOne& s = (*out)[i]; return (uintptr_t)s.src + (uintptr_t)((long long)(s.h - 1) * s.pitch + (long long)s.w * s.bpp); };
  std::sort(by_src.begin(), by_src.end(), [&](int a, int b) { return lo(a) < lo(b); });
  std::vector<uintptr_t> reach((size_t)n);
  for (int k = 0; k < n; k++) reach[k] = std::max(hi(by_src[k]), k ? reach[k - 1] : (uintptr_t)0);
  for (int i = 0; i < n; i++) {
    const uintptr_t d0 = (uintptr_t)(*out)[i].dst, d1 = d0 + (uintptr_t)(*out)[i].npix;
    int k = (int)(std::partition_point(by_src.begin(), by_src.end(), [&](int j) { return lo(j) < d1; }) - by_src.begin()) - 1;
    for (; k >= 0 && reach[k] > d0; k--) {
      const int j = by_src[k];
      if (hi(j) > d0 && touches_rows((*out)[j], d0, d1)) {
        fail(who + "the destination of image " + std::to_string(i) + " (offset " + std::to_string(dst_offsets[i]) + ", " + std::to_string((*out)[i].npix) +
             " bytes) overlaps the source rows of image " + std::to_string(j));
        return false;
      }
    }
  }
  return true;
}

int pixels_bpp(int format) {
  switch (format) {
    case JDA_PIX_GRAY8: return 1;
    case JDA_PIX_BGR24: case JDA_PIX_RGB24: return 3;
    case JDA_PIX_BGRA32: case JDA_PIX_RGBA32: return 4;
  }
  return 0;
}

void pack_weights(int format, int w[3]) {
  const bool rgb = format == JDA_PIX_RGB24 || format == JDA_PIX_RGBA32;
  w[0] = rgb ? kGrayR : kGrayB; w[1] = kGrayG; w[2] = rgb ? kGrayB : kGrayR;
}

bool check_pixels(const std::string& img, const jdaPixels& p, PixelsOne* out) {
  if (!p.data) { fail(img + "null data"); return false; }
  const int bpp = pixels_bpp(p.format);
  if (!bpp) { fail(img + "unknown format " + std::to_string(p.format)); return false; }
  if (p.width < 1 || p.height < 1) { fail(img + "width x height = " + std::to_string(p.width) + " x " + std::to_string(p.height) + ": an image has at least one pixel"); return false; }
  if (p.pitch < (long long)p.width * bpp) {
    fail(img + "pitch " + std::to_string(p.pitch) + " is smaller than a row (width " + std::to_string(p.width) + " x " + std::to_string(bpp) + " bytes per pixel)");
    return false;
  }
  int x = p.x, y = p.y, w = p.w, h = p.h;
  const std::string rect = "rectangle (x, y, w, h) = (" + std::to_string(p.x) + ", " + std::to_string(p.y) + ", " + std::to_string(p.w) + ", " + std::to_string(p.h) + ")";
  if (w == 0 && h == 0) {
    if (x != 0 || y != 0) { fail(img + rect + ": w == h == 0 takes the whole image, from (0, 0)"); return false; }
    w = p.width; h = p.height;
  }
  if (w < 1 || h < 1) { fail(img + rect + ": w and h must be at least 1 (or both 0 for the whole image)"); return false; }
  if (x < 0 || y < 0 || (long long)x + w > p.width || (long long)y + h > p.height) {
    fail(img + rect + " leaves the image of " + std::to_string(p.width) + " x " + std::to_string(p.height));
    return false;
  }
  out->src = p.data + (long long)y * p.pitch + (long long)x * bpp;
  out->pitch = p.pitch; out->x = x; out->y = y; out->w = w; out->h = h; out->bpp = bpp; out->format = p.format;
  return true;
}

int pack_host(const jdaPixels* images, int n, unsigned char* dst, const size_t* dst_offsets) {
  std::vector<PackOne> v;
  if (!check_pack("jdaPackGray: ", images, nullptr, false, n, dst, dst_offsets, &v)) return -1;
  for (const PackOne& o : v) {
    uint8_t* d = o.dst;
    if (o.bpp == 1) {
      for (int y = 0; y < o.h; y++, d += o.w) std::memcpy(d, o.src + (long long)y * o.pitch, (size_t)o.w);
      continue;
    }
    int w[3];
    pack_weights(o.format, w);
    for (int y = 0; y < o.h; y++) {
      const uint8_t* s = o.src + (long long)y * o.pitch;
      for (int x = 0; x < o.w; x++, s += o.bpp) *d++ = (uint8_t)((s[0] * w[0] + s[1] * w[1] + s[2] * w[2] + 8192) >> 14);
    }
  }
  return 0;
}

void pack_stats(jdaPackStats* stats, const std::vector<PackOne>& v, const LaneCall& call) {
  if (!stats) return;
  long long pixels = 0, bytes_in = 0;
  for (const PackOne& o : v) { pixels += o.npix; bytes_in += o.npix * o.bpp; }
  stats->pixels = pixels; stats->bytes_in = bytes_in; stats->bytes_out = pixels; stats->launches = 1;
  stats->device_ms = call.device_ms; stats->call_ms = call.call_ms();
}

int pack_launch(LaneCall& call, const std::string& who, const std::vector<PackOne>& v, hipStream_t user_stream, jdaPackStats* stats) {
  // the image table (units: kernels.h) and the image of every workgroup's first unit
  const int n = (int)v.size();
  std::vector<PackImg> tab(v.size());
  long long total = 0, pixels = 0;
  for (int i = 0; i < n; i++) {
    const PackOne& o = v[(size_t)i];
    PackImg& t = tab[(size_t)i];
    pack_img(&t, o, total);
    const DstUnits u = dst_units(o.dst, o.npix);
    t.head = u.head; t.nq = u.nq; t.tail = u.tail;
    total += u.total();
    pixels += o.npix;
  }
  constexpr long long per = (long long)kPackBlock * kPackRounds;
  const long long groups = (total + per - 1) / per;
  if (groups > 0x7fffffffll) { fail(who + "too many pixels for one launch (" + std::to_string(pixels) + ")"); return -1; }
  std::vector<int> block_img((size_t)groups);
  for (long long b = 0, i = 0; b < groups; b++) {
    while (b * per >= tab[(size_t)i].first + tab[(size_t)i].nq + tab[(size_t)i].head + tab[(size_t)i].tail) i++;
    block_img[(size_t)b] = (int)i;
  }

  if (!call.open(user_stream)) return -1;
  const hipStream_t st = call.st;
  auto body = [&]() -> bool {
    PackImg* d_tab; int* d_blk;
    if (!call.upload(tab, block_img, &d_tab, &d_blk) || !call.begin()) return false;
    PackArgs a{d_tab, d_blk, n, total};
    JDA_HIP(launch_pack(a, st));
    return call.end() && call.sync();
  };
  if (!call.run(stats != nullptr, body)) return -1;
  pack_stats(stats, v, call);
  return 0;
}

int pack_device(Cascador* c, const jdaPixels* images, int n, unsigned char* d_dst, const size_t* dst_offsets, hipStream_t user_stream,
                jdaPackStats* stats) {
  LaneCall call(c);
  const std::string who = "jdaPackGrayDevice: ";
  if (!c) { fail(who + "null cascador"); return -1; }
  std::vector<PackOne> v;
  if (!check_pack(who, images, nullptr, false, n, d_dst, dst_offsets, &v)) return -1;
  if (stats) std::memset(stats, 0, sizeof *stats);
  return n == 0 ? 0 : pack_launch(call, who, v, user_stream, stats);
}

}  // namespace jda
