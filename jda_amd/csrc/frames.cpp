// libjda.so, host side: the one call path of the frame entries (include/jda.h) -- jdaPackGray, jdaPackGrayOriented,
// jdaPackGrayReduced, jdaPackGrayRotated, their Device forms, and the way back (jdaOrientBack, jdaReduceBack, jdaRotateBack).
// A call names its kind and hands over its arrays (FrameSpec); everything is validated before a byte is written or anything is
// launched, and every image comes out of the checks as ONE record (FrameOne) that holds every size the rest needs: the host
// loops (pack.cpp, turn.cpp, reduce.cpp, rotate.cpp), the tables of the one launch, the statistics and the way back read it
// and compute none again.  The device form builds the image table and the item list of the launch, puts them into its lane's
// grow-only buffer and makes one launch for all images.  No model is read.
#include "frames.h"

namespace jda {

namespace {

const char* const kPackName[4] = {"jdaPackGray", "jdaPackGrayOriented", "jdaPackGrayReduced", "jdaPackGrayRotated"};
const char* const kBackName[4] = {"", "jdaOrientBack", "jdaReduceBack", "jdaRotateBack"};

// Does [d0, d1) touch a byte the rectangle takes of any source row?  Row y takes [s + y * pitch, s + y * pitch + L).
bool touches_rows(const FrameOne& s, uintptr_t d0, uintptr_t d1) {
  const long long L = (long long)s.w * s.bpp, s0 = (long long)(uintptr_t)s.src, a = (long long)d0, b = (long long)d1;
  // the first row that ends behind a
  long long y = 0;
  if (a - L - s0 >= 0) y = (a - L - s0) / s.pitch + 1;
  return y < s.h && s0 + y * s.pitch < b;
}

// Everything the pack entries refuse (include/jda.h); on success one FrameOne per image, dst set.  Image i takes npix bytes of
// dst, which every overlap check below reads.  A rotated side above kRotMaxSide is refused here, not on the way back.
bool check_pack(const std::string& who, const FrameSpec& spec, const jdaPixels* images, int n, unsigned char* dst, const size_t* dst_offsets,
                std::vector<FrameOne>* out) {
  if (n < 0) { fail(who + "negative number of images (n = " + std::to_string(n) + ")"); return false; }
  if (n == 0) return true;
  if (!images) { fail(who + "null images"); return false; }
  if (!dst) { fail(who + "null destination"); return false; }
  if (spec.kind == kTurn && !spec.orients) { fail(who + "null orients"); return false; }
  if (spec.kind == kReduce && !spec.factors) { fail(who + "null factors"); return false; }
  if (spec.kind == kRotate && !spec.degrees) { fail(who + "null degrees"); return false; }
  if (!dst_offsets) { fail(who + "null dst_offsets"); return false; }
  out->resize((size_t)n);
  for (int i = 0; i < n; i++) {
    const std::string img = who + "image " + std::to_string(i) + ": ";
    PixelsOne r;
    FrameOne& o = (*out)[(size_t)i];
    if (!check_pixels(img, images[i], &r) || !frame_one(img, spec, i, r, &o)) return false;
    if (o.kind == kRotate && (o.tw > kRotMaxSide || o.th > kRotMaxSide)) {
      fail(img + "a rectangle of " + std::to_string(o.w) + " x " + std::to_string(o.h) + " rotated by " + std::to_string(spec.degrees[i]) + " degrees is " +
           std::to_string(o.tw) + " x " + std::to_string(o.th) + " (at most " + std::to_string(kRotMaxSide) + " a side)");
      return false;
    }
    o.dst = dst + dst_offsets[i];
  }
  // two destination images that overlap: neighbours in address order
  std::vector<int> by_dst((size_t)n);
  std::iota(by_dst.begin(), by_dst.end(), 0);
  std::sort(by_dst.begin(), by_dst.end(), [&](int a, int b) { return (*out)[a].dst < (*out)[b].dst || ((*out)[a].dst == (*out)[b].dst && a < b); });
  for (int k = 0; k + 1 < n; k++) {
    const FrameOne& a = (*out)[by_dst[k]]; const FrameOne& b = (*out)[by_dst[k + 1]];
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
  auto hi = [&](int i) { const FrameOne& s = (*out)[i]; return (uintptr_t)s.src + (uintptr_t)((long long)(s.h - 1) * s.pitch + (long long)s.w * s.bpp); };
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

// The kind whose loop / launch gives a valid call's bytes: every angle a multiple of 90 -- the images as kTurn takes them
// (orientation 0 / 1 / 2 / 3 by the plan's exact table); every factor 1 -- kTurn; every orientation 0 -- kPack
FrameKind settle(FrameKind k, std::vector<FrameOne>* v) {
  if (k == kRotate && std::all_of(v->begin(), v->end(), [](const FrameOne& o) { return (o.c == 0.0 && std::fabs(o.s) == 1.0) || (o.s == 0.0 && std::fabs(o.c) == 1.0); })) {
    for (FrameOne& o : *v) { o.orient = o.c == 1.0 ? 0 : o.s == 1.0 ? 1 : o.c == -1.0 ? 2 : 3; o.tf = kTf[o.orient]; }
    k = kTurn;
  }
  if (k == kReduce && std::all_of(v->begin(), v->end(), [](const FrameOne& o) { return o.f == 1; })) k = kTurn;
  if (k == kTurn && std::all_of(v->begin(), v->end(), [](const FrameOne& o) { return o.tf == 0; })) k = kPack;
  return k;
}

bool one_launch(const std::string& who, long long groups, const std::vector<FrameOne>& v) {
  if (groups <= 0x7fffffffll) return true;
  long long pixels = 0;
  for (const FrameOne& o : v) pixels += o.npix;
  fail(who + "too many pixels for one launch (" + std::to_string(pixels) + ")");
  return false;
}

// What PackImg, TurnImg and RotImg have in common, the rest zero: the image, its first unit / tile in the launch and the Q14
// weights, split into their low and high bytes
template <typename Img>
void frame_img(Img* t, const FrameOne& o, long long first) {
  std::memset(t, 0, sizeof *t);
  t->src = o.src; t->dst = o.dst; t->pitch = o.pitch; t->w = o.w; t->h = o.h; t->bpp = o.bpp; t->first = first;
  if (o.bpp == 1) return;
  int w[3];
  pack_weights(o.format, w);
  t->w_lo = (uint32_t)(w[0] & 255) | ((uint32_t)(w[1] & 255) << 8) | ((uint32_t)(w[2] & 255) << 16);
  t->w_hi = (uint32_t)(w[0] >> 8) | ((uint32_t)(w[1] >> 8) << 8) | ((uint32_t)(w[2] >> 8) << 16);
}
void tile_img(TurnImg* t, const FrameOne& o) { t->w = o.rw; t->h = o.rh; t->tf = o.tf; t->f = o.f; }
void tile_img(RotImg* t, const FrameOne& o) { t->c = o.c; t->s = o.s; t->tw = o.tw; t->th = o.th; }

// k_pack's image table (units: kernels.h) and the image of every workgroup's first unit
bool frame_table(const std::string& who, const std::vector<FrameOne>& v, std::vector<PackImg>* tab, std::vector<int>* block_img, long long* total_out) {
  const int n = (int)v.size();
  tab->resize((size_t)n);
  long long total = 0;
  for (int i = 0; i < n; i++) {
    PackImg& t = (*tab)[(size_t)i];
    frame_img(&t, v[(size_t)i], total);
    const DstUnits u = dst_units(t.dst, v[(size_t)i].npix);
    t.head = u.head; t.nq = u.nq; t.tail = u.tail;
    total += u.total();
  }
  constexpr long long per = (long long)kPackBlock * kPackRounds;
  const long long groups = (total + per - 1) / per;
  if (!one_launch(who, groups, v)) return false;
  block_img->resize((size_t)groups);
  for (long long b = 0, i = 0; b < groups; b++) {
    while (b * per >= (*tab)[(size_t)i].first + (*tab)[(size_t)i].nq + (*tab)[(size_t)i].head + (*tab)[(size_t)i].tail) i++;
    (*block_img)[(size_t)b] = (int)i;
  }
  *total_out = total;
  return true;
}
// The image table of a launch that deals 64 x 64 tiles of the tw x th images (TurnImg, RotImg: kernels.h) and the image of
// every workgroup's tile
template <typename Img>
bool frame_table(const std::string& who, const std::vector<FrameOne>& v, std::vector<Img>* tab, std::vector<int>* block_img, long long* total_out) {
  const int n = (int)v.size();
  tab->resize((size_t)n);
  long long total = 0;
  for (int i = 0; i < n; i++) {
    const FrameOne& o = v[(size_t)i];
    Img& t = (*tab)[(size_t)i];
    frame_img(&t, o, total);
    tile_img(&t, o);
    t.off = (int)((uintptr_t)o.dst & 15);
    t.ntu = (int)(((long long)o.tw + t.off + kTurnTile - 1) / kTurnTile);
    t.ntv = (o.th + kTurnTile - 1) / kTurnTile;
    total += (long long)t.ntu * t.ntv;
  }
  if (!one_launch(who, total, v)) return false;
  block_img->resize((size_t)total);
  for (int i = 0; i < n; i++) std::fill_n(block_img->begin() + (*tab)[(size_t)i].first, (long long)(*tab)[(size_t)i].ntu * (*tab)[(size_t)i].ntv, i);
  *total_out = total;
  return true;
}

// jdaPackStats of a call that made its one launch; bytes_in: the pixels that take part
void pack_stats(jdaPackStats* stats, const std::vector<FrameOne>& v, const LaneCall& call) {
  if (!stats) return;
  long long pixels = 0, bytes_in = 0;
  for (const FrameOne& o : v) { pixels += o.npix; bytes_in += (long long)o.rw * o.f * o.rh * o.f * o.bpp; }
  stats->pixels = pixels; stats->bytes_in = bytes_in; stats->bytes_out = pixels; stats->launches = 1;
  stats->device_ms = call.device_ms; stats->call_ms = call.call_ms();
}

// The one launch of a valid call (at least one image), in the name `who` of the entry the caller called; `what` names the
// launcher where the launch fails
template <typename Img>
int frames_launch(LaneCall& call, const std::string& who, const std::vector<FrameOne>& v, hipStream_t user_stream, jdaPackStats* stats,
                  const char* what, hipError_t (*launch)(const FrameArgs<Img>&, hipStream_t)) {
  std::vector<Img> tab;
  std::vector<int> block_img;
  long long total;
  if (!frame_table(who, v, &tab, &block_img, &total)) return -1;
  const int n = (int)v.size();
  if (!call.launch_one(user_stream, stats != nullptr, tab, block_img, what,
                       [&](Img* d_tab, int* d_blk, hipStream_t st) { return launch(FrameArgs<Img>{d_tab, d_blk, n, total}, st); })) return -1;
  pack_stats(stats, v, call);
  return 0;
}

}  // namespace

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

bool check_orient(const std::string& pre, int orient) {
  if (orient >= 0 && orient <= 7) return true;
  fail(pre + "unknown orientation " + std::to_string(orient) + " (0..7)");
  return false;
}

bool check_factor(const std::string& pre, int factor) {
  if (factor >= 1 && factor <= kReduceMax) return true;
  fail(pre + "factor " + std::to_string(factor) + " (1.." + std::to_string(kReduceMax) + ")");
  return false;
}

bool frame_one(const std::string& img, const FrameSpec& spec, int i, const PixelsOne& r, FrameOne* o) {
  o->src = r.src; o->dst = nullptr; o->pitch = r.pitch;
  o->x = r.x; o->y = r.y; o->w = r.w; o->h = r.h; o->bpp = r.bpp; o->format = r.format;
  o->kind = spec.kind; o->orient = 0; o->tf = 0; o->f = 1; o->c = o->s = 0;
  if (spec.kind == kRotate) {
    jdaRotation rot;
    if (!rotation_plan(img, r.w, r.h, spec.degrees[i], &rot)) return false;
    o->c = rot.c; o->s = rot.s; o->rw = r.w; o->rh = r.h; o->tw = rot.tw; o->th = rot.th;
  } else {
    if (spec.kind != kPack && spec.orients) {
      if (!check_orient(img, spec.orients[i])) return false;
      o->orient = spec.orients[i]; o->tf = kTf[o->orient];
    }
    if (spec.kind == kReduce) {
      const int f = spec.factors[i];
      if (!check_factor(img, f)) return false;
      if (r.w < f || r.h < f) {
        fail(img + "a rectangle of " + std::to_string(r.w) + " x " + std::to_string(r.h) + " reduced by factor " + std::to_string(f) + " has no pixel");
        return false;
      }
      o->f = f;
    }
    const FrameSize z = frame_size(r.w, r.h, o->f, o->tf);
    o->rw = z.rw; o->rh = z.rh; o->tw = z.tw; o->th = z.th;
  }
  o->npix = (long long)o->tw * o->th;
  return true;
}

int frames_host(const FrameSpec& spec, const jdaPixels* images, int n, unsigned char* dst, const size_t* dst_offsets) {
  std::vector<FrameOne> v;
  if (!check_pack(std::string(kPackName[spec.kind]) + ": ", spec, images, n, dst, dst_offsets, &v)) return -1;
  switch (settle(spec.kind, &v)) {                                  // (a kind that settles lower writes the lower kind's bytes)
    case kPack: pack_write(v); break;
    case kTurn: turn_write(v); break;
    case kReduce: reduce_write(v); break;
    case kRotate: rotate_write(v); break;
  }
  return 0;
}

int frames_device(Cascador* c, const FrameSpec& spec, const jdaPixels* images, int n, unsigned char* d_dst, const size_t* dst_offsets,
                  hipStream_t user_stream, jdaPackStats* stats) {
  LaneCall call(c);
  const std::string who = std::string(kPackName[spec.kind]) + "Device: ";
  if (!c) { fail(who + "null cascador"); return -1; }
  std::vector<FrameOne> v;
  if (!check_pack(who, spec, images, n, d_dst, dst_offsets, &v)) return -1;
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (n == 0) return 0;
  switch (settle(spec.kind, &v)) {                                  // (... makes the lower kind's launch: the same bytes)
    case kPack: return frames_launch<PackImg>(call, who, v, user_stream, stats, "launch_pack(a, st)", launch_pack);
    case kTurn: return frames_launch<TurnImg>(call, who, v, user_stream, stats, "launch_turn(a, st)", launch_turn);
    case kReduce: return frames_launch<TurnImg>(call, who, v, user_stream, stats, "launch_reduce(a, st)", launch_reduce);
    case kRotate: return frames_launch<RotImg>(call, who, v, user_stream, stats, "launch_rotate(a, st)", launch_rotate);
  }
  return -1;
}

int frames_back(const FrameSpec& spec, const BackCall& k) {
  const std::string who = std::string(kBackName[spec.kind]) + ": ";
  if (k.n_faces > 0 && spec.kind == kReduce && !spec.factors) { fail(who + "null factors"); return -1; }
  if (k.n_faces > 0 && spec.kind == kRotate && !spec.degrees) { fail(who + "null degrees"); return -1; }
  if (k.n_faces < 0) { fail(who + "negative number of faces (n_faces = " + std::to_string(k.n_faces) + ")"); return -1; }
  if (k.n_images < 0) { fail(who + "negative number of images (n_images = " + std::to_string(k.n_images) + ")"); return -1; }
  if (k.n_faces == 0) return 0;
  if (!k.images) { fail(who + "null images"); return -1; }
  if (spec.kind != kRotate && !spec.orients) { fail(who + "null orients"); return -1; }
  if (!k.face_image) { fail(who + "null face_image"); return -1; }
  if (k.boxes && k.box_ints != 3 && k.box_ints != 4) { fail(who + "box_ints = " + std::to_string(k.box_ints) + ": 3 (x, y, size) or 4 (x, y, w, h)"); return -1; }
  if (k.landmarks) {
    if (k.real_bytes != 4 && k.real_bytes != 8) { fail(who + "real_bytes = " + std::to_string(k.real_bytes) + ": 4 (float) or 8 (double)"); return -1; }
    if (k.landmark_n < 1) { fail(who + "landmark_n = " + std::to_string(k.landmark_n) + ": at least one landmark"); return -1; }
    if (k.sym_n < 0) { fail(who + "negative number of pairs (sym_n = " + std::to_string(k.sym_n) + ")"); return -1; }
    if (k.sym_n > 0 && (!k.left || !k.right)) { fail(who + "null left or right"); return -1; }
    for (int j = 0; j < k.sym_n; j++) {
      if (k.left[j] < 0 || k.left[j] >= k.landmark_n || k.right[j] < 0 || k.right[j] >= k.landmark_n) {
        fail(who + "pair " + std::to_string(j) + " = (" + std::to_string(k.left[j]) + ", " + std::to_string(k.right[j]) + ") names a landmark outside [0, " +
             std::to_string(k.landmark_n) + ")");
        return -1;
      }
    }
  }
  std::vector<FrameOne> img((size_t)k.n_images);
  for (int i = 0; i < k.n_images; i++) {
    const std::string pre = who + "image " + std::to_string(i) + ": ";
    PixelsOne r;
    if (!check_pixels(pre, k.images[i], &r) || !frame_one(pre, spec, i, r, &img[(size_t)i])) return -1;
  }
  for (int f = 0; f < k.n_faces; f++) {
    if (k.face_image[f] < 0 || k.face_image[f] >= k.n_images) {
      fail(who + "face " + std::to_string(f) + ": face_image " + std::to_string(k.face_image[f]) + " is outside [0, " + std::to_string(k.n_images) + ")");
      return -1;
    }
  }
  for (int f = 0; f < k.n_faces; f++) {
    const FrameOne& o = img[(size_t)k.face_image[f]];
    if (o.kind == kRotate) rotate_back_face(k, f, o); else turn_back_face(k, f, o);
  }
  return 0;
}

}  // namespace jda
