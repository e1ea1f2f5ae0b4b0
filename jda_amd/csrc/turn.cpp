// libjda.so, host side: frames in any orientation (include/jda.h) -- jdaOrientSize; jdaPackGrayOriented, plain loops over the
// definition in host memory; jdaPackGrayOrientedDevice on the kernel of k_turn.hip; jdaOrientBack, which takes what a detect
// call returned on turned rectangles back into the source images.  The pack entries refuse what pack.cpp's refuse (check_pack,
// shared) and an orientation outside 0..7; with every orientation 0 they ARE pack.cpp's.  The device form builds the image
// table and the item list (a tile per workgroup), puts them into its lane's grow-only buffer and makes one launch.
#include "detect.h"

namespace jda {

namespace {

// faces [0, n): landmarks in place, the type's own precision, one operation per line.  w x h: the rectangle as it was turned
// (reduced by f, if f: then a reduced pixel's centre goes to the centre of its f x f block, c = (f - 1) / 2)
template <class Real>
void back_landmarks(Real* lm, int L, int tf, bool mirror, const PixelsOne& r, int w, int h, int f, const int* left, const int* right, int sym_n) {
  const Real c = (Real)(f - 1) / 2;
  for (int i = 0; i < L; i++) {
    Real x = lm[2 * i], y = lm[2 * i + 1];
    if (tf & kMineSwap) std::swap(x, y);
    if (tf & kMineFlipX) x = (Real)(w - 1) - x;
    if (tf & kMineFlipY) y = (Real)(h - 1) - y;
    if (f) {
      x = x * (Real)f;
      y = y * (Real)f;
      x = x + c;
      y = y + c;
    }
    x = x + (Real)r.x;
    y = y + (Real)r.y;
    lm[2 * i] = x; lm[2 * i + 1] = y;
  }
  if (!mirror) return;
  for (int j = 0; j < sym_n; j++) {                 // sequentially, in list order: a landmark named in two pairs is swapped twice
    std::swap(lm[2 * left[j]], lm[2 * right[j]]);
    std::swap(lm[2 * left[j] + 1], lm[2 * right[j] + 1]);
  }
}

}  // namespace

int orient_size(int w, int h, int orient, int* tw, int* th) {
  const std::string who = "jdaOrientSize: ";
  if (!tw || !th) { fail(who + "null tw or th"); return -1; }
  if (orient < 0 || orient > 7) { fail(who + "unknown orientation " + std::to_string(orient) + " (0..7)"); return -1; }
  if (w < 0 || h < 0) { fail(who + "w x h = " + std::to_string(w) + " x " + std::to_string(h)); return -1; }
  const bool swap = (kTf[orient] & kMineSwap) != 0;
  *tw = swap ? h : w; *th = swap ? w : h;
  return 0;
}

int turn_host(const jdaPixels* images, const int* orients, int n, unsigned char* dst, const size_t* dst_offsets) {
  std::vector<PackOne> v;
  if (!check_pack("jdaPackGrayOriented: ", images, orients, true, n, dst, dst_offsets, &v)) return -1;
  turn_write(v);
  return 0;
}

void turn_write(const std::vector<PackOne>& v) {
  for (const PackOne& o : v) {
    const bool swap = (o.tf & kMineSwap) != 0;
    const int TW = swap ? o.h : o.w, TH = swap ? o.w : o.h;
    int w[3] = {0, 0, 0};
    if (o.bpp > 1) pack_weights(o.format, w);
    uint8_t* d = o.dst;
    for (int tv = 0; tv < TH; tv++) {
      for (int tu = 0; tu < TW; tu++) {
        int x = swap ? tv : tu, y = swap ? tu : tv;
        if (o.tf & kMineFlipX) x = o.w - 1 - x;
        if (o.tf & kMineFlipY) y = o.h - 1 - y;
        const uint8_t* s = o.src + (long long)y * o.pitch + (long long)x * o.bpp;
        *d++ = o.bpp == 1 ? s[0] : (uint8_t)((s[0] * w[0] + s[1] * w[1] + s[2] * w[2] + 8192) >> 14);
      }
    }
  }
}

int turn_device(Cascador* c, const jdaPixels* images, const int* orients, int n, unsigned char* d_dst, const size_t* dst_offsets,
                hipStream_t user_stream, jdaPackStats* stats) {
  LaneCall call(c);
  const std::string who = "jdaPackGrayOrientedDevice: ";
  if (!c) { fail(who + "null cascador"); return -1; }
  std::vector<PackOne> v;
  if (!check_pack(who, images, orients, true, n, d_dst, dst_offsets, &v)) return -1;
  if (stats) std::memset(stats, 0, sizeof *stats);
  return n == 0 ? 0 : turn_launch(call, who, v, user_stream, stats);
}

int turn_launch(LaneCall& call, const std::string& who, const std::vector<PackOne>& v, hipStream_t user_stream, jdaPackStats* stats) {
  const int n = (int)v.size();
  if (std::all_of(v.begin(), v.end(), [](const PackOne& o) { return o.tf == 0; })) return pack_launch(call, who, v, user_stream, stats);   // the same bytes

  std::vector<TurnImg> tab;
  std::vector<int> block_img;
  long long total;
  if (!turn_tiles(who, v, &tab, &block_img, &total)) return -1;

  if (!call.open(user_stream)) return -1;
  const hipStream_t st = call.st;
  auto body = [&]() -> bool {
    TurnImg* d_tab; int* d_blk;
    if (!call.upload(tab, block_img, &d_tab, &d_blk) || !call.begin()) return false;
    TurnArgs a{d_tab, d_blk, n, total};
    JDA_HIP(launch_turn(a, st));
    return call.end() && call.sync();
  };
  if (!call.run(stats != nullptr, body)) return -1;
  pack_stats(stats, v, call);
  return 0;
}

int orient_back(const OrientBackCall& k) { return orient_back("jdaOrientBack: ", k, nullptr); }

// degrees (rotate.cpp): an angle per image in place of the orientations -- the same refusals, the plan's in place of the
// orientation's, and every face through rotate_back_face
int orient_back(const std::string& who, const OrientBackCall& k, const int* factors, const double* degrees) {
  if (k.n_faces < 0) { fail(who + "negative number of faces (n_faces = " + std::to_string(k.n_faces) + ")"); return -1; }
  if (k.n_images < 0) { fail(who + "negative number of images (n_images = " + std::to_string(k.n_images) + ")"); return -1; }
  if (k.n_faces == 0) return 0;
  if (!k.images) { fail(who + "null images"); return -1; }
  if (!k.orients && !degrees) { fail(who + "null orients"); return -1; }
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
  std::vector<PixelsOne> img((size_t)k.n_images);
  std::vector<jdaRotation> rot(degrees ? (size_t)k.n_images : 0);
  for (int i = 0; i < k.n_images; i++) {
    if (!check_pixels(who + "image " + std::to_string(i) + ": ", k.images[i], &img[(size_t)i])) return -1;
    if (degrees) {
      if (!rotation_plan(who + "image " + std::to_string(i) + ": ", img[(size_t)i].w, img[(size_t)i].h, degrees[i], &rot[(size_t)i])) return -1;
      continue;
    }
    if (k.orients[i] < 0 || k.orients[i] > 7) { fail(who + "image " + std::to_string(i) + ": unknown orientation " + std::to_string(k.orients[i]) + " (0..7)"); return -1; }
    if (!factors) continue;
    const int f = factors[i];
    if (f < 1 || f > kReduceMax) { fail(who + "image " + std::to_string(i) + ": factor " + std::to_string(f) + " (1.." + std::to_string(kReduceMax) + ")"); return -1; }
    if (img[(size_t)i].w < f || img[(size_t)i].h < f) {
      fail(who + "image " + std::to_string(i) + ": a rectangle of " + std::to_string(img[(size_t)i].w) + " x " + std::to_string(img[(size_t)i].h) + " reduced by factor " + std::to_string(f) + " has no pixel");
      return -1;
    }
  }
  for (int f = 0; f < k.n_faces; f++) {
    if (k.face_image[f] < 0 || k.face_image[f] >= k.n_images) {
      fail(who + "face " + std::to_string(f) + ": face_image " + std::to_string(k.face_image[f]) + " is outside [0, " + std::to_string(k.n_images) + ")");
      return -1;
    }
  }
  for (int f = 0; f < k.n_faces; f++) {
    if (degrees) { rotate_back_face(k, f, img[(size_t)k.face_image[f]], rot[(size_t)k.face_image[f]]); continue; }
    const int i = k.face_image[f], t = k.orients[i], tf = kTf[t];
    const PixelsOne& r = img[(size_t)i];
    const int fc = factors ? factors[i] : 0, w = fc ? r.w / fc : r.w, h = fc ? r.h / fc : r.h;   // the rectangle as it was turned
    if (k.boxes) {
      int* b = k.boxes + (size_t)f * k.box_ints;
      const int bw0 = b[2], bh0 = k.box_ints == 4 ? b[3] : b[2];
      const bool swap = (tf & kMineSwap) != 0;
      int x0 = swap ? b[1] : b[0], y0 = swap ? b[0] : b[1];
      int bw = swap ? bh0 : bw0, bh = swap ? bw0 : bh0;
      if (tf & kMineFlipX) x0 = w - bw - x0;
      if (tf & kMineFlipY) y0 = h - bh - y0;
      if (fc) { x0 *= fc; y0 *= fc; bw *= fc; bh *= fc; }
      b[0] = x0 + r.x; b[1] = y0 + r.y; b[2] = bw;
      if (k.box_ints == 4) b[3] = bh;
    }
    if (k.landmarks) {
      const bool mirror = t >= 4;                   // 4, 5, 6, 7: the swap / flip matrix has determinant -1
      if (k.real_bytes == 4) back_landmarks((float*)k.landmarks + (size_t)f * 2 * k.landmark_n, k.landmark_n, tf, mirror, r, w, h, fc, k.left, k.right, k.sym_n);
      else back_landmarks((double*)k.landmarks + (size_t)f * 2 * k.landmark_n, k.landmark_n, tf, mirror, r, w, h, fc, k.left, k.right, k.sym_n);
    }
  }
  return 0;
}

}  // namespace jda
