// libjda.so, host side: frames in any orientation (include/jda.h) -- jdaOrientSize; the definition of jdaPackGrayOriented,
// plain loops over host memory (the device form is k_turn.hip); and one face of jdaOrientBack / jdaReduceBack, which take what
// a detect call returned on turned (and reduced) rectangles back into the source images.  The call path -- what is refused,
// the device entry, the way back's checks -- is frames.cpp's.
#include "frames.h"

namespace jda {

namespace {

// landmarks in place, the type's own precision, one operation per line.  The rectangle was turned as o.rw x o.rh (reduced by
// f, if f: then a reduced pixel's centre goes to the centre of its f x f block, c = (f - 1) / 2)
template <class Real>
void back_landmarks(Real* lm, int L, const FrameOne& o, int f, const int* left, const int* right, int sym_n) {
  const Real c = (Real)(f - 1) / 2;
  for (int i = 0; i < L; i++) {
    Real x = lm[2 * i], y = lm[2 * i + 1];
    if (o.tf & kMineSwap) std::swap(x, y);
    if (o.tf & kMineFlipX) x = (Real)(o.rw - 1) - x;
    if (o.tf & kMineFlipY) y = (Real)(o.rh - 1) - y;
    if (f) {
      x = x * (Real)f;
      y = y * (Real)f;
      x = x + c;
      y = y + c;
    }
    x = x + (Real)o.x;
    y = y + (Real)o.y;
    lm[2 * i] = x; lm[2 * i + 1] = y;
  }
  if (o.orient < 4) return;                         // 4, 5, 6, 7 mirror: the swap / flip matrix has determinant -1
  for (int j = 0; j < sym_n; j++) {                 // sequentially, in list order: a landmark named in two pairs is swapped twice
    std::swap(lm[2 * left[j]], lm[2 * right[j]]);
    std::swap(lm[2 * left[j] + 1], lm[2 * right[j] + 1]);
  }
}

}  // namespace

int orient_size(int w, int h, int orient, int* tw, int* th) {
  const std::string who = "jdaOrientSize: ";
  if (!tw || !th) { fail(who + "null tw or th"); return -1; }
  if (!check_orient(who, orient)) return -1;
  if (w < 0 || h < 0) { fail(who + "w x h = " + std::to_string(w) + " x " + std::to_string(h)); return -1; }
  const FrameSize z = frame_size(w, h, 1, kTf[orient]);
  *tw = z.tw; *th = z.th;
  return 0;
}

void turn_write(const std::vector<FrameOne>& v) {
  for (const FrameOne& o : v) {
    const bool swap = (o.tf & kMineSwap) != 0;
    int w[3] = {0, 0, 0};
    if (o.bpp > 1) pack_weights(o.format, w);
    uint8_t* d = o.dst;
    for (int tv = 0; tv < o.th; tv++) {
      for (int tu = 0; tu < o.tw; tu++) {
        int x = swap ? tv : tu, y = swap ? tu : tv;
        if (o.tf & kMineFlipX) x = o.w - 1 - x;
        if (o.tf & kMineFlipY) y = o.h - 1 - y;
        *d++ = gray_of(o.src + (long long)y * o.pitch + (long long)x * o.bpp, o.bpp, w);
      }
    }
  }
}

void turn_back_face(const BackCall& k, int face, const FrameOne& o) {
  const int fc = o.kind == kReduce ? o.f : 0;       // (jdaOrientBack scales nothing: not even by 1)
  if (k.boxes) {
    int* b = k.boxes + (size_t)face * k.box_ints;
    const int bw0 = b[2], bh0 = k.box_ints == 4 ? b[3] : b[2];
    const bool swap = (o.tf & kMineSwap) != 0;
    int x0 = swap ? b[1] : b[0], y0 = swap ? b[0] : b[1];
    int bw = swap ? bh0 : bw0, bh = swap ? bw0 : bh0;
    if (o.tf & kMineFlipX) x0 = o.rw - bw - x0;
    if (o.tf & kMineFlipY) y0 = o.rh - bh - y0;
    if (fc) { x0 *= fc; y0 *= fc; bw *= fc; bh *= fc; }
    b[0] = x0 + o.x; b[1] = y0 + o.y; b[2] = bw;
    if (k.box_ints == 4) b[3] = bh;
  }
  if (k.landmarks) {
    if (k.real_bytes == 4) back_landmarks((float*)k.landmarks + (size_t)face * 2 * k.landmark_n, k.landmark_n, o, fc, k.left, k.right, k.sym_n);
    else back_landmarks((double*)k.landmarks + (size_t)face * 2 * k.landmark_n, k.landmark_n, o, fc, k.left, k.right, k.sym_n);
  }
}

}  // namespace jda
