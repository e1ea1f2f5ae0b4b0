// libjda.so, host side: frames larger than the faces need (include/jda.h) -- jdaReduceSize and the definition of
// jdaPackGrayReduced, plain loops over host memory (the device form is k_reduce.hip).  The call path -- what is refused, the
// device entry, the way back (turn.cpp's, with the factor) -- is frames.cpp's.
#include "frames.h"

namespace jda {

int reduce_size(int w, int h, int factor, int orient, int* rw, int* rh) {
  const std::string who = "jdaReduceSize: ";
  if (!rw || !rh) { fail(who + "null rw or rh"); return -1; }
  if (!check_factor(who, factor) || !check_orient(who, orient)) return -1;
  if (w < 0 || h < 0) { fail(who + "w x h = " + std::to_string(w) + " x " + std::to_string(h)); return -1; }
  const FrameSize z = frame_size(w, h, factor, kTf[orient]);
  *rw = z.tw; *rh = z.th;
  return 0;
}

void reduce_write(const std::vector<FrameOne>& v) {
  std::vector<uint8_t> gray;                                        // the f source rows of one reduced row, as gray
  for (const FrameOne& o : v) {
    const int f = o.f, rw = o.rw, rh = o.rh;
    const bool swap = (o.tf & kMineSwap) != 0;
    int w[3] = {0, 0, 0};
    if (o.bpp > 1) pack_weights(o.format, w);
    gray.resize((size_t)f * rw * f);
    for (int j = 0; j < rh; j++) {
      for (int r = 0; r < f; r++) {                                 // 1. gray, rounded per pixel
        const uint8_t* s = o.src + ((long long)j * f + r) * o.pitch;
        uint8_t* g = gray.data() + (size_t)r * rw * f;
        for (int x = 0; x < rw * f; x++, s += o.bpp) g[x] = gray_of(s, o.bpp, w);
      }
      for (int i = 0; i < rw; i++) {
        int S = 0;                                                  // 2. the block's mean, to nearest, halves up
        for (int r = 0; r < f; r++) for (int c = 0; c < f; c++) S += gray[(size_t)r * rw * f + (size_t)i * f + c];
        int x = i, y = j;                                           // 3. reduced pixel (x, y) is turned pixel (u, v): the definition, inverted
        if (o.tf & kMineFlipY) y = rh - 1 - y;
        if (o.tf & kMineFlipX) x = rw - 1 - x;
        const int u = swap ? y : x, tv = swap ? x : y;
        o.dst[(long long)tv * o.tw + u] = (uint8_t)((S + f * f / 2) / (f * f));
      }
    }
  }
}

}  // namespace jda
