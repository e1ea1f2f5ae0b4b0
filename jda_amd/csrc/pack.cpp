// libjda.so, host side: frames as they arrive (include/jda.h) -- the definition of jdaPackGray, a plain loop over host memory
// (the device form is k_pack.hip).  The call path -- what is refused, the device entry -- is frames.cpp's.
#include "frames.h"

namespace jda {

void pack_write(const std::vector<FrameOne>& v) {
  for (const FrameOne& o : v) {
    uint8_t* d = o.dst;
    if (o.bpp == 1) {
      for (int y = 0; y < o.h; y++, d += o.w) std::memcpy(d, o.src + (long long)y * o.pitch, (size_t)o.w);
      continue;
    }
    int w[3];
    pack_weights(o.format, w);
    for (int y = 0; y < o.h; y++) {
      const uint8_t* s = o.src + (long long)y * o.pitch;
      for (int x = 0; x < o.w; x++, s += o.bpp) *d++ = gray_of(s, o.bpp, w);
    }
  }
}

}  // namespace jda
