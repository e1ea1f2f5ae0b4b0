// libjda.so, host side: frames larger than the faces need (include/jda.h) -- jdaReduceSize; jdaPackGrayReduced, plain loops over
// the definition in host memory; jdaPackGrayReducedDevice on the kernel of k_reduce.hip; jdaReduceBack, which takes what a
// detect call returned on reduced, turned rectangles back into the source images.  The pack entries refuse what pack.cpp's
// refuse (check_pack, shared, with the factors) and with every factor 1 they ARE turn.cpp's; the way back is turn.cpp's
// orient_back with a factor per image.  The device form builds the image table and the item list (a tile per workgroup: the
// tiles of turn.cpp, of the reduced image), puts them into its lane's grow-only buffer and makes one launch.
#include "detect.h"

namespace jda {

namespace {

// orients == NULL: every image upright
bool check_reduced(const std::string& who, const jdaPixels* images, const int* factors, const int* orients, int n, unsigned char* dst,
                   const size_t* dst_offsets, std::vector<PackOne>* v) {
  return check_pack(who, images, orients, orients != nullptr, n, dst, dst_offsets, v, factors, true);
}

bool all_ones(const std::vector<PackOne>& v) {
  return std::all_of(v.begin(), v.end(), [](const PackOne& o) { return o.f == 1; });
}

}  // namespace

int reduce_size(int w, int h, int factor, int orient, int* rw, int* rh) {
  const std::string who = "jdaReduceSize: ";
  if (!rw || !rh) { fail(who + "null rw or rh"); return -1; }
  if (factor < 1 || factor > kReduceMax) { fail(who + "factor " + std::to_string(factor) + " (1.." + std::to_string(kReduceMax) + ")"); return -1; }
  if (orient < 0 || orient > 7) { fail(who + "unknown orientation " + std::to_string(orient) + " (0..7)"); return -1; }
  if (w < 0 || h < 0) { fail(who + "w x h = " + std::to_string(w) + " x " + std::to_string(h)); return -1; }
  const bool swap = (kTf[orient] & kMineSwap) != 0;
  *rw = swap ? h / factor : w / factor; *rh = swap ? w / factor : h / factor;
  return 0;
}

int reduce_host(const jdaPixels* images, const int* factors, const int* orients, int n, unsigned char* dst, const size_t* dst_offsets) {
  std::vector<PackOne> v;
  if (!check_reduced("jdaPackGrayReduced: ", images, factors, orients, n, dst, dst_offsets, &v)) return -1;
  if (all_ones(v)) { turn_write(v); return 0; }                     // jdaPackGrayOriented's bytes
  std::vector<uint8_t> gray;                                        // the f source rows of one reduced row, as gray
  for (const PackOne& o : v) {
    const int f = o.f, rw = o.w / f, rh = o.h / f;
    const bool swap = (o.tf & kMineSwap) != 0;
    const int TW = swap ? rh : rw;
    int w[3] = {0, 0, 0};
    if (o.bpp > 1) pack_weights(o.format, w);
    gray.resize((size_t)f * rw * f);
    for (int j = 0; j < rh; j++) {
      for (int r = 0; r < f; r++) {                                 // 1. gray, rounded per pixel
        const uint8_t* s = o.src + ((long long)j * f + r) * o.pitch;
        uint8_t* g = gray.data() + (size_t)r * rw * f;
        for (int x = 0; x < rw * f; x++, s += o.bpp) g[x] = o.bpp == 1 ? s[0] : (uint8_t)((s[0] * w[0] + s[1] * w[1] + s[2] * w[2] + 8192) >> 14);
      }
      for (int i = 0; i < rw; i++) {
        int S = 0;                                                  // 2. the block's mean, to nearest, halves up
        for (int r = 0; r < f; r++) for (int c = 0; c < f; c++) S += gray[(size_t)r * rw * f + (size_t)i * f + c];
        int x = i, y = j;                                           // 3. reduced pixel (x, y) is turned pixel (u, v): the definition, inverted
        if (o.tf & kMineFlipY) y = rh - 1 - y;
        if (o.tf & kMineFlipX) x = rw - 1 - x;
        const int u = swap ? y : x, tv = swap ? x : y;
        o.dst[(long long)tv * TW + u] = (uint8_t)((S + f * f / 2) / (f * f));
      }
    }
  }
  return 0;
}

int reduce_device(Cascador* c, const jdaPixels* images, const int* factors, const int* orients, int n, unsigned char* d_dst,
                  const size_t* dst_offsets, hipStream_t user_stream, jdaPackStats* stats) {
  LaneCall call(c);
  const std::string who = "jdaPackGrayReducedDevice: ";
  if (!c) { fail(who + "null cascador"); return -1; }
  std::vector<PackOne> v;
  if (!check_reduced(who, images, factors, orients, n, d_dst, dst_offsets, &v)) return -1;
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (n == 0) return 0;
  if (all_ones(v)) return turn_launch(call, who, v, user_stream, stats);   // the same bytes

  std::vector<ReduceImg> tab;
  std::vector<int> block_img;
  long long total;
  if (!turn_tiles(who, v, &tab, &block_img, &total)) return -1;
  if (!call.open(user_stream)) return -1;
  const hipStream_t st = call.st;
  auto body = [&]() -> bool {
    ReduceImg* d_tab; int* d_blk;
    if (!call.upload(tab, block_img, &d_tab, &d_blk) || !call.begin()) return false;
    ReduceArgs a{d_tab, d_blk, n, total};
    JDA_HIP(launch_reduce(a, st));
    return call.end() && call.sync();
  };
  if (!call.run(stats != nullptr, body)) return -1;
  if (stats) {
    long long pixels = 0, bytes_in = 0;
    for (const PackOne& o : v) { pixels += o.npix; bytes_in += o.npix * o.f * o.f * o.bpp; }   // the pixels that take part
    stats->pixels = pixels; stats->bytes_in = bytes_in; stats->bytes_out = pixels; stats->launches = 1;
    stats->device_ms = call.device_ms; stats->call_ms = call.call_ms();
  }
  return 0;
}

int reduce_back(const OrientBackCall& k, const int* factors) {
  const std::string who = "jdaReduceBack: ";
  if (k.n_faces > 0 && !factors) { fail(who + "null factors"); return -1; }
  return orient_back(who, k, k.n_faces > 0 ? factors : nullptr);
}

}  // namespace jda
