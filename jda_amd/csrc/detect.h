// libjda.so, host side: what the entry points (abi.cpp) and the translation units behind them share.
#pragma once
#include "results.h"
#include "run.h"

namespace jda {

// post_host.cpp
void parallel_for(int n, const std::function<void(int)>& fn, bool small_job = false);
void fill_stats(jdaStats* st, const RunStats& rs, long long patch_n, int T, int K, double host_ms);
RunStats run_stats_of(const jdaStats& st);
RunStats& operator+=(RunStats& a, const RunStats& b);
// NMS, relocation and the results of every frame of a batch from its raw detections (sorted by gid = frame, then scan
// order; frames post-processed on the device, RawDets::p_n[f] >= 0, come as they are).  Returns the time it took (ms).
template <class D>
double post_frames(const std::vector<Level>& levels, const FrameSet& fs, const RawDets<typename D::Real>& dets, int L, bool nms,
                   double overlap, const Sink<D>& sink);

// detect.cpp
bool plan_c_call(Cascador* c, size_t stride, int width, int height, float scale, int min_size, int max_size,
                 ScanPlan* sp, PlanEntry** pe);
bool cpp_model_complete(const Cascador* c);
bool stage_frames(Lane* ln, const unsigned char* const* frames, int n, size_t fbytes, size_t* stride, bool defer = false);
int detect_c_device(Cascador* c, const uint8_t* d_frames, size_t stride, int n, int width, int height,
                    float scale, int min_size, int max_size, float th, const jdaDetectOptions* opt,
                    jdaResult* out, const unsigned char* const* host_frames = nullptr);

// the o / h / q patch sides of the trainer-side entries (k_mine_patches stages the o patch in LDS)
inline bool check_patch_sizes(int os, int hs, int qs) {
  if (os < 1 || hs < 1 || qs < 1 || os > 128 || hs > 128 || qs > 128) { fail("origin/half/quarter_size must be in [1, 128]"); return false; }
  return true;
}

// The trainer-side entries (train.cpp, stage.cpp, reval.cpp) run under the per-sample similarity transform: the transform is on
// AND the caller opted into this library's reading of data.cpp:168 (option "train_similarity", include/jda.h).  On without the
// option: they refuse.
inline bool train_similarity(const Cascador* c) { return c->similarity && c->kn.train_similarity; }

// train.cpp: a caller's sample set / pool features as the trainer-side entries accept them (fail() says what is wrong)
bool check_set(const jdaSamplesCpp* s, const char* name, bool need_weights);
bool check_pool(const jdaFeatureCpp* pool, size_t count, int L);

// fit.cpp: a stage's global regression (jdaGlobalRegressionCpp) and its host-only shuffle (jdaFitShuffleCpp)
int fit_entry(void* cascador, const int* lbf, const double* residual, int n, int K, const int* rows, int n_rows,
              const jdaFitParamsCpp* params, double* w, int* out_iters, double* out_gnorm1, jdaFitStatsCpp* stats);
int fit_shuffle(int* index, int n, uint64_t seed, int iter);

// model_grow.cpp: the model in training (jdaCascadorCreateTrainingCpp, jdaModel*Cpp, jdaCascadorSerializeToCpp)
Cascador* grow_create(int T, int K, int L, int D, const double* mean_shape);
int grow_status(Cascador* c, int* stage, int* cart);
int grow_put_cart(Cascador* c, int k, const jdaFeatureCpp* features, const int* thresholds, const double* leaf_scores, double th,
                  double mean, double stddev);
int grow_close_stage(Cascador* c, const double* w);
int grow_serialize(Cascador* c, const char* path);

// mine.cpp: Validate's own tables on the device
bool mine_model(Cascador* c, MineModel* out);
// reval.cpp: Validate on a resident sample set (jdaValidateSamplesCpp)
int reval_entry(Cascador* c, const jdaSamplesCpp* samples, int os, int hs, int qs, unsigned char* is_face, double* score, int* carts_n,
                double* shape, jdaStageStatsCpp* stats);

// windows.cpp: the cascade on caller-given windows (jdaValidateWindows / jdaValidateWindowsDevice); frames on the device
// (d_frames) or, with host_frames set, in host memory
struct WindowsOut { unsigned char* is_face; float* score; int* carts_n; unsigned int* path_hash; float* shapes; float* landmarks; jdaStats* stats; };
int windows_entry(Cascador* c, const char* fn, const unsigned char* const* host_frames, const uint8_t* d_frames, size_t stride, int n,
                  int width, int height, const int* windows, int n_windows, float th, const WindowsOut& out);

// pack.cpp: frames as they arrive (jdaPackGray / jdaPackGrayDevice)
int pack_host(const jdaPixels* images, int n, unsigned char* dst, const size_t* dst_offsets);
int pack_device(Cascador* c, const jdaPixels* images, int n, unsigned char* d_dst, const size_t* dst_offsets, hipStream_t user_stream,
                jdaPackStats* stats);// ... and what it shares with chips.cpp: everything the entries refuse about ONE jdaPixels (fail() says what, behind the
// prefix `img`), the rectangle resolved; bytes per pixel of a JDA_PIX_* (0: unknown); the Q14 weights of a colour pixel's
// bytes 0, 1, 2 (include/jda.h)
struct PixelsOne { const uint8_t* src; long long pitch; int x, y, w, h, bpp, format; };   // src: the rectangle's first pixel
bool check_pixels(const std::string& img, const jdaPixels& p, PixelsOne* out);
int pixels_bpp(int format);
void pack_weights(int format, int w[3]);

// ... and with turn.cpp: an image of a call, rectangle resolved, and everything the pack entries refuse about a call
struct PackOne {
  const uint8_t* src;                 // the rectangle's first pixel
  uint8_t* dst;
  long long pitch, npix;
  int w, h, bpp, format;
  int tf;                             // kTf[orientation] (0 without orients)
  int f;                              // the factor (1 unless reduced: then npix = (w / f) * (h / f), the bytes of dst)
  double c, s;                        // the rotation's plan (0 unless rotated: then npix = tw * th, the bytes of dst)
  int tw, th;
};
bool check_pack(const std::string& who, const jdaPixels* images, const int* orients, bool turned, int n, unsigned char* dst,
                const size_t* dst_offsets, std::vector<PackOne>* out, const int* factors = nullptr, bool reduced = false,
                const double* degrees = nullptr, bool rotated = false);
// The units of `bytes` bytes at dst (kernels.h: PackImg, ChipArgs): bytes in front of dst's first 16-byte boundary, runs of 16, bytes behind
struct DstUnits { int head; long long nq; int tail; long long total() const { return nq + head + tail; } };
inline DstUnits dst_units(const void* dst, long long bytes) {
  DstUnits u;
  u.head = (int)std::min<long long>(bytes, (long long)((0 - (uintptr_t)dst) & 15));
  u.nq = (bytes - u.head) >> 4;
  u.tail = (int)(bytes - u.head - (u.nq << 4));
  return u;
}
// What PackImg, TurnImg, ReduceImg and RotImg have in common, the rest zero: the image, its first unit / tile in the launch and the Q14 weights,
// split into their low and high bytes
template <typename Img>
void pack_img(Img* t, const PackOne& o, long long first) {
  std::memset(t, 0, sizeof *t);
  t->src = o.src; t->dst = o.dst; t->pitch = o.pitch; t->w = o.w; t->h = o.h; t->bpp = o.bpp; t->first = first;
  if (o.bpp == 1) return;
  int w[3];
  pack_weights(o.format, w);
  t->w_lo = (uint32_t)(w[0] & 255) | ((uint32_t)(w[1] & 255) << 8) | ((uint32_t)(w[2] & 255) << 16);
  t->w_hi = (uint32_t)(w[0] >> 8) | ((uint32_t)(w[1] >> 8) << 8) | ((uint32_t)(w[2] >> 8) << 16);
}
// The image table of a launch that deals 64 x 64 tiles of the turned images (Img: TurnImg, or ReduceImg, whose w x h is the
// rectangle reduced by its factor, or RotImg, whose turned image is the plan's tw x th; kernels.h) and the image of every
// workgroup's tile
template <typename Img>
bool turn_tiles(const std::string& who, const std::vector<PackOne>& v, std::vector<Img>* tab, std::vector<int>* block_img, long long* total_out) {
  const int n = (int)v.size();
  tab->resize((size_t)n);
  long long total = 0, pixels = 0;
  for (int i = 0; i < n; i++) {
    const PackOne& o = v[(size_t)i];
    Img& t = (*tab)[(size_t)i];
    pack_img(&t, o, total);
    int TW, TH;
    if constexpr (std::is_same<Img, RotImg>::value) {
      t.c = o.c; t.s = o.s; t.tw = TW = o.tw; t.th = TH = o.th;
    } else {
      t.tf = o.tf;
      if constexpr (std::is_same<Img, ReduceImg>::value) { t.f = o.f; t.w = o.w / o.f; t.h = o.h / o.f; }
      TW = (o.tf & kMineSwap) ? t.h : t.w; TH = (o.tf & kMineSwap) ? t.w : t.h;
    }
    t.off = (int)((uintptr_t)o.dst & 15);
    t.ntu = (int)(((long long)TW + t.off + kTurnTile - 1) / kTurnTile);
    t.ntv = (TH + kTurnTile - 1) / kTurnTile;
    total += (long long)t.ntu * t.ntv;
    pixels += o.npix;
  }
  if (total > 0x7fffffffll) { fail(who + "too many pixels for one launch (" + std::to_string(pixels) + ")"); return false; }
  block_img->resize((size_t)total);
  for (int i = 0; i < n; i++) std::fill_n(block_img->begin() + (*tab)[(size_t)i].first, (long long)(*tab)[(size_t)i].ntu * (*tab)[(size_t)i].ntv, i);
  *total_out = total;
  return true;
}
// jdaPackStats of a call that made its one launch
void pack_stats(jdaPackStats* stats, const std::vector<PackOne>& v, const LaneCall& call);
// pack_device's launch, on images check_pack has passed (at least one) and in the name `who` of the entry the caller called
// (turn.cpp: every orientation 0)
int pack_launch(LaneCall& call, const std::string& who, const std::vector<PackOne>& v, hipStream_t user_stream, jdaPackStats* stats);

// turn.cpp: frames in any orientation (jdaOrientSize, jdaPackGrayOriented[Device], jdaOrientBack)
int orient_size(int w, int h, int orient, int* tw, int* th);
int turn_host(const jdaPixels* images, const int* orients, int n, unsigned char* dst, const size_t* dst_offsets);
int turn_device(Cascador* c, const jdaPixels* images, const int* orients, int n, unsigned char* d_dst, const size_t* dst_offsets,
                hipStream_t user_stream, jdaPackStats* stats);
struct OrientBackCall {
  const jdaPixels* images; const int* orients; int n_images; const int* face_image; int n_faces; int* boxes; int box_ints;
  void* landmarks; int real_bytes, landmark_n; const int* left; const int* right; int sym_n;
};
int orient_back(const OrientBackCall& call);
// ... and what it shares with reduce.cpp: the writing half of turn_host and the launching half of turn_device (which is
// pack_launch where every image is upright), on images check_pack has passed, in the name `who` of the entry the caller
// called; orient_back with a factor per image (nullptr: jdaOrientBack itself) or, for rotate.cpp, an angle per image in place
// of the orientations
void turn_write(const std::vector<PackOne>& v);
int turn_launch(LaneCall& call, const std::string& who, const std::vector<PackOne>& v, hipStream_t user_stream, jdaPackStats* stats);
int orient_back(const std::string& who, const OrientBackCall& call, const int* factors, const double* degrees = nullptr);

// reduce.cpp: frames larger than the faces need (jdaReduceSize, jdaPackGrayReduced[Device], jdaReduceBack)
int reduce_size(int w, int h, int factor, int orient, int* rw, int* rh);
int reduce_host(const jdaPixels* images, const int* factors, const int* orients, int n, unsigned char* dst, const size_t* dst_offsets);
int reduce_device(Cascador* c, const jdaPixels* images, const int* factors, const int* orients, int n, unsigned char* d_dst,
                  const size_t* dst_offsets, hipStream_t user_stream, jdaPackStats* stats);
int reduce_back(const OrientBackCall& call, const int* factors);

// rotate.cpp: frames whose faces are rolled (jdaRotationPlan, jdaPackGrayRotated[Device], jdaRotateBack)
int rotation_plan(int w, int h, double degrees, jdaRotation* rot);
int rotate_host(const jdaPixels* images, const double* degrees, int n, unsigned char* dst, const size_t* dst_offsets);
int rotate_device(Cascador* c, const jdaPixels* images, const double* degrees, int n, unsigned char* d_dst, const size_t* dst_offsets,
                  hipStream_t user_stream, jdaPackStats* stats);
int rotate_back(const OrientBackCall& call, const double* degrees);
// ... and what it shares with pack.cpp and turn.cpp: the plan in the name `who` of the entry the caller called (false after
// fail()), and one face of the way back -- its box and landmarks through the plan's map into the whole source image
bool rotation_plan(const std::string& who, int w, int h, double degrees, jdaRotation* rot);
void rotate_back_face(const OrientBackCall& call, int face, const PixelsOne& rect, const jdaRotation& rot);

// chips.cpp: faces as they leave (jdaFaceChips / jdaFaceChipsDevice)
struct ChipsCall {
  const jdaPixels* images; int n_images; const int* face_image; const void* landmarks; int real_bytes, n_faces, landmark_n;
  const double* tmpl; const unsigned char* use; int chip_w, chip_h, chip_format, supersample; unsigned char* dst; double* matrices;
};
int chips_host(const ChipsCall& call);
int chips_device(Cascador* c, const ChipsCall& call, hipStream_t user_stream, jdaChipStats* stats);

// detect_cpp.cpp: dialect CPP, method 1 (cascador.cpp:310-376,431-477) on a uniform batch; frames on the device
// (d_frames) or, with host_frames set, in host memory
struct CppCall { int minimum_size, step; double factor, overlap; int nms; };
int detect_cpp_device(Cascador* c, const uint8_t* d_frames, size_t stride, int n, int width, int height, const CppCall& call,
                      jdaStats* stats, jdaResultD* out, const unsigned char* const* host_frames = nullptr);

// tickets.cpp
int submit_c_device(Cascador* c, const uint8_t* d_frames, size_t stride, int n, int width, int height,
                    float scale, int min_size, int max_size, float th, const jdaDetectOptions* opt,
                    const unsigned char* const* host_frames = nullptr);
int wait_c_device(Cascador* c, int slot, jdaStats* stats, jdaResult* out);

// ragged.cpp: a list of differently sized images as one job, either dialect, to n results or to rows
int detect_ragged(Cascador* c, const unsigned char* const* host_imgs, const uint8_t* d_base, const size_t* d_offsets,
                  const int* widths, const int* heights, int n, float scale, int min_size, int max_size, float th,
                  const jdaDetectOptions* opt, const Sink<DialectC>& sink);
int detect_ragged_cpp(Cascador* c, const unsigned char* const* host_imgs, const uint8_t* d_base, const size_t* d_offsets,
                      const int* widths, const int* heights, int n, const CppCall& call, jdaStats* stats, const Sink<DialectCpp>& sink);

}  // namespace jda
