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
