/*
 * jda.h -- C ABI of the MI355X-native JDA sliding-window detector (libjda.so).
 *
 * Section 1 is the drop-in boundary: the six entry points of the reference
 * header (reference c/jda.h:31-68) with identical names, argument order,
 * argument meaning and ownership rules, so a program written against the
 * reference C library links against this one unchanged.
 *
 * Section 2 is additive: batch / device-resident entry points, a second
 * numeric dialect (the fp64 `src/jda` path), per-window trace output used by
 * the parity tests, and an error channel.  Nothing in section 2 changes the
 * behaviour of section 1.
 *
 * Plain C types only: pointers, ints, floats.  No C++/HIP/torch types cross
 * this boundary (a HIP stream is passed as an opaque void*).
 */
#ifndef JDA_AMD_JDA_H_
#define JDA_AMD_JDA_H_

#include <stddef.h>
#include <stdint.h>

#if defined(_MSC_VER)
#  if defined(JDA_EXPORTS)
#    define JDA_API __declspec(dllexport)
#  else
#    define JDA_API __declspec(dllimport)
#  endif
#else
#  define JDA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* 1. Reference-compatible surface                                          */
/* ------------------------------------------------------------------------ */

/* Detection list, returned BY VALUE (reference c/jda.h:18-24).
 * bboxes is n triples (x, y, size); shapes is n rows of 2*landmark_n floats
 * in absolute pixel coordinates (x1, y1, x2, y2, ...); scores is n floats.
 * The three arrays are malloc()ed by the library and owned by the caller
 * until jdaResultRelease(). */
typedef struct {
  int n;
  int landmark_n;
  int *bboxes;
  float *shapes;
  float *scores;
} jdaResult;

/* replaces reference c/jda.c:486-561 (c/jda.h:31).  Loads a model whose real
 * fields are 8-byte doubles (the trainer's format, src/jda/cascador.cpp:79).
 * Returns NULL if the file cannot be opened.  Unlike the reference, the
 * cascade dimensions are taken from the file header at run time, and a file
 * whose size does not match its header is refused (NULL). */
JDA_API void *jdaCascadorCreateDouble(const char *model);

/* replaces reference c/jda.c:563-638 (c/jda.h:32).  Same for the 4-byte float
 * layout that jdaCascadorSerializeTo() writes. */
JDA_API void *jdaCascadorCreateFloat(const char *model);

/* replaces reference c/jda.c:644-716 (c/jda.h:41).  Writes the float layout,
 * including the reference's header convention (stage index T+1, cart -1).
 * Silently returns if the file cannot be created, like the reference. */
JDA_API void jdaCascadorSerializeTo(void *cascador, const char *model);

/* replaces reference c/jda.c:718-720 (c/jda.h:47). NULL is accepted.
 * Batches that were submitted (jdaDetectBatchSubmit*) and never waited for are drained.  Like the reference's, this
 * must not race with a call on the same cascador from another thread: the reference frees what jdaDetect reads; here
 * such a call is given up to ten seconds to return before the cascador goes (tests/test_reentrant.py). */
JDA_API void jdaCascadorRelease(void *cascador);

/* replaces reference c/jda.c:443-480 (c/jda.h:62-63).
 *   data      borrowed, width*height contiguous 8-bit gray, row stride = width
 *   scale     growth factor of the window size between pyramid levels
 *   step      accepted and ignored, exactly like the reference, which
 *             overrides it with 10 % of the window size (c/jda.c:333)
 *   min_size  raised to 24 if smaller (c/jda.c:459)
 *   max_size  <= 0 means min(width, height) (c/jda.c:460)
 *   th        final score cut (c/jda.c:414)
 * Output order: scan order (level, y, x) of the windows that survive NMS.
 * Re-entrant like the reference (no globals, no locks in c/jda.c:443-480): any number of threads may call it -- and
 * every other detect entry below -- on ONE cascador at the same time; each call takes a lane (stream + workspace)
 * from the cascador's pool, the model and the scan plans are shared read-only.
 * Runs the cascade on the GPU (HIP device selected with jdaSetDevice, default
 * the current device).  There is no CPU fallback: if no HIP device is usable
 * the call returns an empty result, sets jdaGetLastError() and prints the
 * reason on stderr. */
JDA_API jdaResult jdaDetect(void *cascador, unsigned char *data, int width, int height,
                            float scale, float step, int min_size, int max_size, float th);

/* replaces reference c/jda.c:722-727 (c/jda.h:68). */
JDA_API void jdaResultRelease(jdaResult result);

/* ------------------------------------------------------------------------ */
/* 2. Additive extensions                                                   */
/* ------------------------------------------------------------------------ */

/* Numeric dialects of the same cascade.
 * JDA_DIALECT_C   : fp32, truncating coordinates, growing window with 10 %
 *                   step -- reference c/jda.c (what jdaDetect runs).
 * JDA_DIALECT_CPP : fp64, round() coordinates, fixed pixel step, no final
 *                   threshold, score-ordered NMS -- reference
 *                   src/jda/cascador.cpp:166-211,310-477 (method 1). */
enum { JDA_DIALECT_C = 0, JDA_DIALECT_CPP = 1 };

/* Thread-local message of the last failed call on this thread ("" if none).
 * No C++ exception leaves the library: an allocation failure inside any entry (std::bad_alloc from the host side's
 * containers, the tables of a large model) is caught at the boundary and turned into the entry's error value -- NULL,
 * -1 or an empty jdaResult, the reference's own answer to a failed malloc (c/jda.c:487-493) -- with the reason here.
 * A successful call leaves it empty.  (When the persistent stage-0 scan kernel gives up waiting inside a launch -- a
 * watchdog; never observed on hardware -- or covers fewer windows than the plan holds, the pass is run again with the
 * closed-tile scan kernel: the call succeeds with correct results, says so on stderr and counts it in
 * jdaStats::scan_fallbacks; it is not an error and is not reported here.) */
JDA_API const char *jdaGetLastError(void);

/* Opens a model of either layout; the layout is inferred from the file size
 * implied by the header (the file has no discriminator). */
JDA_API void *jdaCascadorCreate(const char *model);

typedef struct {
  int T;            /* stages                                   */
  int K;            /* carts per stage                          */
  int landmark_n;   /* landmarks L; a shape has 2L coordinates  */
  int tree_depth;   /* D; a cart has 2^(D-1)-1 split nodes      */
  int multi_scale;  /* 1 if any split node reads the half/quarter image */
  int source_real_bytes; /* 8 or 4: layout of the file it came from */
} jdaModelInfo;

JDA_API int jdaCascadorInfo(void *cascador, jdaModelInfo *info);

/* Pin a cascador to a HIP device ordinal (default: device current at first
 * use).  Must be called before the first detect on this cascador. */
JDA_API int jdaSetDevice(void *cascador, int device);

/* Tuning options of a cascador.  They start from the JDA_* environment variables (read once, when the cascador
 * is created) and can be changed here while NO call is running and no submitted batch is pending
 * on this cascador (refused otherwise); a change drops the cached scan plans.  None of them changes results.  Documented keys:
 *   "handoff"       carts of stage 0 the scan kernel evaluates before the finishing kernel takes over (128)
 *   "lanes"         sub-batches of one synchronous call that run side by side on their own streams (2)
 *   "dense"         whole-stage tile kernel for models that reject little: 0 off, 1 auto, 2 always (1)
 *   "workspace_mb"  device workspace budget of a call in MiB; larger batches run in several passes (24576)
 *   "ws_bound"      size the survivor queues of a pass from the fractions earlier passes left in them ("ws_factor_pct" = 400 % of
 *                   them, at least "ws_min_entries" = 65536) instead of for every window; a pass that outgrows them is rerun (1)
 *   "plan_cache"    scan plans (one per frame size and call parameters) kept per cascador (64)
 *   "predict"       size the finishing launches from the previous pass instead of a host round trip (1)
 *   "scan_p"        the persistent form of the stage-0 scan for large uniform batches: 0 off, 1 where it suits, 2 wherever it fits (1)
 *   "device_post"   per-frame sort, NMS and relocation of batches of 16 frames or more on the device instead of on the host (1)
 *   "hwq_place"     the cascador's streams are placed on the device's hardware queues: the HIP runtime deals a process's streams
 *                   to four queues in creation order, so whether two lanes share one (and run one after the other) depends on
 *                   the streams the host program created before; the library probes which of its streams share a queue and
 *                   hands them out by queue.  0: wherever the runtime puts them (1).  Read-only, what the pool found:
 *                   "hwq_queues", "hwq_streams", "hwq_probes", "hwq_max_mains" (most lanes whose main streams share a queue)
 *   read-only, what the cascador holds on the device: "mem_device_bytes" (its model tables and its lanes' buffers, all
 *                   grow-only; NOT the total: the scan plans' buffers are not in it) and "mem_plan_buffers" (the NUMBER of
 *                   plan buffers in use and pooled, not their bytes); per-call workspaces live only during their call
 * (the other keys of DESIGN.md section 8 are accepted as well; they are experiment switches).
 * Returns 0, or -1 for an unknown key / a running call or pending batch.  jdaGetOption returns the value (-1: unknown key). */
JDA_API int jdaSetOption(void *cascador, const char *key, long long value);
JDA_API long long jdaGetOption(void *cascador, const char *key);

/* Which finishing form the passes of a cascador took.  After the stage-0 scan a pass finishes its
 * windows in one of these forms; the choice depends on the length of the hand-off queue (or its prediction from earlier
 * passes on the same scan plan), on the model, on the options and on how many callers share the cascador, and never
 * changes a result.  A test that names a finishing kernel reads here that the kernel ran. */
enum {
  JDA_FINISH_WIDE_CONC = 0,  /* k_finish_wide, score replay and regression side by side                          */
  JDA_FINISH_WIDE_SEQ,       /* k_finish_wide, one after the other, the weight rows through LDS                  */
  JDA_FINISH_MERGED,         /* one k_finish launch for every stage                                              */
  JDA_FINISH_FILTER0,        /* k_filter0, then k_finish on its survivors                                        */
  JDA_FINISH_MID_DIRECT,     /* the same pair, fed from the mid queue the persistent scan filled itself          */
  JDA_FINISH_TWO_LAUNCH,     /* k_finish for stage 0, then k_finish for the other stages                         */
  JDA_FINISH_DENSE,          /* dense mode: k_stage for every stage and level, no hand-off queue at all          */
  JDA_FINISH_FORM_N
};
/* counts[f]: how often the passes of this cascador have issued form f since it was created -- every entry that runs a
 * pass counts (batches, traces, tickets, ragged jobs, both dialects).  The counts only grow and are added atomically
 * where the launches are issued; a caller takes the difference around its own call, which is that call's alone as long
 * as one thread uses the cascador.  A form counts once per pass, however many launches it takes (DENSE: one per stage
 * and level).  A pass that is issued again -- a queue was too small, or the persistent scan came back short
 * (jdaStats ws_regrows / scan_fallbacks) -- counts again: the difference says what was launched, not what was kept.
 * Returns 0, or -1 for a null argument. */
JDA_API int jdaFinishForms(void *cascador, long long counts[JDA_FINISH_FORM_N]);

/* Which stage-0 scan the passes of a cascador launched.  A scan launch is one instantiation of
 * k_scan or k_scan_p; which one depends on the model, the scan plan's tiles, the options and the size of the job, and
 * never changes a result.  Every launch counts once under the full key of what it instantiates:
 *   kernel   JDA_SCAN_K_SCAN (closed tiles) or JDA_SCAN_K_SCAN_P (the persistent form)
 *   dialect  JDA_DIALECT_C (fp32) or JDA_DIALECT_CPP (fp64)
 *   depth    JDA_SCAN_DEPTH_4, JDA_SCAN_DEPTH_6 or JDA_SCAN_DEPTH_GENERIC (any other tree depth)
 *   pix      JDA_SCAN_T16_256 / JDA_SCAN_T16_512: LDS pixel tile, 16-bit node offsets, workgroups of 256 / 512 threads
 *            (k_scan_p: of fewer than 512 / of 512 or more threads, its size being the scan_p_block option);
 *            JDA_SCAN_T21: LDS tile, 21-bit offsets; JDA_SCAN_GLB: no tile, pixels through the caches
 *   ragged   1: a launch over the block map of a ragged job
 *   lean     1: the form without the per-cart normalisation test (no cart of the scanned range normalises)
 *   trace    1: the pass records carts, score and leaf hash per window
 *   merged   1: one launch over several levels (a ragged launch: over blocks of several levels), 0: a single level
 * at counts[JDA_SCAN_FORM(kernel, dialect, depth, pix, ragged, lean, trace, merged)]. */
enum { JDA_SCAN_K_SCAN = 0, JDA_SCAN_K_SCAN_P = 1 };
enum { JDA_SCAN_DEPTH_4 = 0, JDA_SCAN_DEPTH_6 = 1, JDA_SCAN_DEPTH_GENERIC = 2 };
enum { JDA_SCAN_T16_256 = 0, JDA_SCAN_T16_512 = 1, JDA_SCAN_T21 = 2, JDA_SCAN_GLB = 3 };
#define JDA_SCAN_FORM(kernel, dialect, depth, pix, ragged, lean, trace, merged) \
  ((((((((kernel) * 2 + (dialect)) * 3 + (depth)) * 4 + (pix)) * 2 + (ragged)) * 2 + (lean)) * 2 + (trace)) * 2 + (merged))
#define JDA_SCAN_FORM_N 768
/* counts[i]: how often the passes of this cascador have launched form i since it was created.  Cumulative, added
 * atomically on the host where the launches are issued; take the difference around a call, as with jdaFinishForms.  A
 * pass that is issued again (jdaStats ws_regrows / scan_fallbacks) counts its launches again.  Returns 0, or -1 for a null argument. */
JDA_API int jdaScanForms(void *cascador, long long counts[JDA_SCAN_FORM_N]);

/* Which k_finish and k_filter0 launches the passes of a cascador issued.  The forms MERGED,
 * FILTER0, MID_DIRECT and TWO_LAUNCH above are made of launches of these two kernels; every launch counts once under
 * the full key of what it instantiates and how it was set up:
 *   kernel     JDA_FINISH_K_FINISH or JDA_FINISH_K_FILTER0
 *   dialect    JDA_DIALECT_C (fp32) or JDA_DIALECT_CPP (fp64)
 *   trace      1: the pass records carts, score, leaf hash and shape per window
 *   groups     k_finish: the 64-cart groups a round walks, 1..4 (from K, or 1 for stage 0 of TWO_LAUNCH); k_filter0: 0
 *   multi      1: a multi-scale model, the nodes read the half and quarter images (no window tile)
 *   st         1: dialect CPP under the similarity transform
 *   stream     1: the weight rows are read with non-temporal loads (w_stream_mb; the form without trace, multi and st only)
 *   survivors  1: k_finish on the mid queue as k_filter0 (or the persistent scan) left it
 *   carry      1: the launch writes (k_filter0) or reads (k_finish on survivors) the stage-0 leaves carried in the mid queue
 *   tile       1: windows up to jdaFinishTileWin pixels walk from an LDS copy of their pixels
 * at counts[JDA_FINISH_LAUNCH(kernel, dialect, trace, groups, multi, st, stream, survivors, carry, tile)].  The fields that
 * do not apply to k_filter0 are 0 in its keys. */
enum { JDA_FINISH_K_FINISH = 0, JDA_FINISH_K_FILTER0 = 1 };
#define JDA_FINISH_LAUNCH(kernel, dialect, trace, groups, multi, st, stream, survivors, carry, tile) \
  ((((((((((kernel) * 2 + (dialect)) * 2 + (trace)) * 5 + (groups)) * 2 + (multi)) * 2 + (st)) * 2 + (stream)) * 2 + (survivors)) * 2 + (carry)) * 2 + (tile))
#define JDA_FINISH_LAUNCH_N 2560
/* counts[i]: how often the passes of this cascador have issued launch i since it was created: one count per launch
 * (TWO_LAUNCH adds two k_finish, FILTER0 and MID_DIRECT one k_filter0 and one k_finish).  Cumulative, added atomically on
 * the host where the launches are issued; take the difference around a call, as with jdaFinishForms.  A pass that is issued
 * again (jdaStats ws_regrows / scan_fallbacks) counts its launches again.  Returns 0, or -1 for a null argument. */
JDA_API int jdaFinishLaunches(void *cascador, long long counts[JDA_FINISH_LAUNCH_N]);
/* The largest window side, in pixels, that k_finish copies to LDS with this cascador's model in `dialect` (as the
 * similarity transform stands): windows up to it walk from the copy, larger ones read the frame.  0: no window does (the
 * model's state leaves no room, or it is multi-scale).  -1: a null cascador or an unknown dialect. */
JDA_API int jdaFinishTileWin(void *cascador, int dialect);

/* Which k_stage launches the passes of a cascador issued.  The form DENSE above is made of one
 * k_stage launch per stage and level; every launch counts once under the full key of what it instantiates and how it
 * was set up:
 *   dialect  JDA_DIALECT_C (fp32) or JDA_DIALECT_CPP (fp64)
 *   trace    1: the pass records carts, score, leaf hash and shape per window
 *   glb      1: the pixels of a 16 x 16 tile of the level's windows exceed the LDS pixel cap and are read through the
 *            caches, 0: they are copied to LDS first
 *   acc      the register width of the regression sums, the smallest class that holds the 2 * landmarks shape
 *            coordinates: JDA_STAGE_ACC_12, _32, _64, _160
 *   chunk    the carts whose tables and weight rows are staged in LDS at a time: JDA_STAGE_CHUNK_4, _8, _16, _32, _64
 * at counts[JDA_STAGE_LAUNCH(dialect, trace, glb, acc, chunk)]. */
enum { JDA_STAGE_ACC_12 = 0, JDA_STAGE_ACC_32 = 1, JDA_STAGE_ACC_64 = 2, JDA_STAGE_ACC_160 = 3 };
enum { JDA_STAGE_CHUNK_4 = 0, JDA_STAGE_CHUNK_8 = 1, JDA_STAGE_CHUNK_16 = 2, JDA_STAGE_CHUNK_32 = 3, JDA_STAGE_CHUNK_64 = 4 };
#define JDA_STAGE_LAUNCH(dialect, trace, glb, acc, chunk) \
  ((((((dialect) * 2 + (trace)) * 2 + (glb)) * 4 + (acc)) * 5) + (chunk))
#define JDA_STAGE_LAUNCH_N 160
/* counts[i]: how often the passes of this cascador have issued launch i since it was created: one count per launch, so
 * stages x levels per dense pass.  Cumulative, added atomically on the host where Pass::run_dense issues the launches;
 * take the difference around a call, as with jdaFinishForms.  A pass that is issued again counts its launches again.
 * Returns 0, or -1 for a null argument. */
JDA_API int jdaStageLaunches(void *cascador, long long counts[JDA_STAGE_LAUNCH_N]);
/* Runs nothing: the index in those counts that a level of `win`-pixel windows, `step` pixels apart, would launch with
 * this cascador's model in `dialect`, traced or not; *lds_bytes (may be null) receives that launch's dynamic LDS size.
 * -1: dense mode declines the model (more than 160 shape coordinates or 256 leaves a tree, or a tile's shapes and four
 * carts' tables beyond 160 KB of LDS) or the dialect (dialect CPP under the similarity transform, a multi-scale
 * model), or a null cascador, an unknown dialect, win < 1 or step < 1.  Needs no device. */
JDA_API int jdaStageLaunchFor(void *cascador, int dialect, int trace, int win, int step, int *lds_bytes);

/* Window enumeration of reference c/jda.c:320-339 without running anything:
 * number of candidate windows and pyramid levels for one frame. */
JDA_API int jdaCountWindows(int width, int height, float scale, int min_size, int max_size,
                            long long *n_windows, int *n_levels);

/* Work counters of one detect call: the DetectionStatisic of reference
 * include/jda/cascador.hpp:14-25, plus what the roofline accounting needs. */
typedef struct {
  long long patch_n;          /* candidate windows scanned                    */
  long long face_patch_n;     /* windows that passed every cart (+ final th)  */
  long long nonface_patch_n;  /* patch_n - face_patch_n                       */
  long long cart_gothrough_n; /* reject lengths (Validate's n, cascador.cpp:187) */
                              /* summed over the NON-face windows only, like  */
                              /* the reference (cascador.cpp:359-364)         */
  long long stage_done_n[16]; /* windows that completed stage t (shape update) */
  double average_cart_n;      /* cart_gothrough_n / nonface_patch_n; 0.0 when */
                              /* nonface_patch_n is 0 (every window a face),  */
                              /* where the reference divides 0 by 0 (NaN,     */
                              /* cascador.cpp:307,375)                        */
  /* Dialect CPP on a trainer snapshot (header stage s < T, cart c; jdaDetectBatchCpp): patch_n, face_patch_n,
   * nonface_patch_n and cart_gothrough_n are Validate's.  The pass-through padding makes a face walk all T*K carts and
   * complete every stage, so with ran = s*K + min(K, c+1), the carts Validate runs for a face:
   *   cart_total_n    = Validate's carts over all windows + face_patch_n * (T*K - ran)
   *                   = cart_gothrough_n + face_patch_n * T*K   (snapshot or not)
   *   stage_done_n[t] = Validate's count for t < s;  face_patch_n for s <= t < T (Validate updates no shape there). */
  double gpu_ms;              /* device time of the call (HIP events; the events -- five marker packets per */
                              /* pass -- are only recorded when statistics are asked for)                   */
  double scan_ms;             /* device time of the stage-0 scan launches (first start to last end; */
                              /* two sub-batches scan side by side on big batches)                  */
  double host_ms;             /* host post-processing (sort, NMS, relocation) */
  long long scan_cart_n;      /* part of cart_gothrough_n done by the stage-0 scan kernel */
  long long scan_patch_n;     /* windows the stage-0 scan kernel covered      */
  int scan_launches;          /* launches of the stage-0 scan kernel (one per tiled level) */
  long long handoff_n;        /* windows handed from the scan to the finishing kernel (incl. untiled levels) */
  long long cart_total_n;     /* carts evaluated over ALL windows (roofline accounting) */
  double call_ms;             /* wall clock of the whole C call                 */
  int dense_passes;           /* passes that ran in dense mode (whole stages per window tile, k_stage) */
  double scan_lds_ms;         /* HIP-event span of the LDS-tiled k_scan launches alone; only meaningful when the launches of
                                 a call run back to back on one stream (JDA_LANES=1 JDA_SIDE_STREAM=0), 0 otherwise */
  long long scan_lds_cart_n;  /* carts evaluated by the LDS-tiled k_scan launches (scan_cart_n minus the global-pixel levels) */
  int scan_fallbacks;         /* passes of this call that were run a second time with the closed-tile scan kernel because the
                                 persistent one tripped a watchdog or covered too few windows (results are correct; see stderr) */
  int ws_regrows;             /* passes of this call that were run a second time because a queue sized from earlier passes'
                                 survivor fractions was too small (option "ws_bound"; results are correct; see stderr) */
  int post_passes;            /* passes of this call whose frames were post-processed on the device (option "device_post": scan
                                 order, score order, NMS and relocation by k_post); 0 in dialect CPP and with device_post = 0 */
  int post_declined;          /* passes of this call in which k_post was launched and declined (a frame with more than 1,024
                                 detections, ties or NaN among more than 256 scores, more rows than reserved): the host form took
                                 the pass, the results are the same */
} jdaStats;

typedef struct {
  int dialect;          /* JDA_DIALECT_*                                      */
  int nms;              /* 1: apply NMS (default), 0: return every survivor   */
  float nms_overlap;    /* IoU threshold, 0.3 in reference c/jda.c:238        */
  int cpp_step;         /* dialect CPP: pixel step (config fddb.step)         */
  void *hip_stream;     /* hipStream_t to enqueue on, NULL = library's own    */
  jdaStats *stats;      /* optional out                                       */
} jdaDetectOptions;

JDA_API void jdaDetectOptionsInit(jdaDetectOptions *opt);

/* Batch of n equally sized frames in HOST memory (frames[i] is width*height
 * bytes).  out must point at n jdaResult slots; each is released separately
 * with jdaResultRelease.  Per frame the result is identical to n separate
 * jdaDetect calls.  Returns 0 on success. */
JDA_API int jdaDetectBatch(void *cascador, const unsigned char *const *frames, int n,
                           int width, int height, float scale, float step,
                           int min_size, int max_size, float th,
                           const jdaDetectOptions *opt, jdaResult *out);

/* Same, frames already resident in device memory: frame i starts at
 * d_frames + i*frame_stride (frame_stride >= width*height).  This is the
 * entry the throughput benchmark times. */
JDA_API int jdaDetectBatchDevice(void *cascador, const unsigned char *d_frames,
                                 size_t frame_stride, int n, int width, int height,
                                 float scale, float step, int min_size, int max_size,
                                 float th, const jdaDetectOptions *opt, jdaResult *out);

/* Ragged batch: n images of DIFFERENT sizes in one job -- the reference's FDDB loop, one Detect per image
 * (src/test.cpp:100-170), or any loop of jdaDetect calls over a list of images.  images[i] is widths[i]*heights[i]
 * bytes in HOST memory, rows back to back (the `data` of jdaDetect); out must point at n jdaResult slots.  Per
 * image the result is identical to jdaDetect(cascador, images[i], widths[i], heights[i], scale, step, min_size,
 * max_size, th).  The images are staged on the device with one common row pitch, the pyramid levels (the same
 * window-size series for every image, c/jda.c:331-333) share tile shapes and stage-0 tables, and the job runs as a
 * few large passes (chunks of `ragged_chunk_windows` candidate windows, three in flight) instead of n latency-bound
 * ones.  Models with multi-scale split nodes and cascades that reject almost nothing run image by image inside.
 * Images too small for a window give an empty result, like jdaDetect.  Returns 0 on success. */
JDA_API int jdaDetectBatchRagged(void *cascador, const unsigned char *const *images, const int *widths,
                                 const int *heights, int n, float scale, float step, int min_size, int max_size,
                                 float th, const jdaDetectOptions *opt, jdaResult *out);

/* Same, images already resident in device memory: image i starts at d_base + offsets[i], rows back to back. */
JDA_API int jdaDetectBatchRaggedDevice(void *cascador, const unsigned char *d_base, const size_t *offsets,
                                       const int *widths, const int *heights, int n, float scale, float step,
                                       int min_size, int max_size, float th, const jdaDetectOptions *opt,
                                       jdaResult *out);

/* The same two jobs with the results as ONE matrix instead of n jdaResults: a row per detection,
 *   [frame_offset + image index, x, y, size, score, shape (2L absolute coordinates)]   (5 + 2L floats),
 * images in order, detections of an image in jdaDetect's order -- exactly what jdaResultsPack makes of the n results,
 * and the form the multi-GPU gather ships (include/jda_dist.h).  A job of hundreds of images returns a few hundred
 * KB of rows; three allocations per image cost more host time than that (r06: 50 us of a 1.2-ms job).  *rows is
 * malloc'd by the library (also when *n_rows is 0) and released with jdaRowsRelease.  Returns 0 on success. */
JDA_API int jdaDetectBatchRaggedRows(void *cascador, const unsigned char *const *images, const int *widths,
                                     const int *heights, int n, float scale, float step, int min_size, int max_size,
                                     float th, const jdaDetectOptions *opt, int frame_offset, float **rows, int *n_rows);
JDA_API int jdaDetectBatchRaggedDeviceRows(void *cascador, const unsigned char *d_base, const size_t *offsets,
                                           const int *widths, const int *heights, int n, float scale, float step,
                                           int min_size, int max_size, float th, const jdaDetectOptions *opt,
                                           int frame_offset, float **rows, int *n_rows);
JDA_API void jdaRowsRelease(float *rows);

/* Up to three batches in flight on one cascador, driven by ONE host thread (streams of batches, e.g. video):
 * Submit queues a batch of device-resident frames on a lane of its own (stream + workspace) and returns at once with
 * a ticket (0..2; -1 on error: every ticket in use, multi-scale model); Wait collects that batch, post-processes it
 * and fills out[0..n) exactly like jdaDetectBatchDevice.  When earlier passes on this frame size have shown how many
 * windows survive the scan, the WHOLE batch (scan, finishing launches, copies of the results) is queued by Submit and
 * Wait is a single host wait.  Submitting batch i+1 before waiting for batch i keeps the GPU busy with batch i+1
 * while the host parts of batch i (D2H, sort, NMS, result assembly) run (one batch ahead is enough for frames that
 * are already on the device; frames coming from the host want two ahead, see jdaDetectBatchSubmitHost).
 * The frames must stay valid until Wait returns.  The other entry points keep working while tickets are pending
 * (they run on other lanes).  Wait takes the stats pointer (gpu_ms = that batch's own device span, call_ms = submit
 * to the end of wait); nothing is written through opt->stats by Submit, but a non-NULL opt->stats tells it to bracket
 * the pass with timing events -- without it Wait reports the counters and gpu_ms = scan_ms = 0. */
JDA_API int jdaDetectBatchSubmit(void *cascador, const unsigned char *d_frames, size_t frame_stride, int n,
                                 int width, int height, float scale, float step, int min_size, int max_size,
                                 float th, const jdaDetectOptions *opt);
JDA_API int jdaDetectBatchWait(void *cascador, int ticket, jdaStats *stats, jdaResult *out);

/* Submit for frames in HOST memory (frames[i] is width*height bytes): the batch is copied to a staging buffer
 * of its ticket (uploads of at least `h2d_min_bytes` go batch after batch through one upload stream of the cascador,
 * smaller ones on the ticket's own stream), then scanned like jdaDetectBatchSubmit.  The copy and the scan launches
 * are issued by a helper thread AFTER this call has returned, so in EVERY case -- pageable or pinned frames --
 * the frame BYTES must stay valid and unchanged until jdaDetectBatchWait for this ticket has returned (do not reuse
 * a capture buffer before that).  The frames[] pointer array itself is copied by this call and may go at once.
 * A ticket lives for copy + kernels + host work while the copy alone takes about half of that: keep TWO
 * batches submitted ahead of the one being waited for and the PCIe link never idles. */
JDA_API int jdaDetectBatchSubmitHost(void *cascador, const unsigned char *const *frames, int n,
                                     int width, int height, float scale, float step, int min_size, int max_size,
                                     float th, const jdaDetectOptions *opt);

/* Per-window trace of the cascade (parity instrumentation; HOST output
 * arrays of n*windows_per_frame entries in scan order, any may be NULL):
 *   carts_n    number of carts evaluated, counted like `n` in the reference's
 *              Validate (index of the rejecting cart + 1, or T*K)
 *   score      score when the walk stopped (before the final threshold)
 *   path_hash  FNV-1a over the leaf index of every evaluated cart
 *   shapes     2L floats, window-normalised shape after the last completed
 *              stage (mean shape if none completed)
 * Frames are host memory. Dialect C only. */
JDA_API int jdaTraceBatch(void *cascador, const unsigned char *const *frames, int n,
                          int width, int height, float scale, int min_size, int max_size,
                          int *carts_n, float *score, unsigned int *path_hash, float *shapes);

/* The cascade on windows the CALLER names (a tracker re-checking last frame's boxes, a proposal stage in front of the
 * cascade, a float model scored on annotated boxes): the body of the reference's window loop, c/jda.c:340-414, for each
 * of n_windows windows, 4 ints per window: (frame, x, y, size).  There is no grid, no minimum size of 24, no NMS.
 *   views      o at (x, y); h at ((int)(x*r), (int)(y*r)), r = 1.f / sqrtf(2.f), the product in float; q at (x/2, y/2); all
 *              three patch sides are `size` (c/jda.c:340-354).  Half and quarter images are jdaBuildPyramid's pair of
 *              the frame, built only for a model with a scale != 0 split node; a read that leaves them is clamped into the
 *              image, like every dialect-C entry's (the documented divergence from the reference's out-of-bounds read).
 *   walk       from the stored mean shape, score = (score + leaf - mean) / std in cart order in fp32, reject at the first
 *              score < cart threshold, the K-row regression after each completed stage (c/jda.c:361-412).
 * Outputs are HOST arrays of n_windows entries in the caller's order, any may be NULL; carts_n, score, path_hash and
 * shapes are defined as jdaTraceBatch defines them (shapes also for rejected windows):
 *   is_face    no cart rejected the window (carts_n == T*K and the last cart passed it) && !(score < th)   (c/jda.c:414)
 *   landmarks  2L floats, shapes[2j] * size + x and shapes[2j+1] * size + y in fp32, a multiply and then an add
 *              (c/jda.c:471-472), for every window
 *   stats      patch_n, face_patch_n, nonface_patch_n, cart_gothrough_n (non-faces only), average_cart_n, call_ms -- as
 *              jdaValidateCpp fills them -- and gpu_ms, the kernels' device time; everything else 0
 * A cascador created from a double file or from a trainer snapshot behaves as in jdaTraceBatch.  Returns 0; or -1 with
 * jdaGetLastError() naming the offending window (its index and four values), nothing launched and no output touched, for:
 * a needed pointer that is NULL; n < 0 or n_windows < 0; frame outside [0, n); size < 1, x < 0, y < 0, x + size > width or
 * y + size > height; a frame size the other dialect-C entries refuse.  n_windows == 0 returns 0 and touches nothing;
 * duplicate windows and frames no window names are fine.  Re-entrant on one cascador like the other entries.  Windows
 * up to the side jdaGetOption("windows_tile_limit") reports walk from a copy of their pixels in LDS, larger ones (and
 * every window with option "windows_tile" = 0) read the frame: identical bits.  The list goes through the device in
 * chunks that fit option "workspace_mb". */
JDA_API int jdaValidateWindows(void *cascador, const unsigned char *const *frames, int n, int width, int height,
                               const int *windows, int n_windows, float th,
                               unsigned char *is_face, float *score, int *carts_n, unsigned int *path_hash,
                               float *shapes, float *landmarks, jdaStats *stats);
/* Same, frames already resident in device memory: frame i starts at d_frames + i*frame_stride
 * (frame_stride >= width*height). */
JDA_API int jdaValidateWindowsDevice(void *cascador, const unsigned char *d_frames, size_t frame_stride, int n,
                                     int width, int height, const int *windows, int n_windows, float th,
                                     unsigned char *is_face, float *score, int *carts_n, unsigned int *path_hash,
                                     float *shapes, float *landmarks, jdaStats *stats);

/* The image pair of reference c/jda.c:450-457 (half = 1/sqrt(2), quarter =
 * 1/2) built by the device resize kernel; exposed for the parity tests.
 * half/quarter are HOST buffers of hw*hh and qw*qh bytes. */
JDA_API int jdaBuildPyramid(void *cascador, const unsigned char *data, int width, int height,
                            unsigned char *half, int *hw, int *hh,
                            unsigned char *quarter, int *qw, int *qh);

/* Dialect CPP results carry doubles (reference Detect fills
 * vector<Rect>, vector<double>, vector<Mat_<double>>). */
typedef struct {
  int n;
  int landmark_n;
  int *rects;      /* n * (x, y, w, h)            */
  double *shapes;  /* n * 2L absolute coordinates */
  double *scores;  /* n                           */
} jdaResultD;

JDA_API void jdaResultDRelease(jdaResultD result);

/* Dialect CPP batch detect on host frames: reference JoinCascador::Detect with
 * fddb.method = 1 (src/jda/cascador.cpp:431-477): minimum_size, pixel step,
 * scale factor, NMS overlap, nms on/off come from the arguments instead of
 * the Config singleton.
 * A trainer snapshot (a double file whose header says the model is still in training: stage s < T, cart c) runs the way the
 * reference's Validate runs it -- stages [0, s) in full, then carts [0, c] of stage s without that stage's regression
 * (src/jda/cascador.cpp:177-209) -- in every dialect-CPP entry; jdaStats::cart_total_n counts the padding carts a face walks,
 * nothing else sees them.  With jdaSetSimilarityTransform(1) the stage in training walks with the parameter the stage before
 * it computed (Validate does not recompute stp_mc for it, cascador.cpp:178-200).  Refused (-1, jdaGetLastError): a training
 * status the reference's loader asserts against (cascador.cpp:138-141).  jdaDetect and the other dialect-C entries ignore
 * the header, like c/jda.c:499-505. */
JDA_API int jdaDetectBatchCpp(void *cascador, const unsigned char *const *frames, int n,
                              int width, int height, int minimum_size, int step,
                              double factor, double overlap, int nms,
                              jdaStats *stats, jdaResultD *out);

/* The same with the frames already resident in device memory (frame i at d_frames + i*frame_stride): the entry the
 * dialect-CPP throughput figures of bench.py are timed on. */
JDA_API int jdaDetectBatchCppDevice(void *cascador, const unsigned char *d_frames, size_t frame_stride, int n,
                                    int width, int height, int minimum_size, int step,
                                    double factor, double overlap, int nms,
                                    jdaStats *stats, jdaResultD *out);

/* Dialect CPP ragged batch: n images of DIFFERENT sizes as one job -- literally the loop of the reference's `jda fddb`
 * command, one joincascador.Detect(gray, ...) per image with fddb.method = 1 (src/test.cpp:100-170, line 142;
 * src/jda/cascador.cpp:310-376,431-477).  images[i] is widths[i]*heights[i] bytes in HOST memory, rows back to back;
 * out must point at n jdaResultD slots.  Per image the result is identical to jdaDetectBatchCpp on that image alone.
 * The window sizes minimum_size, int(win*factor), ... (cascador.cpp:314,369) are one series for every image, an image
 * uses the prefix that fits both its sides (cascador.cpp:333): levels, tile shapes and stage-0 tables are shared and
 * the job runs as a few large passes, like jdaDetectBatchRagged.  Models with multi-scale split nodes run image by
 * image inside.  PARITY UNPINNED like every dialect-CPP entry.  Returns 0 on success. */
JDA_API int jdaDetectBatchCppRagged(void *cascador, const unsigned char *const *images, const int *widths,
                                    const int *heights, int n, int minimum_size, int step,
                                    double factor, double overlap, int nms,
                                    jdaStats *stats, jdaResultD *out);

/* Same, images already resident in device memory: image i starts at d_base + offsets[i], rows back to back. */
JDA_API int jdaDetectBatchCppRaggedDevice(void *cascador, const unsigned char *d_base, const size_t *offsets,
                                          const int *widths, const int *heights, int n, int minimum_size, int step,
                                          double factor, double overlap, int nms,
                                          jdaStats *stats, jdaResultD *out);

/* The two dialect-CPP ragged jobs with the results as ONE matrix of rows of (6 + 2*landmark_n) doubles,
 * [frame_offset + image index, x, y, w, h, score, shape...], images in order, an image's rows in Detect's order (after the
 * score-ordered NMS, cascador.cpp:444-474) -- exactly what jdaResultsDPack makes of the n jdaResultDs, without building
 * them: the FDDB-sized job keeps 32 k candidates = 15 MB of rows, and going through 2,845 results and a pack cost 4 ms
 * of a 38-ms job.  *rows is malloc'd by the library (also when *n_rows is 0); release it with jdaRowsDRelease. */
JDA_API int jdaDetectBatchCppRaggedRows(void *cascador, const unsigned char *const *images, const int *widths,
                                        const int *heights, int n, int minimum_size, int step, double factor,
                                        double overlap, int nms, jdaStats *stats, int frame_offset,
                                        double **rows, int *n_rows);
JDA_API int jdaDetectBatchCppRaggedDeviceRows(void *cascador, const unsigned char *d_base, const size_t *offsets,
                                              const int *widths, const int *heights, int n, int minimum_size, int step,
                                              double factor, double overlap, int nms, jdaStats *stats, int frame_offset,
                                              double **rows, int *n_rows);
JDA_API void jdaRowsDRelease(double *rows);

/* Flattens n dialect-CPP results into rows of (6 + 2*landmark_n) doubles: [frame_offset + i, x, y, w, h, score, shape...]
 * (the rows reference src/test.cpp:153-163 prints per image, plus the landmarks) -- what is gathered across GPUs for the
 * dialect-CPP FDDB job.  rows may be NULL to query the row count.  Returns the number of rows, or -1 if capacity_rows is
 * too small. */
JDA_API int jdaResultsDPack(const jdaResultD *results, int n, int frame_offset, double *rows, int capacity_rows);

/* Releases n dialect-CPP results at once (same as n jdaResultDRelease calls). */
JDA_API void jdaResultsDRelease(jdaResultD *results, int n);

/* Dialect CPP only: the similarity-transform mode of Validate (reference
 * src/jda/data.cpp:64-126, config key face.similarity_transform, common.cpp:214; off in
 * the shipped config).  Per stage, sR = Calc(shape, mean_shape) rotates/scales the node
 * offsets and the regressed delta shape.  PARITY UNPINNED twice over: dialect CPP itself,
 * and two OpenCV details it leans on (cv::norm's accumulation order, `Mat_ /= double` as a
 * multiply by the reciprocal), both restated identically in the oracle and the kernel. */
JDA_API int jdaSetSimilarityTransform(void *cascador, int on);

/* Dialect CPP, detect method 0 -- the true image pyramid of reference
 * src/jda/cascador.cpp:216-308 (detectMultiScale + detectSingleScale): a fixed
 * origin_size x origin_size window (config image_size.origin_size, 48 in the shipped
 * config) slides with a pixel step over an image that is shrunk by 1/factor per level
 * ON THE DEVICE with a restatement of cv::resize(INTER_LINEAR); rects are scaled back
 * with truncating int *= double.  scale==0 models only (multi-scale models: jdaDetectBatchCppPyramidMS).  PARITY UNPINNED: cv::resize
 * itself cannot be compared here (no OpenCV), only its restatement in the oracle. */
JDA_API int jdaDetectBatchCppPyramid(void *cascador, const unsigned char *const *frames, int n,
                                     int width, int height, int origin_size, int step,
                                     double factor, double overlap, int nms,
                                     jdaStats *stats, jdaResultD *out);

/* The same for models with multi-scale split nodes: detectSingleScale resizes EVERY window's ROI to the config's
 * three sizes (image_size.origin_size / half_size / quarter_size -- 48 / 36 / 24 in the shipped config,
 * src/jda/cascador.cpp:243-245, common.cpp:129-131); a split node of scale 1 / 2 reads the window's own half / quarter
 * patch with coordinates scaled by that patch's side (data.cpp:21-51).  The patches are built on the device by the
 * cv::resize restatement, one per window and scale.  Serves scale==0 models too (the sizes are then unused).
 * PARITY UNPINNED like the entry above. */
JDA_API int jdaDetectBatchCppPyramidMS(void *cascador, const unsigned char *const *frames, int n,
                                       int width, int height, int origin_size, int half_size, int quarter_size,
                                       int step, double factor, double overlap, int nms,
                                       jdaStats *stats, jdaResultD *out);

/* The cv::resize(INTER_LINEAR, 8-bit gray) restatement by itself (device kernel), for tests. */
JDA_API int jdaResizeCv(void *cascador, const unsigned char *data, int width, int height,
                        unsigned char *out, int out_width, int out_height);

/* Host-only helpers (no GPU needed): the two NMS variants and the model-stream
 * size, exported so that they can be unit-tested and reused.
 * jdaNmsC   : reference c/jda.c:237-316; bboxes are (x,y,size) triples; keep[i]
 *             is set to 1/0; returns the number kept (scan order is preserved).
 * jdaNmsCpp : reference src/jda/cascador.cpp:387-429; rects are (x,y,w,h);
 *             picked[] receives indices in descending-score order; returns count. */
JDA_API int jdaNmsC(const int *bboxes, const float *scores, int n, float overlap, unsigned char *keep);
JDA_API int jdaNmsCpp(const int *rects, const double *scores, int n, double overlap, int *picked);
JDA_API long long jdaModelStreamBytes(int T, int K, int landmark_n, int tree_depth, int real_bytes);

/* The tile plan k_scan would use for a dialect-C call (no GPU needed; tests and tools): per pyramid level
 * 10 ints {win, step, nx, ny, mode, tw, th, pitch, tiles_x, tiles_y}; mode 1/3 = windows share an LDS pixel
 * tile of tw x th windows, 2 = pixels through L1/L2, 0 = not scanned.  Returns the number of levels. */
JDA_API int jdaDebugPlanTiles(void *cascador, int width, int height, float scale, int min_size, int max_size,
                              int *out, int cap_levels);

/* Flattens n per-frame results into rows of (5 + 2*landmark_n) floats:
 * [frame_offset + i, x, y, size, score, shape...] -- the (bbox, score, landmarks)
 * tuple that is gathered across GPUs.  rows may be NULL to query the row count.
 * Returns the number of rows, or -1 if capacity_rows is too small. */
JDA_API int jdaResultsPack(const jdaResult *results, int n, int frame_offset,
                           float *rows, int capacity_rows);

/* Releases n results at once (same as n jdaResultRelease calls). */
JDA_API void jdaResultsRelease(jdaResult *results, int n);

/* Per-window trace of the dialect-CPP cascade, like jdaTraceBatch but with the
 * fp64 state of reference Validate (src/jda/cascador.cpp:166-211): carts_n is
 * Validate's `n`. */
JDA_API int jdaTraceBatchCpp(void *cascador, const unsigned char *const *frames, int n,
                             int width, int height, int minimum_size, int step, double factor,
                             int *carts_n, double *score, unsigned int *path_hash, double *shapes);

/* ---- Dialect CPP: Validate on caller crops, hard-negative mining ------------------------------------------------------
 * The trainer's second caller of JoinCascador::Validate (reference src/jda/cascador.cpp:166-211) is hard-negative mining:
 * DataSet::MoreNegSamples (src/jda/data.cpp:479-530) -> NegGenerator::Generate -> ParallelMining -> Validate
 * (data.cpp:885-1065).  These entries run that Validate on the device.  Every dialect-CPP rule holds: a trainer snapshot
 * runs Validate's own loop bounds (stages [0, s), then carts [0, c] of stage s without its regression), and
 * jdaSetSimilarityTransform(1) applies the similarity transform.  PARITY UNPINNED like every dialect-CPP entry: bit-exact
 * against this project's restatements of Validate and cv::resize, not against the reference, which cannot be built here.
 *
 * Initial shape.  Validate starts from RandomShape(mean_shape) (data.cpp:225-236): mean_shape plus ONE global (x, y), each
 * uniform in [-shift_size, shift_size).  shift_size == 0 gives mean_shape + 0., what every detect entry uses (test() and
 * fddb() force it).  Otherwise crop / window `key` (the crop's index for jdaValidateCpp*, the window's ordinal for the
 * mining entries) draws
 *     x = g(2 key), y = g(2 key + 1),   g(c) = -shift_size + (shift_size - -shift_size) * u(c)
 *     u(c) = (splitmix64(seed + (c + 1) * 0x9E3779B97F4A7C15) >> 11) * 2^-53      (arithmetic mod 2^64)
 *     splitmix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; return z ^ z >> 31
 * -- the a + (b - a) * u form of cv::RNG::uniform(double, double), reproducible and independent of how a job is cut into
 * calls.  (The reference seeds with getTickCount(); its draws cannot be reproduced and are not a goal.)  The shift enters
 * the initial shape only: STParameter::Calc keeps the stored mean_shape as its second argument.
 *
 * Patches.  origin_size / half_size / quarter_size are the config's image_size.* (48 / 36 / 24 shipped, common.cpp:129-131),
 * each in [1, 128].  Every patch is cv::resize(INTER_LINEAR) as restated in this library (jdaResizeCv): the crop -> o, then
 *   resize_mode 0, mining (data.cpp:987-990):           o -> h, o -> q
 *   resize_mode 1, detectSingleScale (cascador.cpp:243-245): crop -> h, crop -> q
 * A model without scale != 0 split nodes only reads o. */

/* Validate on n_crops caller crops, each 5 ints (image, x, y, w, h); a crop must lie inside its image (-1 otherwise).
 * images[i] is widths[i]*heights[i] bytes in HOST memory, rows back to back.  Per crop, into host arrays (any may be NULL):
 *   is_face  1 if Validate returned true
 *   score    the score where the walk stopped
 *   carts_n  Validate's n (cascador.cpp:187): carts it ran -- s*K + c + 1 for a face of a snapshot, T*K for a face of a
 *            complete model
 *   shape    2L doubles, the window-normalised shape as Validate leaves it (rejected crops too)
 * stats: patch_n, face_patch_n, nonface_patch_n, cart_gothrough_n (non-faces only), average_cart_n, call_ms.
 * Returns 0, or -1 with jdaGetLastError(). */
JDA_API int jdaValidateCpp(void *cascador, const unsigned char *const *images, const int *widths, const int *heights,
                           int n_images, const int *crops, int n_crops, int origin_size, int half_size, int quarter_size,
                           int resize_mode, double shift_size, uint64_t seed, unsigned char *is_face, double *score,
                           int *carts_n, double *shape, jdaStats *stats);
/* Same, images resident in device memory: image i at d_base + offsets[i] (jdaDetectBatchCppRaggedDevice's convention). */
JDA_API int jdaValidateCppDevice(void *cascador, const unsigned char *d_base, const size_t *offsets, const int *widths,
                                 const int *heights, int n_images, const int *crops, int n_crops, int origin_size,
                                 int half_size, int quarter_size, int resize_mode, double shift_size, uint64_t seed,
                                 unsigned char *is_face, double *score, int *carts_n, double *shape, jdaStats *stats);

/* Work counters of one mining call; they cover exactly the windows [start, next_start). */
typedef struct {
  long long windows;        /* windows consumed: next_start - start                                   */
  long long nega_n;         /* windows Validate rejected (ParallelMining's nega_n, data.cpp:1001-1004) */
  long long carts_n;        /* their Validate n, summed (rejected windows only, like the reference)   */
  long long next_start;     /* one past the size-th hit, or the end of the enumeration                */
  long long total_windows;  /* windows of the whole enumeration                                       */
  int hits;                 /* hard negatives returned                                                */
  double call_ms;           /* wall clock of the call                                                 */
} jdaMineStats;

/* NegGenerator's background walk (NextImage, data.cpp:885-967), restated per image in list order:
 *   - image i is first transformed by transforms[i] in 0..7 exactly as data.cpp:930-963 composes cv::flip and transpose
 *     (1, 3, 5, 7 transpose, so W and H swap) -- on the device, by remapping coordinates;
 *   - it is skipped unless W > origin_size && H > origin_size (data.cpp:921);
 *   - win starts at origin_size; a level is the full grid, y from 0 in steps of steps[i] while y + win <= H, x the same
 *     against W, row by row; the next level has win = (int)(win * factors[i]) (State::win_size is an int), and the
 *     image ends when win >= W || win >= H (a factor that does not grow win is refused: the reference would never end).
 * The reference draws step and factor from cv::RNG(getTickCount()) (data.cpp:910-911): here they are the caller's.
 * One deliberate difference: the reference skips (0, 0) of the FIRST image of each thread (its `x += step` runs before the
 * first crop) and interleaves threads nondeterministically; here every window is enumerated once, in order.
 * Every window, ordinal by ordinal from `start`, goes through resize_mode 0 and Validate.  Returned: the FIRST `size` faces
 * (hard negatives) at or after `start`, in enumeration order -- hits[4h..4h+3] = (image, x, y, win) in the transformed
 * image, score[h], shape[2L h ..] and patches[h * (o^2 + h^2 + q^2) ..] (the o, h, q patch bytes MoreNegSamples stores,
 * data.cpp:510-520); any output may be NULL, each must hold `size` entries.  Chaining calls through stats->next_start gives
 * the results of one larger call.  The enumeration is processed in chunks in order, and the call stops after the chunk
 * that holds the size-th hit (device workspace within the cascador's "workspace_mb").  Returns the number of hits, or -1. */
JDA_API int jdaMineNegativesCpp(void *cascador, const unsigned char *const *images, const int *widths, const int *heights,
                                int n_images, const int *steps, const double *factors, const int *transforms,
                                int origin_size, int half_size, int quarter_size, long long start, int size,
                                double shift_size, uint64_t seed, int *hits, double *score, double *shape,
                                unsigned char *patches, jdaMineStats *stats);
/* Same, images resident in device memory (image i at d_base + offsets[i]): the throughput entry -- a trainer keeps its
 * background set in HBM across every MoreNegSamples call. */
JDA_API int jdaMineNegativesCppDevice(void *cascador, const unsigned char *d_base, const size_t *offsets, const int *widths,
                                      const int *heights, int n_images, const int *steps, const double *factors,
                                      const int *transforms, int origin_size, int half_size, int quarter_size,
                                      long long start, int size, double shift_size, uint64_t seed, int *hits,
                                      double *score, double *shape, unsigned char *patches, jdaMineStats *stats);

/* What the mining and Validate calls of a cascador launched ("the kernels at their limits").
 * jdaMineNegativesCpp* and jdaValidateCpp* count the launches of the five kernels of k_mine.hip here, where the launch is
 * made: a launcher that returns without launching (nothing to do) counts nothing.  (jdaValidateSamplesCpp's lane-per-sample
 * form borrows k_mine_walk for resident samples; it is no mining call and counts nothing here.)
 *   JDA_MINE_K_SCAN .. JDA_MINE_K_SUM  launches of k_mine_scan, k_mine_items, k_mine_patches, k_mine_walk, k_mine_sum
 *   JDA_MINE_CHUNKS          chunks of the enumeration a mining call scanned (one k_mine_scan launch each)
 *   JDA_MINE_WALK_BATCHES    batches of crops that went through k_mine_patches + k_mine_walk, of mining and of Validate
 *   JDA_MINE_SUM_SATURATED   k_mine_sum launches whose grid stood at its largest, so that a lane read more than one
 *                            window's status (more windows than lanes)
 *   JDA_MINE_SCAN_REJECTS    windows k_mine_scan rejected below a chunk's cut (what k_mine_sum counted)
 *   JDA_MINE_WALK_REJECTS    windows of a mining call that k_mine_walk rejected below a chunk's cut; the two add up to
 *                            jdaMineStats::nega_n over the same calls
 * Those ten are cumulative since the cascador was created, added atomically; take the difference around a call.  Two are
 * not sums:
 *   JDA_MINE_WALK_BATCH_MAX  the largest batch so far, in crops (never shrinks)
 *   JDA_MINE_WALK_CAP        the most crops a batch could hold in the LAST call that sized its walk buffers: what
 *                            "workspace_mb", the model and the patch sizes allow (at most 65,536), and for
 *                            jdaValidateCpp* no more than the call's crops
 * Returns 0, or -1 for a null argument.  Needs no device. */
enum { JDA_MINE_K_SCAN = 0, JDA_MINE_K_ITEMS = 1, JDA_MINE_K_PATCHES = 2, JDA_MINE_K_WALK = 3, JDA_MINE_K_SUM = 4,
       JDA_MINE_CHUNKS = 5, JDA_MINE_WALK_BATCHES = 6, JDA_MINE_SUM_SATURATED = 7, JDA_MINE_SCAN_REJECTS = 8,
       JDA_MINE_WALK_REJECTS = 9, JDA_MINE_WALK_BATCH_MAX = 10, JDA_MINE_WALK_CAP = 11, JDA_MINE_LAUNCH_N = 12 };
JDA_API int jdaMineLaunches(void *cascador, long long counts[JDA_MINE_LAUNCH_N]);

/* Host-only (no GPU): the mining enumeration of ONE (already transformed) w x h image -- windows and levels; the listing
 * writes up to cap (x, y, win) triples in enumeration order and returns the number of windows (-1 on bad arguments). */
JDA_API int jdaMineWindows(int w, int h, int origin_size, int step, double factor, long long *n, int *levels);
JDA_API long long jdaMineWindowList(int w, int h, int origin_size, int step, double factor, int *xyw, long long cap);

/* ---- Dialect CPP: training one CART -------------------------------------------------------------------------------------
 * What the reference's trainer does with the samples mining returns: Cart::Train -> Cart::SplitNode (reference
 * src/jda/cart.cpp:41-162) -- per internal node a pool of candidate features is evaluated on every sample that reached the
 * node (DataSet::CalcFeatureValues, data.cpp:148-173), one (feature, threshold) is picked by weighted entropy
 * (SplitNodeWithClassification, cart.cpp:176-252) or by the variance of one landmark's residual (SplitNodeWithRegression,
 * cart.cpp:288-350), the samples are partitioned and the children split in turn; a leaf's score is
 * 0.5 * (log(pos_w) - log(neg_w)) (cart.cpp:63-89).  PARITY UNPINNED like every dialect-CPP entry: src/jda needs OpenCV and
 * cannot be built here; these entries are bit-exact against a sequential restatement written from the reference's source
 * (tests/train_ref.py), not against the reference.  Out of scope: BoostCart::Train's loop and its restart policy (one step
 * of that loop -- scores, order, cut, weights and the move of the surviving samples -- is the block "from one cart to the
 * next" at the end of this file), the global regression that closes a stage (the blocks "closing a stage" and "a stage's
 * global regression" below), writing the cart into a model file, reading image files (file and JPEG reading stay the
 * caller's; the colour conversion is the block "frames as they arrive", what LoadPositiveDataSet does with the decoded images
 * the block "the positive sample set", both at the end of this file).
 *
 * Samples.  One struct describes a set of n samples.  origin_size / half_size / quarter_size are call arguments, each in
 * [1, 128]; the landmark count L and tree_depth come from the cascador (it also supplies the device, the "workspace_mb"
 * limit of the per-call workspace -- the pool is processed in chunks of features that fit it -- and the error state).
 *
 * Feature values.  Feature::CalcFeatureValue (data.cpp:18-58) with the identity STParameter, evaluated exactly as the
 * dialect-CPP split node is everywhere in this library: fp64 (shape + offset) * side of the patch of the feature's scale,
 * round (halves away from zero), clamp into the patch, pixel difference in [-255, 255].
 *
 * Similarity transform.  With jdaSetSimilarityTransform(1) every entry below refuses (-1) by default: CalcFeatureValues
 * indexes the per-sample transform by the FEATURE index (data.cpp:168, stp_mc[i]), which reads past the array whenever the
 * pool is larger than the set -- that line has no behaviour to reproduce.  Every OTHER consumer of a trained split node uses
 * the sample's own parameter: DataSet::UpdateScores (data.cpp:312), BoostCart::GenLBF (btcart.cpp:399) and Validate
 * (cascador.cpp:180), and the contract below -- a training sample's leaf IS Cart::Forward's -- holds only if feature f on
 * sample j is evaluated with sample j's parameter.  THAT READING IS DEFINED HERE, a deliberate difference from the reference:
 * stp_mc[idx[j]], with stp_mc[s] = STParameter::Calc(shape of s, mean_shape), the mean shape the cascador's.  Because it is
 * this library's definition and not the reference's behaviour the caller opts in: jdaSetOption(cascador, "train_similarity",
 * 1) (environment JDA_TRAIN_SIMILARITY, default 0).  With the option AND jdaSetSimilarityTransform(1) the six device entries
 * of this block, of "closing a stage" and jdaValidateSamplesCpp run under the per-sample transform; with the transform off
 * the option has no effect; it is the only option that turns a refusal into a result and changes no result that exists
 * without it.  The stored parameter of the reference always equals Calc(current shape, mean_shape) where it is used
 * (CalcSTParameters runs at each stage start, cascador.cpp:45-46, and after MoreNegSamples, data.cpp:531; shapes change only
 * when a stage closes), so every entry derives it from samples->shapes (DataSet::CalcSTParameters, data.cpp:131-146, on the
 * device) and jdaSamplesCpp carries no parameter array.  Outside the contract: a sample whose landmarks all coincide has
 * scale1 == 0 and NaN parameters (jdaValidateCpp has the same gap).
 *
 * Randomness is the caller's.  The reference seeds from getTickCount() and per-thread cv::RNGs; none of it is reproducible
 * and none of it is a goal.  The caller passes, per internal node, the pool, the mode (1 classification, 0 regression: the
 * reference's rng.uniform(0., 1.) < probs[stage], cart.cpp:101) and for regression one u per pool feature (the reference's
 * rng.uniform(0.1, 0.9), cart.cpp:320; accepted range [0, 1)).  jdaGenFeaturePoolCpp makes pools the way
 * Cart::GenFeaturePool does (cart.cpp:352-390) on the counter-based generator of the mining block above: with
 *     G = 0x9E3779B97F4A7C15, base(i) = splitmix64(splitmix64(seed + (key + 1) * G) + (i + 1) * G)      (mod 2^64)
 *     draw d = 1, 2, ... of feature i:  r(d) = splitmix64(base(i) + d * G),  unit(d) = (r(d) >> 11) * 2^-53
 * feature i consumes its draws in this order: per round of the rejection loop four draws x1, y1, x2, y2, each
 * -1 + (1 - -1) * unit (the loop ends when x1*x1 + y1*y1 <= 1 and x2*x2 + y2*y2 <= 1); then scale = r % 3 (drawn always,
 * then forced to 0 without multi_scale); landmark_id1 = r % L; landmark_id2 = r % L; offsets = point * radius; last
 * u = 0.1 + (0.9 - 0.1) * unit.
 *
 * Classification split, literally cart.cpp:176-252: per feature two 511-bin weighted histograms and two count histograms
 * over value + 255, the totals wp_r / wn_r, the sweep th = -255 .. 255 with the 0.1 / 0.9 count-ratio gates, calcEntropy
 * (isZero's 1e-9, division by log(2.)) and strict <; across features the first strict minimum.  An empty side follows from
 * the same IEEE expressions (0/0 ratios and NaN entropies never pass a gate or a <) and is part of the contract.
 * SUMMATION ORDER IS THE REFERENCE'S: every bin and both totals add the weights in sample order.
 *
 * Regression split, cart.cpp:288-350: pos_n == 0 -> feature 0, threshold -256 (criterion 0 / thresholds -256 reported for
 * every feature; the reference returns before it computes any).  Otherwise per feature threshold_ = the int(pos_n * u)-th
 * smallest value over ALL positives of the node (an order statistic of integers: taken from a count histogram), left / right
 * by value <= threshold_ over the positives with has_gt, (var(lx) + var(ly)) * n_left + (var(rx) + var(ry)) * n_right,
 * var = m2 - m1 * m1, an empty side 0; first strict minimum.  calcVariance goes through cv::mean and Mat::mul, whose
 * summation order and form of division only the real OpenCV decides.  DEFINED here: m1 = (sum of v in sample order) * (1. / n),
 * m2 = (sum of v * v in sample order) * (1. / n) -- the multiply-by-reciprocal form is how cv::mean is remembered
 * (`s * (1. / nz)`), FROM MEMORY AND UNCHECKED; a third OpenCV-decided detail next to cv::norm and Mat /= double.
 *
 * Whole cart, cart.cpp:57-162: from the root, split, partition stably (a child's samples stay in ascending sample order,
 * which is what makes the children's summation order the reference's), level by level to the leaves (the reference's
 * depth-first order does not change the result); leaf score 0.5 * (log(pos_w) - log(neg_w)), pos_w = esp + the weights in
 * order, esp = 2.2e-16 (common.cpp:143).  Every log() is the HOST C library's: the device makes the histograms and ordered
 * sums, the host runs the sweep.  A training sample's leaf is what Cart::Forward returns for it (same feature, threshold and
 * value), so pos_leaf / neg_leaf ARE DataSet::UpdateScores (data.cpp:305-317): the caller adds out_scores[leaf].
 *
 * Reference quirks kept or avoided: stp_mc[i] indexed by feature (avoided: refused, or with "train_similarity" read as
 * stp_mc[idx[j]], above); threshold -256 sends every sample
 * right (kept); the classification gates use counts while the criterion uses weights (kept); regression takes its order
 * statistic over all positives but the variance over the has_gt ones (kept). */

typedef struct {
  const unsigned char *patches;  /* n * (o*o + h*h + q*q) bytes: o, h, q back to back per sample -- the layout
                                    jdaMineNegativesCpp writes into `patches`                                    */
  int patches_on_device;         /* 0: host pointer, 1: device pointer (a trainer keeps its samples in HBM)      */
  const double *shapes;          /* n * 2L, current shapes (host)                                                */
  const double *weights;         /* n (host)                                                                     */
  const double *residual;        /* positives only, n * 2: CalcShapeResidual(idx, landmark_id) (data.cpp:190-208)
                                    as the caller computed it; NULL for negatives                                */
  const unsigned char *has_gt;   /* positives only, n: DataSet::HasGtShape; NULL = all 1                         */
  int n;
} jdaSamplesCpp;

/* The fields of Feature (reference include/jda/common.hpp), offsets already multiplied by the radius. */
typedef struct {
  int scale, landmark_id1, landmark_id2;
  double offset1_x, offset1_y, offset2_x, offset2_y;
} jdaFeatureCpp;

typedef struct {
  int pos_n, neg_n;      /* samples that reached the node                                   */
  int feature_idx;       /* chosen pool index                                               */
  int threshold;
  int mode, pad;
  double criterion;      /* es_ / vs_ of the chosen feature                                 */
} jdaTrainNodeCpp;

typedef struct {
  double call_ms;            /* wall clock of the call                                                    */
  double setup_ms;           /* ... sample upload, shape transpose, workspace                             */
  double device_ms;          /* ... feature values, histograms / ordered sums, their copies to the host   */
  double sweep_ms;           /* ... the host's entropy sweeps / variance arithmetic                       */
  double partition_ms;       /* ... chosen feature's values and the stable partition                      */
  long long feature_evals;   /* feature evaluations on the device                                         */
  int feature_chunks;        /* (node, feature chunk) passes                                              */
  jdaTrainNodeCpp *nodes;    /* IN: NULL, or nodes_n/2 - 1 slots, slot i - 1 for node i = 1 .. nodes_n/2 - 1 */
} jdaTrainStatsCpp;

/* Host only (no GPU): F pool features (and, out_u != NULL, their regression draws) as specified above. */
JDA_API int jdaGenFeaturePoolCpp(int F, int landmark_n, double radius, int multi_scale, uint64_t seed, uint64_t key,
                                 jdaFeatureCpp *out_features, double *out_u);

/* DataSet::CalcSTParameters (data.cpp:131-146) for n shapes (n * 2L doubles, host): stp_mc[i] = STParameter::Calc(shapes[i],
 * mean_shape) and stp_cm[i] = Calc(mean_shape, shapes[i]), each n rows of five doubles (scale, rot00, rot01, rot10, rot11);
 * either may be NULL.  The mean shape is the cascador's.  With jdaSetSimilarityTransform off every row is STParameter's
 * default (1, 1, 0, 0, 1; data.cpp:68-70) and the device is not touched.  No opt-in is needed: the entry trains nothing.
 * Calc is data.cpp:72-112 in its own order, on the device (cv::norm and Mat /= double as restated for Validate: unpinned).
 * stp_cm is what jdaShapeResidualStCpp takes.  n == 0 returns 0 without touching the device; -1: a NULL cascador, NULL
 * shapes with n > 0, a negative n. */
JDA_API int jdaCalcSTParametersCpp(void *cascador, const double *shapes, int n, double *stp_mc, double *stp_cm);

/* CalcFeatureValues over the whole set: out[f * n + j] = value of pool[f] on sample j (F * n ints, row = feature). */
JDA_API int jdaCalcFeatureValuesCpp(void *cascador, const jdaSamplesCpp *samples, int origin_size, int half_size,
                                    int quarter_size, const jdaFeatureCpp *pool, int F, int *out);

/* One node over the full sets: mode 1 classification / 0 regression (u: F draws, regression only).  criterion (F doubles:
 * es_ / vs_) and thresholds (F ints: ths_) may be NULL. */
JDA_API int jdaSplitNodeCpp(void *cascador, const jdaSamplesCpp *pos, const jdaSamplesCpp *neg, int origin_size,
                            int half_size, int quarter_size, const jdaFeatureCpp *pool, int F, int mode, const double *u,
                            int *feature_idx, int *threshold, double *criterion, int *thresholds);

/* What the device wrote for one node, before the host's sweep reads it (a test and diagnosis entry: the criterion is a lossy
 * function of these).  Every pointer is a caller buffer or NULL (not wanted); the call zeroes the given buffers first, then
 * fills what the node's mode makes: a buffer of the other mode, and everything after a regression node without positives
 * (which launches nothing), stays zero.  P = positives on the node's list, N = negatives on it. */
typedef struct {
  short *pos_values;     /* F * P: value of pool[f] at list position j, row = feature (the device's 16-bit values)  */
  short *neg_values;     /* F * N, mode 1                                                                          */
  double *pos_hist_w;    /* F * 511, mode 1: bin value + 255, the weights added in list order                      */
  double *neg_hist_w;    /* F * 511, mode 1                                                                        */
  int *pos_hist_c;       /* F * 511, both modes: the count histogram                                               */
  int *neg_hist_c;       /* F * 511, mode 1                                                                        */
  double *var_sums;      /* F * 8, mode 0: left x, x*x, y, y*y, right x, x*x, y, y*y in list order over has_gt     */
  int *var_n_left;       /* F, mode 0                                                                              */
  int *var_n_right;      /* F, mode 0                                                                              */
  int *var_th;           /* F, mode 0: the order statistic the device took from the counts                         */
  int chunks;            /* OUT: feature chunks the pool was processed in ("workspace_mb")                         */
} jdaSplitSumsCpp;

/* jdaSplitNodeCpp on caller-given lists, with the device's raw outputs.  pos_list / neg_list: pos_list_n / neg_list_n sample
 * indices, STRICTLY ASCENDING and inside [0, n) -- the form Cart::SplitNode's recursion hands a node's samples down in;
 * anything else is refused (-1).  A NULL list means all samples of the set (its count argument is ignored).  The same launch
 * sequence as jdaSplitNodeCpp and jdaTrainCartCpp: one function, which copies each chunk's buffers into `sums` when it is
 * given.  feature_idx, threshold, criterion and thresholds as in jdaSplitNodeCpp. */
JDA_API int jdaSplitNodeSumsCpp(void *cascador, const jdaSamplesCpp *pos, const jdaSamplesCpp *neg, int origin_size,
                                int half_size, int quarter_size, const jdaFeatureCpp *pool, int F, int mode, const double *u,
                                const int *pos_list, int pos_list_n, const int *neg_list, int neg_list_n, int *feature_idx,
                                int *threshold, double *criterion, int *thresholds, jdaSplitSumsCpp *sums);

/* One cart.  With nodes_n = 2^tree_depth: pools is (nodes_n/2 - 1) * F features, node i = 1 .. nodes_n/2 - 1 (the root is 1,
 * the children of i are 2i and 2i + 1, like Cart::features) uses pools[(i - 1) * F ..], modes[i - 1] and
 * us[(i - 1) * F ..] (us may be NULL when no node is a regression node).  Outputs (any may be NULL): out_features /
 * out_thresholds [nodes_n/2 - 1], out_scores [nodes_n/2 leaves], pos_leaf [pos->n] / neg_leaf [neg->n] the leaf of every
 * sample, stats. */
JDA_API int jdaTrainCartCpp(void *cascador, const jdaSamplesCpp *pos, const jdaSamplesCpp *neg, int origin_size,
                            int half_size, int quarter_size, const jdaFeatureCpp *pools, int F, const int *modes,
                            const double *us, jdaFeatureCpp *out_features, int *out_thresholds, double *out_scores,
                            int *pos_leaf, int *neg_leaf, jdaTrainStatsCpp *stats);

/* ---- Dialect CPP: closing a stage ---------------------------------------------------------------------------------------
 * What BoostCart::Train does after the K-th cart of a stage (reference src/jda/btcart.cpp:255-292): GenLBF (btcart.cpp:390-405)
 * walks all K carts of the stage over every sample that is still alive, positives and negatives; the leaf indicators go to
 * liblinear as X (GlobalRegression, btcart.cpp:328-388); GenDeltaShape (btcart.cpp:407-424) sums K rows of the fitted w per
 * sample and the sum is added to the sample's current shape (btcart.cpp:285-292); calcMeanError (common.cpp:41-77) is the
 * "Regression Mean Error" the stage reports.  These entries are the walk, the update and the error on a resident sample
 * set, with the stage's carts and weights as caller arrays -- the form jdaTrainCartCpp hands carts out in.  Nothing is
 * written into a model.  PARITY UNPINNED like every dialect-CPP entry: src/jda needs OpenCV and cannot be built here; these
 * entries are bit-exact against a sequential restatement written from the reference's source (tests/stage_ref.py), not
 * against the reference.  The fit between the walk and the update is the next block, "a stage's global regression".  Out
 * of scope: BoostCart::Train's loop (one step of it: the last block of this file), writing into a model file.
 *
 * Sizes.  nodes_n = 2^tree_depth and the landmark count L come from the cascador, as in the training block (it also
 * supplies the device, the LDS budget "lbf_lds_kb" and the "workspace_mb" limit of the per-call workspace: the samples are
 * processed in chunks that fit it; device-resident patches are read in place); leafNum = nodes_n/2; origin_size /
 * half_size / quarter_size are call arguments, each in [1, 128].
 *
 * Patches.  GenLBF resizes the sample's image to the half and the quarter size itself (btcart.cpp:397-398): for a set built
 * by the resize_mode-0 chain (data.cpp:987-990, o -> h, o -> q) those are the h / q bytes the set already stores, the layout
 * of jdaSamplesCpp.patches.  The entries READ THE STORED PATCHES and resize nothing.
 *
 * Similarity transform.  With jdaSetSimilarityTransform(1) the two device entries refuse (-1) unless the caller opted in with
 * the option "train_similarity" (the training block, "Similarity transform"): the training entries refuse too, so a sample
 * set for them cannot exist.  Without the transform the split node is evaluated with the identity STParameter and
 * GenDeltaShape's Apply is the identity.  With both, every sample runs under stp_mc = STParameter::Calc(its shape,
 * mean_shape) (btcart.cpp:399): the walk applies it to both offsets of every split node, and out_shapes = shapes +
 * stp_mc.Apply(delta) (btcart.cpp:422) -- also when lbf_in is given and nothing is walked.
 *
 * Refused with -1 and jdaGetLastError(), never a crash: NULL where data is needed, K <= 0, a scale outside 0..2, a landmark
 * id outside [0, L), a patch size outside [1, 128], an lbf_in entry outside its cart's leaves.  n == 0 returns 0 without
 * touching the device. */

typedef struct {
  const jdaFeatureCpp *features;   /* K * (nodes_n/2 - 1): node i = 1 .. nodes_n/2 - 1 of cart k at [k*(nodes_n/2-1) + i-1]
                                      -- K times jdaTrainCartCpp's out_features                                        */
  const int *thresholds;           /* same layout, K times out_thresholds                                              */
  int K;
} jdaStageCartsCpp;

typedef struct {
  double call_ms;            /* wall clock of the call                                                              */
  double upload_ms;          /* ... carts, weights and the chunks' shapes (and host patches) to the device          */
  double device_ms;          /* ... the k_lbf launches, HIP events, summed over the chunks                           */
  double download_ms;        /* ... shapes and leaf indicators back to the host                                      */
  int chunks;                /* chunks the samples were cut into ("workspace_mb")                                   */
  int lds_path;              /* 1: a sample's patches, shape and indicators staged in LDS; 0: read from global memory */
  int waves_per_group;       /* samples (waves) per workgroup                                                       */
  int lds_bytes;             /* LDS of a workgroup                                                                  */
} jdaStageStatsCpp;

/* BoostCart::GenLBF over the set: lbf[i*K + k] = k*leafNum + Cart::Forward(cart k, sample i) (cart.cpp:392-404: from node 1,
 * value <= threshold goes to 2*node, else 2*node + 1, depth - 1 times; the result is node - leafNum).  lbf is the ZERO-based
 * liblinear index: X[i][k].index = lbf[i*K + k] + 1 (btcart.cpp:341).  samples->weights and residual are not read and may
 * be NULL.  A cascador of tree_depth 1 has no split node: every entry is k, features / thresholds may be NULL. */
JDA_API int jdaGenLbfCpp(void *cascador, const jdaSamplesCpp *samples, int origin_size, int half_size, int quarter_size,
                         const jdaStageCartsCpp *carts, int *lbf);

/* The shape update of btcart.cpp:285-292.  w is K*leafNum rows of 2L doubles on the host, row-major: BoostCart::w, as the
 * model file stores a stage's weights.  Per sample, delta[j] starts at 0. and adds w[lbf[k]][j] for k = 0 .. K-1 IN CART
 * ORDER (btcart.cpp:414-420; the order decides bits); then out_shapes[i*2L + j] = shapes[i*2L + j] + delta[j].
 * lbf_in == NULL: the entry walks the carts itself, walk and sums in ONE device pass.  Otherwise it uses the given
 * indices, each checked against 0 <= lbf_in[i*K + k] - k*leafNum < leafNum, and `carts` may be NULL (K is then the cascador's K) or
 * carry NULL arrays (only its K is read).  out_lbf (n*K ints) may be
 * NULL; so may stats.  out_shapes (n * 2L doubles) must not be NULL and MAY ALIAS NOTHING: not samples->shapes, not w. */
JDA_API int jdaStageUpdateShapesCpp(void *cascador, const jdaSamplesCpp *samples, int origin_size, int half_size,
                                    int quarter_size, const jdaStageCartsCpp *carts, const double *w, const int *lbf_in,
                                    double *out_shapes, int *out_lbf, jdaStageStatsCpp *stats);

/* Host only (no GPU, no cascador): calcMeanError (common.cpp:41-77) over n samples of L landmarks, IN ITS OWN ORDER:
 *   per sample i, in order:  left_x, left_y = the gt coordinates of the n_left left-pupil landmarks summed from 0. in list
 *     order, each then divided by (double)n_left; right_x, right_y the same over the right pupils;
 *     pupil_dis = sqrt(dx*dx + dy*dy) with dx = left_x - right_x, dy = left_y - right_y;
 *     e_ = 0., + sqrt(ex*ex + ey*ey) for landmark j = 0 .. L-1 in order, (ex, ey) = gt - current of landmark j;
 *     e += e_ / pupil_dis  (e from 0.);
 *   *out = e / (double)(L * n).
 * The reference writes the squares as std::pow(v, 2): DEFINED here as v * v, what the C library returns for an exponent
 * of exactly 2 and what compilers fold it into -- a detail only the reference's build decides, unchecked like cv::mean.
 * n == 0 gives 0. / 0. = NaN, like the reference.  -1: NULL arguments, n < 0, L < 1, an empty pupil list, an id outside [0, L). */
JDA_API int jdaMeanErrorCpp(const double *gt_shapes, const double *cur_shapes, int n, int L, const int *left_pupils,
                            int n_left, const int *right_pupils, int n_right, double *out);

/* ---- Dialect CPP: a stage's global regression ---------------------------------------------------------------------------
 * BoostCart::GlobalRegression (reference src/jda/btcart.cpp:328-388): the leaf indicators jdaGenLbfCpp writes and the
 * residuals jdaShapeResidualCpp writes go in, the weight matrix w that jdaStageUpdateShapesCpp consumes comes out -- 2L
 * independent regressions, one per shape coordinate, each of them epochs of dual coordinate descent over every used sample.
 * The reference hands each to liblinear (L2R_L2LOSS_SVR_DUAL, p = 0, bias = -1).  Its solver shuffles with rand() and the
 * reference calls it from an OpenMP loop (btcart.cpp:367), so the draws of different landmarks interleave differently on
 * every run: no run of the reference is reproducible against another, and nothing here could be bit-faithful to one.  THE
 * FIT IS THEREFORE DEFINED HERE, to the bit, on the counter-based generator of the mining block above.
 *
 * Arguments.  lbf: n * K ints as jdaGenLbfCpp writes them (zero-based, k * leafNum + leaf).  residual: n * 2L doubles,
 * row-major, as jdaShapeResidualCpp writes them.  rows: the reference's valid_pos_idx (btcart.cpp:273-281), n_rows indices
 * into both arrays in the order the samples enter the problem; a row named twice is two samples; NULL: all n rows in order
 * (n_rows is then not read).  L and leafNum = 2^(tree_depth - 1) come from the cascador, which also supplies the device,
 * "workspace_mb", the options "fit_lds_kb" / "fit_ahead" and the error state; no model table is read, so
 * jdaSetSimilarityTransform does not matter (as for jdaGatherSamplesCpp).  w: K * leafNum rows of 2L doubles, row-major --
 * exactly what jdaStageUpdateShapesCpp takes.  out_iters (2L ints: epochs run per coordinate), out_gnorm1 ([2][2L]:
 * Gnorm1_init, then the last Gnorm1_new), stats and params (NULL: every default, seed 0) may be NULL.
 *
 * The fit of coordinate j.  y[s] = residual[row(s)][j], x_s = the K ones at lbf[row(s)][.], lambda = 0.5 / C,
 * H = (double)K + lambda (QD is K times 1.*1.); every operation an IEEE double operation, no contraction:
 *     beta[s] = 0., w_j[:] = 0., index[s] = s                                  (s = 0 .. n_rows-1)
 *     for iter = 0, 1, ... < max_iter:
 *         jdaFitShuffleCpp(index, n_rows, seed, iter)       -- continues from the array the previous epoch left
 *         Gnorm1 = 0.
 *         for s = 0 .. n_rows-1:  i = index[s]
 *             G = -y[i] + lambda*beta[i];   G = G + dot(i)
 *             violation = beta[i] == 0 ? (G < 0 ? -G : G > 0 ? G : 0.) : fabs(G);   Gnorm1 += violation
 *             d = G < H*beta[i] ? -G/H : G > H*beta[i] ? -G/H : -beta[i]
 *             if fabs(d) < 1.0e-12: continue
 *             old = beta[i]; beta[i] = old + d; d = beta[i] - old;  if d != 0: w_j[lbf[i][k]] += d  for every k
 *         if iter == 0: Gnorm1_init = Gnorm1
 *         if Gnorm1 <= eps*Gnorm1_init: stop (iters = iter + 1)
 * dot(i): 64 partial sums p[c], c = 0 .. 63, each from 0. adding w_j[lbf[i][k]] for k = c, c + 64, .. ascending; then for
 * h = 32, 16, 8, 4, 2, 1: p[c] += p[c + h] for c < h; dot = p[0].
 * jdaFitShuffleCpp: for s = 0 .. n-1: t = s + r(iter, s) % (n - s), swap index[s] and index[t], with
 *     r(iter, s) = splitmix64(splitmix64(seed + (iter + 1) * G) + (s + 1) * G)        (G, splitmix64: the mining block)
 *
 * (a) Origin.  The body is solve_l2r_l1l2_svr for L2R_L2LOSS_SVR_DUAL with p = 0 and bias = -1 AS REMEMBERED from liblinear
 *     2.x: the library's source is not in the reference tree (its submodule is empty), so this is UNCHECKED, like cv::resize.
 *     It is reached through train()'s regression branch, which calls the solver once on the problem as given;
 *     get_decfun_coef(model, j + 1, 0) is w[j].
 * (b) Shrinking.  liblinear's shrinking branch is unreachable at p = 0: it needs G + p > Gmax_old and G - p < -Gmax_old at
 *     once with Gmax_old >= 0.  active_size therefore never changes and the branch is omitted.
 * (c) Deliberate differences.  The shuffle's draws.  ONE index array shared by all 2L coordinates (in the reference every
 *     problem draws its own from the raced rand()).  The shape of dot: liblinear adds the K terms one after the other; since
 *     nothing can reproduce liblinear's result anyway that order protects no parity, and it would cost K dependent fp64 adds
 *     per sample.
 * (d) PARITY UNPINNED like every dialect-CPP entry: bit-exact against a sequential restatement of the text above
 *     (tests/fit_ref.py), which is also checked against the closed-form primal solution; not against the reference.
 *
 * Refused with -1 and jdaGetLastError() before the device is touched: NULL where data is needed, K <= 0, negative n or
 * n_rows, a rows entry outside [0, n), an lbf entry of a used row outside its cart's leaves
 * (0 <= lbf - k*leafNum < leafNum), a non-finite residual in a used row, NULL w, n_rows above 2^30.  n_rows == 0: w zeroed,
 * iters 0, returns 0 without touching the device.  A problem whose device arrays -- the used rows of lbf (n_rows * K ints),
 * y and beta (2 * 2L * n_rows doubles), the weights (2L * K * leafNum doubles) and fit_ahead + 1 orders (n_rows ints each) --
 * do not fit "workspace_mb" is refused with that reason: the fit is one serial pass per epoch, chunks would buy nothing.
 * Out of scope: BoostCart::Train's loop and restarts, writing w into a model file, L1-loss or p != 0 solvers, a bias term,
 * any attempt to match a particular liblinear run. */

typedef struct {
  double C;        /* <= 0: 1. / n_rows (btcart.cpp:363) */
  double eps;      /* <= 0: 0.0001 (btcart.cpp:365)      */
  int max_iter;    /* <= 0: 1000 (liblinear's)           */
  uint64_t seed;
} jdaFitParamsCpp;

typedef struct {
  double call_ms;            /* wall clock of the call                                                              */
  double shuffle_ms;         /* ... the host's shuffles, summed over the epochs                                     */
  double upload_ms;          /* ... lbf, residuals and the epochs' orders to the device                             */
  double device_ms;          /* ... the k_fit launches, HIP events, summed                                          */
  int epochs_launched;       /* launches queued (>= the largest iters: "fit_ahead" queues past a stop, as no-ops)   */
  int lds_path;              /* 1: a coordinate's column of w in LDS; 0: in global memory ("fit_lds_kb")            */
  int lds_bytes;             /* LDS of a workgroup                                                                  */
} jdaFitStatsCpp;

JDA_API int jdaGlobalRegressionCpp(void *cascador, const int *lbf, const double *residual, int n, int K,
                                   const int *rows, int n_rows, const jdaFitParamsCpp *params,
                                   double *w, int *out_iters, double *out_gnorm1, jdaFitStatsCpp *stats);
/* Host only (no cascador, no GPU): one epoch's shuffle of index[0 .. n) as specified above.  -1: n < 0, iter < 0, NULL. */
JDA_API int jdaFitShuffleCpp(int *index, int n, uint64_t seed, int iter);

/* ---- Dialect CPP: from one cart to the next ---------------------------------------------------------------------------
 * What BoostCart::Train does between two carts (reference src/jda/btcart.cpp:146-253 with src/jda/data.cpp:255-448): the new
 * cart's leaf scores are added to every sample (DataSet::UpdateScores), optionally normalised (CalcMeanAndStd /
 * ApplyMeanAndStd), both sets are sorted by score with the reference's own quicksort (_QSort_), the cart's threshold is the
 * score of the drop_n-th positive from the end (CalcThresholdByNumber), both sets are cut at it (PreRemove / Remove), mined
 * negatives are appended (MoreNegSamples) and the weights recomputed (UpdateWeights).  Every sum of the next cart runs in
 * the sample order this leaves, and the quicksort is NOT stable: a caller who sorts with anything else trains other carts.
 * The reference's Swap exchanges cv::Mat headers; here a set is a dense patch array in device memory that k_train_values
 * and k_lbf read in place, so the surviving samples' bytes move, on the device, into the new order
 * (jdaGatherSamplesCpp).  These entries are ONE STEP of the loop as arithmetic on caller arrays.  PARITY UNPINNED like
 * every dialect-CPP entry: bit-exact against a sequential restatement written from the reference's source
 * (tests/boost_ref.py), not against the reference.  Out of scope: the loop itself and the restart decision
 * (btcart.cpp:189-232: the caller compares will_removed with its own policy and, to restart, copies `last` back --
 * ResetScores), the call into mining (the caller invokes jdaMineNegativesCpp* and passes the result as a segment),
 * CalcSTParameters (with "train_similarity" every entry derives the parameters from the shapes it is given;
 * jdaCalcSTParametersCpp returns them), snapshots, writing carts or weights into a
 * model, liblinear.
 *
 * All of it is fp64 in the reference's own order.  The host entries take no cascador, use no GPU and never crash: bad
 * input returns -1 and sets jdaGetLastError().  exp() and sqrt() are the HOST C library's: the weights stay on the host for
 * the reason log() does in the training block -- the device's exp is another function. */

/* DataSet::UpdateScores (data.cpp:305-317) for both sets, then -- normalize != 0 -- CalcMeanAndStd and ApplyMeanAndStd
 * (data.cpp:420-448), literally:
 *   for every positive i in order, then every negative i in order:  last[i] = score[i];  score[i] += cart_scores[leaf[i]];
 *   normalize == 0:  *mean = 0., *stddev = 1., the scores stay as they are.  Otherwise
 *   m = 0., + every positive score in order, then + every negative score in order;  m /= (double)(pos_n + neg_n);
 *   var = 0., + v * v with v = score - m, over the positives in order, then the negatives in order;
 *   var /= (double)(pos_n + neg_n);  *stddev = sqrt(var);  *mean = m;  every score = (score - m) / *stddev.
 * The reference writes the square as std::pow(v, 2): DEFINED as v * v, as jdaMeanErrorCpp defines it (what the C library
 * returns for an exponent of exactly 2 and what compilers fold it into; unchecked).  THE SUMS RUN OVER THE ORDER THE ARRAYS
 * HAVE AT THE CALL, that is before the sort.  leaf is jdaTrainCartCpp's pos_leaf / neg_leaf, cart_scores its out_scores of
 * leaf_n = nodes_n/2 entries; every leaf index is checked against [0, leaf_n) before anything is written.  pos_scores /
 * neg_scores are updated in place; pos_last / neg_last receive the scores from before the call.  *stddev == 0 (all scores
 * equal) gives inf / NaN scores like the reference and the call succeeds; so does an empty pair of sets (0. / 0.).  mean /
 * stddev may be NULL.  -1: NULL where n > 0, a negative count, leaf_n < 1, a leaf index outside [0, leaf_n). */
JDA_API int jdaBoostScoresCpp(const double *cart_scores, int leaf_n, const int *pos_leaf, int pos_n, const int *neg_leaf,
                              int neg_n, int normalize, double *pos_scores, double *neg_scores, double *pos_last,
                              double *neg_last, double *mean, double *stddev);

/* DataSet::_QSort_ (data.cpp:385-410) on one set's scores together with an index array, literally: for a range
 * [left, right], i = left, j = right, t = scores[(left + right) / 2] (the pivot VALUE, read before any swap);
 *   do { while (scores[i] > t) i++;  while (scores[j] < t) j--;  if (i <= j) { swap i and j;  i++;  j--; } } while (i <= j);
 * then [left, j] if left < j and [i, right] if i < right.  The two halves are disjoint, so an explicit stack (no recursion,
 * depth O(log n)) gives the reference's result.  order[i] = the original index of the sample now at position i (descending
 * scores); sorted_scores (may be NULL) = scores[order[i]].  The sort is NOT stable: [3, 2, 2, 1] gives order 0 2 1 3, eight
 * equal scores give 5 4 7 6 1 0 3 2; without ties the result equals a descending stable sort.  `scores` itself is not
 * changed.  n == 0 returns 0 and reads nothing (the reference would read scores[0]).  -1: any NaN score (the reference's
 * scans would run off the array), NULL, n < 0.  +-inf are ordinary values. */
JDA_API int jdaSampleOrderCpp(const double *scores, int n, int *order, double *sorted_scores);

/* DataSet::CalcThresholdByNumber (data.cpp:340-345) on scores ALREADY SORTED by jdaSampleOrderCpp: offset = n - 1 - drop_n,
 * clamped to 0 from below; *th = sorted_scores[offset].  -1: n < 1, drop_n < 0, NULL. */
JDA_API int jdaScoreThresholdCpp(const double *sorted_scores, int n, int drop_n, double *th);

/* DataSet::PreRemove / Remove (data.cpp:347-378) on sorted scores: offset = n - 1; while (offset >= 0 &&
 * sorted_scores[offset] < th) offset--;  *keep = offset + 1 (the leading samples that stay: ties at th stay),
 * *will_removed = n - *keep (either may be NULL).  n == 0 gives 0 / 0.  The restart decision on will_removed is the
 * caller's.  -1: a NaN th, n < 0, NULL scores where n > 0. */
JDA_API int jdaScoreCutCpp(const double *sorted_scores, int n, double th, int *keep, int *will_removed);

/* DataSet::UpdateWeights(pos, neg) (data.cpp:255-303): w = exp(-score) for every positive, exp(score) for every negative
 * (the host C library's exp); sum_pos = 0. + the positive weights in order, sum_neg = 0. + the negative weights in order;
 * r = 1. / (sum_pos + sum_neg); every weight *= r.  Two empty sets: nothing is written.  -1: NULL where n > 0, n < 0. */
JDA_API int jdaUpdateWeightsCpp(const double *pos_scores, int pos_n, const double *neg_scores, int neg_n,
                                double *pos_weights, double *neg_weights);

/* Host only: the per-sample rows that travel with the patches (shapes, ground truth, masks, scores, last) by the same
 * index list.  The source is the concatenation of n_segs (1 .. 8) host arrays, rows[s] holding rows_n[s] rows of
 * row_bytes; dst row i = source row index[i] for i < keep: a memcpy per row.  Every index is checked against the total
 * before anything is written; repeats are allowed.  dst must not overlap a source (refused).  keep == 0 returns 0. */
JDA_API int jdaGatherRowsCpp(const void *const *rows, const int *rows_n, int n_segs, size_t row_bytes, const int *index,
                             int keep, void *dst);

typedef struct {
  const unsigned char *patches;  /* n records of P = o*o + h*h + q*q bytes, jdaSamplesCpp.patches' layout; any alignment */
  int on_device;                 /* 0: host pointer (staged in chunks within "workspace_mb"), 1: device pointer (read in place) */
  int n;                         /* records; 0: an empty segment, patches is not read                                       */
} jdaGatherSegCpp;

typedef struct {
  double call_ms;            /* wall clock of the call                                                          */
  double upload_ms;          /* ... the index list and the chunks of host segments to the device                */
  double device_ms;          /* ... the k_gather launches, HIP events, summed                                   */
  double download_ms;        /* ... a host dst: the gathered records back                                       */
  long long bytes;           /* keep * P: the bytes written to dst                                              */
  int chunks;                /* chunks of host segments (or, for a host dst, of dst) that went through the workspace */
  int launches;              /* k_gather launches                                                               */
} jdaGatherStatsCpp;

/* A new dense sample set from up to 8 segments: with the source set = the concatenation of segs[0 .. n_segs), dst record i
 * = source record index[i] for i < keep, P = o*o + h*h + q*q bytes each (every size in [1, 128]: P = 3 .. 49,152).  One call
 * is "sort and cut" (one segment, index = jdaSampleOrderCpp's order, keep = jdaScoreCutCpp's), "append mined negatives"
 * (two segments, an identity index) or "append, then sort" (two segments, the order of the concatenated scores:
 * MoreNegSamples followed by QSort).  Device segments are read in place, host segments staged in chunks within the
 * cascador's "workspace_mb"; dst is the caller's buffer of keep * P bytes, on the device (dst_on_device = 1) or on the host
 * (then device records come back in chunks and host records are copied by the host).  No byte outside
 * [dst, dst + keep * P) is written, whatever the alignment of dst and of the segments (none is required).  dst MUST NOT
 * OVERLAP A SOURCE: a device dst that overlaps a device segment (or a host dst a host segment) is refused; callers
 * alternate between two buffers.  index is validated entry by entry against the total number of records before anything
 * is launched; repeats are allowed.  keep == 0 returns 0 without touching the device.  The cascador supplies the device,
 * the workspace limit and the error state only -- no model is read, so the entry works with jdaSetSimilarityTransform on or
 * off.  -1: NULL where data is needed, n_segs outside [1, 8], a negative n, more than INT_MAX records in all, a size outside
 * [1, 128], an index outside [0, total), an overlap. */
JDA_API int jdaGatherSamplesCpp(void *cascador, const jdaGatherSegCpp *segs, int n_segs, int origin_size, int half_size,
                                int quarter_size, const int *index, int keep, unsigned char *dst, int dst_on_device,
                                jdaGatherStatsCpp *stats);

/* ---- Dialect CPP: the positive sample set -----------------------------------------------------------------------------
 * What DataSet::LoadPositiveDataSet (reference src/jda/data.cpp:567-678) does once the images are decoded: getFace
 * (data.cpp:542-565) cuts every face box out of its image, three cv::resize calls make the o, h and q patches
 * (data.cpp:630-632), the landmarks are normalised to the box (625-628), face_augment_on adds the mirrored copy of every
 * sample (637-662), CalcMeanShape (210-223) and RandomShapes (237-253) give the mean and the initial shapes; later
 * CalcShapeResidual (175-208) is what jdaSamplesCpp.residual asks for.  The outputs are jdaSamplesCpp's layout: they go
 * into the training entries as they are.  PARITY UNPINNED like every dialect-CPP entry: src/jda needs OpenCV and cannot be
 * built here; these entries are bit-exact against a restatement written from the reference's source
 * (tests/positives_ref.py), not against the reference.  Out of scope: reading the list file and decoding images (the
 * caller hands in 8-bit grey images; jdaPackGray[Device], "frames as they arrive", makes them from decoded colour images),
 * liblinear's fit and the training loop.
 *
 * The face.  getFace(image, bbox) is a w x h crop of the cols x rows image in which every pixel outside the image is 0.
 * The reference takes its clone-the-crop path only when bbox.x >= 0, bbox.y >= 0, bbox.x + w < cols and bbox.y + h < rows
 * -- A STRICT TEST: a face with x + w == cols goes through the padded canvas although it lies inside the image.  The bytes
 * are the same either way, and here both are one path (a pixel is read from the image, or is 0).  The padded canvas is
 * 3 cols x 3 rows with the image at (cols / 2, rows / 2) (integer halves); a box that leaves THE CANVAS makes OpenCV throw,
 * and the entries refuse it: -1 when  x + cols/2 < 0,  y + rows/2 < 0,  x + cols/2 + w > 3 cols  or  y + rows/2 + h > 3 rows,
 * and when w <= 0 or h <= 0.  Everything is validated before the device is touched and before a byte of dst is written.
 *
 * The three patches.  Each is cv::resize(INTER_LINEAR), as restated in this library (jdaResizeCv), OF THE FACE ITSELF:
 * face -> o, face -> h, face -> q.  This is not mining's chain (o -> h, o -> q, resize_mode 0); it is what resize_mode 1
 * computes for a crop inside its image.  The resize clamps to the face's w x h, not to the image; a box that is not square
 * is resized with separate x and y scales; a box of exactly twice a patch side takes OpenCV's 2x2 box average (zeros from
 * outside the image enter it) and a box of the patch's size is copied.
 *
 * Augmentation.  With augment = 1 the set has size = 2 n_faces records and record i + n_faces is cv::flip(patch, 1) of
 * record i's RESIZED o, h and q patches (data.cpp:638-640): the horizontal mirror of the bytes, NOT a resize of the
 * mirrored face (the two differ where the resize is not symmetric under the mirror).
 *
 * Images use jdaValidateCpp's conventions: host images of widths[i]*heights[i] bytes, rows back to back, or
 * (jdaBuildPositivesCppDevice) resident ones at d_base + offsets[i].  faces: n_faces rows of 5 ints (image, x, y, w, h).
 * dst receives size records of P = o*o + h*h + q*q bytes (any alignment, P may be odd), on the device (dst_on_device = 1,
 * written in place) or on the host (the records come back through the workspace in chunks): jdaGatherSamplesCpp's
 * convention for its dst.  Host images are uploaded in chunks that fit the cascador's "workspace_mb" (a chunk holds at
 * least one image); an image no face references is not uploaded.  A device dst must not overlap a referenced resident image
 * (refused).  The cascador supplies the device, the workspace limit and the error state only -- no model is read, so the
 * entries work with jdaSetSimilarityTransform on or off.  n_faces == 0 returns 0 without touching the device.
 * -1 with jdaGetLastError(): NULL where data is needed, a patch size outside [1, 128], augment outside {0, 1}, an image index
 * outside [0, n_images), an empty or NULL referenced image, more than INT_MAX records, the box refusals above, an overlap. */

typedef struct {
  double call_ms;            /* wall clock of the call                                                          */
  double upload_ms;          /* ... the face rows and the chunks of host images to the device                   */
  double device_ms;          /* ... the k_faces launches, HIP events, summed                                    */
  double download_ms;        /* ... a host dst: the records back                                                */
  long long bytes;           /* size * P: the bytes written to dst                                              */
  int image_chunks;          /* chunks the referenced host images were uploaded in (0: images resident)         */
  int images_uploaded;       /* host images uploaded: the referenced ones                                       */
  int chunks;                /* batches of faces that went through the workspace                                */
  int launches;              /* k_faces launches                                                                */
} jdaPositivesStatsCpp;

JDA_API int jdaBuildPositivesCpp(void *cascador, const unsigned char *const *images, const int *widths, const int *heights,
                                 int n_images, const int *faces, int n_faces, int origin_size, int half_size,
                                 int quarter_size, int augment, unsigned char *dst, int dst_on_device,
                                 jdaPositivesStatsCpp *stats);
JDA_API int jdaBuildPositivesCppDevice(void *cascador, const unsigned char *d_base, const size_t *offsets, const int *widths,
                                       const int *heights, int n_images, const int *faces, int n_faces, int origin_size,
                                       int half_size, int quarter_size, int augment, unsigned char *dst, int dst_on_device,
                                       jdaPositivesStatsCpp *stats);

/* Host only (no GPU, no cascador): ground-truth shapes, masks and the mean shape, literally data.cpp:589-598, 625-628,
 * 641-661 and CalcMeanShape (210-223).  faces: the n_faces rows given to jdaBuildPositivesCpp (x, y, w, h are read);
 * landmarks: n_faces * 2L doubles in image coordinates (x0, y0, x1, y1, ...).  With size = augment ? 2 n_faces : n_faces:
 *   shape_mask[i] = -1 when ALL 2L raw values are negative (`>= 0` fails for every one: a NaN counts as negative), else 1;
 *     such shapes are still normalised and mirrored like the others;
 *   gt_shapes[i][2j] = (v - x) / w,  gt_shapes[i][2j + 1] = (v - y) / h   (x, y, w, h converted to double);
 *   augment: gt_shapes[i + n] = gt_shapes[i] with every x replaced by 1 - x, then the pairs (left[j], right[j]),
 *     j = 0 .. sym_n - 1, swapped SEQUENTIALLY IN LIST ORDER -- a landmark named in two pairs is swapped twice;
 *     shape_mask[i + n] = shape_mask[i];
 *   mean_shape = gt_shapes[0] WHATEVER ITS MASK, + gt_shapes[i] for i = 1 .. size - 1 with shape_mask[i] > 0 in order,
 *     valid_n = the number of those (sample 0 is summed but NOT counted: the reference's quirk, kept); then
 *     mean_shape[j] = mean_shape[j] * (1. / (double)valid_n) + 0.  -- `Mat /= double` in the multiply-by-reciprocal form it
 *     has everywhere in this library (a fourth OpenCV-decided detail, FROM MEMORY AND UNCHECKED).  valid_n == 0 follows from
 *     the same IEEE expression (inf and NaN) and the call succeeds.
 * Outputs: gt_shapes [size * 2L], shape_mask [size], mean_shape [2L].  -1: n_faces < 1 (CalcMeanShape reads sample 0),
 * L < 1, NULL, augment outside {0, 1}, w <= 0 or h <= 0, a pair id outside [0, L). */
JDA_API int jdaPositiveShapesCpp(const int *faces, const double *landmarks, int n_faces, int landmark_n, int augment,
                                 const int *left, const int *right, int sym_n, double *gt_shapes, int *shape_mask,
                                 double *mean_shape);

/* Host only: DataSet::RandomShapes (data.cpp:237-253) on the counter-based generator of the mining block: sample i has
 * key = first_key + i and draws x = g(2 key), y = g(2 key + 1); shapes[i][2j] = mean_shape[2j] + x,
 * shapes[i][2j + 1] = mean_shape[2j + 1] + y.  shift_size == 0 gives mean_shape + 0. and draws nothing.  A set built in
 * pieces (first_key = the number of samples before the piece) equals one built at once.  -1: NULL, n < 0, L < 1, a
 * shift_size that is negative or not finite. */
JDA_API int jdaRandomShapesCpp(const double *mean_shape, int landmark_n, int n, double shift_size, uint64_t seed,
                               uint64_t first_key, double *shapes);

/* Host only: both DataSet::CalcShapeResidual overloads (data.cpp:175-208) with the identity STParameter (the similarity
 * transform: jdaShapeResidualStCpp below): over the index list idx[0 .. n) into sets of `size` samples,
 *   landmark_id == -1:  residual[i][j] = gt_shapes[idx[i]][j] - cur_shapes[idx[i]][j], j < 2L       (n * 2L doubles)
 *   landmark_id >= 0:   residual[i] = the (x, y) of that landmark only                             (n * 2 doubles:
 *                       what jdaSamplesCpp.residual takes)
 * and has_gt[i] = shape_mask[idx[i]] > 0 (DataSet::HasGtShape; jdaSamplesCpp.has_gt).  residual or has_gt may be NULL
 * (shape_mask may be NULL when has_gt is).  -1: NULL where data is needed, an index outside [0, size), a landmark_id
 * outside [-1, L). */
JDA_API int jdaShapeResidualCpp(const double *gt_shapes, const double *cur_shapes, const int *shape_mask, int size,
                                int landmark_n, const int *idx, int n, int landmark_id, double *residual,
                                unsigned char *has_gt);

/* Host only: jdaShapeResidualCpp under the similarity transform.  stp_cm: `size` rows of five doubles (scale, rot00, rot01,
 * rot10, rot11), jdaCalcSTParametersCpp's stp_cm of the set's current shapes; row idx[i] is applied to sample i's residual as
 * data.cpp:185 (every landmark's (x, y)) and data.cpp:203 (the one landmark) do: Apply (data.hpp:42-45) is
 * x2 = scale * (rot00 * x + rot01 * y), y2 = scale * (rot10 * x + rot11 * y).  stp_cm == NULL gives jdaShapeResidualCpp's
 * bits.  Refusals as jdaShapeResidualCpp's. */
JDA_API int jdaShapeResidualStCpp(const double *gt_shapes, const double *cur_shapes, const int *shape_mask, int size,
                                  int landmark_n, const int *idx, int n, int landmark_id, const double *stp_cm,
                                  double *residual, unsigned char *has_gt);

/* ---- Dialect CPP: the model in training ----------------------------------------------------------------------------------
 * The model the pieces above train, held by the cascador and grown IN PLACE: JoinCascador's status (current_stage_idx,
 * current_cart_idx: reference src/jda/cascador.cpp:17-29, header ints 5 and 6 of the trainer's file), the carts
 * BoostCart::Train appends one by one or trains again (btcart.cpp:146-253), the weights that close a stage
 * (btcart.cpp:255-292) and JoinCascador::SerializeTo's f64 file (cascador.cpp:79-124).  The loop stays the caller's: mine
 * (jdaMineNegativesCpp*: Validate under the model AS IT STANDS), train (jdaTrainCartCpp), boost (jdaBoostScoresCpp ..),
 * PUT; per stage: indicators (jdaGenLbfCpp), fit (jdaGlobalRegressionCpp), CLOSE, serialize.  PARITY UNPINNED like every
 * dialect-CPP entry: the writer is checked against the layout restated in Python (jda_amd/synth.py), not against a file the
 * reference wrote.
 *
 * THE INVARIANT.  After any sequence of these calls the cascador behaves in every entry of this header -- detect in both
 * dialects, validate, mining, the training and stage entries, jdaCascadorInfo (multi_scale), work counters included --
 * exactly as a cascador created from the file jdaCascadorSerializeToCpp would write at that moment.  At status (s, K - 1),
 * where that entry refuses, the comparison file is the same content with header (s, K - 1), which the loader accepts.
 *
 * A training cascador starts as the reference's constructors leave a model: status (0, -1); in every cart every split node
 * Feature() (scale 0, both landmark ids 0, offsets 0.: common.hpp:76-81) with threshold 0, every leaf score 0., mean 0., std 1.
 * (cart.cpp:23-37); every w 0. (btcart.cpp:104-116).  Cart::th is left UNINITIALISED by the reference and is 0. here.
 *
 * Node order of jdaModelPutCartCpp: with nodes_n = 2^tree_depth, features[i - 1] / thresholds[i - 1] are node i = 1 ..
 * nodes_n/2 - 1 of Cart::features (the root is 1, the children of i are 2i and 2i + 1) and leaf_scores[j] is Cart::scores[j],
 * j = 0 .. nodes_n/2 - 1: jdaTrainCartCpp's out_features / out_thresholds / out_scores as they are, and the order
 * Cart::SerializeTo writes them in (cart.cpp:429-450), followed by th, mean, std.
 *
 * The four mutating entries also work on a cascador loaded from a trainer (f64) snapshot -- that is resuming -- and refuse one
 * read from an f32 file.  Like jdaSetOption they refuse while a call runs or a submitted batch is pending on the cascador;
 * starting a call on another thread while one of them runs is the caller's error.  Every refusal returns -1 with
 * jdaGetLastError() and leaves model and status untouched. */

/* A cascador on JoinCascador::JoinCascador()'s model, status (stage 0, cart -1); mean_shape: 2 * landmark_n doubles.  The
 * dimension limits are the loader's (T in [1, 16], K in [1, 2^20], landmark_n in [1, 4096], tree_depth in [2, 12]).  NULL with
 * jdaGetLastError() otherwise.  Released with jdaCascadorRelease. */
JDA_API void *jdaCascadorCreateTrainingCpp(int T, int K, int landmark_n, int tree_depth, const double *mean_shape);

/* The status: (s, c) with s < T = carts [0, c] of stage s are written and stages [0, s) closed; (T, -1) = complete (a float file
 * reports the (T + 1, -1) it carries).  Either pointer may be NULL. */
JDA_API int jdaModelStatusCpp(void *cascador, int *stage, int *cart);

/* Writes cart k of the stage in training.  k == cart + 1 (< K) appends and moves the status to (stage, k); k == cart >= 0
 * replaces the last cart (the restart path, btcart.cpp:204-206) and leaves the status as it is.  Refused: any other k, a
 * complete model, a scale outside 0..2, a landmark id outside [0, landmark_n), a std that is 0 or not finite, NULL arrays. */
JDA_API int jdaModelPutCartCpp(void *cascador, int k, const jdaFeatureCpp *features, const int *thresholds,
                               const double *leaf_scores, double th, double mean, double std);

/* Closes the stage in training, which must hold all its carts (cart == K - 1): stores its K * leafNum rows of 2 * landmark_n
 * weights (row-major: jdaGlobalRegressionCpp's w) and moves the status to (stage + 1, -1); after stage T - 1 the model is
 * complete, (T, -1). */
JDA_API int jdaModelCloseStageCpp(void *cascador, const double *w);

/* JoinCascador::Validate (cascador.cpp:166-211) on every record of a RESIDENT sample set, under the model as it stands: what a
 * trainer resuming from a model snapshot without a data snapshot, a trainer admitting extra patches, and the check "the
 * model written is the model trained" need (the scores and shapes carried from cart to cart by jdaBoostScoresCpp /
 * jdaStageUpdateShapesCpp must equal what this returns).  The o, h and q patches are taken AS STORED (jdaSamplesCpp's layout,
 * host or device memory as in jdaGenLbfCpp); nothing is resized.  A trainer snapshot runs Validate's own loop bounds: stages
 * [0, s) in full, then carts [0, c] of stage s without its regression.  The initial shape of sample i is samples->shapes[i]:
 * a caller who wants Validate's own start passes mean_shape + 0., a trainer the jdaRandomShapesCpp shapes its positives
 * started from; weights, residual and has_gt are ignored.  Outputs are host arrays of n entries (shape: n * 2L doubles), any
 * may be NULL; shape is written for rejected samples too (the shape as it stood), as jdaValidateCpp does; carts_n is
 * Validate's n.  The samples go through the device in chunks within "workspace_mb".  Option "reval_form": 0 (default) a wave
 * per sample (k_reval: lane = cart, the score chain replayed in cart order, the first failing cart by ballot), 1 the
 * lane-per-sample walk of jdaValidateCpp over the same records; both return identical bits.  "reval_lds_kb": the LDS a
 * workgroup of form 0 may take (a sample's patches, shape and indicators; 0: global memory).  stats (may be NULL): as for
 * jdaStageUpdateShapesCpp.  Similarity transform: with jdaSetSimilarityTransform(1) and the option "train_similarity" (the
 * training block) every FULL stage starts with STParameter::Calc(shape as it stands, mean_shape) (cascador.cpp:180), applied to
 * the offsets of its walk and to its delta before the add; the partial stage of a snapshot walks with the stage before's
 * parameter, or STParameter's default when it is stage 0 (cascador.cpp:198-209), as jdaValidateCpp does; both forms return
 * identical bits.  Refused with -1: jdaSetSimilarityTransform(1) without that option (as the training entries), a patch size outside
 * [1, 128], NULL samples / patches / shapes with n > 0, a negative n.  n == 0 returns 0 without touching the device.
 * PARITY UNPINNED like every dialect-CPP entry: bit-exact against a sequential restatement (tests/model_ref.py). */
JDA_API int jdaValidateSamplesCpp(void *cascador, const jdaSamplesCpp *samples, int origin_size, int half_size,
                                  int quarter_size, unsigned char *is_face, double *score, int *carts_n, double *shape,
                                  jdaStageStatsCpp *stats);

/* JoinCascador::SerializeTo's f64 file with the status in its header.  Refused at (s, K - 1): the reference's writer would
 * turn that into (s + 1, -1), a regression that was never fit, and the reference never writes there (btcart.cpp:243).
 * jdaCascadorSerializeTo (the f32 file) is unchanged. */
JDA_API int jdaCascadorSerializeToCpp(void *cascador, const char *path);

/* ------------------------------------------------------------------------ */
/* Frames as they arrive                                                    */
/* ------------------------------------------------------------------------ */
/* Every entry above takes 8-bit gray, rows back to back.  None of the reference's callers has that in hand: src/live.cpp:32,
 * src/test.cpp:40 and 134 and src/jda/data.cpp:621 each hold a decoded BGR image and call cvtColor(..., CV_BGR2GRAY) just
 * before the line this library replaces; a hardware JPEG or video decoder leaves interleaved RGB / BGR(A) or a pitched luma
 * plane in device memory.  These two entries take such images -- any of the formats below, any row pitch, any rectangle --
 * and write the dense gray images the other entries take.  Decoding stays the caller's.
 *
 * Gray value.  gray = (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14 in integer arithmetic: OpenCV 2.4's 8-bit CV_BGR2GRAY
 * (0.114 / 0.587 / 0.299 in Q14, rounded to nearest), the version the reference is written against.  Later OpenCV SIMD
 * paths use a 15-bit form of the same weights, which differs in the last bit for some colours; THIS LIBRARY'S DEFINITION
 * IS THE 14-BIT ONE ABOVE, on the host and on the device, to the bit.  RGB formats swap the outer weights; alpha is
 * ignored (and never read); GRAY8 is a copy (it serves a pitch or a rectangle).
 *
 * Output layout.  Image i is written at dst + dst_offsets[i] as w * h bytes, rows back to back: exactly what
 * jdaDetectBatchRaggedDevice, jdaDetectBatchCppRaggedDevice, jdaValidateCppDevice, jdaMineNegativesCppDevice and
 * jdaBuildPositivesCppDevice take (d_base = dst, offsets = dst_offsets, widths / heights = the rectangles'), and with
 * dst_offsets[i] = i * frame_stride what jdaDetectBatchDevice, jdaDetectBatchSubmit and jdaValidateWindowsDevice take.
 * RESULTS OF A LATER DETECT CALL ARE IN THE RECTANGLE'S COORDINATES: add (x, y) to get back to the source image, or let
 * jdaOrientBack ("frames in any orientation" below) do it (jdaFaceChips, "faces as they leave", takes the rectangle with the
 * landmarks as they are).
 *
 * jdaPackGray needs no cascador and no GPU: a plain loop over host memory, what a jdaDetect caller with a cv::Mat of BGR
 * uses.  jdaPackGrayDevice makes ONE kernel launch for all n images, of whatever sizes and formats (k_pack.hip); the
 * cascador supplies the device, the error state and a lane, whose grow-only buffer holds the image table -- no model is
 * read.  It runs on hip_stream if given (a hipStream_t: the stream the caller produced the pixels on), otherwise on the
 * lane's own stream, and returns when d_dst is complete, like every entry without a ticket.  Re-entrant on one cascador
 * like the other entries.  stats (may be NULL): pixels written, bytes read (w * h * bytes per pixel) and written, kernel
 * launches (1), the kernel's time between two events and the call's wall time.
 *
 * Refused with -1, jdaGetLastError() naming the image index and the offending values, nothing launched and no byte of dst
 * written: a NULL pointer where one is needed (images, dst, dst_offsets, an image's data; the cascador), n < 0, an unknown
 * format, width / height / w / h below 1 (except w == h == 0: the whole image), a rectangle that leaves the image,
 * pitch < width * bytes per pixel, two destination images that overlap, a destination image that overlaps the bytes the
 * rectangle takes of any source row of any image.  n == 0 returns 0 and touches nothing. */
#define JDA_PIX_GRAY8  0   /* 1 byte per pixel: a copy (pitch / rectangle only); the Y plane of NV12 is this */
#define JDA_PIX_BGR24  1
#define JDA_PIX_RGB24  2
#define JDA_PIX_BGRA32 3   /* alpha ignored */
#define JDA_PIX_RGBA32 4   /* alpha ignored */

typedef struct {
  const unsigned char *data; /* pixel (0,0) of the SOURCE image: host memory for jdaPackGray, device for jdaPackGrayDevice */
  long long pitch;           /* bytes from one row to the next, >= width * bytes per pixel, any alignment */
  int width, height;         /* of the source image */
  int format;                /* JDA_PIX_* */
  int x, y, w, h;            /* rectangle to take; w == 0 && h == 0 means the whole image */
} jdaPixels;

typedef struct { long long pixels, bytes_in, bytes_out; int launches; double device_ms, call_ms; } jdaPackStats;

JDA_API int jdaPackGray(const jdaPixels *images, int n, unsigned char *dst, const size_t *dst_offsets);
JDA_API int jdaPackGrayDevice(void *cascador, const jdaPixels *images, int n, unsigned char *d_dst,
                              const size_t *dst_offsets, void *hip_stream, jdaPackStats *stats);

/* ------------------------------------------------------------------------ */
/* Frames in any orientation                                                */
/* ------------------------------------------------------------------------ */
/* The cascade finds upright faces; frames do not arrive upright.  A phone or camera stores the sensor's rows and says "rotate
 * 90 degrees to display" in a tag, a mirrored front camera delivers flipped frames, a video decoder leaves the rotation to
 * the consumer.  These entries are jdaPackGray[Device] with ONE more step -- every image is written turned by one of the
 * eight orientations -- and the way back: jdaOrientBack takes the boxes and landmarks a detect call found on the turned
 * images into the source images the caller holds.
 *
 * The orientation.  A code t in 0..7, EXACTLY the transforms[] code of jdaMineNegativesCpp (data.cpp:930-963), as three bits:
 *     t      0  1  2  3  4  5  6  7
 *     swap   .  x  .  x  .  x  .  x
 *     flipX  .  .  x  x  x  x  .  .
 *     flipY  .  x  x  .  .  x  x  .
 * For a source rectangle of w x h pixels the turned image is W' x H' with W' = swap ? h : w and H' = swap ? w : h
 * (jdaOrientSize), and its pixel (column u, row v) is the rectangle's pixel (x, y):
 *     (x, y) = swap ? (v, u) : (u, v)
 *     then x = w - 1 - x if flipX
 *     then y = h - 1 - y if flipY
 * In numpy, on the rectangle's gray image a (tests/mining_ref.py: transform; tests/turn_ref.py):
 *     0: a              1: rot90(a, -1)  (a quarter turn clockwise)     2: rot90(a, 2)     3: rot90(a, 1)  (counter-clockwise)
 *     4: fliplr(a)      5: rot90(a, 2).T (the anti-transpose)           6: flipud(a)       7: a.T
 * EXIF.  Turning the STORED image by t gives the image as it should be displayed, for the Orientation tag
 *     tag  1  2  3  4  5  6  7  8
 *     t    0  4  2  6  7  1  5  3
 * Orientations 4, 5, 6 and 7 mirror (the swap / flip matrix has determinant -1): a left eye becomes a right eye.
 *
 * jdaPackGrayOriented / jdaPackGrayOrientedDevice have the contract of jdaPackGray / jdaPackGrayDevice in every respect --
 * formats, pitch, rectangle, the Q14 gray value, the refusals, the overlap checks, the stream, the return on completion,
 * re-entrancy, stats with launches == 1 for n > 0 -- with one difference: image i is written turned by orients[i], as
 * W' * H' bytes (the same number as w * h: the overlap checks are those of jdaPackGray), rows of W' bytes back to back.  An
 * orients[i] outside 0..7 (and NULL orients with n > 0) is refused like an unknown format.  With every orientation 0 the
 * bytes are jdaPackGray[Device]'s.  The host form is plain loops over the definition; the device form makes ONE kernel launch
 * for all n images of whatever sizes, formats and orientations (k_turn.hip: 64 x 64 tiles through LDS) and, like k_pack,
 * never reads a byte outside the rectangle's pixels of a source row's dwords: a source that ends with its allocation is safe.
 *
 * jdaOrientBack (host only, in place).  Face f belongs to image face_image[f]; boxes (n_faces * box_ints ints: box_ints 3
 * (x, y, size) as jdaResult's, 4 (x, y, w, h) as jdaResultD's; may be NULL) and landmarks (n_faces * 2 * landmark_n reals of
 * real_bytes 4 or 8, (x, y) pairs in pixels; may be NULL) are in the coordinates of that image's TURNED rectangle -- what a
 * detect call on the turned image returned -- and on return in those of the WHOLE source image.  With (rx, ry, w, h) the
 * image's rectangle:
 *   boxes, integer exact:   (x0, y0, bw, bh) = swap ? (y, x, bh, bw) : (x, y, bw, bh)
 *                           x0 = w - bw - x0 if flipX      y0 = h - bh - y0 if flipY      then x0 += rx, y0 += ry
 *   landmarks, a pixel's centre being its integer index (how the cascade reads shape * size), in the type's own precision,
 *   one operation per line, no fused multiply-add:
 *                           swap the pair if swap
 *                           x = (real)(w - 1) - x if flipX      y = (real)(h - 1) - y if flipY
 *                           x = x + (real)rx                    y = y + (real)ry
 *   for the mirroring orientations 4, 5, 6, 7 additionally the landmark pairs (left[j], right[j]), j = 0 .. sym_n - 1, are
 *   exchanged SEQUENTIALLY IN LIST ORDER, exactly as jdaPositiveShapesCpp does -- a landmark named in two pairs is swapped
 *   twice; sym_n == 0 leaves the labels alone.  Scores are not touched.
 * Refused with -1, jdaGetLastError() naming the index, nothing written: NULL images, orients or face_image with n_faces > 0,
 * a negative count, box_ints other than 3 or 4 (with boxes), real_bytes other than 4 or 8 or landmark_n < 1 (with
 * landmarks), NULL left / right with sym_n > 0, a pair id outside [0, landmark_n), a face_image outside [0, n_images),
 * everything jdaPackGray refuses about an image, an orientation outside 0..7.  n_faces == 0 returns 0 and touches nothing. */
JDA_API int jdaOrientSize(int w, int h, int orient, int *tw, int *th);
JDA_API int jdaPackGrayOriented(const jdaPixels *images, const int *orients, int n, unsigned char *dst,
                                const size_t *dst_offsets);
JDA_API int jdaPackGrayOrientedDevice(void *cascador, const jdaPixels *images, const int *orients, int n,
                                      unsigned char *d_dst, const size_t *dst_offsets, void *hip_stream,
                                      jdaPackStats *stats);
JDA_API int jdaOrientBack(const jdaPixels *images, const int *orients, int n_images, const int *face_image, int n_faces,
                          int *boxes, int box_ints, void *landmarks, int real_bytes, int landmark_n, const int *left,
                          const int *right, int sym_n);

/* ------------------------------------------------------------------------ */
/* Frames larger than the faces need                                        */
/* ------------------------------------------------------------------------ */
/* A 1080p or 4K camera frame does not need scanning at full resolution to find faces of 100 pixels and more; every consumer
 * of a face detector halves or thirds such frames first.  These entries are jdaPackGrayOriented[Device] with ONE more step in
 * front of the turn -- every image is reduced by an integer factor, block means -- and the way back: jdaReduceBack takes the
 * boxes and landmarks a detect call found on the reduced, turned images into the source images the caller holds, so that
 * jdaFaceChips can cut the faces from the full-resolution frame.
 *
 * Definition, to the bit, on the host and on the device.  For image i with rectangle w x h, factor f = factors[i] in 1..8
 * and orientation t = orients[i] in 0..7 (orients == NULL: every t is 0):
 *   1. Gray.    Every source pixel becomes gray by the Q14 formula of "frames as they arrive" (GRAY8: a copy), ROUNDED PER
 *               PIXEL FIRST: reducing a colour image equals reducing its jdaPackGray image.
 *   2. Reduce.  rw = w / f, rh = h / f (integer division): the w % f rightmost columns and the h % f bottom rows are
 *               dropped.  Reduced pixel (i, j) = (S + f * f / 2) / (f * f) in integer arithmetic, S the sum of the f x f grays
 *               at columns [i f, i f + f) and rows [j f, j f + f): the mean, to nearest, halves up.  For f = 2 that is
 *               (S + 2) >> 2, the fast area path cv::resize takes at exactly 2x (what jdaResizeCv restates).
 *   3. Turn.    The rw x rh image is turned by t exactly as "frames in any orientation" defines, rw and rh in place of w and
 *               h, and written as W' x H' bytes, rows back to back, at dst + dst_offsets[i].  jdaReduceSize gives (W', H')
 *               = swap ? (h / f, w / f) : (w / f, h / f); it refuses NULL rw / rh, a factor outside 1..8, an orientation
 *               outside 0..7 and a negative w or h (a w or h below f gives 0).
 *
 * jdaPackGrayReduced / jdaPackGrayReducedDevice have the contract of jdaPackGrayOriented / jdaPackGrayOrientedDevice in every
 * other respect -- formats, pitch, rectangle, the refusals with nothing written and nothing launched, the stream, the return
 * on completion, re-entrancy, stats with launches == 1 for n > 0 -- where pixels and bytes_out count the rw * rh reduced
 * pixels, bytes_in the bytes of the rectangle's pixels that take part (rw f * rh f * bytes per pixel), and the two overlap
 * checks read the rw * rh destination bytes of an image (against the whole rectangle's bytes of every source row).
 * Additionally refused, the message naming the image index: NULL factors with n > 0, a factor outside 1..8, w < f or h < f
 * (the reduced image would be empty).  With every factor 1 the call forwards to jdaPackGrayOriented[Device] (which forwards
 * to jdaPackGray[Device] when every orientation is 0): the bytes are theirs.  The host form is plain loops over the
 * definition; the device form makes ONE kernel launch for all n images of whatever sizes, formats, factors and orientations
 * (k_reduce.hip: 64 x 64 tiles of the turned reduced image through LDS) and never reads a byte outside the dwords that hold
 * the rectangle's participating pixels of a source row: a source that ends with its allocation is safe.
 *
 * jdaReduceBack (host only, in place) has the arguments of jdaOrientBack and factors.  Boxes and landmarks are in the
 * coordinates of image face_image[f]'s turned, reduced rectangle and on return in those of the WHOLE source image:
 *   first    jdaOrientBack's own mapping with (rw, rh) as the rectangle's size and WITHOUT the rectangle's origin, the
 *            sequential exchange of the (left, right) pairs for orientations 4..7 included;
 *   then     the scale.  Boxes, integer exact: x0 = x0 * f, y0 = y0 * f, every size times f.  Landmarks, under the
 *            pixel-index convention -- reduced pixel i covers source pixels i f .. i f + f - 1, whose centre is
 *            i f + (f - 1) / 2 --, in the type's own precision, one operation per line, no fused multiply-add:
 *                x = x * (real)f      then      x = x + c,   c = (real)(f - 1) / 2  (exact in binary);      y alike
 *   then     x0 += rx, y0 += ry;  x = x + (real)rx, y = y + (real)ry.
 * With every factor 1 the results are jdaOrientBack's, bit for bit.  Refused with nothing written: everything jdaOrientBack
 * refuses, NULL factors with n_faces > 0, a factor outside 1..8, w < f or h < f. */
JDA_API int jdaReduceSize(int w, int h, int factor, int orient, int *rw, int *rh);
JDA_API int jdaPackGrayReduced(const jdaPixels *images, const int *factors, const int *orients, int n, unsigned char *dst,
                               const size_t *dst_offsets);
JDA_API int jdaPackGrayReducedDevice(void *cascador, const jdaPixels *images, const int *factors, const int *orients,
                                     int n, unsigned char *d_dst, const size_t *dst_offsets, void *hip_stream,
                                     jdaPackStats *stats);
JDA_API int jdaReduceBack(const jdaPixels *images, const int *factors, const int *orients, int n_images,
                          const int *face_image, int n_faces, int *boxes, int box_ints, void *landmarks,
                          int real_bytes, int landmark_n, const int *left, const int *right, int sym_n);

/* ------------------------------------------------------------------------ */
/* Frames whose faces are rolled                                            */
/* ------------------------------------------------------------------------ */
/* The cascade finds upright faces; "frames in any orientation" covers the quarter turns and mirrors, and between them there
 * is nothing: a head rolled by 30 - 60 degrees, a tilted phone, a ceiling camera.  Every consumer of an upright-only detector
 * runs it on a few rotated copies of the frame (typically +-30, +-60 degrees) and maps the hits back.  These entries are
 * jdaPackGrayOriented[Device] with a rotation by ANY angle, each image by its own, in place of the orientation, and the way
 * back: jdaRotateBack takes boxes and landmarks found on the rotated images into the source images the caller holds, where
 * jdaFaceChips ("faces as they leave") cuts them upright.
 *
 * The plan (jdaRotationPlan; host only -- everything else is defined from its c, s, tw, th, and the pack entries and the way
 * back call this very function, so libm is never consulted on the device and a restatement takes c and s from here).
 *   if degrees is an integer multiple of 90 (fmod(degrees, 90) == 0), (c, s) comes from the exact table for
 *   k = (degrees / 90) mod 4 in 0..3:   k = 0: (1, 0)    k = 1: (0, 1)    k = 2: (-1, 0)    k = 3: (0, -1)
 *   otherwise c = cos(degrees * (pi / 180)) and s = sin(degrees * (pi / 180)), doubles, from the host's libm
 *   tw = max(1, (int)ceil(((double)w * |c| + (double)h * |s|) - 1. / 1024))
 *   th = max(1, (int)ceil(((double)w * |s| + (double)h * |c|) - 1. / 1024))
 * and w, h are copied.  Refused with -1: NULL rot, a non-finite angle, |degrees| > 36000, w or h below 1.
 *
 * A turned pixel, to the bit, on the host and on the device.  fp64, one operation per step as written, no fused
 * multiply-add.  With cu = (tw - 1) / 2, cv = (th - 1) / 2, cx = (w - 1) / 2, cy = (h - 1) / 2 (all exact), output pixel
 * (column u, row v) of the tw x th image samples the rectangle at
 *   du = u - cu                   dv = v - cv
 *   sx = (c * du + s * dv) + cx   sy = (c * dv - s * du) + cy
 * by the sampling of "faces as they leave" with n = 1, on the RECTANGLE:
 *   the sample is 0 unless sx > -1 && sx < w && sy > -1 && sy < h; otherwise
 *   X = floor(sx * 1024 + 0.5)   Y = floor(sy * 1024 + 0.5)   x0 = X >> 10   fx = X & 1023   y0 = Y >> 10   fy = Y & 1023
 *   the taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), each 0 where outside [0, w) x [0, h) of the rectangle
 *   -- nothing outside the rectangle is read: the pack family's rule --, weigh (1024 - fx) * (1024 - fy), fx * (1024 - fy),
 *   (1024 - fx) * fy, fx * fy; tap * weight is summed in unsigned 32-bit integers
 *   out = (sum + 2^19) >> 20
 * Every TAP is made gray first by the Q14 formula of "frames as they arrive", rounded per tap: the rotated image of a colour
 * source equals the rotated image of its jdaPackGray image.  Positive angles turn the picture clockwise as displayed.  At
 * 90 / 180 / 270 the bytes are those of orientation 1 / 2 / 3 and at 0 jdaPackGray's, for any w x h: every quantity is then
 * an integer or a half-integer, fx = fy = 0 and out is the tap.
 *
 * jdaPackGrayRotated / jdaPackGrayRotatedDevice have the contract of jdaPackGrayOriented / jdaPackGrayOrientedDevice in every
 * other respect -- formats, pitch, rectangle, the refusals with nothing written and nothing launched, the stream, the return on
 * completion, re-entrancy, stats with launches == 1 for n > 0 -- where image i is written as tw * th bytes, rows of tw bytes
 * back to back, both overlap checks read the tw * th destination bytes of an image, pixels and bytes_out count tw * th and
 * bytes_in the rectangle's w * h * bytes per pixel.  Additionally refused, the message naming the image index: NULL degrees
 * with n > 0, an angle the plan refuses, tw or th above 32768.  When every angle is a multiple of 90 the call forwards to
 * jdaPackGrayOriented[Device]: the bytes are equal either way.  The host form is plain loops over the definition; the
 * device form makes ONE kernel launch for all n images of whatever sizes, formats and angles (k_rotate.hip: 64 x 64 tiles
 * of the turned image, the source box of a tile through LDS, gray once per source pixel) and never reads a byte outside the
 * rectangle's pixels of a source row's dwords: a source that ends with its allocation is safe.
 *
 * jdaRotateBack (host only, in place) has the arguments of jdaOrientBack without the pairs: nothing mirrors.  Boxes and
 * landmarks are in the coordinates of image face_image[f]'s turned rectangle and on return in those of the WHOLE source
 * image; (rx, ry) is the rectangle's origin:
 *   landmarks   a feature at turned (x, y) lies at the map above with (x, y) for (u, v); then x = sx + (double)rx,
 *               y = sy + (double)ry.  All in double: floats are widened first and rounded once at the end.
 *   boxes       the centre (x + (bw - 1) / 2, y + (bh - 1) / 2), in double, goes through the same map to (mx, my);
 *               x0 = (int)floor((mx - (bw - 1) / 2) + 0.5) + rx     y0 = (int)floor((my - (bh - 1) / 2) + 0.5) + ry
 *               sizes unchanged: the box in the source frame is the upright box around the rolled face; the caller knows
 *               its angle.
 * At multiples of 90, square boxes equal jdaOrientBack's with orientation 0 / 1 / 2 / 3 bit for bit, and so do landmarks
 * wherever jdaOrientBack's own steps are exact in the landmark's type (it rounds after every step in that type, this
 * rounds in double and once to the type; (x - cu) + cx gives x back only up to double's rounding).  Scores are not touched.
 * Refused with -1, nothing written: what jdaOrientBack refuses (NULL images or face_image with n_faces > 0, a negative
 * count, box_ints other than 3 or 4, real_bytes other than 4 or 8, landmark_n < 1, a face_image outside [0, n_images),
 * everything jdaPackGray refuses about an image), NULL degrees with n_faces > 0, an angle the plan refuses.  n_faces == 0
 * returns 0 and touches nothing. */
typedef struct { double c, s; int w, h, tw, th; } jdaRotation;   /* filled by jdaRotationPlan */

JDA_API int jdaRotationPlan(int w, int h, double degrees, jdaRotation *rot);
JDA_API int jdaPackGrayRotated(const jdaPixels *images, const double *degrees, int n, unsigned char *dst,
                               const size_t *dst_offsets);
JDA_API int jdaPackGrayRotatedDevice(void *cascador, const jdaPixels *images, const double *degrees, int n,
                                     unsigned char *d_dst, const size_t *dst_offsets, void *hip_stream,
                                     jdaPackStats *stats);
JDA_API int jdaRotateBack(const jdaPixels *images, const double *degrees, int n_images, const int *face_image, int n_faces,
                          int *boxes, int box_ints, void *landmarks, int real_bytes, int landmark_n);

/* ------------------------------------------------------------------------ */
/* Faces as they leave                                                      */
/* ------------------------------------------------------------------------ */
/* Every detect entry hands back boxes, scores and landmarks.  What a recogniser, an attribute net, a quality filter or a
 * thumbnailer takes is the face itself, turned upright by its landmarks and resampled to a fixed size: a CHIP.  These entries
 * fit a similarity transform to each face's landmarks and cut its chip out of the source image -- any jdaPixels: the
 * original colour frame, at its pitch, with the rectangle a packed crop was detected on -- in one call for any number of
 * faces of any number of images.  Like the gray value above, the chip is DEFINED here, in fp64 with a stated order of
 * operations up to a coordinate's rounding to 1/1024 pixel and in integers from there on: host form, device form and the
 * restatement in tests/chips_ref.py agree to the byte, the matrices to the bit.
 *
 * The fit (on the host in both forms; fp64, every sum strictly sequential in landmark order from 0., no fused
 * multiply-add).  Face f has landmarks p_i = (landmarks[f][2i], landmarks[f][2i+1]), pixels in the coordinates of its
 * image's RECTANGLE (what a detect call on the packed rectangle returned; real_bytes 4: jdaResult's floats, each widened to
 * double; 8: jdaResultD's doubles), and the template has points q_i = (tmpl[2i], tmpl[2i+1]) in chip pixels.  Only
 * landmarks i with use[i] != 0 take part (use == NULL: all L); m = their number.
 *   sum_qx = 0., then sum_qx = sum_qx + qx_i for the used i in index order; sum_qy, sum_px, sum_py alike
 *   mqx = sum_qx / m    mqy = sum_qy / m    mpx = sum_px / m    mpy = sum_py / m          (m as a double)
 *   per used i:  cqx = qx_i - mqx   cqy = qy_i - mqy   cpx = px_i - mpx   cpy = py_i - mpy
 *   den = 0., sa = 0., sb = 0., then per used i in index order
 *     den = den + (cqx * cqx + cqy * cqy)
 *     sa  = sa  + (cqx * cpx + cqy * cpy)
 *     sb  = sb  + (cqx * cpy - cqy * cpx)
 *   a = sa / den    b = sb / den
 *   tx = (mpx - (a * mqx - b * mqy)) + (double)rect.x
 *   ty = (mpy - (b * mqx + a * mqy)) + (double)rect.y
 *   M = {a, -b, tx, b, a, ty}
 * M maps chip pixels to pixels of the WHOLE source image (least squares over the used landmarks); matrices, if given,
 * receives the six doubles of every face.  A face is refused if fewer than 2 landmarks are used, if den == 0 (the used
 * template points coincide) or if a landmark or template value that is used is not finite.
 *
 * Supersampling.  A chip pixel is the mean of n x n bilinear samples, n per axis, from s2 = a * a + b * b (the squared
 * reduction; no sqrt): n = 1 if s2 <= 1, 2 if s2 <= 4, 3 if s2 <= 9, else 4.  supersample = 0 takes this n, 1..4 force it.
 * BEYOND A 4x REDUCTION ALIASING RETURNS: n stops at 4; reduce the source first (the pyramid of jdaBuildPyramid) for more.
 *
 * A chip pixel (u, v), u < chip_w, v < chip_h.  For j in [0, n) and i in [0, n):
 *   cu = (double)u + (double)((2 * i + 1) - n) / (double)(2 * n)      cv = (double)v + (double)((2 * j + 1) - n) / (double)(2 * n)
 *   sx = (M[0] * cu + M[1] * cv) + M[2]                               sy = (M[3] * cu + M[4] * cv) + M[5]
 *   the sample is 0 unless sx > -1 && sx < W && sy > -1 && sy < H (W, H: the whole source image, not the rectangle -- a
 *   face at a crop's edge keeps its surroundings; a NaN fails the test); otherwise
 *   X = (int64)floor(sx * 1024 + 0.5)   Y = (int64)floor(sy * 1024 + 0.5)
 *   x0 = X >> 10   fx = X & 1023   y0 = Y >> 10   fy = Y & 1023
 *   the taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), each 0 where outside the image, weigh
 *   (1024 - fx) * (1024 - fy), fx * (1024 - fy), (1024 - fx) * fy, fx * fy; tap * weight is summed over all taps of all
 *   samples in unsigned 32-bit integers (255 * 2^20 * 16 fits).
 *   out = ((sum + n * n * 2^19) >> 20) / (n * n)                      (unsigned integer division)
 *
 * Formats.  Chips are JDA_PIX_GRAY8, JDA_PIX_BGR24 or JDA_PIX_RGB24; sources any JDA_PIX_*.  Colour to colour interpolates
 * each channel, the channel order converted, alpha never read; gray to colour replicates the value; colour to gray converts
 * each TAP with the Q14 formula of "frames as they arrive" and then interpolates, so the gray chip of a colour image equals
 * the gray chip of its jdaPackGray image.  No byte outside the source image's pixels is ever read (not a pitch's slack, not
 * alpha): a source that ends with its allocation is safe.
 *
 * Layout.  Chip f is written at dst + f * chip_w * chip_h * bytes per chip pixel, rows back to back, chips back to back.
 *
 * jdaFaceChips needs no cascador and no GPU: the definition in plain loops; tmpl is required.  jdaFaceChipsDevice takes
 * device sources and a device d_dst (landmarks, tmpl, use, face_image and matrices are host memory: the fit runs on the
 * host) and makes ONE kernel launch for all faces of the call, whatever their images' sizes and formats (k_chips.hip); the
 * cascador supplies the device, the error state, a lane whose grow-only buffer holds the face and image records, and with
 * tmpl == NULL the template: its mean shape times the chip size, q_i = (mean[2i] * chip_w, mean[2i+1] * chip_h), which
 * needs landmark_n == the model's.  It runs on hip_stream if given, otherwise on the lane's own stream, returns when d_dst
 * is complete and is re-entrant on one cascador like every other entry.  stats (may be NULL): faces, chip bytes written,
 * taps (4 per sample: chip pixels * n * n * 4, read or not), kernel launches (1), the kernel's time between two events and
 * the call's wall time.  jdaCascadorMeanShape copies the model's mean shape (2 * landmark_n doubles, normalised to the
 * detection window) -- no other entry returns it.
 *
 * Refused with -1, jdaGetLastError() naming the face or image index, nothing launched and no byte of dst or matrices
 * written: a NULL pointer where one is needed (images, face_image, landmarks, dst, tmpl in the host form; the cascador), a
 * negative count, landmark_n < 1, real_bytes other than 4 or 8, a chip format that is not one of the three, chip_w or
 * chip_h outside 1..4096, supersample outside 0..4, a face_image outside [0, n_images), everything jdaPackGray refuses
 * about an image, a face the fit refuses, a destination that overlaps the byte range of any source image (its first pixel
 * to its last).  n_faces == 0 returns 0 and touches nothing. */
typedef struct { long long faces, chip_bytes, taps; int launches; double device_ms, call_ms; } jdaChipStats;

JDA_API int jdaFaceChips(const jdaPixels *images, int n_images, const int *face_image, const void *landmarks, int real_bytes,
                         int n_faces, int landmark_n, const double *tmpl, const unsigned char *use, int chip_w, int chip_h,
                         int chip_format, int supersample, unsigned char *dst, double *matrices);
JDA_API int jdaFaceChipsDevice(void *cascador, const jdaPixels *images, int n_images, const int *face_image,
                               const void *landmarks, int real_bytes, int n_faces, int landmark_n, const double *tmpl,
                               const unsigned char *use, int chip_w, int chip_h, int chip_format, int supersample,
                               unsigned char *d_dst, double *matrices, void *hip_stream, jdaChipStats *stats);
JDA_API int jdaCascadorMeanShape(void *cascador, double *mean_shape);

#ifdef __cplusplus
}
#endif

#endif /* JDA_AMD_JDA_H_ */
