// Device-side data layout and kernel launchers of the detect path (gfx950).
//
// Vocabulary (follows the reference): a *window* is one candidate (level,x,y);
// a *cart* is one depth-D tree of the cascade; a *stage* is K carts followed
// by one global shape regression.  A window's *gid* is
// frame*windows_per_frame + its scan-order index inside the frame.
//
// Two kernels carry the cascade (DESIGN.md "pipeline"):
//   k_scan    lane = window, LDS pixel tile, the first `handoff` carts of
//             stage 0, survivors compacted by ballot/prefix-sum
//   k_finish  wave = window: lanes = carts for the tree walks of a stage,
//             lanes = shape coordinates for the regression gather; runs a
//             survivor through every remaining cart, stage and the final cut
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace jda {

constexpr int kMaxLevels = 64;
constexpr int kMaxStages = 16;

struct DevLevel {
  int win, step, nx, ny;
  int base;              // first window of the level inside a frame (scan order)
  int tiled;             // k_scan pixel mode -- 1: LDS pixel tile, 16-bit node offsets; 3: LDS pixel tile, 21-bit
                         // node offsets (big windows, few per tile); 2: pixels through L1/L2 (windows that do
                         // not fit LDS); 0: not scanned, k_finish takes its windows from cart 0
  int tw, th;            // windows per tile in x / y
  int tiles_x, tiles_y;
  int pitch;             // LDS bytes per tile row
  int s0_table;          // first entry of this level in the stage-0 offset table (units: nodes)
};

struct DevPlan {
  int n_levels;
  int width, height;
  int windows;            // per frame
  DevLevel lv[kMaxLevels];
};

// Ragged batches (images of different sizes in one pass, the FDDB loop of reference src/test.cpp:100-170 as ONE
// job): every image is staged with the same row pitch (DevPlan::width), the pyramid levels are a global list
// (DevPlan::lv: window size, step, tile shape, stage-0 table -- the window sizes of c/jda.c:331-333 do not depend on
// the image, an image only uses the prefix that fits it), and what does depend on the image sits in one record per
// (image, level).  A workgroup of k_scan finds its tile through RagBlk: blockIdx -> (segment, tile).
struct RagSeg {
  unsigned long long img_off;   // byte offset of the image inside WorkT::frames
  uint32_t gid_base;            // gid of this level's first window of this image (scan order: image, level, y, x)
  uint16_t nx, ny;              // windows per row / column (c/jda.c:335-336)
  uint16_t tiles_x;             // tiles per row of windows
  uint16_t level;               // index into DevPlan::lv
  uint16_t image;               // image index inside the pass (the queues pack it in 16 bits)
  uint16_t tw, th;              // windows per tile in x / y for THIS image: the level's tile (DevLevel::tw x th) re-cut to
                                // the image's own grid, inside the level's LDS row pitch (the node offsets depend on
                                // the pitch only)
  uint16_t pad0; uint32_t pad1;
  // the level's own record (copied from DevPlan::lv, so that a workgroup's prologue is blk -> seg and not
  // blk -> seg -> level: three dependent loads in front of the tile load cost the scan 15 % on identical geometry)
  int win, step, pitch, s0_table, tiled; uint32_t pad2, pad3, pad4;
};
static_assert(sizeof(RagSeg) == 64, "RagSeg is read as four 16-byte words");
struct RagBlk { uint32_t seg, tile; };
struct RagImg {                 // k_repack: one image of a ragged batch, tight rows -> common row pitch
  unsigned long long src_off, dst_off;
  int w, h;
};

// Split node as k_finish reads it: 32 bytes, two 16-byte loads (the
// reference's jdaNode is also 32 bytes, c/jda.c:114-127).
struct NodeF {
  int scale;
  int lm1x2, lm2x2;   // landmark index * 2, like c/jda.c:521-523
  int th;
  float o1x, o1y, o2x, o2y;
};
struct NodeD {         // dialect CPP: fp64 offsets (already passed through the identity STParameter)
  int scale;
  int lm1x2, lm2x2;
  int th;
  double o1x, o1y, o2x, o2y;
};

// k_finish walks 64 carts per wave, one cart per lane.  In cart-major order every lane's node sits in its own
// cache line (a cart's nodes are 7 x 32 bytes apart) and the two 16-byte halves of a node are two accesses; the
// L1 tag rate is what bounds k_finish (TA busy 70-75 %).  k_finish therefore reads a second copy of the nodes:
// level-major (the roots of all carts of a stage together, then the second level, ...) and split into the four
// offsets and the integer fields, so that the lanes of a wave read consecutive records.
template <typename Real>
struct NodeOff { Real o1x, o1y, o2x, o2y; };
// index of heap node `node` (on level d) of cart k inside one stage's K*node_n records
__host__ __device__ inline unsigned lm_index(unsigned K, unsigned k, unsigned d, unsigned node) {
  const unsigned first = (1u << d) - 1u;
  return K * first + (k << d) + (node - first);
}

// Levels d >= split of a tree with `levels` node levels: the nodes below one ancestor on level split - 1 form a group of
// lm_deep_group(levels, split) records in level order; the groups of a cart are consecutive, carts follow each other.
__host__ __device__ inline unsigned lm_deep_group(unsigned levels, unsigned split) { return (2u << (levels - split)) - 2u; }
__host__ __device__ inline unsigned lm_deep_index(unsigned k, unsigned d, unsigned node, unsigned levels, unsigned split) {
  const unsigned rel = node - ((1u << d) - 1u);               // position on its level
  const unsigned below = d - split + 1u;                      // levels between the ancestor and this node
  const unsigned anc = rel >> below, within = rel & ((1u << below) - 1u);
  return ((k << (split - 1u)) + anc) * lm_deep_group(levels, split) + ((1u << below) - 2u) + within;
}

// Stage-0 node with its pixel offsets resolved for one level (DESIGN.md
// "stage-0 hoist"): in stage 0 every window holds the mean shape, so the
// feature coordinates depend only on (node, window size).
// Packings of the same 8 bytes:
//   k_scan, tiled == 1    : lo = off1 | off2 << 16 (byte offsets inside the LDS tile), hi = th in [-256,255]
//   k_scan, tiled == 2, 3 : off1 : 21 | off2 : 21 | th + 256 : 10 (byte offsets inside the frame, row pitch = width,
//                           or inside a big LDS tile)
//   k_finish (level-major copy of the table, every level): x1 : 11 | y1 : 11 | x2 : 11 | y2 : 11 | th + 256 : 10,
//                           pixel coordinates inside the window (read from the frame or from the window's LDS copy)
struct S0Node {
  uint32_t lo;
  uint32_t hi;
};
constexpr int kS0GlobalOffBits = 21;

template <typename Real>
struct DevModelT {
  int T, K, L, D, node_n, leaf_n, dim;
  const void* nodes;       // NodeF / NodeD  [T*K*node_n]
  const void* lm_off;      // NodeOff<Real> [T*K*node_n], level-major (lm_index): k_finish's copy of the offsets
  const uint2* lm_meta;    // the same nodes' {lm1x2 | lm2x2 << 15 | scale << 30, th}
  const void* lm_deep;     // NodeF / NodeD of the levels from lm_split on, grouped per (cart, ancestor on level lm_split - 1) in level
  int lm_split;            // order (lm_deep_index): a deep tree's last levels of one path share a line or two instead of one line
                           // per level and array.  lm_split = D - 1: no such levels (depth <= 5), everything level-major
  const Real* leaf;        // [T*K*leaf_n]
  const Real* cth;         // [T*K]
  const Real* cmean;       // [T*K]
  const Real* cstd;        // [T*K]
  const uint8_t* cnorm;    // [T*K] 1 where (mean,std) != (0,1)
  const void* par0;        // {th, norm, mean, std} per cart [T*K], packed for LDS staging (k_scan, k_stage)
  const Real* w;           // [T][K*leaf_n][dim]
  const Real* w_rows;      // the same rows w_pitch elements apart, each starting on a 128-byte line (k_finish gathers one row
  int w_pitch;             // per cart: a tight 216-byte row straddles a third line in most positions); = w, dim when not padded
  int w_stream;            // a stage's weight rows are far larger than an XCD's L2: k_finish reads them with non-temporal loads, so that
                           // they pass through L2 without evicting the stage's split nodes (3 MB for K=2000, D=6)
  const Real* mean_shape;  // [dim]  (dialect CPP: + 0., the zero random shift of RandomShape)
  const Real* mean_shape_raw;  // [dim]  as stored (second argument of STParameter::Calc)
  int similarity;          // dialect CPP: Config::with_similarity_transform -- 0 off, 1 on, 2 + s: on, and stage s of a trainer snapshot is the one in training (it walks with the previous stage's parameter)
};

// Device buffers of one pass over a sub-batch of frames.
template <typename Real>
struct WorkT {
  const uint8_t* frames; size_t frame_stride; int n_frames;
  const uint8_t* half; size_t half_stride; int hw, hh;        // pyramid images, only for multi-scale models
  const uint8_t* quarter; size_t quarter_stride; int qw, qh;
  // dialect CPP, method 0 on a multi-scale model (cascador.cpp:243-245): no half / quarter IMAGE -- every window has its own
  // half_size^2 and quarter_size^2 patches, resized from its ROI: window i of frame f at half + f * half_stride + i * patch_hs^2
  // (quarter alike).  0: the images above
  int patch_hs, patch_qs;
  // hand-off queue k_scan -> k_finish (plus the windows k_scan does not cover)
  uint32_t* q_gid; Real* q_score; uint32_t* q_hash; uint32_t* q_kstart;
  uint32_t* q_xy; uint32_t* q_wf;          // x | y << 16 and win | frame << 16 of the queued window
  unsigned long long* counters;                                // see Counter
  // mid queue: windows alive after stage 0, with their regressed shape (k_finish pass 1 -> pass 2)
  uint32_t* m_gid; Real* m_score; uint32_t* m_hash; Real* m_shape; uint32_t* m_xy; uint32_t* m_wf;
  // ... and the stage-0 leaves k_filter0 found on the way (the carry, see carry_pack): entry o's 64 words at m_leaf + 64 * o --
  // lane l's word holds the leaves of carts l, 64 + l, 128 + l, .. -- for the carts from m_k0[o] on (a multiple of 64; K:
  // nothing carried, the entry comes from a producer that holds no leaves, or lies beyond cap_l).  m_leaf is null in a pass
  // whose model or path does not carry (Pass::carry_ok): k_finish(survivors) then walks every cart of stage 0 itself.
  uint32_t* m_leaf; uint32_t* m_k0; unsigned cap_l;            // cap_l: entries of m_leaf (the first cap_l of the mid queue, kCarryCapMax at most)
  // dense mode (k_stage): per-window state indexed by gid -- m_score / m_hash / m_shape are reused as
  // score / hash / shape, st_carts holds carts evaluated (-1 = still alive)
  int* st_carts;
  // final detections: windows that passed every cart and the final threshold
  uint32_t* out_gid; Real* out_score; Real* out_shape;
  // per-window trace (all null when off), indexed by gid
  int* tr_carts; Real* tr_score; uint32_t* tr_hash; Real* tr_shape;
  unsigned cap;                                                // windows of the pass at most: entries of the per-window arrays (trace; dense mode's state)
  // The queues are sized from what earlier passes left in them, not for the worst case (r06): cap_q entries of the hand-off
  // queue (q_*), cap_m of the mid queue (m_*) and of the detection list (out_*).  A kernel never writes past them; the
  // counters keep counting, so the host sees an overflow as counter > capacity and runs the pass again with room
  // (Pass::recover_overflow).  Dense mode uses m_* as per-window state: the host gives it cap_m >= cap.
  unsigned cap_q, cap_m;
  // ragged batch (all null otherwise): (image, level) segments, the block map of the scan launches, image offsets
  const RagSeg* segs; const RagBlk* blk; const unsigned long long* img_off;
#ifdef JDA_SCAN_TIMING
  unsigned long long* dbg;                                     // [65536][16] shader-clock stamps of k_scan workgroups
#endif
#ifdef JDA_BOUNDS_CHECK
  const uint8_t* bc_lo; const uint8_t* bc_hi;                  // bounds-check build: the device range [lo, hi) the pass's frames occupy
#endif
};

// The carry of stage-0 leaves from k_filter0 to k_finish(survivors): the leaf of cart k lives in word k & 63 of the window's
// 64 words, in the `bits` bits from bit bits * (k >> 6) on -- what lane k & 63 of the wave walked in round k >> 6.
constexpr unsigned kCarryCapMax = 1u << 16;                    // mid-queue entries that get leaf words (16 MB per lane at most)
__host__ __device__ constexpr int carry_bits(int leaf_n) { int b = 0; while ((1 << b) < leaf_n) b++; return b; }
__host__ __device__ constexpr int carry_rounds(int K) { return (K + 63) >> 6; }
__host__ __device__ constexpr bool carry_fits(int leaf_n, int K) { return carry_bits(leaf_n) * carry_rounds(K) <= 32; }
__host__ __device__ constexpr uint32_t carry_pack(uint32_t word, int leaf, int bits, int round) { return word | ((uint32_t)leaf << (bits * round)); }
__host__ __device__ constexpr int carry_unpack(uint32_t word, int bits, int round) { return (int)((word >> (bits * round)) & ((1u << bits) - 1u)); }
namespace carry_check {
// every leaf value in every round of a word comes back, whatever the other rounds hold
__host__ __device__ constexpr bool round_trip(int leaf_n, int K) {
  const int bits = carry_bits(leaf_n), rounds = carry_rounds(K);
  if (!carry_fits(leaf_n, K)) return false;
  for (int seed = 0; seed < leaf_n; seed++) {
    uint32_t word = 0;
    for (int r = 0; r < rounds; r++) word = carry_pack(word, (seed + r * 5) % leaf_n, bits, r);
    for (int r = 0; r < rounds; r++) if (carry_unpack(word, bits, r) != (seed + r * 5) % leaf_n) return false;
  }
  return true;
}
static_assert(carry_bits(2) == 1 && carry_bits(4) == 2 && carry_bits(8) == 3 && carry_bits(1) == 0 && carry_bits(32) == 5, "bits = ceil(log2(leaf_n))");
static_assert(carry_rounds(64) == 1 && carry_rounds(540) == 9 && carry_rounds(682) == 11, "rounds = ceil(K / 64)");
static_assert(round_trip(2, 64) && round_trip(4, 64) && round_trip(8, 64), "K = 64");
static_assert(round_trip(2, 540) && round_trip(4, 540) && round_trip(8, 540), "K = 540: 27 bits with depth-4 trees");
static_assert(round_trip(2, 682) && round_trip(4, 682) && !carry_fits(8, 682), "K = 682: 11 rounds, depth 4 needs 33 bits -- no carry");
static_assert(!carry_fits(32, 2000) && carry_fits(2, 2048) && !carry_fits(2, 2049), "depth 6 with K = 2000 walks as before; 32 rounds of one bit fit");
// the word's edge: bits * rounds == 32 puts the last round's leaf in the top bits (bit 31 included); one cart more does not fit
static_assert(round_trip(4, 1024) && !carry_fits(4, 1025), "depth 3: 2 bits x 16 rounds = 32");
static_assert(round_trip(16, 512) && !carry_fits(16, 513), "depth 5: 4 bits x 8 rounds = 32");
static_assert(round_trip(256, 256) && !carry_fits(256, 257), "depth 9: 8 bits x 4 rounds = 32");
static_assert(round_trip(8, 640) && !carry_fits(8, 641), "depth 4: 3 bits x 10 rounds = 30, an eleventh round would need 33");
static_assert(carry_unpack(carry_pack(0u, 3, 2, 15), 2, 15) == 3 && carry_pack(0u, 3, 2, 15) == 0xc0000000u, "the top round of a full word keeps bit 31");
}  // namespace carry_check

// Work counters live in kCntShards copies, one 256-byte line apart, so that the
// workgroups of a launch do not serialise on one L2 atomic unit; the host sums
// the shards.  kCntTail / kCntOut are queue allocators and exist once (shard 0).
constexpr int kCntShards = 64;
constexpr int kCntStride = 32;   // 64-bit words per shard

enum Counter : int {
  kCntStage0 = 0,                  // kCntStage0 + t : windows that completed stage t
  kCntTail = kMaxStages,           // length of the hand-off queue
  kCntOut = kMaxStages + 1,        // final detections
  kCntCarts = kMaxStages + 2,      // carts evaluated, reference counting (Validate's n)
  kCntCartsScan = kMaxStages + 3,  // carts evaluated inside k_scan
  kCntWinScan = kMaxStages + 4,    // windows k_scan covered
  kCntMid = kMaxStages + 5,        // length of the mid queue (allocator, shard 0 only)
  kCntCartsScanGlb = kMaxStages + 6,  // carts evaluated inside k_scan's global-pixel launches
  kCntTotal = kMaxStages + 7,
  // spare words of a shard: [kCntTotal, kCntMidScan) deal k_scan_p's tiles (PScanCfg::dyn_slot, shards 0..7)
  kCntMidScan = kCntStride - 1,    // windows k_scan_p put into the mid queue itself (they count as handed off)
  kCntPostCursor = kCntTotal,      // shard 8 only: rows k_post has allotted (shards 0..7 use this word to deal tiles)
  kCntScanErr = kCntTotal          // shard 9 only: k_scan_p's watchdog word (bit 0: a wave gave up waiting for work that never came,
                                   // bit 1: a ring commit timed out) -- nonzero: the host runs the pass again with k_scan
};
constexpr int kCntScanErrShard = 9;
static_assert(kCntTotal <= kCntStride, "counter shard too small");

// ---- launchers (k_misc.hip, k_scan.hip, k_finish.hip, k_stage.hip) ------------------------------------------------

// What a launcher of the detect path launched.  Each takes `how` (never null), as launch_lbf / launch_reval / plan_fit do,
// and fills it where it chooses the kernel's template arguments, from the constants that name the instantiation handed to
// hipLaunchKernelGGL -- not from its own arguments: the record cannot name another kernel than the one that ran.
// launched = false: the launcher found nothing to launch and returned hipSuccess.  After an error `how` is unspecified.
// The host turns a record into its public key and counts it in one place (host.h: LaunchLog).
struct ScanLaunch {                    // launch_scan, launch_scan_ragged, launch_scan_persistent
  bool launched, persistent;           // persistent: k_scan_p, else k_scan
  int depth, mode, block;              // DEPTH (scan_depth_class), pixel mode (DevLevel::tiled), threads per workgroup
  bool ragged, lean, trace, merged;    // lean: NORM = false (k_scan) / PScanCfg::any_norm == 0 (k_scan_p); merged: the launch spans levels
};
struct FinishLaunch {                  // launch_finish, launch_filter0
  bool launched, filter0, trace;       // filter0: k_filter0, else k_finish
  int groups;                          // kG, 1..4 (k_filter0: 0, like every field below but carry)
  bool multi, st, stream, survivors;   // MULTI, ST, STREAM; the launch reads the mid queue as k_filter0 left it
  bool carry, tile;                    // the launch sees leaf words (WorkT::m_leaf; k_finish: and reads survivors); a window tile in LDS
};
struct WideLaunch { bool launched, conc; };   // launch_finish_wide; conc: the conc_ok it handed to the kernel
// (launch_stage reports the StageChoice it used: below, with the launcher)

// Pyramid images of reference c/jda.c:450-457 for n frames.
hipError_t launch_resize(const uint8_t* src, size_t src_stride, int n, int sw, int sh,
                         uint8_t* dst, size_t dst_stride, int dw, int dh, float rx, float ry,
                         hipStream_t stream);

// cv::resize(INTER_LINEAR, 8UC1) restatement for dialect CPP (half/quarter images, method-0 pyramid).
hipError_t launch_resize_cv(const uint8_t* src, size_t src_stride, int n, int sw, int sh,
                            uint8_t* dst, size_t dst_stride, int dw, int dh, hipStream_t stream);

// The per-window patches of method 0 (cascador.cpp:243-245): cv::resize(INTER_LINEAR) of the win x win ROI of every window
// of a one-level plan (nx x ny windows, `step` apart, in frames of row pitch lw) to ds x ds, window i of frame f at
// dst + f * dst_stride + i * ds * ds.
hipError_t launch_resize_cv_patches(const uint8_t* src, size_t src_stride, int n, int lw, int nx, int ny, int step, int win,
                                    uint8_t* dst, size_t dst_stride, int ds, hipStream_t stream);

// Resolves stage-0 node offsets for every tiled level (dialect 0 = C, 1 = CPP): cart-major into table (k_scan),
// level-major (lm_index) into table_lm (k_finish).
hipError_t launch_prep_stage0(int dialect, const DevPlan* d_plan, const DevPlan& h_plan,
                              const void* nodes, const void* mean_shape, int K, int node_n,
                              S0Node* table, S0Node* table_lm, hipStream_t stream);

int scan_handoff_cap(int node_n, int leaf_n, int real_bytes);   // carts per LDS table chunk of k_scan
size_t scan_lds_bytes(int pix_bytes, int carts, int node_n, int leaf_n, int real_bytes, bool trace, int block);

// Windows of untiled levels (or of every level) -> head of the hand-off queue, k_start = 0.
template <typename Real>
hipError_t launch_enqueue(const DevPlan* d_plan, const DevPlan& h_plan, bool all_levels,
                          const WorkT<Real>& w, hipStream_t stream);

// Stage-0 scan, carts [0, handoff) of stage 0, for the levels of pixel mode `mode` (DevLevel::tiled):
// level >= 0 = that level; level < 0 = every level of the mode in one launch (small batches).
// cp_max = windows per tile at or below which a phase spreads (window, cart) pairs over the lanes.
// opts: bit 0 = 8 trees in flight per lane instead of 4; bits 8..15 = carts before the first compaction.
template <typename Real>
hipError_t launch_scan(int mode, int level, bool trace, int handoff, int cp_max, int opts, const DevPlan* d_plan,
                       const DevPlan& h_plan, const DevModelT<Real>& m, const S0Node* table,
                       const WorkT<Real>& w, ScanLaunch* how, hipStream_t stream, int lv_lo = 0, int lv_hi = kMaxLevels);
// (level < 0: ONE launch for every level of pixel mode `mode` among levels [lv_lo, lv_hi))

// DEPTH of a scan kernel (k_scan_impl.h, k_scan_p.hip): the tree depths with a kernel of their own, 0 = the generic walk.
inline int scan_depth_class(int D) { return D == 4 ? 4 : (D == 6 ? 6 : 0); }
// Threads per workgroup of a persistent launch (the scan_p_block option, whole waves within 64..1,024).
inline int scan_p_block_of(long long knob) { return (int)std::max<long long>(64, std::min<long long>(1024, knob)) & ~63; }

// The same for a ragged batch: one launch over blocks [blk_base, blk_base + blk_n) of WorkT::blk, all of pixel mode
// `mode` with workgroups of `block` threads and pixel tiles of at most pix_bytes.  level: the level every block belongs
// to, < 0: blocks of several levels (the kernel finds each block's level itself; the record says merged).
template <typename Real>
hipError_t launch_scan_ragged(int mode, int block, bool trace, int handoff, int cp_max, int opts, const DevPlan* d_plan,
                              const DevModelT<Real>& m, const S0Node* table, const WorkT<Real>& w, int pix_bytes,
                              int blk_base, int blk_n, int level, ScanLaunch* how, hipStream_t stream);

// The persistent form of the LDS-tiled scan (k_scan_p.hip; dialect C, pixel mode 1, uniform batches): one workgroup per
// CU walks its share of the level's tiles through `slots` pixel-tile slots; items that have completed bound[b] carts
// wait in ring b; lg[b] = 6: a bucket task is lane = window over 64 items, 4 / 5: pair task over 16 / 32 items.
// bound[nb] = carts done by this kernel (the hand-off).  opts bit 0 / 1: 8 trees in flight per lane in fresh / bucket tasks.
constexpr int kPScanMaxBuckets = 6;
struct PScanCfg {
  int nb;
  int bound[kPScanMaxBuckets + 1];
  int lg[kPScanMaxBuckets];
  int slots, slot_bytes, opts;
  int bound_last;                      // = bound[nb]
  int any_norm;                        // a cart of [0, bound_last) normalises its score (mean, std != 0, 1)
  int tw_magic;                        // ceil(2^20 / tile width in windows) where i / tw == (i * magic) >> 20 for every window index of a tile, else 0
  int ring_cap[kPScanMaxBuckets], ring_off[kPScanMaxBuckets], ring_items;     // items per ring / first item / all rings (scan_p_ring_caps)
  int th, tiles_y;                     // the kernel's own cut of the level in y: rows of windows per tile, tiles per column (the
                                       // row pitch and the tile width are the plan's: the resolved node offsets depend on them)
  int dyn_slot;                        // >= 0: tiles are dealt at run time from the counters' spare word kCntTotal + dyn_slot of shards 0..7 (zeroed with the counters); -1: fixed shares
  int to_mid;                          // bound_last == K: a window that passes every cart of stage 0 goes straight to the mid queue
};
void scan_p_ring_caps(PScanCfg* cfg, int waves);
size_t scan_p_lds_bytes(const PScanCfg& cfg, int carts, int node_n, int leaf_n, int waves);
// rag_blk_n >= 0: a ragged pass -- the launch covers blocks [rag_blk_base, rag_blk_base + rag_blk_n) of WorkT::blk, all of
// `level` (cfg.slot_bytes = the largest tile any image of the chunk cut from it; cfg.th / tiles_y / tw_magic unused).
hipError_t launch_scan_persistent(int level, const PScanCfg& cfg, int block, int grid_max, const DevPlan* d_plan,
                                  const DevPlan& h_plan, const DevModelT<float>& m, const S0Node* table,
                                  const WorkT<float>& w, ScanLaunch* how, hipStream_t stream, int rag_blk_base = 0, int rag_blk_n = -1);

// Tight images (row stride = width) at raw + src_off -> rows of `pitch` bytes at dst + dst_off, n images of at most
// max_h rows.
hipError_t launch_repack(const uint8_t* raw, uint8_t* dst, const RagImg* imgs, int n, int max_h, int pitch, hipStream_t stream);

// Stages [t_begin, t_end) for every queued window: t_begin == 0 reads the hand-off queue,
// t_begin > 0 the mid queue; survivors go to the mid queue (t_end < T) or the detection list.
template <typename Real>
hipError_t launch_finish(bool trace, int t_begin, int t_end, bool apply_final_th, Real final_th,
                         const DevPlan* d_plan, const DevModelT<Real>& m, const WorkT<Real>& w,
                         int groups, long long n_hint, const S0Node* s0_table, int tile_win, FinishLaunch* how,
                         hipStream_t stream, bool survivors = false);
// survivors: the input is the mid queue as launch_filter0 leaves it (windows that passed every cart of stage 0, still
// holding the mean shape); t_begin must be 0.

// The rest of stage 0 for every window of the hand-off queue, four windows per workgroup and nothing but the filtering
// (k_finish.hip: k_filter0): rejected windows are final, survivors go to the mid queue.  Needs the resolved stage-0
// table of every level.
template <typename Real>
hipError_t launch_filter0(bool trace, const DevPlan* d_plan, const DevModelT<Real>& m, const WorkT<Real>& w, long long n_hint,
                          const S0Node* s0_table, FinishLaunch* how, hipStream_t stream);
// s0_table: the plan's resolved stage-0 tables (or null): stage 0 of windows from levels that have one walks from it
// tile_win: windows up to this side copy their pixels to LDS first (0: every pixel is read from the frame,
// < 0: the largest side that leaves the workgroup within kFinishLdsPerGroup)
constexpr size_t kFinishLdsPerGroup = 7680;

// The window tile of a k_finish launch and the LDS in front of it: the launcher (k_finish.hip: launch_finish_impl) asks
// these, and so does jdaFinishTileWin, which answers without a device.
// ST: the similarity transform exists in dialect CPP only.
constexpr bool finish_st(int real_bytes, int similarity) { return real_bytes == 8 && similarity != 0; }
// LDS in front of the window tile: shape, the carts' weight rows, stage counters, the transform's scratch (ST).
constexpr size_t finish_lds_base(int dim, int K, int real_bytes, bool st) {
  const size_t dim_pad = (size_t)((dim + 1) & ~1);
  return dim_pad * (size_t)real_bytes + (size_t)((K + 3) & ~3) * 4 + kMaxStages * sizeof(int) + (st ? (2 * dim_pad + 8) * (size_t)real_bytes : 0);
}
constexpr size_t finish_tile_bytes(int tile_win) { return tile_win > 0 ? (size_t)tile_win * (size_t)((tile_win + 3) & ~3) + 16 : 0; }
// The window tile of a launch asked for `tile_win` (0: none, n: windows up to n pixels, < 0: the largest that keeps the
// workgroup within kFinishLdsPerGroup -- 16 workgroups on a CU; measured on MI355X with one-wave workgroups,
// profiles/r02_finish_experiments.txt: up to 7,680 bytes the launch time does not depend on the LDS size, 7,712 bytes
// cost +17 %, 7,856 +23 %).  A multi-scale model has none: its nodes read the half and quarter images too.
constexpr int finish_tile_win(int dim, int K, int real_bytes, bool st, bool multi, int tile_win) {
  if (multi) return 0;
  if (tile_win >= 0) return tile_win;
  const size_t base = finish_lds_base(dim, K, real_bytes, st);
  int best = 0;
  for (int tw = 16; tw <= 255; tw++)
    if (base + finish_tile_bytes(tw) <= kFinishLdsPerGroup) best = tw;
  return best;
}
static_assert(finish_tile_win(54, 540, 4, false, false, -1) == 72 && finish_tile_win(54, 540, 4, false, true, -1) == 0, "the shipped model's tile (DESIGN.md section 4)");
static_assert(finish_tile_win(10, 1808, 4, false, false, -1) == 16 && finish_tile_win(10, 1828, 4, false, false, -1) == 0, "the search starts at 16 pixels");

// The finishing path of small jobs: one WORKGROUP per queued window (k_wide.hip), every remaining cart, stage and the
// final cut; reads the hand-off queue.  finish_wide_ok: the model fits (single-scale nodes, no similarity transform,
// a weight row within the LDS row buffer).
bool finish_wide_ok(int dim, int K, int leaf_n, int real_bytes, bool multi, bool similarity);
template <typename Real>
hipError_t launch_finish_wide(bool trace, bool apply_final_th, Real final_th, const DevPlan* d_plan,
                              const DevModelT<Real>& m, const WorkT<Real>& w, long long n_hint, const S0Node* s0_table,
                              WideLaunch* how, hipStream_t stream, bool conc = true);
// conc: the stage's score replay (one wave) and its regression (a wave per 64 shape coordinates) run side by side, where
// the model's workgroup has the waves for it (k_wide.hip: finish_wide_conc_ok) -- how->conc says whether it did

// What a k_stage launch over a level of `win`-pixel windows at `step` instantiates and how it is set up (k_stage.hip:
// stage_choice).  acc: the register width of the regression sums, the smallest of 12 / 32 / 64 / 160
// that holds dim; glb: the padded pixel tile of 16 x 16 windows exceeds pix_cap, pixels come through the caches
// (pix_bytes = 0); pitch: the tile's row pitch, a multiple of 16 and never of 128; chunk: carts staged in LDS at a
// time, 4..64 (0: not even four fit under lds_max, launch_stage refuses); lds_bytes: the launch's dynamic LDS.
struct StageChoice { int acc, chunk, pitch, pix_bytes, lds_bytes; bool glb; };
// Dense mode: stage t for every window of one level, a 16 x 8 tile of windows per workgroup.
// pix_cap = largest pixel tile that may live in LDS (larger windows read the frame through L1/L2).
// how (never null): the choice the launch used, acc and glb as the instantiation it picked has them.
template <typename Real>
hipError_t launch_stage(bool trace, int level, int t, bool apply_final_th, Real final_th, const DevPlan* d_plan,
                        const DevPlan& h_plan, const DevModelT<Real>& m, const WorkT<Real>& w, int pix_cap,
                        int lds_max, StageChoice* how, hipStream_t stream);
size_t stage_lds_bytes(int dim, int node_n, int leaf_n, int real_bytes);
// The launcher asks this, and so does jdaStageLaunchFor, which answers without a device.
StageChoice stage_choice(int win, int step, int dim, int node_n, int leaf_n, int K, int real_bytes, int pix_cap, int lds_max);
// Dense mode takes the model at all (Pass::dense_ok's part that depends on the model alone): at most 160 shape
// coordinates and 256 leaves, and the LDS floor -- a 4-cart chunk without a pixel tile -- within lds_max.  *pix_cap:
// min(pix_max, what the floor leaves of lds_max), the largest pixel tile a launch may put in LDS.
bool stage_model_ok(int dim, int node_n, int leaf_n, int real_bytes, int pix_max, int lds_max, int* pix_cap);

// Device -> mapped pinned host memory by a kernel on `stream` (instead of the copy engine): up to 4 segments, 16-byte
// aligned.
hipError_t launch_copy_out(const void* const* src, void* const* dst, const size_t* bytes, int n, hipStream_t stream);

// Per-frame post-processing of a dialect-C pass on the device (k_post.hip): scan order, score order, NMS, relocation --
// one workgroup per frame, results into mapped pinned host memory.  n[f] = detections kept for frame f of the pass
// (-1: the kernel declined, flag[0] = 1: the host post-processes the pass from its raw detections), first[f] = their first
// row in bb (x, y, size) / score / shape (dim floats, relocated); rows are allotted from *cursor (device, zeroed
// with the counters).
struct PostOut {
  int* n; int* first; int* bb; float* score; float* shape; int* flag;
  unsigned long long* cursor;
  unsigned cap_rows;
};
// rag_gid / rag_img: a ragged pass (first gid of every image, n + 1 entries; the images' sizes), else null.
hipError_t launch_post(const DevPlan* d_plan, const WorkT<float>& w, int dim, int n_frames, bool do_nms, float overlap,
                       const PostOut& o, hipStream_t stream, const uint32_t* rag_gid = nullptr, const RagImg* rag_img = nullptr);

template <typename Real>
hipError_t launch_trace_fill(const DevModelT<Real>& m, const WorkT<Real>& w, unsigned n_windows,
                             hipStream_t stream);

// ---- dialect CPP's Validate on caller crops and the hard-negative mining walk (k_mine.hip, mine.cpp) -----------------

// The model as Validate reads it (cascador.cpp:166-211): raw node offsets (the similarity parameter is applied per window),
// unpadded tables, Validate's own loop bounds -- `full` complete stages, then carts [0, part) of stage `full` without its
// regression (a trainer snapshot; part = 0 for a complete model).
struct MineModel {
  int T, K, L, D, node_n, leaf_n, dim;
  int full, part;
  const NodeD* nodes;        // [T*K*node_n], offsets as stored
  const double* leaf;        // [T*K*leaf_n]
  const double* cth; const double* cmean; const double* cstd;   // [T*K]
  const double* w;           // [T][K*leaf_n][dim]
  const double* mean;        // [dim] as stored
};
// One background image of a mining job: d_base + off, w x h as stored (rows back to back); transform 0..7 of
// data.cpp:930-963 as bits (kMineSwap: transpose, kMineFlipX / kMineFlipY: mirror the stored x / y).
struct MineImg { unsigned long long off; int w, h, tf, pad; };
constexpr int kMineSwap = 1, kMineFlipX = 2, kMineFlipY = 4;
// Orientation code t in 0..7 (jdaMineNegativesCpp's transforms[], include/jda.h "frames in any orientation") -> its bits:
// turned pixel (u, v) is stored pixel (x, y) = swap ? (v, u) : (u, v), then x = w-1-x if FlipX, then y = h-1-y if FlipY.
// The ONE table of mine.cpp and turn.cpp.
constexpr int kTf[8] = {0, kMineSwap | kMineFlipY, kMineFlipX | kMineFlipY, kMineSwap | kMineFlipX, kMineFlipX,
                        kMineSwap | kMineFlipX | kMineFlipY, kMineFlipY, kMineSwap};   // data.cpp:930-963, see k_mine.hip
// One (image, level) of the enumeration: its windows are ordinals [first, first + nx*ny), row by row.
struct MineSeg { unsigned long long first; int image, win, step, nx; };
// One crop Validate runs on: (x, y, w, h) in the transformed image, key of its initial-shape draw.
struct MineItem { int image, x, y, w, h, pad; unsigned long long key; };
struct MineSizes { int os, hs, qs, mode; double shift; unsigned long long seed; };
// What a k_mine.hip launcher launched (`how` may be null), filled from the grid it handed to hipLaunchKernelGGL; launched =
// false: nothing to launch, hipSuccess.  saturated (launch_mine_sum): the grid stood at its cap, lanes stride over the range.
// Counted in one place (host.h: LaunchLog, jdaMineLaunches).
enum { kMineKScan = 0, kMineKItems = 1, kMineKPatches = 2, kMineKWalk = 3, kMineKSum = 4 };   // (= JDA_MINE_K_*, host.h checks)
struct MineLaunch { bool launched; int kernel; unsigned grid; bool saturated; };

// Stage-0 prefix of every window with ordinals [lo, hi): carts [0, carts0) with the pixels computed on demand from the
// background image (chain 0).  status[o - lo] = Validate's n of a window rejected there; survivors are appended to
// surv (their ordinals, unordered) through *n_surv, status 0.
hipError_t launch_mine_scan(const MineModel& m, const MineSizes& z, const uint8_t* base, const MineImg* imgs,
                            const MineSeg* segs, int n_segs, unsigned long long lo, unsigned long long hi, int carts0,
                            int* status, unsigned long long* surv, unsigned* n_surv, hipStream_t stream, MineLaunch* how = nullptr);
// Ordinals -> crops (image, x, y, win, win, key = ordinal).
hipError_t launch_mine_items(const MineSeg* segs, int n_segs, const unsigned long long* ords, int n, MineItem* items,
                             hipStream_t stream, MineLaunch* how = nullptr);
// The o / h / q patches of n crops (chain z.mode) at patches + i * pbytes: os^2, then hs^2, then qs^2 bytes.
hipError_t launch_mine_patches(const MineSizes& z, const uint8_t* base, const MineImg* imgs, const MineItem* items, int n,
                               uint8_t* patches, int pbytes, hipStream_t stream, MineLaunch* how = nullptr);
// Validate on the patches of n crops, a lane per crop: face[i], n[i], score[i], shape[i*dim ..] (also the walk's state);
// lbf / t1 / t2: per-crop scratch of K ints and 2 x dim doubles.
// init != nullptr: crop i starts from init[i*dim ..] instead of mean + its key's shift, and items is not read (reval.cpp).
hipError_t launch_mine_walk(const MineModel& m, const MineSizes& z, const MineItem* items, int n, const uint8_t* patches,
                            int pbytes, int similarity, uint8_t* face, int* carts_n, double* score, double* shape, int* lbf,
                            double* t1, double* t2, hipStream_t stream, const double* init = nullptr, MineLaunch* how = nullptr);
// Sum of status[0, n) over the rejected entries (status > 0): out[0] += count, out[1] += sum.
hipError_t launch_mine_sum(const int* status, unsigned long long n, unsigned long long* out, hipStream_t stream,
                           MineLaunch* how = nullptr);

// ---- dialect CPP: training one CART (k_train.hip, train.cpp; reference src/jda/cart.cpp:41-350, data.cpp:148-173) ----

// One pool feature: the fields of Feature (include/jda/common.hpp), jdaFeatureCpp's layout.
struct TrainFeat { int scale, lm1, lm2, pad; double o1x, o1y, o2x, o2y; };
// A sample set on the device: patches tight (o, h, q back to back per sample), shapes TRANSPOSED [2L][n] so that the
// lanes of a wave (lane = sample, the landmark wave-uniform) read neighbouring doubles.  stp: nullptr -- the identity
// STParameter -- or every sample's stp_mc as launch_stp writes it, five planes [5][n] (train_similarity, include/jda.h).
struct TrainSet { const uint8_t* patches; const double* shapes_t; int n, os, hs, qs; const double* stp; };
constexpr int kTrainBins = 511;          // value + 255, cart.cpp:197-198
// Per-feature ordered sums of the regression split (cart.cpp:321-334): left / right x, x*x, y, y*y and the counts.
struct TrainVar { double s[8]; int n_left, n_right, th, pad; };

// shapes [n][dim] -> [dim][n]
hipError_t launch_train_transpose(const double* in, int n, int dim, double* out, hipStream_t stream);
// DataSet::CalcSTParameters (data.cpp:131-146) over shapes_t [2L][n]: stp_mc = Calc(shape, mean), stp_cm = Calc(mean, shape) as
// planes [5][n] (scale, rot00, rot01, rot10, rot11; either may be null).  mean [2L] as stored; ms: 4 + 2L doubles of scratch
// (the mean shape's side of Calc, formed once).
hipError_t launch_stp(const double* shapes_t, int n, int L, const double* mean, double* ms, double* stp_mc, double* stp_cm,
                      hipStream_t stream);
// CalcFeatureValues: out[f * stride + j] = value of pool feature f on sample list[j] (list == nullptr: sample j), j < count.
hipError_t launch_train_values(const TrainSet& set, const int* list, int count, const TrainFeat* pool, int F, short* out,
                               size_t stride, hipStream_t stream);
// Per feature the 511-bin histogram of values[f][0, count): counts, and (weights != nullptr) the weights added IN LIST
// ORDER per bin.  out_w [F][511] doubles, out_c [F][511] ints.
hipError_t launch_train_hist(const short* values, size_t stride, int F, const int* list, int count, const double* weights,
                             double* out_w, int* out_c, hipStream_t stream);
// Regression split per feature: threshold = the kidx[f]-th smallest value (from the counts), then the eight sums over the
// list in order (samples with has_gt only).
hipError_t launch_train_var(const short* values, size_t stride, int F, const int* list, int count, const double* residual,
                            const uint8_t* has_gt, const int* counts, const int* kidx, TrainVar* out, hipStream_t stream);

// ---- dialect CPP: closing a stage (k_lbf.hip, stage.cpp; reference src/jda/btcart.cpp:255-292, 390-424) ----

// A stage's carts as k_lbf reads them: NodeD records (jdaFeatureCpp's fields with the landmark ids doubled, and the threshold),
// level-major: node i (1-based, children 2i and 2i + 1) of cart k, on level d = floor(log2 i), sits at
inline size_t lbf_node_at(int K, int k, int i, int d) { return (size_t)K * (((size_t)1 << d) - 1) + ((size_t)k << d) + ((size_t)i - ((size_t)1 << d)); }
constexpr int kSampleWaves = 4;          // samples (waves) of a workgroup at most, in the wave-per-sample kernels (cpp_wave.h)
// One chunk of a resident sample set (device pointers).  walk = 1: the carts are walked and lbf [n][K] is written;
// walk = 0: lbf is read.  w != nullptr: out_shapes [n][dim] = shapes + the K rows of w [K * 2^(D-1)][dim] in cart order.
// mean != nullptr (train_similarity, include/jda.h): the mean shape [dim] as stored -- every sample walks and updates under
// its own STParameter::Calc(shape, mean) (btcart.cpp:399, 422).
struct LbfArgs {
  const uint8_t* patches; const double* shapes; const NodeD* nodes; const double* w;
  int* lbf; double* out_shapes;
  int n, K, D, dim, os, hs, qs, walk;
  const double* mean;
};
struct WaveLaunch { int lds, waves, lds_bytes; };  // how a wave-per-sample kernel ran: staged in LDS (1) or from global memory (0), waves and LDS bytes per workgroup
// lds_budget: the LDS bytes a workgroup may take (at most the CU's 160 KB); where one sample's slice does not fit, the
// kernel reads everything from global memory.  how (never null): what was launched.
hipError_t launch_lbf(const LbfArgs& a, int lds_budget, WaveLaunch* how, hipStream_t stream);

// ---- dialect CPP: Validate on a resident sample set (k_reval.hip, reval.cpp; reference src/jda/cascador.cpp:166-211) ----
// One chunk of a resident sample set (device pointers): record i's patches at patches + i * (os*os + hs*hs + qs*qs), its start
// shape at start + i*dim; outputs face [n], carts_n [n], score [n], shape [n][dim] (also the walk's state where it runs
// from global memory) and the scratch lbf [n][K] (the same).  m: the mining tables (mine.cpp), Validate's loop bounds in them.
struct RevalArgs {
  MineModel m;
  const uint8_t* patches; const double* start;
  uint8_t* face; int* carts_n; double* score; double* shape; int* lbf;
  int n, os, hs, qs;
  int st;                      // 1: the similarity transform (train_similarity, include/jda.h), per full stage from the shape as it stands
};
// lds_budget and how (never null) as launch_lbf's.
hipError_t launch_reval(const RevalArgs& a, int lds_budget, WaveLaunch* how, hipStream_t stream);

// ---- dialect C: the cascade on caller-given windows (k_windows.hip, windows.cpp; reference c/jda.c:340-414, 471-472) ----
// One chunk of a caller's window list (device pointers): window i is windows[i] = (frame, x, y, size), validated by the host
// (inside its frame, frame inside [0, n_frames)).  Outputs by window index, any may be null: face [n], score [n], carts_n [n],
// hash [n], shapes [n][dim] (window-normalised), landmarks [n][dim] (relocated, c/jda.c:471-472).  half / quarter: the
// jdaBuildPyramid pair of every frame (multi-scale models only, null otherwise).  tile_win: windows up to this side walk from
// an LDS copy of their pixels (single-scale models; 0: every pixel is read from the frame).
struct WinArgs {
  const uint8_t* frames; size_t frame_stride; int n_frames, width, height;
  const uint8_t* half; size_t half_stride; int hw, hh;
  const uint8_t* quarter; size_t quarter_stride; int qw, qh;
  const int4* windows; int n;
  float th;
  uint8_t* face; float* score; int* carts_n; uint32_t* hash; float* shapes; float* landmarks;
  int tile_win;
};
// The largest window side whose pixels fit next to the walk's state within the finishing kernels' LDS budget
// (kFinishLdsPerGroup); 0: none does.
int windows_tile_limit(int dim, int K);
hipError_t launch_windows(const DevModelT<float>& m, const WinArgs& a, hipStream_t stream);

// ---- dialect CPP: a sample set from one cart to the next (k_gather.hip, boost.cpp; reference src/jda/data.cpp:319-410) ----
constexpr int kGatherSegs = 8;           // source segments of one launch at most
constexpr int kGatherWaves = 4;          // destination records (waves) of a workgroup per round of its grid-stride loop
// Records [first, first + n) of the source set (the concatenation of the caller's segments) at `base` (device), P bytes each.
struct GatherSeg { const uint8_t* base; long long first, n; };
struct GatherItem { int dst, src; };     // destination record <- source record (index into the source set)
// One launch: items[0 .. n_items), every item's src inside one of seg[0 .. n_segs) and its dst inside
// [dst_first, dst_first + dst_n); destination record r starts at dst + (r - dst_first) * P.  No alignment is assumed.
struct GatherArgs {
  GatherSeg seg[kGatherSegs]; int n_segs;
  const GatherItem* items; long long n_items;
  uint8_t* dst; long long dst_first, dst_n;
  int P;
};
hipError_t launch_gather(const GatherArgs& a, hipStream_t stream);

// ---- frames as they arrive: colour / pitched / cropped images -> dense 8-bit gray (k_pack.hip, frames.cpp, pack.cpp; include/jda.h) ----
constexpr uint32_t kGrayB = 1868, kGrayG = 9617, kGrayR = 4899;   // the Q14 weights of gray = (B * 1868 + G * 9617 + R * 4899 + 8192) >> 14 (frames.cpp: pack_weights; k_chips.hip)
constexpr int kPackBlock = 256;          // lanes of a workgroup: consecutive lanes take consecutive units
constexpr int kPackRounds = 4;           // units of a lane: a workgroup covers kPackBlock * kPackRounds consecutive units
// One image of a launch: w x h pixels of bpp bytes from src (the rectangle's first pixel; rows `pitch` bytes apart) to the w * h
// bytes at dst.  Its output is dealt in UNITS: nq runs of 16 bytes from dst's first 16-byte boundary on, then one unit per
// byte in front of that boundary (head, at most 15) and behind the last run (tail, at most 15).  first: the image's first unit
// in the launch.  w_lo / w_hi: low and high bytes of the three Q14 weights, in the pixel's byte order (0: bpp == 1, a copy).
struct PackImg {
  const uint8_t* src; uint8_t* dst;
  long long pitch, first, nq;
  int w, h, bpp, head, tail;
  uint32_t w_lo, w_hi;
  int pad;
};
static_assert(sizeof(PackImg) == 72, "PackImg is uploaded as it is");
// One launch of k_pack, k_turn, k_reduce or k_rotate: imgs[0 .. n) and total, the units (k_pack) or tiles of all of them.
// block_img[b]: k_pack -- the image that holds unit b * kPackBlock * kPackRounds (a lane walks on from there); the tile
// kernels -- the image of tile (workgroup) b.
template <typename Img>
struct FrameArgs { const Img* imgs; const int* block_img; int n; long long total; };
using PackArgs = FrameArgs<PackImg>;
hipError_t launch_pack(const PackArgs& a, hipStream_t stream);

// ---- frames in any orientation: the same, turned by one of the eight orientations (k_turn.hip, turn.cpp; include/jda.h) ----
constexpr int kTurnBlock = 256;          // lanes of a workgroup: one tile of one image
constexpr int kTurnTile = 64;            // a tile is at most kTurnTile x kTurnTile pixels of the TURNED image
constexpr int kTurnPitch = 68;           // bytes from one row of the LDS tile to the next (the bank reasoning)
// One image of a launch: the w x h pixels of bpp bytes from src (the rectangle's first pixel; rows `pitch` bytes apart), turned
// by tf (kMineSwap | kMineFlipX | kMineFlipY), to the tw * th bytes at dst (tw = swap ? h : w).  Its tiles are the launch's
// workgroups [first, first + ntu * ntv), row by row; tile column k covers the turned columns [64 k - off, 64 k - off + 64)
// inside [0, tw), off = dst & 15: on the turned row 0 -- and on every row where tw is a multiple of 16 -- a tile begins at a
// 16-byte boundary of dst.  w_lo / w_hi: PackImg's.  For k_reduce w x h is the REDUCED rectangle (w = rectangle width / f) --
// tiles, tf, off, ntu, ntv are those of the w x h image -- and f the factor: reduced pixel (i, j) is the rounded mean of the
// f x f source pixels from column i * f, row j * f of src on.  k_turn does not read f (the host fills it: 1).
struct TurnImg {
  const uint8_t* src; uint8_t* dst;
  long long pitch, first;
  int w, h, bpp, tf, ntu, ntv, off;
  uint32_t w_lo, w_hi;
  int f;
};
static_assert(sizeof(TurnImg) == 72, "TurnImg is uploaded as it is");
using TurnArgs = FrameArgs<TurnImg>;
hipError_t launch_turn(const TurnArgs& a, hipStream_t stream);

// ---- frames larger than the faces need: the same, reduced by an integer factor first (k_reduce.hip, reduce.cpp; include/jda.h) ----
constexpr int kReduceMax = 8;            // factors 1 .. kReduceMax
hipError_t launch_reduce(const TurnArgs& a, hipStream_t stream);   // (k_reduce.hip: the same records, f read)

// ---- frames whose faces are rolled: the same pack, rotated by any angle (k_rotate.hip, rotate.cpp; include/jda.h) ----
constexpr int kRotMaxSide = 32768;       // a rotated image is at most this wide and high
constexpr int kRotBox = 92;             // a tile's source box is at most kRotBox x kRotBox pixels (the covering proof)
constexpr int kRotPitch = 96;            // bytes from one row of the LDS box to the next: 24 dwords, a lane fills one
// One image of a launch: the w x h pixels of bpp bytes from src (the rectangle's first pixel; rows `pitch` bytes apart), rotated
// by the plan's (c, s) (jdaRotationPlan), to the tw * th bytes at dst.  Tiles, first, ntu, ntv and off as TurnImg's, of the
// tw x th image.  w_lo / w_hi: PackImg's.
struct RotImg {
  const uint8_t* src; uint8_t* dst;
  long long pitch, first;
  double c, s;
  int w, h, bpp, tw, th, ntu, ntv, off;
  uint32_t w_lo, w_hi;
};
static_assert(sizeof(RotImg) == 88, "RotImg is uploaded as it is");
using RotArgs = FrameArgs<RotImg>;
hipError_t launch_rotate(const RotArgs& a, hipStream_t stream);

// ---- faces as they leave: upright face chips cut from detections (k_chips.hip, chips.cpp; include/jda.h) ----
constexpr int kChipBlock = 256;          // lanes of a workgroup: consecutive lanes take consecutive units
// One face of a launch: M maps chip pixel centres to source pixels (sx = (m[0] * cu + m[1] * cv) + m[2], sy with m[3..5]),
// its source image and the sub-samples per axis.
struct ChipFace { double m[6]; int image; int n; };
static_assert(sizeof(ChipFace) == 56, "ChipFace is uploaded as it is");
// One source image: the WHOLE image (taps leave the rectangle, never the image); rgb: byte 0 of a colour pixel is red.
struct ChipImg { const uint8_t* data; long long pitch; int width, height, bpp, rgb; };
static_assert(sizeof(ChipImg) == 32, "ChipImg is uploaded as it is");
// One launch: n_faces chips of cw x ch pixels of cbpp (1 | 3) bytes back to back from dst.  The call's `bytes` output bytes are
// ONE run, dealt in UNITS like k_pack's: nq runs of 16 bytes from dst's first 16-byte boundary on, then one unit per byte in
// front of that boundary (head, at most 15) and behind the last run (tail, at most 15).  A chip of 45 bytes begins anywhere
// inside a unit.
struct ChipArgs {
  const ChipFace* faces; const ChipImg* imgs; uint8_t* dst;
  long long bytes, nq;
  int head, tail, n_faces, n_images, cw, ch, cbpp, crgb;
};
hipError_t launch_chips(const ChipArgs& a, hipStream_t stream);

// ---- dialect CPP: the positive sample set (k_faces.hip, faces.cpp; reference src/jda/data.cpp:542-565, 623-640) ----
// One face of a launch: its image (d_base + off, W x H, rows back to back), its box (x, y, w, h) -- which may leave the
// image: getFace pads with black -- and the destination record of its o / h / q patches.
struct FaceItem { unsigned long long off; int W, H, x, y, w, h; long long rec; };
// One launch: workgroup i builds items[i]; record r starts at dst + r * P, P = os*os + hs*hs + qs*qs (no alignment is
// assumed).  mirror > 0: the horizontal mirror of every patch (cv::flip(patch, 1)) goes to record rec + mirror as well.
// [dst, dst + dst_n * P) is what the launch may write (checked in the bounds build).
struct FacesArgs {
  const uint8_t* base; const FaceItem* items; int n;
  uint8_t* dst; long long dst_n, mirror;
  int os, hs, qs;
};
hipError_t launch_faces(const FacesArgs& a, hipStream_t stream);

// ---- dialect CPP: a stage's global regression (k_fit.hip, fit.cpp; reference src/jda/btcart.cpp:328-388) ----
// What a coordinate's fit carries from one epoch (launch) to the next; `done` set: the coordinate's wave returns at once.
struct FitState { double gnorm_init, gnorm_last; int iters, done; };
constexpr int kFitPrefetch = 4;          // samples whose rows of lbf are in registers ahead of the one being stepped
constexpr int kFitMaxRounds = 16;        // rounds of 64 carts (K <= 1024) whose gathered weights stay in registers for the scatter;
                                         // beyond, the scatter reads the weights again
// One epoch of every coordinate that has not stopped (device pointers).  lbf [n_rows][K] and y [dim][n_rows] are only
// read; index [n_rows] is this epoch's order; beta [dim][n_rows], w [dim][f] (the weights TRANSPOSED) and state [dim] are
// read and written, launch after launch.
struct FitArgs {
  const int* lbf; const double* y; const int* index;
  double* beta; double* w; FitState* state;
  int n_rows, K, f, dim;
  double lambda, H, eps;
};
struct FitLaunch { int lds, lds_bytes; };   // how it ran: the coordinate's column of w in LDS (1) or in global memory (0)
// plan_fit, once per call: where one column (f doubles) fits lds_budget -- the LDS bytes a workgroup may take -- the launches
// keep it in LDS (and the instantiation is told its dynamic LDS size), otherwise the same body works on the column in global
// memory.  launch_fit: one epoch as planned.
hipError_t plan_fit(const FitArgs& a, int lds_budget, FitLaunch* how);
hipError_t launch_fit(const FitArgs& a, const FitLaunch& how, hipStream_t stream);

// Hardware-queue probe (k_misc.hip): a one-wave spin of `ticks` wall-clock ticks (100 MHz) that leaves its end time in
// *out (mapped pinned host memory), and a kernel that leaves the time it ran.
hipError_t launch_hwq_spin(long long ticks, unsigned long long* out, hipStream_t stream);
hipError_t launch_hwq_stamp(unsigned long long* out, hipStream_t stream);

}  // namespace jda
