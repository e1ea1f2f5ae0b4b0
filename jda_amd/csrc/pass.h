// libjda.so, host side: one sub-batch of frames through the device pipeline on one lane (Pass), and a submitted batch.
#pragma once
#include "host.h"

namespace jda {

// ---- the persistent scan's configuration, the parts that do not depend on the pass (k_scan_p.hip) ----
// Cart ranges (buckets), task forms, rings, workgroup size of a cascador's persistent scan launches; returns the carts
// it evaluates (the hand-off).
int scan_p_base_cfg(const Cascador* c, PScanCfg* cfg, int* block, int* wgs);
// Pixel-tile slots a persistent workgroup gets for tiles of cfg->slot_bytes, or 0 when the level is left to k_scan's closed
// tiles: fewer than scan_p_min_slots slots (few resident windows per wave) or too few tiles to keep the workgroups fed.
// capped: other kernels are in flight next to the pass (scan_p_slots).  The answer for "will it take the level at all" does
// not depend on `capped` (scan_p_slots >= scan_p_min_slots) -- ragged_build_chunk asks it ahead of the pass.
long long scan_p_slots_for(const Cascador* c, const PScanCfg& cfg_in, int K, int block, int wgs, long long n_tiles, bool capped);
// Will the persistent scan take a single-level launch of a ragged chunk (tiles of at most pix_bytes, n_tiles of them)?
bool scan_p_takes_ragged(const Cascador* c, int pix_bytes, long long n_tiles);

// What a driver (run_device, a submit ticket, a ragged slot) sets for a pass, once, before it is issued (Pass::open).
template <typename Real>
struct PassSetup {
  Cascador* c = nullptr; PlanEntry* pe = nullptr; const TraceOut<Real>* trace = nullptr; RawDets<Real>* dets = nullptr; RunStats* rs = nullptr;
  bool apply_th = true; Real th = 0; bool multi = false;   // multi: hm().multi_scale(), a scan of the model: computed once
  Lane* ln = nullptr; int lane = 0; bool solo = true;      // lane: index inside the call; solo: the only lane of this call
  hipStream_t stream = nullptr;                            // the caller's stream (null: the lane's own)
  bool want_post = false, post_nms = true; float post_overlap = 0.3f;   // the caller takes device-post-processed frames (RawDets::p_*)
  // frames [f0, f0 + nf) of the call's n_call frames, `stride` bytes apart from `frames` on (a ragged pass has none: rag)
  int f0 = 0, nf = 0, n_call = 0; const uint8_t* frames = nullptr; size_t stride = 0;
  const unsigned char* const* host_frames = nullptr; size_t host_fbytes = 0;   // frames of this sub-batch still on the host
  const RaggedChunk* rag = nullptr;   // ragged pass: images of different sizes
  // multi-scale models: room for the half / quarter images (or per-window patches of sides patch_hs / patch_qs), strides per frame
  uint8_t* hbuf = nullptr; size_t hs = 0; uint8_t* qbuf = nullptr; size_t qs = 0;
  int hw = 0, hh = 0, qw = 0, qh = 0, patch_hs = 0, patch_qs = 0;
};

// One sub-batch of frames going through the device pipeline on one lane (stream + workspace).
// A pass is ONE enqueue (issue_scan: scan, finishing launches, counters and a predicted prefix of the results) and ONE
// host wait (after_counters); only a pass without a prediction of its hand-off queue's length waits once more in
// between (after_tail).  The methods are the pieces between the waits, so that run_device can interleave two lanes:
// while one lane's latency-bound finishing kernels and host work run, the other lane's scan keeps the machine busy.
template <typename Real>
struct Pass {
  // ---- what open() set: the driver's PassSetup, the lane, the plan's hints, the scan's launch parameters ----
  Cascador* c = nullptr; PlanEntry* pe = nullptr; const TraceOut<Real>* trace = nullptr; RawDets<Real>* dets = nullptr; RunStats* rs = nullptr;
  bool apply_th = true; Real th = 0; bool multi = false;
  Lane* ln = nullptr; int lane = 0; bool solo = true;
  hipStream_t st = nullptr; hipEvent_t* ev = nullptr; unsigned long long* h_cnt = nullptr;
  bool timed = true;               // RunStats::timed
  bool want_post = false, post_nms = true; float post_overlap = 0.3f;
  int f0 = 0, nf = 0;
  const unsigned char* const* host_frames = nullptr; size_t host_fbytes = 0;   // (dropped by restart(): staged by then)
  const RaggedChunk* rag = nullptr;   // (w.segs / w.blk / w.img_off set by issue_scan_ragged)
  uint8_t* hbuf = nullptr; size_t hs = 0; uint8_t* qbuf = nullptr; size_t qs = 0;
  // the plan's hints as they stood when the pass was set up (the plan is shared with concurrent callers: read and
  // written under c->mu only, see open())
  bool hint_dense = false; double pred_tail = -1, pred_out = -1, pred_mid = -1;
  int busy_lanes = 1;               // lanes of the cascador in use when the pass was set up (concurrent callers)
  // the same for every stage-0 scan launch of the pass: uniform levels, merged closed tiles, ragged
  struct ScanArgs { int handoff = 0, cp_max = 0, opts = 0; } sa;
  WorkT<Real> w; size_t cap = 0;
  size_t cap_q = 0, cap_m = 0;     // entries of the hand-off queue / of the mid queue and the detection list (WorkT::cap_q, cap_m)

  // ---- one issue of the pass: a rerun starts from `at = Attempt{}` (restart()) ----
  struct Attempt {
    bool dense = false, finished = false, lds_span = false;
    bool predicted = false;          // the finishing launches were sized from PlanEntry::pred_tail, no host wait in between
    bool counters_issued = false, results_pending = false;
    int p_launches = 0;              // k_scan_p launches so far (each deals its tiles from its own counter words)
    bool post_issued = false, posted = false; size_t post_cap = 0;         // k_post queued / its results are good
    bool mid_direct = false;         // a scan launch put stage-0 survivors into the mid queue itself (k_scan_p up to cart K)
    long long n_tail = -1;
    size_t n_out = 0, out_copied = 0;   // detections of the pass / how many of them are already on their way to the host
    bool counted = false;            // after_counters has folded and tallied the counters
    int my_scan_launches = 0;        // scan launches counted into rs so far
  } at;

  // ---- what a rerun must NOT forget, and why a pass is issued again a bounded number of times only: no_scan_p is
  //      sticky, so recover_scan runs once (scan_persistent declines from then on, p_launches stays 0 and after_counters
  //      does not ask again); overflow_runs only grows, and the third recover_overflow takes the worst-case sizes.  A rerun
  //      also keeps the workspace it grew (w, cap*) and the prediction recover_overflow withdrew (pred_tail = -1). ----
  bool no_scan_p = false;          // started over without k_scan_p (recover_scan): its watchdog tripped or it covered too few windows
  int overflow_runs = 0;           // times issued again because a queue was too small (recover_overflow)

  // Takes the driver's settings, binds the lane and works out the scan's launch parameters: ready for issue_scan().
  void open(const PassSetup<Real>& s);
  // The pass starts over: what the attempt counted into rs is given back, and the frames are staged already.
  void restart() { rs->scan_launches -= at.my_scan_launches; at = Attempt{}; host_frames = nullptr; }
  // The lane's workspace has been carved again (grown): its array pointers replace the pass's, what the pass itself set
  // (frames, pyramid images, ragged tables) stays.
  void adopt_workspace();
  // Dense mode keeps per-window state in the mid-queue arrays (k_stage): every window needs an entry.
  bool grow_for_dense();
  // The lane's side stream next to the pass's own: it starts behind what the pass has queued so far (fork_side), the
  // end of its work is marked (side_done) and the pass's stream goes on behind that mark (join_side).
  bool fork_side() { JDA_HIP(hipEventRecord(ln->ev_side[0], st)); JDA_HIP(hipStreamWaitEvent(ln->side, ln->ev_side[0], 0)); return true; }
  bool side_done() { JDA_HIP(hipEventRecord(ln->ev_side[1], ln->side)); return true; }
  bool join_side() { JDA_HIP(hipStreamWaitEvent(st, ln->ev_side[1], 0)); return true; }
  // the rest of the pass once its scan is queued, for a driver that has nothing to interleave (tickets, ragged slots)
  bool complete() { return after_tail() && issue_counters() && after_counters() && collect(); }
  // A pass's own spans -> scan_ms, gpu_ms, scan_lds_ms (a driver with several lanes in flight takes the union of their
  // spans instead: run_device_impl)
  static float span_ms(hipEvent_t a, hipEvent_t b) { float ms = 0; return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f; }
  void tally_times(RunStats& to) const;

  const HostModel& hm() const { return c->hm; }
  const DevModelT<Real>& model() const { return Sel<Real>::model(c).m; }
  bool want_trace() const { return trace != nullptr; }
  // 64-cart groups walked per round by a window that is expected to pass whole stages: the count in
  // 2..4 that wastes the fewest speculative walks past cart K-1 (K = 540: 3 groups, 576 walks, not 768)
  int stage_groups() const;
  // resolved stage-0 tables for k_finish (A/B switch: JDA_FIN_S0=0)
  // k_finish reads the level-major copy of the stage-0 tables (second half of the allocation)
  const S0Node* s0_tbl() const { return (pe->fast_scan && pe->table && pe->lm_ok && c->kn.fin_s0) ? pe->table + pe->table_cap : nullptr; }
  const Knobs& kn() const { return c->kn; }
  // k_filter0 + k_finish(survivors) can take this pass's hand-off queue (every level has a resolved stage-0 table)
  bool filter0_ok() const { return kn().filter0 && s0_tbl() != nullptr && pe->fast_scan && !pe->any_untiled && !multi; }
  // ... and its survivors take their stage-0 leaves along to k_finish (WorkT::m_leaf; kernels.h: carry_pack)
  bool carry_ok() const { return kn().fin_carry && filter0_ok() && carry_fits(hm().leaf_n(), hm().K); }
  long long windows() const { return rag ? rag->windows : (long long)nf * pe->sp.windows; }
  // ---- the launch reports (host.h: LaunchLog): a pass counts the record its launcher filled, once the launcher has
  //      returned hipSuccess, and restates none of the launcher's decisions.  A pass that is issued again counts again. ----
  // the finishing form this pass is about to issue, where that is the pass's own decision (launch_finishers, run_dense)
  void count_form(int form) { c->log.count_form(form); }
  template <typename Record> hipError_t counted(hipError_t e, const Record& how) { if (e == hipSuccess) c->log.count(Sel<Real>::dialect, how); return e; }
  // A k_finish / k_filter0 launch of this pass.  wk: the workspace as the launch sees it (w, or launch_finishers' copy
  // without leaf words where the carry does not apply).
  hipError_t finish(const WorkT<Real>& wk, int t_begin, int t_end, int groups, long long n_hint, const S0Node* s0, int tile_win,
                    bool survivors = false) {
    FinishLaunch how;
    return counted(launch_finish<Real>(want_trace(), t_begin, t_end, apply_th, th, pe->dp, model(), wk, groups, n_hint, s0, tile_win, &how, st, survivors), how);
  }
  hipError_t filter0(const WorkT<Real>& wk, long long n_hint) {
    FinishLaunch how;
    return counted(launch_filter0<Real>(want_trace(), pe->dp, model(), wk, n_hint, s0_tbl(), &how, st), how);
  }
  // A scan launcher has returned hipSuccess: its record is counted, and so is the call -- jdaStats::scan_launches counts
  // the calls to a scan launcher, also one that found nothing to launch (no frame, no tile of the mode, no block).
  void count_scan(const ScanLaunch& how) { c->log.count(Sel<Real>::dialect, how); rs->scan_launches++; at.my_scan_launches++; }

  bool dense_ok(int* pix_cap, int* lds_max) const;
  bool run_dense();
  bool clear_counters();
  bool read_counter(int counter) {     // asynchronous: the value is in h_cnt[0] after the next stream sync
    // (the hand-off count comes with the counters up to the mid queue's: h_cnt[kCntMid - kCntTail] = windows k_scan_p
    // put there itself)
    const size_t n = counter == kCntTail ? (size_t)(kCntMid - kCntTail + 1) : 1;
    JDA_HIP(hipMemcpyAsync(h_cnt, w.counters + counter, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    return true;
  }

  // Host frames -> staging buffer, ahead of this pass on its stream.
  bool upload_frames(uint8_t* dst, size_t stride, const unsigned char* const* frames, int n, size_t fbytes);
  // The persistent form of an LDS-tiled level's scan (k_scan_p.hip): dialect C, no trace.  false = not applicable
  // (the caller launches k_scan).
  // rl: a launch of a ragged chunk (all of ONE level): its tiles come from the chunk's block map, re-cut per image
  // dry: only say whether the level would be taken (nothing is launched, no state changes)
  bool scan_persistent(int level, hipStream_t s, const RaggedChunk::Launch* rl = nullptr, bool dry = false);
  // step 1: pyramids (multi-scale models), stage-0 scan (or everything, in dense mode)
  bool issue_scan();
  // With a prediction of the hand-off queue's length (earlier passes on this plan) everything else is queued
  // right behind the scan: finishing launches sized by the prediction, counters and a predicted prefix of
  // the detections -> host.  The pass is then one enqueue and ONE host wait (after_counters).  Without one, the
  // host reads the queue length first (after_tail).
  bool issue_rest();
  // Ragged pass: tables and images -> device (tight rows repacked to the common pitch), then the scan launches of the
  // chunk's block map.  Never dense, never traced (the caller falls back to per-image passes for those).
  bool issue_scan_ragged();
  // Finishing launches for a hand-off queue of (about) n_grid windows: the kernels take the true length from the
  // device counter and stride over it, n_grid only sizes the grids.
  bool launch_finishers(long long n_grid);
  // step 2 (passes without a prediction): every survivor of the scan: remaining carts of stage 0 (+ all stages
  // when few are left)
  bool after_tail();
  // step 3: counters -> host (asynchronous)
  bool issue_counters();
  // k_post for this pass: at most `rows` detections kept in all
  bool issue_post(size_t rows);
  // detections [from, to) of the device list -> the lane's pinned host arrays (asynchronous)
  bool issue_results(size_t from, size_t to, bool with_counters = false);
  // step 4: statistics, (the rest of) the detections -> host (asynchronous)
  bool after_counters();
  // A recovery issues the whole pass again on the same lane, up to the point its caller (after_tail or after_counters)
  // had reached: counted, not yet collected.
  bool run_again();
  // The persistent scan of this pass gave up (watchdog) or came back short: nothing of the pass has been counted or
  // collected yet, so the whole pass is issued again on the same lane with k_scan's closed tiles, and the caller gets
  // correct results, a note on stderr and jdaStats::scan_fallbacks (the call itself succeeds: jdaGetLastError() stays
  // empty -- an empty result with a non-empty error string is jdaDetect's only failure signal).
  bool recover_scan(unsigned long long err, long long got, long long expect);
  // A queue of this pass was too small for what the scan (or a finishing kernel) kept: the kernels dropped what did not
  // fit and kept counting, so nothing of the pass is usable but its counts.  The workspace grows to them -- a queue
  // downstream of the one that overflowed has only seen a part of its input: its count is scaled up -- and the whole pass
  // is issued again on the same lane; a third attempt takes the worst-case sizes.  The caller gets correct results, a note
  // on stderr and jdaStats::ws_regrows; the plan's fractions are updated by the rerun, so the next pass is sized right.
  bool recover_overflow(unsigned long long tail, unsigned long long mid, unsigned long long out);
  // step 5: detections of this pass sorted back into scan order and appended; trace arrays
  bool collect();
};

struct PendingBatch {
  bool active = false;       // submitted, not yet collected
  bool reserved = false;     // a submit is filling this slot
  bool waiting = false;      // a Wait is collecting it
  Lane* lane = nullptr;      // held (busy) from Submit to the end of Wait
  Pass<float> pass;
  RawDets<float> dets;
  RunStats rs;
  PlanEntry* pe = nullptr;   // pinned from Submit to the end of Wait
  ScanPlan sp;
  int n = 0;
  bool opt_set = false;
  jdaDetectOptions opt{};
  double t_submit = 0;
  // host-frame submits: the H2D copy (blocking for pageable memory) and the scan launches run on a helper thread,
  // so that the submitting thread is free to collect the other ticket meanwhile
  std::thread issuer;
  std::vector<const unsigned char*> host_ptrs;   // the caller's frame pointers, copied at Submit (only the frame BYTES must stay valid until Wait)
  bool issue_ok = true;
  std::string issue_err;
  void join_issuer() { if (issuer.joinable()) issuer.join(); }
  void reset() {             // (keeps `reserved`; the issuer has been joined)
    lane = nullptr; pass = Pass<float>(); dets = RawDets<float>(); rs = RunStats(); pe = nullptr; sp = ScanPlan();
    n = 0; opt_set = false; opt = jdaDetectOptions{}; t_submit = 0; issue_ok = true; issue_err.clear();
  }
};

}  // namespace jda
