// libjda.so, host side: one step of dialect CPP's boosting loop between two carts (reference src/jda/btcart.cpp:146-253 with
// src/jda/data.cpp:255-448) -- the scores after a cart, the reference's own quicksort as an index list, threshold and cut,
// the weights (jdaBoostScoresCpp, jdaSampleOrderCpp, jdaScoreThresholdCpp, jdaScoreCutCpp, jdaUpdateWeightsCpp,
// jdaGatherRowsCpp: plain fp64 arithmetic on caller arrays in the reference's order, no cascador, no GPU) and the move of
// the surviving samples' patch bytes into the new order on the kernel of k_gather.hip (jdaGatherSamplesCpp).  The loop, its
// restart policy, mining and the model stay with the caller.
#include <climits>
#include <cmath>

#include "detect.h"

namespace jda {

namespace {

// ---- the device entry ------------------------------------------------------------------------------------------------

struct GatherCall {
  Cascador* c;
  const jdaGatherSegCpp* segs;
  int n_segs;
  size_t P;
  const int* index;
  int keep;
  unsigned char* dst;
  bool dst_dev;
  jdaGatherStatsCpp* stats;
  long long first[kGatherSegs + 1];     // first[s]: segment s's first record in the source set; first[n_segs]: the total
};

bool ranges_overlap(const void* a, size_t an, const void* b, size_t bn) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return an > 0 && bn > 0 && a0 < b0 + bn && b0 < a0 + an;
}

// Everything that can be refused, before the device is touched.
bool check_gather(GatherCall& x, int os, int hs, int qs) {
  if (!x.c || !x.segs) { fail("bad arguments"); return false; }
  if (x.n_segs < 1 || x.n_segs > kGatherSegs) { fail("n_segs must be in [1, " + std::to_string(kGatherSegs) + "]"); return false; }
  if (!check_patch_sizes(os, hs, qs)) return false;
  x.P = (size_t)os * os + (size_t)hs * hs + (size_t)qs * qs;
  if (x.keep < 0) { fail("keep must not be negative"); return false; }
  long long total = 0;
  for (int s = 0; s < x.n_segs; s++) {
    x.first[s] = total;
    if (x.segs[s].n < 0) { fail("segment " + std::to_string(s) + ": n must not be negative"); return false; }
    if (x.segs[s].n > 0 && !x.segs[s].patches) { fail("segment " + std::to_string(s) + ": patches is null"); return false; }
    total += x.segs[s].n;
  }
  x.first[x.n_segs] = total;
  if (total > INT_MAX) { fail("more than INT_MAX records in all"); return false; }
  if (x.keep == 0) return true;
  if (!x.index || !x.dst) { fail("bad arguments: index and dst must be given"); return false; }
  for (int i = 0; i < x.keep; i++)
    if (x.index[i] < 0 || x.index[i] >= total) {
      fail("index[" + std::to_string(i) + "] = " + std::to_string(x.index[i]) + " is outside [0, " + std::to_string(total) + ")");
      return false;
    }
  for (int s = 0; s < x.n_segs; s++)
    if ((x.segs[s].on_device != 0) == x.dst_dev && ranges_overlap(x.dst, (size_t)x.keep * x.P, x.segs[s].patches, (size_t)x.segs[s].n * x.P)) {
      fail("dst overlaps segment " + std::to_string(s) + ": gather into another buffer"); return false;
    }
  return true;
}

int seg_of(const GatherCall& x, int idx) {
  int s = 0;
  while (idx >= x.first[s + 1]) s++;
  return s;
}

bool run_gather(GatherCall& x) {
  const double t0 = now_ms();
  Cascador* c = x.c;
  const size_t P = x.P;
  const int keep = x.keep;
  double upload_ms = 0, device_ms = 0, download_ms = 0;
  int chunks = 0, launches = 0;

  // What passes through the workspace: chunks of the host segments (dst on the device) or of dst (dst on the host, where
  // a host record is a host copy and only device records go through the kernel).
  const size_t budget = (size_t)std::max<long long>(1, c->kn.workspace_mb) << 20;
  const size_t fixed = (size_t)keep * sizeof(GatherItem) + 4096;
  const size_t room = budget > fixed ? budget - fixed : 0;
  long long most = 0;                                    // the most records a staged chunk can be asked to hold
  if (x.dst_dev) { for (int s = 0; s < x.n_segs; s++) if (!x.segs[s].on_device) most = std::max<long long>(most, x.segs[s].n); }
  else most = keep;
  const long long nc = std::max<long long>(1, std::min<long long>(most, (long long)(room / P)));

  // group 0: items with a device source, in dst order; group 1 + k: items whose source lies in chunk k of the host segments
  std::vector<long long> chunk0(x.n_segs + 1, 0);        // a host segment's first chunk number
  for (int s = 0; s < x.n_segs; s++)
    chunk0[s + 1] = chunk0[s] + (x.dst_dev && !x.segs[s].on_device ? (x.segs[s].n + nc - 1) / nc : 0);
  const size_t groups = 1 + (size_t)chunk0[x.n_segs];
  std::vector<long long> start(groups + 1, 0);
  std::vector<int> group_of(keep);
  for (int i = 0; i < keep; i++) {
    const int s = seg_of(x, x.index[i]);
    long long g = 0;
    if (!x.segs[s].on_device) {
      if (x.dst_dev) g = 1 + chunk0[s] + (x.index[i] - x.first[s]) / nc;
      else { std::memcpy(x.dst + (size_t)i * P, x.segs[s].patches + (size_t)(x.index[i] - x.first[s]) * P, P); g = -1; }
    }
    group_of[i] = (int)g;
    if (g >= 0) start[g + 1]++;
  }
  for (size_t g = 0; g < groups; g++) start[g + 1] += start[g];
  const long long n_items = start[groups];
  if (n_items == 0) {                                    // host to host only
    if (x.stats) { x.stats->call_ms = now_ms() - t0; x.stats->bytes = (long long)keep * (long long)P; }
    return true;
  }
  std::vector<GatherItem> items((size_t)n_items);
  {
    std::vector<long long> at(start.begin(), start.end() - 1);
    for (int i = 0; i < keep; i++) if (group_of[i] >= 0) items[(size_t)at[group_of[i]]++] = GatherItem{i, x.index[i]};
  }

  OneLane one(c);
  if (!one.open()) return false;
  hipStream_t st = one.stream;
  const bool staged = !x.dst_dev || groups > 1;
  CallBuf buf;
  GatherItem* d_items; uint8_t* d_stage;
  if (!carve_into(buf, [&](Carver& cv) {
        d_items = cv.take<GatherItem>((size_t)n_items);
        d_stage = staged ? cv.take<uint8_t>((size_t)nc * P) : nullptr;
      })) return false;
  EvTimer timer;
  if (!timer.open(x.stats)) return false;

  double t = now_ms();
  JDA_HIP(hipMemcpyAsync(d_items, items.data(), (size_t)n_items * sizeof(GatherItem), hipMemcpyHostToDevice, st));
  JDA_HIP(hipStreamSynchronize(st));
  upload_ms += now_ms() - t;

  auto launch = [&](GatherArgs& a) -> bool {
    if (!timer.begin(st)) return false;
    JDA_HIP(launch_gather(a, st));
    if (!timer.end(st)) return false;
    JDA_HIP(hipStreamSynchronize(st));
    if (!timer.add(&device_ms)) return false;
    launches++;
    return true;
  };
  GatherArgs dev{};                                      // the device segments, read in place
  for (int s = 0; s < x.n_segs; s++)
    if (x.segs[s].on_device && x.segs[s].n > 0) dev.seg[dev.n_segs++] = GatherSeg{x.segs[s].patches, x.first[s], x.segs[s].n};
  dev.P = (int)P;

  if (x.dst_dev) {
    if (start[1] > 0) {
      GatherArgs a = dev;
      a.items = d_items; a.n_items = start[1]; a.dst = x.dst; a.dst_first = 0; a.dst_n = keep;
      if (!launch(a)) return false;
    }
    for (int s = 0; s < x.n_segs; s++) {
      if (x.segs[s].on_device) continue;
      for (long long k = chunk0[s]; k < chunk0[s + 1]; k++) {
        const long long g = 1 + k, cnt = start[g + 1] - start[g];
        if (cnt == 0) continue;                          // nothing wants a record of this chunk
        const long long r0 = (k - chunk0[s]) * nc, rn = std::min<long long>(nc, x.segs[s].n - r0);
        t = now_ms();
        JDA_HIP(hipMemcpyAsync(d_stage, x.segs[s].patches + (size_t)r0 * P, (size_t)rn * P, hipMemcpyHostToDevice, st));
        JDA_HIP(hipStreamSynchronize(st));
        upload_ms += now_ms() - t;
        GatherArgs a{};
        a.seg[0] = GatherSeg{d_stage, x.first[s] + r0, rn}; a.n_segs = 1; a.P = (int)P;
        a.items = d_items + start[g]; a.n_items = cnt; a.dst = x.dst; a.dst_first = 0; a.dst_n = keep;
        if (!launch(a)) return false;
        chunks++;
      }
    }
  } else {
    // group 0 is in dst order: a chunk is a run of items whose dst records span at most nc records
    for (long long p = 0; p < n_items;) {
      const long long r0 = items[(size_t)p].dst;
      long long q = p;
      while (q < n_items && items[(size_t)q].dst - r0 < nc) q++;
      const long long rn = items[(size_t)(q - 1)].dst - r0 + 1;
      GatherArgs a = dev;
      a.items = d_items + p; a.n_items = q - p; a.dst = d_stage; a.dst_first = r0; a.dst_n = rn;
      if (!launch(a)) return false;
      t = now_ms();
      for (long long i = p; i < q;) {                    // runs of consecutive dst records come back in one copy each
        long long j = i + 1;
        while (j < q && items[(size_t)j].dst == items[(size_t)(j - 1)].dst + 1) j++;
        const long long d0 = items[(size_t)i].dst;
        JDA_HIP(hipMemcpyAsync(x.dst + (size_t)d0 * P, d_stage + (size_t)(d0 - r0) * P, (size_t)(j - i) * P, hipMemcpyDeviceToHost, st));
        i = j;
      }
      JDA_HIP(hipStreamSynchronize(st));
      download_ms += now_ms() - t;
      chunks++;
      p = q;
    }
  }
  if (x.stats) {
    jdaGatherStatsCpp& o = *x.stats;
    o.call_ms = now_ms() - t0; o.upload_ms = upload_ms; o.device_ms = device_ms; o.download_ms = download_ms;
    o.bytes = (long long)keep * (long long)P; o.chunks = chunks; o.launches = launches;
  }
  return true;
}

// ---- DataSet::_QSort_ (data.cpp:385-410) on values and an index array ---------------------------------------------------

void qsort_ref(std::vector<double>& sc, int* order, int n) {
  std::vector<std::pair<int, int>> stack;
  stack.emplace_back(0, n - 1);
  while (!stack.empty()) {
    const int left = stack.back().first, right = stack.back().second;
    stack.pop_back();
    int i = left, j = right;
    const double t = sc[(size_t)(((long long)left + right) / 2)];
    do {
      while (sc[i] > t) i++;
      while (sc[j] < t) j--;
      if (i <= j) {
        std::swap(sc[i], sc[j]); std::swap(order[i], order[j]);
        i++; j--;
      }
    } while (i <= j);
    // the halves are disjoint: their order does not matter; the larger one waits, so the stack stays O(log n)
    const bool lo = left < j, hi = i < right;
    if (lo && hi) {
      if (j - left > right - i) { stack.emplace_back(left, j); stack.emplace_back(i, right); }
      else { stack.emplace_back(i, right); stack.emplace_back(left, j); }
    } else if (lo) stack.emplace_back(left, j);
    else if (hi) stack.emplace_back(i, right);
  }
}

}  // namespace
}  // namespace jda

using namespace jda;

extern "C" {

int jdaBoostScoresCpp(const double* cart_scores, int leaf_n, const int* pos_leaf, int pos_n, const int* neg_leaf, int neg_n,
                      int normalize, double* pos_scores, double* neg_scores, double* pos_last, double* neg_last, double* mean,
                      double* stddev) try {
  g_err.clear();
  if (pos_n < 0 || neg_n < 0 || leaf_n < 1 || !cart_scores || (pos_n > 0 && (!pos_leaf || !pos_scores || !pos_last)) ||
      (neg_n > 0 && (!neg_leaf || !neg_scores || !neg_last))) {
    fail("bad arguments"); return -1;
  }
  for (int i = 0; i < pos_n; i++)
    if (pos_leaf[i] < 0 || pos_leaf[i] >= leaf_n) { fail("pos_leaf[" + std::to_string(i) + "] is outside [0, leaf_n)"); return -1; }
  for (int i = 0; i < neg_n; i++)
    if (neg_leaf[i] < 0 || neg_leaf[i] >= leaf_n) { fail("neg_leaf[" + std::to_string(i) + "] is outside [0, leaf_n)"); return -1; }
  for (int i = 0; i < pos_n; i++) { pos_last[i] = pos_scores[i]; pos_scores[i] += cart_scores[pos_leaf[i]]; }      // data.cpp:313-314
  for (int i = 0; i < neg_n; i++) { neg_last[i] = neg_scores[i]; neg_scores[i] += cart_scores[neg_leaf[i]]; }
  double m = 0., sd = 1.;
  if (normalize) {
    for (int i = 0; i < pos_n; i++) m += pos_scores[i];                       // data.cpp:424-430
    for (int i = 0; i < neg_n; i++) m += neg_scores[i];
    m /= (double)((long long)pos_n + neg_n);
    double var = 0.;
    for (int i = 0; i < pos_n; i++) { const double v = pos_scores[i] - m; var += v * v; }      // data.cpp:432-440
    for (int i = 0; i < neg_n; i++) { const double v = neg_scores[i] - m; var += v * v; }
    var /= (double)((long long)pos_n + neg_n);
    sd = std::sqrt(var);
    for (int i = 0; i < pos_n; i++) pos_scores[i] = (pos_scores[i] - m) / sd;                  // data.cpp:446
    for (int i = 0; i < neg_n; i++) neg_scores[i] = (neg_scores[i] - m) / sd;
  }
  if (mean) *mean = m;
  if (stddev) *stddev = sd;
  return 0;
} JDA_ABI_CATCH(-1)

int jdaSampleOrderCpp(const double* scores, int n, int* order, double* sorted_scores) try {
  g_err.clear();
  if (n < 0) { fail("bad arguments: n is negative"); return -1; }
  if (n == 0) return 0;
  if (!scores || !order) { fail("bad arguments"); return -1; }
  for (int i = 0; i < n; i++)
    if (scores[i] != scores[i]) { fail("scores[" + std::to_string(i) + "] is NaN: the reference's quicksort would run off the array"); return -1; }
  std::vector<double> sc(scores, scores + n);
  for (int i = 0; i < n; i++) order[i] = i;
  qsort_ref(sc, order, n);
  if (sorted_scores) std::memcpy(sorted_scores, sc.data(), (size_t)n * sizeof(double));
  return 0;
} JDA_ABI_CATCH(-1)

int jdaScoreThresholdCpp(const double* sorted_scores, int n, int drop_n, double* th) try {
  g_err.clear();
  if (!sorted_scores || !th) { fail("bad arguments"); return -1; }
  if (n < 1) { fail("an empty set has no threshold"); return -1; }
  if (drop_n < 0) { fail("drop_n must not be negative"); return -1; }
  long long offset = (long long)n - 1 - drop_n;                               // data.cpp:342-344
  if (offset < 0) offset = 0;
  *th = sorted_scores[offset];
  return 0;
} JDA_ABI_CATCH(-1)

int jdaScoreCutCpp(const double* sorted_scores, int n, double th, int* keep, int* will_removed) try {
  g_err.clear();
  if (n < 0 || (n > 0 && !sorted_scores)) { fail("bad arguments"); return -1; }
  if (th != th) { fail("th is NaN"); return -1; }
  int offset = n - 1;
  while (offset >= 0 && sorted_scores[offset] < th) offset--;                 // data.cpp:352, 376
  if (keep) *keep = offset + 1;
  if (will_removed) *will_removed = n - 1 - offset;                           // data.cpp:377
  return 0;
} JDA_ABI_CATCH(-1)

int jdaUpdateWeightsCpp(const double* pos_scores, int pos_n, const double* neg_scores, int neg_n, double* pos_weights,
                        double* neg_weights) try {
  g_err.clear();
  if (pos_n < 0 || neg_n < 0 || (pos_n > 0 && (!pos_scores || !pos_weights)) || (neg_n > 0 && (!neg_scores || !neg_weights))) {
    fail("bad arguments"); return -1;
  }
  for (int i = 0; i < pos_n; i++) pos_weights[i] = std::exp(-1. * pos_scores[i]);      // data.cpp:256-263: flag * score
  for (int i = 0; i < neg_n; i++) neg_weights[i] = std::exp(1. * neg_scores[i]);
  double sum_pos_w = 0., sum_neg_w = 0.;
  for (int i = 0; i < pos_n; i++) sum_pos_w += pos_weights[i];                         // data.cpp:279-287
  for (int i = 0; i < neg_n; i++) sum_neg_w += neg_weights[i];
  const double sum_w = sum_pos_w + sum_neg_w;
  const double sum_w_ = 1. / sum_w;                                                    // data.cpp:291-292
  for (int i = 0; i < pos_n; i++) pos_weights[i] *= sum_w_;
  for (int i = 0; i < neg_n; i++) neg_weights[i] *= sum_w_;
  return 0;
} JDA_ABI_CATCH(-1)

int jdaGatherRowsCpp(const void* const* rows, const int* rows_n, int n_segs, size_t row_bytes, const int* index, int keep,
                     void* dst) try {
  g_err.clear();
  if (!rows || !rows_n || keep < 0 || row_bytes == 0) { fail("bad arguments"); return -1; }
  if (n_segs < 1 || n_segs > kGatherSegs) { fail("n_segs must be in [1, " + std::to_string(kGatherSegs) + "]"); return -1; }
  long long first[kGatherSegs + 1];
  long long total = 0;
  for (int s = 0; s < n_segs; s++) {
    first[s] = total;
    if (rows_n[s] < 0) { fail("segment " + std::to_string(s) + ": rows_n must not be negative"); return -1; }
    if (rows_n[s] > 0 && !rows[s]) { fail("segment " + std::to_string(s) + ": rows is null"); return -1; }
    total += rows_n[s];
  }
  first[n_segs] = total;
  if (total > INT_MAX) { fail("more than INT_MAX rows in all"); return -1; }
  if (keep == 0) return 0;
  if (!index || !dst) { fail("bad arguments: index and dst must be given"); return -1; }
  for (int i = 0; i < keep; i++)
    if (index[i] < 0 || index[i] >= total) {
      fail("index[" + std::to_string(i) + "] = " + std::to_string(index[i]) + " is outside [0, " + std::to_string(total) + ")");
      return -1;
    }
  for (int s = 0; s < n_segs; s++)
    if (ranges_overlap(dst, (size_t)keep * row_bytes, rows[s], (size_t)rows_n[s] * row_bytes)) {
      fail("dst overlaps segment " + std::to_string(s)); return -1;
    }
  for (int i = 0; i < keep; i++) {
    int s = 0;
    while (index[i] >= first[s + 1]) s++;
    std::memcpy((unsigned char*)dst + (size_t)i * row_bytes, (const unsigned char*)rows[s] + (size_t)(index[i] - first[s]) * row_bytes, row_bytes);
  }
  return 0;
} JDA_ABI_CATCH(-1)

int jdaGatherSamplesCpp(void* cascador, const jdaGatherSegCpp* segs, int n_segs, int origin_size, int half_size, int quarter_size,
                        const int* index, int keep, unsigned char* dst, int dst_on_device, jdaGatherStatsCpp* stats) try {
  g_err.clear();
  if (stats) std::memset(stats, 0, sizeof *stats);
  GatherCall x{(Cascador*)cascador, segs, n_segs, 0, index, keep, dst, dst_on_device != 0, stats, {}};
  if (!check_gather(x, origin_size, half_size, quarter_size)) return -1;
  if (keep == 0) return 0;
  return run_gather(x) ? 0 : -1;
} JDA_ABI_CATCH_SYNC(-1)

}  // extern "C"
