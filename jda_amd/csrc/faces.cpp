// libjda.so, host side: dialect CPP's positive sample set (reference src/jda/data.cpp:542-678, DataSet::LoadPositiveDataSet
// without its file and JPEG reading) -- the o / h / q patches of every face box on the kernel of k_faces.hip
// (jdaBuildPositivesCpp*), and the arithmetic that goes with them on caller arrays, no cascador, no GPU: ground-truth shapes,
// masks and the mean shape (jdaPositiveShapesCpp; data.cpp:589-598, 625-628, 641-661, CalcMeanShape 210-223), the initial
// shapes (jdaRandomShapesCpp; RandomShapes 237-253 on include/jda.h's generator) and the shape residual
// (jdaShapeResidualCpp; CalcShapeResidual 175-208 with the identity transform).
#include <climits>
#include <cmath>

#include "detect.h"
#include "splitmix.h"

namespace jda {

namespace {

struct FacesCall {
  Cascador* c;
  const unsigned char* const* host_imgs;     // host images, or
  const uint8_t* d_base; const size_t* offsets;      // ... images resident: image i at d_base + offsets[i]
  const int* widths; const int* heights; int n_images;
  const int* faces; int n;
  int os, hs, qs, augment;
  unsigned char* dst; bool dst_dev;
  jdaPositivesStatsCpp* stats;
  size_t P;
};

std::string face_str(const int* q) {
  return "(image, x, y, w, h) = (" + std::to_string(q[0]) + ", " + std::to_string(q[1]) + ", " + std::to_string(q[2]) + ", " +
         std::to_string(q[3]) + ", " + std::to_string(q[4]) + ")";
}

// Everything that can be refused, before the device is touched.
bool check_faces(FacesCall& x) {
  if (!x.c || x.n_images < 0 || x.n < 0) { fail("bad arguments"); return false; }
  if (!check_patch_sizes(x.os, x.hs, x.qs)) return false;
  x.P = (size_t)x.os * x.os + (size_t)x.hs * x.hs + (size_t)x.qs * x.qs;
  if (x.augment != 0 && x.augment != 1) { fail("augment must be 0 or 1"); return false; }
  if (x.n == 0) return true;
  if (!x.faces || !x.dst || !x.widths || !x.heights || (x.host_imgs ? false : (!x.d_base || !x.offsets))) {
    fail("bad arguments: faces, dst and the images must be given"); return false;
  }
  if ((long long)x.n * (x.augment ? 2 : 1) > INT_MAX) { fail("more than INT_MAX records in all"); return false; }
  for (int i = 0; i < x.n; i++) {
    const int* q = x.faces + 5 * i;
    if (q[0] < 0 || q[0] >= x.n_images) { fail("face " + std::to_string(i) + " " + face_str(q) + ": no such image"); return false; }
    const long long cols = x.widths[q[0]], rows = x.heights[q[0]];
    if (cols < 1 || rows < 1 || (x.host_imgs && !x.host_imgs[q[0]])) { fail("image " + std::to_string(q[0]) + " is null or has an empty size"); return false; }
    if (cols > INT_MAX / 4 || rows > INT_MAX / 4) { fail("image " + std::to_string(q[0]) + " is too large"); return false; }
    if (q[3] <= 0 || q[4] <= 0) { fail("face " + std::to_string(i) + " " + face_str(q) + ": w and h must be positive"); return false; }
    // getFace's canvas (data.cpp:551-564): 3 cols x 3 rows, the image at (cols / 2, rows / 2); OpenCV throws on a box that leaves it
    const long long cx = (long long)q[1] + cols / 2, cy = (long long)q[2] + rows / 2;
    if (cx < 0 || cy < 0 || cx + q[3] > 3 * cols || cy + q[4] > 3 * rows) {
      fail("face " + std::to_string(i) + " " + face_str(q) + " leaves getFace's padded canvas of its " + std::to_string(cols) + " x " +
           std::to_string(rows) + " image (3 cols x 3 rows, the image at (cols / 2, rows / 2))");
      return false;
    }
  }
  if (x.dst_dev && !x.host_imgs) {
    const uintptr_t d0 = (uintptr_t)x.dst, d1 = d0 + (size_t)x.n * (x.augment ? 2 : 1) * x.P;
    for (int i = 0; i < x.n; i++) {
      const int im = x.faces[5 * i];
      const uintptr_t s0 = (uintptr_t)x.d_base + x.offsets[im], s1 = s0 + (size_t)x.widths[im] * x.heights[im];
      if (d0 < s1 && s0 < d1) { fail("dst overlaps image " + std::to_string(im)); return false; }
    }
  }
  return true;
}

bool run_faces(FacesCall& x) {
  const double t0 = now_ms();
  Cascador* c = x.c;
  const size_t P = x.P;
  const int n = x.n, mult = x.augment ? 2 : 1;
  double upload_ms = 0, device_ms = 0, download_ms = 0;
  int chunks = 0, image_chunks = 0, images_uploaded = 0;

  // What passes through the workspace: the faces of a launch, chunks of the referenced host images, and for a host dst the
  // records of a launch.
  const size_t budget = (size_t)std::max<long long>(1, c->kn.workspace_mb) << 20;
  const size_t cap = std::max<size_t>(1, std::min<size_t>({(size_t)n, (size_t)65536, budget / 8 / sizeof(FaceItem)}));
  const size_t fixed = cap * sizeof(FaceItem) + 4096;
  const size_t room = budget > fixed ? budget - fixed : 0;
  const bool both = x.host_imgs && !x.dst_dev;
  const size_t img_room = both ? room / 2 : room, out_room = both ? room / 2 : room;
  const size_t nb_max = x.dst_dev ? cap : std::max<size_t>(1, std::min<size_t>(cap, out_room / (P * mult)));

  // chunks of the referenced images in index order, each within img_room (a chunk holds at least one image); resident
  // images are one chunk that needs no upload
  std::vector<int> chunk_of(x.n_images, -1);
  std::vector<size_t> off(x.n_images, 0);
  std::vector<std::vector<int>> chunk_imgs;
  size_t stage_bytes = 0;
  if (x.host_imgs) {
    std::vector<char> used(x.n_images, 0);
    for (int i = 0; i < n; i++) used[x.faces[5 * i]] = 1;
    size_t at = 0;
    for (int im = 0; im < x.n_images; im++) {
      if (!used[im]) continue;
      const size_t bytes = ((size_t)x.widths[im] * x.heights[im] + 255) & ~(size_t)255;
      if (chunk_imgs.empty() || (at > 0 && at + bytes > img_room)) { chunk_imgs.emplace_back(); at = 0; }
      chunk_of[im] = (int)chunk_imgs.size() - 1; off[im] = at;
      chunk_imgs.back().push_back(im);
      at += bytes;
      stage_bytes = std::max(stage_bytes, at);
    }
  } else {
    chunk_imgs.emplace_back();
    for (int im = 0; im < x.n_images; im++) { chunk_of[im] = 0; off[im] = x.offsets[im]; }
  }
  // the faces of every chunk, in face order
  std::vector<std::vector<int>> chunk_faces(chunk_imgs.size());
  for (int i = 0; i < n; i++) chunk_faces[chunk_of[x.faces[5 * i]]].push_back(i);

  OneLane one(c);
  if (!one.open()) return false;
  hipStream_t st = one.stream;
  CallBuf buf;
  FaceItem* d_items; uint8_t* d_imgs; uint8_t* d_stage;
  if (!carve_into(buf, [&](Carver& cv) {
        d_items = cv.take<FaceItem>(cap);
        d_imgs = x.host_imgs ? cv.take<uint8_t>(stage_bytes) : nullptr;
        d_stage = x.dst_dev ? nullptr : cv.take<uint8_t>(nb_max * mult * P);
      })) return false;
  EvTimer timer;
  if (!timer.open(x.stats)) return false;

  std::vector<FaceItem> items(cap);
  for (size_t k = 0; k < chunk_imgs.size(); k++) {
    const std::vector<int>& fl = chunk_faces[k];
    if (fl.empty()) continue;
    double t = now_ms();
    if (x.host_imgs) {
      for (int im : chunk_imgs[k])
        JDA_HIP(hipMemcpyAsync(d_imgs + off[im], x.host_imgs[im], (size_t)x.widths[im] * x.heights[im], hipMemcpyHostToDevice, st));
      image_chunks++; images_uploaded += (int)chunk_imgs[k].size();
    }
    for (size_t p = 0; p < fl.size(); p += nb_max) {
      const int nb = (int)std::min(nb_max, fl.size() - p);
      for (int j = 0; j < nb; j++) {
        const int i = fl[p + j];
        const int* q = x.faces + 5 * i;
        items[j] = FaceItem{(unsigned long long)off[q[0]], x.widths[q[0]], x.heights[q[0]], q[1], q[2], q[3], q[4], x.dst_dev ? (long long)i : (long long)j};
      }
      JDA_HIP(hipMemcpyAsync(d_items, items.data(), (size_t)nb * sizeof(FaceItem), hipMemcpyHostToDevice, st));
      JDA_HIP(hipStreamSynchronize(st));
      upload_ms += now_ms() - t;
      FacesArgs a{};
      a.base = x.host_imgs ? d_imgs : x.d_base; a.items = d_items; a.n = nb; a.os = x.os; a.hs = x.hs; a.qs = x.qs;
      if (x.dst_dev) { a.dst = x.dst; a.dst_n = (long long)n * mult; a.mirror = x.augment ? n : 0; }
      else { a.dst = d_stage; a.dst_n = (long long)nb * mult; a.mirror = x.augment ? nb : 0; }
      if (!timer.begin(st)) return false;
      JDA_HIP(launch_faces(a, st));
      if (!timer.end(st)) return false;
      t = now_ms();
      if (!x.dst_dev) {
        // runs of consecutive faces come back in one copy each (and one more for their mirrors)
        for (int i = 0; i < nb;) {
          int j = i + 1;
          while (j < nb && fl[p + j] == fl[p + j - 1] + 1) j++;
          const size_t f0 = (size_t)fl[p + i], cnt = (size_t)(j - i);
          JDA_HIP(hipMemcpyAsync(x.dst + f0 * P, d_stage + (size_t)i * P, cnt * P, hipMemcpyDeviceToHost, st));
          if (x.augment) JDA_HIP(hipMemcpyAsync(x.dst + ((size_t)n + f0) * P, d_stage + (size_t)(nb + i) * P, cnt * P, hipMemcpyDeviceToHost, st));
          i = j;
        }
      }
      JDA_HIP(hipStreamSynchronize(st));
      if (!x.dst_dev) download_ms += now_ms() - t;
      if (!timer.add(&device_ms)) return false;
      chunks++;
      t = now_ms();
    }
  }
  if (x.stats) {
    jdaPositivesStatsCpp& o = *x.stats;
    o.call_ms = now_ms() - t0; o.upload_ms = upload_ms; o.device_ms = device_ms; o.download_ms = download_ms;
    o.bytes = (long long)n * mult * (long long)P; o.image_chunks = image_chunks; o.images_uploaded = images_uploaded;
    o.chunks = chunks; o.launches = chunks;
  }
  return true;
}

int build_positives(FacesCall x) {
  if (x.stats) std::memset(x.stats, 0, sizeof *x.stats);
  if (!check_faces(x)) return -1;
  if (x.n == 0) return 0;
  return run_faces(x) ? 0 : -1;
}

// DataSet::CalcShapeResidual (data.cpp:175-208); stp_cm: null -- the identity transform, nothing is applied -- or size rows of
// (scale, rot00, rot01, rot10, rot11), row idx[i] applied to sample i's residual (data.cpp:185, 203; Apply: data.hpp:42-45).
int shape_residual(const double* gt_shapes, const double* cur_shapes, const int* shape_mask, int size, int landmark_n, const int* idx,
                   int n, int landmark_id, const double* stp_cm, double* residual, unsigned char* has_gt) {
  if (size < 0 || n < 0 || landmark_n < 1 || (n > 0 && (!gt_shapes || !cur_shapes || !idx))) { fail("bad arguments"); return -1; }
  if (landmark_id < -1 || landmark_id >= landmark_n) { fail("landmark_id must be -1 (all landmarks) or in [0, landmark_n)"); return -1; }
  if (has_gt && !shape_mask) { fail("bad arguments: has_gt needs shape_mask"); return -1; }
  for (int i = 0; i < n; i++)
    if (idx[i] < 0 || idx[i] >= size) { fail("idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " is outside [0, " + std::to_string(size) + ")"); return -1; }
  const size_t dim = 2 * (size_t)landmark_n;
  for (int i = 0; i < n; i++) {
    const double* g = gt_shapes + (size_t)idx[i] * dim;
    const double* s = cur_shapes + (size_t)idx[i] * dim;
    const double* p = stp_cm ? stp_cm + 5 * (size_t)idx[i] : nullptr;
    auto put = [&](double x, double y, double* out) {
      if (p) { out[0] = p[0] * (p[1] * x + p[2] * y); out[1] = p[0] * (p[3] * x + p[4] * y); }
      else { out[0] = x; out[1] = y; }
    };
    if (residual) {
      if (landmark_id < 0) for (size_t j = 0; j < dim; j += 2) put(g[j] - s[j], g[j + 1] - s[j + 1], residual + (size_t)i * dim + j);   // data.cpp:184-185
      else put(g[2 * landmark_id] - s[2 * landmark_id], g[2 * landmark_id + 1] - s[2 * landmark_id + 1], residual + 2 * (size_t)i);     // data.cpp:199-205
    }
    if (has_gt) has_gt[i] = shape_mask[idx[i]] > 0 ? 1 : 0;                                               // DataSet::HasGtShape
  }
  return 0;
}

}  // namespace
}  // namespace jda

using namespace jda;

extern "C" {

int jdaBuildPositivesCpp(void* cascador, const unsigned char* const* images, const int* widths, const int* heights, int n_images,
                         const int* faces, int n_faces, int origin_size, int half_size, int quarter_size, int augment,
                         unsigned char* dst, int dst_on_device, jdaPositivesStatsCpp* stats) try {
  g_err.clear();
  if (n_faces > 0 && !images) { fail("bad arguments: images is null"); return -1; }
  return build_positives(FacesCall{(Cascador*)cascador, images, nullptr, nullptr, widths, heights, n_images, faces, n_faces, origin_size,
                                   half_size, quarter_size, augment, dst, dst_on_device != 0, stats, 0});
} JDA_ABI_CATCH_SYNC(-1)

int jdaBuildPositivesCppDevice(void* cascador, const unsigned char* d_base, const size_t* offsets, const int* widths,
                               const int* heights, int n_images, const int* faces, int n_faces, int origin_size, int half_size,
                               int quarter_size, int augment, unsigned char* dst, int dst_on_device,
                               jdaPositivesStatsCpp* stats) try {
  g_err.clear();
  return build_positives(FacesCall{(Cascador*)cascador, nullptr, d_base, offsets, widths, heights, n_images, faces, n_faces, origin_size,
                                   half_size, quarter_size, augment, dst, dst_on_device != 0, stats, 0});
} JDA_ABI_CATCH_SYNC(-1)

int jdaPositiveShapesCpp(const int* faces, const double* landmarks, int n_faces, int landmark_n, int augment, const int* left,
                         const int* right, int sym_n, double* gt_shapes, int* shape_mask, double* mean_shape) try {
  g_err.clear();
  if (n_faces < 1) { fail("n_faces must be at least 1: CalcMeanShape reads sample 0"); return -1; }
  if (landmark_n < 1 || sym_n < 0 || !faces || !landmarks || !gt_shapes || !shape_mask || !mean_shape || (sym_n > 0 && (!left || !right))) {
    fail("bad arguments"); return -1;
  }
  if (augment != 0 && augment != 1) { fail("augment must be 0 or 1"); return -1; }
  if ((long long)n_faces * 2 > INT_MAX) { fail("more than INT_MAX samples in all"); return -1; }
  for (int j = 0; j < sym_n; j++)
    if (left[j] < 0 || left[j] >= landmark_n || right[j] < 0 || right[j] >= landmark_n) {
      fail("symmetric pair " + std::to_string(j) + " names a landmark outside [0, landmark_n)"); return -1;
    }
  for (int i = 0; i < n_faces; i++)
    if (faces[5 * i + 3] <= 0 || faces[5 * i + 4] <= 0) { fail("face " + std::to_string(i) + " " + face_str(faces + 5 * i) + ": w and h must be positive"); return -1; }
  const size_t dim = 2 * (size_t)landmark_n;
  const int n = n_faces, size = augment ? 2 * n : n;
  for (int i = 0; i < n; i++) {
    const int* q = faces + 5 * i;
    const double* raw = landmarks + (size_t)i * dim;
    double* g = gt_shapes + (size_t)i * dim;
    bool no_shape = true;                                                      // data.cpp:591-598
    for (size_t j = 0; j < dim; j++) if (raw[j] >= 0) no_shape = false;
    shape_mask[i] = no_shape ? -1 : 1;
    for (int j = 0; j < landmark_n; j++) {                                     // data.cpp:625-628
      g[2 * j] = (raw[2 * j] - q[1]) / q[3];
      g[2 * j + 1] = (raw[2 * j + 1] - q[2]) / q[4];
    }
    if (augment) {                                                             // data.cpp:641-661
      double* m = gt_shapes + (size_t)(i + n) * dim;
      for (size_t j = 0; j < dim; j++) m[j] = g[j];
      for (int j = 0; j < landmark_n; j++) m[2 * j] = 1 - m[2 * j];
      for (int j = 0; j < sym_n; j++) {
        const int idx1 = left[j], idx2 = right[j];
        const double x1 = m[2 * idx2], y1 = m[2 * idx2 + 1], x2 = m[2 * idx1], y2 = m[2 * idx1 + 1];
        m[2 * idx1] = x1; m[2 * idx1 + 1] = y1;
        m[2 * idx2] = x2; m[2 * idx2 + 1] = y2;
      }
      shape_mask[i + n] = shape_mask[i];
    }
  }
  // CalcMeanShape (data.cpp:210-223): sample 0 whatever its mask, valid_n counts from sample 1 on
  for (size_t j = 0; j < dim; j++) mean_shape[j] = gt_shapes[j];
  int valid_n = 0;
  for (int i = 1; i < size; i++) {
    if (!(shape_mask[i] > 0)) continue;
    const double* g = gt_shapes + (size_t)i * dim;
    for (size_t j = 0; j < dim; j++) mean_shape[j] += g[j];
    valid_n++;
  }
  const double r = 1. / (double)valid_n;                                       // Mat /= double: times the reciprocal, plus a zero shift
  for (size_t j = 0; j < dim; j++) mean_shape[j] = mean_shape[j] * r + 0.;
  return 0;
} JDA_ABI_CATCH(-1)

int jdaRandomShapesCpp(const double* mean_shape, int landmark_n, int n, double shift_size, uint64_t seed, uint64_t first_key,
                       double* shapes) try {
  g_err.clear();
  if (n < 0 || landmark_n < 1 || !mean_shape || (n > 0 && !shapes)) { fail("bad arguments"); return -1; }
  if (!(shift_size >= 0.) || !std::isfinite(shift_size)) { fail("shift_size must be finite and >= 0"); return -1; }
  const size_t dim = 2 * (size_t)landmark_n;
  for (int i = 0; i < n; i++) {
    const uint64_t key = first_key + (uint64_t)i;
    double x = 0., y = 0.;
    if (shift_size != 0.) {
      const double a = -shift_size, b = shift_size;                            // cv::RNG::uniform(a, b): a + (b - a) * u
      x = a + (b - a) * splitmix_unit(splitmix_draw(seed, 2ull * key));
      y = a + (b - a) * splitmix_unit(splitmix_draw(seed, 2ull * key + 1ull));
    }
    double* s = shapes + (size_t)i * dim;
    for (int j = 0; j < landmark_n; j++) {                                     // data.cpp:248-251
      s[2 * j] = mean_shape[2 * j] + x;
      s[2 * j + 1] = mean_shape[2 * j + 1] + y;
    }
  }
  return 0;
} JDA_ABI_CATCH(-1)

int jdaShapeResidualCpp(const double* gt_shapes, const double* cur_shapes, const int* shape_mask, int size, int landmark_n,
                        const int* idx, int n, int landmark_id, double* residual, unsigned char* has_gt) try {
  g_err.clear();
  return shape_residual(gt_shapes, cur_shapes, shape_mask, size, landmark_n, idx, n, landmark_id, nullptr, residual, has_gt);
} JDA_ABI_CATCH(-1)

int jdaShapeResidualStCpp(const double* gt_shapes, const double* cur_shapes, const int* shape_mask, int size, int landmark_n,
                          const int* idx, int n, int landmark_id, const double* stp_cm, double* residual, unsigned char* has_gt) try {
  g_err.clear();
  return shape_residual(gt_shapes, cur_shapes, shape_mask, size, landmark_n, idx, n, landmark_id, stp_cm, residual, has_gt);
} JDA_ABI_CATCH(-1)

}  // extern "C"
