// HIP kernel for gfx950 that builds the patches of dialect CPP's positive sample set (reference src/jda/data.cpp:542-565,
// 623-640: getFace, three cv::resize of the face, cv::flip of the three patches for face_augment_on).
//   k_faces  workgroup = face, lane = output pixel.  The face is never materialised: a pixel of getFace(image, bbox) is
//            the image's pixel at (x + bbox.x, y + bbox.y), or 0 where that lies outside the image (the reference's black
//            3 cols x 3 rows canvas, by coordinate test), handed to cv_resize_px as its pixel source -- the resize clamps
//            to the face's own w x h, not to the image.  Each of the o, h and q patches is a resize OF THE FACE
//            (data.cpp:630-632; mining's chain goes o -> h, o -> q instead).  Every output byte is computed once and stored
//            twice: at (x, y) of the face's record and, with augmentation, at (side - 1 - x, y) of the mirrored record
//            (data.cpp:638-640: the flip of the RESIZED patch, not a resize of the flipped face).
//            Records are P = o*o + h*h + q*q bytes apart from any base and P may be odd: all stores are byte stores,
//            consecutive lanes consecutive addresses (the mirrored ones descending within a patch row).  No LDS, no
//            atomics, no scratch; record offsets are 64-bit (2 * 10^5 records of 49,152 B are above 4 GB).
#include "cpp_patch.h"

namespace jda {

namespace {

// Row y of the face: the image row it lies on, or none
struct FaceRow {
  const uint8_t* row; int W, bx;
  Bc bc;
  __device__ __forceinline__ int operator()(int x) const {
    const int u = bx + x;
    if (!row || (unsigned)u >= (unsigned)W) return 0;
    JDA_BC_ADDR(bc, row + u, 1, kBcFacesSrc);
    return row[u];
  }
};

// Pixels of getFace(image, bbox) (data.cpp:542-565): the w x h box at (bx, by) of a W x H image, black outside the image.
struct FacePx {
  const uint8_t* img; int W, H, bx, by;
  Bc bc;
  __device__ __forceinline__ int operator()(int x, int y) const {
    const int u = bx + x, v = by + y;
    if ((unsigned)u >= (unsigned)W || (unsigned)v >= (unsigned)H) return 0;
    JDA_BC_ADDR(bc, img + (size_t)v * W + u, 1, kBcFacesSrc);
    return img[(size_t)v * W + u];
  }
};
__device__ __forceinline__ FaceRow row_of(const FacePx& f, int y) {
  const int v = f.by + y;
  return FaceRow{(unsigned)v < (unsigned)f.H ? f.img + (size_t)v * f.W : nullptr, f.W, f.bx, f.bc};
}

}  // namespace

__global__ __launch_bounds__(256) void k_faces(FacesArgs a) {
  const FaceItem it = a.items[blockIdx.x];
  const uint8_t* img = a.base + it.off;
  const FacePx face{img, it.W, it.H, it.x, it.y, Bc((long long)(uintptr_t)img, (long long)(uintptr_t)img + (long long)it.W * it.H)};
  const size_t P = (size_t)a.os * a.os + (size_t)a.hs * a.hs + (size_t)a.qs * a.qs;
  [[maybe_unused]] const Bc bc_dst((long long)(uintptr_t)a.dst, (long long)(uintptr_t)a.dst + a.dst_n * (long long)P);
  uint8_t* __restrict__ out = a.dst + (size_t)it.rec * P;
  uint8_t* __restrict__ flip = a.mirror > 0 ? a.dst + (size_t)(it.rec + a.mirror) * P : nullptr;
  int at = 0;                                            // the patch's first byte inside the record
  for (int s = 0; s < 3; s++) {
    const int side = s == 0 ? a.os : (s == 1 ? a.hs : a.qs);
    const CvResize r = cv_resize_make(it.w, it.h, side, side);
    for (int e = threadIdx.x; e < side * side; e += blockDim.x) {
      const int y = e / side, x = e - y * side;
      const uint8_t v = (uint8_t)cv_resize_px(face, r, x, y);
      JDA_BC_ADDR(bc_dst, out + at + e, 1, kBcFacesDst);
      out[at + e] = v;
      if (flip) {
        const int m = at + y * side + (side - 1 - x);
        JDA_BC_ADDR(bc_dst, flip + m, 1, kBcFacesDst);
        flip[m] = v;
      }
    }
    at += side * side;
  }
}

hipError_t launch_faces(const FacesArgs& a, hipStream_t stream) {
  if (a.n <= 0) return hipSuccess;
  if (!a.base || !a.items || !a.dst || a.dst_n < 1 || a.mirror < 0 || a.os < 1 || a.hs < 1 || a.qs < 1 || a.os > 128 || a.hs > 128 ||
      a.qs > 128) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_faces, dim3((unsigned)a.n), dim3(256), 0, stream, a);
  return hipGetLastError();
}

JDA_BC_READER(k_faces)

}  // namespace jda
