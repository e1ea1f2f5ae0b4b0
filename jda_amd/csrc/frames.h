// libjda.so, host side: what the frame entries share (include/jda.h: "frames as they arrive", "in any orientation", "larger
// than the faces need", "whose faces are rolled", "faces as they leave").  frames.cpp holds their one call path -- what a call
// is refused for, the device entry, the way back; pack.cpp, turn.cpp, reduce.cpp and rotate.cpp each hold one definition: the
// host loop of their kind and, where the kind has one, a face's way back; chips.cpp the face chips.
#pragma once
#include "host.h"

namespace jda {

// ---- one jdaPixels ----
// Everything the entries refuse about ONE jdaPixels (fail() says what, behind the prefix `img`), the rectangle resolved; bytes
// per pixel of a JDA_PIX_* (0: unknown); the Q14 weights of a colour pixel's bytes 0, 1, 2 and its gray value (include/jda.h)
struct PixelsOne { const uint8_t* src; long long pitch; int x, y, w, h, bpp, format; };   // src: the rectangle's first pixel
bool check_pixels(const std::string& img, const jdaPixels& p, PixelsOne* out);
int pixels_bpp(int format);
void pack_weights(int format, int w[3]);
inline uint8_t gray_of(const uint8_t* p, int bpp, const int w[3]) {
  return bpp == 1 ? p[0] : (uint8_t)((p[0] * w[0] + p[1] * w[1] + p[2] * w[2] + 8192) >> 14);
}

// ---- how a call transforms its images ----
// The entry that is calling and the caller's arrays.  What the kind reads: kPack nothing; kTurn orients (needed); kReduce
// factors (needed) and orients (NULL: every image upright -- but the way back needs them); kRotate degrees (needed).
enum FrameKind { kPack, kTurn, kReduce, kRotate };
struct FrameSpec {
  FrameKind kind; const int* orients; const int* factors; const double* degrees;
  static FrameSpec pack() { return {kPack, nullptr, nullptr, nullptr}; }
  static FrameSpec turn(const int* orients) { return {kTurn, orients, nullptr, nullptr}; }
  static FrameSpec reduce(const int* factors, const int* orients) { return {kReduce, orients, factors, nullptr}; }
  static FrameSpec rotate(const double* degrees) { return {kRotate, nullptr, nullptr, degrees}; }
};
// rw x rh: w x h reduced by f; tw x th: that, turned by tf (kMineSwap | kMineFlipX | kMineFlipY)
struct FrameSize { int rw, rh, tw, th; };
inline FrameSize frame_size(int w, int h, int f, int tf) {
  const int rw = w / f, rh = h / f;
  return (tf & kMineSwap) ? FrameSize{rw, rh, rh, rw} : FrameSize{rw, rh, rw, rh};
}
// One image of a call, rectangle resolved and transform resolved: every size anything downstream needs.
struct FrameOne {
  const uint8_t* src;                 // the rectangle's first pixel
  uint8_t* dst;                       // (pack side)
  long long pitch, npix;              // npix = tw * th, the bytes of dst
  int x, y, w, h, bpp, format;        // the rectangle
  FrameKind kind;                     // the spec's: kRotate -- the plan (c, s) takes w x h to tw x th; otherwise
  int orient, tf, f;                  // kTf[orient] turns the rw x rh rectangle, w x h reduced by f, to tw x th (orient 0, f 1: where the kind has none)
  int rw, rh, tw, th;                 // (kRotate: rw x rh = w x h)
  double c, s;
};
// The refusals about one image's transform, each in its one place: the orientation and the factor's range (behind the prefix
// `pre`), and frame_one -- spec and image i of a call -> the record (dst left alone); refuses, in this order, the
// orientation, the factor's range, a rectangle the factor leaves no pixel of, what the rotation's plan refuses.
bool check_orient(const std::string& pre, int orient);
bool check_factor(const std::string& pre, int factor);
bool frame_one(const std::string& img, const FrameSpec& spec, int i, const PixelsOne& r, FrameOne* out);

// ---- the pack entries: jdaPackGray[Oriented|Reduced|Rotated] and their Device forms ----
int frames_host(const FrameSpec& spec, const jdaPixels* images, int n, unsigned char* dst, const size_t* dst_offsets);
int frames_device(Cascador* c, const FrameSpec& spec, const jdaPixels* images, int n, unsigned char* d_dst, const size_t* dst_offsets,
                  hipStream_t user_stream, jdaPackStats* stats);
// ... and the definition of each kind in plain loops over host memory, on images the call path has passed
void pack_write(const std::vector<FrameOne>& v);      // pack.cpp
void turn_write(const std::vector<FrameOne>& v);      // turn.cpp
void reduce_write(const std::vector<FrameOne>& v);    // reduce.cpp
void rotate_write(const std::vector<FrameOne>& v);    // rotate.cpp

// ---- the way back: jdaOrientBack, jdaReduceBack (spec.kind kReduce), jdaRotateBack ----
struct BackCall {
  const jdaPixels* images; int n_images; const int* face_image; int n_faces; int* boxes; int box_ints;
  void* landmarks; int real_bytes, landmark_n; const int* left; const int* right; int sym_n;
};
int frames_back(const FrameSpec& spec, const BackCall& call);
// ... and one face of a valid call, its box and landmarks taken into the whole source image o
void turn_back_face(const BackCall& call, int face, const FrameOne& o);     // turn.cpp: turned, reduced
void rotate_back_face(const BackCall& call, int face, const FrameOne& o);   // rotate.cpp

// ---- the sizes on their own: jdaOrientSize, jdaReduceSize, jdaRotationPlan ----
int orient_size(int w, int h, int orient, int* tw, int* th);
int reduce_size(int w, int h, int factor, int orient, int* rw, int* rh);
bool rotation_plan(const std::string& who, int w, int h, double degrees, jdaRotation* rot);   // false after fail()

// ---- faces as they leave (chips.cpp): jdaFaceChips / jdaFaceChipsDevice ----
struct ChipsCall {
  const jdaPixels* images; int n_images; const int* face_image; const void* landmarks; int real_bytes, n_faces, landmark_n;
  const double* tmpl; const unsigned char* use; int chip_w, chip_h, chip_format, supersample; unsigned char* dst; double* matrices;
};
int chips_host(const ChipsCall& call);
int chips_device(Cascador* c, const ChipsCall& call, hipStream_t user_stream, jdaChipStats* stats);

// ---- k_pack's and k_chips' destinations ----
// The units of `bytes` bytes at dst (kernels.h: PackImg, ChipArgs): bytes in front of dst's first 16-byte boundary, runs of 16, bytes behind
struct DstUnits { int head; long long nq; int tail; long long total() const { return nq + head + tail; } };
inline DstUnits dst_units(const void* dst, long long bytes) {
  DstUnits u;
  u.head = (int)std::min<long long>(bytes, (long long)((0 - (uintptr_t)dst) & 15));
  u.nq = (bytes - u.head) >> 4;
  u.tail = (int)(bytes - u.head - (u.nq << 4));
  return u;
}

}  // namespace jda
