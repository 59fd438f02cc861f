// pre_source.h — a frame slot's SOURCE frame in the image pre-step (VioSource, include/vio_amd.h): the frame as delivered (size,
// row stride, pixel format, range, crop) and the arithmetic that makes the context's rows x cols gray image of it.
// Host- and device-callable like pre_rectify.h: clahe_lut_frames_kernel (vio_preprocess.hip), the host entries
// vio_source_check / vio_source_camera and the stand-alone host program of the tests (tests/emul/source_scale_main.cpp) compile
// this text, and all of them must give the same bytes.
//
// Gray of one source pixel: RGBA / BGRA (R*4899 + G*9617 + B*1868 + 8192) >> 14; GRAY8 / NV12 the byte itself, with range = 1
// mapped from video range by min(255, ((max(Y, 16) - 16) * 255 + 109) / 219).
// No lens: the exact area average of the crop. With gx = gcd(crop_cols, cols), cw = crop_cols / gx, ow = cols / gx, source
// column j covers [j * ow, (j + 1) * ow) and output column x covers [x * cw, (x + 1) * cw) of one axis of crop_cols * ow
// units; the weight wx(x, j) is the length of their overlap (an integer; the weights of one output column sum to cw). Rows
// likewise with ch, oh, wy. S = sum wy * wx * gray, D = cw * ch, out = (S + D / 2) / D: the nearest value, ties upward.
// 255 * D < 2^32 (vio_source_check) keeps S in 32 bits; the weights are separable and every partial sum is exact.
// A lens: s = min(4, max(ceil(src.cols / cols), ceil(src.rows / rows))) samples per axis at (x + (2 i + 1 - s) / (2 s),
// y + (2 j + 1 - s) / (2 s)), each through pre_rectify.h's arithmetic over the WHOLE delivered frame (the crop is not used),
// out = (sum + s * s / 2) / (s * s). With s = 1 that is pre::rectify_px. The lens is any of pre_rectify.h's (VioLens,
// VioLensModel, LensAs<MODEL>).
// The valid region of a slot (which output pixels are made of delivered pixels only: lens_inside, lens_inside_source,
// valid_region below) is this arithmetic without the clamp; valid_region_kernel, vio_lens_model_valid_region and
// tests/emul/valid_region_main.cpp compile it.
#pragma once
#include "pre_rectify.h"

namespace pre {

// What the kernel needs of a VioSource, derived once on the host (source_plan).
struct SourcePlan {
  int32_t bpp, video;        // bytes per pixel of plane 0 (1 | 4); 1: the video-range map applies
  uint32_t c0, c2;           // 4-byte formats: the gray coefficients of byte 0 and byte 2 (R and B, or B and R)
  int32_t rows, cols, stride;
  int32_t crop_x, crop_y;
  int32_t cw, ow, ch, oh;    // the reduced ratios crop_cols : cols and crop_rows : rows
  int32_t s;                 // samples per axis of a lensed slot
};

VIO_PRE_HD uint32_t video_range(uint32_t y) {
  const uint32_t t = y > 16u ? y - 16u : 0u;
  const uint32_t v = (t * 255u + 109u) / 219u;
  return v > 255u ? 255u : v;
}

// gray of pixel x of a source row (4-byte formats: the row is 4-byte aligned)
template <int BPP, bool VIDEO>
VIO_PRE_HD uint32_t source_gray(const uint8_t *row, int x, uint32_t c0, uint32_t c2) {
  if (BPP == 4) {
    const uint32_t px = *reinterpret_cast<const uint32_t *>(row + 4 * (size_t)x);  // little endian: byte 0 is the low one
    return ((px & 0xff) * c0 + ((px >> 8) & 0xff) * 9617u + ((px >> 16) & 0xff) * c2 + 8192u) >> 14;
  }
  return VIDEO ? video_range(row[x]) : (uint32_t)row[x];
}

// One axis of the area average; c = crop / gcd, o = out / gcd. Source indices [area_first, area_end) overlap output index x.
VIO_PRE_HD int area_first(int x, int c, int o) { return (x * c) / o; }
VIO_PRE_HD int area_end(int x, int c, int o) { return ((x + 1) * c + o - 1) / o; }
VIO_PRE_HD uint32_t area_weight(int x, int j, int c, int o) {
  const int lo = j * o > x * c ? j * o : x * c, hi = (j + 1) * o < (x + 1) * c ? (j + 1) * o : (x + 1) * c;
  return (uint32_t)(hi - lo);
}
// (S + D / 2) / D without leaving 32 bits when S is close to 2^32
VIO_PRE_HD uint32_t area_round(uint32_t S, uint32_t D) {
  const uint32_t q = S / D, rem = S - q * D;
  return q + (rem >= D - D / 2 ? 1u : 0u);
}

// The area average of output pixel (x, y); img is the first byte of plane 0 of the delivered frame.
// Every read is inside the crop: area_end(cols - 1, cw, ow) = crop_cols, likewise for the rows.
template <int BPP, bool VIDEO>
VIO_PRE_HD uint32_t area_px(const uint8_t *img, const SourcePlan &P, int x, int y) {
  uint32_t S = 0;
  for (int r = area_first(y, P.ch, P.oh); r < area_end(y, P.ch, P.oh); r++) {
    const uint8_t *row = img + (size_t)(P.crop_y + r) * P.stride;
    uint32_t h = 0;
    for (int j = area_first(x, P.cw, P.ow); j < area_end(x, P.cw, P.ow); j++)
      h += area_weight(x, j, P.cw, P.ow) * source_gray<BPP, VIDEO>(row, P.crop_x + j, P.c0, P.c2);
    S += area_weight(y, r, P.ch, P.oh) * h;
  }
  return area_round(S, (uint32_t)P.cw * (uint32_t)P.ch);
}

// pre::lens_source at a sample position that is no integer
template <class LENS>
VIO_PRE_HD void lens_source_at(const LENS &L, double xs, double ys, double *u, double *v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double xn = (xs - L.rect_cx) / L.rect_fx;
  const double yn = (ys - L.rect_cy) / L.rect_fy;
  lens_project(L, xn, yn, u, v);
}

// The rectified gray of output pixel (x, y) from the whole delivered frame: the mean of s * s samples of pre::rectify_px's
// arithmetic. Reads stay inside [0, P.rows) x [0, P.cols) by lens_fixed's clamp and the min, as there.
template <int BPP, bool VIDEO, class LENS>
VIO_PRE_HD uint32_t rectify_source_px(const uint8_t *img, const SourcePlan &P, const LENS &L, int x, int y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int s = P.s;
  uint32_t sum = 0;
  for (int j = 0; j < s; j++) {
    const double ys = (double)y + (double)(2 * j + 1 - s) / (double)(2 * s);
    for (int i = 0; i < s; i++) {
      const double xs = (double)x + (double)(2 * i + 1 - s) / (double)(2 * s);
      double u, v;
      lens_source_at(L, xs, ys, &u, &v);
      const int U = lens_fixed(u, P.cols), V = lens_fixed(v, P.rows);
      const int ix = U >> 5, ax = U & 31, iy = V >> 5, ay = V & 31;
      const int x1 = ix + 1 < P.cols ? ix + 1 : P.cols - 1, y1 = iy + 1 < P.rows ? iy + 1 : P.rows - 1;
      const uint8_t *r0 = img + (size_t)iy * P.stride, *r1 = img + (size_t)y1 * P.stride;
      const uint32_t top = source_gray<BPP, VIDEO>(r0, ix, P.c0, P.c2) * (32 - ax) + source_gray<BPP, VIDEO>(r0, x1, P.c0, P.c2) * ax;
      const uint32_t bot = source_gray<BPP, VIDEO>(r1, ix, P.c0, P.c2) * (32 - ax) + source_gray<BPP, VIDEO>(r1, x1, P.c0, P.c2) * ax;
      sum += (top * (32 - ay) + bot * ay + 512u) >> 10;
    }
  }
  return (sum + (uint32_t)(s * s) / 2u) / (uint32_t)(s * s);
}

// ---- the valid region of a slot (vio_preprocess_valid_regions*, vio_lens_model_valid_region) ----------------------------------
// Output pixel (x, y) is INSIDE when nothing it is made of was clamped: without a source the un-clamped (u, v) of lens_source
// lies in the rows x cols raw frame (the complement of what vio_lens_model_coverage counts; a NaN is outside); with a source
// every one of the s * s sample positions of rectify_source_px lies in the whole delivered frame. The mask is the inside map
// eroded by `margin` (Chebyshev distance; neighbours outside the image do not count). The polynomial models fold back far from
// the centre: a folded pixel whose source lands inside the frame counts as inside, as it does in the coverage count.
constexpr int kRegionMaxMargin = 32;

template <class LENS>
VIO_PRE_HD bool lens_inside(const LENS &L, int rows, int cols, int x, int y) {
  double u, v;
  lens_source(L, x, y, &u, &v);
  return !(lens_outside(u, cols) || lens_outside(v, rows));
}

// s samples per axis over a src_rows x src_cols delivered frame: the positions of rectify_source_px
template <class LENS>
VIO_PRE_HD bool lens_inside_source(const LENS &L, int s, int src_rows, int src_cols, int x, int y) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool in = true;
  for (int j = 0; j < s; j++) {
    const double ys = (double)y + (double)(2 * j + 1 - s) / (double)(2 * s);
    for (int i = 0; i < s; i++) {
      const double xs = (double)x + (double)(2 * i + 1 - s) / (double)(2 * s);
      double u, v;
      lens_source_at(L, xs, ys, &u, &v);
      in = in && !(lens_outside(u, src_cols) || lens_outside(v, src_rows));
    }
  }
  return in;
}

// P: the slot's source plan, or null (the frame has the output's size)
template <class LENS>
VIO_PRE_HD bool region_inside(const LENS &L, const SourcePlan *P, int rows, int cols, int x, int y) {
  return P ? lens_inside_source(L, P->s, P->rows, P->cols, x, y) : lens_inside(L, rows, cols, x, y);
}

// One axis of the erosion: is every entry of in[lo .. hi] (clipped to [0, n), `step` apart) nonzero?
VIO_PRE_HD bool region_all(const uint8_t *in, int n, int step, int at, int margin) {
  const int lo = at - margin > 0 ? at - margin : 0, hi = at + margin < n - 1 ? at + margin : n - 1;
  bool all = true;
  for (int k = lo; k <= hi; k++) all = all && in[(size_t)k * step] != 0;
  return all;
}

// The whole mask on the host: lens null = a slot without a lens (all 255). tmp: rows * cols bytes of scratch.
inline void valid_region(const VioLensModel *lens, const SourcePlan *P, int rows, int cols, int margin, uint8_t *mask, uint8_t *tmp) {
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) mask[(size_t)y * cols + x] = !lens || region_inside(*lens, P, rows, cols, x, y) ? 255 : 0;
  if (margin == 0 || !lens) return;
  for (int y = 0; y < rows; y++)  // along the rows, then along the columns: the square window is separable
    for (int x = 0; x < cols; x++) tmp[(size_t)y * cols + x] = region_all(mask + (size_t)y * cols, cols, 1, x, margin) ? 255 : 0;
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) mask[(size_t)y * cols + x] = region_all(tmp + x, rows, cols, y, margin) ? 255 : 0;
}

inline int32_t source_gcd(int32_t a, int32_t b) {
  while (b) {
    const int32_t t = a % b;
    a = b, b = t;
  }
  return a;
}

// vio_source_check: is s a source a rows x cols context can take?
inline bool source_valid(const VioSource &s, int32_t rows, int32_t cols) {
  const bool four = s.format == VIO_PIXEL_RGBA8 || s.format == VIO_PIXEL_BGRA8;
  if (!four && s.format != VIO_PIXEL_GRAY8 && s.format != VIO_PIXEL_NV12) return false;
  if (!(s.range == 0 || s.range == 1) || (s.range == 1 && four)) return false;
  if (rows < 1 || cols < 1 || s.rows < 1 || s.cols < 1 || s.rows > 16384 || s.cols > 16384) return false;
  if ((int64_t)s.stride < (int64_t)s.cols * (four ? 4 : 1) || (four && s.stride % 4 != 0)) return false;
  if (s.crop_x < 0 || s.crop_y < 0 || s.crop_cols < 1 || s.crop_rows < 1 || (int64_t)s.crop_x + s.crop_cols > s.cols ||
      (int64_t)s.crop_y + s.crop_rows > s.rows)
    return false;
  if (s.crop_cols < cols || s.crop_rows < rows) return false;                                    // no upscaling
  if ((int64_t)s.crop_cols > 8 * (int64_t)cols || (int64_t)s.crop_rows > 8 * (int64_t)rows) return false;
  const uint64_t cw = (uint64_t)(s.crop_cols / source_gcd(s.crop_cols, cols)), ch = (uint64_t)(s.crop_rows / source_gcd(s.crop_rows, rows));
  return 255u * cw * ch < (1ull << 32);
}

// of a source that source_valid accepts
inline SourcePlan source_plan(const VioSource &s, int32_t rows, int32_t cols) {
  SourcePlan P;
  const bool four = s.format == VIO_PIXEL_RGBA8 || s.format == VIO_PIXEL_BGRA8;
  P.bpp = four ? 4 : 1, P.video = s.range;
  P.c0 = s.format == VIO_PIXEL_BGRA8 ? 1868u : 4899u, P.c2 = s.format == VIO_PIXEL_BGRA8 ? 4899u : 1868u;
  P.rows = s.rows, P.cols = s.cols, P.stride = s.stride, P.crop_x = s.crop_x, P.crop_y = s.crop_y;
  const int32_t gx = source_gcd(s.crop_cols, cols), gy = source_gcd(s.crop_rows, rows);
  P.cw = s.crop_cols / gx, P.ow = cols / gx, P.ch = s.crop_rows / gy, P.oh = rows / gy;
  const int32_t sx = (s.cols + cols - 1) / cols, sy = (s.rows + rows - 1) / rows, m = sx > sy ? sx : sy;
  P.s = m < 4 ? m : 4;
  return P;
}

// vio_source_camera: the pinhole of the output image of a slot without a lens
inline void source_camera(const VioSource &s, int32_t rows, int32_t cols, const double in[4], double out[4]) {
  const double kx = (double)cols / (double)s.crop_cols, ky = (double)rows / (double)s.crop_rows;
  out[0] = in[0] * kx, out[1] = in[1] * ky;
  out[2] = (in[2] - (double)s.crop_x + 0.5) * kx - 0.5;
  out[3] = (in[3] - (double)s.crop_y + 0.5) * ky - 0.5;
}

}  // namespace pre
