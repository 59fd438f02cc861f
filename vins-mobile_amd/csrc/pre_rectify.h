// pre_rectify.h — lens rectification of the image pre-step, one output pixel at a time (VioLens, include/vio_amd.h).
// Host- and device-callable: clahe_lut_kernel (vio_preprocess.hip), the host entries vio_lens_* and the stand-alone host program
// of the tests (tests/emul/lens_rectify_main.cpp) compile this text, and all three must give the same bytes.
//
// Output pixel (x, y) of the rectified pinhole (rect_fx .. rect_cy) -> ray -> Brown-Conrady forward model (OpenCV's coefficient
// order k1 k2 p1 p2 k3) -> raw pixel (u, v), clamped to the raw image (replicate border), rounded to 1/32 pixel (ties to even),
// bilinear blend of the four raw neighbours in integers. IEEE doubles, every operation rounded on its own, in the order and
// with the parentheses written here: no fused multiply-add (the pragma below; the host build also passes -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include "vio_amd.h"

#if defined(__HIPCC__)
#define VIO_PRE_HD __host__ __device__ __forceinline__
#else
#define VIO_PRE_HD inline
#endif

namespace pre {

// Normalized undistorted (xn, yn) -> raw pixel (u, v), not clamped.
VIO_PRE_HD void lens_project(const VioLens &L, double xn, double yn, double *u, double *v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double r2 = xn * xn + yn * yn;
  const double radial = 1.0 + r2 * (L.k1 + r2 * (L.k2 + r2 * L.k3));
  const double xd = (xn * radial + (2.0 * L.p1) * xn * yn) + L.p2 * (r2 + (2.0 * xn) * xn);
  const double yd = (yn * radial + L.p1 * (r2 + (2.0 * yn) * yn)) + ((2.0 * L.p2) * xn) * yn;
  *u = L.fx * xd + L.cx;
  *v = L.fy * yd + L.cy;
}

// Output pixel (x, y) -> raw pixel (u, v), not clamped.
VIO_PRE_HD void lens_source(const VioLens &L, int x, int y, double *u, double *v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double xn = ((double)x - L.rect_cx) / L.rect_fx;
  const double yn = ((double)y - L.rect_cy) / L.rect_fy;
  lens_project(L, xn, yn, u, v);
}

// A source outside [0, n - 1] (what vio_lens_coverage counts; a NaN is outside).
VIO_PRE_HD bool lens_outside(double u, int n) { return !(u >= 0.0 && u <= (double)(n - 1)); }

// clamp to [0, n - 1] (a NaN goes to 0), then 1/32-pixel fixed point: in [0, 32 * (n - 1)]
VIO_PRE_HD int lens_fixed(double u, int n) {
  if (!(u >= 0.0)) u = 0.0;
  if (u > (double)(n - 1)) u = (double)(n - 1);
  return (int)rint(u * 32.0);
}

VIO_PRE_HD uint32_t gray_of_rgba(uint32_t px) {  // little endian: R in the low byte (cv::cvtColor CV_RGBA2GRAY)
  const uint32_t r = px & 0xff, g = (px >> 8) & 0xff, b = (px >> 16) & 0xff;
  return (r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14;
}

template <int CH>
VIO_PRE_HD uint32_t raw_gray(const uint8_t *img, size_t row_stride, int y, int x) {
  if (CH == 4) return gray_of_rgba(*reinterpret_cast<const uint32_t *>(img + (size_t)y * row_stride + 4 * (size_t)x));
  return img[(size_t)y * row_stride + x];
}

// The rectified gray of output pixel (x, y); img is the raw frame (CH = 1 gray, CH = 4 RGBA with 4-byte aligned rows).
// Every read is inside [0, rows) x [0, cols): ix <= cols - 1 and iy <= rows - 1 by the clamp, x1 / y1 by the min.
template <int CH>
VIO_PRE_HD uint32_t rectify_px(const uint8_t *img, size_t row_stride, int rows, int cols, const VioLens &L, int x, int y) {
  double u, v;
  lens_source(L, x, y, &u, &v);
  const int U = lens_fixed(u, cols), V = lens_fixed(v, rows);
  const int ix = U >> 5, ax = U & 31, iy = V >> 5, ay = V & 31;
  const int x1 = ix + 1 < cols ? ix + 1 : cols - 1, y1 = iy + 1 < rows ? iy + 1 : rows - 1;
  const uint32_t top = raw_gray<CH>(img, row_stride, iy, ix) * (32 - ax) + raw_gray<CH>(img, row_stride, iy, x1) * ax;
  const uint32_t bot = raw_gray<CH>(img, row_stride, y1, ix) * (32 - ax) + raw_gray<CH>(img, row_stride, y1, x1) * ax;
  return (top * (32 - ay) + bot * ay + 512u) >> 10;
}

inline bool lens_valid(const VioLens &L) {
  const double f[13] = {L.fx, L.fy, L.cx, L.cy, L.k1, L.k2, L.p1, L.p2, L.k3, L.rect_fx, L.rect_fy, L.rect_cx, L.rect_cy};
  for (int k = 0; k < 13; k++)
    if (!isfinite(f[k])) return false;
  return L.fx > 0 && L.fy > 0 && L.rect_fx > 0 && L.rect_fy > 0;
}

}  // namespace pre
