// pre_rectify.h — lens rectification of the image pre-step, one output pixel at a time (VioLens / VioLensModel, include/vio_amd.h).
// Host- and device-callable: clahe_lut_kernel (vio_preprocess.hip), the host entries vio_lens_* / vio_lens_model_* and the
// stand-alone host programs of the tests (tests/emul/lens_rectify_main.cpp, lens_model_main.cpp) compile this text, and all of
// them must give the same bytes.
//
// Output pixel (x, y) of the rectified pinhole (rect_fx .. rect_cy) -> ray -> Brown-Conrady forward model (OpenCV's coefficient
// order k1 k2 p1 p2 k3) -> raw pixel (u, v), clamped to the raw image (replicate border), rounded to 1/32 pixel (ties to even),
// bilinear blend of the four raw neighbours in integers. IEEE doubles, every operation rounded on its own, in the order and
// with the parentheses written here: no fused multiply-add (the pragma below; the host build also passes -ffp-contract=off).
//
// VioLensModel adds two forward models between the ray and (u, v), everything around them unchanged:
//   VIO_LENS_RATIONAL  radial = (1 + r2*(k1 + r2*(k2 + r2*k3))) / (1 + r2*(k[5] + r2*(k[6] + r2*k[7]))), then the Brown-Conrady lines
//   VIO_LENS_FISHEYE   r = sqrt(r2), th = lens_atan(r), t2 = th*th, thd = th*(1 + t2*(k[0] + t2*(k[1] + t2*(k[2] + t2*k[3]))))
//                      s = r2 == 0 ? 1 : thd / r,  u = fx*(xn*s) + cx,  v = fy*(yn*s) + cy
// sqrt is the correctly rounded IEEE square root on the host and on the device (the mixed-batch device test compares the bytes).
//
// lens_atan(x), x >= 0: the arctangent to about 1 ulp, the same bits wherever this text is compiled -- which neither libm's nor
// the device library's atan promises (they agree to an ulp: see the head of vio_exact_math.h). + - * /, comparisons and
// constants only. The reduction and the polynomial are those of fdlibm's s_atan.c (public, Sun Microsystems 1993) without
// its low-order correction words; every branch below is a select, so the order of operations is the same for every x:
//   x <  7/16  (0.4375)  num = x              den = 1              hi = 0
//   x < 11/16  (0.6875)  num = (x + x) - 1    den = 2 + x          hi = atan(1/2) = 4.63647609000806093515e-01
//   x < 19/16  (1.1875)  num = x - 1          den = x + 1          hi = atan(1)   = 7.85398163397448278999e-01
//   x < 39/16  (2.4375)  num = x - 1.5        den = 1 + 1.5*x      hi = atan(3/2) = 9.82793723247329054082e-01
//   otherwise            num = -1             den = x              hi = pi/2      = 1.57079632679489655800e+00
//   t = num / den,  z = t*t,  w = z*z
//   s1 = z*(a0 + w*(a2 + w*(a4 + w*(a6 + w*(a8 + w*a10)))))
//   s2 = w*(a1 + w*(a3 + w*(a5 + w*(a7 + w*a9))))
//   atan = hi + (t - t*(s1 + s2))
// with a0 .. a10 = kAtanA below (|t| <= 7/16 in every row; a NaN takes the last row and stays a NaN).
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

VIO_PRE_HD double lens_atan(double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double kAtanA[11] = {3.33333333333329318027e-01,  -1.99999999998764832476e-01, 1.42857142725034663711e-01,
                             -1.11111104054623557880e-01, 9.09088713343650656196e-02,  -7.69187620504482999495e-02,
                             6.66107313738753120669e-02,  -5.83357013379057348645e-02, 4.97687799461593236017e-02,
                             -3.65315727442169155270e-02, 1.62858201153657823623e-02};
  const bool b0 = x < 0.4375, b1 = x < 0.6875, b2 = x < 1.1875, b3 = x < 2.4375;
  const double num = b0 ? x : b1 ? (x + x) - 1.0 : b2 ? x - 1.0 : b3 ? x - 1.5 : -1.0;
  const double den = b0 ? 1.0 : b1 ? 2.0 + x : b2 ? x + 1.0 : b3 ? 1.0 + 1.5 * x : x;
  const double hi = b0   ? 0.0
                    : b1 ? 4.63647609000806093515e-01
                    : b2 ? 7.85398163397448278999e-01
                    : b3 ? 9.82793723247329054082e-01
                         : 1.57079632679489655800e+00;
  const double t = num / den, z = t * t, w = z * z;
  const double s1 = z * (kAtanA[0] + w * (kAtanA[2] + w * (kAtanA[4] + w * (kAtanA[6] + w * (kAtanA[8] + w * kAtanA[10])))));
  const double s2 = w * (kAtanA[1] + w * (kAtanA[3] + w * (kAtanA[5] + w * (kAtanA[7] + w * kAtanA[9]))));
  return hi + (t - t * (s1 + s2));
}

// The forward model of VioLensModel with the model a compile-time constant: the kernels choose it per frame, outside the
// pixel loop, so that a Brown-Conrady frame runs the Brown-Conrady instructions and nothing else.
template <int MODEL>
VIO_PRE_HD void lens_project_as(const VioLensModel &L, double xn, double yn, double *u, double *v) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double r2 = xn * xn + yn * yn;
  if (MODEL == VIO_LENS_FISHEYE) {
    const double r = sqrt(r2), th = lens_atan(r), t2 = th * th;
    const double thd = th * (1.0 + t2 * (L.k[0] + t2 * (L.k[1] + t2 * (L.k[2] + t2 * L.k[3]))));
    const double s = r2 == 0.0 ? 1.0 : thd / r;
    *u = L.fx * (xn * s) + L.cx;
    *v = L.fy * (yn * s) + L.cy;
    return;
  }
  double radial = 1.0 + r2 * (L.k[0] + r2 * (L.k[1] + r2 * L.k[4]));
  if (MODEL == VIO_LENS_RATIONAL) radial = radial / (1.0 + r2 * (L.k[5] + r2 * (L.k[6] + r2 * L.k[7])));
  const double xd = (xn * radial + (2.0 * L.k[2]) * xn * yn) + L.k[3] * (r2 + (2.0 * xn) * xn);
  const double yd = (yn * radial + L.k[2] * (r2 + (2.0 * yn) * yn)) + ((2.0 * L.k[3]) * xn) * yn;
  *u = L.fx * xd + L.cx;
  *v = L.fy * yd + L.cy;
}

// ... and chosen at run time (the host entries)
VIO_PRE_HD void lens_project(const VioLensModel &L, double xn, double yn, double *u, double *v) {
  if (L.model == VIO_LENS_FISHEYE)
    lens_project_as<VIO_LENS_FISHEYE>(L, xn, yn, u, v);
  else if (L.model == VIO_LENS_RATIONAL)
    lens_project_as<VIO_LENS_RATIONAL>(L, xn, yn, u, v);
  else
    lens_project_as<VIO_LENS_BROWN>(L, xn, yn, u, v);
}

// A VioLensModel whose model is the constant MODEL: what the kernels hand to the functions below
template <int MODEL>
struct LensAs {
  const VioLensModel &m;
  double rect_fx, rect_fy, rect_cx, rect_cy;
  VIO_PRE_HD explicit LensAs(const VioLensModel &l) : m(l), rect_fx(l.rect_fx), rect_fy(l.rect_fy), rect_cx(l.rect_cx), rect_cy(l.rect_cy) {}
};
template <int MODEL>
VIO_PRE_HD void lens_project(const LensAs<MODEL> &L, double xn, double yn, double *u, double *v) {
  lens_project_as<MODEL>(L.m, xn, yn, u, v);
}

// Output pixel (x, y) -> raw pixel (u, v), not clamped. LENS: VioLens, VioLensModel or LensAs<MODEL>.
template <class LENS>
VIO_PRE_HD void lens_source(const LENS &L, int x, int y, double *u, double *v) {
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
template <int CH, class LENS>
VIO_PRE_HD uint32_t rectify_px(const uint8_t *img, size_t row_stride, int rows, int cols, const LENS &L, int x, int y) {
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

// The record VioLens stands for: vio_preprocess_set_lenses stores this
inline VioLensModel lens_model_of(const VioLens &L) {
  VioLensModel M = {};
  M.model = VIO_LENS_BROWN;
  M.fx = L.fx, M.fy = L.fy, M.cx = L.cx, M.cy = L.cy;
  M.k[0] = L.k1, M.k[1] = L.k2, M.k[2] = L.p1, M.k[3] = L.p2, M.k[4] = L.k3;
  M.rect_fx = L.rect_fx, M.rect_fy = L.rect_fy, M.rect_cx = L.rect_cx, M.rect_cy = L.rect_cy;
  return M;
}
// of a VIO_LENS_BROWN record
inline VioLens lens_of_model(const VioLensModel &M) {
  return VioLens{M.fx, M.fy, M.cx, M.cy, M.k[0], M.k[1], M.k[2], M.k[3], M.k[4], M.rect_fx, M.rect_fy, M.rect_cx, M.rect_cy};
}

inline bool lens_model_valid(const VioLensModel &M) {
  if (M.reserved != 0 || !(M.model == VIO_LENS_BROWN || M.model == VIO_LENS_RATIONAL || M.model == VIO_LENS_FISHEYE)) return false;
  const int used = M.model == VIO_LENS_BROWN ? 5 : M.model == VIO_LENS_RATIONAL ? 8 : 4;
  for (int k = 0; k < 8; k++)
    if (!isfinite(M.k[k]) || (k >= used && M.k[k] != 0.0)) return false;
  const double f[8] = {M.fx, M.fy, M.cx, M.cy, M.rect_fx, M.rect_fy, M.rect_cx, M.rect_cy};
  for (int k = 0; k < 8; k++)
    if (!isfinite(f[k])) return false;
  return M.fx > 0 && M.fy > 0 && M.rect_fx > 0 && M.rect_fy > 0;
}

}  // namespace pre
