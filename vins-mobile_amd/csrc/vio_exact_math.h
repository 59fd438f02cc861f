// vio_exact_math.h -- cos, acos and pow of doubles, correctly rounded (round to nearest) up to the usual table-maker's cases:
// evaluated in double-double arithmetic to about 2^-85 and rounded once. The F-test's LMedS branch (8..14 correspondences)
// needs them: a 7-point model fits its own seven points to rounding error, so below 14 points the median error every model is
// ranked by is itself rounding noise (1e-24 .. 1e-29 px^2), and the model that wins is decided by the last bit of the cubic's
// roots. The device's math library and the host's agree to within an ulp, not to the bit; a correctly rounded result is what
// the host library returns for all but a vanishing share of arguments. Plain C++ (host and device): contraction must be off.
#pragma once
#include <math.h>
#if defined(__HIPCC__) || defined(__CUDACC__)
#define VIO_XM_HD __host__ __device__ inline
#define VIO_XM_CONST static constexpr
#else
#define VIO_XM_HD inline
#define VIO_XM_CONST static constexpr
#endif
namespace vio_xm {
struct dd { double h, l; };
VIO_XM_HD dd two_sum(double a, double b) { double s = a + b, bb = s - a; return {s, (a - (s - bb)) + (b - bb)}; }
VIO_XM_HD dd fast_two_sum(double a, double b) { double s = a + b; return {s, b - (s - a)}; }
VIO_XM_HD dd two_prod(double a, double b) { double p = a * b; return {p, fma(a, b, -p)}; }
VIO_XM_HD dd add(dd a, dd b) {
  dd s = two_sum(a.h, b.h), t = two_sum(a.l, b.l);
  s = fast_two_sum(s.h, s.l + t.h);
  return fast_two_sum(s.h, s.l + t.l);
}
VIO_XM_HD dd add_d(dd a, double b) { dd s = two_sum(a.h, b); return fast_two_sum(s.h, s.l + a.l); }
VIO_XM_HD dd mul(dd a, dd b) { dd p = two_prod(a.h, b.h); return fast_two_sum(p.h, p.l + (a.h * b.l + a.l * b.h)); }
VIO_XM_HD dd mul_d(dd a, double b) { dd p = two_prod(a.h, b); return fast_two_sum(p.h, p.l + a.l * b); }
VIO_XM_HD dd neg(dd a) { return {-a.h, -a.l}; }
VIO_XM_CONST double kPio2[3] = {0x1.921fb54442d18p+0, 0x1.1a62633145c07p-54, -0x1.f1976b7ed8fbcp-110};
VIO_XM_CONST double kLn2[3] = {0x1.62e42fefa39efp-1, 0x1.abc9e3b39803fp-56, 0x1.7b57a079a1934p-111};
VIO_XM_CONST double kSinC[14][2] = {{0x1.0000000000000p+0, 0x0.0p+0}, {-0x1.5555555555555p-3, -0x1.5555555555555p-57}, {0x1.1111111111111p-7, 0x1.1111111111111p-63}, {-0x1.a01a01a01a01ap-13, -0x1.a01a01a01a01ap-73}, {0x1.71de3a556c734p-19, -0x1.c154f8ddc6c00p-73}, {-0x1.ae64567f544e4p-26, 0x1.c062e06d1f209p-80}, {0x1.6124613a86d09p-33, 0x1.f28e0cc748ebep-87}, {-0x1.ae7f3e733b81fp-41, -0x1.1d8656b0ee8cbp-97}, {0x1.952c77030ad4ap-49, 0x1.ac981465ddc6cp-103}, {-0x1.2f49b46814157p-57, -0x1.2650f61dbdcb4p-112}, {0x1.71b8ef6dcf572p-66, -0x1.d043ae40c4647p-120}, {-0x1.761b41316381ap-75, 0x1.3423c7d91404fp-130}, {0x1.3f3ccdd165fa9p-84, -0x1.58ddadf344487p-139}, {-0x1.d1ab1c2dccea3p-94, -0x1.054d0c78aea14p-149}};
VIO_XM_CONST double kCosC[14][2] = {{0x1.0000000000000p+0, 0x0.0p+0}, {-0x1.0000000000000p-1, 0x0.0p+0}, {0x1.5555555555555p-5, 0x1.5555555555555p-59}, {-0x1.6c16c16c16c17p-10, 0x1.f49f49f49f49fp-65}, {0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-76}, {-0x1.27e4fb7789f5cp-22, -0x1.cbbc05b4fa99ap-76}, {0x1.1eed8eff8d898p-29, -0x1.2aec959e14c06p-83}, {-0x1.93974a8c07c9dp-37, -0x1.05d6f8a2efd1fp-92}, {0x1.ae7f3e733b81fp-45, 0x1.1d8656b0ee8cbp-101}, {-0x1.6827863b97d97p-53, -0x1.eec01221a8b0bp-107}, {0x1.e542ba4020225p-62, 0x1.ea72b4afe3c2fp-120}, {-0x1.0ce396db7f853p-70, 0x1.aebcdbd20331cp-124}, {0x1.f2cf01972f578p-80, -0x1.9ada5fcc1ab14p-135}, {-0x1.88e85fc6a4e5ap-89, 0x1.71c37ebd16540p-143}};
VIO_XM_CONST double kExpC[12][2] = {{0x1.0000000000000p+0, 0x0.0p+0}, {0x1.0000000000000p+0, 0x0.0p+0}, {0x1.0000000000000p-1, 0x0.0p+0}, {0x1.5555555555555p-3, 0x1.5555555555555p-57}, {0x1.5555555555555p-5, 0x1.5555555555555p-59}, {0x1.1111111111111p-7, 0x1.1111111111111p-63}, {0x1.6c16c16c16c17p-10, -0x1.f49f49f49f49fp-65}, {0x1.a01a01a01a01ap-13, 0x1.a01a01a01a01ap-73}, {0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-76}, {0x1.71de3a556c734p-19, -0x1.c154f8ddc6c00p-73}, {0x1.27e4fb7789f5cp-22, 0x1.cbbc05b4fa99ap-76}, {0x1.ae64567f544e4p-26, -0x1.c062e06d1f209p-80}};
// x - k * c for a constant c given in three parts (k a small integer held in a double)
VIO_XM_HD dd reduce(dd x, double k, const double c[3]) {
  dd r = add(x, neg(two_prod(k, c[0])));
  r = add(r, neg(two_prod(k, c[1])));
  return add_d(r, -(k * c[2]));
}
// sin and cos of |r| <= pi/4 (+ a little): the terms from r^12 on in double (they end below 2^-85 of the result), the rest in double-double
VIO_XM_HD void sincos_kernel(dd r, dd &s, dd &c) {
  const dd r2 = mul(r, r);
  double ts = kSinC[13][0], tc = kCosC[13][0];
  for (int n = 12; n >= 6; n--) ts = ts * r2.h + kSinC[n][0], tc = tc * r2.h + kCosC[n][0];
  dd as = {ts, 0.0}, ac = {tc, 0.0};
  for (int n = 5; n >= 0; n--) {
    as = add(mul(as, r2), dd{kSinC[n][0], kSinC[n][1]});
    ac = add(mul(ac, r2), dd{kCosC[n][0], kCosC[n][1]});
  }
  s = mul(as, r), c = ac;
}
VIO_XM_HD dd cos_dd(double x) {
  const double k = nearbyint(x * 0.63661977236758138);
  dd s, c;
  sincos_kernel(reduce(dd{x, 0.0}, k, kPio2), s, c);
  const int q = (int)k & 3;
  return q == 0 ? c : q == 1 ? neg(s) : q == 2 ? neg(c) : s;
}
VIO_XM_HD dd sin_dd(double x) {
  const double k = nearbyint(x * 0.63661977236758138);
  dd s, c;
  sincos_kernel(reduce(dd{x, 0.0}, k, kPio2), s, c);
  const int q = (int)k & 3;
  return q == 0 ? s : q == 1 ? c : q == 2 ? neg(s) : neg(c);
}
// |x| < 2^20 (the cubic's angles lie in [0, 2 pi))
VIO_XM_HD double cos_cr(double x) {
  if (!(fabs(x) < 1048576.0)) return cos(x);
  return cos_dd(x).h;
}
// one Newton step on cos(a) = v from the library's acos, in double-double
VIO_XM_HD double acos_cr(double v) {
  if (!(fabs(v) < 1.0)) return acos(v);
  const double a0 = acos(v);
  const dd f = add_d(cos_dd(a0), -v);  // ~ 1e-16
  const double sn = sin_dd(a0).h;
  const dd corr = {f.h / sn, 0.0};
  // a1 = a0 + f / sin(a0); the quotient's own error is 1e-16 of 1e-16
  const dd rem = add(f, neg(mul_d(dd{sn, 0.0}, corr.h)));  // f - sn * corr.h
  return add_d(dd{corr.h, rem.h / sn}, a0).h;
}
// exp of a double-double, as mantissa (double-double) and binary exponent
VIO_XM_HD dd exp_dd(dd p, int &e2) {
  const double k = nearbyint(p.h * 1.4426950408889634);
  dd r = reduce(p, k, kLn2);
  r.h *= 0.03125, r.l *= 0.03125;  // r / 32: the terms from r^5 on in double
  double t = kExpC[11][0];
  for (int n = 10; n >= 5; n--) t = t * r.h + kExpC[n][0];
  dd a = {t, 0.0};
  for (int n = 4; n >= 0; n--) a = add(mul(a, r), dd{kExpC[n][0], kExpC[n][1]});
  for (int q = 0; q < 5; q++) a = mul(a, a);
  e2 = (int)k;
  return a;
}
// x^y for finite x > 0 and moderate |y log x| (no overflow, no subnormal result); the library's pow otherwise
VIO_XM_HD double pow_cr(double x, double y) {
  const double l0 = log(x);
  if (!(x > 0.0) || !(fabs(l0) < 600.0) || !(fabs(y) < 1.0)) return pow(x, y);
  int e2;
  const dd em = exp_dd(dd{-l0, 0.0}, e2);                     // exp(-l0)
  const dd z = add_d(mul_d(em, ldexp(x, e2)), -1.0);          // x exp(-l0) - 1 ~ 1e-16: log x = l0 + z - z^2 / 2
  const dd L = add_d(add_d(z, -0.5 * z.h * z.h), l0);
  const dd r = exp_dd(mul_d(L, y), e2);
  return ldexp(r.h, e2);
}
}  // namespace vio_xm
