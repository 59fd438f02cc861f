// init_core.h — what solveInitial does around its bundle adjustment, for a batch of independent start-ups: the relative
// pose fit (init::solve_relative_rt, vio_initial.cpp), the PnP chain and the triangulations of GlobalSFM::construct
// (init::sfm_construct_before_ba, inital_sfm.cpp:117-227), construct's closing inversion (sfm_construct_after_ba,
// :287-314) and the PnP of the frames between the window's (VINS.cpp:926-1003). Single source: vio_init_sfm.hip compiles
// it for gfx950, tests/emul/simt_init.cpp compiles the same text for the host with -DVIO_SIMT (every work-item a fiber of
// tests/emul/simt.h; the code uses nothing but s_barrier between its phases).
//
// Every floating-point result is formed by the host code's operations in the host code's order (the unit is built with
// -ffp-contract=off; fp64 division and sqrt are IEEE on both sides):
//   * what belongs to one correspondence / one landmark (a Sampson residual and its five forward differences, a
//     reprojection residual with its 2x6 Jacobian, a triangulation with its 4x4 one-sided Jacobi SVD, a cost term) is one
//     work-item's, written to a per-problem slab of global memory, one row per quantity;
//   * a sum over correspondences or landmarks (the cost, each entry of H and g) belongs to ONE work-item, which walks the
//     row in ascending index (eight loads in flight, the additions in order); landmarks that take no part leave the sum
//     as it is. No floating-point atomics, no reduction trees;
//   * the small serial pieces (tangent basis, Rodrigues, the 5x5 / 6x6 LDL^T with Eigen's pivoting, the accept test, the
//     hint comparison) are one work-item's, and what decides control flow goes through LDS so that the workgroup stays
//     uniform;
//   * the six starts of the fit are the six waves of the head's workgroup; they run in lockstep, round by round, each with
//     its own state (needs a Jacobian / tries a step / done) until all are done.
// Library calls: sin / cos in exp_so3 and acos in the hint comparison. On the device they are vio_exact_math.h's correctly
// rounded ones (the device library's own are good to an ulp, not to the bit). The host route (vio_initial.cpp) calls the C
// library, whose results are the correctly rounded ones for all but a small share of arguments (glibc 2.3x: sin 0.04 %,
// cos 0.003 %, acos 0.07 % of random arguments differ in the last bit), and so does the host build of this header: the
// emulator reproduces the host route to the bit, the device differs from both where the C library rounds the other way.
#pragma once
#include <math.h>
#include <stdint.h>

#include "sfm_core.h"
#include "spmd.h"
#include "vio_amd.h"
#include "vio_exact_math.h"
#include "vio_math.h"

namespace vio {
namespace isfm {

constexpr int kStarts = 6;
constexpr int kHeadThreads = 64 * kStarts;  // one wave per start of the fit
constexpr int kTailThreads = 128;
constexpr int kMaxFrames = sfm::kMaxFrames;
constexpr int kMinChainPoints = 15;  // inital_sfm.cpp:47
constexpr int kMinExtraPoints = 6;   // VINS.cpp:975

// slab rows. Fit, per start: the base residuals, five Jacobian columns, the cost terms. PnP: the gathered points
// (X, xy), the 2x6 Jacobian, the residual, the cost term.
enum { FIT_R0 = 0, FIT_J = 1, FIT_TERM = 6, kFitRows = 7 };
enum { PNP_X = 0, PNP_UV = 3, PNP_J = 5, PNP_R = 17, PNP_TERM = 19, kPnpRows = 20 };
// LDS of one start of the fit (doubles)
enum { FS_R = 0, FS_T = 9, FS_COST = 12, FS_LAMBDA = 13, FS_E = 16 /* [7][9]: five perturbed, base, trial */, FS_RP = 80,
       FS_TP = 89, FS_H = 92, FS_G = 117, kFitLds = 128 };
enum { FI_STATE = 0, FI_IT = 1, FI_TRIES = 2, kFitInts = 4 };
enum { FIT_NEED_J = 0, FIT_TRY = 1, FIT_DONE = 2 };
// LDS of one PnP (doubles)
enum { PL_R = 0, PL_T = 9, PL_RN = 12, PL_TN = 21, PL_H = 24, PL_G = 60, PL_COST = 66, PL_LAMBDA = 67, kPnpLds = 68 };
enum { kPnpInts = 4 };

VIO_HD size_t fit_doubles(int Cm) { return (size_t)kStarts * kFitRows * Cm; }
VIO_HD size_t head_scratch_doubles(int Cm, int Pm) {
  const size_t a = fit_doubles(Cm), b = (size_t)kPnpRows * Pm;
  return a > b ? a : b;
}
VIO_HD size_t head_scratch_ints(int Cm, int Pm) { return 2 * (size_t)Cm + 2 * (size_t)Pm; }
// head LDS: the fit's states and the chain's poses never live at the same time, but both are small: kept apart
constexpr int kHeadLdsDoubles = kStarts * kFitLds + 64 /* selection */ + 24 * kMaxFrames /* Rc | tc | P */ + kPnpLds + 16;
constexpr int kTailLdsDoubles = kPnpLds + 32;

VIO_DEV double lib_sin(double x) {
#ifdef VIO_HOST_BUILD
  return sin(x);
#else
  return vio_xm::sin_dd(x).h;
#endif
}
VIO_DEV double lib_cos(double x) {
#ifdef VIO_HOST_BUILD
  return cos(x);
#else
  return vio_xm::cos_cr(x);
#endif
}
VIO_DEV double lib_acos(double x) {
#ifdef VIO_HOST_BUILD
  return acos(x);
#else
  return vio_xm::acos_cr(x);
#endif
}

// ---- exact small pieces (vio_math.h switches qnormalized / qinv to the hardware seeds on the device) ----
VIO_DEV Quat qnormalized_x(const Quat &q) {
  const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return Quat{q.x / n, q.y / n, q.z / n, q.w / n};
}
VIO_DEV Quat qinv_x(const Quat &q) {
  const double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
  return Quat{-q.x / n2, -q.y / n2, -q.z / n2, q.w / n2};
}

VIO_DEV void exp_so3(const double w[3], double R[9]) {  // vio_initial.cpp exp_so3
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
  double a, b;
  if (th < 1e-8) {
    a = 1.0 - th2 / 6.0, b = 0.5 - th2 / 24.0;
  } else {
    a = lib_sin(th) / th, b = (1.0 - lib_cos(th)) / th2;
  }
  double K[9], K2[9];
  skew3(w, K);
  mat3mul(K, K, K2);
  for (int i = 0; i < 9; i++) R[i] = a * K[i] + b * K2[i];
  R[0] += 1, R[4] += 1, R[8] += 1;
}

VIO_DEV void right_update(double R[9], const double w[3]) {
  double E[9], Rn[9];
  exp_so3(w, E);
  mat3mul(R, E, Rn);
  qtoR(qnormalized_x(RtoQ(Rn)), R);
}

VIO_DEV void tangent_basis(const double g0[3], double bc[6]) {  // initial_aligment.cpp:48-61
  const double n = sqrt(g0[0] * g0[0] + g0[1] * g0[1] + g0[2] * g0[2]);
  const double a[3] = {g0[0] / n, g0[1] / n, g0[2] / n};
  double tmp[3] = {0, 0, 1};
  if (a[0] == tmp[0] && a[1] == tmp[1] && a[2] == tmp[2]) tmp[0] = 1, tmp[2] = 0;
  const double d = a[0] * tmp[0] + a[1] * tmp[1] + a[2] * tmp[2];
  double b[3] = {tmp[0] - a[0] * d, tmp[1] - a[1] * d, tmp[2] - a[2] * d};
  const double bn = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  for (int k = 0; k < 3; k++) b[k] /= bn;
  const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  for (int k = 0; k < 3; k++) bc[2 * k] = b[k], bc[2 * k + 1] = c[k];
}

// dense::ldlt_solve (vio_dense.h) for a fixed size: LDL^T with symmetric pivoting on the largest remaining diagonal entry
template <int N>
VIO_DEV bool ldlt_solve(double *A, double *b, double *x) {
  int perm[N];
  for (int i = 0; i < N; i++) perm[i] = i;
  for (int k = 0; k < N; k++) {
    int p = k;
    double best = fabs(A[k * N + k]);
    for (int i = k + 1; i < N; i++)
      if (fabs(A[i * N + i]) > best) best = fabs(A[i * N + i]), p = i;
    if (p != k) {
      for (int j = 0; j < N; j++) {
        const double s = A[k * N + j];
        A[k * N + j] = A[p * N + j], A[p * N + j] = s;
      }
      for (int i = 0; i < N; i++) {
        const double s = A[i * N + k];
        A[i * N + k] = A[i * N + p], A[i * N + p] = s;
      }
      const double sb = b[k];
      b[k] = b[p], b[p] = sb;
      const int sp = perm[k];
      perm[k] = perm[p], perm[p] = sp;
    }
    const double d = A[k * N + k];
    if (d == 0.0 || !__builtin_isfinite(d)) return false;
    for (int i = k + 1; i < N; i++) {
      const double aik = A[i * N + k];
      if (aik != 0.0) {
        const double l = aik / d;
        for (int j = k + 1; j <= i; j++) A[i * N + j] -= l * A[j * N + k];
      }
    }
    for (int i = k + 1; i < N; i++) {
      A[i * N + k] /= d;
      A[k * N + i] = A[i * N + k];
      for (int j = i + 1; j < N; j++) A[i * N + j] = A[j * N + i];
    }
  }
  double y[N];
  for (int i = 0; i < N; i++) y[i] = b[i];
  for (int i = 0; i < N; i++)
    for (int j = 0; j < i; j++) y[i] -= A[i * N + j] * y[j];
  for (int i = 0; i < N; i++) y[i] /= A[i * N + i];
  for (int i = N - 1; i >= 0; i--)
    for (int j = i + 1; j < N; j++) y[i] -= A[j * N + i] * y[j];
  for (int i = 0; i < N; i++) x[i] = 0.0;
  for (int i = 0; i < N; i++) x[perm[i]] = y[i];
  return true;
}

// GlobalSFM::triangulatePoint (inital_sfm.cpp:5-21) as init::triangulate_point forms it: dense::null_vector of the 4x4
// design matrix = dense::jacobi_svd (one-sided Jacobi, at most 80 sweeps), the column of the smallest singular value.
VIO_DEV void triangulate_point(const double P0[12], const double P1[12], const double x0[2], const double x1[2], double X[3]) {
  double A[16], V[16];
  for (int c = 0; c < 4; c++) {
    A[c] = x0[0] * P0[8 + c] - P0[c], A[4 + c] = x0[1] * P0[8 + c] - P0[4 + c];
    A[8 + c] = x1[0] * P1[8 + c] - P1[c], A[12 + c] = x1[1] * P1[8 + c] - P1[4 + c];
  }
  for (int i = 0; i < 16; i++) V[i] = 0.0;
  for (int i = 0; i < 4; i++) V[i * 4 + i] = 1.0;
  for (int sweep = 0; sweep < 80; sweep++) {
    double off = 0;
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        double alpha = 0, beta = 0, gamma = 0;
        for (int i = 0; i < 4; i++) {
          const double ap = A[i * 4 + p], aq = A[i * 4 + q];
          alpha += ap * ap, beta += aq * aq, gamma += ap * aq;
        }
        if (gamma == 0.0) continue;
        const double ratio = fabs(gamma) / sqrt(alpha * beta + 1e-300);
        off = off < ratio ? ratio : off;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
        for (int i = 0; i < 4; i++) {
          const double ap = A[i * 4 + p], aq = A[i * 4 + q];
          A[i * 4 + p] = c * ap - sn * aq, A[i * 4 + q] = sn * ap + c * aq;
        }
        for (int i = 0; i < 4; i++) {
          const double vp = V[i * 4 + p], vq = V[i * 4 + q];
          V[i * 4 + p] = c * vp - sn * vq, V[i * 4 + q] = sn * vp + c * vq;
        }
      }
    if (off < 1e-15) break;
  }
  double s[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    double t = 0;
    for (int i = 0; i < 4; i++) t += A[i * 4 + j] * A[i * 4 + j];
    s[j] = sqrt(t);
  }
  double v[4] = {V[0], V[4], V[8], V[12]}, sj = s[0];
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (s[k] < sj) {
      sj = s[k];
      for (int i = 0; i < 4; i++) v[i] = V[i * 4 + k];
    }
  for (int k = 0; k < 3; k++) X[k] = v[k] / v[3];
}

VIO_DEV void make_pose(const double R[9], const double t[3], double P[12]) {
  for (int r = 0; r < 3; r++) P[4 * r] = R[3 * r], P[4 * r + 1] = R[3 * r + 1], P[4 * r + 2] = R[3 * r + 2], P[4 * r + 3] = t[r];
}

// ---- the relative pose fit --------------------------------------------------------------------------------------------
VIO_DEV void essential(const double R[9], const double t[3], double E[9]) {
  double tx[9];
  skew3(t, tx);
  mat3mul(tx, R, E);
}
// e and d of one correspondence: the residual is e / sqrt(d + 1e-300), the cost term e e / (d + 1e-300)
VIO_DEV void sampson(const double E[9], const double *xy0, const double *xy1, int i, double *e, double *d) {
  const double x1[3] = {xy0[2 * i], xy0[2 * i + 1], 1.0}, x2[3] = {xy1[2 * i], xy1[2 * i + 1], 1.0};
  double Ex1[3], Etx2[3];
  mat3vec(E, x1, Ex1);
  for (int k = 0; k < 3; k++) Etx2[k] = E[k] * x2[0] + E[3 + k] * x2[1] + E[6 + k] * x2[2];
  *e = x2[0] * Ex1[0] + x2[1] * Ex1[1] + x2[2] * Ex1[2];
  *d = Ex1[0] * Ex1[0] + Ex1[1] * Ex1[1] + Etx2[0] * Etx2[0] + Etx2[1] * Etx2[1];
}
VIO_DEV void perturbed(const double R[9], const double t[3], const double bc[6], const double p[5], double Rp[9], double tp[3]) {
  for (int k = 0; k < 9; k++) Rp[k] = R[k];
  right_update(Rp, p);
  for (int k = 0; k < 3; k++) tp[k] = t[k] + bc[2 * k] * p[3] + bc[2 * k + 1] * p[4];
  const double tn = sqrt(tp[0] * tp[0] + tp[1] * tp[1] + tp[2] * tp[2]);
  for (int k = 0; k < 3; k++) tp[k] /= tn;
}

struct FitOut {
  int ok, inliers, sign;  // sign: +1 / -1, the translation sign the cheirality vote took
};

// init::solve_relative_rt for n >= 9 correspondences. lds: kStarts * kFitLds + 64 doubles, li: kStarts * kFitInts ints;
// rows: fit_doubles(cstride) doubles, good: 2 cstride ints. rel_out: Rout[9] | tout[3]. Every work-item returns the verdict.
VIO_DEV FitOut fit_relative(int tid, int n, const double *xy0, const double *xy1, const double *hint, ldsd lds, ldsi li,
                            double *rows, int cstride, int *good, double *rel_out) {
  const int s = tid >> 6, ln = tid & 63;
  ldsd fs = lds + s * kFitLds;
  ldsi fi = li + s * kFitInts;
  ldsd sel = lds + kStarts * kFitLds;  // bestR[9] | bestt[3] | tt[2][3] | P1[2][12]
  double *r0 = rows + (size_t)(s * kFitRows + FIT_R0) * cstride, *Jr = rows + (size_t)(s * kFitRows + FIT_J) * cstride;
  double *term = rows + (size_t)(s * kFitRows + FIT_TERM) * cstride;
  const double h = 1e-6;
  if (ln == 0) {
    const double dirs[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
    const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {dirs[s][0], dirs[s][1], dirs[s][2]};
    double E[9];
    essential(R, t, E);
    for (int k = 0; k < 9; k++) fs[FS_R + k] = R[k], fs[FS_E + 5 * 9 + k] = E[k];
    for (int k = 0; k < 3; k++) fs[FS_T + k] = t[k];
    fs[FS_LAMBDA] = 1e-3;
    fi[FI_STATE] = FIT_NEED_J, fi[FI_IT] = 0, fi[FI_TRIES] = 0;
  }
  __syncthreads();
  {
    double E[9];
    for (int k = 0; k < 9; k++) E[k] = fs[FS_E + 5 * 9 + k];
    for (int i = ln; i < n; i += 64) {
      double e, d;
      sampson(E, xy0, xy1, i, &e, &d);
      term[i] = e * e / (d + 1e-300);
    }
  }
  __syncthreads();
  if (ln == 0) {
    double cost = 0;
#pragma unroll 8
    for (int i = 0; i < n; i++) cost += term[i];
    fs[FS_COST] = cost;
  }
  __syncthreads();
  for (;;) {
    bool any = false;
    for (int k = 0; k < kStarts; k++) any = any || li[k * kFitInts + FI_STATE] != FIT_DONE;
    if (!any) break;
    const int st = fi[FI_STATE];
    // the five perturbed poses (3 rotation, 2 on the sphere of t) of the forward differences
    if (st == FIT_NEED_J && ln < 5) {
      double R[9], t[3], bc[6], p[5] = {0, 0, 0, 0, 0}, Rp[9], tp[3], E[9];
      for (int k = 0; k < 9; k++) R[k] = fs[FS_R + k];
      for (int k = 0; k < 3; k++) t[k] = fs[FS_T + k];
      tangent_basis(t, bc);
      for (int k = 0; k < 5; k++) p[k] = k == ln ? h : 0.0;
      perturbed(R, t, bc, p, Rp, tp);
      essential(Rp, tp, E);
      for (int k = 0; k < 9; k++) fs[FS_E + ln * 9 + k] = E[k];
    }
    __syncthreads();
    if (st == FIT_NEED_J)
      for (int i = ln; i < n; i += 64) {
        double E[9], e, d;
        for (int k = 0; k < 9; k++) E[k] = fs[FS_E + 5 * 9 + k];
        sampson(E, xy0, xy1, i, &e, &d);
        const double rb = e / sqrt(d + 1e-300);
        r0[i] = rb;
        for (int c = 0; c < 5; c++) {
          for (int k = 0; k < 9; k++) E[k] = fs[FS_E + c * 9 + k];
          sampson(E, xy0, xy1, i, &e, &d);
          const double r1 = e / sqrt(d + 1e-300);
          Jr[(size_t)c * cstride + i] = (r1 - rb) / h;
        }
      }
    __syncthreads();
    if (st == FIT_NEED_J && ln < 30) {
      if (ln < 25) {
        const double *Ja = Jr + (size_t)(ln / 5) * cstride, *Jb = Jr + (size_t)(ln % 5) * cstride;
        double acc = 0.0;
#pragma unroll 8
        for (int i = 0; i < n; i++) acc += Ja[i] * Jb[i];
        fs[FS_H + ln] = acc;
      } else {
        const double *Ja = Jr + (size_t)(ln - 25) * cstride;
        double acc = 0.0;
#pragma unroll 8
        for (int i = 0; i < n; i++) acc -= Ja[i] * r0[i];
        fs[FS_G + ln - 25] = acc;
      }
    }
    __syncthreads();
    // one trial step: damped system, LDL^T, the stepped pose
    if (st != FIT_DONE && ln == 0) {
      if (st == FIT_NEED_J) fi[FI_TRIES] = 0;
      const double lambda = fs[FS_LAMBDA];
      double Hd[25], gd[5], dx[5];
      for (int k = 0; k < 25; k++) Hd[k] = fs[FS_H + k];
      for (int k = 0; k < 5; k++) gd[k] = fs[FS_G + k];
      for (int a = 0; a < 5; a++) Hd[a * 5 + a] += lambda * (fs[FS_H + a * 5 + a] + 1e-12);
      if (!ldlt_solve<5>(Hd, gd, dx)) {
        fi[FI_STATE] = FIT_DONE;  // no step: the start ends where it stands
      } else {
        double R[9], t[3], bc[6], Rp[9], tp[3], E[9];
        for (int k = 0; k < 9; k++) R[k] = fs[FS_R + k];
        for (int k = 0; k < 3; k++) t[k] = fs[FS_T + k];
        tangent_basis(t, bc);
        perturbed(R, t, bc, dx, Rp, tp);
        essential(Rp, tp, E);
        for (int k = 0; k < 9; k++) fs[FS_RP + k] = Rp[k], fs[FS_E + 6 * 9 + k] = E[k];
        for (int k = 0; k < 3; k++) fs[FS_TP + k] = tp[k];
        fi[FI_STATE] = FIT_TRY;
      }
    }
    __syncthreads();
    const int st2 = fi[FI_STATE];
    if (st2 == FIT_TRY) {
      double E[9];
      for (int k = 0; k < 9; k++) E[k] = fs[FS_E + 6 * 9 + k];
      for (int i = ln; i < n; i += 64) {
        double e, d;
        sampson(E, xy0, xy1, i, &e, &d);
        term[i] = e * e / (d + 1e-300);
      }
    }
    __syncthreads();
    if (st2 == FIT_TRY && ln == 0) {
      double c2 = 0;
#pragma unroll 8
      for (int i = 0; i < n; i++) c2 += term[i];
      const double cost = fs[FS_COST];
      if (c2 < cost) {
        const double rel = (cost - c2) / (cost + 1e-300);
        for (int k = 0; k < 9; k++) fs[FS_R + k] = fs[FS_RP + k], fs[FS_E + 5 * 9 + k] = fs[FS_E + 6 * 9 + k];
        for (int k = 0; k < 3; k++) fs[FS_T + k] = fs[FS_TP + k];
        const double l3 = fs[FS_LAMBDA] * 0.3;
        fs[FS_COST] = c2, fs[FS_LAMBDA] = l3 < 1e-9 ? 1e-9 : l3;
        const int it = fi[FI_IT] + 1;
        fi[FI_IT] = it;
        fi[FI_STATE] = (rel < 1e-10 || it >= 60) ? FIT_DONE : FIT_NEED_J;
      } else {
        fs[FS_LAMBDA] = fs[FS_LAMBDA] * 10;
        const int tries = fi[FI_TRIES] + 1;
        fi[FI_TRIES] = tries;
        if (tries >= 8) fi[FI_STATE] = FIT_DONE;
      }
    }
    __syncthreads();
  }
  // the best local minimum; with a hint, among those within a factor of it the one whose rotation is closest
  if (tid == 0) {
    double best_cost = 1e300;
    int best = 0;
    for (int c = 0; c < kStarts; c++)
      if (lds[c * kFitLds + FS_COST] < best_cost) best_cost = lds[c * kFitLds + FS_COST], best = c;
    if (hint) {
      double best_angle = 1e300, Hh[9];
      for (int k = 0; k < 9; k++) Hh[k] = hint[k];
      for (int c = 0; c < kStarts; c++) {
        if (!(lds[c * kFitLds + FS_COST] <= 3.0 * best_cost + 1e-12 * (double)n)) continue;
        double Rc[9], M[9];
        for (int k = 0; k < 9; k++) Rc[k] = lds[c * kFitLds + FS_R + k];
        mat3mul(Rc, Hh, M);
        const double tr0 = M[0] + M[4] + M[8], tr1 = -1.0 < tr0 ? tr0 : -1.0, tr = tr1 < 3.0 ? tr1 : 3.0;
        const double angle = lib_acos((tr - 1.0) / 2.0);
        if (angle < best_angle) best_angle = angle, best = c;
      }
    }
    for (int k = 0; k < 9; k++) sel[k] = lds[best * kFitLds + FS_R + k];
    for (int k = 0; k < 3; k++) sel[9 + k] = lds[best * kFitLds + FS_T + k];
  }
  __syncthreads();
  // recoverPose's part: the sign of t with more points in front of both cameras within distance 50
  {
    double bestR[9], bestt[3];
    for (int k = 0; k < 9; k++) bestR[k] = sel[k];
    for (int k = 0; k < 3; k++) bestt[k] = sel[9 + k];
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0};
    double P0[12];
    make_pose(I3, zero, P0);
    for (int u = tid; u < 2 * n; u += kHeadThreads) {
      const int sgn = u >= n ? 1 : 0, i = u - sgn * n;
      const double tt[3] = {sgn ? -bestt[0] : bestt[0], sgn ? -bestt[1] : bestt[1], sgn ? -bestt[2] : bestt[2]};
      double P1[12], X[3], X2[3];
      make_pose(bestR, tt, P1);
      triangulate_point(P0, P1, &xy0[2 * i], &xy1[2 * i], X);
      mat3vec(bestR, X, X2);
      const double z2 = X2[2] + tt[2];
      good[sgn * cstride + i] = (X[2] > 0 && X[2] < 50 && z2 > 0 && z2 < 50) ? 1 : 0;
    }
  }
  __syncthreads();
  ldsi verdict = li + kStarts * kFitInts;
  if (tid == 0) {
    int best_good = -1;
    double sign = 1;
    for (int sgn = 0; sgn < 2; sgn++) {
      int g = 0;
      for (int i = 0; i < n; i++) g += good[sgn * cstride + i];
      if (g > best_good) best_good = g, sign = sgn ? -1 : 1;
    }
    double bestR[9], Rout[9], v[3];
    for (int k = 0; k < 9; k++) bestR[k] = sel[k];
    mat3T(bestR, Rout);
    const double ts[3] = {sign * sel[9], sign * sel[10], sign * sel[11]};
    mat3vec(Rout, ts, v);
    for (int k = 0; k < 9; k++) rel_out[k] = Rout[k];
    for (int k = 0; k < 3; k++) rel_out[9 + k] = -v[k];
    verdict[0] = best_good > 10 ? 1 : 0, verdict[1] = best_good, verdict[2] = sign < 0 ? -1 : 1;
  }
  __syncthreads();
  FitOut o;
  o.ok = verdict[0], o.inliers = verdict[1], o.sign = verdict[2];
  return o;
}

// ---- PnP ------------------------------------------------------------------------------------------------------------
// init::pnp_refine over the gathered points of rows (PNP_X, PNP_UV; use[j] != 0 takes part), by the nt work-items of a
// workgroup. lds[PL_R], lds[PL_T]: world -> camera guess, refined in place. Every work-item returns the verdict.
VIO_DEV void pnp_cost_terms(int tid, int nt, int N, const int *use, double *rows, size_t rs, cldsd R_, cldsd t_) {
  double R[9], t[3];
  for (int k = 0; k < 9; k++) R[k] = R_[k];
  for (int k = 0; k < 3; k++) t[k] = t_[k];
  for (int j = tid; j < N; j += nt) {
    if (!use[j]) continue;
    const double Xw[3] = {rows[(PNP_X + 0) * rs + j], rows[(PNP_X + 1) * rs + j], rows[(PNP_X + 2) * rs + j]};
    double X[3];
    mat3vec(R, Xw, X);
    for (int k = 0; k < 3; k++) X[k] += t[k];
    const double ex = X[0] / X[2] - rows[(PNP_UV + 0) * rs + j], ey = X[1] / X[2] - rows[(PNP_UV + 1) * rs + j];
    rows[PNP_TERM * rs + j] = ex * ex + ey * ey;
  }
}
VIO_DEV double pnp_cost_sum(int N, const int *use, const double *rows, size_t rs) {
  double c = 0;
#pragma unroll 8
  for (int j = 0; j < N; j++) {  // (a landmark that takes no part leaves the sum as it is: its row entry is never used)
    const double v = c + rows[PNP_TERM * rs + j];
    c = use[j] ? v : c;
  }
  return c;
}

VIO_DEV bool pnp_refine(int tid, int nt, int N, const int *use, double *rows, size_t rs, ldsd lds, ldsi ctl) {
  pnp_cost_terms(tid, nt, N, use, rows, rs, lds + PL_R, lds + PL_T);
  __syncthreads();
  if (tid == 0) lds[PL_COST] = pnp_cost_sum(N, use, rows, rs), lds[PL_LAMBDA] = 1e-3;
  __syncthreads();
  for (int it = 0; it < 20; it++) {
    {
      double R[9], t[3];
      for (int k = 0; k < 9; k++) R[k] = lds[PL_R + k];
      for (int k = 0; k < 3; k++) t[k] = lds[PL_T + k];
      for (int j = tid; j < N; j += nt) {
        if (!use[j]) continue;
        const double Xw[3] = {rows[(PNP_X + 0) * rs + j], rows[(PNP_X + 1) * rs + j], rows[(PNP_X + 2) * rs + j]};
        double X[3];
        mat3vec(R, Xw, X);
        for (int k = 0; k < 3; k++) X[k] += t[k];
        const double iz = 1.0 / X[2], r[2] = {X[0] * iz - rows[(PNP_UV + 0) * rs + j], X[1] * iz - rows[(PNP_UV + 1) * rs + j]};
        const double Jp[6] = {iz, 0, -X[0] * iz * iz, 0, iz, -X[1] * iz * iz};
        double Sx[9], RS[9];
        skew3(Xw, Sx);
        mat3mul(R, Sx, RS);  // dXc/dw = -R [Xw]x
        for (int r2 = 0; r2 < 2; r2++)
          for (int c = 0; c < 3; c++) {
            rows[(PNP_J + r2 * 6 + c) * rs + j] = -(Jp[r2 * 3] * RS[c] + Jp[r2 * 3 + 1] * RS[3 + c] + Jp[r2 * 3 + 2] * RS[6 + c]);
            rows[(PNP_J + r2 * 6 + 3 + c) * rs + j] = Jp[r2 * 3 + c];
          }
        rows[(PNP_R + 0) * rs + j] = r[0], rows[(PNP_R + 1) * rs + j] = r[1];
      }
    }
    __syncthreads();
    if (tid < 42) {
      if (tid < 36) {
        const int a = tid / 6, b = tid % 6;
        const double *Ja = rows + (PNP_J + a) * rs, *Jb = rows + (PNP_J + b) * rs, *Ja6 = rows + (PNP_J + 6 + a) * rs,
                     *Jb6 = rows + (PNP_J + 6 + b) * rs;
        double acc = 0.0;
#pragma unroll 8
        for (int j = 0; j < N; j++) {
          const double v = acc + (Ja[j] * Jb[j] + Ja6[j] * Jb6[j]);
          acc = use[j] ? v : acc;
        }
        lds[PL_H + tid] = acc;
      } else {
        const int a = tid - 36;
        const double *Ja = rows + (PNP_J + a) * rs, *Ja6 = rows + (PNP_J + 6 + a) * rs, *r0 = rows + (PNP_R + 0) * rs,
                     *r1 = rows + (PNP_R + 1) * rs;
        double acc = 0.0;
#pragma unroll 8
        for (int j = 0; j < N; j++) {
          const double v = acc - (Ja[j] * r0[j] + Ja6[j] * r1[j]);
          acc = use[j] ? v : acc;
        }
        lds[PL_G + a] = acc;
      }
    }
    __syncthreads();
    bool improved = false, stop = false;
    for (int tries = 0; tries < 8 && !improved; tries++) {
      if (tid == 0) {
        const double lambda = lds[PL_LAMBDA];
        double Hd[36], gd[6], dx[6];
        for (int k = 0; k < 36; k++) Hd[k] = lds[PL_H + k];
        for (int k = 0; k < 6; k++) gd[k] = lds[PL_G + k];
        for (int a = 0; a < 6; a++) Hd[a * 6 + a] += lambda * (lds[PL_H + a * 6 + a] + 1e-12);
        if (!ldlt_solve<6>(Hd, gd, dx)) {
          ctl[0] = 0;
        } else {
          double Rn[9];
          for (int k = 0; k < 9; k++) Rn[k] = lds[PL_R + k];
          right_update(Rn, dx);
          for (int k = 0; k < 9; k++) lds[PL_RN + k] = Rn[k];
          for (int k = 0; k < 3; k++) lds[PL_TN + k] = lds[PL_T + k] + dx[3 + k];
          ctl[0] = 1;
        }
      }
      __syncthreads();
      if (!ctl[0]) return false;
      pnp_cost_terms(tid, nt, N, use, rows, rs, lds + PL_RN, lds + PL_TN);
      __syncthreads();
      if (tid == 0) {
        const double c2 = pnp_cost_sum(N, use, rows, rs), cost = lds[PL_COST];
        if (__builtin_isfinite(c2) && c2 < cost) {
          const double rel = (cost - c2) / (cost + 1e-300);
          for (int k = 0; k < 9; k++) lds[PL_R + k] = lds[PL_RN + k];
          for (int k = 0; k < 3; k++) lds[PL_T + k] = lds[PL_TN + k];
          const double l3 = lds[PL_LAMBDA] * 0.3;
          lds[PL_COST] = c2, lds[PL_LAMBDA] = l3 < 1e-9 ? 1e-9 : l3;
          ctl[1] = rel < 1e-12 ? 2 : 1;
        } else {
          lds[PL_LAMBDA] = lds[PL_LAMBDA] * 10;
          ctl[1] = 0;
        }
      }
      __syncthreads();
      improved = ctl[1] != 0, stop = ctl[1] == 2;
    }
    if (!improved || stop) break;
  }
  return __builtin_isfinite(lds[PL_COST]);
}

// ---- the head: fit, then construct's steps 1-4 ----------------------------------------------------------------------
// One launch: what the head reads and writes besides the bundle adjustment's batch (sfm::Batch, whose cq | ct | X it fills).
//   hint [n][4]: relative_mode, correspondences, R_hint given, -
//   hin  [n][24 + 4 Cm]: relative_R[9] | relative_T[3] | R_hint[9] | -[3] | xy0[2 Cm] | xy1[2 Cm]
//   status [n][4]: VIO_INIT_SFM_* of the head, inliers, sign of t the cheirality vote took (0: no fit), -;  rel [n][12]: the relative pose the chain started from
struct HeadBatch {
  int n, Cm;
  const int *hint;
  const double *hin;
  int *status;
  double *rel, *scr_d;
  int *scr_i;
};
VIO_HD size_t hin_stride(int Cm) { return 24 + 4 * (size_t)Cm; }

// A problem whose head failed leaves the bundle adjustment a header it ends on at once: no landmarks, no observations, no
// free columns -- cost 0, gradient 0, CONVERGENCE before the first iteration.
VIO_DEV void neuter_ba_header(int *h, int Fm) {
  h[2] = 0, h[3] = 0, h[4] = 0;
  for (int i = 0; i < 2 * Fm; i++) h[8 + i] = -1;
}

VIO_DEV void head(int tid, const sfm::Batch &B, const HeadBatch &HB, int b, ldsd lds) {
  const int Fm = B.Fm, Pm = B.Pm, Om = B.Om;
  int *hdr = (int *)B.ints + (size_t)b * sfm::int_stride(Fm, Pm, Om);
  double *in = (double *)B.in + (size_t)b * sfm::dbl_stride(Fm, Pm, Om);
  const sfm::View v = sfm::view_of(B, b);
  const int F = v.F, l = v.l, np = v.np, last = F - 1;
  const int *hi = HB.hint + 4 * (size_t)b;
  const double *hd = HB.hin + (size_t)b * hin_stride(HB.Cm);
  double *scr = HB.scr_d + (size_t)b * head_scratch_doubles(HB.Cm, Pm);
  int *scri = HB.scr_i + (size_t)b * head_scratch_ints(HB.Cm, Pm);
  int *status = HB.status + 4 * (size_t)b;
  double *rel = HB.rel + 12 * (size_t)b;
  ldsd fit_lds = lds, chain = lds + kStarts * kFitLds + 64, pl = chain + 24 * kMaxFrames;
  ldsi li = (ldsi)(pl + kPnpLds);  // kStarts * kFitInts + 3 for the fit, kPnpInts + 2 for the chain (not at the same time)
  // relative pose
  int inliers = 0;
  if (tid == 0) status[2] = 0;
  if (hi[0] == 1) {
    const int n = hi[1];
    bool ok = false;
    if (n >= 9) {
      const FitOut o = fit_relative(tid, n, hd + 24, hd + 24 + 2 * (size_t)HB.Cm, hi[2] ? hd + 12 : nullptr, fit_lds, li, scr, HB.Cm,
                                    scri, rel);
      ok = o.ok != 0, inliers = o.inliers;
      if (tid == 0) status[2] = o.sign;
    }
    if (!ok) {
      if (tid == 0) status[0] = VIO_INIT_SFM_FAIL_RELATIVE, status[1] = inliers, neuter_ba_header(hdr, Fm);
      return;
    }
  } else {
    if (tid < 12) rel[tid] = hd[tid];
  }
  __syncthreads();
  // construct: camera -> reference poses inverted to world -> camera (c_Rotation, c_Translation)
  ldsd Rc = chain, tc = chain + 9 * kMaxFrames, P = chain + 12 * kMaxFrames;
  ldsi ctl = li;
  int *state = scri + 2 * (size_t)HB.Cm, *use = state + Pm;
  double *X = in + 7 * Fm;
  const double *xy = v.xy;
  for (int p = tid; p < np; p += kHeadThreads) state[p] = 0;
  if (tid == 0) {
    double relR[9], relT[3], Rl[9], vv[3], Pm_[12];
    for (int k = 0; k < 9; k++) relR[k] = rel[k];
    for (int k = 0; k < 3; k++) relT[k] = rel[9 + k];
    for (int k = 0; k < 9 * F; k++) Rc[k] = 0.0;
    for (int k = 0; k < 3 * F; k++) tc[k] = 0.0;
    Rc[9 * l] = 1, Rc[9 * l + 4] = 1, Rc[9 * l + 8] = 1;
    mat3T(relR, Rl);
    mat3vec(Rl, relT, vv);
    for (int k = 0; k < 9; k++) Rc[9 * last + k] = Rl[k];
    for (int k = 0; k < 3; k++) tc[3 * last + k] = -vv[k];
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero[3] = {0, 0, 0}, tl[3] = {-vv[0], -vv[1], -vv[2]};
    make_pose(I3, zero, Pm_);
    for (int k = 0; k < 12; k++) P[12 * l + k] = Pm_[k];
    make_pose(Rl, tl, Pm_);
    for (int k = 0; k < 12; k++) P[12 * last + k] = Pm_[k];
  }
  __syncthreads();
  // triangulate_two_frames (inital_sfm.cpp:76-115): landmarks without a position seen in both frames
  auto two_frames = [&](int f0, int f1) {
    double P0[12], P1[12];
    for (int k = 0; k < 12; k++) P0[k] = P[12 * f0 + k], P1[k] = P[12 * f1 + k];
    for (int p = tid; p < np; p += kHeadThreads) {
      if (state[p]) continue;
      const int k0 = v.pf_obs[p * F + f0], k1 = v.pf_obs[p * F + f1];
      if (k0 < 0 || k1 < 0) continue;
      double Xp[3];
      triangulate_point(P0, P1, &xy[2 * k0], &xy[2 * k1], Xp);
      for (int k = 0; k < 3; k++) X[3 * p + k] = Xp[k];
      state[p] = 1;
    }
  };
  // solveFrameByPnP (inital_sfm.cpp:24-74) of frame i from the pose of frame `from`; 1 solved, 0 not, -1 too few points
  auto frame_pnp = [&](int i, int from) -> int {
    const size_t rs = (size_t)Pm;
    for (int p = tid; p < np; p += kHeadThreads) {
      const int k = v.pf_obs[p * F + i], u = state[p] && k >= 0;
      use[p] = u;
      if (u) {
        for (int c = 0; c < 3; c++) scr[(PNP_X + c) * rs + p] = X[3 * p + c];
        scr[(PNP_UV + 0) * rs + p] = xy[2 * k], scr[(PNP_UV + 1) * rs + p] = xy[2 * k + 1];
      }
    }
    if (tid < 9) pl[PL_R + tid] = Rc[9 * from + tid];
    if (tid < 3) pl[PL_T + tid] = tc[3 * from + tid];
    __syncthreads();
    if (tid == 0) {
      int cnt = 0;
      for (int p = 0; p < np; p++) cnt += use[p];
      ctl[2] = cnt;
    }
    __syncthreads();
    if (ctl[2] < kMinChainPoints) return -1;
    const bool ok = pnp_refine(tid, kHeadThreads, np, use, scr, rs, pl, ctl);
    __syncthreads();
    return ok ? 1 : 0;
  };
  auto set_pose = [&](int i, cldsd R_, cldsd t_) {  // work-item 0, between barriers
    double R[9], t[3], Pm_[12];
    for (int k = 0; k < 9; k++) R[k] = R_[k], Rc[9 * i + k] = R[k];
    for (int k = 0; k < 3; k++) t[k] = t_[k], tc[3 * i + k] = t[k];
    make_pose(R, t, Pm_);
    for (int k = 0; k < 12; k++) P[12 * i + k] = Pm_[k];
  };
  // 1: l .. last-1 against the last frame
  for (int i = l; i < last; i++) {
    if (i > l) {
      if (frame_pnp(i, i - 1) != 1) {
        if (tid == 0) status[0] = VIO_INIT_SFM_FAIL_CHAIN, status[1] = inliers, neuter_ba_header(hdr, Fm);
        return;
      }
      if (tid == 0) set_pose(i, pl + PL_R, pl + PL_T);
      __syncthreads();
    }
    two_frames(i, last);
    __syncthreads();
  }
  // 2: l+1 .. last-1 against l (a landmark takes the first pair that sees it)
  for (int i = l + 1; i < last; i++) two_frames(l, i);
  __syncthreads();
  // 3: l-1 .. 0 (the reference ignores a failing PnP here and keeps the guess)
  for (int i = l - 1; i >= 0; i--) {
    const int r = frame_pnp(i, i + 1);
    if (tid == 0) {
      if (r == 1) set_pose(i, pl + PL_R, pl + PL_T);
      else set_pose(i, Rc + 9 * (i + 1), tc + 3 * (i + 1));
    }
    __syncthreads();
    two_frames(i, l);
    __syncthreads();
  }
  // 4: everything else, from its first and last observation
  for (int p = tid; p < np; p += kHeadThreads) {
    if (state[p]) continue;
    const int k0 = v.pt_start[p], k1 = v.pt_start[p + 1] - 1, f0 = v.obs_frame[k0], f1 = v.obs_frame[k1];
    double P0[12], P1[12], Xp[3];
    for (int k = 0; k < 12; k++) P0[k] = P[12 * f0 + k], P1[k] = P[12 * f1 + k];
    triangulate_point(P0, P1, &xy[2 * k0], &xy[2 * k1], Xp);
    for (int k = 0; k < 3; k++) X[3 * p + k] = Xp[k];
    state[p] = 1;
  }
  // 5: the bundle adjustment's blocks: c_rotation = Quaterniond(c_Rotation[i]) as w x y z, c_translation
  if (tid < F) {
    double R[9];
    for (int k = 0; k < 9; k++) R[k] = Rc[9 * tid + k];
    const Quat q = RtoQ(R);
    in[4 * tid] = q.w, in[4 * tid + 1] = q.x, in[4 * tid + 2] = q.y, in[4 * tid + 3] = q.z;
    for (int k = 0; k < 3; k++) in[4 * Fm + 3 * tid + k] = tc[3 * tid + k];
  }
  if (tid == 0) status[0] = VIO_INIT_SFM_OK, status[1] = inliers;
}

// ---- the tail: construct's inversion, PnP of the frames outside the window ---------------------------------------------
// unit u = (problem, extra frame or -1). Reads the bundle adjustment's output block and trace.
//   units [U][4]: problem, extra (-1: the inversion), first entry of its list, entries
//   ex_point [E]: landmark (index among the bundle adjustment's); ex_xy [E][2]; guess [U]: window frame of the guess
//   qT [n][7 Fm]: q (x y z w) | T;  ex_out [U][12]: R | t;  ex_flag [U]: 0 not run, 1 solved, 2 too few points, 3 PnP failed
struct TailBatch {
  int U, Em;
  const int *units, *ex_point, *guess;
  const double *ex_xy;
  const int *head_status;  // [n][4]
  double *qT, *ex_out, *scr_d;
  int *ex_flag, *scr_i, *ba_ok;  // ba_ok [n]
};

VIO_DEV void tail(int tid, const sfm::Batch &B, const TailBatch &TB, int u, ldsd lds) {
  const int *un = TB.units + 4 * (size_t)u;
  const int b = un[0], e = un[1], first = un[2], cnt = un[3];
  const int Fm = B.Fm, Pm = B.Pm;
  const int F = B.ints[(size_t)b * sfm::int_stride(Fm, Pm, B.Om)];
  const double *out = B.out + (size_t)b * sfm::dbl_stride(Fm, Pm, 0), *cq = out, *ct = out + 4 * Fm, *X = out + 7 * Fm;
  const bool head_ok = TB.head_status[4 * b] == VIO_INIT_SFM_OK;
  const double *sd = B.stats_d + (size_t)b * kStatsDoubles;
  const int *si = B.stats_i + (size_t)b * kStatsInts;
  const bool ba_ok = head_ok && (si[1] == 1 || sd[1] < 3e-03);  // inital_sfm.cpp:279
  if (e < 0) {
    if (tid == 0) TB.ba_ok[b] = ba_ok ? 1 : 0;
    if (!ba_ok) return;
    double *q = TB.qT + (size_t)b * 7 * Fm, *T = q + 4 * Fm;
    for (int i = tid; i < F; i += kTailThreads) {  // q[i] = c_rotation^-1, T[i] = -(q[i] * c_translation) (:287-295)
      const Quat qi = qinv_x(Quat{cq[4 * i + 1], cq[4 * i + 2], cq[4 * i + 3], cq[4 * i]});
      const double t[3] = {ct[3 * i], ct[3 * i + 1], ct[3 * i + 2]};
      double vv[3];
      q[4 * i] = qi.x, q[4 * i + 1] = qi.y, q[4 * i + 2] = qi.z, q[4 * i + 3] = qi.w;
      qrot(qi, t, vv);
      for (int k = 0; k < 3; k++) T[3 * i + k] = -vv[k];
    }
    return;
  }
  if (!ba_ok) {
    if (tid == 0) TB.ex_flag[u] = 0;
    return;
  }
  if (cnt < kMinExtraPoints) {  // "init Not enough points for solve pnp !"
    if (tid == 0) TB.ex_flag[u] = 2;
    return;
  }
  const size_t rs = (size_t)TB.Em;
  double *rows = TB.scr_d + (size_t)u * kPnpRows * rs;
  int *use = TB.scr_i + (size_t)u * rs;
  ldsd pl = lds;
  ldsi ctl = (ldsi)(lds + kPnpLds);
  for (int j = tid; j < cnt; j += kTailThreads) {
    const int p = TB.ex_point[first + j];
    use[j] = 1;
    for (int c = 0; c < 3; c++) rows[(PNP_X + c) * rs + j] = X[3 * p + c];
    rows[(PNP_UV + 0) * rs + j] = TB.ex_xy[2 * (first + j)], rows[(PNP_UV + 1) * rs + j] = TB.ex_xy[2 * (first + j) + 1];
  }
  if (tid == 0) {  // the guess: Q[ii].inverse(), -(R_initial * T[ii]) (VINS.cpp:960-966)
    const int i = TB.guess[u];
    const Quat qi = qinv_x(Quat{cq[4 * i + 1], cq[4 * i + 2], cq[4 * i + 3], cq[4 * i]});
    const double t[3] = {ct[3 * i], ct[3 * i + 1], ct[3 * i + 2]};
    double vv[3], Ti[3], Rq[9], R0[9], w[3];
    qrot(qi, t, vv);
    for (int k = 0; k < 3; k++) Ti[k] = -vv[k];
    qtoR(qi, Rq);
    mat3T(Rq, R0);
    mat3vec(R0, Ti, w);
    for (int k = 0; k < 9; k++) pl[PL_R + k] = R0[k];
    for (int k = 0; k < 3; k++) pl[PL_T + k] = -w[k];
  }
  __syncthreads();
  const bool ok = pnp_refine(tid, kTailThreads, cnt, use, rows, rs, pl, ctl);
  __syncthreads();
  if (tid < 9) TB.ex_out[12 * (size_t)u + tid] = pl[PL_R + tid];
  if (tid < 3) TB.ex_out[12 * (size_t)u + 9 + tid] = pl[PL_T + tid];
  if (tid == 0) TB.ex_flag[u] = ok ? 1 : 3;
}

}  // namespace isfm
}  // namespace vio
