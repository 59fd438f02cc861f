// fe_ransac.h -- cv::findFundamentalMat(FM_RANSAC) of rejectWithF (feature_tracker.cpp:183-205): the 7-point solver and the
// RANSAC loop of calib3d's fundam.cpp / ptsetreg.cpp as one workgroup routine, and the two kernels that are nothing but it
// (vio_fundamental_ransac and, for the loop detector, vio::fundamental_ransac_batch: vio_ransac.h).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "vio_exact_math.h"

namespace {

// ---- findFundamentalMat(FM_RANSAC): device version of calib3d fundam.cpp / ptsetreg.cpp -------------------------
// (kept out of line: inlined, the double-double code cost the RANSAC path of track_update_kernel its last free registers)
__device__ __attribute__((noinline)) double exact_fn(int which, double x) {
  return which == 0 ? vio_xm::acos_cr(x) : which == 1 ? vio_xm::cos_cr(x) : vio_xm::pow_cr(x, 0.333333333333);
}
// exact: acos, cos and pow correctly rounded (vio_exact_math.h) instead of the device library's, which agree with the host's
// only to within an ulp. The LMedS branch asks for it: there the winning model is decided by the roots' last bit.
__device__ int solve_cubic_dev(const double c[4], double r[3], bool exact) {
  double a0 = c[0], a1 = c[1], a2 = c[2], a3 = c[3];
  double x0 = 0, x1 = 0, x2 = 0;
  int n = 0;
  if (a0 == 0) {
    if (a1 == 0) {
      if (a2 == 0) n = a3 == 0 ? -1 : 0;
      else x0 = -a3 / a2, n = 1;
    } else {
      double d = a2 * a2 - 4 * a1 * a3;
      if (d >= 0) {
        d = sqrt(d);
        double q1 = (-a2 + d) * 0.5, q2 = (a2 + d) * -0.5;
        if (fabs(q1) > fabs(q2)) x0 = q1 / a1, x1 = a3 / q1;
        else x0 = q2 / a1, x1 = a3 / q2;
        n = d > 0 ? 2 : 1;
      }
    }
  } else {
    a0 = 1. / a0, a1 *= a0, a2 *= a0, a3 *= a0;
    double Q = (a1 * a1 - 3 * a2) * (1. / 9), R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) * (1. / 54);
    double Qcubed = Q * Q * Q, d = Qcubed - R * R;
    const double kPi = 3.14159265358979323846;
    if (d >= 0) {
      const double av = R / sqrt(Qcubed);
      double theta = exact ? exact_fn(0, av) : acos(av), sqrtQ = sqrt(Q);
      double t0 = -2 * sqrtQ, t1 = theta * (1. / 3), t2 = a1 * (1. / 3);
      const double g0 = t1, g1 = t1 + (2. * kPi / 3), g2 = t1 + (4. * kPi / 3);
      if (exact) x0 = t0 * exact_fn(1, g0) - t2, x1 = t0 * exact_fn(1, g1) - t2, x2 = t0 * exact_fn(1, g2) - t2;
      else x0 = t0 * cos(g0) - t2, x1 = t0 * cos(g1) - t2, x2 = t0 * cos(g2) - t2;
      n = 3;
    } else {
      d = sqrt(-d);
      double e = exact ? exact_fn(2, d + fabs(R)) : pow(d + fabs(R), 0.333333333333);
      if (R > 0) e = -e;
      x0 = (e + Q / e) - a1 * (1. / 3);
      n = 1;
    }
  }
  r[0] = x0, r[1] = x1, r[2] = x2;
  return n;
}

// 7-point models for the subset (ms1, ms2); F[27]; returns the number of models.
// Work area of one 7-point solve. The elimination indexes its 7x9 system, the two null vectors and the column
// permutation dynamically: as local arrays they live in scratch memory (an L2 round trip per access, ~2000 of them on
// the one thread that owns the hypothesis); here they sit in LDS next to the hypothesis' points (track_update_kernel
// 0.30 -> 0.17 ms per 256 sequences).
struct SevenPointWork {
  double a[63], f1[9], f2[9];
  int colperm[10];
};

// The 7-point solve by the 16 lanes of one DPP row (lane l of the group). One thread alone spends ~130 k cycles in it: the
// elimination is ~1300 DEPENDENT LDS accesses (dynamic indexing keeps the system out of registers), and the whole RANSAC
// call waits for it. Here the pivot search (4 candidates per lane, then a 4-step butterfly on (|value|, position) keys
// with the serial scan's tie rule: first position wins), the swaps, the pivot-row division and the elimination (54
// elements, every lane reads its factors and pivot-row entries before anyone writes) run across the lanes; every element
// sees exactly the operations of the serial restatement (oracle run7point), so the result is bit-identical. The cubic and the model assembly
// (~300 flops) stay on lane 0. Returns the number of models on every lane of the group.
__device__ __forceinline__ int run7point_group(const float *ms1, const float *ms2, double *fmatrix, SevenPointWork &wk, int l, bool exact) {
  double *a = wk.a, *f1 = wk.f1, *f2 = wk.f2;
  int *colperm = wk.colperm;
  auto group_sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  if (l < 7) {
    double x0 = ms1[2 * l], y0 = ms1[2 * l + 1], x1 = ms2[2 * l], y1 = ms2[2 * l + 1];
    double *row = a + l * 9;
    row[0] = x1 * x0, row[1] = x1 * y0, row[2] = x1, row[3] = y1 * x0, row[4] = y1 * y0, row[5] = y1, row[6] = x0,
    row[7] = y0, row[8] = 1;
  }
  if (l < 9) colperm[l] = l;
  group_sync();
  for (int k = 0; k < 7; k++) {
    // pivot: largest |a[i][j]| over i >= k, j >= k, the first one in row-major order among equals
    double best = -1;
    int bpos = k * 9 + k;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int e = l + 16 * q, i = e / 9, j = e - 9 * i;
      if (e < 63 && i >= k && j >= k) {
        const double v = fabs(a[e]);
        if (v > best) best = v, bpos = e;
      }
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
      const double ob = __shfl_xor(best, m, 16);
      const int op = __shfl_xor(bpos, m, 16);
      if (ob > best || (ob == best && op < bpos)) best = ob, bpos = op;
    }
    const int pr = bpos / 9, pc = bpos - 9 * pr;
    if (pr != k && l < 9) {
      const double t = a[k * 9 + l];
      a[k * 9 + l] = a[pr * 9 + l], a[pr * 9 + l] = t;
    }
    group_sync();
    if (pc != k) {
      if (l < 7) {
        const double t = a[l * 9 + k];
        a[l * 9 + k] = a[l * 9 + pc], a[l * 9 + pc] = t;
      }
      if (l == 15) {
        const int t = colperm[k];
        colperm[k] = colperm[pc], colperm[pc] = t;
      }
    }
    group_sync();
    const double d = a[k * 9 + k];
    group_sync();
    if (d == 0.0) continue;
    if (l < 9) a[k * 9 + l] /= d;
    group_sync();
    double fv[4], pv[4], av[4];
    int ev[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {  // element q of this lane: rows i != k in order, 9 columns each
      const int e = l + 16 * q, ii = e / 9, j = e - 9 * ii, i = ii < k ? ii : ii + 1;
      const bool on = e < 54;
      ev[q] = on ? i * 9 + j : -1;
      fv[q] = on ? a[i * 9 + k] : 0.0, pv[q] = on ? a[k * 9 + j] : 0.0, av[q] = on ? a[i * 9 + j] : 0.0;
    }
    group_sync();
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (ev[q] >= 0 && fv[q] != 0.0) a[ev[q]] = av[q] - fv[q] * pv[q];
    group_sync();
  }
  if (l < 9) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      double *out = q == 0 ? f1 : f2;
      const double vj = l < 7 ? -a[l * 9 + 7 + q] : (l - 7 == q ? 1.0 : 0.0);
      out[colperm[l]] = vj;
    }
  }
  group_sync();
  if (l < 9) f1[l] -= f2[l];
  group_sync();
  int n = 0;
  if (l == 0) {
    double c[4], r[3];
    double t0 = f2[4] * f2[8] - f2[5] * f2[7], t1 = f2[3] * f2[8] - f2[5] * f2[6], t2 = f2[3] * f2[7] - f2[4] * f2[6];
    c[3] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2;
    c[2] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2 - f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) +
           f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) - f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) +
           f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) - f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
           f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]);
    t0 = f1[4] * f1[8] - f1[5] * f1[7], t1 = f1[3] * f1[8] - f1[5] * f1[6], t2 = f1[3] * f1[7] - f1[4] * f1[6];
    c[1] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2 - f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) +
           f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) - f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) +
           f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) - f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
           f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]);
    c[0] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2;
    n = solve_cubic_dev(c, r, exact);
    if (n >= 1 && n <= 3)
      for (int k = 0; k < n; k++, fmatrix += 9) {
        double lambda = r[k], mu = 1., s = f1[8] * r[k] + f2[8];
        if (fabs(s) > 2.220446049250313e-16) mu = 1. / s, lambda *= mu, fmatrix[8] = 1.;
        else fmatrix[8] = 0.;
        for (int i = 0; i < 8; i++) fmatrix[i] = f1[i] * lambda + f2[i] * mu;
      }
  }
  return __shfl(n, 0, 16);
}

__device__ __forceinline__ float epipolar_error(const double *F, float x1f, float y1f, float x2f, float y2f) {
  double x1 = x1f, y1 = y1f, x2 = x2f, y2 = y2f;
  double a = F[0] * x1 + F[1] * y1 + F[2], b = F[3] * x1 + F[4] * y1 + F[5], c = F[6] * x1 + F[7] * y1 + F[8];
  double s2 = 1. / (a * a + b * b);
  double d2 = x2 * a + y2 * b + c;
  a = F[0] * x2 + F[3] * y2 + F[6], b = F[1] * x2 + F[4] * y2 + F[7], c = F[2] * x2 + F[5] * y2 + F[8];
  double s1 = 1. / (a * a + b * b);
  double d1 = x1 * a + y1 * b + c;
  // std::max(e1, e2), not fmax: where the epipolar line in image 1 degenerates exactly (x2 on the epipole: 0 * inf)
  // e1 is NaN, and std::max keeps a NaN first operand while fmax drops it. LMedS sorts the errors' bit patterns as
  // integers: the host's NaN (x86: sign bit set) sorts first, the device's default NaN (sign bit clear) would sort
  // last, so a NaN is returned as the host makes it. Reached by tests/ransac_cases.py zoom_small_*.
  const double e1 = d1 * d1 * s1, e2 = d2 * d2 * s2;
  const float e = (float)((e1 < e2) ? e2 : e1);
  return e != e ? __int_as_float((int)0xffc00000u) : e;
}
__device__ __forceinline__ bool epipolar_inlier(const double *F, float x1f, float y1f, float x2f, float y2f, float t) {
  return epipolar_error(F, x1f, y1f, x2f, y2f) <= t;
}

__device__ bool have_collinear_dev(const float *p, int count) {
  int i = count - 1;
  for (int j = 0; j < i; j++) {
    double dx1 = p[2 * j] - p[2 * i], dy1 = p[2 * j + 1] - p[2 * i + 1];
    for (int k = 0; k < j; k++) {
      double dx2 = p[2 * k] - p[2 * i], dy2 = p[2 * k + 1] - p[2 * i + 1];
      if (fabs(dx2 * dy1 - dy2 * dx1) <= 1.1920929e-07 * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
    }
  }
  return false;
}

__device__ int ransac_update_iters(double p, double ep, int model_points, int max_iters) {
  p = fmax(p, 0.), p = fmin(p, 1.), ep = fmax(ep, 0.), ep = fmin(ep, 1.);
  double num = fmax(1. - p, 2.2250738585072014e-308), denom = 1. - pow(1. - ep, (double)model_points);
  if (denom < 2.2250738585072014e-308) return 0;
  num = log(num), denom = log(denom);
  return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

constexpr int kHypBatch = 16;  // hypotheses generated / evaluated per round

struct RansacShared {
  SevenPointWork work[kHypBatch];
  float ms1[kHypBatch][14], ms2[kHypBatch][14];
  double F[kHypBatch][27];
  int nmodels[kHypBatch];
  int good[kHypBatch][3];
  int idx[kHypBatch][7];  // drawn point indices of the batch
  int valid[kHypBatch];  // subset found
  int coll[kHypBatch];   // speculative subset failed checkSubset
  unsigned long long rng_before[kHypBatch];
  unsigned long long rng_state;
  int niters, max_good, best_h, best_k, iter, done, failed_first;
  double bestF[9];
  double med[kHypBatch][3], min_median;  // LMedS (fewer than 15 correspondences)
};

// Block-cooperative RANSAC over `count` correspondences; pts(i) -> (x1, y1, x2, y2) of correspondence i, from LDS
// (track_update_kernel's packed list) or global memory (GlobalPts). Writes mask[count] (1 = inlier).
// Exactly reproduces the sequential loop of RANSACPointSetRegistrator::run: subsets are drawn in order from one RNG
// stream; hypotheses are evaluated a batch at a time and then scanned in order with the adaptive iteration bound.
// Forced inline: the callers' operands keep their address space (LDS arrays are read with LDS instructions, not as flat
// accesses) and there is no call frame (as a function with two call sites in track_update_kernel it cost 120 loads and 119
// stores to the private segment per call: the frame plus the spills under the kernel's 256-register cap).
struct GlobalPts {
  const float *m1, *m2;
  __device__ __forceinline__ float4 operator()(int i) const { return make_float4(m1[2 * i], m1[2 * i + 1], m2[2 * i], m2[2 * i + 1]); }
};
template <class MaskT, class Pts>
__device__ __forceinline__ void fundamental_ransac_block(RansacShared &S, const Pts pts, int count, float thresh, double confidence,
                                                         MaskT *mask, long long *prof = nullptr) {
  const int tid = threadIdx.x, nt = blockDim.x;
  long long pt = prof ? clock64() : 0;
#define RS_STAMP(k)                                                    \
  do {                                                                 \
    if (prof && tid == 0) {                                            \
      const long long now = clock64();                                 \
      prof[k] += now - pt, pt = now;                                   \
    }                                                                  \
  } while (0)
  const int model_points = 7, max_iters = 1000;
  // findFundamentalMat (fundam.cpp, 3.0.0) runs RANSAC only from 15 points on, LMedS below; the tracker calls with
  // >= 8 points. LMedS shares the subset stream and the 7-point solver: a fixed number of iterations (300 at
  // confidence 0.99), the model with the smallest median error wins, inliers are cut at sigma^2 of that median.
  const bool lmeds = count < 15;
  if (count < 8) {
    for (int i = tid; i < count; i += nt) mask[i] = 1;
    __syncthreads();
    return;
  }
  if (tid == 0) {
    S.rng_state = 0xffffffffffffffffULL;
    S.niters = lmeds ? ransac_update_iters(confidence, 0.45, model_points, max_iters) : max_iters;
    S.max_good = 0, S.best_h = -1, S.best_k = 0, S.iter = 0, S.done = 0, S.failed_first = 0;
    S.min_median = 1.7976931348623157e308;
  }
  __syncthreads();
  const float t = thresh * thresh;
  while (true) {
    // hypotheses of this round. The adaptive bound usually ends a RANSAC call within its first handful of hypotheses (inlier
    // ratio 0.9: 7 iterations), and every hypothesis of a round is drawn, solved and scored whether the scan reaches it or
    // not: the first round takes 8, later rounds (and LMedS, whose iteration count is fixed) kHypBatch.
    const int nb = (!lmeds && S.iter == 0) ? 8 : kHypBatch;
    // ---- phase 1: draw the next nb subsets sequentially (one RNG stream). The draws are cheap integer
    //      work; checkSubset (collinearity, 2 x 15 cross products in double) is evaluated in parallel afterwards.
    //      Subsets are drawn speculatively as if every check passed, which is the same RNG consumption; if one fails
    //      (rare) the tail from that hypothesis is redrawn with the full serial semantics.
    auto draw = [&](unsigned long long &st, int h, bool with_check) {
      int idx[7], i = 0, iters = 0;
      const int max_attempts = 10000;
      for (; iters < max_attempts; iters++) {
        for (i = 0; i < model_points && iters < max_attempts;) {
          int idx_i = 0;
          for (;;) {
            st = (unsigned long long)(unsigned)st * 4164903690U + (unsigned)(st >> 32);
            idx_i = idx[i] = (int)((unsigned)st % (unsigned)count);
            int j;
            for (j = 0; j < i; j++)
              if (idx_i == idx[j]) break;
            if (j == i) break;
          }
          const float4 q = pts(idx_i);
          S.ms1[h][2 * i] = q.x, S.ms1[h][2 * i + 1] = q.y;
          S.ms2[h][2 * i] = q.z, S.ms2[h][2 * i + 1] = q.w;
          i++;
        }
        if (with_check && i == model_points && (have_collinear_dev(S.ms1[h], i) || have_collinear_dev(S.ms2[h], i))) continue;
        break;
      }
      return (i == model_points && iters < max_attempts) ? 1 : 0;
    };
    if (tid == 0) {
      // the serial part is the RNG stream only: indices go to LDS, the points are gathered by all threads afterwards.
      // x % count without an integer division: q = umulhi(x, floor((2^32 - 1) / count)) underestimates the quotient
      // by at most 2. (Pinning the stream to scalar registers -- the 112 dependent steps on the scalar unit -- measured the
      // same 21 k cycles per call.)
      const unsigned ucount = (unsigned)count, magic = 0xffffffffu / ucount;
      unsigned long long st = S.rng_state;
      for (int h = 0; h < nb; h++) {
        S.rng_before[h] = st;
        int idx[7];
#pragma unroll
        for (int i = 0; i < 7; i++) {
          for (;;) {
            st = (unsigned long long)(unsigned)st * 4164903690U + (unsigned)(st >> 32);
            const unsigned x = (unsigned)st;
            unsigned r = x - __umulhi(x, magic) * ucount;
            r = r >= ucount ? r - ucount : r;
            r = r >= ucount ? r - ucount : r;
            bool dup = false;
#pragma unroll
            for (int j = 0; j < i; j++) dup |= (int)r == idx[j];
            if (!dup) { idx[i] = (int)r; break; }
          }
          S.idx[h][i] = idx[i];
        }
        S.valid[h] = 1;  // (count >= 8 distinct points exist: the attempt cap of getSubset cannot trigger without checks)
      }
      S.rng_state = st;
    }
    __syncthreads();
    RS_STAMP(0);
    for (int it = tid; it < nb * 7; it += nt) {
      const int h = it / 7, i = it - 7 * h;
      const float4 q = pts(S.idx[h][i]);
      S.ms1[h][2 * i] = q.x, S.ms1[h][2 * i + 1] = q.y;
      S.ms2[h][2 * i] = q.z, S.ms2[h][2 * i + 1] = q.w;
    }
    __syncthreads();
    if (tid < nb) S.coll[tid] = (have_collinear_dev(S.ms1[tid], 7) || have_collinear_dev(S.ms2[tid], 7)) ? 1 : 0;
    __syncthreads();
    if (tid == 0) {
      int first = -1;
      for (int h = 0; h < nb && first < 0; h++)
        if (S.coll[h]) first = h;
      if (first >= 0) {
        unsigned long long st = S.rng_before[first];
        for (int h = first; h < nb; h++) {
          S.valid[h] = draw(st, h, true);
          if (!S.valid[h]) {
            for (int hh = h + 1; hh < nb; hh++) S.valid[hh] = 0;
            break;
          }
        }
        S.rng_state = st;
      }
    }
    __syncthreads();
    RS_STAMP(1);
    // ---- phase 2: 7-point models, 16 lanes per hypothesis
    for (int h = tid >> 4; h < nb; h += nt >> 4) {
      int n = 0;
      if (S.valid[h]) n = run7point_group(S.ms1[h], S.ms2[h], S.F[h], S.work[h], tid & 15, lmeds);
      if ((tid & 15) == 0) {
        S.nmodels[h] = n < 0 ? 0 : n;
        S.good[h][0] = S.good[h][1] = S.good[h][2] = 0;
      }
    }
    __syncthreads();
    RS_STAMP(2);
    // ---- phase 3: inlier counts for every (hypothesis, model) [RANSAC] / median error of every model [LMedS]
    if (lmeds) {
      for (int hk = tid; hk < nb * 3; hk += nt) {
        const int h = hk / 3, k = hk - 3 * h;
        if (k >= S.nmodels[h]) continue;
        int bits[14];  // count <= 14; std::sort on the float bit patterns as ints (ptsetreg.cpp)
        for (int i = 0; i < count; i++) {
          const float4 q = pts(i);
          const int b = __float_as_int(epipolar_error(S.F[h] + 9 * k, q.x, q.y, q.z, q.w));
          int j = i;
          for (; j > 0 && bits[j - 1] > b; j--) bits[j] = bits[j - 1];
          bits[j] = b;
        }
        S.med[h][k] = (count & 1) ? (double)__int_as_float(bits[count / 2])
                                  : (double)(__int_as_float(bits[count / 2 - 1]) + __int_as_float(bits[count / 2])) * 0.5;
      }
    } else
    for (int item = tid; item < nb * 3 * count; item += nt) {
      int hk = item / count, i = item - hk * count;
      int h = hk / 3, k = hk - 3 * h;
      if (k < S.nmodels[h]) {
        const float4 q = pts(i);
        if (epipolar_inlier(S.F[h] + 9 * k, q.x, q.y, q.z, q.w, t)) atomicAdd(&S.good[h][k], 1);
      }
    }
    __syncthreads();
    RS_STAMP(3);
    // ---- phase 4: sequential scan with the adaptive bound
    if (tid == 0) {
      for (int h = 0; h < nb; h++) {
        if (S.iter >= S.niters) { S.done = 1; break; }
        if (!S.valid[h]) {
          if (S.iter == 0) S.failed_first = 1;
          S.done = 1;
          break;
        }
        for (int k = 0; k < S.nmodels[h]; k++) {
          if (lmeds) {
            if (S.med[h][k] < S.min_median) {
              S.min_median = S.med[h][k];
              for (int q = 0; q < 9; q++) S.bestF[q] = S.F[h][9 * k + q];
            }
            continue;
          }
          int good = S.good[h][k];
          if (good > max(S.max_good, model_points - 1)) {
            S.max_good = good;
            for (int q = 0; q < 9; q++) S.bestF[q] = S.F[h][9 * k + q];
            S.best_h = h;
            S.niters = ransac_update_iters(confidence, (double)(count - good) / count, model_points, S.niters);
          }
        }
        S.iter++;
      }
      if (S.iter >= S.niters) S.done = 1;
    }
    __syncthreads();
    RS_STAMP(4);
    if (prof && tid == 0) prof[6] += 1;
    if (S.done) break;
  }
  if (lmeds && S.min_median < 1.7976931348623157e308 && !S.failed_first) {
    double sigma = 2.5 * 1.4826 * (1 + 5. / (count - model_points)) * sqrt(S.min_median);
    sigma = fmax(sigma, 0.001);
    const float ts = (float)(sigma * sigma);
    for (int i = tid; i < count; i += nt) {
      const float4 q = pts(i);
      mask[i] = epipolar_inlier(S.bestF, q.x, q.y, q.z, q.w, ts) ? 1 : 0;
    }
  } else if (!lmeds && S.max_good > 0 && !S.failed_first) {
    for (int i = tid; i < count; i += nt) {
      const float4 q = pts(i);
      mask[i] = epipolar_inlier(S.bestF, q.x, q.y, q.z, q.w, t) ? 1 : 0;
    }
  } else {
    for (int i = tid; i < count; i += nt) mask[i] = 1;
  }
  __syncthreads();
  RS_STAMP(5);
#undef RS_STAMP
}

}  // namespace

extern "C" {

__global__ __launch_bounds__(256) void ransac_only_kernel(const float *p1, const float *p2, int n, float thresh, double conf,
                                                          uint8_t *mask) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  RansacShared &R = *reinterpret_cast<RansacShared *>(smem_raw);
  fundamental_ransac_block(R, GlobalPts{p1, p2}, n, thresh, conf, mask);
}

}  // extern "C"

// findFundamentalMat for many independent point sets in one launch (the loop detector's geometric check): problem p =
// p1 / p2 [p][stride][2] with count[p] pairs, one workgroup each, the same block routine as vio_fundamental_ransac.
// A problem with fewer than min_count pairs is left alone (its mask is not written).
__global__ __launch_bounds__(256) void ransac_batch_kernel(const float *p1, const float *p2, const int *count, int stride, int min_count,
                                                           float thresh, double conf, uint8_t *mask) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  RansacShared &R = *reinterpret_cast<RansacShared *>(smem_raw);
  const int p = blockIdx.x, n = count[p];
  if (n < min_count || n > stride) return;  // (uniform per workgroup)
  fundamental_ransac_block(R, GlobalPts{p1 + 2 * (size_t)p * stride, p2 + 2 * (size_t)p * stride}, n, thresh, conf, mask + (size_t)p * stride);
}
