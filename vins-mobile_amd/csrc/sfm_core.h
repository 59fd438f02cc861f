// sfm_core.h — the closing bundle adjustment of GlobalSFM::construct (VINS_ios/inital_sfm.cpp:229-296) for a batch of
// independent problems, one workgroup per problem: 256 work-items in the small layout (up to kSmallFrames frames), 512 in
// the large one (struct Large below, up to 32 frames). Single source: vio_sfm.hip compiles it for gfx950;
// tests/emul/simt_sfm.cpp and simt_sfm_large.cpp compile the same text for the host with -DVIO_SIMT, every work-item a fiber of tests/emul/simt.h
// (the kernel uses nothing but s_barrier between its phases, which that emulator supports in full).
//
// The arithmetic is init::bundle_adjust's (vio_initial.cpp), which restates Ceres' TrustRegionMinimizer /
// LevenbergMarquardtStrategy / DENSE_SCHUR iterate by iterate; the comments there carry the Ceres line references. What
// differs is who computes what:
//   * an observation belongs to one work-item per pass (residual, the 2x6 camera and 2x3 point Jacobians, later the scaled
//     coupling block Hs = S_c J_c^T J_p S_p and W = Hs E^-1); these live in a per-problem slab of global memory, one
//     column per observation (View::ob);
//   * a landmark belongs to one work-item (H_pp, g_p, the Cholesky inverse of its 3x3 e-block, its part of the step),
//     state in LDS while it fits, else in a second global slab (the PP template parameter);
//   * an entry (a, b) of the reduced camera matrix belongs to one work-item, which walks the observation list of a's
//     frame (CSR by frame, built on the host, ascending observation index) and looks the landmark's observation in b's
//     frame up in a landmark x frame table: the Schur term is formed per landmark from that landmark's own blocks, the
//     dense nc x 3np intermediates of the host code never exist, and every sum over landmarks runs in the order the
//     problem fixes -- the host code's order. No floating-point atomics anywhere.
//   * sums over everything (cost, model cost change, step norm, |x|) are block reductions with a fixed tree; the
//     back-substitution of the camera system runs column by column, which accumulates a row's terms from the last
//     column down instead of up. Those two are the only places where the order of a sum differs from the host code's.
// All control flow of the trust-region loop depends on values every work-item reads from the same LDS words, so the
// workgroup stays uniform; a problem ends at its own iteration and its workgroup leaves.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "solve_trace.h"
#include "spmd.h"
#include "vio_amd.h"
#include "vio_math.h"

namespace vio {
namespace sfm {

constexpr int kThreads = 256;
constexpr int kMaxFrames = VIO_INIT_BA_MAX_FRAMES;
constexpr int kLdsBudget = 80 * 1024;  // two workgroups per CU (160 KB of LDS): landmark state moves to global memory beyond it
constexpr int kSmallFrames = 16;       // a problem of up to 16 frames runs the small layout, every other one the large layout
constexpr int kLdsMax = 160 * 1024;    // what one workgroup may declare

// The two layouts of a workgroup. They fix the number of work-items, how the reduced camera matrix is stored and where
// the diagonal camera blocks live; the arithmetic of an entry, a landmark or an observation is the same text for both.
//   Small: the full nc x nc square in LDS (its lower triangle is used), H_cc and the reductions' scratch in LDS.
//   Large: the lower triangle packed row by row, entry (i, j) at i (i + 1) / 2 + j: 139 128 B at 32 frames, where the
//          square would take 277 KB. H_cc, read once per matrix entry, lives in the problem's global slab (View::hcc), and
//          so does the landmark state. The scratch of the block reductions is the head of S: every reduction of the
//          solve runs while S is dead (each linear_solve builds S from nothing, its back-substitution reads it last). One
//          workgroup per CU fits, so it has 512 work-items: two waves per SIMD keep the loads of twice as many matrix
//          entries in flight during the walks.
struct Small {
  static constexpr int kThreads = sfm::kThreads;
  static constexpr bool kPacked = false;
  typedef ldsd HccPtr;
};
struct Large {
  static constexpr int kThreads = 512;
  static constexpr bool kPacked = true;
  typedef double *HccPtr;
};

// per-observation slab. Rows (SoA: row r of observation k at ob[r * ostride + k]) for what one pass writes and an owner
// walks element by element: Jacobians, residual, cost term. Then one block of 36 per observation (AoS, at
// ob[kObsRows * ostride + 36 k]) for the scaled coupling block Hs [6][3] and W = Hs E^-1 [6][3]: the walks of the reduced
// matrix read three consecutive values of one row.
enum { OB_JC = 0, OB_JX = 12, OB_R = 18, OB_COST = 20, kObsRows = 21, OB_HS = 0, OB_W = 18, kObsBlock = 36, kObsDoubles = kObsRows + kObsBlock };
constexpr int kWalk = 8;  // observations of a frame's list an owner has in flight: their loads do not wait for one another
// per-landmark state, SoA: field f of landmark p at pt[f * pts + p]
enum { PT_X = 0 /* two sets of 3 */, PT_HPP = 6, PT_GP = 15, PT_EINV = 18, PT_SP = 27, PT_DG = 30, PT_Y = 33, kPointDoubles = 36 };

// One launch: n problems padded to the launch's largest frame / landmark / observation counts.
//   ints    [n][int_stride]: hdr[8] = F, l, np, nobs, nc | off_q[Fm] | off_t[Fm] | fr_start[Fm+1] | pt_start[Pm+1] |
//           obs_frame[Om] | obs_point[Om] | fr_obs[Om] | fr_point[Om] | pf_obs[Pm*Fm]
//   in/out  [n][dbl_stride]: cq[4Fm] | ct[3Fm] | X[3Pm] | xy[2Om] (out: no xy)
struct Batch {
  int n, Fm, Pm, Om;
  const int *ints;
  const double *in;
  double *out, *ob, *slab, *stats_d;
  int *stats_i;
  double *hcc = nullptr;  // large layout only: [n][36 Fm], the diagonal camera blocks
};
VIO_HD size_t int_stride(int Fm, int Pm, int Om) { return 8 + 2 * (size_t)Fm + (Fm + 1) + (Pm + 1) + 4 * (size_t)Om + (size_t)Pm * Fm; }
VIO_HD size_t dbl_stride(int Fm, int Pm, int Om) { return 7 * (size_t)Fm + 3 * (size_t)Pm + 2 * (size_t)Om; }

struct View {
  int F, l, np, nobs, nc;
  const int *off_q, *off_t, *fr_start, *pt_start, *obs_frame, *obs_point, *fr_obs, *fr_point, *pf_obs;
  double *blk;  // the Hs | W blocks: ob + kObsRows * ostride
  const double *cq0, *ct0, *X0, *xy;
  double *out_cq, *out_ct, *out_X;
  double *ob;
  size_t ostride;
  double *slab;  // landmark state when it is not in LDS: [kPointDoubles][Pm]
  int slab_stride;
  double *hcc;   // large layout: the diagonal camera blocks [F][6][6]
  double *stats_d;
  int *stats_i;
};

VIO_HD View view_of(const Batch &B, int b) {
  const int Fm = B.Fm, Pm = B.Pm, Om = B.Om;
  const int *h = B.ints + (size_t)b * int_stride(Fm, Pm, Om);
  View v;
  v.F = h[0], v.l = h[1], v.np = h[2], v.nobs = h[3], v.nc = h[4];
  v.off_q = h + 8, v.off_t = v.off_q + Fm, v.fr_start = v.off_t + Fm, v.pt_start = v.fr_start + Fm + 1;
  v.obs_frame = v.pt_start + Pm + 1, v.obs_point = v.obs_frame + Om, v.fr_obs = v.obs_point + Om, v.fr_point = v.fr_obs + Om, v.pf_obs = v.fr_point + Om;
  const double *in = B.in + (size_t)b * dbl_stride(Fm, Pm, Om);
  v.cq0 = in, v.ct0 = in + 4 * Fm, v.X0 = in + 7 * Fm, v.xy = in + 7 * Fm + 3 * Pm;
  double *out = B.out + (size_t)b * dbl_stride(Fm, Pm, 0);
  v.out_cq = out, v.out_ct = out + 4 * Fm, v.out_X = out + 7 * Fm;
  v.ob = B.ob + (size_t)b * kObsDoubles * (size_t)Om, v.ostride = (size_t)Om;
  v.blk = v.ob + (size_t)kObsRows * Om;
  v.slab = B.slab ? B.slab + (size_t)b * kPointDoubles * (size_t)Pm : nullptr, v.slab_stride = Pm;
  v.hcc = B.hcc ? B.hcc + (size_t)b * 36 * (size_t)Fm : nullptr;
  v.stats_d = B.stats_d + (size_t)b * kStatsDoubles, v.stats_i = B.stats_i + (size_t)b * kStatsInts;
  return v;
}

// LDS of one workgroup. PP: where the landmark state lives (ldsd, or double * for the global slab).
template <class PP, class L = Small>
struct Work {
  typedef L Layout;
  ldsd S;                       // reduced camera matrix, lower triangle (row stride nc, or packed); its Cholesky factor below the diagonal
  ldsd Ld, v, z, yc;            // the factor's diagonal; right-hand side / forward / backward work vectors: nc each
  ldsd gc, sc, dg;              // camera gradient (unscaled), Jacobi scaling, LM diagonal
  typename L::HccPtr Hcc;       // [F][6][6] diagonal camera blocks (unscaled; rotation columns 0-2, translation 3-5)
  ldsd R;                       // [F][9] rotations of the pose set under evaluation
  ldsd pose;                    // two pose sets of [4F | 3F]: iterate and candidate
  ldsd red;                     // [3][L::kThreads] reductions (large layout: the head of S)
  ldsi col_frame, col_li, flag; // frame and local column (0-5) of a camera column; flag[0]: every e-block factored
  PP pt;
  int pts;
};

VIO_HD int max_columns(int F) { return 6 * F - 6; }  // l == F - 1 keeps one translation constant only
VIO_HD size_t lds_doubles(int Fm) {
  const size_t ncm = (size_t)max_columns(Fm);
  return ncm * ncm + 7 * ncm + (36 + 9 + 14) * (size_t)Fm + 3 * kThreads;
}
VIO_HD size_t lds_ints(int Fm) { return 2 * (size_t)max_columns(Fm) + 4; }
// bytes of dynamic LDS; lds_points: landmarks whose state is kept in LDS (0: the global slab)
VIO_HD size_t lds_bytes(int Fm, int lds_points) {
  return (lds_doubles(Fm) + (size_t)kPointDoubles * lds_points) * sizeof(double) + lds_ints(Fm) * sizeof(int);
}
VIO_HD bool points_fit_lds(int Fm, int Pm) { return lds_bytes(Fm, Pm) <= (size_t)kLdsBudget; }

template <class PP>
VIO_DEV void carve(int Fm, ldsd base, PP pt, int pts, Work<PP> *w) {
  const int ncm = max_columns(Fm);
  ldsd p = base;
  w->S = p, p += (size_t)ncm * ncm;
  w->Ld = p, p += ncm, w->v = p, p += ncm, w->z = p, p += ncm, w->yc = p, p += ncm;
  w->gc = p, p += ncm, w->sc = p, p += ncm, w->dg = p, p += ncm;
  w->Hcc = p, p += 36 * Fm, w->R = p, p += 9 * Fm, w->pose = p, p += 14 * Fm, w->red = p, p += 3 * kThreads;
  ldsd after = p;
  if (pt == nullptr) pt = (PP)p, after = p + (size_t)kPointDoubles * pts;
  w->pt = pt, w->pts = pts;
  ldsi q = (ldsi)after;
  w->col_frame = q, q += ncm, w->col_li = q, q += ncm, w->flag = q;
}

// ---- the large layout's LDS: S packed | seven nc-vectors | R | pose | integer tables ----
constexpr size_t large_s_doubles_of(size_t Fm) {  // (the reductions' scratch is the larger one below 14 frames only: a small problem forced here)
  return (6 * Fm - 6) * (6 * Fm - 5) / 2 > 3 * (size_t)Large::kThreads ? (6 * Fm - 6) * (6 * Fm - 5) / 2 : 3 * (size_t)Large::kThreads;
}
constexpr size_t large_lds_bytes_of(size_t Fm) {
  return (large_s_doubles_of(Fm) + 7 * (6 * Fm - 6) + (9 + 14) * Fm) * sizeof(double) + (2 * (6 * Fm - 6) + 4) * sizeof(int);
}
static_assert(large_lds_bytes_of(32) == 139128 + 10416 + 5888 + 1504, "packed triangle, seven nc-vectors, R and pose, integer tables");
static_assert(large_lds_bytes_of(32) <= (size_t)kLdsMax, "the large layout fits one workgroup's LDS at 32 frames");
VIO_HD size_t large_lds_bytes(int Fm) { return large_lds_bytes_of((size_t)Fm); }  // bytes of dynamic LDS of the large layout

VIO_DEV void carve_large(int Fm, ldsd base, const View &v, int pts, Work<double *, Large> *w) {
  const int ncm = max_columns(Fm);
  ldsd p = base;
  w->S = p, w->red = p, p += large_s_doubles_of((size_t)Fm);
  w->Ld = p, p += ncm, w->v = p, p += ncm, w->z = p, p += ncm, w->yc = p, p += ncm;
  w->gc = p, p += ncm, w->sc = p, p += ncm, w->dg = p, p += ncm;
  w->R = p, p += 9 * Fm, w->pose = p, p += 14 * Fm;
  w->Hcc = v.hcc, w->pt = v.slab, w->pts = pts;
  ldsi q = (ldsi)p;
  w->col_frame = q, q += ncm, w->col_li = q, q += ncm, w->flag = q;
}

// entry (i, j), j <= i, of the reduced camera matrix
template <class L>
VIO_DEV int s_at(int i, int j, int nc) {
  return L::kPacked ? i * (i + 1) / 2 + j : i * nc + j;
}

struct OpSum {
  VIO_DEV double operator()(double a, double b) const { return a + b; }
};
struct OpMax {  // std::max(a, b): a NaN on the right is dropped
  VIO_DEV double operator()(double a, double b) const { return a < b ? b : a; }
};
// v[0..N) over the workgroup, the same tree for every problem and every launch; every work-item gets the result.
template <int kThreads, int N, class OP>
VIO_DEV void block_reduce(int tid, ldsd red, double (&val)[N], OP op) {
  for (int n = 0; n < N; n++) red[n * kThreads + tid] = val[n];
  __syncthreads();
  if (tid < 64)
    for (int n = 0; n < N; n++) {
      ldsd r = red + n * kThreads + tid;
      double a = r[0];
#pragma unroll
      for (int i = 64; i < kThreads; i += 64) a = op(a, r[i]);  // ((r[0] + r[64]) + r[128]) + ...: the waves in ascending order
      r[0] = a;
    }
  __syncthreads();
  for (int n = 0; n < N; n++) {
    double a = red[n * kThreads];
    for (int i = 1; i < 64; i++) a = op(a, red[n * kThreads + i]);
    val[n] = a;
  }
  __syncthreads();
}

// QuaternionParameterization::Plus on (w x y z) (vio_initial.cpp ba_quat_plus)
VIO_DEV void quat_plus(const double q[4], const double d[3], double out[4]) {
  const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (nd > 0.0) {
    const double k = sin(nd) / nd;
    const Quat dq{k * d[0], k * d[1], k * d[2], cos(nd)}, r = qmul(dq, Quat{q[1], q[2], q[3], q[0]});
    out[0] = r.w, out[1] = r.x, out[2] = r.y, out[3] = r.z;
  } else {
    for (int k = 0; k < 4; k++) out[k] = q[k];
  }
}

// camera column of local column li (0-2 rotation, 3-5 translation) of frame f, -1 = constant
VIO_DEV int column_of(const View &v, int f, int li) {
  const int o = li < 3 ? v.off_q[f] : v.off_t[f];
  return o < 0 ? -1 : o + (li < 3 ? li : li - 3);
}

// ba_evaluate: cost at pose / landmark set `s`; with jac, H_pp, g_p, H_cc and g_c of that set as well.
template <class WK>
VIO_DEV double evaluate(int tid, const View &v, const WK &w, int s, bool jac) {
  constexpr int kThreads = WK::Layout::kThreads;
  const int F = v.F, np = v.np, nobs = v.nobs, P = w.pts;
  const size_t os = v.ostride;
  ldsd pq = w.pose + s * 7 * F, ptr = pq + 4 * F;
  if (tid < F) {  // QuaternionRotatePoint normalizes its quaternion
    double R[9];
    qtoR(qnormalized(Quat{pq[4 * tid + 1], pq[4 * tid + 2], pq[4 * tid + 3], pq[4 * tid]}), R);
    for (int k = 0; k < 9; k++) w.R[9 * tid + k] = R[k];
  }
  __syncthreads();
  for (int k = tid; k < nobs; k += kThreads) {
    const int f = v.obs_frame[k], p = v.obs_point[k];
    double Ri[9], Xw[3], RX[3], Y[3];
    for (int c = 0; c < 9; c++) Ri[c] = w.R[9 * f + c];
    for (int c = 0; c < 3; c++) Xw[c] = w.pt[(PT_X + 3 * s + c) * P + p];
    mat3vec(Ri, Xw, RX);
    for (int c = 0; c < 3; c++) Y[c] = RX[c] + ptr[3 * f + c];
    const double iz = 1.0 / Y[2], r0 = Y[0] * iz - v.xy[2 * k], r1 = Y[1] * iz - v.xy[2 * k + 1];
    v.ob[OB_COST * os + k] = r0 * r0 + r1 * r1;
    if (!jac) continue;
    const double Jp[6] = {iz, 0, -Y[0] * iz * iz, 0, iz, -Y[1] * iz * iz};
    double S[9];
    skew3(RX, S);
    for (int a = 0; a < 2; a++)
      for (int c = 0; c < 3; c++) {
        v.ob[(OB_JC + a * 6 + c) * os + k] = -2.0 * (Jp[a * 3] * S[c] + Jp[a * 3 + 1] * S[3 + c] + Jp[a * 3 + 2] * S[6 + c]);
        v.ob[(OB_JC + a * 6 + 3 + c) * os + k] = Jp[a * 3 + c];
        v.ob[(OB_JX + a * 3 + c) * os + k] = Jp[a * 3] * Ri[c] + Jp[a * 3 + 1] * Ri[3 + c] + Jp[a * 3 + 2] * Ri[6 + c];
      }
    v.ob[OB_R * os + k] = r0, v.ob[(OB_R + 1) * os + k] = r1;
  }
  __syncthreads();
  double cost[1] = {0.0};
  for (int k = tid; k < nobs; k += kThreads) cost[0] += v.ob[OB_COST * os + k];
  if (jac) {
    for (int p = tid; p < np; p += kThreads) {  // the landmark's observations in their order
      double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
      for (int k = v.pt_start[p]; k < v.pt_start[p + 1]; k++) {
        double JX[6];
        for (int c = 0; c < 6; c++) JX[c] = v.ob[(OB_JX + c) * os + k];
        const double r0 = v.ob[OB_R * os + k], r1 = v.ob[(OB_R + 1) * os + k];
        for (int a = 0; a < 3; a++) {
          g[a] += JX[a] * r0 + JX[3 + a] * r1;
          for (int b = 0; b < 3; b++) H[a * 3 + b] += JX[a] * JX[b] + JX[3 + a] * JX[3 + b];
        }
      }
      for (int c = 0; c < 9; c++) w.pt[(PT_HPP + c) * P + p] = H[c];
      for (int c = 0; c < 3; c++) w.pt[(PT_GP + c) * P + p] = g[c];
    }
    for (int e = tid; e < 42 * F; e += kThreads) {  // the frame's observations in ascending order: the host code's
      const int f = e / 42, j = e - 42 * f;
      const int a = j < 36 ? j / 6 : j - 36, b = j < 36 ? j - 6 * a : 0;
      double acc = 0.0;
      const int rb = j < 36 ? OB_JC + b : OB_R, rb1 = j < 36 ? OB_JC + 6 + b : OB_R + 1, end = v.fr_start[f + 1];
      for (int i0 = v.fr_start[f]; i0 < end; i0 += kWalk) {
        double ja0[kWalk], ja1[kWalk], jb0[kWalk], jb1[kWalk];
#pragma unroll
        for (int u = 0; u < kWalk; u++) {
          const int k = v.fr_obs[i0 + u < end ? i0 + u : end - 1];
          ja0[u] = v.ob[(OB_JC + a) * os + k], ja1[u] = v.ob[(OB_JC + 6 + a) * os + k], jb0[u] = v.ob[rb * os + k], jb1[u] = v.ob[rb1 * os + k];
        }
#pragma unroll
        for (int u = 0; u < kWalk; u++)
          if (i0 + u < end) acc += ja0[u] * jb0[u] + ja1[u] * jb1[u];
      }
      if (j < 36) {
        w.Hcc[36 * f + j] = acc;
      } else {
        const int col = column_of(v, f, a);
        if (col >= 0) w.gc[col] = acc;
      }
    }
  }
  block_reduce<kThreads>(tid, w.red, cost, OpSum());
  return 0.5 * cost[0];
}

// |Plus(x, -g) - x|_inf (trust_region_minimizer.cc:270-284) at pose set s
template <class WK>
VIO_DEV double gradient_max(int tid, const View &v, const WK &w, int s) {
  constexpr int kThreads = WK::Layout::kThreads;
  const int F = v.F, np = v.np, P = w.pts;
  double m[1] = {0.0};
  OpMax mx;
  for (int p = tid; p < np; p += kThreads)
    for (int c = 0; c < 3; c++) m[0] = mx(m[0], fabs(w.pt[(PT_GP + c) * P + p]));
  if (tid < F) {
    const int i = tid;
    if (v.off_t[i] >= 0)
      for (int k = 0; k < 3; k++) m[0] = mx(m[0], fabs(w.gc[v.off_t[i] + k]));
    if (v.off_q[i] >= 0) {
      double q[4], qn[4], d[3];
      for (int k = 0; k < 4; k++) q[k] = w.pose[s * 7 * F + 4 * i + k];
      for (int k = 0; k < 3; k++) d[k] = -w.gc[v.off_q[i] + k];
      quat_plus(q, d, qn);
      for (int k = 0; k < 4; k++) m[0] = mx(m[0], fabs(qn[k] - q[k]));
    }
  }
  block_reduce<kThreads>(tid, w.red, m, mx);
  return m[0];
}

// Hs = S_c J_c^T J_p S_p of every observation (the scaling is fixed after iteration 0, so once per accepted iterate)
template <class WK>
VIO_DEV void scaled_blocks(int tid, const View &v, const WK &w) {
  constexpr int kThreads = WK::Layout::kThreads;
  const size_t os = v.ostride;
  const int P = w.pts;
  for (int k = tid; k < v.nobs; k += kThreads) {
    const int f = v.obs_frame[k], p = v.obs_point[k];
    double JX[6], sp[3];
    for (int c = 0; c < 6; c++) JX[c] = v.ob[(OB_JX + c) * os + k];
    for (int c = 0; c < 3; c++) sp[c] = w.pt[(PT_SP + c) * P + p];
    for (int li = 0; li < 6; li++) {
      const int col = column_of(v, f, li);
      const double j0 = v.ob[(OB_JC + li) * os + k], j1 = v.ob[(OB_JC + 6 + li) * os + k], sc = col >= 0 ? w.sc[col] : 0.0;
      for (int c = 0; c < 3; c++) v.blk[(size_t)kObsBlock * k + OB_HS + li * 3 + c] = col >= 0 ? sc * (j0 * JX[c] + j1 * JX[3 + c]) * sp[c] : 0.0;
    }
  }
  __syncthreads();
}

// ba_solve: (Hs + D^2) y = gs with D^2 = dg / radius. y: PT_Y of every landmark and w.yc. False where the host code's
// returns false (an e-block or the reduced matrix not positive definite, a non-finite step).
template <class WK>
VIO_DEV bool linear_solve(int tid, const View &v, const WK &w, double radius, double *a_out, double *b_out) {
  typedef typename WK::Layout L;
  constexpr int kThreads = L::kThreads;
  const int np = v.np, nc = v.nc, nobs = v.nobs, P = w.pts;
  const size_t os = v.ostride;
  // (the caller's barrier after the diagonal phase has passed; flag[0] == 1)
  for (int p = tid; p < np; p += kThreads) {
    double M[9], sp[3];
    for (int a = 0; a < 3; a++) sp[a] = w.pt[(PT_SP + a) * P + p];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) M[a * 3 + b] = sp[a] * w.pt[(PT_HPP + a * 3 + b) * P + p] * sp[b];
    for (int a = 0; a < 3; a++) M[a * 3 + a] += w.pt[(PT_DG + a) * P + p] / radius;
    // inverse through the Cholesky factor of the 3x3 block (schur_eliminator_impl.h:258-262 InvertPSDMatrix)
    const double l00 = sqrt(M[0]), l10 = M[3] / l00, l20 = M[6] / l00;
    const double l11 = sqrt(M[4] - l10 * l10), l21 = (M[7] - l20 * l10) / l11, l22 = sqrt(M[8] - l20 * l20 - l21 * l21);
    if (!(l00 > 0.0) || !(l11 > 0.0) || !(l22 > 0.0)) w.flag[0] = 0;
    const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
    const double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22, i20 = -(l20 * i00 + l21 * i10) * i22;
    double I[9];
    I[0] = i00 * i00 + i10 * i10 + i20 * i20, I[1] = I[3] = i10 * i11 + i20 * i21, I[2] = I[6] = i20 * i22;
    I[4] = i11 * i11 + i21 * i21, I[5] = I[7] = i21 * i22, I[8] = i22 * i22;
    for (int c = 0; c < 9; c++) w.pt[(PT_EINV + c) * P + p] = I[c];
  }
  __syncthreads();
  const bool blocks_ok = w.flag[0] != 0;
  __syncthreads();  // (everyone has read the flag before it is set again)
  if (!blocks_ok) {
    if (tid == 0) w.flag[0] = 1;
    __syncthreads();
    return false;
  }
  for (int k = tid; k < nobs; k += kThreads) {  // W = Hs E^-1
    const int p = v.obs_point[k];
    double I[9];
    for (int c = 0; c < 9; c++) I[c] = w.pt[(PT_EINV + c) * P + p];
    for (int li = 0; li < 6; li++) {
      double *bk = v.blk + (size_t)kObsBlock * k;
      const double h0 = bk[OB_HS + li * 3], h1 = bk[OB_HS + li * 3 + 1], h2 = bk[OB_HS + li * 3 + 2];
      for (int c = 0; c < 3; c++) bk[OB_W + li * 3 + c] = h0 * I[c] + h1 * I[3 + c] + h2 * I[6 + c];
    }
  }
  __syncthreads();
  // reduced camera matrix, lower triangle: entry (a, b) walks the observations of a's frame
  // (the large layout enumerates the packed entries themselves; the square's e < nc * nc idles the lanes above the diagonal)
  for (int e = tid; e < (L::kPacked ? nc * (nc + 1) / 2 : nc * nc); e += kThreads) {
    int a, b;
    if (L::kPacked) {
      a = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
      while (a * (a + 1) / 2 > e) a--;  // (the root is exact at these sizes; the two loops make that no assumption)
      while ((a + 1) * (a + 2) / 2 <= e) a++;
      b = e - a * (a + 1) / 2;
    } else {
      a = e / nc, b = e - a * nc;
      if (b > a) continue;
    }
    const int fa = w.col_frame[a], fb = w.col_frame[b], la = w.col_li[a], lb = w.col_li[b];
    double sum = fa == fb ? w.sc[a] * w.Hcc[36 * fa + 6 * la + lb] * w.sc[b] : 0.0;
    const int end = v.fr_start[fa + 1];
    for (int i0 = v.fr_start[fa]; i0 < end; i0 += kWalk) {  // kWalk observations in flight, summed in the list's order
      int k[kWalk], k2[kWalk];
      double wv[kWalk][3], hv[kWalk][3];
#pragma unroll
      for (int u = 0; u < kWalk; u++) {
        const int i = i0 + u < end ? i0 + u : end - 1;
        k[u] = v.fr_obs[i], k2[u] = v.fr_point[i];
      }
#pragma unroll
      for (int u = 0; u < kWalk; u++) k2[u] = i0 + u >= end ? -1 : (fa == fb ? k[u] : v.pf_obs[k2[u] * v.F + fb]);
#pragma unroll
      for (int u = 0; u < kWalk; u++)
        for (int c = 0; c < 3; c++) {
          wv[u][c] = v.blk[(size_t)kObsBlock * k[u] + OB_W + la * 3 + c];
          hv[u][c] = v.blk[(size_t)kObsBlock * (k2[u] < 0 ? 0 : k2[u]) + OB_HS + lb * 3 + c];
        }
#pragma unroll
      for (int u = 0; u < kWalk; u++)
        if (k2[u] >= 0)
          for (int c = 0; c < 3; c++) sum -= wv[u][c] * hv[u][c];
    }
    if (a == b) sum += w.dg[a] / radius;
    w.S[s_at<L>(a, b, nc)] = sum;
  }
  for (int a = tid; a < nc; a += kThreads) {  // rhs = gs_c - W gs_p
    const int fa = w.col_frame[a], la = w.col_li[a];
    double acc = w.sc[a] * w.gc[a];
    const int end = v.fr_start[fa + 1];
    for (int i0 = v.fr_start[fa]; i0 < end; i0 += kWalk) {
      double wv[kWalk][3], gs[kWalk][3];
#pragma unroll
      for (int u = 0; u < kWalk; u++) {
        const int i = i0 + u < end ? i0 + u : end - 1, k = v.fr_obs[i], p = v.fr_point[i];
        for (int c = 0; c < 3; c++) wv[u][c] = v.blk[(size_t)kObsBlock * k + OB_W + la * 3 + c], gs[u][c] = w.pt[(PT_SP + c) * P + p] * w.pt[(PT_GP + c) * P + p];
      }
#pragma unroll
      for (int u = 0; u < kWalk; u++)
        if (i0 + u < end)
          for (int c = 0; c < 3; c++) acc -= wv[u][c] * gs[u][c];
    }
    w.v[a] = acc;
  }
  __syncthreads();
  // Eigen::LLT of the reduced camera matrix (schur_complement_solver.cc:201-213), one column per step. Every work-item
  // forms the pivot itself (broadcast reads), so the exit on a non-positive pivot is uniform.
  for (int j = 0; j < nc; j++) {
    const int rj = s_at<L>(j, 0, nc);
    double d = w.S[rj + j];
    for (int k = 0; k < j; k++) d -= w.S[rj + k] * w.S[rj + k];
    if (!(d > 0.0)) return false;  // (nobody is left behind: the previous step's barrier was passed by all)
    d = sqrt(d);
    if (tid == 0) w.Ld[j] = d;
    for (int i = j + 1 + tid; i < nc; i += kThreads) {
      const int ri = s_at<L>(i, 0, nc);
      double x = w.S[ri + j];
      for (int k = 0; k < j; k++) x -= w.S[ri + k] * w.S[rj + k];
      w.S[ri + j] = x / d;
    }
    __syncthreads();
  }
  for (int i = 0; i < nc; i++) {  // L z = rhs
    const double zi = w.v[i] / w.Ld[i];
    if (tid == 0) w.z[i] = zi;
    for (int k = i + 1 + tid; k < nc; k += kThreads) w.v[k] -= w.S[s_at<L>(k, i, nc)] * zi;
    __syncthreads();
  }
  for (int i = nc - 1; i >= 0; i--) {  // L^T yc = z
    const double yi = w.z[i] / w.Ld[i];
    if (tid == 0) w.yc[i] = yi;
    for (int k = tid; k < i; k += kThreads) w.z[k] -= w.S[s_at<L>(i, k, nc)] * yi;
    __syncthreads();
  }
  // back-substitution yp = E^-1 (gs_p - Hs_pc yc), and the three sums of the step's quality: a = y . gs, b = y . D^2 y
  double r[3] = {0.0, 0.0, 0.0};
  for (int p = tid; p < np; p += kThreads) {
    double x[3], gs[3];
    for (int a = 0; a < 3; a++) gs[a] = x[a] = w.pt[(PT_SP + a) * P + p] * w.pt[(PT_GP + a) * P + p];
    for (int a = 0; a < 3; a++)
      for (int k = v.pt_start[p]; k < v.pt_start[p + 1]; k++) {
        const int f = v.obs_frame[k];
        for (int li = 0; li < 6; li++) {
          const int col = column_of(v, f, li);
          if (col >= 0) x[a] -= v.blk[(size_t)kObsBlock * k + OB_HS + li * 3 + a] * w.yc[col];
        }
      }
    for (int a = 0; a < 3; a++) {
      const double y = w.pt[(PT_EINV + a * 3) * P + p] * x[0] + w.pt[(PT_EINV + a * 3 + 1) * P + p] * x[1] + w.pt[(PT_EINV + a * 3 + 2) * P + p] * x[2];
      w.pt[(PT_Y + a) * P + p] = y;
      r[0] += y * gs[a], r[1] += w.pt[(PT_DG + a) * P + p] / radius * y * y;
      if (!isfinite(y)) r[2] += 1.0;
    }
  }
  for (int a = tid; a < nc; a += kThreads) {
    const double y = w.yc[a];
    r[0] += y * (w.sc[a] * w.gc[a]), r[1] += w.dg[a] / radius * y * y;
    if (!isfinite(y)) r[2] += 1.0;
  }
  if (!isfinite(r[0]) || !isfinite(r[1])) r[0] = r[1] = 0.0, r[2] += 1.0;
  block_reduce<kThreads>(tid, w.red, r, OpSum());
  *a_out = r[0], *b_out = r[1];
  return r[2] == 0.0;
}

// init::bundle_adjust for one problem.
template <class PP, class L>
VIO_DEV void solve(int tid, const View &v, const Work<PP, L> &w) {
  constexpr int kThreads = L::kThreads;
  const int F = v.F, np = v.np, nc = v.nc, P = w.pts;
  for (int i = tid; i < 4 * F; i += kThreads) w.pose[i] = v.cq0[i];
  for (int i = tid; i < 3 * F; i += kThreads) w.pose[4 * F + i] = v.ct0[i];
  for (int i = tid; i < 3 * np; i += kThreads) w.pt[(PT_X + i % 3) * P + i / 3] = v.X0[i];
  if (tid < F)
    for (int li = 0; li < 6; li++) {
      const int col = column_of(v, tid, li);
      if (col >= 0) w.col_frame[col] = tid, w.col_li[col] = li;
    }
  if (tid == 0) w.flag[0] = 1;
  __syncthreads();
  int cur = 0;
  const SolveTrace tr{v.stats_d, v.stats_i};
  double x_cost = evaluate(tid, v, w, cur, true), x_norm = -1.0;
  __syncthreads();
  // Jacobi scaling, fixed at iteration 0 (trust_region_minimizer.cc:239-254)
  for (int i = tid; i < 3 * np; i += kThreads) {
    const int p = i / 3, a = i - 3 * p;
    w.pt[(PT_SP + a) * P + p] = 1.0 / (1.0 + sqrt(w.pt[(PT_HPP + 4 * a) * P + p]));
  }
  for (int a = tid; a < nc; a += kThreads) w.sc[a] = 1.0 / (1.0 + sqrt(w.Hcc[36 * w.col_frame[a] + 7 * w.col_li[a]]));
  __syncthreads();
  scaled_blocks(tid, v, w);
  double gmax = gradient_max(tid, v, w, cur), radius = 1e4, decrease_factor = 2.0;
  bool last_ok = true, reuse_diagonal = false;
  int termination = 0, invalid_run = 0, it = 0, recorded = 1, n_ok = 1, n_bad = 0;
  if (tid == 0) tr.initial(x_cost), tr.record(0, x_cost, radius, 0, 0, gmax, true, true);
  for (;;) {
    if (it >= 50) break;
    if (last_ok && gmax <= 1e-10) { termination = 1; break; }
    if (radius <= 1e-32) { termination = 1; break; }
    it++;
    if (!reuse_diagonal) {  // LevenbergMarquardtStrategy::ComputeStep (:79-89)
      for (int i = tid; i < 3 * np; i += kThreads) {
        const int p = i / 3, a = i - 3 * p;
        const double s = w.pt[(PT_SP + a) * P + p];
        w.pt[(PT_DG + a) * P + p] = fmin(fmax(s * s * w.pt[(PT_HPP + 4 * a) * P + p], 1e-6), 1e32);
      }
      for (int a = tid; a < nc; a += kThreads) w.dg[a] = fmin(fmax(w.sc[a] * w.sc[a] * w.Hcc[36 * w.col_frame[a] + 7 * w.col_li[a]], 1e-6), 1e32);
      __syncthreads();
    }
    reuse_diagonal = true;
    double a = 0.0, b = 0.0;
    const bool solver_ok = linear_solve(tid, v, w, radius, &a, &b);
    const double model_cost_change = 0.5 * (a + b);  // step = -y; -step^T (gs + Hs step / 2) with (Hs + D^2) y = gs
    if (!(solver_ok && model_cost_change > 0.0)) {
      if (++invalid_run >= 5) { termination = 2; break; }
      radius = radius / decrease_factor, decrease_factor *= 2.0;  // StepRejected (:155-159)
      last_ok = false, n_bad++;
      if (tid == 0) tr.record(it, x_cost, radius, 0, 0, gmax, false, false);
      recorded = it + 1;
      __syncthreads();
      continue;
    }
    invalid_run = 0;
    const int cand = cur ^ 1;
    double sn[1] = {0.0};
    for (int i = tid; i < 3 * np; i += kThreads) {
      const int p = i / 3, c = i - 3 * p;
      const double x = w.pt[(PT_X + 3 * cur + c) * P + p], d = -w.pt[(PT_Y + c) * P + p] * w.pt[(PT_SP + c) * P + p], xn = x + d;
      w.pt[(PT_X + 3 * cand + c) * P + p] = xn, sn[0] += (x - xn) * (x - xn);
    }
    if (tid < F) {
      const int i = tid;
      ldsd q = w.pose + cur * 7 * F + 4 * i, qn = w.pose + cand * 7 * F + 4 * i;
      ldsd t = w.pose + cur * 7 * F + 4 * F + 3 * i, tn = w.pose + cand * 7 * F + 4 * F + 3 * i;
      if (v.off_q[i] >= 0) {
        double d[3], q0[4], q1[4];
        for (int k = 0; k < 3; k++) d[k] = -w.yc[v.off_q[i] + k] * w.sc[v.off_q[i] + k];
        for (int k = 0; k < 4; k++) q0[k] = q[k];
        quat_plus(q0, d, q1);
        for (int k = 0; k < 4; k++) qn[k] = q1[k], sn[0] += (q0[k] - q1[k]) * (q0[k] - q1[k]);
      } else {
        for (int k = 0; k < 4; k++) qn[k] = q[k];
      }
      for (int k = 0; k < 3; k++) {
        if (v.off_t[i] >= 0) {
          const double d = -w.yc[v.off_t[i] + k] * w.sc[v.off_t[i] + k], x = t[k], xn = x + d;
          tn[k] = xn, sn[0] += (x - xn) * (x - xn);
        } else {
          tn[k] = t[k];
        }
      }
    }
    block_reduce<kThreads>(tid, w.red, sn, OpSum());
    double cand_cost = evaluate(tid, v, w, cand, false);
    if (!isfinite(cand_cost)) cand_cost = 1.7976931348623157e308;
    const double step_norm = sqrt(sn[0]);
    if (step_norm <= 1e-8 * (x_norm + 1e-8)) { termination = 1; break; }       // ParameterToleranceReached (:666-685)
    if (fabs(x_cost - cand_cost) <= 1e-6 * x_cost) { termination = 1; break; }  // FunctionToleranceReached (:687-704)
    const double rho = (x_cost - cand_cost) / model_cost_change;  // monotonic steps: the step evaluator's reference is x_cost
    if (rho > 1e-3) {
      cur = cand;
      double n2[1] = {0.0};
      for (int i = tid; i < 3 * np; i += kThreads) {
        const double x = w.pt[(PT_X + 3 * cur + i % 3) * P + i / 3];
        n2[0] += x * x;
      }
      if (tid < F) {
        if (v.off_q[tid] >= 0)
          for (int k = 0; k < 4; k++) n2[0] += w.pose[cur * 7 * F + 4 * tid + k] * w.pose[cur * 7 * F + 4 * tid + k];
        if (v.off_t[tid] >= 0)
          for (int k = 0; k < 3; k++) n2[0] += w.pose[cur * 7 * F + 4 * F + 3 * tid + k] * w.pose[cur * 7 * F + 4 * F + 3 * tid + k];
      }
      block_reduce<kThreads>(tid, w.red, n2, OpSum());
      x_norm = sqrt(n2[0]);
      x_cost = evaluate(tid, v, w, cur, true);
      __syncthreads();
      scaled_blocks(tid, v, w);
      gmax = gradient_max(tid, v, w, cur);
      const double q3 = 2.0 * rho - 1.0;
      radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - q3 * q3 * q3));  // StepAccepted (:146-153)
      decrease_factor = 2.0, reuse_diagonal = false, last_ok = true, n_ok++;
      if (tid == 0) tr.record(it, x_cost, radius, step_norm, rho, gmax, true, true);
    } else {
      radius = radius / decrease_factor, decrease_factor *= 2.0, reuse_diagonal = true;  // StepRejected (:155-159)
      last_ok = false, n_bad++;
      if (tid == 0) tr.record(it, cand_cost, radius, step_norm, rho, 0.0, true, false);
    }
    recorded = it + 1;
  }
  __syncthreads();
  for (int i = tid; i < 4 * F; i += kThreads) v.out_cq[i] = w.pose[cur * 7 * F + i];
  for (int i = tid; i < 3 * F; i += kThreads) v.out_ct[i] = w.pose[cur * 7 * F + 4 * F + i];
  for (int i = tid; i < 3 * np; i += kThreads) v.out_X[i] = w.pt[(PT_X + 3 * cur + i % 3) * P + i / 3];
  if (tid == 0) tr.finish(recorded, termination, n_ok, n_bad, x_cost);
}

}  // namespace sfm
}  // namespace vio
