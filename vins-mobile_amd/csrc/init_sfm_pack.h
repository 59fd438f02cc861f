// init_sfm_pack.h — host side of vio_init_sfm_solve (init_core.h): its argument checks, the packing of a group of problems
// into the launch layouts of the three stages (the bundle adjustment's is sfm_pack.h's: after a successful construct,
// point_ok[j] is exactly "landmark j has at least two observations" and l is an input, so its integer tables and xy need
// nothing from the device), and the way back. Shared by vio_init_sfm.hip and the emulator glue of the tests.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "init_core.h"
#include "sfm_pack.h"

namespace vio {
namespace isfm {

struct Shape {
  sfm::Shape ba;   // frames, landmarks seen at least twice, their observations
  int ncorr;       // mode 1: landmarks seen in both frame l and the last
  int max_entries; // longest list of tracked landmarks of an extra frame
};

// VIO_EINVAL, then what the kernels cannot take (VIO_ECAP). Nothing is written.
inline int check_problem(const VioInitSfmProblem &P, Shape *s) {
  if (P.frame_num < 2 || P.l < 0 || P.l >= P.frame_num - 1 || P.n_features < 0 || !P.feat_start || !P.obs_frame || !P.obs_xy || !P.q ||
      !P.T || P.relative_mode < 0 || P.relative_mode > 1 || P.n_extra < 0)
    return VIO_EINVAL;
  if (P.n_extra > 0 && (!P.extra_guess || !P.extra_start || !P.extra_feature || !P.extra_xy || !P.extra_R || !P.extra_T)) return VIO_EINVAL;
  if (P.feat_start[0] < 0) return VIO_EINVAL;
  for (int j = 0; j < P.n_features; j++) {
    if (P.feat_start[j + 1] < P.feat_start[j]) return VIO_EINVAL;
    for (int k = P.feat_start[j]; k < P.feat_start[j + 1]; k++)
      if (P.obs_frame[k] < 0 || P.obs_frame[k] >= P.frame_num) return VIO_EINVAL;
  }
  if (P.n_extra > 0 && P.extra_start[0] < 0) return VIO_EINVAL;
  for (int e = 0; e < P.n_extra; e++) {
    if (P.extra_guess[e] < 0 || P.extra_guess[e] >= P.frame_num || P.extra_start[e + 1] < P.extra_start[e]) return VIO_EINVAL;
    for (int k = P.extra_start[e]; k < P.extra_start[e + 1]; k++)
      if (P.extra_feature[k] < 0 || P.extra_feature[k] >= P.n_features) return VIO_EINVAL;
  }
  if (P.frame_num > kMaxFrames) return VIO_ECAP;
  s->ba.F = P.frame_num, s->ba.np = 0, s->ba.nobs = 0, s->ncorr = 0, s->max_entries = 0;
  for (int j = 0; j < P.n_features; j++) {
    const int no = P.feat_start[j + 1] - P.feat_start[j];
    unsigned seen = 0;
    for (int k = P.feat_start[j]; k < P.feat_start[j + 1]; k++) {
      if (no >= 2 && (seen >> P.obs_frame[k] & 1u)) return VIO_ECAP;
      seen |= 1u << P.obs_frame[k];
    }
    if (no >= 2) s->ba.np++, s->ba.nobs += no;
    if (P.relative_mode == 1 && (seen >> P.l & 1u) && (seen >> (P.frame_num - 1) & 1u)) s->ncorr++;
  }
  for (int e = 0; e < P.n_extra; e++) {
    int cnt = 0;
    for (int k = P.extra_start[e]; k < P.extra_start[e + 1]; k++) {
      const int j = P.extra_feature[k];
      cnt += P.feat_start[j + 1] - P.feat_start[j] >= 2;
    }
    s->max_entries = std::max(s->max_entries, cnt);
  }
  return VIO_OK;
}

// One group (all of one bundle adjustment layout), packed.
struct HostInit {
  int n = 0, Cm = 1, Em = 1, U = 0, E = 0;
  sfm::HostBatch hb;
  std::vector<int> hint, units, ex_point, guess, unit0;  // unit0 [n]: a problem's first unit (its inversion; extras follow)
  std::vector<double> hin, ex_xy;
  std::vector<std::vector<uint8_t>> ok;  // per problem: landmark seen at least twice
};

inline void pack(const VioInitSfmProblem *pr, const Shape *sh, int n, HostInit &h) {
  h.n = n, h.Cm = 1, h.Em = 1, h.U = 0, h.E = 0;
  h.ok.assign(n, std::vector<uint8_t>());
  std::vector<VioInitBaProblem> ba(n);
  std::vector<sfm::Shape> bs(n);
  std::vector<std::vector<double>> zeros(n);
  for (int b = 0; b < n; b++) {
    const VioInitSfmProblem &P = pr[b];
    h.Cm = std::max(h.Cm, sh[b].ncorr), h.Em = std::max(h.Em, sh[b].max_entries);
    h.ok[b].resize((size_t)P.n_features + 1);
    for (int j = 0; j < P.n_features; j++) h.ok[b][j] = P.feat_start[j + 1] - P.feat_start[j] >= 2;
    zeros[b].assign(std::max((size_t)4 * P.frame_num, (size_t)3 * P.n_features) + 4, 0.0);
    VioInitBaProblem &A = ba[b];
    A.frame_num = P.frame_num, A.l = P.l, A.n_points = P.n_features;
    A.c_rotation = A.c_translation = A.points = zeros[b].data();  // (the head fills cq | ct | X on the device)
    A.point_ok = h.ok[b].data(), A.feat_start = P.feat_start, A.obs_frame = P.obs_frame, A.obs_xy = P.obs_xy, A.ok = 0;
    bs[b] = sh[b].ba;
  }
  sfm::pack(ba.data(), bs.data(), n, h.hb);
  const size_t hs = hin_stride(h.Cm);
  h.hint.assign(4 * (size_t)n, 0), h.hin.assign(hs * n, 0.0);
  h.units.clear(), h.ex_point.clear(), h.guess.clear(), h.ex_xy.clear(), h.unit0.assign(n, 0);
  for (int b = 0; b < n; b++) {
    const VioInitSfmProblem &P = pr[b];
    int *hi = &h.hint[4 * (size_t)b];
    double *hd = &h.hin[hs * b];
    hi[0] = P.relative_mode, hi[1] = sh[b].ncorr, hi[2] = P.relative_mode == 1 && P.R_hint ? 1 : 0;
    if (P.relative_mode == 0) memcpy(hd, P.relative_R, 72), memcpy(hd + 9, P.relative_T, 24);
    if (hi[2]) memcpy(hd + 12, P.R_hint, 72);
    std::vector<int> compact(P.n_features + 1, -1);
    int np = 0, nc = 0;
    for (int j = 0; j < P.n_features; j++) {
      if (h.ok[b][j]) compact[j] = np++;
      if (P.relative_mode != 1) continue;
      int k0 = -1, k1 = -1;
      for (int k = P.feat_start[j]; k < P.feat_start[j + 1]; k++) {
        if (P.obs_frame[k] == P.l) k0 = k;
        if (P.obs_frame[k] == P.frame_num - 1) k1 = k;
      }
      if (k0 < 0 || k1 < 0) continue;
      hd[24 + 2 * nc] = P.obs_xy[2 * k0], hd[24 + 2 * nc + 1] = P.obs_xy[2 * k0 + 1];
      hd[24 + 2 * (size_t)h.Cm + 2 * nc] = P.obs_xy[2 * k1], hd[24 + 2 * (size_t)h.Cm + 2 * nc + 1] = P.obs_xy[2 * k1 + 1];
      nc++;
    }
    h.unit0[b] = (int)h.guess.size();
    h.units.insert(h.units.end(), {b, -1, 0, 0}), h.guess.push_back(0);
    for (int e = 0; e < P.n_extra; e++) {
      const int first = (int)h.ex_point.size();
      for (int k = P.extra_start[e]; k < P.extra_start[e + 1]; k++) {
        const int p = compact[P.extra_feature[k]];
        if (p < 0) continue;  // not tracked (VINS.cpp:969-971)
        h.ex_point.push_back(p), h.ex_xy.push_back(P.extra_xy[2 * k]), h.ex_xy.push_back(P.extra_xy[2 * k + 1]);
      }
      h.units.insert(h.units.end(), {b, e, first, (int)h.ex_point.size() - first}), h.guess.push_back(P.extra_guess[e]);
    }
  }
  h.U = (int)h.guess.size(), h.E = (int)h.ex_point.size();
  if (h.ex_point.empty()) h.ex_point.push_back(0), h.ex_xy.resize(2, 0.0);
}

// What comes back: two arrays, doubles and ints, in these segments.
struct OutLayout {
  size_t d_out, d_sd, d_rel, d_qT, d_ex, d_total;
  size_t i_si, i_status, i_flag, i_baok, i_total;
};
inline OutLayout out_layout(const HostInit &h) {
  OutLayout L;
  const size_t n = h.n;
  L.d_out = 0, L.d_sd = L.d_out + sfm::dbl_stride(h.hb.Fm, h.hb.Pm, 0) * n, L.d_rel = L.d_sd + n * kStatsDoubles;
  L.d_qT = L.d_rel + 12 * n, L.d_ex = L.d_qT + 7 * (size_t)h.hb.Fm * n, L.d_total = L.d_ex + 12 * (size_t)h.U;
  L.i_si = 0, L.i_status = L.i_si + n * kStatsInts, L.i_flag = L.i_status + 4 * n, L.i_baok = L.i_flag + h.U, L.i_total = L.i_baok + n;
  return L;
}

// Outputs of problem b. The verdicts in the reference's order: relativePose, construct's chain, its bundle adjustment,
// the extra frames in list order.
inline void unpack(const HostInit &h, const OutLayout &L, const double *od, const int *oi, int b, VioInitSfmProblem &P, VioSolveStats *st) {
  const int Fm = h.hb.Fm, Pm = h.hb.Pm, F = P.frame_num;
  const int head = oi[L.i_status + 4 * b];
  if (P.relative_mode == 1) {
    P.inliers = oi[L.i_status + 4 * b + 1];
    if (h.hint[4 * (size_t)b + 1] >= 9) memcpy(P.relative_R, od + L.d_rel + 12 * (size_t)b, 72), memcpy(P.relative_T, od + L.d_rel + 12 * (size_t)b + 9, 24);
  }
  if (st) memset(st, 0, sizeof(*st));
  if (head != VIO_INIT_SFM_OK) {
    P.status = head;
    return;
  }
  if (st) unpack_solve_stats(od + L.d_sd + (size_t)b * kStatsDoubles, oi + L.i_si + (size_t)b * kStatsInts, st);
  const double *o = od + L.d_out + sfm::dbl_stride(Fm, Pm, 0) * b;
  int np = 0;
  for (int j = 0; j < P.n_features; j++) {
    if (P.point_ok) P.point_ok[j] = h.ok[b][j];
    if (h.ok[b][j]) {
      if (P.points) memcpy(P.points + 3 * (size_t)j, o + 7 * Fm + 3 * np, 24);
      np++;
    }
  }
  if (!oi[L.i_baok + b]) {
    P.status = VIO_INIT_SFM_FAIL_BA;
    return;
  }
  const double *qT = od + L.d_qT + 7 * (size_t)Fm * b;
  memcpy(P.q, qT, sizeof(double) * 4 * F), memcpy(P.T, qT + 4 * Fm, sizeof(double) * 3 * F);
  P.status = VIO_INIT_SFM_OK;
  for (int e = 0; e < P.n_extra; e++) {
    const int u = h.unit0[b] + 1 + e, flag = oi[L.i_flag + u];
    if (flag == 1 || flag == 3) memcpy(P.extra_R + 9 * (size_t)e, od + L.d_ex + 12 * (size_t)u, 72), memcpy(P.extra_T + 3 * (size_t)e, od + L.d_ex + 12 * (size_t)u + 9, 24);
    if (flag != 1 && P.status == VIO_INIT_SFM_OK) P.status = VIO_INIT_SFM_FAIL_PNP;
  }
}

}  // namespace isfm
}  // namespace vio
