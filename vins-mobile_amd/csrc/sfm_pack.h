// sfm_pack.h — host side of the batched bundle adjustment (sfm_core.h): the argument checks of vio_init_ba_solve and the
// packing of its problems into the launch layout (sfm::Batch). Shared by vio_sfm.hip and the emulator glue of the tests,
// so that the kernel source sees the same indices in both.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "sfm_core.h"

namespace vio {
namespace sfm {

struct Shape {
  int F, np, nobs;
};

// The checks of vio_init_bundle_adjust (VIO_EINVAL), then what the kernel cannot take (VIO_ECAP). Nothing is written.
inline int check_problem(const VioInitBaProblem &P, Shape *s) {
  if (P.frame_num < 2 || P.l < 0 || P.l >= P.frame_num || !P.c_rotation || !P.c_translation || P.n_points < 0 || !P.points ||
      !P.point_ok || !P.feat_start || !P.obs_frame || !P.obs_xy)
    return VIO_EINVAL;
  if (P.feat_start[0] < 0) return VIO_EINVAL;
  for (int j = 0; j < P.n_points; j++) {
    if (P.feat_start[j + 1] < P.feat_start[j]) return VIO_EINVAL;
    for (int k = P.feat_start[j]; k < P.feat_start[j + 1]; k++)
      if (P.obs_frame[k] < 0 || P.obs_frame[k] >= P.frame_num) return VIO_EINVAL;
  }
  if (P.frame_num > kMaxFrames) return VIO_ECAP;
  s->F = P.frame_num, s->np = 0, s->nobs = 0;
  for (int j = 0; j < P.n_points; j++) {
    if (!P.point_ok[j]) continue;
    unsigned seen = 0;  // kMaxFrames <= 32
    for (int k = P.feat_start[j]; k < P.feat_start[j + 1]; k++) {
      if (seen >> P.obs_frame[k] & 1u) return VIO_ECAP;
      seen |= 1u << P.obs_frame[k];
    }
    s->np++, s->nobs += P.feat_start[j + 1] - P.feat_start[j];
  }
  return VIO_OK;
}
static_assert(kMaxFrames <= 32, "check_problem keeps a landmark's frames in one word");

struct HostBatch {
  int n = 0, Fm = 2, Pm = 1, Om = 1;
  std::vector<int> ints;
  std::vector<double> in;
};

inline void pack(const VioInitBaProblem *pr, const Shape *sh, int n, HostBatch &hb) {
  hb.n = n, hb.Fm = 2, hb.Pm = 1, hb.Om = 1;
  for (int b = 0; b < n; b++) hb.Fm = std::max(hb.Fm, sh[b].F), hb.Pm = std::max(hb.Pm, sh[b].np), hb.Om = std::max(hb.Om, sh[b].nobs);
  const int Fm = hb.Fm, Pm = hb.Pm, Om = hb.Om;
  const size_t is = int_stride(Fm, Pm, Om), ds = dbl_stride(Fm, Pm, Om);
  hb.ints.assign(is * n, 0), hb.in.assign(ds * n, 0.0);
  for (int b = 0; b < n; b++) {
    const VioInitBaProblem &P = pr[b];
    const int F = P.frame_num;
    int *h = &hb.ints[is * b];
    int *off_q = h + 8, *off_t = off_q + Fm, *fr_start = off_t + Fm, *pt_start = fr_start + Fm + 1, *obs_frame = pt_start + Pm + 1,
        *obs_point = obs_frame + Om, *fr_obs = obs_point + Om, *fr_point = fr_obs + Om, *pf_obs = fr_point + Om;
    double *cq = &hb.in[ds * b], *ct = cq + 4 * Fm, *X = cq + 7 * Fm, *xy = X + 3 * Pm;
    int nc = 0;
    for (int i = 0; i < Fm; i++) off_q[i] = off_t[i] = -1;
    for (int i = 0; i < F; i++) {  // inital_sfm.cpp:244-251
      if (i != P.l) off_q[i] = nc, nc += 3;
      if (i != P.l && i != F - 1) off_t[i] = nc, nc += 3;
    }
    memcpy(cq, P.c_rotation, sizeof(double) * 4 * F), memcpy(ct, P.c_translation, sizeof(double) * 3 * F);
    std::fill(pf_obs, pf_obs + (size_t)Pm * Fm, -1);
    int np = 0, nobs = 0;
    for (int j = 0; j < P.n_points; j++) {
      if (!P.point_ok[j]) continue;
      memcpy(X + 3 * np, P.points + 3 * (size_t)j, 24);
      pt_start[np] = nobs;
      for (int k = P.feat_start[j]; k < P.feat_start[j + 1]; k++, nobs++) {
        obs_frame[nobs] = P.obs_frame[k], obs_point[nobs] = np;
        xy[2 * nobs] = P.obs_xy[2 * k], xy[2 * nobs + 1] = P.obs_xy[2 * k + 1];
        pf_obs[np * F + P.obs_frame[k]] = nobs;
        fr_start[P.obs_frame[k] + 1]++;
      }
      np++;
    }
    pt_start[np] = nobs;
    for (int i = 0; i < F; i++) fr_start[i + 1] += fr_start[i];
    std::vector<int> fill(fr_start, fr_start + F);
    for (int k = 0; k < nobs; k++) {  // ascending observation index within a frame
      const int i = fill[obs_frame[k]]++;
      fr_obs[i] = k, fr_point[i] = obs_point[k];
    }
    h[0] = F, h[1] = P.l, h[2] = np, h[3] = nobs, h[4] = nc;
  }
}

// In/out arrays of problem b from the launch's output block (cq | ct | X, stride dbl_stride(Fm, Pm, 0)).
inline void unpack(const HostBatch &hb, int b, const double *out, const VioSolveStats &st, VioInitBaProblem &P) {
  const double *o = out + dbl_stride(hb.Fm, hb.Pm, 0) * b;
  memcpy(P.c_rotation, o, sizeof(double) * 4 * P.frame_num), memcpy(P.c_translation, o + 4 * hb.Fm, sizeof(double) * 3 * P.frame_num);
  int np = 0;
  for (int j = 0; j < P.n_points; j++)
    if (P.point_ok[j]) memcpy(P.points + 3 * (size_t)j, o + 7 * hb.Fm + 3 * np++, 24);
  P.ok = (st.termination == 1 || st.final_cost < 3e-03) ? 1 : 0;
}

}  // namespace sfm
}  // namespace vio
