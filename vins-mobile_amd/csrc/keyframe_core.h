// keyframe_core.h — KeyFrame::buildKeyFrameFeatures (VINS_ios/loop/keyframe.cpp:128-155) for one landmark: single source of
// the host-side list (vio_features_keyframe, vio_window.cpp) and of the store's fourth pass (store_core.h). Both are
// compiled with -ffp-contract=off and every operation here is an IEEE one, so the two give the same bits.
#pragma once

#include "vio_math.h"

namespace vio {
namespace keyframe {

// :133 and :136 — a landmark of the solved window that reaches frame W - 2 with at least three observations.
// 1: dropped by the first test, 2: it does not reach frame W - 2, 3: fewer than three observations, 0: kept.
VIO_HD int verdict(int n_obs, int start, int W) {
  if (!(n_obs >= 2 && start < W - 2)) return 1;
  if (!(start + n_obs >= W - 1)) return 2;
  return n_obs >= 3 ? 0 : 3;
}

// :139-144 — p: the observation in frame W - 2. cv::Point2f rounds the doubles to float.
VIO_HD void measurement(double fx, double fy, double cx, double cy, const double p[3], float px[2], float norm[2]) {
  px[0] = (float)(fx * p[0] / p[2] + cx), px[1] = (float)(fy * p[1] / p[2] + cy);
  norm[0] = (float)(p[0] / p[2]), norm[1] = (float)(p[1] / p[2]);
}

// :148-149 — Rs[start] * (ric * (first * depth) + tic) + Ps[start]
VIO_HD void cloud(const double R[9], const double P[3], const double ric[9], const double tic[3], const double first[3], double depth,
                  double out[3]) {
  const double pts_i[3] = {first[0] * depth, first[1] * depth, first[2] * depth};
  double c[3], b[3], w[3];
  mat3vec(ric, pts_i, c);
  for (int k = 0; k < 3; k++) b[k] = c[k] + tic[k];
  mat3vec(R, b, w);
  for (int k = 0; k < 3; k++) out[k] = w[k] + P[k];
}

}  // namespace keyframe
}  // namespace vio
