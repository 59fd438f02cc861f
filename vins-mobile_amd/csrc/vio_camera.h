// vio_camera.h — what every set-camera entry checks of a VioCamera (include/vio_amd.h): plain host C++.
// The per-device globals of the reference (FOCUS_LENGTH_X/Y, PX, PY, TIC_*, RIC_*: global_param.cpp:24-131) are a property of
// ONE sequence here; a context's cfg.fx .. cfg.cy and creation tic / ric are what a sequence uses until it is given its own.
#pragma once
#include <math.h>

#include "vio_amd.h"

namespace vio {

// Intrinsics: finite, fx and fy not zero. extrinsic: tic finite as well, ric orthonormal to 1e-6 with determinant +1.
inline bool camera_valid(const VioCamera &c, bool extrinsic) {
  if (!isfinite(c.fx) || !isfinite(c.fy) || !isfinite(c.cx) || !isfinite(c.cy) || c.fx == 0 || c.fy == 0) return false;
  if (!extrinsic) return true;
  for (int k = 0; k < 3; k++)
    if (!isfinite(c.tic[k])) return false;
  const double *R = c.ric;
  for (int k = 0; k < 9; k++)
    if (!isfinite(R[k])) return false;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double d = 0;
      for (int k = 0; k < 3; k++) d += R[3 * i + k] * R[3 * j + k];  // rows of R R^T
      if (fabs(d - (i == j ? 1.0 : 0.0)) > 1e-6) return false;
    }
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  return fabs(det - 1.0) <= 1e-6;
}

}  // namespace vio
