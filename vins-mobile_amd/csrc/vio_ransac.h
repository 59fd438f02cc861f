// vio_ransac.h — the tracker's block-cooperative fundamental-matrix RANSAC (fe_ransac.h) for callers inside the
// library that already hold their points on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vio {
// n_prob independent point sets on stream st: p1 / p2 [n_prob][stride][2] and count [n_prob] in device memory; mask
// [n_prob][stride] receives 1 = inlier for the sets with at least min_count pairs, the others are skipped.
int fundamental_ransac_batch(hipStream_t st, const float *p1, const float *p2, const int *count, int n_prob, int stride, int min_count,
                             float thresh, double conf, uint8_t *mask);
}  // namespace vio
