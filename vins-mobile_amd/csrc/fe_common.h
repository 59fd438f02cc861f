// fe_common.h -- what every front-end kernel shares: the limits vio_frontend_create checks, the pyramid geometry of
// buildOpticalFlowPyramid (calcOpticalFlowPyrLK, feature_tracker.cpp:181), OpenCV's BORDER_REFLECT_101 and descale.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>

namespace {

constexpr int kMaxLevels = 4;   // level 0..3
constexpr int kMaxCap = 512;    // max tracked features per sequence supported by the per-sequence kernels
constexpr int kWin = 21;        // LK window (the kernel is specialised for 21x21; cfg->lk_win must match)
constexpr int kWBits = 14;
constexpr int kMaxRadius = 128;  // largest MIN_DIST (setMask circle radius) the tracker's LDS tables are sized for

struct LevelDims {
  int rows[kMaxLevels], cols[kMaxLevels];
  size_t off[kMaxLevels];  // byte offset of the level inside one pyramid
  size_t pyr_bytes;
  int levels;              // number of levels actually used (maxLevel + 1)
};

__device__ __forceinline__ int reflect101(int p, int len) {
  // valid for |overshoot| < len (callers stay within a window of the image)
  p = p < 0 ? -p : p;
  p = p >= len ? 2 * len - 2 - p : p;
  return p;
}
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

typedef short lk_s2 __attribute__((ext_vector_type(2)));
typedef unsigned short lk_us2 __attribute__((ext_vector_type(2)));

}  // namespace
