// fe_common.h -- what every front-end kernel shares: the limits vio_frontend_create checks, the pyramid geometry of
// buildOpticalFlowPyramid (calcOpticalFlowPyrLK, feature_tracker.cpp:181), OpenCV's BORDER_REFLECT_101 and descale.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

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

// What the subset instantiations of the step's kernels (vio_frontend_submit_subset) take in place of "sequence = block index, one
// pyramid bank for all": the call's plan (fe_subset.h) on the device, n entries per row, and the context's two banks. Call
// position i = a block index; everything read through it is uniform over the workgroup and is kept in scalar registers.
struct SubsetArgs {
  const int *seq;        // [n] sequence of call position i
  const int *slot;       // [n] frame slot
  const int *prev_bank;  // [n] bank LK tracks from, < 0: the sequence's first frame
  const int *forw_bank;  // [n] bank the frame's pyramid goes to
  const int *publish;    // [n]
  const int *pub;        // [n_pub] call positions that publish
  uint8_t *pyr[2];       // the banks, [n_seq][pyr_bytes] each
};
__device__ __forceinline__ int subset_at(const int *row, int i) { return __builtin_amdgcn_readfirstlane(row[i]); }
__device__ __forceinline__ uint8_t *subset_bank(const SubsetArgs &M, int bank) { return bank ? M.pyr[1] : M.pyr[0]; }

// The region of interest of every sequence (vio_frontend_set_regions): what setMask starts from instead of an all-255 mask, one
// bit per pixel (1 = usable). Row y of sequence s is words[(s * rows + y) * wpr ..]: word 0 is padding (all 0), the bit of
// column x is bit (x + 64) % 64 of word (x + 64) / 64, and one more word of padding ends the row, so the 64 columns from any
// c >= -64 are a funnel shift of two words of the row. set[s] = 0: the sequence has no region (all usable), its rows are not read.
// The REGION variants of the step's kernels take this as one more argument (a parameter pack that is empty in the kernels as
// they always were: a context in which no sequence holds a region launches those, with the arguments they always had).
struct RegionArgs {
  const unsigned long long *words;
  const int *set;  // [n_seq]
  int wpr;         // words per row
};
__device__ __forceinline__ RegionArgs region_args() { return RegionArgs{nullptr, nullptr, 0}; }
__device__ __forceinline__ RegionArgs region_args(const RegionArgs &g) { return g; }
// the region bits of columns c0 .. c0 + 63 of one row (c0 >= -64; columns outside the image read 0)
__device__ __forceinline__ unsigned long long region_window(const unsigned long long *row, int wpr, int c0) {
  const int w = (c0 + 64) >> 6, sh = (c0 + 64) & 63;
  const unsigned long long lo = w < wpr ? row[w] : 0ull, hi = w + 1 < wpr ? row[w + 1] : 0ull;
  return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

typedef short lk_s2 __attribute__((ext_vector_type(2)));
typedef unsigned short lk_us2 __attribute__((ext_vector_type(2)));

}  // namespace
