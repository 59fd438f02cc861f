// fe_pyramid.h -- cv::pyrDown for the levels of calcOpticalFlowPyrLK (feature_tracker.cpp:181), byte-wise and dword-wise,
// and forw_img = _img (feature_tracker.cpp:165-170) as a copy kernel or fused into the level-1 pyrDown.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fe_common.h"

namespace {

// ---- pyrDown: separable [1 4 6 4 1], BORDER_REFLECT_101, (v + 128) >> 8 -------------------------------
// One workgroup = 64x8 output pixels: the (2*64+4) x (2*8+4) source patch goes through LDS once, the horizontal pass
// leaves 20 rows of integer sums in LDS, the vertical pass writes the tile.
constexpr int kPdW = 64, kPdH = 8;
__global__ __launch_bounds__(256) void pyr_down_kernel(const uint8_t *src_base, uint8_t *dst_base, size_t seq_stride,
                                                       int srows, int scols, int drows, int dcols) {
  constexpr int SW = 2 * kPdW + 4, SH = 2 * kPdH + 4;
  __shared__ int patch[SH][SW + 1];  // one dword per pixel: sub-dword LDS accesses are slow on this hardware
  __shared__ int hsum[SH][kPdW + 1];
  const uint8_t *src = src_base + (size_t)blockIdx.z * seq_stride;
  uint8_t *dst = dst_base + (size_t)blockIdx.z * seq_stride;
#include "fe_pyr_down_body.inc"
}
// Subset instantiation: blockIdx.z is a call position; level `src_off` -> level `dst_off` inside the sequence's forw bank.
__global__ __launch_bounds__(256) void pyr_down_subset_kernel(SubsetArgs M, size_t src_off, size_t dst_off, size_t seq_stride, int srows,
                                                              int scols, int drows, int dcols) {
  constexpr int SW = 2 * kPdW + 4, SH = 2 * kPdH + 4;
  __shared__ int patch[SH][SW + 1];
  __shared__ int hsum[SH][kPdW + 1];
  uint8_t *pyr = subset_bank(M, subset_at(M.forw_bank, blockIdx.z)) + (size_t)subset_at(M.seq, blockIdx.z) * seq_stride;
  const uint8_t *src = pyr + src_off;
  uint8_t *dst = pyr + dst_off;
#include "fe_pyr_down_body.inc"
}

// The same for source rows that are whole dwords (scols % 4 == 0, dword-aligned level offsets): the patch arrives as 4
// pixels per lane and per load instead of 1, the output leaves as 4 pixels per store. One workgroup = 64 x 16 output
// pixels from a (2*64+8) x (2*16+4) source patch [2 ox - 4, 2 ox + 132) x [2 oy - 2, 2 oy + 34). Rows are reflected as
// whole rows; the (at most two) reflected columns on either side of the image are patched into the staged dwords.
// Arithmetic and rounding are those of pyr_down_kernel (bit-identical output).
constexpr int kPd4H = 16, kPd4Dw = (2 * kPdW + 8) / 4;  // 34 dwords per staged row
// COPY: the source is the caller's frame (forw_img = _img, feature_tracker.cpp:169): the workgroup also writes the core of
// its staged patch to level 0 of the pyramid, so the frame is read ONCE for the copy and for level 1 (a separate copy kernel
// plus the level-1 kernel read it twice and the copy wrote what the level-1 kernel read again).
// A workgroup walks kPd4T tiles down its column of the image: the loads of the NEXT tile's patch are issued (into registers) before
// the barriers and the arithmetic of this one, so a workgroup always has a patch in flight -- with one tile per workgroup the load
// phase was a third of a workgroup's life and the kernel ran at a third of the memory system's rate (2.2 TB/s on level 1).
constexpr int kPd4T = 3;
#define PYR_DOWN4_COPY_ROW(yy) (copy_base + (size_t)blockIdx.z * seq_stride + (size_t)(yy) * scols)
template <bool COPY>
__global__ __launch_bounds__(256) void pyr_down4_kernel(const uint8_t *src_base, size_t src_stride, uint8_t *dst_base, size_t seq_stride,
                                                        int srows, int scols, int drows, int dcols, uint8_t *copy_base) {
  constexpr int SH = 2 * kPd4H + 4;
  constexpr int NE = (SH * kPd4Dw + 255) / 256;  // staged dwords per work-item: 5 (the last one only for some)
  __shared__ uint32_t raw[SH][kPd4Dw + 1];
  __shared__ uint32_t hsum[SH / 2][kPdW + 1];
  const uint8_t *src = src_base + (size_t)blockIdx.z * src_stride;
  uint8_t *dst = dst_base + (size_t)blockIdx.z * seq_stride;
#include "fe_pyr_down4_body.inc"
}
#undef PYR_DOWN4_COPY_ROW
// Subset instantiations: blockIdx.z is a call position. COPY: the source is the call's frame slot (`frames`, src_stride apart)
// and the workgroup also writes level 0 of the sequence's forw bank; otherwise the source is level `src_off` of that bank. The
// destination is level `dst_off` of the bank.
template <bool COPY>
__global__ __launch_bounds__(256) void pyr_down4_subset_kernel(SubsetArgs M, const uint8_t *frames, size_t src_stride, size_t src_off,
                                                               size_t dst_off, size_t seq_stride, int srows, int scols, int drows,
                                                               int dcols) {
  constexpr int SH = 2 * kPd4H + 4;
  constexpr int NE = (SH * kPd4Dw + 255) / 256;
  __shared__ uint32_t raw[SH][kPd4Dw + 1];
  __shared__ uint32_t hsum[SH / 2][kPdW + 1];
  uint8_t *pyr = subset_bank(M, subset_at(M.forw_bank, blockIdx.z)) + (size_t)subset_at(M.seq, blockIdx.z) * seq_stride;
  const uint8_t *src = COPY ? frames + (size_t)subset_at(M.slot, blockIdx.z) * src_stride : pyr + src_off;
  uint8_t *dst = pyr + dst_off;
#define PYR_DOWN4_COPY_ROW(yy) (pyr + (size_t)(yy) * scols)
#include "fe_pyr_down4_body.inc"
}
#undef PYR_DOWN4_COPY_ROW

// forw_img = _img for every sequence: packed frames -> level 0 of each sequence's pyramid (16 B per thread when the
// layout allows it; the runtime's rectangular copy reaches ~140 GB/s on this shape).
__device__ __forceinline__ void copy_frame(const uint8_t *sp, uint8_t *dp, size_t bytes, int vec_ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec_ok) {
    if (i * 16 < bytes) reinterpret_cast<uint4 *>(dp)[i] = reinterpret_cast<const uint4 *>(sp)[i];
  } else {
    const size_t b0 = i * 16, b1 = b0 + 16 < bytes ? b0 + 16 : bytes;
    for (size_t b = b0; b < b1; b++) dp[b] = sp[b];
  }
}
__global__ __launch_bounds__(256) void copy_frames_kernel(const uint8_t *src, size_t src_stride, uint8_t *dst,
                                                          size_t dst_stride, size_t bytes, int vec_ok) {
  const int seq = blockIdx.y;
  copy_frame(src + (size_t)seq * src_stride, dst + (size_t)seq * dst_stride, bytes, vec_ok);
}
// Subset instantiation: frame slot[i] -> level 0 of sequence seq[i]'s forw bank (blockIdx.y = call position i).
__global__ __launch_bounds__(256) void copy_frames_subset_kernel(SubsetArgs M, const uint8_t *frames, size_t src_stride, size_t dst_stride,
                                                                 size_t bytes, int vec_ok) {
  const int i = blockIdx.y;
  copy_frame(frames + (size_t)subset_at(M.slot, i) * src_stride,
             subset_bank(M, subset_at(M.forw_bank, i)) + (size_t)subset_at(M.seq, i) * dst_stride, bytes, vec_ok);
}

}  // namespace
