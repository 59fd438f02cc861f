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
  const int ox = blockIdx.x * kPdW, oy = blockIdx.y * kPdH;
  const int tid = threadIdx.x;
  for (int e = tid; e < SH * SW; e += 256) {
    int ly = e / SW, lx = e - ly * SW;
    int y = reflect101(min(2 * oy + ly - 2, 2 * srows - 2), srows), x = reflect101(min(2 * ox + lx - 2, 2 * scols - 2), scols);
    patch[ly][lx] = src[(size_t)y * scols + x];
  }
  __syncthreads();
  for (int e = tid; e < SH * kPdW; e += 256) {
    int ly = e / kPdW, lx = e - ly * kPdW;
    const int *r = &patch[ly][2 * lx];
    hsum[ly][lx] = r[0] + 4 * r[1] + 6 * r[2] + 4 * r[3] + r[4];
  }
  __syncthreads();
  for (int e = tid; e < kPdH * kPdW; e += 256) {
    int ly = e / kPdW, lx = e - ly * kPdW;
    int x = ox + lx, y = oy + ly;
    if (x < dcols && y < drows) {
      int v = hsum[2 * ly][lx] + 4 * hsum[2 * ly + 1][lx] + 6 * hsum[2 * ly + 2][lx] + 4 * hsum[2 * ly + 3][lx] + hsum[2 * ly + 4][lx];
      dst[(size_t)y * dcols + x] = (uint8_t)((v + 128) >> 8);
    }
  }
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
template <bool COPY>
__global__ __launch_bounds__(256) void pyr_down4_kernel(const uint8_t *src_base, size_t src_stride, uint8_t *dst_base, size_t seq_stride,
                                                        int srows, int scols, int drows, int dcols, uint8_t *copy_base) {
  constexpr int SH = 2 * kPd4H + 4;
  constexpr int NE = (SH * kPd4Dw + 255) / 256;  // staged dwords per work-item: 5 (the last one only for some)
  __shared__ uint32_t raw[SH][kPd4Dw + 1];
  __shared__ uint32_t hsum[SH / 2][kPdW + 1];
  const uint8_t *src = src_base + (size_t)blockIdx.z * src_stride;
  uint8_t *dst = dst_base + (size_t)blockIdx.z * seq_stride;
  const int ox = blockIdx.x * kPdW;
  const int tid = threadIdx.x;
  const int ndw = scols >> 2, dw0 = (2 * ox - 4) >> 2;  // dwords per source row; dword index of the patch's first column
  // this work-item's elements of a patch: the same (row, dword) in every tile
  int e_ly[NE], e_d[NE];
  bool e_ok[NE];
#pragma unroll
  for (int i = 0; i < NE; i++) {
    const int e = tid + 256 * i;
    e_ok[i] = e < SH * kPd4Dw;
    const int ec = e_ok[i] ? e : 0;
    e_ly[i] = ec / kPd4Dw;
    e_d[i] = min(max(dw0 + ec - e_ly[i] * kPd4Dw, 0), ndw - 1);
  }
  const int tile0 = blockIdx.y * kPd4T;
  auto fetch = [&](int oy, uint32_t (&v)[NE]) {
#pragma unroll
    for (int i = 0; i < NE; i++) {
      const int y = reflect101(min(2 * oy + e_ly[i] - 2, 2 * srows - 2), srows);
      v[i] = reinterpret_cast<const uint32_t *>(src + (size_t)y * scols)[e_d[i]];
    }
  };
  uint32_t cur[NE], nxt[NE];
  fetch(tile0 * kPd4H, cur);
#pragma unroll 1
  for (int t = 0; t < kPd4T; t++) {
    const int oy = (tile0 + t) * kPd4H;
    if (oy >= drows) break;  // (uniform)
    const bool more = t + 1 < kPd4T && oy + kPd4H < drows;
    if (more) fetch(oy + kPd4H, nxt);
#pragma unroll
    for (int i = 0; i < NE; i++) {
      if (!e_ok[i]) continue;
      const int ly = e_ly[i], lx = tid + 256 * i - ly * kPd4Dw;
      raw[ly][lx] = cur[i];
      if (COPY) {  // core of the patch: rows 2 oy .. 2 oy + 2 kPd4H - 1, columns 2 ox .. 2 ox + 2 kPdW - 1 (staged dwords 1 .. 32)
        const int yy = 2 * oy + ly - 2, dd = dw0 + lx;
        if (ly >= 2 && ly < SH - 2 && lx >= 1 && lx <= (2 * kPdW) / 4 && yy < srows && dd < ndw)
          reinterpret_cast<uint32_t *>(copy_base + (size_t)blockIdx.z * seq_stride + (size_t)yy * scols)[dd] = cur[i];
      }
    }
    __syncthreads();
    // columns -2, -1 (left-most tile) and scols, scols + 1 (the tile that holds them): BORDER_REFLECT_101
    if (tid < SH) {
      if (ox == 0) {  // dword 0 = columns -4 .. -1, dword 1 = columns 0 .. 3
        const uint32_t d1 = raw[tid][1];
        raw[tid][0] = ((d1 >> 16) & 0xffu) << 16 | ((d1 >> 8) & 0xffu) << 24;  // col -2 <- col 2, col -1 <- col 1
      }
      const int lr = ndw - dw0;  // staged dword that starts at column scols
      if (lr >= 1 && lr < kPd4Dw) {
        const uint32_t dl = raw[tid][lr - 1];  // columns scols - 4 .. scols - 1
        raw[tid][lr] = ((dl >> 16) & 0xffu) | ((dl >> 8) & 0xffu) << 8;  // col scols <- col scols - 2, col scols + 1 <- col scols - 3
      }
    }
    __syncthreads();
    // horizontal pass, two source rows per item: output column ox + lx reads columns 2 lx - 2 .. 2 lx + 2 of the tile = staged
    // bytes 2 lx + 2 .. 2 lx + 6: four of them cut out of a dword pair with one funnel shift and weighted by ONE byte dot product
    // (1 4 6 4), the fifth is its accumulator. The sums (<= 16 * 255) of rows 2 p and 2 p + 1 share a dword, so that the vertical
    // pass below is two 16-bit dot products per output.
    for (int e = tid; e < (SH / 2) * kPdW; e += 256) {
      const int p = e / kPdW, lx = e - p * kPdW;
      const int b = 2 * lx + 2, dwi = b >> 2, sh = (b & 3) * 8;
      auto hrow = [&](int ly) {
        const uint32_t lo = raw[ly][dwi], hi = raw[ly][dwi + 1];
        return __builtin_amdgcn_udot4(__builtin_amdgcn_alignbit(hi, lo, sh), 0x04060401u, __builtin_amdgcn_ubfe(hi, sh, 8), false);
      };
      hsum[p][lx] = hrow(2 * p) | hrow(2 * p + 1) << 16;
    }
    __syncthreads();
    {
      const int ly = tid >> 4, lx = (tid & 15) * 4;
      const int x = ox + lx, y = oy + ly;
      if (x < dcols && y < drows) {
        uint32_t out = 0;
        const lk_us2 w14 = {1, 4}, w64 = {6, 4};
#pragma unroll
        for (int i = 0; i < 4; i++) {  // source rows 2 ly .. 2 ly + 4 = pairs ly, ly + 1 and the low half of pair ly + 2
          lk_us2 p0, p1;
          __builtin_memcpy(&p0, &hsum[ly][lx + i], 4), __builtin_memcpy(&p1, &hsum[ly + 1][lx + i], 4);
          const uint32_t v = __builtin_amdgcn_udot2(p0, w14, __builtin_amdgcn_udot2(p1, w64, hsum[ly + 2][lx + i] & 0xffffu, false), false);
          out |= ((v + 128) >> 8) << (8 * i);
        }
        *reinterpret_cast<uint32_t *>(dst + (size_t)y * dcols + x) = out;  // (dcols % 4 == 0: x + 3 < dcols)
      }
    }
    if (!more) break;
    // (the next tile's patch overwrites `raw` behind this tile's horizontal pass, which the barrier above closed; `hsum` is rewritten
    // behind the next tile's two barriers)
#pragma unroll
    for (int i = 0; i < NE; i++) cur[i] = nxt[i];
  }
}

// forw_img = _img for every sequence: packed frames -> level 0 of each sequence's pyramid (16 B per thread when the
// layout allows it; the runtime's rectangular copy reaches ~140 GB/s on this shape).
__global__ __launch_bounds__(256) void copy_frames_kernel(const uint8_t *src, size_t src_stride, uint8_t *dst,
                                                          size_t dst_stride, size_t bytes, int vec_ok) {
  const int seq = blockIdx.y;
  const uint8_t *sp = src + (size_t)seq * src_stride;
  uint8_t *dp = dst + (size_t)seq * dst_stride;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec_ok) {
    if (i * 16 < bytes) reinterpret_cast<uint4 *>(dp)[i] = reinterpret_cast<const uint4 *>(sp)[i];
  } else {
    const size_t b0 = i * 16, b1 = b0 + 16 < bytes ? b0 + 16 : bytes;
    for (size_t b = b0; b < b1; b++) dp[b] = sp[b];
  }
}

}  // namespace
