// vio_preprocess.hip — the image pre-step of the camera callback on the device, batched over frames:
//   cv::cvtColor(input_frame, gray, CV_RGBA2GRAY); clahe = cv::createCLAHE(); clahe->setClipLimit(3); clahe->apply(gray, img_equa)
// (VINS_ios/ViewController.mm:432-437), i.e. what every frame goes through right before FeatureTracker::readImage.
//
// Algorithm restated from the published OpenCV implementation the reference links (third-party, not in /root/reference:
// opencv2.framework for iOS, 3.x; modules/imgproc/src/color.cpp RGB2Gray<uchar> and modules/imgproc/src/clahe.cpp):
//   gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14
//   per tile (8 x 8 grid; image extended by BORDER_REFLECT_101 to a multiple of the grid when needed):
//     histogram -> clip at max(int(clipLimit * tileArea / 256), 1) -> the clipped mass is handed back, clipped/256 to
//     every bin and the remainder one count each to every (256/remainder)-th bin -> lut[i] = round(cdf[i] * 255/tileArea)
//   per pixel: bilinear blend (fp32, the order of operations of CLAHE_Interpolation_Body) of the four surrounding
//     tiles' lut[gray], rounded to nearest-even and saturated.
// Integer / fp32 work with a fixed operation order: the device result is bit-exact against the CPU oracle
// (oracle/vio_oracle_frontend.cpp::vio_oracle_preprocess); there is no OpenCV in this image to pin the oracle itself.
//
// Two kernels per batch, both HBM-bound streaming passes:
//   clahe_lut_kernel    one workgroup per (tile, frame): RGBA -> gray (written once), LDS histogram (u32 LDS atomics),
//                       clip + redistribution + 256-wide scan in the same workgroup, 256-byte LUT out
//   clahe_apply_kernel  one workgroup per band of 8 rows: the <= 3 tile rows of LUTs it needs staged in LDS as fp32
//                       (aligned dword reads), 4 pixels per lane (one dword load, one dword store)
// Algorithmic bytes per RGBA frame: 4*R*C (read) + R*C (gray out) + R*C (gray in) + R*C (equalized out) = 7*R*C.
//
// Lens rectification (VioLens, vio_preprocess_set_lenses) is fused into the gray pass: for a frame slot that holds a lens, the
// pixel clahe_lut_kernel writes and counts is the rectified one (pre_rectify.h: ~70 fp64 instructions and four raw reads that
// mostly hit the lines the neighbouring lanes read), so there is no map and no extra full-frame buffer. Lens or no lens is a
// per-frame, wave-uniform branch outside the pixel loop of the <CH, true> instantiation; a context that holds no lens at
// all launches <CH, false>, which is the kernel as it was before lenses existed.
// The lens MODEL (VioLensModel, vio_preprocess_set_lens_models: Brown-Conrady, rational, fisheye) is the frame's as well: each
// model has a pixel loop of its own behind a second wave-uniform branch, so one launch serves a batch that mixes them. The
// fisheye loop (sqrt, pre::lens_atan, two more divisions) needs registers that would cost every frame of the kernel a wave, so
// it exists only in the FISHEYE instantiations, launched while some slot of the context holds a fisheye lens.
//
// Native-size source frames (VioSource, vio_preprocess_set_sources, vio_preprocess_run_frames*) go through
// clahe_lut_frames_kernel, the same gray pass with a per-frame record (pre_source.h) and a per-frame base pointer: the tile's
// gray pixels are the exact area average of the slot's crop, or the supersampled rectification of the whole frame for a lensed
// slot. Format, identity / scaled / lensed are block-uniform branches outside the pixel loops, so one launch serves a batch that
// mixes them. The area path is separable: lanes walk SOURCE rows, consecutive lanes reading consecutive dwords of a row (one
// RGBA / BGRA pixel, or four one-byte pixels), and sum the rows of one output row with the vertical weights into LDS; then one
// lane per output pixel takes the horizontal weighted sum from LDS and divides once. Algorithmic bytes of a scaled frame:
// bpp * crop_rows * crop_cols (read once; a source row that two output rows share is read twice, from L2) + 3 * R * C,
// e.g. 8.3 MB + 0.9 MB for 1080p RGBA to 640 x 480.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include <algorithm>

#include <vector>

#include "pre_rectify.h"
#include "pre_source.h"
#include "vio_amd.h"
#include "vio_device.h"
#include "vio_pool.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTiles = 16;  // per axis
constexpr int kBandRows = 8;

struct PreGeom {
  int rows, cols, tiles_x, tiles_y, tw, th;  // tw/th: tile size of the (virtually) extended image
  int clip;                                  // 0: no clipping
  float lut_scale;
};

struct LensSlot {  // one per frame slot, in device memory
  VioLensModel lens;  // vio_preprocess_set_lenses stores VIO_LENS_BROWN
  int32_t is_set, pad;
};

__device__ __forceinline__ int reflect101(int i, int n) { return i < n ? i : 2 * n - 2 - i; }

__device__ __forceinline__ uint32_t rgba_gray(uint32_t px) {  // little endian: R in the low byte
  const uint32_t r = px & 0xff, g = (px >> 8) & 0xff, b = (px >> 16) & 0xff;
  return (r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14;
}

// hist[256] of one tile (complete after the barrier below) -> its 256-byte LUT: clip, redistribution, scan, scale
__device__ __forceinline__ void lut_of_histogram(uint32_t *hist, uint32_t *scan, uint32_t *wsum, const PreGeom &G, int tid,
                                                 uint8_t *__restrict__ lut_out) {
  __syncthreads();
  uint32_t h = hist[tid];
  if (G.clip > 0) {
    uint32_t excess = h > (uint32_t)G.clip ? h - G.clip : 0;
    if (excess) h = G.clip;
    // block sum of the clipped mass
    uint32_t s = excess;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    uint32_t clipped = 0;
    for (int w = 0; w < kThreads / 64; w++) clipped += wsum[w];
    const uint32_t batch = clipped / 256u;
    uint32_t residual = clipped - batch * 256u;
    h += batch;
    if (residual != 0) {
      const uint32_t step = 256u / residual > 1u ? 256u / residual : 1u;  // MAX(histSize / residual, 1)
      if ((uint32_t)tid % step == 0 && (uint32_t)tid / step < residual) h += 1;
    }
  }
  // inclusive scan over the 256 bins
  scan[tid] = h;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const uint32_t add = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const float f = (float)(int)scan[tid] * G.lut_scale;
  int r = __float2int_rn(f);  // cvRound
  r = r < 0 ? 0 : (r > 255 ? 255 : r);
  lut_out[tid] = (uint8_t)r;
}

// The rectified gray pixels of one tile of a frame whose slot holds a lens of model MODEL, counted in hist
template <int CH, int MODEL>
__device__ __forceinline__ void rect_tile(const uint8_t *__restrict__ img, int row_stride, const VioLensModel &lens, const PreGeom &G, int tx,
                                          int ty, uint8_t *__restrict__ gout, uint32_t *hist) {
  const pre::LensAs<MODEL> L(lens);
  for (int p = threadIdx.x; p < G.tw * G.th; p += kThreads) {
    const int yy = p / G.tw, xx = p - yy * G.tw;
    const int ey = ty * G.th + yy, ex = tx * G.tw + xx;
    const int sy = reflect101(ey, G.rows), sx = reflect101(ex, G.cols);  // the extension is one of OUTPUT coordinates
    const uint32_t v = pre::rectify_px<CH>(img, (size_t)row_stride, G.rows, G.cols, L, sx, sy);
    if (ey < G.rows && ex < G.cols) gout[(size_t)ey * G.cols + ex] = (uint8_t)v;
    atomicAdd(&hist[v], 1u);
  }
}

// FISHEYE: the instantiation a context launches while one of its slots holds a VIO_LENS_FISHEYE (its atan and square root take
// registers that would cost the other models' frames a wave of occupancy); without it the fisheye route does not exist
template <int CH, bool LENS, bool FISHEYE>
__global__ __launch_bounds__(kThreads) void clahe_lut_kernel(const uint8_t *__restrict__ src, size_t frame_stride,
                                                              int row_stride, uint8_t *__restrict__ gray,
                                                              uint8_t *__restrict__ lut, PreGeom G,
                                                              const LensSlot *__restrict__ lenses) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t scan[256];
  __shared__ uint32_t wsum[kThreads / 64];
  const int tid = threadIdx.x, tile = blockIdx.x, frame = blockIdx.y;
  const int tx = tile % G.tiles_x, ty = tile / G.tiles_x;
  hist[tid] = 0;
  __syncthreads();
  const uint8_t *img = src + (size_t)frame * frame_stride;
  uint8_t *gout = gray + (size_t)frame * G.rows * G.cols;
  const int area = G.tw * G.th;
  if (LENS && lenses[frame].is_set) {  // the frame's record: the same for every lane, read through the scalar cache
    const VioLensModel L = lenses[frame].lens;
    // the model is the frame's too: each has a pixel loop of its own, so a Brown-Conrady frame runs the instructions it always ran
    if (FISHEYE && L.model == VIO_LENS_FISHEYE)
      rect_tile<CH, VIO_LENS_FISHEYE>(img, row_stride, L, G, tx, ty, gout, hist);
    else if (L.model == VIO_LENS_RATIONAL)
      rect_tile<CH, VIO_LENS_RATIONAL>(img, row_stride, L, G, tx, ty, gout, hist);
    else
      rect_tile<CH, VIO_LENS_BROWN>(img, row_stride, L, G, tx, ty, gout, hist);
  } else {
    for (int p = tid; p < area; p += kThreads) {
      const int yy = p / G.tw, xx = p - yy * G.tw;
      const int ey = ty * G.th + yy, ex = tx * G.tw + xx;
      const int sy = reflect101(ey, G.rows), sx = reflect101(ex, G.cols);
      uint32_t v;
      if (CH == 4)
        v = rgba_gray(*reinterpret_cast<const uint32_t *>(img + (size_t)sy * row_stride + 4 * sx));
      else
        v = img[(size_t)sy * row_stride + sx];
      if (ey < G.rows && ex < G.cols) gout[(size_t)ey * G.cols + ex] = (uint8_t)v;  // every image pixel is in one tile
      atomicAdd(&hist[v], 1u);
    }
  }
  lut_of_histogram(hist, scan, wsum, G, tid, lut + ((size_t)frame * G.tiles_x * G.tiles_y + tile) * 256);
}

struct SourceSlot {  // one per frame slot, in device memory
  pre::SourcePlan plan;
  int32_t is_set, pad;
};

struct FrameRef {  // one per frame of a vio_preprocess_run_frames* call
  const uint8_t *base;  // row `row0` of the frame's plane 0 (the host route stages only the rows the slot reads)
  int32_t row0, pad;
};

constexpr int kAreaWords = 4096;  // LDS words of the area path's vertical sums
constexpr int kRowBatch = 4;      // source rows a lane of the area path reads before it uses them: that many loads in flight

// it / n for 0 <= it < kAreaWords, n >= 1, inv_n = 1.0f / n: (it + 0.5) / n is at least 0.5 / n away from an integer and the
// two float roundings move it by less than (it + 0.5) * 2^-23, so the truncation is the exact quotient
__device__ __forceinline__ int div_small(int it, float inv_n) { return (int)(((float)it + 0.5f) * inv_n); }

// The gray pixels of one tile of a frame that holds a source, counted in hist: three routes, chosen per block.
// (1) a lens in the slot: one lane per output pixel, the supersampled rectification of the whole delivered frame
template <int BPP, bool VIDEO, int MODEL>
__device__ __forceinline__ void lens_tile(const uint8_t *__restrict__ img, const pre::SourcePlan &P, const VioLensModel &lens, const PreGeom &G,
                                          int tx, int ty, uint8_t *__restrict__ gout, uint32_t *hist) {
  const pre::LensAs<MODEL> L(lens);
  for (int p = threadIdx.x; p < G.tw * G.th; p += kThreads) {
    const int yy = p / G.tw, xx = p - yy * G.tw;
    const int ey = ty * G.th + yy, ex = tx * G.tw + xx;
    const int sy = reflect101(ey, G.rows), sx = reflect101(ex, G.cols);  // the extension is one of OUTPUT coordinates
    const uint32_t v = pre::rectify_source_px<BPP, VIDEO>(img, P, L, sx, sy);
    if (ey < G.rows && ex < G.cols) gout[(size_t)ey * G.cols + ex] = (uint8_t)v;
    atomicAdd(&hist[v], 1u);
  }
}

// (2) a crop of the output's size: one lane per pixel, clahe_lut_kernel's loop with the slot's origin, stride and format
template <int BPP, bool VIDEO>
__device__ __forceinline__ void direct_tile(const uint8_t *__restrict__ img, const pre::SourcePlan &P, const PreGeom &G, int tx, int ty,
                                            uint8_t *__restrict__ gout, uint32_t *hist) {
  const uint8_t *org = img + (size_t)P.crop_y * P.stride + (size_t)P.crop_x * BPP;
  for (int p = threadIdx.x; p < G.tw * G.th; p += kThreads) {
    const int yy = p / G.tw, xx = p - yy * G.tw;
    const int ey = ty * G.th + yy, ex = tx * G.tw + xx;
    const int sy = reflect101(ey, G.rows), sx = reflect101(ex, G.cols);
    const uint32_t v = pre::source_gray<BPP, VIDEO>(org + (size_t)sy * P.stride, sx, P.c0, P.c2);
    if (ey < G.rows && ex < G.cols) gout[(size_t)ey * G.cols + ex] = (uint8_t)v;
    atomicAdd(&hist[v], 1u);
  }
}

// (3) the area average, separable. Output columns go in chunks whose source span fits V; of each chunk, groups of `rg` output
// rows: first one lane per (output row, SOURCE column) sums that column over the row's source rows with wy -- consecutive
// lanes read consecutive dwords of a source row: one RGBA / BGRA pixel, or four one-byte pixels where the rows are dword
// aligned -- then one lane per output pixel sums its span of V with wx and divides.
template <int BPP, bool VIDEO>
__device__ __forceinline__ void area_tile(const uint8_t *__restrict__ img, const pre::SourcePlan &P, const PreGeom &G, int tx, int ty,
                                          uint8_t *__restrict__ gout, uint32_t *hist, uint32_t *V) {
  const int tid = threadIdx.x;
  const uint32_t D = (uint32_t)P.cw * (uint32_t)P.ch;
  const int ex_end = tx * G.tw + G.tw, ey_end = ty * G.th + G.th;
  const int xc = min(G.tw, (int)(((int64_t)(kAreaWords - 2) * P.ow) / P.cw));  // >= 511: cw <= 8 ow
  const int span_max = (int)(((int64_t)xc * P.cw + P.ow - 1) / P.ow) + 1;      // <= kAreaWords
  const int rg = min(G.th, kAreaWords / span_max);
  for (int ex0 = tx * G.tw; ex0 < ex_end; ex0 += xc) {
    const int ex1 = min(ex0 + xc, ex_end), nx = ex1 - ex0;
    // the output columns this chunk reads, reflected ones included: [lo, hi), hi - lo <= nx
    const int a = reflect101(ex0, G.cols), b = reflect101(ex1 - 1, G.cols);
    const int lo = min(a, b), hi = (ex0 < G.cols && ex1 > G.cols) ? G.cols : max(a, b) + 1;
    const int j0 = pre::area_first(lo, P.cw, P.ow), span = pre::area_end(hi - 1, P.cw, P.ow) - j0;
    const uint8_t *col0 = img + (size_t)P.crop_y * P.stride + (size_t)(P.crop_x + j0) * BPP;  // source column j0 of crop row 0
    // one-byte pixels, four to a lane: the dwords that hold columns j0 .. j0 + span - 1 of a row. Their first and last may
    // reach up to 3 bytes beyond the row's pixels (never beyond the aligned dword a pixel of the frame lies in).
    const bool quads = BPP == 1 && (P.stride & 3) == 0;
    const int mis = quads ? (int)(reinterpret_cast<uintptr_t>(col0) & 3) : 0;
    const int n1 = quads ? (mis + span + 3) >> 2 : span;                       // lanes of one output row in the first step
    const float inv_n1 = 1.0f / (float)n1, inv_nx = 1.0f / (float)nx;
    for (int ey0 = ty * G.th; ey0 < ey_end; ey0 += rg) {
      const int nr = min(rg, ey_end - ey0);
      for (int it = tid; it < nr * n1; it += kThreads) {
        const int rr = div_small(it, inv_n1), g = it - rr * n1;
        const int sy = reflect101(ey0 + rr, G.rows);
        const int r0 = pre::area_first(sy, P.ch, P.oh), r1 = pre::area_end(sy, P.ch, P.oh);
        if (quads) {
          const int jj = 4 * g - mis;
          const uint8_t *at = col0 + jj;
          uint32_t acc[4] = {0, 0, 0, 0};
          for (int r = r0; r < r1; r += kRowBatch) {
            uint32_t w[kRowBatch], q[kRowBatch];
#pragma unroll
            for (int b = 0; b < kRowBatch; b++) {  // (a row past the last one: that one again, with weight 0)
              const int rb = min(r + b, r1 - 1);
              w[b] = r + b < r1 ? pre::area_weight(sy, rb, P.ch, P.oh) : 0u;
              q[b] = *reinterpret_cast<const uint32_t *>(at + (size_t)rb * P.stride);
            }
#pragma unroll
            for (int b = 0; b < kRowBatch; b++)
#pragma unroll
              for (int k = 0; k < 4; k++) {
                const uint32_t y = (q[b] >> (8 * k)) & 0xff;
                acc[k] += w[b] * (VIDEO ? pre::video_range(y) : y);
              }
          }
#pragma unroll
          for (int k = 0; k < 4; k++)
            if (jj + k >= 0 && jj + k < span) V[rr * span + jj + k] = acc[k];
        } else {
          uint32_t acc = 0;
          for (int r = r0; r < r1; r += kRowBatch) {
            uint32_t w[kRowBatch], y[kRowBatch];
#pragma unroll
            for (int b = 0; b < kRowBatch; b++) {
              const int rb = min(r + b, r1 - 1);
              w[b] = r + b < r1 ? pre::area_weight(sy, rb, P.ch, P.oh) : 0u;
              y[b] = pre::source_gray<BPP, VIDEO>(col0 + (size_t)rb * P.stride, g, P.c0, P.c2);
            }
#pragma unroll
            for (int b = 0; b < kRowBatch; b++) acc += w[b] * y[b];
          }
          V[rr * span + g] = acc;
        }
      }
      __syncthreads();
      for (int it = tid; it < nr * nx; it += kThreads) {
        const int rr = div_small(it, inv_nx), xx = it - rr * nx;
        const int ey = ey0 + rr, ex = ex0 + xx;
        const int sx = reflect101(ex, G.cols);
        const int j1 = pre::area_end(sx, P.cw, P.ow);
        const uint32_t *row = V + rr * span - j0;
        uint32_t S = 0;
        for (int j = pre::area_first(sx, P.cw, P.ow); j < j1; j++) S += pre::area_weight(sx, j, P.cw, P.ow) * row[j];
        const uint32_t v = pre::area_round(S, D);
        if (ey < G.rows && ex < G.cols) gout[(size_t)ey * G.cols + ex] = (uint8_t)v;
        atomicAdd(&hist[v], 1u);
      }
      __syncthreads();
    }
  }
}

template <int BPP, bool VIDEO, bool FISHEYE>
__device__ __forceinline__ void source_tile(const uint8_t *img, const pre::SourcePlan &P, const VioLensModel *lens, const PreGeom &G,
                                            int tx, int ty, uint8_t *__restrict__ gout, uint32_t *hist, uint32_t *V) {
  if (FISHEYE && lens && lens->model == VIO_LENS_FISHEYE)
    lens_tile<BPP, VIDEO, VIO_LENS_FISHEYE>(img, P, *lens, G, tx, ty, gout, hist);
  else if (lens && lens->model == VIO_LENS_RATIONAL)
    lens_tile<BPP, VIDEO, VIO_LENS_RATIONAL>(img, P, *lens, G, tx, ty, gout, hist);
  else if (lens)
    lens_tile<BPP, VIDEO, VIO_LENS_BROWN>(img, P, *lens, G, tx, ty, gout, hist);
  else if (P.cw == 1 && P.ch == 1)
    direct_tile<BPP, VIDEO>(img, P, G, tx, ty, gout, hist);
  else
    area_tile<BPP, VIDEO>(img, P, G, tx, ty, gout, hist, V);
}

// clahe_lut_kernel for frames that lie where the caller has them, each described by its slot's record.
// (7 waves per SIMD: left alone the allocator takes 81 registers for the area route's loads in flight, 5 waves, and the
// one-pixel-per-lane routes, which live on occupancy, pay for it: identity frames 0.578 -> 0.554 ms per 512, 2 x RGBA 1.71 -> 1.65;
// at 8 it spills to scratch)
// FISHEYE as for clahe_lut_kernel: launched while a slot holds a fisheye lens, with one wave less so that its route does not spill
template <bool FISHEYE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(FISHEYE ? 6 : 7))) void clahe_lut_frames_kernel(const FrameRef *__restrict__ frames,
                                                                     const SourceSlot *__restrict__ sources,
                                                                     uint8_t *__restrict__ gray, uint8_t *__restrict__ lut,
                                                                     PreGeom G, const LensSlot *__restrict__ lenses) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t scan[256];
  __shared__ uint32_t wsum[kThreads / 64];
  __shared__ uint32_t V[kAreaWords];
  const int tid = threadIdx.x, tile = blockIdx.x, frame = blockIdx.y;
  const int tx = tile % G.tiles_x, ty = tile / G.tiles_x;
  hist[tid] = 0;
  __syncthreads();
  // the frame's records: the same for every lane, read through the scalar cache
  const pre::SourcePlan P = sources[frame].plan;
  const uint8_t *img = frames[frame].base - (ptrdiff_t)frames[frame].row0 * P.stride;
  const VioLensModel *lens = lenses && lenses[frame].is_set ? &lenses[frame].lens : nullptr;
  uint8_t *gout = gray + (size_t)frame * G.rows * G.cols;
  if (P.bpp == 4)
    source_tile<4, false, FISHEYE>(img, P, lens, G, tx, ty, gout, hist, V);
  else if (P.video)
    source_tile<1, true, FISHEYE>(img, P, lens, G, tx, ty, gout, hist, V);
  else
    source_tile<1, false, FISHEYE>(img, P, lens, G, tx, ty, gout, hist, V);
  lut_of_histogram(hist, scan, wsum, G, tid, lut + ((size_t)frame * G.tiles_x * G.tiles_y + tile) * 256);
}

// ---- the valid region of a slot: where the rectified image is made of delivered pixels only (pre_source.h) --------------------
// One workgroup per tile of kRegTile x kRegTile output pixels of one entry of the call: one lane per pixel of the tile and its
// halo of `margin` pixels evaluates the inside test into LDS (a position outside the image counts as inside: it is no
// neighbour), then the erosion as two passes over LDS, along the rows and along the columns. Not in the per-frame path: a
// mask is static per lens. The halo is evaluated again by the neighbouring tiles ((64 + 2 * 12)^2 / 64^2 = 1.9 at margin 12).
constexpr int kRegTile = 64;
constexpr int kRegSpan = kRegTile + 2 * pre::kRegionMaxMargin;

template <int MODEL>
__device__ __forceinline__ void region_tile(const VioLensModel &lens, const pre::SourcePlan *P, int rows, int cols, int x0, int y0,
                                            int margin, uint8_t (*in)[kRegSpan]) {
  const pre::LensAs<MODEL> L(lens);
  const int span = kRegTile + 2 * margin;
  for (int p = threadIdx.x; p < span * span; p += kThreads) {
    const int yy = p / span, xx = p - yy * span;
    const int y = y0 - margin + yy, x = x0 - margin + xx;
    in[yy][xx] = y < 0 || y >= rows || x < 0 || x >= cols || pre::region_inside(L, P, rows, cols, x, y) ? 1 : 0;
  }
}

__global__ __launch_bounds__(kThreads) void valid_region_kernel(const int32_t *__restrict__ slots, const LensSlot *__restrict__ lenses,
                                                                const SourceSlot *__restrict__ sources, int rows, int cols, int margin,
                                                                uint8_t *__restrict__ masks) {
  __shared__ uint8_t in[kRegSpan][kRegSpan];
  __shared__ uint8_t hz[kRegSpan][kRegTile];
  const int tid = threadIdx.x, tiles_x = (cols + kRegTile - 1) / kRegTile;
  const int x0 = (blockIdx.x % tiles_x) * kRegTile, y0 = (blockIdx.x / tiles_x) * kRegTile;
  const int slot = slots[blockIdx.y];  // the entry's records: the same for every lane
  uint8_t *out = masks + (size_t)blockIdx.y * rows * cols;
  if (!(lenses && lenses[slot].is_set)) {  // a crop is always inside its frame
    for (int p = tid; p < kRegTile * kRegTile; p += kThreads) {
      const int y = y0 + p / kRegTile, x = x0 + p % kRegTile;
      if (y < rows && x < cols) out[(size_t)y * cols + x] = 255;
    }
    return;
  }
  const VioLensModel L = lenses[slot].lens;
  pre::SourcePlan plan;
  const pre::SourcePlan *P = nullptr;
  if (sources && sources[slot].is_set) plan = sources[slot].plan, P = &plan;
  if (L.model == VIO_LENS_FISHEYE)
    region_tile<VIO_LENS_FISHEYE>(L, P, rows, cols, x0, y0, margin, in);
  else if (L.model == VIO_LENS_RATIONAL)
    region_tile<VIO_LENS_RATIONAL>(L, P, rows, cols, x0, y0, margin, in);
  else
    region_tile<VIO_LENS_BROWN>(L, P, rows, cols, x0, y0, margin, in);
  __syncthreads();
  const int span = kRegTile + 2 * margin;
  for (int p = tid; p < span * kRegTile; p += kThreads) {  // column xx of hz <-> columns xx .. xx + 2 margin of in
    const int yy = p / kRegTile, xx = p % kRegTile;
    uint32_t all = 1;
    for (int k = 0; k <= 2 * margin; k++) all &= in[yy][xx + k];
    hz[yy][xx] = (uint8_t)all;
  }
  __syncthreads();
  for (int p = tid; p < kRegTile * kRegTile; p += kThreads) {
    const int yy = p / kRegTile, xx = p % kRegTile, y = y0 + yy, x = x0 + xx;
    uint32_t all = 1;
    for (int k = 0; k <= 2 * margin; k++) all &= hz[yy + k][xx];
    if (y < rows && x < cols) out[(size_t)y * cols + x] = all ? 255 : 0;
  }
}

__device__ __forceinline__ uint32_t blend_px(const float *__restrict__ L1, const float *__restrict__ L2, int i1, int i2,
                                              uint32_t v, float xa, float xa1, float ya, float ya1) {
  const float res = (L1[i1 + v] * xa1 + L1[i2 + v] * xa) * ya1 + (L2[i1 + v] * xa1 + L2[i2 + v] * xa) * ya;
  int r = __float2int_rn(res);
  r = r < 0 ? 0 : (r > 255 ? 255 : r);
  return (uint32_t)r;
}

template <bool VEC4>
__global__ __launch_bounds__(kThreads) void clahe_apply_kernel(const uint8_t *__restrict__ gray,
                                                                const uint8_t *__restrict__ lut, uint8_t *__restrict__ dst,
                                                                size_t dst_frame_stride, int dst_row_stride, PreGeom G) {
  __shared__ float L[3 * kMaxTiles * 256];
  const int tid = threadIdx.x, frame = blockIdx.y;
  const int y0 = blockIdx.x * kBandRows, y1 = min(y0 + kBandRows, G.rows);
  const float inv_th = 1.0f / G.th, inv_tw = 1.0f / G.tw;
  int t_lo = (int)floorf(y0 * inv_th - 0.5f);
  t_lo = t_lo < 0 ? 0 : t_lo;
  int t_hi = (int)floorf((y1 - 1) * inv_th - 0.5f) + 1;
  t_hi = t_hi > G.tiles_y - 1 ? G.tiles_y - 1 : t_hi;
  const int n_lut = (t_hi - t_lo + 1) * G.tiles_x * 256;  // <= 3 tile rows (kBandRows <= th is checked on the host)
  const uint8_t *fl = lut + ((size_t)frame * G.tiles_y + t_lo) * G.tiles_x * 256;
  for (int i = tid * 4; i < n_lut; i += kThreads * 4) {
    const uint32_t q = *reinterpret_cast<const uint32_t *>(fl + i);
    L[i] = (float)(q & 0xff), L[i + 1] = (float)((q >> 8) & 0xff), L[i + 2] = (float)((q >> 16) & 0xff), L[i + 3] = (float)(q >> 24);
  }
  __syncthreads();
  const uint8_t *gin = gray + (size_t)frame * G.rows * G.cols;
  uint8_t *out = dst + (size_t)frame * dst_frame_stride;
  const int groups = VEC4 ? G.cols / 4 : G.cols;
  for (int p = tid; p < (y1 - y0) * groups; p += kThreads) {
    const int y = y0 + p / groups, gx = p % groups;
    const float tyf = y * inv_th - 0.5f;
    int ty1 = (int)floorf(tyf);
    int ty2 = ty1 + 1;
    const float ya = tyf - ty1, ya1 = 1.0f - ya;
    ty1 = ty1 < 0 ? 0 : ty1;
    ty2 = ty2 > G.tiles_y - 1 ? G.tiles_y - 1 : ty2;
    const float *L1 = L + (ty1 - t_lo) * G.tiles_x * 256, *L2 = L + (ty2 - t_lo) * G.tiles_x * 256;
    if (VEC4) {
      const uint32_t q = *reinterpret_cast<const uint32_t *>(gin + (size_t)y * G.cols + 4 * gx);
      uint32_t o = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int x = 4 * gx + k;
        const float txf = x * inv_tw - 0.5f;
        int tx1 = (int)floorf(txf);
        int tx2 = tx1 + 1;
        const float xa = txf - tx1, xa1 = 1.0f - xa;
        tx1 = tx1 < 0 ? 0 : tx1;
        tx2 = tx2 > G.tiles_x - 1 ? G.tiles_x - 1 : tx2;
        o |= blend_px(L1, L2, tx1 * 256, tx2 * 256, (q >> (8 * k)) & 0xff, xa, xa1, ya, ya1) << (8 * k);
      }
      *reinterpret_cast<uint32_t *>(out + (size_t)y * dst_row_stride + 4 * gx) = o;
    } else {
      const int x = gx;
      const float txf = x * inv_tw - 0.5f;
      int tx1 = (int)floorf(txf);
      int tx2 = tx1 + 1;
      const float xa = txf - tx1, xa1 = 1.0f - xa;
      tx1 = tx1 < 0 ? 0 : tx1;
      tx2 = tx2 > G.tiles_x - 1 ? G.tiles_x - 1 : tx2;
      out[(size_t)y * dst_row_stride + x] =
          (uint8_t)blend_px(L1, L2, tx1 * 256, tx2 * 256, gin[(size_t)y * G.cols + x], xa, xa1, ya, ya1);
    }
  }
}

}  // namespace

struct vio_preprocess {
  int device = -1;  // HIP device the context lives on (current device at create)
  int max_frames = 0, rows = 0, cols = 0;
  double clip_limit = 3.0;  // clahe->setClipLimit(3) ViewController.mm:436
  int tiles_x = 8, tiles_y = 8;  // cv::createCLAHE() default tileGridSize
  vio::DevBuf<uint8_t> d_src, d_gray, d_lut, d_out;
  vio::DevBuf<LensSlot> d_lens;   // [max_frames]: written whole by every set_lenses, read by launches while n_lens > 0
  std::vector<LensSlot> h_lens;   // the table as last set (zero: no lens)
  int n_lens = 0;                 // slots that hold a lens: 0 launches the kernel without the lens branch
  int n_fisheye = 0;              // ... a VIO_LENS_FISHEYE: 0 launches the kernels without the fisheye route
  vio::PinnedBuf<uint8_t> h_in, h_out;  // page-locked staging of the host-buffer entry point
  // native-size source frames (vio_preprocess_run_frames*)
  static constexpr int kRing = 8;
  vio::DevBuf<SourceSlot> d_source;   // [max_frames]: written whole by every set_sources
  std::vector<SourceSlot> h_source;   // the table as last set (zero: no source)
  std::vector<VioSource> h_source_abi;  // what get_source returns
  // the frame table of a call lives in one of kRing entries, page-locked on the host and in device memory, until the
  // call's launch has run (ring_ev): a call returns before that, and the next calls take the next entries
  vio::PinnedBuf<FrameRef> h_refs;
  vio::DevBuf<FrameRef> d_refs;
  hipEvent_t ring_ev[kRing] = {};
  bool ring_used[kRing] = {};
  int ring_next = 0;
  vio::PinnedBuf<uint8_t> h_frames;   // staging of the host route: the rows each slot reads, grown on demand
  vio::DevBuf<uint8_t> d_frames;
  // vio_preprocess_valid_regions*: the slot list of the call in flight (region_ev: its kernel has run)
  vio::PinnedBuf<int32_t> h_region_slots;
  vio::DevBuf<int32_t> d_region_slots;
  hipEvent_t region_ev = nullptr;
  bool region_used = false;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double ms_sum = 0;
  int launches = 0;
  ~vio_preprocess() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (region_ev) (void)hipEventDestroy(region_ev);
    for (hipEvent_t e : ring_ev)
      if (e) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

PreGeom geometry(int rows, int cols, int tiles_x, int tiles_y, double clip_limit) {
  PreGeom G;
  G.rows = rows, G.cols = cols, G.tiles_x = tiles_x, G.tiles_y = tiles_y;
  // an image that is not a multiple of the grid in BOTH directions is extended on the right by tiles_x - cols % tiles_x
  // and at the bottom by tiles_y - rows % tiles_y (a whole extra `tiles` in a direction that did divide: as published)
  const bool fits = cols % tiles_x == 0 && rows % tiles_y == 0;
  const int ext_c = fits ? cols : cols + (tiles_x - cols % tiles_x);
  const int ext_r = fits ? rows : rows + (tiles_y - rows % tiles_y);
  G.tw = ext_c / tiles_x, G.th = ext_r / tiles_y;
  const int area = G.tw * G.th;
  G.lut_scale = (float)(256 - 1) / area;
  G.clip = 0;
  if (clip_limit > 0.0) {
    G.clip = (int)(clip_limit * area / 256);
    if (G.clip < 1) G.clip = 1;
  }
  return G;
}

void account(vio_preprocess *p) {
  float ms = 0;
  if (hipEventElapsedTime(&ms, p->ev0, p->ev1) == hipSuccess) p->ms_sum += ms, p->launches++;
  else (void)hipGetLastError();  // (no gray pass was launched yet, e.g. a sync behind valid_regions alone: not an error to keep)
}

// the apply pass of a batch whose gray images and LUTs the gray pass has just been launched for; closes the timed interval
int launch_apply(vio_preprocess *p, const PreGeom &G, int n_frames, uint8_t *d_out, size_t out_frame_stride, int out_row_stride,
                 hipStream_t st) {
  const dim3 g2((G.rows + kBandRows - 1) / kBandRows, n_frames);
  const bool vec4 = G.cols % 4 == 0 && out_row_stride % 4 == 0 && out_frame_stride % 4 == 0 &&
                    (reinterpret_cast<uintptr_t>(d_out) & 3) == 0;
  if (vec4)
    hipLaunchKernelGGL(clahe_apply_kernel<true>, g2, dim3(kThreads), 0, st, p->d_gray.p, p->d_lut.p, d_out, out_frame_stride,
                       out_row_stride, G);
  else
    hipLaunchKernelGGL(clahe_apply_kernel<false>, g2, dim3(kThreads), 0, st, p->d_gray.p, p->d_lut.p, d_out, out_frame_stride,
                       out_row_stride, G);
  (void)hipEventRecord(p->ev1, st);
  return hipGetLastError() == hipSuccess ? VIO_OK : VIO_ENODEV;
}

int launch(vio_preprocess *p, const uint8_t *d_src, int channels, int n_frames, size_t frame_stride, int row_stride,
           uint8_t *d_out, size_t out_frame_stride, int out_row_stride, hipStream_t st) {
  const PreGeom G = geometry(p->rows, p->cols, p->tiles_x, p->tiles_y, p->clip_limit);
  const dim3 g1(G.tiles_x * G.tiles_y, n_frames);
  (void)hipEventRecord(p->ev0, st);
  const LensSlot *ls = p->d_lens.p;
  auto *lut_kernel = channels == 4 ? (p->n_fisheye ? clahe_lut_kernel<4, true, true> : p->n_lens ? clahe_lut_kernel<4, true, false> : clahe_lut_kernel<4, false, false>)
                                   : (p->n_fisheye ? clahe_lut_kernel<1, true, true> : p->n_lens ? clahe_lut_kernel<1, true, false> : clahe_lut_kernel<1, false, false>);
  hipLaunchKernelGGL(lut_kernel, g1, dim3(kThreads), 0, st, d_src, frame_stride, row_stride, p->d_gray.p, p->d_lut.p, G, ls);
  return launch_apply(p, G, n_frames, d_out, out_frame_stride, out_row_stride, st);
}

// vio_preprocess_run_frames*: refs[f] is frame f of the call. The table goes to the device through the next ring entry, on
// `st` ahead of the kernels, so the caller's array and this entry's host copy are free as soon as the call returns / the
// launch has run.
int launch_frames(vio_preprocess *p, const FrameRef *refs, int n_frames, uint8_t *d_out, hipStream_t st) {
  const int k = p->ring_next;
  if (p->ring_used[k] && hipEventSynchronize(p->ring_ev[k]) != hipSuccess) return VIO_ENODEV;  // kRing calls in flight
  FrameRef *h = p->h_refs.p + (size_t)k * p->max_frames, *d = p->d_refs.p + (size_t)k * p->max_frames;
  memcpy(h, refs, sizeof(FrameRef) * n_frames);
  if (hipMemcpyAsync(d, h, sizeof(FrameRef) * n_frames, hipMemcpyHostToDevice, st) != hipSuccess) return VIO_ENODEV;
  const PreGeom G = geometry(p->rows, p->cols, p->tiles_x, p->tiles_y, p->clip_limit);
  const dim3 g1(G.tiles_x * G.tiles_y, n_frames);
  (void)hipEventRecord(p->ev0, st);
  const LensSlot *ls = p->n_lens ? p->d_lens.p : nullptr;
  hipLaunchKernelGGL(p->n_fisheye ? clahe_lut_frames_kernel<true> : clahe_lut_frames_kernel<false>, g1, dim3(kThreads), 0, st, (const FrameRef *)d, (const SourceSlot *)p->d_source.p,
                     p->d_gray.p, p->d_lut.p, G, ls);
  const int rc = launch_apply(p, G, n_frames, d_out, (size_t)p->rows * p->cols, p->cols, st);
  (void)hipEventRecord(p->ring_ev[k], st);
  p->ring_used[k] = true, p->ring_next = (k + 1) % vio_preprocess::kRing;
  return rc;
}

// the batch's results to caller memory through the page-locked staging; waits for them
int download(vio_preprocess *p, int n_frames, uint8_t *gray_out, uint8_t *equalized_out, hipStream_t st) {
  const size_t px = (size_t)p->rows * p->cols, N = (size_t)n_frames;
  if (hipMemcpyAsync(p->h_out.p, p->d_out.p, px * N, hipMemcpyDeviceToHost, st) != hipSuccess) return VIO_ENODEV;
  if (gray_out && hipMemcpyAsync(p->h_out.p + (size_t)p->max_frames * px, p->d_gray.p, px * N, hipMemcpyDeviceToHost, st) != hipSuccess)
    return VIO_ENODEV;
  if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) return VIO_ENODEV;
  vio::HostPool::get().parallel_for(n_frames, [&](int f) {
    memcpy(equalized_out + (size_t)f * px, p->h_out.p + (size_t)f * px, px);
    if (gray_out) memcpy(gray_out + (size_t)f * px, p->h_out.p + ((size_t)p->max_frames + f) * px, px);
  });
  account(p);
  return VIO_OK;
}

// vio_preprocess_set_lenses / _set_lens_models: lens(i) is entry i as a model record (nullptr: refused), clear: no entries
template <class Entry>
int set_lens_table(vio_preprocess_t *p, int32_t n, const int32_t *slot, bool clear, Entry lens) {
  if (!p || n < 0 || (n > 0 && !slot) || n > p->max_frames) return VIO_EINVAL;  // more than max_frames names a slot twice
  std::vector<LensSlot> next;
  std::vector<uint8_t> named;
  try {
    next = p->h_lens;
    named.assign((size_t)p->max_frames, 0);
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
  for (int i = 0; i < n; i++) {
    const int s = slot[i];
    if (s < 0 || s >= p->max_frames || named[s]) return VIO_EINVAL;
    named[s] = 1;
    next[s] = LensSlot{};
    if (clear) continue;
    VioLensModel m;
    if (!lens(i, &m)) return VIO_EINVAL;
    next[s].lens = m, next[s].is_set = 1;
  }
  if (n == 0) return VIO_OK;
  VIO_ON_DEVICE_OF(p);
  // launches of this context that are still in flight read the table: let the last one finish, then replace it, and
  // return only when the new table is in device memory (a later launch on ANY stream then sees it)
  if (hipEventSynchronize(p->ev1) != hipSuccess || (p->region_used && hipEventSynchronize(p->region_ev) != hipSuccess)) return VIO_ENODEV;
  if (hipMemcpyAsync(p->d_lens.p, next.data(), sizeof(LensSlot) * next.size(), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
      hipStreamSynchronize(p->stream) != hipSuccess)
    return VIO_ENODEV;
  p->h_lens.swap(next);
  p->n_lens = p->n_fisheye = 0;
  for (const LensSlot &s : p->h_lens) p->n_lens += s.is_set, p->n_fisheye += s.is_set && s.lens.model == VIO_LENS_FISHEYE;
  return VIO_OK;
}

// vio_preprocess_valid_regions*: the checked call's one launch on `st`, masks to d_masks [n][rows][cols]
int launch_regions(vio_preprocess *p, int n, const int32_t *slot, int margin, uint8_t *d_masks, hipStream_t st) {
  if (p->h_region_slots.ensure((size_t)p->max_frames) != VIO_OK || p->d_region_slots.ensure((size_t)p->max_frames) != VIO_OK) return VIO_ENOMEM;
  // the slot list of the last call is read until its kernel has run
  if (p->region_used && hipEventSynchronize(p->region_ev) != hipSuccess) return VIO_ENODEV;
  memcpy(p->h_region_slots.p, slot, sizeof(int32_t) * n);
  if (hipMemcpyAsync(p->d_region_slots.p, p->h_region_slots.p, sizeof(int32_t) * n, hipMemcpyHostToDevice, st) != hipSuccess) return VIO_ENODEV;
  int n_source = 0;
  for (const SourceSlot &s : p->h_source) n_source += s.is_set;
  const int tiles = ((p->cols + kRegTile - 1) / kRegTile) * ((p->rows + kRegTile - 1) / kRegTile);
  hipLaunchKernelGGL(valid_region_kernel, dim3(tiles, n), dim3(kThreads), 0, st, (const int32_t *)p->d_region_slots.p,
                     p->n_lens ? (const LensSlot *)p->d_lens.p : nullptr, n_source ? (const SourceSlot *)p->d_source.p : nullptr, p->rows,
                     p->cols, margin, d_masks);
  (void)hipEventRecord(p->region_ev, st);
  p->region_used = true;
  return hipGetLastError() == hipSuccess ? VIO_OK : VIO_ENODEV;
}

int regions_check(vio_preprocess *p, int32_t n, const int32_t *slot, int32_t margin, const void *out) {
  if (!p || !slot || !out || n < 0 || n > p->max_frames || margin < 0 || margin > pre::kRegionMaxMargin) return VIO_EINVAL;
  std::vector<uint8_t> named;
  try {
    named.assign((size_t)p->max_frames, 0);
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
  for (int i = 0; i < n; i++) {
    if (slot[i] < 0 || slot[i] >= p->max_frames || named[slot[i]]) return VIO_EINVAL;
    named[slot[i]] = 1;
  }
  return VIO_OK;
}

}  // namespace

extern "C" {

int vio_preprocess_create(int32_t max_frames, int32_t rows, int32_t cols, vio_preprocess_t **out) {
  if (!out || max_frames < 1 || rows < 16 || cols < 16 || rows > 16384 || cols > 16384) return VIO_EINVAL;
  if (!vio::device_ready("the image pre-step")) return VIO_ENODEV;
  vio_preprocess *p = new (std::nothrow) vio_preprocess();
  if (!p) return VIO_ENOMEM;
  p->device = vio::current_device();
  p->max_frames = max_frames, p->rows = rows, p->cols = cols;
  const size_t px = (size_t)rows * cols;
  if (p->d_src.ensure(px * 4 * max_frames) != VIO_OK || p->d_gray.ensure(px * max_frames) != VIO_OK ||
      p->d_out.ensure(px * max_frames) != VIO_OK || p->d_lut.ensure((size_t)kMaxTiles * kMaxTiles * 256 * max_frames) != VIO_OK ||
      p->d_lens.ensure(max_frames) != VIO_OK || p->d_source.ensure(max_frames) != VIO_OK ||
      p->d_refs.ensure((size_t)vio_preprocess::kRing * max_frames) != VIO_OK ||
      p->h_refs.ensure((size_t)vio_preprocess::kRing * max_frames) != VIO_OK ||
      hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&p->ev0) != hipSuccess ||
      hipEventCreate(&p->ev1) != hipSuccess || hipEventCreateWithFlags(&p->region_ev, hipEventDisableTiming) != hipSuccess) {
    delete p;
    return VIO_ENOMEM;
  }
  for (hipEvent_t &e : p->ring_ev)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      delete p;
      return VIO_ENOMEM;
    }
  try {
    p->h_lens.assign((size_t)max_frames, LensSlot{});
    p->h_source.assign((size_t)max_frames, SourceSlot{});
    p->h_source_abi.assign((size_t)max_frames, VioSource{});
  } catch (const std::bad_alloc &) {
    delete p;
    return VIO_ENOMEM;
  }
  if (vio_preprocess_set_clahe(p, 3.0, 8, 8) != VIO_OK) {  // the reference's setting must fit the frame size
    delete p;
    return VIO_EINVAL;
  }
  *out = p;
  return VIO_OK;
}

void vio_preprocess_destroy(vio_preprocess_t *p) {
  if (!p) return;
  vio::DeviceScope scope(p->device);
  delete p;
}

int vio_preprocess_set_clahe(vio_preprocess_t *p, double clip_limit, int32_t tiles_x, int32_t tiles_y) {
  if (!p || tiles_x < 1 || tiles_y < 1 || tiles_x > kMaxTiles || tiles_y > kMaxTiles) return VIO_EINVAL;
  const PreGeom G = geometry(p->rows, p->cols, tiles_x, tiles_y, clip_limit);
  // a band of kBandRows rows must not span more than 3 tile rows; the reflected extension must stay inside the image
  if (G.th < kBandRows || G.tw < 1 || G.th * tiles_y - p->rows >= p->rows || G.tw * tiles_x - p->cols >= p->cols) return VIO_EINVAL;
  p->clip_limit = clip_limit, p->tiles_x = tiles_x, p->tiles_y = tiles_y;
  return VIO_OK;
}

int vio_preprocess_set_lenses(vio_preprocess_t *p, int32_t n, const int32_t *slot, const VioLens *lens) {
  return set_lens_table(p, n, slot, !lens, [&](int i, VioLensModel *m) {
    if (!pre::lens_valid(lens[i])) return false;
    *m = pre::lens_model_of(lens[i]);
    return true;
  });
}

int vio_preprocess_set_lens_models(vio_preprocess_t *p, int32_t n, const int32_t *slot, const VioLensModel *lens) {
  return set_lens_table(p, n, slot, !lens, [&](int i, VioLensModel *m) {
    if (!pre::lens_model_valid(lens[i])) return false;
    *m = lens[i];
    return true;
  });
}

int vio_preprocess_get_lens(vio_preprocess_t *p, int32_t slot, VioLens *out, int32_t *is_set) {
  if (!p || !out || !is_set || slot < 0 || slot >= p->max_frames) return VIO_EINVAL;
  const LensSlot &s = p->h_lens[slot];
  if (s.is_set && s.lens.model != VIO_LENS_BROWN) return VIO_ESTATE;  // no VioLens says what this slot holds
  *out = pre::lens_of_model(s.lens), *is_set = s.is_set;
  return VIO_OK;
}

int vio_preprocess_get_lens_model(vio_preprocess_t *p, int32_t slot, VioLensModel *out, int32_t *is_set) {
  if (!p || !out || !is_set || slot < 0 || slot >= p->max_frames) return VIO_EINVAL;
  *out = p->h_lens[slot].lens, *is_set = p->h_lens[slot].is_set;
  return VIO_OK;
}

int vio_lens_distort_points(const VioLens *lens, const double *xn, int32_t n, double *uv) {
  if (!lens || n < 0 || (n > 0 && (!xn || !uv))) return VIO_EINVAL;
  for (int i = 0; i < n; i++) pre::lens_project(*lens, xn[2 * i], xn[2 * i + 1], &uv[2 * i], &uv[2 * i + 1]);
  return VIO_OK;
}

int vio_lens_undistort_points(const VioLens *lens, const double *uv, int32_t n, double *xn, uint8_t *converged) {
  if (!lens || n < 0 || (n > 0 && (!uv || !xn)) || !(lens->fx > 0) || !(lens->fy > 0)) return VIO_EINVAL;
  VioLens unit = *lens;  // the forward model in normalized coordinates: x_d = D(x)
  unit.fx = unit.fy = 1.0, unit.cx = unit.cy = 0.0;
  for (int i = 0; i < n; i++) {
    const double xd = (uv[2 * i] - lens->cx) / lens->fx, yd = (uv[2 * i + 1] - lens->cy) / lens->fy;
    double x = xd, y = yd;
    uint8_t done = 0;
    for (int round = 0; round < 50 && !done; round++) {  // x <- x + (x_d - D(x)): contracts while |1 - D'| < 1
      double dx, dy;
      pre::lens_project(unit, x, y, &dx, &dy);
      const double sx = xd - dx, sy = yd - dy;
      x += sx, y += sy;
      done = fabs(sx) < 1e-12 && fabs(sy) < 1e-12;
    }
    xn[2 * i] = x, xn[2 * i + 1] = y;
    if (converged) converged[i] = done;
  }
  return VIO_OK;
}

int vio_lens_coverage(const VioLens *lens, int32_t rows, int32_t cols, int64_t *n_outside) {
  if (!lens || !n_outside || rows < 1 || cols < 1 || !pre::lens_valid(*lens)) return VIO_EINVAL;
  int64_t n = 0;
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      double u, v;
      pre::lens_source(*lens, x, y, &u, &v);
      n += pre::lens_outside(u, cols) || pre::lens_outside(v, rows);
    }
  *n_outside = n;
  return VIO_OK;
}

static bool lens_model_known(const VioLensModel *lens) {
  return lens && lens->reserved == 0 && (lens->model == VIO_LENS_BROWN || lens->model == VIO_LENS_RATIONAL || lens->model == VIO_LENS_FISHEYE);
}

int vio_lens_model_distort_points(const VioLensModel *lens, const double *xn, int32_t n, double *uv) {
  if (!lens_model_known(lens) || n < 0 || (n > 0 && (!xn || !uv))) return VIO_EINVAL;
  for (int i = 0; i < n; i++) pre::lens_project(*lens, xn[2 * i], xn[2 * i + 1], &uv[2 * i], &uv[2 * i + 1]);
  return VIO_OK;
}

int vio_lens_model_undistort_points(const VioLensModel *lens, const double *uv, int32_t n, double *xn, uint8_t *converged) {
  if (!lens_model_known(lens) || n < 0 || (n > 0 && (!uv || !xn)) || !(lens->fx > 0) || !(lens->fy > 0)) return VIO_EINVAL;
  VioLensModel unit = *lens;  // the forward model in normalized coordinates: x_d = D(x)
  unit.fx = unit.fy = 1.0, unit.cx = unit.cy = 0.0;
  const double *k = lens->k;
  for (int i = 0; i < n; i++) {
    const double xd = (uv[2 * i] - lens->cx) / lens->fx, yd = (uv[2 * i + 1] - lens->cy) / lens->fy;
    double x = xd, y = yd;
    uint8_t done = 0;
    if (lens->model == VIO_LENS_FISHEYE) {
      // th * (1 + k1 th^2 + k2 th^4 + k3 th^6 + k4 th^8) = thd by Newton from th = thd; the ray is (xd, yd) * tan(th) / thd
      const double thd = hypot(xd, yd);
      double th = thd;
      for (int round = 0; round < 50 && !done; round++) {
        const double t2 = th * th;
        const double f = th * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])))) - thd;
        const double df = 1.0 + t2 * (3.0 * k[0] + t2 * (5.0 * k[1] + t2 * (7.0 * k[2] + t2 * (9.0 * k[3]))));
        const double step = f / df;
        th -= step;
        done = fabs(step) < 1e-12;
      }
      const double s = thd > 0.0 ? tan(th) / thd : 1.0;
      x = xd * s, y = yd * s;
      if (!(th >= 0.0 && th < 1.5707963267948966)) done = 0;  // at or behind the image plane's horizon (or a NaN)
    } else {
      for (int round = 0; round < 50 && !done; round++) {  // x <- x + (x_d - D(x)): contracts while |1 - D'| < 1
        double dx, dy;
        pre::lens_project(unit, x, y, &dx, &dy);
        const double sx = xd - dx, sy = yd - dy;
        x += sx, y += sy;
        done = fabs(sx) < 1e-12 && fabs(sy) < 1e-12;
      }
    }
    xn[2 * i] = x, xn[2 * i + 1] = y;
    if (converged) converged[i] = done;
  }
  return VIO_OK;
}

int vio_lens_model_coverage(const VioLensModel *lens, int32_t rows, int32_t cols, int64_t *n_outside) {
  if (!lens || !n_outside || rows < 1 || cols < 1 || !pre::lens_model_valid(*lens)) return VIO_EINVAL;
  int64_t n = 0;
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      double u, v;
      pre::lens_source(*lens, x, y, &u, &v);
      n += pre::lens_outside(u, cols) || pre::lens_outside(v, rows);
    }
  *n_outside = n;
  return VIO_OK;
}

int vio_lens_model_valid_region(const VioLensModel *lens, const VioSource *src, int32_t rows, int32_t cols, int32_t margin,
                                uint8_t *mask) {
  if (!lens || !mask || rows < 1 || cols < 1 || rows > 16384 || cols > 16384 || margin < 0 || margin > pre::kRegionMaxMargin ||
      !pre::lens_model_valid(*lens) || (src && !pre::source_valid(*src, rows, cols)))
    return VIO_EINVAL;
  std::vector<uint8_t> tmp;
  try {
    tmp.resize((size_t)rows * cols);
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
  pre::SourcePlan plan;
  if (src) plan = pre::source_plan(*src, rows, cols);
  pre::valid_region(lens, src ? &plan : nullptr, rows, cols, margin, mask, tmp.data());
  return VIO_OK;
}

int vio_preprocess_valid_regions_resident(vio_preprocess_t *p, int32_t n, const int32_t *slot, int32_t margin, void *d_masks,
                                          void *stream) {
  const int rc = regions_check(p, n, slot, margin, d_masks);
  if (rc != VIO_OK || n == 0) return rc;
  VIO_ON_DEVICE_OF(p);
  return launch_regions(p, n, slot, margin, (uint8_t *)d_masks, stream ? (hipStream_t)stream : p->stream);
}

int vio_preprocess_valid_regions(vio_preprocess_t *p, int32_t n, const int32_t *slot, int32_t margin, uint8_t *masks_out) {
  int rc = regions_check(p, n, slot, margin, masks_out);
  if (rc != VIO_OK || n == 0) return rc;
  VIO_ON_DEVICE_OF(p);
  const size_t bytes = (size_t)p->rows * p->cols * n;
  if (p->h_out.ensure((size_t)p->max_frames * p->rows * p->cols * 2) != VIO_OK) return VIO_ENOMEM;
  // d_out and the staging are the host routes' own, used in the order of the context's stream
  if ((rc = launch_regions(p, n, slot, margin, p->d_out.p, p->stream)) != VIO_OK) return rc;
  if (hipMemcpyAsync(p->h_out.p, p->d_out.p, bytes, hipMemcpyDeviceToHost, p->stream) != hipSuccess ||
      hipStreamSynchronize(p->stream) != hipSuccess || hipGetLastError() != hipSuccess)
    return VIO_ENODEV;
  memcpy(masks_out, p->h_out.p, bytes);
  return VIO_OK;
}

int vio_preprocess_run(vio_preprocess_t *p, const uint8_t *pixels, int32_t channels, int32_t n_frames, int32_t stride,
                       uint8_t *gray_out, uint8_t *equalized_out) {
  if (!p || !pixels || !equalized_out || !(channels == 1 || channels == 4) || n_frames < 1 || stride < channels * p->cols)
    return VIO_EINVAL;
  if (n_frames > p->max_frames) return VIO_ECAP;
  VIO_ON_DEVICE_OF(p);
  const size_t px = (size_t)p->rows * p->cols, row_bytes = (size_t)channels * p->cols, fb = row_bytes * p->rows;
  hipStream_t st = p->stream;
  // caller memory is pageable: gather into / scatter from page-locked staging with the host pool, a few frames per chunk,
  // so that the DMA of one chunk overlaps the host copy of the next (a direct pageable copy runs at ~5 GB/s)
  const size_t N = (size_t)n_frames;
  if (p->h_in.ensure((size_t)p->max_frames * px * 4) != VIO_OK || p->h_out.ensure((size_t)p->max_frames * px * 2) != VIO_OK) return VIO_ENOMEM;
  const size_t n_chunks = N >= 16 ? 8 : 1, per = (N + n_chunks - 1) / n_chunks;
  for (size_t c0 = 0; c0 < N; c0 += per) {
    const size_t c1 = std::min(N, c0 + per);
    vio::HostPool::get().parallel_for((int)(c1 - c0), [&](int i) {
      const size_t f = c0 + i;
      const uint8_t *src = pixels + f * (size_t)p->rows * stride;
      uint8_t *dst = p->h_in.p + f * fb;
      if ((size_t)stride == row_bytes) memcpy(dst, src, fb);
      else
        for (int r = 0; r < p->rows; r++) memcpy(dst + (size_t)r * row_bytes, src + (size_t)r * stride, row_bytes);
    });
    if (hipMemcpyAsync(p->d_src.p + c0 * fb, p->h_in.p + c0 * fb, (c1 - c0) * fb, hipMemcpyHostToDevice, st) != hipSuccess) return VIO_ENODEV;
  }
  int rc = launch(p, p->d_src.p, channels, n_frames, fb, (int)row_bytes, p->d_out.p, px, p->cols, st);
  if (rc != VIO_OK) return rc;
  return download(p, n_frames, gray_out, equalized_out, st);
}

int vio_preprocess_run_resident(vio_preprocess_t *p, const void *d_pixels, int32_t channels, int32_t n_frames, int32_t stride,
                                void *d_equalized, void *stream) {
  if (!p || !d_pixels || !d_equalized || !(channels == 1 || channels == 4) || n_frames < 1 || stride < channels * p->cols)
    return VIO_EINVAL;
  if (n_frames > p->max_frames) return VIO_ECAP;
  if (channels == 4 && ((reinterpret_cast<uintptr_t>(d_pixels) | (uintptr_t)stride) & 3)) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(p);
  hipStream_t st = stream ? (hipStream_t)stream : p->stream;
  return launch(p, (const uint8_t *)d_pixels, channels, n_frames, (size_t)stride * p->rows, stride, (uint8_t *)d_equalized,
                (size_t)p->rows * p->cols, p->cols, st);
}

int vio_source_check(const VioSource *s, int32_t rows, int32_t cols) {
  return s && pre::source_valid(*s, rows, cols) ? VIO_OK : VIO_EINVAL;
}

int vio_source_camera(const VioSource *s, int32_t rows, int32_t cols, const double in[4], double out[4]) {
  if (!s || !in || !out || !pre::source_valid(*s, rows, cols)) return VIO_EINVAL;
  pre::source_camera(*s, rows, cols, in, out);
  return VIO_OK;
}

int vio_preprocess_set_sources(vio_preprocess_t *p, int32_t n, const int32_t *slot, const VioSource *src) {
  if (!p || n < 0 || (n > 0 && !slot) || n > p->max_frames) return VIO_EINVAL;  // more than max_frames names a slot twice
  std::vector<SourceSlot> next;
  std::vector<VioSource> next_abi;
  std::vector<uint8_t> named;
  try {
    next = p->h_source, next_abi = p->h_source_abi;
    named.assign((size_t)p->max_frames, 0);
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
  for (int i = 0; i < n; i++) {
    const int s = slot[i];
    if (s < 0 || s >= p->max_frames || named[s]) return VIO_EINVAL;
    if (src && !pre::source_valid(src[i], p->rows, p->cols)) return VIO_EINVAL;
    named[s] = 1;
    next[s] = SourceSlot{}, next_abi[s] = VioSource{};
    if (src) next[s].plan = pre::source_plan(src[i], p->rows, p->cols), next[s].is_set = 1, next_abi[s] = src[i];
  }
  if (n == 0) return VIO_OK;
  VIO_ON_DEVICE_OF(p);
  // as vio_preprocess_set_lenses: let the last launch finish, replace the table, return with it in device memory
  if (hipEventSynchronize(p->ev1) != hipSuccess || (p->region_used && hipEventSynchronize(p->region_ev) != hipSuccess)) return VIO_ENODEV;
  if (hipMemcpyAsync(p->d_source.p, next.data(), sizeof(SourceSlot) * next.size(), hipMemcpyHostToDevice, p->stream) != hipSuccess ||
      hipStreamSynchronize(p->stream) != hipSuccess)
    return VIO_ENODEV;
  p->h_source.swap(next), p->h_source_abi.swap(next_abi);
  return VIO_OK;
}

int vio_preprocess_get_source(vio_preprocess_t *p, int32_t slot, VioSource *out, int32_t *is_set) {
  if (!p || !out || !is_set || slot < 0 || slot >= p->max_frames) return VIO_EINVAL;
  *out = p->h_source_abi[slot], *is_set = p->h_source[slot].is_set;
  return VIO_OK;
}

int vio_preprocess_run_frames(vio_preprocess_t *p, const void *const *pixels, int32_t n_frames, uint8_t *gray_out,
                              uint8_t *equalized_out) {
  if (!p || !pixels || !equalized_out || n_frames < 1) return VIO_EINVAL;
  if (n_frames > p->max_frames) return VIO_ECAP;
  for (int f = 0; f < n_frames; f++) {
    if (!pixels[f]) return VIO_EINVAL;
    if (!p->h_source[f].is_set) return VIO_ESTATE;
  }
  VIO_ON_DEVICE_OF(p);
  const size_t px = (size_t)p->rows * p->cols, N = (size_t)n_frames;
  hipStream_t st = p->stream;
  // per frame the rows its slot reads, each with the frame's own stride: the crop's rows, or all of plane 0 under a lens.
  // The last row ends with its last pixel (a caller's plane need not be padded to the stride there).
  struct Part {
    size_t src_off, bytes, dst_off;
    int32_t row0;
  };
  std::vector<Part> part;
  std::vector<FrameRef> refs;
  try {
    part.resize(N), refs.resize(N);
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
  size_t total = 0;
  for (size_t f = 0; f < N; f++) {
    const pre::SourcePlan &S = p->h_source[f].plan;
    const VioSource &A = p->h_source_abi[f];
    const bool lens = p->h_lens[f].is_set != 0;
    const int32_t row0 = lens ? 0 : A.crop_y, n_rows = lens ? A.rows : A.crop_rows;
    part[f] = Part{(size_t)row0 * A.stride, (size_t)(n_rows - 1) * A.stride + (size_t)A.cols * S.bpp, total, row0};
    total += (part[f].bytes + 15) & ~(size_t)15;
  }
  if (p->h_frames.ensure(total) != VIO_OK || p->d_frames.ensure(total) != VIO_OK ||
      p->h_out.ensure((size_t)p->max_frames * px * 2) != VIO_OK)
    return VIO_ENOMEM;
  // the chunked gather of vio_preprocess_run: the DMA of one chunk overlaps the host copy of the next
  const size_t n_chunks = N >= 16 ? 8 : 1, per = (N + n_chunks - 1) / n_chunks;
  for (size_t c0 = 0; c0 < N; c0 += per) {
    const size_t c1 = std::min(N, c0 + per);
    vio::HostPool::get().parallel_for((int)(c1 - c0), [&](int i) {
      const Part &q = part[c0 + i];
      memcpy(p->h_frames.p + q.dst_off, (const uint8_t *)pixels[c0 + i] + q.src_off, q.bytes);
    });
    const size_t b0 = part[c0].dst_off, b1 = part[c1 - 1].dst_off + part[c1 - 1].bytes;
    if (hipMemcpyAsync(p->d_frames.p + b0, p->h_frames.p + b0, b1 - b0, hipMemcpyHostToDevice, st) != hipSuccess) return VIO_ENODEV;
  }
  for (size_t f = 0; f < N; f++) refs[f] = FrameRef{p->d_frames.p + part[f].dst_off, part[f].row0, 0};
  const int rc = launch_frames(p, refs.data(), n_frames, p->d_out.p, st);
  if (rc != VIO_OK) return rc;
  return download(p, n_frames, gray_out, equalized_out, st);
}

int vio_preprocess_run_frames_resident(vio_preprocess_t *p, const void *const *d_pixels, int32_t n_frames, void *d_equalized,
                                       void *stream) {
  if (!p || !d_pixels || !d_equalized || n_frames < 1) return VIO_EINVAL;
  if (n_frames > p->max_frames) return VIO_ECAP;
  std::vector<FrameRef> refs;
  try {
    refs.resize((size_t)n_frames);
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
  for (int f = 0; f < n_frames; f++) {
    if (!d_pixels[f]) return VIO_EINVAL;
    if (!p->h_source[f].is_set) return VIO_ESTATE;
    if (p->h_source[f].plan.bpp == 4 && (reinterpret_cast<uintptr_t>(d_pixels[f]) & 3)) return VIO_EINVAL;
    refs[f] = FrameRef{(const uint8_t *)d_pixels[f], 0, 0};
  }
  VIO_ON_DEVICE_OF(p);
  hipStream_t st = stream ? (hipStream_t)stream : p->stream;
  return launch_frames(p, refs.data(), n_frames, (uint8_t *)d_equalized, st);
}

int vio_preprocess_sync(vio_preprocess_t *p) {
  if (!p) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(p);
  if (p->region_used && hipEventSynchronize(p->region_ev) != hipSuccess) return VIO_ENODEV;
  if (hipEventSynchronize(p->ev1) != hipSuccess || hipGetLastError() != hipSuccess) return VIO_ENODEV;
  account(p);
  return VIO_OK;
}

int vio_preprocess_kernel_ms(vio_preprocess_t *p, double *ms_avg, int32_t *launches) {
  if (!p || !ms_avg || !launches) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(p);
  *launches = p->launches;
  *ms_avg = p->launches ? p->ms_sum / p->launches : 0.0;
  p->ms_sum = 0, p->launches = 0;
  return VIO_OK;
}

}  // extern "C"
