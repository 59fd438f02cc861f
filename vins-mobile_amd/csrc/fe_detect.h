// fe_detect.h -- goodFeaturesToTrack, front half (feature_tracker.cpp:80, :263): cornerMinEigenVal, the masked maximum, the
// 3x3 non-maximum test and the setMask discs, fused into one pass that writes nothing but the corner candidates.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fe_common.h"

namespace {

// ---- goodFeaturesToTrack -----------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned ordered_bits(float v) {  // monotone float -> uint map (atomicMax on it)
  unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// goodFeaturesToTrack front half, fused: cornerMinEigenVal (Sobel/1/3060 -> products -> 3x3 box -> min eigenvalue),
// the masked maximum (minMaxLoc) and the candidate test "equal to its 3x3 maximum, inside the mask, 1-px border
// excluded". Nothing but the candidates goes to memory and nothing is staged in LDS:
//   * a wave owns 64 consecutive columns (60 outputs + 2 halo each side) and walks down a strip of kDetR rows;
//   * each lane forms the derivative products of ITS column for one row from nine image bytes (row addresses are
//     scalar, a product position outside the image takes the value of its reflected position: boxFilter's
//     BORDER_REFLECT_101 acts on the product images);
//   * horizontal neighbours travel on the DPP network (wave_shr / wave_shl), vertical neighbours are the previous two
//     rows kept in registers: box sums, eigenvalues and the 3x3 maximum all slide down the strip;
//   * the mask is either an image (stand-alone operator) or the discs setMask painted (feature_tracker.cpp:80),
//     rasterised once per workgroup into one 64-bit word per (wave, row).
// The quality threshold needs the global maximum, so it is applied later by the selection kernel.
// (Round 6 built the two-pixels-per-lane form with v_pk_add / v_pk_mul / v_pk_fma_f32 for everything that takes no DPP operand --
// bit-exact, 124 outputs per wave -- and measured it SLOWER, 500 vs 406 us per 512 frames: 228 M against 209 M vector instructions
// per launch. What packs is a third of a row's instructions; the DPP neighbour sums, the square-root selects, the 3x3 maximum and
// the candidate tests are per pixel either way, and building the operand pairs costs moves. commit 3f94e20 has the kernel.)
constexpr int kDetW = 60;      // output columns per wave
constexpr int kDetWaves = 4;   // waves per workgroup, side by side
constexpr int kDetR = 32;      // output rows per strip (64 halves the halo rows but its 31 KB candidate buffer halves the resident
                               // workgroups: 548 instead of 413 us per 512 frames)

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));  // (bound_ctrl: an edge lane reads 0 without a zero-initialised destination)
}
#define LANE_LEFT(v) dpp_f32<0x138>(v)   /* wave_shr:1 -> value of lane - 1 */
#define LANE_RIGHT(v) dpp_f32<0x130>(v)  /* wave_shl:1 -> value of lane + 1 */

// sqrtf, correctly rounded, for arguments that are zero or normal numbers (what cornerMinEigenVal feeds it here: the
// derivative products are multiples of (1 / 3060)^2 rounded to float, so (a - c)^2 + b^2 is either 0 or above 1e-30 -- never a
// denormal, which is the one case the library expansion spends five more instructions on): the hardware estimate, then the
// neighbour whose residual changes sign (the same correction step the library uses).
__device__ __forceinline__ float sqrt_rn_normal(float x) {
  const float r = __builtin_amdgcn_sqrtf(x);
  const float rm = __int_as_float(__float_as_int(r) - 1), rp = __int_as_float(__float_as_int(r) + 1);
  const float em = __builtin_fmaf(-rm, r, x), ep = __builtin_fmaf(-rp, r, x);
  float y = em <= 0.f ? rm : r;
  y = ep > 0.f ? rp : y;
  // x == 0 needs no case of its own: r = 0, rm is a NaN pattern (0 - 1 ulp), so em is NaN and `em <= 0` is false; rp is the smallest
  // denormal, ep = fma(-rp, 0, 0) = 0 and `ep > 0` is false: y = r = 0. (Infinity cannot occur: the products are bounded by 255^2.)
  return y;
}

// One tile of the detector: NW waves side by side (NW * kDetW output columns), one strip of kDetR rows, tile (bxi, byi) of
// sequence `seq`. FULL = false is the product path (detect_kernel): candidates go to the workgroup's LDS list and from there
// to the strip's segment of the sequence's list, and a list that cannot take them all raises the sequence's flag in `ovf`.
// FULL = true is the exact redo of a flagged sequence (corner_select_kernel's redo workgroups): every pixel of the tile writes
// its key, or 0 when it is no candidate, to its own place y * cols + x of `full` -- no list, no counter, nothing to overflow.
// REGION: the sequence's region of interest (RegionArgs, fe_common.h) is what the discs are painted on: one more item per
// (wave, strip row) ORs the complement of the row's region bits under the wave's 64 columns into the same mask words.
template <bool IMG_MASK, bool FULL, int NW, bool REGION = false>
__device__ __forceinline__ void detect_tile(const uint8_t *img_base, size_t img_stride, const uint8_t *mask_base, size_t mask_stride,
                                            const int *kept_xy, const int *n_kept, int cap, const int *hw, int radius,
                                            unsigned *max_bits, int rows, int cols, unsigned long long *cand_base, int seg_cap,
                                            int *n_cand, int *ovf, int epoch, unsigned long long *full, int seq, int bxi, int byi, int nseg,
                                            const RegionArgs G = RegionArgs{nullptr, nullptr, 0}) {
  // Equal eigenvalues (a plateau: a tiled pattern, upscaled or saturated content) make EVERY pixel of the plateau a candidate
  // -- `v == m` holds for all of them, as in the reference's val == dilated --, so no list shorter than the tile holds every
  // input. The lists are sized for what ordinary images produce (a strict 3x3 maximum occupies at most one pixel in four);
  // what does not fit is not kept, the flag is raised, and the sequence is redone exactly behind this kernel.
  constexpr int kCandLds = NW * kDetW * kDetR / 4 + 64;
  __shared__ unsigned long long s_mask[NW][kDetR];
  __shared__ unsigned long long s_cand[FULL ? 1 : kCandLds];
  __shared__ unsigned smax;
  __shared__ int s_ncand, s_base, s_ndisc;
  __shared__ int2 s_disc[kMaxCap];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint8_t *img = img_base + (size_t)seq * img_stride;
  const int XB = bxi * (NW * kDetW), Y0 = byi * kDetR;
  const int X0 = XB + wave * kDetW;  // first output column of this wave; lane l <-> extended column X0 - 2 + l
  if (tid == 0) smax = 0, s_ncand = 0, s_ndisc = 0;
  if (tid < NW * kDetR) s_mask[tid / kDetR][tid % kDetR] = 0ull;
  __syncthreads();
  if (!IMG_MASK) {
    // disc rows that cross this workgroup's strip -> bits of the (wave, row) words
    // (1) every thread tests one kept feature against the strip, the few that touch it are listed in LDS;
    // (2) one item per (listed disc, strip row, wave) ORs the lanes the disc covers on that row.
    const int nk = n_kept[seq];
    for (int k = tid; k < nk; k += NW * 64) {
      const int cx = kept_xy[((size_t)seq * cap + k) * 2], cy = kept_xy[((size_t)seq * cap + k) * 2 + 1];
      if (cy + radius >= Y0 && cy - radius < Y0 + kDetR && cx + radius >= XB - 2 && cx - radius < XB + NW * kDetW + 2) {
        const int slot = atomicAdd(&s_ndisc, 1);
        s_disc[slot] = make_int2(cx, cy);  // (at most cap entries: every feature at most once)
      }
    }
    __syncthreads();
    const int nd = s_ndisc;
    for (int it = tid; it < nd * kDetR * NW; it += NW * 64) {
      const int wv = it % NW, r = (it / NW) % kDetR, dsc = it / (NW * kDetR);
      const int cx = s_disc[dsc].x, dy = Y0 + r - s_disc[dsc].y;
      if (dy < -radius || dy > radius) continue;
      const int h = hw[radius + dy];
      const int l0 = max(cx - h - (XB + wv * kDetW - 2), 0), l1 = min(cx + h - (XB + wv * kDetW - 2), 63);
      if (l0 > l1) continue;
      const unsigned long long bits = (l1 - l0 == 63 ? ~0ull : ((1ull << (l1 - l0 + 1)) - 1ull)) << l0;
      atomicOr(&s_mask[wv][r], bits);
    }
    if (REGION && G.set[seq]) {  // (uniform) the wave's window starts at column X0 - 2: a funnel shift of two region words
      for (int it = tid; it < NW * kDetR; it += NW * 64) {
        const int wv = it % NW, r = it / NW, y = Y0 + r;
        if (y < rows) atomicOr(&s_mask[wv][r], ~region_window(G.words + ((size_t)seq * rows + y) * G.wpr, G.wpr, XB + wv * kDetW - 2));
      }
    }
    __syncthreads();
  }
  const float s = (float)(1.0 / (4.0 * 3.0 * 255.0));
  const float s2 = s * 2.f;
  const __amdgpu_buffer_rsrc_t img_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)img, 0, rows * cols, 0x00020000);  // (raw bytes, bounds = the frame)
  // this lane's column (reflected like the product image) and its two neighbours for the Sobel taps
  const int xe = X0 - 2 + lane;
  const int xr = reflect101(min(max(xe, -cols + 1), 2 * cols - 2), cols);
  const int xm = reflect101(xr - 1, cols), xp = reflect101(xr + 1, cols);
  // Everything that slides down the strip has period three -- the (d, t) pairs of the three image rows in flight, the horizontal sums of
  // three product rows, three rows of eigenvalues --: each lives in a ring of three registers and the row loop is unrolled by three, so
  // that the slot of "the row that enters at this step" is a compile-time constant and NOTHING is moved when the window slides (with
  // named variables shifted at the end of a step the compiler kept ~11 register moves per row, a seventh of the loop's vector instructions:
  // the reload path of the border rows turned the shifted values into phi nodes it could not coalesce).
  float D[3] = {0.f, 0.f, 0.f}, T[3] = {0.f, 0.f, 0.f};                                  // slot s % 3: the image row that enters at step s
  float Hxx[3] = {0.f, 0.f, 0.f}, Hxy[3] = {0.f, 0.f, 0.f}, Hyy[3] = {0.f, 0.f, 0.f};    // slot s % 3: horizontal sums of step s's product row
  float E[3] = {0.f, 0.f, 0.f};                                                           // slot s % 3: eigenvalues formed at step s
  float my_max = -INFINITY;  // running masked maximum of this lane's column (one v_max per row; mapped to ordered bits once)
  int prev_yr = -1, prev_yp = -1;               // rows of the previous step (uniform)
  const bool out_lane = lane >= 2 && lane < 2 + kDetW && xe < cols;
  static_assert((kDetR + 4) % 3 == 0, "the row loop is unrolled by the rotation period");
  // The three bytes of the row that ENTERS at step s + 1 are fetched during step s (ring RB, slot s % 3): a step never waits for its own
  // loads. (Fetched where they were used, every row began with a memory round trip that seven resident waves per SIMD did not cover:
  // dropping 15 % of the row's vector instructions in a timing experiment bought 3.5 %.)
  unsigned RB[3][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}, {0u, 0u, 0u}};
  // The strip as a function of INNER (a compile-time flag): a strip whose rows y - 1 .. y + 1 all lie inside the image (13 of the 15
  // strips of a 480-row frame) needs no reflected row indices, never reloads rows and has no row bounds to test on its outputs. Those
  // were ~20 of the ~45 SCALAR instructions of a step -- and the CU's one scalar unit, shared by the 28 resident waves, was what the
  // kernel was bound by once the loads were out of the way (the row arithmetic without reflection, as a timing experiment: 324 -> 264 us).
  const bool inner_rows = Y0 - 3 >= 0 && Y0 + kDetR + 2 <= rows - 1;  // (uniform)
  auto strip = [&](auto inner_tag) {
  constexpr bool INNER = decltype(inner_tag)::value;
  auto entering_row = [&](int step) {  // image row that enters at `step`: y + 1 of extended product row Y0 - 2 + step
    if (INNER) return Y0 - 1 + step;
    const int yr_ = reflect101(min(max(Y0 - 2 + step, -rows + 1), 2 * rows - 2), rows);
    return reflect101(yr_ + 1, rows);
  };
  auto fetch_raw = [&](int y, unsigned (&b)[3]) {
    const int ro = __builtin_amdgcn_readfirstlane(y * cols);
    b[0] = __builtin_amdgcn_raw_buffer_load_b8(img_rsrc, xm, ro, 0), b[1] = __builtin_amdgcn_raw_buffer_load_b8(img_rsrc, xr, ro, 0),
    b[2] = __builtin_amdgcn_raw_buffer_load_b8(img_rsrc, xp, ro, 0);
  };
  fetch_raw(entering_row(0), RB[2]);
  // (three steps; HEAD: the first six of a strip, which still test whether an eigenvalue / an output row exists -- the loop behind them
  // does not: two scalar compares and branches per step less)
  auto three_steps = [&](int s0, auto head_tag) {
    constexpr bool HEAD = decltype(head_tag)::value;
#pragma unroll
    for (int u = 0; u < 3; u++) {
      const int step = s0 + u;
      const int jn = u, jm = (u + 1) % 3, jr = (u + 2) % 3;  // slots of the entering row (y + 1), of row y - 1 and of row y
      const int ye = Y0 - 2 + step;  // extended product row (uniform)
      const int yr = INNER ? ye : reflect101(min(max(ye, -rows + 1), 2 * rows - 2), rows);
      const int ym = INNER ? ye - 1 : reflect101(yr - 1, rows), yp = INNER ? ye + 1 : reflect101(yr + 1, rows);
      // Per image row the Sobel pair needs two numbers per column: the horizontal difference d = a(x+1) - a(x-1) and the
      // horizontal smoothing t = 2s a(x) + s (a(x-1) + a(x+1)); dx = 2s d(y) + s (d(y-1) + d(y+1)), dy = t(y+1) - t(y-1). Inside
      // the image the rows (y-1, y) of this step are the rows (y, y+1) of the previous one: only the entering row is loaded.
      auto row_dt = [&](int y, float &d, float &t) {
        // buffer loads: the row offset rides in the scalar offset operand, the column in the lane offset -- no address arithmetic
        // on the vector unit (three 64-bit adds per row with flat pointers)
        const int ro = __builtin_amdgcn_readfirstlane(y * cols);
        const float a0 = (float)__builtin_amdgcn_raw_buffer_load_b8(img_rsrc, xm, ro, 0), a1 = (float)__builtin_amdgcn_raw_buffer_load_b8(img_rsrc, xr, ro, 0),
                    a2 = (float)__builtin_amdgcn_raw_buffer_load_b8(img_rsrc, xp, ro, 0);
        d = a2 - a0;
        t = s2 * a1 + s * (a0 + a2);
      };
      if (INNER ? step == 0 : !(step > 0 && ym == prev_yr && yr == prev_yp)) row_dt(ym, D[jm], T[jm]), row_dt(yr, D[jr], T[jr]);  // (first step; image border: reflected rows)
      if (step + 1 < kDetR + 4) fetch_raw(entering_row(step + 1), RB[jn]);  // (uniform) next step's row, on its way under this step's arithmetic
      {
        const float a0 = (float)RB[jr][0], a1 = (float)RB[jr][1], a2 = (float)RB[jr][2];  // this step's row yp: fetched during the previous step
        D[jn] = a2 - a0;
        T[jn] = s2 * a1 + s * (a0 + a2);
      }
      prev_yr = yr, prev_yp = yp;
      const float dx = s2 * D[jr] + s * (D[jm] + D[jn]);
      const float dy = T[jn] - T[jm];
      const float pxx = dx * dx, pxy = dx * dy, pyy = dy * dy;
      // 3-tap horizontal sums (left + centre) + right, then the 3-row vertical sums (top + middle) + bottom
      Hxx[jn] = (LANE_LEFT(pxx) + pxx) + LANE_RIGHT(pxx);
      Hxy[jn] = (LANE_LEFT(pxy) + pxy) + LANE_RIGHT(pxy);
      Hyy[jn] = (LANE_LEFT(pyy) + pyy) + LANE_RIGHT(pyy);
      float e2 = 0.f;
      if (!HEAD || step >= 2) {  // eigenvalue of extended row ye - 1
        const float a = ((Hxx[jm] + Hxx[jr]) + Hxx[jn]) * 0.5f;
        const float b = (Hxy[jm] + Hxy[jr]) + Hxy[jn];
        const float c = ((Hyy[jm] + Hyy[jr]) + Hyy[jn]) * 0.5f;
        e2 = (a + c) - sqrt_rn_normal((a - c) * (a - c) + b * b);
      }
      E[jn] = e2;
      if (!HEAD || step >= 4) {  // output row ye - 2: centre E[jr], neighbours E[jm] / E[jn] and the lanes left and right
        const int y = ye - 2, r = step - 4;
        float m = fmaxf(fmaxf(E[jm], E[jr]), E[jn]);
        m = fmaxf(m, fmaxf(LANE_LEFT(m), LANE_RIGHT(m)));
        if (out_lane && (INNER || y < rows)) {
          const float v = E[jr];
          bool unmasked;
          if (IMG_MASK) unmasked = mask_base[(size_t)seq * mask_stride + (size_t)y * cols + xe] != 0;
          else unmasked = ((s_mask[wave][r] >> lane) & 1ull) == 0ull;
          if (FULL) {
            const bool is_cand = unmasked && xe >= 1 && xe < cols - 1 && (INNER || (y >= 1 && y < rows - 1)) && v > 0.f && v == m;
            const unsigned idx = (unsigned)y << 16 | (unsigned)xe;
            full[(size_t)y * cols + xe] = is_cand ? ((unsigned long long)__float_as_uint(v) << 32) | (0xffffffffu - idx) : 0ull;
          } else if (unmasked) {
            my_max = fmaxf(my_max, v);
            if (xe >= 1 && xe < cols - 1 && (INNER || (y >= 1 && y < rows - 1)) && v > 0.f && v == m) {
              const int slot = atomicAdd(&s_ncand, 1);
              const unsigned idx = (unsigned)y << 16 | (unsigned)xe;  // (row-major order like y * cols + x, and no division to take it apart)
              if (slot < kCandLds) s_cand[slot] = ((unsigned long long)__float_as_uint(v) << 32) | (0xffffffffu - idx);
            }
          }
        }
      }
    }
  };  // three_steps
  static_assert(kDetR + 4 > 6 && (kDetR + 4) % 6 == 0, "two head rounds, then rounds of six steps");
  three_steps(0, std::true_type{}), three_steps(3, std::true_type{});
#pragma unroll 1
  for (int s0 = 6; s0 < kDetR + 4; s0 += 6) three_steps(s0, std::false_type{}), three_steps(s0 + 3, std::false_type{});
  };  // strip
  if (inner_rows) strip(std::true_type{});
  else strip(std::false_type{});
  if (FULL) return;  // (the masked maximum is the first pass's: a list that overflows loses candidates, not the maximum)
  // masked maximum: wave max on the DPP/shuffle network, then one LDS atomic per wave
  {
    unsigned m = my_max == -INFINITY ? 0u : ordered_bits(my_max);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if (lane == 0 && m) atomicMax(&smax, m);
  }
  __syncthreads();
  // every strip of a sequence owns a segment of the candidate list and a counter / maximum slot, so the global
  // atomics of one address come from the few workgroups of that strip only
  const size_t segi = (size_t)seq * nseg + byi;
  const int nc = min(s_ncand, kCandLds);
  if (tid == 0 && nc) s_base = atomicAdd(&n_cand[segi], nc);
  __syncthreads();
  for (int i = tid; i < nc; i += NW * 64) {
    const int slot = s_base + i;
    if (slot < seg_cap) cand_base[segi * seg_cap + slot] = s_cand[i];
  }
  if (tid == 0 && smax) atomicMax(&max_bits[segi], smax);
  // candidates this workgroup's list or the strip's segment had no slot for: the sequence is redone (every workgroup that sees
  // it stores the same value; which candidates were dropped depends on the order the atomics arrived in, the flag does not).
  // The flag is this detection pass's number and is never cleared: a redo workgroup that cleared it could do so before the
  // sequence's ordinary selection workgroup has read it.
  if (tid == 0 && (s_ncand > kCandLds || (nc && s_base + nc > seg_cap))) ovf[seq] = epoch;
}

template <bool IMG_MASK, class... REG>
__global__ __launch_bounds__(256) void detect_kernel(const uint8_t *img_base, size_t img_stride, const uint8_t *mask_base,
                                                     size_t mask_stride, const int *kept_xy, const int *n_kept, int cap,
                                                     const int *hw, int radius, unsigned *max_bits, int rows, int cols,
                                                     unsigned long long *cand_base, int seg_cap, int *n_cand, int *ovf,
                                                     int epoch, const int *n_have, int max_corners, REG... region) {
  // n_max_cnt = MAX_CNT - forw_pts.size() <= 0: the reference does not call goodFeaturesToTrack at all (feature_tracker.cpp:256-266);
  // the sequence's candidate counters and maxima stay zero, which is "no corners" to the selection kernel
  if (n_have && n_have[blockIdx.z] >= max_corners) return;
  detect_tile<IMG_MASK, false, kDetWaves, sizeof...(REG) != 0>(img_base, img_stride, mask_base, mask_stride, kept_xy, n_kept, cap, hw, radius,
                                                               max_bits, rows, cols, cand_base, seg_cap, n_cand, ovf, epoch,
                                                               (unsigned long long *)nullptr, blockIdx.z, blockIdx.x, blockIdx.y, gridDim.y,
                                                               region_args(region...));
}

// Subset instantiation (the step's form: setMask discs, no mask image): blockIdx.z counts the PUBLISHED sequences of the call;
// the image is level 0 of the sequence's forw bank (M.pyr, img_stride apart).
template <class... REG>
__global__ __launch_bounds__(256) void detect_subset_kernel(SubsetArgs M, size_t img_stride, const int *kept_xy, const int *n_kept, int cap,
                                                            const int *hw, int radius, unsigned *max_bits, int rows, int cols,
                                                            unsigned long long *cand_base, int seg_cap, int *n_cand, int *ovf, int epoch,
                                                            const int *n_have, int max_corners, REG... region) {
  const int i = subset_at(M.pub, blockIdx.z), seq = subset_at(M.seq, i);
  if (n_have && n_have[seq] >= max_corners) return;
  detect_tile<false, false, kDetWaves, sizeof...(REG) != 0>(subset_bank(M, subset_at(M.forw_bank, i)), img_stride, (const uint8_t *)nullptr,
                                                            (size_t)0, kept_xy, n_kept, cap, hw, radius, max_bits, rows, cols, cand_base, seg_cap,
                                                            n_cand, ovf, epoch, (unsigned long long *)nullptr, seq, blockIdx.x, blockIdx.y, gridDim.y,
                                                            region_args(region...));
}

// vio_frontend_set_regions: byte masks (nonzero = usable) -> the bit rows of RegionArgs (fe_common.h), padding words included.
// Entry e of the call: image index[e] of `masks` (rows * cols bytes each) becomes the region of sequence seq[e]. One thread per
// word of a row; not in the per-frame path.
__global__ __launch_bounds__(256) void region_pack_kernel(const uint8_t *masks, const int *index, const int *seq, int rows, int cols, int wpr,
                                                          unsigned long long *words) {
  const int it = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
  if (it >= rows * wpr) return;
  const int y = it / wpr, w = it - y * wpr;
  const uint8_t *row = masks + ((size_t)index[e] * rows + y) * cols;
  unsigned long long bits = 0;
  const int x0 = (w - 1) * 64;  // (word 0 is padding: x0 < 0 reads nothing)
  for (int b = 0; b < 64; b++) {
    const int x = x0 + b;
    if (x >= 0 && x < cols && row[x] != 0) bits |= 1ull << b;
  }
  words[((size_t)seq[e] * rows + y) * wpr + w] = bits;
}

#undef LANE_LEFT
#undef LANE_RIGHT

}  // namespace
