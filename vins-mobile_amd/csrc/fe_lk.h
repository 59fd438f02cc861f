// fe_lk.h -- calcOpticalFlowPyrLK (feature_tracker.cpp:181): one wave64 per feature, all pyramid levels, LK's sums
// accumulated exactly on the DPP network. The LDS layout of the staged windows is lk_layout.h.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "fe_common.h"
#include "lk_layout.h"

namespace {

// ---- pyramidal LK -------------------------------------------------------------------------------------
// Smallest float threshold such that fl(dx*dx + dy*dy) > threshold implies dx^2 + dy^2 > eps_sq in exact arithmetic (the float
// sum is within 2^-22 relative of the exact one; the margin is 1e-5).
inline float lk_eps_screen(double eps_sq) { return nextafterf((float)(eps_sq * (1.0 + 1e-5)), INFINITY); }
struct LkParams {
  LevelDims ld;
  int cap;             // feature slots per sequence
  int max_count;       // criteria.maxCount
  float epsilon_sq_f;  // screen of the convergence test: a float sum of squares above it cannot pass the double compare
  double epsilon_sq;
  float min_eig;
  // level 0 of either pyramid outside its pyramid buffer (resident frames are tracked where they lie: `forw_img = _img` is a
  // reference to the caller's pixels in the reference too, feature_tracker.cpp:169); null: level 0 is the pyramid's own copy
  const uint8_t *prev0, *next0;
  size_t stride0;  // bytes between the sequences' frames there
};

// Wave-wide integer sum on the DPP network (row_shr 1/2/4/8, row_bcast 15/31): no LDS round trips. The total lands
// in lane 63 and is broadcast through an SGPR.
__device__ __forceinline__ int wave_sum_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8   -> lane 15 of each row = row sum
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, 63);
}
// Exact sum over the wave of per-lane partials |p| < 2^30: split into 16-bit low part and high part so that both
// 32-bit reductions cannot overflow; returned as a double holding the exact integer.
__device__ __forceinline__ double wave_sum_exact(int p) {
  int lo = p & 0xffff, hi = p >> 16;
  int slo = wave_sum_i32(lo), shi = wave_sum_i32(hi);
  return (double)shi * 65536.0 + (double)slo;
}

__device__ __forceinline__ void lk_weights(float a, float b, int &iw00, int &iw01, int &iw10, int &iw11) {
  iw00 = __float2int_rn((1.f - a) * (1.f - b) * (1 << kWBits));
  iw01 = __float2int_rn(a * (1.f - b) * (1 << kWBits));
  iw10 = __float2int_rn((1.f - a) * b * (1 << kWBits));
  iw11 = (1 << kWBits) - iw00 - iw01 - iw10;
}

// LDS staging of one wave: the 24x24 template neighbourhood of I, its 22x22 Scharr derivative image and a
// (21+1+2*kJMargin)^2 region of J around the current estimate. Waves of a workgroup are independent (one feature
// each); LDS traffic of a wave is ordered, so a wave-level fence is all the synchronisation staging needs.
constexpr int kIP = kWin + 3;              // 24: window + 1 (bilinear) + 2 (Scharr halo)
constexpr int kDP = kWin + 1;              // 22: derivative positions
constexpr int kJMargin = 3;
constexpr int kJP = kWin + 1 + 2 * kJMargin;  // 28
// Row strides (dwords) of the staged arrays and the lane -> window pixel ownership come from lk_layout.h, with the model of
// the LDS banking they are chosen for: 32 dword banks, lanes 0-31 and 32-63 served apart, one extra cycle per further
// distinct dword on a busy bank. Every window read of the template build and of the iterations is conflict-free under it.
// (The previous layout -- lane l on column l % 21 of rows l / 21 + 3 q, strides 25 / 22 / 43 -- was laid out for 64 banks across the
// whole wave: +2 / +1 / +2 cycles on every 2-cycle read, 45 % of the kernel's LDS-array cycles were conflicts.)
constexpr int kIS = lk_layout::kStrideI, kDS = lk_layout::kStrideDI, kJS = lk_layout::kStrideJ;
static_assert(lk_layout::kWin == kWin && kIS >= kIP && kDS >= kDP && kJS >= kJP, "strides hold a row");
static_assert(lk_layout::window_reads_extra_cycles(kIS) == 0 && lk_layout::window_reads_extra_cycles(kDS) == 0 &&
                  lk_layout::window_reads_extra_cycles(kJS) == 0,
              "window reads of I, dI and J are free of LDS bank conflicts");
// Every staged pixel is ONE ALIGNED DWORD holding the pair (v[x] | v[x+1] << 16): sub-dword and unaligned LDS accesses
// crawl on this hardware (the byte-array version of this kernel spent 40 % of its wave cycles in LDS issue stalls).
// A pair is also exactly one v_dot2_u32_u16 operand, so a bilinear sample is two reads and two dot instructions
// (weights < 2^15, products < 2^22).
// The template patch and its derivatives are consumed (into registers) before the first J region of a level is staged,
// so the two share their LDS: 5.3 KB per feature (six workgroups per CU: 128 of 160 KB).
struct LkWaveLds {
  union {
    struct {
      uint32_t I[kIP][kIS];
      uint32_t dI[kDP][kDS];  // short2 {dx, dy}
    };
    uint32_t J[kJP][kJS];
  };
};

// Four consecutive pixels from an arbitrary byte address (global memory takes unaligned dword loads on this hardware).
struct __attribute__((packed)) LkU32 {
  uint32_t v;
};
__device__ __forceinline__ uint32_t lk_load4(const uint8_t *p) { return reinterpret_cast<const LkU32 *>(p)->v; }
// Pair words (v[x] | v[x+1] << 16) of the four pixels of `cur`; the fifth pixel is byte 0 of `next`.
__device__ __forceinline__ void lk_pairs(uint32_t cur, uint32_t next, uint32_t w[4]) {
  // v_perm_b32 selects bytes of {src0 (bytes 4..7), src1 (bytes 0..3)}; selector 0x0c yields 0x00
  w[0] = __builtin_amdgcn_perm(0u, cur, 0x0c010c00u);
  w[1] = __builtin_amdgcn_perm(0u, cur, 0x0c020c01u);
  w[2] = __builtin_amdgcn_perm(0u, cur, 0x0c030c02u);
  w[3] = __builtin_amdgcn_perm(next, cur, 0x0c040c03u);
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Two exact sums at once: the four 32-bit chains advance in lockstep, so that every DPP step finds
// its operand written three instructions earlier (a chain on its own waits two issue slots after every step).
// (every partial below 2^24 in magnitude -- what a window of ordinary contrast gives: the bounds are 2^28 -- means the 64-lane sums fit
// 32 bits unsplit: half the chains. The split form stays for the rest; both give the exact integer, rounded once.)
__device__ __forceinline__ bool wave_all_small(int p, int q, int r = 0) {
  const bool small = (unsigned)(p + (1 << 24)) < (1u << 25) && (unsigned)(q + (1 << 24)) < (1u << 25) && (unsigned)(r + (1 << 24)) < (1u << 25);
  return __builtin_amdgcn_ballot_w64(!small) == 0ull;
}
__device__ __forceinline__ void wave_sum_exact2(int p, int q, float &sp, float &sq) {
  if (wave_all_small(p, q)) {  // (uniform)
    int u[2] = {p, q};
#define VIO_DPPS(ctrl, rmask)                                                  \
  {                                                                            \
    const int t0 = __builtin_amdgcn_update_dpp(0, u[0], ctrl, rmask, 0xf, false); \
    const int t1 = __builtin_amdgcn_update_dpp(0, u[1], ctrl, rmask, 0xf, false); \
    u[0] += t0, u[1] += t1;                                                    \
  }
    VIO_DPPS(0x111, 0xf) VIO_DPPS(0x112, 0xf) VIO_DPPS(0x114, 0xf) VIO_DPPS(0x118, 0xf) VIO_DPPS(0x142, 0xa) VIO_DPPS(0x143, 0xc)
#undef VIO_DPPS
    sp = (float)__builtin_amdgcn_readlane(u[0], 63), sq = (float)__builtin_amdgcn_readlane(u[1], 63);
    return;
  }
  int a = p & 0xffff, b = q & 0xffff, c = p >> 16, d = q >> 16;
#define VIO_DPP4(ctrl, rmask)                                              \
  {                                                                        \
    const int ta = __builtin_amdgcn_update_dpp(0, a, ctrl, rmask, 0xf, false); \
    const int tb = __builtin_amdgcn_update_dpp(0, b, ctrl, rmask, 0xf, false); \
    const int tc = __builtin_amdgcn_update_dpp(0, c, ctrl, rmask, 0xf, false); \
    const int td = __builtin_amdgcn_update_dpp(0, d, ctrl, rmask, 0xf, false); \
    a += ta, b += tb, c += tc, d += td;                                    \
  }
  VIO_DPP4(0x111, 0xf) VIO_DPP4(0x112, 0xf) VIO_DPP4(0x114, 0xf) VIO_DPP4(0x118, 0xf) VIO_DPP4(0x142, 0xa) VIO_DPP4(0x143, 0xc)
#undef VIO_DPP4
  const int sa = __builtin_amdgcn_readlane(a, 63), sb = __builtin_amdgcn_readlane(b, 63), sc = __builtin_amdgcn_readlane(c, 63),
            sd = __builtin_amdgcn_readlane(d, 63);
  // |high sum| < 2^20 and low sum < 2^22 are exact floats, the product by 2^16 is exact: the one rounding is that of the add,
  // i.e. the result is the correctly rounded float of the exact integer (= (float) of the exact double)
  sp = (float)sc * 65536.f + (float)sa, sq = (float)sd * 65536.f + (float)sb;
}

// Three at once (the 2 x 2 system's A11, A12, A22; per-lane partials |p| <= 7 * 4080^2): the sum of a ROW of 16 lanes still
// fits 32 bits (< 1.87e9), so the four in-row steps run on the three unsplit values; only the two cross-row steps need the
// 16-bit halves (six chains).
__device__ __forceinline__ void wave_sum_exact3(int p, int q, int r, float &sp, float &sq, float &sr) {
  if (wave_all_small(p, q, r)) {  // (uniform)
    int w[3] = {p, q, r};
#define VIO_DPPS3(ctrl, rmask)                                                                                       \
  {                                                                                                                   \
    int t[3];                                                                                                         \
    _Pragma("unroll") for (int k = 0; k < 3; k++) t[k] = __builtin_amdgcn_update_dpp(0, w[k], ctrl, rmask, 0xf, false); \
    _Pragma("unroll") for (int k = 0; k < 3; k++) w[k] += t[k];                                                       \
  }
    VIO_DPPS3(0x111, 0xf) VIO_DPPS3(0x112, 0xf) VIO_DPPS3(0x114, 0xf) VIO_DPPS3(0x118, 0xf) VIO_DPPS3(0x142, 0xa) VIO_DPPS3(0x143, 0xc)
#undef VIO_DPPS3
    sp = (float)__builtin_amdgcn_readlane(w[0], 63), sq = (float)__builtin_amdgcn_readlane(w[1], 63), sr = (float)__builtin_amdgcn_readlane(w[2], 63);
    return;
  }
  int u[3] = {p, q, r};
#define VIO_DPPN(N, arr, ctrl, rmask)                                               \
  {                                                                                 \
    int t[N];                                                                       \
    _Pragma("unroll") for (int k = 0; k < N; k++) t[k] = __builtin_amdgcn_update_dpp(0, arr[k], ctrl, rmask, 0xf, false); \
    _Pragma("unroll") for (int k = 0; k < N; k++) arr[k] += t[k];                   \
  }
  VIO_DPPN(3, u, 0x111, 0xf) VIO_DPPN(3, u, 0x112, 0xf) VIO_DPPN(3, u, 0x114, 0xf) VIO_DPPN(3, u, 0x118, 0xf)
  int v[6] = {u[0] & 0xffff, u[1] & 0xffff, u[2] & 0xffff, u[0] >> 16, u[1] >> 16, u[2] >> 16};
  VIO_DPPN(6, v, 0x142, 0xa) VIO_DPPN(6, v, 0x143, 0xc)
#undef VIO_DPPN
  int s[6];
#pragma unroll
  for (int k = 0; k < 6; k++) s[k] = __builtin_amdgcn_readlane(v[k], 63);
  sp = (float)s[3] * 65536.f + (float)s[0], sq = (float)s[4] * 65536.f + (float)s[1], sr = (float)s[5] * 65536.f + (float)s[2];
}

// One feature per wave. prev/next pyramids: per sequence `pyr_bytes` apart. pts arrays: [seq][cap][2].
// Occupancy: the kernel is latency-bound on its dependent chains (LDS round trips, DPP reductions), not on VALU issue —
// two features per wave (half the wave-uniform instructions per feature, but 154 VGPRs = 3 waves per SIMD) was measured
// SLOWER (1.36 vs 1.28 ms per front-end step), more resident waves are faster: with the LDS per feature down to 4.3 KB the
// register count is what limits residency, so the kernel is compiled for 6 waves per SIMD (80 VGPRs, no spills; 95 -> 5
// waves before): front-end step 1.28 -> 1.17 ms. (8 waves per SIMD = 64 VGPRs spills 17 registers and gains another 0.5 %.)
// ERR: the error output of calcOpticalFlowPyrLK (mean |J - I| over the window at the final position: one more bilinear pass,
// at times a re-stage of J, and a wave sum per tracked feature). readImage never reads it, so the step path launches
// ERR = false: no pass and no store to `err`; next_pts and status are the same in both.
template <bool STATS = false, bool ERR = true>
__global__ __launch_bounds__(256, 6) void lk_track_kernel(const uint8_t *prev_pyr, const uint8_t *next_pyr, LkParams P,
                                                       const int *n_pts, const float *prev_pts, float *next_pts,
                                                       uint8_t *status, float *err, unsigned long long *stats) {
  __shared__ LkWaveLds lds_all[4];
  const int seq = blockIdx.y;
  // (the wave index off the scalar unit: the feature's slot and its output index stay in scalar registers to the end)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int pt = blockIdx.x * (blockDim.x >> 6) + wave;
  if (pt >= n_pts[seq]) return;
  LkWaveLds &L = lds_all[wave];
  const uint8_t *pp = prev_pyr + (size_t)seq * P.ld.pyr_bytes, *np = next_pyr + (size_t)seq * P.ld.pyr_bytes;
  const size_t pidx = ((size_t)seq * P.cap + pt) * 2;
#include "fe_lk_body.inc"
}

// Subset instantiation (the step's form: no counters, no error pass): blockIdx.y is a call position, the sequence and its two
// banks come from the call's plan -- three scalar loads ahead of the feature's work, nothing in a vector register. A sequence's
// first frame has nothing to track from (prev_bank < 0). Same launch bounds: 80 VGPRs, six waves per SIMD (DESIGN.md has the
// compiler's figures for both).
__global__ __launch_bounds__(256, 6) void lk_track_subset_kernel(SubsetArgs M, LkParams P, const int *n_pts, const float *prev_pts,
                                                                 float *next_pts, uint8_t *status) {
  constexpr bool STATS = false, ERR = false;
  float *const err = nullptr;
  unsigned long long *const stats = nullptr;
  __shared__ LkWaveLds lds_all[4];
  const int pb = subset_at(M.prev_bank, blockIdx.y);
  if (pb < 0) return;
  const int seq = subset_at(M.seq, blockIdx.y);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int pt = blockIdx.x * (blockDim.x >> 6) + wave;
  if (pt >= n_pts[seq]) return;
  LkWaveLds &L = lds_all[wave];
  const uint8_t *pp = subset_bank(M, pb) + (size_t)seq * P.ld.pyr_bytes;
  const uint8_t *np = subset_bank(M, subset_at(M.forw_bank, blockIdx.y)) + (size_t)seq * P.ld.pyr_bytes;
  const size_t pidx = ((size_t)seq * P.cap + pt) * 2;
#include "fe_lk_body.inc"
}

}  // namespace
