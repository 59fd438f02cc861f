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
  const float ptx = prev_pts[pidx], pty = prev_pts[pidx + 1];
  const float half = (kWin - 1) * 0.5f;
  const float FLT_SCALE = 1.f / (1 << 20);
  constexpr int NPX = (kWin * kWin + 63) / 64;  // window pixels per lane: 7
  // This lane's window pixels (lk_layout.h): seven consecutive rows wy0 + q (q = 0..6) of column wx0 -- the q-th pixel sits a
  // CONSTANT q rows below the first, so the LDS reads of an iteration share one address register (+ immediate offsets)
  // instead of one address computation per pixel. (The sums over the window are exact integers: which lane owns which pixel
  // does not reach the result.)
  static_assert(NPX == lk_layout::kPxPerLane, "pixels per lane");
  const lk_layout::Px px0 = lk_layout::lane_pixel0(lane);
  const int wy0 = px0.row, wx0 = px0.col;  // (lane 63 owns nothing: it shadows lane 42's addresses, masked below)
  const int joff = wy0 * kJS + wx0;  // element offset of the first pixel in the staged J region
  bool st = true;
  float er = 0.f;
  float nxx = 0.f, nxy = 0.f;
  const int max_level = P.ld.levels - 1;
  for (int level = max_level; level >= 0; level--) {
    const int rows = P.ld.rows[level], cols = P.ld.cols[level];
    const uint8_t *I = pp + P.ld.off[level], *J = np + P.ld.off[level];
    if (level == 0) {  // (scalar selects)
      if (P.prev0) I = P.prev0 + (size_t)seq * P.stride0;
      if (P.next0) J = P.next0 + (size_t)seq * P.stride0;
    }
    const float scale = __int_as_float((127 - level) << 23);  // (float)(1. / (1 << level)) = 2^-level, without the double division
    float px = ptx * scale, py = pty * scale;
    float qx, qy;
    if (level == max_level) qx = px, qy = py;
    else qx = nxx * 2.f, qy = nxy * 2.f;
    nxx = qx, nxy = qy;
    px -= half, py -= half;
    int ipx = (int)floorf(px), ipy = (int)floorf(py);
    if (ipx < -kWin || ipx >= cols || ipy < -kWin || ipy >= rows) {
      if (level == 0) st = false, er = 0.f;
      continue;
    }
    float a = px - ipx, b = py - ipy;
    int iw00, iw01, iw10, iw11;
    lk_weights(a, b, iw00, iw01, iw10, iw11);
    // stage I on [ipx-1, ipx+23) x [ipy-1, ipy+23) (BORDER_REFLECT_101), then its Scharr derivatives on
    // [ipx, ipx+22) x [ipy, ipy+22): zero outside the image (copyMakeBorder BORDER_CONSTANT of derivI)
    wave_lds_fence();  // previous level's readers are done
    if (ipx >= 1 && ipx + kIP - 1 <= cols && ipy >= 1 && ipy + kIP - 1 <= rows) {
      // the patch lies inside the image (all but the features within a window of the border): FOUR pixels per lane and
      // load, 6 lanes per row, 10 rows per trip -- 3 trips instead of 12 (the kernel is VALU-issue-bound: staging the two
      // patches byte by byte was a quarter of a level's instructions)
      const int r = lane / 6, d = lane - 6 * r;
      constexpr int TI = (kIP + 9) / 10;
      uint32_t curs[TI];
#pragma unroll
      for (int t = 0; t < TI; t++) {  // (the loads of all trips in flight together: one global round trip per patch, not one per trip)
        const int ly = r + 10 * t;
        curs[t] = lk_load4(I + (unsigned)(__mul24(ipy - 1 + (ly < kIP ? ly : 0), cols) + ipx - 1 + 4 * d));
      }
#pragma unroll
      for (int t = 0; t < TI; t++) {  // (uniform trip count: the DPP below needs every lane)
        const int ly = r + 10 * t;
        const bool ok = lane < 60 && ly < kIP;
        const uint32_t cur = curs[t];
        uint32_t next = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cur, 0x130, 0xf, 0xf, false);  // dword of lane + 1
        if (d == 5) next = cur >> 24;  // (the pair behind the last pixel repeats it, like the byte path's clamped lane)
        uint32_t w4[4];
        lk_pairs(cur, next, w4);
        if (ok) {
#pragma unroll
          for (int k = 0; k < 4; k++) L.I[ly][4 * d + k] = w4[k];
        }
      }
    } else {  // 32 lanes per row (24 used), two rows per trip: the column index is reflected once per lane; the right-hand
       // neighbour of every pixel comes from the next lane (DPP wave_shl) so that a pair can be stored as one dword
      const int lx = lane & 31;
      const int x = reflect101(ipx - 1 + min(lx, kIP - 1), cols);
      // (a third of the features take this path at the coarse levels, where the patch is a quarter of the image: all loads
      // of the patch are issued before the first is consumed -- one memory round trip instead of one per trip)
      constexpr int RPT = 2, TB = kIP / RPT;
      static_assert(kIP % RPT == 0, "whole trips");
      int vs[TB];
#pragma unroll
      for (int t = 0; t < TB; t++) {
        // (the patch origin is the same in every lane, so the reflected ROW of a trip is one of two scalars -- even / odd half
        // of the wave -- and comes off the scalar unit: 2 vector instructions per trip instead of ~16; the border path is not
        // rare: 58 % of the features take it at level 3, 32 % at level 2)
        const int s_y0 = __builtin_amdgcn_readfirstlane(ipy) - 1 + RPT * t;
        const int ro_a = reflect101(s_y0, rows) * cols, ro_b = reflect101(s_y0 + 1, rows) * cols;
        vs[t] = I[(unsigned)(((lane >> 5) ? ro_b : ro_a) + x)];
      }
#pragma unroll
      for (int t = 0; t < TB; t++) {
        const int ly = (lane >> 5) + RPT * t, v = vs[t];
        const int vr = __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false);  // value of lane + 1
        if (lx < kIP) L.I[ly][lx] = (uint32_t)v | ((uint32_t)vr << 16);
      }
    }
    wave_lds_fence();
    // Scharr derivatives by COLUMN-PAIR WALK on packed 16-bit arithmetic: lanes 0..54 = 11 column pairs x five segments of five
    // output rows (the last one starts at row 17 and repeats three rows of its neighbour). A staged dword is a pixel pair
    // (I[x] | I[x+1] << 16), so the three pair words at columns c, c + 1, c + 2 are the left / centre / right taps of the derivative
    // columns c AND c + 1 at once: per input row h = P2 - P0 and v = 3 (P0 + P2) + 10 P1, per output row dx = 3 (h0 + h2) + 10 h1 and
    // dy = v2 - v0, each ONE v_pk_* instruction for both columns (|values| <= 16 x 255: exact in 16 bits) -- the same integers as the
    // 3 x 3 sums of calcSharrDeriv. (The one-column walk on 32-bit values, rounds 4-6: 168 vector instructions per level on 44 lanes,
    // a seventh of the kernel's; this form: ~75 on 55 lanes.)
    constexpr int SEG = 5, NSEG = 5, NCP = kDP / 2;
    static_assert(kDP % 2 == 0 && NCP * NSEG <= 64 && SEG * NSEG >= kDP && kDP >= SEG, "column pairs x segments");
    const bool inside = ipx >= 0 && ipx + kDP <= cols && ipy >= 0 && ipy + kDP <= rows;  // every derivative position is in the image
    if (lane < NCP * NSEG) {
      const int seg = lane / NCP, cp = lane - NCP * seg, c = 2 * cp;
      const int r0 = seg * SEG < kDP - SEG ? seg * SEG : kDP - SEG;
      const uint32_t *Ip = &L.I[0][0] + (__mul24(r0, kIS) + c);
      uint32_t *Dp = reinterpret_cast<uint32_t *>(&L.dI[0][0]) + (__mul24(r0, kDS) + c);
      const lk_s2 k3 = {3, 3}, k10 = {10, 10};
      auto walk = [&](auto checked) {  // (checked: the patch leaves the image -- derivI's BORDER_CONSTANT zeros)
        const unsigned ok0 = (unsigned)(ipx + c) < (unsigned)cols, ok1 = (unsigned)(ipx + c + 1) < (unsigned)cols;
        lk_s2 P0[SEG + 2], P1[SEG + 2], P2[SEG + 2];  // pair words of input row r0 + r: the staged patch holds reflected values at the image border
#pragma unroll
        for (int r = 0; r < SEG + 2; r++)  // (all reads ahead of the first write: one wait instead of one per row)
          __builtin_memcpy(&P0[r], Ip + r * kIS, 4), __builtin_memcpy(&P1[r], Ip + r * kIS + 1, 4), __builtin_memcpy(&P2[r], Ip + r * kIS + 2, 4);
        lk_s2 h[SEG + 2], v[SEG + 2];
#pragma unroll
        for (int r = 0; r < SEG + 2; r++) h[r] = P2[r] - P0[r], v[r] = (P0[r] + P2[r]) * k3 + P1[r] * k10;
#pragma unroll
        for (int r = 2; r < SEG + 2; r++) {
          const lk_s2 dx = (h[r - 2] + h[r]) * k3 + h[r - 1] * k10, dy = v[r] - v[r - 2];
          uint32_t ux, uy;
          __builtin_memcpy(&ux, &dx, 4), __builtin_memcpy(&uy, &dy, 4);
          uint32_t d0 = __builtin_amdgcn_perm(uy, ux, 0x05040100u), d1 = __builtin_amdgcn_perm(uy, ux, 0x07060302u);  // short2 {dx, dy} of columns c, c + 1
          if (decltype(checked)::value) {
            const unsigned rok = (unsigned)(ipy + r0 + r - 2) < (unsigned)rows;
            d0 &= 0u - (ok0 & rok), d1 &= 0u - (ok1 & rok);
          }
          Dp[(r - 2) * kDS] = d0, Dp[(r - 2) * kDS + 1] = d1;
        }
      };
      if (inside) walk(std::false_type{});
      else walk(std::true_type{});
    }
    wave_lds_fence();
    // template patch + derivatives for this lane's window pixels, kept in registers across the iterations
    // (the template value enters the iterations as the accumulator seed of the bilinear sample: rounding constant minus
    // Iv << n, so that the arithmetic shift that ends the sample yields J - I directly -- (a + r - (Iv << n)) >> n ==
    // ((a + r) >> n) - Iv exactly)
    // Ix, Iy of pixels 2h and 2h + 1 share a register: the iterations multiply-accumulate them pairwise (v_dot2_i32_i16).
    constexpr int NPP = (NPX + 1) / 2;
    const lk_s2 sw_top = {(short)iw00, (short)iw01}, sw_bot = {(short)iw10, (short)iw11};
    lk_s2 IxP[NPP], IyP[NPP];
    int Ic[NPX];
    int p11 = 0, p12 = 0, p22 = 0;  // per-lane partials: <= 14 products of |v| <= 4080^2 fit 32 bits
#pragma unroll
    for (int h = 0; h < NPP; h++) IxP[h] = IyP[h] = lk_s2{0, 0};
    // bilinear taps as dot products of packed pairs (a 32-bit integer multiply is a quarter-rate instruction here; the
    // element-wise form of this block was 12 of them per pixel): the I patch is staged as pairs already; the derivative
    // pairs (d[x], d[x+1]) are cut out of two (dx, dy) words with v_perm_b32. Weights <= 2^14 fit int16, and the SIGNED
    // dot keeps iw11 = 2^14 - iw00 - iw01 - iw10 right when the three roundings push it to -1.
    // The lane's pixels are consecutive rows of one column: the bottom row words of pixel q are the top row words of pixel
    // q + 1, read (and cut) once -- 8 reads of I and 16 of dI per lane instead of 14 and 28.
    const uint32_t *Iw = &L.I[wy0 + 1][wx0 + 1], *Dw = &L.dI[wy0][wx0];  // (I[x+1], I[x+2]) of row y + 1; (dx, dy) of [y][x]
    auto tap_row = [&](int k, lk_s2 &iv, lk_s2 &sx, lk_s2 &sy) {
      uint32_t d0, d1;
      __builtin_memcpy(&iv, Iw + k * kIS, 4);
      __builtin_memcpy(&d0, Dw + k * kDS, 4), __builtin_memcpy(&d1, Dw + k * kDS + 1, 4);
      const uint32_t xs = __builtin_amdgcn_perm(d1, d0, 0x05040100u), ys = __builtin_amdgcn_perm(d1, d0, 0x07060302u);
      __builtin_memcpy(&sx, &xs, 4), __builtin_memcpy(&sy, &ys, 4);
    };
    lk_s2 it, sxt, syt;
    tap_row(0, it, sxt, syt);
#pragma unroll
    for (int q = 0; q < NPX; q++) {  // (rows wy0 + q: always inside the window)
      lk_s2 ib, sxb, syb;
      tap_row(q + 1, ib, sxb, syb);
      const int ival = __builtin_amdgcn_sdot2(it, sw_top, __builtin_amdgcn_sdot2(ib, sw_bot, 1 << (kWBits - 5 - 1), false), false) >> (kWBits - 5);
      int ixval = __builtin_amdgcn_sdot2(sxt, sw_top, __builtin_amdgcn_sdot2(sxb, sw_bot, 1 << (kWBits - 1), false), false) >> kWBits;
      int iyval = __builtin_amdgcn_sdot2(syt, sw_top, __builtin_amdgcn_sdot2(syb, sw_bot, 1 << (kWBits - 1), false), false) >> kWBits;
      it = ib, sxt = sxb, syt = syb;
      if (lane >= 3 * kWin) ixval = iyval = 0;  // a pixel this lane does not own: weight zero in every sum below
      Ic[q] = (1 << (kWBits - 5 - 1)) - (int)((unsigned)ival << (kWBits - 5));
      if (q & 1) IxP[q >> 1].y = (short)ixval, IyP[q >> 1].y = (short)iyval;
      else IxP[q >> 1].x = (short)ixval, IyP[q >> 1].x = (short)iyval;
      p11 += ixval * ixval, p12 += ixval * iyval, p22 += iyval * iyval;
    }
    float f11, f12, f22;  // exact integer sums, rounded once to float
    wave_sum_exact3(p11, p12, p22, f11, f12, f22);
    float A11 = f11 * FLT_SCALE, A12 = f12 * FLT_SCALE, A22 = f22 * FLT_SCALE;
    float D = A11 * A22 - A12 * A12;
    float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (2 * kWin * kWin);
    if (minEig < P.min_eig || D < 1.1920929e-07f) {
      if (level == 0) st = false;
      continue;
    }
    D = 1.f / D;
    qx -= half, qy -= half;
    float pdx = 0.f, pdy = 0.f;
    int jox = 0, joy = 0;      // origin of the staged J region
    bool j_staged = false;
    auto stage_j = [&](int iqx, int iqy) {
      jox = iqx - kJMargin, joy = iqy - kJMargin;
      wave_lds_fence();
      if (jox >= 0 && jox + kJP <= cols && joy >= 0 && joy + kJP <= rows) {
        // inside the image: 4 pixels per lane and load, 7 lanes per row, 9 rows per trip -- 4 trips instead of 14
        const int r = lane / 7, d = lane - 7 * r;
        constexpr int TJ = (kJP + 8) / 9;
        uint32_t curs[TJ];
#pragma unroll
        for (int t = 0; t < TJ; t++) {
          const int ly = r + 9 * t;
          curs[t] = lk_load4(J + (unsigned)(__mul24(joy + (ly < kJP ? ly : 0), cols) + jox + 4 * d));
        }
#pragma unroll
        for (int t = 0; t < TJ; t++) {
          const int ly = r + 9 * t;
          const bool ok = lane < 63 && ly < kJP;
          const uint32_t cur = curs[t];
          uint32_t next = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cur, 0x130, 0xf, 0xf, false);
          if (d == 6) next = cur >> 24;
          uint32_t w4[4];
          lk_pairs(cur, next, w4);
          if (ok) {
#pragma unroll
            for (int k = 0; k < 4; k++) L.J[ly][4 * d + k] = w4[k];
          }
        }
      } else {  // 32 lanes per row (28 used), two rows per trip; pairs (J[x] | J[x+1] << 16) like the template patch
        const int lx = lane & 31;
        const int x = reflect101(min(max(jox + min(lx, kJP - 1), -cols + 1), 2 * cols - 2), cols);
        constexpr int RPT = 2, TB = kJP / RPT;
        static_assert(kJP % RPT == 0, "whole trips");
        int vs[TB];
#pragma unroll
        for (int t = 0; t < TB; t++) {  // (rows on the scalar unit, as in the template patch's border path)
          const int s_y0 = __builtin_amdgcn_readfirstlane(joy) + RPT * t;
          const int ro_a = reflect101(min(max(s_y0, -rows + 1), 2 * rows - 2), rows) * cols;
          const int ro_b = reflect101(min(max(s_y0 + 1, -rows + 1), 2 * rows - 2), rows) * cols;
          vs[t] = J[(unsigned)(((lane >> 5) ? ro_b : ro_a) + x)];
        }
#pragma unroll
        for (int t = 0; t < TB; t++) {
          const int ly = (lane >> 5) + RPT * t, v = vs[t];
          const int vr = __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false);  // value of lane + 1
          if (lx < kJP) L.J[ly][lx] = (uint32_t)v | ((uint32_t)vr << 16);
        }
      }
      wave_lds_fence();
      j_staged = true;
    };
    const uint32_t *Jl = &L.J[0][0];
    // (the top-row weights are never negative: their dot is the unsigned three-operand instruction, seeded with Ic without
    // a copy; the bottom row, whose iw11 can be -1, goes through the signed accumulate-in-place one)
    // (the pair words of the lane's eight rows, each read once: row q + 1 is the bottom of pixel q and the top of pixel q + 1)
    auto load_j = [&](int base, uint32_t (&jr)[NPX + 1]) {
#pragma unroll
      for (int k = 0; k <= NPX; k++) jr[k] = Jl[base + (joff + k * kJS)];  // (one address register + immediate offsets)
    };
    auto diff_j = [&](const uint32_t (&jr)[NPX + 1], int q, lk_us2 wtop, lk_s2 wbot) {  // bilinear J at this lane's q-th window pixel, minus I there
      lk_us2 top;
      lk_s2 bot;
      __builtin_memcpy(&top, &jr[q], 4);
      __builtin_memcpy(&bot, &jr[q + 1], 4);
      return __builtin_amdgcn_sdot2(bot, wbot, (int)__builtin_amdgcn_udot2(top, wtop, (unsigned)Ic[q], false), false) >> (kWBits - 5);  // (mod 2^32)
    };
    int nit = 0;  // (STATS only)
    for (int j = 0; j < P.max_count; j++) {
      int iqx = (int)floorf(qx), iqy = (int)floorf(qy);
      if (iqx < -kWin || iqx >= cols || iqy < -kWin || iqy >= rows) {
        if (level == 0) st = false;
        break;
      }
      if (STATS) nit++;
      if (!j_staged || iqx < jox || iqx > jox + 2 * kJMargin || iqy < joy || iqy > joy + 2 * kJMargin) stage_j(iqx, iqy);
      a = qx - iqx, b = qy - iqy;
      lk_weights(a, b, iw00, iw01, iw10, iw11);
      int pb1 = 0, pb2 = 0;  // |diff * dI| <= 16320 * 4080 per pixel, <= 14 pixels per lane: 9.3e8 fits 32 bits
      const lk_us2 wtop = {(unsigned short)iw00, (unsigned short)iw01};
      const lk_s2 wbot = {(short)iw10, (short)iw11};
      const int jbase = __mul24(iqy - joy, kJS) + (iqx - jox);
      uint32_t jr[NPX + 1];
      load_j(jbase, jr);
#pragma unroll
      for (int h = 0; h < NPP; h++) {  // (a pixel the lane does not own has Ix = Iy = 0)
        const int d0 = diff_j(jr, 2 * h, wtop, wbot), d1 = 2 * h + 1 < NPX ? diff_j(jr, 2 * h + 1, wtop, wbot) : 0;
        const unsigned pk = __builtin_amdgcn_perm((unsigned)d1, (unsigned)d0, 0x05040100u);  // |J - I| <= 8160: (d0, d1) as two int16
        lk_s2 dp;
        __builtin_memcpy(&dp, &pk, 4);
        pb1 = __builtin_amdgcn_sdot2(dp, IxP[h], pb1, false), pb2 = __builtin_amdgcn_sdot2(dp, IyP[h], pb2, false);
      }
      float fb1, fb2;  // the exact integer sums, rounded once to float (what (float) of the exact double gave)
      wave_sum_exact2(pb1, pb2, fb1, fb2);
      float b1 = fb1 * FLT_SCALE, b2 = fb2 * FLT_SCALE;
      float ddx = (A12 * b2 - A22 * b1) * D, ddy = (A12 * b1 - A11 * b2) * D;
      qx += ddx, qy += ddy;
      nxx = qx + half, nxy = qy + half;
      // delta.ddot(delta) <= epsilon in double, behind a float screen that only lets candidates through (conversions to and
      // from double are slow instructions; all but the last iteration of a level stop at the screen)
      if (!(ddx * ddx + ddy * ddy > P.epsilon_sq_f) && (double)ddx * ddx + (double)ddy * ddy <= P.epsilon_sq) break;
      // |x| < 0.01 for a float x: 0.01 (double) lies strictly between 0.01f and the next float up, so the float compare against
      // that next float decides the same
      constexpr float kCentiUp = 0.010000000707805157f;
      static_assert((double)kCentiUp > 0.01 && (double)0.01f < 0.01, "float neighbours of 0.01");
      if (j > 0 && fabsf(ddx + pdx) < kCentiUp && fabsf(ddy + pdy) < kCentiUp) {
        nxx -= ddx * 0.5f, nxy -= ddy * 0.5f;
        break;
      }
      pdx = ddx, pdy = ddy;
    }
    if (STATS && lane == 0) {  // (64 copies of the counters, picked by block: one address would serialize every wave of the launch)
      unsigned long long *sl = stats + ((blockIdx.x + 7 * blockIdx.y) & 63) * 16;
      atomicAdd(sl + level, (unsigned long long)nit);
      atomicAdd(sl + P.ld.levels + level, 1ull);
    }
    if (st && level == 0) {
      float ex = nxx - half, ey = nxy - half;
      int iex = (int)floorf(ex), iey = (int)floorf(ey);
      if (iex < -kWin || iex >= cols || iey < -kWin || iey >= rows) {
        st = false;
        continue;
      }
      if (!ERR) continue;  // (the range test above is the status' last word: it stays)
      if (!j_staged || iex < jox || iex > jox + 2 * kJMargin || iey < joy || iey > joy + 2 * kJMargin) stage_j(iex, iey);
      float aa = ex - iex, bb = ey - iey;
      lk_weights(aa, bb, iw00, iw01, iw10, iw11);
      int pe = 0;
      const lk_us2 wtop = {(unsigned short)iw00, (unsigned short)iw01};
      const lk_s2 wbot = {(short)iw10, (short)iw11};
      const int jbase = __mul24(iey - joy, kJS) + (iex - jox);
      uint32_t jr[NPX + 1];
      load_j(jbase, jr);
#pragma unroll
      for (int q = 0; q < NPX; q++) {
        const int d = abs(diff_j(jr, q, wtop, wbot));
        pe += lane < 3 * kWin ? d : 0;
      }
      const int se = wave_sum_i32(pe);  // <= 441 * 16320 < 2^23
      er = (float)se * 1.f / (32 * kWin * kWin);
    }
  }
  if (lane == 0) {
    next_pts[pidx] = nxx, next_pts[pidx + 1] = nxy;
    status[(size_t)seq * P.cap + pt] = st ? 1 : 0;
    if (ERR) err[(size_t)seq * P.cap + pt] = er;
  }
}

}  // namespace
