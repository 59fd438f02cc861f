// vio_window_kernel.inc -- the window kernel (one workgroup per window, or several: cooperative windows) and its launch table.
// Included by vio_wk_unit.hip, compiled once per (variant, PROF) pair of vio_window_variants.h (PROF = true: the stage clock).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "batch.h"
#include "marg_core.h"

#include "vio_window_variants.h"

namespace vio_wk {
using namespace vio;

// What a launch of the WS > 0 instantiations promises (checked by the launcher, static_launch_ok): spelled out to the compiler.
template <int WS>
__device__ __forceinline__ void static_dims(BatchPtrs &B) {
  if constexpr (WS > 0) {
    BatchDims &d = B.d;
    d.Wcap = WS, d.Pcap = WS + 1, d.nblk_cap = WS + 1, d.n6cap = 6 * (WS + 2), d.Ncap = 6 * WS + 15;
    d.pair_cap = (WS + 2) * (WS + 3) / 2;
    BatchStrides &s = B.s;
    s.pose = 7 * (WS + 1), s.sb = 9 * (WS + 1), s.ex = 7, s.preint = (size_t)WS * kPreintDoubles, s.pair = d.pair_cap;
    s.pr_int = kMaxPriorBlocks, s.pr_x0 = 9 * (size_t)kMaxPriorBlocks, s.pr_J = (size_t)d.Ncap * d.Ncap, s.pr_r = d.Ncap;
    s.out_pose = s.pose, s.out_sb = s.sb, s.out_loop = 7, s.stats_d = kStatsDoubles, s.stats_i = kStatsInts;
    // (offsets inside the per-window scratch block that do not depend on the landmark / factor capacities)
    s.s_WTf = scratch_fixed_offsets(WS, d.Ncap, d.nblk_cap, s);
  }
}
template <int WS>
__device__ __forceinline__ WinView static_view(WinView v) {
  if constexpr (WS > 0) {
    v.W = WS, v.P = WS + 1, v.has_loop = 0, v.np = kBS * (WS + 1), v.nblk = WS + 1, v.npose6 = 6 * (WS + 1);
    v.Pcap = WS + 1, v.nblk_cap = WS + 1, v.n6cap = 6 * (WS + 2);
    v.n6 = v.npose6, v.nrows = v.n6 + 1, v.nT = (v.nrows + 15) >> 4, v.jp = (6 * (WS + 1) + 1 + 15) / 16 * 16;
  }
  return v;
}

// NT threads; WPE: waves per SIMD the register budget is sized for (2: 256 VGPRs, two 256-thread workgroups or one
// 512-thread workgroup per CU)
// LDS_ASP: the IMU speed-bias x pose coupling is in LDS as well (B.d.lds_asp says the same to the layout)
// PROF: the stage clock (vio_backend_set_profile). The product launches PROF = false: cx.prof is then a compile-time null and every
// stamp() of the kernel folds away -- with the counters' pointer a run-time value each of the ~100 stamps a wave passes per
// iteration cost ~18 instructions whether the clock ran or not (the pointer sits in a spilled scalar register), 9 % of the
// kernel's instructions. The PROF = true instantiations are translation units of their own (vio_wk_unit.hip, vio_window_variants.h).
// WS: 0 = the window size, the batch capacities and with them every stride and the LDS layout are run-time values (any window the
// layout takes); WS > 0 = a launch whose windows all have W = WS frames, no relocalization pose and the capacities that go with
// it (static_dims / static_view below: the launcher checks, vio_backend.hip) -- the reference's WINDOW_SIZE is a compile-time 10
// as well (VINS_ios/global_param.hpp:28). Strides, trip counts, tile counts and the addresses of the fixed-size LDS arrays are
// then constants instead of ~90 scalar registers that live (mostly spilled) through the whole kernel.
template <bool LDS_MATRIX, bool LDS_ASP, int NT, bool PROF, int WS>
__global__ __launch_bounds__(NT, 2) void vio_window_kernel(BatchPtrs B_, MargPtrs MP, int lds_doubles) {
  BatchPtrs B = B_;
  static_dims<WS>(B);
  extern __shared__ __attribute__((aligned(16))) double smem[];
  // Cooperative windows (B.coop > 1 workgroups per window, solver_core.h): the members of window i are the blocks
  // 8 coop (i / 8) + 8 m + i % 8 -- workgroups go to the XCDs round-robin by block index, so the members of a window share
  // an XCD and meet in its L2.
  const int coop = LDS_MATRIX ? 1 : B.coop;
  int widx = (int)blockIdx.x, member = 0;
  if (coop > 1) {
    const int grp = (int)blockIdx.x / (8 * coop), r = (int)blockIdx.x - grp * 8 * coop;
    member = r >> 3, widx = grp * 8 + (r & 7);
    if (widx >= B.n_launch) return;  // (the last group of eight is padded)
  }
  const int b = B.order ? B.order[widx] : widx;
  WinView v = static_view<WS>(make_view(B, b));
  typedef typename std::conditional<LDS_MATRIX, ldsd, double *>::type MatP;
  typedef typename std::conditional<LDS_MATRIX && LDS_ASP, ldsd, double *>::type AspP;
  ldsd lds = (ldsd)smem;
  // (by value: neither struct ever has its address taken, so both live in registers)
  // (the layout flag as a compile-time constant: as a run-time value it costs the LDS variant ~80 more scratch reloads)
  BatchDims dims = B.d;
  dims.lds_asp = LDS_ASP ? 1 : 0;
  dims.prof_stages = PROF ? ST_COUNT : 0;  // (the launcher sets the same: the layout with / without the clock's LDS slots)
  const Carved<MatP, AspP> cw = carve_all<MatP, AspP>(dims, LDS_MATRIX, NT, lds, B.hm + (size_t)b * B.s.hm, v.AspG, (size_t)lds_doubles);
  WorkT<MatP, AspP> w = cw.w;
  Ctx cx;
  cx.tid = threadIdx.x, cx.nt = NT;
  cx.wave64 = __builtin_amdgcn_readfirstlane((int)threadIdx.x & ~63);
  cx.prof = (PROF && MP.prof) ? MP.prof + (size_t)b * ST_COUNT : nullptr;
  cx.prof_tid = MP.prof_tid;
  {
    // which workgroup slot of its CU this workgroup occupies (HW_ID.TG_ID, bits 19:16): the second workgroup of a CU
    // rotates its wave roles so that its pivot-chain wave sits on another SIMD than the first one's
    if (threadIdx.x == 0) cw.w.flag[0] = (int)__builtin_amdgcn_s_getreg(0x1C04) & 3;
    __syncthreads();
    cx.wrot = MP.wrot >= 0 ? MP.wrot : (NT == 256 ? cw.w.flag[0] : 0);
    __syncthreads();
  }
  // (the stage clock follows the chain wave: work-item 0 of role 0)
  if (MP.prof_tid == 0) cx.prof_tid = ((NT / 64 - cx.wrot) & (NT / 64 - 1)) * 64;
  else cx.prof_tid = (((MP.prof_tid >> 6) - cx.wrot) & (NT / 64 - 1)) * 64;
  cx.red = cw.red, cx.lprof = cw.lprof;
  cx.coop = coop, cx.member = member;
  cx.coop_spin = LDS_MATRIX ? 0u : B.coop_spin;
  if (!LDS_MATRIX && member > 0) {
    if (!B.coop_fault) coop_helper(cx, v, w);
    return;
  }
  const size_t state_end = cw.state_end_doubles;
  // (the window index as an opaque scalar: the view a phase asks for is derived again from the kernel's arguments)
  auto fresh = [&]() {
    int bb = b;
    asm volatile("" : "+s"(bb));
    // (the window's header values stay in registers: a re-derived view reads them from global memory again otherwise, a dependent
    // scalar load at the head of every phase)
    WinView f = static_view<WS>(make_view(B, bb));
    f.F = v.F, f.M = v.M, f.marg_flag = v.marg_flag, f.prior_n = v.prior_n, f.prior_nb = v.prior_nb, f.npairs = v.npairs;
    f.nslots = v.nslots, f.nrev = v.nrev, f.use_origin = v.use_origin, f.loop_frame = v.loop_frame;
    f.s_info = v.s_info;  // (the same for the window's sqrt_info, a header double: every phase with projection factors reads it)
    if (WS == 0) f.W = v.W, f.P = v.P, f.has_loop = v.has_loop, f.np = v.np, f.nblk = v.nblk, f.npose6 = v.npose6, f.n6 = v.n6, f.nrows = v.nrows, f.nT = v.nT;
    return f;
  };
  auto fresh_work = [&]() { return w; };  // (the LDS layout derived again per iteration was tried: 5 % slower)
  solve_window<LDS_MATRIX, NT / 64>(cx, v, w, fresh, fresh_work);

  MargOut mo;
  int *mi = MP.ints + (size_t)b * MP.s_ints;
  mo.n = mi, mo.kind = mi + 4, mo.index = mo.kind + kMaxPriorBlocks, mo.offset = mo.index + kMaxPriorBlocks;
  mo.x0 = MP.x0 + (size_t)b * MP.s_x0, mo.J = MP.J + (size_t)b * MP.s_J, mo.r = MP.r + (size_t)b * MP.s_r;
  mo.scratch = MP.scratch ? MP.scratch + (size_t)b * MP.s_scratch : nullptr;
  mo.ncap = B.d.Ncap;
  if (B.ptab && B.ptab[b].mJ) mo.x0 = B.ptab[b].mx0, mo.J = B.ptab[b].mJ, mo.r = B.ptab[b].mr, mo.ncap = B.ptab[b].ncap;
  MargWorkT<MatP> mw = carve_marg_all<MatP>(B.d, LDS_MATRIX, lds + state_end, mo.scratch, (size_t)lds_doubles - state_end - cw.tail_doubles).m;
  __syncthreads();
  if (coop > 1) {  // the helpers go home (the marginalization below is the owner's alone)
    coop_post(cx, v, COOP_EXIT);
    // (a wait between the workgroups of this window timed out: the solve is wrong. The host reads -9, reports the window as
    // FAILURE and returns VIO_ETIMEOUT from the download)
    if (cx.tid == 0 && coop_flags(v)[2]) v.stats_i[1] = -9;
  }
  marginalize_window_impl<LDS_MATRIX ? 0 : 1>(cx, fresh(), w.xpose, w.xsb, w.xfeat, w.ex, mw, mo);
  if (cx.prof && cx.tid == cx.prof_tid) {  // stage counters: LDS -> global
    cx.lprof[ST_TOTAL] += clock64();
    for (int q = 0; q < ST_COUNT; q++) cx.prof[q] = cx.lprof[q];
  }
}


}  // namespace vio_wk

