// spmd.h — the SPMD vocabulary every kernel header of the project is written in: the build modes, the phase macros
// (VIO_PARFOR / VIO_SYNC), LDS pointer types, atomics, the per-workgroup context with its stage clock, the block
// reductions and the wave-priority / flag / scheduling macros. Lowest layer: it knows nothing of any solver.
#pragma once

#include <math.h>
#include <stdint.h>

#include "vio_math.h"

// Three builds of the kernel headers:
//   hipcc (product)   the gfx950 kernel body;
//   -DVIO_EMUL        tests only: ONE emulated thread, no barriers, scalar stand-ins for the wave-level sections;
//   -DVIO_SIMT        tests only: the DEVICE sections themselves on the host, every work-item a fiber and every
//                     wave-level instruction (v_mfma, v_readlane, DPP, ballot, s_barrier) evaluated with the hardware's
//                     lane semantics by tests/emul/simt.h (included by the test harness before this file).
// (-DVIO_EMUL reaches this header, factors.h and pnp_core.h only: tests/emul/emul_pnp.cpp. The window solver and the
// wave-level tile code of mfma_tiles.h are built by hipcc and with -DVIO_SIMT.)
#if defined(VIO_EMUL) || defined(VIO_SIMT)
#define VIO_HOST_BUILD 1
#endif
#ifdef VIO_HOST_BUILD
#define VIO_DEV inline
#define VIO_ATOMIC_ADD(p, v) ::vio::atomic_add((p), (v))
#else
#define VIO_DEV __device__ __forceinline__
#define VIO_ATOMIC_ADD(p, v) ::vio::atomic_add((p), (v))
#endif
#if defined(VIO_EMUL)
#define VIO_SYNC() ((void)0)
#define VIO_SYNC_LDS() ((void)0)
#elif defined(VIO_SIMT)
#define VIO_SYNC() __syncthreads()
#define VIO_SYNC_LDS() __syncthreads()
#else
#define VIO_SYNC() __syncthreads()
// Workgroup barrier that only orders LDS traffic: __syncthreads() waits for every outstanding memory operation of the
// wave (s_waitcnt vmcnt(0)), which puts an L2 round trip behind each barrier a global prefetch is meant to cross.
// ONLY where the waves exchange nothing through global memory across the barrier.
#define VIO_SYNC_LDS()                                                      \
  do {                                                                      \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");         \
    __builtin_amdgcn_s_barrier();                                           \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");         \
  } while (0)
#endif
// The thread index every phase starts from passes through an empty asm: LLVM otherwise hoists the per-lane address
// arithmetic of ALL phases out of the trust-region loop (loop-invariant), keeps hundreds of values alive across the whole
// kernel and spills them to scratch -- a scratch_load (L2 latency) where two integer instructions would do.
#ifdef VIO_HOST_BUILD
#define VIO_TID(cx) ((int)(cx).tid)
#else
// (round 6: the index is REBUILT where it is asked for -- lane count of the wave + the wave's first index from a scalar register, two
// vector instructions -- instead of passing the kernel's v0 through the empty asm: the register allocator kept that one value in
// scratch and every phase began with a scratch_load of it, 111 of them in the W = 10 variant)
#define VIO_TID(cx) ::vio::hw_tid((cx).wave64)
#endif
#define VIO_PARFOR(i, n) for (int i = VIO_TID(cx); i < (int)(n); i += (int)cx.nt)
// The same for any per-lane value inside a loop: per-lane addresses that do not depend on the loop counter (the 60 tile
// offsets of a panel step, say) are otherwise computed once, kept alive around the loop and come back as scratch loads.
#ifdef VIO_HOST_BUILD
#define VIO_OPAQUE(x) (x)
#else
#define VIO_OPAQUE(x) ::vio::opaque_tid(x)
#endif

// LDS pointers carry their address space in the type: generic pointers make hipcc emit flat_load/flat_store for every
// LDS access (no ds_read/ds_write at all in the first version of this kernel), which is several times slower.
#ifdef VIO_HOST_BUILD
#define VIO_AS3
#else
#define VIO_AS3 __attribute__((address_space(3)))
#endif

namespace vio {

#ifndef VIO_HOST_BUILD
__device__ __forceinline__ int opaque_tid(int t) {
  asm volatile("" : "+v"(t));
  return t;
}
__device__ __forceinline__ int hw_tid(int wave64) {
  int t;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, %1\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(t) : "s"(wave64));
  return t;
}
#endif

typedef VIO_AS3 double *ldsd;
typedef const VIO_AS3 double *cldsd;
typedef VIO_AS3 int *ldsi;

#ifdef VIO_HOST_BUILD
inline void atomic_add(double *p, double v) { *p += v; }
inline void atomic_add_noret(double *p, double v) { *p += v; }
#else
// Global memory that several workgroups of ONE window may add to (cooperative windows): device scope. No return value: the
// instruction is fire-and-forget (global_atomic_add_f64 at the L2).
__device__ __forceinline__ void atomic_add_noret(double *p, double v) {
  (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void atomic_add(ldsd p, double v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void atomic_add(double *p, double v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // only this workgroup touches its scratch
}
#endif

// Per-stage cycle counters (the kernel-side counterpart of the reference's TS/TE timers, global_param.hpp:85-92).
enum Stage {
  ST_SETUP_IMU = 0, ST_SETUP_PRIOR, ST_EVAL_PRIOR, ST_EVAL_IMU, ST_EVAL_PROJ, ST_SCALE, ST_SCHUR, ST_RHS, ST_CHOL,
  ST_TRISOLVE, ST_QUADFORM, ST_DOGLEG, ST_COST_EVAL, ST_NEW2OLD, ST_MARG_BUILD, ST_MARG_CHOL, ST_TOTAL,
  // finer attribution (sub-stages; their cycles are NOT included in the stages above)
  ST_P_ZERO, ST_P_FACT, ST_P_GRAM, ST_P_FEAT,      // projection factors: zeroing, evaluation+staging, Gram, per-feature
  ST_C_POTRF, ST_C_TRSM,                           // Cholesky: first diagonal block, panel
  ST_IMU_RAW,                                      // raw IMU residual/Jacobian (one thread per factor)
  ST_C_WAIT, ST_Q_W, ST_BACKSOLVE, ST_C_AHEAD,     // trailing-update wait, W part of quad_form, back-substitution, wave-0 look-ahead
  ST_TR_VEC,                                       // trust-region vector phase before the linear solve
  ST_M_PRIOR, ST_M_IMU, ST_M_FACT, ST_M_GRAM,      // marginalization: prior/setup, IMU factor, factor staging, Gram
  ST_D0, ST_D1, ST_D2, ST_D3, ST_D4, ST_D5,         // free slots for timing experiments (VIO_AMD_PROF_TID picks the clock's lane)
  // round 6: the O(n) vector phases of a trust-region iteration, one slot per barrier interval
  ST_V_GD,                                         // |g_d|^2, Cauchy direction, quad_form vectors (one pass + reduction)
  ST_V_DOT, ST_V_STEP,                             // dogleg: the two inner products (+ reduction); step -> t2 / tf (+ barrier)
  ST_V_PLUS,                                       // Plus in place, stash of the iterate, norms (+ reduction)
  ST_V_GMAX,                                       // gradient max norm + the iteration record
  ST_V_REST,                                       // restore after a rejected step
  ST_B_INIT, ST_B_POSE, ST_B_ASP, ST_B_BAND, ST_B_GN,  // backsolve: copies; pose tiles; A_sp z_p; band chains (+ landmarks); GN step
  ST_E_HEAD, ST_E_COPY, ST_E_H0DX, ST_E_TAIL,      // evaluate(jac): rotations + zeroing; AppPr + PP copy (+ raw IMU); H0 dx + diagonal blocks; diag / scaling tail
  ST_X0, ST_X1, ST_X2, ST_X3,
  ST_S0, ST_S1, ST_S2, ST_S3,                       // round 11: the set-up's inner intervals together with D5 and X1 .. X3 (solve_window, setup_prior)
  ST_COUNT = 64                                    // (last slot = time of the previous stamp)
};

struct Ctx {
  int tid, nt;
  int wave64 = 0;     // index of the wave's first work-item (device: a scalar register, VIO_TID builds the index from it)
  ldsd red;           // LDS scratch for block reductions: two halves of [3 nt/64]
  mutable int red_phase = 0;  // which half the next reduction writes (uniform across the block)
  long long *prof;    // global [ST_COUNT] cycle accumulators of this window, or null; prof[ST_COUNT-1] = last stamp
  int wrot = 0;       // rotation of the wave ROLES in the serial phases: role = (wave + wrot) mod waves, role 0 runs the pivot
                      // chains. Two workgroups share a CU and the hardware puts wave w of both on the same SIMD: with the
                      // same roles the two chains would fight over one SIMD's matrix pipe while three stand idle.
  int prof_tid = 0;   // the work-item that keeps the stage clock (0; another wave's first lane to time what wave 0 does not run)
  VIO_AS3 long long *lprof;  // the same counters while the kernel runs (LDS); copied to prof at the end
  // cooperative windows (round 5): `coop` workgroups serve one window; member 0 owns the solve, the others wait for commands
  int coop = 1, member = 0;
  unsigned coop_spin = 1u << 24;  // polls before a wait between the workgroups of a window gives up (BatchPtrs::coop_spin)
  mutable unsigned coop_seq = 0;  // commands issued (owner) / served (helper) so far: the same value in every work-item
};

// Charges the cycles since the previous stamp to `stage` (thread 0 only; call between barriers).
VIO_DEV void stamp(const Ctx &cx, int stage) {
#if !defined(VIO_EMUL)
  if (cx.prof && cx.tid == cx.prof_tid) {  // accumulators live in LDS (a global read-modify-write per stamp costs ~3k cycles)
    long long t = clock64();
    cx.lprof[stage] += t - cx.lprof[ST_COUNT - 1];
    cx.lprof[ST_COUNT - 1] = t;
  }
#else
  (void)cx, (void)stage;
#endif
}

// ---- block reductions: every thread receives the same value ------------------------------------------------------
// Wave level on the DPP network (row_shr 1/2/4/8, row_bcast 15/31; total in lane 63, broadcast through SGPRs), block
// level through cx.red. Two alternating halves of cx.red make ONE barrier per reduction enough: a half is rewritten
// two calls later, and the barrier of the call in between orders that against its last readers.
#ifndef VIO_EMUL
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_move_f64(double v) {
  int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWMASK, 0xf, false);
  int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWMASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
  v += dpp_move_f64<0x111, 0xf>(v);
  v += dpp_move_f64<0x112, 0xf>(v);
  v += dpp_move_f64<0x114, 0xf>(v);
  v += dpp_move_f64<0x118, 0xf>(v);
  v += dpp_move_f64<0x142, 0xa>(v);
  v += dpp_move_f64<0x143, 0xc>(v);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ __forceinline__ double wave_max_f64(double v) {  // operands >= 0 (norms, flags): a shifted-in 0 is neutral
  v = fmax(v, dpp_move_f64<0x111, 0xf>(v));
  v = fmax(v, dpp_move_f64<0x112, 0xf>(v));
  v = fmax(v, dpp_move_f64<0x114, 0xf>(v));
  v = fmax(v, dpp_move_f64<0x118, 0xf>(v));
  v = fmax(v, dpp_move_f64<0x142, 0xa>(v));
  v = fmax(v, dpp_move_f64<0x143, 0xc>(v));
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
#endif
VIO_DEV double block_sum(const Ctx &cx, double v) {
#ifdef VIO_EMUL
  return v;
#else
  const int nw = cx.nt >> 6;
  ldsd red = cx.red + (cx.red_phase ^= 1) * 3 * nw;
  v = wave_sum_f64(v);
  if ((cx.tid & 63) == 0) red[cx.tid >> 6] = v;
  VIO_SYNC();
  double s = 0;
  for (int w = 0; w < nw; w++) s += red[w];
  return s;
#endif
}
// Three sums with one barrier.
VIO_DEV void block_sum3(const Ctx &cx, double &a, double &b, double &c) {
#ifndef VIO_EMUL
  const int nw = cx.nt >> 6;
  ldsd red = cx.red + (cx.red_phase ^= 1) * 3 * nw;
  a = wave_sum_f64(a), b = wave_sum_f64(b), c = wave_sum_f64(c);
  if ((cx.tid & 63) == 0) red[cx.tid >> 6] = a, red[nw + (cx.tid >> 6)] = b, red[2 * nw + (cx.tid >> 6)] = c;
  VIO_SYNC();
  a = b = c = 0;
  for (int w = 0; w < nw; w++) a += red[w], b += red[nw + w], c += red[2 * nw + w];
#else
  (void)cx, (void)a, (void)b, (void)c;
#endif
}
// Maximum of non-negative values.
VIO_DEV double block_max(const Ctx &cx, double v) {
#ifdef VIO_EMUL
  return v;
#else
  const int nw = cx.nt >> 6;
  ldsd red = cx.red + (cx.red_phase ^= 1) * 3 * nw;
  v = wave_max_f64(v);
  if ((cx.tid & 63) == 0) red[cx.tid >> 6] = v;
  VIO_SYNC();
  double s = red[0];
  for (int w = 1; w < nw; w++) s = fmax(s, red[w]);
  return s;
#endif
}

// Issue priority of the wave that walks a serial chain (pivots, band substitutions): with two windows per CU its SIMD is shared
// with a wave of the other window, and every cycle that wave wins the issue slot is a cycle on this window's critical path.
#if defined(VIO_HOST_BUILD)
#define VIO_PRIO(n) ((void)0)
#else
#define VIO_PRIO(n) __builtin_amdgcn_s_setprio(n)
#endif
// A flag in LDS that one wave posts and others poll (factor_band_regs)
#if defined(VIO_HOST_BUILD)
#define VIO_FLAG_STORE(p, x) (*(volatile int *)(p) = (x))
#define VIO_FLAG_LOAD(p) (*(volatile int *)(p))
#else
#define VIO_FLAG_STORE(p, x) __hip_atomic_store((p), (x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define VIO_FLAG_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#endif
#if defined(VIO_HOST_BUILD)
#define VIO_SCHED_FENCE() ((void)0)
#else
#define VIO_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

}  // namespace vio
