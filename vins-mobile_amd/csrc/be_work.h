// be_work.h — part of vio_backend.hip: what the host-window path and the device-resident path share once a batch is planned
// (wk_plan.h) -- the work and output buffers, a slot's entry of the prior table, and the two launches of the window kernel.
#pragma once
#include "be_state.h"

namespace {

// Debug aid (VIO_AMD_POISON=1): every launch is preceded by NaN patterns in the whole LDS of every CU and in all device
// scratch / output buffers, so that a read of something the kernel did not write itself cannot go unnoticed.
__global__ __launch_bounds__(1024) void poison_lds_kernel(int n_doubles) {
  extern __shared__ __attribute__((aligned(16))) double poison_smem[];
  for (int i = threadIdx.x; i < n_doubles; i += blockDim.x) poison_smem[i] = __longlong_as_double(0x7ff8dead0000beefLL);
  __syncthreads();
  if (poison_smem[(threadIdx.x * 7) % n_doubles] == 1.0) poison_smem[0] = 2.0;  // keep the stores alive
}

}  // namespace

// Work and output buffers of the planned batch of N windows with strides s (sticky: they only grow), and the work / output side
// of be->B and be->MP over them (the input arrays and B.ptab are bound by the caller).
static int bind_work_buffers(vio_backend *be, const BatchStrides &s, size_t N) {
  const BatchDims &d = be->plan.d;
  const size_t m_scr = be->plan.lds_matrix() ? 0 : marg_scratch_doubles(d.Wcap), s_J = (size_t)d.Ncap * d.Ncap;
  int rc = VIO_OK;
  auto ensure = [&rc](auto &buf, size_t count) {
    if (rc == VIO_OK) rc = buf.ensure(count);
  };
  ensure(be->d_scratch, N * s.scratch);
  ensure(be->d_hm, be->plan.lds_matrix() ? 1 : N * s.hm);  // (indexed by window: sized for the whole batch when any window needs it)
  ensure(be->d_out_pose, N * s.out_pose);
  ensure(be->d_out_sb, N * s.out_sb);
  ensure(be->d_out_feat, N * s.out_feat);
  ensure(be->d_raw_pose, N * s.out_pose);
  ensure(be->d_raw_sb, N * s.out_sb);
  ensure(be->d_raw_feat, N * s.out_feat);
  ensure(be->d_out_loop, N * s.out_loop);
  ensure(be->d_stats_d, N * s.stats_d);
  ensure(be->d_stats_i, N * s.stats_i);
  ensure(be->d_m_ints, N * kMargInts);
  ensure(be->d_m_x0, N * 9 * kMaxPriorBlocks);
  ensure(be->d_m_J, N * s_J);
  ensure(be->d_m_r, N * (size_t)d.Ncap);
  ensure(be->d_m_scratch, m_scr ? N * m_scr : 1);
  if (be->profile) ensure(be->d_prof, N * ST_COUNT);
  if (rc != VIO_OK) return rc;
  BatchPtrs &B = be->B;
  B.scratch = be->d_scratch.p, B.hm = be->d_hm.p, B.order = nullptr, B.coop = 1, B.n_launch = 0;
  B.coop_spin = vio::kCoopSpinLimit, B.coop_fault = 0;
  B.out_pose = be->d_out_pose.p, B.out_sb = be->d_out_sb.p, B.out_feat = be->d_out_feat.p;
  B.raw_pose = be->d_raw_pose.p, B.raw_sb = be->d_raw_sb.p, B.raw_feat = be->d_raw_feat.p;
  B.out_loop = be->d_out_loop.p, B.stats_d = be->d_stats_d.p, B.stats_i = be->d_stats_i.p;
  MargPtrs &MP = be->MP;
  MP.ints = be->d_m_ints.p, MP.x0 = be->d_m_x0.p, MP.J = be->d_m_J.p, MP.r = be->d_m_r.p;
  MP.scratch = m_scr ? be->d_m_scratch.p : nullptr;
  MP.s_ints = kMargInts, MP.s_x0 = 9 * kMaxPriorBlocks, MP.s_J = s_J, MP.s_r = d.Ncap, MP.s_scratch = m_scr;
  MP.prof = be->profile ? be->d_prof.p : nullptr;
  MP.prof_tid = vio::env_int("VIO_AMD_PROF_TID", 0);
  MP.wrot = vio::env_int("VIO_AMD_WAVE_ROT", -1);
  return VIO_OK;
}

// Where the window of prior slot k reads its prior (from_store: it has one, and its data lives in the store) and where it writes
// the next one: the two banks of the prior store. ncap: capacity the kernel may assume of the next prior's arrays.
static PriorTab prior_tab(const vio_backend *be, int k, bool from_store, int ncap) {
  const size_t sx = 9 * kMaxPriorBlocks, sJ = (size_t)be->st_ncap * be->st_ncap, sr = be->st_ncap;
  const int cur = be->st_bank[k], nxt = 1 - cur;
  PriorTab t = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ncap};
  if (from_store) t.x0 = be->d_st_x0[cur].p + k * sx, t.J = be->d_st_J[cur].p + k * sJ, t.r = be->d_st_r[cur].p + k * sr;
  t.mx0 = be->d_st_x0[nxt].p + k * sx, t.mJ = be->d_st_J[nxt].p + k * sJ, t.mr = be->d_st_r[nxt].p + k * sr;
  return t;
}

// The launches of the bound batch B (with be->MP, by be->plan; the order list is on the device) on stream st: the LDS variant's
// windows, then the global-matrix variant's.
static int launch_windows(vio_backend *be, hipStream_t st, const BatchPtrs &B) {
  const vio_wk::Layout &P = be->plan;
  const bool prof = be->MP.prof != nullptr;
  be->last_stream = st;
  if (poison()) {
    HIP_OK(hipMemsetAsync(be->d_scratch.p, 0xff, be->d_scratch.n * sizeof(double), st));
    HIP_OK(hipMemsetAsync(be->d_hm.p, 0xff, be->d_hm.n * sizeof(double), st));
    HIP_OK(hipMemsetAsync(be->d_out_pose.p, 0xff, be->d_out_pose.n * sizeof(double), st));
    HIP_OK(hipMemsetAsync(be->d_stats_d.p, 0xff, be->d_stats_d.n * sizeof(double), st));
    HIP_OK(hipFuncSetAttribute((const void *)poison_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)vio_wk::kLdsLimit));
    hipLaunchKernelGGL(poison_lds_kernel, dim3(2048), dim3(1024), vio_wk::kLdsLimit, st, (int)(vio_wk::kLdsLimit / sizeof(double)));
  }
  if (const int rc = be->timer.begin(st); rc != VIO_OK) return rc;
  if (P.n_lds > 0) {
    BatchPtrs Bl = B;
    Bl.d = P.d_lds, Bl.order = be->d_order.p;
    vio_wk::variant(P.variant, prof).launch(P.n_lds, P.lds_bytes, st, Bl, be->MP);
  }
  be->coop_width = 1;
  if (P.n_glb > 0) {
    BatchPtrs Bg = B;
    Bg.d = P.d_glb, Bg.order = be->d_order.p + P.n_lds;
    // VIO_AMD_COOP = 1 / 2 / 4 forces the cooperative width (read per launch: tests switch it within one process)
    int coop = vio_wk::coop_width(P.n_glb, P.d_glb.Wcap, P.lds_bytes_glb, be->n_cus, be->peers, vio::env_int("VIO_AMD_COOP", 0), prof, be->coop_ok);
    // every workgroup of the launch has to be resident at once (the members of a window wait for each other): ask the runtime
    // what the device holds of this kernel at this LDS size instead of trusting the plan's arithmetic alone
    int per_cu = 0;
    if (coop > 1 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, vio_wk::variant(vio_wk::kGlbVariant, false).fn, vio_wk::kThreadsGlb,
                                                                  P.lds_bytes_glb) != hipSuccess ||
                     (long long)per_cu * vio_wk::cus_share(be->n_cus, be->peers) < (long long)vio_wk::coop_grid(P.n_glb, coop)))
      coop = 1;
    Bg.coop = coop, Bg.n_launch = P.n_glb;
    be->coop_width = coop;
    // test hooks of the timeout path (tests/test_backend_gpu.py): read per launch
    const int spin = vio::env_int("VIO_AMD_COOP_SPIN", 0);
    Bg.coop_spin = spin > 0 ? (unsigned)spin : vio::kCoopSpinLimit;
    Bg.coop_fault = vio::env_flag("VIO_AMD_COOP_FAULT") ? 1 : 0;
    if (coop > 1)
      // flag words of every window of the batch: command, completions, error (the first 32 bytes of the cooperative area)
      HIP_OK(hipMemset2DAsync(be->d_scratch.p + B.s.s_coop, B.s.scratch * sizeof(double), 0, 32, (size_t)B.n, st));
    vio_wk::variant(vio_wk::kGlbVariant, prof).launch(vio_wk::coop_grid(P.n_glb, coop), P.lds_bytes_glb, st, Bg, be->MP);
  }
  HIP_OK(hipGetLastError());
  return be->timer.end(st);
}
