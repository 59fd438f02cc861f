// vio_backend.hip — gfx950 kernels and C ABI of the sliding-window back-end (include/vio_amd.h).
//
// One workgroup owns one window for the whole of VINS::solve_ceres (VINS_ios/VINS.cpp:480-831): solve, new2old,
// marginalization. At W <= 12 the reduced system (pose matrix 22 KB + speed-bias band 14 KB, solver_core.h) and every
// vector of the solve fit in 80 KB of LDS: 256 threads (4 wave64) per window, TWO windows resident per CU, so that one
// window's serial pivot chains run in the shadow of the other's parallel phases. The batch of independent sequences
// is the grid: a launch of >= 512 windows fills the chip and each XCD's L2 only ever sees its own windows' scratch.
// Larger windows keep the pose matrix in global scratch and take a CU each (512 threads).
// This file: the table of instantiations and the entry points of the host-window path. The contexts are in be_state.h, what both
// paths share once a batch is planned in be_work.h, the launch policy in wk_plan.h, the device-resident path in be_resident.h.
#include <cmath>

#include "be_state.h"
#include "be_work.h"
#include "be_resident.h"

// The instantiations of the window kernel, one translation unit each (vio_wk_unit.hip, csrc/Makefile).
#define VIO_WK_DECL(v) vio_wk::VariantFns vio_wk_variant_##v##_0(); vio_wk::VariantFns vio_wk_variant_##v##_1();
VIO_WK_DECL(0) VIO_WK_DECL(1) VIO_WK_DECL(2) VIO_WK_DECL(3) VIO_WK_DECL(4)
#undef VIO_WK_DECL
const vio_wk::VariantFns &vio_wk::variant(int v, bool prof) {
  static const VariantFns tab[kVariants][2] = {{vio_wk_variant_0_0(), vio_wk_variant_0_1()}, {vio_wk_variant_1_0(), vio_wk_variant_1_1()},
                                               {vio_wk_variant_2_0(), vio_wk_variant_2_1()}, {vio_wk_variant_3_0(), vio_wk_variant_3_1()},
                                               {vio_wk_variant_4_0(), vio_wk_variant_4_1()}};
  return tab[v][prof ? 1 : 0];
}

extern "C" {

const char *vio_version(void) { return "vio_amd 0.1 (gfx950)"; }

int vio_host_pool_width(int32_t *n_pools) {
  if (n_pools) *n_pools = vio::HostPool::count();
  return vio::HostPool::get().width();
}

int vio_hip_runtime(char *path, int32_t cap, int32_t *n_runtimes) {
  const std::vector<std::string> r = vio::hip_runtimes();
  if (n_runtimes) *n_runtimes = (int32_t)r.size();
  if (path && cap > 0) {
    std::string all;
    for (size_t i = 0; i < r.size(); i++) all += (i ? ";" : "") + r[i];
    strncpy(path, all.c_str(), (size_t)cap - 1);
    path[cap - 1] = 0;
  }
  return VIO_OK;
}

void vio_config_default(VioConfig *c) {
  // iPhone7P, global_param.cpp:27-42; feature_tracker.hpp:24-29; global_param.hpp:28-58
  c->window_size = 10, c->max_features = 1000, c->max_factors = 8192, c->max_iterations = 10;
  c->image_rows = 640, c->image_cols = 480, c->max_corners = 70, c->min_dist = 30, c->freq = 3;
  c->lk_win = 21, c->lk_levels = 3, c->lk_max_iters = 30, c->lk_eps = 0.01, c->lk_min_eig = 1e-4;
  c->quality_level = 0.01, c->f_threshold = 1.0, c->f_confidence = 0.99;
  c->fx = 526.600, c->fy = 526.678, c->cx = 243.481, c->cy = 315.280;
  c->gravity = 9.805, c->acc_n = 0.5, c->acc_w = 0.002, c->gyr_n = 0.2, c->gyr_w = 4.0e-5, c->cauchy_a = 1.0;
}

int32_t vio_prior_capacity(int32_t window_size) { return 15 * (window_size + 1) + 6; }

int vio_backend_create(const VioConfig *cfg, int32_t max_batch, vio_backend_t **out) {
  if (!cfg || !out || max_batch < 1) return VIO_EINVAL;
  if (!vio::device_ready("the back-end")) return VIO_ENODEV;
  vio_backend *be = new (std::nothrow) vio_backend();
  if (!be) return VIO_ENOMEM;
  be->cfg = *cfg;
  be->max_batch = max_batch;
  be->device = vio::current_device();
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, be->device) == hipSuccess && prop.multiProcessorCount > 0) be->n_cus = prop.multiProcessorCount;
  }
  // the dynamic-LDS ceiling is a property of the FUNCTION, not of a launch: raised once to the CU's whole LDS for both
  // variants (several contexts on several host threads launch these kernels; a per-launch value could be lowered by
  // another thread between this thread's set and its launch)
  for (int v = 0; v < vio_wk::kVariants; v++)
    for (int p = 0; p < 2; p++)
      if (hipFuncSetAttribute(vio_wk::variant(v, p != 0).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)vio_wk::kLdsLimit) != hipSuccess) {
        delete be;
        return VIO_ENODEV;
      }
  if (hipStreamCreateWithFlags(&be->stream, hipStreamNonBlocking) != hipSuccess) {
    delete be;
    return VIO_ENODEV;
  }
  *out = be;
  return VIO_OK;
}

int vio_backend_get_device(const vio_backend_t *be, int32_t *device) {
  if (!be || !device) return VIO_EINVAL;
  *device = be->device;
  return VIO_OK;
}

void vio_backend_destroy(vio_backend_t *be) {
  if (!be) return;
  vio::DeviceScope scope(be->device);
  delete be;
}

int vio_backend_reserve_priors(vio_backend_t *be, int32_t n_slots) {
  if (!be || n_slots < 0) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(be);
  HIP_OK(hipStreamSynchronize(be->last_stream ? be->last_stream : be->stream));
  be->uploaded = false;
  be->st_n = 0;
  const int ncap = 6 * be->cfg.window_size + 15;  // what marginalize() can leave behind: W poses, one speed-bias, the extrinsic
  for (int k = 0; k < 2; k++) {
    int rc = be->d_st_x0[k].ensure((size_t)n_slots * 9 * kMaxPriorBlocks);
    if (rc == VIO_OK) rc = be->d_st_J[k].ensure((size_t)n_slots * ncap * ncap);
    if (rc == VIO_OK) rc = be->d_st_r[k].ensure((size_t)n_slots * ncap);
    if (rc != VIO_OK) return rc;
  }
  be->st_n = n_slots, be->st_ncap = ncap;
  be->st_bank.assign(n_slots, 0);
  return VIO_OK;
}

int vio_backend_upload(vio_backend_t *be, const VioWindow *windows, int32_t n) { return vio_backend_upload_cam(be, windows, n, nullptr); }

int vio_backend_upload_cam(vio_backend_t *be, const VioWindow *windows, int32_t n, const double *sqrt_info) try {  // (the staging vectors and the packers allocate: no exception crosses the ABI)
  if (!be || !windows || n < 1) return VIO_EINVAL;
  if (n > be->max_batch) return VIO_ECAP;
  for (int b = 0; sqrt_info && b < n; b++)
    if (!(std::isfinite(sqrt_info[b]) && sqrt_info[b] > 0)) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(be);
  be->uploaded = false;  // a failed upload leaves nothing to launch or download
  be->coop_ok = false;  // (set again below once every global-matrix window is known to be packed for a cooperative launch)
  // an earlier launch may still be reading the device inputs this upload overwrites (it may have gone to a caller's
  // stream): wait for it first
  if (be->last_stream && be->last_stream != be->stream) HIP_OK(hipStreamSynchronize(be->last_stream));
  // device-resident prior chain: which windows name a slot, and whether any prior data crosses the host at all
  be->slot_of.assign(n, -1);
  be->host_prior_in = false, be->host_prior_out = false;
  bool any_slot = false;
  {
    std::vector<char> taken(be->st_n, 0);
    for (int b = 0; b < n; b++) {
      const VioWindow &w = windows[b];
      if (w.resident_prior < 0 || w.resident_prior > be->st_n) return VIO_EINVAL;
      const int slot = w.resident_prior - 1;
      if (slot >= 0) {
        if (taken[slot]) return VIO_EINVAL;
        taken[slot] = 1, any_slot = true;
        if (w.prior && w.prior->n > be->st_ncap) return VIO_ECAP;
      }
      be->slot_of[b] = slot;
      if (w.prior && w.prior->n > 0 && w.prior->linearized_jacobians) be->host_prior_in = true;
      if (w.next_prior && slot < 0) be->host_prior_out = true;
    }
  }
  int Wmax = 1, Fmax = 1, Mmax = 1, Nmax = 0;
  bool any_loop = false, all_w = true;  // all_w: every window has the size the compile-time instantiations are built for
  std::vector<int> nfeat(n);
  for (int b = 0; b < n; b++) {
    const VioWindow &w = windows[b];
    nfeat[b] = w.n_features, all_w = all_w && w.window_size == vio_wk::kStaticW;
    if (w.window_size < 1 || w.n_features < 0 || w.n_factors < 0) return VIO_EINVAL;
    if (w.window_size > be->cfg.window_size || w.n_features > be->cfg.max_features ||
        w.n_factors > be->cfg.max_factors)
      return VIO_ECAP;
    Wmax = std::max(Wmax, w.window_size), Fmax = std::max(Fmax, w.n_features), Mmax = std::max(Mmax, w.n_factors);
    if (w.prior) Nmax = std::max(Nmax, w.prior->n);
    if (w.factor_target)
      for (int k = 0; k < w.n_factors; k++)
        if (w.factor_target[k] == w.window_size + 1) any_loop = true;
  }
  // The capacities are sticky while the batch keeps its size (wk_plan.h); the plan carves the LDS for THIS batch's landmarks.
  const vio_wk::Need need = {Wmax, Fmax, Mmax, Nmax, any_loop};
  const bool keep = be->hb.sized && n == be->hb.n && vio_wk::fits(be->hb.d, need);
  be->plan = vio_wk::plan_layout(keep ? be->hb.d : vio_wk::grow_dims(be->cfg, need, vio_wk::kHostGrowth, nullptr), n, nfeat.data(), nullptr, all_w,
                                 be->n_cus, be->peers, be->profile);
  if (be->plan.rc != VIO_OK) return be->plan.rc;
  const vio_wk::Layout &P = be->plan;
  const BatchDims &d = P.d;
  // the previous upload's copy may still be reading the staging arena (uploads do not wait for their own transfer)
  HIP_OK(hipStreamSynchronize(be->stream));
  const double t0 = now_ms();
  be->hb.resize(d, n, poison());
  {
    std::vector<int> rcs(n, VIO_OK);
    std::vector<char> glb(n, 0), strad(n, 0);
    for (size_t i = (size_t)P.n_lds; i < P.order.size(); i++) glb[P.order[i]] = 1;
    vio::HostPool::get().parallel_for(n, [&](int b) {
      try {
        bool st_ = false;
        rcs[b] = pack_window(be->hb, b, windows[b], be->slot_of[b] >= 0, glb[b] ? P.chunk_glb : P.chunk, &st_);
        if (sqrt_info) be->hb.hdr_d[(size_t)b * kHdrDoubles + 4] = sqrt_info[b];  // the window's own camera (VINS.cpp:31)
        strad[b] = st_ ? 1 : 0;
      } catch (const std::bad_alloc &) {  // (worker thread: must not unwind out of the pool)
        rcs[b] = VIO_ENOMEM;
      }
    });
    for (int b = 0; b < n; b++)
      if (rcs[b] != VIO_OK) return rcs[b];
    be->coop_ok = P.n_glb > 0;
    for (int b = 0; b < n; b++)
      if (glb[b] && strad[b]) be->coop_ok = false;
  }
  const double t1 = now_ms();
  const BatchStrides &s = be->hb.s;
  if (be->d_order.ensure(n) != VIO_OK) return VIO_ENOMEM;
  be->h_order.assign(P.order.begin(), P.order.end());  // page-locked: goes up with the other staging copies below

  const size_t N = (size_t)n;
  if (const int rc = be->d_in.ensure(be->hb.total_bytes); rc != VIO_OK) return rc;
  if (const int rc = bind_work_buffers(be, s, N); rc != VIO_OK) return rc;
  hipStream_t st = be->stream;
  HIP_OK(hipMemcpyAsync(be->d_order.p, be->h_order.data(), sizeof(int) * N, hipMemcpyHostToDevice, st));
  // one copy for every input array; the prior data ([in_bytes, total_bytes): the bulk, ~45 KB per window at W=10) only
  // when some prior of this upload travels through the host
  HIP_OK(hipMemcpyAsync(be->d_in.p, be->hb.arena.data(), be->host_prior_in ? be->hb.total_bytes : be->hb.in_bytes,
                        hipMemcpyHostToDevice, st));
  if (any_slot) {
    if (be->d_ptab.ensure(n) != VIO_OK) return VIO_ENOMEM;
    be->h_ptab.resize(n);
    for (int b = 0; b < n; b++) {
      const VioPrior *p = windows[b].prior;
      const int k = be->slot_of[b];
      be->h_ptab[b] = k >= 0 ? prior_tab(be, k, p && p->n > 0 && !p->linearized_jacobians, std::min(be->st_ncap, d.Ncap)) : PriorTab{};
    }
    HIP_OK(hipMemcpyAsync(be->d_ptab.p, be->h_ptab.data(), sizeof(PriorTab) * N, hipMemcpyHostToDevice, st));
  }
  if (!be->upload_done) HIP_OK(hipEventCreateWithFlags(&be->upload_done, hipEventDisableTiming));
  HIP_OK(hipEventRecord(be->upload_done, st));
  // (no wait here: the launch follows on the same stream, and the staging arena is not touched again before the wait at
  // the top of the next upload)
  if (host_timing()) fprintf(stderr, "vio_backend_upload: pack %.2f ms, alloc+H2D calls %.2f ms (n=%d)\n", t1 - t0, now_ms() - t1, n);

  BatchPtrs &B = be->B;
  B.n = n, B.d = d, B.s = s;
  {
    const size_t *o = be->hb.off;
    unsigned char *base = be->d_in.p;
    auto ip = [&](int k) { return reinterpret_cast<int *>(base + o[k]); };
    auto dp = [&](int k) { return reinterpret_cast<double *>(base + o[k]); };
    B.hdr = ip(0), B.fhost = ip(1), B.ftarget = ip(2), B.ffeat = ip(3), B.fslot = ip(4), B.fstart = ip(5);
    B.pair_h = ip(6), B.pair_t = ip(7), B.pair_s0 = ip(8), B.pair_s1 = ip(9);
    B.pr_kind = ip(10), B.pr_index = ip(11), B.pr_offset = ip(12);
    B.hdr_d = dp(13), B.pose = dp(14), B.sb = dp(15), B.ex = dp(16), B.feat = dp(17), B.pts_i = dp(18), B.pts_j = dp(19);
    B.preint = dp(20), B.pr_x0 = dp(21), B.pr_J = dp(22), B.pr_r = dp(23);
  }
  B.ptab = any_slot ? be->d_ptab.p : nullptr;
  be->n = n;
  be->uploaded = true, be->slots_advanced = false;
  return VIO_OK;
} catch (const std::bad_alloc &) {
  return VIO_ENOMEM;
}

int vio_backend_launch(vio_backend_t *be, void *stream) {
  if (!be) return VIO_EINVAL;
  if (!be->uploaded) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(be);
  hipStream_t st = stream ? (hipStream_t)stream : be->stream;
  if (st != be->stream && be->upload_done) HIP_OK(hipStreamWaitEvent(st, be->upload_done, 0));
  return launch_windows(be, st, be->B);
}

int vio_backend_sync(vio_backend_t *be) {
  if (!be) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(be);
  HIP_OK(hipDeviceSynchronize());
  return VIO_OK;
}

int vio_backend_kernel_ms(vio_backend_t *be, double *ms_avg, int32_t *launches) {
  if (!be || !ms_avg || !launches) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(be);
  HIP_OK(hipDeviceSynchronize());
  return be->timer.drain(ms_avg, launches);
}

int vio_backend_coop_width(const vio_backend_t *be, int32_t *width) {
  if (!be || !width) return VIO_EINVAL;
  *width = be->coop_width;
  return VIO_OK;
}

int vio_backend_set_profile(vio_backend_t *be, int32_t enable) {
  if (!be) return VIO_EINVAL;
  be->profile = enable != 0;
  be->uploaded = false;  // takes effect at the next upload
  return VIO_OK;
}

int vio_backend_stage_cycles(vio_backend_t *be, int32_t window, int64_t *cycles, int32_t n_stages) {
  if (!be || !cycles || n_stages < 1) return VIO_EINVAL;
  if (!be->uploaded || !be->profile || window < 0 || window >= be->n) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(be);
  HIP_OK(hipDeviceSynchronize());
  long long tmp[ST_COUNT];
  HIP_OK(hipMemcpy(tmp, be->d_prof.p + (size_t)window * ST_COUNT, sizeof(tmp), hipMemcpyDeviceToHost));
  for (int i = 0; i < n_stages; i++) cycles[i] = i < ST_COUNT ? (int64_t)tmp[i] : 0;
  return VIO_OK;
}

int vio_backend_download(vio_backend_t *be, VioWindow *windows, int32_t n, VioSolveStats *stats) try {  // (the page-locked host copies are (re)sized here)
  if (!be || !windows) return VIO_EINVAL;
  if (!be->uploaded || n != be->n) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(be);
  const double t0 = now_ms();
  // only this context's launch: other contexts (other host threads) keep the device busy meanwhile
  HIP_OK(hipStreamSynchronize(be->last_stream ? be->last_stream : be->stream));
  const double t1 = now_ms();
  hipStream_t st = be->stream;
  HIP_OK(d2h(be->h_out_pose, be->d_out_pose, st));
  HIP_OK(d2h(be->h_out_sb, be->d_out_sb, st));
  HIP_OK(d2h(be->h_out_feat, be->d_out_feat, st));
  HIP_OK(d2h(be->h_raw_pose, be->d_raw_pose, st));
  HIP_OK(d2h(be->h_raw_sb, be->d_raw_sb, st));
  HIP_OK(d2h(be->h_raw_feat, be->d_raw_feat, st));
  HIP_OK(d2h(be->h_out_loop, be->d_out_loop, st));
  HIP_OK(d2h(be->h_stats_d, be->d_stats_d, st));
  HIP_OK(d2h(be->h_stats_i, be->d_stats_i, st));
  HIP_OK(d2h(be->h_m_ints, be->d_m_ints, st));
  if (be->host_prior_out) {
    HIP_OK(d2h(be->h_m_x0, be->d_m_x0, st));
    HIP_OK(d2h(be->h_m_J, be->d_m_J, st));
    HIP_OK(d2h(be->h_m_r, be->d_m_r, st));
  }
  HIP_OK(hipStreamSynchronize(st));
  const double t2 = now_ms();
  const BatchStrides &s = be->hb.s;
  vio::HostPool::get().parallel_for(n, [&](int b) {
    unpack_window(s, b, be->h_out_pose.data(), be->h_out_sb.data(), be->h_out_feat.data(), be->h_raw_pose.data(),
                  be->h_raw_sb.data(), be->h_raw_feat.data(), be->h_out_loop.data(), be->h_stats_d.data(),
                  be->h_stats_i.data(), windows[b], stats ? stats + b : nullptr);
    if (windows[b].next_prior) {
      MargOut mo = marg_header(be->h_m_ints.data() + (size_t)b * be->MP.s_ints, be->B.d.Ncap);
      const int k = be->slot_of[b];
      if (k < 0) mo.x0 = be->h_m_x0.data() + (size_t)b * be->MP.s_x0, mo.J = be->h_m_J.data() + (size_t)b * be->MP.s_J,
                 mo.r = be->h_m_r.data() + (size_t)b * be->MP.s_r;
      unpack_prior(mo, *windows[b].next_prior, k < 0);
    }
  });
  // a cooperative window whose workgroups did not meet (solver_core.h, coop_spin): FAILURE, and the call says so
  bool timed_out = false;
  for (int b = 0; b < n; b++)
    if (be->h_stats_i[(size_t)b * s.stats_i + 1] == -9) {
      timed_out = true;
      if (stats) stats[b].termination = 2;
      if (windows[b].next_prior) windows[b].next_prior->n = 0, windows[b].next_prior->n_blocks = 0;
      be->h_m_ints[(size_t)b * be->MP.s_ints] = 0;  // (its slot keeps the previous prior)
    }
  // advance the slots whose window produced a new prior; once per upload (a second download of the same launch, or a
  // re-launch of the same upload, reads and writes the same banks again)
  if (!be->slots_advanced) {
    for (int b = 0; b < n; b++) {
      const int k = be->slot_of[b];
      if (k >= 0 && be->h_m_ints[(size_t)b * be->MP.s_ints] > 0) be->st_bank[k] ^= 1;
    }
    be->slots_advanced = true;
  }
  if (host_timing())
    fprintf(stderr, "vio_backend_download: wait for kernel %.2f ms, D2H %.2f ms, unpack %.2f ms\n", t1 - t0, t2 - t1, now_ms() - t2);
  return timed_out ? VIO_ETIMEOUT : VIO_OK;
} catch (const std::bad_alloc &) {
  return VIO_ENOMEM;
}

int vio_backend_solve_windows(vio_backend_t *be, VioWindow *windows, int32_t n, int32_t buf_num, VioSolveStats *stats) {
  (void)buf_num;  // wall-clock budget selector in the reference (VINS.cpp:648-653); no time limit here
  return vio_backend_solve_windows_cam(be, windows, n, nullptr, stats);
}

int vio_backend_solve_windows_cam(vio_backend_t *be, VioWindow *windows, int32_t n, const double *sqrt_info, VioSolveStats *stats) {
  const double t0 = now_ms();
  int rc = vio_backend_upload_cam(be, windows, n, sqrt_info);
  if (rc != VIO_OK) return rc;
  const double t1 = now_ms();
  rc = vio_backend_launch(be, nullptr);
  if (rc != VIO_OK) return rc;
  const double t2 = now_ms();
  rc = vio_backend_download(be, windows, n, stats);
  if (host_timing()) fprintf(stderr, "vio_backend_solve_windows: upload %.2f ms, launch call %.2f ms, download %.2f ms\n", t1 - t0, t2 - t1, now_ms() - t2);
  return rc;
}

}  // extern "C"
