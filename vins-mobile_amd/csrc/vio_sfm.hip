// vio_sfm.hip — device launch of the batched bundle adjustment (sfm_core.h): the closing "full BA" of
// GlobalSFM::construct (VINS_ios/inital_sfm.cpp:229-296) for n independent problems, one workgroup each, and the host
// packing around it (sfm_pack.h).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "sfm_core.h"
#include "sfm_launch.h"
#include "sfm_pack.h"
#include "vio_amd.h"
#include "vio_device.h"

using namespace vio;

namespace {

// kLdsPoints: the landmark state in LDS (it fits next to the reduced camera matrix), else in the global slab.
// (Two workgroups per CU: the walks of the reduced matrix wait for memory, the second workgroup's waves fill the gaps.)
template <bool kLdsPoints>
__global__ __launch_bounds__(sfm::kThreads, 2) void sfm_ba_kernel(sfm::Batch B) {
  extern __shared__ __attribute__((aligned(16))) double sfm_smem[];
  const sfm::View v = sfm::view_of(B, blockIdx.x);
  if constexpr (kLdsPoints) {
    sfm::Work<ldsd> w;
    sfm::carve<ldsd>(B.Fm, (ldsd)sfm_smem, nullptr, B.Pm, &w);
    sfm::solve(threadIdx.x, v, w);
  } else {
    sfm::Work<double *> w;
    sfm::carve<double *>(B.Fm, (ldsd)sfm_smem, v.slab, B.Pm, &w);
    sfm::solve(threadIdx.x, v, w);
  }
}

// The large layout (more than sfm::kSmallFrames frames): the packed reduced matrix takes up to 157 KB of LDS, so one
// workgroup per CU, and 512 work-items so that each SIMD still has two waves to switch between during the walks.
__global__ __launch_bounds__(sfm::Large::kThreads, 1) void sfm_ba_large_kernel(sfm::Batch B) {
  extern __shared__ __attribute__((aligned(16))) double sfm_smem[];
  const sfm::View v = sfm::view_of(B, blockIdx.x);
  sfm::Work<double *, sfm::Large> w;
  sfm::carve_large(B.Fm, (ldsd)sfm_smem, v, B.Pm, &w);
  sfm::solve(threadIdx.x, v, w);
}

}  // namespace

// The launch of sfm_launch.h in its two steps: the kernel's dynamic LDS limit (a host call, kept out of the timed interval),
// then one workgroup per problem of B on stream st.
static size_t ba_lds_bytes(const sfm::Batch &B, bool large, bool in_lds) {
  return large ? sfm::large_lds_bytes(B.Fm) : sfm::lds_bytes(B.Fm, in_lds ? B.Pm : 0);
}
int vio::sfm::prepare_ba(const sfm::Batch &B, bool large, bool in_lds) {
  const void *fn = large ? (const void *)sfm_ba_large_kernel : in_lds ? (const void *)sfm_ba_kernel<true> : (const void *)sfm_ba_kernel<false>;
  HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ba_lds_bytes(B, large, in_lds)));
  return VIO_OK;
}
int vio::sfm::launch_ba(const sfm::Batch &B, bool large, bool in_lds, hipStream_t st) {
  const size_t lds = ba_lds_bytes(B, large, in_lds);
  if (large) hipLaunchKernelGGL(sfm_ba_large_kernel, dim3(B.n), dim3(sfm::Large::kThreads), lds, st, B);
  else if (in_lds) hipLaunchKernelGGL(sfm_ba_kernel<true>, dim3(B.n), dim3(sfm::kThreads), lds, st, B);
  else hipLaunchKernelGGL(sfm_ba_kernel<false>, dim3(B.n), dim3(sfm::kThreads), lds, st, B);
  return VIO_OK;
}

struct vio_init_ba {
  int device = -1;
  int max_batch = 0, max_frames = 0, max_points = 0, max_obs = 0;
  hipStream_t stream = nullptr;
  vio::LaunchTimer timer;
  vio::DevBuf<int> d_ints, d_stats_i;
  vio::DevBuf<double> d_in, d_out, d_ob, d_slab, d_hcc, d_stats_d;
  ~vio_init_ba() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

extern "C" {

int vio_init_ba_create(int32_t max_batch, int32_t max_frames, int32_t max_points, int32_t max_obs, vio_init_ba_t **out) {
  if (!out || max_batch < 1 || max_frames < 2 || max_points < 0 || max_obs < 0) return VIO_EINVAL;
  if (!vio::device_ready("the batched bundle adjustment")) return VIO_ENODEV;
  if (max_frames > VIO_INIT_BA_MAX_FRAMES) return VIO_ECAP;
  vio_init_ba *c = new (std::nothrow) vio_init_ba();
  if (!c) return VIO_ENOMEM;
  c->device = vio::current_device();
  c->max_batch = max_batch, c->max_frames = max_frames, c->max_points = max_points, c->max_obs = max_obs;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return VIO_ENODEV;
  }
  *out = c;
  return VIO_OK;
}

void vio_init_ba_destroy(vio_init_ba_t *c) {
  if (!c) return;
  vio::DeviceScope scope(c->device);
  delete c;
}

int vio_init_ba_get_device(const vio_init_ba_t *c, int32_t *device) {
  if (!c || !device) return VIO_EINVAL;
  *device = c->device;
  return VIO_OK;
}

// One launch: n problems of one layout (large: every one has more than sfm::kSmallFrames frames), packed, solved and
// written back to pr[]. The stream is idle again when it returns.
static int solve_group(vio_init_ba *c, VioInitBaProblem *pr, const sfm::Shape *sh, int n, bool large, VioSolveStats *stats) {
  sfm::HostBatch hb;
  sfm::pack(pr, sh, n, hb);
  const size_t N = n, out_doubles = sfm::dbl_stride(hb.Fm, hb.Pm, 0) * N;
  const bool in_lds = !large && sfm::points_fit_lds(hb.Fm, hb.Pm);
  if (c->d_ints.ensure(hb.ints.size()) != VIO_OK || c->d_in.ensure(hb.in.size()) != VIO_OK || c->d_out.ensure(out_doubles) != VIO_OK ||
      c->d_ob.ensure(N * sfm::kObsDoubles * hb.Om) != VIO_OK || (!in_lds && c->d_slab.ensure(N * sfm::kPointDoubles * hb.Pm) != VIO_OK) ||
      (large && c->d_hcc.ensure(N * 36 * hb.Fm) != VIO_OK) || c->d_stats_d.ensure(N * kStatsDoubles) != VIO_OK ||
      c->d_stats_i.ensure(N * kStatsInts) != VIO_OK)
    return VIO_ENOMEM;
  hipStream_t st = c->stream;
  HIP_OK(hipMemcpyAsync(c->d_ints.p, hb.ints.data(), hb.ints.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(c->d_in.p, hb.in.data(), hb.in.size() * sizeof(double), hipMemcpyHostToDevice, st));
  sfm::Batch B;
  B.n = n, B.Fm = hb.Fm, B.Pm = hb.Pm, B.Om = hb.Om;
  B.ints = c->d_ints.p, B.in = c->d_in.p, B.out = c->d_out.p, B.ob = c->d_ob.p, B.slab = in_lds ? nullptr : c->d_slab.p;
  B.stats_d = c->d_stats_d.p, B.stats_i = c->d_stats_i.p, B.hcc = large ? c->d_hcc.p : nullptr;
  int rc = sfm::prepare_ba(B, large, in_lds);
  if (rc != VIO_OK) return rc;
  if ((rc = c->timer.begin(st)) != VIO_OK) return rc;
  if ((rc = sfm::launch_ba(B, large, in_lds, st)) != VIO_OK) return rc;
  if ((rc = c->timer.end(st)) != VIO_OK) return rc;
  HIP_OK(hipGetLastError());
  std::vector<double> out(out_doubles), sd(N * kStatsDoubles);
  std::vector<int> si(N * kStatsInts);
  HIP_OK(hipMemcpyAsync(out.data(), c->d_out.p, out.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(sd.data(), c->d_stats_d.p, sd.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(si.data(), c->d_stats_i.p, si.size() * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipGetLastError());
  for (int b = 0; b < n; b++) {
    VioSolveStats s;
    unpack_solve_stats(&sd[(size_t)b * kStatsDoubles], &si[(size_t)b * kStatsInts], &s);
    sfm::unpack(hb, b, out.data(), s, pr[b]);
    if (stats) stats[b] = s;
  }
  return VIO_OK;
}

int vio_init_ba_solve(vio_init_ba_t *c, VioInitBaProblem *problems, int32_t n, VioSolveStats *stats) {
  if (!c || n < 0 || (n > 0 && !problems)) return VIO_EINVAL;
  if (n == 0) return VIO_OK;
  std::vector<sfm::Shape> sh(n);
  int n_large = 0;
  for (int b = 0; b < n; b++) {  // every problem is checked before anything is written or uploaded
    const int rc = sfm::check_problem(problems[b], &sh[b]);
    if (rc != VIO_OK) return rc;
    if (sh[b].F > c->max_frames || sh[b].np > c->max_points || sh[b].nobs > c->max_obs) return VIO_ECAP;
    n_large += sh[b].F > sfm::kSmallFrames;
  }
  if (n > c->max_batch) return VIO_ECAP;
  VIO_ON_DEVICE_OF(c);
  // The layout follows the problem's own frame count: one launch when all share it, else the small ones, then the large ones.
  if (n_large == 0 || n_large == n) return solve_group(c, problems, sh.data(), n, n_large != 0, stats);
  for (int large = 0; large < 2; large++) {
    std::vector<VioInitBaProblem> pr;
    std::vector<sfm::Shape> gs;
    std::vector<int> slot;
    for (int b = 0; b < n; b++)
      if ((sh[b].F > sfm::kSmallFrames) == (large != 0)) pr.push_back(problems[b]), gs.push_back(sh[b]), slot.push_back(b);
    std::vector<VioSolveStats> gst(stats ? pr.size() : 0);
    const int rc = solve_group(c, pr.data(), gs.data(), (int)pr.size(), large != 0, stats ? gst.data() : nullptr);
    if (rc != VIO_OK) return rc;
    for (size_t g = 0; g < pr.size(); g++) {
      problems[slot[g]].ok = pr[g].ok;  // (the arrays were written through the problem's own pointers)
      if (stats) stats[slot[g]] = gst[g];
    }
  }
  return VIO_OK;
}

int vio_init_ba_kernel_ms(vio_init_ba_t *c, double *ms_avg, int32_t *launches) {
  if (!c || !ms_avg || !launches) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(c);
  return c->timer.drain(ms_avg, launches);  // (every solve waited for its stream: the events have completed)
}

}  // extern "C"
