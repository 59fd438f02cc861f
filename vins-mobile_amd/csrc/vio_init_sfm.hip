// vio_init_sfm.hip — device launch of estimator start-up around its bundle adjustment (init_core.h): relativePose's fit
// (VINS_ios/motion_estimator.cpp:200-236), GlobalSFM::construct (inital_sfm.cpp:117-316) and the PnP of the frames outside
// the window (VINS.cpp:926-1003) for n independent problems: head kernel, the bundle adjustment kernels of vio_sfm.hip,
// tail kernel on one stream between one upload and one download, and the host packing around them (init_sfm_pack.h).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "init_core.h"
#include "init_sfm_pack.h"
#include "sfm_launch.h"
#include "vio_amd.h"
#include "vio_device.h"

using namespace vio;

namespace {

// One workgroup per problem; six waves, one per start of the fit. (The serial walks keep one work-item per sum busy: a
// second workgroup on the CU fills the gaps, and the registers of 384 work-items leave room for it.)
__global__ __launch_bounds__(isfm::kHeadThreads) void init_head_kernel(sfm::Batch B, isfm::HeadBatch HB) {
  __shared__ __attribute__((aligned(16))) double head_smem[isfm::kHeadLdsDoubles];
  isfm::head(threadIdx.x, B, HB, blockIdx.x, (ldsd)head_smem);
}

// One workgroup per (problem, extra frame), and one per problem for construct's inversion.
__global__ __launch_bounds__(isfm::kTailThreads) void init_tail_kernel(sfm::Batch B, isfm::TailBatch TB) {
  __shared__ __attribute__((aligned(16))) double tail_smem[isfm::kTailLdsDoubles];
  isfm::tail(threadIdx.x, B, TB, blockIdx.x, (ldsd)tail_smem);
}

}  // namespace

struct vio_init_sfm {
  int device = -1;
  int max_batch = 0, max_frames = 0, max_points = 0, max_obs = 0, max_extra = 0;
  hipStream_t stream = nullptr;
  vio::LaunchTimer timer[3];
  vio::DevBuf<int> d_ints, d_oi, d_hscri, d_tscri;
  vio::DevBuf<double> d_dbl, d_od, d_ob, d_slab, d_hcc, d_hscr, d_tscr;
  // the last solve, for vio_init_sfm_head_state: per problem the offset of its cq | ct | X in d_dbl (-1: head failed), the
  // strides of its group and which landmarks it packed
  struct Last {
    long off = -1;
    int F = 0, Fm = 0;
    std::vector<uint8_t> ok;
  };
  std::vector<Last> last;
  ~vio_init_sfm() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

extern "C" {

int vio_init_sfm_create(int32_t max_batch, int32_t max_frames, int32_t max_points, int32_t max_obs, int32_t max_extra,
                        vio_init_sfm_t **out) {
  if (!out || max_batch < 1 || max_frames < 2 || max_points < 0 || max_obs < 0 || max_extra < 0) return VIO_EINVAL;
  if (!vio::device_ready("the start-up structure from motion")) return VIO_ENODEV;
  if (max_frames > VIO_INIT_BA_MAX_FRAMES) return VIO_ECAP;
  vio_init_sfm_t *c = new (std::nothrow) vio_init_sfm_t();
  if (!c) return VIO_ENOMEM;
  c->device = vio::current_device();
  c->max_batch = max_batch, c->max_frames = max_frames, c->max_points = max_points, c->max_obs = max_obs, c->max_extra = max_extra;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return VIO_ENODEV;
  }
  *out = c;
  return VIO_OK;
}

void vio_init_sfm_destroy(vio_init_sfm_t *c) {
  if (!c) return;
  vio::DeviceScope scope(c->device);
  delete c;
}

int vio_init_sfm_get_device(const vio_init_sfm_t *c, int32_t *device) {
  if (!c || !device) return VIO_EINVAL;
  *device = c->device;
  return VIO_OK;
}

// One group: n problems of one bundle adjustment layout through the three stages. slot[b]: the problem's place in the call.
static int solve_group(vio_init_sfm_t *c, VioInitSfmProblem *pr, const isfm::Shape *sh, const int *slot, int n, bool large,
                       VioSolveStats *stats) {
  isfm::HostInit h;
  isfm::pack(pr, sh, n, h);
  const sfm::HostBatch &hb = h.hb;
  const isfm::OutLayout L = isfm::out_layout(h);
  const size_t N = n;
  const bool in_lds = !large && sfm::points_fit_lds(hb.Fm, hb.Pm);
  // one array of ints and one of doubles up ...
  std::vector<int> ints(hb.ints);
  const size_t i_hint = ints.size();
  ints.insert(ints.end(), h.hint.begin(), h.hint.end());
  const size_t i_units = ints.size();
  ints.insert(ints.end(), h.units.begin(), h.units.end());
  const size_t i_point = ints.size();
  ints.insert(ints.end(), h.ex_point.begin(), h.ex_point.end());
  const size_t i_guess = ints.size();
  ints.insert(ints.end(), h.guess.begin(), h.guess.end());
  std::vector<double> dbl(hb.in);
  const size_t d_hin = dbl.size();
  dbl.insert(dbl.end(), h.hin.begin(), h.hin.end());
  const size_t d_exy = dbl.size();
  dbl.insert(dbl.end(), h.ex_xy.begin(), h.ex_xy.end());
  if (c->d_ints.ensure(ints.size()) != VIO_OK || c->d_dbl.ensure(dbl.size()) != VIO_OK || c->d_od.ensure(L.d_total) != VIO_OK ||
      c->d_oi.ensure(L.i_total) != VIO_OK || c->d_ob.ensure(N * sfm::kObsDoubles * hb.Om) != VIO_OK ||
      (!in_lds && c->d_slab.ensure(N * sfm::kPointDoubles * hb.Pm) != VIO_OK) || (large && c->d_hcc.ensure(N * 36 * hb.Fm) != VIO_OK) ||
      c->d_hscr.ensure(N * isfm::head_scratch_doubles(h.Cm, hb.Pm)) != VIO_OK ||
      c->d_hscri.ensure(N * isfm::head_scratch_ints(h.Cm, hb.Pm)) != VIO_OK ||
      c->d_tscr.ensure((size_t)h.U * isfm::kPnpRows * h.Em) != VIO_OK || c->d_tscri.ensure((size_t)h.U * h.Em) != VIO_OK)
    return VIO_ENOMEM;
  hipStream_t st = c->stream;
  HIP_OK(hipMemcpyAsync(c->d_ints.p, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(c->d_dbl.p, dbl.data(), dbl.size() * sizeof(double), hipMemcpyHostToDevice, st));
  sfm::Batch B;
  B.n = n, B.Fm = hb.Fm, B.Pm = hb.Pm, B.Om = hb.Om;
  B.ints = c->d_ints.p, B.in = c->d_dbl.p, B.out = c->d_od.p + L.d_out, B.ob = c->d_ob.p, B.slab = in_lds ? nullptr : c->d_slab.p;
  B.stats_d = c->d_od.p + L.d_sd, B.stats_i = c->d_oi.p + L.i_si, B.hcc = large ? c->d_hcc.p : nullptr;
  isfm::HeadBatch HB;
  HB.n = n, HB.Cm = h.Cm, HB.hint = c->d_ints.p + i_hint, HB.hin = c->d_dbl.p + d_hin, HB.status = c->d_oi.p + L.i_status;
  HB.rel = c->d_od.p + L.d_rel, HB.scr_d = c->d_hscr.p, HB.scr_i = c->d_hscri.p;
  isfm::TailBatch TB;
  TB.U = h.U, TB.Em = h.Em, TB.units = c->d_ints.p + i_units, TB.ex_point = c->d_ints.p + i_point, TB.guess = c->d_ints.p + i_guess;
  TB.ex_xy = c->d_dbl.p + d_exy, TB.head_status = c->d_oi.p + L.i_status, TB.qT = c->d_od.p + L.d_qT, TB.ex_out = c->d_od.p + L.d_ex;
  TB.scr_d = c->d_tscr.p, TB.ex_flag = c->d_oi.p + L.i_flag, TB.scr_i = c->d_tscri.p, TB.ba_ok = c->d_oi.p + L.i_baok;
  int rc = sfm::prepare_ba(B, large, in_lds);
  if (rc != VIO_OK) return rc;
  if ((rc = c->timer[0].begin(st)) != VIO_OK) return rc;
  hipLaunchKernelGGL(init_head_kernel, dim3(n), dim3(isfm::kHeadThreads), 0, st, B, HB);
  if ((rc = c->timer[0].end(st)) != VIO_OK) return rc;
  HIP_OK(hipGetLastError());
  if ((rc = c->timer[1].begin(st)) != VIO_OK) return rc;
  if ((rc = sfm::launch_ba(B, large, in_lds, st)) != VIO_OK) return rc;
  if ((rc = c->timer[1].end(st)) != VIO_OK) return rc;
  HIP_OK(hipGetLastError());
  if ((rc = c->timer[2].begin(st)) != VIO_OK) return rc;
  hipLaunchKernelGGL(init_tail_kernel, dim3(h.U), dim3(isfm::kTailThreads), 0, st, B, TB);
  if ((rc = c->timer[2].end(st)) != VIO_OK) return rc;
  HIP_OK(hipGetLastError());
  // ... and one of each down
  std::vector<double> od(L.d_total);
  std::vector<int> oi(L.i_total);
  HIP_OK(hipMemcpyAsync(od.data(), c->d_od.p, od.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(oi.data(), c->d_oi.p, oi.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipGetLastError());
  for (int b = 0; b < n; b++) {
    isfm::unpack(h, L, od.data(), oi.data(), b, pr[b], stats ? &stats[b] : nullptr);
    vio_init_sfm_t::Last &l = c->last[slot[b]];
    l.off = oi[L.i_status + 4 * b] == VIO_INIT_SFM_OK ? (long)(sfm::dbl_stride(hb.Fm, hb.Pm, hb.Om) * b) : -1;
    l.F = sh[b].ba.F, l.Fm = hb.Fm, l.ok = h.ok[b];
  }
  return VIO_OK;
}

int vio_init_sfm_solve(vio_init_sfm_t *c, VioInitSfmProblem *problems, int32_t n, VioSolveStats *ba_stats) {
  if (!c || n < 0 || (n > 0 && !problems)) return VIO_EINVAL;
  if (n == 0) return VIO_OK;
  std::vector<isfm::Shape> sh(n);
  int n_large = 0;
  for (int b = 0; b < n; b++) {  // every problem is checked before anything is written or uploaded
    const int rc = isfm::check_problem(problems[b], &sh[b]);
    if (rc != VIO_OK) return rc;
  }
  for (int b = 0; b < n; b++) {
    if (sh[b].ba.F > c->max_frames || sh[b].ba.np > c->max_points || sh[b].ba.nobs > c->max_obs || problems[b].n_extra > c->max_extra)
      return VIO_ECAP;
    n_large += sh[b].ba.F > sfm::kSmallFrames;
  }
  if (n > c->max_batch) return VIO_ECAP;
  VIO_ON_DEVICE_OF(c);
  c->last.assign(n, vio_init_sfm_t::Last());
  // The bundle adjustment's layout follows the problem's own frame count: the problems of up to 16 frames, then the others.
  // (With both present only the last group's head state stays on the device: vio_init_sfm_head_state answers for that group.)
  for (int large = 0; large < 2; large++) {
    if ((large ? n_large : n - n_large) == 0) continue;
    std::vector<VioInitSfmProblem> pr;
    std::vector<isfm::Shape> gs;
    std::vector<int> slot;
    for (int b = 0; b < n; b++)
      if ((sh[b].ba.F > sfm::kSmallFrames) == (large != 0)) pr.push_back(problems[b]), gs.push_back(sh[b]), slot.push_back(b);
    if (large && n_large != n)
      for (int b = 0; b < n; b++)
        if (sh[b].ba.F <= sfm::kSmallFrames) c->last[b].off = -1;
    std::vector<VioSolveStats> gst(ba_stats ? pr.size() : 0);
    const int rc = solve_group(c, pr.data(), gs.data(), slot.data(), (int)pr.size(), large != 0, ba_stats ? gst.data() : nullptr);
    if (rc != VIO_OK) return rc;
    for (size_t g = 0; g < pr.size(); g++) {
      VioInitSfmProblem &d = problems[slot[g]];  // (the arrays were written through the problem's own pointers)
      d.status = pr[g].status, d.inliers = pr[g].inliers;
      memcpy(d.relative_R, pr[g].relative_R, sizeof(d.relative_R)), memcpy(d.relative_T, pr[g].relative_T, sizeof(d.relative_T));
      if (ba_stats) ba_stats[slot[g]] = gst[g];
    }
  }
  return VIO_OK;
}

int vio_init_sfm_kernel_ms(vio_init_sfm_t *c, double ms[3], int32_t *launches) {
  if (!c || !ms || !launches) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(c);
  *launches = 0;
  for (int s = 0; s < 3; s++) {  // (every solve waited for its stream: the events have completed)
    double avg = 0;
    int32_t k = 0;
    const int rc = c->timer[s].drain(&avg, &k);
    if (rc != VIO_OK) return rc;
    ms[s] = avg * k, *launches += k;
  }
  return VIO_OK;
}

int vio_init_sfm_head_state(vio_init_sfm_t *c, int32_t index, double *c_rotation, double *c_translation, double *points) {
  if (!c || !c_rotation || !c_translation || !points) return VIO_EINVAL;
  if (index < 0 || index >= (int)c->last.size() || c->last[index].off < 0) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(c);
  const vio_init_sfm_t::Last &l = c->last[index];
  size_t np = 0;
  for (size_t j = 0; j + 1 < l.ok.size(); j++) np += l.ok[j];
  std::vector<double> s(7 * (size_t)l.Fm + 3 * np);
  HIP_OK(hipMemcpy(s.data(), c->d_dbl.p + l.off, s.size() * sizeof(double), hipMemcpyDeviceToHost));
  memcpy(c_rotation, s.data(), sizeof(double) * 4 * l.F), memcpy(c_translation, s.data() + 4 * l.Fm, sizeof(double) * 3 * l.F);
  size_t p = 0;
  for (size_t j = 0; j + 1 < l.ok.size(); j++)
    if (l.ok[j]) memcpy(points + 3 * j, s.data() + 7 * (size_t)l.Fm + 3 * p++, 24);
  return VIO_OK;
}

}  // extern "C"
