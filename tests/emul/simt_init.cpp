// tests/emul/simt_init.cpp — TEST-ONLY: the three stages of vio_init_sfm_solve executed on the host by the SIMT emulator: the
// head and the tail of vins-mobile_amd/csrc/init_core.h (384 / 128 fibers per workgroup) around the batched bundle adjustment of
// sfm_core.h in both layouts, s_barrier with the hardware's semantics, LDS and every slab poisoned with NaN before each
// workgroup. Checks and packing are the product's (init_sfm_pack.h). Not part of the product library.
#define SIMT_IMPLEMENTATION
#include "simt.h"

#include <limits>
#include <vector>

#include "init_sfm_pack.h"

using namespace vio;

namespace {

std::vector<std::vector<double>> g_head_state;  // per problem of the last call: cq [4F] | ct [3F] | X [3 np], empty: head failed
std::vector<std::vector<uint8_t>> g_head_ok;
std::vector<int> g_sign;  // per problem: the translation sign the cheirality vote took (0: no fit ran)

void run_group(VioInitSfmProblem *pr, const isfm::Shape *sh, const int *slot, int n, bool large, int order, int stages, VioSolveStats *stats) {
  isfm::HostInit h;
  isfm::pack(pr, sh, n, h);
  const sfm::HostBatch &hb = h.hb;
  const isfm::OutLayout L = isfm::out_layout(h);
  const double kNaN = std::numeric_limits<double>::quiet_NaN();
  const bool in_lds = !large && sfm::points_fit_lds(hb.Fm, hb.Pm);
  std::vector<double> od(L.d_total, kNaN), ob((size_t)n * sfm::kObsDoubles * hb.Om, kNaN),
      slab(in_lds ? 1 : (size_t)n * sfm::kPointDoubles * hb.Pm, kNaN), hcc(large ? (size_t)n * 36 * hb.Fm : 1, kNaN),
      hscr(isfm::head_scratch_doubles(h.Cm, hb.Pm) * n, kNaN), tscr((size_t)h.U * isfm::kPnpRows * h.Em, kNaN);
  std::vector<int> oi(L.i_total, -1), hscri(isfm::head_scratch_ints(h.Cm, hb.Pm) * n, -1), tscri((size_t)h.U * h.Em, -1);
  sfm::Batch B;
  B.n = n, B.Fm = hb.Fm, B.Pm = hb.Pm, B.Om = hb.Om;
  B.ints = h.hb.ints.data(), B.in = h.hb.in.data(), B.out = od.data() + L.d_out, B.ob = ob.data(), B.slab = in_lds ? nullptr : slab.data();
  B.stats_d = od.data() + L.d_sd, B.stats_i = oi.data() + L.i_si, B.hcc = large ? hcc.data() : nullptr;
  isfm::HeadBatch HB;
  HB.n = n, HB.Cm = h.Cm, HB.hint = h.hint.data(), HB.hin = h.hin.data(), HB.status = oi.data() + L.i_status, HB.rel = od.data() + L.d_rel;
  HB.scr_d = hscr.data(), HB.scr_i = hscri.data();
  for (int b = 0; b < n; b++) {
    std::vector<double> lds(isfm::kHeadLdsDoubles, kNaN);
    simt::launch(isfm::kHeadThreads, [&](int tid) { isfm::head(tid, B, HB, b, lds.data()); }, order);
  }
  for (int b = 0; b < n; b++) {
    g_head_state[slot[b]].clear(), g_head_ok[slot[b]] = h.ok[b], g_sign[slot[b]] = oi[L.i_status + 4 * b + 2];
    if (oi[L.i_status + 4 * b] != VIO_INIT_SFM_OK) continue;
    const double *in = &h.hb.in[sfm::dbl_stride(hb.Fm, hb.Pm, hb.Om) * b];
    std::vector<double> &s = g_head_state[slot[b]];
    s.insert(s.end(), in, in + 4 * sh[b].ba.F), s.insert(s.end(), in + 4 * hb.Fm, in + 4 * hb.Fm + 3 * sh[b].ba.F);
    s.insert(s.end(), in + 7 * hb.Fm, in + 7 * hb.Fm + 3 * sh[b].ba.np);
  }
  if (stages >= 2)
    for (int b = 0; b < n; b++) {
      const sfm::View v = sfm::view_of(B, b);
      if (large) {
        std::vector<double> lds(sfm::large_lds_bytes(hb.Fm) / sizeof(double) + 2, kNaN);
        simt::launch(sfm::Large::kThreads, [&](int tid) {
          sfm::Work<double *, sfm::Large> w;
          sfm::carve_large(hb.Fm, lds.data(), v, hb.Pm, &w);
          sfm::solve(tid, v, w);
        }, order);
      } else {
        std::vector<double> lds(sfm::lds_bytes(hb.Fm, in_lds ? hb.Pm : 0) / sizeof(double) + 2, kNaN);
        simt::launch(sfm::kThreads, [&](int tid) {
          sfm::Work<double *> w;
          sfm::carve<double *>(hb.Fm, lds.data(), in_lds ? nullptr : v.slab, hb.Pm, &w);
          sfm::solve(tid, v, w);
        }, order);
      }
    }
  else
    for (int b = 0; b < n; b++) oi[L.i_si + (size_t)b * kStatsInts + 1] = 0, od[L.d_sd + (size_t)b * kStatsDoubles + 1] = 1.0;  // (no verdict)
  isfm::TailBatch TB;
  TB.U = h.U, TB.Em = h.Em, TB.units = h.units.data(), TB.ex_point = h.ex_point.data(), TB.guess = h.guess.data(), TB.ex_xy = h.ex_xy.data();
  TB.head_status = oi.data() + L.i_status, TB.qT = od.data() + L.d_qT, TB.ex_out = od.data() + L.d_ex, TB.scr_d = tscr.data();
  TB.ex_flag = oi.data() + L.i_flag, TB.scr_i = tscri.data(), TB.ba_ok = oi.data() + L.i_baok;
  for (int u = 0; u < h.U; u++) {
    std::vector<double> lds(isfm::kTailLdsDoubles, kNaN);
    simt::launch(isfm::kTailThreads, [&](int tid) { isfm::tail(tid, B, TB, u, lds.data()); }, order);
  }
  for (int b = 0; b < n; b++) isfm::unpack(h, L, od.data(), oi.data(), b, pr[b], stats ? &stats[b] : nullptr);
}

}  // namespace

// order: lane order of the emulator (0 forward, 1 reverse, >= 2 seeded shuffle). stages: 1 = the head alone (the bundle
// adjustment is skipped and counts as failed: status _FAIL_BA where the head succeeded), 3 = the whole call.
extern "C" int simt_init_sfm_solve(VioInitSfmProblem *problems, int n, VioSolveStats *stats, int order, int stages) {
  if (n < 0 || (n > 0 && !problems)) return VIO_EINVAL;
  std::vector<isfm::Shape> sh(n);
  for (int b = 0; b < n; b++) {
    const int rc = isfm::check_problem(problems[b], &sh[b]);
    if (rc != VIO_OK) return rc;
  }
  g_head_state.assign(n, std::vector<double>()), g_head_ok.assign(n, std::vector<uint8_t>()), g_sign.assign(n, 0);
  for (int large = 0; large < 2; large++) {
    std::vector<VioInitSfmProblem> pr;
    std::vector<isfm::Shape> gs;
    std::vector<int> slot;
    for (int b = 0; b < n; b++)
      if ((sh[b].ba.F > sfm::kSmallFrames) == (large != 0)) pr.push_back(problems[b]), gs.push_back(sh[b]), slot.push_back(b);
    if (pr.empty()) continue;
    std::vector<VioSolveStats> gst(pr.size());
    run_group(pr.data(), gs.data(), slot.data(), (int)pr.size(), large != 0, order, stages, gst.data());
    for (size_t g = 0; g < pr.size(); g++) {
      VioInitSfmProblem &d = problems[slot[g]];
      d.status = pr[g].status, d.inliers = pr[g].inliers;
      memcpy(d.relative_R, pr[g].relative_R, 72), memcpy(d.relative_T, pr[g].relative_T, 24);
      if (stats) stats[slot[g]] = gst[g];
    }
  }
  return VIO_OK;
}

// What the head of problem `index` of the last call left for the bundle adjustment: c_rotation [F][4], c_translation [F][3],
// points [n_features][3] where the landmark was seen at least twice. VIO_ESTATE when that head failed.
extern "C" int simt_init_head_state(int index, double *cq, double *ct, double *points) {
  if (index < 0 || index >= (int)g_head_state.size() || g_head_state[index].empty()) return VIO_ESTATE;
  const std::vector<double> &s = g_head_state[index];
  const std::vector<uint8_t> &ok = g_head_ok[index];
  size_t np = 0;
  for (size_t j = 0; j + 1 < ok.size(); j++) np += ok[j];
  const size_t F = (s.size() - 3 * np) / 7;
  memcpy(cq, s.data(), 32 * F), memcpy(ct, s.data() + 4 * F, 24 * F);
  size_t p = 0;
  for (size_t j = 0; j + 1 < ok.size(); j++)
    if (ok[j]) memcpy(points + 3 * j, s.data() + 7 * F + 3 * p++, 24);
  return VIO_OK;
}

extern "C" int simt_init_fit_sign(int index) { return index >= 0 && index < (int)g_sign.size() ? g_sign[index] : 0; }
