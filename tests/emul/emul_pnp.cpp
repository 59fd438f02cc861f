// tests/emul/emul_pnp.cpp — TEST-ONLY host emulation of the PnP window kernel: compiles vins-mobile_amd/csrc/pnp_core.h
// with -DVIO_EMUL (one "thread", no barriers). Not part of the product library, not a CPU fallback.
#include <string.h>

#include <limits>
#include <vector>

#include "vio_amd.h"
#include "pnp_core.h"

using namespace vio;

extern "C" int emul_pnp_solve(const VioConfig *cfg, VioPnpWindow *win, VioSolveStats *stats) {
  const int n = win->n_frames, M = win->feat_start[n];
  const double kNaN = std::numeric_limits<double>::quiet_NaN();
  std::vector<int> fixed(n), si(kStatsInts, 0);
  for (int k = 0; k < n; k++) fixed[k] = win->fixed[k] ? 1 : 0;
  std::vector<double> out_pose(7 * n, kNaN), out_speed(3 * n, kNaN), sd(kStatsDoubles, 0.0), Jraw(450 * (n - 1), kNaN);
  pnp::View v;
  v.n = n, v.M = M, v.max_iter = 5;
  v.fixed = fixed.data(), v.feat_start = win->feat_start;
  v.pose0 = win->pose, v.speed0 = win->speed, v.bias = win->bias, v.ex = win->ex_pose;
  v.preint = reinterpret_cast<const double *>(win->preint);
  v.obs = win->observation, v.pos = win->position, v.track = win->track_num;
  v.out_pose = out_pose.data(), v.out_speed = out_speed.data(), v.stats_d = sd.data(), v.stats_i = si.data();
  v.Jraw = Jraw.data();
  v.s_info = cfg->fx / 1.5, v.gravity = cfg->gravity, v.cauchy_b = cfg->cauchy_a * cfg->cauchy_a;
  Ctx cx;
  cx.tid = 0, cx.nt = 1, cx.prof = nullptr, cx.lprof = nullptr;
  std::vector<double> work(pnp::carve<double *>(n, 64, nullptr, nullptr, nullptr) / sizeof(double) + 8, kNaN);
  pnp::Work<double *> w;
  pnp::carve<double *>(n, 64, work.data(), &w, &cx);
  pnp::solve(cx, v, w);
  for (int i = 0; i < 7 * n; i++) win->pose[i] = out_pose[i];
  for (int i = 0; i < 3 * n; i++) win->speed[i] = out_speed[i];
  if (stats) unpack_solve_stats(sd.data(), si.data(), stats);
  return VIO_OK;
}
