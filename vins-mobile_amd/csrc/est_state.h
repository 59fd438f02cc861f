// est_state.h — part of vio_estimator.cpp: the estimator's state and the steps that touch nothing else. Restates the members of
// class VINS (VINS.hpp:47-200) and RetriveData (:28-45), clearState (VINS.cpp:36-81), IntegrationBase::repropagate, slideWindow /
// slideWindowOld / slideWindowNew (:1149-1273), vector2double (:89-129) and the last_R / last_P bookkeeping (:431-434, 472-475).
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <new>
#include <vector>

#include "vio_amd.h"
#include "vio_camera.h"
#include "vio_env.h"
#include "vio_resident.h"
#include "vio_math.h"
#include "vio_initial.h"
#include "vio_pool.h"
#include "vio_preint.h"

using namespace vio;

namespace est {  // (named: struct vio_estimator, which the C ABI declares, has members of these types)

struct Relocalization {  // RetriveData (VINS.hpp:28-45), the fields the solve reads and writes
  double header = -1;
  double P_old[3] = {0, 0, 0};
  Quat Q_old{0, 0, 0, 1};
  std::vector<int32_t> ids;
  std::vector<double> xy;
  double loop_pose[7] = {0, 0, 0, 0, 0, 0, 1};
  double relative_t[3] = {0, 0, 0};
  Quat relative_q{0, 0, 0, 1};
  double relative_yaw = 0;
};

struct PriorBuf {
  VioPrior p;
  std::vector<double> x0, J, r;
  // resident: only the header lives here, the data stays in the back-end's device store (vio_backend_reserve_priors)
  void init(int cap, bool resident) {
    memset(&p, 0, sizeof(p));
    if (resident) return;
    x0.assign((size_t)VIO_MAX_PRIOR_BLOCKS * 9, 0.0), J.assign((size_t)cap * cap, 0.0), r.assign(cap, 0.0);
    p.block_x0 = x0.data(), p.linearized_jacobians = J.data(), p.linearized_residuals = r.data();
  }
};

struct Sequence {
  int index = 0;  // position in the estimator = slot of the device-resident prior store
  // the sequence's camera (vio_estimator_set_camera): the context's cfg.fx .. cy and creation tic / ric until one is set.
  // Outlives clearState: the reference reads the same per-device globals again there (VINS.cpp:36-81, global_param.cpp:24-131)
  VioCamera cam;
  int frame_count = 0, solver_flag = VIO_SOLVER_INITIAL, marginalization_flag = VIO_MARGIN_OLD;
  bool first_imu = false;
  int failure_occur = 0;
  double acc_0[3] = {0, 0, 0}, gyr_0[3] = {0, 0, 0};
  std::vector<double> Ps, Rs, Vs, Bas, Bgs, Headers;  // [W+1] x {3, 9, 3, 3, 3, 1}
  std::vector<host::Preint> pre;                      // pre_integrations[i]
  std::vector<char> pre_valid;
  std::vector<std::vector<double>> dt_buf, acc_buf, gyr_buf;
  std::vector<double> lin_acc, lin_gyr;  // [W+1][3] IntegrationBase::linearized_acc / linearized_gyr (the first sample)
  vio_features_t *fm = nullptr;
  PriorBuf prior[2];
  int cur_prior = 0;
  bool has_prior = false;
  double last_R[9], last_P[3], last_R_old[9], last_P_old[3];
  double r_drift[9], t_drift[3];
  Relocalization retrive, front;
  bool loop_enable = false;
  double final_cost = 0;
  // solveInitial's bookkeeping: every published frame since the window's oldest one, with the IMU interval that leads
  // to it integrated from zero biases (all_image_frame / tmp_pre_integration, VINS.cpp:402-404)
  std::map<double, init::Frame> all_image_frame;
  init::Frame tmp;           // the interval being integrated
  bool tmp_valid = false;
  double initial_timestamp = 0;
  double g[3] = {0, 0, 0};
  // initial window handed over in place of solveInitial
  bool init_pending = false;
  std::vector<double> init_headers, init_Ps, init_Rs, init_Vs, init_Bas, init_Bgs;
  // scratch of the window being solved
  std::vector<double> pose, sb, inv_depth, raw_pose, raw_sb, pts_i, pts_j;
  std::vector<int32_t> f_host, f_target, f_feat;
  std::vector<VioPreintegration> preint;
  double ex_pose[7], loop_pose[7];
  int loop_frame = -1, n_loop_factors = 0;
  int last_track_num = 0;
  // device-resident path (vio_resident.h): the landmark list, the pre-integration blocks and the prior of this sequence live
  // in its slot of the group's back-end; `fm` is empty meanwhile
  bool on_device = false;
  std::vector<char> pre_dirty;  // [W+1] pre[i] changed since the device last saw it
  // IMU samples integrated on the device (resident_imu): pre[i] keeps its header (linearization biases, first sample) and
  // the sample buffers, its Jacobian / covariance are not propagated on the host (pre_stale) until the sequence returns to
  // the host-side list; pre_merge[i]: trailing samples of interval i that the device has not seen yet (non-keyframe slide)
  std::vector<char> pre_stale;
  std::vector<int> pre_merge;
};

// solve_initial between its host halves: what relativePose and GlobalSFM::construct have produced when the bundle adjustment
// starts, and that bundle adjustment's arguments in the layout of vio_init_ba_solve.
struct InitStage {
  int l = -1;
  std::vector<init::SfmFeature> sfm_f;
  std::vector<double> cq, tc;  // [P][4] w x y z, [P][3]: world -> camera, in/out of the bundle adjustment
  std::vector<double> points, xy;
  std::vector<uint8_t> ok;
  std::vector<int32_t> start, frame;
  int n_ok = 0;
  int device_rc = VIO_OK, verdict = 0;  // of the device call: its return, and the problem's ok (level 1) / status (level 2)
  // vio_estimator_set_init_device(est, 2): the rest of a VioInitSfmProblem and its outputs
  int mode = 0;
  double relative_R[9], relative_T[3], hint[9];
  std::vector<int32_t> ex_guess, ex_start, ex_feature;
  std::vector<double> ex_xy, ex_R, ex_T, q, T;
};

const double kI3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

}  // namespace est
using namespace est;

struct vio_estimator {
  VioConfig cfg;
  int W = 10, n_seq = 0;
  double tic[3], ric[9];  // of the context: what a sequence without a camera of its own uses
  bool any_camera = false;  // some sequence has been given a camera (vio_estimator_set_camera): the back ends are told per slot / window
  std::vector<Sequence> seq;
  // Created at the first solve: IMU propagation and window filling need no device. The sequences are split into
  // n_groups contiguous groups with one back-end context (own stream, own resident batch, own prior store) each: while
  // the kernel of group g runs, the host packs group g + 1 and unpacks group g - 1. The window kernel occupies one CU
  // per window, so n_groups launches of n_seq / n_groups windows run side by side on the device.
  static constexpr int kMaxGroups = 8;
  vio_backend_t *be[kMaxGroups] = {nullptr};
  int n_groups = 1, group_size = 1;
  std::vector<VioWindow> windows;
  std::vector<VioSolveStats> stats;
  bool enable_init = false;
  bool init_relpose_fit = false;  // relativePose by the all-correspondence fit instead of the reference's five-point RANSAC
  // the marginalization prior of every sequence stays in device memory between launches; only its header comes back
  // (VIO_AMD_HOST_PRIORS=1: carry it through host memory instead, ~45 KB per sequence and direction)
  bool resident_priors = !vio::env_flag("VIO_AMD_HOST_PRIORS");
  // Sequences in the NON_LINEAR state keep their landmark list on the device and have their windows assembled there
  // (on by default; vio_estimator_set_resident / VIO_AMD_RESIDENT=0 turn it off); needs the device-resident priors.
  bool resident = !vio::env_flag("VIO_AMD_RESIDENT", '0');
  int res_list_cap = 0, res_obs_cap = 0;
  // VIO_AMD_RESIDENT_IMU=1: the IMU samples of their intervals travel instead of the integrated blocks and a kernel integrates
  // them (preint_core.h: the host's bits). Off by default: measured at 512 sequences the kernel takes what the host pool saves
  // (124 us against ~120 us of host::propagate on 16 AVX2 threads) and sits on the frame's critical path.
  bool resident_imu = vio::env_flag("VIO_AMD_RESIDENT_IMU");
  std::vector<int> res_rc;  // per sequence: outcome of staging in the current call
  std::vector<int> solving;  // sequences of the current launch
  std::vector<VioWindow> staged;   // per sequence, built in parallel, compacted into `windows`
  std::vector<char> wants_solve;
  double ms_pre = 0, ms_solve = 0, ms_post = 0;  // wall time of the last process_images call, by phase
  // vio_estimator_set_init_device: the bundle adjustment of solveInitial for every sequence that reaches it in one call goes to
  // the device in one launch (vio_init_ba_solve); the context exists from the first such call on
  // (level 2: the relative pose fit, construct and the PnP of the in-between frames as well, in one vio_init_sfm_solve)
  int init_device = 0;
  vio_init_ba_t *init_ba = nullptr;
  vio_init_sfm_t *init_sfm = nullptr;
  std::vector<InitStage> init_stage;     // per sequence: solve_initial between its two host halves
  std::vector<char> init_wait;           // per sequence: its start-up is part of this call's vio_init_ba_solve / vio_init_sfm_solve
  std::vector<int> init_device_count;    // per sequence: initialisations whose bundle adjustment ran on the device
};

namespace {
void clear_state(vio_estimator *e, Sequence &s) {  // VINS::clearState (VINS.cpp:36-81)
  const int P = e->W + 1;
  for (int i = 0; i < P; i++) {
    memcpy(&s.Rs[9 * i], kI3, sizeof(kI3));
    for (int k = 0; k < 3; k++) s.Ps[3 * i + k] = s.Vs[3 * i + k] = s.Bas[3 * i + k] = s.Bgs[3 * i + k] = 0;
    s.pre_valid[i] = 0;
    s.dt_buf[i].clear(), s.acc_buf[i].clear(), s.gyr_buf[i].clear();
  }
  s.frame_count = 0;
  s.first_imu = false;
  s.solver_flag = VIO_SOLVER_INITIAL;
  s.has_prior = false;
  s.init_pending = false;
  s.all_image_frame.clear();
  s.tmp_valid = false;
  s.initial_timestamp = 0;
  s.on_device = false;
  std::fill(s.pre_stale.begin(), s.pre_stale.end(), 0), std::fill(s.pre_merge.begin(), s.pre_merge.end(), 0);
  vio_features_clear(s.fm);
}
void restart_with_error(vio_estimator *e, Sequence &s, VioFrameResult &res, int rc) {  // ... and the frame says why
  clear_state(e, s);
  res.action = VIO_FRAME_ERROR, res.error = rc;
}

void new_preintegration(vio_estimator *e, Sequence &s, int i) {
  host::preint_init(s.pre[i], &e->cfg, s.acc_0, s.gyr_0, &s.Bas[3 * i], &s.Bgs[3 * i]);
  memcpy(&s.lin_acc[3 * i], s.acc_0, 24), memcpy(&s.lin_gyr[3 * i], s.gyr_0, 24);
  s.pre_valid[i] = 1;
  s.pre_stale[i] = 0, s.pre_merge[i] = 0;
}

// IntegrationBase::repropagate (integration_base.h:47-61): the same samples again from new linearization biases
void repropagate(vio_estimator *e, Sequence &s, int i, const double ba[3], const double bg[3]) {
  if (!s.pre_valid[i]) return;
  host::preint_init(s.pre[i], &e->cfg, &s.lin_acc[3 * i], &s.lin_gyr[3 * i], ba, bg);
  for (size_t k = 0; k < s.dt_buf[i].size(); k++)
    host::propagate(s.pre[i], s.dt_buf[i][k], &s.acc_buf[i][3 * k], &s.gyr_buf[i][3 * k]);
}

// slideWindow (VINS.cpp:1149-1237) + slideWindowOld / slideWindowNew (:1239-1273)
void slide_window(vio_estimator *e, Sequence &s) {
  const int W = e->W;
  if (s.frame_count != W) return;
  if (s.marginalization_flag == VIO_MARGIN_OLD) {
    double back_R0[9], back_P0[3];
    memcpy(back_R0, &s.Rs[0], sizeof(back_R0)), memcpy(back_P0, &s.Ps[0], sizeof(back_P0));
    for (int i = 0; i < W; i++) {
      for (int k = 0; k < 9; k++) std::swap(s.Rs[9 * i + k], s.Rs[9 * (i + 1) + k]);
      std::swap(s.pre[i], s.pre[i + 1]), std::swap(s.pre_valid[i], s.pre_valid[i + 1]);
      std::swap(s.pre_stale[i], s.pre_stale[i + 1]), std::swap(s.pre_merge[i], s.pre_merge[i + 1]);
      s.dt_buf[i].swap(s.dt_buf[i + 1]), s.acc_buf[i].swap(s.acc_buf[i + 1]), s.gyr_buf[i].swap(s.gyr_buf[i + 1]);
      for (int k = 0; k < 3; k++)
        std::swap(s.lin_acc[3 * i + k], s.lin_acc[3 * (i + 1) + k]), std::swap(s.lin_gyr[3 * i + k], s.lin_gyr[3 * (i + 1) + k]);
      s.Headers[i] = s.Headers[i + 1];
      for (int k = 0; k < 3; k++)
        std::swap(s.Ps[3 * i + k], s.Ps[3 * (i + 1) + k]), std::swap(s.Vs[3 * i + k], s.Vs[3 * (i + 1) + k]);
    }
    // (Bas / Bgs are not rotated by the reference's loop: only the newest slot is overwritten below — restated as is;
    // the solve rewrites all of them from para_SpeedBias every frame)
    s.Headers[W] = s.Headers[W - 1];
    memcpy(&s.Rs[9 * W], &s.Rs[9 * (W - 1)], 72);
    for (int k = 0; k < 3; k++) {
      s.Ps[3 * W + k] = s.Ps[3 * (W - 1) + k], s.Vs[3 * W + k] = s.Vs[3 * (W - 1) + k];
      s.Bas[3 * W + k] = s.Bas[3 * (W - 1) + k], s.Bgs[3 * W + k] = s.Bgs[3 * (W - 1) + k];
    }
    new_preintegration(e, s, W);
    s.dt_buf[W].clear(), s.acc_buf[W].clear(), s.gyr_buf[W].clear();
    if (s.solver_flag == VIO_SOLVER_INITIAL)  // frames older than the new oldest one leave all_image_frame (VINS.cpp:1190-1197)
      s.all_image_frame.erase(s.all_image_frame.begin(), s.all_image_frame.lower_bound(s.Headers[0]));
    // slideWindowOld: the landmarks hosted in the departed frame move to the next one (store_finish did it on the device
    // for a resident sequence, together with the shift of the pre-integration blocks)
    if (!s.on_device && s.solver_flag == VIO_SOLVER_NON_LINEAR) {
      double R0[9], R1[9], P0[3], P1[3], t[3];
      mat3mul(back_R0, s.cam.ric, R0), mat3mul(&s.Rs[0], s.cam.ric, R1);
      mat3vec(back_R0, s.cam.tic, t);
      for (int k = 0; k < 3; k++) P0[k] = back_P0[k] + t[k];
      mat3vec(&s.Rs[0], s.cam.tic, t);
      for (int k = 0; k < 3; k++) P1[k] = s.Ps[k] + t[k];
      vio_features_remove_back_shift_depth(s.fm, R0, P0, R1, P1);
    } else if (!s.on_device) {
      vio_features_remove_back(s.fm);
    }
  } else {
    // the second-newest frame leaves; its IMU samples extend the interval of the frame before it
    const int fc = s.frame_count;
    const bool dev_imu = s.on_device && e->resident_imu;
    if (dev_imu) s.pre_stale[fc - 1] = 1, s.pre_merge[fc - 1] += (int)s.dt_buf[fc].size();
    for (size_t i = 0; i < s.dt_buf[fc].size(); i++) {
      const double dt = s.dt_buf[fc][i];
      if (s.pre_valid[fc - 1] && !dev_imu) host::propagate(s.pre[fc - 1], dt, &s.acc_buf[fc][3 * i], &s.gyr_buf[fc][3 * i]);
      s.dt_buf[fc - 1].push_back(dt);
      for (int k = 0; k < 3; k++)
        s.acc_buf[fc - 1].push_back(s.acc_buf[fc][3 * i + k]), s.gyr_buf[fc - 1].push_back(s.gyr_buf[fc][3 * i + k]);
    }
    s.Headers[fc - 1] = s.Headers[fc];
    memcpy(&s.Rs[9 * (fc - 1)], &s.Rs[9 * fc], 72);
    for (int k = 0; k < 3; k++) {
      s.Ps[3 * (fc - 1) + k] = s.Ps[3 * fc + k], s.Vs[3 * (fc - 1) + k] = s.Vs[3 * fc + k];
      s.Bas[3 * (fc - 1) + k] = s.Bas[3 * fc + k], s.Bgs[3 * (fc - 1) + k] = s.Bgs[3 * fc + k];
    }
    new_preintegration(e, s, W);
    s.dt_buf[W].clear(), s.acc_buf[W].clear(), s.gyr_buf[W].clear();
    if (s.on_device) s.pre_dirty[fc - 1] = 1;  // the interval that took over the departed frame's samples
    else vio_features_remove_front(s.fm, s.frame_count);
  }
}

// para_Pose / para_SpeedBias of the window (vector2double, VINS.cpp:89-129) into s.pose / s.sb.
void fill_pose_arrays(vio_estimator *e, Sequence &s) {
  const int P = e->W + 1;
  for (int i = 0; i < P; i++) {
    const Quat q = RtoQ(&s.Rs[9 * i]);
    double *p = &s.pose[7 * i], *b = &s.sb[9 * i];
    p[0] = s.Ps[3 * i], p[1] = s.Ps[3 * i + 1], p[2] = s.Ps[3 * i + 2], p[3] = q.x, p[4] = q.y, p[5] = q.z, p[6] = q.w;
    for (int k = 0; k < 3; k++) b[k] = s.Vs[3 * i + k], b[3 + k] = s.Bas[3 * i + k], b[6 + k] = s.Bgs[3 * i + k];
  }
}

void remember_last(vio_estimator *e, Sequence &s) {  // VINS.cpp:431-434, 472-475
  const int W = e->W;
  memcpy(s.last_R, &s.Rs[9 * W], 72), memcpy(s.last_P, &s.Ps[3 * W], 24);
  memcpy(s.last_R_old, &s.Rs[0], 72), memcpy(s.last_P_old, &s.Ps[0], 24);
}
}  // namespace
