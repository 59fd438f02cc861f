// est_window.h — part of vio_estimator.cpp: what one call of vio_estimator_process_images is given (FrameCall), and one frame's
// window on its way to the solver and back. Restates the host half of VINS::solve_ceres: old2new (VINS.cpp:89-129), the factor
// list (:528-637), the relocalization frame (:571-596), the loop bookkeeping (:664-680), new2old (:168-189); the end of a solved
// frame in processImage (:455-476); the re-triangulation of visualInitialAlign (:1094-1100).
#pragma once
#include "est_state.h"

namespace {
// The arguments of one vio_estimator_process_images call and what is constant during it. Lives on the caller's stack.
struct FrameCall {
  vio_estimator *e;
  const VioObs *obs;
  const int32_t *n_obs;
  int32_t obs_stride;
  const double *headers;
  const uint8_t *active;
  VioFrameResult *results;
  int ba_max_points, ba_max_obs;  // what the bundle adjustment context takes (vio_init_ba_create): a larger problem stays on the host
  int sfm_max_extra;  // frames of all_image_frame outside the window a vio_init_sfm_solve problem may bring
  // Windows the device route serves. vio_init_ba_* takes up to VIO_INIT_BA_MAX_FRAMES = 32 frames, but the estimator stays at 16:
  // with self-initialisation on, the synthetic replays the tests use never leave VIO_FRAME_INIT_FAILED at WINDOW_SIZE 16 or 20 on
  // EITHER route (seeds 1-8, 80 frames), so there is no solved window of a larger estimator to compare the two routes on.
  static constexpr int kInitDeviceMaxFrames = 16;
  static_assert(kInitDeviceMaxFrames <= VIO_INIT_BA_MAX_FRAMES, "the context's own bound");
  const VioObs *obs_of(int q) const { return obs + (size_t)q * obs_stride; }
};

bool obs_count_ok(int32_t n_obs, int32_t stride) { return n_obs >= 0 && (stride <= 0 || n_obs <= stride); }
// The call's first error: `first` where there is one already, else that of the first VIO_FRAME_ERROR among sequences q0 .. q1.
int first_error_of(const VioFrameResult *results, int q0, int q1, int first) {
  for (int q = q0; q < q1 && first == VIO_OK; q++)
    if (results[q].action == VIO_FRAME_ERROR) first = results[q].error;
  return first;
}
void extrinsic_pose(const double tic[3], const double ric[9], double out7[7]) {  // para_Ex_Pose: tic, then ric as x y z w
  const Quat q = RtoQ(ric);
  out7[0] = tic[0], out7[1] = tic[1], out7[2] = tic[2], out7[3] = q.x, out7[4] = q.y, out7[5] = q.z, out7[6] = q.w;
}

// Relocalization constraint: front_pose follows retrive_pose_data; it enters when its frame is still in the window. The sweep at
// the top of a call that decides which sequences stay resident needs the first half only and calls the whole: the scan reads
// nothing that sweep changes, and build_window or stage_resident_frame run it again before anything reads s.loop_frame.
void select_loop_frame(Sequence &s, int W) {
  if (s.front.header != s.retrive.header) s.front = s.retrive;
  s.loop_frame = -1;
  if (!s.front.ids.empty() && s.front.header >= s.Headers[0])
    for (int i = 0; i < W; i++)
      if (s.front.header == s.Headers[i]) s.loop_frame = i;
}

// visualInitialAlign re-triangulates every landmark with the aligned poses (VINS.cpp:1094-1100): depths to -1, then triangulate
void retriangulate(vio_estimator *e, Sequence &s, const double tic[3]) {
  int nfe = 0;
  vio_features_count(s.fm, &nfe);
  std::vector<double> minus1(nfe > 0 ? nfe : 1, -1.0);
  vio_features_clear_depth(s.fm, minus1.data(), nfe);
  vio_features_triangulate(s.fm, s.Ps.data(), s.Rs.data(), tic, s.cam.ric);
}

// old2new + the factor list + the loop pose: everything solve_ceres hands to the solver (VINS.cpp:89-129, 505-637)
int build_window(vio_estimator *e, Sequence &s, VioWindow *w) {
  const int W = e->W;
  fill_pose_arrays(e, s);
  extrinsic_pose(s.cam.tic, s.cam.ric, s.ex_pose);
  int nf = 0;
  int rc = vio_features_get_depth_vector(s.fm, s.inv_depth.data(), e->cfg.max_features, &nf);
  if (rc != VIO_OK) return rc;
  select_loop_frame(s, W);
  int m = 0, nf2 = 0;
  rc = vio_features_export_factors_loop(s.fm, e->cfg.max_factors, s.loop_frame, s.front.ids.data(), s.front.xy.data(),
                                        (int)s.front.ids.size(), s.f_host.data(), s.f_target.data(), s.f_feat.data(),
                                        s.pts_i.data(), s.pts_j.data(), &m, &nf2, &s.n_loop_factors);
  if (rc != VIO_OK) return rc;
  if (nf2 != nf) return VIO_ESTATE;
  if (s.n_loop_factors > 0) s.loop_enable = true;
  if (s.loop_frame >= 0 && s.n_loop_factors == 0) s.loop_frame = -1;  // a loop pose without factors is a free block
  for (int i = 0; i < W; i++) {
    if (!s.pre_valid[i + 1]) return VIO_ESTATE;
    host::preint_export(s.pre[i + 1], &s.preint[i]);
  }
  memset(w, 0, sizeof(*w));
  w->window_size = W, w->n_features = nf, w->n_factors = m, w->marginalization_flag = s.marginalization_flag;
  w->pose = s.pose.data(), w->speed_bias = s.sb.data(), w->ex_pose = s.ex_pose, w->inv_depth = s.inv_depth.data();
  w->factor_host = s.f_host.data(), w->factor_target = s.f_target.data(), w->factor_feature = s.f_feat.data();
  w->factor_pts_i = s.pts_i.data(), w->factor_pts_j = s.pts_j.data();
  w->preint = s.preint.data();
  w->prior = s.has_prior ? &s.prior[s.cur_prior].p : nullptr;
  w->loop_frame = s.loop_frame, w->loop_pose = s.loop_pose;
  if (s.failure_occur) {  // new2old anchors the window where the failed one stood (VINS.cpp:139-144)
    double ypr[3];
    R2ypr(s.last_R_old, ypr);
    w->use_origin_override = 1, w->origin_yaw_deg = ypr[0];
    memcpy(w->origin_p, s.last_P_old, sizeof(w->origin_p));
  }
  w->raw_pose = s.raw_pose.data(), w->raw_speed_bias = s.raw_sb.data(), w->raw_inv_depth = nullptr;
  w->next_prior = &s.prior[1 - s.cur_prior].p;
  w->resident_prior = e->resident_priors ? s.index % e->group_size + 1 : 0;  // slot in the store of the sequence's group
  return VIO_OK;
}

double normalize_angle(double a) {  // Utility::normalizeAngle, degrees (utility.hpp:171-179)
  const double two_pi = 2.0 * 180;
  if (a > 0) return a - two_pi * floor((a + 180.0) / two_pi);
  return a + two_pi * floor((-a + 180.0) / two_pi);
}

// double2vector of the solved window (the device already applied new2old to the para arrays), the loop bookkeeping
// (VINS.cpp:664-680, 168-189) and the prior hand-over.
void take_solution(vio_estimator *e, Sequence &s, int n_features, const VioPrior *next_prior, const VioSolveStats &st) {
  const int W = e->W, P = W + 1;
  s.final_cost = st.final_cost;
  if (s.loop_frame >= 0) {
    const int i = s.loop_frame;
    const double *rp = &s.raw_pose[7 * i];
    double Rs_i[9], Rs_loop[9], RlT[9], d[3], ypr_i[3], ypr_l[3];
    qtoR(qnormalized(qfrom_pose(rp)), Rs_i);
    qtoR(qnormalized(qfrom_pose(s.loop_pose)), Rs_loop);
    mat3T(Rs_loop, RlT);
    for (int k = 0; k < 3; k++) d[k] = rp[k] - s.loop_pose[k];
    mat3vec(RlT, d, s.front.relative_t);
    double Rrel[9];
    mat3mul(RlT, Rs_i, Rrel);
    s.front.relative_q = RtoQ(Rrel);
    R2ypr(Rs_i, ypr_i), R2ypr(Rs_loop, ypr_l);
    s.front.relative_yaw = normalize_angle(ypr_i[0] - ypr_l[0]);
    memcpy(s.front.loop_pose, s.loop_pose, sizeof(s.loop_pose));
  }
  // the gauge the device applied: rot_diff and origin_P0 of new2old, needed once more for the loop pose
  double origin_ypr[3], origin_P0[3], raw_ypr[3], R00[9], rot_diff[9];
  if (s.failure_occur) {
    R2ypr(s.last_R_old, origin_ypr), memcpy(origin_P0, s.last_P_old, 24);
  } else {
    R2ypr(&s.Rs[0], origin_ypr), memcpy(origin_P0, &s.Ps[0], 24);
  }
  qtoR(qfrom_pose(&s.raw_pose[0]), R00);
  R2ypr(R00, raw_ypr);
  const double yd[3] = {origin_ypr[0] - raw_ypr[0], 0, 0};
  ypr2R(yd, rot_diff);
  for (int i = 0; i < P; i++) {
    const double *p = &s.pose[7 * i], *b = &s.sb[9 * i];
    qtoR(qfrom_pose(p), &s.Rs[9 * i]);
    for (int k = 0; k < 3; k++)
      s.Ps[3 * i + k] = p[k], s.Vs[3 * i + k] = b[k], s.Bas[3 * i + k] = b[3 + k], s.Bgs[3 * i + k] = b[6 + k];
  }
  if (s.loop_enable) {  // drift of the window against the old keyframe (VINS.cpp:168-189)
    s.loop_enable = false;
    if (s.loop_frame >= 0) {
      double Rl[9], Rloop[9], d[3], Pl[3], ypr_old[3], ypr_loop[3], Rold[9];
      qtoR(qnormalized(qfrom_pose(s.loop_pose)), Rl);
      mat3mul(rot_diff, Rl, Rloop);
      for (int k = 0; k < 3; k++) d[k] = s.loop_pose[k] - s.raw_pose[k];
      mat3vec(rot_diff, d, Pl);
      for (int k = 0; k < 3; k++) Pl[k] += origin_P0[k];
      qtoR(s.front.Q_old, Rold);
      R2ypr(Rold, ypr_old), R2ypr(Rloop, ypr_loop);
      const double dy[3] = {ypr_old[0] - ypr_loop[0], 0, 0};
      ypr2R(dy, s.r_drift);
      double t[3];
      mat3vec(s.r_drift, Pl, t);
      for (int k = 0; k < 3; k++) s.t_drift[k] = s.front.P_old[k] - t[k];
    }
  }
  if (!s.on_device) vio_features_set_depth(s.fm, s.inv_depth.data(), n_features);
  // n == -1: MARGIN_SECOND_NEW without the second-newest pose in the old prior leaves it as it was (VINS.cpp:778-779)
  if (next_prior && next_prior->n > 0) s.cur_prior = 1 - s.cur_prior, s.has_prior = true;
}

void stage_window(const FrameCall &fc, int q) {
  vio_estimator *e = fc.e;
  const int rc = build_window(e, e->seq[q], &e->staged[q]);
  // (an error is typically VIO_ECAP: more landmarks / factors than cfg.max_features / max_factors.) The frame's observations
  // are in the landmark store but the window will not slide: without a restart add_check_parallax refuses every
  // following frame and the sequence stays stuck until the caller clears it.
  if (rc != VIO_OK) return restart_with_error(e, e->seq[q], fc.results[q], rc);
  e->wants_solve[q] = 1;
}

// The end of a solved NON_LINEAR frame (VINS.cpp:455-476); `reasons`: failureDetection's verdict, of the host or of the store
void finish_nonlinear_frame(vio_estimator *e, Sequence &s, VioFrameResult &res, int reasons) {
  if (reasons) {
    s.failure_occur = 1;
    clear_state(e, s);
    res.action = VIO_FRAME_FAILURE, res.failure_reasons = reasons;
    return;
  }
  slide_window(e, s);
  if (!s.on_device) vio_features_remove_failures(s.fm);  // (a resident sequence's list is in its store slot, `fm` is empty)
  remember_last(e, s);
  res.action = VIO_FRAME_SOLVED;
}
}  // namespace
