// vio_estimator.cpp — the estimator state machine around the device solve (host side), for n independent sequences.
//
// Reference: class VINS (VINS_ios/VINS.hpp:47-200): processIMU (VINS.cpp:333-375), processImage (:377-478), the host
// half of solve_ceres (old2new :89-129, the factor list :528-637, the loop bookkeeping :664-680 and new2old :168-189),
// failureDetection (:214-265), slideWindow / slideWindowOld / slideWindowNew (:1149-1273), clearState (:36-81),
// solveInitial / relativePose / visualInitialAlign (:833-1145).
// One reference VINS object = one sequence here; the solve of ALL sequences that have a frame to solve goes to the
// device in ONE launch of the window kernel (vio_backend_solve_windows), everything else is the same small host
// bookkeeping the reference does on its "mainLoop" thread.
//
// Here: the extern "C" entries, the grouping of the sequences and the pipeline of one frame (vio_estimator_process_images, its
// phases A and C and its two group stages). In the headers this one translation unit includes: est_state.h the state and its own
// steps, est_window.h a call's arguments and the window to the solver and back, est_resident.h sequences that live on the
// device, est_startup.h solveInitial and its three routes: vio_estimator_set_init_device 0 keeps it on the host pool, 1 sends a
// call's bundle adjustments to the device in one vio_init_ba_solve, 2 everything between relativePose's scan and the alignment
// in one vio_init_sfm_solve; a window handed over with vio_estimator_set_initial_state takes solveInitial's place.
#include "est_state.h"
#include "est_window.h"
#include "est_startup.h"
#include "est_resident.h"

namespace {
// The sequences are solved in n_groups contiguous groups, one back-end context each. Decided before the first solve.
void regroup(vio_estimator *e) {
  for (int g = 0; g < vio_estimator::kMaxGroups; g++)
    if (e->be[g]) return;  // (contexts exist: slots and prior stores are bound to the grouping)
  const int n_seq = e->n_seq;
  // Two groups by default: more groups only pay while every group's stream has a hardware queue of its own (HIP maps
  // streams onto 4 queues by default; in a process that holds other streams — a torch process, say — four groups
  // alias, two of the kernels serialize and the frame gets slower than with one group: 36 k instead of 48 k solves/s).
  // groups of about 256 sequences (one window-kernel launch that fills every CU's two workgroup slots half), at least two
  int ng = n_seq >= 64 ? std::max(2, (n_seq + 128) / 256) : 1;
  // Resident sequences leave the host little to overlap with the kernel, and one launch of all windows fills the CUs'
  // second workgroup slots by itself (measured, 512 sequences: 4.9 ms per frame with one group, 6.7 ms with two)
  if (e->resident && e->resident_priors) ng = 1;
  ng = std::max(1, std::min(std::min(ng, (int)vio_estimator::kMaxGroups), n_seq));
  e->group_size = (n_seq + ng - 1) / ng;
  e->n_groups = (n_seq + e->group_size - 1) / e->group_size;
}

// Phase A of a sequence in the INITIAL state: the frame joins all_image_frame; a full window starts up or waits.
void phase_a_initial(const FrameCall &fc, int q) {
  vio_estimator *e = fc.e;
  Sequence &s = e->seq[q];
  VioFrameResult &res = fc.results[q];
  // ImageFrame imageframe(image_msg, header); pre_integration = tmp_pre_integration; a fresh one starts (VINS.cpp:402-404)
  init::Frame f = s.tmp_valid ? s.tmp : init::Frame();
  f.header = fc.headers[q];
  f.points.assign(fc.obs_of(q), fc.obs_of(q) + fc.n_obs[q]);
  s.all_image_frame[fc.headers[q]] = f;
  s.tmp = init::Frame();
  memcpy(s.tmp.lin_acc, s.acc_0, 24), memcpy(s.tmp.lin_gyr, s.gyr_0, 24);
  const double zero[3] = {0, 0, 0};
  init::repropagate(e->cfg, s.tmp, zero, zero);
  s.tmp_valid = true;
  if (s.frame_count != e->W) {
    s.frame_count++;
    res.action = VIO_FRAME_FILLING;
    return;
  }
  if (s.last_track_num < 20) {
    clear_state(e, s);
    res.action = VIO_FRAME_RESET;
    return;
  }
  if (take_initial_state(e, s)) return stage_window(fc, q);
  Startup started = Startup::kFailed;
  if (e->enable_init && fc.headers[q] - s.initial_timestamp > 0.3) started = begin_startup(fc, q);  // VINS.cpp:413-417
  if (started == Startup::kWaitBa || started == Startup::kWaitSfm) e->init_wait[q] = 1;
  else end_startup(fc, q, started == Startup::kSucceeded);
}

// Phase A, per sequence (pool): landmark bookkeeping, the INITIAL / NON_LINEAR branch, triangulation, the window for the solver.
void phase_a(const FrameCall &fc, int q) {
  vio_estimator *e = fc.e;
  VioFrameResult &res = fc.results[q];
  memset(&res, 0, sizeof(res));
  res.action = VIO_FRAME_SKIPPED;
  if (fc.active && !fc.active[q]) return;
  Sequence &s = e->seq[q];
  if (s.on_device) return;  // its frame goes through the resident path
  int enough = 0, parallax_num = 0;
  if (!obs_count_ok(fc.n_obs[q], fc.obs_stride)) {
    res.action = VIO_FRAME_ERROR, res.error = VIO_EINVAL;
    return;
  }
  const int rc = vio_features_add_check_parallax(s.fm, s.frame_count, fc.obs_of(q), fc.n_obs[q], &enough, &parallax_num, &s.last_track_num);
  // the landmark store may hold part of this frame while the window did not advance: every later frame would be
  // refused as out of order (VIO_ESTATE). Restart the sequence, as after a device error.
  if (rc != VIO_OK) return restart_with_error(e, s, res, rc);
  s.marginalization_flag = enough ? VIO_MARGIN_OLD : VIO_MARGIN_SECOND_NEW;
  res.marginalization_flag = s.marginalization_flag, res.track_num = s.last_track_num;
  vio_features_count(s.fm, &res.n_features);
  s.Headers[s.frame_count] = fc.headers[q];
  if (s.solver_flag == VIO_SOLVER_INITIAL) return phase_a_initial(fc, q);
  vio_features_triangulate(s.fm, s.Ps.data(), s.Rs.data(), s.cam.tic, s.cam.ric);
  stage_window(fc, q);
}

// Phase C, per solved sequence (pool): double2vector, loop bookkeeping, failure detection, slide.
void phase_c(const FrameCall &fc, int k) {
  vio_estimator *e = fc.e;
  const int W = e->W, q = e->solving[k];
  Sequence &s = e->seq[q];
  VioFrameResult &res = fc.results[q];
  const VioWindow &w = e->windows[k];
  res.stats = e->stats[k];
  res.n_factors = w.n_factors, res.n_loop_factors = s.n_loop_factors, res.n_features = w.n_features;
  take_solution(e, s, w.n_features, w.next_prior, e->stats[k]);
  if (s.solver_flag == VIO_SOLVER_INITIAL && s.final_cost > 200) {  // initialization failed, need reinitialize (VINS.cpp:415-424)
    s.has_prior = false;
    res.action = VIO_FRAME_INIT_FAILED;
    slide_window(e, s);
    return;
  }
  s.failure_occur = 0;
  int reasons = 0;
  if (s.solver_flag == VIO_SOLVER_INITIAL) s.solver_flag = VIO_SOLVER_NON_LINEAR;  // (the first solve: no failure detection)
  else vio_failure_detection(s.last_track_num, &s.Bgs[3 * W], &s.Ps[3 * W], &s.Rs[9 * W], s.last_P, s.last_R, &reasons);
  finish_nonlinear_frame(e, s, res, reasons);
}

struct GroupRun {  // what the two group loops of a call share
  int g0[vio_estimator::kMaxGroups + 1] = {0};  // the group's first window among e->solving / e->windows
  bool launched[vio_estimator::kMaxGroups] = {};
  int rc = VIO_OK, first_error = VIO_OK;
  double ms_a = 0, ms_c = 0;
};
double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

// Group g, first half: phase A on the pool, its start-ups in one device call, its windows compacted, uploaded, launched -- no wait.
void launch_group(const FrameCall &fc, int g, GroupRun &run) {
  vio_estimator *e = fc.e;
  const int q0 = g * e->group_size, q1 = std::min(e->n_seq, q0 + e->group_size);
  const auto ta = std::chrono::steady_clock::now();
  // (small groups: one sweep of the pool over all sequences is cheaper than a sweep per group -- measured 5.15 vs 5.4 ms
  // per frame with 2 x 128 sequences, 12.1 vs 15.5 ms the other way round with 4 x 256)
  const bool pipelined = e->n_groups > 1 && e->group_size >= 256;
  const int a0 = pipelined ? q0 : 0, a1 = pipelined ? q1 : (g == 0 ? e->n_seq : 0);
  if (a1 > a0) {
    HostPool::get().parallel_for(a1 - a0, [&](int i) { phase_a(fc, a0 + i); });
    run_startup_batch(fc, a0, a1);
  }
  run.g0[g] = (int)e->solving.size();
  run.first_error = first_error_of(fc.results, q0, q1, run.first_error);
  for (int q = q0; q < q1; q++) {
    if (!e->wants_solve[q]) continue;
    e->windows[e->solving.size()] = e->staged[q];
    e->solving.push_back(q);
  }
  run.g0[g + 1] = (int)e->solving.size();
  run.ms_a += ms_between(ta, std::chrono::steady_clock::now());
  const int ng = run.g0[g + 1] - run.g0[g];
  if (ng == 0 || run.rc != VIO_OK) return;
  int rc = VIO_OK;
  if (!e->be[g]) {
    rc = vio_backend_create(&e->cfg, e->group_size, &e->be[g]);
    if (rc == VIO_OK) rc = vio_backend_set_peers(e->be[g], e->n_groups);
    if (rc == VIO_OK && e->resident_priors) rc = vio_backend_reserve_priors(e->be[g], e->group_size);
  }
  if (rc == VIO_OK && e->any_camera) {  // ProjectionFactor::sqrt_info of every window's own camera (VINS.cpp:31)
    std::vector<double> si(ng);
    for (int k = 0; k < ng; k++) si[k] = e->seq[e->solving[run.g0[g] + k]].cam.fx / 1.5;
    rc = vio_backend_upload_cam ? vio_backend_upload_cam(e->be[g], e->windows.data() + run.g0[g], ng, si.data()) : VIO_ENODEV;
  } else if (rc == VIO_OK) {
    rc = vio_backend_upload(e->be[g], e->windows.data() + run.g0[g], ng);
  }
  if (rc == VIO_OK) rc = vio_backend_launch(e->be[g], nullptr);
  run.launched[g] = rc == VIO_OK;
  run.rc = rc;
}
}  // namespace

extern "C" {

int vio_estimator_create(const VioConfig *cfg, int32_t n_seq, const double tic[3], const double ric[9],
                         vio_estimator_t **out) {
  if (!cfg || !out || n_seq < 1 || !tic || !ric || cfg->window_size < 3 || cfg->max_features < 1 || cfg->max_factors < 1)
    return VIO_EINVAL;
  vio_estimator *e = new (std::nothrow) vio_estimator();
  if (!e) return VIO_ENOMEM;
  e->cfg = *cfg, e->W = cfg->window_size, e->n_seq = n_seq;
  regroup(e);
  memcpy(e->tic, tic, 24), memcpy(e->ric, ric, 72);
  const int W = e->W, P = W + 1, cap = vio_prior_capacity(W);
  e->seq.resize(n_seq);
  for (Sequence &s : e->seq) {
    s.Ps.assign(3 * P, 0), s.Rs.assign(9 * P, 0), s.Vs.assign(3 * P, 0), s.Bas.assign(3 * P, 0), s.Bgs.assign(3 * P, 0);
    s.Headers.assign(P, 0);
    s.pre.resize(P), s.pre_valid.assign(P, 0);
    s.dt_buf.resize(P), s.acc_buf.resize(P), s.gyr_buf.resize(P);
    s.lin_acc.assign(3 * P, 0), s.lin_gyr.assign(3 * P, 0);
    if (vio_features_create(W, &s.fm) != VIO_OK) {
      vio_estimator_destroy(e);
      return VIO_ENOMEM;
    }
    s.index = (int)(&s - e->seq.data());
    vio_camera_from_config(cfg, tic, ric, &s.cam);
    s.prior[0].init(cap, e->resident_priors), s.prior[1].init(cap, e->resident_priors);
    memcpy(s.last_R, kI3, 72), memcpy(s.last_R_old, kI3, 72), memcpy(s.r_drift, kI3, 72);
    for (int k = 0; k < 3; k++) s.last_P[k] = s.last_P_old[k] = s.t_drift[k] = 0;
    s.pose.assign(7 * P, 0), s.sb.assign(9 * P, 0), s.raw_pose.assign(7 * P, 0), s.raw_sb.assign(9 * P, 0);
    s.inv_depth.assign(cfg->max_features, 0);
    s.pts_i.assign((size_t)3 * cfg->max_factors, 0), s.pts_j.assign((size_t)3 * cfg->max_factors, 0);
    s.f_host.assign(cfg->max_factors, 0), s.f_target.assign(cfg->max_factors, 0), s.f_feat.assign(cfg->max_factors, 0);
    s.preint.resize(W);
    s.pre_dirty.assign(P, 0), s.pre_stale.assign(P, 0), s.pre_merge.assign(P, 0);
    clear_state(e, s);
  }
  e->windows.resize(n_seq), e->stats.resize(n_seq);
  e->init_stage.resize(n_seq), e->init_wait.assign(n_seq, 0), e->init_device_count.assign(n_seq, 0);
  *out = e;
  return VIO_OK;
}

void vio_estimator_destroy(vio_estimator_t *e) {
  if (!e) return;
  for (Sequence &s : e->seq)
    if (s.fm) vio_features_destroy(s.fm);
  for (int g = 0; g < vio_estimator::kMaxGroups; g++)
    if (e->be[g]) vio_backend_destroy(e->be[g]);
  if (e->init_ba && vio_init_ba_destroy) vio_init_ba_destroy(e->init_ba);
  if (e->init_sfm && vio_init_sfm_destroy) vio_init_sfm_destroy(e->init_sfm);
  delete e;
}

int vio_estimator_enable_initialization(vio_estimator_t *e, int32_t enable) {
  if (!e) return VIO_EINVAL;
  e->enable_init = enable != 0;
  e->init_relpose_fit = enable == 2;
  return VIO_OK;
}

int vio_estimator_set_init_device(vio_estimator_t *e, int32_t enable) {
  if (!e || enable < 0 || enable > 2) return VIO_EINVAL;
  e->init_device = enable;
  return VIO_OK;
}

int vio_estimator_set_resident(vio_estimator_t *e, int32_t enable) {
  if (!e) return VIO_EINVAL;
  if (enable && !e->resident_priors) return VIO_ESTATE;  // (VIO_AMD_HOST_PRIORS=1: the priors travel through the host)
  e->resident = enable != 0;
  regroup(e);
  if (!e->resident)
    for (Sequence &s : e->seq) {
      const int rc = demote(e, s);
      if (rc != VIO_OK) return rc;
    }
  return VIO_OK;
}

int vio_estimator_clear(vio_estimator_t *e, int32_t seq) {
  if (!e || seq < 0 || seq >= e->n_seq) return VIO_EINVAL;
  Sequence &s = e->seq[seq];
  clear_state(e, s);
  // a manual reset starts the sequence over as the constructor leaves it (VINS.cpp:19-21): no loop drift either. The
  // clearState of a failure inside process_image keeps the drift, as in the reference.
  memcpy(s.r_drift, kI3, 72);
  for (int k = 0; k < 3; k++) s.t_drift[k] = 0;
  return VIO_OK;
}

// The per-device globals of setGlobalParam (global_param.cpp:24-131) for ONE sequence. Only while the sequence holds no frame:
// every landmark, pre-integration and prior of a window was made with one camera.
int vio_estimator_set_camera(vio_estimator_t *e, int32_t seq, const VioCamera *cam) {
  if (!e || seq < 0 || seq >= e->n_seq || !cam) return VIO_EINVAL;
  // (fx > 0: ProjectionFactor::sqrt_info = fx / 1.5 weighs the residuals, VINS.cpp:31; the back end takes no other)
  if (!camera_valid(*cam, true) || !(cam->fx > 0)) return VIO_EINVAL;
  Sequence &s = e->seq[seq];
  if (s.frame_count != 0 || s.on_device) return VIO_ESTATE;
  s.cam = *cam;
  e->any_camera = true;
  return VIO_OK;
}

int vio_estimator_get_camera(vio_estimator_t *e, int32_t seq, VioCamera *out) {
  if (!e || seq < 0 || seq >= e->n_seq || !out) return VIO_EINVAL;
  *out = e->seq[seq].cam;
  return VIO_OK;
}

// VINS::processIMU (VINS.cpp:333-375): extend the pre-integration of the interval that ends in the frame being filled
// and propagate that frame's state with the midpoint rule.
int vio_estimator_process_imu(vio_estimator_t *e, int32_t seq, double dt, const double acc[3], const double gyr[3]) {
  if (!e || seq < 0 || seq >= e->n_seq || !acc || !gyr) return VIO_EINVAL;
  Sequence &s = e->seq[seq];
  if (!s.first_imu) {
    s.first_imu = true;
    memcpy(s.acc_0, acc, 24), memcpy(s.gyr_0, gyr, 24);
  }
  const int j = s.frame_count;
  if (!s.pre_valid[j]) new_preintegration(e, s, j);
  if (j != 0) {
    if (s.on_device && e->resident_imu) s.pre_stale[j] = 1;  // (the device integrates this interval from the buffered samples)
    else host::propagate(s.pre[j], dt, acc, gyr);
    if (s.solver_flag != VIO_SOLVER_NON_LINEAR && s.tmp_valid) {  // tmp_pre_integration->push_back (VINS.cpp:350-351)
      host::propagate(s.tmp.pre, dt, acc, gyr);
      s.tmp.dt.push_back(dt);
      for (int k = 0; k < 3; k++) s.tmp.acc.push_back(acc[k]), s.tmp.gyr.push_back(gyr[k]);
    }
    s.dt_buf[j].push_back(dt);
    for (int k = 0; k < 3; k++) s.acc_buf[j].push_back(acc[k]), s.gyr_buf[j].push_back(gyr[k]);
    const double g[3] = {0, 0, e->cfg.gravity};
    double *R = &s.Rs[9 * j], *Pj = &s.Ps[3 * j], *V = &s.Vs[3 * j];
    const double *ba = &s.Bas[3 * j], *bg = &s.Bgs[3 * j];
    double a0[3], ua0[3], w[3], a1[3], ua1[3];
    for (int k = 0; k < 3; k++) a0[k] = s.acc_0[k] - ba[k], w[k] = 0.5 * (s.gyr_0[k] + gyr[k]) - bg[k];
    mat3vec(R, a0, ua0);
    // Rs[j] *= deltaQ(un_gyr * dt).toRotationMatrix()  (utility.hpp:22-34: a small-angle quaternion, NOT normalized)
    double dR[9], Rn[9];
    qtoR(Quat{w[0] * dt / 2, w[1] * dt / 2, w[2] * dt / 2, 1.0}, dR);
    mat3mul(R, dR, Rn);
    memcpy(R, Rn, 72);
    for (int k = 0; k < 3; k++) a1[k] = acc[k] - ba[k];
    mat3vec(R, a1, ua1);
    for (int k = 0; k < 3; k++) {
      const double ua = 0.5 * ((ua0[k] - g[k]) + (ua1[k] - g[k]));
      Pj[k] += dt * V[k] + 0.5 * dt * dt * ua;
      V[k] += dt * ua;
    }
  }
  memcpy(s.acc_0, acc, 24), memcpy(s.gyr_0, gyr, 24);
  return VIO_OK;
}

// processIMU for every sequence at once: sequence q receives n_samples[q] samples dt/acc/gyr[q*stride ...], in order.
// Sequences are independent, so they are spread over the host pool (one frame interval of 256 sequences is a few
// thousand 15x15 covariance propagations).
int vio_estimator_process_imu_batch(vio_estimator_t *e, const int32_t *n_samples, int32_t stride, const double *dt,
                                    const double *acc, const double *gyr) {
  if (!e || !n_samples || stride < 0 || !dt || !acc || !gyr) return VIO_EINVAL;
  for (int q = 0; q < e->n_seq; q++)
    if (n_samples[q] < 0 || n_samples[q] > stride) return VIO_EINVAL;
  HostPool::get().parallel_for(e->n_seq, [&](int q) {
    for (int i = 0; i < n_samples[q]; i++) {
      const size_t k = (size_t)q * stride + i;
      vio_estimator_process_imu(e, q, dt[k], acc + 3 * k, gyr + 3 * k);
    }
  });
  return VIO_OK;
}

int vio_estimator_set_initial_state(vio_estimator_t *e, int32_t seq, const double *headers, const double *Ps,
                                    const double *Rs, const double *Vs, const double *Bas, const double *Bgs) {
  if (!e || seq < 0 || seq >= e->n_seq || !headers || !Ps || !Rs || !Vs || !Bas || !Bgs) return VIO_EINVAL;
  Sequence &s = e->seq[seq];
  if (s.solver_flag != VIO_SOLVER_INITIAL) return VIO_ESTATE;
  const int P = e->W + 1;
  s.init_headers.assign(headers, headers + P);
  s.init_Ps.assign(Ps, Ps + 3 * P), s.init_Rs.assign(Rs, Rs + 9 * P), s.init_Vs.assign(Vs, Vs + 3 * P);
  s.init_Bas.assign(Bas, Bas + 3 * P), s.init_Bgs.assign(Bgs, Bgs + 3 * P);
  s.init_pending = true;
  return VIO_OK;
}

int vio_estimator_set_relocalization(vio_estimator_t *e, int32_t seq, double header, const double P_old[3],
                                     const double Q_old[4], const int32_t *ids, const double *xy, int32_t n) {
  if (!e || seq < 0 || seq >= e->n_seq || n < 0 || (n > 0 && (!ids || !xy || !P_old || !Q_old))) return VIO_EINVAL;
  Relocalization &r = e->seq[seq].retrive;
  r = Relocalization();
  r.header = header;
  if (n > 0) {
    memcpy(r.P_old, P_old, 24);
    r.Q_old = Quat{Q_old[0], Q_old[1], Q_old[2], Q_old[3]};
    r.ids.assign(ids, ids + n), r.xy.assign(xy, xy + 2 * n);
  }
  return VIO_OK;
}

// VINS::processImage for every active sequence (VINS.cpp:377-478); the solves of all of them are ONE device launch.
int vio_estimator_process_images(vio_estimator_t *e, const VioObs *obs, const int32_t *n_obs, int32_t obs_stride,
                                 const double *headers, const uint8_t *active, VioFrameResult *results) {
  if (!e || !obs || !n_obs || !headers || !results || obs_stride < 0) return VIO_EINVAL;
  const int P = e->W + 1;
  const FrameCall fc{e, obs, n_obs, obs_stride, headers, active, results, e->cfg.max_features, e->cfg.max_factors + e->cfg.max_features, 4 * P};
  GroupRun run;
  e->solving.clear();
  const auto t_begin = std::chrono::steady_clock::now();
  // resident sequences that cannot stay on the device for this frame go back to the host-side list first
  bool any_resident = false;
  for (Sequence &s : e->seq) {
    if (!s.on_device || (active && !active[s.index])) continue;
    select_loop_frame(s, e->W);
    if (!resident_eligible(e, s) || n_obs[s.index] > e->res_obs_cap) {
      const int rcd = demote(e, s);
      if (rcd != VIO_OK) clear_state(e, s);
      if (run.first_error == VIO_OK) run.first_error = rcd;
    }
    any_resident = any_resident || s.on_device;
  }
  e->staged.resize(e->n_seq);
  e->wants_solve.assign(e->n_seq, 0);
  // The sequences form n_groups contiguous groups with a back-end context each (own stream, own resident batch, own
  // prior store). Group after group: phase A of the group on the host pool, its windows packed, uploaded and launched --
  // no device wait, so the kernels of the earlier groups run while the host prepares the later ones. Then, group after
  // group again: wait, download, phase C -- while the later groups' kernels are still running.
  for (int g = 0; g < e->n_groups; g++) launch_group(fc, g, run);
  for (int g = 0; g < e->n_groups; g++) {
    const int k0 = run.g0[g], ng = run.g0[g + 1] - k0;
    if (ng == 0 || !run.launched[g]) continue;  // (every LAUNCHED group is waited for, also after an error in another group)
    // (status per group: a group whose own launch and download succeeded runs its phase C also when another group failed;
    // the first error is still what the call returns, and only the sequences of the failed / unlaunched groups restart)
    const int rd = vio_backend_download(e->be[g], e->windows.data() + k0, ng, e->stats.data() + k0);
    if (run.rc == VIO_OK) run.rc = rd;
    if (rd != VIO_OK) continue;
    const auto tc = std::chrono::steady_clock::now();
    HostPool::get().parallel_for(ng, [&](int i) { phase_c(fc, k0 + i); });
    run.ms_c += ms_between(tc, std::chrono::steady_clock::now());
  }
  if (any_resident) {
    const int rcr = resident_frame(fc);
    if (rcr != VIO_OK && run.first_error == VIO_OK) run.first_error = rcr;
  }
  if (run.rc != VIO_OK) {
    // The frame is in the landmark stores of every sequence that wanted a solve. Sequences whose phase C has run (every group
    // whose own launch and download went through) have slid their windows and stay; the others did not advance: they
    // restart rather than carry an inconsistent window (and a prior slot that may or may not have advanced) into the next call.
    for (int q : e->solving)
      if (results[q].action != VIO_FRAME_SOLVED && results[q].action != VIO_FRAME_FAILURE && results[q].action != VIO_FRAME_INIT_FAILED)
        restart_with_error(e, e->seq[q], results[q], run.rc);
    return run.rc;
  }
  // (phases A and C are interleaved with the device work of the other groups: their own sums, and the rest)
  e->ms_pre = run.ms_a, e->ms_post = run.ms_c;
  e->ms_solve = ms_between(t_begin, std::chrono::steady_clock::now()) - run.ms_a - run.ms_c;
  // sequences that reached the NON_LINEAR state on the host path continue on the device
  for (int g = 0; g < e->n_groups && e->resident; g++) {  // (a store that cannot be reserved turns `resident` off for good)
    std::vector<int> go;
    for (int q = g * e->group_size; q < std::min(e->n_seq, (g + 1) * e->group_size); q++)
      if (!e->seq[q].on_device && results[q].action == VIO_FRAME_SOLVED && resident_eligible(e, e->seq[q])) go.push_back(q);
    promote_group(e, g, go);
  }
  return run.first_error;
}

int vio_estimator_get_timing(vio_estimator_t *e, double ms[3]) {
  if (!e || !ms) return VIO_EINVAL;
  ms[0] = e->ms_pre, ms[1] = e->ms_solve, ms[2] = e->ms_post;
  return VIO_OK;
}

int vio_estimator_process_image(vio_estimator_t *e, int32_t seq, const VioObs *obs, int32_t n_obs, double header,
                                VioFrameResult *result) {
  if (!e || seq < 0 || seq >= e->n_seq || !result || n_obs < 0 || (n_obs > 0 && !obs)) return VIO_EINVAL;
  std::vector<uint8_t> active(e->n_seq, 0);
  std::vector<int32_t> n(e->n_seq, 0);
  std::vector<double> hdr(e->n_seq, 0);
  std::vector<VioFrameResult> res(e->n_seq);
  active[seq] = 1, n[seq] = n_obs, hdr[seq] = header;
  // stride 0: every sequence would read the same list, only `seq` is active
  static const VioObs none = {0, 0, 0, 0};
  int rc = vio_estimator_process_images(e, n_obs > 0 ? obs : &none, n.data(), 0, hdr.data(), active.data(), res.data());
  *result = res[seq];
  return rc;
}

int vio_estimator_get_status(vio_estimator_t *e, int32_t seq, VioEstimatorStatus *st) {
  if (!e || seq < 0 || seq >= e->n_seq || !st) return VIO_EINVAL;
  const Sequence &s = e->seq[seq];
  memset(st, 0, sizeof(*st));
  st->frame_count = s.frame_count, st->solver_flag = s.solver_flag, st->marginalization_flag = s.marginalization_flag;
  st->failure_occur = s.failure_occur, st->prior_rows = s.has_prior ? s.prior[s.cur_prior].p.n : 0;
  st->final_cost = s.final_cost;
  memcpy(st->r_drift, s.r_drift, 72), memcpy(st->t_drift, s.t_drift, 24);
  memcpy(st->relative_t, s.front.relative_t, 24);
  st->relative_q[0] = s.front.relative_q.x, st->relative_q[1] = s.front.relative_q.y;
  st->relative_q[2] = s.front.relative_q.z, st->relative_q[3] = s.front.relative_q.w;
  st->relative_yaw = s.front.relative_yaw;
  memcpy(st->loop_pose, s.front.loop_pose, sizeof(st->loop_pose));
  st->resident = s.on_device ? 1 : 0;
  st->init_device_count = e->init_device_count[seq];
  return VIO_OK;
}

int vio_estimator_get_window(vio_estimator_t *e, int32_t seq, double *Ps, double *Rs, double *Vs, double *Bas, double *Bgs,
                             double *headers) {
  if (!e || seq < 0 || seq >= e->n_seq) return VIO_EINVAL;
  const Sequence &s = e->seq[seq];
  const int P = e->W + 1;
  if (Ps) memcpy(Ps, s.Ps.data(), sizeof(double) * 3 * P);
  if (Rs) memcpy(Rs, s.Rs.data(), sizeof(double) * 9 * P);
  if (Vs) memcpy(Vs, s.Vs.data(), sizeof(double) * 3 * P);
  if (Bas) memcpy(Bas, s.Bas.data(), sizeof(double) * 3 * P);
  if (Bgs) memcpy(Bgs, s.Bgs.data(), sizeof(double) * 3 * P);
  if (headers) memcpy(headers, s.Headers.data(), sizeof(double) * P);
  return VIO_OK;
}

// update_loop_correction (VINS.cpp:302-331): the window poses with the loop drift applied.
int vio_estimator_get_corrected_window(vio_estimator_t *e, int32_t seq, double *correct_Ps, double *correct_Rs) {
  if (!e || seq < 0 || seq >= e->n_seq || !correct_Ps || !correct_Rs) return VIO_EINVAL;
  const Sequence &s = e->seq[seq];
  for (int i = 0; i <= e->W; i++) {
    double t[3];
    mat3vec(s.r_drift, &s.Ps[3 * i], t);
    for (int k = 0; k < 3; k++) correct_Ps[3 * i + k] = t[k] + s.t_drift[k];
    mat3mul(s.r_drift, &s.Rs[9 * i], &correct_Rs[9 * i]);
  }
  return VIO_OK;
}

// vins.t_drift = loop_correct_t; vins.r_drift = loop_correct_r (ViewController.mm:998-999)
int vio_estimator_set_drift(vio_estimator_t *e, int32_t seq, const double *r_drift, const double *t_drift) {
  if (!e || seq < 0 || seq >= e->n_seq || !r_drift || !t_drift) return VIO_EINVAL;
  memcpy(e->seq[seq].r_drift, r_drift, 72), memcpy(e->seq[seq].t_drift, t_drift, 24);
  return VIO_OK;
}

int vio_estimator_features(vio_estimator_t *e, int32_t seq, vio_features_t **fm) {
  if (!e || seq < 0 || seq >= e->n_seq || !fm) return VIO_EINVAL;
  {  // a resident sequence's list comes back to the host first (it returns to the device after its next solved frame)
    const int rc = demote(e, e->seq[seq]);
    if (rc != VIO_OK) return rc;
  }
  *fm = e->seq[seq].fm;
  return VIO_OK;
}

// KeyFrame::buildKeyFrameFeatures (loop/keyframe.cpp:128-155) with the states of the moment, the ones get_window returns:
// the sequences on the host-side list on the host pool, the resident ones group by group on the device, where they stay.
int vio_estimator_keyframe_features(vio_estimator_t *e, int32_t n, const int32_t *seq, int32_t stride, int32_t *ids, float *px, float *norm,
                                    double *cloud, int32_t *count) {
  if (!e || n < 0 || stride < 0 || (n > 0 && (!seq || !count)) || (n > 0 && stride > 0 && (!ids || !px || !norm || !cloud))) return VIO_EINVAL;
  if (n > e->n_seq) return VIO_EINVAL;  // (some sequence would be named twice)
  std::vector<char> seen(e->n_seq, 0);
  for (int i = 0; i < n; i++) {
    if (seq[i] < 0 || seq[i] >= e->n_seq || seen[seq[i]]) return VIO_EINVAL;
    seen[seq[i]] = 1;
  }
  std::vector<int> host_rows;
  std::vector<std::vector<int>> dev_rows(e->n_groups);
  for (int i = 0; i < n; i++) {
    const Sequence &s = e->seq[seq[i]];
    count[i] = -1;
    if (s.solver_flag != VIO_SOLVER_NON_LINEAR || s.frame_count != e->W) continue;
    if (s.on_device) dev_rows[group_of(e, s)].push_back(i);
    else host_rows.push_back(i);
  }
  int first_error = VIO_OK;
  auto note = [&first_error](int rc) {
    if (rc != VIO_OK && (first_error == VIO_OK || first_error == VIO_ECAP)) first_error = rc;  // (a real error outranks "stride too small")
  };
  std::vector<int> host_rc(host_rows.size(), VIO_OK);
  HostPool::get().parallel_for((int)host_rows.size(), [&](int k) {
    const int i = host_rows[k];
    Sequence &s = e->seq[seq[i]];
    const size_t o = (size_t)i * stride;
    VioConfig cf = e->cfg;  // (the sequence's intrinsics: vio_features_keyframe takes them per call)
    cf.fx = s.cam.fx, cf.fy = s.cam.fy, cf.cx = s.cam.cx, cf.cy = s.cam.cy;
    host_rc[k] = vio_features_keyframe(s.fm, &cf, s.Ps.data(), s.Rs.data(), s.cam.tic, s.cam.ric, stride, ids + o, px + 2 * o, norm + 2 * o, cloud + 3 * o,
                                       &count[i]);
  });
  for (int rc : host_rc) note(rc);
  const double intr[4] = {e->cfg.fx, e->cfg.fy, e->cfg.cx, e->cfg.cy};
  std::vector<double> intr_of;  // [slots of the call][4], when some sequence has a camera of its own
  for (int g = 0; g < e->n_groups; g++) {
    const std::vector<int> &rows = dev_rows[g];
    if (rows.empty()) continue;
    if (!vio_backend_resident_keyframe || !e->be[g]) {
      note(VIO_ENODEV);
      continue;
    }
    std::vector<int32_t> slots;
    std::vector<const double *> pp, rr;
    intr_of.clear();
    for (int i : rows) {
      const Sequence &s = e->seq[seq[i]];
      slots.push_back(slot_of(e, s)), pp.push_back(s.Ps.data()), rr.push_back(s.Rs.data());
      if (e->any_camera) intr_of.insert(intr_of.end(), {s.cam.fx, s.cam.fy, s.cam.cx, s.cam.cy});
    }
    if (!e->any_camera)
      note(vio_backend_resident_keyframe(e->be[g], (int)rows.size(), slots.data(), rows.data(), pp.data(), rr.data(), intr, stride, ids, px, norm,
                                         cloud, count));
    else
      note(vio_backend_resident_keyframe_cam
               ? vio_backend_resident_keyframe_cam(e->be[g], (int)rows.size(), slots.data(), rows.data(), pp.data(), rr.data(), intr_of.data(), 4,
                                                   stride, ids, px, norm, cloud, count)
               : VIO_ENODEV);
  }
  return first_error;
}

}  // extern "C"
