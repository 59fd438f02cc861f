// est_startup.h — part of vio_estimator.cpp: the start-up of a sequence whose window has filled. Restates VINS::solveInitial,
// relativePose and visualInitialAlign (VINS.cpp:833-1145), Utility::g2R (utility.cpp:11-21) and the branch of processImage around
// them (:406-446), in host halves around the device call that can take the middle (vio_estimator_set_init_device: 0 none,
// 1 vio_init_ba_solve, 2 vio_init_sfm_solve): begin_startup picks the route, run_startup_batch calls the device, end_startup ends.
#pragma once
#include "est_window.h"

// The device side of solveInitial's bundle adjustment is vio_sfm.hip. This file is also built without any device code (the
// sanitizer walk of the tests links the host sources alone, with the back-end's entry points it needs stubbed): weak
// references, and where they are absent vio_estimator_set_init_device leaves every bundle adjustment on the host route.
extern "C" {
__attribute__((weak)) int vio_init_ba_create(int32_t, int32_t, int32_t, int32_t, vio_init_ba_t **);
__attribute__((weak)) void vio_init_ba_destroy(vio_init_ba_t *);
__attribute__((weak)) int vio_init_ba_solve(vio_init_ba_t *, VioInitBaProblem *, int32_t, VioSolveStats *);
__attribute__((weak)) int vio_init_sfm_create(int32_t, int32_t, int32_t, int32_t, int32_t, vio_init_sfm_t **);
__attribute__((weak)) void vio_init_sfm_destroy(vio_init_sfm_t *);
__attribute__((weak)) int vio_init_sfm_solve(vio_init_sfm_t *, VioInitSfmProblem *, int32_t, VioSolveStats *);
}

namespace {
// Eigen::Quaterniond::FromTwoVectors(a, b).toRotationMatrix() for unit a, b (Geometry/Quaternion.h)
void rotation_between(const double a[3], const double b[3], double R[9]) {
  const double c = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  if (c < -1.0 + 1e-12) {  // opposite vectors: any axis orthogonal to a, angle pi
    double ax[3] = {1, 0, 0};
    if (fabs(a[0]) > 0.9) ax[0] = 0, ax[1] = 1;
    double v[3] = {a[1] * ax[2] - a[2] * ax[1], a[2] * ax[0] - a[0] * ax[2], a[0] * ax[1] - a[1] * ax[0]};
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    qtoR(Quat{v[0] / n, v[1] / n, v[2] / n, 0.0}, R);
    return;
  }
  const double axis[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double sq = sqrt((1.0 + c) * 2.0), inv = 1.0 / sq;
  qtoR(Quat{axis[0] * inv, axis[1] * inv, axis[2] * inv, sq * 0.5}, R);
}

void g2R(const double g[3], double R0[9]) {  // Utility::g2R (utility.cpp:11-21)
  const double n = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  const double ng1[3] = {g[0] / n, g[1] / n, g[2] / n}, ng2[3] = {0, 0, 1};
  double R[9], ypr[3], Y[9], T[9];
  rotation_between(ng1, ng2, R);
  R2ypr(R, ypr);
  const double y1[3] = {-ypr[0], 0, 0};
  ypr2R(y1, Y);
  mat3mul(Y, R, T);
  const double y2[3] = {-90, 0, 0};
  ypr2R(y2, Y);
  mat3mul(Y, T, R0);
}

// The decision-free part of the head: the landmark dump and relativePose's scan (VINS.cpp:1106-1145) up to the fit: st.sfm_f,
// st.l, the correspondences of frames l and W and the gyroscope's rotation between them.
bool solve_initial_scan(vio_estimator *e, Sequence &s, InitStage &st, std::vector<double> &a, std::vector<double> &b, double hint[9]) {
  const int W = e->W, P = W + 1;
  // the landmark store as SfM features (VINS.cpp:883-899) and as correspondences (getCorresponding)
  int nfe = 0, npts = 0;
  vio_features_dump(s.fm, nullptr, 0, &nfe, nullptr, 0, &npts);
  std::vector<VioFeatureInfo> info(nfe > 0 ? nfe : 1);
  std::vector<double> pts(3 * (size_t)(npts > 0 ? npts : 1));
  if (vio_features_dump(s.fm, info.data(), nfe, &nfe, pts.data(), npts, &npts) != VIO_OK) return false;
  std::vector<init::SfmFeature> &sfm_f = st.sfm_f;
  sfm_f.assign(nfe, init::SfmFeature());
  std::vector<size_t> first(nfe);
  {
    size_t off = 0;
    for (int j = 0; j < nfe; j++) {
      first[j] = off;
      sfm_f[j].id = info[j].id;
      if (info[j].start_frame < 0 || info[j].start_frame + info[j].n_obs > P) return false;  // not a window's store
      for (int k = 0; k < info[j].n_obs; k++)
        sfm_f[j].observation.push_back({info[j].start_frame + k, {pts[3 * (off + k)], pts[3 * (off + k) + 1]}});
      off += info[j].n_obs;
    }
  }
  // relativePose (VINS.cpp:1106-1145): the oldest frame with enough parallax against the newest one
  for (int i = 0; i < W; i++) {
    a.clear(), b.clear();
    for (int j = 0; j < nfe; j++)
      if (info[j].start_frame <= i && info[j].start_frame + info[j].n_obs - 1 >= W) {
        const double *pa = &pts[3 * (first[j] + (i - info[j].start_frame))], *pb = &pts[3 * (first[j] + (W - info[j].start_frame))];
        a.push_back(pa[0]), a.push_back(pa[1]), b.push_back(pb[0]), b.push_back(pb[1]);
      }
    const int nc = (int)a.size() / 2;
    if (nc > 20) {
      double sum = 0;
      for (int k = 0; k < nc; k++) sum += sqrt((a[2 * k] - b[2 * k]) * (a[2 * k] - b[2 * k]) + (a[2 * k + 1] - b[2 * k + 1]) * (a[2 * k + 1] - b[2 * k + 1]));
      if (sum / nc * 520 < 30) return false;  // FAIL_PARALLAX
      // the gyroscope's rotation between frame i and the newest one, as a tie-breaker for planar scenes only: the product
      // of the pre-integrated delta_q of the intervals in between (body frame), moved into the camera frame
      Quat dq{0, 0, 0, 1};
      for (int k = i + 1; k <= W; k++) dq = qmul(dq, s.pre[k].dq);
      double Rb[9], Rt[9], ricT[9];
      qtoR(qnormalized(dq), Rb);
      mat3T(s.cam.ric, ricT);
      mat3mul(ricT, Rb, Rt), mat3mul(Rt, s.cam.ric, hint);
      st.l = i;
      return true;
    }
  }
  return false;
}

// VINS::solveInitial + relativePose + visualInitialAlign (VINS.cpp:833-1145), in two halves around the bundle adjustment
// that closes GlobalSFM::construct: solve_initial_head runs relativePose and construct up to it, solve_initial_tail the
// rest (the tail of construct, PnP of the in-between frames, the alignment).
bool solve_initial_head(vio_estimator *e, Sequence &s, InitStage &st) {
  std::vector<double> a, b;
  double hint[9], relative_R[9], relative_T[3];
  st.l = -1;
  if (!solve_initial_scan(e, s, st, a, b, hint)) return false;
  const bool got = e->init_relpose_fit ? init::solve_relative_rt(a, b, relative_R, relative_T, nullptr, hint)
                                       : init::solve_relative_rt_five_point(a, b, relative_R, relative_T, nullptr);
  if (!got) return false;  // FAIL_RELATIVE
  if (!init::sfm_construct_before_ba(e->W + 1, st.l, relative_R, relative_T, st.sfm_f, st.cq, st.tc)) {
    s.marginalization_flag = VIO_MARGIN_OLD;  // FAIL_SFM (VINS.cpp:915-917)
    return false;
  }
  return true;
}

// The bundle adjustment's arguments as vio_init_ba_solve takes them (the layout of vio_init_bundle_adjust).
void stage_ba_problem(InitStage &st) {
  const size_t n = st.sfm_f.size();
  st.points.assign(3 * n + 3, 0.0), st.ok.assign(n + 1, 0), st.start.assign(n + 1, 0), st.frame.clear(), st.xy.clear();
  st.n_ok = 0;
  for (size_t j = 0; j < n; j++) {
    const init::SfmFeature &f = st.sfm_f[j];
    memcpy(&st.points[3 * j], f.position, 24), st.ok[j] = f.state ? 1 : 0, st.n_ok += f.state ? 1 : 0;
    for (const auto &o : f.observation) st.frame.push_back(o.first), st.xy.push_back(o.second.first), st.xy.push_back(o.second.second);
    st.start[j + 1] = (int32_t)st.frame.size();
  }
  if (st.frame.empty()) st.frame.push_back(0), st.xy.resize(2, 0.0);  // (non-null pointers for a problem without observations)
}
// what the context's max_obs counts: the observations of the point_ok landmarks, or (level 2) of those seen at least twice
int staged_observations(const InitStage &st, bool seen_twice) {
  int n = 0;
  for (const init::SfmFeature &f : st.sfm_f)
    if (seen_twice ? f.observation.size() >= 2 : f.state != 0) n += (int)f.observation.size();
  return n;
}

// The walk over all_image_frame that gives every frame its camera pose (VINS.cpp:926-1003): the frames of the window's P slots
// go to on_window_frame(f, slot), every other one to on_extra_frame(f, guess, x) with the slot whose pose is its first guess and
// its running number among the extra frames; false from there ends the walk. The host route and both ends of level 2 use it.
template <class OnWindowFrame, class OnExtraFrame>
bool for_each_startup_frame(Sequence &s, int P, OnWindowFrame on_window_frame, OnExtraFrame on_extra_frame) {
  int i = 0, x = 0;
  for (auto &kv : s.all_image_frame) {
    init::Frame &f = kv.second;
    if (i < P && f.header == s.Headers[i]) {
      on_window_frame(f, i++);
      continue;
    }
    if (i < P && f.header > s.Headers[i]) i++;
    if (!on_extra_frame(f, std::min(i, P - 1), x++)) return false;
  }
  return true;
}
void window_frame_pose(init::Frame &f, const double q[4], const double T[3], const double ricT[9]) {
  double Rq[9];
  qtoR(Quat{q[0], q[1], q[2], q[3]}, Rq);
  f.is_key_frame = true;
  mat3mul(Rq, ricT, f.R);
  memcpy(f.T, T, 24);
}

// visualInitialAlign (VINS.cpp:1021-1104), once every frame of all_image_frame has its camera pose.
bool solve_initial_align(vio_estimator *e, Sequence &s) {
  const int W = e->W;
  std::vector<init::Frame> frames;
  frames.reserve(s.all_image_frame.size());
  for (auto &kv : s.all_image_frame) frames.push_back(kv.second);
  std::vector<double> x;
  if (!init::visual_imu_alignment(e->cfg, s.cam.tic, frames, W, s.Bgs.data(), s.g, x)) return false;  // FAIL_ALIGN
  {
    size_t k = 0;
    for (auto &kv : s.all_image_frame) kv.second = frames[k++];  // the re-integrated intervals
  }
  for (int k = 0; k <= s.frame_count; k++) {
    init::Frame &f = s.all_image_frame[s.Headers[k]];
    memcpy(&s.Ps[3 * k], f.T, 24), memcpy(&s.Rs[9 * k], f.R, 72);
    f.is_key_frame = true;
  }
  const double tic0[3] = {0, 0, 0};  // "triangulat on cam pose , no tic"
  retriangulate(e, s, tic0);
  const double sc = x.back();
  const double zero[3] = {0, 0, 0};
  for (int k = 0; k <= W; k++) repropagate(e, s, k, zero, &s.Bgs[3 * k]);
  {
    double r0t[3], base[3];
    mat3vec(&s.Rs[0], s.cam.tic, r0t);
    for (int k = 0; k < 3; k++) base[k] = sc * s.Ps[k] - r0t[k];
    for (int k = s.frame_count; k >= 0; k--) {
      double rt[3];
      mat3vec(&s.Rs[9 * k], s.cam.tic, rt);
      for (int c = 0; c < 3; c++) s.Ps[3 * k + c] = sc * s.Ps[3 * k + c] - rt[c] - base[c];
    }
  }
  {
    int kv = -1;
    for (auto &f : s.all_image_frame)
      if (f.second.is_key_frame) {
        kv++;
        if (kv <= W && 3 * (size_t)kv + 2 < x.size()) mat3vec(f.second.R, &x[3 * kv], &s.Vs[3 * kv]);  // x.segment<3>(kv * 3), as written
      }
  }
  vio_features_scale_depth(s.fm, sc);
  double R0[9], ypr[3], Yr[9], Rd[9], gn[3];
  g2R(s.g, R0);
  R2ypr(R0, ypr);
  const double yneg[3] = {-ypr[0], 0, 0};
  ypr2R(yneg, Yr);
  mat3mul(Yr, R0, Rd);
  mat3vec(Rd, s.g, gn);
  memcpy(s.g, gn, sizeof(gn));
  for (int k = 0; k <= s.frame_count; k++) {
    double v[3], M[9];
    mat3vec(Rd, &s.Ps[3 * k], v), memcpy(&s.Ps[3 * k], v, 24);
    mat3vec(Rd, &s.Vs[3 * k], v), memcpy(&s.Vs[3 * k], v, 24);
    mat3mul(Rd, &s.Rs[9 * k], M), memcpy(&s.Rs[9 * k], M, 72);
  }
  return true;
}

// ba_ok: the bundle adjustment's verdict (inital_sfm.cpp:279).
bool solve_initial_tail(vio_estimator *e, Sequence &s, InitStage &st, bool ba_ok) {
  const int W = e->W, P = W + 1;
  if (!ba_ok) {  // "vision only BA not converge"
    s.marginalization_flag = VIO_MARGIN_OLD;  // FAIL_SFM (VINS.cpp:915-917)
    return false;
  }
  std::vector<double> Q(4 * (size_t)P), T(3 * (size_t)P);
  std::map<int, std::vector<double>> tracked;
  init::sfm_construct_after_ba(P, st.cq, st.tc, st.sfm_f, Q.data(), T.data(), tracked);
  // PnP for every frame of all_image_frame (VINS.cpp:926-1003)
  double ricT[9];
  mat3T(s.cam.ric, ricT);
  const bool posed = for_each_startup_frame(
      s, P, [&](init::Frame &f, int i) { window_frame_pose(f, &Q[4 * i], &T[3 * i], ricT); },
      [&](init::Frame &f, int ii, int) {
        double Rq[9], R_init[9], P_init[3], v[3];
        qtoR(Quat{Q[4 * ii], Q[4 * ii + 1], Q[4 * ii + 2], Q[4 * ii + 3]}, Rq);
        mat3T(Rq, R_init);  // Q[i].inverse()
        mat3vec(R_init, &T[3 * ii], v);
        for (int k = 0; k < 3; k++) P_init[k] = -v[k];
        f.is_key_frame = false;
        std::vector<double> p3, p2;
        for (const VioObs &o : f.points) {
          auto it = tracked.find(o.id);
          if (it == tracked.end()) continue;
          p3.insert(p3.end(), it->second.begin(), it->second.end());
          p2.push_back(o.x), p2.push_back(o.y);
        }
        if (p2.size() / 2 < 6) return false;                       // "init Not enough points for solve pnp !"
        if (!init::pnp_refine(p3, p2, R_init, P_init)) return false;  // FAIL_PNP
        double R_pnp[9];
        mat3T(R_init, R_pnp);
        mat3mul(R_pnp, ricT, f.R);
        mat3vec(R_pnp, P_init, v);
        for (int k = 0; k < 3; k++) f.T[k] = -v[k];
        return true;
      });
  return posed && solve_initial_align(e, s);
}

bool solve_initial(vio_estimator *e, Sequence &s, InitStage &st) {
  if (!solve_initial_head(e, s, st)) return false;
  return solve_initial_tail(e, s, st, init::bundle_adjust(e->W + 1, st.l, st.cq, st.tc, st.sfm_f, nullptr));
}

// vio_estimator_set_init_device(est, 2). The pool's part ahead of the device call: the landmark dump, relativePose's scan, on
// the five-point route the relative pose itself, and the lists of the frames outside the window in the order
// solve_initial_tail walks them (VINS.cpp:926-1003). False: this attempt ends here, as solve_initial_head's would.
bool stage_sfm_problem(vio_estimator *e, Sequence &s, InitStage &st) {
  const int P = e->W + 1;
  std::vector<double> a, b;
  st.l = -1;
  if (!solve_initial_scan(e, s, st, a, b, st.hint)) return false;
  st.mode = e->init_relpose_fit ? 1 : 0;
  if (!e->init_relpose_fit && !init::solve_relative_rt_five_point(a, b, st.relative_R, st.relative_T, nullptr)) return false;
  stage_ba_problem(st);  // (the observation lists; its points / flags are outputs here)
  st.n_ok = 0;
  for (const init::SfmFeature &f : st.sfm_f) st.n_ok += f.observation.size() >= 2;
  std::map<int, int> index_of;
  for (size_t j = 0; j < st.sfm_f.size(); j++) index_of[st.sfm_f[j].id] = (int)j;
  st.ex_guess.clear(), st.ex_start.assign(1, 0), st.ex_feature.clear(), st.ex_xy.clear();
  for_each_startup_frame(
      s, P, [](init::Frame &, int) {},
      [&](init::Frame &f, int guess, int) {
        st.ex_guess.push_back(guess);
        for (const VioObs &o : f.points) {
          auto it = index_of.find(o.id);
          if (it == index_of.end()) continue;
          st.ex_feature.push_back(it->second), st.ex_xy.push_back(o.x), st.ex_xy.push_back(o.y);
        }
        st.ex_start.push_back((int32_t)st.ex_feature.size());
        return true;
      });
  const size_t ne = st.ex_guess.size();
  st.q.assign(4 * (size_t)P, 0.0), st.T.assign(3 * (size_t)P, 0.0), st.ex_R.assign(9 * ne + 9, 0.0), st.ex_T.assign(3 * ne + 3, 0.0);
  if (st.ex_feature.empty()) st.ex_feature.push_back(0), st.ex_xy.resize(2, 0.0);
  if (st.ex_guess.empty()) st.ex_guess.push_back(0);
  return true;
}

// ... and the pool's part behind it: the failure branches of solveInitial by the call's status, else the frames' camera poses
// from the call's outputs and the alignment.
bool finish_sfm_problem(vio_estimator *e, Sequence &s, InitStage &st) {
  const int P = e->W + 1;
  if (st.verdict == VIO_INIT_SFM_FAIL_CHAIN || st.verdict == VIO_INIT_SFM_FAIL_BA) s.marginalization_flag = VIO_MARGIN_OLD;  // FAIL_SFM (VINS.cpp:915-917)
  if (st.verdict != VIO_INIT_SFM_OK) return false;
  double ricT[9];
  mat3T(s.cam.ric, ricT);
  for_each_startup_frame(
      s, P, [&](init::Frame &f, int i) { window_frame_pose(f, &st.q[4 * i], &st.T[3 * i], ricT); },
      [&](init::Frame &f, int, int x) {
        f.is_key_frame = false;
        double R_pnp[9], v[3];
        mat3T(&st.ex_R[9 * (size_t)x], R_pnp);
        mat3mul(R_pnp, ricT, f.R);
        mat3vec(R_pnp, &st.ex_T[3 * (size_t)x], v);
        for (int k = 0; k < 3; k++) f.T[k] = -v[k];
        return true;
      });
  return solve_initial_align(e, s);
}

// The window handed over with vio_estimator_set_initial_state, where its headers are the window's: what solveInitial leaves behind (VINS.cpp:1081-1143)
bool take_initial_state(vio_estimator *e, Sequence &s) {
  const int P = e->W + 1;
  if (!s.init_pending || !std::equal(s.Headers.begin(), s.Headers.begin() + P, s.init_headers.begin())) return false;
  s.Ps = s.init_Ps, s.Rs = s.init_Rs, s.Vs = s.init_Vs, s.Bas = s.init_Bas, s.Bgs = s.init_Bgs;
  s.init_pending = false;
  // visualInitialAlign re-integrates every interval from the biases it found (VINS.cpp:1057-1060, with ba = 0 there)
  for (int i = 1; i < P; i++) repropagate(e, s, i, &s.Bas[3 * i], &s.Bgs[3 * i]);
  retriangulate(e, s, s.cam.tic);
  return true;
}

enum class Startup { kFailed, kSucceeded, kWaitBa, kWaitSfm };
// solveInitial is due for sequence q (pool): all of it, or its part ahead of the device call; a problem beyond the context's capacity stays on the host
Startup begin_startup(const FrameCall &fc, int q) {
  vio_estimator *e = fc.e;
  Sequence &s = e->seq[q];
  InitStage &st = e->init_stage[q];
  const int P = e->W + 1;
  const auto ended = [](bool result) { return result ? Startup::kSucceeded : Startup::kFailed; };
  if (e->init_device == 2 && P <= FrameCall::kInitDeviceMaxFrames) {
    const bool staged = stage_sfm_problem(e, s, st);
    s.initial_timestamp = fc.headers[q];
    if (!staged) return Startup::kFailed;
    if (st.n_ok <= fc.ba_max_points && staged_observations(st, true) <= fc.ba_max_obs && (int)st.ex_start.size() - 1 <= fc.sfm_max_extra)
      return Startup::kWaitSfm;  // continues in resume_startup, after this call's vio_init_sfm_solve
    return ended(solve_initial(e, s, st));
  }
  if (e->init_device) {
    const bool head = solve_initial_head(e, s, st);
    s.initial_timestamp = fc.headers[q];
    if (!head) return Startup::kFailed;
    if (P <= FrameCall::kInitDeviceMaxFrames) {
      stage_ba_problem(st);
      if (st.n_ok <= fc.ba_max_points && staged_observations(st, false) <= fc.ba_max_obs) return Startup::kWaitBa;  // ... after vio_init_ba_solve
    }
    return ended(solve_initial_tail(e, s, st, init::bundle_adjust(P, st.l, st.cq, st.tc, st.sfm_f, nullptr)));
  }
  const bool result = solve_initial(e, s, st);
  s.initial_timestamp = fc.headers[q];
  return ended(result);
}

// The start-up attempt of sequence q is over (pool): its window goes to the solver, or the frame waits for the next attempt.
void end_startup(const FrameCall &fc, int q, bool result) {
  fc.e->init_stage[q] = InitStage();  // (also on a frame without an attempt: the stage is empty then, nothing is freed or allocated)
  if (result) return stage_window(fc, q);
  VioFrameResult &res = fc.results[q];
  slide_window(fc.e, fc.e->seq[q]);
  res.action = VIO_FRAME_WAIT_INIT;
}

// ... after this call's device solve (pool); without a device context or after a failed call nothing was written: the host route
void resume_startup(const FrameCall &fc, int q) {
  vio_estimator *e = fc.e;
  Sequence &s = e->seq[q];
  InitStage &st = e->init_stage[q];
  const bool solved = st.device_rc == VIO_OK;
  bool result;
  if (e->init_device == 2) {
    result = solved ? finish_sfm_problem(e, s, st) : solve_initial(e, s, st);
  } else {
    for (size_t j = 0; solved && j < st.sfm_f.size(); j++)
      if (st.sfm_f[j].state) memcpy(st.sfm_f[j].position, &st.points[3 * j], 24);
    result = solve_initial_tail(e, s, st, solved ? st.verdict != 0 : init::bundle_adjust(e->W + 1, st.l, st.cq, st.tc, st.sfm_f, nullptr));
  }
  e->init_device_count[q] += solved;
  end_startup(fc, q, result);
}

void fill_problem(InitStage &st, int P, VioInitBaProblem &p) {
  p.frame_num = P, p.l = st.l, p.n_points = (int32_t)st.sfm_f.size();
  p.c_rotation = st.cq.data(), p.c_translation = st.tc.data(), p.points = st.points.data();
  p.point_ok = st.ok.data(), p.feat_start = st.start.data(), p.obs_frame = st.frame.data(), p.obs_xy = st.xy.data(), p.ok = 0;
}
void fill_problem(InitStage &st, int P, VioInitSfmProblem &p) {  // (p comes zeroed)
  p.frame_num = P, p.l = st.l, p.n_features = (int32_t)st.sfm_f.size();
  p.feat_start = st.start.data(), p.obs_frame = st.frame.data(), p.obs_xy = st.xy.data();
  p.relative_mode = st.mode, p.R_hint = st.hint;
  memcpy(p.relative_R, st.relative_R, sizeof(p.relative_R)), memcpy(p.relative_T, st.relative_T, sizeof(p.relative_T));
  p.n_extra = (int32_t)st.ex_start.size() - 1, p.extra_guess = st.ex_guess.data(), p.extra_start = st.ex_start.data();
  p.extra_feature = st.ex_feature.data(), p.extra_xy = st.ex_xy.data();
  p.q = st.q.data(), p.T = st.T.data(), p.points = st.points.data(), p.point_ok = st.ok.data();
  p.extra_R = st.ex_R.data(), p.extra_T = st.ex_T.data();
}

// The device call for the sequences of [q0, q1) that wait for it (main thread): collect them in ascending order, the context at
// first use, fill the problems, ONE solve, device_rc and the verdicts back, resume on the pool. The level is the estimator's, so
// all of them wait for the same solve (sfm: vio_init_sfm_solve, else vio_init_ba_solve); the other level's vector stays empty.
void run_startup_batch(const FrameCall &fc, int q0, int q1) {
  vio_estimator *e = fc.e;
  const int P = e->W + 1, np = fc.ba_max_points, no = fc.ba_max_obs;
  const bool sfm = e->init_device == 2;
  std::vector<int> wait;
  for (int q = q0; q < q1; q++)
    if (e->init_wait[q]) wait.push_back(q), e->init_wait[q] = 0;
  if (wait.empty()) return;
  const size_t n = wait.size();
  int rc = (sfm ? vio_init_sfm_create && vio_init_sfm_solve : vio_init_ba_create && vio_init_ba_solve) ? VIO_OK : VIO_ENODEV;
  if (rc == VIO_OK && !(sfm ? (void *)e->init_sfm : (void *)e->init_ba)) {
    rc = sfm ? vio_init_sfm_create(e->n_seq, P, np, no, fc.sfm_max_extra, &e->init_sfm) : vio_init_ba_create(e->n_seq, P, np, no, &e->init_ba);
    if (rc != VIO_OK)
      fprintf(stderr, "vio_amd: no device context for the %s (%d): it runs on the host\n", sfm ? "start-up structure from motion" : "initial bundle adjustment", rc);
  }
  std::vector<VioInitSfmProblem> ps(sfm ? n : 0);
  std::vector<VioInitBaProblem> pb(sfm ? 0 : n);
  for (size_t i = 0; i < n; i++) sfm ? fill_problem(e->init_stage[wait[i]], P, ps[i]) : fill_problem(e->init_stage[wait[i]], P, pb[i]);
  if (rc == VIO_OK) rc = sfm ? vio_init_sfm_solve(e->init_sfm, ps.data(), (int32_t)n, nullptr) : vio_init_ba_solve(e->init_ba, pb.data(), (int32_t)n, nullptr);
  for (size_t i = 0; i < n; i++) e->init_stage[wait[i]].device_rc = rc, e->init_stage[wait[i]].verdict = sfm ? ps[i].status : pb[i].ok;
  HostPool::get().parallel_for((int)n, [&](int i) { resume_startup(fc, wait[i]); });
}
}  // namespace
