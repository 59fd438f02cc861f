// est_resident.h — part of vio_estimator.cpp: sequences whose landmark list lives on the device. Restates VINS::processImage for a
// NON_LINEAR sequence (VINS.cpp:377-478) with f_manager's work (addFeatureCheckParallax, triangulate, the factor list :528-637,
// slideWindowOld / New :1239-1273) done by the store of the sequence's back-end (vio_resident.h); moving a list to the device and
// back has no counterpart in the reference.
#pragma once
#include "est_window.h"

// (a weak reference like those of est_startup.h: the store's keyframe pass, vio_resident.h, is a C++ entry of vio_backend.hip)
__attribute__((weak)) int vio_backend_resident_keyframe(vio_backend_t *, int32_t, const int32_t *, const int32_t *, const double *const *,
                                                        const double *const *, const double *, int32_t, int32_t *, float *, float *, double *,
                                                        int32_t *);
__attribute__((weak)) int vio_backend_resident_keyframe_cam(vio_backend_t *, int32_t, const int32_t *, const int32_t *, const double *const *,
                                                            const double *const *, const double *, int32_t, int32_t, int32_t *, float *, float *,
                                                            double *, int32_t *);
// (weak as well: only an estimator some sequence of which was given a camera of its own calls these)
__attribute__((weak)) int vio_backend_resident_set_cameras(vio_backend_t *, int32_t, const int32_t *, const double *);
extern "C" __attribute__((weak)) int vio_backend_upload_cam(vio_backend_t *, const VioWindow *, int32_t, const double *);

namespace {
// ---- device-resident sequences (vio_resident.h) --------------------------------------------------------------------------
int group_of(const vio_estimator *e, const Sequence &s) { return s.index / e->group_size; }
int slot_of(const vio_estimator *e, const Sequence &s) { return s.index % e->group_size; }

bool resident_eligible(const vio_estimator *e, const Sequence &s) {
  // (a relocalization frame with more matched ids than a store slot takes stays with the host-side list while the frame
  // is in the window, VINS.cpp:571-596)
  const bool reloc = (int)s.retrive.ids.size() > 256 && s.retrive.header >= s.Headers[0];
  return e->resident && e->resident_priors && s.solver_flag == VIO_SOLVER_NON_LINEAR && s.frame_count == e->W && !reloc && !s.failure_occur;
}

// The group's store exists (reserved at the first promotion). Main thread: HIP calls.
int ensure_store(vio_estimator *e, int g) {
  if (!e->be[g]) return VIO_ESTATE;
  int lcap = 0, ocap = 0;
  if (vio_backend_resident_caps(e->be[g], &lcap, &ocap) == VIO_OK) return VIO_OK;
  // A frame may bring twice the tracker's feature budget; the list holds a window's worth of frames whose features were
  // all new (a sequence that tracks nothing fails the failure detection long before: last_track_num < 4). A list that
  // outgrows its slot ends the frame with VIO_ECAP for that sequence, which restarts.
  e->res_obs_cap = std::min(1024, std::max(256, 2 * e->cfg.max_corners));
  // (the last term: store_pack scans its (W + 2)^2 bucket keys through a landmark-sized array, vio_backend_resident_reserve)
  e->res_list_cap = std::max({1024, (e->W + 2) * e->cfg.max_corners, e->res_obs_cap, (e->W + 2) * (e->W + 2)});
  double ex[7];
  extrinsic_pose(e->tic, e->ric, ex);  // (every slot starts with the context's camera: promote_group brings a sequence's own)
  const int rc = vio_backend_resident_reserve(e->be[g], e->group_size, e->res_list_cap, e->res_obs_cap, ex, e->tic, e->ric);
  if (rc != VIO_OK) e->resident = false;  // (a window size the store does not take, or no memory: every sequence stays on the host-side lists)
  return rc;
}

// The landmark lists of these sequences (ascending, one group) move to their slots of the group's back-end: dumped in
// parallel, uploaded together. A list that does not fit its slot stays on the host.
void promote_group(vio_estimator *e, int g, const std::vector<int> &seqs) {
  if (seqs.empty() || ensure_store(e, g) != VIO_OK) return;
  const int n = (int)seqs.size();
  std::vector<std::vector<VioFeatureInfo>> infos(n);
  std::vector<std::vector<double>> pts(n);
  std::vector<int> ok(n, 0);
  HostPool::get().parallel_for(n, [&](int k) {
    Sequence &s = e->seq[seqs[k]];
    int cnt = 0, np = 0;
    if (vio_features_dump(s.fm, nullptr, 0, &cnt, nullptr, 0, &np) != VIO_OK || cnt > e->res_list_cap) return;
    infos[k].resize(cnt + 1), pts[k].resize(3 * (size_t)np + 3);
    if (vio_features_dump(s.fm, infos[k].data(), cnt, &cnt, pts[k].data(), np, &np) != VIO_OK) return;
    infos[k].resize(cnt);
    ok[k] = 1;
  });
  std::vector<int32_t> slots, counts;
  std::vector<const VioFeatureInfo *> ip;
  std::vector<const double *> pp;
  std::vector<double> lp, lr;
  std::vector<int> who;
  for (int k = 0; k < n; k++) {
    if (!ok[k]) continue;
    Sequence &s = e->seq[seqs[k]];
    slots.push_back(slot_of(e, s)), counts.push_back((int32_t)infos[k].size()), ip.push_back(infos[k].data()), pp.push_back(pts[k].data());
    lp.insert(lp.end(), s.last_P, s.last_P + 3), lr.insert(lr.end(), s.last_R, s.last_R + 9);
    who.push_back(seqs[k]);
  }
  if (who.empty()) return;
  if (e->any_camera) {  // the slots' cameras first: the store kernels of the next frame read them
    std::vector<double> rec;
    for (int q : who) {
      const Sequence &s = e->seq[q];
      double ex[7];
      extrinsic_pose(s.cam.tic, s.cam.ric, ex);
      rec.insert(rec.end(), ex, ex + 7), rec.insert(rec.end(), s.cam.tic, s.cam.tic + 3), rec.insert(rec.end(), s.cam.ric, s.cam.ric + 9);
      rec.push_back(s.cam.fx / 1.5);  // ProjectionFactor::sqrt_info of the sequence's camera (VINS.cpp:31)
    }
    if (!vio_backend_resident_set_cameras || vio_backend_resident_set_cameras(e->be[g], (int)who.size(), slots.data(), rec.data()) != VIO_OK) return;
  }
  if (vio_backend_resident_load_batch(e->be[g], (int)who.size(), slots.data(), ip.data(), counts.data(), pp.data(), lp.data(), lr.data()) != VIO_OK)
    return;
  for (int q : who) {
    Sequence &s = e->seq[q];
    vio_features_clear(s.fm);
    s.pre_dirty.assign(e->W + 1, 1);
    s.on_device = true;
  }
}

// ... and back: the host-side list takes over again (relocalization, a caller that wants to look at the list).
int demote(vio_estimator *e, Sequence &s) {
  if (!s.on_device) return VIO_OK;
  const int g = group_of(e, s);
  int n = 0, np = 0;
  int rc = vio_backend_resident_fetch(e->be[g], slot_of(e, s), nullptr, 0, &n, nullptr, 0, &np);
  if (rc != VIO_OK) return rc;
  std::vector<VioFeatureInfo> info(n + 1);
  std::vector<double> pts(3 * (size_t)np + 3);
  rc = vio_backend_resident_fetch(e->be[g], slot_of(e, s), info.data(), n + 1, &n, pts.data(), np + 1, &np);
  if (rc != VIO_OK) return rc;
  rc = vio_features_load(s.fm, info.data(), n, pts.data());
  if (rc != VIO_OK) return rc;
  s.on_device = false;
  // the intervals the device integrated: integrate them here again from the buffered samples (the same operations in the
  // same order as the incremental propagation: the same bits)
  for (int i = 1; i <= e->W; i++)
    if (s.pre_stale[i]) {
      const double ba[3] = {s.pre[i].ba[0], s.pre[i].ba[1], s.pre[i].ba[2]}, bg[3] = {s.pre[i].bg[0], s.pre[i].bg[1], s.pre[i].bg[2]};
      repropagate(e, s, i, ba, bg);
      s.pre_stale[i] = 0, s.pre_merge[i] = 0;
    }
  return VIO_OK;
}

// double2vector of a window solved on the resident path: the results take the places unpack_window gives them on the host
// path and take_solution runs as it does there (the relocalization bookkeeping included; the landmarks took their depths
// in store_finish).
void take_resident_solution(vio_estimator *e, Sequence &s, const VioResidentResult &r, VioPrior &next) {
  const int P = e->W + 1;
  memcpy(s.pose.data(), r.pose, sizeof(double) * 7 * P), memcpy(s.sb.data(), r.speed_bias, sizeof(double) * 9 * P);
  if (r.raw_pose) memcpy(s.raw_pose.data(), r.raw_pose, sizeof(double) * 7 * P);
  if (r.loop_pose && r.n_loop_factors > 0) memcpy(s.loop_pose, r.loop_pose, sizeof(s.loop_pose));
  take_solution(e, s, r.n_features, &next, r.stats);
}

// The pool's first part of resident_frame: the frame of resident sequence q into its group's staging; the outcome goes to res_rc[q].
void stage_resident_frame(const FrameCall &fc, int q) {
  vio_estimator *e = fc.e;
  const int W = e->W;
  Sequence &s = e->seq[q];
  vio_backend_t *be = e->be[group_of(e, s)];
  const int slot = slot_of(e, s);
  int r = obs_count_ok(fc.n_obs[q], fc.obs_stride) ? VIO_OK : VIO_EINVAL;
  s.Headers[s.frame_count] = fc.headers[q];
  fill_pose_arrays(e, s);
  VioPreintegration blk;
  for (int k = 1; k <= W && r == VIO_OK; k++) {
    if (!s.pre_dirty[k] && k != W) continue;  // (the newest interval is new with every frame)
    if (!s.pre_valid[k]) {
      r = VIO_ESTATE;
      break;
    }
    if (s.pre_stale[k]) {
      // the device integrates: the whole of the newest interval, or the samples an older one absorbed at a non-keyframe slide
      const int ns = (int)s.dt_buf[k].size();
      const bool fresh = k == W || s.pre_merge[k] <= 0 || s.pre_merge[k] >= ns;
      const int first = fresh ? 0 : ns - s.pre_merge[k];
      int ri = VIO_ECAP;
      if (k == W || s.pre_merge[k] > 0)
        ri = vio_backend_resident_stage_imu(be, slot, k - 1, fresh ? 1 : 0, &s.lin_acc[3 * k], &s.lin_gyr[3 * k], s.pre[k].ba, s.pre[k].bg,
                                            ns - first, s.dt_buf[k].data() + first, s.acc_buf[k].data() + 3 * first,
                                            s.gyr_buf[k].data() + 3 * first);
      if (ri == VIO_ECAP) {  // (no room for the samples, or a stale interval whose new samples are not known: the block instead)
        host::Preint tmp = s.pre[k];
        host::preint_init(tmp, &e->cfg, &s.lin_acc[3 * k], &s.lin_gyr[3 * k], s.pre[k].ba, s.pre[k].bg);
        for (int i = 0; i < ns; i++) host::propagate(tmp, s.dt_buf[k][i], &s.acc_buf[k][3 * i], &s.gyr_buf[k][3 * i]);
        host::preint_export(tmp, &blk);
        ri = vio_backend_resident_stage_preint(be, slot, k - 1, &blk, tmp.acc_0, tmp.gyr_0);
      }
      r = ri;
      s.pre_merge[k] = 0;
    } else {
      host::preint_export(s.pre[k], &blk);
      r = vio_backend_resident_stage_preint(be, slot, k - 1, &blk, s.pre[k].acc_0, s.pre[k].gyr_0);
    }
    s.pre_dirty[k] = 0;
  }
  select_loop_frame(s, W);
  if (r == VIO_OK)
    r = vio_backend_resident_stage(be, slot, fc.obs_of(q), fc.n_obs[q], s.Ps.data(), s.Rs.data(), s.pose.data(), s.sb.data(),
                                   s.has_prior ? &s.prior[s.cur_prior].p : nullptr, s.loop_frame, s.front.ids.data(), s.front.xy.data(),
                                   (int)s.front.ids.size());
  e->res_rc[q] = r;
}

// ... and its second part, behind the device: double2vector, prior header, failure / slide of the host-side states.
void finish_resident_frame(const FrameCall &fc, int q) {
  vio_estimator *e = fc.e;
  Sequence &s = e->seq[q];
  VioFrameResult &res = fc.results[q];
  VioResidentResult r;
  VioPrior &next = s.prior[1 - s.cur_prior].p;
  int rr = e->res_rc[q];
  if (rr == VIO_OK) rr = vio_backend_resident_result(e->be[group_of(e, s)], slot_of(e, s), &r, &next);
  if (rr == VIO_OK) rr = r.status;
  if (rr != VIO_OK) return restart_with_error(e, s, res, rr);  // (not staged, or the store refused the frame: the slot's list is undefined now)
  s.marginalization_flag = r.marginalization_flag, s.last_track_num = r.track_num;
  res.marginalization_flag = r.marginalization_flag, res.track_num = r.track_num;
  res.n_features = r.n_features, res.n_factors = r.n_factors, res.n_loop_factors = r.n_loop_factors;
  res.stats = r.stats;
  s.n_loop_factors = r.n_loop_factors;
  if (s.n_loop_factors > 0) s.loop_enable = true;
  if (s.loop_frame >= 0 && s.n_loop_factors == 0) s.loop_frame = -1;  // a loop pose without factors is a free block (build_window)
  take_resident_solution(e, s, r, next);
  s.failure_occur = 0;
  finish_nonlinear_frame(e, s, res, r.failure_reasons);
}

// One published frame of every resident sequence: what processImage does with it, with the landmark work on the device.
//   main thread   begin (per group)
//   pool          per sequence: para_Pose / para_SpeedBias, the pre-integration blocks that changed, the observations -> staging
//   main thread   ingest (H2D + store_ingest, per group, no wait), then launch per group (waits for the group's counts:
//                 layout, store_pack, window kernel, store_finish, results queued), then collect per group
//   pool          per sequence: double2vector, prior header, failure / slide of the host-side states
int resident_frame(const FrameCall &fc) {
  vio_estimator *e = fc.e;
  std::vector<char> in_group(e->n_groups, 0);
  std::vector<int> todo;
  for (int q = 0; q < e->n_seq; q++) {
    Sequence &s = e->seq[q];
    if (!s.on_device || (fc.active && !fc.active[q])) continue;
    in_group[group_of(e, s)] = 1;
    todo.push_back(q);
  }
  if (todo.empty()) return VIO_OK;
  int rc = VIO_OK;
  const auto each_group = [&](int (*step)(vio_backend_t *)) {  // (until the first error)
    for (int g = 0; g < e->n_groups && rc == VIO_OK; g++)
      if (in_group[g]) rc = step(e->be[g]);
  };
  each_group(vio_backend_resident_begin);
  e->res_rc.assign(e->n_seq, VIO_OK);
  if (rc == VIO_OK) HostPool::get().parallel_for((int)todo.size(), [&](int i) { stage_resident_frame(fc, todo[i]); });
  each_group(vio_backend_resident_ingest), each_group(vio_backend_resident_launch);
  for (int g = 0; g < e->n_groups; g++)  // (every group that began is brought back to idle, also after an error in another)
    if (in_group[g]) {
      const int rcc = vio_backend_resident_collect(e->be[g]);
      if (rc == VIO_OK && rcc != VIO_ESTATE) rc = rcc;
    }
  if (rc != VIO_OK) {  // device error: the stores may or may not have advanced; every sequence of this path restarts
    for (int q : todo) restart_with_error(e, e->seq[q], fc.results[q], rc);
    return rc;
  }
  HostPool::get().parallel_for((int)todo.size(), [&](int i) { finish_resident_frame(fc, todo[i]); });
  // (all sequences, not `todo` alone: an error of the host path has been counted by then and outranks this one in the caller)
  return first_error_of(fc.results, 0, e->n_seq, VIO_OK);
}
}  // namespace
