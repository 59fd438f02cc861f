// be_resident.h — part of vio_backend.hip: the entry points of the device-resident path (vio_resident.h). The store kernels
// (vio_store.h) ingest, pack and finish a frame of every slot on the device; the windows they pack run through the plan, the
// work buffers and the launch function that the host-window path uses (wk_plan.h, be_work.h).
#pragma once
#include "be_work.h"

static vio::StoreDev resident_store_dev(vio_backend *be) {
  vio_resident *r = be->res.get();
  vio::StoreDev S;
  S.d = r->sd, S.n_slots = r->n_slots;
  S.fid = r->fid.p, S.start = r->start.p, S.nobs = r->nobs.p, S.flag = r->flag.p, S.depth = r->depth.p, S.obs = r->obs.p;
  S.ctl = r->ctl.p, S.ctld = r->ctld.p;
  S.active = r->dp<int>(r->o_active), S.n_obs = r->dp<int>(r->o_nobs), S.obs_in = r->dp<VioObs>(r->o_obs), S.obs_off = r->dp<int>(r->o_obsoff);
  S.loop_frame = r->dp<int>(r->o_loopf), S.loop_n = r->dp<int>(r->o_loopn), S.loop_off = r->dp<int>(r->o_loopoff);
  S.loop_ids = r->dp<int>(r->o_loopids), S.loop_xy = r->dp<double>(r->o_loopxy);
  S.Ps = r->dp<double>(r->o_Ps), S.Rs = r->dp<double>(r->o_Rs);
  S.tic = r->consts.p + 7, S.ric = r->consts.p + 10, S.cam_stride = vio_resident::kCamDev;  // one record per slot
  S.preint = r->preint.p, S.pre_idx = r->dp<int>(r->o_preidx), S.pre_blk = r->dp<double>(r->o_preblk);
  S.n_pre = r->n_pre.load();
  S.imu_jobs = r->dp<double>(r->o_jobs), S.imu_samples = r->dp<double>(r->o_samples), S.n_imu_jobs = r->n_jobs.load();
  S.pre_side = r->pre_side.p, S.noise = r->consts.p + (size_t)r->n_slots * vio_resident::kCamDev;
  S.prof = nullptr;
  static const bool prof = vio::env_flag("VIO_AMD_STORE_PROF");
  if (prof && r->prof.ensure(32) == VIO_OK) S.prof = r->prof.p;
  return S;
}

int vio_backend_resident_reserve(vio_backend_t *be, int32_t n_slots, int32_t list_cap, int32_t obs_cap, const double ex_pose[7],
                                 const double tic[3], const double ric[9]) {
  if (!be || n_slots < 1 || n_slots > be->max_batch || list_cap < 16 || obs_cap < 1 || !ex_pose || !tic || !ric) return VIO_EINVAL;
  const int W = be->cfg.window_size, P = W + 1;
  if (P > vio::store::kMaxP || P > 255) return VIO_ECAP;
  // landmark-sized LDS arrays double as scratch: the observation ingest needs obs_cap entries, store_pack scans its (P + 1)^2
  // (host, target) bucket keys through scanA[0 .. nkeys] (an array of list_cap + 1 ints with scanB right behind it)
  if ((P + 1) * (P + 1) > list_cap || obs_cap > list_cap) return VIO_EINVAL;
  {  // the store kernels keep a sequence's scan arrays in LDS: the whole of it must fit one CU at the largest factor capacity
    vio::store::Dims sd;
    sd.W = W, sd.Lcap = list_cap, sd.Ocap = obs_cap;
    if (list_cap > 65535 || vio::store_pack_lds_bytes(sd, be->cfg.max_factors) > vio_wk::kLdsLimit) return VIO_ECAP;
  }
  VIO_ON_DEVICE_OF(be);
  HIP_OK(hipStreamSynchronize(be->last_stream ? be->last_stream : be->stream));
  if (be->st_n == 0) {
    const int rc = vio_backend_reserve_priors(be, n_slots);
    if (rc != VIO_OK) return rc;
  } else if (be->st_n < n_slots) {
    return VIO_EINVAL;
  }
  be->res.reset();
  std::unique_ptr<vio_resident> r(new (std::nothrow) vio_resident());
  if (!r) return VIO_ENOMEM;
  try {
    r->n_slots = n_slots, r->W = W, r->P = P;
    r->sd.W = W, r->sd.Lcap = list_cap, r->sd.Ocap = obs_cap;
    const size_t N = n_slots, L = (size_t)list_cap;
    int rc = VIO_OK;
    DevBuf<int> *ib[] = {&r->fid, &r->start, &r->nobs, &r->flag};
    for (auto *b : ib)
      if (rc == VIO_OK) rc = b->ensure(2 * N * L);
    if (rc == VIO_OK) rc = r->depth.ensure(2 * N * L);
    if (rc == VIO_OK) rc = r->obs.ensure(2 * N * L * P * 3);
    if (rc == VIO_OK) rc = r->ctl.ensure(N * vio::store::C_COUNT);
    if (rc == VIO_OK) rc = r->ctld.ensure(N * vio::store::kCtlDoubles);
    if (rc == VIO_OK) rc = r->preint.ensure(N * W * kPreintDoubles);
    if (rc == VIO_OK) rc = r->consts.ensure(N * vio_resident::kCamDev + 18);
    if (rc == VIO_OK) rc = r->pre_side.ensure(N * W * vio::preint::kSide);
    if (rc == VIO_OK) rc = r->b_dummy.ensure(16);
    if (rc != VIO_OK) return rc;
    HIP_OK(hipMemset(r->ctl.p, 0, N * vio::store::C_COUNT * sizeof(int)));
    HIP_OK(hipMemset(r->preint.p, 0, N * W * kPreintDoubles * sizeof(double)));
    // every slot starts with the context's camera; a sequence with its own brings it along (vio_backend_resident_set_cameras)
    r->cam_rec.assign(N * vio_resident::kCamRec, 0.0);
    for (size_t b = 0; b < N; b++) {
      double *rec = &r->cam_rec[b * vio_resident::kCamRec];
      memcpy(rec, ex_pose, 56), memcpy(rec + 7, tic, 24), memcpy(rec + 10, ric, 72);
      rec[19] = be->cfg.fx / 1.5;  // ProjectionFactor::sqrt_info (VINS.cpp:31)
    }
    std::vector<double> cv(N * vio_resident::kCamDev + 18);
    for (size_t b = 0; b < N; b++) memcpy(&cv[b * vio_resident::kCamDev], &r->cam_rec[b * vio_resident::kCamRec], sizeof(double) * vio_resident::kCamDev);
    {  // noise diagonal of the pre-integration, integration_base.h:30-36 (vio_preint.h preint_init)
      const VioConfig &cf = be->cfg;
      const double an = cf.acc_n * cf.acc_n, gn = cf.gyr_n * cf.gyr_n, aw = cf.acc_w * cf.acc_w, gw = cf.gyr_w * cf.gyr_w;
      double *c = &cv[N * vio_resident::kCamDev];
      for (int k = 0; k < 3; k++) c[k] = an, c[3 + k] = gn, c[6 + k] = an, c[9 + k] = gn, c[12 + k] = aw, c[15 + k] = gw;
    }
    HIP_OK(hipMemset(r->pre_side.p, 0, N * W * vio::preint::kSide * sizeof(double)));
    memcpy(r->ex_pose, ex_pose, 56);
    HIP_OK(hipMemcpy(r->consts.p, cv.data(), sizeof(double) * cv.size(), hipMemcpyHostToDevice));
    // staging layout: ints, doubles, observations, then the pre-integration blocks (only the ones in use travel)
    size_t o = 0;
    auto place = [&](size_t bytes) {
      const size_t at = o;
      o = (o + bytes + 255) & ~(size_t)255;
      return at;
    };
    r->o_active = place(N * 4), r->o_nobs = place(N * 4), r->o_hdr = place(N * kHdrInts * 4);
    r->o_prk = place(N * kMaxPriorBlocks * 4), r->o_pri = place(N * kMaxPriorBlocks * 4), r->o_pro = place(N * kMaxPriorBlocks * 4);
    r->o_preidx = place(N * W * 4);
    r->o_hdrd = place(N * kHdrDoubles * 8), r->o_pose = place(N * 7 * P * 8), r->o_sb = place(N * 9 * P * 8), r->o_ex = place(N * 7 * 8);
    r->o_Ps = place(N * 3 * P * 8), r->o_Rs = place(N * 9 * P * 8);
    r->o_obsoff = place(N * 4);
    r->o_loopf = place(N * 4), r->o_loopn = place(N * 4), r->o_loopoff = place(N * 4);
    r->o_obs = place(N * obs_cap * sizeof(VioObs));
    r->cap_loop = (int)(N * kResidentLoopIds);
    r->o_loopids = place((size_t)r->cap_loop * 4);
    r->o_loopxy = place((size_t)r->cap_loop * 16);
    r->cap_jobs = (int)(N * W), r->cap_samples = (int)(N * 64);
    r->o_jobs = place((size_t)r->cap_jobs * 16 * 8);
    r->o_samples = place((size_t)r->cap_samples * 7 * 8);
    r->o_preblk = place(N * W * (kPreintDoubles + 6) * 8);
    r->total_bytes = o;
    r->h_in.assign(o, 0);
    rc = r->d_in.ensure(o);
    if (rc != VIO_OK) return rc;
    HIP_OK(hipMemset(r->d_in.p, 0, o));
    for (size_t b = 0; b < N; b++) memcpy(r->hp<double>(r->o_ex) + 7 * b, ex_pose, 56);
    r->h_ctl.assign(N * vio::store::C_COUNT, 0);
    r->solved.assign(N, 0);
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
  be->res = std::move(r);
  be->uploaded = false;
  return VIO_OK;
}

int vio_backend_set_peers(vio_backend_t *be, int32_t peers) {
  if (!be || peers < 1) return VIO_EINVAL;
  be->peers = peers;
  return VIO_OK;
}

// The cameras of n slots (any order, distinct): rec[k] = ex_pose 7 | tic 3 | ric 9 | sqrt_info of slot slots[k]. Between two frames
// only. The extrinsic the window kernel reads is staged per slot with every frame; the store kernels' records go up here.
int vio_backend_resident_set_cameras(vio_backend_t *be, int32_t n, const int32_t *slots, const double *rec) {
  if (!be || !be->res) return VIO_ESTATE;
  vio_resident *r = be->res.get();
  if (n < 0 || (n > 0 && (!slots || !rec))) return VIO_EINVAL;
  if (r->phase != 0) return VIO_ESTATE;
  if (n == 0) return VIO_OK;
  constexpr int R = vio_resident::kCamRec, D = vio_resident::kCamDev;
  for (int k = 0; k < n; k++) {
    if (slots[k] < 0 || slots[k] >= r->n_slots) return VIO_EINVAL;
    for (int i = 0; i < R; i++)
      if (!std::isfinite(rec[(size_t)k * R + i])) return VIO_EINVAL;
    if (!(rec[(size_t)k * R + 19] > 0)) return VIO_EINVAL;
  }
  VIO_ON_DEVICE_OF(be);
  HIP_OK(hipStreamSynchronize(be->last_stream ? be->last_stream : be->stream));  // (a keyframe pass may still read the records)
  HIP_OK(hipStreamSynchronize(be->stream));
  for (int k = 0; k < n; k++) {
    const size_t b = slots[k];
    memcpy(&r->cam_rec[b * R], rec + (size_t)k * R, sizeof(double) * R);
    memcpy(r->hp<double>(r->o_ex) + 7 * b, rec + (size_t)k * R, 56);
  }
  // one copy of the whole table of records (19 doubles per slot; the IMU noise behind it stays)
  std::vector<double> dev((size_t)r->n_slots * D);
  for (size_t b = 0; b < (size_t)r->n_slots; b++) memcpy(&dev[b * D], &r->cam_rec[b * R], sizeof(double) * D);
  HIP_OK(hipMemcpy(r->consts.p, dev.data(), sizeof(double) * dev.size(), hipMemcpyHostToDevice));
  return VIO_OK;
}

int vio_backend_resident_caps(const vio_backend_t *be, int32_t *list_cap, int32_t *obs_cap) {
  if (!be || !be->res) return VIO_ESTATE;
  if (list_cap) *list_cap = be->res->sd.Lcap;
  if (obs_cap) *obs_cap = be->res->sd.Ocap;
  return VIO_OK;
}

// n lists at once (the sequences of a group usually reach the NON_LINEAR state in the same frame): the arrays are staged
// slot by slot at a common pitch and go up with one strided copy per array and run of consecutive slots, not eight small
// synchronous copies per sequence.
int vio_backend_resident_load_batch(vio_backend_t *be, int32_t n, const int32_t *slots, const VioFeatureInfo *const *infos,
                                    const int32_t *counts, const double *const *points, const double *last_P /* [n][3] */,
                                    const double *last_R /* [n][9] */) {
  if (!be || !be->res) return VIO_ESTATE;
  vio_resident *r = be->res.get();
  if (n < 0 || (n > 0 && (!slots || !infos || !counts || !points || !last_P || !last_R))) return VIO_EINVAL;
  if (n == 0) return VIO_OK;
  if (r->phase != 0) return VIO_ESTATE;
  const int P = r->P;
  const size_t L = r->sd.Lcap;
  int maxn = 1;
  for (int k = 0; k < n; k++) {
    if (slots[k] < 0 || slots[k] >= r->n_slots || counts[k] < 0 || (counts[k] > 0 && (!infos[k] || !points[k]))) return VIO_EINVAL;
    if (k > 0 && slots[k] <= slots[k - 1]) return VIO_EINVAL;  // ascending, distinct
    if (counts[k] > (int)L) return VIO_ECAP;
    maxn = std::max(maxn, counts[k]);
    for (int i = 0; i < counts[k]; i++) {
      const VioFeatureInfo &f = infos[k][i];
      if (f.n_obs < 1 || f.n_obs > P || f.start_frame < 0 || f.start_frame + f.n_obs - 1 > r->W) return VIO_EINVAL;
    }
  }
  VIO_ON_DEVICE_OF(be);
  try {
    const size_t pitch = maxn, N = n;
    std::vector<int> fid(N * pitch), start(N * pitch), nobs(N * pitch), flag(N * pitch), ctl(N * vio::store::C_COUNT, 0);
    std::vector<double> depth(N * pitch), obs(N * pitch * P * 3), cd(N * vio::store::kCtlDoubles);
    vio::HostPool::get().parallel_for(n, [&](int k) {
      size_t p = 0;
      for (int i = 0; i < counts[k]; i++) {
        const VioFeatureInfo &f = infos[k][i];
        const size_t e = k * pitch + i;
        fid[e] = f.id, start[e] = f.start_frame, nobs[e] = f.n_obs, flag[e] = f.solve_flag, depth[e] = f.estimated_depth;
        memcpy(&obs[e * P * 3], points[k] + 3 * p, sizeof(double) * 3 * f.n_obs);
        p += f.n_obs;
      }
      ctl[(size_t)k * vio::store::C_COUNT + vio::store::C_N] = counts[k];
      memcpy(&cd[(size_t)k * vio::store::kCtlDoubles], last_P + 3 * k, 24);
      memcpy(&cd[(size_t)k * vio::store::kCtlDoubles + 3], last_R + 9 * k, 72);
    });
    HIP_OK(hipStreamSynchronize(be->stream));
    for (int k0 = 0; k0 < n;) {  // runs of consecutive slots (bank 0)
      int k1 = k0 + 1;
      while (k1 < n && slots[k1] == slots[k1 - 1] + 1) k1++;
      const size_t rows = k1 - k0, e = (size_t)slots[k0] * L, h = k0 * pitch;
      HIP_OK(hipMemcpy2D(r->fid.p + e, L * 4, fid.data() + h, pitch * 4, pitch * 4, rows, hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy2D(r->start.p + e, L * 4, start.data() + h, pitch * 4, pitch * 4, rows, hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy2D(r->nobs.p + e, L * 4, nobs.data() + h, pitch * 4, pitch * 4, rows, hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy2D(r->flag.p + e, L * 4, flag.data() + h, pitch * 4, pitch * 4, rows, hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy2D(r->depth.p + e, L * 8, depth.data() + h, pitch * 8, pitch * 8, rows, hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy2D(r->obs.p + e * P * 3, L * P * 24, obs.data() + h * P * 3, pitch * P * 24, pitch * P * 24, rows, hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(r->ctl.p + (size_t)slots[k0] * vio::store::C_COUNT, ctl.data() + (size_t)k0 * vio::store::C_COUNT,
                       rows * vio::store::C_COUNT * sizeof(int), hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(r->ctld.p + (size_t)slots[k0] * vio::store::kCtlDoubles, cd.data() + (size_t)k0 * vio::store::kCtlDoubles,
                       rows * vio::store::kCtlDoubles * sizeof(double), hipMemcpyHostToDevice));
      k0 = k1;
    }
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
  return VIO_OK;
}

int vio_backend_resident_load(vio_backend_t *be, int32_t slot, const VioFeatureInfo *info, int32_t n, const double *points,
                              const double last_P[3], const double last_R[9]) {
  if (n < 0 || (n > 0 && (!info || !points)) || !last_P || !last_R) return VIO_EINVAL;
  const int32_t slots[1] = {slot}, counts[1] = {n};
  const VioFeatureInfo *infos[1] = {info};
  const double *pts[1] = {points};
  return vio_backend_resident_load_batch(be, 1, slots, infos, counts, pts, last_P, last_R);
}

int vio_backend_resident_fetch(vio_backend_t *be, int32_t slot, VioFeatureInfo *info, int32_t cap, int32_t *n, double *points,
                               int32_t cap_points, int32_t *n_points) {
  if (!be || !be->res) return VIO_ESTATE;
  vio_resident *r = be->res.get();
  if (slot < 0 || slot >= r->n_slots || !n || cap < 0 || (cap > 0 && !info)) return VIO_EINVAL;
  if (r->phase != 0) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(be);
  HIP_OK(hipStreamSynchronize(be->stream));
  const int P = r->P;
  const size_t L = r->sd.Lcap;
  int ctl[vio::store::C_COUNT];
  HIP_OK(hipMemcpy(ctl, r->ctl.p + (size_t)slot * vio::store::C_COUNT, sizeof(ctl), hipMemcpyDeviceToHost));
  const int cnt = ctl[vio::store::C_N], bank = ctl[vio::store::C_BANK];
  try {
    std::vector<int> fid(cnt + 1), start(cnt + 1), nobs(cnt + 1), flag(cnt + 1);
    std::vector<double> depth(cnt + 1), obs((size_t)(cnt + 1) * P * 3);
    const size_t e = ((size_t)bank * r->n_slots + slot) * L;
    if (cnt > 0) {
      HIP_OK(hipMemcpy(fid.data(), r->fid.p + e, sizeof(int) * cnt, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(start.data(), r->start.p + e, sizeof(int) * cnt, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(nobs.data(), r->nobs.p + e, sizeof(int) * cnt, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(flag.data(), r->flag.p + e, sizeof(int) * cnt, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(depth.data(), r->depth.p + e, sizeof(double) * cnt, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(obs.data(), r->obs.p + e * P * 3, sizeof(double) * (size_t)cnt * P * 3, hipMemcpyDeviceToHost));
    }
    int np = 0;
    for (int i = 0; i < cnt; i++) np += nobs[i];
    *n = cnt;
    if (n_points) *n_points = np;
    if (cap == 0) return VIO_OK;  // count only
    if (cnt > cap || (points && np > cap_points)) return VIO_ECAP;
    size_t p = 0;
    for (int i = 0; i < cnt; i++) {
      VioFeatureInfo &o = info[i];
      memset(&o, 0, sizeof(o));
      o.id = fid[i], o.start_frame = start[i], o.n_obs = nobs[i], o.used_num = nobs[i], o.solve_flag = flag[i];
      o.estimated_depth = depth[i];
      if (points) memcpy(points + 3 * p, &obs[(size_t)i * P * 3], sizeof(double) * 3 * nobs[i]);
      p += nobs[i];
    }
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
  return VIO_OK;
}

int vio_backend_resident_keyframe(vio_backend_t *be, int32_t n, const int32_t *slots, const int32_t *rows, const double *const *Ps,
                                  const double *const *Rs, const double intr[4], int32_t stride, int32_t *ids, float *px, float *norm,
                                  double *cloud, int32_t *count) {
  return vio_backend_resident_keyframe_cam(be, n, slots, rows, Ps, Rs, intr, 0, stride, ids, px, norm, cloud, count);
}

// intr_stride: doubles between the intrinsics of two slots of the call (4: one camera per slot, 0: one for all)
int vio_backend_resident_keyframe_cam(vio_backend_t *be, int32_t n, const int32_t *slots, const int32_t *rows, const double *const *Ps,
                                      const double *const *Rs, const double *intr, int32_t intr_stride, int32_t stride, int32_t *ids,
                                      float *px, float *norm, double *cloud, int32_t *count) {
  if (!be || !be->res) return VIO_ESTATE;
  if (intr_stride != 0 && intr_stride != 4) return VIO_EINVAL;
  vio_resident *r = be->res.get();
  if (n < 0 || stride < 0 || (n > 0 && (!slots || !rows || !Ps || !Rs || !intr || !count)) || (n > 0 && stride > 0 && (!ids || !px || !norm || !cloud)))
    return VIO_EINVAL;
  if (n == 0) return VIO_OK;
  if (n > r->n_slots) return VIO_EINVAL;
  if (r->phase != 0) return VIO_ESTATE;
  const int P = r->P;
  try {
    std::vector<char> seen(r->n_slots, 0);
    for (int k = 0; k < n; k++) {
      if (slots[k] < 0 || slots[k] >= r->n_slots || seen[slots[k]] || rows[k] < 0 || !Ps[k] || !Rs[k]) return VIO_EINVAL;
      seen[slots[k]] = 1;
    }
    VIO_ON_DEVICE_OF(be);
    hipStream_t st = be->stream;
    // a list holds at most Lcap landmarks: device rows never need to be wider
    const int cap = std::max(1, std::min((int)stride, r->sd.Lcap));
    const size_t N = r->n_slots, T = (size_t)n * cap;
    int rc = r->kf_jobs.ensure(N);
    if (rc == VIO_OK) rc = r->kf_states.ensure(N * (12 * P + 4));  // (behind the states: fx fy cx cy of every job)
    if (rc == VIO_OK) rc = r->kf_out.ensure(44 * N * (size_t)r->sd.Lcap + 4 * N);
    if (rc != VIO_OK) return rc;
    r->kf_hjobs.assign(slots, slots + n);
    const size_t o_intr = (size_t)n * 12 * P;
    r->kf_hstates.resize(o_intr + (intr_stride ? 4 * (size_t)n : 0));
    for (int k = 0; k < n; k++) {
      memcpy(&r->kf_hstates[(size_t)k * 12 * P], Ps[k], sizeof(double) * 3 * P);
      memcpy(&r->kf_hstates[(size_t)k * 12 * P + 3 * P], Rs[k], sizeof(double) * 9 * P);
      if (intr_stride) memcpy(&r->kf_hstates[o_intr + 4 * (size_t)k], intr + (size_t)k * intr_stride, sizeof(double) * 4);
    }
    // the sections of the download: cloud | px | norm | ids | count
    const size_t o_cloud = 0, o_px = 24 * T, o_norm = 32 * T, o_ids = 40 * T, o_count = 44 * T, bytes = 44 * T + 4 * (size_t)n;
    if (r->kf_hout.size() < bytes) r->kf_hout.resize(bytes);
    unsigned char *D = r->kf_out.p, *Hb = r->kf_hout.data();
    HIP_OK(hipMemcpyAsync(r->kf_jobs.p, r->kf_hjobs.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(r->kf_states.p, r->kf_hstates.data(), sizeof(double) * r->kf_hstates.size(), hipMemcpyHostToDevice, st));
    vio::StoreKeyframe K;
    K.jobs = r->kf_jobs.p, K.states = r->kf_states.p, K.fx = intr[0], K.fy = intr[1], K.cx = intr[2], K.cy = intr[3], K.cap = cap;
    K.intr = intr_stride ? r->kf_states.p + o_intr : nullptr;
    K.cloud = (double *)(D + o_cloud), K.px = (float *)(D + o_px), K.norm = (float *)(D + o_norm), K.ids = (int *)(D + o_ids);
    K.count = (int *)(D + o_count);
    rc = vio::store_launch_keyframe(resident_store_dev(be), K, n, st);
    if (rc != VIO_OK) return rc;
    HIP_OK(hipMemcpyAsync(Hb, D, bytes, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const int *cnt = (const int *)(Hb + o_count);
    int out_rc = VIO_OK;
    for (int k = 0; k < n; k++) {
      const size_t src = (size_t)k * cap, dst = (size_t)rows[k] * stride;
      int c = cnt[k];
      if (c < 0) c = -c;                       // (the device row was narrower than the list: only when stride was)
      count[rows[k]] = c > stride ? -c : c;
      if (c > stride) out_rc = VIO_ECAP;
      const size_t m = (size_t)std::min(c, std::min(cap, (int)stride));
      if (m == 0) continue;
      memcpy(cloud + 3 * dst, Hb + o_cloud + 24 * src, 24 * m);
      memcpy(px + 2 * dst, Hb + o_px + 8 * src, 8 * m);
      memcpy(norm + 2 * dst, Hb + o_norm + 8 * src, 8 * m);
      memcpy(ids + dst, Hb + o_ids + 4 * src, 4 * m);
    }
    return out_rc;
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
}

int vio_backend_resident_begin(vio_backend_t *be) {
  if (!be || !be->res) return VIO_ESTATE;
  vio_resident *r = be->res.get();
  if (r->phase != 0) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(be);
  // the previous frame's copy out of the arena, and whatever the host-window path left running on this context
  HIP_OK(hipStreamSynchronize(be->last_stream ? be->last_stream : be->stream));
  HIP_OK(hipStreamSynchronize(be->stream));
  memset(r->hp<int>(r->o_active), 0, sizeof(int) * r->n_slots);
  r->n_pre.store(0), r->n_jobs.store(0), r->n_samples.store(0), r->n_obs_total.store(0), r->n_loop_total.store(0);
  r->any_loop = false;
  for (int k = 0; k < r->n_slots; k++) r->hp<int>(r->o_loopf)[k] = -1, r->hp<int>(r->o_loopn)[k] = 0, r->hp<int>(r->o_loopoff)[k] = 0;
  r->active_list.clear();
  std::fill(r->solved.begin(), r->solved.end(), 0);
  r->phase = 1;
  return VIO_OK;
}

int vio_backend_resident_stage(vio_backend_t *be, int32_t slot, const VioObs *obs, int32_t n_obs, const double *Ps, const double *Rs,
                               const double *pose, const double *speed_bias, const VioPrior *prior, int32_t loop_frame,
                               const int32_t *loop_ids, const double *loop_xy, int32_t n_loop) {
  if (!be || !be->res) return VIO_ESTATE;
  vio_resident *r = be->res.get();
  if (r->phase != 1) return VIO_ESTATE;
  if (slot < 0 || slot >= r->n_slots || n_obs < 0 || (n_obs > 0 && !obs) || !Ps || !Rs || !pose || !speed_bias) return VIO_EINVAL;
  if (n_obs > r->sd.Ocap) return VIO_ECAP;
  if (loop_frame >= r->W || n_loop < 0 || (loop_frame >= 0 && n_loop > 0 && (!loop_ids || !loop_xy))) return VIO_EINVAL;
  if (loop_frame >= 0 && n_loop > kResidentLoopIds) return VIO_ECAP;
  const int P = r->P;
  int *h = r->hp<int>(r->o_hdr) + (size_t)slot * kHdrInts;
  memset(h, 0, sizeof(int) * kHdrInts);
  h[H_W] = r->W, h[H_LOOP_FRAME] = -1;
  if (prior && prior->n > 0) {
    if (prior->n > be->st_ncap || prior->n_blocks > kMaxPriorBlocks || prior->n_blocks < 0) return VIO_ECAP;
    int nsb = 0;
    int *pk = r->hp<int>(r->o_prk) + (size_t)slot * kMaxPriorBlocks, *pi = r->hp<int>(r->o_pri) + (size_t)slot * kMaxPriorBlocks,
        *po = r->hp<int>(r->o_pro) + (size_t)slot * kMaxPriorBlocks;
    for (int k = 0; k < prior->n_blocks; k++) {
      const int kind = prior->block_kind[k], idx = prior->block_index[k], o = prior->block_offset[k];
      const int ls = kind == VIO_BLOCK_SPEEDBIAS ? 9 : 6;
      if (kind < 0 || kind > 2 || idx < 0 || idx >= P || o < 0 || o + ls > prior->n) return VIO_EINVAL;
      nsb += kind == VIO_BLOCK_SPEEDBIAS;
      pk[k] = kind, pi[k] = idx, po[k] = o;
    }
    if (nsb > 1) return VIO_EINVAL;
    h[H_PRIOR_N] = prior->n, h[H_PRIOR_NB] = prior->n_blocks;
  }
  memset(r->hp<double>(r->o_hdrd) + (size_t)slot * kHdrDoubles, 0, sizeof(double) * kHdrDoubles);
  r->hp<double>(r->o_hdrd)[(size_t)slot * kHdrDoubles + 4] = r->cam_rec[(size_t)slot * vio_resident::kCamRec + 19];  // sqrt_info of the slot's camera
  memcpy(r->hp<double>(r->o_pose) + (size_t)slot * 7 * P, pose, sizeof(double) * 7 * P);
  memcpy(r->hp<double>(r->o_sb) + (size_t)slot * 9 * P, speed_bias, sizeof(double) * 9 * P);
  memcpy(r->hp<double>(r->o_Ps) + (size_t)slot * 3 * P, Ps, sizeof(double) * 3 * P);
  memcpy(r->hp<double>(r->o_Rs) + (size_t)slot * 9 * P, Rs, sizeof(double) * 9 * P);
  {  // the observations of all slots are packed one after the other: only what there is travels
    const int off = r->n_obs_total.fetch_add(n_obs);
    if (n_obs) memcpy(r->hp<VioObs>(r->o_obs) + off, obs, sizeof(VioObs) * n_obs);
    r->hp<int>(r->o_obsoff)[slot] = off;
  }
  if (loop_frame >= 0 && n_loop > 0) {
    const int off = r->n_loop_total.fetch_add(n_loop);  // (<= n_slots * kResidentLoopIds in total: always room)
    memcpy(r->hp<int>(r->o_loopids) + off, loop_ids, sizeof(int) * n_loop);
    memcpy(r->hp<double>(r->o_loopxy) + 2 * (size_t)off, loop_xy, sizeof(double) * 2 * n_loop);
    r->hp<int>(r->o_loopf)[slot] = loop_frame, r->hp<int>(r->o_loopn)[slot] = n_loop, r->hp<int>(r->o_loopoff)[slot] = off;
  }
  r->hp<int>(r->o_nobs)[slot] = n_obs;
  r->hp<int>(r->o_active)[slot] = 1;
  return VIO_OK;
}

int vio_backend_resident_stage_preint(vio_backend_t *be, int32_t slot, int32_t interval, const VioPreintegration *block,
                                      const double last_acc[3], const double last_gyr[3]) {
  if (!be || !be->res) return VIO_ESTATE;
  vio_resident *r = be->res.get();
  if (r->phase != 1) return VIO_ESTATE;
  if (slot < 0 || slot >= r->n_slots || interval < 0 || interval >= r->W || !block || !last_acc || !last_gyr) return VIO_EINVAL;
  const int k = r->n_pre.fetch_add(1);
  if (k >= r->n_slots * r->W) return VIO_ECAP;
  r->hp<int>(r->o_preidx)[k] = slot * r->W + interval;
  double *dst = r->hp<double>(r->o_preblk) + (size_t)k * (kPreintDoubles + 6);
  memcpy(dst, block, sizeof(double) * kPreintDoubles);
  memcpy(dst + kPreintDoubles, last_acc, 24), memcpy(dst + kPreintDoubles + 3, last_gyr, 24);  // what a continuation starts from
  return VIO_OK;
}

// The raw samples of an interval instead of its integrated block: fresh = 1 a new interval (acc_0 / gyr_0: the sample it
// starts from, ba / bg: its linearization biases), 0 more samples for the block in place. VIO_ECAP: no room left in this
// frame's staging (the caller sends the block instead).
int vio_backend_resident_stage_imu(vio_backend_t *be, int32_t slot, int32_t interval, int32_t fresh, const double acc_0[3],
                                   const double gyr_0[3], const double ba[3], const double bg[3], int32_t n, const double *dt,
                                   const double *acc, const double *gyr) {
  if (!be || !be->res) return VIO_ESTATE;
  vio_resident *r = be->res.get();
  if (r->phase != 1) return VIO_ESTATE;
  if (slot < 0 || slot >= r->n_slots || interval < 0 || interval >= r->W || n < 0 || (n > 0 && (!dt || !acc || !gyr))) return VIO_EINVAL;
  if (fresh && (!acc_0 || !gyr_0 || !ba || !bg)) return VIO_EINVAL;
  const int first = r->n_samples.fetch_add(n);
  if (first + n > r->cap_samples) return VIO_ECAP;  // (the counter stays past the end: later callers fail as well, ingest clamps)
  const int j = r->n_jobs.fetch_add(1);
  if (j >= r->cap_jobs) return VIO_ECAP;
  double *rec = r->hp<double>(r->o_jobs) + (size_t)j * 16;
  rec[0] = slot * r->W + interval, rec[1] = fresh ? 1 : 0, rec[2] = n, rec[3] = first;
  for (int k = 0; k < 3; k++) rec[4 + k] = fresh ? acc_0[k] : 0, rec[7 + k] = fresh ? gyr_0[k] : 0, rec[10 + k] = fresh ? ba[k] : 0, rec[13 + k] = fresh ? bg[k] : 0;
  double *smp = r->hp<double>(r->o_samples) + (size_t)first * 7;
  for (int i = 0; i < n; i++) {
    smp[7 * i] = dt[i];
    for (int k = 0; k < 3; k++) smp[7 * i + 1 + k] = acc[3 * i + k], smp[7 * i + 4 + k] = gyr[3 * i + k];
  }
  return VIO_OK;
}

int vio_backend_resident_ingest(vio_backend_t *be) {
  if (!be || !be->res) return VIO_ESTATE;
  vio_resident *r = be->res.get();
  if (r->phase != 1) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(be);
  hipStream_t st = be->stream;
  const double t0 = now_ms();
  const int n_pre = std::min(r->n_pre.load(), r->n_slots * r->W);
  r->n_pre.store(n_pre);
  const int n_jobs = std::min(r->n_jobs.load(), r->cap_jobs), n_samples = std::min(r->n_samples.load(), r->cap_samples);
  r->n_jobs.store(n_jobs);
  // the fixed part, then what is in use of the variable regions (observations, IMU jobs and samples, blocks)
  size_t bytes = r->o_obs;
  HIP_OK(hipMemcpyAsync(r->d_in.p, r->h_in.data(), r->o_obs, hipMemcpyHostToDevice, st));
  auto part = [&](size_t off, size_t n_bytes) {
    if (n_bytes) bytes += n_bytes;
    return n_bytes ? hipMemcpyAsync(r->d_in.p + off, r->h_in.data() + off, n_bytes, hipMemcpyHostToDevice, st) : hipSuccess;
  };
  HIP_OK(part(r->o_obs, (size_t)r->n_obs_total.load() * sizeof(VioObs)));
  r->any_loop = r->n_loop_total.load() > 0;
  HIP_OK(part(r->o_loopids, (size_t)r->n_loop_total.load() * sizeof(int)));
  HIP_OK(part(r->o_loopxy, (size_t)r->n_loop_total.load() * 2 * sizeof(double)));
  HIP_OK(part(r->o_jobs, (size_t)n_jobs * 16 * sizeof(double)));
  HIP_OK(part(r->o_samples, (size_t)n_samples * 7 * sizeof(double)));
  HIP_OK(part(r->o_preblk, (size_t)n_pre * (kPreintDoubles + 6) * sizeof(double)));
  // where every slot's prior is read from and where the next one goes (the banks of the prior store)
  {
    const int n = r->n_slots;
    if (be->d_ptab.ensure(n) != VIO_OK) return VIO_ENOMEM;
    be->h_ptab.resize(n);
    const int *hdr = r->hp<int>(r->o_hdr), *act = r->hp<int>(r->o_active);
    for (int k = 0; k < n; k++) be->h_ptab[k] = act[k] ? prior_tab(be, k, hdr[(size_t)k * kHdrInts + H_PRIOR_N] > 0, be->st_ncap) : PriorTab{};
    HIP_OK(hipMemcpyAsync(be->d_ptab.p, be->h_ptab.data(), sizeof(PriorTab) * n, hipMemcpyHostToDevice, st));
  }
  const vio::StoreDev S = resident_store_dev(be);
  int rc = vio::store_launch_imu(S, st);
  if (rc == VIO_OK) rc = vio::store_launch_ingest(S, st);
  if (rc != VIO_OK) return rc;
  r->phase = 2;  // (the counts are fetched by launch: a queued device-to-host copy would hold up the other contexts' uploads)
  if (host_timing()) fprintf(stderr, "resident_ingest: calls %.3f ms (%zu bytes up, %d pre-integration blocks, %d IMU jobs with %d samples)\n", now_ms() - t0, bytes, n_pre, n_jobs, n_samples);
  return VIO_OK;
}

int vio_backend_resident_launch(vio_backend_t *be) {
  if (!be || !be->res) return VIO_ESTATE;
  vio_resident *r = be->res.get();
  if (r->phase != 2) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(be);
  hipStream_t st = be->stream;
  const double t0 = now_ms();
  HIP_OK(hipMemcpyAsync(r->h_ctl.data(), r->ctl.p, sizeof(int) * r->h_ctl.size(), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));  // the counts of store_ingest
  const double t1 = now_ms();
  r->phase = 3;
  // (store_pack aligns buckets to the LDS variant's chunk and reports no straddles: windows packed on the device never run as
  // cooperative windows, whatever an earlier host upload on this context left in the flag)
  be->coop_ok = false;
  const int n = r->n_slots;
  const int *act = r->hp<int>(r->o_active);
  std::vector<int> nfeat(n, 0);
  int Fmax = 1, Mmax = 1;
  r->active_list.clear();
  for (int k = 0; k < n; k++) {
    if (!act[k]) continue;
    int *c = r->h_ctl.data() + (size_t)k * vio::store::C_COUNT;
    if (c[vio::store::C_STATUS] != VIO_OK) continue;
    // (a relocalization frame adds at most one factor per matched id: counted here, so that only THIS slot is refused --
    // store_pack's LDS fit was validated at reserve for max_factors, and a failed pack launch clears the whole group)
    if (c[vio::store::C_F] > be->cfg.max_features || c[vio::store::C_M] + r->hp<int>(r->o_loopn)[k] > be->cfg.max_factors) {
      // more landmarks / factors than the configuration allows: the window is not solved; the device learns it too
      c[vio::store::C_STATUS] = VIO_ECAP;
      HIP_OK(hipMemcpyAsync(r->ctl.p + (size_t)k * vio::store::C_COUNT + vio::store::C_STATUS, &c[vio::store::C_STATUS], sizeof(int),
                            hipMemcpyHostToDevice, st));
      continue;
    }
    nfeat[k] = c[vio::store::C_F];
    // (store_ingest counts the window's own factors; a relocalization frame adds at most one per matched id)
    Fmax = std::max(Fmax, c[vio::store::C_F]), Mmax = std::max(Mmax, c[vio::store::C_M] + r->hp<int>(r->o_loopn)[k]);
    r->active_list.push_back(k);
  }
  if (r->active_list.empty()) return VIO_OK;
  try {
    // sticky capacities. (A loop pose is one more 6-dof block: other strides, another LDS layout.)
    const vio_wk::Need need = {r->W, Fmax, Mmax, 0, r->any_loop};
    if (!r->bound || !vio_wk::fits(r->d, need)) {
      const BatchDims d = vio_wk::grow_dims(be->cfg, need, vio_wk::kResidentGrowth, r->bound ? &r->d : nullptr);
      const BatchStrides s = make_strides(d);
      const size_t N = n;
      int rc = VIO_OK;
      DevBuf<int> *ib[] = {&r->b_fhost, &r->b_ftarget, &r->b_ffeat, &r->b_fslot};
      for (auto *b : ib)
        if (rc == VIO_OK) rc = b->ensure(N * s.fint);
      if (rc == VIO_OK) rc = r->b_fstart.ensure(N * s.fstart);
      DevBuf<int> *pb[] = {&r->b_pair_h, &r->b_pair_t, &r->b_pair_s0, &r->b_pair_s1};
      for (auto *b : pb)
        if (rc == VIO_OK) rc = b->ensure(N * s.pair);
      if (rc == VIO_OK) rc = r->b_feat.ensure(N * s.feat);
      if (rc == VIO_OK) rc = r->b_pts_i.ensure(N * s.pts);
      if (rc == VIO_OK) rc = r->b_pts_j.ensure(N * s.pts);
      if (rc != VIO_OK) return rc;
      {
        std::vector<double> ones(N * s.feat, 1.0);  // the padding behind a window's landmarks is read (whole tiles): keep it finite
        HIP_OK(hipMemcpy(r->b_feat.p, ones.data(), sizeof(double) * ones.size(), hipMemcpyHostToDevice));
      }
      r->d = d, r->s = s, r->bound = true;
    }
    const BatchStrides &s = r->s;
    be->uploaded = false;  // the context's plan and bindings are this path's from here on: nothing for vio_backend_launch / _download
    // (every resident window has the store's window size)
    be->plan = vio_wk::plan_layout(r->d, n, nfeat.data(), &r->active_list, r->W == vio_wk::kStaticW, be->n_cus, be->peers, be->profile);
    if (be->plan.rc != VIO_OK) return be->plan.rc;
    const BatchDims &d = be->plan.d;
    int rc = bind_work_buffers(be, s, n);
    if (rc != VIO_OK) return rc;
    if (be->d_order.ensure(n) != VIO_OK) return VIO_ENOMEM;
    be->h_order.assign(be->plan.order.begin(), be->plan.order.end());
    HIP_OK(hipMemcpyAsync(be->d_order.p, be->h_order.data(), sizeof(int) * be->h_order.size(), hipMemcpyHostToDevice, st));
    BatchPtrs &B = be->B;
    B.n = n, B.d = d, B.s = s;
    B.hdr = r->dp<int>(r->o_hdr), B.hdr_d = r->dp<double>(r->o_hdrd);
    B.pose = r->dp<double>(r->o_pose), B.sb = r->dp<double>(r->o_sb), B.ex = r->dp<double>(r->o_ex);
    B.pr_kind = r->dp<int>(r->o_prk), B.pr_index = r->dp<int>(r->o_pri), B.pr_offset = r->dp<int>(r->o_pro);
    B.feat = r->b_feat.p, B.fhost = r->b_fhost.p, B.ftarget = r->b_ftarget.p, B.ffeat = r->b_ffeat.p, B.fslot = r->b_fslot.p;
    B.fstart = r->b_fstart.p, B.pair_h = r->b_pair_h.p, B.pair_t = r->b_pair_t.p, B.pair_s0 = r->b_pair_s0.p, B.pair_s1 = r->b_pair_s1.p;
    B.pts_i = r->b_pts_i.p, B.pts_j = r->b_pts_j.p, B.preint = r->preint.p;
    B.pr_x0 = r->b_dummy.p, B.pr_J = r->b_dummy.p, B.pr_r = r->b_dummy.p;  // (every prior of this path sits in the store: ptab)
    B.ptab = be->d_ptab.p;
    const vio::StoreDev S = resident_store_dev(be);
    rc = vio::store_launch_pack(S, B, be->plan.chunk, st);
    if (rc != VIO_OK) return rc;
    rc = launch_windows(be, st, B);  // (on the stream of the pack: nothing to wait for)
    if (rc != VIO_OK) return rc;
    rc = vio::store_launch_finish(S, B, st);
    if (rc != VIO_OK) return rc;
    for (int k : r->active_list) r->solved[k] = 1;
    if (host_timing())
      fprintf(stderr, "resident_launch: wait for the counts %.3f ms, layout + launches %.3f ms (%zu windows, F <= %d, M <= %d, %d LDS / %d global)\n",
              t1 - t0, now_ms() - t1, r->active_list.size(), Fmax, Mmax, be->plan.n_lds, be->plan.n_glb);
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
  return VIO_OK;
}

int vio_backend_resident_collect(vio_backend_t *be) {
  if (!be || !be->res) return VIO_ESTATE;
  vio_resident *r = be->res.get();
  if (r->phase != 2 && r->phase != 3) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(be);
  const double t0 = now_ms();
  // The results are queued HERE, not behind the launch: a device-to-host copy waiting for this context's window kernel
  // holds up the host-to-device copies that other contexts issue meanwhile (their uploads, and with them their kernels,
  // would start only after this kernel: measured, two groups ran one after the other).
  if (r->phase == 3 && !r->active_list.empty()) {
    hipStream_t st = be->stream;
    HIP_OK(hipMemcpyAsync(r->h_ctl.data(), r->ctl.p, sizeof(int) * r->h_ctl.size(), hipMemcpyDeviceToHost, st));
    HIP_OK(d2h(r->h_out_pose, be->d_out_pose, st));
    HIP_OK(d2h(r->h_out_sb, be->d_out_sb, st));
    HIP_OK(d2h(r->h_stats_d, be->d_stats_d, st));
    HIP_OK(d2h(r->h_stats_i, be->d_stats_i, st));
    HIP_OK(d2h(r->h_m_ints, be->d_m_ints, st));
    if (r->any_loop) {
      HIP_OK(d2h(r->h_raw_pose, be->d_raw_pose, st));
      HIP_OK(d2h(r->h_out_loop, be->d_out_loop, st));
    }
  }
  HIP_OK(hipStreamSynchronize(be->stream));
  if (host_timing()) fprintf(stderr, "resident_collect: wait %.3f ms\n", now_ms() - t0);
  if (r->prof.p) {
    long long c[32];
    HIP_OK(hipMemcpy(c, r->prof.p, sizeof(c), hipMemcpyDeviceToHost));
    fprintf(stderr, "store cycles (slot 0): pack scans %lld, factors %lld, buckets %lld, slots %lld\n", c[9] - c[8], c[10] - c[9], c[11] - c[10], c[12] - c[11]);
    fprintf(stderr, "   ingest: sort %lld, match %lld, new %lld, parallax %lld, triangulate %lld, counts %lld; finish: scan+failure %lld, states %lld, move %lld\n", c[1] - c[0],
            c[2] - c[1], c[3] - c[2], c[4] - c[3], c[5] - c[4], c[6] - c[5], c[17] - c[16], c[18] - c[17], c[19] - c[18]);
  }
  for (int k : r->active_list)
    if (r->solved[k] && r->h_m_ints[(size_t)k * be->MP.s_ints] > 0) be->st_bank[k] ^= 1;
  r->phase = 0;
  return VIO_OK;
}

int vio_backend_resident_result(vio_backend_t *be, int32_t slot, VioResidentResult *out, VioPrior *next_prior_header) {
  if (!be || !be->res || !out) return VIO_ESTATE;
  vio_resident *r = be->res.get();
  if (slot < 0 || slot >= r->n_slots) return VIO_EINVAL;
  if (r->phase != 0) return VIO_ESTATE;
  const int *c = r->h_ctl.data() + (size_t)slot * vio::store::C_COUNT;
  memset(out, 0, sizeof(*out));
  out->status = c[vio::store::C_STATUS];
  out->marginalization_flag = c[vio::store::C_MARG], out->track_num = c[vio::store::C_TRACK], out->parallax_num = c[vio::store::C_PNUM];
  out->n_features = c[vio::store::C_F], out->n_factors = c[vio::store::C_M], out->n_list = c[vio::store::C_N];
  if (!r->solved[slot]) {
    if (out->status == VIO_OK) out->status = VIO_ESTATE;  // not part of this frame
    return VIO_OK;
  }
  out->failure_reasons = c[vio::store::C_FAIL];
  out->n_loop_factors = c[vio::store::C_NLOOP];
  const BatchStrides &s = r->s;
  if (r->any_loop && r->h_raw_pose.size() >= ((size_t)slot + 1) * s.out_pose) {
    out->raw_pose = r->h_raw_pose.data() + (size_t)slot * s.out_pose;
    out->loop_pose = r->h_out_loop.data() + (size_t)slot * s.out_loop;
  }
  out->pose = r->h_out_pose.data() + (size_t)slot * s.out_pose;
  out->speed_bias = r->h_out_sb.data() + (size_t)slot * s.out_sb;
  unpack_solve_stats(r->h_stats_d.data() + (size_t)slot * s.stats_d, r->h_stats_i.data() + (size_t)slot * s.stats_i, &out->stats);
  if (next_prior_header) {
    const MargOut mo = marg_header(r->h_m_ints.data() + (size_t)slot * be->MP.s_ints, be->B.d.Ncap);
    unpack_prior(mo, *next_prior_header, false);
  }
  return VIO_OK;
}
