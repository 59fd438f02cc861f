// vio_frontend.hip — host side and C ABI of the KLT front-end (include/vio_amd.h); its gfx950 kernels are the fe_*.h headers.
//
// Drop-in for FeatureTracker::readImage (VINS_ios/feature_tracker.cpp:162-321) over a batch of independent sequences:
// every kernel takes (sequence, item) grids so one set of launches advances all trackers by one frame.
//   fe_common.h        limits, LevelDims, reflect101, descale: what the headers below share
//   fe_subset.h        (host only) the plan of a subset call: per-sequence phase bits -> launch lists; every kernel below has a
//                      subset instantiation next to it that takes the plan (SubsetArgs) in place of "sequence = block index"
//   fe_pyramid.h       pyr_down_kernel        cv::pyrDown levels of calcOpticalFlowPyrLK                  (feature_tracker.cpp:181)
//                      pyr_down4_kernel       the same for rows of whole dwords; the level-1 launch can also write level 0
//                                                                                      (feature_tracker.cpp:165-170,181)
//                      copy_frames_kernel     forw_img = _img                                              (feature_tracker.cpp:165-170)
//   fe_lk.h            lk_track_kernel        calcOpticalFlowPyrLK, one wave64 per feature, all levels    (feature_tracker.cpp:181)
//   fe_ransac.h        fundamental_ransac_block, the workgroup routine of findFundamentalMat(RANSAC); ransac_only_kernel and
//                      ransac_batch_kernel are that routine alone                      (feature_tracker.cpp:183-205)
//   fe_track_update.h  track_update_kernel    inBorder + reduceVector + findFundamentalMat(RANSAC) [+ rejectWithF, track_cnt++, setMask]
//                                                                                      (feature_tracker.cpp:183-205,235-255)
//   fe_detect.h        detect_kernel          goodFeaturesToTrack front half, fused: cornerMinEigenVal, masked maximum, 3x3 non-max and
//                                             the setMask discs evaluated analytically (cv::circle(mask, pt, MIN_DIST, 0, -1))
//                                                                                      (feature_tracker.cpp:80,263)
//   fe_select.h        corner_select_kernel   quality threshold, sorted greedy min-distance pick, addPoints, updateID, image_msg
//                                                                                      (feature_tracker.cpp:263-307)
// Arithmetic follows the OpenCV 3.0 integer/float sequences restated in oracle/vio_oracle_frontend.cpp so the two
// agree bit for bit; sums that OpenCV accumulates in float (LK's A and b) are accumulated exactly.
// One translation unit: the headers are included once, below, in dependency order. The non-template kernels are emitted in
// that order and the template kernels in the order of the launch sites in this file.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "vio_amd.h"
#include "vio_camera.h"
#include "vio_device.h"
#include "vio_pool.h"

#include "fe_subset.h"
#include "fe_common.h"
#include "fe_pyramid.h"
#include "fe_lk.h"
#include "fe_ransac.h"
#include "fe_track_update.h"
#include "fe_detect.h"
#include "fe_select.h"

namespace {

void circle_halfwidths(int radius, std::vector<int> &hw) {  // cv::circle filled midpoint raster (drawing.cpp Circle())
  hw.assign(2 * radius + 1, -1);
  int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
  while (dx >= dy) {
    hw[radius + dy] = std::max(hw[radius + dy], dx), hw[radius - dy] = std::max(hw[radius - dy], dx);
    hw[radius + dx] = std::max(hw[radius + dx], dy), hw[radius - dx] = std::max(hw[radius - dx], dy);
    dy++;
    err += plus;
    plus += 2;
    int mask = (err <= 0) - 1;
    err -= minus & mask;
    dx += mask;
    minus -= mask & 2;
  }
}

}  // namespace

using vio::DevBuf;
using vio::PinnedBuf;

struct vio_frontend {
  int device = -1;  // HIP device the context lives on (current device at create)
  VioConfig cfg;
  int n_seq = 0, cap = 0;
  LevelDims ld;
  hipStream_t stream = nullptr;
  // device state
  DevBuf<uint8_t> pyr[2];  // [n_seq][pyr_bytes]; cur = pyr[cur_idx], forw = pyr[1 - cur_idx]
  int cur_idx = 0;
  bool have_img = false;
  // level 0 of pyr[k] when it is NOT the pyramid's own copy: the frame inside the resident ring (vio_frontend_upload_frames) the
  // pyramid was built from -- the ring belongs to the context and outlives the two steps that read the frame
  const uint8_t *lvl0[2] = {nullptr, nullptr};
  DevBuf<uint8_t> mask;  // [rows*cols], only the stand-alone vio_good_features uses a mask image
  DevBuf<unsigned> max_bits;
  DevBuf<unsigned long long> cand;
  int nseg = 0, seg_cap = 0;  // candidate list: one segment per strip of kDetR rows
  DevBuf<int> n_cand;
  // a detection pass that had to drop candidates (a plateau of equal eigenvalues) stamps its number into the sequence's ovf[]; the
  // selection kernel's redo workgroups then redo that sequence exactly, each in its own full-size list of redo_full
  DevBuf<int> ovf, n_redo;
  DevBuf<unsigned long long> redo_full;  // [n_redo_wg][rows * cols]
  int n_redo_wg = 0, det_epoch = 0;
  bool redo_report = false;  // VIO_AMD_REDO_REPORT=1 (measurement aid): destroy prints how many sequences were redone
  DevBuf<float> cur_pts, pre_pts, forw_pts, lk_err;
  DevBuf<unsigned long long> lk_stats;  // [64][16] iteration counters of lk_track_kernel (vio_frontend_lk_iterations)
  bool lk_stats_on = false;
  DevBuf<int> ids, track_cnt, n_pts, n_forw, n_id, kept_xy, n_kept, hw, n_obs, pnp_ids, n_pnp;
  DevBuf<float> pnp_pts;
  DevBuf<uint8_t> lk_status;
  DevBuf<VioObs> obs;
  // the camera of every sequence (vio_frontend_set_cameras): cfg's until one is set; image_msg reads the device table
  DevBuf<double> cam;       // [n_seq][4] fx, fy, cx, cy
  std::vector<double> h_cam;  // the same on the host (vio_frontend_get_camera)
  // the region of interest of every sequence (vio_frontend_set_regions; RegionArgs of fe_common.h): allocated with the first one.
  // n_region = 0 launches the kernels as they always were, anything else their REGION variants for all sequences.
  DevBuf<unsigned long long> region_words;  // [n_seq][rows][region_wpr]
  DevBuf<int> region_set;                   // [n_seq]
  std::vector<int> h_region_set;
  int region_wpr = 0, n_region = 0;
  DevBuf<long long> d_prof;  // stage clock of track_update_kernel (VIO_AMD_TU_PROF=1)
  DevBuf<long long> d_cs_prof;  // stage clock of corner_select_kernel (VIO_AMD_CS_PROF=1, read at create)
  bool cs_prof = false;
  bool attr_set = false, attr_set_region = false, attr_set_subset_region = false;
  bool detect_always = false;  // VIO_AMD_DETECT_ALWAYS=1 (measurement aid): detect_kernel also runs for sequences that need no new corner
  // resident frames (throughput runs)
  DevBuf<uint8_t> frames;
  int n_frames = 0;
  vio::LaunchTimer timer;  // vio_frontend_step_resident -> vio_frontend_kernel_ms
  // host-buffer path (vio_frontend_read_images): device staging for the frames, pinned memory for the observations
  DevBuf<uint8_t> d_stage;
  PinnedBuf<VioObs> p_obs;
  PinnedBuf<int> p_nobs;
  PinnedBuf<uint8_t> p_frames;  // page-locked gathering buffer of read_images
  bool pending = false, pending_publish = false;  // a submitted frame waits for vio_frontend_collect
  bool pending_async = false;                     // ... and it was queued by vio_frontend_submit_images_async (Async::rc is its status)
  // vio_frontend_submit_images_async: the submit itself (gather + transfers + launches) runs on this context's own host
  // thread, the caller returns at once; collect waits for it first
  struct Async {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    bool has_job = false, busy = false, quit = false;
    const uint8_t *gray = nullptr;
    int rows = 0, cols = 0, stride = 0, publish = 0, rc = VIO_OK;
  } *async = nullptr;
  // Subset calls (vio_frontend_submit_subset / vio_frontend_reset, fe_subset.h): every sequence has its own phase. While all of them
  // are in the same one (in_step) cur_idx / have_img above are the record, the lock-step entry points are allowed and keep it;
  // the vectors are filled from it at the head of a subset call. Out of step the vectors are the record.
  std::vector<uint8_t> ph_bank, ph_have, ph_seen;
  bool in_step = true;
  bool foreign_stream = false;  // a lock-step step was queued on a caller's stream: a subset call waits for the device once
  PinnedBuf<int32_t> p_arena;   // the call's plan: seq | slot | prev bank | forw bank | publish | published list
  DevBuf<int> d_arena;
  DevBuf<VioObs> obs_sub;  // [n][cap] image_msg of a subset call in the call's order, and their counts
  DevBuf<int> n_obs_sub;
  bool pending_subset = false;  // the frame in flight came from submit_subset (pending_n sequences, pending_pub of them published)
  int pending_n = 0, pending_pub = 0;
  bool attr_set_subset = false;
  // host staging
  std::vector<VioObs> h_obs;
  std::vector<int> h_nobs;
  ~vio_frontend() {
    if (redo_report && n_redo.p) {
      int n = -1;
      if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(&n, n_redo.p, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess)
        fprintf(stderr, "detector: %d sequence-frames redone from the full-size candidate list (%d detection passes)\n", n, det_epoch);
    }
    if (async) {
      {
        std::lock_guard<std::mutex> lk(async->m);
        async->quit = true;
      }
      async->cv.notify_all();
      if (async->th.joinable()) async->th.join();
      delete async;
    }
    (void)hipDeviceSynchronize();
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

int next_epoch(vio_frontend *fe) {  // number of the detection pass being launched: never 0, which is what ovf[] starts as
  fe->det_epoch = fe->det_epoch == INT_MAX ? 1 : fe->det_epoch + 1;
  return fe->det_epoch;
}

RedoParams redo_params(vio_frontend *fe, const uint8_t *img_base, size_t img_stride, const uint8_t *mask_base, size_t mask_stride, int radius) {
  RedoParams R;
  R.img_base = img_base, R.mask_base = mask_base, R.img_stride = img_stride, R.mask_stride = mask_stride;
  R.kept_xy = fe->kept_xy.p, R.n_kept = fe->n_kept.p, R.hw = fe->hw.p, R.radius = radius;
  R.full = fe->redo_full.p, R.ovf = fe->ovf.p, R.epoch = fe->det_epoch, R.n_seq = fe->n_seq, R.n_wg = fe->n_redo_wg, R.n_redo = fe->n_redo.p;
  return R;
}

// criteria and thresholds of calcOpticalFlowPyrLK as the context was configured; the caller sets prev0, next0 and stride0
LkParams lk_params(const VioConfig &cfg, const LevelDims &ld) {
  LkParams P;
  P.ld = ld, P.cap = cfg.max_corners;
  P.max_count = std::min(std::max(cfg.lk_max_iters, 0), 100);
  double eps = std::min(std::max(cfg.lk_eps, 0.), 10.);
  P.epsilon_sq = eps * eps, P.epsilon_sq_f = lk_eps_screen(eps * eps), P.min_eig = (float)cfg.lk_min_eig;
  return P;
}

SelectParams select_params(const vio_frontend *fe) {
  const VioConfig &cfg = fe->cfg;
  SelectParams SP;
  SP.cap = cfg.max_corners, SP.rows = cfg.image_rows, SP.cols = cfg.image_cols, SP.max_corners = cfg.max_corners, SP.min_dist = (float)cfg.min_dist;
  SP.cam = fe->cam.p;
  return SP;
}

// feature_tracker.cpp:183-205 (+ :235-255, :50-87 on publish frames) for every sequence: one workgroup each
RegionArgs region_of(const vio_frontend *fe) { return RegionArgs{fe->region_words.p, fe->region_set.p, fe->region_wpr}; }

TrackerArrays tracker_arrays(vio_frontend *fe) {
  TrackerArrays A;
  A.cap = fe->cap, A.rows = fe->cfg.image_rows, A.cols = fe->cfg.image_cols;
  A.cur_pts = fe->cur_pts.p, A.pre_pts = fe->pre_pts.p, A.forw_pts = fe->forw_pts.p, A.ids = fe->ids.p, A.track_cnt = fe->track_cnt.p;
  A.n_pts = fe->n_pts.p, A.n_forw = fe->n_forw.p, A.n_id = fe->n_id.p, A.lk_status = fe->lk_status.p, A.kept_xy = fe->kept_xy.p;
  A.n_kept = fe->n_kept.p, A.hw = fe->hw.p, A.radius = fe->cfg.min_dist, A.f_thresh = (float)fe->cfg.f_threshold;
  A.pnp_pts = fe->pnp_pts.p, A.pnp_ids = fe->pnp_ids.p, A.n_pnp = fe->n_pnp.p;
  A.f_conf = fe->cfg.f_confidence;
  A.prof = nullptr;
  return A;
}

int launch_track_update(vio_frontend *fe, int publish, hipStream_t st) {
  TrackerArrays A = tracker_arrays(fe);
  static const bool tu_prof = vio::env_flag("VIO_AMD_TU_PROF");
  if (tu_prof) (void)fe->d_prof.ensure(32);
  A.prof = tu_prof ? fe->d_prof.p : nullptr;
  // the smallest LDS layout that holds this tracker's feature slots (fe->cap <= kMaxCap is checked at create)
  const bool small = fe->cap <= 256;
  const size_t shm = ((small ? sizeof(TrackShared<256>) : sizeof(TrackShared<kMaxCap>)) + 15 & ~(size_t)15) + sizeof(RansacShared);
  const void *kern = small ? (const void *)track_update_kernel<256> : (const void *)track_update_kernel<kMaxCap>;
  if (!fe->attr_set) {
    HIP_OK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    fe->attr_set = true;
  }
  if (fe->n_region && !fe->attr_set_region) {
    HIP_OK(hipFuncSetAttribute(small ? (const void *)track_update_kernel<256, RegionArgs> : (const void *)track_update_kernel<kMaxCap, RegionArgs>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
    fe->attr_set_region = true;
  }
  if (A.prof) (void)hipMemsetAsync(A.prof, 0, 32 * sizeof(long long), st);
  if (fe->n_region) {
    if (small) hipLaunchKernelGGL((track_update_kernel<256, RegionArgs>), dim3(fe->n_seq), dim3(256), shm, st, A, publish, region_of(fe));
    else hipLaunchKernelGGL((track_update_kernel<kMaxCap, RegionArgs>), dim3(fe->n_seq), dim3(256), shm, st, A, publish, region_of(fe));
  } else if (small) hipLaunchKernelGGL(track_update_kernel<256>, dim3(fe->n_seq), dim3(256), shm, st, A, publish);
  else hipLaunchKernelGGL(track_update_kernel<kMaxCap>, dim3(fe->n_seq), dim3(256), shm, st, A, publish);
  if (A.prof) {  // (debug only: synchronises)
    long long h[32];
    if (hipStreamSynchronize(st) == hipSuccess && hipMemcpy(h, A.prof, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) {
      static const char *name[11] = {"load", "compact", "ransac(cur,forw)", "compact", "pnp list", "ransac(pre,forw)", "compact", "counts+rank",
                                     "inside bits", "greedy", "outputs"};
      fprintf(stderr, "track_update cycles (sequence 0, publish %d):", publish);
      const int map[11][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 6}, {6, 7}, {7, 8}, {8, 9}, {9, 10}, {10, 11}};
      for (int k = 0; k < 11; k++) fprintf(stderr, " %s %lld,", name[k], h[map[k][1]] - h[map[k][0]]);
      fprintf(stderr, " total %lld\n", h[11] - h[0]);
      for (int c = 0; c < 2; c++)
        fprintf(stderr, "   ransac call %d: draw %lld, gather+collinear %lld, 7-point %lld, scoring %lld, scan %lld, mask %lld, rounds %lld\n", c,
                h[16 + 8 * c], h[17 + 8 * c], h[18 + 8 * c], h[19 + 8 * c], h[20 + 8 * c], h[21 + 8 * c], h[22 + 8 * c]);
    }
  }
  return VIO_OK;
}

// keep_frames: d_frames stays valid and unchanged until the frame after the next one has been tracked (the context's resident ring):
// level 0 is then read where it lies instead of being copied into the pyramid.
int fe_step(vio_frontend *fe, const uint8_t *d_frames /* [n_seq][rows*cols] on device */, int publish, hipStream_t st, bool keep_frames = false) {
  const int S = fe->n_seq, rows = fe->cfg.image_rows, cols = fe->cfg.image_cols, cap = fe->cap;
  const size_t img_bytes = (size_t)rows * cols;
  // forw_img = _img : level 0 of the forw pyramid
  const int fidx = fe->have_img ? 1 - fe->cur_idx : fe->cur_idx;
  uint8_t *forw = fe->pyr[fidx].p;
  // level 0 and level 1 from ONE read of the frame when the rows of both are whole dwords (640x480, 720p, 1080p)
  const bool fused0 = fe->ld.levels >= 2 && cols % 4 == 0 && fe->ld.cols[1] % 4 == 0 && cols >= 8 && fe->ld.pyr_bytes % 4 == 0 &&
                      img_bytes % 4 == 0 && (uintptr_t)d_frames % 4 == 0 && (uintptr_t)forw % 4 == 0 && fe->ld.off[1] % 4 == 0;
  const bool alias0 = keep_frames && fused0 && !vio::env_flag("VIO_AMD_COPY_LEVEL0");
  fe->lvl0[fidx] = alias0 ? d_frames : nullptr;
  if (!fused0) {
    const int vec_ok = img_bytes % 16 == 0 && fe->ld.pyr_bytes % 16 == 0 && (uintptr_t)d_frames % 16 == 0 &&
                       (uintptr_t)forw % 16 == 0;
    dim3 grd((unsigned)((img_bytes + 16 * 256 - 1) / (16 * 256)), S);
    hipLaunchKernelGGL(copy_frames_kernel, grd, dim3(256), 0, st, d_frames, img_bytes, forw, fe->ld.pyr_bytes, img_bytes,
                       vec_ok);
  }
  for (int l = 1; l < fe->ld.levels; l++) {
    const uint8_t *sp = forw + fe->ld.off[l - 1];
    uint8_t *dp = forw + fe->ld.off[l];
    const int sc = fe->ld.cols[l - 1], dc = fe->ld.cols[l];
    if (l == 1 && fused0) {
      dim3 blk(256), grd((dc + kPdW - 1) / kPdW, (fe->ld.rows[1] + kPd4H * kPd4T - 1) / (kPd4H * kPd4T), S);
      if (alias0)
        hipLaunchKernelGGL(pyr_down4_kernel<false>, grd, blk, 0, st, d_frames, img_bytes, dp, fe->ld.pyr_bytes, rows, cols, fe->ld.rows[1], dc,
                           (uint8_t *)nullptr);
      else
        hipLaunchKernelGGL(pyr_down4_kernel<true>, grd, blk, 0, st, d_frames, img_bytes, dp, fe->ld.pyr_bytes, rows, cols, fe->ld.rows[1], dc, forw);
      continue;
    }
    // whole-dword rows on both sides (and at least two staged dwords of image): 4 pixels per load and per store
    const bool dwords = sc % 4 == 0 && dc % 4 == 0 && sc >= 8 && fe->ld.pyr_bytes % 4 == 0 && (uintptr_t)sp % 4 == 0 && (uintptr_t)dp % 4 == 0;
    if (dwords) {
      dim3 blk(256), grd((dc + kPdW - 1) / kPdW, (fe->ld.rows[l] + kPd4H * kPd4T - 1) / (kPd4H * kPd4T), S);
      hipLaunchKernelGGL(pyr_down4_kernel<false>, grd, blk, 0, st, sp, fe->ld.pyr_bytes, dp, fe->ld.pyr_bytes, fe->ld.rows[l - 1], sc, fe->ld.rows[l], dc,
                         (uint8_t *)nullptr);
    } else {
      dim3 blk(256), grd((dc + kPdW - 1) / kPdW, (fe->ld.rows[l] + kPdH - 1) / kPdH, S);
      hipLaunchKernelGGL(pyr_down_kernel, grd, blk, 0, st, sp, dp, fe->ld.pyr_bytes, fe->ld.rows[l - 1], sc, fe->ld.rows[l], dc);
    }
  }
  if (!fe->have_img) {  // pre_img = cur_img = forw_img = _img (:166-167); no points to track yet
    fe->have_img = true;
    fe->cur_idx = fidx;
  } else {
    LkParams P = lk_params(fe->cfg, fe->ld);
    P.prev0 = fe->lvl0[fe->cur_idx], P.next0 = fe->lvl0[fidx], P.stride0 = img_bytes;
    dim3 grd((cap + 3) / 4, S);
    // (the counting variant is a kernel of its own: STATS = [2 * levels] iterations run / (feature, level) visits of this launch,
    // vio_frontend_lk_iterations; the product kernel sits at 80 registers for six waves per SIMD and has none to spare)
    if (fe->lk_stats_on && fe->lk_stats.p)
      hipLaunchKernelGGL((lk_track_kernel<true>), grd, dim3(256), 0, st, fe->pyr[fe->cur_idx].p, forw, P, fe->n_pts.p, fe->cur_pts.p,
                         fe->forw_pts.p, fe->lk_status.p, fe->lk_err.p, fe->lk_stats.p);
    else
      hipLaunchKernelGGL((lk_track_kernel<false, false>), grd, dim3(256), 0, st, fe->pyr[fe->cur_idx].p, forw, P, fe->n_pts.p, fe->cur_pts.p,
                         fe->forw_pts.p, fe->lk_status.p, (float *)nullptr, (unsigned long long *)nullptr);  // (nobody reads the step's LK error)
  }
  int rcu = launch_track_update(fe, publish, st);
  if (rcu != VIO_OK) return rcu;
  if (publish) {
    dim3 tb(256), tg((cols + kDetWaves * kDetW - 1) / (kDetWaves * kDetW), fe->nseg, S);
    const int epoch = next_epoch(fe);
    const int *n_have = fe->detect_always ? (const int *)nullptr : fe->n_forw.p;
    if (fe->n_region)
      hipLaunchKernelGGL((detect_kernel<false, RegionArgs>), tg, tb, 0, st, alias0 ? d_frames : forw, alias0 ? img_bytes : fe->ld.pyr_bytes, (const uint8_t *)nullptr,
                         (size_t)0, fe->kept_xy.p, fe->n_kept.p, cap, fe->hw.p, fe->cfg.min_dist, fe->max_bits.p, rows, cols, fe->cand.p,
                         fe->seg_cap, fe->n_cand.p, fe->ovf.p, epoch, n_have, fe->cfg.max_corners, region_of(fe));
    else
      hipLaunchKernelGGL(detect_kernel<false>, tg, tb, 0, st, alias0 ? d_frames : forw, alias0 ? img_bytes : fe->ld.pyr_bytes, (const uint8_t *)nullptr, (size_t)0,
                         fe->kept_xy.p, fe->n_kept.p, cap, fe->hw.p, fe->cfg.min_dist, fe->max_bits.p, rows, cols, fe->cand.p,
                         fe->seg_cap, fe->n_cand.p, fe->ovf.p, epoch, n_have, fe->cfg.max_corners);
    const SelectParams SP = select_params(fe);
    const RedoParams RP = redo_params(fe, alias0 ? d_frames : forw, alias0 ? img_bytes : fe->ld.pyr_bytes, nullptr, 0, fe->cfg.min_dist);
    if (fe->n_region)
      hipLaunchKernelGGL((corner_select_kernel<false, RegionArgs>), dim3(S + fe->n_redo_wg), dim3(kSelThreads), 0, st, fe->cand.p, fe->seg_cap, fe->nseg,
                         fe->n_cand.p, fe->max_bits.p, RP, fe->cfg.quality_level, SP, fe->forw_pts.p, fe->cur_pts.p, fe->pre_pts.p, fe->ids.p,
                         fe->track_cnt.p, fe->n_forw.p, fe->n_pts.p, fe->n_id.p, fe->obs.p, fe->n_obs.p, fe->cs_prof ? fe->d_cs_prof.p : nullptr,
                         region_of(fe));
    else
      hipLaunchKernelGGL(corner_select_kernel<false>, dim3(S + fe->n_redo_wg), dim3(kSelThreads), 0, st, fe->cand.p, fe->seg_cap, fe->nseg,
                         fe->n_cand.p, fe->max_bits.p, RP, fe->cfg.quality_level, SP, fe->forw_pts.p, fe->cur_pts.p, fe->pre_pts.p, fe->ids.p,
                         fe->track_cnt.p, fe->n_forw.p, fe->n_pts.p, fe->n_id.p, fe->obs.p, fe->n_obs.p, fe->cs_prof ? fe->d_cs_prof.p : nullptr);
    if (fe->cs_prof) {  // (debug only: synchronises)
      long long h[5];
      if (hipStreamSynchronize(st) == hipSuccess && hipMemcpy(h, fe->d_cs_prof.p, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess)
        fprintf(stderr, "corner_select cycles (sequence 0): threshold %lld, selection %lld, ids %lld, outputs %lld, total %lld\n", h[1] - h[0],
                h[2] - h[1], h[3] - h[2], h[4] - h[3], h[4] - h[0]);
    }
  }
  HIP_OK(hipGetLastError());
  fe->cur_idx = fidx;  // cur_img = forw_img (:284)
  return VIO_OK;
}

// An image that is still read in place from the context's ring (fe->lvl0) moves into its pyramid: the ring is about to go
// (upload_frames), or the sequences are about to leave the lock-step phase the aliasing relies on (subset calls, reset).
int own_level0(vio_frontend *fe) {
  if (!fe->lvl0[0] && !fe->lvl0[1]) return VIO_OK;
  const size_t px = (size_t)fe->cfg.image_rows * fe->cfg.image_cols;
  HIP_OK(hipDeviceSynchronize());
  for (int k = 0; k < 2; k++) {
    if (fe->lvl0[k]) HIP_OK(hipMemcpy2D(fe->pyr[k].p, fe->ld.pyr_bytes, fe->lvl0[k], px, px, fe->n_seq, hipMemcpyDeviceToDevice));
    fe->lvl0[k] = nullptr;
  }
  return VIO_OK;
}

// The phase vectors as the lock-step record says (in step), ready for a subset call or a reset to change them.
void phase_from_lockstep(vio_frontend *fe) {
  if (!fe->in_step && !fe->ph_bank.empty()) return;
  fe->ph_bank.assign(fe->n_seq, fe->have_img ? (uint8_t)fe->cur_idx : 0), fe->ph_have.assign(fe->n_seq, fe->have_img ? 1 : 0);
  fe->ph_seen.assign(fe->n_seq, 0);
  if (!fe->have_img) fe->cur_idx = 0;
}
// ... and back: a call that leaves every sequence in the same phase hands the record to the lock-step entry points again.
void phase_to_lockstep(vio_frontend *fe) {
  fe->in_step = fe_subset::in_step(fe->n_seq, fe->ph_bank.data(), fe->ph_have.data());
  if (fe->in_step) fe->cur_idx = fe->ph_bank[0], fe->have_img = fe->ph_have[0] != 0;
}

// readImage for the n sequences of a plan (feature_tracker.cpp:162-310): the subset instantiations of fe_step's kernels, every one
// launched once over the call's sequences (detection and selection: over the n_pub that publish). d_frames: packed frame slots
// on the device; M: the plan on the device. Level 0 always becomes the pyramid's own copy.
int fe_step_subset(vio_frontend *fe, const SubsetArgs &M, int n, int n_pub, const uint8_t *d_frames, hipStream_t st) {
  const int rows = fe->cfg.image_rows, cols = fe->cfg.image_cols, cap = fe->cap;
  const size_t img_bytes = (size_t)rows * cols;
  const LevelDims &ld = fe->ld;
  const bool fused0 = ld.levels >= 2 && cols % 4 == 0 && ld.cols[1] % 4 == 0 && cols >= 8 && ld.pyr_bytes % 4 == 0 && img_bytes % 4 == 0 &&
                      (uintptr_t)d_frames % 4 == 0 && (uintptr_t)M.pyr[0] % 4 == 0 && (uintptr_t)M.pyr[1] % 4 == 0 && ld.off[1] % 4 == 0;
  if (!fused0) {
    const int vec_ok = img_bytes % 16 == 0 && ld.pyr_bytes % 16 == 0 && (uintptr_t)d_frames % 16 == 0 && (uintptr_t)M.pyr[0] % 16 == 0 &&
                       (uintptr_t)M.pyr[1] % 16 == 0;
    dim3 grd((unsigned)((img_bytes + 16 * 256 - 1) / (16 * 256)), n);
    hipLaunchKernelGGL(copy_frames_subset_kernel, grd, dim3(256), 0, st, M, d_frames, img_bytes, ld.pyr_bytes, img_bytes, vec_ok);
  }
  for (int l = 1; l < ld.levels; l++) {
    const int sc = ld.cols[l - 1], dc = ld.cols[l];
    if (l == 1 && fused0) {
      dim3 grd((dc + kPdW - 1) / kPdW, (ld.rows[1] + kPd4H * kPd4T - 1) / (kPd4H * kPd4T), n);
      hipLaunchKernelGGL(pyr_down4_subset_kernel<true>, grd, dim3(256), 0, st, M, d_frames, img_bytes, (size_t)0, ld.off[1], ld.pyr_bytes, rows,
                         cols, ld.rows[1], dc);
      continue;
    }
    const bool dwords = sc % 4 == 0 && dc % 4 == 0 && sc >= 8 && ld.pyr_bytes % 4 == 0 && ld.off[l - 1] % 4 == 0 && ld.off[l] % 4 == 0 &&
                        (uintptr_t)M.pyr[0] % 4 == 0 && (uintptr_t)M.pyr[1] % 4 == 0;
    if (dwords) {
      dim3 grd((dc + kPdW - 1) / kPdW, (ld.rows[l] + kPd4H * kPd4T - 1) / (kPd4H * kPd4T), n);
      hipLaunchKernelGGL(pyr_down4_subset_kernel<false>, grd, dim3(256), 0, st, M, (const uint8_t *)nullptr, (size_t)0, ld.off[l - 1], ld.off[l],
                         ld.pyr_bytes, ld.rows[l - 1], sc, ld.rows[l], dc);
    } else {
      dim3 grd((dc + kPdW - 1) / kPdW, (ld.rows[l] + kPdH - 1) / kPdH, n);
      hipLaunchKernelGGL(pyr_down_subset_kernel, grd, dim3(256), 0, st, M, ld.off[l - 1], ld.off[l], ld.pyr_bytes, ld.rows[l - 1], sc,
                         ld.rows[l], dc);
    }
  }
  {  // (a sequence on its first frame leaves at once: pre_img = cur_img = forw_img, :166-167)
    LkParams P = lk_params(fe->cfg, ld);
    P.prev0 = P.next0 = nullptr, P.stride0 = 0;
    hipLaunchKernelGGL(lk_track_subset_kernel, dim3((cap + 3) / 4, n), dim3(256), 0, st, M, P, fe->n_pts.p, fe->cur_pts.p, fe->forw_pts.p,
                       fe->lk_status.p);
  }
  {
    const TrackerArrays A = tracker_arrays(fe);
    const bool small = cap <= 256;
    const size_t shm = ((small ? sizeof(TrackShared<256>) : sizeof(TrackShared<kMaxCap>)) + 15 & ~(size_t)15) + sizeof(RansacShared);
    if (!fe->attr_set_subset) {
      const void *kern = small ? (const void *)track_update_subset_kernel<256> : (const void *)track_update_subset_kernel<kMaxCap>;
      HIP_OK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
      fe->attr_set_subset = true;
    }
    if (fe->n_region && !fe->attr_set_subset_region) {
      HIP_OK(hipFuncSetAttribute(small ? (const void *)track_update_subset_kernel<256, RegionArgs> : (const void *)track_update_subset_kernel<kMaxCap, RegionArgs>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
      fe->attr_set_subset_region = true;
    }
    if (fe->n_region) {
      if (small) hipLaunchKernelGGL((track_update_subset_kernel<256, RegionArgs>), dim3(n), dim3(256), shm, st, A, M, region_of(fe));
      else hipLaunchKernelGGL((track_update_subset_kernel<kMaxCap, RegionArgs>), dim3(n), dim3(256), shm, st, A, M, region_of(fe));
    } else if (small) hipLaunchKernelGGL(track_update_subset_kernel<256>, dim3(n), dim3(256), shm, st, A, M);
    else hipLaunchKernelGGL(track_update_subset_kernel<kMaxCap>, dim3(n), dim3(256), shm, st, A, M);
  }
  if (n_pub > 0) {
    dim3 tg((cols + kDetWaves * kDetW - 1) / (kDetWaves * kDetW), fe->nseg, n_pub);
    const int epoch = next_epoch(fe);
    const int *n_have = fe->detect_always ? (const int *)nullptr : fe->n_forw.p;
    if (fe->n_region)
      hipLaunchKernelGGL(detect_subset_kernel<RegionArgs>, tg, dim3(256), 0, st, M, ld.pyr_bytes, fe->kept_xy.p, fe->n_kept.p, cap, fe->hw.p, fe->cfg.min_dist,
                         fe->max_bits.p, rows, cols, fe->cand.p, fe->seg_cap, fe->n_cand.p, fe->ovf.p, epoch, n_have, fe->cfg.max_corners,
                         region_of(fe));
    else
      hipLaunchKernelGGL(detect_subset_kernel<>, tg, dim3(256), 0, st, M, ld.pyr_bytes, fe->kept_xy.p, fe->n_kept.p, cap, fe->hw.p, fe->cfg.min_dist,
                         fe->max_bits.p, rows, cols, fe->cand.p, fe->seg_cap, fe->n_cand.p, fe->ovf.p, epoch, n_have, fe->cfg.max_corners);
    const SelectParams SP = select_params(fe);
    RedoParams RP = redo_params(fe, nullptr, ld.pyr_bytes, nullptr, 0, fe->cfg.min_dist);
    RP.n_wg = std::min(fe->n_redo_wg, n_pub);
    if (fe->n_region)
      hipLaunchKernelGGL(corner_select_subset_kernel<RegionArgs>, dim3(n_pub + RP.n_wg), dim3(kSelThreads), 0, st, M, n_pub, fe->cand.p, fe->seg_cap,
                         fe->nseg, fe->n_cand.p, fe->max_bits.p, RP, fe->cfg.quality_level, SP, fe->forw_pts.p, fe->cur_pts.p, fe->pre_pts.p, fe->ids.p,
                         fe->track_cnt.p, fe->n_forw.p, fe->n_pts.p, fe->n_id.p, fe->obs.p, fe->n_obs.p, region_of(fe));
    else
      hipLaunchKernelGGL(corner_select_subset_kernel<>, dim3(n_pub + RP.n_wg), dim3(kSelThreads), 0, st, M, n_pub, fe->cand.p, fe->seg_cap, fe->nseg,
                         fe->n_cand.p, fe->max_bits.p, RP, fe->cfg.quality_level, SP, fe->forw_pts.p, fe->cur_pts.p, fe->pre_pts.p, fe->ids.p,
                         fe->track_cnt.p, fe->n_forw.p, fe->n_pts.p, fe->n_id.p, fe->obs.p, fe->n_obs.p);
  }
  // image_msg in the call's order: only these rows travel back
  hipLaunchKernelGGL(gather_obs_subset_kernel, dim3(n), dim3(256), 0, st, M, cap, fe->obs.p, fe->n_obs.p, fe->obs_sub.p, fe->n_obs_sub.p);
  HIP_OK(hipGetLastError());
  return VIO_OK;
}

}  // namespace

extern "C" {

int vio_frontend_create(const VioConfig *cfg, int32_t n_seq, vio_frontend_t **out) {
  if (!cfg || !out || n_seq < 1) return VIO_EINVAL;
  if (cfg->lk_win != kWin || cfg->lk_levels < 0 || cfg->lk_levels >= kMaxLevels || cfg->max_corners < 1 ||
      cfg->max_corners > kMaxCap || cfg->image_rows < 32 || cfg->image_cols < 32 || cfg->min_dist < 0 || cfg->min_dist > kMaxRadius ||
      cfg->image_rows > 32767 || cfg->image_cols > 65535)  // (corner candidates carry their position as y << 16 | x)
    return VIO_EINVAL;
  if (!vio::device_ready("the front-end")) return VIO_ENODEV;
  vio_frontend *fe = new vio_frontend();
  fe->device = vio::current_device();
  fe->cfg = *cfg, fe->n_seq = n_seq, fe->cap = cfg->max_corners;
  fe->detect_always = vio::env_flag("VIO_AMD_DETECT_ALWAYS");
  fe->cs_prof = vio::env_flag("VIO_AMD_CS_PROF") && fe->d_cs_prof.ensure(8) == VIO_OK;
  // buildOpticalFlowPyramid: levels stop when one would not hold the window
  LevelDims &ld = fe->ld;
  ld.rows[0] = cfg->image_rows, ld.cols[0] = cfg->image_cols, ld.off[0] = 0, ld.levels = 1;
  size_t off = (size_t)ld.rows[0] * ld.cols[0];
  for (int l = 1; l <= cfg->lk_levels; l++) {
    int r = (ld.rows[l - 1] + 1) / 2, c = (ld.cols[l - 1] + 1) / 2;
    if (c <= kWin || r <= kWin) break;
    ld.rows[l] = r, ld.cols[l] = c, ld.off[l] = off, off += (size_t)r * c, ld.levels = l + 1;
  }
  ld.pyr_bytes = (off + 255) & ~(size_t)255;
  const size_t S = n_seq, cap = fe->cap;
  fe->nseg = (cfg->image_rows + kDetR - 1) / kDetR;
  if (fe->nseg > kSelMaxSeg) {
    delete fe;
    return VIO_ECAP;
  }
  // a STRICT 3x3 local maximum occupies at most one pixel in four. Equal neighbours are all candidates (a plateau): a strip that
  // has more of them than this raises the sequence's flag and the sequence is redone from a full-size list (corner_select_kernel)
  fe->seg_cap = kDetR * cfg->image_cols / 4;
  fe->n_redo_wg = (int)std::min<size_t>(S, kRedoSlots);
  fe->redo_report = vio::env_flag("VIO_AMD_REDO_REPORT");
  if (hipStreamCreateWithFlags(&fe->stream, hipStreamNonBlocking) != hipSuccess) {
    delete fe;
    return VIO_ENODEV;
  }
  if (fe->pyr[0].ensure(S * ld.pyr_bytes) != VIO_OK || fe->pyr[1].ensure(S * ld.pyr_bytes) != VIO_OK ||
      fe->max_bits.ensure(S * fe->nseg) != VIO_OK || fe->cand.ensure(S * fe->nseg * fe->seg_cap) != VIO_OK ||
      fe->n_cand.ensure(S * fe->nseg) != VIO_OK || fe->ovf.ensure(S) != VIO_OK || fe->n_redo.ensure(1) != VIO_OK ||
      fe->redo_full.ensure((size_t)fe->n_redo_wg * cfg->image_rows * cfg->image_cols) != VIO_OK || fe->cur_pts.ensure(S * cap * 2) != VIO_OK ||
      fe->pre_pts.ensure(S * cap * 2) != VIO_OK || fe->forw_pts.ensure(S * cap * 2) != VIO_OK || fe->lk_err.ensure(S * cap) != VIO_OK ||
      fe->ids.ensure(S * cap) != VIO_OK || fe->track_cnt.ensure(S * cap) != VIO_OK || fe->n_pts.ensure(S) != VIO_OK ||
      fe->n_forw.ensure(S) != VIO_OK || fe->n_id.ensure(S) != VIO_OK || fe->kept_xy.ensure(S * cap * 2) != VIO_OK ||
      fe->n_kept.ensure(S) != VIO_OK || fe->pnp_pts.ensure(S * cap * 2) != VIO_OK || fe->pnp_ids.ensure(S * cap) != VIO_OK ||
      fe->n_pnp.ensure(S) != VIO_OK || fe->n_obs.ensure(S) != VIO_OK || fe->lk_status.ensure(S * cap) != VIO_OK ||
      fe->obs.ensure(S * cap) != VIO_OK || fe->hw.ensure((size_t)2 * cfg->min_dist + 1) != VIO_OK || fe->cam.ensure(S * 4) != VIO_OK) {
    delete fe;
    return VIO_ENOMEM;
  }
  std::vector<int> hw;
  circle_halfwidths(cfg->min_dist, hw);
  fe->h_cam.resize(S * 4);
  for (size_t q = 0; q < S; q++) fe->h_cam[4 * q] = cfg->fx, fe->h_cam[4 * q + 1] = cfg->fy, fe->h_cam[4 * q + 2] = cfg->cx, fe->h_cam[4 * q + 3] = cfg->cy;
  if (hipMemcpy(fe->hw.p, hw.data(), hw.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(fe->cam.p, fe->h_cam.data(), fe->h_cam.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(fe->max_bits.p, 0, sizeof(unsigned) * S * fe->nseg) != hipSuccess ||
      hipMemset(fe->n_cand.p, 0, sizeof(int) * S * fe->nseg) != hipSuccess || hipMemset(fe->n_pts.p, 0, sizeof(int) * S) != hipSuccess ||
      hipMemset(fe->ovf.p, 0, sizeof(int) * S) != hipSuccess || hipMemset(fe->n_redo.p, 0, sizeof(int)) != hipSuccess ||
      hipMemset(fe->n_forw.p, 0, sizeof(int) * S) != hipSuccess || hipMemset(fe->n_id.p, 0, sizeof(int) * S) != hipSuccess ||
      hipMemset(fe->n_kept.p, 0, sizeof(int) * S) != hipSuccess || hipMemset(fe->n_pnp.p, 0, sizeof(int) * S) != hipSuccess ||
      hipMemset(fe->n_obs.p, 0, sizeof(int) * S) != hipSuccess) {
    delete fe;
    return VIO_ENODEV;
  }
  *out = fe;
  return VIO_OK;
}

int vio_frontend_get_device(const vio_frontend_t *fe, int32_t *device) {
  if (!fe || !device) return VIO_EINVAL;
  *device = fe->device;
  return VIO_OK;
}

void vio_frontend_destroy(vio_frontend_t *fe) {
  if (!fe) return;
  vio::DeviceScope scope(fe->device);
  delete fe;
}

int vio_frontend_upload_frames(vio_frontend_t *fe, const uint8_t *gray, int32_t n_frames, int32_t rows, int32_t cols,
                               int32_t stride) {
  if (!fe || !gray || n_frames < 1) return VIO_EINVAL;
  if (rows != fe->cfg.image_rows || cols != fe->cfg.image_cols || stride < cols) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(fe);
  const size_t px = (size_t)rows * cols, total = (size_t)n_frames * fe->n_seq;
  if (fe->pending) return VIO_ESTATE;
  // the current image may still be read in place from the ring that is about to go: it moves into its pyramid first
  HIP_OK(hipDeviceSynchronize());
  const int rco = own_level0(fe);
  if (rco != VIO_OK) return rco;
  fe->frames.release();  // (exactly the new size)
  if (fe->frames.ensure(total * px) != VIO_OK) return VIO_ENOMEM;
  HIP_OK(hipMemcpy2D(fe->frames.p, cols, gray, stride, cols, total * rows, hipMemcpyHostToDevice));
  fe->n_frames = n_frames;
  return VIO_OK;
}

int vio_frontend_step_resident(vio_frontend_t *fe, int32_t frame_index, int32_t publish, void *stream) {
  if (!fe) return VIO_EINVAL;
  if (!fe->frames.p || frame_index < 0 || frame_index >= fe->n_frames) return VIO_ESTATE;
  if (fe->pending) return VIO_ESTATE;  // a submitted frame owns the tracker state and the observation staging until it is collected
  if (!fe->in_step) return VIO_ESTATE;  // subset calls or resets left the sequences in different phases (vio_frontend_in_step)
  VIO_ON_DEVICE_OF(fe);
  hipStream_t st = stream ? (hipStream_t)stream : fe->stream;
  if (st != fe->stream) fe->foreign_stream = true;
  int rc = fe->timer.begin(st);
  if (rc != VIO_OK) return rc;
  const size_t px = (size_t)fe->cfg.image_rows * fe->cfg.image_cols;
  rc = fe_step(fe, fe->frames.p + (size_t)frame_index * fe->n_seq * px, publish, st, true);
  if (rc != VIO_OK) return rc;
  return fe->timer.end(st);
}

int vio_frontend_sync(vio_frontend_t *fe) {
  if (!fe) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(fe);
  HIP_OK(hipDeviceSynchronize());
  return VIO_OK;
}

int vio_frontend_kernel_ms(vio_frontend_t *fe, double *ms_avg, int32_t *launches) {
  if (!fe || !ms_avg || !launches) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(fe);
  HIP_OK(hipDeviceSynchronize());
  return fe->timer.drain(ms_avg, launches);
}

// Host buffers the caller registered (vio_host_register): page-locked in place, so their frames go to the device by DMA straight
// from where the camera / decoder wrote them -- no gathering pass over them on the host pool.
namespace {
struct HostRange {
  const uint8_t *p;
  size_t n;
};
std::mutex g_host_reg_m;
std::vector<HostRange> g_host_reg;
bool host_range_registered(const void *ptr, size_t bytes) {
  const uint8_t *b = static_cast<const uint8_t *>(ptr);
  std::lock_guard<std::mutex> lk(g_host_reg_m);
  for (const HostRange &r : g_host_reg)
    if (b >= r.p && b + bytes <= r.p + r.n) return true;
  return false;
}
}  // namespace

int vio_host_register(void *ptr, size_t bytes) {
  if (!ptr || bytes == 0) return VIO_EINVAL;
  if (!vio::device_ready("host-buffer registration")) return VIO_ENODEV;
  {
    std::lock_guard<std::mutex> lk(g_host_reg_m);
    const uint8_t *b = static_cast<const uint8_t *>(ptr);
    for (const HostRange &r : g_host_reg)
      if (b < r.p + r.n && r.p < b + bytes) return VIO_ESTATE;  // overlaps a registered range: unregister that one first
  }
  if (hipHostRegister(ptr, bytes, hipHostRegisterPortable) != hipSuccess) {
    (void)hipGetLastError();
    return VIO_ENOMEM;  // (the pages could not be locked: RLIMIT_MEMLOCK, or not the caller's memory)
  }
  std::lock_guard<std::mutex> lk(g_host_reg_m);
  g_host_reg.push_back({static_cast<const uint8_t *>(ptr), bytes});
  return VIO_OK;
}

int vio_host_unregister(void *ptr) {
  if (!ptr) return VIO_EINVAL;
  {
    std::lock_guard<std::mutex> lk(g_host_reg_m);
    size_t i = 0;
    for (; i < g_host_reg.size(); i++)
      if (g_host_reg[i].p == static_cast<const uint8_t *>(ptr)) break;
    if (i == g_host_reg.size()) return VIO_ESTATE;
    g_host_reg.erase(g_host_reg.begin() + (long)i);
  }
  // (a transfer still queued from this range must not lose its pages under it)
  if (hipDeviceSynchronize() != hipSuccess || hipHostUnregister(ptr) != hipSuccess) {
    (void)hipGetLastError();
    return VIO_ENODEV;
  }
  return VIO_OK;
}

// The two halves of read_images. submit: gathers the caller's (pageable) frames into page-locked memory, queues their
// transfer, every kernel of the frame and the copy of the published observations on the context's stream and returns
// without waiting for the device; collect: waits and hands the observations over. A caller that submits frame k+1 before
// it runs the estimator on frame k overlaps the front-end's transfers and kernels with the estimator's host phases.
static int submit_body(vio_frontend_t *fe, const uint8_t *gray, int32_t rows, int32_t cols, int32_t stride, int32_t publish) {
  VIO_ON_DEVICE_OF(fe);
  const size_t px = (size_t)rows * cols, S = fe->n_seq;
  // host frames land in a device staging buffer kept for the life of the context; observations come back through
  // pinned host memory (no allocation, no pageable bounce on the return path)
  if (fe->d_stage.ensure(S * px) != VIO_OK) return VIO_ENOMEM;
  if (fe->p_obs.ensure(S * fe->cap) != VIO_OK || fe->p_nobs.ensure(S) != VIO_OK) return VIO_ENOMEM;
  hipStream_t st = fe->stream;
  // The caller's frames are pageable memory: a direct copy bounces through the runtime's staging at ~5 GB/s. They are
  // gathered into page-locked memory by the host pool (one sequence per task, rows packed) in a few chunks, each chunk
  // going to the device as soon as it is complete, so the DMA of one overlaps the gathering of the next.
  if (stride == cols && host_range_registered(gray, S * px)) {
    // frames in a buffer the caller registered: one DMA from where they are
    HIP_OK(hipMemcpyAsync(fe->d_stage.p, gray, S * px, hipMemcpyHostToDevice, st));
  } else {
    if (fe->p_frames.ensure(S * px) != VIO_OK) return VIO_ENOMEM;
    const size_t n_chunks = S >= 32 ? 8 : 1, per = (S + n_chunks - 1) / n_chunks;
    for (size_t c0 = 0; c0 < S; c0 += per) {
      const size_t c1 = std::min(S, c0 + per);
      vio::HostPool::get().parallel_for((int)(c1 - c0), [&](int i) {
        const size_t s = c0 + i;
        const uint8_t *src = gray + s * (size_t)rows * stride;
        uint8_t *dst = fe->p_frames.p + s * px;
        if (stride == cols) memcpy(dst, src, px);
        else
          for (int r = 0; r < rows; r++) memcpy(dst + (size_t)r * cols, src + (size_t)r * stride, cols);
      });
      HIP_OK(hipMemcpyAsync(fe->d_stage.p + c0 * px, fe->p_frames.p + c0 * px, (c1 - c0) * px, hipMemcpyHostToDevice, st));
    }
  }
  int rc = fe_step(fe, fe->d_stage.p, publish, st);
  if (rc != VIO_OK) return rc;
  if (publish) {
    HIP_OK(hipMemcpyAsync(fe->p_obs.p, fe->obs.p, sizeof(VioObs) * S * fe->cap, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(fe->p_nobs.p, fe->n_obs.p, sizeof(int) * S, hipMemcpyDeviceToHost, st));
  }
  return VIO_OK;
}

int vio_frontend_submit_images(vio_frontend_t *fe, const uint8_t *gray, int32_t rows, int32_t cols, int32_t stride, int32_t publish) {
  if (!fe || !gray) return VIO_EINVAL;
  if (rows != fe->cfg.image_rows || cols != fe->cfg.image_cols || stride < cols) return VIO_EINVAL;
  if (fe->pending) return VIO_ESTATE;  // one frame in flight per context: collect it first
  if (!fe->in_step) return VIO_ESTATE;  // (vio_frontend_in_step)
  const int rc = submit_body(fe, gray, rows, cols, stride, publish);
  if (rc != VIO_OK) return rc;
  fe->pending = true, fe->pending_publish = publish != 0, fe->pending_async = false;
  return VIO_OK;
}

// The same with the submit's host work (gathering the frames into page-locked memory, queueing the transfers and the
// kernels) on the context's own host thread: the call returns at once, `gray` must stay valid and unchanged until
// vio_frontend_collect, which reports what the submit returned.
int vio_frontend_submit_images_async(vio_frontend_t *fe, const uint8_t *gray, int32_t rows, int32_t cols, int32_t stride, int32_t publish) {
  if (!fe || !gray) return VIO_EINVAL;
  if (rows != fe->cfg.image_rows || cols != fe->cfg.image_cols || stride < cols) return VIO_EINVAL;
  if (fe->pending) return VIO_ESTATE;
  if (!fe->in_step) return VIO_ESTATE;
  try {
    if (!fe->async) {
      fe->async = new vio_frontend::Async();
      vio_frontend::Async *a = fe->async;
      a->th = std::thread([fe, a] {
        for (;;) {
          std::unique_lock<std::mutex> lk(a->m);
          a->cv.wait(lk, [&] { return a->quit || a->has_job; });
          if (a->quit) return;
          a->has_job = false;
          lk.unlock();
          const int rc = submit_body(fe, a->gray, a->rows, a->cols, a->stride, a->publish);
          lk.lock();
          a->rc = rc, a->busy = false;
          lk.unlock();
          a->cv.notify_all();
        }
      });
    }
  } catch (...) {
    return VIO_ENOMEM;
  }
  vio_frontend::Async *a = fe->async;
  {
    std::lock_guard<std::mutex> lk(a->m);
    a->gray = gray, a->rows = rows, a->cols = cols, a->stride = stride, a->publish = publish;
    a->has_job = true, a->busy = true, a->rc = VIO_OK;
  }
  a->cv.notify_all();
  fe->pending = true, fe->pending_publish = publish != 0, fe->pending_async = true;
  return VIO_OK;
}

int vio_frontend_collect(vio_frontend_t *fe, VioObs *out_obs, int32_t *n_obs) {
  if (!fe || !n_obs) return VIO_EINVAL;
  if (!fe->pending || fe->pending_subset) return VIO_ESTATE;  // (a subset submit is collected by vio_frontend_collect_subset)
  if (fe->pending_publish && !out_obs) return VIO_EINVAL;
  if (fe->async && fe->pending_async) {  // an asynchronous submit finishes queueing first (a->rc belongs to THAT submit only)
    vio_frontend::Async *a = fe->async;
    std::unique_lock<std::mutex> lk(a->m);
    a->cv.wait(lk, [&] { return !a->busy; });
    if (a->rc != VIO_OK) {
      fe->pending = false;
      return a->rc;
    }
  }
  VIO_ON_DEVICE_OF(fe);
  fe->pending = false;
  HIP_OK(hipStreamSynchronize(fe->stream));
  const size_t S = fe->n_seq;
  for (size_t s = 0; s < S; s++) n_obs[s] = 0;
  if (fe->pending_publish)
    for (size_t s = 0; s < S; s++) {
      n_obs[s] = fe->p_nobs.p[s];
      memcpy(out_obs + s * fe->cap, fe->p_obs.p + s * fe->cap, sizeof(VioObs) * fe->p_nobs.p[s]);
    }
  return VIO_OK;
}

int vio_frontend_read_images(vio_frontend_t *fe, const uint8_t *gray, int32_t rows, int32_t cols, int32_t stride,
                             const double *headers, int32_t publish, VioObs *out_obs, int32_t *n_obs) {
  (void)headers;  // the reference only forwards the header to the (default-off) vinsPnP branch
  if (!fe || !gray || !n_obs || (publish && !out_obs)) return VIO_EINVAL;
  int rc = vio_frontend_submit_images(fe, gray, rows, cols, stride, publish);
  if (rc != VIO_OK) return rc;
  return vio_frontend_collect(fe, out_obs, n_obs);
}

int vio_frontend_read_image(vio_frontend_t *fe, int32_t seq, const uint8_t *gray, int32_t rows, int32_t cols, int32_t stride,
                            double header, int32_t publish, VioObs *out_obs, int32_t *n_obs, VioTrackViz *viz) {
  (void)seq, (void)viz;
  if (!fe || fe->n_seq != 1 || seq != 0) return VIO_EINVAL;  // single-sequence contexts only; batches use read_images
  return vio_frontend_read_images(fe, gray, rows, cols, stride, &header, publish, out_obs, n_obs);
}

// ---- frames for a subset of the sequences, per-sequence publish, reset (fe_subset.h plans, fe_step_subset launches) -----------
int vio_frontend_submit_subset(vio_frontend_t *fe, int32_t n, const int32_t *seq, const void *frames, int32_t frames_on_device,
                               const int32_t *frame_index, int32_t rows, int32_t cols, int32_t stride, const uint8_t *publish) {
  if (!fe || n < 0 || n > fe->n_seq) return VIO_EINVAL;
  if (rows != fe->cfg.image_rows || cols != fe->cfg.image_cols || stride < cols) return VIO_EINVAL;
  if (n > 0 && (!seq || !frames || !publish)) return VIO_EINVAL;
  if (frames_on_device ? stride != cols : frame_index != nullptr) return VIO_EINVAL;  // (packed slots; host frames lie in call order)
  if (fe->pending) return VIO_ESTATE;  // one frame in flight per context, lock-step or subset
  VIO_ON_DEVICE_OF(fe);
  phase_from_lockstep(fe);
  const size_t S = fe->n_seq, px = (size_t)rows * cols;
  if (fe->p_arena.ensure(fe_subset::arena_ints((int)S)) != VIO_OK || fe->d_arena.ensure(fe_subset::arena_ints((int)S)) != VIO_OK) return VIO_ENOMEM;
  const fe_subset::Arena H = fe_subset::carve(fe->p_arena.p, n);
  int n_pub = 0;
  if (!fe_subset::plan((int)S, fe->ph_bank.data(), fe->ph_have.data(), n, seq, frame_index, -1, publish, fe->ph_seen.data(), H, &n_pub))
    return VIO_EINVAL;  // (nothing was changed)
  fe->pending = true, fe->pending_subset = true, fe->pending_async = false, fe->pending_publish = n_pub > 0;
  fe->pending_n = n, fe->pending_pub = n_pub;
  if (n == 0) return VIO_OK;  // nothing to launch: collect_subset hands back nothing
  auto fail = [&](int rc) {
    fe->pending = fe->pending_subset = false;
    return rc;
  };
  hipStream_t st = fe->stream;
  if (fe->foreign_stream) {  // (a lock-step step on a caller's stream may still be running)
    if (hipDeviceSynchronize() != hipSuccess) return fail(VIO_ENODEV);
    fe->foreign_stream = false;
  }
  int rc = own_level0(fe);
  if (rc != VIO_OK) return fail(rc);
  if (fe->p_obs.ensure(S * fe->cap) != VIO_OK || fe->p_nobs.ensure(S) != VIO_OK || fe->obs_sub.ensure(S * fe->cap) != VIO_OK ||
      fe->n_obs_sub.ensure(S) != VIO_OK)
    return fail(VIO_ENOMEM);
  const uint8_t *d_frames = static_cast<const uint8_t *>(frames);
  if (!frames_on_device) {
    const uint8_t *gray = static_cast<const uint8_t *>(frames);
    if (fe->d_stage.ensure(S * px) != VIO_OK) return fail(VIO_ENOMEM);
    if (stride == cols && host_range_registered(gray, (size_t)n * px)) {
      if (hipMemcpyAsync(fe->d_stage.p, gray, (size_t)n * px, hipMemcpyHostToDevice, st) != hipSuccess) return fail(VIO_ENODEV);
    } else {  // the gather of read_images, over the call's n frames
      if (fe->p_frames.ensure(S * px) != VIO_OK) return fail(VIO_ENOMEM);
      const size_t N = n, n_chunks = N >= 32 ? 8 : 1, per = (N + n_chunks - 1) / n_chunks;
      for (size_t c0 = 0; c0 < N; c0 += per) {
        const size_t c1 = std::min(N, c0 + per);
        vio::HostPool::get().parallel_for((int)(c1 - c0), [&](int i) {
          const size_t s = c0 + i;
          const uint8_t *src = gray + s * (size_t)rows * stride;
          uint8_t *dst = fe->p_frames.p + s * px;
          if (stride == cols) memcpy(dst, src, px);
          else
            for (int r = 0; r < rows; r++) memcpy(dst + (size_t)r * cols, src + (size_t)r * stride, cols);
        });
        if (hipMemcpyAsync(fe->d_stage.p + c0 * px, fe->p_frames.p + c0 * px, (c1 - c0) * px, hipMemcpyHostToDevice, st) != hipSuccess)
          return fail(VIO_ENODEV);
      }
    }
    d_frames = fe->d_stage.p;
  }
  if (frames_on_device && (rc = fe->timer.begin(st)) != VIO_OK) return fail(rc);  // (vio_frontend_kernel_ms, as step_resident)
  if (hipMemcpyAsync(fe->d_arena.p, fe->p_arena.p, sizeof(int32_t) * fe_subset::arena_ints(n), hipMemcpyHostToDevice, st) != hipSuccess)
    return fail(VIO_ENODEV);
  const fe_subset::Arena D = fe_subset::carve(fe->d_arena.p, n);
  SubsetArgs M;
  M.seq = D.seq, M.slot = D.slot, M.prev_bank = D.prev_bank, M.forw_bank = D.forw_bank, M.publish = D.publish, M.pub = D.pub;
  M.pyr[0] = fe->pyr[0].p, M.pyr[1] = fe->pyr[1].p;
  if ((rc = fe_step_subset(fe, M, n, n_pub, d_frames, st)) != VIO_OK) return fail(rc);
  if (frames_on_device && (rc = fe->timer.end(st)) != VIO_OK) return fail(rc);
  if (hipMemcpyAsync(fe->p_nobs.p, fe->n_obs_sub.p, sizeof(int) * n, hipMemcpyDeviceToHost, st) != hipSuccess) return fail(VIO_ENODEV);
  if (n_pub > 0 && hipMemcpyAsync(fe->p_obs.p, fe->obs_sub.p, sizeof(VioObs) * (size_t)n * fe->cap, hipMemcpyDeviceToHost, st) != hipSuccess)
    return fail(VIO_ENODEV);
  fe_subset::commit(fe->ph_bank.data(), fe->ph_have.data(), n, H);
  phase_to_lockstep(fe);
  return VIO_OK;
}

int vio_frontend_collect_subset(vio_frontend_t *fe, VioObs *out_obs, int32_t *n_obs) {
  if (!fe) return VIO_EINVAL;
  if (!fe->pending || !fe->pending_subset) return VIO_ESTATE;  // (a lock-step submit is collected by vio_frontend_collect)
  const size_t n = fe->pending_n;
  if (n > 0 && (!n_obs || (fe->pending_pub > 0 && !out_obs))) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(fe);
  fe->pending = fe->pending_subset = false;
  if (n == 0) return VIO_OK;
  HIP_OK(hipStreamSynchronize(fe->stream));
  for (size_t i = 0; i < n; i++) {
    n_obs[i] = fe->p_nobs.p[i];
    if (n_obs[i] > 0) memcpy(out_obs + i * fe->cap, fe->p_obs.p + i * fe->cap, sizeof(VioObs) * n_obs[i]);
  }
  return VIO_OK;
}

int vio_frontend_read_subset(vio_frontend_t *fe, int32_t n, const int32_t *seq, const void *frames, int32_t frames_on_device,
                             const int32_t *frame_index, int32_t rows, int32_t cols, int32_t stride, const uint8_t *publish,
                             VioObs *out_obs, int32_t *n_obs) {
  if (n > 0 && (!n_obs || !out_obs)) return VIO_EINVAL;
  const int rc = vio_frontend_submit_subset(fe, n, seq, frames, frames_on_device, frame_index, rows, cols, stride, publish);
  if (rc != VIO_OK) return rc;
  return vio_frontend_collect_subset(fe, out_obs, n_obs);
}

int vio_frontend_reset(vio_frontend_t *fe, int32_t n, const int32_t *seq) {
  if (!fe) return VIO_EINVAL;
  if (fe->pending) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(fe);
  phase_from_lockstep(fe);
  const int S = fe->n_seq;
  if (seq && !fe_subset::valid_list(S, n, seq, fe->ph_seen.data())) return VIO_EINVAL;
  if (seq && n == 0) return VIO_OK;
  HIP_OK(hipDeviceSynchronize());  // (rare: whatever stream the last step ran on)
  fe->foreign_stream = false;
  int rc = VIO_OK;
  if (!seq) {  // all of them: the aliased images go with their sequences
    fe->lvl0[0] = fe->lvl0[1] = nullptr;
    for (int *p : {fe->n_pts.p, fe->n_forw.p, fe->n_id.p, fe->n_pnp.p, fe->n_kept.p, fe->ovf.p}) HIP_OK(hipMemsetAsync(p, 0, sizeof(int) * S, fe->stream));
  } else {
    if ((rc = own_level0(fe)) != VIO_OK) return rc;
    if (fe->p_arena.ensure(fe_subset::arena_ints(S)) != VIO_OK || fe->d_arena.ensure(fe_subset::arena_ints(S)) != VIO_OK) return VIO_ENOMEM;
    memcpy(fe->p_arena.p, seq, sizeof(int32_t) * n);
    HIP_OK(hipMemcpyAsync(fe->d_arena.p, fe->p_arena.p, sizeof(int32_t) * n, hipMemcpyHostToDevice, fe->stream));
    hipLaunchKernelGGL(reset_sequences_kernel, dim3((n + 255) / 256), dim3(256), 0, fe->stream, fe->d_arena.p, n, fe->n_pts.p, fe->n_forw.p,
                       fe->n_id.p, fe->n_pnp.p, fe->n_kept.p, fe->ovf.p);
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipStreamSynchronize(fe->stream));
  fe_subset::reset(S, fe->ph_bank.data(), fe->ph_have.data(), n, seq);
  phase_to_lockstep(fe);
  return VIO_OK;
}

// The camera of a sequence is what image_msg divides by (feature_tracker.cpp:300-306; FOCUS_LENGTH_X/Y, PX, PY are per device,
// global_param.cpp:24-131). The table is rewritten between steps only: every launch that reads it has been collected.
int vio_frontend_set_cameras(vio_frontend_t *fe, int32_t n, const int32_t *seq, const VioCamera *cam) {
  if (!fe || n < 0 || (n > 0 && (!seq || !cam))) return VIO_EINVAL;
  if (fe->pending) return VIO_ESTATE;
  const int S = fe->n_seq;
  std::vector<uint8_t> seen(S, 0);
  if (!fe_subset::valid_list(S, n, seq, seen.data())) return VIO_EINVAL;
  for (int i = 0; i < n; i++)
    if (!vio::camera_valid(cam[i], false)) return VIO_EINVAL;
  if (n == 0) return VIO_OK;
  VIO_ON_DEVICE_OF(fe);
  // a step that is not collected through this context may still read the table: vio_frontend_step_resident on the context's
  // stream, or on a caller's (only then the whole device is waited for: sessions that join one by one must not stall the others)
  if (fe->foreign_stream) {
    HIP_OK(hipDeviceSynchronize());
    fe->foreign_stream = false;
  } else {
    HIP_OK(hipStreamSynchronize(fe->stream));
  }
  for (int i = 0; i < n; i++) {
    double *row = &fe->h_cam[4 * (size_t)seq[i]];
    row[0] = cam[i].fx, row[1] = cam[i].fy, row[2] = cam[i].cx, row[3] = cam[i].cy;
  }
  HIP_OK(hipMemcpy(fe->cam.p, fe->h_cam.data(), fe->h_cam.size() * sizeof(double), hipMemcpyHostToDevice));
  return VIO_OK;
}

int vio_frontend_get_camera(vio_frontend_t *fe, int32_t seq, VioCamera *out) {
  if (!fe || seq < 0 || seq >= fe->n_seq || !out) return VIO_EINVAL;
  const double *row = &fe->h_cam[4 * (size_t)seq];
  memset(out, 0, sizeof(*out));
  out->fx = row[0], out->fy = row[1], out->cx = row[2], out->cy = row[3];
  out->ric[0] = out->ric[4] = out->ric[8] = 1.0;  // (the front end has no use for the extrinsic)
  return VIO_OK;
}

// The region of interest of a sequence is what setMask starts from on a publish frame (feature_tracker.cpp:50-87 with the
// static mask of the upstream family in place of the all-255 one). Like the camera table it is rewritten between steps only.
int vio_frontend_set_regions(vio_frontend_t *fe, int32_t n, const int32_t *seq, const void *masks, int32_t masks_on_device,
                             const int32_t *mask_index) {
  if (!fe || n < 0 || (n > 0 && !seq)) return VIO_EINVAL;
  if (fe->pending) return VIO_ESTATE;
  const int S = fe->n_seq, rows = fe->cfg.image_rows, cols = fe->cfg.image_cols;
  std::vector<uint8_t> seen(S, 0);
  if (!fe_subset::valid_list(S, n, seq, seen.data())) return VIO_EINVAL;
  if (masks && mask_index)
    for (int i = 0; i < n; i++)
      if (mask_index[i] < 0) return VIO_EINVAL;
  if (n == 0) return VIO_OK;
  VIO_ON_DEVICE_OF(fe);
  // a step that still runs reads the table, and a caller's device buffer may still be written on a stream of the caller's
  HIP_OK(hipDeviceSynchronize());
  fe->foreign_stream = false;
  if (!fe->region_words.p) {
    if (!masks) return VIO_OK;  // nothing was ever set
    const int wpr = (cols + 63) / 64 + 2;
    if (fe->region_words.ensure((size_t)S * rows * wpr) != VIO_OK || fe->region_set.ensure(S) != VIO_OK) {
      fe->region_words.release();
      return VIO_ENOMEM;
    }
    fe->region_wpr = wpr;
    fe->h_region_set.assign(S, 0);
    HIP_OK(hipMemset(fe->region_set.p, 0, sizeof(int) * S));
  }
  if (masks) {
    const size_t px = (size_t)rows * cols;
    DevBuf<uint8_t> d_masks;  // the host route's staging, gone when the call returns
    DevBuf<int> d_list;       // mask index | sequence of every entry
    std::vector<int> list(2 * (size_t)n);
    for (int i = 0; i < n; i++) list[i] = masks_on_device && mask_index ? mask_index[i] : i, list[n + i] = seq[i];
    if (d_list.ensure(2 * (size_t)n) != VIO_OK) return VIO_ENOMEM;
    const uint8_t *src = static_cast<const uint8_t *>(masks);
    if (!masks_on_device) {
      if (d_masks.ensure((size_t)n * px) != VIO_OK) return VIO_ENOMEM;
      for (int i = 0; i < n; i++)  // image mask_index[i] of the caller's array -> staging image i
        HIP_OK(hipMemcpy(d_masks.p + (size_t)i * px, src + (size_t)(mask_index ? mask_index[i] : i) * px, px, hipMemcpyHostToDevice));
      src = d_masks.p;
    }
    HIP_OK(hipMemcpy(d_list.p, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(region_pack_kernel, dim3((rows * fe->region_wpr + 255) / 256, n), dim3(256), 0, fe->stream, src, (const int *)d_list.p,
                       (const int *)d_list.p + n, rows, cols, fe->region_wpr, fe->region_words.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(fe->stream));
  }
  for (int i = 0; i < n; i++) fe->h_region_set[seq[i]] = masks ? 1 : 0;
  HIP_OK(hipMemcpy(fe->region_set.p, fe->h_region_set.data(), sizeof(int) * S, hipMemcpyHostToDevice));
  fe->n_region = 0;
  for (int s = 0; s < S; s++) fe->n_region += fe->h_region_set[s];
  return VIO_OK;
}

int vio_frontend_get_region(vio_frontend_t *fe, int32_t seq, uint8_t *mask_out, int32_t *is_set, int64_t *n_usable) {
  if (!fe || seq < 0 || seq >= fe->n_seq || !is_set || !n_usable) return VIO_EINVAL;
  if (fe->pending) return VIO_ESTATE;
  const int rows = fe->cfg.image_rows, cols = fe->cfg.image_cols;
  const size_t px = (size_t)rows * cols;
  if (!fe->region_words.p || !fe->h_region_set[seq]) {  // no region: every pixel is usable
    *is_set = 0, *n_usable = (int64_t)px;
    if (mask_out) memset(mask_out, 255, px);
    return VIO_OK;
  }
  VIO_ON_DEVICE_OF(fe);
  const int wpr = fe->region_wpr;
  std::vector<unsigned long long> words((size_t)rows * wpr);
  HIP_OK(hipMemcpy(words.data(), fe->region_words.p + (size_t)seq * rows * wpr, sizeof(unsigned long long) * words.size(), hipMemcpyDeviceToHost));
  int64_t usable = 0;
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      const int bit = (int)((words[(size_t)y * wpr + ((x + 64) >> 6)] >> ((x + 64) & 63)) & 1ull);
      usable += bit;
      if (mask_out) mask_out[(size_t)y * cols + x] = bit ? 255 : 0;
    }
  *is_set = 1, *n_usable = usable;
  return VIO_OK;
}

int vio_frontend_in_step(vio_frontend_t *fe, int32_t *in_step) {
  if (!fe || !in_step) return VIO_EINVAL;
  *in_step = fe->in_step ? 1 : 0;
  return VIO_OK;
}

int vio_frontend_get_state(vio_frontend_t *fe, int32_t seq, float *cur_pts, int32_t *ids, int32_t *track_cnt, int32_t cap,
                           int32_t *n) {
  if (!fe || seq < 0 || seq >= fe->n_seq || !n) return VIO_EINVAL;
  if (fe->pending) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(fe);
  HIP_OK(hipDeviceSynchronize());
  int m = 0;
  HIP_OK(hipMemcpy(&m, fe->n_pts.p + seq, sizeof(int), hipMemcpyDeviceToHost));
  *n = m;
  if (m > cap) return VIO_ECAP;
  const size_t base = (size_t)seq * fe->cap;
  if (m > 0) {
    HIP_OK(hipMemcpy(cur_pts, fe->cur_pts.p + base * 2, sizeof(float) * 2 * m, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ids, fe->ids.p + base, sizeof(int) * m, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(track_cnt, fe->track_cnt.p + base, sizeof(int) * m, hipMemcpyDeviceToHost));
  }
  return VIO_OK;
}

// forw_pts / ids at the point of readImage where solveVinsPnP runs (feature_tracker.cpp:207): the tracked points behind
// the first F-RANSAC of the last frame, ahead of rejectWithF / setMask. A frame that tracked nothing (the first one)
// leaves the list empty.
int vio_frontend_lk_iterations(vio_frontend_t *fe, int32_t enable, uint64_t *iterations, uint64_t *visits, int32_t levels_cap) {
  if (!fe || (iterations && (!visits || levels_cap < 1))) return VIO_EINVAL;
  if (fe->pending) return VIO_ESTATE;  // (a submitted frame's worker reads lk_stats_on / lk_stats while it queues the step)
  VIO_ON_DEVICE_OF(fe);
  constexpr int kSlots = 16 * 64;  // 64 copies of [iterations (levels) | visits (levels)], summed here
  if (!fe->lk_stats.p) {
    if (fe->lk_stats.ensure(kSlots) != VIO_OK) return VIO_ENOMEM;
    HIP_OK(hipMemset(fe->lk_stats.p, 0, sizeof(unsigned long long) * kSlots));
  }
  HIP_OK(hipStreamSynchronize(fe->stream));
  if (iterations) {
    unsigned long long h[kSlots];
    HIP_OK(hipMemcpy(h, fe->lk_stats.p, sizeof(h), hipMemcpyDeviceToHost));
    const int L = fe->ld.levels;
    for (int l = 0; l < levels_cap; l++) {
      iterations[l] = visits[l] = 0;
      for (int c = 0; c < 64 && l < L; c++) iterations[l] += h[16 * c + l], visits[l] += h[16 * c + L + l];
    }
    HIP_OK(hipMemset(fe->lk_stats.p, 0, sizeof(h)));
  }
  if (enable >= 0) fe->lk_stats_on = enable != 0;
  return VIO_OK;
}

int vio_frontend_get_pnp_points(vio_frontend_t *fe, int32_t seq, float *forw_pts, int32_t *ids, int32_t cap, int32_t *n) {
  if (!fe || seq < 0 || seq >= fe->n_seq || !n) return VIO_EINVAL;
  if (fe->pending) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(fe);
  HIP_OK(hipDeviceSynchronize());
  int m = 0;
  HIP_OK(hipMemcpy(&m, fe->n_pnp.p + seq, sizeof(int), hipMemcpyDeviceToHost));
  *n = m;
  if (m > cap) return VIO_ECAP;
  const size_t base = (size_t)seq * fe->cap;
  if (m > 0) {
    if (!forw_pts || !ids) return VIO_EINVAL;
    HIP_OK(hipMemcpy(forw_pts, fe->pnp_pts.p + base * 2, sizeof(float) * 2 * m, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ids, fe->pnp_ids.p + base, sizeof(int) * m, hipMemcpyDeviceToHost));
  }
  return VIO_OK;
}

// ---- the tracker's public fields in / out and the update step on its own (isolated tests of F3/F4/F6/F7) ---------------
int vio_frontend_set_tracks(vio_frontend_t *fe, int32_t seq, int32_t n, const float *pre_pts, const float *cur_pts,
                            const float *forw_pts, const int32_t *ids, const int32_t *track_cnt, const uint8_t *lk_status) {
  if (!fe || seq < 0 || seq >= fe->n_seq || n < 0 || (n > 0 && (!pre_pts || !cur_pts || !forw_pts || !ids || !track_cnt || !lk_status)))
    return VIO_EINVAL;
  if (n > fe->cap) return VIO_ECAP;
  if (fe->pending) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(fe);
  HIP_OK(hipDeviceSynchronize());
  const size_t base = (size_t)seq * fe->cap;
  if (n > 0) {
    HIP_OK(hipMemcpy(fe->pre_pts.p + base * 2, pre_pts, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(fe->cur_pts.p + base * 2, cur_pts, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(fe->forw_pts.p + base * 2, forw_pts, sizeof(float) * 2 * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(fe->ids.p + base, ids, sizeof(int) * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(fe->track_cnt.p + base, track_cnt, sizeof(int) * n, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(fe->lk_status.p + base, lk_status, n, hipMemcpyHostToDevice));
  }
  HIP_OK(hipMemcpy(fe->n_pts.p + seq, &n, sizeof(int), hipMemcpyHostToDevice));
  return VIO_OK;
}

int vio_frontend_update_tracks(vio_frontend_t *fe, int32_t publish) {
  if (!fe) return VIO_EINVAL;
  if (fe->pending) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(fe);
  int rc = launch_track_update(fe, publish, fe->stream);
  if (rc != VIO_OK) return rc;
  HIP_OK(hipStreamSynchronize(fe->stream));
  HIP_OK(hipGetLastError());
  return VIO_OK;
}

int vio_frontend_get_tracks(vio_frontend_t *fe, int32_t seq, float *forw_pts, int32_t *ids, int32_t *track_cnt, int32_t cap,
                            int32_t *n) {
  if (!fe || seq < 0 || seq >= fe->n_seq || !n) return VIO_EINVAL;
  if (fe->pending) return VIO_ESTATE;
  VIO_ON_DEVICE_OF(fe);
  HIP_OK(hipDeviceSynchronize());
  int m = 0;
  HIP_OK(hipMemcpy(&m, fe->n_forw.p + seq, sizeof(int), hipMemcpyDeviceToHost));
  *n = m;
  if (m > cap) return VIO_ECAP;
  const size_t base = (size_t)seq * fe->cap;
  if (m > 0) {
    HIP_OK(hipMemcpy(forw_pts, fe->forw_pts.p + base * 2, sizeof(float) * 2 * m, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ids, fe->ids.p + base, sizeof(int) * m, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(track_cnt, fe->track_cnt.p + base, sizeof(int) * m, hipMemcpyDeviceToHost));
  }
  return VIO_OK;
}

// ---- stand-alone operators (one reference call site each), for isolated parity tests --------------------------------
// (each runs on a temporary context, destroyed on every return path)
using FrontendPtr = std::unique_ptr<vio_frontend, void (*)(vio_frontend_t *)>;

int vio_klt_track(const VioConfig *cfg, const uint8_t *prev, const uint8_t *next, int32_t rows, int32_t cols, int32_t stride,
                  const float *prev_pts, int32_t n, float *next_pts, uint8_t *status, float *err) {
  if (!cfg || !prev || !next || n < 0 || (n > 0 && (!prev_pts || !next_pts || !status || !err))) return VIO_EINVAL;
  if (n == 0) return VIO_OK;
  VioConfig c = *cfg;
  c.image_rows = rows, c.image_cols = cols, c.max_corners = std::min(std::max(n, 1), kMaxCap);
  if (n > kMaxCap) return VIO_ECAP;
  vio_frontend *raw = nullptr;
  int rc = vio_frontend_create(&c, 1, &raw);
  if (rc != VIO_OK) return rc;
  const FrontendPtr fe(raw, vio_frontend_destroy);
  const size_t px = (size_t)rows * cols;
  DevBuf<uint8_t> d;  // prev | next
  if (d.ensure(2 * px) != VIO_OK) return VIO_ENOMEM;
  if (hipMemcpy2D(d.p, cols, prev, stride, cols, rows, hipMemcpyHostToDevice) != hipSuccess) return VIO_ENODEV;
  if (hipMemcpy2D(d.p + px, cols, next, stride, cols, rows, hipMemcpyHostToDevice) != hipSuccess) return VIO_ENODEV;
  hipStream_t st = fe->stream;
  for (int k = 0; k < 2; k++) {
    uint8_t *dst = fe->pyr[k].p;
    if (hipMemcpyAsync(dst, d.p + k * px, px, hipMemcpyDeviceToDevice, st) != hipSuccess) return VIO_ENODEV;
    for (int l = 1; l < fe->ld.levels; l++) {
      dim3 blk(256), grd((fe->ld.cols[l] + kPdW - 1) / kPdW, (fe->ld.rows[l] + kPdH - 1) / kPdH, 1);
      hipLaunchKernelGGL(pyr_down_kernel, grd, blk, 0, st, dst + fe->ld.off[l - 1], dst + fe->ld.off[l], fe->ld.pyr_bytes,
                         fe->ld.rows[l - 1], fe->ld.cols[l - 1], fe->ld.rows[l], fe->ld.cols[l]);
    }
  }
  if (hipMemcpyAsync(fe->cur_pts.p, prev_pts, sizeof(float) * 2 * n, hipMemcpyHostToDevice, st) != hipSuccess) return VIO_ENODEV;
  if (hipMemcpyAsync(fe->n_pts.p, &n, sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess) return VIO_ENODEV;
  LkParams P = lk_params(fe->cfg, fe->ld);
  P.prev0 = P.next0 = nullptr, P.stride0 = 0;
  hipLaunchKernelGGL((lk_track_kernel<false>), dim3((fe->cap + 3) / 4, 1), dim3(256), 0, st, fe->pyr[0].p, fe->pyr[1].p, P, fe->n_pts.p,
                     fe->cur_pts.p, fe->forw_pts.p, fe->lk_status.p, fe->lk_err.p, (unsigned long long *)nullptr);
  if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) return VIO_ENODEV;
  if (hipMemcpy(next_pts, fe->forw_pts.p, sizeof(float) * 2 * n, hipMemcpyDeviceToHost) != hipSuccess) return VIO_ENODEV;
  if (hipMemcpy(status, fe->lk_status.p, n, hipMemcpyDeviceToHost) != hipSuccess) return VIO_ENODEV;
  if (hipMemcpy(err, fe->lk_err.p, sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess) return VIO_ENODEV;
  return VIO_OK;
}

int vio_good_features(const VioConfig *cfg, const uint8_t *img, const uint8_t *mask, int32_t rows, int32_t cols, int32_t stride,
                      int32_t max_corners, float *corners, int32_t *n_corners) {
  if (!cfg || !img || !corners || !n_corners || max_corners < 1) return VIO_EINVAL;
  if (max_corners > kMaxCap) return VIO_ECAP;
  VioConfig c = *cfg;
  c.image_rows = rows, c.image_cols = cols, c.max_corners = max_corners;
  vio_frontend *raw = nullptr;
  int rc = vio_frontend_create(&c, 1, &raw);
  if (rc != VIO_OK) return rc;
  const FrontendPtr fe(raw, vio_frontend_destroy);
  const size_t px = (size_t)rows * cols;
  hipStream_t st = fe->stream;
  if (hipMemcpy2D(fe->pyr[0].p, cols, img, stride, cols, rows, hipMemcpyHostToDevice) != hipSuccess) return VIO_ENODEV;
  if (fe->mask.ensure(px) != VIO_OK) return VIO_ENOMEM;
  if (mask) {
    if (hipMemcpy2D(fe->mask.p, cols, mask, stride, cols, rows, hipMemcpyHostToDevice) != hipSuccess) return VIO_ENODEV;
  } else if (hipMemset(fe->mask.p, 255, px) != hipSuccess) {
    return VIO_ENODEV;
  }
  if (hipMemset(fe->max_bits.p, 0, sizeof(unsigned) * fe->nseg) != hipSuccess ||
      hipMemset(fe->n_cand.p, 0, sizeof(int) * fe->nseg) != hipSuccess)
    return VIO_ENODEV;
  dim3 tb(256), tg((cols + kDetWaves * kDetW - 1) / (kDetWaves * kDetW), fe->nseg, 1);
  hipLaunchKernelGGL(detect_kernel<true>, tg, tb, 0, st, fe->pyr[0].p, fe->ld.pyr_bytes, fe->mask.p, px, fe->kept_xy.p, fe->n_kept.p,
                     fe->cap, fe->hw.p, c.min_dist, fe->max_bits.p, rows, cols, fe->cand.p, fe->seg_cap, fe->n_cand.p, fe->ovf.p,
                     next_epoch(fe.get()), (const int *)nullptr, 0);
  const SelectParams SP = select_params(fe.get());
  const RedoParams RP = redo_params(fe.get(), fe->pyr[0].p, fe->ld.pyr_bytes, fe->mask.p, px, c.min_dist);
  hipLaunchKernelGGL(corner_select_kernel<true>, dim3(1 + fe->n_redo_wg), dim3(kSelThreads), 0, st, fe->cand.p, fe->seg_cap, fe->nseg,
                     fe->n_cand.p, fe->max_bits.p, RP, c.quality_level, SP, fe->forw_pts.p, fe->cur_pts.p, fe->pre_pts.p, fe->ids.p, fe->track_cnt.p, fe->n_forw.p, fe->n_pts.p,
                     fe->n_id.p, fe->obs.p, fe->n_obs.p, (long long *)nullptr);
  if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) return VIO_ENODEV;
  int n = 0;
  if (hipMemcpy(&n, fe->n_pts.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return VIO_ENODEV;
  *n_corners = n;
  if (n > 0 && hipMemcpy(corners, fe->forw_pts.p, sizeof(float) * 2 * n, hipMemcpyDeviceToHost) != hipSuccess) return VIO_ENODEV;
  return VIO_OK;
}

int vio_fundamental_ransac(const VioConfig *cfg, const float *pts1, const float *pts2, int32_t n, uint8_t *inlier_mask) {
  if (!cfg || !pts1 || !pts2 || !inlier_mask || n < 0) return VIO_EINVAL;
  if (n == 0) return VIO_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return VIO_ENODEV;
  DevBuf<float> d1, d2;
  DevBuf<uint8_t> dm;
  if (d1.ensure((size_t)2 * n) != VIO_OK || d2.ensure((size_t)2 * n) != VIO_OK || dm.ensure((size_t)n) != VIO_OK) return VIO_ENOMEM;
  if (hipMemcpy(d1.p, pts1, sizeof(float) * 2 * n, hipMemcpyHostToDevice) != hipSuccess) return VIO_ENODEV;
  if (hipMemcpy(d2.p, pts2, sizeof(float) * 2 * n, hipMemcpyHostToDevice) != hipSuccess) return VIO_ENODEV;
  hipLaunchKernelGGL(ransac_only_kernel, dim3(1), dim3(256), sizeof(RansacShared), 0, d1.p, d2.p, n, (float)cfg->f_threshold,
                     cfg->f_confidence, dm.p);
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return VIO_ENODEV;
  if (hipMemcpy(inlier_mask, dm.p, n, hipMemcpyDeviceToHost) != hipSuccess) return VIO_ENODEV;
  return VIO_OK;
}

}  // extern "C"

namespace vio {
int fundamental_ransac_batch(hipStream_t st, const float *p1, const float *p2, const int *count, int n_prob, int stride, int min_count,
                             float thresh, double conf, uint8_t *mask) {
  if (n_prob < 1) return VIO_OK;
  hipLaunchKernelGGL(ransac_batch_kernel, dim3(n_prob), dim3(256), sizeof(RansacShared), st, p1, p2, count, stride, min_count, thresh, conf,
                     mask);
  HIP_OK(hipGetLastError());
  return VIO_OK;
}
}  // namespace vio
