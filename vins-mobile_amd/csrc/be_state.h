// be_state.h — part of vio_backend.hip: the back-end's context (include/vio_amd.h, vio_backend_t) and the state of its
// device-resident path (vio_resident.h), null until reserved. Both paths bind the context's one set of work buffers and launch by
// the context's one plan (wk_plan.h).
#pragma once
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <vector>

#include "vio_pool.h"
#include "vio_device.h"
#include "vio_window_variants.h"
#include "vio_resident.h"
#include "vio_store.h"

using namespace vio;

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static bool poison() {
  static const bool on = vio::env_flag("VIO_AMD_POISON");
  return on;
}

constexpr int kResidentLoopIds = 256;  // matched ids of a relocalization frame a slot takes (vio_resident.h)

struct vio_resident {
  int n_slots = 0, W = 0, P = 0;
  vio::store::Dims sd;
  // the store: two banks per slot, control blocks, pre-integration blocks, the extrinsic
  DevBuf<int> fid, start, nobs, flag, ctl;
  DevBuf<double> depth, obs, ctld, preint, consts;  // consts: [n_slots] x (ex_pose 7 | tic 3 | ric 9), then the IMU noise 18
  double ex_pose[7];
  // the camera of every slot (vio_backend_resident_set_cameras; the one of reserve until then): kCamRec doubles per slot,
  // ex_pose 7 | tic 3 | ric 9 as in consts, then sqrt_info = FOCUS_LENGTH_X / 1.5 (VINS.cpp:31)
  static constexpr int kCamRec = 20, kCamDev = 19;
  std::vector<double> cam_rec;
  // per-frame inputs: page-locked arena and its device mirror (same offsets)
  HostVec<unsigned char> h_in;
  DevBuf<unsigned char> d_in;
  size_t o_active = 0, o_nobs = 0, o_hdr = 0, o_prk = 0, o_pri = 0, o_pro = 0, o_preidx = 0, o_hdrd = 0, o_pose = 0, o_sb = 0, o_ex = 0,
         o_Ps = 0, o_Rs = 0, o_obs = 0, o_preblk = 0, total_bytes = 0;
  std::atomic<int> n_pre{0};
  // IMU samples integrated on the device: job records (16 doubles) and samples (7 doubles), both behind the fixed part
  size_t o_jobs = 0, o_samples = 0;
  int cap_jobs = 0, cap_samples = 0;
  std::atomic<int> n_jobs{0}, n_samples{0}, n_obs_total{0};
  size_t o_obsoff = 0;  // per slot: where its observations start in the packed observation region
  // relocalization frames: per slot frame / count / offset (fixed part), packed ids and observations (variable)
  size_t o_loopf = 0, o_loopn = 0, o_loopoff = 0, o_loopids = 0, o_loopxy = 0;
  int cap_loop = 0;
  std::atomic<int> n_loop_total{0};
  bool any_loop = false;
  HostVec<double> h_raw_pose, h_out_loop;
  DevBuf<double> pre_side;  // [n_slots][W][preint::kSide]
  // landmark side of the batch (written by store_pack), sized by the sticky dims
  BatchDims d;
  BatchStrides s;
  bool bound = false;
  DevBuf<int> b_fhost, b_ftarget, b_ffeat, b_fslot, b_fstart, b_pair_h, b_pair_t, b_pair_s0, b_pair_s1;
  DevBuf<double> b_feat, b_pts_i, b_pts_j, b_dummy;
  DevBuf<long long> prof;
  // results
  HostVec<int> h_ctl, h_stats_i, h_m_ints;
  HostVec<double> h_out_pose, h_out_sb, h_stats_d;
  std::vector<int> active_list;  // slots whose window was solved in this frame
  std::vector<char> solved;
  int phase = 0;  // 0 idle / collected, 1 begun, 2 ingested, 3 launched
  // vio_backend_resident_keyframe: the jobs and their window states up, the sections of one download back
  DevBuf<int> kf_jobs;
  DevBuf<double> kf_states;
  DevBuf<unsigned char> kf_out;
  std::vector<int> kf_hjobs;
  std::vector<double> kf_hstates;
  HostVec<unsigned char> kf_hout;  // (page-locked: the download is a few MB at 512 slots)
  template <class T>
  T *hp(size_t off) { return reinterpret_cast<T *>(h_in.data() + off); }
  template <class T>
  T *dp(size_t off) { return reinterpret_cast<T *>(d_in.p + off); }
};

struct vio_backend {
  VioConfig cfg;
  std::unique_ptr<vio_resident> res;  // device-resident path (vio_resident.h), null until reserved
  int peers = 2;  // contexts whose window kernels share the device at the same time (vio_backend_set_peers)
  int device = -1;  // HIP device the context lives on (current device at create)
  int max_batch = 0;
  hipStream_t stream = nullptr;
  LaunchTimer timer;
  // current batch
  int n = 0;
  bool uploaded = false;
  hipStream_t last_stream = nullptr;  // where the last launch went: what sync / download wait for
  hipEvent_t upload_done = nullptr;   // recorded behind the upload's copies on `stream`: launches on another stream wait for it
  vio_wk::Layout plan;  // of the bound batch: which windows go to which of the two launches, and how (wk_plan.h)
  DevBuf<int> d_order;
  HostVec<int> h_order;
  bool profile = false;
  int n_cus = 256;  // compute units of the device (hipDeviceProp_t::multiProcessorCount)
  int coop_width = 1;    // workgroups per global-matrix window of the last launch (vio_backend_coop_width)
  bool coop_ok = false;  // the global-matrix windows of the uploaded batch may run as cooperative windows (host-packed, no bucket across chunks)
  DevBuf<long long> d_prof;
  HostBatch hb;
  BatchPtrs B;
  MargPtrs MP;
  DevBuf<unsigned char> d_in;  // every input array, laid out like the host staging arena (HostBatch::off)
  DevBuf<int> d_stats_i, d_m_ints;
  DevBuf<double> d_scratch,
      d_hm, d_out_pose, d_out_sb, d_out_feat, d_raw_pose, d_raw_sb, d_raw_feat, d_out_loop, d_stats_d, d_m_x0, d_m_J,
      d_m_r, d_m_scratch;
  // device-resident prior chain (vio_backend_reserve_priors): st_n slots x 2 banks; st_bank[k] = the bank slot k's
  // current prior lives in; the kernel writes the next one into the other bank
  int st_n = 0, st_ncap = 0;
  DevBuf<double> d_st_x0[2], d_st_J[2], d_st_r[2];
  std::vector<unsigned char> st_bank;
  std::vector<int> slot_of;  // [n] slot of window b in this upload or -1
  DevBuf<PriorTab> d_ptab;
  HostVec<PriorTab> h_ptab;
  bool host_prior_in = true, host_prior_out = true, slots_advanced = false;  // any window of this upload moves prior data through the host
  // host copies of the outputs
  HostVec<double> h_out_pose, h_out_sb, h_out_feat, h_raw_pose, h_raw_sb, h_raw_feat, h_out_loop, h_stats_d, h_m_x0,
      h_m_J, h_m_r;
  HostVec<int> h_stats_i, h_m_ints;
  ~vio_backend() {
    if (!stream) return;
    (void)hipStreamSynchronize(stream);
    if (upload_done) (void)hipEventDestroy(upload_done);
    (void)hipStreamDestroy(stream);
  }
};

// the whole of a device buffer into its host copy, queued on st
template <class Host, class Dev>
static hipError_t d2h(Host &dst, const Dev &src, hipStream_t st) {
  if (dst.size() != src.n) dst.resize(src.n);
  return hipMemcpyAsync(dst.data(), src.p, src.n * sizeof(dst[0]), hipMemcpyDeviceToHost, st);
}
