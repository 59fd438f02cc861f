// vio_keyframe_db.hip — KeyFrameDatabase (VINS_ios/loop/keyfame_database.{h,cpp}) for n sessions with the keyframe poses
// resident in device memory: the list passes of kfdb_core.h, one workgroup per session, around the pose graph solve of
// vio_posegraph.hip. optimize = kfdb_build -> posegraph_kernel -> kfdb_apply in one stream without leaving the device:
// per call the host uploads one small job record per session and downloads the drift and the solve statistics.
//
// The host keeps a mirror of the integer bookkeeping of every session (global_index, header, has_loop, is_looped,
// loop_index, segment, list length, earliest_loop_index): every change to those values is decided by arguments the host
// sees, so every argument error is caught here, before anything is launched, and the kernels only meet lengths and
// positions the host validated. Poses, loop_info, total_length and the drift live on the device only.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "vio_amd.h"
#include "vio_device.h"
#include "batch.h"
#include "kfdb_core.h"
#include "solve_trace.h"
#include "vio_posegraph_launch.h"

using namespace vio;
namespace kd = vio::kfdb;

namespace {

// what one session of one call needs on the device: the list it is about and the record of the pass that reads it
struct AddJob {
  int pos, global_index, segment;
  double header, P[3], R[9];
};
struct UpdateJob {
  int loop_pos;  // the keyframe the relocalization belongs to, -1: none
  int wrong;     // |relative_yaw| > 30 or |relative_t| > 10
  int count;     // newest keyframes to compare with header0
  double header0, rel[8] /* relative_t, relative_q (x y z w), relative_yaw */, P0[3], R0[9];
};
struct PoseJob {
  int pos;
};
struct OptimizeJob {
  int first, cur;                  // the graph's range of the list
  int list_short, max_iterations;  // list_size < max_frame_num
  int seg_cur, seg_old;            // segment of the current keyframe and of the one its loop points to
};
struct Job {
  int session, bank, n;
  union {
    AddJob add;
    UpdateJob update;
    PoseJob pose;
    OptimizeJob opt;
  } u;
};

struct DbDev {
  int S, K;  // sessions, keyframes per list
  VioPoseGraphKeyframe *kf;  // [2][S][K]
  double *header;            // [2][S][K]
  int *seg;                  // [2][S][K]
  double *state;             // [S][kStateD]
  int *skip;                 // [S][K]
  double *ypr;               // [S][K][3]
  const Job *jobs;
};

__device__ kd::List list_of(const DbDev &D, int session, int bank) {
  const size_t o = ((size_t)bank * D.S + session) * D.K;
  return kd::List{D.kf + o, D.header + o, D.seg + o};
}
__device__ kd::Cx make_cx() {
  return kd::Cx{(int)threadIdx.x, (int)blockDim.x, __builtin_amdgcn_readfirstlane((int)threadIdx.x & ~63)};
}
__device__ kd::Graph graph_of(const PgPtrs &P, int g) {
  return kd::Graph{const_cast<int *>(P.hdr) + (size_t)g * kPgHdr, const_cast<int *>(P.col) + (size_t)g * P.node_cap,
                   const_cast<double *>(P.node0) + (size_t)g * P.node_cap * 4, const_cast<int *>(P.edge_i) + (size_t)g * P.edge_cap,
                   const_cast<int *>(P.edge_j) + (size_t)g * P.edge_cap, const_cast<int *>(P.edge_kind) + (size_t)g * P.edge_cap,
                   const_cast<double *>(P.meas) + (size_t)g * P.edge_cap * 6};
}

// the constructor's state of sessions [first, first + count)
__global__ void kfdb_clear_kernel(DbDev D, int first, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count * kd::kStateD) return;
  const int k = i % kd::kStateD;
  D.state[(size_t)first * kd::kStateD + i] = (k == kd::S_RD || k == kd::S_RD + 4 || k == kd::S_RD + 8) ? 1.0 : 0.0;
}

// one work-item per job
__global__ void kfdb_add_kernel(DbDev D, int n_jobs) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_jobs) return;
  const Job &J = D.jobs[j];
  kd::kfdb_add(list_of(D, J.session, J.bank), J.u.add.pos, D.state + (size_t)J.session * kd::kStateD, J.u.add.header, J.u.add.P, J.u.add.R,
               J.u.add.global_index, J.u.add.segment);
}

__global__ void kfdb_set_loop_kernel(DbDev D, int session, int bank, int cur_pos, int old_pos, int old_index) {
  if (threadIdx.x != 0) return;
  const kd::List ls = list_of(D, session, bank);
  ls.kf[cur_pos].has_loop = 1, ls.kf[cur_pos].loop_index = old_index;  // detectLoop (keyframe.cpp:356-360)
  ls.kf[old_pos].is_looped = 1;
}

// one wave per job
__global__ __launch_bounds__(kd::kUpdateThreads) void kfdb_update_kernel(DbDev D) {
  const Job &J = D.jobs[blockIdx.x];
  const UpdateJob &U = J.u.update;
  kd::kfdb_update(make_cx(), list_of(D, J.session, J.bank), J.n, U.loop_pos, U.wrong, U.rel, U.count, U.header0, U.P0, U.R0);
}

// out [j][13]: P, R, header of keyframe pos
__global__ void kfdb_get_pose_kernel(DbDev D, int n_jobs, double *out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_jobs) return;
  const Job &J = D.jobs[j];
  const kd::List ls = list_of(D, J.session, J.bank);
  const VioPoseGraphKeyframe &k = ls.kf[J.u.pose.pos];
  for (int a = 0; a < 3; a++) out[13 * j + a] = k.t[a];
  for (int a = 0; a < 9; a++) out[13 * j + 3 + a] = k.r[a];
  out[13 * j + 12] = ls.header[J.u.pose.pos];
}

// one workgroup per job = graph
__global__ __launch_bounds__(kd::kThreads) void kfdb_build_kernel(DbDev D, PgPtrs P, int max_frame_num) {
  extern __shared__ __attribute__((aligned(16))) double kfdb_smem[];
  const Job &J = D.jobs[blockIdx.x];
  const kd::Lds l = kd::carve_lds(D.K, (ldsd)kfdb_smem);
  const kd::List ls = list_of(D, J.session, J.bank);
  const double *state = D.state + (size_t)J.session * kd::kStateD;
  const OptimizeJob &O = J.u.opt;
  kd::kfdb_build(make_cx(), ls.kf + O.first, O.cur - O.first + 1, state[kd::S_LEN], max_frame_num, O.list_short != 0, O.max_iterations, l,
                 graph_of(P, blockIdx.x),
                 D.skip + (size_t)J.session * D.K, D.ypr + (size_t)J.session * D.K * 3);
}

__global__ __launch_bounds__(kd::kThreads) void kfdb_apply_kernel(DbDev D, PgPtrs P, double *drift) {
  extern __shared__ __attribute__((aligned(16))) double kfdb_smem[];
  const Job &J = D.jobs[blockIdx.x];
  const kd::Lds l = kd::carve_lds(D.K, (ldsd)kfdb_smem);
  const OptimizeJob &O = J.u.opt;
  kd::kfdb_apply(make_cx(), list_of(D, J.session, J.bank), J.n, O.first, O.cur, O.seg_cur, O.seg_old, l, graph_of(P, blockIdx.x),
                 P.xout + (size_t)blockIdx.x * P.ld, D.skip + (size_t)J.session * D.K, D.ypr + (size_t)J.session * D.K * 3,
                 D.state + (size_t)J.session * kd::kStateD, drift + (size_t)blockIdx.x * kd::kDriftD);
}

// one session per call: erased [K] | counts [2]
__global__ __launch_bounds__(kd::kThreads) void kfdb_resample_kernel(DbDev D, int max_frame_num, int *erased) {
  extern __shared__ __attribute__((aligned(16))) double kfdb_smem[];
  const Job &J = D.jobs[0];
  const kd::Lds l = kd::carve_lds(D.K, (ldsd)kfdb_smem);
  kd::kfdb_resample(make_cx(), list_of(D, J.session, J.bank), list_of(D, J.session, 1 - J.bank), J.n, max_frame_num, l,
                    D.state + (size_t)J.session * kd::kStateD, erased, erased + D.K);
}

// the host's mirror of one session
struct Session {
  int n = 0, bank = 0, next_index = 0, earliest = -1, cur_seg = 0, max_seg = 0;
  std::vector<int> gidx, has_loop, is_looped, loop_index, seg;
  std::vector<double> header;
  // position of a global_index in the list (ascending by construction), -1: unknown or erased
  int find(int index) const {
    const auto it = std::lower_bound(gidx.begin(), gidx.begin() + n, index);
    return (it != gidx.begin() + n && *it == index) ? (int)(it - gidx.begin()) : -1;
  }
};

}  // namespace

struct vio_keyframe_db {
  int device = 0;
  int S = 0, K = 0, G = 0, max_frame_num = 0, ld = 0, edge_cap = 0;
  size_t pg_lds = 0, list_lds = 0, out_bytes = 0;
  hipStream_t stream = nullptr;
  std::vector<Session> sess;
  vio::DevBuf<VioPoseGraphKeyframe> kf;
  vio::DevBuf<double> header, state, ypr, node0, meas, xout, H, A, pose_d;
  vio::DevBuf<int> seg, skip, hdr, col, ei, ej, ek, erased_d;
  vio::DevBuf<char> out_d;    // stats_d [G][kStatsDoubles] | drift [G][kDriftD] | stats_i [G][kStatsInts]: one download
  vio::PinnedBuf<char> out_h;
  vio::DevBuf<Job> jobs_d;
  vio::PinnedBuf<Job> jobs_h;
  vio::PinnedBuf<double> pose_h;
  vio::PinnedBuf<int> erased_h;
  ~vio_keyframe_db() {
    if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
  }
  DbDev dev() const { return DbDev{S, K, kf.p, header.p, seg.p, state.p, skip.p, ypr.p, jobs_d.p}; }
  double *stats_d() const { return (double *)out_d.p; }
  double *drift_d() const { return stats_d() + (size_t)G * kStatsDoubles; }
  int *stats_i() const { return (int *)(drift_d() + (size_t)G * kd::kDriftD); }
  PgPtrs pg() const {
    PgPtrs P;
    P.ld = ld, P.node_cap = K, P.edge_cap = edge_cap;
    P.hdr = hdr.p, P.col = col.p, P.node0 = node0.p, P.edge_i = ei.p, P.edge_j = ej.p, P.edge_kind = ek.p, P.meas = meas.p;
    P.H = H.p, P.A = A.p, P.xout = xout.p, P.stats_d = stats_d(), P.stats_i = stats_i();
    return P;
  }
  hipError_t upload_jobs(int n) { return hipMemcpyAsync(jobs_d.p, jobs_h.p, (size_t)n * sizeof(Job), hipMemcpyHostToDevice, stream); }
};

namespace {

// every session index valid and named at most once
int check_sessions(const vio_keyframe_db *db, int32_t n, const int32_t *session) {
  if (n < 1 || !session || n > db->S) return VIO_EINVAL;
  std::vector<char> seen(db->S, 0);
  for (int i = 0; i < n; i++) {
    if (session[i] < 0 || session[i] >= db->S || seen[session[i]]) return VIO_EINVAL;
    seen[session[i]] = 1;
  }
  return VIO_OK;
}

}  // namespace

extern "C" {

int vio_keyframe_db_create(int32_t n_sessions, int32_t max_keyframes, int32_t max_graphs, int32_t max_frame_num, vio_keyframe_db_t **out) {
  if (!out || n_sessions < 1 || max_keyframes < 2 || max_graphs < 1 || max_frame_num < 1) return VIO_EINVAL;
  if (!vio::device_ready("the keyframe database")) return VIO_ENODEV;
  vio_keyframe_db *db = new (std::nothrow) vio_keyframe_db();
  if (!db) return VIO_ENOMEM;
  db->device = vio::current_device();
  db->S = n_sessions, db->K = max_keyframes, db->G = std::min(max_graphs, n_sessions), db->max_frame_num = max_frame_num;
  db->ld = vio::pg_ld(max_keyframes), db->edge_cap = 6 * max_keyframes;  // five sequential edges and a loop per keyframe at most
  db->pg_lds = vio::pg_lds_bytes(db->ld), db->list_lds = kd::lds_bytes(max_keyframes);
  if (db->pg_lds > vio::kLdsBytes || db->list_lds > 64 * 1024) {  // (the solver's seven N-vectors: ~730 keyframes)
    delete db;
    return VIO_ECAP;
  }
  const size_t S = db->S, K = db->K, G = db->G, mat = (size_t)db->ld * db->ld, SK = S * K;
  db->out_bytes = G * ((size_t)(kStatsDoubles + kd::kDriftD) * sizeof(double) + kStatsInts * sizeof(int));
  // the dense scratch dominates: refuse before allocating what the device does not have
  size_t free_b = 0, total_b = 0;
  const size_t need = 2 * G * mat * sizeof(double) + 2 * SK * (sizeof(VioPoseGraphKeyframe) + 12) + SK * 28;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b) {
    delete db;
    return VIO_ENOMEM;
  }
  if (hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) != hipSuccess) {
    delete db;
    return VIO_ENODEV;
  }
  if (db->kf.ensure(2 * SK) != VIO_OK || db->header.ensure(2 * SK) != VIO_OK || db->seg.ensure(2 * SK) != VIO_OK ||
      db->state.ensure(S * kd::kStateD) != VIO_OK || db->skip.ensure(SK) != VIO_OK || db->ypr.ensure(3 * SK) != VIO_OK ||
      db->hdr.ensure(G * kPgHdr) != VIO_OK || db->col.ensure(G * K) != VIO_OK || db->ei.ensure(G * db->edge_cap) != VIO_OK ||
      db->ej.ensure(G * db->edge_cap) != VIO_OK || db->ek.ensure(G * db->edge_cap) != VIO_OK || db->node0.ensure(G * K * 4) != VIO_OK ||
      db->meas.ensure(G * db->edge_cap * 6) != VIO_OK || db->xout.ensure(G * db->ld) != VIO_OK || db->H.ensure(G * mat) != VIO_OK ||
      db->A.ensure(G * mat) != VIO_OK || db->out_d.ensure(db->out_bytes) != VIO_OK || db->out_h.ensure(db->out_bytes) != VIO_OK ||
      db->jobs_d.ensure(S) != VIO_OK || db->jobs_h.ensure(S) != VIO_OK || db->pose_d.ensure(S * 13) != VIO_OK ||
      db->pose_h.ensure(S * 13) != VIO_OK || db->erased_d.ensure(K + 2) != VIO_OK || db->erased_h.ensure(K + 2) != VIO_OK) {
    delete db;
    return VIO_ENOMEM;
  }
  db->sess.resize(S);
  for (Session &s : db->sess) {
    s.gidx.assign(K, 0), s.has_loop.assign(K, 0), s.is_looped.assign(K, 0), s.loop_index.assign(K, -1), s.seg.assign(K, 0);
    s.header.assign(K, 0.0);
  }
  // the factorization reads whole 16 x 16 tiles: no uninitialised memory may reach the matrix cores (vio_posegraph.hip)
  bool ok = hipMemsetAsync(db->H.p, 0, G * mat * sizeof(double), db->stream) == hipSuccess &&
            hipMemsetAsync(db->A.p, 0, G * mat * sizeof(double), db->stream) == hipSuccess &&
            hipMemsetAsync(db->kf.p, 0, 2 * SK * sizeof(VioPoseGraphKeyframe), db->stream) == hipSuccess && vio::pg_prepare() == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(kfdb_clear_kernel, dim3((db->S * kd::kStateD + 255) / 256), dim3(256), 0, db->stream, db->dev(), 0, db->S);
    ok = hipGetLastError() == hipSuccess;
  }
  if (!ok || hipStreamSynchronize(db->stream) != hipSuccess) {
    delete db;
    return VIO_ENODEV;
  }
  *out = db;
  return VIO_OK;
}

int vio_keyframe_db_get_device(const vio_keyframe_db_t *db, int32_t *device) {
  if (!db || !device) return VIO_EINVAL;
  *device = db->device;
  return VIO_OK;
}

void vio_keyframe_db_destroy(vio_keyframe_db_t *db) {
  if (!db) return;
  vio::DeviceScope scope(db->device);
  delete db;
}

int vio_keyframe_db_clear(vio_keyframe_db_t *db, int32_t session) {
  if (!db || session < 0 || session >= db->S) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(db);
  hipLaunchKernelGGL(kfdb_clear_kernel, dim3(1), dim3(64), 0, db->stream, db->dev(), session, 1);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(db->stream));
  Session &s = db->sess[session];
  s.n = 0, s.next_index = 0, s.earliest = -1, s.cur_seg = s.max_seg = 0;
  return VIO_OK;
}

int vio_keyframe_db_size(const vio_keyframe_db_t *db, int32_t session, int32_t *n) {
  if (!db || session < 0 || session >= db->S || !n) return VIO_EINVAL;
  *n = db->sess[session].n;
  return VIO_OK;
}

int vio_keyframe_db_new_segment(vio_keyframe_db_t *db, int32_t session) {
  if (!db || session < 0 || session >= db->S) return VIO_EINVAL;
  Session &s = db->sess[session];
  s.max_seg++, s.cur_seg = s.max_seg;
  return VIO_OK;
}

int vio_keyframe_db_add(vio_keyframe_db_t *db, int32_t n, const int32_t *session, const double *header, const double *P, const double *R,
                        int32_t *global_index_out) {
  if (!db || !header || !P || !R) return VIO_EINVAL;
  const int rc = check_sessions(db, n, session);
  if (rc != VIO_OK) return rc;
  for (int i = 0; i < n; i++)
    if (db->sess[session[i]].n >= db->K) return VIO_ECAP;
  VIO_ON_DEVICE_OF(db);
  for (int i = 0; i < n; i++) {
    const Session &s = db->sess[session[i]];
    Job &J = db->jobs_h.p[i];
    J.session = session[i], J.bank = s.bank, J.n = s.n;
    AddJob &A = J.u.add;
    A.pos = s.n, A.global_index = s.next_index, A.segment = s.cur_seg, A.header = header[i];
    memcpy(A.P, P + 3 * i, 24), memcpy(A.R, R + 9 * i, 72);
  }
  HIP_OK(db->upload_jobs(n));
  hipLaunchKernelGGL(kfdb_add_kernel, dim3((n + 63) / 64), dim3(64), 0, db->stream, db->dev(), n);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(db->stream));
  for (int i = 0; i < n; i++) {
    Session &s = db->sess[session[i]];
    const int p = s.n++;
    s.gidx[p] = s.next_index, s.header[p] = header[i], s.has_loop[p] = 0, s.is_looped[p] = 0, s.loop_index[p] = -1, s.seg[p] = s.cur_seg;
    if (global_index_out) global_index_out[i] = s.next_index;
    s.next_index++;
  }
  return VIO_OK;
}

int vio_keyframe_db_set_loop(vio_keyframe_db_t *db, int32_t session, int32_t cur_index, int32_t old_index) {
  if (!db || session < 0 || session >= db->S || old_index >= cur_index) return VIO_EINVAL;
  Session &s = db->sess[session];
  const int pc = s.find(cur_index), po = s.find(old_index);
  if (pc < 0 || po < 0) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(db);
  hipLaunchKernelGGL(kfdb_set_loop_kernel, dim3(1), dim3(64), 0, db->stream, db->dev(), session, s.bank, pc, po, old_index);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(db->stream));
  s.has_loop[pc] = 1, s.loop_index[pc] = old_index, s.is_looped[po] = 1;
  return VIO_OK;
}

int vio_keyframe_db_get_pose(vio_keyframe_db_t *db, int32_t n, const int32_t *session, const int32_t *index, double *P, double *R,
                             double *header) {
  if (!db || !index) return VIO_EINVAL;
  const int rc = check_sessions(db, n, session);
  if (rc != VIO_OK) return rc;
  for (int i = 0; i < n; i++)
    if (db->sess[session[i]].find(index[i]) < 0) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(db);
  for (int i = 0; i < n; i++) {
    const Session &s = db->sess[session[i]];
    Job &J = db->jobs_h.p[i];
    J.session = session[i], J.bank = s.bank, J.n = s.n, J.u.pose.pos = s.find(index[i]);
  }
  HIP_OK(db->upload_jobs(n));
  hipLaunchKernelGGL(kfdb_get_pose_kernel, dim3((n + 63) / 64), dim3(64), 0, db->stream, db->dev(), n, db->pose_d.p);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(db->pose_h.p, db->pose_d.p, (size_t)n * 13 * sizeof(double), hipMemcpyDeviceToHost, db->stream));
  HIP_OK(hipStreamSynchronize(db->stream));
  for (int i = 0; i < n; i++) {
    const double *o = db->pose_h.p + 13 * i;
    if (P) memcpy(P + 3 * i, o, 24);
    if (R) memcpy(R + 9 * i, o + 3, 72);
    if (header) header[i] = o[12];
  }
  return VIO_OK;
}

int vio_keyframe_db_update(vio_keyframe_db_t *db, int32_t n, const int32_t *session, const int32_t *loop_kf, const double *relative_t,
                           const double *relative_q, const double *relative_yaw, int32_t window_size, const double *header0,
                           const double *P0, const double *R0, int32_t *optimize_index_out) {
  if (!db || !loop_kf || !header0 || !P0 || !R0 || window_size < 1) return VIO_EINVAL;
  const int rc = check_sessions(db, n, session);
  if (rc != VIO_OK) return rc;
  for (int i = 0; i < n; i++) {
    if (loop_kf[i] < 0) continue;
    if (!relative_t || !relative_q || !relative_yaw || db->sess[session[i]].find(loop_kf[i]) < 0) return VIO_EINVAL;
  }
  VIO_ON_DEVICE_OF(db);
  std::vector<int> wrong(n, 0), found(n, -1);
  int n_jobs = 0;  // a session with an empty list has nothing to search and no keyframe to mark: no workgroup for it
  for (int i = 0; i < n; i++) {
    const Session &s = db->sess[session[i]];
    if (s.n == 0) continue;
    Job &J = db->jobs_h.p[n_jobs++];
    J.session = session[i], J.bank = s.bank, J.n = s.n;
    UpdateJob &U = J.u.update;
    U.loop_pos = -1, U.wrong = 0, U.header0 = header0[i];
    if (loop_kf[i] >= 0) {
      const double *t = relative_t + 3 * i;
      wrong[i] = fabs(relative_yaw[i]) > 30.0 || sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) > 10.0;  // ViewController.mm:836
      U.loop_pos = s.find(loop_kf[i]), U.wrong = wrong[i];
      memcpy(U.rel, t, 24), memcpy(U.rel + 3, relative_q + 4 * i, 32), U.rel[7] = relative_yaw[i];
    }
    // search_cnt > 2 * WINDOW_SIZE breaks after the miss (:870): 2 W + 1 keyframes are examined
    U.count = std::min(s.n, 2 * window_size + 1);
    memcpy(U.P0, P0 + 3 * i, 24), memcpy(U.R0, R0 + 9 * i, 72);
    for (int k = 0; k < U.count && found[i] < 0; k++)
      if (s.header[s.n - 1 - k] == header0[i]) found[i] = s.n - 1 - k;
  }
  if (n_jobs > 0) {
    HIP_OK(db->upload_jobs(n_jobs));
    hipLaunchKernelGGL(kfdb_update_kernel, dim3(n_jobs), dim3(kd::kUpdateThreads), 0, db->stream, db->dev());
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(db->stream));
  }
  for (int i = 0; i < n; i++) {
    Session &s = db->sess[session[i]];
    if (loop_kf[i] >= 0 && wrong[i]) s.has_loop[s.find(loop_kf[i])] = 0;  // removeLoop (keyframe.cpp:362-366)
    if (optimize_index_out) optimize_index_out[i] = (found[i] >= 0 && s.has_loop[found[i]]) ? s.gidx[found[i]] : -1;
  }
  return VIO_OK;
}

int vio_keyframe_db_optimize(vio_keyframe_db_t *db, int32_t n, const int32_t *session, const int32_t *cur_index, int32_t max_iterations,
                             double *yaw_drift, double *r_drift, double *t_drift, VioSolveStats *stats) {
  if (!db || !cur_index || max_iterations < 0) return VIO_EINVAL;
  const int rc = check_sessions(db, n, session);
  if (rc != VIO_OK) return rc;
  if (n > db->G) return VIO_ECAP;
  std::vector<int> earliest(n), old_pos(n);
  for (int i = 0; i < n; i++) {
    const Session &s = db->sess[session[i]];
    const int cur = s.find(cur_index[i]);
    if (cur < 0 || !s.has_loop[cur]) return VIO_EINVAL;  // (the reference asserts, :148)
    const int li = s.loop_index[cur];
    earliest[i] = (s.earliest > li || s.earliest == -1) ? li : s.earliest;  // (:146-147)
    const int first = (int)(std::lower_bound(s.gidx.begin(), s.gidx.begin() + s.n, earliest[i]) - s.gidx.begin());
    old_pos[i] = s.find(li);
    if (old_pos[i] < 0) return VIO_EINVAL;
    if (cur - first + 1 > db->K) return VIO_ECAP;
    for (int k = first; k <= cur; k++) {
      if (!s.has_loop[k]) continue;
      const int c = s.find(s.loop_index[k]);
      if (s.loop_index[k] < earliest[i] || c < first || c > cur) return VIO_EINVAL;  // (the reference asserts, :276-280)
    }
    Job &J = db->jobs_h.p[i];
    J.session = session[i], J.bank = s.bank, J.n = s.n, J.u.opt.first = first, J.u.opt.cur = cur;
  }
  VIO_ON_DEVICE_OF(db);
  hipStream_t st = db->stream;
  const DbDev D = db->dev();
  const PgPtrs P = db->pg();
  for (int i = 0; i < n; i++) {
    const Session &s = db->sess[session[i]];
    OptimizeJob &O = db->jobs_h.p[i].u.opt;
    O.list_short = s.n < db->max_frame_num ? 1 : 0, O.max_iterations = std::min<int>(max_iterations, kMaxTrace - 1);
    O.seg_cur = s.seg[O.cur], O.seg_old = s.seg[old_pos[i]];
  }
  HIP_OK(db->upload_jobs(n));
  hipLaunchKernelGGL(kfdb_build_kernel, dim3(n), dim3(kd::kThreads), db->list_lds, st, D, P, db->max_frame_num);
  HIP_OK(hipGetLastError());
  HIP_OK(vio::launch_posegraph(P, n, db->pg_lds, st));
  hipLaunchKernelGGL(kfdb_apply_kernel, dim3(n), dim3(kd::kThreads), db->list_lds, st, D, P, db->drift_d());
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(db->out_h.p, db->out_d.p, db->out_bytes, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  const double *sd = (const double *)db->out_h.p, *dr = sd + (size_t)db->G * kStatsDoubles;
  const int *si = (const int *)(dr + (size_t)db->G * kd::kDriftD);
  for (int i = 0; i < n; i++) {
    Session &s = db->sess[session[i]];
    const OptimizeJob &O = db->jobs_h.p[i].u.opt;
    s.earliest = earliest[i];
    for (int k = O.first; k < O.cur; k++)
      if (s.seg[k] == O.seg_cur) s.seg[k] = O.seg_old;
    s.cur_seg = O.seg_old;  // (:303-305)
    if (yaw_drift) yaw_drift[i] = dr[kd::kDriftD * i];
    if (r_drift) memcpy(r_drift + 9 * i, dr + kd::kDriftD * i + 1, 72);
    if (t_drift) memcpy(t_drift + 3 * i, dr + kd::kDriftD * i + 10, 24);
    if (stats) unpack_solve_stats(sd + (size_t)i * kStatsDoubles, si + (size_t)i * kStatsInts, &stats[i]);
  }
  return VIO_OK;
}

int vio_keyframe_db_resample(vio_keyframe_db_t *db, int32_t session, int32_t *erase_index_out, int32_t cap, int32_t *n_erased) {
  if (!db || session < 0 || session >= db->S || !n_erased || cap < 0 || (cap > 0 && !erase_index_out)) return VIO_EINVAL;
  Session &s = db->sess[session];
  *n_erased = 0;
  if (s.n < db->max_frame_num) return VIO_OK;  // (:47-48)
  if (cap < s.n - 1) return VIO_ECAP;           // (how many go is the device's decision: room for all but the first)
  VIO_ON_DEVICE_OF(db);
  Job &J = db->jobs_h.p[0];
  J.session = session, J.bank = s.bank, J.n = s.n;
  HIP_OK(db->upload_jobs(1));
  hipLaunchKernelGGL(kfdb_resample_kernel, dim3(1), dim3(kd::kThreads), db->list_lds, db->stream, db->dev(), db->max_frame_num, db->erased_d.p);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(db->erased_h.p, db->erased_d.p, (size_t)(db->K + 2) * sizeof(int), hipMemcpyDeviceToHost, db->stream));
  HIP_OK(hipStreamSynchronize(db->stream));
  const int n_kept = db->erased_h.p[db->K], n_gone = db->erased_h.p[db->K + 1];
  if (n_kept < 1 || n_kept + n_gone != s.n) return VIO_ENODEV;
  // which positions stay: decided in full before the mirror or the caller's array is touched
  std::vector<int> keep;
  keep.reserve(n_kept);
  int e = 0;
  for (int k = 0; k < s.n; k++) {
    if (e < n_gone && db->erased_h.p[e] == s.gidx[k]) e++;
    else keep.push_back(k);
  }
  if ((int)keep.size() != n_kept || e != n_gone) return VIO_ENODEV;
  for (int i = 0; i < n_gone; i++) erase_index_out[i] = db->erased_h.p[i];
  for (int w = 0; w < n_kept; w++) {  // (keep[w] >= w: in place, front to back)
    const int k = keep[w];
    s.gidx[w] = s.gidx[k], s.header[w] = s.header[k], s.has_loop[w] = s.has_loop[k], s.is_looped[w] = s.is_looped[k];
    s.loop_index[w] = s.loop_index[k], s.seg[w] = s.seg[k];
  }
  s.n = n_kept, s.bank ^= 1;
  *n_erased = n_gone;
  return VIO_OK;
}

int vio_keyframe_db_download(vio_keyframe_db_t *db, int32_t session, VioPoseGraphKeyframe *kf, double *header, int32_t *segment_index,
                             int32_t cap, int32_t *n, double *state, int32_t *index_state) {
  if (!db || session < 0 || session >= db->S || !n || cap < 0) return VIO_EINVAL;
  const Session &s = db->sess[session];
  *n = s.n;
  if ((kf || header || segment_index) && cap < s.n) return VIO_ECAP;
  VIO_ON_DEVICE_OF(db);
  const size_t o = ((size_t)s.bank * db->S + session) * db->K;
  HIP_OK(hipStreamSynchronize(db->stream));
  if (kf && s.n) HIP_OK(hipMemcpy(kf, db->kf.p + o, (size_t)s.n * sizeof(*kf), hipMemcpyDeviceToHost));
  if (header && s.n) HIP_OK(hipMemcpy(header, db->header.p + o, (size_t)s.n * sizeof(double), hipMemcpyDeviceToHost));
  if (segment_index && s.n) HIP_OK(hipMemcpy(segment_index, db->seg.p + o, (size_t)s.n * sizeof(int), hipMemcpyDeviceToHost));
  if (state) HIP_OK(hipMemcpy(state, db->state.p + (size_t)session * kd::kStateD, kd::kStateD * sizeof(double), hipMemcpyDeviceToHost));
  if (index_state) index_state[0] = s.earliest, index_state[1] = s.cur_seg, index_state[2] = s.max_seg;
  return VIO_OK;
}

}  // extern "C"
