// kfdb_core.h — the keyframe list of a session on the device: KeyFrameDatabase (VINS_ios/loop/keyfame_database.{h,cpp}) as
// flat arrays in HBM, one workgroup per session, and the pose graph of optimize4DoFLoopPoseGraph (:140-356) written
// straight into the solver's input arrays (vio_posegraph_launch.h) instead of being walked on the host and uploaded.
//
// A list is an array of VioPoseGraphKeyframe (the struct vio_posegraph_build takes: origin pose, current pose, indices,
// flags, loop_info) plus the headers and segment indices beside it. The passes, all of them list work (a few hundred
// keyframes, integer traffic, ballots): nothing here is shaped for the matrix cores.
//   kfdb_add       KeyFrame::KeyFrame (keyframe.cpp:4-14) + KeyFrameDatabase::add (:21-42), one work-item
//   kfdb_update    removeLoop / updateLoopConnection, the header search and updateOriginPose (ViewController.mm:831-873)
//   kfdb_build     need_resample, parameter values, sequential and loop edges (:166-291) -> hdr / col / node0 / edges / meas
//   kfdb_apply     poses after the solve, drift, tail, segment relabelling, updateVisualization (:301-378)
//   kfdb_resample  resample (:44-76), compacted into the other bank
//
// kfdb_build and kfdb_apply perform the floating-point operations of vio_posegraph_build / vio_posegraph_apply
// (vio_posegraph_host.cpp) in the same order (this file is compiled with -ffp-contract=off like that one), so with the
// same libm a list gives the same bits on either path: tests/emul/simt_kfdb.cpp runs these functions on the host through
// the SIMT emulator against the two host functions.
#pragma once

#include "spmd.h"
#include "vio_amd.h"
#include "vio_math.h"

namespace vio {
namespace kfdb {

constexpr int kThreads = 256;
constexpr int kUpdateThreads = 64;  // the header search: one wave
// state of a session (doubles): total_length, last_P, yaw_drift, r_drift, t_drift (keyfame_database.cpp:12-18)
enum { S_LEN = 0, S_LASTP = 1, S_YAW = 4, S_RD = 5, S_TD = 14, kStateD = 17 };
constexpr int kDriftD = 13;  // what an optimize hands back per session: yaw_drift, r_drift, t_drift

struct Cx {
  int tid, nt;
  int wave64 = 0;  // (VIO_TID of spmd.h)
};

struct List {
  VioPoseGraphKeyframe *kf;  // [cap]
  double *header;            // [cap]
  int *seg;                  // [cap] segment_index
};

// LDS of the list passes, cap = the list capacity
struct Lds {
  ldsd dist;   // [cap] step norms
  ldsd misc;   // [16]
  ldsi flag;   // [cap]
  ldsi rank;   // [cap]
  ldsi rank2;  // [cap]
  ldsi kept;   // [cap] rank -> node
  ldsi used;   // [cap]
  ldsi part;   // [nt / 64 + 1]
};
VIO_HD size_t lds_bytes(int cap) { return sizeof(double) * ((size_t)cap + 16) + sizeof(int) * (5 * (size_t)cap + kThreads / 64 + 1); }
template <class PD>
VIO_DEV Lds carve_lds(int cap, PD dbase) {
  Lds l;
  l.dist = dbase, l.misc = dbase + cap;
  ldsi p = (ldsi)(dbase + cap + 16);
  l.flag = p, l.rank = p + cap, l.rank2 = p + 2 * cap, l.kept = p + 3 * cap, l.used = p + 4 * cap, l.part = p + 5 * cap;
  return l;
}

// ---- the rotation helpers of vio_posegraph_host.cpp, operation for operation ------------------------------------------
constexpr double kPi = 3.14159265358979323846;

// Utility::R2ypr (VINS_ios/utility.hpp:76-91): degrees
VIO_DEV void rot_to_ypr(const double *R, double *ypr) {
  const double y = atan2(R[3], R[0]);
  const double p = atan2(-R[6], R[0] * cos(y) + R[3] * sin(y));
  const double r = atan2(R[2] * sin(y) - R[5] * cos(y), -R[1] * sin(y) + R[4] * cos(y));
  ypr[0] = y / kPi * 180.0, ypr[1] = p / kPi * 180.0, ypr[2] = r / kPi * 180.0;
}
VIO_DEV void mul3(const double *A, const double *B, double *C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
// Utility::ypr2R (utility.hpp:93-121): Rz(y) Ry(p) Rx(r), degrees in
VIO_DEV void ypr_to_rot(const double *ypr, double *R) {
  const double y = ypr[0] / 180.0 * kPi, p = ypr[1] / 180.0 * kPi, r = ypr[2] / 180.0 * kPi;
  const double Rz[9] = {cos(y), -sin(y), 0, sin(y), cos(y), 0, 0, 0, 1};
  const double Ry[9] = {cos(p), 0., sin(p), 0., 1., 0., -sin(p), 0., cos(p)};
  const double Rx[9] = {1., 0., 0., 0., cos(r), -sin(r), 0., sin(r), cos(r)};
  double T[9];
  mul3(Rz, Ry, T), mul3(T, Rx, R);
}
// R v + t
VIO_DEV void move_point(const double *R, const double *v, const double *t, double *out) {
  for (int a = 0; a < 3; a++) out[a] = R[3 * a] * v[0] + R[3 * a + 1] * v[1] + R[3 * a + 2] * v[2] + t[a];
}
// |a - b|, b = null: the origin (the walks start with last_P = 0)
VIO_DEV double step_norm(const double *a, const double *b) {
  const double q[3] = {b ? b[0] : 0.0, b ? b[1] : 0.0, b ? b[2] : 0.0};
  return sqrt((a[0] - q[0]) * (a[0] - q[0]) + (a[1] - q[1]) * (a[1] - q[1]) + (a[2] - q[2]) * (a[2] - q[2]));
}

// rank[i] = how many k < i satisfy pred(k); returns the total. Every work-item calls it. The list is walked nt elements
// at a time as in store_keyframe (store_core.h): a ballot per wave, the waves' counts through LDS, a running base. No
// atomics, so the ranks are the list's order whatever the timing.
template <class F>
VIO_DEV int ballot_rank(const Cx &cx, int n, ldsi rank, ldsi part, F pred) {
  const int t = VIO_TID(cx), lane = t & 63, wave = t >> 6, nw = (cx.nt + 63) >> 6;
  int run = 0;
  for (int base = 0; base < n; base += cx.nt) {
    const int i = base + t;
    const bool p = i < n && pred(i);
    const unsigned long long m = __builtin_amdgcn_ballot_w64(p);
    if (lane == 0) part[wave] = __builtin_popcountll(m);
    VIO_SYNC();
    int k = run + __builtin_popcountll(m & ((1ull << lane) - 1)), total = 0;
    for (int w = 0; w < nw; w++) {
      const int c = part[w];
      k += w < wave ? c : 0, total += c;
    }
    if (i < n) rank[i] = k;
    run += total;
    VIO_SYNC();  // (part is written again in the next trip; rank is read by other work-items after the last one)
  }
  return run;
}

// total_length / last_P over a whole list in list order (updateVisualization :358-378): norms in parallel, one
// work-item sums them (the sum's order is the reference's). Every work-item calls it.
VIO_DEV void path_length(const Cx &cx, const VioPoseGraphKeyframe *kf, int n, const Lds &l, double *state) {
  VIO_PARFOR(i, n) l.dist[i] = step_norm(kf[i].t, i > 0 ? kf[i - 1].t : nullptr);
  VIO_SYNC();
  if (VIO_TID(cx) == 0) {
    double len = 0;
    for (int i = 0; i < n; i++) len += l.dist[i];
    state[S_LEN] = len;
    for (int a = 0; a < 3; a++) state[S_LASTP + a] = n > 0 ? kf[n - 1].t[a] : 0.0;
  }
  VIO_SYNC();
}

// ---- add ---------------------------------------------------------------------------------------------------------------
// One work-item. The origin pose is the pose given, the current pose r_drift P + t_drift, r_drift R.
VIO_DEV void kfdb_add(const List &ls, int pos, double *state, double header, const double *P, const double *R, int global_index,
                      int segment) {
  VioPoseGraphKeyframe &k = ls.kf[pos];
  for (int a = 0; a < 3; a++) k.origin_t[a] = P[a];
  for (int a = 0; a < 9; a++) k.origin_r[a] = R[a];
  double t[3], r[9];
  move_point(state + S_RD, P, state + S_TD, t);
  mul3(state + S_RD, R, r);
  state[S_LEN] += step_norm(t, state + S_LASTP);
  for (int a = 0; a < 3; a++) k.t[a] = t[a], state[S_LASTP + a] = t[a];
  for (int a = 0; a < 9; a++) k.r[a] = r[a];
  k.global_index = global_index, k.has_loop = 0, k.is_looped = 0, k.loop_index = -1;
  for (int a = 0; a < 8; a++) k.loop_info[a] = 0.0;
  ls.header[pos] = header, ls.seg[pos] = segment;
}

// ---- update ------------------------------------------------------------------------------------------------------------
// One wave. loop_pos >= 0: the keyframe the relocalization belongs to; wrong: the host's verdict on |relative_yaw| > 30
// or |relative_t| > 10 (it sees the same arguments). rel = relative_t [3], relative_q (x y z w) [4], relative_yaw. The
// newest `count` keyframes (the host's min(n, 2 window_size + 1)) are compared with header0, `nt` per trip.
VIO_DEV void kfdb_update(const Cx &cx, const List &ls, int n, int loop_pos, int wrong, const double *rel, int count, double header0,
                         const double *P0, const double *R0) {
  const int t = VIO_TID(cx);
  if (t == 0 && loop_pos >= 0) {
    VioPoseGraphKeyframe &k = ls.kf[loop_pos];
    if (wrong) {
      k.has_loop = 0;
    } else {  // updateLoopConnection (keyframe.cpp:347-354): t, q as w x y z, yaw
      k.loop_info[0] = rel[0], k.loop_info[1] = rel[1], k.loop_info[2] = rel[2];
      k.loop_info[3] = rel[6], k.loop_info[4] = rel[3], k.loop_info[5] = rel[4], k.loop_info[6] = rel[5];
      k.loop_info[7] = rel[7];
    }
  }
  int found = -1;
  for (int base = 0; base < count && found < 0; base += cx.nt) {  // (uniform: every lane sees the same ballot)
    const int i = base + t;
    const bool hit = i < count && ls.header[n - 1 - i] == header0;
    const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
    if (m) found = base + __builtin_ctzll(m);
  }
  if (t == 0 && found >= 0) {
    VioPoseGraphKeyframe &k = ls.kf[n - 1 - found];
    for (int a = 0; a < 3; a++) k.origin_t[a] = P0[a];
    for (int a = 0; a < 9; a++) k.origin_r[a] = R0[a];
  }
}

// ---- build -------------------------------------------------------------------------------------------------------------
// The solver's inputs of one graph (rows of PgPtrs)
struct Graph {
  int *hdr, *col;
  double *node0;
  int *ei, *ej, *ek;
  double *meas;
};

// kf[0 .. m): the list from the first keyframe with global_index >= earliest_loop_index to cur_index (the host found both
// and checked that every loop of the range lands inside it). skip [m] and ypr [m][3] stay in global memory for kfdb_apply.
VIO_DEV void kfdb_build(const Cx &cx, const VioPoseGraphKeyframe *kf, int m, double total_length, int max_frame_num, bool list_short,
                        int max_iterations, const Lds &l, const Graph &g, int *skip, double *ypr) {
  const int t = VIO_TID(cx);
  // (i) step norms against the keyframe before, kept or not (last_P follows every keyframe); the first against the origin
  VIO_PARFOR(k, m) {
    l.dist[k] = step_norm(kf[k].t, k > 0 ? kf[k - 1].t : nullptr);
    l.flag[k] = (kf[k].has_loop || kf[k].is_looped) ? 1 : 0;
    l.used[k] = 0;
    double y[3];
    rot_to_ypr(kf[k].origin_r, y);
    ypr[3 * k] = y[0], ypr[3 * k + 1] = y[1], ypr[3 * k + 2] = y[2];
    g.node0[4 * k] = y[0], g.node0[4 * k + 1] = kf[k].origin_t[0], g.node0[4 * k + 2] = kf[k].origin_t[1], g.node0[4 * k + 3] = kf[k].origin_t[2];
  }
  VIO_SYNC();
  // (ii) need_resample (:170-198): the distance since the last kept keyframe is a running sum that a kept keyframe resets,
  // and its comparison with min_dis decides a discrete flag. One work-item walks the norms in LDS in list order: a few
  // hundred to a few thousand additions, against a scan that would reassociate the sum and could flip a flag.
  if (t == 0) {
    const double min_dis = total_length / (1.0 * max_frame_num);
    double travelled = 0;
    for (int k = 0; k < m; k++) {
      travelled += l.dist[k];
      const bool keep = k == 0 || travelled > min_dis || l.flag[k] || list_short;
      if (keep) travelled = 0;
      l.flag[k] = keep ? 1 : 0;
    }
  }
  VIO_SYNC();
  // (iii) kept rank, and the loops before every node (a keyframe with a loop is always kept)
  const int n_kept = ballot_rank(cx, m, l.rank, l.part, [&](int k) { return l.flag[k] != 0; });
  const int n_loops = ballot_rank(cx, m, l.rank2, l.part, [&](int k) { return kf[k].has_loop != 0; });
  VIO_PARFOR(k, m) {
    skip[k] = l.flag[k] ? 0 : 1;
    if (l.flag[k]) l.kept[l.rank[k]] = k;
  }
  VIO_SYNC();
  // (iv) edges of a kept node: min(5, rank) sequential ones, nearest kept predecessor first, then its loop edge. Their
  // first slot is the exclusive scan of that count over the kept nodes = a closed form of the rank + the loops before.
  auto seq_before = [](int r) { return r <= 5 ? r * (r - 1) / 2 : 10 + 5 * (r - 5); };
  VIO_PARFOR(k, m) {
    if (!l.flag[k]) continue;
    const int r = l.rank[k];
    int e = seq_before(r) + l.rank2[k];
    // (v) relative translation in the predecessor's frame, yaw difference, the predecessor's pitch and roll (:254-259)
    for (int j = 1; j <= 5 && j <= r; j++, e++) {
      const int c = l.kept[r - j];
      const double d[3] = {kf[k].origin_t[0] - kf[c].origin_t[0], kf[k].origin_t[1] - kf[c].origin_t[1], kf[k].origin_t[2] - kf[c].origin_t[2]};
      const double *Rc = kf[c].origin_r;
      double *ms = g.meas + 6 * e;
      for (int a = 0; a < 3; a++) ms[a] = Rc[a] * d[0] + Rc[3 + a] * d[1] + Rc[6 + a] * d[2];
      ms[3] = ypr[3 * k] - ypr[3 * c], ms[4] = ypr[3 * c + 1], ms[5] = ypr[3 * c + 2];
      g.ei[e] = c, g.ej[e] = k, g.ek[e] = 0;
      l.used[c] = 1, l.used[k] = 1;
    }
    if (kf[k].has_loop) {  // (:273-290) the partner by its global_index: the list is ascending by construction
      const int want = kf[k].loop_index;
      int lo = 0, hi = m;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (kf[mid].global_index < want) lo = mid + 1;
        else hi = mid;
      }
      const int c = lo < m ? lo : 0;  // (the host refused the call otherwise; asked again because c becomes an address)
      double *ms = g.meas + 6 * e;
      ms[0] = kf[k].loop_info[0], ms[1] = kf[k].loop_info[1], ms[2] = kf[k].loop_info[2], ms[3] = kf[k].loop_info[7];
      ms[4] = ypr[3 * c + 1], ms[5] = ypr[3 * c + 2];
      g.ei[e] = c, g.ej[e] = k, g.ek[e] = 1;
      l.used[c] = 1, l.used[k] = 1;
    }
  }
  VIO_SYNC();
  // (vi) unknowns: the first node is constant (:224-228), a node no edge names is not part of the program
  const int nv = ballot_rank(cx, m, l.rank, l.part, [&](int k) { return k > 0 && l.used[k] != 0; });
  VIO_PARFOR(k, m) g.col[k] = (k > 0 && l.used[k]) ? 4 * l.rank[k] : -1;
  if (t == 0) g.hdr[0] = m, g.hdr[1] = seq_before(n_kept) + n_loops, g.hdr[2] = 4 * nv, g.hdr[3] = max_iterations;
}

// ---- apply -------------------------------------------------------------------------------------------------------------
// ls: the whole list (n keyframes); the graph was nodes first .. cur of it. xout: the solver's unknowns of this graph.
// seg_cur / seg_old: segment of the current keyframe and of the one its loop points to (the host's mirror has both).
// drift_out [kDriftD]: yaw_drift, r_drift, t_drift, for the host.
VIO_DEV void kfdb_apply(const Cx &cx, const List &ls, int n, int first, int cur, int seg_cur, int seg_old, const Lds &l, const Graph &g,
                        const double *xout, const int *skip, const double *ypr, double *state, double *drift_out) {
  const int t = VIO_TID(cx), m = cur - first + 1;
  VioPoseGraphKeyframe *kf = ls.kf + first;
  // the last kept node at or before a skipped one = the kept node of rank (kept before it) - 1: node 0 is always kept
  ballot_rank(cx, m, l.rank, l.part, [&](int k) { return skip[k] == 0; });
  VIO_PARFOR(k, m)
    if (!skip[k]) l.kept[l.rank[k]] = k;
  VIO_SYNC();
  auto pose_of = [&](int k, double *p, double *R) {  // ypr2R(optimized yaw, pitch, roll) and the optimized t (:313-315)
    double y[3] = {ypr[3 * k], ypr[3 * k + 1], ypr[3 * k + 2]};
    const int c = g.col[k];
    if (c >= 0) y[0] = xout[c], p[0] = xout[c + 1], p[1] = xout[c + 2], p[2] = xout[c + 3];
    else p[0] = g.node0[4 * k + 1], p[1] = g.node0[4 * k + 2], p[2] = g.node0[4 * k + 3];
    ypr_to_rot(y, R);
  };
  VIO_PARFOR(k, m) {
    double p[3], R[9];
    pose_of(k, p, R);
    if (skip[k]) {  // r_drift_it, t_drift_it of the last kept node (:316-327)
      const int c = l.kept[l.rank[k] - 1];
      double pc[3], Rc[9], Ro_t[9], dr[9], dt[3], Rn[9], pn[3];
      pose_of(c, pc, Rc);
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) Ro_t[3 * a + b] = kf[c].origin_r[3 * b + a];
      mul3(Rc, Ro_t, dr);
      const double *po = kf[c].origin_t;
      for (int a = 0; a < 3; a++) dt[a] = pc[a] - (dr[3 * a] * po[0] + dr[3 * a + 1] * po[1] + dr[3 * a + 2] * po[2]);
      mul3(dr, R, Rn);
      move_point(dr, p, dt, pn);
      for (int a = 0; a < 9; a++) kf[k].r[a] = Rn[a];
      for (int a = 0; a < 3; a++) kf[k].t[a] = pn[a];
    } else {
      for (int a = 0; a < 9; a++) kf[k].r[a] = R[a];
      for (int a = 0; a < 3; a++) kf[k].t[a] = p[a];
    }
    // the reference's quirk: the break comes before the relabelling, the current keyframe keeps its segment (:329-333)
    if (k < m - 1 && ls.seg[first + k] == seg_cur) ls.seg[first + k] = seg_old;
  }
  VIO_SYNC();
  if (t == 0) {  // drift of the current keyframe (:336-342)
    const int c = m - 1;
    double now[3], org[3];
    rot_to_ypr(kf[c].r, now), rot_to_ypr(kf[c].origin_r, org);
    const double yd[3] = {now[0] - org[0], 0, 0};
    double Rd[9];
    ypr_to_rot(yd, Rd);
    const double *po = kf[c].origin_t;
    state[S_YAW] = yd[0];
    for (int a = 0; a < 9; a++) state[S_RD + a] = Rd[a];
    for (int a = 0; a < 3; a++) state[S_TD + a] = kf[c].t[a] - (Rd[3 * a] * po[0] + Rd[3 * a + 1] * po[1] + Rd[3 * a + 2] * po[2]);
    for (int a = 0; a < kDriftD; a++) drift_out[a] = state[S_YAW + a], l.misc[a] = state[S_YAW + a];
  }
  VIO_SYNC();
  // every keyframe after cur_index follows the drift (:344-352)
  VIO_PARFOR(i, n - cur - 1) {
    VioPoseGraphKeyframe &k = ls.kf[cur + 1 + i];
    double Rd[9], td[3], pn[3], Rn[9];
    for (int a = 0; a < 9; a++) Rd[a] = l.misc[1 + a];
    for (int a = 0; a < 3; a++) td[a] = l.misc[10 + a];
    move_point(Rd, k.origin_t, td, pn);
    mul3(Rd, k.origin_r, Rn);
    for (int a = 0; a < 3; a++) k.t[a] = pn[a];
    for (int a = 0; a < 9; a++) k.r[a] = Rn[a];
  }
  VIO_SYNC();
  path_length(cx, ls.kf, n, l, state);
}

// ---- resample ----------------------------------------------------------------------------------------------------------
// src (n keyframes, n >= max_frame_num: the host returns early otherwise) compacted into dst in order. erased: the
// global_index of every erased keyframe, ascending; counts[0] = kept, counts[1] = erased.
VIO_DEV void kfdb_resample(const Cx &cx, const List &src, const List &dst, int n, int max_frame_num, const Lds &l, double *state,
                           int *erased, int *counts) {
  const int t = VIO_TID(cx);
  VIO_PARFOR(i, n) {
    l.dist[i] = step_norm(src.kf[i].t, i > 0 ? src.kf[i - 1].t : nullptr);
    l.flag[i] = (src.kf[i].has_loop || src.kf[i].is_looped) ? 1 : 0;
  }
  VIO_SYNC();
  if (t == 0) {  // the same recurrence as need_resample: one work-item, list order (see kfdb_build)
    const double min_dis = state[S_LEN] / (0.8 * max_frame_num);
    double dis = 0;
    for (int i = 0; i < n; i++) {
      dis += l.dist[i];
      const bool keep = i == 0 || dis > min_dis || l.flag[i];
      if (keep) dis = 0;
      l.flag[i] = keep ? 1 : 0;
    }
  }
  VIO_SYNC();
  const int n_kept = ballot_rank(cx, n, l.rank, l.part, [&](int i) { return l.flag[i] != 0; });
  VIO_PARFOR(i, n) {
    const int r = l.rank[i];
    if (l.flag[i]) dst.kf[r] = src.kf[i], dst.header[r] = src.header[i], dst.seg[r] = src.seg[i];
    else erased[i - r] = src.kf[i].global_index;
  }
  if (t == 0) counts[0] = n_kept, counts[1] = n - n_kept;
  VIO_SYNC();
  path_length(cx, dst.kf, n_kept, l, state);
}

}  // namespace kfdb
}  // namespace vio
