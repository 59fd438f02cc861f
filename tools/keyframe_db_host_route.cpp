// tools/keyframe_db_host_route.cpp — the route a C / C++ caller that keeps its own keyframe lists takes through one
// optimize4DoFLoopPoseGraph for S sessions, as one C call so that tools/keyframe_db_timing.py times no interpreter work:
// vio_posegraph_build per session, ONE batched vio_posegraph_optimize, vio_posegraph_apply per session, updatePose of the
// graph's keyframes and the move of the keyframes after cur_index (keyfame_database.cpp:344-352). All buffers are
// allocated at create. Built by the timing tool against csrc/libvio_amd.so; not part of the product library.
#include <string.h>

#include <vector>

#include "vio_amd.h"

namespace {

struct HostRoute {
  int S, n_kf;
  std::vector<double> t, ypr, meas, out_t, out_r;  // per session: n_kf nodes, 6 n_kf edges
  std::vector<uint8_t> skip, kind;
  std::vector<int32_t> ei, ej;
  std::vector<VioPoseGraph> graphs;
  std::vector<VioSolveStats> stats;
};

}  // namespace

extern "C" {

void *kfdb_host_route_create(int S, int n_kf) {
  HostRoute *h = new HostRoute();
  h->S = S, h->n_kf = n_kf;
  const size_t N = (size_t)S * n_kf, E = 6 * N;
  h->t.resize(3 * N), h->ypr.resize(3 * N), h->meas.resize(6 * E), h->out_t.resize(3 * N), h->out_r.resize(9 * N);
  h->skip.resize(N), h->kind.resize(E), h->ei.resize(E), h->ej.resize(E);
  h->graphs.resize(S), h->stats.resize(S);
  return h;
}

void kfdb_host_route_destroy(void *p) { delete (HostRoute *)p; }

// kf [S][n_kf]: the lists (the current poses are updated in place). first [S]: the first keyframe of each graph; cur_pos:
// the current keyframe's position (the same in every list). -> VIO_OK; t_drift [S][3], the sum of the solves' iterations.
int kfdb_host_route_run(void *p, vio_posegraph_t *pg, VioPoseGraphKeyframe *kf, const int32_t *first, int32_t cur_pos,
                        const double *total_length, int32_t max_frame_num, double *t_drift, int32_t *iterations) {
  HostRoute *h = (HostRoute *)p;
  const int S = h->S, K = h->n_kf;
  for (int s = 0; s < S; s++) {
    const size_t o = (size_t)s * K, eo = 6 * o;
    const int m = cur_pos + 1 - first[s];
    int32_t ne = 0;
    const int rc = vio_posegraph_build(kf + o + first[s], m, total_length[s], max_frame_num, K, &h->t[3 * o], &h->ypr[3 * o], &h->skip[o], 6 * m,
                                       &h->ei[eo], &h->ej[eo], &h->kind[eo], &h->meas[6 * eo], &ne);
    if (rc != VIO_OK) return rc;
    h->graphs[s] = VioPoseGraph{m, &h->t[3 * o], &h->ypr[3 * o], 0, ne, &h->ei[eo], &h->ej[eo], &h->kind[eo], &h->meas[6 * eo]};
  }
  int rc = vio_posegraph_optimize(pg, h->graphs.data(), S, 5, h->stats.data());
  if (rc != VIO_OK) return rc;
  *iterations = 0;
  for (int s = 0; s < S; s++) {
    const size_t o = (size_t)s * K;
    const int m = cur_pos + 1 - first[s];
    VioPoseGraphKeyframe *list = kf + o;
    double yaw, rd[9], *td = t_drift + 3 * s;
    rc = vio_posegraph_apply(list + first[s], m, &h->t[3 * o], &h->ypr[3 * o], &h->skip[o], &h->out_t[3 * o], &h->out_r[9 * o], &yaw, rd, td);
    if (rc != VIO_OK) return rc;
    for (int k = 0; k < m; k++) {  // updatePose
      memcpy(list[first[s] + k].t, &h->out_t[3 * (o + k)], 24);
      memcpy(list[first[s] + k].r, &h->out_r[9 * (o + k)], 72);
    }
    for (int i = cur_pos + 1; i < K; i++) {  // r_drift * origin + t_drift
      VioPoseGraphKeyframe &k = list[i];
      for (int a = 0; a < 3; a++) {
        k.t[a] = rd[3 * a] * k.origin_t[0] + rd[3 * a + 1] * k.origin_t[1] + rd[3 * a + 2] * k.origin_t[2] + td[a];
        for (int b = 0; b < 3; b++) k.r[3 * a + b] = rd[3 * a] * k.origin_r[b] + rd[3 * a + 1] * k.origin_r[3 + b] + rd[3 * a + 2] * k.origin_r[6 + b];
      }
    }
    *iterations += h->stats[s].iterations;
  }
  return VIO_OK;
}

}  // extern "C"
