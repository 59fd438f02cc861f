// tests/emul/simt_kfdb.cpp — TEST-ONLY: the list passes of the keyframe database (kfdb_build, kfdb_apply, kfdb_resample of
// vins-mobile_amd/csrc/kfdb_core.h) executed on the host by the SIMT emulator: 256 fibers, one workgroup, the wave ballots
// with the hardware's lane semantics. Every launch gets a freshly poisoned LDS (nothing survives from one launch to the
// next); the caller (tests/test_keyframe_db.py) poisons the outputs and compares them with vio_posegraph_build /
// vio_posegraph_apply of the product library and with its own restatement of resample.
// Not part of the product library.
#define SIMT_IMPLEMENTATION
#include "simt.h"

#include <vector>

#include "kfdb_core.h"

using namespace vio;
namespace kd = vio::kfdb;

namespace {

struct PoisonedLds {
  std::vector<double> mem;
  kd::Lds l;
  explicit PoisonedLds(int cap) : mem(kd::lds_bytes(cap) / sizeof(double) + 2) {
    memset(mem.data(), 0xff, mem.size() * sizeof(double));  // NaN as doubles, -1 as ints
    l = kd::carve_lds(cap, mem.data());
  }
};

}  // namespace

// kf [m]: the graph's range of the list. cap >= m: the capacity the LDS is carved for. Outputs as the solver takes them.
extern "C" int simt_kfdb_build(const VioPoseGraphKeyframe *kf, int m, int cap, double total_length, int max_frame_num, int list_short,
                               int max_iterations, int order, int *hdr, int *col, double *node0, int *ei, int *ej, int *ek, double *meas,
                               int *skip, double *ypr) {
  if (m < 1 || cap < m) return -1;
  PoisonedLds lds(cap);
  const kd::Graph g{hdr, col, node0, ei, ej, ek, meas};
  simt::launch(kd::kThreads, [&](int tid) {
    kd::Cx cx{tid, kd::kThreads};
    kd::kfdb_build(cx, kf, m, total_length, max_frame_num, list_short != 0, max_iterations, lds.l, g, skip, ypr);
  }, order);
  return 0;
}

// kf / seg [n]: the whole list, changed in place. state [17] in / out, drift [13] out.
extern "C" int simt_kfdb_apply(VioPoseGraphKeyframe *kf, double *header, int *seg, int n, int cap, int first, int cur, int seg_cur, int seg_old,
                               int order, int *hdr, int *col, double *node0, const double *xout, const int *skip, const double *ypr,
                               double *state, double *drift) {
  if (n < 1 || cap < n || first < 0 || cur < first || cur >= n) return -1;
  PoisonedLds lds(cap);
  const kd::List ls{kf, header, seg};
  const kd::Graph g{hdr, col, node0, nullptr, nullptr, nullptr, nullptr};
  simt::launch(kd::kThreads, [&](int tid) {
    kd::Cx cx{tid, kd::kThreads};
    kd::kfdb_apply(cx, ls, n, first, cur, seg_cur, seg_old, lds.l, g, xout, skip, ypr, state, drift);
  }, order);
  return 0;
}

extern "C" int simt_kfdb_resample(VioPoseGraphKeyframe *src_kf, double *src_header, int *src_seg, int n, int cap, int max_frame_num, int order,
                                  VioPoseGraphKeyframe *dst_kf, double *dst_header, int *dst_seg, double *state, int *erased, int *counts) {
  if (n < 1 || cap < n) return -1;
  PoisonedLds lds(cap);
  const kd::List src{src_kf, src_header, src_seg}, dst{dst_kf, dst_header, dst_seg};
  simt::launch(kd::kThreads, [&](int tid) {
    kd::Cx cx{tid, kd::kThreads};
    kd::kfdb_resample(cx, src, dst, n, max_frame_num, lds.l, state, erased, counts);
  }, order);
  return 0;
}
