// tests/emul/simt_sfm_large.cpp — TEST-ONLY: the large layout of the batched bundle adjustment kernel
// (vins-mobile_amd/csrc/sfm_core.h: packed reduced matrix, 512 work-items, diagonal camera blocks and landmarks in global
// slabs) executed on the host by the SIMT emulator: 512 fibers per problem, LDS of exactly sfm::large_lds_bytes bytes, LDS
// and every slab poisoned with NaN before a problem. The host checks and packing are the product's (sfm_pack.h). A batch
// is split by frame count as vio_init_ba_solve splits it; `force` sends the problems of up to sfm::kSmallFrames frames
// through the large layout too. Not part of the product library.
#define SIMT_IMPLEMENTATION
#include "simt.h"

#include <stdint.h>
#include <string.h>

#include <limits>
#include <vector>

#include "sfm_pack.h"

using namespace vio;

namespace {

constexpr size_t kGuard = 64;  // doubles behind the large layout's LDS

// false: a work-item wrote behind the LDS the large layout declares
bool run_group(VioInitBaProblem *pr, const sfm::Shape *sh, int n, bool large, int order, VioSolveStats *stats) {
  sfm::HostBatch hb;
  sfm::pack(pr, sh, n, hb);
  const double kNaN = std::numeric_limits<double>::quiet_NaN();
  const bool in_lds = !large && sfm::points_fit_lds(hb.Fm, hb.Pm);
  std::vector<double> out(sfm::dbl_stride(hb.Fm, hb.Pm, 0) * n, kNaN), ob((size_t)n * sfm::kObsDoubles * hb.Om, kNaN),
      slab(in_lds ? 1 : (size_t)n * sfm::kPointDoubles * hb.Pm, kNaN), hcc(large ? (size_t)n * 36 * hb.Fm : 1, kNaN), sd((size_t)n * kStatsDoubles, kNaN);
  std::vector<int> si((size_t)n * kStatsInts, -1);
  sfm::Batch B;
  B.n = n, B.Fm = hb.Fm, B.Pm = hb.Pm, B.Om = hb.Om;
  B.ints = hb.ints.data(), B.in = hb.in.data(), B.out = out.data(), B.ob = ob.data(), B.slab = in_lds ? nullptr : slab.data();
  B.stats_d = sd.data(), B.stats_i = si.data(), B.hcc = large ? hcc.data() : nullptr;
  for (int b = 0; b < n; b++) {
    const sfm::View v = sfm::view_of(B, b);
    if (large) {
      // exactly the bytes the launch declares (a multiple of 8: the integer tables hold an even count), then a guard zone
      // of NaNs with a payload: a read past the end poisons the result, a write past the end is found below
      const size_t words = sfm::large_lds_bytes(hb.Fm) / sizeof(double);
      std::vector<double> lds(words + kGuard, kNaN);
      const uint64_t mark = 0x7ff8c0dec0dec0deull;
      for (size_t i = 0; i < kGuard; i++) memcpy(&lds[words + i], &mark, 8);
      simt::launch(sfm::Large::kThreads, [&](int tid) {
        sfm::Work<double *, sfm::Large> w;
        sfm::carve_large(hb.Fm, lds.data(), v, hb.Pm, &w);
        sfm::solve(tid, v, w);
      }, order);
      for (size_t i = 0; i < kGuard; i++)
        if (memcmp(&lds[words + i], &mark, 8) != 0) return false;
    } else {
      std::vector<double> lds(sfm::lds_bytes(hb.Fm, in_lds ? hb.Pm : 0) / sizeof(double) + 2, kNaN);
      simt::launch(sfm::kThreads, [&](int tid) {
        sfm::Work<double *> w;
        sfm::carve<double *>(hb.Fm, lds.data(), in_lds ? nullptr : v.slab, hb.Pm, &w);
        sfm::solve(tid, v, w);
      }, order);
    }
  }
  for (int b = 0; b < n; b++) {
    VioSolveStats st;
    unpack_solve_stats(&sd[(size_t)b * kStatsDoubles], &si[(size_t)b * kStatsInts], &st);
    sfm::unpack(hb, b, out.data(), st, pr[b]);
    if (stats) stats[b] = st;
  }
  return true;
}

}  // namespace

enum { kLdsOverrun = -1000 };  // (no VIO_* status)

// order: lane order of the emulator (0 forward, 1 reverse, >= 2 seeded shuffle); force != 0: every problem runs the large
// layout, whatever its frame count.
extern "C" int simt_sfm_large_solve(VioInitBaProblem *problems, int n, VioSolveStats *stats, int order, int force) {
  if (n < 0 || (n > 0 && !problems)) return VIO_EINVAL;
  std::vector<sfm::Shape> sh(n);
  for (int b = 0; b < n; b++) {
    const int rc = sfm::check_problem(problems[b], &sh[b]);
    if (rc != VIO_OK) return rc;
  }
  for (int large = 0; large < 2; large++) {
    std::vector<VioInitBaProblem> pr;
    std::vector<sfm::Shape> gs;
    std::vector<int> slot;
    for (int b = 0; b < n; b++)
      if ((force || sh[b].F > sfm::kSmallFrames) == (large != 0)) pr.push_back(problems[b]), gs.push_back(sh[b]), slot.push_back(b);
    if (pr.empty()) continue;
    std::vector<VioSolveStats> gst(pr.size());
    if (!run_group(pr.data(), gs.data(), (int)pr.size(), large != 0, order, gst.data())) return kLdsOverrun;
    for (size_t g = 0; g < pr.size(); g++) {
      problems[slot[g]].ok = pr[g].ok;
      if (stats) stats[slot[g]] = gst[g];
    }
  }
  return VIO_OK;
}

// bytes of LDS the large layout declares for a launch whose largest problem has `frames` frames
extern "C" long simt_sfm_large_lds_bytes(int frames) { return (long)sfm::large_lds_bytes(frames); }
