// tests/emul/simt_sfm.cpp — TEST-ONLY: the batched bundle adjustment kernel (vins-mobile_amd/csrc/sfm_core.h) executed on the
// host by the SIMT emulator: 256 fibers per problem, s_barrier with the hardware's semantics, LDS and the global slabs
// poisoned with NaN before every problem. The host packing is the product's (sfm_pack.h). Not part of the product library.
#define SIMT_IMPLEMENTATION
#include "simt.h"

#include <limits>
#include <vector>

#include "sfm_pack.h"

using namespace vio;

// order: lane order of the emulator (0 forward, 1 reverse, >= 2 seeded shuffle); slab != 0 keeps the landmark state in the
// global slab whatever the size (the route of problems too large for LDS).
extern "C" int simt_sfm_solve(VioInitBaProblem *problems, int n, VioSolveStats *stats, int order, int slab) {
  if (n < 0 || (n > 0 && !problems)) return VIO_EINVAL;
  std::vector<sfm::Shape> sh(n);
  for (int b = 0; b < n; b++) {
    const int rc = sfm::check_problem(problems[b], &sh[b]);
    if (rc != VIO_OK) return rc;
  }
  if (n == 0) return VIO_OK;
  sfm::HostBatch hb;
  sfm::pack(problems, sh.data(), n, hb);
  const double kNaN = std::numeric_limits<double>::quiet_NaN();
  const bool in_lds = !slab && sfm::points_fit_lds(hb.Fm, hb.Pm);
  std::vector<double> out(sfm::dbl_stride(hb.Fm, hb.Pm, 0) * n, kNaN), ob((size_t)n * sfm::kObsDoubles * hb.Om, kNaN),
      slab_d(in_lds ? 1 : (size_t)n * sfm::kPointDoubles * hb.Pm, kNaN), sd((size_t)n * kStatsDoubles, kNaN);
  std::vector<int> si((size_t)n * kStatsInts, -1);
  sfm::Batch B;
  B.n = n, B.Fm = hb.Fm, B.Pm = hb.Pm, B.Om = hb.Om;
  B.ints = hb.ints.data(), B.in = hb.in.data(), B.out = out.data(), B.ob = ob.data(), B.slab = in_lds ? nullptr : slab_d.data();
  B.stats_d = sd.data(), B.stats_i = si.data();
  for (int b = 0; b < n; b++) {
    std::vector<double> lds(sfm::lds_bytes(hb.Fm, in_lds ? hb.Pm : 0) / sizeof(double) + 2, kNaN);
    const sfm::View v = sfm::view_of(B, b);
    simt::launch(sfm::kThreads, [&](int tid) {
      sfm::Work<double *> w;
      sfm::carve<double *>(hb.Fm, lds.data(), in_lds ? nullptr : v.slab, hb.Pm, &w);
      sfm::solve(tid, v, w);
    }, order);
  }
  for (int b = 0; b < n; b++) {
    VioSolveStats st;
    unpack_solve_stats(&sd[(size_t)b * kStatsDoubles], &si[(size_t)b * kStatsInts], &st);
    sfm::unpack(hb, b, out.data(), st, problems[b]);
    if (stats) stats[b] = st;
  }
  return VIO_OK;
}
