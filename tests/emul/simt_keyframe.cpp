// tests/emul/simt_keyframe.cpp — TEST-ONLY: the fourth pass of the landmark store (store_keyframe, vins-mobile_amd/csrc/
// store_core.h) executed on the host by the SIMT emulator: 256 fibers, one workgroup, the wave ballots with the hardware's
// lane semantics. The list arrives as vio_features_dump gives it and goes into a NaN-poisoned bank; the caller (tests/
// test_keyframe_features.py) poisons the outputs and compares them with vio_features_keyframe of the product library.
// Not part of the product library.
#define SIMT_IMPLEMENTATION
#include "simt.h"

#include <limits>
#include <vector>

#include "store_core.h"

using namespace vio;
namespace st = vio::store;

// bank: which of the two banks holds the list (the other one stays poisoned). Returns 0, or -1 for a list the store would
// not have taken.
extern "C" int simt_store_keyframe(int W, int Lcap, int bank, int n, const VioFeatureInfo *info, const double *points, const double *Ps,
                                   const double *Rs, const double *tic, const double *ric, const double *intr, int cap, int order, int *ids,
                                   float *px, float *norm, double *cloud, int *count) {
  const int P = W + 1;
  if (n > Lcap || bank < 0 || bank > 1) return -1;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<int> fid[2], start[2], nobs[2], flag[2], ctl(st::C_COUNT, 0);
  std::vector<double> depth[2], obs[2];
  for (int b = 0; b < 2; b++) {
    fid[b].assign(Lcap, -7), start[b].assign(Lcap, -7), nobs[b].assign(Lcap, -7), flag[b].assign(Lcap, -7);
    depth[b].assign(Lcap, nan), obs[b].assign((size_t)Lcap * P * 3, nan);
  }
  size_t p = 0;
  for (int i = 0; i < n; i++) {
    const VioFeatureInfo &f = info[i];
    if (f.n_obs < 1 || f.start_frame < 0 || f.start_frame + f.n_obs > P) return -1;
    fid[bank][i] = f.id, start[bank][i] = f.start_frame, nobs[bank][i] = f.n_obs, flag[bank][i] = f.solve_flag, depth[bank][i] = f.estimated_depth;
    for (int j = 0; j < f.n_obs; j++, p++)
      for (int c = 0; c < 3; c++) obs[bank][((size_t)i * P + j) * 3 + c] = points[3 * p + c];
  }
  ctl[st::C_N] = n, ctl[st::C_BANK] = bank;
  st::Dims d;
  d.W = W, d.Lcap = Lcap, d.Ocap = 1;
  const st::Bank bk{fid[bank].data(), start[bank].data(), nobs[bank].data(), flag[bank].data(), depth[bank].data(), obs[bank].data()};
  std::vector<int> part(st::kThreads / 64 + 1, -1);  // nothing survives in LDS from one launch to the next
  const st::KeyOut o{ids, px, norm, cloud, count, cap};
  simt::launch(st::kThreads, [&](int tid) {
    st::Cx cx{tid, st::kThreads};
    st::store_keyframe(cx, d, bk, ctl.data(), part.data(), Ps, Rs, tic, ric, intr[0], intr[1], intr[2], intr[3], o);
  }, order);
  return 0;
}
