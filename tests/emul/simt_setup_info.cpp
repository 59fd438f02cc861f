// tests/emul/simt_setup_info.cpp — TEST-ONLY: the sizes that the set-up of a solve (solver_core.h: solve_window's head,
// build_gram_pieces, setup_prior) works with for one window, from the same pack / carve code and the same LDS rule as
// tests/emul/simt_backend.cpp's simt_solve_window. The tests of the set-up check by these numbers that every window is the case
// it claims to be (slots against the workgroup size, the prior's size against the tile and batch sizes, staged or unstaged J0).
// Nothing is executed.
#define SIMT_IMPLEMENTATION
#include "simt.h"

#include <algorithm>

#include "wk_plan.h"

using namespace vio;

// out[0] = factors, out[1] = slots (nslots), out[2] = (host, target) buckets, out[3] = columns of the prior, out[4] = its blocks,
// out[5] = 1: matrix in LDS, out[6] = doubles of the staging area (J0 is staged when n^2 fits), out[7] = work-items.
// variant / order: as simt_solve_window. Returns VIO_OK, or the error simt_solve_window would return.
extern "C" int simt_setup_info(const VioConfig *cfg, const VioWindow *win, int nthreads, int variant, int order, int *out, int cap) {
  if (nthreads != 256 && nthreads != 512) return VIO_EINVAL;
  if (cap < 8) return VIO_EINVAL;
  bool any_loop = false;
  for (int k = 0; k < win->n_factors; k++)
    if (win->factor_target[k] == win->window_size + 1) any_loop = true;
  HostBatch hb;
  hb.resize(make_dims(*cfg, win->window_size, win->n_features, win->n_factors, any_loop), 1);
  hb.d.lds_asp = variant == 2 ? 0 : 1;
  const bool lds_shape = pose_jp(hb.d) <= 16 * kPanelTiles && variant != 0;
  int rc = pack_window(hb, 0, *win, false, order % 2 ? 0 : stage_chunk_slots(hb.d, lds_shape, nthreads));
  if (rc != VIO_OK) return rc;
  BatchDims d = hb.d;
  d.Flds = std::max(1, win->n_features);
  d.lds_asp = variant == 2 ? 0 : 1;
  // LDS or global matrix: the launcher's rule for one window (wk_plan.h)
  bool lds_matrix = vio_wk::lds_eligible(d, nthreads, d.lds_asp != 0);
  if ((variant == 1 || variant == 2) && !lds_matrix) return VIO_ECAP;
  if (variant == 0) lds_matrix = false;
  const size_t need = vio_wk::lds_need(d, lds_matrix, nthreads, d.lds_asp != 0);
  if (need > kLdsBytes) return VIO_ECAP;
  const size_t lds_bytes = lds_matrix ? vio_wk::lds_grant(need) : need;
  const Carved<double *> cw = carve_all<double *>(d, lds_matrix, nthreads, nullptr, nullptr, nullptr, lds_bytes / sizeof(double));
  const int *h = hb.hdr.data();
  out[0] = h[H_M], out[1] = h[H_NSLOTS], out[2] = h[H_NPAIRS], out[3] = h[H_PRIOR_N], out[4] = h[H_PRIOR_NB];
  out[5] = lds_matrix ? 1 : 0, out[6] = cw.w.nstage, out[7] = nthreads;
  return VIO_OK;
}
