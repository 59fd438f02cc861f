// tests/emul/simt_marg_info.cpp — TEST-ONLY: what the marginalization's factor pass (marg_core.h) works with for one window,
// from the same pack / carve code and the same LDS rule as tests/emul/simt_backend.cpp's simt_solve_window: the staging chunk
// (MargWorkT::stage_slots) and the slot ranges of the buckets hosted at frame 0. The tests of the factor pass size their
// windows by these numbers instead of hard-coding them. Nothing is executed.
#define SIMT_IMPLEMENTATION
#include "simt.h"

#include <algorithm>

#include "wk_plan.h"

using namespace vio;

// out[0] = staging chunk in slots, out[1] = S0 (slots of the factor pass), out[2] = nb0 (buckets (0, t) it walks),
// out[3] = 1: matrix in LDS, then (s0, s1, t) of every bucket hosted at frame 0, at most `cap` ints in all.
// variant / order: as simt_solve_window. Returns VIO_OK, or the error simt_solve_window would return.
extern "C" int simt_marg_info(const VioConfig *cfg, const VioWindow *win, int nthreads, int variant, int order, int *out, int cap) {
  if (nthreads != 256 && nthreads != 512) return VIO_EINVAL;
  if (cap < 4) return VIO_EINVAL;
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
  const size_t lds_doubles = lds_bytes / sizeof(double);
  const Carved<double *> cw = carve_all<double *>(d, lds_matrix, nthreads, nullptr, nullptr, nullptr, lds_doubles);
  const MargWorkT<double *> mw =
      carve_marg_all<double *>(d, lds_matrix, nullptr, nullptr, lds_doubles - cw.state_end_doubles - cw.tail_doubles).m;
  const int P = win->window_size + 1, npairs = hb.hdr[H_NPAIRS];
  int S0 = 0, nb0 = 0, o = 4;
  for (int p = 0; p < npairs && hb.pair_h[p] == 0; p++) {
    if (hb.pair_t[p] != P) S0 = (hb.pair_s1[p] + 1) & ~1, nb0 = p + 1;
    if (o + 3 <= cap) out[o++] = hb.pair_s0[p], out[o++] = hb.pair_s1[p], out[o++] = hb.pair_t[p];
  }
  out[0] = mw.stage_slots, out[1] = S0, out[2] = nb0, out[3] = lds_matrix ? 1 : 0;
  return VIO_OK;
}
