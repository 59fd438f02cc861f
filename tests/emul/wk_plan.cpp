// wk_plan.cpp -- drives the window launcher's plan (csrc/wk_plan.h, plain host C++) from cases on stdin, for tests/test_wk_plan.py.
// One case per line, one line of answer each. max_features / max_factors: the VioConfig's.
//   plan host|resident max_features max_factors W loop n_cus peers profile forced coop_ok  na active[0..na)  n nfeat[0..n)
//       (na = -1: no active list, all n windows take part.) The dims are the path's growth rule for the landmark maximum F of the
//       windows that take part, 8 F factors, no prior columns beyond 6 W + 15, and room for a relocalization pose when loop = 1.
//       Answer: rc n_lds n_glb variant static_w lds_asp Flds lds_bytes need Flds_glb lds_bytes_glb chunk chunk_glb width grid
//               | order | lds_matrix lds_asp threads ws   (the traits of `variant`; need: LDS need of the chosen LDS layout)
//   fcap host|resident max_features max_factors F     -> the landmark capacity of a first batch with landmark maximum F
//   walk W loop lds_asp                                -> the largest F in [1, 1000] whose LDS layout fits half a CU (0: none)
#define SIMT_IMPLEMENTATION
#include "simt.h"  // (the solver headers under wk_plan.h build for the host with -DVIO_SIMT; nothing is executed)

#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "wk_plan.h"

using namespace vio;

static BatchDims grown(const std::string &path, int max_features, int max_factors, int W, int F, bool loop) {
  VioConfig cfg = {};
  cfg.window_size = W, cfg.max_features = max_features, cfg.max_factors = max_factors, cfg.max_iterations = 10;
  return vio_wk::grow_dims(cfg, vio_wk::Need{W, F, 8 * F, 0, loop}, path == "resident" ? vio_wk::kResidentGrowth : vio_wk::kHostGrowth, nullptr);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, path;
    in >> cmd;
    if (cmd == "plan") {
      int maxf, maxm, W, loop, n_cus, peers, profile, forced, coop_ok, na, n;
      in >> path >> maxf >> maxm >> W >> loop >> n_cus >> peers >> profile >> forced >> coop_ok >> na;
      std::vector<int> active(na > 0 ? na : 0);
      for (auto &a : active) in >> a;
      in >> n;
      std::vector<int> nfeat(n);
      for (auto &f : nfeat) in >> f;
      if (!in) return 2;
      int F = 1;
      for (int b = 0; b < n; b++)
        if (na < 0) F = std::max(F, nfeat[b]);
      for (int b : active) F = std::max(F, nfeat[b]);
      const BatchDims d = grown(path, maxf, maxm, W, F, loop != 0);
      const vio_wk::Layout L = vio_wk::plan_layout(d, n, nfeat.data(), na < 0 ? nullptr : &active, W == vio_wk::kStaticW, n_cus, peers, profile != 0);
      if (L.rc != VIO_OK) {
        printf("%d\n", L.rc);
        continue;
      }
      const int width = L.n_glb > 0 ? vio_wk::coop_width(L.n_glb, L.d_glb.Wcap, L.lds_bytes_glb, n_cus, peers, forced, profile != 0, coop_ok != 0) : 1;
      const size_t need = L.n_lds > 0 ? vio_wk::lds_need(L.d_lds, true, vio_wk::kThreadsLds, L.d_lds.lds_asp != 0) : 0;
      printf("%d %d %d %d %d %d %d %zu %zu %d %zu %d %d %d %d |", L.rc, L.n_lds, L.n_glb, L.variant, L.static_w ? 1 : 0, L.d_lds.lds_asp, L.d_lds.Flds,
             L.lds_bytes, need, L.n_glb > 0 ? L.d_glb.Flds : 0, L.n_glb > 0 ? L.lds_bytes_glb : (size_t)0, L.chunk, L.chunk_glb, width,
             vio_wk::coop_grid(L.n_glb, width));
      for (int b : L.order) printf(" %d", b);
      const vio_wk::VariantTraits &t = vio_wk::kTraits[L.variant];
      printf(" | %d %d %d %d\n", t.lds_matrix ? 1 : 0, t.lds_asp ? 1 : 0, t.threads, t.ws);
    } else if (cmd == "fcap") {
      int maxf, maxm, F;
      in >> path >> maxf >> maxm >> F;
      if (!in) return 2;
      printf("%d\n", grown(path, maxf, maxm, 10, F, false).Fcap);
    } else if (cmd == "walk") {
      int W, loop, asp, best = 0;
      in >> W >> loop >> asp;
      if (!in) return 2;
      BatchDims d = grown("host", 1000, 8192, W, 1000, loop != 0);
      for (int F = 1; F <= 1000; F++) {
        d.Flds = F;
        if (vio_wk::lds_eligible(d, vio_wk::kThreadsLds, asp != 0) && vio_wk::lds_need(d, true, vio_wk::kThreadsLds, asp != 0) <= vio_wk::kLdsHalf) best = F;
      }
      printf("%d\n", best);
    } else {
      return 2;
    }
  }
  return 0;
}
