// wk_plan.h -- how the back end launches a batch of windows (vio_backend.hip): plain host C++, no HIP. Which windows run with the
// pose matrix in LDS and which in global scratch, in which order, at which instantiation of the window kernel, at half or a whole
// CU of LDS, at which cooperative width and grid, and how a batch's capacities grow. Every answer is returned by value: tests/emul/
// wk_plan.cpp checks the policy without a device, and the emulator (tests/emul/simt_*.cpp) sizes its one window by lds_need.
#pragma once
#include <algorithm>
#include <vector>

#include "batch.h"
#include "marg_core.h"

namespace vio_wk {

using vio::BatchDims;

constexpr int kThreadsLds = 256, kThreadsGlb = 512;

// variant: pose matrix in LDS?, IMU coupling in LDS?, work-items, compile-time window size (0: run-time)
//   0  LDS, LDS, 256, 0     the fat layout (two windows per CU up to 186 landmarks at W = 10, 126 with a relocalization pose)
//   1  LDS, scratch, 256, 0 the lean layout (two per CU up to 340 landmarks, 280 with a relocalization pose)
//   2  scratch, scratch, 512, 0   W > 12 (cooperative windows)
//   3  = 0 with W = 10 at compile time (the reference's WINDOW_SIZE, global_param.hpp:28), no relocalization pose in the batch
//   4  = 1 with W = 10 at compile time
constexpr int kVariants = 5, kGlbVariant = 2;
constexpr int kStaticW = 10;
struct VariantTraits {
  bool lds_matrix, lds_asp;
  int threads, ws;
};
constexpr VariantTraits kTraits[kVariants] = {{true, true, kThreadsLds, 0},        {true, false, kThreadsLds, 0}, {false, false, kThreadsGlb, 0},
                                              {true, true, kThreadsLds, kStaticW}, {true, false, kThreadsLds, kStaticW}};
// the instantiation of an LDS launch
constexpr int lds_variant(bool lds_asp, bool static_w) { return (lds_asp ? 0 : 1) + (static_w ? 3 : 0); }
constexpr bool variant_is(int v, bool lds_matrix, bool lds_asp, int threads, int ws) {
  return kTraits[v].lds_matrix == lds_matrix && kTraits[v].lds_asp == lds_asp && kTraits[v].threads == threads && kTraits[v].ws == ws;
}
static_assert(variant_is(lds_variant(true, false), true, true, kThreadsLds, 0) && variant_is(lds_variant(false, false), true, false, kThreadsLds, 0) &&
                  variant_is(lds_variant(true, true), true, true, kThreadsLds, kStaticW) &&
                  variant_is(lds_variant(false, true), true, false, kThreadsLds, kStaticW) && variant_is(kGlbVariant, false, false, kThreadsGlb, 0),
              "the launcher's variant indices and the table of instantiations");

constexpr size_t kLdsLimit = vio::kLdsBytes;      // one CU
constexpr size_t kLdsHalf = vio::kLdsBytes / 2;   // two resident workgroups per CU

// ---- one window ---------------------------------------------------------------------------------------------------------
// LDS that a workgroup of `threads` work-items needs for a window of dims d (d.Flds landmarks): both phases have to fit. The
// marginalization phase re-carves what lies between the fixed part of the iterate and its landmarks and additionally wants >= 64
// staging slots behind its matrix (matrix in global scratch: behind its vectors, it stages its Jacobian rows in LDS there too).
inline size_t lds_need(BatchDims d, bool lds_matrix, int threads, bool lds_asp) {
  d.lds_asp = lds_asp ? 1 : 0;
  size_t se = 0, tail = 0;
  const size_t bs = vio::carve_work<double *>(d, lds_matrix, threads, nullptr, nullptr, nullptr, nullptr, &se, &tail);
  const size_t bm = (se + tail) * sizeof(double) + vio::carve_marg<double *>(d, lds_matrix, nullptr, nullptr, nullptr, 0);
  return std::max(bs, bm + 64 * (lds_matrix ? vio::kMargSlot : vio::kWideSlot) * sizeof(double));
}
// May the window run with its pose matrix in LDS? That variant keeps the fill tiles of the speed-bias band in registers (pose
// matrices of at most kPanelTiles tile rows: W <= 12) and needs both phases inside the CU's LDS.
inline bool lds_eligible(const BatchDims &d, int threads, bool lds_asp) {
  return vio::pose_jp(d) <= 16 * vio::kPanelTiles && lds_need(d, true, threads, lds_asp) <= kLdsLimit;
}
// what an LDS-matrix workgroup is given: half a CU whenever that is enough, so that two windows share a CU
inline size_t lds_grant(size_t need) { return need <= kLdsHalf ? kLdsHalf : kLdsLimit; }

// ---- capacities of a batch ------------------------------------------------------------------------------------------------
// Capacities (global strides, allocations) are sticky and grow in generous steps: a batch that fits the previous layout re-stages
// and reallocates nothing (hipFree synchronizes the device and page-locked reallocation costs milliseconds, which stalls every
// other context on the GPU), and landmark and factor counts of a running batch drift by a few percent from frame to frame.
struct Growth {
  int f_div, m_div;      // headroom: 1 / f_div of the landmarks, 1 / m_div of the factors, then rounded to 64 / 128
  int f_floor, m_floor;  // smallest capacities of a growth
};
// windows from the host: 25 % landmarks, 12.5 % factors (every factor slot is ~60 bytes of upload per window)
constexpr Growth kHostGrowth = {4, 8, 0, 0};
// windows packed on the device: nothing here travels over the bus and every growth is a round of hipFree / hipMalloc that stalls
// the device for ~10 ms
constexpr Growth kResidentGrowth = {2, 2, 384, 3072};
struct Need {
  int W, F, M, N;  // largest window size, landmark, factor and prior-column counts of the batch
  bool loop;       // some window carries a relocalization pose: one more 6-dof block, other strides, another LDS layout
};
// may a batch with these needs keep the layout d?
inline bool fits(const BatchDims &d, const Need &q) {
  return q.W == d.Wcap && q.F <= d.Fcap && q.M <= d.Mcap && q.N <= d.Ncap && (!q.loop || d.nblk_cap == d.Pcap + 1);
}
// floor: a layout the new one does not go below (capacities, room for a relocalization pose), null: none
inline BatchDims grow_dims(const VioConfig &cfg, const Need &q, const Growth &g, const BatchDims *floor) {
  const int Fr = std::min(cfg.max_features, std::max(g.f_floor, (q.F + q.F / g.f_div + 63) / 64 * 64)),
            Mr = std::min(cfg.max_factors, std::max(g.m_floor, (q.M + q.M / g.m_div + 127) / 128 * 128));
  BatchDims d = vio::make_dims(cfg, q.W, std::max({Fr, q.F, floor ? floor->Fcap : 1}), std::max({Mr, q.M, floor ? floor->Mcap : 1}),
                               q.loop || (floor && floor->nblk_cap == floor->Pcap + 1));
  d.Ncap = std::max(6 * q.W + 15, q.N);  // what marginalize() can leave behind: W poses, one speed-bias, the extrinsic
  return d;
}

// ---- the two launches of a batch --------------------------------------------------------------------------------------------
// A batch is split by variant: windows whose matrix and vectors fit the CU's LDS, and the rest (relocalization pose, very many
// landmarks) with the matrix in global scratch.
struct Layout {
  int rc = VIO_OK;  // VIO_ECAP: a window fits neither variant (nothing else is valid then)
  BatchDims d{};    // the batch: strides and allocations
  std::vector<int> order;  // launch-local block -> window: the LDS launch's windows, then the global-matrix launch's
  int n_lds = 0, n_glb = 0;
  BatchDims d_lds{}, d_glb{};  // d carved for the landmark maximum of each launch
  size_t lds_bytes = kLdsLimit, lds_bytes_glb = 0;
  int variant = 0;        // of the LDS launch (the other one is kGlbVariant)
  bool static_w = false;  // ... and whether it is one with the window size at compile time
  int chunk = 0, chunk_glb = 0;  // staging slots per pass of the Jacobian evaluation: what each launch's buckets are aligned to
  bool lds_matrix() const { return n_glb == 0; }  // every window of the batch runs an LDS variant
};

// May the LDS launch of this batch take the instantiations with the window size at compile time? Every window has W = kStaticW
// frames, no window carries a relocalization pose (one more 6-dof block: other strides, another LDS layout) and the prior capacity
// is what marginalize() can leave at that size.
inline bool static_launch_ok(const BatchDims &d, bool all_windows_static_w) {
  constexpr int W = kStaticW;
  return all_windows_static_w && d.Wcap == W && d.Pcap == W + 1 && d.nblk_cap == W + 1 && d.n6cap == 6 * (W + 2) &&
         d.Ncap == 6 * W + 15 && d.pair_cap == (W + 2) * (W + 3) / 2;
}

// LDS layout and launch split of a batch of n windows whose dims are d. nfeat[b]: landmarks of window b; active: the windows that
// take part (null: all n); peers: contexts whose window kernels share the device's n_cus compute units at the same time.
inline Layout plan_layout(BatchDims d, int n, const int *nfeat, const std::vector<int> *active, bool all_windows_static_w, int n_cus,
                          int peers, bool profile) {
  Layout L;
  std::vector<int> all;  // the windows that take part, in input order
  if (active) all = *active;
  else
    for (int b = 0; b < n; b++) all.push_back(b);
  std::vector<int> cand = all;
  int Fmax = 1;
  for (int b : all) Fmax = std::max(Fmax, nfeat[b]);
  // (the LDS layout is carved for the exact landmark maximum of THIS batch: every landmark costs LDS)
  d.Flds = Fmax;
  d.prof_stages = profile ? vio::ST_COUNT : 0;  // (the stage clock's accumulators live in LDS: only the profiling launches pay for them)
  // LDS or global pose matrix, per window. Eligible windows (the lean layout, IMU coupling in global memory, inside one CU) are
  // ordered by landmark count; the largest prefix whose layout (carved for its own landmark maximum) fits runs the LDS variant in
  // one launch, everything else the global-matrix variant in a second one. (Decided before packing: the staging chunk the buckets
  // are aligned to depends on the layout.)
  std::stable_sort(cand.begin(), cand.end(), [&](int a, int b2) { return nfeat[a] < nfeat[b2]; });
  BatchDims dl = d;
  int n_lds = (int)cand.size();
  while (n_lds > 0) {
    dl.Flds = std::max(1, nfeat[cand[n_lds - 1]]);
    if (lds_eligible(dl, kThreadsLds, false)) break;
    n_lds--;
  }
  std::vector<char> in_lds(n, 0);
  for (int i = 0; i < n_lds; i++) in_lds[cand[i]] = 1, L.order.push_back(cand[i]);
  for (int b : all)
    if (!in_lds[b]) L.order.push_back(b);
  L.n_lds = n_lds, L.n_glb = (int)all.size() - n_lds;
  // Two workgroups per CU (half its LDS each) beat everything else; inside that, the IMU speed-bias x pose coupling is
  // better off in LDS. Windows with many landmarks give its 14 KB up (global scratch, L2-resident) to stay two per CU.
  // The marginalization phase stages Jacobian rows in whatever LDS is left behind its matrix.
  if (n_lds > 0) {
    const size_t fat = lds_need(dl, true, kThreadsLds, true), lean = lds_need(dl, true, kThreadsLds, false);
    // (the lean layout costs a window ~10 % of its latency -- a few more round trips to L2 per Gauss-Newton step --: it only
    // pays when the launch has enough windows to fill the second workgroup slot of the CUs. Measured with closed-loop
    // windows of ~190 landmarks: 2 x 128 windows are faster with the fat layout on whole CUs, 2 x 256 windows take 7.3
    // instead of 9.4 ms per frame with the lean one.)
    const bool crowded = n_lds * std::max(1, peers) > n_cus;  // (with the other contexts' launches: more windows than CUs)
    if (fat <= kLdsHalf) dl.lds_asp = 1, L.lds_bytes = kLdsHalf;
    else if (crowded && lean <= kLdsHalf) dl.lds_asp = 0, L.lds_bytes = kLdsHalf;
    else dl.lds_asp = fat <= kLdsLimit ? 1 : 0;
  }
  L.d = d, L.d_lds = dl;
  if (L.n_glb > 0) {
    BatchDims dg = d;
    dg.Flds = 1;
    for (size_t i = n_lds; i < L.order.size(); i++) dg.Flds = std::max(dg.Flds, nfeat[L.order[i]]);
    L.lds_bytes_glb = lds_need(dg, false, kThreadsGlb, false);
    if (L.lds_bytes_glb > kLdsLimit) {
      L.rc = VIO_ECAP;
      return L;
    }
    L.d_glb = dg;
  }
  L.static_w = static_launch_ok(d, all_windows_static_w);
  L.variant = lds_variant(dl.lds_asp != 0, L.static_w);
  const bool lds_shape = vio::pose_jp(d) <= 16 * vio::kPanelTiles;
  L.chunk = vio::stage_chunk_slots(dl, lds_shape, lds_shape ? kThreadsLds : kThreadsGlb);
  // (windows of the global-matrix launch have their own layout and chunk; a cooperative launch needs every bucket inside a chunk)
  L.chunk_glb = L.n_glb > 0 ? vio::stage_chunk_slots(L.d_glb, false, kThreadsGlb) : 0;
  return L;
}

// ---- cooperative windows (solver_core.h) ------------------------------------------------------------------------------------
// Few large windows leave most CUs idle -- a window of the global-matrix launch gets 2 or 4 workgroups when all of them fit the
// chip at once (one per CU: this variant's workgroup takes more than half a CU's LDS). forced: 1 / 2 / 4 asks for that width
// (1: off; 0: none asked for). The profiling clock follows one workgroup per window: off while it runs. coop_ok: every bucket of
// these windows was packed inside one staging chunk. The answer is what the launch asks the runtime's occupancy for.
inline int cus_share(int n_cus, int peers) { return n_cus / std::max(1, peers); }
inline int coop_grid(int n_glb, int width) {  // (grids are padded to whole groups of eight windows: the XCD mapping)
  return width > 1 ? (n_glb + 7) / 8 * 8 * width : n_glb;
}
inline int coop_width(int n_glb, int Wcap, size_t lds_bytes_glb, int n_cus, int peers, int forced, bool profile, bool coop_ok) {
  if (!coop_ok || profile || lds_bytes_glb <= kLdsHalf) return 1;
  const int cus = cus_share(n_cus, peers), padded = coop_grid(n_glb, 2) / 2;
  // (measured, profiles/r05_*_large_windows.txt: four members pay at W = 30 up to a full chip, at W = 20 only while half the
  // CUs stay free -- with every CU busy the shared phases of 64 windows hit the memory system together)
  const bool four = padded * 4 <= cus && (Wcap >= 24 || padded * 8 <= cus);
  const int width = four ? 4 : padded * 2 <= cus ? 2 : 1;
  return forced >= 1 && forced <= vio::kCoopMax && padded * forced <= cus ? forced : width;  // (a forced width obeys the peers bound too)
}

}  // namespace vio_wk
