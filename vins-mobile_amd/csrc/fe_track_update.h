// fe_track_update.h -- the tracker's per-sequence update, one workgroup per sequence: inBorder + reduceVector, rejectWithF
// (findFundamentalMat, fe_ransac.h), track_cnt++ and setMask (feature_tracker.cpp:183-205, :235-255, :50-87).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fe_common.h"
#include "fe_ransac.h"

namespace {

// ---- per-sequence tracker update -------------------------------------------------------------------------------
struct TrackerArrays {
  int cap;
  int rows, cols;
  float *cur_pts, *pre_pts, *forw_pts;  // [seq][cap][2]
  int *ids, *track_cnt;                  // [seq][cap]
  int *n_pts;                            // [seq] number of tracked points (cur)
  int *n_forw;                           // [seq] after this kernel: points kept
  int *n_id;                             // [seq] next id
  uint8_t *lk_status;                    // [seq][cap]
  int *kept_xy;                          // [seq][cap][2] rounded centres of kept features (for the mask painter)
  int *n_kept;                           // [seq]
  float *pnp_pts;                        // [seq][cap][2] forw_pts / ids as solveVinsPnP sees them (feature_tracker.cpp:207:
  int *pnp_ids, *n_pnp;                  // behind the first F-RANSAC, ahead of rejectWithF / setMask)
  const int *hw;                         // [2 r + 1] half-widths of the filled circle
  int radius;
  float f_thresh;
  double f_conf;
  long long *prof;  // null, or cycle stamps of sequence 0's workgroup (VIO_AMD_TU_PROF, tools/tu_prof.sh)
};

// The per-feature arrays are staged in LDS once and never moved: the tracks still alive are a stable list of their slots
// (idx), which every filter shortens. The launcher picks the smallest instantiation (CAP) that holds the tracker's feature
// slots: with the 512-slot layout only ONE workgroup fits a CU and the 512 sequences of the bench ran as two rounds.
template <int CAP>
struct TrackShared {
  float pre[CAP][2], cur[CAP][2], forw[CAP][2];  // by slot, as loaded
  int ids[CAP], cnt[CAP];
  int keep[CAP];  // flags of the filter in hand: by slot for the first one, by list position afterwards (dword flags: sub-dword LDS accesses are slow)
  int idx[CAP];   // the list
  int pos[CAP];
  float4 pack[CAP];  // (x1, y1, x2, y2) of the list's correspondences, for the F-test in hand
  int n;             // length of the list
  int order[CAP];
  int ncnt[CAP];  // publish frames: track_cnt + 1, by list position
  int ixy[CAP][2];
  unsigned long long inside[CAP][CAP / 64];
  int hw[2 * kMaxRadius + 1];  // half-widths of the filled circle (setMask), staged from global memory
};

// Shortens the list to the entries whose keep flag is set, in order: idx[rank of i among the kept] = idx[i] (FIRST: = i, the
// flags are by slot and the list is all of them). The caller's last barrier lies behind the writes of keep[] and T.n.
// Exclusive rank: a ballot per wave and chunk of blockDim items, the waves' counts through LDS. In place: a chunk reads its
// entries before its barrier and writes behind it, to positions no later chunk reads.
// (This replaces a compaction that also copied the eight arrays to temporaries and back after every filter: six barriers and
// two passes over the arrays per call, three calls per publish frame.)
template <int CAP, bool FIRST>
__device__ __forceinline__ void shorten_list(TrackShared<CAP> &T) {
  __shared__ int s_wcnt[16];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int wave = tid >> 6, lane = tid & 63, nwv = nt >> 6;
  const int n = T.n;
  int running = 0;
  for (int base = 0; base < n; base += nt) {
    const int i = base + tid;
    const bool k = i < n && T.keep[i];
    const int v = FIRST ? i : (i < n ? T.idx[i] : 0);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(k);
    if (lane == 0) s_wcnt[wave] = __builtin_popcountll(b);
    __syncthreads();
    int off = running, total = 0;
    for (int w = 0; w < nwv; w++) {
      const int c = s_wcnt[w];
      if (w < wave) off += c;
      total += c;
    }
    if (k) T.idx[off + __builtin_popcountll(b & ((1ull << lane) - 1ull))] = v;
    running += total;
    if (base + nt < n) __syncthreads();  // (the next chunk writes the waves' counts again)
  }
  if (tid == 0) T.n = running;  // (everyone read n ahead of the chunk barrier; n == 0 stays 0)
  __syncthreads();
}

struct PackedPts {
  const float4 *pack;
  __device__ __forceinline__ float4 operator()(int i) const { return pack[i]; }
};

// One workgroup per sequence: everything between the LK call and goodFeaturesToTrack.
// (two waves per SIMD: left to itself the compiler takes 289 registers per work-item for the double-precision 7-point code --
// ONE wave per SIMD, one workgroup per CU, and the 512 sequences of the bench ran as two rounds of 256 workgroups)
// (REG: the region of interest, RegionArgs of fe_common.h, or nothing: the kernel as it always was)
template <int CAP, class... REG>
__global__ __launch_bounds__(256, 2) void track_update_kernel(TrackerArrays A, int publish, REG... region) {
  constexpr bool REGION = sizeof...(REG) != 0;
  const RegionArgs G = region_args(region...);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  TrackShared<CAP> &T = *reinterpret_cast<TrackShared<CAP> *>(smem_raw);
  RansacShared &R = *reinterpret_cast<RansacShared *>(smem_raw + ((sizeof(TrackShared<CAP>) + 15) & ~(size_t)15));
  const int seq = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
#include "fe_track_update_body.inc"
}

// Subset instantiation: one launch over the call's n sequences, workgroup i takes sequence seq[i] with publish[i].
template <int CAP, class... REG>
__global__ __launch_bounds__(256, 2) void track_update_subset_kernel(TrackerArrays A, SubsetArgs M, REG... region) {
  constexpr bool REGION = sizeof...(REG) != 0;
  const RegionArgs G = region_args(region...);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  TrackShared<CAP> &T = *reinterpret_cast<TrackShared<CAP> *>(smem_raw);
  RansacShared &R = *reinterpret_cast<RansacShared *>(smem_raw + ((sizeof(TrackShared<CAP>) + 15) & ~(size_t)15));
  const int seq = subset_at(M.seq, blockIdx.x), publish = subset_at(M.publish, blockIdx.x);
  const int tid = threadIdx.x, nt = blockDim.x;
#include "fe_track_update_body.inc"
}

}  // namespace
