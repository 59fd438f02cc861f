// fe_select.h -- goodFeaturesToTrack, back half, and what follows it (feature_tracker.cpp:263-307): quality threshold, greedy
// min-distance pick in sorted order, addPoints, updateID, image_msg; the redo workgroups run the detector (fe_detect.h) again.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "fe_common.h"
#include "fe_detect.h"
#include "vio_amd.h"

namespace {

struct SelectParams {
  int cap, rows, cols, max_corners;
  float min_dist;
  const double *cam;  // [n_seq][4] fx, fy, cx, cy of every sequence's camera (vio_frontend_set_cameras)
};

constexpr int kSelThreads = 512;
constexpr int kSelMaxSeg = 256;  // strips of kDetR rows: images up to 8192 rows
constexpr int kSelLds = 8192;  // candidate keys kept in LDS (64 KB); larger lists are processed in place in HBM

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    unsigned long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// goodFeaturesToTrack back half: quality threshold, then greedy pick in sorted order with the min-distance rule
// == repeat { take the best alive candidate; kill everything closer than min_dist }. Then addPoints / updateID /
// image_msg and the end-of-publish copies (feature_tracker.cpp:271-307).
// Sequence `seq` from the list `cand`: nseg segments of seg_cap keys. full = false: the detector's ordinary list, segment g
// holds n_cand[g] keys. full = true: the redo's list, one slot per pixel (seg_cap = kDetR * cols, key or 0), every slot of a
// strip's rows is visited. skip: the detector flagged the sequence and a redo workgroup has it -- nothing is written (the flag is
// loaded with the sequence's counters and looked at behind them, so that it adds no trip to memory of its own in front of the work).
__device__ __forceinline__ void select_sequence(unsigned long long *cand, int seg_cap, int nseg, int *n_cand, unsigned *max_bits,
                                                double quality, const SelectParams &P, float *forw_pts, float *cur_pts,
                                                float *pre_pts, int *ids, int *track_cnt, int *n_forw, int *n_pts, int *n_id,
                                                VioObs *obs, int *n_obs, long long *prof, int seq, bool full, bool skip) {
  // prof: null, or cycle stamps of sequence 0's workgroup (VIO_AMD_CS_PROF, tools/cs_prof.sh)
#define CS_STAMP(k)                                                  \
  do {                                                               \
    if (prof && seq == 0 && threadIdx.x == 0) prof[k] = clock64(); \
  } while (0)
  CS_STAMP(0);
  __shared__ unsigned long long keys[kSelLds];
  __shared__ unsigned long long red[2][kSelThreads / 64];
  __shared__ int s_n, s_cnt;
  __shared__ unsigned s_mb;
  __shared__ int s_off[kSelMaxSeg + 1];
  __shared__ unsigned s_pick[kMaxCap];  // y << 16 | x of the corners taken, by output position
  __shared__ int s_wnew[kSelThreads / 64];
  static_assert(kMaxCap <= kSelThreads, "the id pass gives every feature slot its own work-item");
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  const size_t base = (size_t)seq * P.cap;
  const int n_old = n_forw[seq];
  int n = n_old;
  const int want = P.max_corners - n;
  const float md2 = P.min_dist * P.min_dist;
  // what the id and output passes need of the tracks that are already there: asked for now, used behind the selection
  const int nid0 = n_id[seq];
  int my_id = -1;
  float my_x = 0.f, my_y = 0.f;
  if (tid < n_old) my_id = ids[base + tid], my_x = forw_pts[(base + tid) * 2], my_y = forw_pts[(base + tid) * 2 + 1];
  // threshold(eig, maxVal * qualityLevel, THRESH_TOZERO): keep v > thr. Only the slots the detector really filled are
  // visited (prefix of the per-segment counts), survivors go to LDS and NOTHING is written back to the candidate list:
  // the first version zeroed every rejected and unused slot in HBM (0.6 MB per sequence and publish frame, twice the
  // frame itself) although only the rare in-place path below reads the list again.
  // The per-segment prefix and the maximum over the segments: one wave, one load of each counter per lane (work-item 0 walking
  // the counters was a chain of nseg dependent loads).
  if (wave == 0) {
    int carry = 0;
    unsigned mb = 0;
    for (int g0 = 0; g0 < nseg; g0 += 64) {
      const int g = g0 + lane;
      int c = 0;
      if (g < nseg) c = full ? min(kDetR, P.rows - g * kDetR) * P.cols : min(n_cand[(size_t)seq * nseg + g], seg_cap);
      mb = max(mb, g < nseg ? max_bits[(size_t)seq * nseg + g] : 0u);
      int incl = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        incl += lane >= o ? t : 0;
      }
      if (g < nseg) s_off[g] = carry + incl - c;
      carry += __shfl(incl, 63, 64);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mb = max(mb, (unsigned)__shfl_xor((int)mb, o, 64));
    if (lane == 0) s_off[nseg] = carry, s_mb = mb, s_n = n, s_cnt = 0;
  }
  __syncthreads();
  if (skip) return;  // (uniform)
  const unsigned mb = s_mb;
  const float thr = mb ? (float)((double)from_ordered_bits(mb) * quality) : 3.4e38f;
  const int real = s_off[nseg];
  // (every lane of a wave runs every trip: the survivors of a trip take their slots with ONE atomic per wave -- ballot and
  // popcount -- instead of one returning atomic per candidate on one address. The order of keys[] is free: keys are unique and
  // the rounds below take maxima. A work-item's indices only grow, so its segment search resumes where it stopped.)
  int sg = 0;
  for (int i0 = 0; i0 < real; i0 += nt) {
    const int i = i0 + tid;
    unsigned long long k = 0;
    if (i < real) {
      while (s_off[sg + 1] <= i) sg++;  // (i < s_off[nseg]: stops at a segment < nseg)
      k = cand[(size_t)sg * seg_cap + (i - s_off[sg])];
    }
    const bool ok = k && __uint_as_float((unsigned)(k >> 32)) > thr;
    const unsigned long long b = __builtin_amdgcn_ballot_w64(ok);
    if (b) {
      int slot0 = 0;
      if (lane == 0) slot0 = atomicAdd(&s_cnt, __builtin_popcountll(b));
      slot0 = __builtin_amdgcn_readfirstlane(slot0);
      const int slot = slot0 + __builtin_popcountll(b & ((1ull << lane) - 1ull));
      if (ok && slot < kSelLds) keys[slot] = k;
    }
  }
  __syncthreads();
  CS_STAMP(1);
  // this kernel is the only consumer of the per-segment counters: leave them zeroed for the next detection pass
  for (int g = tid; g < nseg; g += nt) n_cand[(size_t)seq * nseg + g] = 0, max_bits[(size_t)seq * nseg + g] = 0;
  if (s_cnt > kSelLds) {
    // More survivors than LDS holds (a cold start at 1280 x 720 / 1920 x 1080: ~10^5 candidates for 300 / 500 corners). The
    // first versions ran the round loop below over the WHOLE candidate range in HBM -- want x nseg x seg_cap visits, 43 ms /
    // 170 ms per frame at those sizes. The candidates are already bucketed: segment g holds the local maxima of strip g
    // (kDetR rows). So: one live maximum per strip in LDS, the global best is the maximum of those, and taking a corner only
    // touches the strips within min_dist of its row -- their candidates are suppressed and their maxima recomputed, the
    // others are not visited. Same picks in the same order (greedy in sorted order).
    __shared__ unsigned long long smax[kSelMaxSeg];
    __shared__ unsigned long long part[kSelThreads / 64][4];
    const int wv = tid >> 6, nwv = nt >> 6;
    // strips [g0, g0 + ng) (ng <= 4): suppress around (bx, by) when md2s >= 0 (else apply the quality threshold: first visit),
    // new maxima -> smax
    auto rescan = [&](int g0, int ng, int bx, int by, bool first) {
      unsigned long long m[4] = {0, 0, 0, 0};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (q >= ng) continue;
        unsigned long long *seg = cand + (size_t)(g0 + q) * seg_cap;
        const int cnt = s_off[g0 + q + 1] - s_off[g0 + q];
        for (int j = tid; j < cnt; j += nt) {
          const unsigned long long c = seg[j];
          if (!c) continue;
          bool dead;
          if (first) {
            dead = !(__uint_as_float((unsigned)(c >> 32)) > thr);
          } else if (P.min_dist >= 1.f) {
            const unsigned idx = 0xffffffffu - (unsigned)(c & 0xffffffffu);
            const float dx = (float)((int)(idx & 0xffffu) - bx), dy = (float)((int)(idx >> 16) - by);
            dead = dx * dx + dy * dy < md2;
          } else {
            const unsigned idx = 0xffffffffu - (unsigned)(c & 0xffffffffu);
            dead = (int)(idx & 0xffffu) == bx && (int)(idx >> 16) == by;
          }
          if (dead) seg[j] = 0;
          else m[q] = c > m[q] ? c : m[q];
        }
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const unsigned long long x = wave_max_u64(m[q]);
        if ((tid & 63) == 0) part[wv][q] = x;
      }
      __syncthreads();
      if (tid < ng) {
        unsigned long long x = part[0][tid];
        for (int w2 = 1; w2 < nwv; w2++) x = part[w2][tid] > x ? part[w2][tid] : x;
        smax[g0 + tid] = x;
      }
      __syncthreads();
    };
    for (int g0 = 0; g0 < nseg; g0 += 4) rescan(g0, min(4, nseg - g0), 0, 0, true);
    const int reach = P.min_dist >= 1.f ? (int)ceilf(P.min_dist) : 0;
    for (int round = 0; round < want; round++) {
      unsigned long long best = 0;  // (every wave takes the maximum over the strips for itself: no barrier)
      for (int g = tid & 63; g < nseg; g += 64) best = smax[g] > best ? smax[g] : best;
      best = wave_max_u64(best);
      if (best == 0) break;
      const unsigned bidx = 0xffffffffu - (unsigned)(best & 0xffffffffu);
      const int bx = bidx & 0xffffu, by = bidx >> 16;
      if (tid == 0) s_pick[s_n++] = bidx;  // addPoints :36-48 (the arrays are written by the output pass)
      const int glo = max(0, (by - reach) / kDetR), ghi = min(nseg - 1, (by + reach) / kDetR);
      for (int g0 = glo; g0 <= ghi; g0 += 4) rescan(g0, min(4, ghi - g0 + 1), bx, by, false);
    }
  } else {
  unsigned long long *K = keys;
  const int nc = s_cnt;
  // One pass over the candidates per round: it suppresses around the corner just taken AND collects the maximum of what
  // survives (the next corner) -- the first version walked the list twice per round with a barrier in between.
  unsigned long long mine = 0;  // this thread's largest live key
  for (int i = tid; i < nc; i += nt) {
    const unsigned long long k = K[i];
    mine = k > mine ? k : mine;
  }
  for (int round = 0; round < want; round++) {
    // (the waves' maxima alternate between two rows: a wave writes row r & 1 again only behind the barrier of round r + 1,
    // which every wave reaches behind its reads of round r -- one barrier per round, not two)
    unsigned long long best = wave_max_u64(mine);
    unsigned long long *rd = red[round & 1];
    if (lane == 0) rd[wave] = best;
    __syncthreads();
    best = rd[0];
#pragma unroll
    for (int w = 1; w < kSelThreads / 64; w++) best = rd[w] > best ? rd[w] : best;
    if (best == 0) break;
    const unsigned bidx = 0xffffffffu - (unsigned)(best & 0xffffffffu);
    const int bx = bidx & 0xffffu, by = bidx >> 16;
    if (tid == 0) s_pick[s_n++] = bidx;  // addPoints :36-48 (the arrays are written by the output pass)
    mine = 0;
    if (P.min_dist >= 1.f) {
      for (int i = tid; i < nc; i += nt) {
        const unsigned long long c = K[i];
        if (c) {
          const unsigned idx = 0xffffffffu - (unsigned)(c & 0xffffffffu);
          const float dx = (float)((int)(idx & 0xffffu) - bx), dy = (float)((int)(idx >> 16) - by);
          if (dx * dx + dy * dy < md2) K[i] = 0;
          else mine = c > mine ? c : mine;
        }
      }
    } else {
      for (int i = tid; i < nc; i += nt) {
        const unsigned long long c = K[i];
        if (c == best) K[i] = 0;
        else mine = c > mine ? c : mine;
      }
    }
  }
  }
  __syncthreads();
  CS_STAMP(2);
  n = s_n;
  // updateID (:311-321), image_msg (:297-306), pre_pts = cur_pts = forw_pts (:274, :285)
  // Work-item i owns feature i (n <= kMaxCap <= kSelThreads): a track that was there keeps the id loaded at the start, a
  // corner taken above has none (-1). The features without an id are numbered from n_id in index order, like the serial loop
  // (which was up to n dependent trips to global memory on one lane): rank = exclusive count of the -1 entries before i,
  // from a ballot per wave and the waves' counts through LDS.
  // the sequence's camera for image_msg below: one uniform load per workgroup, asked for ahead of the barrier of the id pass (the
  // selection rounds above do not carry it)
  const double *cam = P.cam + 4 * (size_t)seq;
  const double cam_fx = cam[0], cam_fy = cam[1], cam_cx = cam[2], cam_cy = cam[3];
  const bool is_new = tid >= n_old && tid < n;
  if (is_new) {
    const unsigned bidx = s_pick[tid];
    my_x = (float)(int)(bidx & 0xffffu), my_y = (float)(int)(bidx >> 16);
  }
  const bool no_id = tid < n && my_id == -1;
  const unsigned long long nb = __builtin_amdgcn_ballot_w64(no_id);
  if (lane == 0) s_wnew[wave] = __builtin_popcountll(nb);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kSelThreads / 64; w++) {
    const int c = s_wnew[w];
    before += w < wave ? c : 0;
    total += c;
  }
  if (no_id) my_id = nid0 + before + __builtin_popcountll(nb & ((1ull << lane) - 1ull));
  if (tid == 0) n_id[seq] = nid0 + total, n_forw[seq] = n, n_pts[seq] = n, n_obs[seq] = n;
  CS_STAMP(3);
  if (tid < n) {
    const int i = tid;
    const float x = my_x, y = my_y;
    if (is_new) forw_pts[(base + i) * 2] = x, forw_pts[(base + i) * 2 + 1] = y, track_cnt[base + i] = 1;
    if (no_id) ids[base + i] = my_id;
    cur_pts[(base + i) * 2] = x, cur_pts[(base + i) * 2 + 1] = y;
    pre_pts[(base + i) * 2] = x, pre_pts[(base + i) * 2 + 1] = y;
    VioObs o;
    o.id = my_id;
    o.x = ((double)x - cam_cx) / cam_fx, o.y = ((double)y - cam_cy) / cam_fy, o.z = 1.0;
    obs[base + i] = o;
  }
  CS_STAMP(4);
#undef CS_STAMP
}

constexpr int kRedoSlots = 4;  // full-size candidate lists a context owns: flagged sequences redone at the same time

struct RedoParams {  // what a redo workgroup needs to run the detector again, and where it finds the flags
  const uint8_t *img_base, *mask_base;
  size_t img_stride, mask_stride;
  const int *kept_xy, *n_kept, *hw;
  int radius;
  unsigned long long *full;  // [redo workgroups][rows * cols]
  const int *ovf;            // [n_seq] number of the last detection pass that dropped candidates of the sequence
  int epoch, n_seq, n_wg;    // this detection pass; redo workgroups behind the n_seq ordinary ones
  int *n_redo;               // sequences redone so far (statistics)
};

// Workgroups [0, n_seq): sequence blockIdx.x from the detector's list, unless the detector flagged it.
// Workgroups [n_seq, gridDim.x), the redo workgroups: the flagged sequences, each by ONE workgroup from start to end -- the
// detector again over the whole frame, tile by tile, into the workgroup's own full-size list (one key per pixel), then the same
// selection on that list. Redo workgroup k takes the flagged sequences k, k + n, k + 2n, ... in turn (n = redo workgroups), so
// any number of flagged sequences is served by n lists, no workgroup waits for another, and nothing depends on an order of
// arrival. With no flag up -- every frame of an ordinary stream -- a redo workgroup reads its share of the flags and exits.
// (Slow where it runs, one workgroup per frame: it is the exact answer for inputs the lists are not sized for, not a fast path.)
// (REG: the region of interest, as for detect_kernel: the exact redo reads the same mask words)
template <bool IMG_MASK, class... REG>
__global__ __launch_bounds__(kSelThreads) void corner_select_kernel(unsigned long long *cand_base, int seg_cap, int nseg,
                                                                    int *n_cand, unsigned *max_bits, RedoParams R,
                                                                    double quality, SelectParams P, float *forw_pts,
                                                                    float *cur_pts, float *pre_pts, int *ids, int *track_cnt,
                                                                    int *n_forw, int *n_pts, int *n_id, VioObs *obs,
                                                                    int *n_obs, long long *prof, REG... region) {
  const bool redo = (int)blockIdx.x >= R.n_seq;
  const int slot = (int)blockIdx.x - R.n_seq, n_slots = R.n_wg;
  if (redo) {
    int any = 0;
    for (int s = slot + n_slots * (int)threadIdx.x; s < R.n_seq; s += n_slots * kSelThreads) any |= R.ovf[s] == R.epoch;
    if (!__syncthreads_or(any)) return;
  }
  // (one call site of select_sequence for both kinds of workgroup: its 64 KB key list exists once)
  for (int seq = redo ? slot : (int)blockIdx.x; seq < R.n_seq; seq += redo ? n_slots : R.n_seq) {
    const bool flagged = R.ovf[seq] == R.epoch;  // (uniform)
    if (redo && !flagged) continue;
    unsigned long long *cand = cand_base + (size_t)seq * nseg * seg_cap;
    int cand_seg = seg_cap;
    if (redo) {
      cand = R.full + (size_t)slot * P.rows * P.cols, cand_seg = kDetR * P.cols;
      constexpr int NW = kSelThreads / 64;
      const int nbx = (P.cols + NW * kDetW - 1) / (NW * kDetW);
      for (int by = 0; by < nseg; by++)
        for (int bx = 0; bx < nbx; bx++) {
          detect_tile<IMG_MASK, true, NW, sizeof...(REG) != 0>(R.img_base, R.img_stride, R.mask_base, R.mask_stride, R.kept_xy, R.n_kept, P.cap, R.hw,
                                                               R.radius, (unsigned *)nullptr, P.rows, P.cols, (unsigned long long *)nullptr, 0,
                                                               (int *)nullptr, (int *)nullptr, 0, cand, seq, bx, by, nseg, region_args(region...));
          __syncthreads();  // (the next tile clears the mask words this one reads; behind the last tile: the list is written)
        }
      if (threadIdx.x == 0) atomicAdd(R.n_redo, 1);
    }
    select_sequence(cand, cand_seg, nseg, n_cand, max_bits, quality, P, forw_pts, cur_pts, pre_pts, ids, track_cnt, n_forw, n_pts, n_id,
                    obs, n_obs, redo ? (long long *)nullptr : prof, seq, redo, !redo && flagged);
    if (redo) __syncthreads();  // (the next sequence reuses the selection's LDS)
  }
}

// Subset instantiation (the step's form: no mask image): the same two kinds of workgroup over the n_pub PUBLISHED sequences of a
// call. Workgroup k < n_pub takes call position pub[k]; the redo workgroups behind them find the flagged sequences among those
// n_pub through ovf[] == epoch as above (a sequence outside the call keeps an older stamp or, after a reset, none). The image
// of a redo is level 0 of the sequence's forw bank (M.pyr, R.img_stride apart; R.img_base, R.mask_base and R.n_seq are not used).
// select_sequence is the lock-step kernel's, untouched: image_msg lands in the sequence's own row of obs / n_obs, and
// gather_obs_subset_kernel below packs the call's rows.
template <class... REG>
__global__ __launch_bounds__(kSelThreads) void corner_select_subset_kernel(SubsetArgs M, int n_pub, unsigned long long *cand_base,
                                                                           int seg_cap, int nseg, int *n_cand, unsigned *max_bits,
                                                                           RedoParams R, double quality, SelectParams P, float *forw_pts,
                                                                           float *cur_pts, float *pre_pts, int *ids, int *track_cnt,
                                                                           int *n_forw, int *n_pts, int *n_id, VioObs *obs, int *n_obs,
                                                                           REG... region) {
  const bool redo = (int)blockIdx.x >= n_pub;
  const int slot = (int)blockIdx.x - n_pub, n_slots = R.n_wg;
  if (redo) {
    int any = 0;
    for (int k = slot + n_slots * (int)threadIdx.x; k < n_pub; k += n_slots * kSelThreads) any |= R.ovf[M.seq[M.pub[k]]] == R.epoch;
    if (!__syncthreads_or(any)) return;
  }
  for (int k = redo ? slot : (int)blockIdx.x; k < n_pub; k += redo ? n_slots : n_pub) {
    const int i = subset_at(M.pub, k), seq = subset_at(M.seq, i);
    const bool flagged = R.ovf[seq] == R.epoch;  // (uniform)
    if (redo && !flagged) continue;
    unsigned long long *cand = cand_base + (size_t)seq * nseg * seg_cap;
    int cand_seg = seg_cap;
    if (redo) {
      cand = R.full + (size_t)slot * P.rows * P.cols, cand_seg = kDetR * P.cols;
      constexpr int NW = kSelThreads / 64;
      const int nbx = (P.cols + NW * kDetW - 1) / (NW * kDetW);
      const uint8_t *img = subset_bank(M, subset_at(M.forw_bank, i));
      for (int by = 0; by < nseg; by++)
        for (int bx = 0; bx < nbx; bx++) {
          detect_tile<false, true, NW, sizeof...(REG) != 0>(img, R.img_stride, (const uint8_t *)nullptr, (size_t)0, R.kept_xy, R.n_kept, P.cap, R.hw,
                                                            R.radius, (unsigned *)nullptr, P.rows, P.cols, (unsigned long long *)nullptr, 0, (int *)nullptr,
                                                            (int *)nullptr, 0, cand, seq, bx, by, nseg, region_args(region...));
          __syncthreads();  // (the next tile clears the mask words this one reads; behind the last tile: the list is written)
        }
      if (threadIdx.x == 0) atomicAdd(R.n_redo, 1);
    }
    select_sequence(cand, cand_seg, nseg, n_cand, max_bits, quality, P, forw_pts, cur_pts, pre_pts, ids, track_cnt, n_forw, n_pts, n_id, obs,
                    n_obs, (long long *)nullptr, seq, redo, !redo && flagged);
    if (redo) __syncthreads();  // (the next sequence reuses the selection's LDS)
  }
}

// image_msg of a subset call in the call's order: row i of obs_out / n_out = the observations of sequence seq[i] if it published,
// none otherwise -- the rows that travel back to the host are the call's n, not the context's n_seq. One workgroup per call position.
__global__ __launch_bounds__(256) void gather_obs_subset_kernel(SubsetArgs M, int cap, const VioObs *obs, const int *n_obs, VioObs *obs_out,
                                                                int *n_out) {
  const int i = blockIdx.x, seq = subset_at(M.seq, i);
  const int m = subset_at(M.publish, i) ? min(subset_at(n_obs, seq), cap) : 0;
  if (threadIdx.x == 0) n_out[i] = m;
  for (int k = threadIdx.x; k < m; k += blockDim.x) obs_out[(size_t)i * cap + k] = obs[(size_t)seq * cap + k];
}

// vio_frontend_reset: a fresh FeatureTracker for the listed sequences -- no points, ids from 0 again (n_id, feature_tracker.cpp:311),
// and no overflow stamp, so that a stamp from before the reset can never match a later detection pass.
__global__ void reset_sequences_kernel(const int *seq, int n, int *n_pts, int *n_forw, int *n_id, int *n_pnp, int *n_kept, int *ovf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = seq[i];
  n_pts[s] = 0, n_forw[s] = 0, n_id[s] = 0, n_pnp[s] = 0, n_kept[s] = 0, ovf[s] = 0;
}

}  // namespace
