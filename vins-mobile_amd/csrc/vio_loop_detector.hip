// vio_loop_detector.hip — the loop detector of the app's loop_thread (VINS_ios/ViewController.mm:929-947 ->
// LoopClosure::startLoopClosure -> TemplatedLoopDetector::detectLoop, VINS_ios/loop/TemplatedLoopDetector.h:668-877) for
// the newest keyframe of n independent sessions per call, decision for decision:
//   * transform(features, bowvec, featvec, di_levels)   ThirdParty/DBoW/TemplatedVocabulary.h:1121-1189, :1212-1254
//   * query (max_db_results, max_id = entry - dislocal) BEFORE add   :697-703, TemplatedDatabase.h:603-720, 439-470
//   * ns_factor = L1Scoring::score(bowvec, m_last_bowvec)            ThirdParty/DBoW/ScoringObject.cpp:23-68
//   * removeLowScores :1228-1246, computeIslands :891-965, updateTemporalWindow :982-1017
//   * isGeometricallyConsistent_DI :1056-1144 = getMatches_neighratio :1164-1223 per common node + checkFoundamental
//     :1031-1053 (findFundamentalMat(old, cur, FM_RANSAC, 1.0, 0.99), more than 20 inliers)
//   * eraseIndex :1250-1259 -> TemplatedDatabase::delete_entry (TemplatedDatabase.h:476-499), clear :882-886
// Every session owns one slab of each device array ([session][max_entries * max_keypoints]): the keyframes' keys and
// descriptors (m_image_keys / m_image_descriptors), their FeatureVectors as (node, feature) pairs sorted by node then
// feature (the iteration order of the reference's std::map<NodeId, vector<unsigned>>), their BowVectors (the direct
// file) and the inverted file of vio_bow.hip (postings word << 32 | entry, sorted, two copies). blockIdx.y of every
// kernel is the keyframe of the batch, so the sessions cost one launch, not one each.
// One call is two rounds on the detector's stream:
//   round A  ld_lookup_kernel    the descent of bow_lookup_kernel that also records the direct-index node
//            bow_vector_kernel   (vio_bow_core.h) the BowVector, bit for bit the one of vio_vocabulary_transform
//            ld_store_kernel     keys / descriptors into the slab; (node, feature) pairs sorted in LDS
//            ld_candidates_kernel / ld_score_kernel   queryL1 against entries below max_id (skipped up to dislocal)
//            ld_ns_kernel        score(bowvec, m_last_bowvec), one wave per session, ascending common words
//            ld_insert_kernel / ld_commit_kernel      the add: postings merged, direct file + m_last_bowvec written
//            ld_top_kernel       the best max_db_results candidates in queryL1's order
//   host     per session on those candidates: cut, islands, temporal window (one round trip before, one after)
//   round B  ld_match_kernel     (sessions that reached the geometric check) neighbour-ratio matches per common node,
//                                claims resolved in parallel to the reference's order (proof at the kernel)
//            vio::fundamental_ransac_batch (fe_ransac.h), ld_keep_kernel   the kept pairs, compacted in order
// vio_loop_detector_connect is the step behind a detected loop, KeyFrame::findConnectionWithOldFrame (VINS_ios/loop/keyframe.cpp
// :267-273) for one (current, old) pair of entries per session, read from the slabs above: no descriptor crosses the bus.
//   ld_connect_search_kernel   searchByDes :161-190 (search_by_des_kernel of vio_loop.hip on slab offsets)
//   ld_connect_count_kernel    the pairs whose queries all found a match go to the RANSAC
//   vio::fundamental_ransac_batch, ld_connect_keep_kernel   rejectWithF :35-58 and its reduceVector calls, one download
// vio_loop_detector_keyframes is the loop thread's whole keyframe step (ViewController.mm:913-975): the extraction of
// vio_brief.hip launched through vio_brief_launch.h, its rows packed into in_keys / in_desc on the device
// (vio_brief_pack.hip) where detect has its two uploads, then detect and, for the sessions that detected, connect.
// There is no CPU path: without a device vio_loop_detector_create answers VIO_ENODEV.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "vio_amd.h"
#include "vio_bow_core.h"
#include "vio_brief_launch.h"
#include "vio_camera.h"
#include "vio_device.h"
#include "vio_ransac.h"

namespace {

constexpr int kMaxLdKeys = 4096;  // descriptors per keyframe: the (node, feature) sort and the claim table live in LDS

// what a kernel needs to know about keyframe q of the batch
struct LdItem {
  int session, n_keys, in_off;  // its descriptors in the call's arrays: [in_off, in_off + n_keys)
  int entry, off;               // the entry it becomes; its first feature slot in the session's slab
  int do_query, max_id;         // entry > dislocal: query entries below max_id
  int n_post, cur;              // the session's inverted file: postings, live copy
  int store_last;               // entry + 1 > dislocal (and use_nss): becomes m_last_bowvec
};
struct LdGeom {
  int q, session, old_entry, cur_entry;
};
// the slabs; S sessions, E entries and K keypoints at most, cap = E * K feature slots per session
struct LdStore {
  unsigned long long *desc;  // [S][cap][4]
  float *keys;               // [S][cap][2]
  int *fv_node, *fv_feat;    // [S][cap]  FeatureVector pairs of entry e at [e_off[e], + e_fv[e])
  int *dw;                   // [S][cap]  BowVector of entry e at [e_off[e], + e_bow[e])
  double *dv;
  unsigned long long *inv;   // [2][S][cap]
  int *e_off, *e_fv, *e_bow; // [S][E]
  int *last_w, *last_n;      // [S][K], [S]
  double *last_v;
  size_t cap;
  int S, E, K;
};

// 16 lanes per descriptor as in bow_lookup_kernel (vio_bow.hip), plus transform(feature, id, w, &nid, levelsup)
// :1221-1247: the node chosen at level nid_level (levels count from 1 below the root); the root when nid_level <= 0;
// the leaf where the descent ends above that level
__global__ __launch_bounds__(256) void ld_lookup_kernel(const unsigned long long *node_desc, const double *node_weight, const int *node_word,
                                                         const int *child_off, const int *child, const unsigned long long *desc, int n,
                                                         int depth, int nid_level, int *word, double *weight, int *di_node) {
  const int g = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 4), l = threadIdx.x & 15;
  const bool have = g < n;
  const unsigned long long *f = desc + 4 * (size_t)(have ? g : 0);
  const unsigned long long f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
  int node = 0, nid = nid_level <= 0 ? 0 : -1;
  for (int level = 0; level < depth; level++) {
    const int c0 = child_off[node], nc = child_off[node + 1] - c0;
    if (nc <= 0) break;
    unsigned best = 0xffffffffu;
    for (int c = l; c < nc; c += 16) {
      const unsigned long long *d = node_desc + 4 * (size_t)child[c0 + c];
      const unsigned dist = __popcll(f0 ^ d[0]) + __popcll(f1 ^ d[1]) + __popcll(f2 ^ d[2]) + __popcll(f3 ^ d[3]);
      const unsigned key = (dist << 20) | (unsigned)c;
      best = key < best ? key : best;
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
      const unsigned o = (unsigned)__shfl_xor((int)best, m, 16);
      best = o < best ? o : best;
    }
    node = child[c0 + (int)(best & 0xfffffu)];
    if (level + 1 == nid_level) nid = node;
  }
  if (have && l == 0) word[g] = node_word[node], weight[g] = node_weight[node], di_node[g] = nid < 0 ? node : nid;
}

// one workgroup per keyframe: its keys and descriptors into the session's slab; FeatureVector = (node, feature) of the
// descriptors that are not stopped (w > 0, :1152-1156), bitonic sort of node << 32 | feature in LDS
__global__ __launch_bounds__(256) void ld_store_kernel(const LdItem *items, LdStore st, const float *keys, const unsigned long long *desc,
                                                        const double *weight, const int *di_node) {
  __shared__ unsigned long long key[kMaxLdKeys];
  __shared__ int cnt_s;
  const LdItem it = items[blockIdx.x];
  const int tid = threadIdx.x, nt = blockDim.x, n = it.n_keys;
  const size_t base = (size_t)it.session * st.cap + it.off;
  for (int i = tid; i < 4 * n; i += nt) st.desc[4 * base + i] = desc[4 * (size_t)it.in_off + i];
  for (int i = tid; i < 2 * n; i += nt) st.keys[2 * base + i] = keys[2 * (size_t)it.in_off + i];
  int np2 = nt;
  while (np2 < n) np2 <<= 1;
  for (int i = tid; i < np2; i += nt)
    key[i] = (i < n && weight[it.in_off + i] > 0.0) ? ((unsigned long long)(unsigned)di_node[it.in_off + i] << 32 | (unsigned)i) : ~0ull;
  if (tid == 0) cnt_s = 0;
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < np2; i += nt) {
        const int p = i ^ j;
        if (p > i) {
          const unsigned long long a = key[i], b = key[p];
          if (((i & k) == 0) == (a > b)) key[i] = b, key[p] = a;
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < np2; i += nt) {
    const unsigned long long v = key[i];
    if (v == ~0ull) continue;
    st.fv_node[base + i] = (int)(v >> 32), st.fv_feat[base + i] = (int)(unsigned)v;  // (at most n of them: i < n)
    if (i + 1 == np2 || key[i + 1] == ~0ull) cnt_s = i + 1;
  }
  __syncthreads();
  if (tid == 0) {
    const size_t e = (size_t)it.session * st.E + it.entry;
    st.e_off[e] = it.off, st.e_fv[e] = cnt_s;
  }
}

__device__ __forceinline__ int ld_lower_bound(const int *key, int n, int k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (key[m] < k) lo = m + 1;
    else hi = m;
  }
  return lo;
}
// sum over the lanes that hit, ascending lane = ascending word, added to s in that order
__device__ __forceinline__ double ld_add_in_lane_order(double s, bool hit, double t) {
  unsigned long long m = __ballot(hit);
  while (m) {
    const int l = __builtin_ctzll(m);
    m &= m - 1;
    s += readlane_f64(t, l);
  }
  return s;
}

// bow_candidates_kernel (vio_bow.hip) with the database chosen per keyframe: one wave per query word, lanes over the
// word's run of postings below max_id; flag / cand [n][E] (flag and n_cand zeroed)
__global__ __launch_bounds__(256) void ld_candidates_kernel(const LdItem *items, LdStore st, const int *q_count, const int *q_word, int *flag,
                                                             int *n_cand, int *cand) {
  const int q = blockIdx.y, lane = threadIdx.x & 63;
  const LdItem it = items[q];
  if (!it.do_query) return;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), n_waves = gridDim.x * 4;
  const unsigned long long *key = st.inv + ((size_t)it.cur * st.S + it.session) * st.cap;
  const int ni = q_count[q];
  for (int i = wave; i < ni; i += n_waves) {
    const int w = q_word[(size_t)q * st.K + i];
    const unsigned long long base = (unsigned long long)(unsigned)w << 32, top = base | (unsigned)max(it.max_id, 0);
    const int lo = posting_lower_bound(key, it.n_post, base), hi = posting_lower_bound(key, it.n_post, top);
    for (int p = lo + lane; p < hi; p += 64) {
      const int e = (int)(unsigned)(key[p] & 0xffffffffull);
      if (atomicExch(&flag[(size_t)q * st.E + e], 1) == 0) cand[(size_t)q * st.E + atomicAdd(&n_cand[q], 1)] = e;
    }
  }
}

// bow_score_kernel (vio_bow.hip) per keyframe: wave c scores candidate cand[q][c], the common words in ascending order
__global__ __launch_bounds__(256) void ld_score_kernel(const LdItem *items, LdStore st, const int *q_count, const int *q_word,
                                                        const double *q_value, const int *n_cand, const int *cand, double *cscore) {
  __shared__ int qw_s[kMaxLdKeys];
  const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const LdItem it = items[q];
  const int nc = it.do_query ? n_cand[q] : 0;
  if (nc == 0) return;  // (uniform per workgroup)
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (tid >> 6)), n_waves = gridDim.x * 4;
  const int ni = q_count[q];
  const double *qv = q_value + (size_t)q * st.K;
  for (int i = tid; i < ni; i += 256) qw_s[i] = q_word[(size_t)q * st.K + i];
  __syncthreads();
  const size_t sb = (size_t)it.session * st.cap, eb = (size_t)it.session * st.E;
  for (int c = wave; c < nc; c += n_waves) {
    const int e = cand[(size_t)q * st.E + c];
    const size_t j0 = sb + st.e_off[eb + e];
    const int nw = st.e_bow[eb + e];
    double s = 0.0;
    for (int jb = 0; jb < nw; jb += 64) {
      const int j = jb + lane;
      bool hit = false;
      double t = 0.0;
      if (j < nw) {
        const int b = st.dw[j0 + j];
        const int lo = ld_lower_bound(qw_s, ni, b);
        hit = lo < ni && qw_s[lo] == b;
        if (hit) {
          const double qq = qv[lo], dd = st.dv[j0 + j];
          t = fabs(qq - dd) - fabs(qq) - fabs(dd);
        }
      }
      s = ld_add_in_lane_order(s, hit, t);
    }
    if (lane == 0) cscore[(size_t)q * st.E + c] = s;
  }
}

// the tail of queryL1 (TemplatedDatabase.h:696-719) up to the cut at max_results: candidate c goes to place rank(c) = the
// number of candidates that sort before it by (raw score ascending = best first, entry id ascending: ids are unique, so
// are the ranks) when that is below R; one work-item per candidate, the others staged through LDS 256 at a time.
// n_top [n] (zeroed) counts the candidates, top_id / top_score [n][R].
__global__ __launch_bounds__(256) void ld_top_kernel(const LdItem *items, int E, int R, const int *n_cand, const int *cand, const double *cscore,
                                                      int *n_top, int *top_id, double *top_score) {
  __shared__ double ts[256];
  __shared__ int ti[256];
  const int q = blockIdx.y, tid = threadIdx.x, c = blockIdx.x * 256 + tid;
  const int nc = items[q].do_query ? n_cand[q] : 0;
  if ((int)blockIdx.x * 256 >= nc) return;  // (uniform per workgroup)
  const bool have = c < nc;
  const double s = have ? cscore[(size_t)q * E + c] : 0.0;
  const int id = have ? cand[(size_t)q * E + c] : 0;
  const bool valid = have && s <= 0.0;  // (as vio_bow_database_query: a sum of terms |q - d| - |q| - |d|, none positive)
  int rank = 0;
  for (int j0 = 0; j0 < nc; j0 += 256) {
    __syncthreads();
    if (j0 + tid < nc) ts[tid] = cscore[(size_t)q * E + j0 + tid], ti[tid] = cand[(size_t)q * E + j0 + tid];
    __syncthreads();
    const int nj = min(256, nc - j0);
    if (valid)
      for (int j = 0; j < nj; j++) rank += (ts[j] <= 0.0 && (ts[j] < s || (ts[j] == s && ti[j] < id))) ? 1 : 0;
  }
  if (!valid) return;
  atomicAdd(&n_top[q], 1);
  if (rank < R) top_id[(size_t)q * R + rank] = id, top_score[(size_t)q * R + rank] = s;
}

// L1Scoring::score(bowvec, m_last_bowvec) (ScoringObject.cpp:23-68): one wave per keyframe, lanes over m_last_bowvec
__global__ __launch_bounds__(64) void ld_ns_kernel(const LdItem *items, LdStore st, const int *q_count, const int *q_word, const double *q_value,
                                                    double *ns) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const LdItem it = items[q];
  if (!it.do_query) return;
  const int ni = q_count[q], nl = st.last_n[it.session];
  const int *qw = q_word + (size_t)q * st.K, *lw = st.last_w + (size_t)it.session * st.K;
  const double *qv = q_value + (size_t)q * st.K, *lv = st.last_v + (size_t)it.session * st.K;
  double s = 0.0;
  for (int jb = 0; jb < nl; jb += 64) {
    const int j = jb + lane;
    bool hit = false;
    double t = 0.0;
    if (j < nl) {
      const int b = lw[j];
      const int lo = ld_lower_bound(qw, ni, b);
      hit = lo < ni && qw[lo] == b;
      if (hit) {
        const double vi = qv[lo], wi = lv[j];
        t = fabs(vi - wi) - fabs(vi) - fabs(wi);
      }
    }
    s = ld_add_in_lane_order(s, hit, t);
  }
  if (lane == 0) ns[q] = -s / 2.0;
}

// bow_insert_kernel (vio_bow.hip) per keyframe: the new entry's postings merged into the session's other copy
__global__ __launch_bounds__(256) void ld_insert_kernel(const LdItem *items, LdStore st, const int *q_count, const int *q_word) {
  const int q = blockIdx.y;
  const LdItem it = items[q];
  const int n_new = q_count[q], n_old = it.n_post;
  if (n_new == 0) return;  // (the live copy stays the live copy)
  const unsigned long long *old_key = st.inv + ((size_t)it.cur * st.S + it.session) * st.cap;
  unsigned long long *out = st.inv + ((size_t)(1 - it.cur) * st.S + it.session) * st.cap;
  const int *new_word = q_word + (size_t)q * st.K;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < n_old + n_new; t += gridDim.x * 256) {
    if (t < n_old) {
      const unsigned long long key = old_key[t];
      out[t + ld_lower_bound(new_word, n_new, (int)(key >> 32))] = key;
    } else {
      const int j = t - n_old, w = new_word[j];
      out[posting_lower_bound(old_key, n_old, (unsigned long long)(unsigned)(w + 1) << 32) + j] = (unsigned long long)(unsigned)w << 32 | (unsigned)it.entry;
    }
  }
}

// the entry's BowVector into the direct file; m_last_bowvec = bowvec (:871-874). After ld_ns_kernel on the stream.
__global__ __launch_bounds__(256) void ld_commit_kernel(const LdItem *items, LdStore st, const int *q_count, const int *q_word,
                                                         const double *q_value) {
  const int q = blockIdx.y;
  const LdItem it = items[q];
  const int nw = q_count[q];
  const size_t base = (size_t)it.session * st.cap + it.off;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nw; i += gridDim.x * 256) {
    const int w = q_word[(size_t)q * st.K + i];
    const double v = q_value[(size_t)q * st.K + i];
    st.dw[base + i] = w, st.dv[base + i] = v;
    if (it.store_last) st.last_w[(size_t)it.session * st.K + i] = w, st.last_v[(size_t)it.session * st.K + i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st.e_bow[(size_t)it.session * st.E + it.entry] = nw;
    if (it.store_last) st.last_n[it.session] = nw;
  }
}

// delete_entry (TemplatedDatabase.h:476-499): one compaction pass, the mirror of the insert. A posting (w, e') moves down
// by the number of the erased entry's postings that sort before it: its words below w, and w itself when e < e'.
__global__ __launch_bounds__(256) void ld_erase_kernel(const unsigned long long *old_key, int n_old, const int *word, int n_word, int entry,
                                                        unsigned long long *out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_old) return;
  const unsigned long long key = old_key[t];
  const int w = (int)(key >> 32), e = (int)(unsigned)(key & 0xffffffffull);
  if (e == entry) return;
  const int lo = ld_lower_bound(word, n_word, w);
  out[t - lo - ((lo < n_word && word[lo] == w && entry < e) ? 1 : 0)] = key;
}

// isGeometricallyConsistent_DI :1063-1109 for one (old entry, current entry) pair per workgroup. The FeatureVector pairs of
// the old entry are visited in their order t = 0, 1, ... (node ascending, feature ascending = the reference's outer
// loops); one work-item per old feature scans the current features of the same node in ascending order, so
// `d < best_dist_1` keeps the first of equal distances and best_dist_2 follows the reference's else-branch exactly (the
// lists of a node are short: n_keys / k^(L - di_levels) on average). d1 / d2 in double: 0 / 0 is NaN and fails `<=`, a
// lone candidate gives d / 1e9.
// The claims (:1203-1219), resolved in parallel. Sequentially, t claims its current feature b: the first claimant
// appends the pair (so the pair's place in the list is the rank of that first claimant among all first claimants), and a
// later claimant takes the pair over only on a strictly smaller distance than the holder's (whose distance to b is its
// own d1). Induction over t: the holder is the claimant so far with the smallest (d1, t) in lexicographic order. Hence
//   holder(b) = min over the claimants of d1 << 16 | t        (atomicMin; d1 <= 256, t < 4096)
//   place(b)  = number of first claimants t' < first(b), first(b) = min over the claimants of t   (atomicMin + scan)
// and a current feature is claimed only from its own node, so one table serves all nodes as the reference's per-node
// lists do.
__global__ __launch_bounds__(256) void ld_match_kernel(const LdGeom *geom, LdStore st, double max_ratio, int *n_pairs, float *p_old, float *p_cur) {
  __shared__ int m_b[kMaxLdKeys];
  __shared__ unsigned holder[kMaxLdKeys], first[kMaxLdKeys];
  __shared__ int scan[257];
  const LdGeom g = geom[blockIdx.x];
  const int tid = threadIdx.x;
  const size_t sb = (size_t)g.session * st.cap, eb = (size_t)g.session * st.E;
  const size_t oo = sb + st.e_off[eb + g.old_entry], co = sb + st.e_off[eb + g.cur_entry];
  const int no = st.e_fv[eb + g.old_entry], nc = st.e_fv[eb + g.cur_entry];
  const int *c_node = st.fv_node + co, *c_feat = st.fv_feat + co;
  for (int i = tid; i < kMaxLdKeys; i += 256) holder[i] = 0xffffffffu, first[i] = 0xffffffffu;
  __syncthreads();
  for (int t = tid; t < no; t += 256) {
    const int node = st.fv_node[oo + t];
    const unsigned long long *a = st.desc + 4 * (oo + st.fv_feat[oo + t]);
    const unsigned long long a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
    int best_j = -1;
    double d1 = 1e9, d2 = 1e9;
    for (int j = ld_lower_bound(c_node, nc, node); j < nc && c_node[j] == node; j++) {
      const unsigned long long *b = st.desc + 4 * (co + c_feat[j]);
      const double d = (double)(__popcll(a0 ^ b[0]) + __popcll(a1 ^ b[1]) + __popcll(a2 ^ b[2]) + __popcll(a3 ^ b[3]));
      if (d < d1) best_j = j, d2 = d1, d1 = d;
      else if (d < d2) d2 = d;
    }
    const bool ok = best_j >= 0 && d1 / d2 <= max_ratio;
    const int b = ok ? c_feat[best_j] : -1;
    m_b[t] = b;
    if (ok) atomicMin(&holder[b], (unsigned)d1 << 16 | (unsigned)t), atomicMin(&first[b], (unsigned)t);
  }
  __syncthreads();
  // every work-item owns a contiguous piece of t: first claimants counted, scanned, then written at their places
  const int chunk = (no + 255) / 256, t0 = min(tid * chunk, no), t1 = min(t0 + chunk, no);
  int cnt = 0;
  for (int t = t0; t < t1; t++) cnt += m_b[t] >= 0 && first[m_b[t]] == (unsigned)t;
  scan[tid + 1] = cnt;
  if (tid == 0) scan[0] = 0;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = tid + 1 > o ? scan[tid + 1 - o] : 0;
    __syncthreads();
    scan[tid + 1] += v;
    __syncthreads();
  }
  float *po = p_old + 2 * (size_t)blockIdx.x * st.K, *pc = p_cur + 2 * (size_t)blockIdx.x * st.K;
  int p = scan[tid];
  for (int t = t0; t < t1; t++) {
    const int b = m_b[t];
    if (b < 0 || first[b] != (unsigned)t) continue;
    const int a = st.fv_feat[oo + (holder[b] & 0xffffu)];
    po[2 * p] = st.keys[2 * (oo + a)], po[2 * p + 1] = st.keys[2 * (oo + a) + 1];
    pc[2 * p] = st.keys[2 * (co + b)], pc[2 * p + 1] = st.keys[2 * (co + b) + 1];
    p++;
  }
  if (tid == 0) n_pairs[blockIdx.x] = scan[256];
}

// reduceInputToOutput :1021-1028 for both lists: one wave per pair of keyframes, the kept pairs in their order
__global__ __launch_bounds__(64) void ld_keep_kernel(const int *n_pairs, int min_count, const unsigned char *mask, int K, float *p_old, float *p_cur,
                                                      float *k_old, float *k_cur, int *n_kept) {
  const int g = blockIdx.x, lane = threadIdx.x, n = n_pairs[g];
  int cnt = 0;
  if (n >= min_count)
    for (int b = 0; b < n; b += 64) {
      const int i = b + lane;
      const bool keep = i < n && mask[(size_t)g * K + i] != 0;
      const unsigned long long m = __ballot(keep);
      if (keep) {
        const size_t o = 2 * ((size_t)g * K + cnt + __popcll(m & ((1ull << lane) - 1))), s = 2 * ((size_t)g * K + i);
        k_old[o] = p_old[s], k_old[o + 1] = p_old[s + 1], k_cur[o] = p_cur[s], k_cur[o + 1] = p_cur[s + 1];
      }
      cnt += __popcll(m);
    }
  if (lane == 0) n_kept[g] = cnt;
}

// ---- findConnectionWithOldFrame on the slabs ---------------------------------------------------------------------------
constexpr int kCnWaves = 4;    // queries per workgroup, one wave each
constexpr int kCnStage = 512;  // old descriptors staged per round: 16 KB of LDS (kStage of vio_loop.hip)

struct LdPair {
  int session, n_window, n_old;
  int cur_off, old_off;  // slab slots of the first window descriptor of the current entry / the first one of the old entry
};

// search_by_des_kernel (vio_loop.hip) on the slabs: grid (ceil(stride / 4), n pairs), one wave per window descriptor, the
// old entry's descriptors staged through LDS once per workgroup. key = distance << 16 | index: the minimum is the smallest
// distance and, among equals, the first index. Rows of `stride` (the call's largest n_window) per pair: p_cur = the window
// keys (the measurements), p_old = the key of the best old descriptor, unmatched = nothing closer than 256 bits.
__global__ __launch_bounds__(64 * kCnWaves) void ld_connect_search_kernel(const LdPair *pairs, LdStore st, int stride, float *p_cur, float *p_old,
                                                                           int *unmatched) {
  __shared__ unsigned long long stage[kCnStage][4];
  const LdPair pr = pairs[blockIdx.y];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nc = pr.n_window, no = pr.n_old;
  if ((int)blockIdx.x * kCnWaves >= nc) return;  // (uniform per workgroup)
  const int q = blockIdx.x * kCnWaves + wave;
  const bool have = q < nc;
  const size_t sb = (size_t)pr.session * st.cap;
  unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  if (have) {
    const unsigned long long *c = st.desc + 4 * (sb + pr.cur_off + q);
    a0 = c[0], a1 = c[1], a2 = c[2], a3 = c[3];
  }
  unsigned best = 256u << 16;  // bestDist = 256, bestIndex = -1 (keyframe.cpp:169-170)
  const unsigned long long *ob = st.desc + 4 * (sb + pr.old_off);
  for (int j0 = 0; j0 < no; j0 += kCnStage) {
    const int nj = min(kCnStage, no - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < nj * 4; e += blockDim.x) (&stage[0][0])[e] = ob[4 * (size_t)j0 + e];
    __syncthreads();
    if (have)
      for (int j = lane; j < nj; j += 64) {
        const unsigned d = __popcll(a0 ^ stage[j][0]) + __popcll(a1 ^ stage[j][1]) + __popcll(a2 ^ stage[j][2]) + __popcll(a3 ^ stage[j][3]);
        const unsigned key = (d << 16) | (unsigned)(j0 + j);
        best = key < best ? key : best;
      }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = __shfl_xor(best, o, 64);
    best = t < best ? t : best;
  }
  if (have && lane == 0) {
    const bool hit = (best >> 16) < 256u;  // `if (bestDist < 256)` (:182)
    const size_t o = (size_t)blockIdx.y * stride + q, ck = sb + pr.cur_off + q, ok = sb + pr.old_off + (hit ? (best & 0xffffu) : 0u);
    p_cur[2 * o] = st.keys[2 * ck], p_cur[2 * o + 1] = st.keys[2 * ck + 1];
    p_old[2 * o] = hit ? st.keys[2 * ok] : 0.f, p_old[2 * o + 1] = hit ? st.keys[2 * ok + 1] : 0.f;
    unmatched[o] = hit ? 0 : 1;
  }
}

// one wave per pair: count = n_window when every query found a match, else 0 (the reference's arrays go out of step there:
// "no connection", as vio_loop_find_connection restates it). The RANSAC runs on the pairs with count >= 8.
__global__ __launch_bounds__(64) void ld_connect_count_kernel(const LdPair *pairs, int stride, const int *unmatched, int *count) {
  const int p = blockIdx.x, lane = threadIdx.x, n = pairs[p].n_window;
  bool any = false;
  for (int i = lane; i < n; i += 64) any = any || unmatched[(size_t)p * stride + i] != 0;
  if (__ballot(any) != 0ull) any = true;
  if (lane == 0) count[p] = any ? 0 : n;
}

// rejectWithF :35-58 behind the RANSAC, one wave per pair: status, and the reduceVector calls as one ballot compaction in
// window order. The batch RANSAC leaves the mask of a problem below 8 pairs unwritten: fewer than 8 keep everything (and
// have no normalised points, measurements_old_norm stays empty), an unmatched query keeps nothing.
// hdr [n][2] = n_kept, ransac_ran. intr [sessions][4] = cx cy fx fy of every session's camera, in float.
__global__ __launch_bounds__(64) void ld_connect_keep_kernel(const LdPair *pairs, int stride, const int *count, const unsigned char *mask,
                                                              const float *p_old, const int *ids, const float *intr,
                                                              unsigned char *status, int *kept_index, int *kept_ids, double *kept_norm, int *hdr) {
  const int p = blockIdx.x, lane = threadIdx.x, n = pairs[p].n_window;
  const float *in = intr + 4 * (size_t)pairs[p].session;  // (uniform)
  const float cx = in[0], cy = in[1], fx = in[2], fy = in[3];
  const size_t o = (size_t)p * stride;
  const bool matched = count[p] == n, ran = matched && n >= 8;
  int cnt = 0;
  for (int b = 0; b < n; b += 64) {
    const int i = b + lane;
    const bool keep = i < n && matched && (!ran || mask[o + i] != 0);
    if (i < n) status[o + i] = keep ? 1 : 0;
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const size_t k = o + cnt + __popcll(m & ((1ull << lane) - 1));
      kept_index[k] = i;
      if (ids) kept_ids[k] = ids[o + i];
      if (ran) {  // (pt - (cx, cy)) / (fx, fy) in float (:45-46), widened
        kept_norm[2 * k] = (double)((p_old[2 * (o + i)] - cx) / fx);
        kept_norm[2 * k + 1] = (double)((p_old[2 * (o + i) + 1] - cy) / fy);
      }
    }
    cnt += __popcll(m);
  }
  if (lane == 0) hdr[2 * p] = cnt, hdr[2 * p + 1] = ran ? 1 : 0;
}

struct Island {  // tIsland
  int first, last, best_entry;
  double score, best_score;
};

}  // namespace

using vio::DevBuf;

struct vio_loop_detector {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool timed_a = false, timed_b = false;
  VioLoopDetectorParams P;
  int S = 0, E = 0, K = 0, R = 0, height = 0, nid_level = 0, accumulate = 0;
  size_t cap = 0;
  // the vocabulary's tree (copied at create)
  DevBuf<unsigned long long> v_desc;
  DevBuf<double> v_weight, v_wweight;
  DevBuf<int> v_word, v_child_off, v_child;
  // the slabs
  DevBuf<unsigned long long> desc, inv;
  DevBuf<float> keys;
  DevBuf<int> fv_node, fv_feat, dw, e_off, e_fv, e_bow, last_w, last_n;
  DevBuf<double> dv, last_v;
  // per call
  DevBuf<LdItem> items;
  DevBuf<LdGeom> geom;
  DevBuf<unsigned long long> in_desc;
  DevBuf<float> in_keys, p_old, p_cur, k_old, k_cur;
  DevBuf<int> t_word, t_node, t_off, q_count, q_word, flag, n_cand, cand, n_top, top_id, n_pairs, n_kept;
  DevBuf<double> t_weight, q_value, cscore, top_score, ns;
  DevBuf<unsigned char> mask;
  // vio_loop_detector_connect (sized by S * K at its first call): the pairs, the callers' ids, the unmatched flags, and the
  // sections of one download (kept_old_norm | matched old points | kept_index | kept_ids | hdr | status)
  DevBuf<LdPair> cn_pairs;
  DevBuf<int> cn_ids, cn_unmatched;
  // the camera of every session (vio_loop_detector_set_cameras), and what a call's connect kernel reads: cx cy fx fy in
  // float per session, a session's own camera or the call's cfg
  std::vector<VioCamera> cam;
  std::vector<char> has_cam;
  DevBuf<float> cn_intr;
  vio::PinnedBuf<float> cn_hintr;
  DevBuf<unsigned char> cn_out;
  vio::PinnedBuf<unsigned char> cn_host;  // (page-locked: the one download of a call)
  std::vector<LdPair> cn_hpairs;
  std::vector<char> cn_seen;
  std::vector<int> cn_hids;  // the ids of the pairs of a call whose rows do not lie behind each other (the keyframe step)
  // vio_loop_detector_keyframes: n_fast | n_keypoints of the call's extraction (page-locked, sized at its first call)
  vio::PinnedBuf<int> kf_counts;
  // host mirror of every session
  struct Session {
    int n_entries = 0, n_post = 0, cur = 0;
    std::vector<int> off, bow;  // [E + 1] feature slots, [E] BowVector sizes (0 once erased)
    std::vector<char> erased;   // [E] vio_loop_detector_erase named the entry (an empty keyframe has bow == 0 as well)
    int win_n = 0, win_first = 0, win_last = 0, win_query = 0;  // m_window
  };
  std::vector<Session> sess;
  LdStore store() const {
    LdStore s;
    s.desc = desc.p, s.keys = keys.p, s.fv_node = fv_node.p, s.fv_feat = fv_feat.p, s.dw = dw.p, s.dv = dv.p, s.inv = inv.p;
    s.e_off = e_off.p, s.e_fv = e_fv.p, s.e_bow = e_bow.p, s.last_w = last_w.p, s.last_n = last_n.p, s.last_v = last_v.p;
    s.cap = cap, s.S = S, s.E = E, s.K = K;
    return s;
  }
  ~vio_loop_detector() {
    if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

// computeIslands :891-965 on the results that survived the cut (q in descending score order)
void compute_islands(const VioLoopDetectorParams &P, std::vector<std::pair<int, double>> &q, std::vector<Island> &islands) {
  islands.clear();
  if (q.size() == 1) {
    islands.push_back(Island{q[0].first, q[0].first, q[0].first, q[0].second, q[0].second});
    return;
  }
  if (q.empty()) return;
  std::sort(q.begin(), q.end(), [](const std::pair<int, double> &a, const std::pair<int, double> &b) { return a.first < b.first; });  // (ids are unique)
  int first = q[0].first, last = q[0].first, best_entry = q[0].first;
  size_t i_first = 0, i_last = 0;
  double best_score = q[0].second;
  auto close_island = [&]() {
    if (last - first + 1 >= P.min_matches_per_group) {
      double sum = 0;
      for (size_t i = i_first; i <= i_last; i++) sum += q[i].second;  // calculateIslandScore :970-977
      islands.push_back(Island{first, last, best_entry, sum, best_score});
    }
  };
  for (size_t idx = 1; idx < q.size(); idx++) {
    if (q[idx].first - last < P.max_intragroup_gap) {
      last = q[idx].first, i_last = idx;
      if (q[idx].second > best_score) best_score = q[idx].second, best_entry = q[idx].first;
    } else {
      close_island();
      first = last = q[idx].first, i_first = i_last = idx, best_score = q[idx].second, best_entry = q[idx].first;
    }
  }
  close_island();
}

// what vio_loop_detector_detect refuses about its sessions, on the host mirror: a session out of range or twice
// (VIO_EINVAL), a session that already holds max_entries (VIO_ECAP)
int check_sessions(const vio_loop_detector *d, int n, const int32_t *session) {
  if (n > d->S) return VIO_EINVAL;  // (some session would be named twice)
  std::vector<char> seen(d->S, 0);
  for (int q = 0; q < n; q++) {
    if (session[q] < 0 || session[q] >= d->S || seen[session[q]]) return VIO_EINVAL;
    seen[session[q]] = 1;
  }
  for (int q = 0; q < n; q++)
    if (d->sess[session[q]].n_entries >= d->E) return VIO_ECAP;
  return VIO_OK;
}

}  // namespace

extern "C" {

void vio_loop_detector_params_default(VioLoopDetectorParams *p, float f) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->use_nss = 1, p->alpha = 0.3f, p->k = 1, p->geom_check = 1, p->di_levels = 2;  // Parameters(height, width) :165-167
  p->dislocal = (int)(20 * f), p->max_db_results = (int)(50 * f), p->min_nss_factor = (float)0.005;  // set(f) :525-541
  p->min_matches_per_group = (int)f, p->max_intragroup_gap = (int)(3 * f), p->max_distance_between_groups = (int)(3 * f);
  p->max_distance_between_queries = (int)(2 * f);
  p->min_Fpoints = 12, p->max_neighbor_ratio = 0.6;
  p->f_threshold = 1.0, p->f_confidence = 0.99, p->min_inliers = 20;  // checkFoundamental :1036-1047
}

int vio_loop_detector_create(vio_vocabulary_t *v, const VioLoopDetectorParams *p, int32_t n_sessions, int32_t max_entries,
                             int32_t max_keypoints, vio_loop_detector_t **out) {
  if (!p || !out || n_sessions < 1 || max_entries < 1 || max_keypoints < 1) return VIO_EINVAL;
  if (!vio::device_ready("the loop detector")) return VIO_ENODEV;
  if (!v) return VIO_EINVAL;  // (after the device: no vocabulary exists without one, and the answer is then "no device")
  if (n_sessions > 65535) return VIO_ECAP;  // (grid.y: one block row per keyframe of a call)
  if (max_keypoints > kMaxLdKeys) return VIO_ECAP;
  if ((long long)max_entries * max_keypoints > 0x7fffffffll) return VIO_ECAP;
  if (p->geom_check != 1 && p->geom_check != 3) return VIO_EINVAL;  // GEOM_EXHAUSTIVE / GEOM_FLANN: the app never selects them
  if (v->scoring != 0 || p->di_levels < 0 || p->di_levels > v->L) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(v);
  vio_loop_detector *d = new (std::nothrow) vio_loop_detector();
  if (!d) return VIO_ENOMEM;
  d->device = v->device, d->P = *p, d->S = n_sessions, d->E = max_entries, d->K = max_keypoints;
  d->cap = (size_t)max_entries * max_keypoints;
  d->R = p->max_db_results > 0 ? std::min(p->max_db_results, max_entries) : max_entries;  // query results kept per keyframe
  d->height = v->height, d->nid_level = v->L - p->di_levels, d->accumulate = v->weighting == 0 || v->weighting == 1;
  try {
    d->sess.resize(n_sessions);
    d->cam.resize(n_sessions), d->has_cam.assign(n_sessions, 0);
    for (auto &s : d->sess) s.off.assign((size_t)max_entries + 1, 0), s.bow.assign(max_entries, 0), s.erased.assign(max_entries, 0);
  } catch (const std::bad_alloc &) {
    delete d;
    return VIO_ENOMEM;
  }
  bool ok = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) == hipSuccess;
  for (int i = 0; i < 4 && ok; i++) ok = hipEventCreate(&d->ev[i]) == hipSuccess;
  if (!ok) {
    delete d;
    return VIO_ENODEV;
  }
  const size_t N = (size_t)v->n_nodes, S = n_sessions, E = max_entries, K = max_keypoints, SK = S * K, SE = S * E, SC = S * d->cap;
  int rc = VIO_OK;
  auto need = [&rc](int r) { rc = rc == VIO_OK ? r : rc; };
  need(d->v_desc.ensure(4 * N)), need(d->v_weight.ensure(N)), need(d->v_word.ensure(N)), need(d->v_child_off.ensure(N + 1));
  need(d->v_child.ensure(N)), need(d->v_wweight.ensure(v->n_words));
  need(d->desc.ensure(4 * SC)), need(d->keys.ensure(2 * SC)), need(d->inv.ensure(2 * SC)), need(d->fv_node.ensure(SC)), need(d->fv_feat.ensure(SC));
  need(d->dw.ensure(SC)), need(d->dv.ensure(SC)), need(d->e_off.ensure(SE)), need(d->e_fv.ensure(SE)), need(d->e_bow.ensure(SE));
  need(d->last_w.ensure(SK)), need(d->last_v.ensure(SK)), need(d->last_n.ensure(S));
  need(d->items.ensure(S)), need(d->geom.ensure(S)), need(d->in_desc.ensure(4 * SK)), need(d->in_keys.ensure(2 * SK));
  need(d->p_old.ensure(2 * SK)), need(d->p_cur.ensure(2 * SK)), need(d->k_old.ensure(2 * SK)), need(d->k_cur.ensure(2 * SK)), need(d->mask.ensure(SK));
  need(d->t_word.ensure(SK)), need(d->t_node.ensure(SK)), need(d->t_weight.ensure(SK)), need(d->t_off.ensure(S + 1));
  need(d->q_count.ensure(S)), need(d->q_word.ensure(SK)), need(d->q_value.ensure(SK)), need(d->ns.ensure(S));
  need(d->flag.ensure(SE)), need(d->n_cand.ensure(S)), need(d->cand.ensure(SE)), need(d->cscore.ensure(SE));
  need(d->n_top.ensure(S)), need(d->top_id.ensure(S * d->R)), need(d->top_score.ensure(S * d->R));
  need(d->n_pairs.ensure(S)), need(d->n_kept.ensure(S));
  if (rc != VIO_OK) {
    delete d;
    return rc;
  }
  hipStream_t st = d->stream;
  if (hipMemcpyAsync(d->v_desc.p, v->d_desc.p, 32 * N, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d->v_weight.p, v->d_weight.p, 8 * N, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d->v_word.p, v->d_word.p, 4 * N, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d->v_child_off.p, v->d_child_off.p, 4 * (N + 1), hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d->v_child.p, v->d_child.p, 4 * (N - 1), hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d->v_wweight.p, v->d_wweight.p, 8 * (size_t)v->n_words, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemsetAsync(d->last_n.p, 0, 4 * S, st) != hipSuccess || hipMemsetAsync(d->e_fv.p, 0, 4 * SE, st) != hipSuccess ||
      hipMemsetAsync(d->e_bow.p, 0, 4 * SE, st) != hipSuccess || hipMemsetAsync(d->e_off.p, 0, 4 * SE, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    delete d;
    return VIO_ENODEV;
  }
  *out = d;
  return VIO_OK;
}

void vio_loop_detector_destroy(vio_loop_detector_t *d) {
  if (!d) return;
  vio::DeviceScope scope(d->device);
  delete d;
}

int vio_loop_detector_get_device(const vio_loop_detector_t *d, int32_t *device) {
  if (!d || !device) return VIO_EINVAL;
  *device = d->device;
  return VIO_OK;
}

int vio_loop_detector_size(const vio_loop_detector_t *d, int32_t session, int32_t *n_entries) {
  if (!d || !n_entries || session < 0 || session >= d->S) return VIO_EINVAL;
  *n_entries = d->sess[session].n_entries;
  return VIO_OK;
}

int vio_loop_detector_clear(vio_loop_detector_t *d, int32_t session) {
  if (!d || session < 0 || session >= d->S) return VIO_EINVAL;
  vio_loop_detector::Session &s = d->sess[session];
  s.n_entries = 0, s.n_post = 0, s.win_n = 0;  // m_database->clear(); m_window.nentries = 0 (m_last_bowvec stays, as there:
  return VIO_OK;                                // it is stored again before entry dislocal + 1 reads it)
}

int vio_loop_detector_kernel_ms(vio_loop_detector_t *d, float *ms) {
  if (!d || !ms) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(d);
  float a = 0, b = 0;
  if (d->timed_a) HIP_OK(hipEventElapsedTime(&a, d->ev[0], d->ev[1]));
  if (d->timed_b) HIP_OK(hipEventElapsedTime(&b, d->ev[2], d->ev[3]));
  *ms = a + b;
  return VIO_OK;
}

int vio_loop_detector_erase(vio_loop_detector_t *d, int32_t session, int32_t n, const int32_t *entries) {
  if (!d || session < 0 || session >= d->S || n < 0 || (n > 0 && !entries)) return VIO_EINVAL;
  vio_loop_detector::Session &s = d->sess[session];
  for (int i = 0; i < n; i++)
    if (entries[i] < 0 || entries[i] >= s.n_entries) return VIO_EINVAL;
  VIO_ON_DEVICE_OF(d);
  hipStream_t st = d->stream;
  const size_t sb = (size_t)session * d->cap, eb = (size_t)session * d->E;
  for (int i = 0; i < n; i++) {
    const int e = entries[i], nw = s.bow[e];
    if (nw > 0) {
      hipLaunchKernelGGL(ld_erase_kernel, dim3((s.n_post + 255) / 256), dim3(256), 0, st, d->inv.p + ((size_t)s.cur * d->S + session) * d->cap,
                         s.n_post, d->dw.p + sb + s.off[e], nw, e, d->inv.p + ((size_t)(1 - s.cur) * d->S + session) * d->cap);
      HIP_OK(hipGetLastError());
      s.cur = 1 - s.cur, s.n_post -= nw, s.bow[e] = 0;
    }
    s.erased[e] = 1;
    HIP_OK(hipMemsetAsync(d->e_bow.p + eb + e, 0, 4, st));  // m_dBowfile[entry].clear(); m_dfile[entry].clear()
    HIP_OK(hipMemsetAsync(d->e_fv.p + eb + e, 0, 4, st));
  }
  HIP_OK(hipStreamSynchronize(st));
  return VIO_OK;
}

}  // extern "C"

namespace {

// vio_loop_detector_detect. from_device: the keyframes are the rows of an extraction that has been launched (its counts
// are n_keys); they are packed into in_keys / in_desc on the device behind its `done` event, keys / desc are not read.
int detect_run(vio_loop_detector *d, int32_t n, const int32_t *session, const int32_t *n_keys, const float *keys, const uint64_t *desc,
               const vio::BriefResult *from_device, VioLoopDetection *out, float *cur_pts, float *old_pts, int32_t pts_stride) {
  if (!d || n < 1 || !session || !n_keys || !out) return VIO_EINVAL;
  if ((cur_pts || old_pts) && pts_stride < d->K) return VIO_EINVAL;
  if (n > d->S) return VIO_EINVAL;  // (some session would be named twice)
  const VioLoopDetectorParams &P = d->P;
  const int E = d->E, K = d->K, R = d->R;
  try {
    std::vector<LdItem> items(n);
    std::vector<int> off(n + 1, 0);
    std::vector<char> seen(d->S, 0);
    for (int q = 0; q < n; q++) {
      if (session[q] < 0 || session[q] >= d->S || seen[session[q]] || n_keys[q] < 0) return VIO_EINVAL;
      seen[session[q]] = 1;
    }
    int max_post = 0;
    bool any_query = false;
    for (int q = 0; q < n; q++) {
      const vio_loop_detector::Session &s = d->sess[session[q]];
      if (n_keys[q] > K || s.n_entries >= E) return VIO_ECAP;
      LdItem &it = items[q];
      it.session = session[q], it.n_keys = n_keys[q], it.in_off = off[q], it.entry = s.n_entries, it.off = s.off[s.n_entries];
      it.do_query = it.entry > P.dislocal, it.max_id = it.entry - P.dislocal;  // :687, :697
      it.n_post = s.n_post, it.cur = s.cur, it.store_last = P.use_nss && it.entry + 1 > P.dislocal;
      off[q + 1] = off[q] + n_keys[q];
      max_post = std::max(max_post, s.n_post), any_query = any_query || it.do_query;
    }
    const int total = off[n];
    if (total > 0 && !from_device && (!keys || !desc)) return VIO_EINVAL;
    VIO_ON_DEVICE_OF(d);
    hipStream_t st = d->stream;
    const LdStore S = d->store();
    d->timed_a = d->timed_b = false;
    // ---- round A: transform, query, ns_factor, add
    HIP_OK(hipMemcpyAsync(d->items.p, items.data(), sizeof(LdItem) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d->t_off.p, off.data(), 4 * (size_t)(n + 1), hipMemcpyHostToDevice, st));
    if (total > 0 && from_device) {  // the extractor's stream is ordered before this one by its event, not by the host
      HIP_OK(hipStreamWaitEvent(st, from_device->done, 0));
      HIP_OK(vio::launch_brief_pack(*from_device, n, d->t_off.p, d->in_keys.p, d->in_desc.p, st));
    } else if (total > 0) {
      HIP_OK(hipMemcpyAsync(d->in_desc.p, desc, 32 * (size_t)total, hipMemcpyHostToDevice, st));
      HIP_OK(hipMemcpyAsync(d->in_keys.p, keys, 8 * (size_t)total, hipMemcpyHostToDevice, st));
    }
    HIP_OK(hipEventRecord(d->ev[0], st));
    if (total > 0)
      hipLaunchKernelGGL(ld_lookup_kernel, dim3((unsigned)(((size_t)total * 16 + 255) / 256)), dim3(256), 0, st, d->v_desc.p, d->v_weight.p,
                         d->v_word.p, d->v_child_off.p, d->v_child.p, d->in_desc.p, total, d->height + 1, d->nid_level, d->t_word.p,
                         d->t_weight.p, d->t_node.p);
    hipLaunchKernelGGL(bow_vector_kernel, dim3(n), dim3(256), 0, st, d->t_off.p, d->t_word.p, d->t_weight.p, d->v_wweight.p, d->accumulate,
                       d->q_count.p, d->q_word.p, d->q_value.p, K);
    hipLaunchKernelGGL(ld_store_kernel, dim3(n), dim3(256), 0, st, d->items.p, S, d->in_keys.p, d->in_desc.p, d->t_weight.p, d->t_node.p);
    if (any_query) {
      HIP_OK(hipMemsetAsync(d->flag.p, 0, 4 * (size_t)n * E, st));
      HIP_OK(hipMemsetAsync(d->n_cand.p, 0, 4 * (size_t)n, st));
      HIP_OK(hipMemsetAsync(d->n_top.p, 0, 4 * (size_t)n, st));
      hipLaunchKernelGGL(ld_candidates_kernel, dim3(std::min((K + 3) / 4, 256), n), dim3(256), 0, st, d->items.p, S, d->q_count.p, d->q_word.p,
                         d->flag.p, d->n_cand.p, d->cand.p);
      hipLaunchKernelGGL(ld_score_kernel, dim3(std::min((E + 3) / 4, 64), n), dim3(256), 0, st, d->items.p, S, d->q_count.p, d->q_word.p,
                         d->q_value.p, d->n_cand.p, d->cand.p, d->cscore.p);
      hipLaunchKernelGGL(ld_top_kernel, dim3((E + 255) / 256, n), dim3(256), 0, st, d->items.p, E, R, d->n_cand.p, d->cand.p, d->cscore.p,
                         d->n_top.p, d->top_id.p, d->top_score.p);
      if (P.use_nss)
        hipLaunchKernelGGL(ld_ns_kernel, dim3(n), dim3(64), 0, st, d->items.p, S, d->q_count.p, d->q_word.p, d->q_value.p, d->ns.p);
    }
    hipLaunchKernelGGL(ld_insert_kernel, dim3(std::min((max_post + K + 255) / 256, 1024), n), dim3(256), 0, st, d->items.p, S, d->q_count.p,
                       d->q_word.p);
    hipLaunchKernelGGL(ld_commit_kernel, dim3((K + 255) / 256, n), dim3(256), 0, st, d->items.p, S, d->q_count.p, d->q_word.p, d->q_value.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(d->ev[1], st));
    std::vector<int> h_count(n, 0), nc(n, 0), h_id;
    std::vector<double> h_ns(n, 1.0), h_score;
    HIP_OK(hipMemcpyAsync(h_count.data(), d->q_count.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    if (any_query) {  // at most R results per keyframe come back, in the same trip as the counts
      h_id.resize((size_t)n * R), h_score.resize((size_t)n * R);
      HIP_OK(hipMemcpyAsync(nc.data(), d->n_top.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(h_id.data(), d->top_id.p, 4 * (size_t)n * R, hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(h_score.data(), d->top_score.p, 8 * (size_t)n * R, hipMemcpyDeviceToHost, st));
      if (P.use_nss) HIP_OK(hipMemcpyAsync(h_ns.data(), d->ns.p, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    d->timed_a = true;
    // the add has happened on the device: the host mirror follows
    for (int q = 0; q < n; q++) {
      vio_loop_detector::Session &s = d->sess[session[q]];
      s.off[s.n_entries + 1] = s.off[s.n_entries] + n_keys[q], s.bow[s.n_entries] = h_count[q], s.erased[s.n_entries] = 0;
      if (h_count[q] > 0) s.cur = 1 - s.cur, s.n_post += h_count[q];
      s.n_entries++;
    }
    // ---- the scalar chain per session (:705-853) up to the geometric check
    std::vector<LdGeom> geom;
    std::vector<std::pair<int, double>> qr;
    std::vector<Island> islands;
    for (int q = 0; q < n; q++) {
      vio_loop_detector::Session &s = d->sess[session[q]];
      VioLoopDetection &r = out[q];
      memset(&r, 0, sizeof(r));
      r.query = items[q].entry, r.match = -1, r.ns_factor = 1.0;
      r.island_first = r.island_last = r.island_best_entry = -1;
      r.consistent_entries = s.win_n;
      if (!items[q].do_query) {
        r.status = VIO_LOOP_CLOSE_MATCHES_ONLY;
        continue;
      }
      r.n_results = std::min(nc[q], R);  // (ld_top_kernel: best first, equal scores in ascending entry id)
      if (r.n_results == 0) {
        r.status = VIO_LOOP_NO_DB_RESULTS;
        continue;
      }
      if (P.use_nss) r.ns_factor = h_ns[q];
      if (P.use_nss && !(r.ns_factor >= (double)P.min_nss_factor)) {
        r.status = VIO_LOOP_LOW_NSS_FACTOR;
        continue;
      }
      const double threshold = (double)P.alpha * r.ns_factor;  // removeLowScores(qret, m_params.alpha * ns_factor): float * double
      qr.clear();
      for (int i = 0; i < r.n_results; i++) {
        const double score = -h_score[(size_t)q * R + i] / 2.0;  // the scaling to [0, 1] of queryL1 (:716-718)
        if (!(score >= threshold)) break;  // descending scores: lower_bound with Result::geq
        qr.push_back(std::make_pair(h_id[(size_t)q * R + i], score));
      }
      r.n_after_cut = (int)qr.size();
      if (qr.empty()) {
        r.status = VIO_LOOP_LOW_SCORES;
        continue;
      }
      r.match = qr[0].first;
      compute_islands(P, qr, islands);
      if (islands.empty()) {
        r.status = VIO_LOOP_NO_GROUPS;
        continue;
      }
      const Island *best = &islands[0];  // std::max_element with tIsland::operator< on the score: the first of the largest
      for (const Island &i : islands)
        if (best->score < i.score) best = &i;
      // updateTemporalWindow :982-1017
      if (s.win_n == 0 || r.query - s.win_query > P.max_distance_between_queries) {
        s.win_n = 1;
      } else {
        const int a1 = s.win_first, a2 = s.win_last, b1 = best->first, b2 = best->last;
        bool fit = (b1 <= a1 && a1 <= b2) || (a1 <= b1 && b1 <= a2);
        if (!fit) fit = std::max(a1 - b2, b1 - a2) <= P.max_distance_between_groups;
        s.win_n = fit ? s.win_n + 1 : 1;
      }
      s.win_first = best->first, s.win_last = best->last, s.win_query = r.query;
      r.island_first = best->first, r.island_last = best->last, r.island_best_entry = best->best_entry;
      r.island_score = best->score, r.island_best_score = best->best_score;
      r.consistent_entries = s.win_n;
      r.match = best->best_entry;
      if (s.win_n > P.k) {
        if (P.geom_check == 1) {
          r.status = VIO_LOOP_NO_GEOMETRICAL_CONSISTENCY;  // until round B says otherwise
          geom.push_back(LdGeom{q, session[q], best->best_entry, r.query});
        } else {
          r.status = VIO_LOOP_DETECTED;  // GEOM_NONE
        }
      } else {
        r.status = VIO_LOOP_NO_TEMPORAL_CONSISTENCY;
      }
    }
    // ---- round B: the geometric check of the sessions that reached it
    const int ng = (int)geom.size();
    if (ng > 0) {
      const int min_count = std::max(P.min_Fpoints, 8);  // :1112 and checkFoundamental's `size() >= 8`
      HIP_OK(hipMemcpyAsync(d->geom.p, geom.data(), sizeof(LdGeom) * (size_t)ng, hipMemcpyHostToDevice, st));
      HIP_OK(hipEventRecord(d->ev[2], st));
      hipLaunchKernelGGL(ld_match_kernel, dim3(ng), dim3(256), 0, st, d->geom.p, S, P.max_neighbor_ratio, d->n_pairs.p, d->p_old.p, d->p_cur.p);
      HIP_OK(hipGetLastError());
      int rc = vio::fundamental_ransac_batch(st, d->p_old.p, d->p_cur.p, d->n_pairs.p, ng, K, min_count, (float)P.f_threshold, P.f_confidence,
                                             d->mask.p);  // findFundamentalMat(old, cur, ...)
      if (rc != VIO_OK) return rc;
      hipLaunchKernelGGL(ld_keep_kernel, dim3(ng), dim3(64), 0, st, d->n_pairs.p, min_count, d->mask.p, K, d->p_old.p, d->p_cur.p, d->k_old.p,
                         d->k_cur.p, d->n_kept.p);
      HIP_OK(hipGetLastError());
      HIP_OK(hipEventRecord(d->ev[3], st));
      // the kept pairs come back in the same trip as their counts: rows as wide as the largest keyframe that was checked
      int widest = 1;
      for (const LdGeom &g : geom) widest = std::max(widest, (int)n_keys[g.q]);
      std::vector<int> h_pairs(ng), h_kept(ng);
      std::vector<float> h_cur, h_old;
      HIP_OK(hipMemcpyAsync(h_pairs.data(), d->n_pairs.p, 4 * (size_t)ng, hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(h_kept.data(), d->n_kept.p, 4 * (size_t)ng, hipMemcpyDeviceToHost, st));
      if (cur_pts) {
        h_cur.resize(2 * (size_t)ng * widest);
        HIP_OK(hipMemcpy2DAsync(h_cur.data(), 8 * (size_t)widest, d->k_cur.p, 8 * (size_t)K, 8 * (size_t)widest, ng, hipMemcpyDeviceToHost, st));
      }
      if (old_pts) {
        h_old.resize(2 * (size_t)ng * widest);
        HIP_OK(hipMemcpy2DAsync(h_old.data(), 8 * (size_t)widest, d->k_old.p, 8 * (size_t)K, 8 * (size_t)widest, ng, hipMemcpyDeviceToHost, st));
      }
      HIP_OK(hipStreamSynchronize(st));
      d->timed_b = true;
      for (int g = 0; g < ng; g++) {
        VioLoopDetection &r = out[geom[g].q];
        r.n_di_matches = h_pairs[g], r.n_inliers = h_kept[g];
        if (h_pairs[g] >= min_count && h_kept[g] > P.min_inliers) {
          r.status = VIO_LOOP_DETECTED;
          const size_t o = 2 * (size_t)geom[g].q * pts_stride;
          if (cur_pts) memcpy(cur_pts + o, h_cur.data() + 2 * (size_t)g * widest, 8 * (size_t)h_kept[g]);
          if (old_pts) memcpy(old_pts + o, h_old.data() + 2 * (size_t)g * widest, 8 * (size_t)h_kept[g]);
        }
      }
    }
    return VIO_OK;
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
}

// vio_loop_detector_connect. row: pair i reads row row[i] of ids and writes row row[i] of every output (NULL: row i);
// its VioLoopConnection is the one at (char *)out + row * out_step.
int connect_run(vio_loop_detector *d, const VioConfig *cfg, int32_t min_loop_num, int32_t n, const int32_t *session, const int32_t *cur_entry,
                const int32_t *old_entry, const int32_t *n_window, const int32_t *ids, int32_t stride, const int32_t *row, void *out,
                size_t out_step, uint8_t *status, float *matched_old_pts, int32_t *kept_index, int32_t *kept_ids, double *kept_old_norm) {
  auto row_of = [row](int i) { return row ? row[i] : i; };
  auto result = [&](int i) -> VioLoopConnection & { return *(VioLoopConnection *)((char *)out + (size_t)row_of(i) * out_step); };
  if (!d || !cfg || n < 1 || !session || !cur_entry || !old_entry || !n_window || stride < 0 || !out || !status || !kept_index || !kept_old_norm)
    return VIO_EINVAL;
  if (ids && !kept_ids) return VIO_EINVAL;
  if (n > d->S) return VIO_EINVAL;  // (some session would be named twice)
  try {
    // every refusal is decided on the host mirror, before anything is launched or written
    d->cn_hpairs.resize(d->S), d->cn_seen.assign(d->S, 0);
    int wmax = 0;
    for (int i = 0; i < n; i++) {
      if (session[i] < 0 || session[i] >= d->S || d->cn_seen[session[i]]) return VIO_EINVAL;
      d->cn_seen[session[i]] = 1;
      const vio_loop_detector::Session &s = d->sess[session[i]];
      const int c = cur_entry[i], o = old_entry[i], nw = n_window[i];
      if (c < 0 || c >= s.n_entries || o < 0 || o >= c || s.erased[c] || s.erased[o]) return VIO_EINVAL;
      if (nw < 0 || nw > stride || nw > s.off[c + 1] - s.off[c]) return VIO_EINVAL;
      d->cn_hpairs[i] = LdPair{session[i], nw, s.off[o + 1] - s.off[o], s.off[c + 1] - nw, s.off[o]};
      wmax = std::max(wmax, nw);
    }
    for (int i = 0; i < n; i++) memset(&result(i), 0, sizeof(VioLoopConnection)), result(i).n_window = n_window[i];
    if (wmax == 0) return VIO_OK;  // (no queries anywhere: nothing kept, nothing connected)
    VIO_ON_DEVICE_OF(d);
    hipStream_t st = d->stream;
    const size_t SK = (size_t)d->S * d->K, T = (size_t)n * wmax;  // T <= SK: n <= S, n_window <= the entry's keys <= K
    const size_t full = 33 * SK + 8 * (size_t)d->S;
    int rc = d->cn_pairs.ensure(d->S);
    if (rc == VIO_OK) rc = d->cn_ids.ensure(SK);
    if (rc == VIO_OK) rc = d->cn_intr.ensure(4 * (size_t)d->S);
    if (rc == VIO_OK && !d->cn_hintr.p) {  // (first call: the rows of sessions no call has named yet travel too, as zeros)
      rc = d->cn_hintr.ensure(4 * (size_t)d->S);
      if (rc == VIO_OK) memset(d->cn_hintr.p, 0, sizeof(float) * 4 * (size_t)d->S);
    }
    if (rc == VIO_OK) rc = d->cn_unmatched.ensure(SK);
    if (rc == VIO_OK) rc = d->cn_out.ensure(full);
    // (page-locked memory for what this call brings back; it grows to the largest call seen and stays)
    if (rc == VIO_OK) rc = d->cn_host.ensure(33 * T + 8 * (size_t)n);
    if (rc != VIO_OK) return rc;
    // the sections of the download, rows of wmax per pair
    const size_t o_norm = 0, o_pts = 16 * T, o_kidx = 24 * T, o_kids = 28 * T, o_hdr = 32 * T, o_status = 32 * T + 8 * (size_t)n;
    const size_t bytes = o_status + T;
    unsigned char *D = d->cn_out.p, *Hb = d->cn_host.p;
    HIP_OK(hipMemcpyAsync(d->cn_pairs.p, d->cn_hpairs.data(), sizeof(LdPair) * (size_t)n, hipMemcpyHostToDevice, st));
    for (int i = 0; i < n; i++) {  // the rows of the call's sessions (the other rows are not read)
      const int q = session[i];
      float *in = d->cn_hintr.p + 4 * (size_t)q;
      if (d->has_cam[q]) in[0] = (float)d->cam[q].cx, in[1] = (float)d->cam[q].cy, in[2] = (float)d->cam[q].fx, in[3] = (float)d->cam[q].fy;
      else in[0] = (float)cfg->cx, in[1] = (float)cfg->cy, in[2] = (float)cfg->fx, in[3] = (float)cfg->fy;
    }
    HIP_OK(hipMemcpyAsync(d->cn_intr.p, d->cn_hintr.p, sizeof(float) * 4 * (size_t)d->S, hipMemcpyHostToDevice, st));
    if (ids && row) {  // the rows of the pairs do not lie behind each other: gathered on the host, one upload
      d->cn_hids.resize(T);
      for (int i = 0; i < n; i++) memcpy(d->cn_hids.data() + (size_t)i * wmax, ids + (size_t)row[i] * stride, 4 * (size_t)n_window[i]);
      HIP_OK(hipMemcpyAsync(d->cn_ids.p, d->cn_hids.data(), 4 * T, hipMemcpyHostToDevice, st));
    } else if (ids) {
      HIP_OK(hipMemcpy2DAsync(d->cn_ids.p, 4 * (size_t)wmax, ids, 4 * (size_t)stride, 4 * (size_t)wmax, n, hipMemcpyHostToDevice, st));
    }
    const LdStore S = d->store();
    hipLaunchKernelGGL(ld_connect_search_kernel, dim3((wmax + kCnWaves - 1) / kCnWaves, n), dim3(64 * kCnWaves), 0, st, d->cn_pairs.p, S, wmax,
                       d->p_cur.p, (float *)(D + o_pts), d->cn_unmatched.p);
    hipLaunchKernelGGL(ld_connect_count_kernel, dim3(n), dim3(64), 0, st, d->cn_pairs.p, wmax, d->cn_unmatched.p, d->n_pairs.p);
    HIP_OK(hipGetLastError());
    // cv::findFundamentalMat(measurements, measurements_old, FM_RANSAC, 2.0, 0.99) (:49)
    rc = vio::fundamental_ransac_batch(st, d->p_cur.p, (const float *)(D + o_pts), d->n_pairs.p, n, wmax, 8, 2.0f, 0.99, d->mask.p);
    if (rc != VIO_OK) return rc;
    hipLaunchKernelGGL(ld_connect_keep_kernel, dim3(n), dim3(64), 0, st, d->cn_pairs.p, wmax, d->n_pairs.p, d->mask.p, (const float *)(D + o_pts),
                       ids ? d->cn_ids.p : nullptr, d->cn_intr.p, D + o_status,
                       (int *)(D + o_kidx), (int *)(D + o_kids), (double *)(D + o_norm), (int *)(D + o_hdr));
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(Hb, D, bytes, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const int *hdr = (const int *)(Hb + o_hdr);
    for (int i = 0; i < n; i++) {
      const int nw = n_window[i], nk = hdr[2 * i], ran = hdr[2 * i + 1];
      const size_t src = (size_t)i * wmax, dst = (size_t)row_of(i) * stride;
      VioLoopConnection &r = result(i);
      r.ransac_ran = ran, r.n_kept = nk, r.connected = ran && nk > min_loop_num ? 1 : 0;
      memcpy(status + dst, Hb + o_status + src, (size_t)nw);
      const bool matched = nw < 8 ? nk == nw : ran != 0;  // (with an unmatched query the old points mean nothing: not written)
      if (matched_old_pts && matched) memcpy(matched_old_pts + 2 * dst, Hb + o_pts + 8 * src, 8 * (size_t)nw);
      memcpy(kept_index + dst, Hb + o_kidx + 4 * src, 4 * (size_t)nk);
      if (ids) memcpy(kept_ids + dst, Hb + o_kids + 4 * src, 4 * (size_t)nk);
      if (ran) memcpy(kept_old_norm + 2 * dst, Hb + o_norm + 16 * src, 16 * (size_t)nk);
    }
    return VIO_OK;
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
}

}  // namespace

extern "C" {

int vio_loop_detector_detect(vio_loop_detector_t *d, int32_t n, const int32_t *session, const int32_t *n_keys, const float *keys,
                             const uint64_t *desc, VioLoopDetection *out, float *cur_pts, float *old_pts, int32_t pts_stride) {
  return detect_run(d, n, session, n_keys, keys, desc, nullptr, out, cur_pts, old_pts, pts_stride);
}

// The intrinsics findConnectionWithOldFrame normalises the old keyframe's pixels with (loop/keyframe.cpp:45-46; FOCUS_LENGTH_X/Y,
// PX, PY per device: global_param.cpp:24-131), per session.
int vio_loop_detector_set_cameras(vio_loop_detector_t *d, int32_t n, const int32_t *session, const VioCamera *cam) {
  if (!d || n < 0 || (n > 0 && (!session || !cam)) || n > d->S) return VIO_EINVAL;
  std::vector<char> seen(d->S, 0);
  for (int i = 0; i < n; i++) {
    if (session[i] < 0 || session[i] >= d->S || seen[session[i]] || !vio::camera_valid(cam[i], false)) return VIO_EINVAL;
    seen[session[i]] = 1;
  }
  for (int i = 0; i < n; i++) d->cam[session[i]] = cam[i], d->has_cam[session[i]] = 1;
  return VIO_OK;
}

int vio_loop_detector_get_camera(vio_loop_detector_t *d, int32_t session, VioCamera *out) {
  if (!d || session < 0 || session >= d->S || !out) return VIO_EINVAL;
  if (!d->has_cam[session]) return VIO_ESTATE;  // (none set: the session uses the cfg of every call)
  *out = d->cam[session];
  return VIO_OK;
}

int vio_loop_detector_connect(vio_loop_detector_t *d, const VioConfig *cfg, int32_t min_loop_num, int32_t n, const int32_t *session,
                              const int32_t *cur_entry, const int32_t *old_entry, const int32_t *n_window, const int32_t *ids, int32_t stride,
                              VioLoopConnection *out, uint8_t *status, float *matched_old_pts, int32_t *kept_index, int32_t *kept_ids,
                              double *kept_old_norm) {
  return connect_run(d, cfg, min_loop_num, n, session, cur_entry, old_entry, n_window, ids, stride, nullptr, out, sizeof(VioLoopConnection), status,
                     matched_old_pts, kept_index, kept_ids, kept_old_norm);
}

// The loop thread's keyframe step (VINS_ios/ViewController.mm:913-975: extractBrief, startLoopClosure,
// findConnectionWithOldFrame) = vio_brief_extract, vio_loop_detector_detect, vio_loop_detector_connect for the sessions
// that detected, with the keys and descriptors handed over on the device (vio_brief_pack.hip). The host waits once for
// the per-frame counts (its mirror of the slab offsets needs them); the detector's stream waits for the extractor's by
// its event.
int vio_loop_detector_keyframes(vio_loop_detector_t *d, vio_brief_t *b, const VioConfig *cfg, int32_t min_loop_num, int32_t n,
                                const int32_t *session, const void *frames, int32_t frames_on_device, const int32_t *frame_index,
                                const float *window_pts, const int32_t *n_window, const int32_t *ids, int32_t stride, int32_t fast_threshold,
                                VioLoopKeyframe *out, uint8_t *status, float *matched_old_pts, int32_t *kept_index, int32_t *kept_ids,
                                double *kept_old_norm, float *cur_pts, float *old_pts, int32_t pts_stride) {
  if (!d || !b || !cfg || n < 1 || !session || !frames || !n_window || stride < 0 || !out || !status || !kept_index || !kept_old_norm)
    return VIO_EINVAL;
  if (ids && !kept_ids) return VIO_EINVAL;
  if ((cur_pts || old_pts) && pts_stride < d->K) return VIO_EINVAL;
  // every refusal is decided here, on the host, before anything is launched or written
  const vio::BriefShape shape = vio::brief_shape(b);
  if (shape.device != d->device || shape.cap > d->K) return VIO_EINVAL;
  // (the intrinsics normalise the old frame's pixels: they belong to the image size the extractor was made for)
  if (cfg->image_rows != shape.rows || cfg->image_cols != shape.cols || !(cfg->fx != 0.0) || !(cfg->fy != 0.0)) return VIO_EINVAL;
  int rc = check_sessions(d, n, session);
  if (rc == VIO_EINVAL) return rc;
  const int rc_brief = vio::brief_check(b, frames, frames_on_device != 0, frame_index, n, window_pts, n_window, stride);
  if (rc_brief == VIO_EINVAL) return rc_brief;
  if (rc != VIO_OK) return rc;
  if (rc_brief != VIO_OK) return rc_brief;
  try {
    VIO_ON_DEVICE_OF(d);
    rc = d->kf_counts.ensure(2 * (size_t)d->S);
    if (rc != VIO_OK) return rc;
    vio::BriefResult ex;
    rc = vio::brief_launch(b, frames, frames_on_device != 0, frame_index, n, window_pts, n_window, stride, fast_threshold, &ex);
    if (rc != VIO_OK) return rc;
    int *n_fast = d->kf_counts.p, *n_keys = d->kf_counts.p + d->S;
    HIP_OK(hipMemcpyAsync(n_fast, ex.n_fast, 4 * (size_t)n, hipMemcpyDeviceToHost, ex.stream));
    HIP_OK(hipMemcpyAsync(n_keys, ex.n_keypoints, 4 * (size_t)n, hipMemcpyDeviceToHost, ex.stream));
    HIP_OK(hipStreamSynchronize(ex.stream));
    std::vector<VioLoopDetection> det(n);
    rc = detect_run(d, n, session, n_keys, nullptr, nullptr, &ex, det.data(), cur_pts, old_pts, pts_stride);
    if (rc != VIO_OK) return rc;
    std::vector<int> row, ses, cur, old, nw;
    for (int q = 0; q < n; q++) {
      memset(&out[q], 0, sizeof(out[q]));
      out[q].detection = det[q];
      out[q].n_fast = n_fast[q], out[q].n_keys = n_keys[q], out[q].fast_cut = n_fast[q] > shape.cap - n_window[q] ? 1 : 0;
      if (det[q].status != VIO_LOOP_DETECTED) continue;
      row.push_back(q), ses.push_back(session[q]), cur.push_back(det[q].query), old.push_back(det[q].match), nw.push_back(n_window[q]);
    }
    if (row.empty()) return VIO_OK;
    return connect_run(d, cfg, min_loop_num, (int)row.size(), ses.data(), cur.data(), old.data(), nw.data(), ids, stride, row.data(),
                       &out[0].connection, sizeof(VioLoopKeyframe), status, matched_old_pts, kept_index, kept_ids, kept_old_norm);
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
}

}  // extern "C"
