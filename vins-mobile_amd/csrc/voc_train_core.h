// voc_train_core.h — vocabulary training on the device: TemplatedVocabulary<FBrief>::create
// (ThirdParty/DBoW/TemplatedVocabulary.h:551-580) as level-synchronous passes over ONE index array segmented by node.
//   HKmeansStep            :635-812   hierarchical k-medians, one tree level per group of launches
//   initiateClustersKMpp   :827-908   k-means++ seeding (the random stream is stated in include/vio_amd.h)
//   createWords            :913-933   word ids in node-id order over the leaves
//   setNodeWeights         :938-991   Ni per word through the ordinary descent, log on the host
//   FBrief::meanValue / distance      ThirdParty/DBoW/FBrief.cpp:22-57  bitwise majority (> floor(N/2)), Hamming distance
//
// The n training descriptors keep their place in `desc`; `idx` is a permutation of 0..n-1 in which every node of the
// current level owns one contiguous SEGMENT, members in list order. The segments of a level partition [0, n): the ones that
// are split at this level ("expandable": the root, or a group of more than one member above level L) carry an ordinal e
// into the per-node arrays, the others (finished groups of one, children of level L) only keep their positions. Every
// kernel is one workgroup of 256 work-items per BLOCK of 256 consecutive positions (or per 256 nodes / per cluster), so the
// number of launches depends on k, L and the iteration count only, and the work per pass is n * k distance evaluations
// whatever the number of nodes. A block sees the segments that intersect it (consecutive segment ids); a segment that
// lies inside one block is finished by that block alone (LDS counters, plain stores), a segment that crosses a block
// boundary gets the global counter row of the block it starts in (only the last segment of a block can cross its end:
// one row per block is enough) and integer atomics, so every result is independent of arrival order.
//
// Per level (host loop of train_tree below; M = max_iterations):
//   fill_pos_seg                       position -> segment (binary search)
//   seed_first                         first centre = uniform draw; trivial nodes (n <= k): child i = descriptor i
//   k - 1 times seed_dist, scan_total, seed_pick
//                                      distance to the newest centre, min, per-segment 64-bit sum, block totals; exclusive
//                                      scan of the block totals; the first position whose running sum reaches cut
//   up to M + 1 times associate (+ majority when a splitting segment crosses a block)
//                                      nearest centre (first on ties), changed flag against the previous association, the
//                                      256 bit counters and sizes per cluster: work-item t owns bit t and walks the
//                                      segment's members staged in LDS; new centres by ballot (wave w = word w)
//   hist, hist_scan, scatter           cluster sizes, per-block cluster counts and their scan, stable partition
// and once: the descent of every training descriptor (bow_lookup_kernel), ni_count (per image unique words).
// No kernel waits on another workgroup; every device loop is bounded by k, 256, the segment count of a block (<= 256),
// log2(n) or an image's descriptor count.
//
// The bodies are written in spmd.h's vocabulary: tests/emul/simt_voc_train.cpp runs them workgroup by workgroup on the
// SIMT emulator through the same host loop (train_tree<Backend>).
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "spmd.h"
#include "vio_amd.h"

namespace vio {
namespace voc {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kMaxK = 32;                 // clusters per node (LDS counters, the 8-bit cluster field of the key)
constexpr int kMaxL = 10;                 // levels
constexpr int kMaxDescriptors = 1 << 22;  // training descriptors
constexpr int kMaxPerImage = 1 << 16;     // descriptors of one image (ni_count compares an image's words pairwise)
constexpr int kMaxIterations = 4096;      // refusal bound of max_iterations
constexpr int kDefaultIterations = 128;
constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;

// ---- the random stream (include/vio_amd.h states it) --------------------------------------------------------------------
VIO_HD u64 mix(u64 x) {
  x += kGolden;
  u64 z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
VIO_HD u64 child_key(u64 parent, int c) { return mix(parent ^ (u64)(c + 1)); }
VIO_HD u64 draw(u64 key, int j) { return mix(key + (u64)j * kGolden); }
VIO_HD int first_centre(u64 key, int n) {
  const double u = (double)(draw(key, 0) >> 11) * 0x1p-53;  // [0, 1)
  const int i = (int)(u * (double)n);
  return i < n - 1 ? i : n - 1;
}
VIO_HD double cut_of(u64 key, int m, u64 sum) { return ((double)((draw(key, m) >> 11) + 1) * 0x1p-53) * (double)sum; }  // factor in (0, 1]
VIO_HD int hamming(const u64 *a, u64 b0, u64 b1, u64 b2, u64 b3) {
  return __builtin_popcountll(a[0] ^ b0) + __builtin_popcountll(a[1] ^ b1) + __builtin_popcountll(a[2] ^ b2) + __builtin_popcountll(a[3] ^ b3);
}

enum State { ST_ITERATING = 0, ST_CONVERGED = 1, ST_CAPPED = 2, ST_TRIVIAL = 3 };
enum Kernel { K_FILL = 0, K_SEED_FIRST, K_SEED_DIST, K_SCAN_TOTAL, K_SEED_PICK, K_ASSOCIATE, K_MAJORITY, K_HIST, K_HIST_SCAN, K_SCATTER, K_NI };
enum Pass { P_SEED = 0, P_ITERATE, P_REGROUP, P_WEIGHTS, kPasses };

struct Args {
  int n, k, nb;        // descriptors = positions; clusters per node; blocks of 256 positions
  int n_seg, n_exp;    // segments of the level; the ones that are split
  int m;               // seed_dist / seed_pick: the centre being chosen (1 .. k-1)
  int it, last;        // associate / majority: mean passes done so far; 1 = the cap is reached, associate only
  const u64 *desc;     // [n][4]
  const int *idx;      // [n] position -> descriptor
  int *idx_out;        // [n] scatter
  const int *seg_start;  // [n_seg + 1]
  const int *seg_exp;    // [n_seg] ordinal among the split segments, -1 = not split
  const int *exp_seg;    // [n_exp]
  const u64 *key;        // [n_exp] the node's key of the random stream
  int *pos_seg;          // [n]
  int *nc, *state, *iters, *changed, *lbase;  // [n_exp] centres so far; State; mean passes; association changed; scan base
  u64 *centre;           // [n_exp][k][4]
  int *size;             // [n_exp][k] final group sizes
  u64 *sum;              // [k][n_exp] sum of min_dists before centre m is drawn
  int *md, *assoc;       // [n] per position
  u64 *btotal, *bprefix;  // [nb], [nb + 1]
  int *gcnt, *gsize;      // [nb][k][256], [nb][k]: counters of the segment that crosses the end of block b
  int *ghist, *hprefix;   // [nb][k] cluster counts of block b's last segment; [k][nb + 1] their exclusive scans
  int *n_iterating;       // [max_iterations + 2] segments that went on after pass `it`
  // ni_count
  const int *img_off;  // [n_images + 1]
  const int *word;     // [n] word of every training descriptor (original order)
  int *ni;             // [n_words]
};

struct Cx {
  int tid, nt, block;
};

struct LdsMem {
  u64 d[4][kThreads];  // the block's descriptors, word-major: work-item t reads word t >> 6 of every member (broadcast)
  u64 part[kThreads];
  int a[kThreads];     // cluster of the position, -1 = none
  int scan[2][kThreads];
  int chg[kThreads];   // per segment of the block: a member changed its cluster
  int sz[kMaxK];
  unsigned short cnt[kMaxK][kThreads];  // [cluster][bit]: a block holds at most 256 members
};
typedef VIO_AS3 LdsMem *Lds;

#define VOC_ATOMIC_ADD(p, v) __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// inclusive scan over the block; the result of every work-item stays in l->scan[0] until the next call
VIO_DEV int block_scan_inc(const Cx &cx, Lds l, int v) {
  int cur = 0;
  l->scan[0][cx.tid] = v;
  VIO_SYNC();
  for (int off = 1; off < kThreads; off <<= 1) {
    int x = l->scan[cur][cx.tid];
    if (cx.tid >= off) x += l->scan[cur][cx.tid - off];
    l->scan[cur ^ 1][cx.tid] = x;
    cur ^= 1;
    VIO_SYNC();
  }
  return l->scan[0][cx.tid];  // (8 steps: back in half 0)
}

VIO_DEV void fill_pos_seg(const Cx &cx, const Args &a) {
  const int i = cx.block * kThreads + cx.tid;
  if (i >= a.n) return;
  int lo = 0, hi = a.n_seg;  // last segment with start <= i
  for (int step = 0; step < 32 && hi - lo > 1; step++) {
    const int mid = (lo + hi) >> 1;
    if (a.seg_start[mid] <= i) lo = mid;
    else hi = mid;
  }
  a.pos_seg[i] = lo;
}

// one work-item per split segment
VIO_DEV void seed_first(const Cx &cx, const Args &a) {
  const int e = cx.block * kThreads + cx.tid;
  if (e >= a.n_exp) return;
  const int s = a.exp_seg[e], st = a.seg_start[s], n = a.seg_start[s + 1] - st;
  u64 *c = a.centre + (size_t)e * a.k * 4;
  if (n <= a.k) {  // :653-663 one cluster per feature
    for (int j = 0; j < n; j++) {
      const u64 *f = a.desc + 4 * (size_t)a.idx[st + j];
      c[4 * j] = f[0], c[4 * j + 1] = f[1], c[4 * j + 2] = f[2], c[4 * j + 3] = f[3];
      a.assoc[st + j] = j;
    }
    a.nc[e] = n, a.state[e] = ST_TRIVIAL;
  } else {
    const u64 *f = a.desc + 4 * (size_t)a.idx[st + first_centre(a.key[e], n)];
    c[0] = f[0], c[1] = f[1], c[2] = f[2], c[3] = f[3];
    a.nc[e] = 1, a.state[e] = ST_ITERATING;
  }
  a.iters[e] = 0;
}

// min_dists against centre m - 1, their sum per segment (into sum[m]), the block's total, the segment's scan base
VIO_DEV void seed_dist(const Cx &cx, const Args &a, Lds l) {
  const int blk0 = cx.block * kThreads, i = blk0 + cx.tid;
  const bool valid = i < a.n;
  int s = -1, e = -1, md = 0;
  bool act = false;
  if (valid) {
    s = a.pos_seg[i], e = a.seg_exp[s];
    act = e >= 0 && a.state[e] == ST_ITERATING && a.nc[e] == a.m;  // (a node whose seeding ended early has nc < m)
    if (act) {
      const u64 *c = a.centre + ((size_t)e * a.k + (a.m - 1)) * 4;
      const int d = hamming(a.desc + 4 * (size_t)a.idx[i], c[0], c[1], c[2], c[3]);
      md = a.m == 1 ? d : (a.md[i] < d ? a.md[i] : d);
    }
    a.md[i] = md;
  }
  const int inc = block_scan_inc(cx, l, md);
  if (cx.tid == kThreads - 1) a.btotal[cx.block] = (u64)inc;
  if (act) {
    const int st = a.seg_start[s], en = a.seg_start[s + 1];
    if (i == st) a.lbase[e] = inc - md;
    if (i + 1 == en || cx.tid == kThreads - 1) {  // last member of the segment in this block: the segment's part
      const int fs = (st > blk0 ? st : blk0) - blk0;
      const int part = inc - (fs > 0 ? l->scan[0][fs - 1] : 0);
      u64 *dst = a.sum + (size_t)a.m * a.n_exp + e;
      if (st >= blk0 && en <= blk0 + kThreads) *dst = (u64)part;
      else if (part) VOC_ATOMIC_ADD(dst, (u64)part);
    }
  }
}

// exclusive scan of in[0], in[stride], ... (nb values) -> out[0 .. nb]; one workgroup
template <class T>
VIO_DEV void scan_blocks(const Cx &cx, const T *in, int stride, int nb, T *out, Lds l) {
  const int chunk = (nb + kThreads - 1) / kThreads, b0 = cx.tid * chunk;
  u64 s = 0;
  for (int j = 0; j < chunk; j++)
    if (b0 + j < nb) s += (u64)in[(size_t)(b0 + j) * stride];
  l->part[cx.tid] = s;
  VIO_SYNC();
  if (cx.tid == 0) {
    u64 run = 0;
    for (int t = 0; t < kThreads; t++) {
      const u64 v = l->part[t];
      l->part[t] = run, run += v;
    }
  }
  VIO_SYNC();
  u64 run = l->part[cx.tid];
  for (int j = 0; j < chunk; j++)
    if (b0 + j < nb) out[b0 + j] = (T)run, run += (u64)in[(size_t)(b0 + j) * stride];
  if (b0 <= nb && nb < b0 + chunk) out[nb] = (T)run;
  if (nb == kThreads * chunk && cx.tid == kThreads - 1) out[nb] = (T)run;
}

// the first position whose running sum of min_dists reaches cut becomes centre m
VIO_DEV void seed_pick(const Cx &cx, const Args &a, Lds l) {
  const int blk0 = cx.block * kThreads, i = blk0 + cx.tid;
  const bool valid = i < a.n;
  const int md = valid ? a.md[i] : 0;
  const int inc = block_scan_inc(cx, l, md);
  if (!valid || md == 0) return;  // (the pick has a positive min_dist)
  const int s = a.pos_seg[i], e = a.seg_exp[s];
  if (e < 0) return;
  const u64 total = a.sum[(size_t)a.m * a.n_exp + e];
  if (total == 0) return;  // :880-904 every descriptor equals some centre: the seeding of this node is over
  const int st = a.seg_start[s], b0 = st / kThreads;
  const u64 pref = (b0 == cx.block ? 0 : a.bprefix[cx.block] - a.bprefix[b0]) + (u64)inc - (u64)a.lbase[e];
  const double cut = cut_of(a.key[e], a.m, total);
  if ((double)pref >= cut && !((double)(pref - (u64)md) >= cut)) {
    const u64 *f = a.desc + 4 * (size_t)a.idx[i];
    u64 *c = a.centre + ((size_t)e * a.k + a.m) * 4;
    c[0] = f[0], c[1] = f[1], c[2] = f[2], c[3] = f[3];
    a.nc[e] = a.m + 1;
  }
}

// the members [lo, hi) of segment s in this block
struct Span {
  int st, en, lo, hi;
  bool whole;
};
VIO_DEV Span span_of(const Args &a, int s, int blk0) {
  Span p;
  p.st = a.seg_start[s], p.en = a.seg_start[s + 1];
  p.lo = (p.st > blk0 ? p.st : blk0) - blk0;
  p.hi = (p.en < blk0 + kThreads ? p.en : blk0 + kThreads) - blk0;
  p.whole = p.st >= blk0 && p.en <= blk0 + kThreads;
  return p;
}

// bit t of cluster c's new centre from the counters, written by the first lane of wave w as word w
VIO_DEV void write_centre(const Cx &cx, const Args &a, int e, int c, bool bit) {
  const u64 m = (u64)__builtin_amdgcn_ballot_w64(bit);
  if ((cx.tid & 63) == 0) a.centre[((size_t)e * a.k + c) * 4 + (cx.tid >> 6)] = m;
}

// :714-765 associate, compare with the previous association, and -- unless the node is done -- :687-710 the new centres
VIO_DEV void associate(const Cx &cx, const Args &a, Lds l) {
  const int blk0 = cx.block * kThreads, i = blk0 + cx.tid;
  const bool valid = i < a.n;
  const int s_lo = a.pos_seg[blk0], s_hi = a.pos_seg[blk0 + kThreads - 1 < a.n ? blk0 + kThreads - 1 : a.n - 1];
  int s = -1, e = -1, mine = -1;
  u64 f0 = 0, f1 = 0, f2 = 0, f3 = 0;
  l->chg[cx.tid] = 0;
  if (valid) s = a.pos_seg[i], e = a.seg_exp[s];
  const bool act = e >= 0 && a.state[e] == ST_ITERATING;
  VIO_SYNC();
  if (act) {
    const u64 *f = a.desc + 4 * (size_t)a.idx[i];
    f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
    const int nc = a.nc[e];
    const u64 *c = a.centre + (size_t)e * a.k * 4;
    unsigned best = 0xffffffffu;
    for (int j = 0; j < nc; j++) {
      const unsigned key = (unsigned)hamming(c + 4 * j, f0, f1, f2, f3) << 8 | (unsigned)j;  // smallest distance, first centre on ties
      best = key < best ? key : best;
    }
    mine = (int)(best & 255u);
    if (a.it > 0 && a.assoc[i] != mine) l->chg[s - s_lo] = 1;
    a.assoc[i] = mine;
  }
  l->a[cx.tid] = mine;
  l->d[0][cx.tid] = f0, l->d[1][cx.tid] = f1, l->d[2][cx.tid] = f2, l->d[3][cx.tid] = f3;
  VIO_SYNC();
  const int w = cx.tid >> 6, bit = cx.tid & 63;
  for (int s2 = s_lo; s2 <= s_hi; s2++) {  // (at most 256 segments meet a block)
    const int e2 = a.seg_exp[s2];
    if (e2 < 0) continue;
    if (a.state[e2] != ST_ITERATING) continue;
    const Span p = span_of(a, s2, blk0);
    const int nc = a.nc[e2];
    for (int c = 0; c < nc; c++) l->cnt[c][cx.tid] = 0;
    for (int j = p.lo; j < p.hi; j++) l->cnt[l->a[j]][cx.tid] += (unsigned short)((l->d[w][j] >> bit) & 1);
    if (cx.tid < nc) {
      int z = 0;
      for (int j = p.lo; j < p.hi; j++) z += l->a[j] == cx.tid;
      l->sz[cx.tid] = z;
    }
    VIO_SYNC();
    const bool chg = a.it == 0 || l->chg[s2 - s_lo] != 0;
    if (p.whole) {
      if (chg && !a.last)
        for (int c = 0; c < nc; c++) write_centre(cx, a, e2, c, (int)l->cnt[c][cx.tid] > (l->sz[c] >> 1));
      if (cx.tid == 0) {
        if (!chg) a.state[e2] = ST_CONVERGED;
        else if (a.last) a.state[e2] = ST_CAPPED;
        else a.iters[e2] = a.it + 1, VOC_ATOMIC_ADD(a.n_iterating + a.it, 1);
      }
    } else {
      const int slot = p.st / kThreads;
      for (int c = 0; c < nc; c++) {
        const int v = l->cnt[c][cx.tid];
        if (v) VOC_ATOMIC_ADD(a.gcnt + ((size_t)slot * a.k + c) * kThreads + cx.tid, v);
      }
      if (cx.tid < nc && l->sz[cx.tid]) VOC_ATOMIC_ADD(a.gsize + (size_t)slot * a.k + cx.tid, l->sz[cx.tid]);
      if (cx.tid == 0 && l->chg[s2 - s_lo]) a.changed[e2] = 1;
    }
    VIO_SYNC();
  }
}

// block b: the segment that starts in b and crosses its end, from the global counters; leaves them zeroed
VIO_DEV void majority(const Cx &cx, const Args &a, Lds l) {
  const int b = cx.block, lastp = (b + 1) * kThreads - 1 < a.n ? (b + 1) * kThreads - 1 : a.n - 1;
  const int s = a.pos_seg[lastp], e = a.seg_exp[s];
  if (e < 0) return;
  if (a.state[e] != ST_ITERATING) return;
  const int st = a.seg_start[s], en = a.seg_start[s + 1];
  if (st / kThreads != b || en <= (b + 1) * kThreads) return;
  const int nc = a.nc[e];
  const bool chg = a.it == 0 || a.changed[e] != 0;
  if (cx.tid < nc) l->sz[cx.tid] = a.gsize[(size_t)b * a.k + cx.tid];
  VIO_SYNC();
  for (int c = 0; c < nc; c++) {
    int *g = a.gcnt + ((size_t)b * a.k + c) * kThreads + cx.tid;
    if (chg && !a.last) write_centre(cx, a, e, c, *g > (l->sz[c] >> 1));
    *g = 0;
  }
  VIO_SYNC();
  if (cx.tid < nc) a.gsize[(size_t)b * a.k + cx.tid] = 0;
  if (cx.tid == 0) {
    a.changed[e] = 0;
    if (!chg) a.state[e] = ST_CONVERGED;
    else if (a.last) a.state[e] = ST_CAPPED;
    else a.iters[e] = a.it + 1, VOC_ATOMIC_ADD(a.n_iterating + a.it, 1);
  }
}

// final group sizes of every split segment; ghist[b] = the cluster counts of block b's last segment inside b
VIO_DEV void hist(const Cx &cx, const Args &a, Lds l) {
  const int blk0 = cx.block * kThreads, i = blk0 + cx.tid;
  const int s_lo = a.pos_seg[blk0], s_hi = a.pos_seg[blk0 + kThreads - 1 < a.n ? blk0 + kThreads - 1 : a.n - 1];
  l->a[cx.tid] = i < a.n ? a.assoc[i] : -1;
  if (cx.tid < a.k) a.ghist[(size_t)cx.block * a.k + cx.tid] = 0;
  VIO_SYNC();
  for (int s2 = s_lo; s2 <= s_hi; s2++) {
    const int e2 = a.seg_exp[s2];
    if (e2 < 0) continue;
    const Span p = span_of(a, s2, blk0);
    if (cx.tid < a.nc[e2]) {
      int z = 0;
      for (int j = p.lo; j < p.hi; j++) z += l->a[j] == cx.tid;
      int *dst = a.size + (size_t)e2 * a.k + cx.tid;
      if (p.whole) *dst = z;
      else if (z) VOC_ATOMIC_ADD(dst, z);
      if (s2 == s_hi) a.ghist[(size_t)cx.block * a.k + cx.tid] = z;
    }
  }
}

// :789-811 the children's descriptor lists: a STABLE partition of every split segment by cluster
VIO_DEV void scatter(const Cx &cx, const Args &a, Lds l) {
  const int blk0 = cx.block * kThreads, i = blk0 + cx.tid;
  const bool valid = i < a.n;
  l->a[cx.tid] = valid ? a.assoc[i] : -1;
  VIO_SYNC();
  if (!valid) return;
  const int s = a.pos_seg[i], e = a.seg_exp[s];
  if (e < 0) {
    a.idx_out[i] = a.idx[i];
    return;
  }
  const int st = a.seg_start[s], en = a.seg_start[s + 1], b0 = st / kThreads, c = l->a[cx.tid];
  int p = st;
  for (int j = 0; j < c; j++) p += a.size[(size_t)e * a.k + j];
  if (b0 != cx.block) p += a.hprefix[(size_t)c * (a.nb + 1) + cx.block] - a.hprefix[(size_t)c * (a.nb + 1) + b0];
  for (int j = (st > blk0 ? st : blk0) - blk0; j < cx.tid; j++) p += l->a[j] == c;
  if (p >= st && p < en) a.idx_out[p] = a.idx[i];
}

// :957-978 Ni: one workgroup per image, a word counts once per image (its first occurrence)
VIO_DEV void ni_count(const Cx &cx, const Args &a) {
  const int o = a.img_off[cx.block], n = a.img_off[cx.block + 1] - o;
  for (int i = cx.tid; i < n; i += kThreads) {
    const int wd = a.word[o + i];
    bool dup = false;
    for (int j = 0; j < i; j++) dup = dup || a.word[o + j] == wd;
    if (!dup) VOC_ATOMIC_ADD(a.ni + wd, 1);
  }
}

template <class L>
VIO_DEV void run_kernel(int kernel, const Cx &cx, const Args &a, L l) {
  switch (kernel) {
    case K_FILL: fill_pos_seg(cx, a); break;
    case K_SEED_FIRST: seed_first(cx, a); break;
    case K_SEED_DIST: seed_dist(cx, a, l); break;
    case K_SCAN_TOTAL: scan_blocks<u64>(cx, a.btotal, 1, a.nb, a.bprefix, l); break;
    case K_SEED_PICK: seed_pick(cx, a, l); break;
    case K_ASSOCIATE: associate(cx, a, l); break;
    case K_MAJORITY: majority(cx, a, l); break;
    case K_HIST: hist(cx, a, l); break;
    case K_HIST_SCAN: scan_blocks<int>(cx, a.ghist + cx.block, a.k, a.nb, a.hprefix + (size_t)cx.block * (a.nb + 1), l); break;
    case K_SCATTER: scatter(cx, a, l); break;
    case K_NI: ni_count(cx, a); break;
    default: break;
  }
}

// ---- the host loop --------------------------------------------------------------------------------------------------------
struct Node {
  int parent = -1, level = 0, n = 0;  // index of the parent in discovery (level) order; members of its group
  int first_child = -1, n_children = 0;
  int id = 0;                         // creation order of the reference's recursion
  u64 key = 0;
  u64 d[4] = {0, 0, 0, 0};
};

struct Tree {
  std::vector<Node> nodes;   // discovery order, nodes[0] = root
  std::vector<int> by_id;    // id -> index
  std::vector<int> word_node;  // word id -> node id
  VioVocabularyTrainStats stats;
};

// buffers a backend keeps (grow-only)
enum Buf { B_DESC = 0, B_IDX0, B_IDX1, B_POS_SEG, B_MD, B_ASSOC, B_SEG_START, B_SEG_EXP, B_EXP_SEG, B_KEY, B_NC, B_STATE, B_ITERS, B_CHANGED,
           B_LBASE, B_CENTRE, B_SIZE, B_SUM, B_BTOTAL, B_BPREFIX, B_GCNT, B_GSIZE, B_GHIST, B_HPREFIX, B_NITER, B_IMG_OFF, B_WORD, B_NI, kBufs };

// Backend: void *buf(int id, size_t bytes) (nullptr = out of memory), zero / up / down (down returns after the data is
// there), launch(kernel, blocks, args), pass(id) (the launches that follow belong to pass id), bool ok().
template <class B>
int train_tree(B &be, const VioVocabularyTrainParams &P, int n, const u64 *h_desc, Tree &T) {
  const int k = P.k, L = P.L, M = P.max_iterations, nb = (n + kThreads - 1) / kThreads;
  VioVocabularyTrainStats &S = T.stats;
  memset(&S, 0, sizeof(S));
  S.n_descriptors = n;
  Args a;
  memset(&a, 0, sizeof(a));
  a.n = n, a.k = k, a.nb = nb;
  u64 *d_desc = (u64 *)be.buf(B_DESC, 32 * (size_t)n);
  int *d_idx[2] = {(int *)be.buf(B_IDX0, 4 * (size_t)n), (int *)be.buf(B_IDX1, 4 * (size_t)n)};
  a.pos_seg = (int *)be.buf(B_POS_SEG, 4 * (size_t)n), a.md = (int *)be.buf(B_MD, 4 * (size_t)n), a.assoc = (int *)be.buf(B_ASSOC, 4 * (size_t)n);
  a.btotal = (u64 *)be.buf(B_BTOTAL, 8 * (size_t)nb), a.bprefix = (u64 *)be.buf(B_BPREFIX, 8 * (size_t)(nb + 1));
  a.gcnt = (int *)be.buf(B_GCNT, 4 * (size_t)nb * k * kThreads), a.gsize = (int *)be.buf(B_GSIZE, 4 * (size_t)nb * k);
  a.ghist = (int *)be.buf(B_GHIST, 4 * (size_t)nb * k), a.hprefix = (int *)be.buf(B_HPREFIX, 4 * (size_t)k * (nb + 1));
  a.n_iterating = (int *)be.buf(B_NITER, 4 * (size_t)(M + 2));
  if (!d_desc || !d_idx[0] || !d_idx[1] || !a.pos_seg || !a.md || !a.assoc || !a.btotal || !a.bprefix || !a.gcnt || !a.gsize || !a.ghist ||
      !a.hprefix || !a.n_iterating)
    return VIO_ENOMEM;
  a.desc = d_desc;
  be.up(d_desc, h_desc, 32 * (size_t)n);
  {
    std::vector<int> id0(n);
    for (int i = 0; i < n; i++) id0[i] = i;
    be.up(d_idx[0], id0.data(), 4 * (size_t)n);
  }
  be.zero(a.gcnt, 4 * (size_t)nb * k * kThreads), be.zero(a.gsize, 4 * (size_t)nb * k);
  be.zero(a.md, 4 * (size_t)n), be.zero(a.assoc, 4 * (size_t)n);
  int cur = 0;
  size_t e_cap = 1;
  for (int l = 1; l < L && e_cap < (size_t)n; l++) e_cap *= (size_t)k;
  e_cap = std::max<size_t>(1, std::min<size_t>(e_cap, (size_t)n / 2));

  struct Seg {
    int start, n, node;
    bool split;
  };
  std::vector<Seg> segs(1, Seg{0, n, 0, true}), next;
  T.nodes.assign(1, Node());
  T.nodes[0].n = n, T.nodes[0].key = mix(P.seed);
  std::vector<int> h_start, h_sexp, h_eseg, h_nc, h_state, h_iters, h_size;
  std::vector<u64> h_key, h_centre;
  for (int level = 1; level <= L; level++) {
    h_start.clear(), h_sexp.clear(), h_eseg.clear(), h_key.clear();
    bool nontrivial = false, crossing = false;
    for (size_t s = 0; s < segs.size(); s++) {
      h_start.push_back(segs[s].start);
      h_sexp.push_back(segs[s].split ? (int)h_eseg.size() : -1);
      if (!segs[s].split) continue;
      h_eseg.push_back((int)s), h_key.push_back(T.nodes[segs[s].node].key);
      if (segs[s].n > k) {
        nontrivial = true;
        crossing = crossing || segs[s].start / kThreads != (segs[s].start + segs[s].n - 1) / kThreads;
      }
    }
    h_start.push_back(n);
    const int ns = (int)segs.size(), ne = (int)h_eseg.size();
    if (ne == 0) break;
    if ((size_t)ne > e_cap || ns > n) return VIO_ENODEV;  // (cannot happen)
    a.n_seg = ns, a.n_exp = ne;
    // (sized once for the widest level: at most min(k^(L-1), n / 2) nodes are split on a level, n segments exist)
    int *d_start = (int *)be.buf(B_SEG_START, 4 * ((size_t)n + 1)), *d_sexp = (int *)be.buf(B_SEG_EXP, 4 * (size_t)n);
    int *d_eseg = (int *)be.buf(B_EXP_SEG, 4 * e_cap);
    u64 *d_key = (u64 *)be.buf(B_KEY, 8 * e_cap);
    a.nc = (int *)be.buf(B_NC, 4 * e_cap), a.state = (int *)be.buf(B_STATE, 4 * e_cap), a.iters = (int *)be.buf(B_ITERS, 4 * e_cap);
    a.changed = (int *)be.buf(B_CHANGED, 4 * e_cap), a.lbase = (int *)be.buf(B_LBASE, 4 * e_cap);
    a.centre = (u64 *)be.buf(B_CENTRE, 32 * e_cap * k), a.size = (int *)be.buf(B_SIZE, 4 * e_cap * k);
    a.sum = (u64 *)be.buf(B_SUM, 8 * e_cap * k);
    if (!d_start || !d_sexp || !d_eseg || !d_key || !a.nc || !a.state || !a.iters || !a.changed || !a.lbase || !a.centre || !a.size || !a.sum)
      return VIO_ENOMEM;
    a.seg_start = d_start, a.seg_exp = d_sexp, a.exp_seg = d_eseg, a.key = d_key;
    a.idx = d_idx[cur], a.idx_out = d_idx[cur ^ 1];
    be.up(d_start, h_start.data(), 4 * (size_t)(ns + 1)), be.up(d_sexp, h_sexp.data(), 4 * (size_t)ns);
    be.up(d_eseg, h_eseg.data(), 4 * (size_t)ne), be.up(d_key, h_key.data(), 8 * (size_t)ne);
    be.zero(a.changed, 4 * (size_t)ne), be.zero(a.size, 4 * (size_t)ne * k), be.zero(a.sum, 8 * (size_t)ne * k);
    be.zero(a.centre, 32 * (size_t)ne * k), be.zero(a.n_iterating, 4 * (size_t)(M + 2));

    be.pass(P_SEED);
    be.launch(K_FILL, nb, a);
    be.launch(K_SEED_FIRST, (ne + kThreads - 1) / kThreads, a);
    if (nontrivial) {
      for (int m = 1; m < k; m++) {
        a.m = m;
        be.launch(K_SEED_DIST, nb, a), be.launch(K_SCAN_TOTAL, 1, a), be.launch(K_SEED_PICK, nb, a);
      }
      be.pass(P_ITERATE);
      for (int it = 0; it <= M; it++) {
        a.it = it, a.last = it == M;
        be.launch(K_ASSOCIATE, nb, a);
        if (crossing) be.launch(K_MAJORITY, nb, a);
        int going = 0;
        be.down(&going, a.n_iterating + it, 4);
        if (!be.ok()) return VIO_ENODEV;
        if (going == 0) break;
      }
    }
    be.pass(P_REGROUP);
    be.launch(K_HIST, nb, a), be.launch(K_HIST_SCAN, k, a), be.launch(K_SCATTER, nb, a);
    cur ^= 1;
    h_nc.resize(ne), h_state.resize(ne), h_iters.resize(ne), h_size.resize((size_t)ne * k), h_centre.resize((size_t)ne * k * 4);
    be.down(h_nc.data(), a.nc, 4 * (size_t)ne), be.down(h_state.data(), a.state, 4 * (size_t)ne), be.down(h_iters.data(), a.iters, 4 * (size_t)ne);
    be.down(h_size.data(), a.size, 4 * (size_t)ne * k), be.down(h_centre.data(), a.centre, 32 * (size_t)ne * k);
    if (!be.ok()) return VIO_ENODEV;

    // :778-811 the children of every split node, consecutive; the next level's segments in position order
    next.clear();
    for (size_t s = 0; s < segs.size(); s++) {
      if (!segs[s].split) {
        next.push_back(segs[s]);
        continue;
      }
      const int e = h_sexp[s], p = segs[s].node, nc = h_nc[e];
      if (nc < 1 || nc > k) return VIO_ENODEV;  // (cannot happen: a device fault would have been reported above)
      T.nodes[p].first_child = (int)T.nodes.size(), T.nodes[p].n_children = nc;
      if (segs[s].n > k) {
        S.short_nodes += nc < k, S.capped_nodes += h_state[e] == ST_CAPPED;
        S.iterations_max[level - 1] = std::max(S.iterations_max[level - 1], (int32_t)h_iters[e]);
      }
      int at = segs[s].start, total = 0;
      for (int c = 0; c < nc; c++) {
        Node ch;
        ch.parent = p, ch.level = level, ch.n = h_size[(size_t)e * k + c], ch.key = child_key(T.nodes[p].key, c);
        memcpy(ch.d, &h_centre[((size_t)e * k + c) * 4], 32);
        S.empty_clusters += ch.n == 0;
        if (ch.n > 0) next.push_back(Seg{at, ch.n, (int)T.nodes.size(), level < L && ch.n > 1});
        at += ch.n, total += ch.n;
        T.nodes.push_back(ch);
      }
      if (total != segs[s].n) return VIO_ENODEV;
    }
    segs.swap(next);
  }
  // ids in the order the reference's recursion creates the nodes: all children of a node, then the subtrees in order
  const int nn = (int)T.nodes.size();
  T.by_id.assign(nn, 0);
  {
    int next_id = 1;
    std::vector<std::pair<int, int>> stack(1, std::make_pair(0, -1));  // (node, child cursor; -1 = children not yet numbered)
    while (!stack.empty()) {
      const int p = stack.back().first;
      int &c = stack.back().second;
      const Node &N = T.nodes[p];
      if (c < 0) {
        for (int j = 0; j < N.n_children; j++) T.nodes[N.first_child + j].id = next_id, T.by_id[next_id++] = N.first_child + j;
        c = 0;
      }
      while (c < N.n_children && T.nodes[N.first_child + c].n_children == 0) c++;
      if (c >= N.n_children) {
        stack.pop_back();
        continue;
      }
      const int child = N.first_child + c;
      c++;
      stack.push_back(std::make_pair(child, -1));
    }
  }
  T.word_node.clear();
  for (int id = 1; id < nn; id++)
    if (T.nodes[T.by_id[id]].n_children == 0) T.word_node.push_back(id);
  S.n_nodes = nn - 1, S.n_words = (int32_t)T.word_node.size();
  return VIO_OK;
}

// the file (loop/VocabularyBinary.hpp:17-50), canonical: nodes in id order, words in id order. word_weight may be null (0).
inline std::vector<unsigned char> make_blob(const Tree &T, const VioVocabularyTrainParams &P, const double *word_weight) {
  const int nn = (int)T.nodes.size() - 1, nw = (int)T.word_node.size();
  std::vector<unsigned char> blob(24 + (size_t)nn * 48 + (size_t)nw * 8);
  const int32_t hdr[6] = {P.k, P.L, 0, P.weighting, nn, nw};
  memcpy(blob.data(), hdr, 24);
  unsigned char *q = blob.data() + 24;
  for (int id = 1; id <= nn; id++, q += 48) {
    const Node &N = T.nodes[T.by_id[id]];
    const int32_t ids[2] = {id, T.nodes[N.parent].id};
    const double w = 0.0;
    memcpy(q, ids, 8), memcpy(q + 8, &w, 8), memcpy(q + 16, N.d, 32);
  }
  for (int w = 0; w < nw; w++, q += 8) {
    const int32_t rec[2] = {T.word_node[w], w};
    memcpy(q, rec, 8);
    if (word_weight) memcpy(blob.data() + 24 + (size_t)(T.word_node[w] - 1) * 48 + 8, &word_weight[w], 8);
  }
  return blob;
}

}  // namespace voc
}  // namespace vio
