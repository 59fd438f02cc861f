// tools/vocabulary_train_host_route.cpp — the host route tools/vocabulary_train_timing.py times vio_vocabulary_train
// against: a plain C++ restatement of TemplatedVocabulary::create for FBrief (ThirdParty/DBoW/TemplatedVocabulary.h:551-991,
// FBrief.cpp:22-57) with the semantics, the random stream and the iteration cap include/vio_amd.h states, on `threads`
// std::threads. The tree is grown level by level: a node with many members runs alone and splits its loops over the
// threads, the other nodes of the level are dealt one at a time to the threads (the stream depends on a node's path, not
// on when it runs). Not part of the product library; tests/test_vocabulary_train.py compares its file with the model's.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <thread>
#include <vector>

#include "vio_amd.h"

namespace {

typedef uint64_t u64;
const u64 kGolden = 0x9E3779B97F4A7C15ull;
const int kWide = 4096;  // members from which a node's loops are split over the threads

u64 mix(u64 x) {
  x += kGolden;
  u64 z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
u64 draw(u64 key, int j) { return mix(key + (u64)j * kGolden); }
int dist(const u64 *a, const u64 *b) {
  return __builtin_popcountll(a[0] ^ b[0]) + __builtin_popcountll(a[1] ^ b[1]) + __builtin_popcountll(a[2] ^ b[2]) + __builtin_popcountll(a[3] ^ b[3]);
}

struct Node {
  int parent = -1, level = 0, first_child = -1, n_children = 0, id = 0;
  u64 key = 0, d[4] = {0, 0, 0, 0};
  std::vector<int> members;
  int iterations = 0;
  bool ran = false, capped = false;
};

// fn(lo, hi) over [0, n) on `threads` threads
void split(int n, int threads, const std::function<void(int, int, int)> &fn) {
  if (threads <= 1 || n < 2 * threads) return fn(0, n, 0);
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++) pool.emplace_back(fn, (int)((long long)n * t / threads), (int)((long long)n * (t + 1) / threads), t);
  for (auto &th : pool) th.join();
}

// fn(t) on `threads` threads
void each_thread(int threads, const std::function<void(int)> &fn) {
  if (threads <= 1) return fn(0);
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; t++) pool.emplace_back(fn, t);
  for (auto &th : pool) th.join();
}

// HKmeansStep's clustering of one node: centres [nc][4] and the cluster of every member
void cluster(const u64 *desc, const Node &N, int k, int M, int threads, std::vector<u64> &centres, std::vector<int> &assoc, int &iterations,
             bool &capped) {
  const std::vector<int> &mem = N.members;
  const int n = (int)mem.size();
  assoc.assign(n, 0);
  if (n <= k) {
    centres.resize(4 * (size_t)n);
    for (int i = 0; i < n; i++) memcpy(&centres[4 * (size_t)i], desc + 4 * (size_t)mem[i], 32), assoc[i] = i;
    return;
  }
  if (n < kWide) threads = 1;
  std::vector<int> md(n);
  centres.clear();
  const double u = (double)(draw(N.key, 0) >> 11) * 0x1p-53;
  int pick = (int)(u * (double)n);
  if (pick > n - 1) pick = n - 1;
  for (int m = 1;; m++) {
    const u64 *c = desc + 4 * (size_t)mem[pick];
    centres.insert(centres.end(), c, c + 4);
    if (m == k) break;
    std::vector<u64> part(threads > 1 ? threads : 1, 0);
    split(n, threads, [&](int lo, int hi, int t) {
      u64 s = 0;
      for (int i = lo; i < hi; i++) {
        const int d = dist(desc + 4 * (size_t)mem[i], c);
        md[i] = m == 1 ? d : (d < md[i] ? d : md[i]);
        s += (u64)md[i];
      }
      part[t] = s;
    });
    u64 sum = 0;
    for (u64 s : part) sum += s;
    if (sum == 0) break;
    const double cut = ((double)((draw(N.key, m) >> 11) + 1) * 0x1p-53) * (double)sum;
    u64 run = 0;
    pick = n - 1;
    for (int i = 0; i < n; i++) {
      run += (u64)md[i];
      if ((double)run >= cut) {
        pick = i;
        break;
      }
    }
  }
  const int nc = (int)(centres.size() / 4);
  auto associate = [&](bool compare) {
    std::vector<int> changed(threads > 1 ? threads : 1, 0);
    split(n, threads, [&](int lo, int hi, int t) {
      for (int i = lo; i < hi; i++) {
        const u64 *f = desc + 4 * (size_t)mem[i];
        int best = 0, bd = dist(f, &centres[0]);
        for (int c = 1; c < nc; c++) {
          const int d = dist(f, &centres[4 * (size_t)c]);
          if (d < bd) bd = d, best = c;
        }
        if (compare && assoc[i] != best) changed[t] = 1;
        assoc[i] = best;
      }
    });
    int any = 0;
    for (int c : changed) any |= c;
    return any != 0;
  };
  associate(false);
  capped = true;
  std::vector<int> cnt((size_t)std::max(threads, 1) * nc * 257);
  while (iterations < M) {
    std::fill(cnt.begin(), cnt.end(), 0);
    split(n, threads, [&](int lo, int hi, int t) {
      int *my = &cnt[(size_t)t * nc * 257];
      for (int i = lo; i < hi; i++) {
        const u64 *f = desc + 4 * (size_t)mem[i];
        int *row = my + (size_t)assoc[i] * 257;
        row[256]++;
        for (int w = 0; w < 4; w++)
          for (u64 x = f[w]; x; x &= x - 1) row[64 * w + __builtin_ctzll(x)]++;
      }
    });
    for (int c = 0; c < nc; c++) {
      u64 *out = &centres[4 * (size_t)c];
      out[0] = out[1] = out[2] = out[3] = 0;
      int size = 0;
      for (int t = 0; t < std::max(threads, 1); t++) size += cnt[((size_t)t * nc + c) * 257 + 256];
      for (int b = 0; b < 256; b++) {
        int s = 0;
        for (int t = 0; t < std::max(threads, 1); t++) s += cnt[((size_t)t * nc + c) * 257 + b];
        if (s > size / 2) out[b >> 6] |= 1ull << (b & 63);
      }
    }
    iterations++;
    if (!associate(true)) {
      capped = false;
      break;
    }
  }
}

}  // namespace

// -> milliseconds of the whole training (tree, words, weights, the file), or -1
extern "C" double vocabulary_train_host_route_run(const VioVocabularyTrainParams *P, int32_t n_images, const int32_t *n_desc, const uint64_t *desc,
                                                  int32_t threads, unsigned char *blob, size_t cap, size_t *bytes, VioVocabularyTrainStats *S) {
  if (!P || !n_desc || !desc || !blob || !bytes || !S || threads < 1 || P->k < 2 || P->L < 1 || P->L > 16) return -1.0;
  const auto t0 = std::chrono::steady_clock::now();
  const int k = P->k, L = P->L;
  int n = 0;
  for (int g = 0; g < n_images; g++) n += n_desc[g];
  if (n < 1) return -1.0;
  memset(S, 0, sizeof(*S));
  std::vector<Node> nodes(1);
  nodes[0].key = mix(P->seed);
  nodes[0].members.resize(n);
  for (int i = 0; i < n; i++) nodes[0].members[i] = i;
  std::vector<int> level_nodes(1, 0), next_level;
  for (int level = 1; level <= L && !level_nodes.empty(); level++) {
    const int m = (int)level_nodes.size();
    std::vector<std::vector<u64>> centres(m);
    std::vector<std::vector<int>> assoc(m);
    for (int j = 0; j < m; j++)  // wide nodes: alone, loops split over the threads
      if ((int)nodes[level_nodes[j]].members.size() >= kWide) {
        Node &N = nodes[level_nodes[j]];
        N.ran = true;
        cluster(desc, N, k, P->max_iterations, threads, centres[j], assoc[j], N.iterations, N.capped);
      }
    std::atomic<int> next(0);
    each_thread(threads, [&](int) {  // the others: one node at a time per thread
      for (int j = next++; j < m; j = next++) {
        Node &N = nodes[level_nodes[j]];
        if ((int)N.members.size() >= kWide) continue;
        N.ran = (int)N.members.size() > k;
        cluster(desc, N, k, P->max_iterations, 1, centres[j], assoc[j], N.iterations, N.capped);
      }
    });
    next_level.clear();
    for (int j = 0; j < m; j++) {
      const int p = level_nodes[j], nc = (int)(centres[j].size() / 4);
      nodes[p].first_child = (int)nodes.size(), nodes[p].n_children = nc;
      if (nodes[p].ran) {
        S->short_nodes += nc < k, S->capped_nodes += nodes[p].capped;
        if (nodes[p].iterations > S->iterations_max[level - 1]) S->iterations_max[level - 1] = nodes[p].iterations;
      }
      const size_t first = nodes.size();
      nodes.resize(first + nc);
      for (int c = 0; c < nc; c++) {
        Node &C = nodes[first + c];
        C.parent = p, C.level = level, C.key = mix(nodes[p].key ^ (u64)(c + 1));
        memcpy(C.d, &centres[j][4 * (size_t)c], 32);
      }
      for (size_t i = 0; i < assoc[j].size(); i++) nodes[first + assoc[j][i]].members.push_back(nodes[p].members[i]);
      for (int c = 0; c < nc; c++) {
        S->empty_clusters += nodes[first + c].members.empty();
        if (level < L && nodes[first + c].members.size() > 1) next_level.push_back((int)(first + c));
      }
      std::vector<int>().swap(nodes[p].members);
    }
    level_nodes.swap(next_level);
  }
  // ids in the recursion's creation order, words over the leaves
  const int nn = (int)nodes.size();
  std::vector<int> by_id(nn, 0), word_node;
  {
    int next_id = 1;
    std::function<void(int)> visit = [&](int p) {
      for (int c = 0; c < nodes[p].n_children; c++) nodes[nodes[p].first_child + c].id = next_id, by_id[next_id++] = nodes[p].first_child + c;
      for (int c = 0; c < nodes[p].n_children; c++)
        if (nodes[nodes[p].first_child + c].n_children > 0) visit(nodes[p].first_child + c);
    };
    visit(0);
  }
  std::vector<int> word_of(nn, -1);
  for (int id = 1; id < nn; id++)
    if (nodes[by_id[id]].n_children == 0) word_of[by_id[id]] = (int)word_node.size(), word_node.push_back(id);
  const int nw = (int)word_node.size();
  std::vector<double> ww(nw, 1.0);
  if (P->weighting == 0 || P->weighting == 2) {
    std::vector<int> word(n), off(n_images + 1, 0);
    for (int g = 0; g < n_images; g++) off[g + 1] = off[g] + n_desc[g];
    split(n, threads, [&](int lo, int hi, int) {
      for (int i = lo; i < hi; i++) {
        const u64 *f = desc + 4 * (size_t)i;
        int node = 0;
        while (nodes[node].n_children > 0) {
          int best = nodes[node].first_child, bd = dist(f, nodes[best].d);
          for (int c = 1; c < nodes[node].n_children; c++) {
            const int d = dist(f, nodes[nodes[node].first_child + c].d);
            if (d < bd) bd = d, best = nodes[node].first_child + c;
          }
          node = best;
        }
        word[i] = word_of[node];
      }
    });
    std::vector<std::vector<int>> ni(std::max(threads, 1), std::vector<int>(nw, 0));
    split(n_images, threads, [&](int lo, int hi, int t) {
      std::vector<int> stamp(nw, -1);
      for (int g = lo; g < hi; g++)
        for (int i = off[g]; i < off[g + 1]; i++)
          if (stamp[word[i]] != g) stamp[word[i]] = g, ni[t][word[i]]++;
    });
    for (int w = 0; w < nw; w++) {
      int c = 0;
      for (auto &v : ni) c += v[w];
      ww[w] = c > 0 ? log((double)n_images / (double)c) : 0.0;
    }
  }
  *bytes = 24 + (size_t)(nn - 1) * 48 + (size_t)nw * 8;
  if (*bytes > cap) return -1.0;
  const int32_t hdr[6] = {k, L, 0, P->weighting, nn - 1, nw};
  memcpy(blob, hdr, 24);
  unsigned char *q = blob + 24;
  for (int id = 1; id < nn; id++, q += 48) {
    const Node &N = nodes[by_id[id]];
    const int32_t ids[2] = {id, nodes[N.parent].id};
    const double w = N.n_children == 0 ? ww[word_of[by_id[id]]] : 0.0;
    memcpy(q, ids, 8), memcpy(q + 8, &w, 8), memcpy(q + 16, N.d, 32);
  }
  for (int w = 0; w < nw; w++, q += 8) {
    const int32_t rec[2] = {word_node[w], w};
    memcpy(q, rec, 8);
  }
  S->n_descriptors = n, S->n_nodes = nn - 1, S->n_words = nw;
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
