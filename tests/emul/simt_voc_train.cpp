// tests/emul/simt_voc_train.cpp — TEST-ONLY: the passes of vocabulary training (vins-mobile_amd/csrc/voc_train_core.h)
// executed on the host by the SIMT emulator, workgroup after workgroup (256 fibers each, ballots with the hardware's lane
// semantics, a freshly poisoned LDS per workgroup), driven by the product's own host loop train_tree<Backend>. The descent
// that gives every training descriptor its word (bow_lookup_kernel in the product) is plain C++ here; ni_count runs
// on the emulator. The caller (tests/test_vocabulary_train.py) compares file, stats and Ni with tests/voc_train_model.py.
// Not part of the product library.
#define SIMT_IMPLEMENTATION
#include "simt.h"

#include <math.h>

#include <vector>

#include "voc_train_core.h"

namespace vc = vio::voc;

namespace {

struct EmulBackend {
  std::vector<std::vector<unsigned char>> mem = std::vector<std::vector<unsigned char>>(vc::kBufs);
  int order = 0, launches = 0;
  bool ok() const { return true; }
  void *buf(int id, size_t bytes) {
    if (mem[id].size() < bytes + 64) mem[id].assign(bytes + 64, 0xee);  // (grow-only, contents not kept: as DevBuf::ensure)
    return mem[id].data();
  }
  void zero(void *p, size_t bytes) { memset(p, 0, bytes); }
  void up(void *d, const void *h, size_t bytes) { memcpy(d, h, bytes); }
  void down(void *h, const void *d, size_t bytes) { memcpy(h, d, bytes); }
  void pass(int) {}
  void launch(int kernel, int blocks, const vc::Args &a) {
    launches++;
    for (int b = 0; b < blocks; b++) {
      std::vector<unsigned char> lds(sizeof(vc::LdsMem), 0xff);
      simt::launch(vc::kThreads, [&](int tid) {
        const vc::Cx cx{tid, vc::kThreads, b};
        vc::run_kernel(kernel, cx, a, (vc::Lds)lds.data());
      }, order, 64 * 1024);
    }
  }
};

int descend(const vc::Tree &T, const vc::u64 *f) {
  int node = 0;
  while (T.nodes[node].n_children > 0) {
    const vc::Node &N = T.nodes[node];
    int best = -1, bd = 1 << 30;
    for (int c = 0; c < N.n_children; c++) {
      const int d = vc::hamming(T.nodes[N.first_child + c].d, f[0], f[1], f[2], f[3]);
      if (d < bd) bd = d, best = N.first_child + c;
    }
    node = best;
  }
  return node;
}

}  // namespace

// blob [cap] out (bytes written in *bytes), ni [n_words] out (cap_words), stats out. -> VIO_* code, -100 - x for harness errors
extern "C" int simt_voc_train(const VioVocabularyTrainParams *p, int n_images, const int32_t *n_desc, const uint64_t *desc, int order,
                              unsigned char *blob, size_t cap, size_t *bytes, int32_t *ni, int cap_words, VioVocabularyTrainStats *stats) {
  int n = 0;
  for (int g = 0; g < n_images; g++) n += n_desc[g];
  if (n < 1 || p->k < 2 || p->k > vc::kMaxK || p->L < 1 || p->L > vc::kMaxL) return VIO_EINVAL;
  EmulBackend be;
  be.order = order;
  vc::Tree T;
  const int rc = vc::train_tree(be, *p, n, (const vc::u64 *)desc, T);
  if (rc != VIO_OK) return rc;
  const int nw = (int)T.word_node.size();
  if (nw > cap_words) return -101;
  std::vector<int> word_of_id(T.nodes.size(), -1), word(n), off(n_images + 1, 0), cnt(nw, 0);
  for (int w = 0; w < nw; w++) word_of_id[T.word_node[w]] = w;
  for (int i = 0; i < n; i++) word[i] = word_of_id[T.nodes[descend(T, (const vc::u64 *)desc + 4 * (size_t)i)].id];
  for (int g = 0; g < n_images; g++) off[g + 1] = off[g] + n_desc[g];
  vc::Args a;
  memset(&a, 0, sizeof(a));
  a.img_off = off.data(), a.word = word.data(), a.ni = cnt.data();
  be.launch(vc::K_NI, n_images, a);
  std::vector<double> ww(nw, 1.0);
  if (p->weighting == 0 || p->weighting == 2)
    for (int w = 0; w < nw; w++) ww[w] = cnt[w] > 0 ? log((double)n_images / (double)cnt[w]) : 0.0;
  const std::vector<unsigned char> out = vc::make_blob(T, *p, ww.data());
  *bytes = out.size();
  if (out.size() > cap) return -102;
  memcpy(blob, out.data(), out.size());
  for (int w = 0; w < nw; w++) ni[w] = cnt[w];
  T.stats.launches = be.launches + 1;  // (+ the descent, one launch in the product)
  *stats = T.stats;
  return VIO_OK;
}
