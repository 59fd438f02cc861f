// vio_voc_train.hip — vio_vocabulary_train: the kernels of voc_train_core.h (one __global__ per body, 256 work-items per
// block of 256 positions) behind the backend its host loop asks for, the words' Ni through vio_bow.hip's lookup kernel,
// the weights on the host (std::log, TemplatedVocabulary.h:980-987) and the vocabulary through vio_vocabulary_create.
#include <hip/hip_runtime.h>

#include <math.h>

#include <new>
#include <vector>

#include "vio_amd.h"
#include "vio_bow_core.h"
#include "vio_device.h"
#include "voc_train_core.h"

namespace vc = vio::voc;

namespace {

template <int K>
__global__ __launch_bounds__(vc::kThreads) void voc_train_kernel(vc::Args a) {
  __shared__ vc::LdsMem mem;
  const vc::Cx cx{(int)threadIdx.x, vc::kThreads, (int)blockIdx.x};
  vc::run_kernel(K, cx, a, (vc::Lds)&mem);
}

struct DeviceBackend {
  hipStream_t st = nullptr;
  vio::DevBuf<unsigned char> bufs[vc::kBufs];
  hipError_t err = hipSuccess;
  int launches = 0;
  std::vector<std::pair<int, hipEvent_t>> marks;  // (pass, the event before its first launch)
  ~DeviceBackend() {
    if (st) (void)hipStreamSynchronize(st);
    for (auto &m : marks) (void)hipEventDestroy(m.second);
    if (st) (void)hipStreamDestroy(st);
  }
  void note(hipError_t e) {
    if (e != hipSuccess && err == hipSuccess) {
      err = e;
      fprintf(stderr, "vio_amd: vocabulary training: %s\n", hipGetErrorString(e));
    }
  }
  bool ok() const { return err == hipSuccess; }
  void *buf(int id, size_t bytes) { return bufs[id].ensure(bytes) == VIO_OK ? bufs[id].p : nullptr; }
  void zero(void *p, size_t bytes) {
    if (ok()) note(hipMemsetAsync(p, 0, bytes, st));
  }
  void up(void *d, const void *h, size_t bytes) {  // (pageable source: the copy has left the host buffer on return)
    if (ok()) note(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
    if (ok()) note(hipStreamSynchronize(st));
  }
  void down(void *h, const void *d, size_t bytes) {
    if (ok()) note(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st));
    if (ok()) note(hipStreamSynchronize(st));
  }
  void pass(int id) {
    if (!ok()) return;
    hipEvent_t e;
    note(hipEventCreate(&e));
    if (!ok()) return;
    marks.push_back({id, e});
    note(hipEventRecord(e, st));
  }
  template <int K>
  void go(int blocks, const vc::Args &a) {
    hipLaunchKernelGGL(voc_train_kernel<K>, dim3(blocks), dim3(vc::kThreads), 0, st, a);
  }
  void launch(int kernel, int blocks, const vc::Args &a) {
    if (!ok() || blocks < 1) return;
    switch (kernel) {
      case vc::K_FILL: go<vc::K_FILL>(blocks, a); break;
      case vc::K_SEED_FIRST: go<vc::K_SEED_FIRST>(blocks, a); break;
      case vc::K_SEED_DIST: go<vc::K_SEED_DIST>(blocks, a); break;
      case vc::K_SCAN_TOTAL: go<vc::K_SCAN_TOTAL>(blocks, a); break;
      case vc::K_SEED_PICK: go<vc::K_SEED_PICK>(blocks, a); break;
      case vc::K_ASSOCIATE: go<vc::K_ASSOCIATE>(blocks, a); break;
      case vc::K_MAJORITY: go<vc::K_MAJORITY>(blocks, a); break;
      case vc::K_HIST: go<vc::K_HIST>(blocks, a); break;
      case vc::K_HIST_SCAN: go<vc::K_HIST_SCAN>(blocks, a); break;
      case vc::K_SCATTER: go<vc::K_SCATTER>(blocks, a); break;
      case vc::K_NI: go<vc::K_NI>(blocks, a); break;
      default: return;
    }
    launches++;
    note(hipGetLastError());
  }
  // closes the last pass and sums the intervals per pass
  void times(double pass_ms[vc::kPasses]) {
    for (int i = 0; i < vc::kPasses; i++) pass_ms[i] = 0.0;
    pass(-1);
    if (ok()) note(hipStreamSynchronize(st));
    for (size_t i = 0; ok() && i + 1 < marks.size(); i++) {
      float ms = 0;
      note(hipEventElapsedTime(&ms, marks[i].second, marks[i + 1].second));
      if (marks[i].first >= 0 && marks[i].first < vc::kPasses) pass_ms[marks[i].first] += ms;
    }
  }
};

}  // namespace

extern "C" {

void vio_vocabulary_train_params_default(VioVocabularyTrainParams *p) {
  if (!p) return;
  p->k = 10, p->L = 6, p->weighting = 0, p->max_iterations = vc::kDefaultIterations, p->seed = 0;
}

int vio_vocabulary_train(const VioVocabularyTrainParams *p, int32_t n_images, const int32_t *n_desc, const uint64_t *desc,
                         vio_vocabulary_t **out, VioVocabularyTrainStats *stats) {
  if (!p || !out || n_images < 1 || !n_desc) return VIO_EINVAL;
  if (p->k < 2 || p->k > vc::kMaxK || p->L < 1 || p->L > vc::kMaxL || p->weighting < 0 || p->weighting > 3 || p->max_iterations < 0 ||
      p->max_iterations > vc::kMaxIterations)
    return VIO_EINVAL;
  long long total = 0;
  bool wide = false;
  for (int g = 0; g < n_images; g++) {
    if (n_desc[g] < 0) return VIO_EINVAL;
    wide = wide || n_desc[g] > vc::kMaxPerImage;
    total += n_desc[g];
  }
  if (total == 0 || !desc) return VIO_EINVAL;
  if (total > vc::kMaxDescriptors || wide) return VIO_ECAP;
  if (!vio::device_ready("vocabulary training")) return VIO_ENODEV;
  const int n = (int)total;
  try {
    DeviceBackend be;
    HIP_OK(hipStreamCreateWithFlags(&be.st, hipStreamNonBlocking));
    vc::Tree T;
    int rc = vc::train_tree(be, *p, n, (const vc::u64 *)desc, T);
    if (rc != VIO_OK) return rc;
    if (!be.ok()) return VIO_ENODEV;
    const int nw = (int)T.word_node.size();
    std::vector<unsigned char> blob = vc::make_blob(T, *p, nullptr);
    vio_vocabulary_t *v = nullptr;
    rc = vio_vocabulary_create(blob.data(), blob.size(), &v);
    if (rc != VIO_OK) return rc;
    std::vector<double> ww(nw, 1.0);  // :944-949 TF, BINARY: the idf part is 1
    be.pass(vc::P_WEIGHTS);
    if (p->weighting == 0 || p->weighting == 2) {
      vc::Args a;
      memset(&a, 0, sizeof(a));
      std::vector<int> off(n_images + 1, 0), ni(nw, 0);
      for (int g = 0; g < n_images; g++) off[g + 1] = off[g] + n_desc[g];
      int *d_off = (int *)be.buf(vc::B_IMG_OFF, 4 * (size_t)(n_images + 1)), *d_word = (int *)be.buf(vc::B_WORD, 4 * (size_t)n);
      int *d_ni = (int *)be.buf(vc::B_NI, 4 * (size_t)nw);
      if (!d_off || !d_word || !d_ni) {
        vio_vocabulary_destroy(v);
        return VIO_ENOMEM;
      }
      be.up(d_off, off.data(), 4 * (size_t)(n_images + 1));
      be.zero(d_ni, 4 * (size_t)nw);
      if (be.ok()) be.note(hipStreamSynchronize(be.st));
      rc = be.ok() ? vio::bow_lookup_words(v, (const unsigned long long *)be.bufs[vc::B_DESC].p, n, d_word) : VIO_ENODEV;
      be.launches++;
      if (rc == VIO_OK) {
        a.img_off = d_off, a.word = d_word, a.ni = d_ni;
        be.launch(vc::K_NI, n_images, a);
        be.down(ni.data(), d_ni, 4 * (size_t)nw);
        if (!be.ok()) rc = VIO_ENODEV;
      }
      if (rc != VIO_OK) {
        vio_vocabulary_destroy(v);
        return rc;
      }
      for (int w = 0; w < nw; w++) ww[w] = ni[w] > 0 ? log((double)n_images / (double)ni[w]) : 0.0;  // :981-987
    }
    rc = vio::bow_set_word_weights(v, ww.data());
    if (rc != VIO_OK) {
      vio_vocabulary_destroy(v);
      return rc;
    }
    T.stats.launches = be.launches;
    be.times(T.stats.pass_ms);
    for (int i = 0; i < vc::kPasses; i++) T.stats.kernel_ms += T.stats.pass_ms[i];
    if (!be.ok()) {
      vio_vocabulary_destroy(v);
      return VIO_ENODEV;
    }
    if (stats) *stats = T.stats;
    *out = v;
    return VIO_OK;
  } catch (const std::bad_alloc &) {
    return VIO_ENOMEM;
  }
}

}  // extern "C"
