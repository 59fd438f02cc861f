// vio_bow_core.h — what the bag-of-words contexts share (vio_bow.hip: vocabulary + database; vio_loop_detector.hip: the
// loop detector): the vocabulary context and the BowVector kernel. Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "vio_amd.h"
#include "vio_device.h"

namespace {

constexpr int kMaxBowFeatures = 8192;  // descriptors per keyframe the BowVector kernel sorts in LDS

// one workgroup per keyframe: its descriptors' (word, weight) -> ascending unique words with their L1-normalised values
__global__ __launch_bounds__(256) void bow_vector_kernel(const int *kf_off, const int *word, const double *weight, const double *word_weight,
                                                          int accumulate, int *bow_count, int *bow_word, double *bow_value, int stride) {
  __shared__ int key[kMaxBowFeatures];
  __shared__ int scan[257];
  __shared__ double norm_s;
  const int kf = blockIdx.x, o = kf_off[kf], n = kf_off[kf + 1] - o, tid = threadIdx.x, nt = blockDim.x;
  int np2 = nt;
  while (np2 < n) np2 <<= 1;
  for (int i = tid; i < np2; i += nt) key[i] = (i < n && weight[o + i] > 0.0) ? word[o + i] : 0x7fffffff;  // stopped words drop out
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < np2; i += nt) {
        const int p = i ^ j;
        if (p > i) {
          const int a = key[i], b = key[p];
          if (((i & k) == 0) == (a > b)) key[i] = b, key[p] = a;
        }
      }
      __syncthreads();
    }
  // heads of runs of equal words: every lane owns a contiguous piece of the sorted list
  const int chunk = np2 / nt, i0 = tid * chunk;
  int cnt = 0;
  for (int i = i0; i < i0 + chunk; i++) cnt += key[i] != 0x7fffffff && (i == 0 || key[i] != key[i - 1]);
  scan[tid + 1] = cnt;
  if (tid == 0) scan[0] = 0;
  __syncthreads();
  if (tid == 0)
    for (int t = 0; t < nt; t++) scan[t + 1] += scan[t];
  __syncthreads();
  const int u = scan[nt];
  int *ow = bow_word + (size_t)kf * stride;
  double *ov = bow_value + (size_t)kf * stride;
  if (u > stride) {  // caller's capacity too small: report the count, write nothing
    if (tid == 0) bow_count[kf] = -u;
    return;
  }
  int q = scan[tid];
  for (int i = i0; i < i0 + chunk; i++) {
    const int wd = key[i];
    if (wd == 0x7fffffff || (i > 0 && wd == key[i - 1])) continue;
    int i1 = i + 1;
    while (i1 < np2 && key[i1] == wd) i1++;
    // BowVector::addWeight adds the word's weight once per occurrence (in that order: w + w + ...), addIfNotExist keeps it once
    const double wv = word_weight[wd];
    double sv = wv;
    if (accumulate)
      for (int r = i + 1; r < i1; r++) sv += wv;
    ow[q] = wd, ov[q] = sv;
    q++;
  }
  __syncthreads();
  if (tid == 0) {
    double norm = 0.0;
    for (int r = 0; r < u; r++) norm += fabs(ov[r]);  // ascending word order, like BowVector::normalize over the std::map
    norm_s = norm;
    bow_count[kf] = u;
  }
  __syncthreads();
  const double norm = norm_s;
  if (norm > 0.0)
    for (int r = tid; r < u; r += nt) ov[r] /= norm;
}

// first posting of a sorted inverted file (key = word << 32 | entry) that is not below k
__device__ __forceinline__ int posting_lower_bound(const unsigned long long *key, int n, unsigned long long k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (key[m] < k) lo = m + 1;
    else hi = m;
  }
  return lo;
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
  return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
}

}  // namespace

struct vio_vocabulary {
  int device = -1;
  int32_t k = 0, L = 0, scoring = 0, weighting = 0, n_nodes = 0, n_words = 0;  // n_nodes incl. the root
  int height = 0;  // levels below the root: bounds the descent of bow_lookup_kernel
  hipStream_t stream = nullptr;
  vio::DevBuf<unsigned long long> d_desc;
  vio::DevBuf<double> d_weight, d_wweight;  // per node; per word
  vio::DevBuf<int> d_word, d_child_off, d_child;
  // transform scratch
  vio::DevBuf<unsigned long long> t_desc;
  vio::DevBuf<int> t_word, t_off, t_bcount, t_bword;
  vio::DevBuf<double> t_weight, t_bvalue;
  std::vector<unsigned char> blob;  // the file the vocabulary was made from (vio_vocabulary_serialize / _save)
  ~vio_vocabulary() {
    if (stream) (void)hipStreamSynchronize(stream), (void)hipStreamDestroy(stream);
  }
};

namespace vio {
// what vocabulary training (vio_voc_train.hip) needs from vio_bow.hip: the descent of bow_lookup_kernel for n descriptors
// that are on the device already (word [n] on the device; the call returns after the kernel has run), and the word
// weights of a vocabulary made with weights 0 (nodes, words, and the weight fields of v->blob)
int bow_lookup_words(vio_vocabulary *v, const unsigned long long *d_desc, int n, int *d_word);
int bow_set_word_weights(vio_vocabulary *v, const double *word_weight);
}  // namespace vio
