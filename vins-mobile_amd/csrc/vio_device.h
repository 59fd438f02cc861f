// vio_device.h — a context belongs to the HIP device that was current when it was created.
//
// HIP's current device is per host thread (default 0). The reference calls readImage on the camera-callback thread and
// solve_ceres on the mainLoop thread (VINS_ios/ViewController.mm:458 vs :688-724), and a multi-GPU host runs one
// context per device: every ABI entry therefore switches the calling thread to the context's device for the duration
// of the call (and puts the thread's previous device back), so a context works from any thread.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "vio_amd.h"
#include "vio_env.h"

// A failed HIP call ends the ABI entry with VIO_ENODEV (and says which call on stderr).
#define HIP_OK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      fprintf(stderr, "vio_amd: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return VIO_ENODEV;                                                                   \
    }                                                                                      \
  } while (0)

namespace vio {

// The HIP runtime(s) mapped into this process: distinct files named libamdhip64* in /proc/self/maps. The library binds
// to whichever one the process loaded first (next to PyTorch that is the copy bundled with the wheel, not /opt/rocm's).
// Two different copies in one process each keep their own device state -- streams, allocations and kernels of one are
// invisible to the other -- so the contexts refuse to start in that case instead of failing in obscure ways later.
inline std::vector<std::string> hip_runtimes() {
  std::vector<std::string> out;
  FILE *f = fopen("/proc/self/maps", "r");
  if (!f) return out;
  char line[4096];
  while (fgets(line, sizeof(line), f)) {
    const char *lib = strstr(line, "libamdhip64");
    if (!lib) continue;
    const char *path = strchr(line, '/');
    if (!path) continue;
    std::string p(path);
    while (!p.empty() && (p.back() == '\n' || p.back() == ' ')) p.pop_back();
    bool seen = false;
    for (const std::string &q : out) seen = seen || q == p;
    if (!seen) out.push_back(p);
  }
  fclose(f);
  return out;
}
// The host-only translation units are built with $(HOST_ARCH) (csrc/Makefile: -mavx2 by default). On a host CPU without
// that instruction set the first such function would die with SIGILL; the *_create entries (built without the flag: every
// .hip file) refuse with VIO_ENODEV instead.
inline bool host_isa_ok() {
#if defined(VIO_HOST_NEEDS_AVX2) && !defined(__HIP_DEVICE_COMPILE__) && (defined(__x86_64__) || defined(__i386__))
  static const bool ok = [] {
    __builtin_cpu_init();
    const bool have = __builtin_cpu_supports("avx2");
    if (!have) fprintf(stderr, "vio_amd: this host CPU has no AVX2 and the library's host code was built with it (rebuild with `make HOST_ARCH=`)\n");
    return have;
  }();
  return ok;
#else
  return true;
#endif
}
inline bool single_hip_runtime() {
  static const int n = [] {
    const std::vector<std::string> r = hip_runtimes();
    if (r.size() > 1 && env_flag("VIO_AMD_ALLOW_TWO_RUNTIMES")) return 1;  // (the caller knows what it is doing)
    if (r.size() > 1) {
      fprintf(stderr, "vio_amd: %zu different HIP runtimes are mapped into this process:\n", r.size());
      for (const std::string &p : r) fprintf(stderr, "vio_amd:   %s\n", p.c_str());
      fprintf(stderr, "vio_amd: refusing to create device contexts (load one runtime only, e.g. import torch before this library; "
                      "VIO_AMD_ALLOW_TWO_RUNTIMES=1 overrides)\n");
    }
    return (int)r.size();
  }();
  return n <= 1 && host_isa_ok();
}

// The preamble of every *_create: a device is visible, one HIP runtime is mapped, the host CPU runs the host code.
inline bool device_ready(const char *what) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    fprintf(stderr, "vio_amd: no HIP device visible; %s has no CPU fallback\n", what);
    return false;
  }
  return single_hip_runtime();
}

// Owning device (DevBuf) / page-locked host (PinnedBuf) arrays. ensure() grows only -- the old contents are not kept --
// and allocates at least one element; the memory goes back at release() or destruction. A context that holds these
// frees them after its destructor body has synchronized its stream. Never give one static storage duration: its
// destructor would run after the HIP runtime has gone at exit.
template <class T, hipError_t (*Alloc)(void **, size_t), hipError_t (*Free)(void *)>
struct OwnedBuf {
  T *p = nullptr;
  size_t n = 0;
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf &) = delete;
  OwnedBuf &operator=(const OwnedBuf &) = delete;
  ~OwnedBuf() { release(); }
  int ensure(size_t count) {
    if (count <= n && p) return VIO_OK;
    if (host_timing()) fprintf(stderr, "vio_amd: device buffer grows %zu -> %zu elements of %zu bytes\n", n, count, sizeof(T));
    release();
    if (Alloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
      p = nullptr;
      return VIO_ENOMEM;
    }
    n = count;
    return VIO_OK;
  }
  void release() {
    if (p) (void)Free(p);
    p = nullptr, n = 0;
  }
};
inline hipError_t dev_malloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t dev_free(void *p) { return hipFree(p); }
inline hipError_t pinned_malloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
inline hipError_t pinned_free(void *p) { return hipHostFree(p); }
template <class T>
using DevBuf = OwnedBuf<T, dev_malloc, dev_free>;
template <class T>
using PinnedBuf = OwnedBuf<T, pinned_malloc, pinned_free>;

// Device time of a context's launches (*_kernel_ms): an event pair around each, up to 4096 pairs kept; drain() sums
// what was recorded since the last drain.
class LaunchTimer {
 public:
  LaunchTimer() = default;
  LaunchTimer(const LaunchTimer &) = delete;
  LaunchTimer &operator=(const LaunchTimer &) = delete;
  ~LaunchTimer() {
    for (auto &e : ev_) (void)hipEventDestroy(e.first), (void)hipEventDestroy(e.second);
  }
  int begin(hipStream_t st) {
    if (used_ == ev_.size()) {
      if (ev_.size() >= 4096) {  // recycle: fold what is pending into nothing (the caller did not ask for it)
        used_ = 0;
      } else {
        hipEvent_t a, b;
        HIP_OK(hipEventCreate(&a));
        HIP_OK(hipEventCreate(&b));
        ev_.push_back({a, b});
      }
    }
    HIP_OK(hipEventRecord(ev_[used_++].first, st));
    return VIO_OK;
  }
  int end(hipStream_t st) {
    HIP_OK(hipEventRecord(ev_[used_ - 1].second, st));
    return VIO_OK;
  }
  // average ms over the launches recorded since the last drain (the events must have completed)
  int drain(double *ms_avg, int32_t *launches) {
    double sum = 0;
    for (size_t i = 0; i < used_; i++) {
      float ms = 0;
      HIP_OK(hipEventElapsedTime(&ms, ev_[i].first, ev_[i].second));
      sum += ms;
    }
    *launches = (int32_t)used_;
    *ms_avg = used_ ? sum / used_ : 0.0;
    used_ = 0;
    return VIO_OK;
  }

 private:
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_;
  size_t used_ = 0;
};

inline int current_device() {
  int d = 0;
  return hipGetDevice(&d) == hipSuccess ? d : -1;
}

class DeviceScope {
 public:
  explicit DeviceScope(int device) {
    if (device < 0) return;
    if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
    if (prev_ != device) {
      ok_ = hipSetDevice(device) == hipSuccess;
      switched_ = ok_;
    }
  }
  ~DeviceScope() {
    if (switched_ && prev_ >= 0) (void)hipSetDevice(prev_);
  }
  bool ok() const { return ok_; }
  DeviceScope(const DeviceScope &) = delete;
  DeviceScope &operator=(const DeviceScope &) = delete;

 private:
  int prev_ = -1;
  bool switched_ = false, ok_ = true;
};

}  // namespace vio

// First statement of every ABI entry that takes a context.
#define VIO_ON_DEVICE_OF(ctx)              \
  vio::DeviceScope vio_dev_scope_((ctx)->device); \
  if (!vio_dev_scope_.ok()) return VIO_ENODEV
