// tools/init_align_host_route.cpp — the host route of the stage that closes estimator start-up, driven from C++ (no
// interpreter in the timed part), for tools/init_align_timing.py: per problem what solve_initial_align (vio_estimator.cpp)
// spends its time in -- one vio_visual_imu_alignment, then the re-integration of the window's W + 1 intervals from
// (0, Bgs[k]) (vio_preintegrate = host::preint_init + host::propagate, what repropagate runs) -- with the problems dealt to
// `threads` host threads one at a time, as the estimator's pool deals sequences. Every buffer is the caller's. Built on
// first use against csrc/libvio_amd.so; not part of the product library.
#include <atomic>
#include <chrono>
#include <thread>
#include <vector>

#include "vio_amd.h"

extern "C" {

typedef struct AlignHostProblem {
  double tic[3];
  const VioInitFrame *frames;  // [n_frames]
  int32_t n_frames, window_size;
  const VioInitFrame *window;  // [window_size + 1]: n_samples, dt, acc, gyr, acc_0, gyr_0 of pre_integrations[k]
  // out
  double *Bgs;                 // [(window_size + 1)][3], zeroed here before the alignment
  double *x;                   // [3 n_frames + 1]
  VioPreintegration *pre;      // [window_size + 1]
  double g[3];
  int32_t ok, rc;
} AlignHostProblem;

static void run_one(const VioConfig *cfg, AlignHostProblem &p) {
  const int P = p.window_size + 1;
  for (int i = 0; i < 3 * P; i++) p.Bgs[i] = 0.0;
  p.rc = vio_visual_imu_alignment(cfg, p.tic, p.frames, p.n_frames, p.window_size, p.Bgs, p.g, p.x, &p.ok);
  const double zero[3] = {0, 0, 0};
  for (int k = 0; k < P && p.rc == VIO_OK; k++) {
    const VioInitFrame &w = p.window[k];
    p.rc = vio_preintegrate(cfg, w.acc_0, w.gyr_0, zero, p.Bgs + 3 * k, w.n_samples, w.dt, w.acc, w.gyr, &p.pre[k]);
  }
}

// Runs the n problems on min(threads, n) threads (one: the calling thread) and returns the wall time in ms, thread start and
// join included; -1 when a library call failed.
double init_align_host_route_run(const VioConfig *cfg, AlignHostProblem *problems, int32_t n, int32_t threads) {
  if (!cfg || !problems || n < 1 || threads < 1) return -1.0;
  const auto t0 = std::chrono::steady_clock::now();
  const int T = threads < n ? threads : n;
  if (T == 1) {
    for (int i = 0; i < n; i++) run_one(cfg, problems[i]);
  } else {
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < T; t++)
      pool.emplace_back([&] {
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) run_one(cfg, problems[i]);
      });
    for (std::thread &th : pool) th.join();
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (int i = 0; i < n; i++)
    if (problems[i].rc != VIO_OK) return -1.0;
  return ms;
}

}  // extern "C"
