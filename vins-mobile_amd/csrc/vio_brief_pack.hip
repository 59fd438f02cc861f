// vio_brief_pack.hip — the hand-over from the descriptor extraction (vio_brief.hip) to the loop detector
// (vio_loop_detector.hip) on the device: the extraction leaves rows of `cap` keypoints per frame, the detector reads the
// keyframes of a call behind each other (in_keys / in_desc at the offsets of its t_off). A copy kernel, HBM-bound:
// 40 bytes per keypoint in and out.
#include <hip/hip_runtime.h>

#include "vio_brief_launch.h"

namespace {

// grid (chunks, n_frames): frame f moves off[f + 1] - off[f] keypoints (<= cap) from row f to [off[f], off[f + 1])
__global__ __launch_bounds__(256) void brief_pack_kernel(const float *kp, const unsigned long long *desc, int cap, const int *off, float *keys,
                                                         unsigned long long *out_desc) {
  const int f = blockIdx.y, o = off[f], n = min(off[f + 1] - o, cap);
  const size_t src = (size_t)f * cap, dst = (size_t)o;
  const int t0 = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  for (int i = t0; i < 4 * n; i += step) out_desc[4 * dst + i] = desc[4 * src + i];
  for (int i = t0; i < 2 * n; i += step) keys[2 * dst + i] = kp[2 * src + i];
}

}  // namespace

namespace vio {

hipError_t launch_brief_pack(const BriefResult &r, int n_frames, const int *off, float *keys, unsigned long long *desc, hipStream_t stream) {
  const int chunks = (4 * r.cap + 255) / 256;
  hipLaunchKernelGGL(brief_pack_kernel, dim3(chunks < 16 ? chunks : 16, n_frames), dim3(256), 0, stream, r.keypoints, r.desc, r.cap, off, keys,
                     desc);
  return hipGetLastError();
}

}  // namespace vio
