// vio_brief_launch.h — the launch sequence of the descriptor extraction (vio_brief.hip: blur9, fast_score, fast_collect,
// brief) for callers inside the library: vio_brief_extract and vio_brief_extract_device download what it leaves on the
// device, vio_loop_detector_keyframes (vio_loop_detector.hip) packs it into the detector's input arrays and never leaves
// the device. One vio_brief_t serves one call at a time: its device arrays hold the results until the next launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct vio_brief;

namespace vio {

struct BriefShape {
  int device, rows, cols, max_frames, cap;
};
// where a launched extraction leaves its results: rows of `cap` keypoints per frame of the call
struct BriefResult {
  const float *keypoints;               // [n_frames][cap][2]
  const unsigned long long *desc;       // [n_frames][cap][4]
  const int *n_fast, *n_keypoints;      // [n_frames]
  int cap;
  hipStream_t stream;                   // the extractor's stream
  hipEvent_t done;                      // recorded behind the last kernel
};

BriefShape brief_shape(const vio_brief *b);

// Every refusal of an extraction, decided before anything is launched. Frame f of the call is slot frame_index[f]
// (f when NULL) of `frames`, rows * cols bytes per slot. on_device: `frames` must be device memory of the extractor's
// device (hipPointerGetAttributes) that holds every slot named, else VIO_EINVAL.
int brief_check(const vio_brief *b, const void *frames, bool on_device, const int32_t *frame_index, int n_frames, const float *window_pts,
                const int32_t *n_window, int window_stride);
// The uploads (n_window, the window points; host frames go up once, slot by slot) and the four kernels on the
// extractor's stream; no wait. Device frames are read in place: frames of the call that lie behind each other in the
// buffer are one launch of blur9 / fast_score. Arguments as checked by brief_check, on the extractor's device.
int brief_launch(vio_brief *b, const void *frames, bool on_device, const int32_t *frame_index, int n_frames, const float *window_pts,
                 const int32_t *n_window, int window_stride, int fast_threshold, BriefResult *out);

// vio_brief_pack.hip: the rows of an extraction behind each other, frame f at [off[f], off[f + 1]) of keys / desc
// (off [n_frames + 1] on the device, off[f + 1] - off[f] = n_keypoints[f] <= cap). No synchronization.
hipError_t launch_brief_pack(const BriefResult &r, int n_frames, const int *off, float *keys, unsigned long long *desc, hipStream_t stream);

}  // namespace vio
