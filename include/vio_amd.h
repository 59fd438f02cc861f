/*
 * vio_amd.h — C ABI of the MI355X-native VIO hot path.
 *
 * This is the drop-in boundary behind VINS-Mobile's two per-frame entry points
 * (all citations are into /root/reference/VINS_ios unless another root is named):
 *
 *   front-end  FeatureTracker::readImage            feature_tracker.hpp:59, feature_tracker.cpp:162-310
 *   back-end   VINS::processIMU / VINS::solve_ceres  VINS.hpp:153,163-164, VINS.cpp:333-375,480-831
 *
 * Conventions
 *   - plain pointers and sizes, caller-owned host buffers, no C++/torch types;
 *   - every function returns VIO_OK (0) or a negative VIO_E* code, never throws;
 *   - one context per sequence (or per batch); contexts are thread-compatible,
 *     not thread-safe (the reference objects are not re-entrant either:
 *     static n_id feature_tracker.cpp:11, static sqrt_info projection_facor.cpp:11);
 *   - all matrices are row-major; quaternions are stored x y z w exactly like
 *     para_Pose (VINS.cpp:93-101);
 *   - the product path needs a gfx950 device: there is no CPU fallback inside
 *     this library (the CPU restatement lives in oracle/ and is test-only);
 *   - DEVICE BINDING: a context lives on the HIP device that is current on the
 *     creating thread at *_create (hipSetDevice(k) before the call; default 0).
 *     Every later call on the context may come from ANY host thread — the
 *     reference calls readImage on the camera-callback thread and solve_ceres
 *     on the mainLoop thread (ViewController.mm:458 vs :688-724) — the entry
 *     point switches the calling thread to the context's device for the call
 *     and restores the thread's previous device on return. One process per GPU
 *     or one context per GPU in one process both work; vio_*_get_device reports
 *     the binding.
 */
#ifndef VIO_AMD_H
#define VIO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIO_ABI_VERSION 1

#define VIO_OK 0
#define VIO_EINVAL (-1)   /* bad argument / inconsistent sizes            */
#define VIO_ENODEV (-2)   /* no gfx950 device / HIP runtime error         */
#define VIO_ENOMEM (-3)   /* host or device allocation failed             */
#define VIO_ECAP (-4)     /* problem exceeds the context's capacity       */
#define VIO_ESTATE (-5)   /* call order violated                          */
#define VIO_ETIMEOUT (-6) /* the workgroups of a cooperative window did not
                             meet on the device (co-residency lost): the
                             window's termination reads 2 (FAILURE), its
                             outputs and next prior must be discarded      */

#define VIO_SIZE_POSE 7       /* global_param.hpp:30 */
#define VIO_SIZE_SPEEDBIAS 9  /* global_param.hpp:31 */
#define VIO_MAX_PRIOR_BLOCKS 96

/* ------------------------------------------------------------------------- */
/* Runtime configuration (the reference's compile-time macros and per-device
 * globals: global_param.hpp:23-58, global_param.cpp:24-131,
 * feature_tracker.hpp:24-29).                                                */
typedef struct VioConfig {
  int32_t window_size;    /* WINDOW_SIZE (10); frames in window P = W+1       */
  int32_t max_features;   /* capacity of inv_depth (NUM_OF_F = 1000)          */
  int32_t max_factors;    /* capacity of the projection-factor list           */
  int32_t max_iterations; /* options.max_num_iterations (10) VINS.cpp:645     */
  int32_t image_rows;     /* ROW (640)                                        */
  int32_t image_cols;     /* COL (480)                                        */
  int32_t max_corners;    /* MAX_CNT (70)                                     */
  int32_t min_dist;       /* MIN_DIST (30)                                    */
  int32_t freq;           /* FREQ (3): publish every freq-th frame            */
  int32_t lk_win;         /* LK window (21)        feature_tracker.cpp:181    */
  int32_t lk_levels;      /* maxLevel (3)          feature_tracker.cpp:181    */
  int32_t lk_max_iters;   /* TermCriteria COUNT (30) OpenCV default           */
  double lk_eps;          /* TermCriteria EPS (0.01)                          */
  double lk_min_eig;      /* minEigThreshold (1e-4)                           */
  double quality_level;   /* goodFeaturesToTrack qualityLevel (0.01) :263     */
  double f_threshold;     /* F_THRESHOLD (1.0 px)                             */
  double f_confidence;    /* RANSAC confidence (0.99)                         */
  double fx, fy, cx, cy;  /* FOCUS_LENGTH_X/Y, PX, PY                         */
  double gravity;         /* GRAVITY 9.805                                    */
  double acc_n, acc_w, gyr_n, gyr_w; /* ACC_N 0.5, ACC_W 2e-3, GYR_N 0.2, GYR_W 4e-5 */
  double cauchy_a;        /* CauchyLoss(1.0)       VINS.cpp:485               */
} VioConfig;

/* Fills *cfg with the reference's iPhone7P values at W=10
 * (global_param.cpp:27-42, feature_tracker.hpp:24-29).                       */
void vio_config_default(VioConfig *cfg);

/* The camera of ONE sequence: the per-device globals setGlobalParam switches
 * by phone model (global_param.cpp:24-131). cfg.fx .. cfg.cy, and the tic / ric
 * a context is created with, are what a sequence uses until a camera is set for
 * it: a context whose sequences set none computes exactly what it always did.
 * Pinhole only. Lens distortion is NOT modelled, as in the reference, whose
 * rejectWithF works on raw pixels (feature_tracker.cpp:95,198); the frames of
 * a distorted lens are rectified to a pinhole by the image pre-step, on the
 * device (VioLens, vio_preprocess_set_lenses; VioLensModel,
 * vio_preprocess_set_lens_models for a rational or a fisheye lens), and the
 * intrinsics given here are then those of the rectified image (rect_* of
 * either record).                                                             */
typedef struct VioCamera {
  double fx, fy, cx, cy;   /* FOCUS_LENGTH_X/Y, PX, PY  global_param.cpp:24-131 */
  double tic[3], ric[9];   /* camera -> body, ric row-major (TIC_*, RIC_*)      */
} VioCamera;
/* The camera a context's configuration stands for: cfg's intrinsics with the
 * given extrinsic (NULL: tic = 0, ric = identity).                            */
void vio_camera_from_config(const VioConfig *cfg, const double tic[3], const double ric[9], VioCamera *out);

/* ------------------------------------------------------------------------- */
/* IMU pre-integration between two frames: the public state of
 * IntegrationBase (integration_base.h:200-221) after the last push_back.     */
typedef struct VioPreintegration {
  double sum_dt;
  double delta_p[3];
  double delta_q[4]; /* x y z w */
  double delta_v[3];
  double linearized_ba[3];
  double linearized_bg[3];
  double jacobian[225];   /* 15x15 row-major, order O_P,O_R,O_V,O_BA,O_BG     */
  double covariance[225]; /* 15x15 row-major                                  */
} VioPreintegration;

/* Linearized prior = the kept side of MarginalizationInfo
 * (marginalization_factor.hpp:66-88): r = r0 + J0*dx.                        */
#define VIO_BLOCK_POSE 0
#define VIO_BLOCK_SPEEDBIAS 1
#define VIO_BLOCK_EXPOSE 2
typedef struct VioPrior {
  int32_t n;        /* residual rows = sum of kept local sizes (info->n)      */
  int32_t n_blocks; /* keep_block_size.size()                                 */
  int32_t block_kind[VIO_MAX_PRIOR_BLOCKS];   /* VIO_BLOCK_*                  */
  int32_t block_index[VIO_MAX_PRIOR_BLOCKS];  /* frame index the block is
                          bound to in the *next* window (after addr_shift,
                          VINS.cpp:760-769); 0 for the extrinsic             */
  int32_t block_offset[VIO_MAX_PRIOR_BLOCKS]; /* keep_block_idx - m           */
  double *block_x0;              /* [n_blocks][9] keep_block_data, 7- and
                                    9-sized blocks left-aligned               */
  double *linearized_jacobians;  /* [n][n] row-major                          */
  double *linearized_residuals;  /* [n]                                       */
} VioPrior;

#define VIO_MARGIN_OLD 0        /* VINS.hpp MarginalizationFlag               */
#define VIO_MARGIN_SECOND_NEW 1
#define VIO_MARGIN_NONE 2       /* skip the marginalization step              */

/* One sliding window as solve_ceres sees it after old2new() (VINS.cpp:505).  */
typedef struct VioWindow {
  int32_t window_size; /* W, 1 <= W <= cfg.window_size (VIO_EINVAL below, VIO_ECAP
                          above); the windows of one batch may differ in W: the batch
                          is laid out for its largest, every window solved at its own */
  int32_t n_features;  /* rows of inv_depth in use = getFeatureCount()        */
  int32_t n_factors;   /* M projection factors, grouped by feature in
                          ascending feature order as VINS.cpp:528-567 emits
                          them, loop factors (target == W+1) included          */
  int32_t marginalization_flag; /* VIO_MARGIN_*                                */
  double *pose;        /* [(W+1)][7] para_Pose        in: initial, out: see below */
  double *speed_bias;  /* [(W+1)][9] para_SpeedBias                            */
  double *ex_pose;     /* [7] para_Ex_Pose[0] (constant block)                 */
  double *inv_depth;   /* [n_features] para_Feature                            */
  const int32_t *factor_host;    /* [M] imu_i                                  */
  const int32_t *factor_target;  /* [M] imu_j; W+1 selects loop_pose           */
  const int32_t *factor_feature; /* [M] feature_index                          */
  const double *factor_pts_i;    /* [M][3] */
  const double *factor_pts_j;    /* [M][3] */
  const VioPreintegration *preint; /* [W]; preint[k] links frame k -> k+1
                                      (pre_integrations[k+1], VINS.cpp:516-521) */
  const VioPrior *prior;         /* NULL when last_marginalization_info == nullptr */
  int32_t loop_frame;  /* -1: no loop constraint; else window index i whose
                          pose initialises loop_pose (VINS.cpp:590-596)         */
  double *loop_pose;   /* [7] front_pose.loop_pose, out: optimised              */
  /* new2old() gauge anchor (VINS.cpp:133-155). 0: use pose[0] as passed in.    */
  int32_t use_origin_override;
  double origin_yaw_deg; /* Utility::R2ypr(last_R_old).x()                      */
  double origin_p[3];    /* last_P_old                                          */
  /* outputs --------------------------------------------------------------- */
  /* pose / speed_bias / inv_depth are overwritten with the state after
   * new2old() re-expressed in para_* form (what the second old2new() at
   * VINS.cpp:693 produces). raw_* (optional, may be NULL) receive the arrays
   * exactly as ceres::Solve left them.                                        */
  double *raw_pose;       /* [(W+1)][7] or NULL */
  double *raw_speed_bias; /* [(W+1)][9] or NULL */
  double *raw_inv_depth;  /* [n_features] or NULL */
  VioPrior *next_prior;   /* caller-allocated buffers sized for
                             vio_prior_capacity(W); NULL to skip               */
  /* Device-resident prior chain (vio_backend_reserve_priors). 0: the prior
   * travels through host memory as described above. k >= 1: slot k-1 of the
   * back-end's prior store. Then (a) a `prior` whose three data pointers are
   * NULL names the prior the slot holds (n, n_blocks and the block_* arrays
   * still come from the struct); a `prior` with data pointers is uploaded as
   * usual; (b) the next prior is written into the slot instead of host
   * memory: `next_prior` receives n, n_blocks and the block_* arrays only
   * (its data pointers may be NULL), and the slot is advanced when n > 0.   */
  int32_t resident_prior;
} VioWindow;

#define VIO_MAX_TRACE 64
/* Filled by the solve entries; the it_* slots at index >= iterations are 0 (csrc/solve_trace.h is the one reader of the
 * device trace).                                                              */
typedef struct VioSolveStats {
  double initial_cost;
  double final_cost;     /* summary.final_cost VINS.cpp:660 */
  int32_t iterations;    /* iteration records incl. iteration 0 */
  int32_t termination;   /* 0 NO_CONVERGENCE, 1 CONVERGENCE, 2 FAILURE */
  int32_t num_successful_steps;   /* vio_pnp_*: both counts -1 for a window of constant frames only (Summary's default) */
  int32_t num_unsuccessful_steps;
  /* per-iteration trace (IterationSummary, CS/include/ceres/iteration_callback.h) */
  double it_cost[VIO_MAX_TRACE];
  double it_radius[VIO_MAX_TRACE];
  double it_step_norm[VIO_MAX_TRACE];
  double it_relative_decrease[VIO_MAX_TRACE];
  double it_gradient_max_norm[VIO_MAX_TRACE];
  int32_t it_flags[VIO_MAX_TRACE]; /* bit0 step_is_valid, bit1 step_is_successful */
} VioSolveStats;

/* Upper bound of prior dimension for a window of size W: every pose (6),
 * every speed-bias (9) and the extrinsic (6).                                */
int32_t vio_prior_capacity(int32_t window_size);

/* ------------------------------------------------------------------------- */
/* Back-end                                                                   */
typedef struct vio_backend vio_backend_t;

/* max_batch = number of independent windows one launch may carry.            */
int vio_backend_create(const VioConfig *cfg, int32_t max_batch, vio_backend_t **out);
/* HIP device ordinal the context was created on (see DEVICE BINDING above). */
int vio_backend_get_device(const vio_backend_t *be, int32_t *device);
void vio_backend_destroy(vio_backend_t *be);

/* IntegrationBase(acc_0, gyr_0, ba, bg) followed by n push_back(dt, acc, gyr)
 * (integration_base.h:20-45, VINS.cpp:333-358). Host-side, IMU-rate path.     */
int vio_preintegrate(const VioConfig *cfg, const double acc_0[3], const double gyr_0[3],
                     const double ba[3], const double bg[3], int32_t n,
                     const double *dt, const double *acc, const double *gyr,
                     VioPreintegration *out);

/* solve_ceres(buf_num) for `n` independent windows in one device launch
 * (VINS.cpp:480-831). buf_num only selected a wall-clock budget in the
 * reference (VINS.cpp:648-653); it is accepted and ignored (no time limit, so
 * results are deterministic).                                                */
int vio_backend_solve_windows(vio_backend_t *be, VioWindow *windows, int32_t n,
                              int32_t buf_num, VioSolveStats *stats /* [n] or NULL */);
/* The same for windows of DIFFERENT cameras in one launch: sqrt_info[b] is
 * window b's ProjectionFactor::sqrt_info = FOCUS_LENGTH_X / 1.5 of ITS camera
 * (VINS.cpp:31; setGlobalParam switches the focal length by device,
 * global_param.cpp:24-131), ex_pose is per window already. sqrt_info == NULL:
 * cfg.fx / 1.5 for every window, which is what vio_backend_solve_windows calls
 * this with. An entry that is not finite and > 0 is VIO_EINVAL.               */
int vio_backend_solve_windows_cam(vio_backend_t *be, VioWindow *windows, int32_t n,
                                  const double *sqrt_info /* [n] or NULL */,
                                  VioSolveStats *stats /* [n] or NULL */);

/* Device-resident prior chain. The prior a window leaves behind (the output of
 * marginalize(), VINS.cpp:697-831) is the next window's
 * last_marginalization_info (VINS.cpp:523-528): a caller that chains windows
 * frame after frame only needs its header on the host. This reserves
 * `n_slots` slots of two banks each in device memory (2 x ~46 KB per slot at
 * W=10); VioWindow.resident_prior selects a slot, see there. Reserving again
 * forgets what the slots held. One slot belongs to one chain: two windows of
 * one batch must not name the same slot (VIO_EINVAL).                        */
int vio_backend_reserve_priors(vio_backend_t *be, int32_t n_slots);

/* Resident-batch API for throughput runs: pack + upload once, launch many
 * times from the same initial state, download when wanted. `stream` is a
 * hipStream_t (or NULL for the library's own stream).                        */
int vio_backend_upload(vio_backend_t *be, const VioWindow *windows, int32_t n);
/* vio_backend_upload with a sqrt_info per window, as vio_backend_solve_windows_cam
 * (VINS.cpp:31 per camera); NULL is vio_backend_upload.                       */
int vio_backend_upload_cam(vio_backend_t *be, const VioWindow *windows, int32_t n,
                           const double *sqrt_info /* [n] or NULL */);
int vio_backend_launch(vio_backend_t *be, void *stream);
int vio_backend_sync(vio_backend_t *be);
int vio_backend_download(vio_backend_t *be, VioWindow *windows, int32_t n, VioSolveStats *stats);
/* Average device time (ms) of the solve kernel over the launches since the
 * last call, measured with HIP events on the launch stream.                  */
int vio_backend_kernel_ms(vio_backend_t *be, double *ms_avg, int32_t *launches);
/* Workgroups per window that the last launch gave its large windows (pose
 * matrix in global scratch): 1, 2 or 4. 1 when the launch had none, when the
 * batch did not fit the chip at a larger width, and while the stage clock
 * below is on (it follows one workgroup per window).                         */
int vio_backend_coop_width(const vio_backend_t *be, int32_t *width);

/* Per-stage device cycle counters of the solve kernel: the kernel-side counterpart
 * of the reference's TS()/TE() printf timers (global_param.hpp:85-92, VINS.cpp:657-662,
 * 753-758). Enable before vio_backend_upload; read after a launch. Stage order:
 * setup_imu, setup_prior, eval_prior, eval_imu, eval_proj, scale, schur, rhs,
 * cholesky, tri_solve, quad_form, dogleg, cost_eval, new2old, marg_build,
 * marg_chol, total (shader-clock cycles, thread 0 of the window's workgroup).
 * Asking for more than VIO_N_STAGES entries also returns the finer sub-stage
 * breakdown listed in csrc/spmd.h (Stage enum) / vins-mobile_amd/abi.py. */
#define VIO_N_STAGES 17
int vio_backend_set_profile(vio_backend_t *be, int32_t enable);
int vio_backend_stage_cycles(vio_backend_t *be, int32_t window, int64_t *cycles, int32_t n_stages);

/* ------------------------------------------------------------------------- */
/* Front-end                                                                  */
typedef struct vio_frontend vio_frontend_t;

typedef struct VioObs {      /* one entry of image_msg (feature_tracker.cpp:300-306) */
  int32_t id;
  double x, y, z;            /* ((u-PX)/fx, (v-PY)/fy, 1) */
} VioObs;

typedef struct VioTrackViz { /* good_pts / track_len (UI only), optional */
  float *good_pts;           /* [cap][2] */
  double *track_len;         /* [cap]    */
  int32_t cap;
  int32_t n;
} VioTrackViz;

/* n_seq independent trackers (sequences) share one context and one launch.
 * VIO_EINVAL for configurations the kernels are not laid out for: lk_win != 21,
 * more than 512 corners, images below 32 x 32 or above 32767 rows / 65535
 * columns (corner candidates carry their position as y << 16 | x).
 * Environment, read here: VIO_AMD_DETECT_ALWAYS=1 (measurement aid) runs the
 * corner detector on every published frame of every sequence; by default a
 * sequence that still tracks max_corners features skips it, like the
 * reference's n_max_cnt > 0 test (feature_tracker.cpp:256-266) -- the results
 * are the same either way. VIO_AMD_REDO_REPORT=1 (measurement aid) makes
 * vio_frontend_destroy print on stderr how many sequence-frames had more
 * corner candidates than the detector's lists hold (plateaus of equal
 * eigenvalues) and were redone from a full-size list; the corners are exact
 * either way.                                                                 */
int vio_frontend_create(const VioConfig *cfg, int32_t n_seq, vio_frontend_t **out);
int vio_frontend_get_device(const vio_frontend_t *fe, int32_t *device);
void vio_frontend_destroy(vio_frontend_t *fe);

/* readImage for sequence `seq` (feature_tracker.cpp:162-310). `publish` is the
 * caller's img_cnt == 0 (ViewController.mm:467,494). out_obs has room for
 * cfg->max_corners entries.                                                  */
int vio_frontend_read_image(vio_frontend_t *fe, int32_t seq, const uint8_t *gray,
                            int32_t rows, int32_t cols, int32_t stride, double header,
                            int32_t publish, VioObs *out_obs, int32_t *n_obs,
                            VioTrackViz *viz /* may be NULL */);

/* Batched form: one frame for every sequence in one set of launches.
 * gray = n_seq images, each rows*stride bytes, back to back.                 */
int vio_frontend_read_images(vio_frontend_t *fe, const uint8_t *gray, int32_t rows,
                             int32_t cols, int32_t stride, const double *headers,
                             int32_t publish, VioObs *out_obs /* [n_seq][max_corners] */,
                             int32_t *n_obs /* [n_seq] */);

/* The same in two halves, for callers that overlap the front-end of frame k+1
 * with the estimator of frame k (the app runs readImage and processImage on
 * two threads: ViewController.mm:458 and :688-724). submit gathers the frames,
 * queues the transfer, the kernels and the copy of the observations and returns
 * without waiting for the device; collect waits and hands the observations
 * over. One frame in flight per context: a second submit before collect is
 * VIO_ESTATE, as is collect without submit.                                    */
int vio_frontend_submit_images(vio_frontend_t *fe, const uint8_t *gray, int32_t rows,
                               int32_t cols, int32_t stride, int32_t publish);
/* vio_frontend_submit_images with the submit's own host work (gathering the frames into page-locked memory, queueing
 * transfers and kernels) on a host thread the context owns: returns at once; `gray` must stay valid and unchanged until
 * vio_frontend_collect, which also reports an error of the submit. */
int vio_frontend_submit_images_async(vio_frontend_t *fe, const uint8_t *gray, int32_t rows, int32_t cols, int32_t stride,
                                     int32_t publish);
int vio_frontend_collect(vio_frontend_t *fe, VioObs *out_obs /* [n_seq][max_corners] */,
                         int32_t *n_obs /* [n_seq] */);

/* Frames for a SUBSET of the context's sequences, each with its own publish flag
 * (feature_tracker.cpp:162-310 per sequence): cameras of a server have their own
 * clocks, lose frames and keep their own img_cnt phase (ViewController.mm:467,494).
 * One frame for n of the sequences, any n in 0..n_seq, seq[] in any order without
 * duplicates: sequence seq[i] takes frame i and publish[i]; every other sequence is
 * not touched in any way (its images, points, ids and counters stay as they are).
 * A sequence's first frame after create or reset is the reference's `first image`
 * (pre = cur = forw, :166-167).
 *   frames, frames_on_device = 0: host memory, n images back to back in call order,
 *     rows * stride bytes each (frame_index must be NULL). Frames inside a range
 *     registered with vio_host_register (stride == cols) go to the device by DMA from
 *     where they lie, others through the gather of read_images.
 *   frames_on_device = 1: a packed [slots][rows][cols] device buffer the caller owns
 *     (stride == cols; what vio_preprocess_run_resident writes); frame_index[i] names
 *     the slot of seq[i], NULL = slot i. The caller guarantees the frames are complete
 *     (its producer has finished) before the call.
 * On EVERY route -- pageable host memory, a registered host range, device memory --
 * the frames must stay valid and unchanged until vio_frontend_collect_subset returns.
 * One frame in flight per context, shared with the lock-step submit: a second submit
 * of either kind before the collect is VIO_ESTATE; vio_frontend_collect after
 * submit_subset and vio_frontend_collect_subset after submit_images are VIO_ESTATE
 * (the frame stays in flight). Duplicates or out-of-range entries of seq[], a wrong
 * image size, a negative frame_index or publish == NULL with n > 0 are VIO_EINVAL and
 * change no sequence. n == 0 is VIO_OK and launches nothing.
 * collect_subset: out_obs [n][max_corners] and n_obs [n] in the CALL's order (row i
 * belongs to seq[i]; 0 observations for a sequence that did not publish); the bytes
 * that travel back scale with n, not with n_seq.
 * vio_frontend_kernel_ms also averages the device time of subset calls made with
 * frames_on_device = 1; the counters of vio_frontend_lk_iterations cover the
 * lock-step entry points only.                                                      */
int vio_frontend_submit_subset(vio_frontend_t *fe, int32_t n, const int32_t *seq, const void *frames,
                               int32_t frames_on_device, const int32_t *frame_index /* [n], NULL = i */,
                               int32_t rows, int32_t cols, int32_t stride, const uint8_t *publish /* [n] */);
int vio_frontend_collect_subset(vio_frontend_t *fe, VioObs *out_obs /* [n][max_corners], call order */,
                                int32_t *n_obs /* [n] */);
/* submit_subset + collect_subset */
int vio_frontend_read_subset(vio_frontend_t *fe, int32_t n, const int32_t *seq, const void *frames,
                             int32_t frames_on_device, const int32_t *frame_index, int32_t rows, int32_t cols,
                             int32_t stride, const uint8_t *publish, VioObs *out_obs, int32_t *n_obs);
/* A fresh FeatureTracker (feature_tracker.cpp:162-310: first image, no points, n_id = 0,
 * empty track_cnt) for the n sequences of seq[]; seq == NULL: for all of them. Other
 * sequences are not touched. VIO_ESTATE while a frame is in flight, VIO_EINVAL for
 * duplicates or entries out of range. Waits for the device. The estimator's
 * counterpart is vio_estimator_clear.                                                */
int vio_frontend_reset(vio_frontend_t *fe, int32_t n, const int32_t *seq);
/* *in_step = 1 while every sequence of the context is in the same phase (same pyramid
 * bank, all with or all without an image). The lock-step entry points --
 * read_image(s), submit_images(_async), step_resident -- need that: after subset calls
 * or resets have put the sequences out of phase they return VIO_ESTATE until the
 * sequences are in phase again, which vio_frontend_reset(fe, 0, NULL) always brings
 * about. A context that never calls the subset entries is always in step. The
 * context's resident ring (upload_frames / step_resident) stays lock-step; a subset
 * call on a context whose current image is still read in place from the ring first
 * moves that image into the pyramid's own storage.                                    */
int vio_frontend_in_step(vio_frontend_t *fe, int32_t *in_step);
/* The camera of sequence seq[i] becomes cam[i]: what image_msg divides by,
 * ((u - PX) / FOCUS_LENGTH_X, (v - PY) / FOCUS_LENGTH_Y, 1) (feature_tracker.cpp:300-306),
 * the per-device globals of setGlobalParam (global_param.cpp:24-131). Only fx, fy, cx, cy
 * are used; a sequence without one uses cfg's. It takes effect at the next publish,
 * changes nothing of the tracker's pixel state and survives vio_frontend_reset.
 * VIO_ESTATE between a submit and its collect; VIO_EINVAL for an entry of seq[] out of
 * range or named twice, for fx or fy zero, and for a value that is not finite (no camera
 * is changed then). Waits for the device. get_camera: tic = 0, ric = identity.          */
int vio_frontend_set_cameras(vio_frontend_t *fe, int32_t n, const int32_t *seq /* [n] */, const VioCamera *cam /* [n] */);
int vio_frontend_get_camera(vio_frontend_t *fe, int32_t seq, VioCamera *out);
/* The region of interest of sequence seq[i]: what setMask starts from on a publish
 * frame instead of an all-255 mask (feature_tracker.cpp:50-87; the static mask of the
 * upstream family, FISHEYE_MASK in VINS-Mono's setMask). A tracked feature whose
 * rounded position lies on a 0 pixel is not kept and paints no disc, and
 * goodFeaturesToTrack receives the region minus the discs: its masked maximum and its
 * candidates come from usable pixels only. Frames that do not publish, the list behind
 * vio_frontend_get_pnp_points (it is ahead of setMask) and the rule that skips the
 * detector when max_corners features survive are untouched; a sequence without a region
 * computes what it always did. Uses: the valid region of a rectified wide lens
 * (vio_preprocess_valid_regions_resident), a bonnet, a housing, a burnt-in overlay.
 * masks: n images [rows][cols], nonzero = usable; NULL clears the named sequences.
 * On the host, image i is the region of seq[i] (image mask_index[i] when mask_index is
 * given). masks_on_device = 1: a packed [slots][rows][cols] device buffer (what
 * vio_preprocess_valid_regions_resident writes), mask_index[i] names the slot of seq[i],
 * NULL = slot i; the slots named must exist. The contract of vio_frontend_set_cameras:
 * VIO_ESTATE between a submit and its collect; VIO_EINVAL, and nothing changed, for an
 * entry of seq[] out of range or named twice or a negative mask_index; waits for the
 * device (work queued on a caller's stream included); takes effect at the next publish
 * frame; changes nothing of the tracker's pixel state; survives vio_frontend_reset; the
 * caller's buffer is not referenced after the call returns.
 * get_region: mask_out (may be NULL) receives 0 / 255, all 255 for a sequence without
 * a region (*is_set = 0); *n_usable = the number of usable pixels.                    */
int vio_frontend_set_regions(vio_frontend_t *fe, int32_t n, const int32_t *seq /* [n] */, const void *masks,
                             int32_t masks_on_device, const int32_t *mask_index /* [n] or NULL */);
int vio_frontend_get_region(vio_frontend_t *fe, int32_t seq, uint8_t *mask_out /* [rows][cols], may be NULL */,
                            int32_t *is_set, int64_t *n_usable);

/* Host frame buffers registered once (camera / decoder ring buffers, the cv::Mat
 * storage behind `_img` in FeatureTracker::readImage, feature_tracker.cpp:162):
 * the range is page-locked in place, and read_images / submit_images(_async)
 * whose `gray` lies inside a registered range (with stride == cols) send the
 * frames to the device by DMA from where they are, without the gathering pass
 * through the library's own page-locked staging. Results are the same either
 * way. Process-wide (every context and device sees the registration);
 * overlapping a registered range or unregistering an unknown pointer is
 * VIO_ESTATE, pages that cannot be locked VIO_ENOMEM. Unregister (with the
 * pointer that was registered) before the memory is freed; it waits for the
 * device first.                                                               */
int vio_host_register(void *ptr, size_t bytes);
int vio_host_unregister(void *ptr);

/* Resident form for throughput runs: frames already in HBM.                  */
int vio_frontend_upload_frames(vio_frontend_t *fe, const uint8_t *gray, int32_t n_frames,
                               int32_t rows, int32_t cols, int32_t stride);
int vio_frontend_step_resident(vio_frontend_t *fe, int32_t frame_index, int32_t publish,
                               void *stream);
int vio_frontend_sync(vio_frontend_t *fe);
int vio_frontend_kernel_ms(vio_frontend_t *fe, double *ms_avg, int32_t *launches);

/* The image pre-step of the camera callback, batched on the device
 * (ViewController.mm:432-437): cv::cvtColor(CV_RGBA2GRAY) then CLAHE with
 * clipLimit 3 on the default 8x8 grid; its output is what readImage receives.
 * channels = 4 (RGBA as UIImageToMat delivers it) or 1 (already gray).         */
typedef struct vio_preprocess vio_preprocess_t;
int vio_preprocess_create(int32_t max_frames, int32_t rows, int32_t cols, vio_preprocess_t **out);
void vio_preprocess_destroy(vio_preprocess_t *p);
int vio_preprocess_set_clahe(vio_preprocess_t *p, double clip_limit, int32_t tiles_x, int32_t tiles_y);
/* Host buffers: pixels = n_frames images of rows*stride bytes back to back;
 * equalized_out (and gray_out, may be NULL) = n_frames * rows * cols bytes.    */
int vio_preprocess_run(vio_preprocess_t *p, const uint8_t *pixels, int32_t channels, int32_t n_frames, int32_t stride,
                       uint8_t *gray_out, uint8_t *equalized_out);
/* Resident form: device pointers, asynchronous on `stream` (a hipStream_t, NULL =
 * the context's own); d_equalized is packed [n_frames][rows][cols], ready for
 * vio_frontend_step_resident-style consumers.                                  */
int vio_preprocess_run_resident(vio_preprocess_t *p, const void *d_pixels, int32_t channels, int32_t n_frames,
                                int32_t stride, void *d_equalized, void *stream);
int vio_preprocess_sync(vio_preprocess_t *p);
int vio_preprocess_kernel_ms(vio_preprocess_t *p, double *ms_avg, int32_t *launches);

/* Lens rectification inside the pre-step. A frame slot that holds a lens is
 * rectified to the pinhole rect_* while it is converted to gray: gray_out of
 * vio_preprocess_run is then the RECTIFIED gray, CLAHE runs on it, and
 * everything downstream sees a pinhole image. Per output pixel (x, y), in IEEE
 * doubles, every operation rounded on its own (no fused multiply-add):
 *   xn = (x - rect_cx) / rect_fx,  yn = (y - rect_cy) / rect_fy,  r2 = xn*xn + yn*yn
 *   radial = 1 + r2*(k1 + r2*(k2 + r2*k3))
 *   xd = (xn*radial + (2*p1)*xn*yn) + p2*(r2 + (2*xn)*xn)
 *   yd = (yn*radial + p1*(r2 + (2*yn)*yn)) + ((2*p2)*xn)*yn
 *   u = fx*xd + cx, v = fy*yd + cy, clamped to the raw image (replicate border)
 *   U = rint(32 u), V = rint(32 v)   (ties to even: 1/32-pixel fixed point)
 *   out = integer bilinear blend of the four raw grays around (U, V) / 32,
 *         (top*(32-ay) + bot*ay + 512) >> 10; RGBA is converted at each neighbour.
 * The rectified image has the size of the raw one.                            */
typedef struct VioLens {            /* Brown-Conrady, OpenCV's coefficient order */
  double fx, fy, cx, cy;            /* intrinsics of the RAW image                */
  double k1, k2, p1, p2, k3;
  double rect_fx, rect_fy, rect_cx, rect_cy;  /* pinhole of the rectified image: what VioCamera / cfg take */
} VioLens;
/* slot = position of a frame inside a vio_preprocess_run / _run_resident call,
 * 0 .. max_frames-1 (the sequence, in the throughput deployments). lens[i]
 * goes to slot[i]; lens = NULL clears the named slots. A lens stays until it
 * is replaced or cleared. The call waits for the context's last launch and
 * returns with the lenses in device memory: a later run on any stream sees
 * them. VIO_EINVAL, and nothing changed, for a slot out of range or named
 * twice, a non-finite field, or fx, fy, rect_fx, rect_fy <= 0. Slots without a
 * lens, and a context that never sets one, compute what they always did.      */
int vio_preprocess_set_lenses(vio_preprocess_t *p, int32_t n, const int32_t *slot /* [n] */, const VioLens *lens /* [n] or NULL: clear */);
int vio_preprocess_get_lens(vio_preprocess_t *p, int32_t slot, VioLens *out, int32_t *is_set);
/* The forward model on the host: normalized undistorted points -> raw pixels
 * (not clamped), and its inverse by fixed-point iteration x <- x + (x_d - D(x))
 * from x_d = ((u-cx)/fx, (v-cy)/fy), until a step is below 1e-12 in both
 * coordinates (converged[i] = 1) or 50 rounds have passed (converged[i] = 0). */
int vio_lens_distort_points(const VioLens *lens, const double *xn /* [n][2] normalized */, int32_t n, double *uv /* [n][2] raw px */);
int vio_lens_undistort_points(const VioLens *lens, const double *uv /* [n][2] */, int32_t n, double *xn /* [n][2] */,
                              uint8_t *converged /* [n] or NULL */);
/* Output pixels of a rows x cols frame whose source lies outside the raw image
 * (u outside [0, cols-1] or v outside [0, rows-1]; the kernel clamps these):
 * what a caller looks at when choosing rect_*.                                */
int vio_lens_coverage(const VioLens *lens, int32_t rows, int32_t cols, int64_t *n_outside);

/* Lens models. A slot's lens is one of three forward models; VioLensModel is
 * VioLens with the model named and eight coefficients. Pixel -> (xn, yn), the
 * clamp, rint(32 .), the integer blend and the supersampled form of a slot
 * that also holds a VioSource are those of VioLens above, for every model; so
 * are IEEE doubles, every operation rounded on its own, no contraction.
 *   VIO_LENS_BROWN     the lines above with k1 k2 p1 p2 k3 = k[0..4]
 *   VIO_LENS_RATIONAL  OpenCV's CALIB_RATIONAL_MODEL:
 *     radial = (1 + r2*(k1 + r2*(k2 + r2*k3))) / (1 + r2*(k[5] + r2*(k[6] + r2*k[7])))
 *     xd, yd, u, v as above. With k[5..7] = 0 the divisor is exactly 1: the
 *     bytes of the same VioLens.
 *   VIO_LENS_FISHEYE   cv::fisheye (equidistant, Kannala-Brandt over theta):
 *     r = sqrt(r2), th = atan(r), t2 = th*th
 *     thd = th*(1 + t2*(k[0] + t2*(k[1] + t2*(k[2] + t2*k[3]))))
 *     s = r2 == 0 ? 1 : thd / r
 *     u = fx*(xn*s) + cx, v = fy*(yn*s) + cy
 *     sqrt is the correctly rounded IEEE one. atan is NOT a math library's
 *     (those agree between host and device to an ulp, not to the bit) but the
 *     fixed sequence of + - * / written out at the head of csrc/pre_rectify.h
 *     (lens_atan: four breakpoints 7/16, 11/16, 19/16, 39/16, one division, an
 *     odd polynomial of eleven terms; within 4 ulp of the true value), the
 *     same bits on the host, on the device and in a restatement.              */
#define VIO_LENS_BROWN    0  /* k = k1 k2 p1 p2 k3, k[5..7] = 0: VioLens, byte for byte            */
#define VIO_LENS_RATIONAL 1  /* k = k1 k2 p1 p2 k3 k4 k5 k6, OpenCV's order                        */
#define VIO_LENS_FISHEYE  2  /* k = k1 k2 k3 k4 of cv::fisheye over theta, k[4..7] = 0             */
typedef struct VioLensModel {
  int32_t model, reserved;                 /* reserved = 0 */
  double fx, fy, cx, cy;                   /* raw image */
  double k[8];
  double rect_fx, rect_fy, rect_cx, rect_cy;
} VioLensModel;
/* The contract of vio_preprocess_set_lenses. VIO_EINVAL, and nothing changed,
 * also for an unknown model, reserved != 0, or a coefficient the model does
 * not use that is not 0. A slot holds ONE lens, whichever call set it:
 * vio_preprocess_set_lenses stores its argument as VIO_LENS_BROWN, _get_lens_model
 * reads any slot, and vio_preprocess_get_lens on a slot that holds another model
 * returns VIO_ESTATE and leaves *out and *is_set alone.                        */
int vio_preprocess_set_lens_models(vio_preprocess_t *p, int32_t n, const int32_t *slot /* [n] */, const VioLensModel *lens /* [n] or NULL: clear */);
int vio_preprocess_get_lens_model(vio_preprocess_t *p, int32_t slot, VioLensModel *out, int32_t *is_set);
/* Host only, as vio_lens_*. Undistort: Brown-Conrady and rational by the
 * fixed-point iteration above with the same stopping rule; fisheye by
 * thd = hypot(xd, yd), Newton on th*(1 + ...) = thd from th = thd, at most 50
 * rounds, until a step is below 1e-12, xn = xd * tan(th)/thd (thd = 0: the
 * centre); converged[i] = 0 when it does not settle or th >= pi/2 (such a ray
 * has no pinhole image; xn, yn are then not meaningful). VIO_EINVAL for an
 * unknown model or reserved != 0; undistort also for fx or fy <= 0, coverage
 * for any record vio_preprocess_set_lens_models would refuse.                  */
int vio_lens_model_distort_points(const VioLensModel *lens, const double *xn /* [n][2] */, int32_t n, double *uv /* [n][2] */);
int vio_lens_model_undistort_points(const VioLensModel *lens, const double *uv /* [n][2] */, int32_t n, double *xn /* [n][2] */,
                                    uint8_t *converged /* [n] or NULL */);
int vio_lens_model_coverage(const VioLensModel *lens, int32_t rows, int32_t cols, int64_t *n_outside);

/* Native-size source frames. A frame slot that holds a VioSource takes its
 * frame as the camera or the decoder delivers it (size, row stride, pixel
 * format, range) and the pre-step scales the crop rectangle to the context's
 * rows x cols while it converts to gray; CLAHE and everything downstream see
 * rows x cols as always. Exact integer arithmetic, the same bytes on the
 * device and in csrc/pre_source.h on the host:
 *   gray of a source pixel: RGBA / BGRA (R*4899 + G*9617 + B*1868 + 8192) >> 14;
 *     GRAY8 / NV12 the byte Y, with range = 1 min(255, ((max(Y,16) - 16)*255 + 109) / 219)
 *   no lens in the slot: the exact area average of the crop. gx = gcd(crop_cols, cols),
 *     cw = crop_cols/gx, ow = cols/gx; source column j of the crop covers [j*ow, (j+1)*ow),
 *     output column x covers [x*cw, (x+1)*cw), wx(x, j) = the length of their overlap
 *     (sum over j = cw); rows likewise with ch, oh, wy. S = sum wy*wx*gray, D = cw*ch,
 *     out = (S + D/2) / D: the nearest value, ties upward. A crop of rows x cols has D = 1.
 *   a lens in the slot: VioLens.fx .. k3 refer to the whole delivered frame, rect_* to the
 *     rows x cols output; the crop is not used and source coordinates are clamped to the
 *     whole frame. s = min(4, max(ceil(src.cols/cols), ceil(src.rows/rows))); output pixel
 *     (x, y) is the mean of s*s samples at (x + (2i+1-s)/(2s), y + (2j+1-s)/(2s)), i, j = 0..s-1,
 *     each by the lens arithmetic above (gray / range at each neighbour),
 *     out = (sum + s*s/2) / (s*s). s = 1 is the rectification above, byte for byte.
 * The chroma plane of NV12 is never read.                                      */
#define VIO_PIXEL_GRAY8 1   /* one byte per pixel                                   */
#define VIO_PIXEL_RGBA8 4   /* R in byte 0 (what channels = 4 means)                */
#define VIO_PIXEL_BGRA8 5   /* B in byte 0                                          */
#define VIO_PIXEL_NV12  12  /* plane 0 = luma, rows x stride; the chroma plane is never read */
typedef struct VioSource {
  int32_t format, range;            /* range: 0 full, 1 video (16..235); 1 only with GRAY8 / NV12 */
  int32_t rows, cols, stride;       /* the frame as delivered; stride = bytes per row of plane 0  */
  int32_t crop_x, crop_y, crop_cols, crop_rows;  /* the part that becomes the output image        */
} VioSource;
/* Host only. VIO_EINVAL for: an unknown format; range not 0 / 1, or 1 with RGBA /
 * BGRA; rows or cols outside 1..16384; stride below the bytes of a row, or no
 * multiple of 4 for RGBA / BGRA; a crop that is not inside the frame; crop_cols <
 * cols or crop_rows < rows (no upscaling); crop_cols > 8*cols or crop_rows > 8*rows;
 * 255*cw*ch >= 2^32 (the sums stay in 32 bits; crop one pixel off to avoid it). */
int vio_source_check(const VioSource *s, int32_t rows, int32_t cols);
/* The pinhole of the rows x cols output of a slot without a lens, from the pinhole
 * in[] = fx fy cx cy of the delivered frame: fx' = fx*cols/crop_cols,
 * cx' = (cx - crop_x + 0.5)*cols/crop_cols - 0.5, fy' and cy' likewise with rows.
 * This is what goes into that sequence's VioCamera, or into rect_* of a lens.  */
int vio_source_camera(const VioSource *s, int32_t rows, int32_t cols, const double in[4], double out[4]);
/* Slots as for vio_preprocess_set_lenses, and the same contract: src[i] goes to
 * slot[i], src = NULL clears the named slots, a source stays until it is replaced
 * or cleared; the call waits for the context's last launch and returns with the
 * table in device memory. VIO_EINVAL, and nothing changed, for a slot out of range
 * or named twice or an entry vio_source_check refuses.                           */
int vio_preprocess_set_sources(vio_preprocess_t *p, int32_t n, const int32_t *slot /* [n] */, const VioSource *src /* [n] or NULL: clear */);
int vio_preprocess_get_source(vio_preprocess_t *p, int32_t slot, VioSource *out, int32_t *is_set);
/* Frame i of the call is slot i and lies at pixels[i] (the first byte of its plane
 * 0), each frame where it is: sizes and formats may differ from slot to slot, with
 * and without lenses, in one call and one launch of each of the two kernels. Every
 * slot 0 .. n_frames-1 must hold a source (else VIO_ESTATE, nothing is launched).
 * Outputs are laid out as those of vio_preprocess_run / _run_resident. The host
 * form reads the crop's rows only (the whole plane 0 of a lensed slot). The resident
 * form takes a HOST array of device pointers, which it copies before it returns
 * (asynchronous like _run_resident; RGBA / BGRA pointers 4-byte aligned, else
 * VIO_EINVAL). One-byte formats are read in aligned dwords where the stride is a
 * multiple of 4: up to 3 bytes before the first and after the last pixel a row
 * needs, inside the aligned dword that pixel lies in, are loaded and not used (no
 * further: never another page, never the chroma plane's rows).
 * vio_preprocess_run / _run_resident keep their meaning, frames of
 * rows x cols with `channels`, whether or not sources are set.                   */
int vio_preprocess_run_frames(vio_preprocess_t *p, const void *const *pixels /* [n_frames] host */, int32_t n_frames,
                              uint8_t *gray_out /* may be NULL */, uint8_t *equalized_out);
int vio_preprocess_run_frames_resident(vio_preprocess_t *p, const void *const *d_pixels /* host array of n_frames device pointers */,
                                       int32_t n_frames, void *d_equalized, void *stream);

/* The valid region of a slot: where the rectified image is made of delivered
 * pixels only, none of them the clamp's repeated border. Output pixel (x, y) is
 * INSIDE
 *   lens, no source:  when its un-clamped source (u, v) lies in the rows x cols
 *     raw frame, u in [0, cols-1] and v in [0, rows-1] -- the complement of what
 *     vio_lens_model_coverage counts; a NaN is outside;
 *   lens and source:  when every one of the s*s sample positions lies in the
 *     whole delivered frame (src.cols, src.rows), by the same test;
 *   no lens:          always (a crop is inside its frame).
 * mask[y][x] = 255 where (x, y) and every output pixel within `margin` of it
 * (Chebyshev distance; neighbours outside the image do not count) is INSIDE,
 * else 0. margin = 0 .. 32. Entry i of the call is the mask of slot[i], from the
 * lens and source tables the context holds; one launch for all n slots of
 * mixed models. A mask is static per lens: this is no per-frame call. VIO_EINVAL,
 * and nothing written, for a slot out of range or named twice, a margin out of
 * range or a null pointer. The resident form is asynchronous on `stream` (NULL =
 * the context's own) and copies slot[] before it returns; the host form waits.
 * vio_lens_model_valid_region is the same arithmetic on the host without a
 * context (csrc/pre_source.h, the text the kernel compiles: the same bytes);
 * src may be NULL (the frame has the output's size); VIO_EINVAL also for a lens
 * or a source that the setters would refuse.
 * Not covered: the polynomial models fold back far from the centre, and a
 * folded pixel whose source lands inside the frame counts as inside, as it does
 * in vio_lens_model_coverage.                                                   */
int vio_preprocess_valid_regions(vio_preprocess_t *p, int32_t n, const int32_t *slot /* [n] */, int32_t margin,
                                 uint8_t *masks_out /* host [n][rows][cols] */);
int vio_preprocess_valid_regions_resident(vio_preprocess_t *p, int32_t n, const int32_t *slot /* [n] */, int32_t margin,
                                          void *d_masks /* device [n][rows][cols] */, void *stream);
int vio_lens_model_valid_region(const VioLensModel *lens, const VioSource *src /* may be NULL */, int32_t rows, int32_t cols,
                                int32_t margin, uint8_t *mask /* [rows][cols] */);

/* Introspection of tracker state (cur_pts / ids / track_cnt,
 * feature_tracker.hpp:72-75) for parity tests.                               */
int vio_frontend_get_state(vio_frontend_t *fe, int32_t seq, float *cur_pts /* [cap][2] */,
                           int32_t *ids, int32_t *track_cnt, int32_t cap, int32_t *n);
/* forw_pts / ids at the point of readImage where solveVinsPnP joins them with the
 * solved landmarks (feature_tracker.cpp:207): the last frame's tracked points behind
 * the first findFundamentalMat rejection (:194-205), AHEAD of the publish-frame
 * steps rejectWithF (:235) and setMask (:255), which drop more of them.           */
int vio_frontend_get_pnp_points(vio_frontend_t *fe, int32_t seq, float *forw_pts /* [cap][2] */, int32_t *ids,
                                int32_t cap, int32_t *n);
/* Measured iteration counts of calcOpticalFlowPyrLK's inner loop (the reference passes
 * TermCriteria(COUNT + EPS, 30, 0.01), feature_tracker.cpp:181; how many iterations a
 * level takes is data dependent): enable = 1 / 0 switches the counters of the LK kernel
 * on / off (-1: leave), iterations / visits (may both be NULL) receive, per pyramid level,
 * the iterations run and the (feature, level) visits since the last read and are reset.
 * Diagnostics for the roofline's byte formula (bench.py: roofline_frontend.lk_mean_iterations);
 * with the counters on the kernel adds two atomics per (feature, level).               */
int vio_frontend_lk_iterations(vio_frontend_t *fe, int32_t enable, uint64_t *iterations, uint64_t *visits, int32_t levels_cap);
/* While a frame submitted with vio_frontend_submit_images has not been collected,
 * every other entry point that reads or changes the tracker state or the
 * observation staging (step_resident, get_state, get_pnp_points, set / update /
 * get_tracks, a second submit) returns VIO_ESTATE.                                */

/* The tracker's public fields (feature_tracker.hpp:68-80: pre_pts / cur_pts /
 * forw_pts, ids, track_cnt) of one sequence in and out, and the steps of readImage
 * between the LK call and goodFeaturesToTrack on their own
 * (feature_tracker.cpp:183-205 status && inBorder, reduceVector, F-RANSAC; on
 * publish frames also :235-255 rejectWithF, track_cnt++ and :50-87 setMask), for
 * every sequence of the context. After the update forw_pts / ids / track_cnt
 * hold what the step kept (in setMask's order on publish frames).               */
int vio_frontend_set_tracks(vio_frontend_t *fe, int32_t seq, int32_t n, const float *pre_pts,
                            const float *cur_pts, const float *forw_pts, const int32_t *ids,
                            const int32_t *track_cnt, const uint8_t *lk_status);
int vio_frontend_update_tracks(vio_frontend_t *fe, int32_t publish);
int vio_frontend_get_tracks(vio_frontend_t *fe, int32_t seq, float *forw_pts, int32_t *ids,
                            int32_t *track_cnt, int32_t cap, int32_t *n);

/* Stand-alone operators of the front-end (each is one reference call site),
 * exposed so they can be parity-tested in isolation:
 *   calcOpticalFlowPyrLK  feature_tracker.cpp:181
 *   goodFeaturesToTrack   feature_tracker.cpp:263
 *   findFundamentalMat    feature_tracker.cpp:95,198                          */
int vio_klt_track(const VioConfig *cfg, const uint8_t *prev, const uint8_t *next,
                  int32_t rows, int32_t cols, int32_t stride, const float *prev_pts,
                  int32_t n, float *next_pts, uint8_t *status, float *err);
int vio_good_features(const VioConfig *cfg, const uint8_t *img, const uint8_t *mask,
                      int32_t rows, int32_t cols, int32_t stride, int32_t max_corners,
                      float *corners /* [max_corners][2] */, int32_t *n_corners);
int vio_fundamental_ransac(const VioConfig *cfg, const float *pts1, const float *pts2,
                           int32_t n, uint8_t *inlier_mask);

/* ------------------------------------------------------------------------- */
/* Loop-closure producer, descriptor side:
 *   KeyFrame::searchByDes               loop/keyframe.cpp:161-187
 *   KeyFrame::HammingDis                loop/keyframe.cpp:368-373
 *   KeyFrame::rejectWithF               loop/keyframe.cpp:35-58
 *   KeyFrame::findConnectionWithOldFrame loop/keyframe.cpp:267-273
 * A BRIEF descriptor (BRIEF::bitset, 256 bits) is four uint64_t words, word 0 =
 * bits 0..63. The matcher context is bound to a device like every other
 * context.                                                                     */
typedef struct vio_matcher vio_matcher_t;
int vio_matcher_create(vio_matcher_t **out);
void vio_matcher_destroy(vio_matcher_t *m);
/* searchByDes for n_pairs (current keyframe, old keyframe) pairs in one launch.
 * cur_desc holds the pairs' window descriptors back to back (sum n_cur x 4
 * words), old_desc the old keyframes' descriptors (sum n_old x 4, at most 65535
 * per keyframe). Per query, in the order of cur_desc: best_index = index into
 * that pair's old list of the smallest Hamming distance (first one on ties, as
 * the reference's `dis < bestDist` scan), best_dist = that distance;
 * best_index = -1 / best_dist = 256 when nothing is closer than 256 bits
 * (empty old list).                                                            */
int vio_matcher_search_by_des(vio_matcher_t *m, int32_t n_pairs, const int32_t *n_cur,
                              const int32_t *n_old, const uint64_t *cur_desc,
                              const uint64_t *old_desc, int32_t *best_index,
                              int32_t *best_dist);
/* findConnectionWithOldFrame: searchByDes, matched_old_pts[i] = keypoint of the
 * best old descriptor (pixels), then, from 8 matches on, rejectWithF =
 * findFundamentalMat(cur_pts, matched_old_pts, FM_RANSAC, 2.0, 0.99) ->
 * status[i] (1 = kept), matched_old_norm = (pt - (cx, cy)) / (fx, fy)
 * (optional). Fewer than 8 matches keep everything. cfg is read per call:
 * pass the intrinsics of THAT session's camera (VioCamera).                    */
int vio_loop_find_connection(vio_matcher_t *m, const VioConfig *cfg, int32_t n_cur,
                             const uint64_t *cur_desc, const float *cur_pts /* [n_cur][2] */,
                             int32_t n_old, const uint64_t *old_desc,
                             const float *old_pts /* [n_old][2] */,
                             float *matched_old_pts /* [n_cur][2] */,
                             float *matched_old_norm /* [n_cur][2] or NULL */,
                             uint8_t *status /* [n_cur] */, int32_t *n_inliers);

/* Bag-of-words query (DBoW2 as LoopClosure::startLoopClosure drives it, loop/loop_closure.cpp:20-36 ->
 * TemplatedLoopDetector::detectLoop, loop/TemplatedLoopDetector.h:668-700):
 *   vocabulary file layout             loop/VocabularyBinary.hpp:17-50 (k, L, scoringType, weightingType, nNodes,
 *                                      nWords; Node{nodeId, parentId, weight, descriptor[4]}; Word{nodeId, wordId}),
 *                                      TemplatedVocabulary::loadBin  ThirdParty/DBoW/TemplatedVocabulary.h:1505-1554
 *   TemplatedVocabulary::transform     TemplatedVocabulary.h:1213-1253 (descriptor -> word id, weight),
 *                                      :1061-1117 (descriptors of a keyframe -> BowVector, L1-normalised)
 *   TemplatedDatabase::add / query     ThirdParty/DBoW/TemplatedDatabase.h:439-470, 603-720 (queryL1)
 * Only L1_NORM scoring (scoringType 0, the app's vocabulary) is implemented; other vocabularies are refused with
 * VIO_EINVAL. Contexts are bound to the device current at creation.                                                  */
typedef struct vio_vocabulary vio_vocabulary_t;
int vio_vocabulary_create(const void *blob, size_t bytes, vio_vocabulary_t **out);  /* the file's bytes            */
int vio_vocabulary_load(const char *path, vio_vocabulary_t **out);                  /* TemplatedVocabulary(filename) */
void vio_vocabulary_destroy(vio_vocabulary_t *v);
int vio_vocabulary_info(const vio_vocabulary_t *v, int32_t info[6]);  /* k, L, scoring, weighting, nodes, words */
int vio_vocabulary_get_device(const vio_vocabulary_t *v, int32_t *device);
/* transform for n_keyframes keyframes in one launch. desc: the keyframes' descriptors back to back (sum n_desc x 4
 * words, vio_matcher_* layout; at most 8192 per keyframe). word_id / word_weight (optional): transform(feature, id, w)
 * per descriptor. bow_*: the BowVector of keyframe f in [f * bow_stride, ...): bow_count[f] entries, ascending word id.
 * VIO_ECAP when a keyframe has more distinct words than bow_stride (bow_count[f] = -(needed)).                        */
int vio_vocabulary_transform(vio_vocabulary_t *v, int32_t n_keyframes, const int32_t *n_desc, const uint64_t *desc,
                             int32_t *word_id, double *word_weight, int32_t *bow_count, int32_t *bow_word,
                             double *bow_value, int32_t bow_stride);
/* Vocabulary training: TemplatedVocabulary::create(training_features, k, L, weighting, L1_NORM) for FBrief
 * (ThirdParty/DBoW/TemplatedVocabulary.h:551-580), node by node:
 *   HKmeansStep            :635-812  on a node's descriptor list (original order: image after image, inside an image
 *                          the given order): an empty list makes nothing; n <= k makes one child per descriptor, in
 *                          order; otherwise k-means++ seeds, every descriptor goes to the nearest centre (Hamming
 *                          distance, FIRST centre on ties, :727-738), then centres = meanValue(groups), associate,
 *                          until the association equals the previous one (:748-765). A child is made for every centre,
 *                          empty groups included, and split further while level < L and its group has more than one
 *                          member (:789-811); groups keep their members in list order.
 *   FBrief::meanValue      ThirdParty/DBoW/FBrief.cpp:22-49: bit i is set iff more than floor(N/2) members have it; an
 *                          EMPTY group gives the all-zero descriptor (the reference's comment says it cannot happen; it
 *                          can, after a re-association; the cluster stays and may be re-populated).
 *   initiateClustersKMpp   :827-908: first centre = a uniform index; after each new centre min_dists is updated and
 *                          summed (integers 0..256: the 64-bit sum is exact), cut = random * sum, the next centre is the
 *                          first index whose running sum reaches cut; seeding ends early, with fewer than k centres,
 *                          when the sum is 0.
 *   createWords / setNodeWeights  :913-933, :938-991: node ids in the order the recursion creates them (all children
 *                          of a node consecutively, then the first child's subtree, ...), word ids in node-id order
 *                          over the leaves; weight 1 for TF / BINARY, log(NDocs / Ni) for IDF / TF_IDF where Ni = the
 *                          images in which at least one descriptor TRANSFORMS to the word (the ordinary descent, counted
 *                          on the device; std::log on the host), NDocs counts images without descriptors too, a word
 *                          with Ni = 0 keeps weight 0; inner nodes have weight 0.
 * Two departures from the reference:
 *  1. Random stream. The reference draws from rand() seeded by the clock, in recursion order. Here every draw is a pure
 *     function of `seed` and the node's PATH, so the result does not depend on the order in which nodes are processed:
 *       mix(x)            = splitmix64's step: x += 0x9E3779B97F4A7C15; z = x; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                           z = (z ^ z >> 27) * 0x94D049BB133111EB; result z ^ z >> 31          (64-bit wrap-around)
 *       key(root)         = mix(seed);   key(child c of p) = mix(key(p) ^ (c + 1))             c = 0 .. the child's place
 *       h_j               = mix(key(node) + j * 0x9E3779B97F4A7C15)                             draw j of a node
 *       first centre      = min(n - 1, floor(((h_0 >> 11) * 2^-53) * n))                       one fp64 multiply
 *       centre m >= 1     : cut = (((h_m >> 11) + 1) * 2^-53) * (double)sum                    factor in (0, 1], one fp64
 *                           multiply; the pick is the first index with (double)prefix >= cut
 *  2. Iteration cap. The reference loops without bound, and a deterministic tie rule does not exclude a cycle of
 *     equal-cost states. max_iterations caps the meanValue passes of a node; a node stopped by the cap (its association
 *     after the last allowed pass still differs from the one before; with max_iterations = 0: every node that runs
 *     k-means) keeps its last centres and its last association, which is always computed with those centres, and is
 *     counted in capped_nodes. max_iterations = 0 is seeds plus one association. Default 128: Lloyd passes on binary
 *     descriptors settle within a few tens of passes at every size measured (profiles/vocabulary_train_timing.txt: at
 *     most 32 at 10^6 descriptors), a pass over 10^6 descriptors costs well under a millisecond, so 128 leaves a factor
 *     of four and still bounds a cycle. Values below 0 or above 4096 are refused.
 * Limits: 2 <= k <= 32, 1 <= L <= 10, at most 4 194 304 descriptors and 65 536 per image (VIO_ECAP beyond). VIO_EINVAL
 * for k / L / weighting / max_iterations outside their ranges, a negative count, no descriptor at all; VIO_ENODEV
 * without a device (no CPU fallback). Only L1_NORM scoring.
 * Level-synchronous (csrc/voc_train_core.h): all nodes of a tree level are processed by the same launches.
 * stats.launches counts kernel launches: at most 3 k + 2 iterations_max[level] + 4 per level and 2 for the weights, so
 *   launches <= c0 + c1 * sum over levels of (k + iterations_max[level])       with c0 = 2, c1 = 5.
 * stats: n_nodes without the root (= the file's nNodes); capped_nodes as above; short_nodes = nodes whose k-means++
 * ended below k centres; empty_clusters = children whose final group is empty; iterations_max[l] = most meanValue passes
 * of a node whose children are on level l + 1; kernel_ms = the sum of pass_ms, the time on the stream between the first
 * launch of a pass and the first of the next (seeding, iterations, regrouping, weights), host round trips included.
 * Measured on one MI355X (profiles/vocabulary_train_timing.txt; k = 10, the whole call against the same semantics in plain
 * C++, tools/vocabulary_train_host_route.cpp, on one host thread / on 16): L = 4, 10^5 descriptors 6.1 ms against 245 / 139 ms;
 * L = 6, 10^6 descriptors in 2 000 images 94 ms against 6 587 / 2 145 ms (54 ms of the 94 pass between a level's regrouping and
 * the next pass's first launch: the level's centres come back, the host lays out the tables of 674 k nodes and, after the
 * last level, makes the vocabulary from the file). The device route wins at both sizes: no break-even in that range.
 * The vocabulary that comes back is an ordinary one, bound to the current device.                                   */
typedef struct VioVocabularyTrainParams {
  int32_t k, L;
  int32_t weighting;       /* 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY (WeightingType, as in the file) */
  int32_t max_iterations;
  uint64_t seed;
} VioVocabularyTrainParams;
typedef struct VioVocabularyTrainStats {
  int32_t n_descriptors, n_nodes, n_words, capped_nodes, empty_clusters, short_nodes, launches;
  int32_t iterations_max[16];
  double kernel_ms;
  double pass_ms[4];       /* seeding, iterations, regrouping, weights */
} VioVocabularyTrainStats;
void vio_vocabulary_train_params_default(VioVocabularyTrainParams *p);  /* k 10, L 6, TF_IDF, 128 passes, seed 0 */
/* desc: the images' descriptors back to back, 4 words each (vio_brief_extract's layout); n_desc [n_images].       */
int vio_vocabulary_train(const VioVocabularyTrainParams *p, int32_t n_images, const int32_t *n_desc,
                         const uint64_t *desc, vio_vocabulary_t **out, VioVocabularyTrainStats *stats /* or NULL */);
/* The vocabulary's file (loop/VocabularyBinary.hpp:17-50, what the app's loadBin reads, TemplatedVocabulary.h:
 * 1505-1554). A trained vocabulary gives canonical bytes (nodes in id order, words in id order); a loaded one gives
 * back the bytes it was made from. vio_vocabulary_create(serialize(v)) transforms identically to v. blob == NULL
 * reports the size in *bytes; VIO_ECAP (with the size) when cap is too small.                                        */
int vio_vocabulary_serialize(const vio_vocabulary_t *v, void *blob, size_t cap, size_t *bytes);
int vio_vocabulary_save(const vio_vocabulary_t *v, const char *path);
typedef struct vio_bow_database vio_bow_database_t;
/* The database takes what it needs from the vocabulary (device, word count) at create and
 * owns its stream: it stays valid after vio_vocabulary_destroy, and a vocabulary and its
 * database may be used from two threads at the same time. A vocabulary file whose node
 * records do not form one tree under node 0 (an id twice, a parent cycle) is refused
 * with VIO_EINVAL by vio_vocabulary_create / _load.                                  */
int vio_bow_database_create(vio_vocabulary_t *v, int32_t max_entries, int32_t max_total_words, vio_bow_database_t **out);
void vio_bow_database_destroy(vio_bow_database_t *d);
int vio_bow_database_size(const vio_bow_database_t *d, int32_t *n_entries);
/* TemplatedDatabase::add(BowVector) -> entry id = number of entries before the call.                                  */
int vio_bow_database_add(vio_bow_database_t *d, int32_t n, const int32_t *word, const double *value, int32_t *entry_id);
/* TemplatedDatabase::query(BowVector, ret, max_results, max_id) for n_queries BowVectors in one launch: entries with
 * id < max_id[q] (all if -1) that share a word with the query, best first, at most max_results (all if <= 0);
 * score in [0, 1] = 1 - ||v - w||_1 / 2. Equal scores come out in ascending entry id.                                 */
int vio_bow_database_query(vio_bow_database_t *d, int32_t n_queries, const int32_t *bow_count, const int32_t *bow_word,
                           const double *bow_value, int32_t bow_stride, const int32_t *max_id, int32_t max_results,
                           int32_t *n_results, int32_t *entry, double *score, int32_t result_stride);

/* The loop detector: TemplatedLoopDetector::detectLoop (VINS_ios/loop/TemplatedLoopDetector.h:668-877), the step of
 * the app's loop_thread (VINS_ios/ViewController.mm:929-947, LoopClosure::startLoopClosure) that decides whether the
 * newest keyframe closes a loop and with which old keyframe, for n independent sessions that share one vocabulary:
 *   transform(features, bowvec, featvec, levelsup)  ThirdParty/DBoW/TemplatedVocabulary.h:1121-1189, :1212-1254
 *   TemplatedDatabase::query / add / delete_entry   ThirdParty/DBoW/TemplatedDatabase.h:603-720, 439-470, 476-499
 *   L1Scoring::score (ns_factor)                    ThirdParty/DBoW/ScoringObject.cpp:23-68
 *   removeLowScores :1228-1246, computeIslands :891-965, updateTemporalWindow :982-1017
 *   isGeometricallyConsistent_DI :1056-1144, getMatches_neighratio :1164-1223, checkFoundamental :1031-1053
 *   eraseIndex :1250-1259, clear :882-886
 * The FeatureVector of a keyframe maps the node met at level L - di_levels of the descent (the root when that level is
 * <= 0) to the indices of its descriptors. For a descriptor whose descent ends at a leaf above that level the reference
 * leaves the node unset; here it is the leaf's node id.                                                            */
typedef struct VioLoopDetectorParams {     /* TemplatedLoopDetector::Parameters, TemplatedLoopDetector.h:94-147      */
  int32_t use_nss; float alpha; int32_t k;
  int32_t geom_check;                      /* GeometricalCheck :32-43: 1 GEOM_DI, 3 GEOM_NONE; 0 / 2 are refused     */
  int32_t di_levels;
  int32_t dislocal, max_db_results; float min_nss_factor;
  int32_t min_matches_per_group, max_intragroup_gap, max_distance_between_groups, max_distance_between_queries;
  int32_t min_Fpoints; double max_neighbor_ratio;
  double f_threshold, f_confidence; int32_t min_inliers;  /* checkFoundamental's literals :1036-1047: 1.0, 0.99, "> 20" */
} VioLoopDetectorParams;
/* What the app constructs: Parameters(height, width) = (frequency 1, nss, alpha 0.3f, k 1, GEOM_DI, di_levels 2)
 * (:165-167) + set(frequency) (:525-541, products truncated to int).                                              */
void vio_loop_detector_params_default(VioLoopDetectorParams *p, float frequency);

enum {                                     /* DetectionStatus :46-64                                                 */
  VIO_LOOP_DETECTED = 0, VIO_LOOP_CLOSE_MATCHES_ONLY = 1, VIO_LOOP_NO_DB_RESULTS = 2, VIO_LOOP_LOW_NSS_FACTOR = 3,
  VIO_LOOP_LOW_SCORES = 4, VIO_LOOP_NO_GROUPS = 5, VIO_LOOP_NO_TEMPORAL_CONSISTENCY = 6,
  VIO_LOOP_NO_GEOMETRICAL_CONSISTENCY = 7
};
typedef struct VioLoopDetection {          /* DetectionResult :67-84 + what decided it                               */
  int32_t status;                          /* VIO_LOOP_*                                                             */
  int32_t query, match;                    /* match = -1 where the reference leaves it unset                         */
  double  ns_factor;                       /* 1.0 when not computed                                                  */
  int32_t n_results, n_after_cut;          /* query results; after removeLowScores (0 when the cut was not reached)  */
  int32_t island_first, island_last, island_best_entry;  /* the chosen island; -1 / 0.0 when there is none           */
  double island_score, island_best_score;
  int32_t consistent_entries;              /* m_window.nentries after the call                                       */
  int32_t n_di_matches, n_inliers;         /* geometric check: pairs of the direct-index matcher; pairs RANSAC kept
                                            * (0 when it did not run: fewer than max(min_Fpoints, 8) pairs)          */
} VioLoopDetection;

typedef struct vio_loop_detector vio_loop_detector_t;
/* A detector for n_sessions sessions of at most max_entries keyframes with at most max_keypoints (<= 4096) descriptors
 * each. It copies what it needs from the vocabulary and owns its stream and device memory: it stays valid after
 * vio_vocabulary_destroy. VIO_EINVAL for geom_check other than 1 / 3, di_levels outside 0..L, a vocabulary whose
 * scoring is not L1.                                                                                               */
int  vio_loop_detector_create(vio_vocabulary_t *voc, const VioLoopDetectorParams *p, int32_t n_sessions,
                              int32_t max_entries, int32_t max_keypoints, vio_loop_detector_t **out);
void vio_loop_detector_destroy(vio_loop_detector_t *d);
int  vio_loop_detector_get_device(const vio_loop_detector_t *d, int32_t *device);
/* detectLoop (:668-877) for the newest keyframe of n sessions (each session at most once per call: VIO_EINVAL), one
 * batch of launches. keys [sum n_keys][2] pixels, desc [sum n_keys][4] words (vio_matcher_* layout). cur_pts / old_pts
 * [n][pts_stride][2] (optional): the RANSAC-kept pairs of a VIO_LOOP_DETECTED result in the reference's order
 * (n_inliers each; VIO_EINVAL when pts_stride < max_keypoints). The keyframe's keys, descriptors, BowVector and
 * FeatureVector stay on the device as entry out[i].query of its session. VIO_ECAP (nothing changed) when a keyframe has
 * more than max_keypoints descriptors or a session already holds max_entries.                                       */
int  vio_loop_detector_detect(vio_loop_detector_t *d, int32_t n, const int32_t *session, const int32_t *n_keys,
                              const float *keys, const uint64_t *desc, VioLoopDetection *out,
                              float *cur_pts, float *old_pts, int32_t pts_stride);
/* eraseIndex (:1250-1259) -> TemplatedDatabase::delete_entry: the entries' postings leave the inverted file, their
 * BowVector and FeatureVector are emptied; ids are not reused and vio_loop_detector_size keeps counting. Erasing an
 * entry twice is a no-op; an id outside [0, size) is VIO_EINVAL (nothing erased).                                   */
int  vio_loop_detector_erase(vio_loop_detector_t *d, int32_t session, int32_t n, const int32_t *entries);
int  vio_loop_detector_clear(vio_loop_detector_t *d, int32_t session);   /* clear() :882-886: database + window      */
int  vio_loop_detector_size(const vio_loop_detector_t *d, int32_t session, int32_t *n_entries);
int  vio_loop_detector_kernel_ms(vio_loop_detector_t *d, float *ms);     /* device time of the last detect           */
/* KeyFrame::findConnectionWithOldFrame (loop/keyframe.cpp:267-273: searchByDes :161-190, rejectWithF :35-58; the call
 * at ViewController.mm:946-952) for one (current, old) pair of entries of n sessions in one batch of launches, both
 * keyframes read from the detector's own device copies: no descriptor or keypoint is uploaded. The queries of pair i
 * are the LAST n_window[i] descriptors of entry cur_entry[i] (BriefExtractor appends the window points behind the FAST
 * corners, :401-406; extractBrief takes them from there, :65-70) and their keys are the measurements; the old keyframe
 * is every key and descriptor of old_entry[i]. Semantics of vio_loop_find_connection, bit for bit: the best match is
 * the smallest Hamming distance, the first index on ties; a query with nothing closer than 256 bits means no
 * connection (status all 0, n_kept 0, matched_old_pts not written); from 8 queries on
 * findFundamentalMat(measurements, matched old keys, FM_RANSAC, 2.0, 0.99) decides status; fewer than 8 keep everything
 * and have no normalised points (kept_old_norm not written, connected = 0).
 * Rows of `stride` per pair: status [n_window]; matched_old_pts [n_window][2] pixels (optional); kept_index [n_kept] =
 * the window indices with status 1, ascending (reduceVector :52-56); kept_ids[k] = ids[kept_index[k]] (both NULL or
 * both given); kept_old_norm [n_kept][2] = (double)((matched old key - (cx, cy)) / (fx, fy)) in float as :45-46 --
 * what vio_estimator_set_relocalization takes. VIO_EINVAL, with nothing launched or written: a session twice in one
 * call, an entry outside [0, size), old_entry >= cur_entry, an erased entry, n_window > stride or larger than the
 * current entry's key count.                                                                                       */
typedef struct VioLoopConnection {
  int32_t n_window;    /* queries = window descriptors of the current entry                         */
  int32_t ransac_ran;  /* 1 when rejectWithF ran (n_window >= 8 and every query found a match)      */
  int32_t n_kept;      /* status == 1                                                               */
  int32_t connected;   /* ransac_ran && n_kept > min_loop_num   (ViewController.mm:952)             */
} VioLoopConnection;
int  vio_loop_detector_connect(vio_loop_detector_t *d, const VioConfig *cfg /* fx fy cx cy */,
                               int32_t min_loop_num /* MIN_LOOP_NUM = 22 */, int32_t n, const int32_t *session,
                               const int32_t *cur_entry, const int32_t *old_entry, const int32_t *n_window,
                               const int32_t *ids /* [n][stride] or NULL */, int32_t stride, VioLoopConnection *out,
                               uint8_t *status /* [n][stride] */, float *matched_old_pts /* [n][stride][2] or NULL */,
                               int32_t *kept_index /* [n][stride] */, int32_t *kept_ids /* [n][stride], with ids */,
                               double *kept_old_norm /* [n][stride][2] */);
/* The camera of session[i] becomes cam[i] (only fx, fy, cx, cy are used): what findConnectionWithOldFrame normalises
 * the old keyframe's pixels with, (pt - (PX, PY)) / (FOCUS_LENGTH_X, FOCUS_LENGTH_Y) in float (loop/keyframe.cpp:45-46;
 * per device in the reference, global_param.cpp:24-131). A session with a camera uses it in vio_loop_detector_connect
 * and vio_loop_detector_keyframes in place of the cfg passed to the call; a session without one keeps using that cfg.
 * VIO_EINVAL: a session out of range or named twice, fx or fy zero, a value that is not finite (nothing is changed).
 * get_camera: VIO_ESTATE for a session that has none. The camera outlives vio_loop_detector_clear.                */
int  vio_loop_detector_set_cameras(vio_loop_detector_t *d, int32_t n, const int32_t *session /* [n] */, const VioCamera *cam /* [n] */);
int  vio_loop_detector_get_camera(vio_loop_detector_t *d, int32_t session, VioCamera *out);

/* Keyframe descriptor extraction: BriefExtractor::operator() (loop/keyframe.cpp:395-409) =
 * cv::FAST(im, keys, 20, true); keys += window_pts; DVision::BRIEF::compute
 * (ThirdParty/DVision/BRIEF.cpp:40-105: GaussianBlur 9x9 sigma 2, then n_bits
 * intensity tests im(pt + (x1,y1)) < im(pt + (x2,y2)) per keypoint, a test with
 * an end outside the image leaves its bit 0). The pattern is the app's
 * Resources/brief_pattern.yml (BriefExtractor::BriefExtractor, :375-393).
 * A batch of keyframes per call. keypoints[f] = the FAST corners in cv::FAST's
 * order (at most max_keypoints - n_window[f] are kept: VIO_ECAP says some were
 * cut) followed by the frame's window points; descriptors [f][k][4] words, bit
 * i of a descriptor = bit (i & 63) of word i >> 6 (vio_matcher_* layout).      */
typedef struct vio_brief vio_brief_t;
int vio_brief_load_pattern(const char *yml_path, int32_t *x1, int32_t *y1, int32_t *x2, int32_t *y2, int32_t cap,
                           int32_t *n);
int vio_brief_create(int32_t rows, int32_t cols, int32_t max_frames, int32_t max_keypoints, const int32_t *x1,
                     const int32_t *y1, const int32_t *x2, const int32_t *y2, int32_t n_bits, vio_brief_t **out);
int vio_brief_get_device(const vio_brief_t *b, int32_t *device);
void vio_brief_destroy(vio_brief_t *b);
int vio_brief_extract(vio_brief_t *b, const uint8_t *gray /* [n_frames][rows*cols] */, int32_t n_frames,
                      const float *window_pts /* [n_frames][window_stride][2] */, const int32_t *n_window,
                      int32_t window_stride, int32_t fast_threshold,
                      float *keypoints /* [n_frames][max_keypoints][2] */,
                      uint64_t *descriptors /* [n_frames][max_keypoints][4] */, int32_t *n_fast,
                      int32_t *n_keypoints);
/* The same extraction from frames that are on the device already (extractBrief, loop/keyframe.cpp:61-71, on the image
 * the front end holds): d_frames is a packed device buffer of rows*cols bytes per slot that the caller owns (a ring,
 * e.g. what vio_preprocess_run_resident writes); frame f of the call is slot frame_index[f] (f when NULL; slots may
 * repeat and come in any order). The kernels read the slots in place: no copy of an image is made, slots that follow
 * each other in the call are one launch. window_pts / n_window are host arrays as above. keypoints / descriptors may be
 * NULL: then only the two count arrays come back. Results and return codes are those of vio_brief_extract on the same
 * pixels, bit for bit, the capacity cut and its VIO_ECAP included. VIO_EINVAL, with nothing launched: d_frames is not
 * device memory of the extractor's device (hipPointerGetAttributes) or its allocation does not hold every slot named;
 * a negative slot.
 * One vio_brief_t serves one call at a time (its device arrays hold the results of the last launch): never give the
 * same one to two calls that can overlap, vio_loop_detector_keyframes included.                                    */
int vio_brief_extract_device(vio_brief_t *b, const void *d_frames, const int32_t *frame_index, int32_t n_frames,
                             const float *window_pts, const int32_t *n_window, int32_t window_stride,
                             int32_t fast_threshold, float *keypoints /* or NULL */,
                             uint64_t *descriptors /* or NULL */, int32_t *n_fast, int32_t *n_keypoints);

/* The loop thread's keyframe step in one call (VINS_ios/ViewController.mm:913-975: extractBrief loop/keyframe.cpp:61-71
 * + BriefExtractor :395-409, startLoopClosure, findConnectionWithOldFrame :267-273) for the newest keyframe of n
 * sessions. It does exactly what this sequence does:
 *   1. vio_brief_extract on the n frames (frame i = slot frame_index[i] of `frames`, i when NULL);
 *   2. vio_loop_detector_detect with n_keys = n_keypoints, the keys and descriptors packed back to back;
 *   3. for the sessions with detection.status == VIO_LOOP_DETECTED one vio_loop_detector_connect with cur_entry =
 *      detection.query, old_entry = detection.match and the session's n_window and ids;
 * every field of out[i], every row i of status / matched_old_pts / kept_* ([n][stride]) and cur_pts / old_pts
 * ([n][pts_stride][2]) and the detector's state afterwards are bit for bit that sequence's. Rows of sessions that did not
 * detect are not written. A FAST list that had to be cut is no error here: the cut list is used, fast_cut says so.
 * Data movement: with frames_on_device = 1 no image, key or descriptor crosses the bus in either direction (frames as
 * in vio_brief_extract_device); with 0 `frames` is host memory and goes up once (by DMA from where it lies when the
 * range is registered, vio_host_register). Up go the window points, n_window, ids and the detector's item records;
 * down come the per-frame counts and what detect and connect download. The host waits once for the counts between
 * extraction and detection; the two contexts' streams are ordered by an event.
 * Refused before anything is launched, nothing changed: VIO_EINVAL for b and d on different devices, b's max_keypoints
 * above the detector's, cfg->image_rows / image_cols other than b's rows / cols or a zero fx / fy, a session twice or
 * out of range, n_window[i] > stride, pts_stride < max_keypoints with cur_pts / old_pts given, a frames pointer that
 * fails the device-memory check; VIO_ECAP for n above b's max_frames, n_window above b's max_keypoints, a session
 * that already holds max_entries. A keyframe without corners and window points (n_keys 0) is legal.
 * Measured on one MI355X (tools/loop_keyframes_timing.py, profiles/loop_keyframes_timing.txt; wall time per call, median
 * of 5 with the minimum in brackets; 640x480 keyframes of ~1700 descriptors and ~147 window points, a loop detected and
 * connected in every session), 1 / 64 / 512 sessions per call: device frames 1.39 (1.21) / 2.15 (2.06) / 7.72 (7.32) ms,
 * host frames 1.38 (1.20) / 2.44 (2.38) / 10.46 (10.14) ms, the three calls it replaces 1.50 (1.30) / 2.80 (2.73) /
 * 11.96 (11.62) ms (inside the C calls; the caller's packing between them not counted).                             */
typedef struct VioLoopKeyframe {
  VioLoopDetection  detection;   /* as vio_loop_detector_detect                                                      */
  VioLoopConnection connection;  /* as vio_loop_detector_connect; zeroed unless detection.status == VIO_LOOP_DETECTED */
  int32_t n_fast, n_keys;        /* FAST corners found; descriptors stored (the kept corners + n_window)             */
  int32_t fast_cut;              /* 1: n_fast > max_keypoints - n_window, the cut list was used                      */
} VioLoopKeyframe;
int vio_loop_detector_keyframes(vio_loop_detector_t *d, vio_brief_t *b, const VioConfig *cfg /* fx fy cx cy, image size */,
                                int32_t min_loop_num /* MIN_LOOP_NUM = 22 */, int32_t n, const int32_t *session,
                                const void *frames, int32_t frames_on_device, const int32_t *frame_index /* or NULL */,
                                const float *window_pts /* [n][stride][2] */, const int32_t *n_window,
                                const int32_t *ids /* [n][stride] or NULL */, int32_t stride, int32_t fast_threshold,
                                VioLoopKeyframe *out, uint8_t *status /* [n][stride] */,
                                float *matched_old_pts /* [n][stride][2] or NULL */, int32_t *kept_index /* [n][stride] */,
                                int32_t *kept_ids /* [n][stride], with ids */, double *kept_old_norm /* [n][stride][2] */,
                                float *cur_pts, float *old_pts /* [n][pts_stride][2] or NULL */, int32_t pts_stride);

/* 4-DoF loop pose graph: KeyFrameDatabase::optimize4DoFLoopPoseGraph
 * (VINS_ios/loop/keyfame_database.cpp:140-353). Per keyframe the unknowns are
 * yaw (degrees, AngleLocalParameterization) and translation; pitch and roll of
 * the odometry pose are kept. Edges: FourDOFError (keyfame_database.h:271-313)
 * under HuberLoss(1.0) to up to five preceding kept keyframes (:232-262), and
 * FourDOFWeightError (:315-366, weight 10, no loss) for every loop (:264-285).
 * Solver: Ceres trust region, Levenberg-Marquardt, max_num_iterations = 5
 * (:154-159; DENSE_SCHUR there is an exact linear solve).
 *
 * The graph is given in resample-index order: node k = k-th keyframe from
 * earliest_loop_index on. `skip[k]` = need_resample (:176-198): the keyframe
 * keeps its parameter blocks but gets no edge, so it is not part of the solve
 * and is moved by the drift of the last kept keyframe afterwards (:316-319).   */
typedef struct VioPoseGraph {
  int32_t n_nodes;
  double *t;            /* [n][3] in: origin translation; out: optimized (kept nodes) */
  double *ypr;          /* [n][3] in: R2ypr(origin rotation), degrees; out: [k][0] = optimized yaw */
  int32_t fixed_node;   /* SetParameterBlockConstant: the earliest_loop_index keyframe (:224-228) */
  int32_t n_edges;
  const int32_t *edge_i;   /* first pair of parameter blocks: the earlier / connected keyframe */
  const int32_t *edge_j;   /* second pair: the keyframe the edge was created for */
  const uint8_t *edge_kind; /* 0: sequential (Huber), 1: loop (weighted, no loss) */
  const double *edge_meas; /* [n_edges][6]: t_x, t_y, t_z, relative_yaw, pitch_i, roll_i */
} VioPoseGraph;

/* Keyframe list as optimize4DoFLoopPoseGraph walks it (from earliest_loop_index to cur_index). */
typedef struct VioPoseGraphKeyframe {
  double origin_t[3], origin_r[9]; /* getOriginPose (VIO odometry) */
  double t[3], r[9];               /* getPose (current, drift-corrected) — read by the resampling only */
  int32_t global_index;
  int32_t has_loop, is_looped;
  int32_t loop_index;              /* global_index of the matched old keyframe (has_loop) */
  double loop_info[8];             /* relative_t (0..2), relative_q (3..6), relative_yaw (7) */
} VioPoseGraphKeyframe;

typedef struct vio_posegraph vio_posegraph_t;
/* max_nodes / max_edges bound one graph; n_graphs = graphs one call may carry (one workgroup each). */
int vio_posegraph_create(int32_t max_nodes, int32_t max_edges, int32_t n_graphs, vio_posegraph_t **out);
int vio_posegraph_get_device(const vio_posegraph_t *pg, int32_t *device);
void vio_posegraph_destroy(vio_posegraph_t *pg);
/* The ceres::Solve of :287: n graphs in one launch; t / ypr are updated in place, stats[g] carries the trace.
 * max_iterations is 5 in the reference (:159); values above VIO_MAX_TRACE - 1 are clamped to it.               */
int vio_posegraph_optimize(vio_posegraph_t *pg, VioPoseGraph *graphs, int32_t n, int32_t max_iterations,
                           VioSolveStats *stats);
/* Host side of :166-285: resampling flags and the edge list from a keyframe list (kf[0] = earliest_loop_index,
 * kf[n_kf-1] = cur_index). Arrays are caller-owned: t/ypr [n_kf][3], skip [n_kf], edges up to cap_edges.
 * total_length, max_frame_num, list_size: the database's fields (keyfame_database.cpp:16-17,34,185).          */
int vio_posegraph_build(const VioPoseGraphKeyframe *kf, int32_t n_kf, double total_length, int32_t max_frame_num,
                        int32_t list_size, double *t, double *ypr, uint8_t *skip, int32_t cap_edges,
                        int32_t *edge_i, int32_t *edge_j, uint8_t *edge_kind, double *edge_meas, int32_t *n_edges);
/* Host side of :303-339: poses after the solve (kept keyframes take the optimized pose, skipped ones the drift of
 * the last kept one) and the drift of the current keyframe (yaw_drift, r_drift, t_drift).                      */
int vio_posegraph_apply(const VioPoseGraphKeyframe *kf, int32_t n_kf, const double *t, const double *ypr,
                        const uint8_t *skip, double *out_t /* [n_kf][3] */, double *out_r /* [n_kf][9] */,
                        double *yaw_drift, double *r_drift /* [9] */, double *t_drift /* [3] */);

/* ------------------------------------------------------------------------- */
/* KeyFrameDatabase (VINS_ios/loop/keyfame_database.{h,cpp}) for n_sessions    */
/* independent keyframe lists whose poses stay in device memory. The pose     */
/* graph of optimize4DoFLoopPoseGraph is built on the device from the         */
/* resident list, solved there (the kernel of vio_posegraph_optimize) and     */
/* applied to the list there; per call the host uploads a few scalars per     */
/* session and downloads the drift and the solve statistics. A session may    */
/* appear at most once per call (VIO_EINVAL), as in vio_loop_detector_detect. */
/* Every argument error is found before anything is launched or changed.      */
typedef struct vio_keyframe_db vio_keyframe_db_t;
/* max_keyframes bounds one list (and so one graph); max_frame_num is the reference's 500 (keyfame_database.cpp:16).
 * max_graphs = sessions one optimize call may carry: it sizes the solver's dense scratch, which is
 * 2 x (4 max_keyframes)^2 x 8 bytes per graph (two square matrices of doubles over the unknowns); VIO_ENOMEM when
 * the device does not have that, VIO_ECAP beyond the solver's ~730 keyframes, VIO_ENODEV without a device.       */
int vio_keyframe_db_create(int32_t n_sessions, int32_t max_keyframes, int32_t max_graphs, int32_t max_frame_num,
                           vio_keyframe_db_t **out);
int vio_keyframe_db_get_device(const vio_keyframe_db_t *db, int32_t *device);
void vio_keyframe_db_destroy(vio_keyframe_db_t *db);
/* The constructor's state (keyfame_database.cpp:10-20): empty list, no drift, segment 0, global_index from 0.     */
int vio_keyframe_db_clear(vio_keyframe_db_t *db, int32_t session);
int vio_keyframe_db_size(const vio_keyframe_db_t *db, int32_t session, int32_t *n);
/* KeyFrame::KeyFrame (loop/keyframe.cpp:4-14) + KeyFrameDatabase::add (keyfame_database.cpp:21-42) for one new
 * keyframe of each of n sessions: the origin pose is the pose given, the current pose r_drift P + t_drift,
 * r_drift R; total_length and last_P advance; segment_index = the session's cur_seg_index; global_index = the
 * session's count of adds since clear, never reused (the entry ids of vio_loop_detector_detect count the same
 * way). VIO_ECAP with nothing changed when a session is full.                                                    */
int vio_keyframe_db_add(vio_keyframe_db_t *db, int32_t n, const int32_t *session, const double *header,
                        const double *P /* [n][3] */, const double *R /* [n][9] */, int32_t *global_index_out);
/* max_seg_index++; cur_seg_index = max_seg_index (ViewController.mm:776-777). */
int vio_keyframe_db_new_segment(vio_keyframe_db_t *db, int32_t session);
/* cur_kf->detectLoop(old_index); old_kf->is_looped = 1 (ViewController.mm:969-971, keyframe.cpp:356-360).
 * VIO_EINVAL for unknown or erased indices or old_index >= cur_index.                                            */
int vio_keyframe_db_set_loop(vio_keyframe_db_t *db, int32_t session, int32_t cur_index, int32_t old_index);
/* getKeyframe(index)->getPose for n sessions in one download: what RetriveData.P_old / Q_old are made of
 * (ViewController.mm:946, 955-960). P / R / header may be NULL.                                                  */
int vio_keyframe_db_get_pose(vio_keyframe_db_t *db, int32_t n, const int32_t *session, const int32_t *index,
                             double *P /* [n][3] */, double *R /* [n][9] */, double *header /* [n] */);
/* The per-solved-frame block ViewController.mm:831-873 for n sessions in one launch. (a) loop_kf[i] >= 0 (the
 * front_pose.cur_index of a frame whose header was found in the window): |relative_yaw| > 30 or |relative_t| > 10
 * -> removeLoop (has_loop = 0), otherwise updateLoopConnection: loop_info = t, q (w x y z), yaw. relative_q is
 * x y z w as VioEstimatorStatus gives it. (b) the newest 2 window_size + 1 keyframes are searched for header0
 * (search_cnt > 2 * WINDOW_SIZE breaks after the miss, :870); the one found takes updateOriginPose(P0, R0), and
 * optimize_index_out[i] is its global_index when it has a loop (start_global_optimization), -1 otherwise.        */
int vio_keyframe_db_update(vio_keyframe_db_t *db, int32_t n, const int32_t *session, const int32_t *loop_kf,
                           const double *relative_t /* [n][3] */, const double *relative_q /* [n][4] */,
                           const double *relative_yaw /* [n] */, int32_t window_size, const double *header0 /* [n] */,
                           const double *P0 /* [n][3] */, const double *R0 /* [n][9] */, int32_t *optimize_index_out);
/* optimize4DoFLoopPoseGraph (keyfame_database.cpp:140-356) for n sessions: earliest_loop_index, need_resample,
 * parameter values and edges (:166-291), the solve (:297), the poses of the graph, the drift, the keyframes after
 * cur_index, the segment relabelling and updateVisualization (:301-378), all on the device. max_iterations is 5 in
 * the reference. yaw_drift [n], r_drift [n][9], t_drift [n][3] (loop_correct_r / loop_correct_t) and stats [n] may
 * be NULL. VIO_EINVAL with nothing launched or changed when cur_index is unknown or has no loop (the reference
 * asserts, :148) or a loop inside the range points before earliest_loop_index (asserts, :276-280); VIO_ECAP when
 * n > max_graphs.                                                                                                */
int vio_keyframe_db_optimize(vio_keyframe_db_t *db, int32_t n, const int32_t *session, const int32_t *cur_index,
                             int32_t max_iterations, double *yaw_drift, double *r_drift, double *t_drift,
                             VioSolveStats *stats);
/* resample (keyfame_database.cpp:44-76), with its early return below max_frame_num (n_erased = 0): the list is
 * compacted in order, total_length recomputed (updateVisualization); the erased global_index values come back
 * ascending: what vio_loop_detector_erase takes. cap must hold size - 1 entries (VIO_ECAP, nothing changed).    */
int vio_keyframe_db_resample(vio_keyframe_db_t *db, int32_t session, int32_t *erase_index_out, int32_t cap,
                             int32_t *n_erased);
/* The whole list of a session (kf / header / segment_index may be NULL, cap entries each) for tests and for
 * vio_replay_write_keyframes. state [17]: total_length, last_P [3], yaw_drift, r_drift [9], t_drift [3];
 * index_state [3]: earliest_loop_index, cur_seg_index, max_seg_index.                                            */
int vio_keyframe_db_download(vio_keyframe_db_t *db, int32_t session, VioPoseGraphKeyframe *kf, double *header,
                             int32_t *segment_index, int32_t cap, int32_t *n, double *state, int32_t *index_state);

/* ------------------------------------------------------------------------- */
/* Window bookkeeping around the solve (host side): FeatureManager            */
/* (VINS_ios/feature_manager.hpp:71-103). It decides which landmarks and      */
/* observations become factors of a VioWindow; the window size is a run-time  */
/* parameter (global_param.hpp:28 fixes WINDOW_SIZE = 10).                    */
typedef struct vio_features vio_features_t;

typedef struct VioFeatureInfo { /* FeaturePerId (feature_manager.hpp:47-69), list order */
  int32_t id, start_frame, n_obs, used_num;
  int32_t solve_flag;            /* 0 not solved yet, 1 ok, 2 negative depth (setDepth) */
  int32_t is_outlier, fixed;
  double estimated_depth;        /* -1: not triangulated yet */
} VioFeatureInfo;

int vio_features_create(int32_t window_size, vio_features_t **out);
void vio_features_destroy(vio_features_t *fm);
int vio_features_clear(vio_features_t *fm);                       /* clearState  feature_manager.cpp:315 */
/* addFeatureCheckParallax feature_manager.cpp:103-155. obs = image_msg of one
 * published frame (unique ids; taken in ascending id like the std::map).
 * enough_parallax = its return value (true -> MARGIN_OLD, VINS.cpp:397-400).  */
int vio_features_add_check_parallax(vio_features_t *fm, int32_t frame_count, const VioObs *obs, int32_t n_obs,
                                    int32_t *enough_parallax, int32_t *parallax_num, int32_t *last_track_num);
int vio_features_count(vio_features_t *fm, int32_t *n);           /* getFeatureCount :284 */
int vio_features_get_depth_vector(vio_features_t *fm, double *inv_depth, int32_t cap, int32_t *n); /* :270 */
int vio_features_set_depth(vio_features_t *fm, const double *inv_depth, int32_t n);                /* :300 */
int vio_features_clear_depth(vio_features_t *fm, const double *inv_depth, int32_t n);              /* :176 */
/* triangulate :189-248. Ps [W+1][3], Rs [W+1][9] row-major (body -> world),
 * tic [3], ric [9] row-major (camera -> body).                               */
int vio_features_triangulate(vio_features_t *fm, const double *Ps, const double *Rs, const double tic[3],
                             const double ric[9]);
int vio_features_remove_failures(vio_features_t *fm);             /* :259 */
int vio_features_remove_back(vio_features_t *fm);                 /* :320 */
int vio_features_remove_back_shift_depth(vio_features_t *fm, const double marg_R[9], const double marg_P[3],
                                         const double new_R[9], const double new_P[3]);            /* :250 */
int vio_features_remove_front(vio_features_t *fm, int32_t frame_count);                             /* :343 */
/* The factor enumeration of solve_ceres (VINS.cpp:528-567): fills the factor
 * arrays a VioWindow points to, landmark index = row of the depth vector.     */
int vio_features_export_factors(vio_features_t *fm, int32_t cap_factors, int32_t *host, int32_t *target,
                                int32_t *feature, double *pts_i /* [cap][3] */, double *pts_j /* [cap][3] */,
                                int32_t *n_factors, int32_t *n_features);
/* As above plus the relocalization factors of solve_ceres (VINS.cpp:597-631): landmarks
 * observed in window frame `loop_frame` whose id appears in loop_ids (ascending,
 * RetriveData::features_ids) get one more factor with target W+1 (the loop pose)
 * and pts_j = (loop_xy, 1) (RetriveData::measurements); it closes the landmark's
 * group of factors. loop_frame = -1: no loop.                                  */
int vio_features_export_factors_loop(vio_features_t *fm, int32_t cap_factors, int32_t loop_frame,
                                     const int32_t *loop_ids, const double *loop_xy /* [n_loop][2] */, int32_t n_loop,
                                     int32_t *host, int32_t *target, int32_t *feature, double *pts_i, double *pts_j,
                                     int32_t *n_factors, int32_t *n_features, int32_t *n_loop_factors /* may be NULL */);
/* estimated_depth *= s for the landmarks of the solve (visualInitialAlign VINS.cpp:1079-1085). */
int vio_features_scale_depth(vio_features_t *fm, double s);
/* Introspection: per-landmark records (and, optionally, all observation points
 * [sum n_obs][3]) in list order. cap = 0: only the counts.                   */
int vio_features_dump(vio_features_t *fm, VioFeatureInfo *info, int32_t cap, int32_t *n, double *points,
                      int32_t cap_points, int32_t *n_points);
/* The inverse of vio_features_dump: the list becomes exactly these entries (list order; points [sum n_obs][3]). Used
 * when a sequence's list returns from the device-resident store (vio_estimator_set_resident). */
int vio_features_load(vio_features_t *fm, const VioFeatureInfo *info, int32_t n, const double *points);
/* KeyFrame::buildKeyFrameFeatures (loop/keyframe.cpp:128-155, called at ViewController.mm:818) on a landmark list, as
 * written and in list order: used_num = n_obs for every landmark; a landmark is kept iff n_obs >= 2 && start_frame <
 * W - 2 (:133) and then start_frame + n_obs >= W - 1 && n_obs >= 3 (:136). For a kept one, p = obs[W - 2 - start_frame]:
 * px = (float)(fx p.x / p.z + cx), (float)(fy p.y / p.z + cy) (measurements); norm = (float)(p.x / p.z), (float)(p.y /
 * p.z) (pts_normalize); ids = feature_id; cloud = Rs[start] (ric (obs[0] estimated_depth) + tic) + Ps[start]
 * (point_clouds). No test of the depth's sign or of solve_flag: the reference has none. Ps [W+1][3], Rs [W+1][9] are
 * the states of the moment (vio_estimator_get_window). The call writes used_num and nothing else of the list.
 * VIO_ECAP with *n = -(needed) when more than cap landmarks qualify (the first cap are written).
 * cfg, tic and ric are read per call: pass the camera of THAT sequence (VioCamera).                                  */
int vio_features_keyframe(vio_features_t *fm, const VioConfig *cfg /* fx fy cx cy */, const double *Ps, const double *Rs,
                          const double tic[3], const double ric[9], int32_t cap, int32_t *ids, float *px /* [cap][2] */,
                          float *norm /* [cap][2] */, double *cloud /* [cap][3] */, int32_t *n);

/* failureDetection VINS.cpp:214-265 on the newest frame after a solve (the
 * failure_hand switch of the UI stays with the caller). reasons: bit mask.    */
#define VIO_FAIL_FEW_FEATURES 1   /* f_manager.last_track_num < 4              */
#define VIO_FAIL_GYR_BIAS 2       /* |Bgs[W]| > 1                              */
#define VIO_FAIL_TRANSLATION 4    /* |Ps[W] - last_P| > 1                      */
#define VIO_FAIL_Z_TRANSLATION 8  /* |Ps[W].z - last_P.z| > 0.5                */
#define VIO_FAIL_ROTATION 16      /* angle(Rs[W]^T last_R) > 40 "degrees"      */
int vio_failure_detection(int32_t last_track_num, const double Bg_newest[3], const double P_newest[3],
                          const double R_newest[9], const double last_P[3], const double last_R[9],
                          int32_t *reasons);

/* ------------------------------------------------------------------------- */
/* Estimator: class VINS after initialisation (VINS.hpp:47-200), host side, for
 * n_seq independent sequences whose window solves share ONE device launch.
 * processIMU VINS.cpp:333-375, processImage :377-478, old2new/new2old :89-212,
 * the relocalization bookkeeping :571-637,664-680, failureDetection :214-265,
 * slideWindow :1149-1273, clearState :36-81. solveInitial (:833-1145) is not
 * part of it: the caller hands the window states over instead
 * (vio_estimator_set_initial_state) and the branches after it are the
 * reference's (first solve, final_cost > 200 -> back to INITIAL).              */
typedef struct vio_estimator vio_estimator_t;

#define VIO_SOLVER_INITIAL 0      /* VINS::SolverFlag (VINS.hpp:60-64) */
#define VIO_SOLVER_NON_LINEAR 1

#define VIO_FRAME_SKIPPED 0      /* sequence not active in this call                               */
#define VIO_FRAME_FILLING 1      /* window not full yet: frame_count++            VINS.cpp:448-452 */
#define VIO_FRAME_WAIT_INIT 2    /* window full, no initial state: slid, no solve VINS.cpp:443-446 */
#define VIO_FRAME_INIT_FAILED 3  /* first solve ended with final_cost > 200       VINS.cpp:415-424 */
#define VIO_FRAME_SOLVED 4       /* solve_ceres + slideWindow                                      */
#define VIO_FRAME_FAILURE 5      /* failureDetection fired: state cleared         VINS.cpp:462-467 */
#define VIO_FRAME_RESET 6        /* track_num < 20 with a full INITIAL window     VINS.cpp:408-412 */
#define VIO_FRAME_ERROR 7        /* capacity / argument error for this sequence, see .error        */

typedef struct VioFrameResult {
  int32_t action;               /* VIO_FRAME_*                                   */
  int32_t error;                /* VIO_E* when action == VIO_FRAME_ERROR          */
  int32_t marginalization_flag; /* VIO_MARGIN_OLD = the frame is a keyframe       */
  int32_t failure_reasons;      /* VIO_FAIL_* mask                                */
  int32_t track_num;            /* f_manager.last_track_num                       */
  int32_t n_features, n_factors, n_loop_factors;
  VioSolveStats stats;          /* valid when a solve ran                         */
} VioFrameResult;

typedef struct VioEstimatorStatus {
  int32_t frame_count, solver_flag, marginalization_flag, failure_occur;
  int32_t prior_rows;           /* rows of last_marginalization_info (0: none)    */
  double final_cost;
  double r_drift[9], t_drift[3];                 /* VINS.hpp r_drift / t_drift    */
  double relative_t[3], relative_q[4], relative_yaw, loop_pose[7]; /* front_pose  */
  int32_t resident;             /* 1: the landmark list lives in the device store */
  int32_t init_device_count;    /* solveInitial runs whose bundle adjustment ran on the device (set_init_device) */
} VioEstimatorStatus;

/* tic [3], ric [9] row-major: the camera-to-body extrinsic (TIC_*, RIC_*).     */
int vio_estimator_create(const VioConfig *cfg, int32_t n_seq, const double tic[3], const double ric[9],
                         vio_estimator_t **out);
void vio_estimator_destroy(vio_estimator_t *est);
int vio_estimator_clear(vio_estimator_t *est, int32_t seq);   /* clearState + the constructor's r_drift / t_drift */
/* The camera of ONE sequence: what setGlobalParam switches per device model (FOCUS_LENGTH_X/Y, PX, PY, TIC_*, RIC_*:
 * global_param.cpp:24-131) and VINS reads as globals (VINS.cpp:31 sqrt_info, :36-81 clearState, the triangulation, the
 * start-up's gyroscope hint and alignment, slideWindowOld, buildKeyFrameFeatures). A sequence uses cfg.fx .. cfg.cy and
 * the tic / ric of vio_estimator_create until one is set; get returns what it uses. Allowed only while the sequence holds
 * no frame -- after create or vio_estimator_clear, frame_count == 0 -- VIO_ESTATE otherwise: a window is built with one
 * camera. VIO_EINVAL for a value that is not finite, fx <= 0 (sqrt_info = fx / 1.5 is a weight), fy zero, or a ric that
 * is not orthonormal to 1e-6 with determinant +1. The camera survives vio_estimator_clear and every clearState inside process_images.                 */
int vio_estimator_set_camera(vio_estimator_t *est, int32_t seq, const VioCamera *cam);
int vio_estimator_get_camera(vio_estimator_t *est, int32_t seq, VioCamera *out);
/* solveInitial (VINS.cpp:833-1145) inside process_image when the window is full and no
 * state was handed over: relative pose, global SfM, PnP of the in-between frames,
 * visual-inertial alignment. Off by default (0): the caller hands states over.
 * 1: relativePose as the reference computes it (vio_init_relative_pose_mode 0: five-point
 * RANSAC; a frame on which it draws a non-physical root fails and the next frame retries,
 * VINS.cpp:893-901); 2: the fit over all correspondences with the gyroscope's rotation as
 * tie-breaker (mode 1: succeeds on the first frame with enough parallax, planar scenes
 * included).                                                                      */
int vio_estimator_enable_initialization(vio_estimator_t *est, int32_t enable);
/* Where solveInitial's bundle adjustment (the "full BA" of GlobalSFM::construct, inital_sfm.cpp:229-296) runs. 0 (default):
 * on the host, inside each sequence's phase of process_images. 1: relativePose and construct() up to the bundle adjustment
 * run on the host pool, the bundle adjustments of ALL sequences that got this far in the call go to the device in one
 * vio_init_ba_solve launch, and the rest of solveInitial continues on the pool. Every failure branch acts as before
 * (VINS.cpp:893-917). A problem beyond the context's capacity (cfg.max_features point_ok landmarks, cfg.max_factors +
 * cfg.max_features observations) or of more than 16 frames (WINDOW_SIZE above 15) takes the host route. vio_init_ba_solve
 * itself takes VIO_INIT_BA_MAX_FRAMES = 32 frames; the estimator keeps the bound of 16 until an estimator of a larger window
 * initialises on the host route in a replay the two routes can be compared on (the synthetic ones end in
 * VIO_FRAME_INIT_FAILED at WINDOW_SIZE 16 and 20 on either route). The context is created at the first such call and lives as
 * long as the estimator; VioEstimatorStatus.init_device_count counts the device-route runs. Measured on an MI355X
 * (profiles/init_ba_timing.txt, init_ba_timing_large.txt): one problem is faster on the host (6 ms against 9-10 ms at 21 and 31
 * frames); the device call overtakes a 16-thread host pool from 64 problems per launch (12-13 ms against 26-28 ms; 256: 19-20 ms
 * against 97-101 ms). Off by default either way.
 * 2: the pool keeps only the landmark dump, relativePose's scan (correspondence counts, parallax test, gyroscope hint; with
 * vio_estimator_enable_initialization(est, 1) the five-point relative pose as well, passed in with relative_mode 0) and the
 * lists of the frames outside the window; relative pose fit, construct() with its bundle adjustment and the PnP of those frames
 * (VINS.cpp:926-1003) of ALL sequences that got this far run in one vio_init_sfm_solve; alignment and the first window follow
 * on the pool. Failure branches, the 16-frame gate, the capacity fallback (also beyond 4 (WINDOW_SIZE + 1) frames outside the
 * window) and init_device_count as for 1; where the context cannot be created or a launch fails the host route takes over.
 * Measured on an MI355X (profiles/init_sfm_timing.txt: 11 frames, 150 correspondences, 210 landmarks, 9 extra frames): one
 * problem is twice as slow on the device (7.7 ms against 3.5 ms), the routes are even at 64 problems per call (71 ms
 * against 68 ms on a 16-thread pool), at 512 the device call takes 190 ms against 424 ms. Other values: VIO_EINVAL.        */
int vio_estimator_set_init_device(vio_estimator_t *est, int32_t enable);
int vio_estimator_process_imu(vio_estimator_t *est, int32_t seq, double dt, const double acc[3],
                              const double gyr[3]);                                /* processIMU */
/* processIMU for all sequences in one call (spread over host threads): sequence q
 * gets n_samples[q] <= stride samples dt[q*stride + i], acc/gyr[(q*stride + i)*3]. */
int vio_estimator_process_imu_batch(vio_estimator_t *est, const int32_t *n_samples, int32_t stride, const double *dt,
                                    const double *acc, const double *gyr);
/* The states solveInitial would leave for the W+1 frames with these headers
 * (Ps [W+1][3], Rs [W+1][9], Vs, Bas, Bgs [W+1][3]); consumed by the next
 * process_image that finds the window full with exactly these headers.        */
int vio_estimator_set_initial_state(vio_estimator_t *est, int32_t seq, const double *headers, const double *Ps,
                                    const double *Rs, const double *Vs, const double *Bas, const double *Bgs);
/* retrive_pose_data = ... (ViewController.mm:964): the old keyframe matched to the
 * window frame with this header; ids ascending; n = 0 withdraws it.            */
int vio_estimator_set_relocalization(vio_estimator_t *est, int32_t seq, double header, const double P_old[3],
                                     const double Q_old[4] /* x y z w */, const int32_t *ids,
                                     const double *xy /* [n][2] */, int32_t n);
/* processImage of one published frame for every active sequence (active NULL =
 * all). obs of sequence q starts at obs + q*obs_stride and has n_obs[q] entries.
 * The window solves of all sequences go to the device in one launch.          */
int vio_estimator_process_images(vio_estimator_t *est, const VioObs *obs, const int32_t *n_obs, int32_t obs_stride,
                                 const double *headers, const uint8_t *active, VioFrameResult *results /* [n_seq] */);
int vio_estimator_process_image(vio_estimator_t *est, int32_t seq, const VioObs *obs, int32_t n_obs, double header,
                                VioFrameResult *result);
int vio_estimator_get_status(vio_estimator_t *est, int32_t seq, VioEstimatorStatus *st);
/* Ps/Rs/Vs/Bas/Bgs/Headers of the window (any pointer may be NULL).            */
int vio_estimator_get_window(vio_estimator_t *est, int32_t seq, double *Ps, double *Rs, double *Vs, double *Bas,
                             double *Bgs, double *headers);
/* update_loop_correction VINS.cpp:302-331: r_drift * Ps + t_drift, r_drift * Rs. */
int vio_estimator_get_corrected_window(vio_estimator_t *est, int32_t seq, double *correct_Ps, double *correct_Rs);
/* globalLoopThread hands the pose graph's drift to the estimator: vins.t_drift = loop_correct_t; vins.r_drift =
 * loop_correct_r (ViewController.mm:998-999). Only the two fields that get_status and get_corrected_window read
 * are written; vio_estimator_clear puts the identity back (VINS.cpp:19-20).      */
int vio_estimator_set_drift(vio_estimator_t *est, int32_t seq, const double *r_drift /* [9] */,
                            const double *t_drift /* [3] */);
/* Wall time (ms) of the last process_image(s) call by phase: bookkeeping before
 * the solve, vio_backend_solve_windows (pack, upload, kernel, download), and
 * the bookkeeping after it.                                                    */
int vio_estimator_get_timing(vio_estimator_t *est, double ms[3]);
/* The sequence's landmark store (owned by the estimator), for introspection.   */
/* Device-resident landmark stores (on by default; 0 or VIO_AMD_RESIDENT=0 turn them off): a sequence that has reached the
 * NON_LINEAR state keeps its landmark list, its pre-integration blocks and its prior in device memory; per frame the host
 * sends the observations and the propagated window states (about 12 KB instead of about 125 KB per window), kernels do
 * addFeatureCheckParallax / triangulate / the factor list / setDepth / the slide (feature_manager.cpp:103-372), and the
 * results are the host path's bit for bit (relocalization factors included). Sequences use the host-side list while they
 * initialize, for a frame with more observations (or a relocalization frame with more matched ids) than a store slot takes,
 * and when vio_estimator_features() asks for the list. */
int vio_estimator_set_resident(vio_estimator_t *est, int32_t enable);
int vio_estimator_features(vio_estimator_t *est, int32_t seq, vio_features_t **fm);
/* vio_features_keyframe for n sequences (each at most once per call: VIO_EINVAL) with the states the estimator holds
 * now -- what vio_estimator_get_window returns, the moment ViewController.mm:791-822 builds a keyframe. Rows of `stride`
 * per sequence: ids [n][stride], px / norm [n][stride][2], cloud [n][stride][3], count [n]. A sequence whose list is in
 * the device store is served there (a fourth pass of the store kernels: all such sequences of a back-end group share one
 * launch and one download) and STAYS resident: nothing is fetched, VioEstimatorStatus.resident is still 1. A sequence
 * on the host-side list goes through vio_features_keyframe. count[i] = -1 for a sequence that is not NON_LINEAR with a
 * full window; count[i] = -(needed), and VIO_ECAP after the others have been filled, where stride is too small.     */
int vio_estimator_keyframe_features(vio_estimator_t *est, int32_t n, const int32_t *seq, int32_t stride, int32_t *ids,
                                    float *px, float *norm, double *cloud, int32_t *count);

/* ------------------------------------------------------------------------- */
/* Motion-only window of the front-end: vinsPnP (vins_pnp.hpp:45-91), the 30 Hz
 * pose the tracker can compute between two back-end solves
 * (FeatureTracker::solveVinsPnP feature_tracker.cpp:107-160, called from readImage
 * :207; USE_PNP is off by default, ViewController.mm:144).                       */
#define VIO_PNP_MAX_FRAMES 8   /* PNP_SIZE + 1 = 7 in the reference (global_param.hpp) */
typedef struct VioPnpWindow {  /* vinsPnP::solve_ceres vins_pnp.cpp:264-341 after old2new() */
  int32_t n_frames;            /* PNP_SIZE + 1                                         */
  double *pose;                /* [n][7] para_Pose   in: initial, out: solved          */
  double *speed;               /* [n][3] para_Speed                                    */
  const double *bias;          /* [n][6] para_Bias (Ba, Bg): constant blocks           */
  const uint8_t *fixed;        /* [n] find_solved: pose and speed constant (:279-284)  */
  const double *ex_pose;       /* [7] para_Ex_Pose[0], constant                        */
  const VioPreintegration *preint; /* [n-1]; preint[k] links frame k -> k+1            */
  const int32_t *feat_start;   /* [n+1] frame k owns factors feat_start[k..k+1)        */
  const double *observation;   /* [M][2] IMG_MSG_LOCAL::observation                    */
  const double *position;      /* [M][3] IMG_MSG_LOCAL::position (fixed 3D point)      */
  const int32_t *track_num;    /* [M]    IMG_MSG_LOCAL::track_num (weight / 10)        */
} VioPnpWindow;
typedef struct vio_pnp vio_pnp_t;
int vio_pnp_create(const VioConfig *cfg, int32_t max_batch, vio_pnp_t **out);
void vio_pnp_destroy(vio_pnp_t *p);
/* n independent windows in one device launch (one workgroup each).              */
int vio_pnp_solve_windows(vio_pnp_t *p, VioPnpWindow *windows, int32_t n, VioSolveStats *stats /* [n] or NULL */);
/* The same for windows of different cameras in one launch: sqrt_info[b] is window b's
 * PerspectiveFactor::sqrt_info = FOCUS_LENGTH_X / 1.5 of its camera (vins_pnp.cpp:19,
 * global_param.cpp:24-131); ex_pose is per window already. NULL: cfg.fx / 1.5 for all,
 * which is vio_pnp_solve_windows. An entry that is not finite and > 0 is VIO_EINVAL. */
int vio_pnp_solve_windows_cam(vio_pnp_t *p, VioPnpWindow *windows, int32_t n, const double *sqrt_info /* [n] or NULL */,
                              VioSolveStats *stats /* [n] or NULL */);
int vio_pnp_kernel_ms(vio_pnp_t *p, double *ms_avg, int32_t *launches);

/* The vinsPnP object around that solve (vins_pnp.cpp:16-382), n_seq sequences sharing one launch; what
 * FeatureTracker::solveVinsPnP drives inside readImage (feature_tracker.cpp:107-160).                   */
typedef struct VioPnpFeature {  /* IMG_MSG_LOCAL vins_pnp.hpp:36-41; lists ascending in id */
  int32_t id;
  double observation[2];        /* ((forw_pts.x - PX) / fx, (forw_pts.y - PY) / fy) feature_tracker.cpp:131 */
  double position[3];           /* the landmark as the back-end solved it (world frame)   */
  int32_t track_num;
} VioPnpFeature;
typedef struct VioVinsResult {  /* VINS_RESULT vins_pnp.hpp:27-34: the newest back-end state */
  double header;
  double Ba[3], Bg[3], P[3], R[9], V[3];
} VioVinsResult;
typedef struct vio_pnp_tracker vio_pnp_tracker_t;
int vio_pnp_tracker_create(const VioConfig *cfg, int32_t n_seq, int32_t pnp_size /* PNP_SIZE = 6 */, const double tic[3],
                           const double ric[9], vio_pnp_tracker_t **out);
void vio_pnp_tracker_destroy(vio_pnp_tracker_t *t);
int vio_pnp_tracker_clear(vio_pnp_tracker_t *t, int32_t seq);                                       /* clearState */
/* The camera of one sequence, as vio_estimator_set_camera: the extrinsic of its windows (para_Ex_Pose, vins_pnp.cpp:94-135)
 * and the focal length of PerspectiveFactor::sqrt_info (vins_pnp.cpp:19; global_param.cpp:24-131). Only on a cleared
 * sequence (frame_count == 0), VIO_ESTATE otherwise; the same argument checks; it survives vio_pnp_tracker_clear.   */
int vio_pnp_tracker_set_camera(vio_pnp_tracker_t *t, int32_t seq, const VioCamera *cam);
int vio_pnp_tracker_get_camera(vio_pnp_tracker_t *t, int32_t seq, VioCamera *out);
int vio_pnp_tracker_set_init(vio_pnp_tracker_t *t, int32_t seq, const VioVinsResult *r);           /* setInit    */
int vio_pnp_tracker_process_imu(vio_pnp_tracker_t *t, int32_t seq, double dt, const double acc[3], const double gyr[3]);
/* processImage(feature_msg, header, use_pnp) for every active sequence; P_out [n_seq][3] / R_out [n_seq][9] =
 * Ps / Rs[PNP_SIZE - 1] as solveVinsPnP returns them; solved[q] = 1 when a solve ran for sequence q.       */
int vio_pnp_tracker_process_images(vio_pnp_tracker_t *t, const VioPnpFeature *features, const int32_t *n_features,
                                   int32_t stride, const double *headers, int32_t use_pnp, const uint8_t *active,
                                   double *P_out, double *R_out, int32_t *solved);
/* feature_msg of solveVinsPnP (feature_tracker.cpp:121-134): solved landmarks (id, position, track_num; ascending id)
 * joined by id with the tracker's current ids / pixel positions (vio_frontend_get_state); observation =
 * ((x - PX) / fx, (y - PY) / fy). cfg is read per call: pass the intrinsics of THAT sequence's camera.       */
int vio_pnp_match_features(const VioConfig *cfg, const int32_t *ids, const float *forw_pts /* [n_pts][2] */, int32_t n_pts,
                           const VioPnpFeature *solved, int32_t n_solved, VioPnpFeature *out, int32_t cap, int32_t *n_out);
int vio_pnp_tracker_get_window(vio_pnp_tracker_t *t, int32_t seq, double *Ps, double *Rs, double *Vs, double *headers,
                               uint8_t *find_solved, int32_t *frame_count);

/* ------------------------------------------------------------------------- */
/* Initialisation pieces (host side, one-off): VINS::solveInitial VINS.cpp:833-1145.
 * Exposed one by one so that each can be tested against its reference.         */
typedef struct VioInitFrame {  /* ImageFrame initial_aligment.hpp:24-39            */
  double header;
  double R[9];                 /* body attitude in the SfM frame (Q[i] * ric^T)   */
  double T[3];                 /* camera position in the SfM frame, unknown scale  */
  int32_t is_key_frame;
  int32_t n_samples;           /* IMU samples from the previous frame to this one  */
  const double *dt, *acc, *gyr; /* [n_samples], [n_samples][3], [n_samples][3]      */
  double acc_0[3], gyr_0[3];   /* the sample the interval starts from              */
} VioInitFrame;
/* VisualIMUAlignment initial_aligment.cpp:223-229 (solveGyroscopeBias, SolveScale,
 * RefineGravity). Bgs [(W+1)][3] in/out (+= delta_bg); g [3] out; x out =
 * [n_frames][3] body-frame velocities followed by the metric scale; ok = its
 * return value.                                                                */
int vio_visual_imu_alignment(const VioConfig *cfg, const double tic[3], const VioInitFrame *frames, int32_t n_frames,
                             int32_t window_size, double *Bgs, double g[3], double *x, int32_t *ok);

/* solveRelativeRT motion_estimator.cpp:200-236: pose of the second camera in the first
 * (R [9], unit t [3]) from n >= 9 normalized correspondences xy0/xy1 [n][2];
 * inliers = points in front of both cameras, ok = inliers > 10.                */
/* R_hint (may be NULL): roughly known rotation of the second camera in the first (e.g.
 * gyroscope), used only to pick between the two exact solutions of a planar scene. */
int vio_init_relative_pose(const double *xy0, const double *xy1, int32_t n, const double *R_hint /* [9] or NULL */,
                           double R[9], double t[3], int32_t *inliers, int32_t *ok);
/* The two routes to the relative pose. mode 0 = the reference's: cv::findEssentialMat(ll, rr)
 * (five-point minimal solver inside RANSAC, RNG((uint64)-1), threshold 1.0, confidence 0.999)
 * followed by cv::recoverPose's cheirality count, restated from OpenCV 3.0.0
 * (csrc/vio_fivepoint.cpp; parity unpinned: OpenCV is not in the tree). With these arguments the
 * threshold accepts every correspondence, so the result is the first essential matrix of the
 * first random sample -- whether it is the physical one is chance, in the reference too; its
 * caller retries on the next frame. mode 1 = vio_init_relative_pose's fit over all
 * correspondences (rotation hint for planar scenes).                                   */
int vio_init_relative_pose_mode(const double *xy0, const double *xy1, int32_t n, int32_t mode, const double *R_hint,
                                double R[9], double t[3], int32_t *inliers, int32_t *ok);
/* EMEstimatorCallback::runKernel (OpenCV 3.0.0 calib3d/five-point.cpp): the essential matrices
 * (row-major, unit Frobenius norm, x2^T E x1 = 0) of five correspondences
 * xy0 / xy1 [5][2]; E [10][9], n_models <= 10.                                          */
int vio_init_five_point(const double *xy0, const double *xy1, double *E, int32_t *n_models);
/* cv::recoverPose(E, points1, points2, R, t) with focal 1, pp (0, 0): the (R, t) of the four
 * decompositions of E (x2 ~ R x1 + t) with the most triangulated points in front of both
 * cameras and closer than 50; inliers = that count.                                     */
int vio_init_recover_pose(const double E[9], const double *xy0, const double *xy1, int32_t n, double R[9], double t[3],
                          int32_t *inliers);
/* cv::solvePnP(..., useExtrinsicGuess = true) with K = I as inital_sfm.cpp:57 and
 * VINS.cpp:982 call it: refines world->camera R [9], t [3] in place.            */
int vio_init_pnp(const double *pts3, const double *pts2, int32_t n, double R[9], double t[3], int32_t *ok);
/* GlobalSFM::triangulatePoint inital_sfm.cpp:5-21: linear two-view triangulation.
 * pose0 / pose1: 3x4 row-major [R | t], world -> camera; xy: normalized image
 * coordinates; point = the null vector of the 4x4 design matrix, dehomogenised. */
int vio_init_triangulate_point(const double pose0[12], const double pose1[12], const double xy0[2], const double xy1[2],
                               double point[3]);
/* The "full BA" that closes GlobalSFM::construct, inital_sfm.cpp:229-296: ceres
 * problem over c_rotation [frame_num][4] (w x y z, QuaternionParameterization),
 * c_translation [frame_num][3] (both world -> camera) and the points with
 * point_ok != 0; frame l's rotation and the translations of frames l and
 * frame_num-1 are constant; ReprojectionError3D residuals (inital_sfm.hpp:25-54),
 * DENSE_SCHUR, Levenberg-Marquardt with the Solver's default options. In/out:
 * c_rotation, c_translation, points. stats (may be NULL): the Solver::Summary
 * fields and the per-iteration trace. ok = CONVERGENCE || final_cost < 3e-3
 * (:279), the value construct() returns.                                        */
int vio_init_bundle_adjust(int32_t frame_num, int32_t l, double *c_rotation, double *c_translation, int32_t n_points,
                           double *points, const uint8_t *point_ok, const int32_t *feat_start, const int32_t *obs_frame,
                           const double *obs_xy, VioSolveStats *stats, int32_t *ok);
/* GlobalSFM::construct inital_sfm.cpp:117-316. Landmark j has observations
 * obs_frame/obs_xy[feat_start[j] .. feat_start[j+1]) (frame index, normalized xy).
 * Out: q [frame_num][4] (x y z w) and T [frame_num][3] = camera poses in frame l's
 * camera frame, points [n_features][3] with point_ok flags.                     */
int vio_init_sfm(int32_t frame_num, int32_t l, const double relative_R[9], const double relative_T[3], int32_t n_features,
                 const int32_t *feat_start, const int32_t *obs_frame, const double *obs_xy, double *q, double *T,
                 double *points, uint8_t *point_ok, int32_t *ok);

/* That bundle adjustment (inital_sfm.cpp:229-296) for n independent problems in one
 * device launch, one workgroup per problem: the arithmetic of vio_init_bundle_adjust
 * iterate by iterate (trust_region_minimizer.cc loop, Levenberg-Marquardt, the points
 * eliminated as 3x3 blocks, LLT of the reduced camera matrix), every sum in an order
 * the problem fixes: a problem gives the same bits alone and in any slot of any batch.
 * The reduced camera matrix lives in LDS, in one of two layouts chosen by the problem's
 * OWN frame count. Up to 16 frames (the reference's WINDOW_SIZE + 1 is 11): the full
 * square, 256 work-items, two workgroups per compute unit. 17 to VIO_INIT_BA_MAX_FRAMES
 * frames (windows up to WINDOW_SIZE 31): the packed lower triangle (139 128 B at 32
 * frames), 512 work-items, one workgroup per compute unit, the diagonal camera blocks and
 * the landmark state in global memory. A landmark's frames are kept in one 32-bit word,
 * which sets the bound. vio_init_ba_solve sends a mixed batch as two launches on the
 * context's stream, the problems of up to 16 frames first, so the guarantee above holds
 * across the boundary as well: a 31-frame problem gives the same bits alone, twice in a
 * row and next to 11-frame problems, and an 11-frame problem the bits it gave when 16 was
 * the bound. (The two layouts sum a block reduction over 4 and over 8 waves: one problem
 * forced through both gives results that agree to rounding, not to the bit.)          */
#define VIO_INIT_BA_MAX_FRAMES 32
typedef struct vio_init_ba vio_init_ba_t;
typedef struct VioInitBaProblem {   /* the arguments of one vio_init_bundle_adjust call  */
  int32_t frame_num, l, n_points;
  double *c_rotation;               /* [frame_num][4] w x y z, in/out                    */
  double *c_translation;            /* [frame_num][3], in/out                            */
  double *points;                   /* [n_points][3], in/out where point_ok              */
  const uint8_t *point_ok;          /* [n_points]                                        */
  const int32_t *feat_start;        /* [n_points + 1]                                    */
  const int32_t *obs_frame;         /* [feat_start[n_points]]                            */
  const double *obs_xy;             /* [feat_start[n_points]][2]                         */
  int32_t ok;                       /* out: CONVERGENCE || final_cost < 3e-3 (:279)      */
} VioInitBaProblem;
/* Capacities: problems per launch, frames, point_ok landmarks and their observations per
 * problem. max_frames up to VIO_INIT_BA_MAX_FRAMES = 32; a context created for more than
 * 16 frames takes problems of both layouts. Device memory follows the largest launch so
 * far. VIO_ENODEV without a device; VIO_ECAP for max_frames > VIO_INIT_BA_MAX_FRAMES.   */
int vio_init_ba_create(int32_t max_batch, int32_t max_frames, int32_t max_points, int32_t max_obs, vio_init_ba_t **out);
void vio_init_ba_destroy(vio_init_ba_t *c);
int vio_init_ba_get_device(const vio_init_ba_t *c, int32_t *device);
/* Everything is checked on the host before anything is written or sent: VIO_EINVAL where
 * vio_init_bundle_adjust returns it (and for a feat_start that is negative or descends);
 * VIO_ECAP for n > max_batch, a problem beyond the capacities, or a landmark with two
 * observations in one frame (the reference's per-frame observation lists cannot hold
 * one). In either case no array of any problem has been touched. n = 0 is VIO_OK.       */
int vio_init_ba_solve(vio_init_ba_t *c, VioInitBaProblem *problems, int32_t n, VioSolveStats *stats /* [n] or NULL */);
/* Average kernel time over the launches since the last call. A solve counts one launch per
 * layout present in its batch: two for a batch that holds problems on both sides of 16 frames. */
int vio_init_ba_kernel_ms(vio_init_ba_t *c, double *ms_avg, int32_t *launches);

/* Everything solveInitial does between the landmark dump and the alignment, for n independent
 * start-ups in one call: relativePose's fit (motion_estimator.cpp:200-236, as
 * vio_init_relative_pose restates it), GlobalSFM::construct (inital_sfm.cpp:117-316: PnP chain,
 * triangulations, the full BA above, the inversion) and the PnP of the frames outside the
 * window (VINS.cpp:926-1003). Three device stages on one stream around one upload and one
 * download: the head (one workgroup per problem: the fit when relative_mode = 1, then
 * construct's steps 1-4, written straight into the bundle adjustment's batch), the bundle
 * adjustment kernels of vio_init_ba_solve (both layouts, by frame count), the tail (one
 * workgroup per problem and per extra frame). The head and the tail form every
 * floating-point result with the host code's operations in the host code's order (sums over
 * correspondences and landmarks in ascending index, no atomics), sin / cos / acos correctly
 * rounded: up to the bundle adjustment the results are the host route's. A problem whose
 * head fails runs no bundle adjustment iteration. A problem gives the same bits alone, in any
 * slot of any batch, next to failing problems and run after run.                           */
#define VIO_INIT_SFM_OK 0
#define VIO_INIT_SFM_FAIL_RELATIVE 1 /* solveRelativeRT: fewer than 9 correspondences or inliers <= 10   */
#define VIO_INIT_SFM_FAIL_CHAIN 2    /* construct: a forward frame of the PnP chain (inital_sfm.cpp:47)  */
#define VIO_INIT_SFM_FAIL_BA 3       /* "vision only BA not converge" (:279)                             */
#define VIO_INIT_SFM_FAIL_PNP 4      /* an extra frame: fewer than 6 points or solvePnP (VINS.cpp:975-990) */
typedef struct vio_init_sfm vio_init_sfm_t;
typedef struct VioInitSfmProblem {
  /* in: the arguments of vio_init_sfm */
  int32_t frame_num, l, n_features;
  const int32_t *feat_start, *obs_frame;
  const double *obs_xy;
  int32_t relative_mode;     /* 0: relative_R / relative_T are inputs (vio_init_sfm); 1: fitted on the device from the
                                features seen in both frame l and frame_num-1, in list order (vio_init_relative_pose) */
  const double *R_hint;      /* [9] or NULL, mode 1 only */
  /* in: frames outside the window, placed by PnP after the bundle adjustment (VINS.cpp:926-1003) */
  int32_t n_extra;
  const int32_t *extra_guess;    /* [n_extra] window frame whose pose is the guess */
  const int32_t *extra_start;    /* [n_extra+1] */
  const int32_t *extra_feature;  /* landmark index; landmarks seen fewer than twice are skipped (not tracked) */
  const double *extra_xy;
  /* out */
  int32_t status;            /* VIO_INIT_SFM_OK, _FAIL_RELATIVE (ok = 0), _FAIL_CHAIN (construct's PnP chain),
                                _FAIL_BA, _FAIL_PNP (an extra frame) */
  int32_t inliers;           /* mode 1 */
  double relative_R[9], relative_T[3];  /* mode 1: written when the fit ran (9 correspondences or more) */
  double *q, *T;             /* as vio_init_sfm; written when status is _OK or _FAIL_PNP */
  double *points;            /* as vio_init_sfm; written whenever the head succeeded (status not _FAIL_RELATIVE /
                                _FAIL_CHAIN), for the landmarks with point_ok; may be NULL */
  uint8_t *point_ok;         /* written whenever the head succeeded; may be NULL */
  double *extra_R, *extra_T; /* [n_extra][9], [n_extra][3]: as vio_init_pnp leaves them, for the frames whose PnP ran */
} VioInitSfmProblem;
/* Capacities: problems per call, frames (up to VIO_INIT_BA_MAX_FRAMES), landmarks seen at least
 * twice and their observations per problem, extra frames per problem.                       */
int vio_init_sfm_create(int32_t max_batch, int32_t max_frames, int32_t max_points, int32_t max_obs, int32_t max_extra,
                        vio_init_sfm_t **out);
void vio_init_sfm_destroy(vio_init_sfm_t *c);
int vio_init_sfm_get_device(const vio_init_sfm_t *c, int32_t *device);
/* Everything is checked on the host before anything is written or sent: VIO_EINVAL for null or
 * descending arrays, frame or landmark indices out of range, l outside [0, frame_num - 2],
 * relative_mode other than 0 / 1; VIO_ECAP for n > max_batch, a problem beyond a capacity, a
 * landmark seen twice in one frame. In either case no output of any problem has been touched.
 * n = 0 is VIO_OK. ba_stats [n] (may be NULL): the bundle adjustment's summary and trace
 * (zeros for a problem whose head failed).                                                  */
int vio_init_sfm_solve(vio_init_sfm_t *c, VioInitSfmProblem *problems, int32_t n, VioSolveStats *ba_stats /* [n] or NULL */);
/* Device time per stage (head, bundle adjustment, extra-frame PnP), summed over the launches
 * since the last call; launches counts them (three per layout present in a batch).          */
int vio_init_sfm_kernel_ms(vio_init_sfm_t *c, double ms[3] /* head, bundle adjustment, extra-frame PnP */, int32_t *launches);
/* What the head left for the bundle adjustment of problem `index` of the last solve (a
 * diagnostic: one small copy from the device): c_rotation [frame_num][4] (w x y z),
 * c_translation [frame_num][3], points [n_features][3] where point_ok. VIO_ESTATE when that
 * problem's head failed or no solve has run.                                                */
int vio_init_sfm_head_state(vio_init_sfm_t *c, int32_t index, double *c_rotation, double *c_translation, double *points);

/* ------------------------------------------------------------------------- */
/* Replay I/O: the record / playback formats of the app and the IMU-image
 * association of its estimator thread (host side; PNG through the image's zlib). */
typedef struct VioImuMsg {     /* IMU_MSG ViewController.h:58-62 (56 bytes)      */
  double header;
  double acc[3];
  double gyr[3];
} VioImuMsg;

typedef struct VioKeyframeData { /* KEYFRAME_DATA loop/keyfame_database.h:22-27  */
  double header;
  double translation[3];
  double rotation[4];            /* Eigen::Quaterniond coefficient order x y z w */
} VioKeyframeData;

/* "IMU" file: back-to-back IMU_MSG, closed by a header == 0 record
 * (ViewController.mm:1120-1150,1505-1511,1614-1622). cap = 0: count only.      */
int vio_replay_read_imu(const char *path, VioImuMsg *out, int32_t cap, int32_t *n);
int vio_replay_write_imu(const char *path, const VioImuMsg *msgs, int32_t n);
/* "IMAGE_TIME/<index>": 8-byte timestamp; "IMAGE/<index>": PNG
 * (ViewController.mm:1634-1708). read_image returns the gray frame the camera
 * callback feeds the tracker before CLAHE: cv::cvtColor CV_RGBA2GRAY
 * (ViewController.mm:432-433); cap = bytes available in gray (VIO_ECAP with
 * rows/cols set when too small).                                               */
int vio_replay_read_image_time(const char *dir, uint64_t index, double *header);
int vio_replay_write_image_time(const char *dir, uint64_t index, double header);
int vio_replay_read_image(const char *dir, uint64_t index, uint8_t *gray, int64_t cap, int32_t *rows, int32_t *cols);
int vio_replay_decode_png_gray(const uint8_t *png, int64_t png_bytes, uint8_t *gray, int64_t cap, int32_t *rows,
                               int32_t *cols);
/* channels 1 (gray), 3 (RGB) or 4 (RGBA, what UIImagePNGRepresentation stores). */
int vio_replay_write_image(const char *dir, uint64_t index, const uint8_t *pixels, int32_t rows, int32_t cols,
                           int32_t channels);
int vio_replay_rgba_to_gray(const uint8_t *rgba, int32_t rows, int32_t cols, int32_t stride, uint8_t *gray);
/* Pose log: back-to-back KEYFRAME_DATA records.                                */
int vio_replay_read_keyframes(const char *path, VioKeyframeData *out, int32_t cap, int32_t *n);
int vio_replay_write_keyframes(const char *path, const VioKeyframeData *kf, int32_t n);

/* getMeasurements + send_imu (ViewController.mm:603-682): queue IMU samples and
 * published image_msg lists as they arrive; each call to _next hands out one
 * (IMU batch with header <= image header, image) pair in the reference's order,
 * with the dt send_imu would pass to processIMU. available = 0: wait for more.  */
typedef struct vio_measurements vio_measurements_t;
int vio_measurements_create(vio_measurements_t **out);
void vio_measurements_destroy(vio_measurements_t *q);
int vio_measurements_push_imu(vio_measurements_t *q, const VioImuMsg *msg);
int vio_measurements_push_image(vio_measurements_t *q, double header, const VioObs *obs, int32_t n_obs);
int vio_measurements_next(vio_measurements_t *q, VioImuMsg *imu, double *dt /* may be NULL */, int32_t cap_imu,
                          int32_t *n_imu, double *header, VioObs *obs, int32_t cap_obs, int32_t *n_obs,
                          int32_t *available);

const char *vio_version(void);
/* The HIP runtime(s) mapped into the calling process (files named libamdhip64*
 * in /proc/self/maps), ';'-separated, and their number. The library binds to
 * the copy the process loaded first (next to PyTorch: the one bundled with the
 * wheel). With more than one copy mapped the device contexts refuse to start
 * (VIO_ENODEV, both paths on stderr): each copy would keep its own device state. */
int vio_hip_runtime(char *path, int32_t cap, int32_t *n_runtimes);
/* Width (threads, the caller's included) of the process-wide host pool that spreads per-sequence host work
 * (window packing, IMU feeds, observation gathers: csrc/vio_pool.h) and the number of such pools. (None in the
 * reference: one sequence per phone.) Sized from the CPUs the process may run on, its cgroup CPU quota and -- one
 * process per GPU on a node -- divided by LOCAL_WORLD_SIZE; VIO_AMD_HOST_THREADS overrides. A launcher that is
 * not torchrun sets one of the two per rank. Creates the pools on first use. */
int vio_host_pool_width(int32_t *n_pools /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* VIO_AMD_H */
