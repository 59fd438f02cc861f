"""Host-side mirror of the reference's front-end entry point for batches of independent sequences.

`FeatureTracker.read_images(frames, publish)` is FeatureTracker::readImage (VINS_ios/feature_tracker.cpp:162-310) for
one frame of every sequence in one set of device launches; it returns the image_msg of each sequence (id, x, y, z)
when `publish` (the caller's img_cnt == 0, ViewController.mm:467,494). Tracker state (cur/pre/forw points, ids,
track_cnt, n_id) lives on the device between calls, like the reference object's fields.

All compute happens in csrc/libvio_amd.so (HIP, gfx950). There is no CPU path here.
"""
import ctypes as C

import numpy as np

from . import abi

_u8p, _fp, _ip = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32)


_OBS_DTYPE = np.dtype({"names": ["id", "x", "y", "z"], "formats": ["<i4", "<f8", "<f8", "<f8"],
                       "offsets": [0, 8, 16, 24], "itemsize": 32})
assert C.sizeof(abi.VioObs) == 32


class TrackerError(RuntimeError):
    """A front-end call that did not return VIO_OK; `rc` is the code (abi.VIO_EINVAL, abi.VIO_ESTATE, ...)."""

    def __init__(self, what, rc):
        super().__init__("%s failed rc=%d" % (what, rc))
        self.rc = rc


class FeatureTracker:
    def __init__(self, cfg=None, n_seq=1):
        self.lib = abi.load_product()
        self.cfg = cfg if cfg is not None else abi.default_config()
        self.n_seq = n_seq
        self._h = C.c_void_p()
        rc = self.lib.vio_frontend_create(C.byref(self.cfg), n_seq, C.byref(self._h))
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_frontend_create failed rc=%d (a gfx950 device is required)" % rc)
        self._frames = None

    def close(self):
        if self._h:
            self.lib.vio_frontend_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _check(rc, what):
        if rc != abi.VIO_OK:
            raise TrackerError(what, rc)

    def device(self):
        """HIP device the tracker's contexts live on (vio_frontend_get_device)."""
        d = C.c_int32(-1)
        self._check(self.lib.vio_frontend_get_device(self._h, C.byref(d)), "get_device")
        return d.value

    def read_images(self, frames, publish):
        """frames: uint8 [n_seq, rows, cols]. Returns a list (per sequence) of (ids int32[n], xyz float64[n,3])."""
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.shape == (self.n_seq, self.cfg.image_rows, self.cfg.image_cols), frames.shape
        cap = self.cfg.max_corners
        obs = np.zeros(self.n_seq * cap, _OBS_DTYPE)      # VioObs records, read back without per-element ctypes access
        n_obs = np.zeros(self.n_seq, np.int32)
        self._check(self.lib.vio_frontend_read_images(self._h, frames.ctypes.data_as(_u8p), frames.shape[1], frames.shape[2],
                                                      frames.shape[2], None, 1 if publish else 0,
                                                      C.cast(obs.ctypes.data, C.POINTER(abi.VioObs)), n_obs.ctypes.data_as(_ip)),
                    "read_images")
        obs = obs.reshape(self.n_seq, cap)
        out = []
        for s in range(self.n_seq):
            o = obs[s, :int(n_obs[s])]
            out.append((o["id"].copy(), np.stack([o["x"], o["y"], o["z"]], axis=1)))
        return out

    def register_host(self, array):
        """vio_host_register on a numpy buffer of frames: read_images / submit of frames inside it skip the gathering pass."""
        assert array.flags["C_CONTIGUOUS"]
        self._check(self.lib.vio_host_register(C.c_void_p(array.ctypes.data), array.nbytes), "host_register")

    def unregister_host(self, array):
        self._check(self.lib.vio_host_unregister(C.c_void_p(array.ctypes.data)), "host_unregister")

    def submit(self, frames, publish, asynchronous=False):
        """vio_frontend_submit_images (asynchronous: ..._async, the submit's host work on the context's own thread; the frame
        buffer is kept alive here until collect)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.shape == (self.n_seq, self.cfg.image_rows, self.cfg.image_cols), frames.shape
        self._pending_frames = frames
        fn = self.lib.vio_frontend_submit_images_async if asynchronous else self.lib.vio_frontend_submit_images
        rc = fn(self._h, frames.ctypes.data_as(_u8p), frames.shape[1], frames.shape[2], frames.shape[2], 1 if publish else 0)
        if rc != abi.VIO_OK:
            self._pending_frames = None
        self._check(rc, "submit_images")

    def collect(self):
        """vio_frontend_collect -> the list read_images returns."""
        cap = self.cfg.max_corners
        obs = np.zeros(self.n_seq * cap, _OBS_DTYPE)
        n_obs = np.zeros(self.n_seq, np.int32)
        rc = self.lib.vio_frontend_collect(self._h, C.cast(obs.ctypes.data, C.POINTER(abi.VioObs)), n_obs.ctypes.data_as(_ip))
        self._pending_frames = None
        self._check(rc, "collect")
        obs = obs.reshape(self.n_seq, cap)
        out = []
        for s in range(self.n_seq):
            o = obs[s, :int(n_obs[s])]
            out.append((o["id"].copy(), np.stack([o["x"], o["y"], o["z"]], axis=1)))
        return out

    # ---- frames for a subset of the sequences (asynchronous cameras): per-sequence publish, reset ----------------------
    def _subset_args(self, seqs, frames, publish, frame_index):
        seqs = np.ascontiguousarray(seqs, np.int32).reshape(-1)
        n = len(seqs)
        publish = np.ascontiguousarray(np.broadcast_to(np.asarray(publish, np.uint8), (n,)))
        fi = None if frame_index is None else np.ascontiguousarray(frame_index, np.int32).reshape(-1)
        assert fi is None or len(fi) == n
        if isinstance(frames, int):  # a device pointer: packed [slots][rows][cols]
            ptr, on_dev, rows, cols, keep = C.c_void_p(frames), 1, self.cfg.image_rows, self.cfg.image_cols, None
        else:
            keep = frames if (isinstance(frames, np.ndarray) and frames.dtype == np.uint8 and frames.flags["C_CONTIGUOUS"]) \
                else np.ascontiguousarray(frames, np.uint8)
            assert keep.ndim == 3 and keep.shape[0] >= n, keep.shape
            ptr, on_dev, rows, cols = C.c_void_p(keep.ctypes.data), 0, keep.shape[1], keep.shape[2]
        return (n, seqs, publish, fi, keep), (self._h, n, seqs.ctypes.data_as(_ip), ptr, on_dev,
                                              fi.ctypes.data_as(_ip) if fi is not None else None, rows, cols, cols,
                                              publish.ctypes.data_as(_u8p))

    def submit_subset(self, seqs, frames, publish, frame_index=None):
        """vio_frontend_submit_subset: frame i for sequence seqs[i] with publish[i] (one flag or one per sequence). frames:
        uint8 [n, rows, cols] on the host (taken where it lies when C-contiguous, so a registered range is used in place), or
        an int device pointer to packed [slots, rows, cols] frames, frame_index naming the slots. Kept alive until collect."""
        keep, args = self._subset_args(seqs, frames, publish, frame_index)
        rc = self.lib.vio_frontend_submit_subset(*args)
        if rc == abi.VIO_OK:
            self._pending_subset = keep
        self._check(rc, "submit_subset")

    def collect_subset(self):
        """vio_frontend_collect_subset -> [(ids, xyz)] in the order of the submit's seqs (empty for a sequence that did not
        publish)."""
        n = self._pending_subset[0] if getattr(self, "_pending_subset", None) else 0
        cap = self.cfg.max_corners
        obs = np.zeros(max(n, 1) * cap, _OBS_DTYPE)
        n_obs = np.zeros(max(n, 1), np.int32)
        rc = self.lib.vio_frontend_collect_subset(self._h, C.cast(obs.ctypes.data, C.POINTER(abi.VioObs)), n_obs.ctypes.data_as(_ip))
        if rc != abi.VIO_ESTATE:
            self._pending_subset = None
        self._check(rc, "collect_subset")
        obs = obs.reshape(max(n, 1), cap)
        out = []
        for i in range(n):
            o = obs[i, :int(n_obs[i])]
            out.append((o["id"].copy(), np.stack([o["x"], o["y"], o["z"]], axis=1)))
        return out

    def read_subset(self, seqs, frames, publish, frame_index=None):
        """readImage for the sequences of `seqs` only (vio_frontend_read_subset): submit_subset + collect_subset."""
        self.submit_subset(seqs, frames, publish, frame_index)
        return self.collect_subset()

    def reset(self, seqs=None):
        """vio_frontend_reset: a fresh FeatureTracker for the sequences of `seqs` (None: all of them)."""
        if seqs is None:
            rc = self.lib.vio_frontend_reset(self._h, 0, None)
        else:
            seqs = np.ascontiguousarray(seqs, np.int32).reshape(-1)
            rc = self.lib.vio_frontend_reset(self._h, len(seqs), seqs.ctypes.data_as(_ip))
        self._check(rc, "reset")

    def set_cameras(self, seqs, cams):
        """vio_frontend_set_cameras: sequence seqs[i] publishes with the intrinsics of cams[i] (abi.VioCamera) from its next
        published frame on. -> rc."""
        seqs = np.ascontiguousarray(seqs, np.int32).reshape(-1)
        arr = (abi.VioCamera * max(len(cams), 1))(*cams)
        return self.lib.vio_frontend_set_cameras(self._h, len(seqs), seqs.ctypes.data_as(_ip), arr)

    def get_camera(self, seq=0):
        out = abi.VioCamera()
        self._check(self.lib.vio_frontend_get_camera(self._h, seq, C.byref(out)), "get_camera")
        return out

    def set_regions(self, seqs, masks=None, mask_index=None):
        """vio_frontend_set_regions: setMask of sequence seqs[i] starts from masks[i] (uint8 [n, rows, cols] on the host,
        nonzero = usable) from its next published frame on; masks an int: a device pointer to packed [slots, rows, cols] masks,
        mask_index naming the slots; masks None clears the named sequences. -> rc."""
        seqs = np.ascontiguousarray(seqs, np.int32).reshape(-1)
        mi = None if mask_index is None else np.ascontiguousarray(mask_index, np.int32).reshape(-1)
        assert mi is None or len(mi) == len(seqs)
        mip = mi.ctypes.data_as(_ip) if mi is not None else None
        if masks is None or isinstance(masks, int):
            return self.lib.vio_frontend_set_regions(self._h, len(seqs), seqs.ctypes.data_as(_ip), C.c_void_p(masks or 0),
                                                     0 if masks is None else 1, mip)
        masks = np.ascontiguousarray(masks, np.uint8)
        assert masks.ndim == 3 and masks.shape[1:] == (self.cfg.image_rows, self.cfg.image_cols), masks.shape
        assert len(masks) > (int(mi.max()) if mi is not None and len(mi) else len(seqs) - 1)
        return self.lib.vio_frontend_set_regions(self._h, len(seqs), seqs.ctypes.data_as(_ip), C.c_void_p(masks.ctypes.data), 0, mip)

    def region(self, seq=0):
        """vio_frontend_get_region -> (mask uint8 [rows, cols] of 0 / 255, is_set, n_usable)."""
        mask = np.zeros((self.cfg.image_rows, self.cfg.image_cols), np.uint8)
        is_set, n = C.c_int32(), C.c_int64()
        self._check(self.lib.vio_frontend_get_region(self._h, seq, mask.ctypes.data_as(_u8p), C.byref(is_set), C.byref(n)), "get_region")
        return mask, bool(is_set.value), n.value

    def in_step(self):
        """True while every sequence is in the same phase, i.e. while the lock-step calls (read_images, submit, step) are allowed."""
        v = C.c_int32()
        self._check(self.lib.vio_frontend_in_step(self._h, C.byref(v)), "in_step")
        return bool(v.value)

    def state(self, seq=0):
        cap = self.cfg.max_corners
        pts = np.zeros((cap, 2), np.float32)
        ids = np.zeros(cap, np.int32)
        cnt = np.zeros(cap, np.int32)
        n = C.c_int32()
        self._check(self.lib.vio_frontend_get_state(self._h, seq, pts.ctypes.data_as(_fp), ids.ctypes.data_as(_ip),
                                                    cnt.ctypes.data_as(_ip), cap, C.byref(n)), "get_state")
        return pts[: n.value].copy(), ids[: n.value].copy(), cnt[: n.value].copy()

    def pnp_points(self, seq=0):
        """forw_pts / ids where solveVinsPnP joins them (feature_tracker.cpp:207): ahead of rejectWithF / setMask."""
        cap = self.cfg.max_corners
        pts = np.zeros((cap, 2), np.float32)
        ids = np.zeros(cap, np.int32)
        n = C.c_int32()
        self._check(self.lib.vio_frontend_get_pnp_points(self._h, seq, pts.ctypes.data_as(_fp), ids.ctypes.data_as(_ip), cap,
                                                         C.byref(n)), "get_pnp_points")
        return pts[: n.value].copy(), ids[: n.value].copy()

    def lk_iterations(self, enable=None, read=True):
        """vio_frontend_lk_iterations: switches the LK kernel's iteration counters (enable True / False / None = leave) and,
        with read, returns (iterations, visits) per pyramid level since the last read."""
        it = (C.c_uint64 * 8)()
        vis = (C.c_uint64 * 8)()
        self._check(self.lib.vio_frontend_lk_iterations(self._h, -1 if enable is None else (1 if enable else 0),
                                                        it if read else None, vis if read else None, 8), "lk_iterations")
        return (np.array(it[:], np.float64), np.array(vis[:], np.float64)) if read else None

    # resident API (throughput runs): frames [n_frames, n_seq, rows, cols] uploaded once
    def upload_frames(self, frames):
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.ndim == 4 and frames.shape[1] == self.n_seq
        self._check(self.lib.vio_frontend_upload_frames(self._h, frames.ctypes.data_as(_u8p), frames.shape[0], frames.shape[2],
                                                        frames.shape[3], frames.shape[3]), "upload_frames")

    def step(self, frame_index, publish, stream=None):
        self._check(self.lib.vio_frontend_step_resident(self._h, frame_index, 1 if publish else 0,
                                                        C.c_void_p(stream) if stream else None), "step_resident")

    def sync(self):
        self._check(self.lib.vio_frontend_sync(self._h), "sync")

    def kernel_ms(self):
        ms = C.c_double()
        n = C.c_int32()
        self._check(self.lib.vio_frontend_kernel_ms(self._h, C.byref(ms), C.byref(n)), "kernel_ms")
        return ms.value, n.value


def klt_track(cfg, prev, nxt, pts):
    """cv::calcOpticalFlowPyrLK(prev, next, pts, ..., Size(21,21), 3) (feature_tracker.cpp:181)."""
    lib = abi.load_product()
    prev, nxt = np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(nxt, np.uint8)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    out = np.zeros((n, 2), np.float32)
    st = np.zeros(n, np.uint8)
    err = np.zeros(n, np.float32)
    rc = lib.vio_klt_track(C.byref(cfg), prev.ctypes.data_as(_u8p), nxt.ctypes.data_as(_u8p), prev.shape[0], prev.shape[1],
                           prev.shape[1], pts.ctypes.data_as(_fp), n, out.ctypes.data_as(_fp), st.ctypes.data_as(_u8p),
                           err.ctypes.data_as(_fp))
    if rc != abi.VIO_OK:
        raise RuntimeError("vio_klt_track rc=%d" % rc)
    return out, st, err


def good_features(cfg, img, mask, max_corners):
    """cv::goodFeaturesToTrack(img, pts, max_corners, 0.01, MIN_DIST, mask) (feature_tracker.cpp:263)."""
    lib = abi.load_product()
    img = np.ascontiguousarray(img, np.uint8)
    corners = np.zeros((max_corners, 2), np.float32)
    n = C.c_int32()
    mp = np.ascontiguousarray(mask, np.uint8).ctypes.data_as(_u8p) if mask is not None else None
    rc = lib.vio_good_features(C.byref(cfg), img.ctypes.data_as(_u8p), mp, img.shape[0], img.shape[1], img.shape[1],
                               max_corners, corners.ctypes.data_as(_fp), C.byref(n))
    if rc != abi.VIO_OK:
        raise RuntimeError("vio_good_features rc=%d" % rc)
    return corners[: n.value].copy()


def fundamental_ransac(cfg, p1, p2):
    """status of cv::findFundamentalMat(p1, p2, FM_RANSAC, F_THRESHOLD, 0.99, status) (feature_tracker.cpp:95,198)."""
    lib = abi.load_product()
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
    m = np.zeros(len(p1), np.uint8)
    rc = lib.vio_fundamental_ransac(C.byref(cfg), p1.ctypes.data_as(_fp), p2.ctypes.data_as(_fp), len(p1), m.ctypes.data_as(_u8p))
    if rc != abi.VIO_OK:
        raise RuntimeError("vio_fundamental_ransac rc=%d" % rc)
    return m


class Preprocessor:
    """The image pre-step of the camera callback on the device (cvtColor RGBA2GRAY + CLAHE, ViewController.mm:432-437):
    ctypes wrapper over vio_preprocess_*."""

    def __init__(self, rows, cols, max_frames=1, lib=None):
        self.lib = lib or abi.load_product()
        self.rows, self.cols, self.max_frames = rows, cols, max_frames
        self._h = C.c_void_p()
        rc = self.lib.vio_preprocess_create(max_frames, rows, cols, C.byref(self._h))
        if rc != 0:
            raise RuntimeError("vio_preprocess_create failed: %d" % rc)

    def close(self):
        if self._h:
            self.lib.vio_preprocess_destroy(self._h)
            self._h = C.c_void_p()

    def set_clahe(self, clip_limit=3.0, tiles_x=8, tiles_y=8):
        rc = self.lib.vio_preprocess_set_clahe(self._h, float(clip_limit), tiles_x, tiles_y)
        if rc != 0:
            raise RuntimeError("vio_preprocess_set_clahe failed: %d" % rc)

    def set_lenses(self, slots, lenses=None):
        """vio_preprocess_set_lenses: lenses[i] (abi.VioLens) rectifies the frame at position slots[i] of every later run;
        lenses=None clears the named slots. -> the return code (VIO_EINVAL: nothing changed)."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        arr = None
        if lenses is not None:
            assert len(lenses) == len(slots)
            arr = (abi.VioLens * max(len(slots), 1))(*lenses)
        return self.lib.vio_preprocess_set_lenses(self._h, len(slots), slots.ctypes.data_as(C.POINTER(C.c_int32)), arr)

    def get_lens(self, slot):
        """-> the slot's abi.VioLens, or None when it holds none (a slot that holds a rational or a fisheye model: VIO_ESTATE,
        raised)."""
        out, is_set = abi.VioLens(), C.c_int32()
        rc = self.lib.vio_preprocess_get_lens(self._h, slot, C.byref(out), C.byref(is_set))
        if rc != 0:
            raise RuntimeError("vio_preprocess_get_lens failed: %d" % rc)
        return out if is_set.value else None

    def set_lens_models(self, slots, lenses=None):
        """vio_preprocess_set_lens_models: set_lenses with abi.VioLensModel records (Brown-Conrady, rational or fisheye);
        both write the same table. -> the return code (VIO_EINVAL: nothing changed)."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        arr = None
        if lenses is not None:
            assert len(lenses) == len(slots)
            arr = (abi.VioLensModel * max(len(slots), 1))(*lenses)
        return self.lib.vio_preprocess_set_lens_models(self._h, len(slots), slots.ctypes.data_as(C.POINTER(C.c_int32)), arr)

    def get_lens_model(self, slot):
        """-> the slot's lens as an abi.VioLensModel, whichever setter put it there, or None when it holds none."""
        out, is_set = abi.VioLensModel(), C.c_int32()
        rc = self.lib.vio_preprocess_get_lens_model(self._h, slot, C.byref(out), C.byref(is_set))
        if rc != 0:
            raise RuntimeError("vio_preprocess_get_lens_model failed: %d" % rc)
        return out if is_set.value else None

    def run(self, frames):
        """frames: [n, rows, cols] gray or [n, rows, cols, 4] RGBA (uint8) -> (gray [n, rows, cols], equalized); for a slot
        that holds a lens both are of the rectified frame."""
        frames = np.ascontiguousarray(frames, np.uint8)
        ch = 4 if frames.ndim == 4 else 1
        n = frames.shape[0]
        assert frames.shape[1:3] == (self.rows, self.cols)
        gray, eq = np.zeros((n, self.rows, self.cols), np.uint8), np.zeros((n, self.rows, self.cols), np.uint8)
        u8p = C.POINTER(C.c_uint8)
        rc = self.lib.vio_preprocess_run(self._h, frames.ctypes.data_as(u8p), ch, n, self.cols * ch, gray.ctypes.data_as(u8p),
                                         eq.ctypes.data_as(u8p))
        if rc != 0:
            raise RuntimeError("vio_preprocess_run failed: %d" % rc)
        return gray, eq

    def run_resident(self, d_pixels, channels, n_frames, d_equalized, stream=None):
        rc = self.lib.vio_preprocess_run_resident(self._h, C.c_void_p(d_pixels), channels, n_frames, self.cols * channels,
                                                  C.c_void_p(d_equalized), C.c_void_p(stream or 0))
        if rc != 0:
            raise RuntimeError("vio_preprocess_run_resident failed: %d" % rc)

    def set_sources(self, slots, sources=None):
        """vio_preprocess_set_sources: sources[i] (abi.VioSource) describes the frame at position slots[i] of every later
        run_frames / run_frames_resident; sources=None clears the named slots. -> the return code (VIO_EINVAL: nothing changed)."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        arr = None
        if sources is not None:
            assert len(sources) == len(slots)
            arr = (abi.VioSource * max(len(slots), 1))(*sources)
        return self.lib.vio_preprocess_set_sources(self._h, len(slots), slots.ctypes.data_as(C.POINTER(C.c_int32)), arr)

    def get_source(self, slot):
        """-> the slot's abi.VioSource, or None when it holds none."""
        out, is_set = abi.VioSource(), C.c_int32()
        rc = self.lib.vio_preprocess_get_source(self._h, slot, C.byref(out), C.byref(is_set))
        if rc != 0:
            raise RuntimeError("vio_preprocess_get_source failed: %d" % rc)
        return out if is_set.value else None

    def run_frames(self, frames, want_gray=True):
        """frames[i]: a uint8 numpy array whose first byte is the first byte of plane 0 of slot i's frame, laid out as the
        slot's source says -> (rc, gray [n, rows, cols] or None, equalized [n, rows, cols])."""
        n = len(frames)
        ptrs = (C.c_void_p * max(n, 1))(*[f.ctypes.data for f in frames])
        gray = np.zeros((n, self.rows, self.cols), np.uint8) if want_gray else None
        eq = np.zeros((n, self.rows, self.cols), np.uint8)
        u8p = C.POINTER(C.c_uint8)
        rc = self.lib.vio_preprocess_run_frames(self._h, ptrs, n, gray.ctypes.data_as(u8p) if want_gray else None,
                                                eq.ctypes.data_as(u8p))
        return rc, gray, eq

    def run_frames_resident(self, d_pixels, d_equalized, stream=None):
        """d_pixels: one device pointer per frame (slot i's frame at d_pixels[i]); asynchronous -> the return code."""
        n = len(d_pixels)
        ptrs = (C.c_void_p * max(n, 1))(*[int(x) for x in d_pixels])
        return self.lib.vio_preprocess_run_frames_resident(self._h, ptrs, n, C.c_void_p(d_equalized), C.c_void_p(stream or 0))

    def valid_regions(self, slots, margin=0):
        """vio_preprocess_valid_regions -> (rc, masks [n, rows, cols] of 0 / 255): where slot slots[i]'s rectified image is made
        of delivered pixels only, eroded by margin (VIO_EINVAL: nothing written)."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        masks = np.zeros((len(slots), self.rows, self.cols), np.uint8)
        rc = self.lib.vio_preprocess_valid_regions(self._h, len(slots), slots.ctypes.data_as(C.POINTER(C.c_int32)), margin,
                                                   masks.ctypes.data_as(C.POINTER(C.c_uint8)))
        return rc, masks

    def valid_regions_resident(self, slots, margin, d_masks, stream=None):
        """The same into the device buffer d_masks [n][rows][cols], asynchronous on stream -> the return code."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        return self.lib.vio_preprocess_valid_regions_resident(self._h, len(slots), slots.ctypes.data_as(C.POINTER(C.c_int32)), margin,
                                                              C.c_void_p(d_masks), C.c_void_p(stream or 0))

    def sync(self):
        rc = self.lib.vio_preprocess_sync(self._h)
        if rc != 0:
            raise RuntimeError("vio_preprocess_sync failed: %d" % rc)

    def kernel_ms(self):
        ms, n = C.c_double(), C.c_int32()
        self.lib.vio_preprocess_kernel_ms(self._h, C.byref(ms), C.byref(n))
        return ms.value, n.value
