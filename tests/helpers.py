"""Shared test plumbing: loads the CHECKERS (oracle/) and golden fixtures. Only tests/, smoke() and bench.py's
cpu_baseline leg and input set-up may touch oracle/ — the product library never does."""
import ctypes as C
import glob
import importlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
pkg = importlib.import_module("vins-mobile_amd")
abi, synth = pkg.abi, pkg.synth
_dp = C.POINTER(C.c_double)

_oracle = None


class OracleRansacTrace(C.Structure):  # oracle/vio_oracle.h
    _fields_ = [(k, C.c_int32) for k in (
        "lmeds", "iterations", "niters", "niters_lowered", "models", "subset_redraws", "first_redraw_iteration",
        "subset_failed", "subset_failed_iteration", "zero_pivots", "cubic_three", "cubic_one", "cubic_quadratic",
        "cubic_linear", "cubic_none", "models_f8_zero", "best_updates", "last_best_iteration", "max_good",
        "nan_errors", "nan_errors_positive")] + [("redraw_mask", C.c_uint64), ("min_median", C.c_double)]


def oracle_lib():
    """oracle/libvio_oracle.so (plain C++ restatement); built on demand with g++."""
    global _oracle
    if _oracle is None:
        so = os.path.join(ROOT, "oracle", "libvio_oracle.so")
        srcs = glob.glob(os.path.join(ROOT, "oracle", "vio_oracle*")) + [os.path.join(ROOT, "include", "vio_amd.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "port"], stdout=subprocess.DEVNULL)
        lib = C.CDLL(so)
        lib.oracle_eval_projection.argtypes = [C.POINTER(abi.VioConfig)] + [_dp] * 8
        lib.oracle_eval_imu.argtypes = [C.POINTER(abi.VioConfig), C.POINTER(abi.VioPreintegration)] + [_dp] * 6
        u8p, fp, ip = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32)
        cfgp = C.POINTER(abi.VioConfig)
        lib.oracle_pyr_down.argtypes = [u8p, C.c_int32, C.c_int32, C.c_int32, u8p]
        lib.oracle_preprocess.argtypes = [u8p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                          u8p, u8p]
        lib.oracle_klt_track.argtypes = [cfgp, u8p, u8p, C.c_int32, C.c_int32, C.c_int32, fp, C.c_int32, fp, u8p, fp]
        lib.oracle_min_eigen_map.argtypes = [u8p, C.c_int32, C.c_int32, C.c_int32, fp]
        lib.oracle_good_features.argtypes = [cfgp, u8p, u8p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, fp, ip]
        lib.oracle_fundamental_ransac.argtypes = [cfgp, fp, fp, C.c_int32, u8p]
        lib.oracle_fundamental_ransac_trace.argtypes = [cfgp, fp, fp, C.c_int32, u8p, C.POINTER(OracleRansacTrace)]
        lib.oracle_run7point.argtypes = [fp, fp, _dp]
        lib.oracle_tracker_create.restype = C.c_void_p
        lib.oracle_tracker_create.argtypes = [cfgp]
        lib.oracle_tracker_destroy.argtypes = [C.c_void_p]
        lib.oracle_tracker_read_image.argtypes = [C.c_void_p, u8p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                                  C.POINTER(abi.VioObs), ip]
        lib.oracle_tracker_get_state.argtypes = [C.c_void_p, fp, ip, ip, C.c_int32, ip]
        lib.oracle_set_lk_accum_mode.argtypes = [C.c_int]
        _oracle = lib
    return _oracle


def oracle_backend():
    return abi.bind_backend_solver(oracle_lib(), "oracle")


EMUL_DIR = os.path.join(ROOT, "tests", "emul")


def build_emul_lib(source_name, so_name, define, extra_flags=()):
    """tests/emul/<source_name> compiled for the host with -D<define> (VIO_SIMT: every work-item a fiber of simt.h; VIO_EMUL:
    one thread) into tests/emul/<so_name>, loaded. Rebuilt when the library is older than its source or ANY header the
    kernel sources could reach: a hand-kept list goes stale the day a header is split."""
    csrc, inc = os.path.join(ROOT, "vins-mobile_amd", "csrc"), os.path.join(ROOT, "include")
    so, src = os.path.join(EMUL_DIR, so_name), os.path.join(EMUL_DIR, source_name)
    deps = [src] + [f for pat in ((csrc, "*.h"), (csrc, "*.inc"), (csrc, "*.cpp"), (EMUL_DIR, "*.h"), (inc, "*.h"))
                    for f in glob.glob(os.path.join(*pat))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-psabi", *extra_flags, "-D" + define,
                               "-I" + inc, "-I" + csrc, "-I" + EMUL_DIR, "-shared", "-o", so, src])
    return C.CDLL(so)


def ref_lib_or_none():
    so = os.path.join(ROOT, "oracle", "_ref", "libvio_ref.so")
    return C.CDLL(so) if os.path.exists(so) else None


def cfg_from_npz(d):
    cfg = abi.VioConfig()
    for k, _ in abi.VioConfig._fields_:
        setattr(cfg, k, d["cfg_" + k].item())
    return cfg


def load_golden_window(name):
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    w = abi.Window.from_npz_dict({k[3:]: v for k, v in d.items() if k.startswith("in_")})
    return cfg_from_npz(d), w, d


def golden_window_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "win_*.npz")))


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300)) if a.size else 0.0


def pose_relerr(a, b):
    """Position and quaternion parts separately (quaternion sign-insensitive)."""
    a, b = np.asarray(a).reshape(-1, 7), np.asarray(b).reshape(-1, 7)
    ep = relerr(a[:, :3], b[:, :3])
    s = np.sign(np.sum(a[:, 3:] * b[:, 3:], axis=1, keepdims=True))
    eq = float(np.abs(a[:, 3:] * s - b[:, 3:]).max())
    return max(ep, eq)


def solve_with(solve_fn, cfg, w):
    wc = w.copy()
    st = abi.VioSolveStats()
    rc = solve_fn(C.byref(cfg), C.byref(wc.struct()), C.byref(st))
    assert rc == abi.VIO_OK, rc
    return wc, abi.stats_to_dict(st)


def check_solution(got_w, got_s, d, tol, tol_prior=None, check_trace=True):
    """Compares a solved window with the reference outputs stored in a golden fixture `d`.
    `tol` is relative (north_star: 1e-4 on poses and inverse depths)."""
    assert pose_relerr(got_w.raw_pose, d["ref_raw_pose"]) < tol
    assert relerr(got_w.raw_speed_bias, d["ref_raw_speed_bias"]) < tol
    assert relerr(got_w.raw_inv_depth, d["ref_raw_inv_depth"]) < tol
    assert pose_relerr(got_w.pose, d["ref_pose"]) < tol
    assert relerr(got_w.speed_bias, d["ref_speed_bias"]) < tol
    assert relerr(got_w.inv_depth, d["ref_inv_depth"]) < tol
    if got_w.loop_frame >= 0:
        assert pose_relerr(got_w.loop_pose, d["ref_loop_pose"]) < tol
    if check_trace:
        assert got_s["iterations"] == int(d["ref_iterations"])
        assert got_s["termination"] == int(d["ref_termination"])
        assert list(got_s["it_flags"]) == list(d["ref_it_flags"])
        assert relerr(got_s["it_cost"], d["ref_it_cost"]) < max(tol, 1e-6)
        assert relerr(got_s["it_radius"], d["ref_it_radius"]) < max(tol, 1e-4)
        assert abs(got_s["final_cost"] - float(d["ref_final_cost"])) <= max(tol, 1e-6) * float(d["ref_final_cost"])
    n_ref = int(d["ref_next_prior_n"])
    assert got_w.next_prior.n == n_ref
    if n_ref > 0:
        ref_prior = abi.Prior.from_npz_dict(d, "ref_next_prior_", got_w.W)
        Hr, br, xr = ref_prior.canonical()
        Hg, bg, xg = got_w.next_prior.canonical()
        assert [(k, i) for k, i, _ in xr] == [(k, i) for k, i, _ in xg]
        tp = tol_prior if tol_prior is not None else tol
        assert relerr(Hg, Hr) < tp
        assert relerr(bg, br) < tp
        for (_, _, a), (_, _, b) in zip(xg, xr):
            assert np.abs(a - b).max() < tol


# ---- front-end oracle wrappers -----------------------------------------------------------------------
_u8p, _fp, _ip = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32)


def oracle_klt(cfg, prev, nxt, pts):
    lib = oracle_lib()
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = len(pts)
    out, st, err = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
    lib.oracle_klt_track(C.byref(cfg), prev.ctypes.data_as(_u8p), nxt.ctypes.data_as(_u8p), prev.shape[0], prev.shape[1],
                         prev.shape[1], pts.ctypes.data_as(_fp), n, out.ctypes.data_as(_fp), st.ctypes.data_as(_u8p),
                         err.ctypes.data_as(_fp))
    return out, st, err


def oracle_good_features(cfg, img, mask, max_corners):
    lib = oracle_lib()
    corners = np.zeros((max_corners, 2), np.float32)
    n = C.c_int32()
    mp = np.ascontiguousarray(mask, np.uint8).ctypes.data_as(_u8p) if mask is not None else None
    lib.oracle_good_features(C.byref(cfg), img.ctypes.data_as(_u8p), mp, img.shape[0], img.shape[1], img.shape[1],
                             max_corners, corners.ctypes.data_as(_fp), C.byref(n))
    return corners[: n.value].copy()


def oracle_min_eigen_map(img):
    """cornerMinEigenVal(img, blockSize 3, Sobel 3) of the CPU oracle -> float32 [rows, cols]."""
    lib = oracle_lib()
    img = np.ascontiguousarray(img, np.uint8)
    eig = np.zeros(img.shape, np.float32)
    rc = lib.oracle_min_eigen_map(img.ctypes.data_as(_u8p), img.shape[0], img.shape[1], img.shape[1], eig.ctypes.data_as(_fp))
    assert rc == 0, rc
    return eig


def detector_candidates(img, mask=None):
    """The detector's candidate rule before the quality threshold, from the oracle's eigenvalue map alone: boolean map of
    v > 0 && v == max3x3(v), 1 <= x < cols - 1, 1 <= y < rows - 1, inside the mask."""
    eig = oracle_min_eigen_map(img)
    rows, cols = eig.shape
    pad = np.full((rows + 2, cols + 2), -np.inf, np.float32)
    pad[1:-1, 1:-1] = eig
    m = eig.copy()
    for dy in range(3):
        for dx in range(3):
            m = np.maximum(m, pad[dy:dy + rows, dx:dx + cols])
    cand = (eig > 0) & (eig == m)
    cand[0, :] = cand[-1, :] = False
    cand[:, 0] = cand[:, -1] = False
    if mask is not None:
        cand &= np.asarray(mask) != 0
    return cand


def oracle_ransac(cfg, p1, p2):
    lib = oracle_lib()
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
    m = np.zeros(len(p1), np.uint8)
    lib.oracle_fundamental_ransac(C.byref(cfg), p1.ctypes.data_as(_fp), p2.ctypes.data_as(_fp), len(p1), m.ctypes.data_as(_u8p))
    return m


def oracle_ransac_trace(cfg, p1, p2):
    """-> (mask, dict of the OracleRansacTrace counters) of one oracle findFundamentalMat call."""
    lib = oracle_lib()
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
    m, t = np.zeros(len(p1), np.uint8), OracleRansacTrace()
    lib.oracle_fundamental_ransac_trace(C.byref(cfg), p1.ctypes.data_as(_fp), p2.ctypes.data_as(_fp), len(p1), m.ctypes.data_as(_u8p),
                                        C.byref(t))
    return m, {k: getattr(t, k) for k, _ in OracleRansacTrace._fields_}


def oracle_run7point(ms1, ms2):
    """run7Point on seven pairs -> [n, 3, 3] models (n <= 3; empty when the solver returns none)."""
    lib = oracle_lib()
    ms1 = np.ascontiguousarray(ms1, np.float32).reshape(7, 2)
    ms2 = np.ascontiguousarray(ms2, np.float32).reshape(7, 2)
    F = np.zeros(27)
    n = lib.oracle_run7point(ms1.ctypes.data_as(_fp), ms2.ctypes.data_as(_fp), F.ctypes.data_as(_dp))
    return F[: 9 * max(n, 0)].reshape(-1, 3, 3).copy()


class OracleTracker:
    def __init__(self, cfg):
        self.lib, self.cfg = oracle_lib(), cfg
        self.h = self.lib.oracle_tracker_create(C.byref(cfg))

    def read_image(self, img, publish):
        cap = self.cfg.max_corners
        obs = (abi.VioObs * cap)()
        n = C.c_int32()
        rc = self.lib.oracle_tracker_read_image(self.h, img.ctypes.data_as(_u8p), img.shape[0], img.shape[1], img.shape[1],
                                                0.0, 1 if publish else 0, obs, C.byref(n))
        assert rc == 0, rc
        ids = np.array([obs[i].id for i in range(n.value)], np.int32)
        xyz = np.array([[obs[i].x, obs[i].y, obs[i].z] for i in range(n.value)]).reshape(n.value, 3)
        return ids, xyz

    def state(self):
        cap = self.cfg.max_corners
        pts, ids, cnt = np.zeros((cap, 2), np.float32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = C.c_int32()
        self.lib.oracle_tracker_get_state(self.h, pts.ctypes.data_as(_fp), ids.ctypes.data_as(_ip), cnt.ctypes.data_as(_ip),
                                          cap, C.byref(n))
        return pts[: n.value].copy(), ids[: n.value].copy(), cnt[: n.value].copy()

    def close(self):
        self.lib.oracle_tracker_destroy(self.h)


ODD_SHAPES = [  # (W, features, with_loop, seed): odd sizes around every chunk / strip / tile boundary of the kernel source
    (10, 1, 0, 1), (10, 5, 0, 2), (10, 7, 0, 3), (10, 8, 0, 4), (10, 23, 0, 5), (10, 25, 0, 6), (10, 97, 0, 7),
    (10, 170, 0, 8), (10, 260, 0, 9), (6, 40, 0, 10), (3, 12, 0, 11), (10, 60, 6, 12), (5, 30, 4, 13), (13, 120, 0, 14),
]




def oracle_preprocess(frame, clip_limit=3.0, tiles_x=8, tiles_y=8):
    """cvtColor + CLAHE of one frame ([rows, cols] gray or [rows, cols, 4] RGBA) by the CPU oracle -> (gray, equalized)."""
    lib = oracle_lib()
    frame = np.ascontiguousarray(frame, np.uint8)
    ch = 4 if frame.ndim == 3 else 1
    rows, cols = frame.shape[:2]
    gray, eq = np.zeros((rows, cols), np.uint8), np.zeros((rows, cols), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    rc = lib.oracle_preprocess(frame.ctypes.data_as(u8p), ch, rows, cols, cols * ch, float(clip_limit), tiles_x, tiles_y,
                               gray.ctypes.data_as(u8p), eq.ctypes.data_as(u8p))
    assert rc == 0, rc
    return gray, eq
