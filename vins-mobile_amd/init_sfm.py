"""Host-side mirror of vio_init_sfm_* (estimator start-up on the device: relative pose fit, GlobalSFM::construct with its
bundle adjustment, PnP of the frames outside the window; VINS_ios/VINS.cpp:833-1003): a numpy container for one problem and
thin ctypes wrappers. No logic lives here."""
import ctypes as C

import numpy as np

from . import abi
from .pnp import stats_dict

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_u8 = C.POINTER(C.c_uint8)


class SfmProblem:
    """The arguments of one VioInitSfmProblem and room for its outputs.

    extras: list of (guess frame, landmark indices, xy [k][2]) for the frames outside the window."""

    def __init__(self, frame_num, l, feat_start, obs_frame, obs_xy, relative=None, hint=None, extras=()):
        f = lambda a: np.ascontiguousarray(a, np.float64)
        self.frame_num, self.l = int(frame_num), int(l)
        self.feat_start, self.obs_frame = np.ascontiguousarray(feat_start, np.int32), np.ascontiguousarray(obs_frame, np.int32)
        self.obs_xy = f(obs_xy)
        self.n_features = len(self.feat_start) - 1
        self.relative = None if relative is None else (f(relative[0]).reshape(9).copy(), f(relative[1]).reshape(3).copy())
        self.hint = None if hint is None else f(hint).reshape(9).copy()
        self.extras = [(int(g), np.ascontiguousarray(idx, np.int32), f(xy).reshape(-1, 2)) for g, idx, xy in extras]
        ne = len(self.extras)
        self.extra_guess = np.array([g for g, _, _ in self.extras] + [0], np.int32)
        self.extra_start = np.concatenate([[0], np.cumsum([len(i) for _, i, _ in self.extras])]).astype(np.int32)
        self.extra_feature = np.concatenate([i for _, i, _ in self.extras] + [np.zeros(1, np.int32)]).astype(np.int32)
        self.extra_xy = np.concatenate([xy for _, _, xy in self.extras] + [np.zeros((1, 2))])
        n = max(self.n_features, 1)
        self.q, self.T = np.zeros((self.frame_num, 4)), np.zeros((self.frame_num, 3))
        self.points, self.point_ok = np.zeros((n, 3)), np.zeros(n, np.uint8)
        self.extra_R, self.extra_T = np.zeros((max(ne, 1), 9)), np.zeros((max(ne, 1), 3))
        self.status, self.inliers = -1, -1
        self.relative_R, self.relative_T = np.zeros(9), np.zeros(3)

    def copy(self):
        return SfmProblem(self.frame_num, self.l, self.feat_start, self.obs_frame, self.obs_xy, self.relative, self.hint, self.extras)

    def fill_struct(self, s):
        s.frame_num, s.l, s.n_features = self.frame_num, self.l, self.n_features
        s.feat_start, s.obs_frame, s.obs_xy = self.feat_start.ctypes.data_as(_ip), self.obs_frame.ctypes.data_as(_ip), self.obs_xy.ctypes.data_as(_dp)
        s.relative_mode = 1 if self.relative is None else 0
        s.R_hint = None if self.hint is None else self.hint.ctypes.data_as(_dp)
        s.n_extra = len(self.extras)
        s.extra_guess, s.extra_start = self.extra_guess.ctypes.data_as(_ip), self.extra_start.ctypes.data_as(_ip)
        s.extra_feature, s.extra_xy = self.extra_feature.ctypes.data_as(_ip), self.extra_xy.ctypes.data_as(_dp)
        s.status, s.inliers = -1, -1
        for k in range(9):
            s.relative_R[k] = 0.0 if self.relative is None else self.relative[0][k]
        for k in range(3):
            s.relative_T[k] = 0.0 if self.relative is None else self.relative[1][k]
        s.q, s.T, s.points = (a.ctypes.data_as(_dp) for a in (self.q, self.T, self.points))
        s.point_ok = self.point_ok.ctypes.data_as(_u8)
        s.extra_R, s.extra_T = self.extra_R.ctypes.data_as(_dp), self.extra_T.ctypes.data_as(_dp)

    def read_struct(self, s):
        self.status, self.inliers = s.status, s.inliers
        self.relative_R, self.relative_T = np.array(s.relative_R[:]), np.array(s.relative_T[:])


def solve_with(fn, problems, *extra):
    """fn(VioInitSfmProblem*, n, VioSolveStats*, *extra) -> status: outputs into the problems; (status, stats dicts)."""
    n = len(problems)
    arr, st = (abi.VioInitSfmProblem * max(n, 1))(), (abi.VioSolveStats * max(n, 1))()
    for a, p in zip(arr, problems):
        p.fill_struct(a)
    rc = fn(arr, n, st, *extra)
    for a, p in zip(arr, problems):
        p.read_struct(a)
    return rc, [stats_dict(s) for s in st[:n]]


class SfmSolver:
    def __init__(self, max_batch, max_frames, max_points, max_obs, max_extra, lib=None):
        self.lib = lib or abi.load_product()
        self._h = C.c_void_p()
        rc = self.lib.vio_init_sfm_create(max_batch, max_frames, max_points, max_obs, max_extra, C.byref(self._h))
        if rc != 0:
            raise RuntimeError("vio_init_sfm_create failed: %d" % rc)

    def close(self):
        if self._h:
            self.lib.vio_init_sfm_destroy(self._h)
            self._h = C.c_void_p()

    def device(self):
        d = C.c_int32(-1)
        self.lib.vio_init_sfm_get_device(self._h, C.byref(d))
        return d.value

    def solve_rc(self, problems):
        return solve_with(lambda arr, n, st: self.lib.vio_init_sfm_solve(self._h, arr, n, st), problems)

    def solve(self, problems):
        rc, st = self.solve_rc(problems)
        if rc != 0:
            raise RuntimeError("vio_init_sfm_solve failed: %d" % rc)
        return st

    def head_state(self, index, problem):
        """(status, c_rotation [F][4], c_translation [F][3], points [n][3]) the head of problem `index` of the last solve left."""
        cq, ct = np.zeros((problem.frame_num, 4)), np.zeros((problem.frame_num, 3))
        pts = np.zeros((max(problem.n_features, 1), 3))
        rc = self.lib.vio_init_sfm_head_state(self._h, index, cq.ctypes.data_as(_dp), ct.ctypes.data_as(_dp), pts.ctypes.data_as(_dp))
        return rc, cq, ct, pts

    def kernel_ms(self):
        """((head, bundle adjustment, extra-frame PnP) ms summed since the last call, launches)."""
        ms, k = (C.c_double * 3)(), C.c_int32()
        self.lib.vio_init_sfm_kernel_ms(self._h, ms, C.byref(k))
        return tuple(ms), k.value
