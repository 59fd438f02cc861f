"""Host-side mirror of the batched bundle adjustment (the closing "full BA" of GlobalSFM::construct,
VINS_ios/inital_sfm.cpp:229-296): a numpy container for one problem and thin ctypes wrappers over vio_init_ba_*. No logic
lives here."""
import ctypes as C

import numpy as np

from . import abi
from .pnp import stats_dict

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_u8 = C.POINTER(C.c_uint8)


class BaProblem:
    """The arguments of one vio_init_bundle_adjust call; c_rotation, c_translation and points are solved in place."""

    def __init__(self, frame_num, l, c_rotation, c_translation, points, point_ok, feat_start, obs_frame, obs_xy):
        f = lambda a: np.ascontiguousarray(a, np.float64)
        self.frame_num, self.l = int(frame_num), int(l)
        self.c_rotation, self.c_translation, self.points = f(c_rotation).copy(), f(c_translation).copy(), f(points).copy()
        self.point_ok = np.ascontiguousarray(point_ok, np.uint8)
        self.feat_start, self.obs_frame = np.ascontiguousarray(feat_start, np.int32), np.ascontiguousarray(obs_frame, np.int32)
        self.obs_xy = f(obs_xy)
        self.ok = -1

    def copy(self):
        return BaProblem(self.frame_num, self.l, self.c_rotation, self.c_translation, self.points, self.point_ok, self.feat_start,
                         self.obs_frame, self.obs_xy)

    def fill_struct(self, s):
        s.frame_num, s.l, s.n_points = self.frame_num, self.l, len(self.points.reshape(-1, 3))
        s.c_rotation, s.c_translation, s.points = (a.ctypes.data_as(_dp) for a in (self.c_rotation, self.c_translation, self.points))
        s.point_ok = self.point_ok.ctypes.data_as(_u8)
        s.feat_start, s.obs_frame = self.feat_start.ctypes.data_as(_ip), self.obs_frame.ctypes.data_as(_ip)
        s.obs_xy = self.obs_xy.ctypes.data_as(_dp)
        s.ok = -1


def solve_with(fn, problems, *extra):
    """fn(VioInitBaProblem*, n, VioSolveStats*, *extra) -> status: problems solved in place; (status, stats dicts)."""
    n = len(problems)
    arr, st = (abi.VioInitBaProblem * max(n, 1))(), (abi.VioSolveStats * max(n, 1))()
    for a, p in zip(arr, problems):
        p.fill_struct(a)
    rc = fn(arr, n, st, *extra)
    for a, p in zip(arr, problems):
        p.ok = a.ok
    return rc, [stats_dict(s) for s in st[:n]]


class BaSolver:
    def __init__(self, max_batch, max_frames, max_points, max_obs, lib=None):
        self.lib = lib or abi.load_product()
        self._h = C.c_void_p()
        rc = self.lib.vio_init_ba_create(max_batch, max_frames, max_points, max_obs, C.byref(self._h))
        if rc != 0:
            raise RuntimeError("vio_init_ba_create failed: %d" % rc)

    def close(self):
        if self._h:
            self.lib.vio_init_ba_destroy(self._h)
            self._h = C.c_void_p()

    def device(self):
        d = C.c_int32(-1)
        self.lib.vio_init_ba_get_device(self._h, C.byref(d))
        return d.value

    def solve_rc(self, problems):
        """Solves the problems in place; returns (status, one stats dict per problem)."""
        return solve_with(lambda arr, n, st: self.lib.vio_init_ba_solve(self._h, arr, n, st), problems)

    def solve(self, problems):
        rc, st = self.solve_rc(problems)
        if rc != 0:
            raise RuntimeError("vio_init_ba_solve failed: %d" % rc)
        return st

    def kernel_ms(self):
        ms, k = C.c_double(), C.c_int32()
        self.lib.vio_init_ba_kernel_ms(self._h, C.byref(ms), C.byref(k))
        return ms.value, k.value
