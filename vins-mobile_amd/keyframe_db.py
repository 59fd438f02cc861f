"""Host-side mirror of the keyframe database, KeyFrameDatabase (VINS_ios/loop/keyfame_database.{h,cpp}) for n sessions
with the lists resident on the device (csrc/vio_keyframe_db.hip, csrc/kfdb_core.h). Thin ctypes wrappers over
vio_keyframe_db_*; no compute here."""
import ctypes as C

import numpy as np

from . import abi
from .posegraph import VioPoseGraphKeyframe

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
_KF_FIELDS = ("origin_t", "origin_r", "t", "r", "global_index", "has_loop", "is_looped", "loop_index", "loop_info")


def bind(lib):
    vp, i32 = C.c_void_p, C.c_int32
    lib.vio_keyframe_db_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    lib.vio_keyframe_db_destroy.argtypes = [vp]
    lib.vio_keyframe_db_destroy.restype = None
    lib.vio_keyframe_db_get_device.argtypes = [vp, _ip]
    lib.vio_keyframe_db_clear.argtypes = [vp, i32]
    lib.vio_keyframe_db_size.argtypes = [vp, i32, _ip]
    lib.vio_keyframe_db_add.argtypes = [vp, i32, _ip, _dp, _dp, _dp, _ip]
    lib.vio_keyframe_db_new_segment.argtypes = [vp, i32]
    lib.vio_keyframe_db_set_loop.argtypes = [vp, i32, i32, i32]
    lib.vio_keyframe_db_get_pose.argtypes = [vp, i32, _ip, _ip, _dp, _dp, _dp]
    lib.vio_keyframe_db_update.argtypes = [vp, i32, _ip, _ip, _dp, _dp, _dp, i32, _dp, _dp, _dp, _ip]
    lib.vio_keyframe_db_optimize.argtypes = [vp, i32, _ip, _ip, i32, _dp, _dp, _dp, C.POINTER(abi.VioSolveStats)]
    lib.vio_keyframe_db_resample.argtypes = [vp, i32, _ip, i32, _ip]
    lib.vio_keyframe_db_download.argtypes = [vp, i32, C.POINTER(VioPoseGraphKeyframe), _dp, _ip, i32, _ip, _dp, _ip]
    return lib


def _i(a):
    return np.ascontiguousarray(a, np.int32)


def _d(a):
    return np.ascontiguousarray(a, np.float64)


class KeyframeDbError(RuntimeError):
    def __init__(self, what, rc):
        RuntimeError.__init__(self, "vio_keyframe_db_%s failed: %d" % (what, rc))
        self.rc = rc


class KeyFrameDatabase:
    """n_sessions independent keyframe lists; every call takes the sessions it is for (each at most once)."""

    def __init__(self, n_sessions=1, max_keyframes=512, max_graphs=1, max_frame_num=500, lib=None):
        self.lib = bind(lib or abi.load_product())
        self.n_sessions, self.max_keyframes = n_sessions, max_keyframes
        self._h = C.c_void_p()
        self._check(self.lib.vio_keyframe_db_create(n_sessions, max_keyframes, max_graphs, max_frame_num, C.byref(self._h)), "create")

    def _check(self, rc, what):
        if rc != abi.VIO_OK:
            raise KeyframeDbError(what, rc)

    def close(self):
        if self._h:
            self.lib.vio_keyframe_db_destroy(self._h)
            self._h = C.c_void_p()

    def device(self):
        d = C.c_int32(-1)
        self._check(self.lib.vio_keyframe_db_get_device(self._h, C.byref(d)), "get_device")
        return d.value

    def clear(self, session=0):
        self._check(self.lib.vio_keyframe_db_clear(self._h, session), "clear")

    def size(self, session=0):
        n = C.c_int32(0)
        self._check(self.lib.vio_keyframe_db_size(self._h, session, C.byref(n)), "size")
        return n.value

    def add(self, sessions, headers, P, R):
        """-> the global_index of the new keyframe of every session."""
        s, h, P, R = _i(sessions), _d(headers), _d(P), _d(R)
        n = len(s)
        assert h.size == n and P.size == 3 * n and R.size == 9 * n
        out = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.vio_keyframe_db_add(self._h, n, s.ctypes.data_as(_ip), h.ctypes.data_as(_dp), P.ctypes.data_as(_dp),
                                                 R.ctypes.data_as(_dp), out.ctypes.data_as(_ip)), "add")
        return out[:n]

    def new_segment(self, session=0):
        self._check(self.lib.vio_keyframe_db_new_segment(self._h, session), "new_segment")

    def set_loop(self, cur_index, old_index, session=0):
        self._check(self.lib.vio_keyframe_db_set_loop(self._h, session, cur_index, old_index), "set_loop")

    def get_pose(self, sessions, indices):
        """-> P [n][3], R [n][3][3], header [n]."""
        s, ix = _i(sessions), _i(indices)
        n = len(s)
        assert len(ix) == n
        P, R, h = np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3, 3)), np.zeros(max(n, 1))
        self._check(self.lib.vio_keyframe_db_get_pose(self._h, n, s.ctypes.data_as(_ip), ix.ctypes.data_as(_ip), P.ctypes.data_as(_dp),
                                                      R.ctypes.data_as(_dp), h.ctypes.data_as(_dp)), "get_pose")
        return P[:n], R[:n], h[:n]

    def update(self, sessions, loop_kf, relative_t, relative_q, relative_yaw, window_size, header0, P0, R0):
        """-> optimize_index per session (-1: nothing to optimize). relative_q is x y z w."""
        s, lk = _i(sessions), _i(loop_kf)
        n = len(s)
        rt, rq, ry, h0, P0, R0 = _d(relative_t), _d(relative_q), _d(relative_yaw), _d(header0), _d(P0), _d(R0)
        assert len(lk) == n and rt.size == 3 * n and rq.size == 4 * n and ry.size == n and h0.size == n and P0.size == 3 * n and R0.size == 9 * n
        out = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.vio_keyframe_db_update(self._h, n, s.ctypes.data_as(_ip), lk.ctypes.data_as(_ip), rt.ctypes.data_as(_dp),
                                                    rq.ctypes.data_as(_dp), ry.ctypes.data_as(_dp), window_size, h0.ctypes.data_as(_dp),
                                                    P0.ctypes.data_as(_dp), R0.ctypes.data_as(_dp), out.ctypes.data_as(_ip)), "update")
        return out[:n]

    def optimize(self, sessions, cur_indices, max_iterations=5):
        """-> per session dict(yaw_drift, r_drift, t_drift, stats)."""
        s, ci = _i(sessions), _i(cur_indices)
        n = len(s)
        assert len(ci) == n
        yd, rd, td = np.zeros(max(n, 1)), np.zeros((max(n, 1), 3, 3)), np.zeros((max(n, 1), 3))
        st = (abi.VioSolveStats * max(n, 1))()
        self._check(self.lib.vio_keyframe_db_optimize(self._h, n, s.ctypes.data_as(_ip), ci.ctypes.data_as(_ip), max_iterations,
                                                      yd.ctypes.data_as(_dp), rd.ctypes.data_as(_dp), td.ctypes.data_as(_dp), st), "optimize")
        return [{"yaw_drift": float(yd[i]), "r_drift": rd[i].copy(), "t_drift": td[i].copy(), "stats": abi.stats_to_dict(st[i])}
                for i in range(n)]

    def resample(self, session=0):
        """-> the erased global_index values, ascending (what vio_loop_detector_erase takes)."""
        cap = self.max_keyframes
        out, n = np.zeros(cap, np.int32), C.c_int32(0)
        self._check(self.lib.vio_keyframe_db_resample(self._h, session, out.ctypes.data_as(_ip), cap, C.byref(n)), "resample")
        return out[:n.value].copy()

    def download(self, session=0):
        """-> dict(kf: list of dicts as posegraph.keyframes_struct takes them, header, segment_index, total_length, last_P,
        yaw_drift, r_drift, t_drift, earliest_loop_index, cur_seg_index, max_seg_index)."""
        cap = self.max_keyframes
        arr = (VioPoseGraphKeyframe * cap)()
        hdr, seg, n, state, ist = np.zeros(cap), np.zeros(cap, np.int32), C.c_int32(0), np.zeros(17), np.zeros(3, np.int32)
        self._check(self.lib.vio_keyframe_db_download(self._h, session, arr, hdr.ctypes.data_as(_dp), seg.ctypes.data_as(_ip), cap,
                                                      C.byref(n), state.ctypes.data_as(_dp), ist.ctypes.data_as(_ip)), "download")
        kfs = []
        for a in arr[:n.value]:
            kfs.append({"origin_t": np.array(a.origin_t), "origin_r": np.array(a.origin_r).reshape(3, 3), "t": np.array(a.t),
                        "r": np.array(a.r).reshape(3, 3), "global_index": a.global_index, "has_loop": a.has_loop,
                        "is_looped": a.is_looped, "loop_index": a.loop_index, "loop_info": np.array(a.loop_info)})
        return {"kf": kfs, "header": hdr[:n.value].copy(), "segment_index": seg[:n.value].copy(), "total_length": float(state[0]),
                "last_P": state[1:4].copy(), "yaw_drift": float(state[4]), "r_drift": state[5:14].reshape(3, 3).copy(),
                "t_drift": state[14:17].copy(), "earliest_loop_index": int(ist[0]), "cur_seg_index": int(ist[1]),
                "max_seg_index": int(ist[2])}
