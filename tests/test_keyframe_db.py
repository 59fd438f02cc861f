"""The keyframe database on the device (vio_keyframe_db_*, csrc/vio_keyframe_db.hip + csrc/kfdb_core.h):
KeyFrameDatabase (VINS_ios/loop/keyfame_database.{h,cpp}) and the per-solved-frame block ViewController.mm:831-873 for n
sessions, the pose graph built, solved and applied without leaving the device.

The comparison truth is RefDb below: a plain-Python KeyFrameDatabase (a list of dicts) restated after the reference,
which calls the ORACLE's build / optimize / apply for the graph (pinned to the reference fixture at 1e-8 by
tests/test_posegraph.py) and never the code under test.

CPU: the entry points; the list passes of kfdb_core.h on the SIMT emulator (tests/emul/simt_kfdb.cpp) bit for bit against the
product's own host functions vio_posegraph_build / vio_posegraph_apply and against the restatement of resample.
GPU: the database against RefDb driven through the same sequence of calls.

The need_resample / resample flags compare an accumulated distance with min_dis. After the first solve the device and
the restatement hold poses that differ at the 1e-6 level, so every GPU case is chosen (seed, spacing) such that on the
restatement's walk every comparison that decides a flag (the keyframe is not kept anyway: first of the walk, has_loop,
is_looped, short list; those reset the distance whatever the comparison says) has |dis - min_dis| > 1e-3 min_dis.
RefDb records the smallest margin of every walk and the tests assert it before comparing."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import helpers as H
from test_posegraph import TOL_GPU, TOL_ORACLE   # the project's two numbers: oracle vs reference, device vs oracle

pkg = H.pkg
abi, pg, synth, kdb = pkg.abi, pkg.posegraph, pkg.synth, pkg.keyframe_db
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
MARGIN = 1e-3


def norm3(a, b):
    """|a - b| with the operations of the C code, in their order."""
    d0, d1, d2 = float(a[0]) - float(b[0]), float(a[1]) - float(b[1]), float(a[2]) - float(b[2])
    return math.sqrt(d0 * d0 + d1 * d1 + d2 * d2)


def move(R, p, t):
    """R p + t, row by row, left to right."""
    return np.array([float(R[a][0]) * float(p[0]) + float(R[a][1]) * float(p[1]) + float(R[a][2]) * float(p[2]) + float(t[a]) for a in range(3)])


def mul3(A, B):
    return np.array([[float(A[i][0]) * float(B[0][j]) + float(A[i][1]) * float(B[1][j]) + float(A[i][2]) * float(B[2][j]) for j in range(3)]
                     for i in range(3)])


def resample_walk(ts, forced, min_dis, first_forced=True):
    """The recurrence of need_resample (:170-198) and resample (:50-73): -> keep flags, smallest relative margin of the
    comparisons that decide a flag."""
    dis, last, keep, margin = 0.0, (0.0, 0.0, 0.0), [], float("inf")
    for k, t in enumerate(ts):
        dis += norm3(t, last)
        f = (k == 0 and first_forced) or bool(forced[k])
        if not f and min_dis > 0:
            margin = min(margin, abs(dis - min_dis) / min_dis)
        kp = f or dis > min_dis
        if kp:
            dis = 0.0
        last = t
        keep.append(kp)
    return keep, margin


# ---- the comparison truth ---------------------------------------------------------------------------------------------
class RefDb:
    """KeyFrameDatabase restated: keyfame_database.cpp, keyframe.cpp:4-14, 282-287, 347-366, ViewController.mm:831-873."""

    def __init__(self, max_frame_num=500):
        self.olib = pg.bind_host(H.oracle_lib(), "oracle")
        self.ofn = pg.bind_checker(H.oracle_lib(), "oracle")
        self.max_frame_num = max_frame_num
        self.clear()

    def clear(self):                                                     # :10-20
        self.kfs, self.earliest, self.next_index = [], -1, 0
        self.t_drift, self.yaw_drift, self.r_drift = np.zeros(3), 0.0, np.eye(3)
        self.total_length, self.last_P = 0.0, np.zeros(3)
        self.cur_seg = self.max_seg = 0
        self.min_margin = float("inf")

    def get(self, index):
        for k in self.kfs:
            if k["global_index"] == index:
                return k
        return None

    def add(self, header, P, R):                                         # keyframe.cpp:4-14, keyfame_database.cpp:21-42
        P, R = np.array(P, float), np.array(R, float).reshape(3, 3)
        t, r = self.r_drift @ P + self.t_drift, self.r_drift @ R
        self.kfs.append({"origin_t": P, "origin_r": R, "t": t, "r": r, "global_index": self.next_index, "has_loop": 0, "is_looped": 0,
                         "loop_index": -1, "loop_info": np.zeros(8), "header": float(header), "segment": self.cur_seg})
        self.total_length += float(np.linalg.norm(t - self.last_P))
        self.last_P = t
        self.next_index += 1
        return self.next_index - 1

    def new_segment(self):                                               # ViewController.mm:776-777
        self.max_seg += 1
        self.cur_seg = self.max_seg

    def set_loop(self, cur, old):                                        # ViewController.mm:969-971
        c, o = self.get(cur), self.get(old)
        c["has_loop"], c["loop_index"] = 1, old
        o["is_looped"] = 1

    def update(self, loop_kf, rel_t, rel_q, rel_yaw, W, header0, P0, R0):   # ViewController.mm:831-873
        if loop_kf >= 0:
            k = self.get(loop_kf)
            if abs(rel_yaw) > 30.0 or float(np.linalg.norm(rel_t)) > 10.0:
                k["has_loop"] = 0
            else:
                k["loop_info"] = np.array([rel_t[0], rel_t[1], rel_t[2], rel_q[3], rel_q[0], rel_q[1], rel_q[2], rel_yaw], float)
        opt, cnt = -1, 0
        for i in range(len(self.kfs)):
            cnt += 1
            k = self.kfs[-1 - i]
            if k["header"] == header0:
                k["origin_t"], k["origin_r"] = np.array(P0, float), np.array(R0, float).reshape(3, 3)
                if k["has_loop"]:
                    opt = k["global_index"]
                break
            if cnt > 2 * W:
                break
        return opt

    def optimize(self, cur_index, max_iterations=5):                     # :140-356
        cur = self.get(cur_index)
        assert cur is not None and cur["has_loop"] == 1
        li = cur["loop_index"]
        if self.earliest > li or self.earliest == -1:
            self.earliest = li
        pos = [i for i, k in enumerate(self.kfs) if self.earliest <= k["global_index"] <= cur_index]
        rng = [self.kfs[i] for i in pos]
        short = len(self.kfs) < self.max_frame_num
        keep, m = resample_walk([k["t"] for k in rng], [k["has_loop"] or k["is_looped"] or short for k in rng],
                                self.total_length / (1.0 * self.max_frame_num))
        self.min_margin = min(self.min_margin, m)
        g, skip = pg.build_with(self.olib, "oracle", rng, self.total_length, max_frame_num=self.max_frame_num, list_size=len(self.kfs))
        assert [int(not k) for k in keep] == list(skip)
        st = pg.optimize_with(self.ofn, g, max_iterations)
        out = pg.apply_with(self.olib, "oracle", rng, g, skip)
        seg_cur, seg_old = cur["segment"], self.get(li)["segment"]
        self.cur_seg = seg_old
        for j, k in enumerate(rng):
            k["t"], k["r"] = out["t"][j].copy(), out["r"][j].copy()
            if k is not cur and k["segment"] == seg_cur:                 # (the break comes before the relabelling, :329-333)
                k["segment"] = seg_old
        self.yaw_drift, self.r_drift, self.t_drift = out["yaw_drift"], out["r_drift"].copy(), out["t_drift"].copy()
        for k in self.kfs[pos[-1] + 1:]:                                 # :344-352
            k["t"], k["r"] = self.r_drift @ k["origin_t"] + self.t_drift, self.r_drift @ k["origin_r"]
        self.update_visualization()
        return {"yaw_drift": self.yaw_drift, "r_drift": self.r_drift.copy(), "t_drift": self.t_drift.copy(), "stats": st,
                "n_nodes": len(rng), "skipped": int(np.sum(skip))}

    def update_visualization(self):                                      # :358-378
        self.total_length, self.last_P = 0.0, np.zeros(3)
        for k in self.kfs:
            self.total_length += float(np.linalg.norm(k["t"] - self.last_P))
            self.last_P = k["t"]

    def resample(self):                                                  # :44-76
        if len(self.kfs) < self.max_frame_num:
            return []
        keep, m = resample_walk([k["t"] for k in self.kfs], [k["has_loop"] or k["is_looped"] for k in self.kfs],
                                self.total_length / (0.8 * self.max_frame_num))
        self.min_margin = min(self.min_margin, m)
        erased = [k["global_index"] for k, kp in zip(self.kfs, keep) if not kp]
        self.kfs = [k for k, kp in zip(self.kfs, keep) if kp]
        self.update_visualization()
        return erased

    def snapshot(self):
        kfs = [{f: (np.array(v) if isinstance(v, np.ndarray) else v) for f, v in k.items()} for k in self.kfs]   # (copies)
        return {"kf": kfs, "header": np.array([k["header"] for k in self.kfs]),
                "segment_index": np.array([k["segment"] for k in self.kfs], np.int32), "total_length": self.total_length,
                "last_P": np.array(self.last_P), "yaw_drift": self.yaw_drift, "r_drift": np.array(self.r_drift), "t_drift": np.array(self.t_drift),
                "earliest_loop_index": self.earliest, "cur_seg_index": self.cur_seg, "max_seg_index": self.max_seg}


class DevSession:
    """One session of a device database behind RefDb's method names."""

    def __init__(self, db, session=0):
        self.db, self.s = db, session

    def add(self, header, P, R):
        return int(self.db.add([self.s], [header], P, R)[0])

    def new_segment(self):
        self.db.new_segment(self.s)

    def set_loop(self, cur, old):
        self.db.set_loop(cur, old, self.s)

    def update(self, loop_kf, rel_t, rel_q, rel_yaw, W, header0, P0, R0):
        return int(self.db.update([self.s], [loop_kf], rel_t, rel_q, [rel_yaw], W, [header0], P0, R0)[0])

    def optimize(self, cur_index, max_iterations=5):
        return self.db.optimize([self.s], [cur_index], max_iterations)[0]

    def resample(self):
        return [int(x) for x in self.db.resample(self.s)]

    def snapshot(self):
        return self.db.download(self.s)


INT_KEYS = ("global_index", "has_loop", "is_looped", "loop_index")


def ints_of(snap):
    return ([tuple(int(k[f]) for f in INT_KEYS) for k in snap["kf"]], [float(h) for h in snap["header"]],
            [int(s) for s in snap["segment_index"]], snap["earliest_loop_index"], snap["cur_seg_index"], snap["max_seg_index"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def snapshots_identical(a, b):
    if ints_of(a) != ints_of(b):
        return False
    for ka, kb in zip(a["kf"], b["kf"]):
        if not all(same_bits(np.asarray(ka[f], float), np.asarray(kb[f], float)) for f in ("origin_t", "origin_r", "t", "r", "loop_info")):
            return False
    return all(same_bits(np.asarray(a[f], float), np.asarray(b[f], float)) for f in ("total_length", "last_P", "yaw_drift", "r_drift", "t_drift"))


def compare(got, want, tol, tol_origin=None):
    """Integer state exact; poses, loop_info, total_length and the drift within tol (times the scale of the positions, yaw
    times 180 degrees, as check_against_golden of tests/test_posegraph.py applies it)."""
    assert ints_of(got) == ints_of(want)
    to = tol if tol_origin is None else tol_origin
    scale = max(1.0, max(float(np.abs(k["t"]).max()) for k in want["kf"]))
    for g, w in zip(got["kf"], want["kf"]):
        assert np.abs(g["origin_t"] - w["origin_t"]).max() <= to * scale and np.abs(g["origin_r"] - w["origin_r"]).max() <= to
        assert np.abs(g["loop_info"] - w["loop_info"]).max() <= to * scale
        assert np.abs(g["t"] - w["t"]).max() < tol * scale, (g["global_index"], g["t"], w["t"])
        assert np.abs(g["r"] - w["r"]).max() < tol
    assert abs(got["total_length"] - want["total_length"]) < tol * max(1.0, want["total_length"])
    assert np.abs(got["last_P"] - want["last_P"]).max() < tol * scale
    assert abs((got["yaw_drift"] - want["yaw_drift"] + 180.0) % 360.0 - 180.0) < tol * 180.0
    assert np.abs(got["r_drift"] - want["r_drift"]).max() < tol and np.abs(got["t_drift"] - want["t_drift"]).max() < tol * scale


def compare_result(got, want, tol):
    gs, ws = got["stats"], want["stats"]
    n = ws["iterations"]
    assert gs["iterations"] == n and gs["termination"] == ws["termination"] and list(gs["it_flags"]) == list(ws["it_flags"])
    assert gs["num_successful_steps"] == ws["num_successful_steps"] and gs["num_unsuccessful_steps"] == ws["num_unsuccessful_steps"]
    assert np.allclose(np.asarray(gs["it_cost"])[:n], np.asarray(ws["it_cost"])[:n], rtol=tol, atol=0)
    assert abs((got["yaw_drift"] - want["yaw_drift"] + 180.0) % 360.0 - 180.0) < tol * 180.0
    scale = max(1.0, float(np.abs(want["t_drift"]).max()))
    assert np.abs(got["r_drift"] - want["r_drift"]).max() < tol and np.abs(got["t_drift"] - want["t_drift"]).max() < tol * scale


def header_of(k):
    return 100.0 + 0.05 * k


def loop_args(info):
    """loop_info (t, q as w x y z, yaw) -> relative_t, relative_q (x y z w), relative_yaw."""
    return info[0:3].copy(), np.array([info[4], info[5], info[6], info[3]]), float(info[7])


def feed(dbs, kfs, start=0, stop=None, W=10, loops=None, solve=None):
    """add -> set_loop -> update for keyframes [start, stop) of a synthetic list, the same calls on every database. The
    update of keyframe k also plays the solved frame that slides out of the window: keyframe k - 3 takes a slightly moved
    origin pose. loops: {cur: (old, loop_info)} in place of the list's own. solve: called with the optimize_index whenever
    an update returns one (start_global_optimization). -> optimize_index of every update."""
    out = []
    for k in range(start, len(kfs) if stop is None else stop):
        kf = kfs[k]
        lp = loops.get(k) if loops is not None else ((kf["loop_index"], kf["loop_info"]) if kf["has_loop"] else None)
        j = k - 3
        h0 = header_of(j) if j >= 0 else -1.0
        P0 = kfs[max(j, 0)]["origin_t"] + 1e-3 * np.array([math.sin(j), math.cos(j), 0.5])
        R0 = kfs[max(j, 0)]["origin_r"]
        res = []
        for d in dbs:
            assert d.add(header_of(k), kf["origin_t"], kf["origin_r"]) == k
            if lp is not None:
                d.set_loop(k, lp[0])
                res.append(d.update(k, *loop_args(np.asarray(lp[1], float)), W, h0, P0, R0))
            else:
                res.append(d.update(-1, np.zeros(3), np.array([0, 0, 0, 1.0]), 0.0, W, h0, P0, R0))
        assert len(set(res)) == 1, res
        out.append(res[0])
        if solve is not None and res[0] >= 0:
            solve(res[0])
    return out


def truth_poses(n, laps, radius=8.0):
    """The ground truth of synth.make_loop_keyframes (translations, rotations, yaw in degrees)."""
    ang = np.linspace(0, 2 * np.pi * laps, n)
    t = np.stack([radius * np.cos(ang), radius * np.sin(ang), 0.3 * np.sin(3 * ang)], 1)
    ypr = np.stack([np.rad2deg(ang) + 90.0, 4.0 * np.sin(2 * ang), 3.0 * np.cos(ang)], 1)
    ypr[:, 0] = (ypr[:, 0] + 180.0) % 360.0 - 180.0
    return t, [synth._ypr_to_R(a) for a in ypr], ypr[:, 0]


def true_loop(truth, k, old):
    t, R, yaw = truth
    info = np.zeros(8)
    info[0:3], info[3], info[7] = R[old].T @ (t[k] - t[old]), 1.0, (yaw[k] - yaw[old] + 180.0) % 360.0 - 180.0
    return old, info


# ---- 1. entry points ---------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_validate_arguments():
    lib = kdb.bind(abi.load_product())
    for sym in ("create", "destroy", "get_device", "clear", "size", "add", "new_segment", "set_loop", "get_pose", "update", "optimize",
                "resample", "download"):
        assert hasattr(lib, "vio_keyframe_db_" + sym), sym
    assert hasattr(lib, "vio_estimator_set_drift")
    h = C.c_void_p()
    assert lib.vio_keyframe_db_create(0, 64, 1, 500, C.byref(h)) == abi.VIO_EINVAL
    assert lib.vio_keyframe_db_create(1, 1, 1, 500, C.byref(h)) == abi.VIO_EINVAL
    assert lib.vio_keyframe_db_create(1, 64, 0, 500, C.byref(h)) == abi.VIO_EINVAL
    assert lib.vio_keyframe_db_create(1, 64, 1, 0, C.byref(h)) == abi.VIO_EINVAL
    assert lib.vio_keyframe_db_create(1, 64, 1, 500, None) == abi.VIO_EINVAL
    n = C.c_int32(0)
    assert lib.vio_keyframe_db_size(None, 0, C.byref(n)) == abi.VIO_EINVAL
    assert lib.vio_keyframe_db_clear(None, 0) == abi.VIO_EINVAL
    assert lib.vio_keyframe_db_add(None, 0, None, None, None, None, None) == abi.VIO_EINVAL
    assert lib.vio_keyframe_db_optimize(None, 0, None, None, 5, None, None, None, None) == abi.VIO_EINVAL
    assert lib.vio_estimator_set_drift(None, 0, None, None) == abi.VIO_EINVAL
    if not os.path.exists("/dev/kfd"):                                  # no device: like every other context, no CPU fallback
        assert lib.vio_keyframe_db_create(1, 64, 1, 500, C.byref(h)) == abi.VIO_ENODEV


# ---- 2. the list passes on the SIMT emulator ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul():
    # (-fno-builtin-sin / -cos: g++ would merge sin(x) and cos(x) into one sincos(x), which is not the same libm entry as
    # the sin and cos the product's host object calls and differs from them in the last bit for a few arguments)
    l = H.build_emul_lib("simt_kfdb.cpp", "libvio_simt_kfdb.so", "VIO_SIMT", extra_flags=("-fno-builtin-sin", "-fno-builtin-cos"))
    kfp = C.POINTER(pg.VioPoseGraphKeyframe)
    l.simt_kfdb_build.argtypes = [kfp, C.c_int, C.c_int, C.c_double] + [C.c_int] * 4 + [_ip, _ip, _dp, _ip, _ip, _ip, _dp, _ip, _dp]
    l.simt_kfdb_apply.argtypes = [kfp, _dp, _ip] + [C.c_int] * 7 + [_ip, _ip, _dp, _dp, _ip, _dp, _dp, _dp]
    l.simt_kfdb_resample.argtypes = [kfp, _dp, _ip, C.c_int, C.c_int, C.c_int, C.c_int, kfp, _dp, _ip, _dp, _ip, _ip]
    return l


def emul_list(m, seed, n_loops, n_before, tail):
    """n_before keyframes the graph does not reach, the m of a synthetic lap (the last n_loops carry loops), `tail`
    keyframes after cur_index. The current poses differ from the origin poses (an earlier drift)."""
    rng = np.random.default_rng(seed)
    lap, _, _ = synth.make_loop_keyframes(m, seed, n_loops=n_loops, first_index=n_before)
    def stray(src, gi, step):
        k = {f: np.array(src[f], float).copy() if f not in INT_KEYS else src[f] for f in src}
        k["origin_t"] = src["origin_t"] + step
        k.update(global_index=gi, has_loop=0, is_looped=0, loop_index=-1, loop_info=np.zeros(8))
        return k
    walk = np.cumsum(0.3 * rng.standard_normal((n_before + tail + 1, 3)), 0)
    kfs = [stray(lap[0], i, walk[i] - walk[n_before]) for i in range(n_before)] + lap
    kfs += [stray(lap[-1], n_before + m + i, walk[n_before + 1 + i] - walk[n_before]) for i in range(tail)]
    Rd, td = synth._ypr_to_R([3.0, 0, 0]), np.array([0.4, -0.2, 0.1])
    for k in kfs:
        k["t"], k["r"] = Rd @ k["origin_t"] + td, Rd @ np.asarray(k["origin_r"]).reshape(3, 3)
    seg = np.array([(i * 3) // max(len(kfs), 1) for i in range(len(kfs))], np.int32)
    return kfs, seg


def total_length_of(ts):
    s, last = 0.0, (0.0, 0.0, 0.0)
    for t in ts:
        s += norm3(t, last)
        last = t
    return s


EMUL_CASES = [  # m (graph nodes), loops, max_frame_num, list_size (None: the list's), keyframes before the graph, tail
    (2, 1, 500, None, 0, 0),          # the smallest legal graph
    (4, 1, 500, None, 0, 1),          # fewer than five predecessors
    (7, 2, 500, None, 3, 0),          # two loops onto the same old keyframe; a late earliest_loop_index
    (63, 5, 500, None, 0, 0), (64, 5, 500, None, 2, 1), (65, 6, 500, None, 0, 70),   # ballot boundaries
    (129, 9, 500, None, 5, 0),
    (129, 9, 20, 500, 0, 1),          # skipped nodes around the first wave boundaries
    (300, 12, 40, 300, 0, 0),         # most nodes skipped, more than one trip of the 256 work-items
    (300, 12, 40, 300, 7, 70),
]
LANE_ORDERS = [0, 1, 2, 3]            # forward, reverse, two seeded shuffles: every case at every one


@pytest.mark.parametrize("order", LANE_ORDERS)
@pytest.mark.parametrize("m,n_loops,mfn,ls,n_before,tail", EMUL_CASES)
def test_build_and_apply_passes_match_the_host_functions_bit_for_bit(emul, m, n_loops, mfn, ls, n_before, tail, order):
    plib = pg.bind_host(abi.load_product(), "vio")
    kfs, seg = emul_list(m, 7 + m, n_loops, n_before, tail)
    n, first, cur = len(kfs), n_before, n_before + m - 1
    rng_kfs = kfs[first:cur + 1]
    total = total_length_of([k["t"] for k in kfs])
    list_size = n if ls is None else ls
    want, skip = pg.build_with(plib, "vio", rng_kfs, total, max_frame_num=mfn, list_size=list_size)
    if m == 7:
        assert sorted(k["loop_index"] for k in rng_kfs if k["has_loop"]) == [first, first]
    if mfn < 100:   # the case must not degenerate: skip runs longer than five, and one that crosses a wave boundary
        runs, r = [], 0
        for s in list(skip) + [0]:
            if s:
                r += 1
            elif r:
                runs.append(r)
                r = 0
        assert max(runs) > 5 and 0 < int(skip.sum()) < m
        assert m < 300 or any(skip[b - 1] and skip[b] for b in range(64, m, 64))
    # -- build
    cap, ecap = n + 3, 6 * (n + 3)
    arr = pg.keyframes_struct(kfs)
    rng_arr = C.cast(C.addressof(arr) + first * C.sizeof(pg.VioPoseGraphKeyframe), C.POINTER(pg.VioPoseGraphKeyframe))
    hdr, col = np.full(4, -7, np.int32), np.full(cap, -7, np.int32)
    node0, ypr = np.full((cap, 4), np.nan), np.full((cap, 3), np.nan)
    ei, ej, ek, meas = np.full(ecap, -7, np.int32), np.full(ecap, -7, np.int32), np.full(ecap, -7, np.int32), np.full((ecap, 6), np.nan)
    dskip = np.full(cap, -7, np.int32)
    rc = emul.simt_kfdb_build(rng_arr, m, cap, total, mfn, int(list_size < mfn), 5, order, hdr.ctypes.data_as(_ip), col.ctypes.data_as(_ip),
                              node0.ctypes.data_as(_dp), ei.ctypes.data_as(_ip), ej.ctypes.data_as(_ip), ek.ctypes.data_as(_ip),
                              meas.ctypes.data_as(_dp), dskip.ctypes.data_as(_ip), ypr.ctypes.data_as(_dp))
    assert rc == 0
    ne = len(want.edge_i)
    assert np.array_equal(dskip[:m], skip.astype(np.int32)) and (dskip[m:] == -7).all()
    assert same_bits(node0[:m, 1:], want.t) and same_bits(ypr[:m], want.ypr) and same_bits(node0[:m, 0], want.ypr[:, 0])
    assert np.isnan(node0[m:]).all() and np.isnan(ypr[m:]).all()
    assert np.array_equal(ei[:ne], want.edge_i) and np.array_equal(ej[:ne], want.edge_j) and np.array_equal(ek[:ne], want.edge_kind.astype(np.int32))
    assert same_bits(meas[:ne], want.edge_meas)
    assert (ei[ne:] == -7).all() and (ej[ne:] == -7).all() and (ek[ne:] == -7).all() and np.isnan(meas[ne:]).all()
    # col as vio_posegraph_optimize numbers the unknowns: nodes an edge names, except the fixed one, in order
    used = np.zeros(m, bool)
    used[want.edge_i], used[want.edge_j] = True, True
    used[0] = False
    wcol = np.where(used, 4 * (np.cumsum(used) - 1), -1).astype(np.int32)
    assert np.array_equal(col[:m], wcol) and (col[m:] == -7).all()
    assert list(hdr) == [m, ne, 4 * int(used.sum()), 5]
    # -- the solve (restatement), then apply
    solved = want.copy()
    pg.optimize_with(pg.bind_checker(H.oracle_lib(), "oracle"), solved)
    wa = pg.apply_with(plib, "vio", rng_kfs, solved, skip)
    xout = np.full(4 * m + 16, np.nan)
    for k in range(m):
        if wcol[k] >= 0:
            xout[wcol[k]], xout[wcol[k] + 1:wcol[k] + 4] = solved.ypr[k, 0], solved.t[k]
        else:   # not part of the program: the solver left it alone
            assert same_bits(solved.t[k], want.t[k]) and same_bits(solved.ypr[k], want.ypr[k])
    headers = np.array([header_of(i) for i in range(n)])
    seg_cur, seg_old = int(seg[cur]), int(seg[rng_kfs[-1]["loop_index"]])   # (global_index = position here)
    dseg = seg.copy()
    state, drift = np.full(17, np.nan), np.full(13, np.nan)
    before = [bytes(arr[i]) for i in range(n)]
    rc = emul.simt_kfdb_apply(arr, headers.ctypes.data_as(_dp), dseg.ctypes.data_as(_ip), n, cap, first, cur, seg_cur, seg_old, order,
                              hdr.ctypes.data_as(_ip), col.ctypes.data_as(_ip), node0.ctypes.data_as(_dp), xout.ctypes.data_as(_dp),
                              dskip.ctypes.data_as(_ip), ypr.ctypes.data_as(_dp), state.ctypes.data_as(_dp), drift.ctypes.data_as(_dp))
    assert rc == 0
    for i in range(first):
        assert bytes(arr[i]) == before[i]
    for j in range(m):
        a = arr[first + j]
        assert same_bits(np.array(a.t), wa["t"][j]) and same_bits(np.array(a.r).reshape(3, 3), wa["r"][j]), j
        assert same_bits(np.array(a.origin_t), np.asarray(kfs[first + j]["origin_t"], float))
    assert drift[0] == wa["yaw_drift"] and same_bits(drift[1:10].reshape(3, 3), wa["r_drift"]) and same_bits(drift[10:13], wa["t_drift"])
    assert same_bits(state[4:17], drift)
    for i in range(cur + 1, n):   # the tail follows the drift (:344-352)
        assert same_bits(np.array(arr[i].t), move(wa["r_drift"], kfs[i]["origin_t"], wa["t_drift"]))
        assert same_bits(np.array(arr[i].r).reshape(3, 3), mul3(wa["r_drift"], np.asarray(kfs[i]["origin_r"]).reshape(3, 3)))
    wseg = seg.copy()
    for i in range(first, cur):
        if wseg[i] == seg_cur:
            wseg[i] = seg_old
    assert np.array_equal(dseg, wseg)
    assert state[0] == total_length_of([np.array(arr[i].t) for i in range(n)]) and same_bits(state[1:4], np.array(arr[n - 1].t))


@pytest.mark.parametrize("order", LANE_ORDERS)
@pytest.mark.parametrize("n,n_loops,mfn", [(2, 1, 2), (7, 2, 5), (64, 3, 20), (65, 3, 20), (129, 5, 40), (300, 12, 40), (300, 12, 300)])
def test_resample_pass_matches_the_restatement(emul, n, n_loops, mfn, order):
    kfs, seg = emul_list(n, 40 + n, n_loops, 0, 0)
    total = total_length_of([k["t"] for k in kfs])
    keep, _ = resample_walk([k["t"] for k in kfs], [k["has_loop"] or k["is_looped"] for k in kfs], total / (0.8 * mfn))
    if n >= 64:
        assert 0 < sum(keep) < n
    cap = n + 5
    src, dst = pg.keyframes_struct(kfs), (pg.VioPoseGraphKeyframe * cap)()
    C.memset(dst, 0xff, C.sizeof(dst))
    hdr = np.array([header_of(i) for i in range(n)])
    dh, ds = np.full(cap, np.nan), np.full(cap, -7, np.int32)
    state = np.full(17, np.nan)
    state[0] = total
    erased, counts = np.full(cap, -7, np.int32), np.full(2, -7, np.int32)
    sseg = seg.copy()
    rc = emul.simt_kfdb_resample(src, hdr.ctypes.data_as(_dp), sseg.ctypes.data_as(_ip), n, cap, mfn, order, dst, dh.ctypes.data_as(_dp),
                                 ds.ctypes.data_as(_ip), state.ctypes.data_as(_dp), erased.ctypes.data_as(_ip), counts.ctypes.data_as(_ip))
    assert rc == 0
    kept = [i for i in range(n) if keep[i]]
    gone = [kfs[i]["global_index"] for i in range(n) if not keep[i]]
    assert list(counts) == [len(kept), len(gone)]
    assert list(erased[:len(gone)]) == gone and (erased[len(gone):] == -7).all()
    for r, i in enumerate(kept):
        assert bytes(dst[r]) == bytes(src[i]) and dh[r] == hdr[i] and ds[r] == seg[i]
    assert np.isnan(dh[len(kept):]).all() and (ds[len(kept):] == -7).all()
    assert all(b == 0xff for b in bytes(dst[len(kept)]))
    assert state[0] == total_length_of([kfs[i]["t"] for i in kept]) and same_bits(state[1:4], np.asarray(kfs[kept[-1]]["t"], float))
    assert np.isnan(state[4:]).all()


# ---- 8. vio_estimator_set_drift (the estimator's host state: no device involved) -------------------------------------------
def test_estimator_set_drift_reaches_status_and_the_corrected_window():
    cfg = abi.default_config()
    P = cfg.window_size + 1
    est = pkg.estimator.Estimator(cfg, np.array([0.0, 0.065, 0.0]), np.diag([1.0, -1.0, -1.0]), n_seq=2)
    rng = np.random.default_rng(3)
    Rs = np.array([synth._ypr_to_R(a) for a in rng.uniform(-40, 40, (P, 3))])
    est.set_initial_state([float(k) for k in range(P)], rng.standard_normal((P, 3)), Rs, np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 3)), seq=1)
    rd, td = synth._ypr_to_R([12.5, 0, 0]), np.array([0.7, -1.3, 0.25])
    est.set_drift(rd, td, seq=1)
    st = est.status(1)
    assert same_bits(np.array(st.r_drift).reshape(3, 3), rd) and same_bits(np.array(st.t_drift), td)
    st0 = est.status(0)                                                  # the other sequence keeps the identity
    assert same_bits(np.array(st0.r_drift).reshape(3, 3), np.eye(3)) and same_bits(np.array(st0.t_drift), np.zeros(3))
    w = est.window(1)
    cP, cR = est.corrected_window(1)
    for i in range(P):   # update_loop_correction (VINS.cpp:302-331) on get_window's values, bit for bit
        assert same_bits(cP[i], move(rd, w["Ps"][i], td)) and same_bits(cR[i], mul3(rd, w["Rs"][i]))
    lib = est.lib
    assert lib.vio_estimator_set_drift(est._h, 2, rd.ctypes.data_as(_dp), td.ctypes.data_as(_dp)) == abi.VIO_EINVAL
    assert lib.vio_estimator_set_drift(est._h, -1, rd.ctypes.data_as(_dp), td.ctypes.data_as(_dp)) == abi.VIO_EINVAL
    assert lib.vio_estimator_set_drift(est._h, 1, None, td.ctypes.data_as(_dp)) == abi.VIO_EINVAL
    assert lib.vio_estimator_set_drift(est._h, 1, rd.ctypes.data_as(_dp), None) == abi.VIO_EINVAL
    est.clear(1)
    st = est.status(1)
    assert same_bits(np.array(st.r_drift).reshape(3, 3), np.eye(3)) and same_bits(np.array(st.t_drift), np.zeros(3))
    est.close()


# ---- device ------------------------------------------------------------------------------------------------------------
# keyframes -> (seed, laps, loops): None = the list's own (the last keyframes onto the lap before, a step or so off);
# (cur, old) pairs = true loops between keyframes at the same place of different laps. max_frame_num = 30 below.
SINGLE = {2: (11, 1.0, [(1, 0)]), 7: (12, 2.0, [(3, 0), (6, 0)]), 65: (13, 1.15, None), 130: (29, 1.15, None)}


def single_list(n):
    seed, laps, pairs = SINGLE[n]
    kfs = synth.make_loop_keyframes(n, seed, n_loops=0 if pairs else 2 + n // 16, laps=laps, yaw_drift_deg=0.3, pos_drift=0.03)[0]
    return kfs, ({c: true_loop(truth_poses(n, laps), c, o) for c, o in pairs} if pairs else None)


def run_single(dbs, n, check_before=None):
    """add -> set_loop -> update for the whole list with an optimize whenever update asks for one (the keyframe that slid
    out of the window has a loop), then one at the last keyframe (it carries a loop). -> list, loops, optimize_index of
    every update, [(cur_index, result per database)]."""
    kfs, loops = single_list(n)
    solves = []
    def solve(cur):
        if not solves and check_before is not None:
            check_before()
        solves.append((cur, [d.optimize(cur) for d in dbs]))
    opt = feed(dbs, kfs, loops=loops, solve=solve)
    solve(n - 1)
    return kfs, loops, opt, solves


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 7, 65, 130])
def test_one_session_follows_the_restatement(n):
    db = kdb.KeyFrameDatabase(n_sessions=1, max_keyframes=160, max_graphs=1, max_frame_num=30)
    try:
        dev, ref = DevSession(db), RefDb(max_frame_num=30)
        # everything before the first solve: only the pose arithmetic of add / update separates the two
        kfs, loops, opt, solves = run_single([dev, ref], n, check_before=lambda: compare(dev.snapshot(), ref.snapshot(), TOL_ORACLE))
        # update reports the keyframe that slid out of the window when it has a loop: keyframe k - 3 at the update of k
        has = set(loops) if loops else {k for k in range(n) if kfs[k]["has_loop"]}
        assert opt == [(k - 3 if k - 3 in has else -1) for k in range(n)] and n - 1 in has
        assert [c for c, _ in solves] == sorted(h for h in has if h < n - 3) + [n - 1]
        assert ref.min_margin > MARGIN
        for _, (rd, rr) in solves:
            compare_result(rd, rr, TOL_GPU)
        if n >= 65:
            assert solves[-1][1][1]["skipped"] > n // 2   # the list is longer than max_frame_num: most nodes are resampled away
        compare(dev.snapshot(), ref.snapshot(), TOL_GPU, tol_origin=TOL_ORACLE)
        assert db.size() == n and db.device() >= 0
        # add with a non-trivial drift: r_drift P + t_drift, r_drift R of the DEVICE's drift at the oracle's tolerance
        # (only the pose arithmetic in between), and the restatement's result at the device's
        s0 = dev.snapshot()
        P, R = kfs[-1]["origin_t"] + np.array([0.3, 0.1, 0.0]), kfs[-1]["origin_r"]
        assert dev.add(header_of(n), P, R) == n and ref.add(header_of(n), P, R) == n
        s1 = dev.snapshot()
        scale = max(1.0, float(np.abs(P).max()))
        assert np.abs(s1["kf"][n]["t"] - (s0["r_drift"] @ P + s0["t_drift"])).max() < TOL_ORACLE * scale
        assert np.abs(s1["kf"][n]["r"] - s0["r_drift"] @ R).max() < TOL_ORACLE
        assert abs(s1["total_length"] - (s0["total_length"] + np.linalg.norm(s1["kf"][n]["t"] - s0["last_P"]))) < TOL_ORACLE * s0["total_length"]
        assert np.abs(s0["t_drift"]).max() > 1e-3 and np.abs(s0["r_drift"] - np.eye(3)).max() > 0   # (non-trivial)
        compare(s1, ref.snapshot(), TOL_GPU, tol_origin=TOL_ORACLE)
        Pg, Rg, hg = db.get_pose([0], [n])
        assert same_bits(Pg[0], s1["kf"][n]["t"]) and same_bits(Rg[0], s1["kf"][n]["r"]) and hg[0] == header_of(n)
    finally:
        db.close()


CHAIN = dict(n=90, seed=10, laps=3.0, mfn=40)


def run_chain(dbs, log=None):
    """optimize at a first loop; more adds; a second loop whose old keyframe lies before the first; optimize; resample;
    optimize once more on the compacted list. -> per database the results of every step."""
    c = CHAIN
    kfs, _, _ = synth.make_loop_keyframes(c["n"], c["seed"], n_loops=0, laps=c["laps"], yaw_drift_deg=0.3, pos_drift=0.03)
    truth = truth_poses(c["n"], c["laps"])
    loops = {55: true_loop(truth, 55, 25), 56: true_loop(truth, 56, 26), 70: true_loop(truth, 70, 10), 71: true_loop(truth, 71, 41)}
    out = [[] for _ in dbs]
    def step(fn):
        for d, o in zip(dbs, out):
            o.append(fn(d))
        if log is not None:
            log()
    feed(dbs, kfs, 0, 60, loops=loops)
    step(lambda d: d.optimize(55))          # earliest_loop_index = 25; keyframes 56 .. 59 follow the drift
    step(lambda d: d.optimize(56))
    step(lambda d: d.new_segment())         # keyframes 60 .. 74 are segment 1
    feed(dbs, kfs, 60, 75, loops=loops)     # ... and take the new drift
    step(lambda d: d.optimize(70))          # ... 10: the graph grows at the front; 60 .. 69 join segment 0, 70 itself does not
    feed(dbs, kfs, 75, 90, loops=loops)     # cur_seg_index is 0 again
    step(lambda d: d.resample())
    step(lambda d: d.optimize(71))          # on the compacted list; 70 joins segment 0 now
    step(lambda d: d.resample())            # below max_frame_num now: the early return
    return out


@pytest.mark.gpu
def test_chain_of_optimizes_adds_and_a_resample_follows_the_restatement():
    db = kdb.KeyFrameDatabase(n_sessions=1, max_keyframes=96, max_graphs=1, max_frame_num=CHAIN["mfn"])
    try:
        dev, ref = DevSession(db), RefDb(max_frame_num=CHAIN["mfn"])
        snaps = []
        od, orf = run_chain([dev, ref], log=lambda: snaps.append((dev.snapshot(), ref.snapshot())))
        assert ref.min_margin > MARGIN
        for (a, b) in snaps:
            compare(a, b, TOL_GPU, tol_origin=TOL_ORACLE)
        for i in (0, 1, 3, 5):
            compare_result(od[i], orf[i], TOL_GPU)
        assert [snaps[i][1]["earliest_loop_index"] for i in (0, 1, 3)] == [25, 25, 10]
        assert orf[3]["n_nodes"] == 61 and orf[3]["skipped"] > 10
        seg = dict(zip([k["global_index"] for k in snaps[3][1]["kf"]], snaps[3][1]["segment_index"]))
        assert [seg[g] for g in (59, 60, 69, 70, 71, 74)] == [0, 0, 0, 1, 1, 1] and snaps[3][1]["cur_seg_index"] == 0
        erased = orf[4]
        assert od[4] == erased and len(erased) > 30 and erased == sorted(erased)        # the erase list is exact
        final = snaps[-1][1]
        alive = [k["global_index"] for k in final["kf"]]
        for gi in (10, 25, 26, 41, 55, 56, 70, 71):                                    # has_loop / is_looped survive
            assert gi in alive
        assert od[6] == [] and orf[6] == [] and db.size() == len(alive) < CHAIN["mfn"]
        seg = dict(zip(alive, final["segment_index"]))
        assert final["max_seg_index"] == 1 and seg[70] == 0 and seg[71] == 1 and seg[74] == 1 and seg[89] == 0
    finally:
        db.close()


@pytest.mark.gpu
def test_batch_of_three_sessions_equals_three_single_contexts():
    sizes = [2, 65, 130]
    big = kdb.KeyFrameDatabase(n_sessions=4, max_keyframes=160, max_graphs=3, max_frame_num=30)
    singles = [kdb.KeyFrameDatabase(n_sessions=1, max_keyframes=160, max_graphs=1, max_frame_num=30) for _ in sizes]
    try:
        for s, n in enumerate(sizes):
            kfs, loops = single_list(n)
            feed([DevSession(big, s), DevSession(singles[s])], kfs, loops=loops)
        kfs, loops = single_list(7)
        feed([DevSession(big, 3)], kfs, loops=loops)                    # a session no call below names
        idle = big.download(3)
        # at the first loop of every list (earliest_loop_index = its old keyframe, a tail behind it), then at the last
        firsts = {2: 1, 65: min(k for k, kf in enumerate(single_list(65)[0]) if kf["has_loop"]),
                  130: min(k for k, kf in enumerate(single_list(130)[0]) if kf["has_loop"])}
        for cur in ([firsts[n] for n in sizes], [n - 1 for n in sizes]):
            res = big.optimize([2, 0, 1], [cur[2], cur[0], cur[1]])
            res = [res[1], res[2], res[0]]
            for s, n in enumerate(sizes):
                one = singles[s].optimize([0], [cur[s]])[0]
                compare_result(res[s], one, TOL_GPU)
                compare(big.download(s), singles[s].download(0), TOL_GPU)
        assert snapshots_identical(big.download(3), idle)
        before = [big.download(s) for s in (0, 2, 3)]
        big.optimize([1], [sizes[1] - 1])
        assert all(snapshots_identical(big.download(s), b) for s, b in zip((0, 2, 3), before))
    finally:
        big.close()
        for d in singles:
            d.close()


@pytest.mark.gpu
def test_update_search_cutoff_and_wrong_loop_thresholds():
    W, n = 3, 12
    db = kdb.KeyFrameDatabase(n_sessions=1, max_keyframes=32, max_graphs=1)
    try:
        dev, ref = DevSession(db), RefDb()
        kfs, _, _ = synth.make_loop_keyframes(n, 3, n_loops=0)
        for k in range(n):
            for d in (dev, ref):
                assert d.add(header_of(k), kfs[k]["origin_t"], kfs[k]["origin_r"]) == k
        q, P0, R0 = np.array([0, 0, 0, 1.0]), np.array([9.0, 8.0, 7.0]), synth._ypr_to_R([10.0, 20.0, 30.0])
        # depth 1 = the newest keyframe; 2 W + 1 keyframes are examined
        for depth, found in ((2 * W, True), (2 * W + 1, True), (2 * W + 2, False)):
            k = n - depth
            for d in (dev, ref):
                assert d.update(-1, np.zeros(3), q, 0.0, W, header_of(k), P0 + depth, R0) == -1
            got = dev.snapshot()["kf"][k]
            assert same_bits(got["origin_t"], (P0 + depth) if found else np.asarray(kfs[k]["origin_t"], float))
            assert same_bits(got["origin_r"], R0 if found else np.asarray(kfs[k]["origin_r"], float))
            compare(dev.snapshot(), ref.snapshot(), TOL_ORACLE)
        # wrong loop: |yaw| > 30.0 or |t| > 10.0, at the threshold (kept) and just above (removed)
        cases = [(8, 30.0, [1.0, 0, 0], 1), (9, -math.nextafter(30.0, 40.0), [1.0, 0, 0], 0), (10, 5.0, [10.0, 0, 0], 1),
                 (11, 5.0, [0, -math.nextafter(10.0, 20.0), 0], 0)]
        for cur, yaw, t, kept in cases:
            for d in (dev, ref):
                d.set_loop(cur, cur - 6)
                # the keyframe is also the one found by header0: start_global_optimization only while it has a loop
                assert d.update(cur, np.array(t, float), np.array([0.1, 0.2, 0.3, 0.9]), yaw, W, header_of(cur), kfs[cur]["origin_t"],
                                kfs[cur]["origin_r"]) == (cur if kept else -1)
            s = dev.snapshot()
            assert s["kf"][cur]["has_loop"] == kept and s["kf"][cur]["loop_index"] == cur - 6 and s["kf"][cur - 6]["is_looped"] == 1
            if kept:
                assert same_bits(s["kf"][cur]["loop_info"], np.array(t + [0.9, 0.1, 0.2, 0.3, yaw], float))   # t, q (w x y z), yaw
            else:
                assert same_bits(s["kf"][cur]["loop_info"], np.zeros(8))
            compare(s, ref.snapshot(), TOL_ORACLE)
        before = dev.snapshot()
        with pytest.raises(kdb.KeyframeDbError) as e:
            dev.optimize(9)                                               # its loop was removed (the reference asserts)
        assert e.value.rc == abi.VIO_EINVAL and snapshots_identical(dev.snapshot(), before)
        compare_result(dev.optimize(8), ref.optimize(8), TOL_GPU)         # 2 .. 8: the removed loop of 9 is not an edge
        compare(dev.snapshot(), ref.snapshot(), TOL_GPU, tol_origin=TOL_ORACLE)
    finally:
        db.close()


@pytest.mark.gpu
def test_errors_and_capacity_leave_the_database_unchanged():
    db = kdb.KeyFrameDatabase(n_sessions=2, max_keyframes=10, max_graphs=1)
    try:
        kfs, _, _ = synth.make_loop_keyframes(10, 4, n_loops=0)
        for s, n in ((0, 10), (1, 8)):
            for k in range(n):
                assert db.add([s], [header_of(k)], kfs[k]["origin_t"], kfs[k]["origin_r"])[0] == k
        db.set_loop(5, 1, 0), db.set_loop(7, 3, 0), db.set_loop(6, 2, 1)
        before = [db.download(s) for s in (0, 1)]
        P2, R2, h2 = np.zeros((2, 3)), np.tile(np.eye(3), (2, 1, 1)), [1.0, 2.0]
        bad = [
            (abi.VIO_ECAP, lambda: db.add([1, 0], h2, P2, R2)),             # session 0 is full: session 1 gets nothing either
            (abi.VIO_ECAP, lambda: db.optimize([0, 1], [7, 6])),            # n > max_graphs
            (abi.VIO_EINVAL, lambda: db.optimize([0], [99])),               # unknown index
            (abi.VIO_EINVAL, lambda: db.optimize([0], [4])),                # no loop
            (abi.VIO_EINVAL, lambda: db.set_loop(99, 0, 0)),
            (abi.VIO_EINVAL, lambda: db.set_loop(4, 4, 0)),                 # old_index >= cur_index
            (abi.VIO_EINVAL, lambda: db.set_loop(9, 8, 1)),                 # session 1 has no keyframe 8 / 9
            (abi.VIO_EINVAL, lambda: db.get_pose([0], [10])),
            (abi.VIO_EINVAL, lambda: db.add([1, 1], h2, P2, R2)),           # a session twice in one call
            (abi.VIO_EINVAL, lambda: db.get_pose([0, 0], [1, 2])),
            (abi.VIO_EINVAL, lambda: db.optimize([1, 1], [6, 6])),
            (abi.VIO_EINVAL, lambda: db.update([0, 0], [-1, -1], np.zeros((2, 3)), np.zeros((2, 4)), [0, 0], 10, h2, P2, R2)),
            (abi.VIO_EINVAL, lambda: db.update([0], [42], np.zeros(3), np.zeros(4), [0], 10, [1.0], P2[0], R2[0])),
            (abi.VIO_EINVAL, lambda: db.add([2], [1.0], P2[0], R2[0])),     # no such session
            # the range 3 .. 7 holds keyframe 5, whose loop points to 1, before earliest_loop_index = 3 (the reference asserts)
            (abi.VIO_EINVAL, lambda: db.optimize([0], [7])),
        ]
        for rc, call in bad:
            with pytest.raises(kdb.KeyframeDbError) as e:
                call()
            assert e.value.rc == rc
            assert all(snapshots_identical(db.download(s), b) for s, b in zip((0, 1), before))
        # an erased index is unknown afterwards; the context is still usable
        small = kdb.KeyFrameDatabase(n_sessions=1, max_keyframes=10, max_graphs=1, max_frame_num=8)
        try:
            for k in range(10):
                small.add([0], [header_of(k)], kfs[k]["origin_t"], kfs[k]["origin_r"])
            small.set_loop(9, 0)
            erased = list(small.resample())
            assert erased and 0 not in erased and 9 not in erased
            snap = small.download()
            for call in (lambda: small.get_pose([0], [erased[0]]), lambda: small.set_loop(9, erased[0]), lambda: small.optimize([0], [erased[0]])):
                with pytest.raises(kdb.KeyframeDbError) as e:
                    call()
                assert e.value.rc == abi.VIO_EINVAL and snapshots_identical(small.download(), snap)
            assert small.optimize([0], [9])[0]["stats"]["iterations"] >= 1
        finally:
            small.close()
        assert db.optimize([0], [5])[0]["stats"]["iterations"] >= 1        # 1 .. 5: legal, and now 7 is too
        assert db.optimize([0], [7])[0]["stats"]["iterations"] >= 1
        db.clear(0)
        s = db.download(0)
        assert db.size(0) == 0 and s["earliest_loop_index"] == -1 and s["total_length"] == 0 and same_bits(s["r_drift"], np.eye(3))
        assert db.add([0], [1.0], P2[0], R2[0])[0] == 0 and snapshots_identical(db.download(1), before[1])
    finally:
        db.close()


@pytest.mark.gpu
def test_database_closes_the_loop_end_to_end():
    """One session of 40 keyframes on the drifting lap, one true loop with loop_info from the ground truth: after optimize
    the last keyframe is closer to the truth (the criterion of test_device_closes_the_loop_end_to_end: 0.35 of before)."""
    n = 40
    kfs, _, truth_t = synth.make_loop_keyframes(n, 21, n_loops=0, yaw_drift_deg=0.4, pos_drift=0.05)
    old = n - 1 - int(round(n / 1.15))
    loops = {n - 1: true_loop(truth_poses(n, 1.15), n - 1, old)}
    db = kdb.KeyFrameDatabase(n_sessions=1, max_keyframes=64, max_graphs=1)
    try:
        dev = DevSession(db)
        feed([dev], kfs, loops=loops)
        before = np.linalg.norm(dev.snapshot()["kf"][n - 1]["t"] - truth_t[n - 1])
        res = dev.optimize(n - 1)
        s = dev.snapshot()
        after = np.linalg.norm(s["kf"][n - 1]["t"] - truth_t[n - 1])
        assert after < 0.35 * before
        assert s["earliest_loop_index"] == old and np.abs(res["t_drift"] - s["t_drift"]).max() == 0
    finally:
        db.close()
