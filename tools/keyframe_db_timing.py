#!/usr/bin/env python3
"""Wall time of one optimize4DoFLoopPoseGraph for 1 / 64 / 512 sessions of 200 keyframes with 4 loops each, on the two
routes a caller has. Needs a gfx950 device; writes profiles/keyframe_db_timing.txt (median of --reps with the minimum
beside it).

  resident   one vio_keyframe_db_optimize for all sessions: the graphs are built from the lists on the device, solved and
             applied there; the host uploads a job record per session and downloads the drift and the solve statistics.
  host list  what a caller that keeps its own list does: vio_posegraph_build per session, one batched
             vio_posegraph_optimize, vio_posegraph_apply per session, updatePose and the move of the keyframes after
             cur_index.

Both start from the same lists: the host route's keyframes are downloaded from the database before the timed calls.
Either route is ONE C call from here, so no interpreter work is timed: the host route is the C++ driver
tools/keyframe_db_host_route.cpp (built on first use against csrc/libvio_amd.so), with every buffer allocated beforehand.

The measuring runs in a child process under its own time limit (`timeout -k 10 --limit`), so a device that hangs ends the
tool instead of holding it:

    python tools/keyframe_db_timing.py [--reps 5] [--limit 600] [--out profiles/keyframe_db_timing.txt]
"""
import argparse
import ctypes as C
import importlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_KF, N_LOOPS = 200, 4
_dp, _ip, _u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def line(name, v, unit="ms"):
    return "%-58s %9.3f %s   (median of %d; min %.3f)" % (name, float(np.median(v)), unit, len(v), min(v))


def host_route_driver():
    """tools/libkfdb_host_route.so, built with g++ when missing or older than its source."""
    src, so = os.path.join(ROOT, "tools", "keyframe_db_host_route.cpp"), os.path.join(ROOT, "tools", "libkfdb_host_route.so")
    csrc = os.path.join(ROOT, "vins-mobile_amd", "csrc")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-o", so, src,
                               "-L" + csrc, "-lvio_amd", "-Wl,-rpath," + csrc])
    d = C.CDLL(so)
    d.kfdb_host_route_create.restype = C.c_void_p
    d.kfdb_host_route_create.argtypes = [C.c_int, C.c_int]
    d.kfdb_host_route_destroy.argtypes = [C.c_void_p]
    d.kfdb_host_route_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _ip, C.c_int32, _dp, C.c_int32, _dp, _ip]
    return d


def fill(db, lists):
    """add -> set_loop -> update (loop_info) for every session, all sessions per call."""
    S = len(lists)
    ses = np.arange(S, dtype=np.int32)
    for k in range(N_KF):
        db.add(ses, np.full(S, 100.0 + 0.05 * k), np.array([l[k]["origin_t"] for l in lists]), np.array([l[k]["origin_r"] for l in lists]))
    for k in range(N_KF):
        if not lists[0][k]["has_loop"]:
            continue
        for s in range(S):
            db.set_loop(k, lists[s][k]["loop_index"], s)
        info = np.array([l[k]["loop_info"] for l in lists])
        db.update(ses, np.full(S, k, np.int32), info[:, 0:3], info[:, [4, 5, 6, 3]], info[:, 7], 10, np.full(S, -1.0), np.zeros((S, 3)),
                  np.tile(np.eye(3).reshape(9), (S, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_db_timing.txt"))
    ap.add_argument("--limit", type=int, default=600, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not a.child:   # (this process never opens the device)
        host_route_driver()
        sys.exit(subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps),
                                  "--out", a.out]))
    import torch  # (its HIP runtime first, see __graft_entry__.py)
    pkg = importlib.import_module("vins-mobile_amd")
    kdb, pg, synth, abi = pkg.keyframe_db, pkg.posegraph, pkg.synth, pkg.abi
    lib = pg.bind(kdb.bind(abi.load_product()))
    driver = host_route_driver()
    prop = torch.cuda.get_device_properties(0)
    out = ["keyframe database: tools/keyframe_db_timing.py on one %s (%s, %d CUs), wall time in ms" %
           (prop.name, getattr(prop, "gcnArchName", "?").split(":")[0], prop.multi_processor_count),
           "one optimize4DoFLoopPoseGraph per session: %d keyframes, %d loops, max_iterations 5" % (N_KF, N_LOOPS)]
    pool = [synth.make_loop_keyframes(N_KF, 100 + i, n_loops=N_LOOPS)[0] for i in range(16)]
    for S in (1, 64, 512):
        lists = [pool[s % len(pool)] for s in range(S)]
        first_loop = min(k for k in range(N_KF) if lists[0][k]["has_loop"])
        db = kdb.KeyFrameDatabase(n_sessions=S, max_keyframes=N_KF, max_graphs=S, max_frame_num=500)
        fill(db, lists)
        ses = np.arange(S, dtype=np.int32)
        db.optimize(ses, np.full(S, first_loop, np.int32))          # earliest_loop_index = the first loop's old keyframe
        cur_pos = N_KF - 2                                          # one keyframe follows cur_index: the tail move
        cur = np.full(S, cur_pos, np.int32)
        # the host route's lists: the database's, as they stand now
        kfs, totals, firsts = (pg.VioPoseGraphKeyframe * (S * N_KF))(), np.zeros(S), np.zeros(S, np.int32)
        for s in range(S):
            arr = C.cast(C.addressof(kfs) + s * N_KF * C.sizeof(pg.VioPoseGraphKeyframe), C.POINTER(pg.VioPoseGraphKeyframe))
            n, state, ist = C.c_int32(0), np.zeros(17), np.zeros(3, np.int32)
            assert lib.vio_keyframe_db_download(db._h, s, arr, None, None, N_KF, C.byref(n), state.ctypes.data_as(_dp), ist.ctypes.data_as(_ip)) == 0
            firsts[s] = next(i for i in range(n.value) if arr[i].global_index >= ist[0])
            totals[s] = state[0]
        opt = pg.PoseGraphOptimizer(max_nodes=N_KF, max_edges=6 * N_KF, n_graphs=S)
        route = driver.kfdb_host_route_create(S, N_KF)
        P = lambda x, ty: x.ctypes.data_as(ty)
        td, it_host = np.zeros((S, 3)), C.c_int32(0)
        r_stats = (abi.VioSolveStats * S)()
        r_yd, r_rd, r_td = np.zeros(S), np.zeros((S, 9)), np.zeros((S, 3))
        t_res, t_host = [], []
        for r in range(a.reps + 2):
            t0 = time.perf_counter()
            rc = lib.vio_keyframe_db_optimize(db._h, S, P(ses, _ip), P(cur, _ip), 5, P(r_yd, _dp), P(r_rd, _dp), P(r_td, _dp), r_stats)
            ta = time.perf_counter() - t0
            t0 = time.perf_counter()
            rc2 = driver.kfdb_host_route_run(route, opt._h, kfs, P(firsts, _ip), cur_pos, P(totals, _dp), 500, P(td, _dp), C.byref(it_host))
            tb = time.perf_counter() - t0
            assert rc == 0 and rc2 == 0, (rc, rc2)
            if r >= 2:
                t_res.append(ta * 1e3), t_host.append(tb * 1e3)
        it_res, it_host = sum(st.iterations for st in r_stats), it_host.value
        driver.kfdb_host_route_destroy(route)
        err = float(np.abs(r_td - td).max())
        out.append(line("%3d sessions, one vio_keyframe_db_optimize" % S, t_res))
        out.append(line("%3d x (build + apply + tail) in C, one posegraph_optimize" % S, t_host) +
                   "   iterations %d / %d, t_drift differs by %.1e" % (it_res, it_host, err))
        out.append("    samples: resident %s | host list %s" % (" ".join("%.3f" % v for v in t_res), " ".join("%.3f" % v for v in t_host)))
        opt.close(), db.close()
    txt = "\n".join(out) + "\n"
    print(txt, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
