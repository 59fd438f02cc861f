#!/usr/bin/env python3
"""Times estimator start-up between the landmark dump and the alignment on both routes, on the same problems and the same
box: vio_init_sfm_solve (head, bundle adjustment and extra-frame PnP kernels around one upload and one download) for 1, 64
and 512 problems per call -- device-event time per stage from vio_init_sfm_kernel_ms and wall time of the whole call -- and
the host route, vio_init_relative_pose + vio_init_sfm + one vio_init_pnp per extra frame, for the same problems on as many
host threads as the box grants this process. The problems are eight seeded scenes of 11 frames (the generator of
tests/test_init_sfm_device.py: 150 correspondences between frame l and the newest frame, 210 landmarks seen at least
twice, 9 extra frames of 50 points), round-robin. Warm-up first, then the two routes alternate.
    python tools/init_sfm_timing.py [--repeat 5] > profiles/init_sfm_timing.txt"""
import argparse
import ctypes as C
import importlib
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("vins-mobile_amd")
abi, init_sfm = pkg.abi, pkg.init_sfm
SEEDS = [101, 102, 103, 104, 105, 106, 107, 108]


def host_width():
    for k in ("VIO_AMD_HOST_THREADS", "OMP_NUM_THREADS"):
        if os.environ.get(k, "").isdigit() and int(os.environ[k]) > 0:
            return int(os.environ[k])
    return len(os.sched_getaffinity(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    import torch  # noqa: F401  (HIP runtime first)
    import test_init_sfm_device as T
    scenes = [T._scene(seed, l=1 + seed % 3, n_both=150, n_head=30, n_tail=30, n_extra=9) for seed in SEEDS]

    lib = abi.load_product()
    _dp, _ip, _u8 = T._dp, T._ip, T._u8
    p = lambda a, ty=_dp: a.ctypes.data_as(ty)

    def prepare(sc):                              # everything the host route's three calls read, outside the timed part
        xy0, xy1 = T._correspondences(sc)
        two = np.diff(sc["start"]) >= 2
        ex = [(g, idx[two[idx]], np.ascontiguousarray(xy[two[idx]])) for g, idx, xy in sc["extras"]]
        return dict(sc=sc, xy0=np.ascontiguousarray(xy0), xy1=np.ascontiguousarray(xy1), hint=np.ascontiguousarray(T._hint(sc)), ex=ex)

    def host_route(pr):
        sc = pr["sc"]
        F, n = sc["F"], len(sc["start"]) - 1
        R, t, inl, ok = np.zeros(9), np.zeros(3), C.c_int32(), C.c_int32()
        lib.vio_init_relative_pose(p(pr["xy0"]), p(pr["xy1"]), len(pr["xy0"]), p(pr["hint"]), p(R), p(t), C.byref(inl), C.byref(ok))
        if not ok.value:
            return T.FAIL_RELATIVE
        q, Tw, pts, pok = np.zeros((F, 4)), np.zeros((F, 3)), np.zeros((n, 3)), np.zeros(n, np.uint8)
        lib.vio_init_sfm(F, sc["l"], p(R), p(t), n, p(sc["start"], _ip), p(sc["fr"], _ip), p(sc["xy"]), p(q), p(Tw), p(pts), p(pok, _u8), C.byref(ok))
        if not ok.value:
            return T.FAIL_BA
        for g, idx, xy in pr["ex"]:
            R0 = np.ascontiguousarray(T._q_to_R(*q[g]).T)
            t0 = -(R0 @ Tw[g])
            p3 = np.ascontiguousarray(pts[idx])
            lib.vio_init_pnp(p(p3), p(xy), len(idx), p(R0), p(t0), C.byref(ok))
            if len(idx) < 6 or not ok.value:
                return T.FAIL_PNP
        return T.OK

    scenes = [prepare(sc) for sc in scenes]
    width = host_width()
    print("estimator start-up (relative pose fit, construct with its bundle adjustment, PnP of 9 extra frames): device "
          "(vio_init_sfm_solve) against host (vio_init_relative_pose + vio_init_sfm + vio_init_pnp on %d threads)" % width)
    print("problems: scenes %s of tests/test_init_sfm_device.py::_scene, 11 frames, round-robin; host route status per scene %s"
          % (SEEDS, [host_route(sc) for sc in scenes]))
    solver = init_sfm.SfmSolver(512, 11, 256, 4096, 9)
    warm = [T._problem(scenes[0]["sc"], hint=scenes[0]["hint"])]
    solver.solve(warm)                            # first call: module load, buffers
    solver.kernel_ms()
    print("%-10s %10s %10s %10s %10s %12s %14s" % ("problems", "head ms", "BA ms", "tail ms", "kernels", "device call", "host pool ms"))
    with ThreadPoolExecutor(width) as pool:
        list(pool.map(host_route, scenes))
        for n in (1, 64, 512):
            todo = [scenes[i % len(scenes)] for i in range(n)]
            stage, call, host = [], [], []
            for _ in range(args.repeat):
                ps = [T._problem(pr["sc"], hint=pr["hint"]) for pr in todo]
                t0 = time.perf_counter()
                solver.solve(ps)
                call.append(1e3 * (time.perf_counter() - t0))
                stage.append(solver.kernel_ms()[0])
                t0 = time.perf_counter()
                st = list(pool.map(host_route, todo))
                host.append(1e3 * (time.perf_counter() - t0))
                assert [p.status for p in ps] == st
            m = np.median(np.array(stage), axis=0)
            print("%-10d %10.3f %10.3f %10.3f %10.3f %12.3f %14.3f   (median of %d; min call %.3f, min host %.3f)"
                  % (n, m[0], m[1], m[2], m.sum(), np.median(call), np.median(host), args.repeat, min(call), min(host)))
    solver.close()
    print("(host: per problem 11 library calls from a Python thread pool, their inputs prepared beforehand; device call: packing of the"
          " problems on one host thread (ctypes structs included), upload, three kernels, download)")


if __name__ == "__main__":
    main()
