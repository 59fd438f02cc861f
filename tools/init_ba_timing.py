#!/usr/bin/env python3
"""Times the bundle adjustment of estimator start-up on both routes: vio_init_ba_solve (one launch, one workgroup per
problem) for batches of 1, 64 and 512 recorded problems -- device time per launch from vio_init_ba_kernel_ms and wall time
of the whole call (packing, upload, kernel, download) -- and vio_init_bundle_adjust for the same 512 problems on as many
host threads as the box grants this process. The problems are the four recorded cases of tests/golden/init_sfm.npz
(11 frames, 90 landmarks, about 880 observations; 10, 13, 19 and 51 iterations), repeated round-robin.
    python tools/init_ba_timing.py [--repeat 5] > profiles/init_ba_timing.txt"""
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
pkg = importlib.import_module("vins-mobile_amd")
abi, init_ba = pkg.abi, pkg.init_ba
_dp, _ip, _u8 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
SEEDS = [43, 21, 25, 22]


def load_cases():
    d = np.load(os.path.join(ROOT, "tests", "golden", "init_sfm.npz"))
    out = []
    for seed in SEEDS:
        pre = "c%d_in_" % seed
        c = {k[len(pre):]: d[k] for k in d.files if k.startswith(pre)}
        out.append((c, int(d["c%d_out_iterations" % seed])))
    return out


def problem_of(c):
    return init_ba.BaProblem(int(c["F"]), int(c["l"]), c["cq"], c["ct"], c["pts"], c["ok"], c["start"], c["fr"], c["xy"])


def host_width():
    for k in ("VIO_AMD_HOST_THREADS", "OMP_NUM_THREADS"):
        if os.environ.get(k, "").isdigit() and int(os.environ[k]) > 0:
            return int(os.environ[k])
    return len(os.sched_getaffinity(0))


def host_solve(lib, c):
    cq, ct, pts = c["cq"].copy(), c["ct"].copy(), c["pts"].copy()
    ok = C.c_int32()
    p = lambda a, t: a.ctypes.data_as(t)
    rc = lib.vio_init_bundle_adjust(int(c["F"]), int(c["l"]), p(cq, _dp), p(ct, _dp), len(pts), p(pts, _dp), p(c["ok"], _u8),
                                    p(c["start"], _ip), p(c["fr"], _ip), p(c["xy"], _dp), None, C.byref(ok))
    assert rc == 0 and ok.value == 1
    return cq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    import torch  # noqa: F401  (HIP runtime first)
    lib = abi.load_product()
    cases = load_cases()
    print("bundle adjustment of estimator start-up: device (vio_init_ba_solve) against host (vio_init_bundle_adjust)")
    print("problems: recorded cases %s of tests/golden/init_sfm.npz, iterations %s, round-robin" % (SEEDS, [c[1] for c in cases]))
    solver = init_ba.BaSolver(512, 11, 128, 1024)
    solver.solve([problem_of(cases[0][0])])      # first launch: module load, buffers
    solver.kernel_ms()
    print("%-28s %12s %12s" % ("device, problems per launch", "kernel ms", "call ms"))
    for n in (1, 64, 512):
        ker, wall = [], []
        for _ in range(args.repeat):
            ps = [problem_of(cases[i % len(cases)][0]) for i in range(n)]
            t0 = time.perf_counter()
            solver.solve(ps)
            wall.append(1e3 * (time.perf_counter() - t0))
            ker.append(solver.kernel_ms()[0])
            assert all(p.ok == 1 for p in ps)
        print("%-28d %12.3f %12.3f   (median of %d; min %.3f / %.3f)" % (n, np.median(ker), np.median(wall), args.repeat, min(ker), min(wall)))
    solver.close()
    width = host_width()
    todo = [cases[i % len(cases)][0] for i in range(512)]
    wall = []
    with ThreadPoolExecutor(width) as pool:
        list(pool.map(lambda c: host_solve(lib, c), todo[:width]))
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            list(pool.map(lambda c: host_solve(lib, c), todo))
            wall.append(1e3 * (time.perf_counter() - t0))
    print("%-28s %12s %12.3f   (median of %d; min %.3f)" % ("host, 512 on %d threads" % width, "-", np.median(wall), args.repeat, min(wall)))
    t0 = time.perf_counter()
    for c, _ in cases:
        host_solve(lib, c)
    print("%-28s %12s %12.3f" % ("host, the 4 cases, 1 thread", "-", 1e3 * (time.perf_counter() - t0)))


if __name__ == "__main__":
    main()
