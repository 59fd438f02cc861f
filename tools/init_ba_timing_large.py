#!/usr/bin/env python3
"""Times the bundle adjustment of estimator start-up beyond 16 frames on both routes, per frame count: vio_init_ba_solve
(the large layout of csrc/sfm_core.h: one workgroup of 512 work-items per problem, one workgroup per compute unit) for
1, 64 and 256 problems per launch -- device time per launch from vio_init_ba_kernel_ms and wall time of the whole call
(packing, upload, kernel, download) -- against vio_init_bundle_adjust for the SAME problems on as many host threads as the
box grants this process. The problems are the recorded cases of tests/golden/init_sfm_large.npz with the chosen frame
count (--frames 21: f21, the shape of WINDOW_SIZE 20; --frames 31: f31, WINDOW_SIZE 30), repeated round-robin. Median of
--repeat runs after a warm-up launch.
    python tools/init_ba_timing_large.py [--frames 21 31] [--repeat 5] > profiles/init_ba_timing_large.txt"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_ba_timing as small  # noqa: E402  (problem_of, host_solve, host_width; it puts the package on the path)

init_ba, abi = small.init_ba, small.abi
BATCHES = (1, 64, 256)


def load_cases(frames):
    d = np.load(os.path.join(small.ROOT, "tests", "golden", "init_sfm_large.npz"))
    out = []
    for nm in sorted({k.split("_in_")[0] for k in d.files if "_in_" in k}):
        if int(d[nm + "_in_F"]) == frames:
            c = {k[len(nm) + 4:]: d[k] for k in d.files if k.startswith(nm + "_in_")}
            out.append((nm, c, int(d[nm + "_out_iterations"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[21, 31])
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    import torch  # noqa: F401  (HIP runtime first)
    lib = abi.load_product()
    width = small.host_width()
    print("bundle adjustment of estimator start-up beyond 16 frames: device (vio_init_ba_solve, large layout) against host "
          "(vio_init_bundle_adjust, %d threads)" % width)
    for frames in args.frames:
        cases = load_cases(frames)
        assert cases, "no recorded case of %d frames" % frames
        for nm, c, it in cases:
            nobs = int(np.diff(c["start"])[c["ok"] != 0].sum())
            print("\n%d frames: case %s of tests/golden/init_sfm_large.npz, %d landmarks, %d observations, %d iterations"
                  % (frames, nm, int(np.count_nonzero(c["ok"])), nobs, it))
        solver = init_ba.BaSolver(max(BATCHES), frames, 300, 4000)
        solver.solve([small.problem_of(cases[0][1])])      # first launch: module load, buffers
        solver.kernel_ms()
        print("%-22s %12s %12s %12s" % ("problems per launch", "kernel ms", "call ms", "host ms"))
        overtakes = None
        with ThreadPoolExecutor(width) as pool:
            list(pool.map(lambda c: small.host_solve(lib, c), [cases[0][1]] * width))
            for n in BATCHES:
                todo = [cases[i % len(cases)][1] for i in range(n)]
                ker, wall, host = [], [], []
                for _ in range(args.repeat):
                    ps = [small.problem_of(c) for c in todo]
                    t0 = time.perf_counter()
                    solver.solve(ps)
                    wall.append(1e3 * (time.perf_counter() - t0))
                    ker.append(solver.kernel_ms()[0])
                    assert all(p.ok == 1 for p in ps)
                    t0 = time.perf_counter()
                    list(pool.map(lambda c: small.host_solve(lib, c), todo))
                    host.append(1e3 * (time.perf_counter() - t0))
                print("%-22d %12.3f %12.3f %12.3f   (median of %d; min %.3f / %.3f / %.3f)"
                      % (n, np.median(ker), np.median(wall), np.median(host), args.repeat, min(ker), min(wall), min(host)))
                if overtakes is None and np.median(wall) < np.median(host):
                    overtakes = n
        solver.close()
        print("%d frames: the device call %s" % (frames, "is faster than the host pool from %d problems per launch" % overtakes
                                                 if overtakes else "does not overtake the host pool at any of these batch sizes"))


if __name__ == "__main__":
    main()
