#!/usr/bin/env python3
"""Times what closes estimator start-up on the host route, the stage nobody had measured: per problem one
vio_visual_imu_alignment (solveGyroscopeBias with the re-integration of every image interval, SolveScale, the four passes of
RefineGravity) plus the re-integration of the window's W + 1 intervals from the corrected biases (vio_preintegrate, what
solve_initial_align's loop runs), for 1, 64 and 512 problems: on ONE thread, and dealt one problem at a time to as many host
threads as the box grants this process. The timed part is C++ (tools/init_align_host_route.cpp, built on first use against
csrc/libvio_amd.so): no interpreter, no allocation, every pointer and output buffer made beforehand. The problems are eight
seeded frame sets of tests/test_initial_cpu.py::make_frames -- 20 frames, 10 IMU samples per interval; the 11 window
intervals are the sets' own frame intervals 1 .. 11 integrated again (a window's pre_integrations hold the same kind of
samples), round-robin. Warm-up first, medians of --repeat runs. Host only: the stage has no device form.
    python tools/init_align_timing.py [--repeat 5] > profiles/init_align_timing.txt"""
import argparse
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("vins-mobile_amd")
abi = pkg.abi
from init_sfm_timing import host_width  # noqa: E402  (the threads the box grants: one definition for the start-up tools)

SEEDS = [7, 8, 9, 10, 11, 12, 13, 14]
FRAMES, SAMPLES, W = 20, 10, 10
_dp = C.POINTER(C.c_double)


class AlignHostProblem(C.Structure):  # tools/init_align_host_route.cpp
    _fields_ = [("tic", C.c_double * 3), ("frames", C.POINTER(abi.VioInitFrame)), ("n_frames", C.c_int32), ("window_size", C.c_int32),
                ("window", C.POINTER(abi.VioInitFrame)), ("Bgs", _dp), ("x", _dp), ("pre", C.POINTER(abi.VioPreintegration)),
                ("g", C.c_double * 3), ("ok", C.c_int32), ("rc", C.c_int32)]


def driver():
    """tools/libinit_align_host_route.so, built with g++ when missing or older than its source."""
    src, so = os.path.join(ROOT, "tools", "init_align_host_route.cpp"), os.path.join(ROOT, "tools", "libinit_align_host_route.so")
    csrc = os.path.join(ROOT, "vins-mobile_amd", "csrc")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I" + os.path.join(ROOT, "include"), "-o", so, src,
                               "-L" + csrc, "-lvio_amd", "-Wl,-rpath," + csrc])
    abi.load_product()
    d = C.CDLL(so)
    d.init_align_host_route_run.restype = C.c_double
    d.init_align_host_route_run.argtypes = [C.POINTER(abi.VioConfig), C.POINTER(AlignHostProblem), C.c_int32, C.c_int32]
    return d


def window_frames(frames):
    """The window's W + 1 intervals of a frame set: its frame intervals 1 .. W + 1."""
    return [frames[1 + k] for k in range(W + 1)]


class Batch:
    """n problems, round-robin over the frame sets, each with output buffers of its own; everything the timed call reads or
    writes exists before it."""

    def __init__(self, sets, n):
        import test_initial_cpu as TI
        self.keep, self.n = [], n
        cs = []
        for frames, truth in sets:
            arr, k1 = TI.to_c(frames)
            win, k2 = TI.to_c(window_frames(frames))
            self.keep += [arr, k1, win, k2]
            cs.append((arr, win, truth["tic"], len(frames)))
        self.arr = (AlignHostProblem * n)()
        self.Bgs, self.x = np.zeros((n, W + 1, 3)), np.zeros((n, 3 * FRAMES + 1))
        self.pre = np.zeros((n, W + 1, abi.PREINT_DOUBLES))
        for i, p in enumerate(self.arr):
            arr, win, tic, nf = cs[i % len(cs)]
            p.tic[:] = list(tic)
            p.frames, p.n_frames, p.window_size, p.window = arr, nf, W, win
            p.Bgs, p.x = self.Bgs[i].ctypes.data_as(_dp), self.x[i].ctypes.data_as(_dp)
            p.pre = C.cast(self.pre[i].ctypes.data, C.POINTER(abi.VioPreintegration))

    def run(self, drv, cfg, threads):
        ms = drv.init_align_host_route_run(C.byref(cfg), self.arr, self.n, threads)
        assert ms >= 0 and all(p.ok == 1 for p in self.arr), "a library call failed or a frame set did not align"
        return ms


def frame_sets():
    import test_initial_cpu as TI
    return [TI.make_frames(seed, FRAMES, imu_per_frame=SAMPLES) for seed in SEEDS]


def measure(sets, counts=(1, 64, 512), repeat=5, width=None):
    """-> [(count, one-thread median ms, one-thread min, pool median ms, pool min)]"""
    width = width or host_width()
    drv, cfg = driver(), abi.default_config()
    Batch(sets, len(sets)).run(drv, cfg, width)  # warm-up: code and data of every set, the threads' first start
    rows = []
    for n in counts:
        b = Batch(sets, n)
        b.run(drv, cfg, 1), b.run(drv, cfg, width)
        one = [b.run(drv, cfg, 1) for _ in range(repeat)]
        pool = [b.run(drv, cfg, width) for _ in range(repeat)]
        rows.append((n, float(np.median(one)), min(one), float(np.median(pool)), min(pool)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    width = host_width()
    print("estimator start-up, the closing stage on the host route: vio_visual_imu_alignment + re-integration of the window's %d "
          "intervals (vio_preintegrate), C++ driver, one thread and %d threads" % (W + 1, width))
    print("problems: frame sets %s of tests/test_initial_cpu.py::make_frames, %d frames of %d samples; window intervals = the sets' frame "
          "intervals 1 .. %d integrated again; round-robin" % (SEEDS, FRAMES, SAMPLES, W + 1))
    print("%-10s %14s %16s %14s %10s" % ("problems", "one thread ms", "per problem ms", "pool ms", "speed-up"))
    for n, one, one_lo, pool, pool_lo in measure(frame_sets(), repeat=args.repeat, width=width):
        print("%-10d %14.3f %16.4f %14.3f %10.1f   (median of %d; min one thread %.3f, min pool %.3f)"
              % (n, one, one / n, pool, one / pool, args.repeat, one_lo, pool_lo))
    print("(the timed call deals the problems one at a time to min(threads, problems) std::threads, their start and join included; "
          "inputs, pointers and output buffers are made beforehand)")


if __name__ == "__main__":
    main()
