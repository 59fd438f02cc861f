"""tools/init_align_timing.py and its C++ driver (tools/init_align_host_route.cpp): the host route of the stage that closes
estimator start-up as the tool times it. What the driver computes per problem has to be the route itself: the alignment's
ok / Bgs / g / x are vio_visual_imu_alignment's on the same frames, and every window interval is vio_preintegrate of that
interval's samples from (0, Bgs[k]) -- bit for bit, on one thread and on several, for every problem of a batch."""
import ctypes as C
import os
import sys

import numpy as np

import helpers as H
import test_initial_cpu as TI
from helpers import abi

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
import init_align_timing as AT  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_driver_runs_the_host_route():
    sets = [TI.make_frames(seed, AT.FRAMES, imu_per_frame=AT.SAMPLES) for seed in AT.SEEDS[:2]]
    cfg, drv = abi.default_config(), AT.driver()
    W = cfg.window_size
    assert AT.W == W and AT.FRAMES == 20 and AT.SAMPLES == 10
    want = []
    for frames, truth in sets:
        r = TI.product(frames, truth["tic"])
        assert r["ok"] == 1 and np.abs(r["Bgs"]).max() > 1e-3   # (a bias the re-integration has to pick up)
        win = AT.window_frames(frames)
        assert len(win) == W + 1 and all(len(f["dt"]) == AT.SAMPLES for f in win) and win[0] is frames[1] and win[W] is frames[W + 1]
        pre = [abi.preintegrate_with(abi.load_product().vio_preintegrate, cfg, f["acc_0"], f["gyr_0"], np.zeros(3), r["Bgs"][k],
                                     f["dt"], f["acc"], f["gyr"]) for k, f in enumerate(win)]
        want.append((r, np.array(pre)))
    for threads in (1, 3):
        b = AT.Batch(sets, 5)
        assert b.run(drv, cfg, threads) > 0
        for i in range(5):
            r, pre = want[i % 2]
            p = b.arr[i]
            assert p.ok == 1 and p.rc == 0
            assert np.array_equal(_bits(b.Bgs[i]), _bits(r["Bgs"])) and np.array_equal(_bits(b.x[i]), _bits(r["x"]))
            assert np.array_equal(_bits(np.array(p.g[:])), _bits(r["g"]))
            assert np.array_equal(_bits(b.pre[i]), _bits(pre))
            assert np.array_equal(b.pre[i][:, 14:17], r["Bgs"])  # linearized_bg of every interval


def test_rows_of_the_table():
    sets = [TI.make_frames(AT.SEEDS[0], AT.FRAMES, imu_per_frame=AT.SAMPLES)]
    rows = AT.measure(sets, counts=(1, 3), repeat=1, width=2)
    assert [r[0] for r in rows] == [1, 3] and all(np.isfinite(r[1:]).all() and r[1] >= r[2] > 0 and r[3] >= r[4] > 0 for r in rows)
    null = C.POINTER(AT.AlignHostProblem)()
    assert AT.driver().init_align_host_route_run(C.byref(abi.default_config()), null, 1, 1) == -1.0
