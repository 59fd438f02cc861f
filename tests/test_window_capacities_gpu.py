"""Windows smaller than the batch they are solved in, on the device: ragged batches through WindowSolver.solve against the CPU
oracle solving every window alone under default_config(window_size=W). vio_backend_upload sizes Wcap, Pcap, nblk_cap, the strides
and the LDS layout for the largest window of the batch; the windows are tests/capacity_cases.py's (the emulator runs the same ones
with the capacities handed in: tests/test_window_capacities.py). Covered: the run-time-W LDS instantiation at window_size 10 and 12,
the dims kept and rebuilt between uploads, the global-matrix instantiation alone and as a cooperative window, the resident prior
slots, and all of it once more with poisoned LDS and scratch.
Bars: marg_pass_windows.check_against_oracle's (1e-6 states, 1e-5 prior H and b; block lists, iterations, terminations, flags equal)."""
import os

import numpy as np
import pytest

import helpers as H
from helpers import abi, pkg, synth
import capacity_cases as CC
import marg_pass_windows as MW

pytestmark = pytest.mark.gpu

# one relocalization pose, one MARGIN_SECOND_NEW, one window without a prior
MIXED = [(3, "prior"), (6, "loop"), (9, "second_new"), (10, "no_prior"), (10, "prior")]
BELOW = [(3, "prior"), (6, "loop"), (9, "second_new"), (9, "prior"), (6, "prior")]  # as many windows, the largest W = 9


def solve_batch(solver, keys, label, F=40):
    """The windows `keys` = [(W, shape)] as one batch; every window against its oracle expectation. Returns the solved windows."""
    pairs = [CC.window(W, shape, F) for W, shape in keys]
    got = [w.copy() for w, _ in pairs]
    stats = solver.solve(got)
    for (W, shape), g, s, (_, exp) in zip(keys, got, stats, pairs):
        MW.check_against_oracle(g, s, *exp, report="%s W%d %s" % (label, W, shape))
    return got


def test_recorded_w6_window_in_a_w10_batch():
    """The batch DESIGN section 0 (round 10) recorded as solved wrongly: the W = 6 window `bucket_even` of marg_pass_windows
    (seed 43) beside W = 10 windows under default_config(). The W = 10 windows are capacity_cases' (relocalization pose, prior, no
    prior) instead of the three edited ones the record names: those take a search over edits to build, and what made the W = 6
    window go wrong is the batch's window capacity, not which larger windows set it."""
    cfg = abi.default_config()
    osolve, opre = CC.oracle()
    w6 = MW.build_windows(cfg, lambda *a: abi.preintegrate_with(opre, cfg, *a), osolve, W=6, seed=43, full=False)["bucket_even"]
    exp6 = MW.expectations(abi.default_config(window_size=6), osolve, {"w": w6})["w"]
    tens = [CC.window(10, shape) for shape in ("loop", "prior", "no_prior")]
    solver = pkg.backend.WindowSolver(cfg, max_batch=8)
    try:
        got = [w6.copy()] + [w.copy() for w, _ in tens]
        stats = solver.solve(got)
    finally:
        solver.close()
    MW.check_against_oracle(got[0], stats[0], *exp6, report="recorded w6")
    for g, s, (_, exp) in zip(got[1:], stats[1:], tens):
        MW.check_against_oracle(g, s, *exp, report="recorded w10")


def test_mixed_sizes_runtime_w_lds_variant_and_sticky_dims():
    """W = 3, 6, 9, 10, 10 in one batch under default_config() (a relocalization pose among them: the run-time-W LDS
    instantiation). Solved twice by one solver: the recorded defect differed from run to run. Then a batch of as many windows whose
    largest W is 9 (the upload rebuilds the dims: Wmax != Wcap), and the mixed batch again (rebuilt once more)."""
    solver = pkg.backend.WindowSolver(abi.default_config(), max_batch=8)
    try:
        a = solve_batch(solver, MIXED, "mixed")
        b = solve_batch(solver, MIXED, "mixed again")
        for x, y in zip(a, b):
            assert np.abs(x.pose - y.pose).max() < 1e-9 and np.abs(x.speed_bias - y.speed_bias).max() < 1e-9
            assert np.abs(x.inv_depth - y.inv_depth).max() < 1e-9
        solve_batch(solver, BELOW, "largest W 9")
        solve_batch(solver, MIXED, "mixed after W 9")
    finally:
        solver.close()


def test_largest_lds_window_size():
    """window_size 12, the largest pose matrix of the LDS instantiations, with W = 9, 11, 12."""
    cfg = abi.default_config(window_size=12)
    keys = [(9, "prior"), (11, "second_new"), (12, "prior"), (11, "no_prior")]
    # the batch's layout is the W = 12 window's own when no window has more landmarks: the launcher's rule, on the emulator build
    w12 = CC.window(12, "prior")[0]
    assert all(CC.window(*k)[0].n_features <= w12.n_features for k in keys)
    assert MW.marg_info(cfg, w12)["lds"] == 1
    solver = pkg.backend.WindowSolver(cfg, max_batch=8)
    try:
        solve_batch(solver, keys, "cap 12")
    finally:
        solver.close()


@pytest.mark.parametrize("forced", [None, "1"])
def test_global_matrix_variant(forced, monkeypatch):
    """window_size 20 with W = 6, 14, 20 at 60 landmarks: the matrix in global scratch, 512 work-items; at the cooperative width the
    launcher picks for three windows and with one workgroup per window."""
    cfg = abi.default_config(window_size=20)
    if forced is None:
        monkeypatch.delenv("VIO_AMD_COOP", raising=False)
    else:
        monkeypatch.setenv("VIO_AMD_COOP", forced)
    assert MW.marg_info(cfg, CC.window(20, "prior", 60)[0], nthreads=512)["lds"] == 0
    solver = pkg.backend.WindowSolver(cfg, max_batch=8)
    try:
        solve_batch(solver, [(6, "prior"), (14, "loop"), (20, "prior"), (14, "no_prior")], "cap 20 coop %s" % forced, F=60)
        print("coop_width", solver.coop_width())
        if forced == "1":
            assert solver.coop_width() == 1
    finally:
        solver.close()


def test_resident_prior_slots_with_mixed_sizes():
    """A W = 6 and a W = 10 sequence chained over two solves through reserved prior slots of a window_size 10 solver, beside the
    same chains with the priors carried through the host (tests/test_backend_gpu.py: test_prior_chain_resident_in_device_memory).
    The host-carried windows are held to the oracle, which is given the prior the device left; the resident ones to the
    host-carried ones at that test's bar (another workgroup: the sums differ in rounding)."""
    cfg = abi.default_config()
    osolve, opre = CC.oracle()
    solver = pkg.backend.WindowSolver(cfg, max_batch=4)
    try:
        solver.reserve_priors(2)
        prior_h, prior_r = {6: None, 10: None}, {6: None, 10: None}
        for k in range(2):
            batch, exp = [], []
            for slot, W in enumerate((6, 10)):
                cw = abi.default_config(window_size=W)
                w = synth.make_window(cw, lambda *a: abi.preintegrate_with(opre, cw, *a), seed=800 + 10 * W + k, traj_seed=60 + W,
                                      frame_offset=k, n_features=40, W=W)
                wh, wr = w.copy(), w.copy()
                wh.prior, wr.prior = prior_h[W], prior_r[W]
                wr.resident_prior = slot + 1
                exp.append(MW.expectations(cw, osolve, {"w": wh})["w"])
                batch += [wh, wr]
            stats = solver.solve(batch)
            for i, W in enumerate((6, 10)):
                wh, wr, sh, sr = batch[2 * i], batch[2 * i + 1], stats[2 * i], stats[2 * i + 1]
                MW.check_against_oracle(wh, sh, *exp[i], report="chain step %d W%d" % (k, W))
                assert sh["iterations"] == sr["iterations"] and list(sh["it_flags"]) == list(sr["it_flags"])
                assert np.abs(wh.pose - wr.pose).max() < 1e-7 and np.abs(wh.inv_depth - wr.inv_depth).max() < 1e-7
                nh, nr = wh.next_prior.c, wr.next_prior.c
                assert nh.n == nr.n and nh.n > 0 and nh.n_blocks == nr.n_blocks
                assert list(nh.block_index[: nh.n_blocks]) == list(nr.block_index[: nr.n_blocks])
                assert not wr.next_prior.J.any()  # the data stayed on the device
                prior_h[W], prior_r[W] = wh.next_prior.copy(), wr.next_prior.header_only()
    finally:
        solver.close()


def test_poisoned_device_buffers():
    """This file once more in a process of its own with VIO_AMD_POISON=1 (LDS of every CU, scratch and outputs filled with NaN
    patterns before each launch): a band block that no pass wrote turns the solve into NaNs instead of passing by luck."""
    import subprocess, sys
    env = dict(os.environ, VIO_AMD_POISON="1")
    env.pop("VIO_AMD_COOP", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "not poisoned",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
