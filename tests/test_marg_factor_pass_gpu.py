"""The marginalization's factor pass (csrc/marg_core.h) on the device: the windows of tests/test_marg_factor_pass.py
(tests/marg_pass_windows.py) as ragged batches through WindowSolver.solve, against the CPU oracle, in the three instantiations of
the window kernel that run the pass differently: the static W = 10 LDS variant, the run-time-W LDS variant (W = 6 windows and a
window with a relocalization pose in the batch) and the global-matrix variant (W = 20, 512 work-items).
Bars: tests/test_backend_gpu.py's (1e-6 states, 1e-5 prior H and b); block lists, iteration counts and flags equal."""
import pytest

import helpers as H
from helpers import abi, pkg
import marg_pass_windows as MW

pytestmark = pytest.mark.gpu


def solve_and_check(cfg, ws, exp, label, max_batch=16):
    names = sorted(ws)
    solver = pkg.backend.WindowSolver(cfg, max_batch=max_batch)
    try:
        got = [ws[n].copy() for n in names]
        stats = solver.solve(got)
    finally:
        solver.close()
    for n, g, s in zip(names, got, stats):
        MW.check_against_oracle(g, s, *exp[n], report=label + " " + n)


@pytest.fixture(scope="module")
def w10():
    cfg = abi.default_config()
    osolve, _ = H.oracle_backend()
    ws = MW.build_windows(cfg, lambda *a: pkg.backend.preintegrate(cfg, *a), osolve)
    return cfg, ws, MW.expectations(cfg, osolve, ws)


def test_static_w10_lds_variant(w10):
    """Every window has W = 10 and no relocalization pose: the launcher takes the compile-time W = 10 instantiation."""
    cfg, ws, exp = w10
    batch = {n: w for n, w in ws.items() if n != "with_loop"}
    assert all(w.W == 10 and not (w.factor_target == w.W + 1).any() for w in batch.values())
    solve_and_check(cfg, batch, exp, "static")


def test_runtime_w_lds_variant_with_loop(w10):
    """A window with a relocalization pose in the batch: the launcher takes the run-time-W instantiation for all of it (buckets (0, P)
    are not part of the pass)."""
    cfg, ws, exp = w10
    batch = {n: ws[n] for n in ("with_loop", "full", "chunk_plus1", "straddle_odd", "one_factor")}
    solve_and_check(cfg, batch, exp, "runtime")


def test_runtime_w_lds_variant_w6():
    """W = 6 in a configuration of its own (batches that mix window sizes: tests/test_window_capacities_gpu.py): window size, strides
    and the staging chunk are run-time values."""
    cfg = abi.default_config(window_size=6)
    osolve, _ = H.oracle_backend()
    w6 = MW.build_windows(cfg, lambda *a: pkg.backend.preintegrate(cfg, *a), osolve, W=6, seed=43, full=False)
    assert MW.marg_info(cfg, w6["full"])["lds"] == 1
    solve_and_check(cfg, w6, MW.expectations(cfg, osolve, w6), "w6")


def test_global_matrix_variant():
    """A W = 20 window and its edits: the dense matrix in global scratch, the wide factor pass run by the owner workgroup alone; the
    unedited window has more slots hosted at frame 0 than work-items and more than one staging chunk."""
    cfg = abi.default_config(window_size=20)
    osolve, _ = H.oracle_backend()
    ws = MW.build_windows(cfg, lambda *a: pkg.backend.preintegrate(cfg, *a), osolve, W=20, n_features=150, seed=7, full=False)
    inf = MW.marg_info(cfg, ws["full"], nthreads=512)
    assert inf["lds"] == 0 and inf["S0"] > 512 and inf["S0"] > inf["CH"]
    solve_and_check(cfg, ws, MW.expectations(cfg, osolve, ws), "w20")
