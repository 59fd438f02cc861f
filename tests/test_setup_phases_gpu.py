"""The set-up of a solve (csrc/solver_core.h: the head of solve_window, build_gram_pieces, setup_imu_info, setup_prior) on the
device: the windows of tests/test_setup_phases.py (tests/setup_cases.py) as ragged batches through WindowSolver.solve, against
the CPU oracle, in the instantiations of the window kernel that run the set-up differently: the static W = 10 LDS variants
(fat and lean layout), the run-time-W LDS variant (a W = 6 configuration in a batch of its own) and the global-matrix variant
(W = 20, 512 work-items, J0 read from global memory).
Bars: tests/test_backend_gpu.py's (1e-6 states, 1e-5 prior H and b); block lists, iteration counts, terminations and flags equal."""
import pytest

import helpers as H
from helpers import abi, pkg
import marg_pass_windows as MW
import setup_cases as SC

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


def test_static_w10_lds_variant():
    """Every window has W = 10 and no relocalization pose: the launcher takes the compile-time W = 10 instantiation. Priors of 21,
    33, 63 and 75 columns, none, a MARGIN_SECOND_NEW one; one factor, factor and slot counts around the workgroup size."""
    cfg = abi.default_config()
    osolve, _ = H.oracle_backend()
    ws = SC.build_windows(cfg, lambda *a: pkg.backend.preintegrate(cfg, *a), osolve)
    assert all(w.W == 10 and not (w.factor_target == w.W + 1).any() for w in ws.values())
    assert [ws["prior_m%d" % m].prior.n for m in (1, 3, 8)] + [ws["full"].prior.n] == [21, 33, 63, 75]
    solve_and_check(cfg, ws, MW.expectations(cfg, osolve, ws), "static")


def test_static_w10_lean_variant_many_factors():
    """More than 1024 factors (200 landmarks: the lean LDS layout): the slot-record fill takes a second batch of trips."""
    cfg = abi.default_config()
    osolve, _ = H.oracle_backend()
    ws = {"many_factors": SC.many_factors_window(cfg, lambda *a: pkg.backend.preintegrate(cfg, *a), osolve)}
    solve_and_check(cfg, ws, MW.expectations(cfg, osolve, ws), "lean")


def test_runtime_w_lds_variant_w6():
    """W = 6 (a configuration of its own, as every batch of the suite has one window size): priors of 21, 33 and 51 columns."""
    cfg = abi.default_config(window_size=6)
    osolve, _ = H.oracle_backend()
    ws = SC.build_windows(cfg, lambda *a: pkg.backend.preintegrate(cfg, *a), osolve, W=6, seed=43, prior_m=(1, 3, 6), sizes=False)
    assert SC.setup_info(cfg, ws["full"])["lds"] == 1 and ws["full"].prior.n == 51
    solve_and_check(cfg, ws, MW.expectations(cfg, osolve, ws), "w6")


def test_global_matrix_variant():
    """W = 20: the dense matrix in global scratch, 512 work-items; the uncut window's prior has 135 columns and its J0 does not fit
    the staging area (H0 and b0 from global memory), the prior of the m = 1 cut does (21 columns)."""
    cfg = abi.default_config(window_size=20)
    osolve, _ = H.oracle_backend()
    ws = SC.build_windows(cfg, lambda *a: pkg.backend.preintegrate(cfg, *a), osolve, W=20, seed=7, prior_m=(1, 8, 20), sizes=False)
    inf = SC.setup_info(cfg, ws["full"], nthreads=512)
    assert inf["lds"] == 0 and inf["prior_n"] == 135 and not inf["staged"] and inf["M"] > 2 * 512
    assert SC.setup_info(cfg, ws["prior_m1"], nthreads=512)["staged"]
    solve_and_check(cfg, ws, MW.expectations(cfg, osolve, ws), "w20")
