"""GPU half of tests/test_cauchy_on_demand.py: the window kernel forms the Cauchy point of a linearization only when a dogleg step
leaves the trust region (csrc/solver_core.h, minimize, `cauchy_known`). Windows that take the on-demand path next to windows that
never do in one launch, the stage clock of both kinds, and the path on a cooperative large window."""
import numpy as np
import pytest

import helpers as H
from helpers import pkg
from cauchy_cases import assert_binds_both_ways, bind_w20_window

pytestmark = pytest.mark.gpu

CAUCHY_STAGES = ("v_gd", "quad_form", "q_w")


def profiled_solve(solver, w):
    solver.set_profile(True)
    got = w.copy()
    stats = solver.solve([got])[0]
    cyc = solver.stage_cycles(0)
    solver.set_profile(False)
    return got, stats, cyc


def test_mixed_batch_of_binding_and_free_windows():
    """Eight windows in one launch, neighbours on a CU on different paths: two that never bind, one that binds right after a solve,
    one that binds on a reused step after four rejections, each twice; every copy against the reference's golden output and trace."""
    names = ["win_chain_b_prior", "win_c2_easy", "win_c2_hard8", "win_c2_hard20"] * 2
    loaded = [H.load_golden_window(n) for n in names]
    solver = pkg.backend.WindowSolver(loaded[0][0], max_batch=8)
    ws = [w.copy() for _, w, _ in loaded]
    stats = solver.solve(ws)
    solver.close()
    for (_, _, d), w, s in zip(loaded, ws, stats):
        H.check_solution(w, s, d, tol=1e-6, tol_prior=1e-5)


def test_stage_clock_reads_zero_unless_the_region_binds():
    """v_gd / quad_form / q_w are the clock of the on-demand path alone: 0 for the benchmark's window type, > 0 where the first step
    is cut back to the region."""
    cfg, w, d = H.load_golden_window("win_chain_b_prior")
    solver = pkg.backend.WindowSolver(cfg, max_batch=4)
    got, stats, free = profiled_solve(solver, w)
    H.check_solution(got, stats, d, tol=1e-6, tol_prior=1e-5)
    cfg2, w2, d2 = H.load_golden_window("win_c2_hard20")
    got2, stats2, bound = profiled_solve(solver, w2)
    solver.close()
    H.check_solution(got2, stats2, d2, tol=1e-6, tol_prior=1e-5)
    print("stage cycles, never binds:", {k: free[k] for k in CAUCHY_STAGES + ("total",)})
    print("stage cycles, binds:      ", {k: bound[k] for k in CAUCHY_STAGES + ("total",)})
    assert free["total"] > 0
    for k in CAUCHY_STAGES:
        assert free[k] == 0, (k, free[k])
    assert bound["quad_form"] > 0 and bound["v_gd"] > 0


def test_cooperative_large_window_binds(monkeypatch):
    """One W = 20 window whose trust region binds right after a solve (iteration 1) and on a reused step (iteration 9), solved by 1, 2
    and 4 workgroups, against the CPU oracle: iterations, flags, poses and depths. The window is BIND_W20 of tests/cauchy_cases.py
    (synth.make_window seed 12, 40 landmarks, perturb_scale 20; that file says how the seed was found). At widths 2 and 4 the
    on-demand path posts COOP_EVAL to the helpers from inside the dogleg step, the owner's quadratic form reads the coupling the
    helpers' sums went into, and the Schur command carries no Cauchy vector any more. The launcher is asked what width each launch
    really had (a forced width is dropped when the batch does not fit the chip, and the stage clock turns cooperation off), so the
    stage clock's quad_form > 0 comes from a solve of its own, which runs at width 1."""
    cfg, w, ref, rs = bind_w20_window()
    assert_binds_both_ways(rs)
    first = None
    for width in (1, 2, 4):
        monkeypatch.setenv("VIO_AMD_COOP", str(width))
        solver = pkg.backend.WindowSolver(cfg, max_batch=4)
        got = w.copy()
        gs = solver.solve([got])[0]
        assert solver.coop_width() == width
        solver.close()
        assert np.isfinite(got.pose).all() and np.isfinite(got.inv_depth).all()
        assert gs["iterations"] == rs["iterations"] and list(gs["it_flags"]) == list(rs["it_flags"]), width
        assert H.pose_relerr(got.pose, ref.pose) < 1e-6, width
        assert H.relerr(got.inv_depth, ref.inv_depth) < 1e-6, width
        if first is None:
            first = np.asarray(got.pose).copy()
        else:  # the widths differ in summation order only
            assert H.pose_relerr(got.pose, first) < 1e-8, width
    solver = pkg.backend.WindowSolver(cfg, max_batch=4)
    got, gs, cyc = profiled_solve(solver, w)
    assert solver.coop_width() == 1
    solver.close()
    assert gs["iterations"] == rs["iterations"] and list(gs["it_flags"]) == list(rs["it_flags"])
    assert cyc["quad_form"] > 0 and cyc["v_gd"] > 0
