"""The Cauchy point of the dogleg step is formed on demand (csrc/solver_core.h, minimize, `cauchy_known`): a linearization whose
Gauss-Newton step stays inside the trust region never computes |g_d|^2, the Cauchy direction or its quadratic form; the first
dogleg step that leaves the region linearizes at the iterate once more and forms them, and a run of rejected steps keeps them.

CPU half: the kernel body on the wave64 SIMT emulator (tests/test_simt_backend.py runs every golden through it; the cases here are
the ones that take the new path, and the guards keep them from passing silently should the fixtures change). The large window of
tests/cauchy_cases.py is solved here by one emulated workgroup; the cooperative launch of it exists on the device only
(tests/test_cauchy_on_demand_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from helpers import abi
from cauchy_cases import assert_binds_both_ways, bind_w20_window, tripled


@pytest.fixture(scope="module")
def simt():
    lib = H.build_emul_lib("simt_backend.cpp", "libvio_simt.so", "VIO_SIMT")
    lib.simt_solve_window.argtypes = [C.POINTER(abi.VioConfig), C.POINTER(abi.VioWindow), C.POINTER(abi.VioSolveStats),
                                      C.c_int, C.c_int, C.c_int]
    return lib


def run(simt, nthreads, variant, order):
    return lambda cfg, win, st: simt.simt_solve_window(cfg, win, st, nthreads, variant, order)


def test_fixture_binds_right_after_a_solve():
    """win_c2_hard20: the first step is cut back to the region (radius 10000 -> 30000 = 3 x the dogleg step norm)."""
    d = H.load_golden_window("win_c2_hard20")[2]
    assert d["ref_it_radius"][1] == 3 * d["ref_it_radius"][0]
    assert int(d["ref_it_flags"][1]) == 3


def test_fixture_binds_on_a_reused_step():
    """win_c2_hard8: four rejections halve the radius until the REUSED Gauss-Newton step no longer fits; the last step is accepted on
    the boundary."""
    d = H.load_golden_window("win_c2_hard8")[2]
    fl, r = [int(x) for x in d["ref_it_flags"]], d["ref_it_radius"]
    assert fl[-5:] == [1, 1, 1, 1, 3]
    assert abs(r[-1] - 3 * r[-2]) <= 1e-12 * r[-1]
    assert tripled(r) == [len(r) - 1]  # (and never before: the Cauchy point is first needed after the rejections)


def test_fixture_never_binds():
    """win_chain_b_prior (the window type of the benchmark): constant radius, every step accepted."""
    d = H.load_golden_window("win_chain_b_prior")[2]
    assert (d["ref_it_radius"] == d["ref_it_radius"][0]).all()
    assert all(int(x) == 3 for x in d["ref_it_flags"])


@pytest.mark.parametrize("mode", [(256, -1, 1), (256, 0, 2)])
@pytest.mark.parametrize("name", ["win_c2_hard20", "win_c2_hard8", "win_tiny_w4_f3", "win_chain_b_prior"])
def test_on_demand_cauchy_point_on_simt_emulator(name, mode, simt):
    """The binding goldens and the one that never binds, matrix in LDS and in global scratch, traces included."""
    cfg, w, d = H.load_golden_window(name)
    got, stats = H.solve_with(run(simt, *mode), cfg, w)
    H.check_solution(got, stats, d, tol=1e-6, tol_prior=1e-5)


def test_large_window_binds_on_simt_emulator(simt):
    """BIND_W20 through the emulated workgroup against the CPU oracle, with the guard that the oracle's trace binds both ways."""
    cfg, w, ref, rs = bind_w20_window()
    assert_binds_both_ways(rs)
    n = rs["iterations"] + 1
    got, gs = H.solve_with(run(simt, 256, -1, 1), cfg, w)
    assert gs["iterations"] == rs["iterations"] and list(gs["it_flags"]) == list(rs["it_flags"])
    assert H.relerr(np.asarray(gs["it_radius"])[:n], np.asarray(rs["it_radius"])[:n]) < 1e-6
    assert H.pose_relerr(got.pose, ref.pose) < 1e-6
    assert H.relerr(got.inv_depth, ref.inv_depth) < 1e-6
