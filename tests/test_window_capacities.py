"""Windows in a layout carved for larger ones, on the SIMT emulator against the CPU oracle.

vio_backend_upload sizes a batch for its largest window, so a window's W, landmark, factor and prior counts are usually below the
capacities its kernel runs with. tests/emul/simt_backend.cpp's simt_solve_window_caps takes those capacities from outside
(simt_solve_window always made them the window's own, which left this whole class unreachable on the CPU).

Group 1: W < Wcap in every emulator variant, lane order and window shape (tests/capacity_cases.py), and with room for a relocalization
pose the window does not carry. Group 2: Wcap == W with the landmark / factor / LDS / prior capacities raised as the launcher raises
them. The expectation is the oracle solving the window alone under default_config(window_size=W); bars: marg_pass_windows' (1e-6
states, 1e-5 prior H and b; block lists, iteration counts, terminations and flags equal)."""
import ctypes as C

import pytest

import helpers as H
from helpers import abi
import capacity_cases as CC
import marg_pass_windows as MW


@pytest.fixture(scope="module")
def simt():
    lib = H.build_emul_lib("simt_backend.cpp", "libvio_simt.so", "VIO_SIMT")
    lib.simt_solve_window_caps.argtypes = [C.POINTER(abi.VioConfig), C.POINTER(abi.VioWindow), C.POINTER(abi.VioSolveStats),
                                           C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return lib


def solve_caps(simt, cfg, w, nthreads, variant, order, caps, want=abi.VIO_OK):
    arr = (C.c_int * 6)(*caps)
    if want != abi.VIO_OK:
        st = abi.VioSolveStats()
        return simt.simt_solve_window_caps(C.byref(cfg), C.byref(w.copy().struct()), C.byref(st), nthreads, variant, order, arr)
    return H.solve_with(lambda c, x, s: simt.simt_solve_window_caps(c, x, s, nthreads, variant, order, arr), cfg, w)


def _smaller_than_capacity():
    """(W, Wcap, work-items, shape, variant, lane order, loop_cap): the launcher's pick (-1) in all three lane orders, the lean LDS
    layout (2) in one that rotates, for every size pair and shape; the global matrix at 256 work-items (0) and a layout with room
    for a relocalization pose around windows that have none."""
    out = []
    for i, (W, Wcap, nt0) in enumerate(CC.WCAP_CASES):
        for j, shape in enumerate(CC.SHAPES):
            # (a Wcap = 12 layout with a relocalization pose is past the LDS variant: the launcher's global-matrix workgroup)
            nt = 512 if (Wcap == 12 and shape == "loop") else nt0
            out += [(W, Wcap, nt, shape, -1, order, 0) for order in (0, 1, 2)]
            if nt == 256:
                out.append((W, Wcap, nt, shape, 2, (i + j) % 3, 0))
    out.append((6, 10, 256, "prior", 0, 1, 0))
    out += [(3, 10, 256, "prior", -1, 0, 1), (6, 10, 256, "second_new", -1, 1, 1), (9, 10, 256, "no_prior", 2, 2, 1),
            (14, 20, 512, "prior", -1, 1, 1)]
    return out


@pytest.mark.parametrize("W,Wcap,nthreads,shape,variant,order,loop_cap", _smaller_than_capacity(),
                         ids=lambda v: str(v))
def test_window_smaller_than_capacity(W, Wcap, nthreads, shape, variant, order, loop_cap, simt):
    w, exp = CC.window(W, shape, F=60 if Wcap == 20 else 40)
    cfg = abi.default_config(window_size=Wcap)
    got, gs = solve_caps(simt, cfg, w, nthreads, variant, order, CC.caps(Wcap=Wcap, loop_cap=loop_cap))
    MW.check_against_oracle(got, gs, *exp, report="W%d/cap%d %s v%d o%d" % (W, Wcap, shape, variant, order))


@pytest.mark.parametrize("shares", [2, 4])
@pytest.mark.parametrize("W", [6, 14])
def test_band_product_shares_of_a_smaller_window(W, shares, simt):
    """The band's trailing product dealt out to the workgroups of a cooperative window (band_syrk_share; the emulated workgroup runs
    the shares one after the other, tests/test_simt_backend.py) for a window below the capacity of its global-matrix layout."""
    w, exp = CC.window(W, "prior", F=60)
    simt.simt_set_syrk_shares(shares)
    try:
        got, gs = solve_caps(simt, abi.default_config(window_size=20), w, 512, -1, 0, CC.caps(Wcap=20))
    finally:
        simt.simt_set_syrk_shares(1)
    MW.check_against_oracle(got, gs, *exp, report="W%d/cap20 shares %d" % (W, shares))


def _raised_capacities():
    """(W, work-items, shape, variant, order, Flds, Mcap, Ncap): Wcap == W; Flds 0 = the window's F, Fcap = the launcher's rounding of
    Flds; Mcap 0 = the window's M; Ncap 1 = the launcher's 6 W + 15, else a prior capacity above that."""
    out = []
    k = 0
    for W, nt in ((6, 256), (10, 256), (12, 256), (20, 512)):
        for flds in (0, 97, 150):
            for mcap in (0, 1024):
                shape = CC.SHAPES[k % 4]
                # (a W = 12 pose matrix with a relocalization pose is past the LDS variant: the launcher's global-matrix workgroup)
                n = 512 if (W == 12 and shape == "loop") else nt
                out.append((W, n, shape, 2 if (n == 256 and k % 2) else -1, k % 3, flds, mcap, (1, 200)[k % 2]))
                k += 1
    return out


@pytest.mark.parametrize("W,nthreads,shape,variant,order,flds,mcap,ncap", _raised_capacities(), ids=lambda v: str(v))
def test_capacities_above_the_windows_counts(W, nthreads, shape, variant, order, flds, mcap, ncap, simt):
    w, exp = CC.window(W, shape, F=60 if W == 20 else 40)
    cfg = abi.default_config(window_size=W)
    flds = flds or w.n_features
    assert mcap == 0 or mcap > w.n_factors
    assert w.prior is None or ncap == 1 or ncap > max(w.prior.n, 6 * W + 15)
    caps = CC.caps(Wcap=W, Fcap=CC.launcher_fcap(cfg, flds), Mcap=mcap, Ncap=ncap, Flds=flds)
    got, gs = solve_caps(simt, cfg, w, nthreads, variant, order, caps)
    MW.check_against_oracle(got, gs, *exp, report="W%d %s v%d o%d caps %s" % (W, shape, variant, order, caps))


def test_capacity_below_the_window_is_rejected(simt):
    w, _ = CC.window(6, "prior")
    cfg = abi.default_config(window_size=10)
    for caps in (CC.caps(Wcap=5), CC.caps(Fcap=w.n_features - 1, Flds=w.n_features - 1), CC.caps(Mcap=w.n_factors - 1),
                 CC.caps(Fcap=64, Flds=w.n_features - 1), CC.caps(Fcap=64, Flds=65)):
        assert solve_caps(simt, cfg, w, 256, -1, 0, caps, want=abi.VIO_EINVAL) == abi.VIO_EINVAL, caps
