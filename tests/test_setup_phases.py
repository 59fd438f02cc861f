"""The set-up of a solve (csrc/solver_core.h: state load and slot records at the head of solve_window, build_gram_pieces,
setup_imu_info, setup_prior with H0 scattered from its accumulators) on the SIMT emulator, in all three lane orders, against the
CPU oracle.

The windows (tests/setup_cases.py) put the sizes of that code on their edges: priors of 21 / 33 / 63 / 75 columns (two tiles and
less than one operand batch; one column past a tile edge; one short of a tile edge and two whole batches; the benchmark's), no
prior, the prior of a MARGIN_SECOND_NEW solve; one factor, 255 / 256 / 257 factors, slot counts just below / at / just past 256, the full window and a
window of more than 1024 factors. The emulator's global scratch starts as NaN, so an entry of the reduced matrix that the
set-up leaves unwritten shows. Bars: tests/test_backend_gpu.py's (1e-6 states, 1e-5 prior H and b); block lists, iteration counts,
terminations and flags equal."""
import ctypes as C

import pytest

import helpers as H
from helpers import abi
import marg_pass_windows as MW
import setup_cases as SC


@pytest.fixture(scope="module")
def simt():
    lib = H.build_emul_lib("simt_backend.cpp", "libvio_simt.so", "VIO_SIMT")
    lib.simt_solve_window.argtypes = [C.POINTER(abi.VioConfig), C.POINTER(abi.VioWindow), C.POINTER(abi.VioSolveStats),
                                      C.c_int, C.c_int, C.c_int]
    return lib


@pytest.fixture(scope="module")
def cases():
    cfg = abi.default_config()
    osolve, opre = H.oracle_backend()
    pre = lambda *a: abi.preintegrate_with(opre, cfg, *a)
    ws = SC.build_windows(cfg, pre, osolve)
    ws["many_factors"] = SC.many_factors_window(cfg, pre, osolve)
    return cfg, ws, MW.expectations(cfg, osolve, ws)


NAMES = ["prior_m1", "prior_m3", "prior_m8", "full", "no_prior", "prior_second_new", "one_factor", "factors_255", "factors_256",
         "factors_257", "slots_below", "slots_exact", "slots_above", "many_factors"]


def test_windows_are_what_they_claim(cases):
    """The sizes of every window as the emulator build packs it (the device's layout: buckets aligned to the staging chunk)."""
    cfg, ws, _ = cases
    assert sorted(ws) == sorted(NAMES)
    inf = {n: SC.setup_info(cfg, w) for n, w in ws.items()}
    for m, n in ((1, 21), (3, 33), (8, 63)):
        assert inf["prior_m%d" % m]["prior_n"] == n
    assert inf["full"]["prior_n"] == 75 and inf["no_prior"]["prior_n"] == 0 and inf["prior_second_new"]["prior_n"] > 0
    assert all(i["staged"] and i["lds"] == 1 for i in inf.values())  # (J0 through LDS in every W = 10 layout)
    assert inf["one_factor"]["M"] == 1 and inf["one_factor"]["nslots"] == 2 and inf["one_factor"]["npairs"] == 1
    for c in (255, 256, 257):
        assert inf["factors_%d" % c]["M"] == c
    assert 250 <= inf["slots_below"]["nslots"] < 256 == inf["slots_exact"]["nslots"] < inf["slots_above"]["nslots"]
    before = SC.setup_info(cfg, SC.first_factors(ws["full"], ws["slots_above"].n_factors - 1))
    assert before["nslots"] <= 256  # (the first prefix past the workgroup size)
    assert 3 * 256 < inf["full"]["M"] <= 4 * 256 and inf["many_factors"]["M"] > 4 * 256
    assert ws["prior_second_new"].prior.n_blocks > 0


# (threads, variant, lane order) as tests/test_simt_backend.py: what the launcher picks in two lane orders, the lean LDS layout in the third
MODES = [(256, -1, 0), (256, -1, 1), (256, 2, 2)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_setup_on_simt_emulator(name, mode, simt, cases):
    cfg, ws, exp = cases
    nthreads, variant, order = mode
    got, gs = H.solve_with(lambda c, w, s: simt.simt_solve_window(c, w, s, nthreads, variant, order), cfg, ws[name])
    MW.check_against_oracle(got, gs, *exp[name], report=name)


def test_global_matrix_variant_on_simt_emulator(simt):
    """W = 20, 512 work-items: the staging area is too small for J0, so H0 and b0 read their operands from global memory (the
    unstaged path), and the prior of the uncut window has 135 columns (nine tiles, 34 k-steps). The uncut window runs in all three
    lane orders, the others in one each."""
    cfg = abi.default_config(window_size=20)
    osolve, opre = H.oracle_backend()
    pre = lambda *a: abi.preintegrate_with(opre, cfg, *a)
    ws = SC.build_windows(cfg, pre, osolve, W=20, seed=7, prior_m=(1, 8, 20), sizes=False)
    inf = SC.setup_info(cfg, ws["full"], nthreads=512)
    assert inf["lds"] == 0 and inf["prior_n"] == 135 and not inf["staged"] and inf["M"] > 2 * 512
    assert SC.setup_info(cfg, ws["prior_m1"], nthreads=512)["staged"]  # (a small prior is staged in this instantiation too)
    exp = MW.expectations(cfg, osolve, ws)
    for k, (name, w) in enumerate(sorted(ws.items())):
        for order in ((0, 1, 2) if name == "full" else (k % 3,)):
            got, gs = H.solve_with(lambda c, x, s: simt.simt_solve_window(c, x, s, 512, -1, order), cfg, w)
            MW.check_against_oracle(got, gs, *exp[name], report="w20 %s order %d" % (name, order))
