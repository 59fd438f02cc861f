"""The marginalization's factor pass (csrc/marg_core.h, MARGIN_OLD: projection factors hosted at frame 0 -> staging chunks -> one Gram
tile per (0, t) bucket -> dense matrix) on the SIMT emulator, in all three lane orders, against the CPU oracle.

The windows (tests/marg_pass_windows.py) are the smallest at which the slot ranges of the pass can go wrong: no / one factor
hosted at frame 0, a single odd / even bucket, a bucket longer than a Gram piece, the last slot at / one short of / one past the
staging chunk, a bucket that continues behind a chunk boundary with an odd tail, a relocalization pose, no prior, MARGIN_SECOND_NEW.
The chunk size is read from the emulator build. Bars: tests/test_backend_gpu.py's (1e-6 states, 1e-5 prior H and b); block lists,
iteration counts and flags equal."""
import ctypes as C

import pytest

import helpers as H
from helpers import abi
import marg_pass_windows as MW


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
    ws = MW.build_windows(cfg, lambda *a: abi.preintegrate_with(opre, cfg, *a), osolve)
    return cfg, ws, MW.expectations(cfg, osolve, ws)


NAMES = ["full", "s0_zero", "one_factor", "bucket_odd", "bucket_even", "bucket_long", "chunk_minus1", "chunk_exact", "chunk_plus1",
         "straddle_odd", "with_loop", "no_prior", "second_new"]


def test_windows_are_what_they_claim(cases):
    """The layout of every edited window, as the emulator build packs it (order 1: buckets where the slot order puts them)."""
    cfg, ws, _ = cases
    assert sorted(ws) == sorted(NAMES)
    inf = {n: MW.marg_info(cfg, w) for n, w in ws.items()}
    assert inf["s0_zero"]["S0"] == 0 and inf["s0_zero"]["buckets"] == []
    assert inf["one_factor"]["buckets"] == [(0, 1, 1)]
    assert inf["bucket_odd"]["buckets"] == [(0, 7, 1)] and inf["bucket_even"]["buckets"] == [(0, 8, 1)]
    (s0, s1, t), = inf["bucket_long"]["buckets"]
    assert s1 - s0 > 30 and s1 <= inf["bucket_long"]["CH"]
    for n, d in (("chunk_minus1", -1), ("chunk_exact", 0), ("chunk_plus1", 1)):
        assert inf[n]["buckets"][-1][1] == inf[n]["CH"] + d
    s0, s1, _ = inf["straddle_odd"]["buckets"][1]
    assert s0 < inf["straddle_odd"]["CH"] < s1 and (s1 - inf["straddle_odd"]["CH"]) % 2 == 1
    assert inf["full"]["S0"] > 4 * inf["full"]["CH"] and len(inf["full"]["buckets"]) == ws["full"].W
    assert ws["no_prior"].prior is None and ws["second_new"].marginalization_flag == abi.VIO_MARGIN_SECOND_NEW
    assert all(i["CH"] % 2 == 0 and i["lds"] == 1 for i in inf.values())


# (threads, variant, lane order) as tests/test_simt_backend.py: what the launcher picks in two lane orders, the lean LDS layout in the third
MODES = [(256, -1, 0), (256, -1, 1), (256, 2, 2)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_factor_pass_on_simt_emulator(name, mode, simt, cases):
    cfg, ws, exp = cases
    nthreads, variant, order = mode
    got, gs = H.solve_with(lambda c, w, s: simt.simt_solve_window(c, w, s, nthreads, variant, order), cfg, ws[name])
    MW.check_against_oracle(got, gs, *exp[name], report=name)


def test_global_matrix_variant_on_simt_emulator(simt):
    """W = 20: the dense matrix in global scratch, 512 work-items (eight waves own the buckets), the wide factor pass with its own
    staging chunk. The unedited window has more slots hosted at frame 0 than work-items and several chunks, so buckets continue
    behind chunk boundaries; it runs in all three lane orders."""
    cfg = abi.default_config(window_size=20)
    osolve, opre = H.oracle_backend()
    ws = MW.build_windows(cfg, lambda *a: abi.preintegrate_with(opre, cfg, *a), osolve, W=20, n_features=150, seed=7, full=False)
    inf = MW.marg_info(cfg, ws["full"], nthreads=512)
    assert inf["lds"] == 0 and inf["S0"] > 512 and inf["S0"] > inf["CH"]
    exp = MW.expectations(cfg, osolve, ws)
    for k, (name, w) in enumerate(sorted(ws.items())):
        for order in ((0, 1, 2) if name == "full" else (k % 3,)):
            got, gs = H.solve_with(lambda c, x, s: simt.simt_solve_window(c, x, s, 512, -1, order), cfg, w)
            MW.check_against_oracle(got, gs, *exp[name], report="w20 %s order %d" % (name, order))
