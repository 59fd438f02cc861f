"""Windows and capacity tables for the tests of windows that are smaller than the layout they run in. vio_backend_upload sizes a
batch for its largest window (Wcap, Pcap, nblk_cap, the strides, the LDS layout), rounds the landmark and factor capacities up and
carves the LDS for the batch's landmark maximum, so on the device a window's own W / F / M / prior n are almost never the
capacities. Shared by tests/test_window_capacities.py (SIMT emulator, capacities handed to simt_solve_window_caps) and
tests/test_window_capacities_gpu.py (device, ragged batches through WindowSolver.solve).

The windows are marg_pass_windows.chained_window outputs (window B of a sequence with the prior the oracle's solve of window A
leaves) with 40 or 60 landmarks, in four shapes: with that prior, with a relocalization pose on top, MARGIN_SECOND_NEW, and without
a prior. The expectation of a window is always the CPU oracle solving it alone under default_config(window_size=W), computed once
per process; the comparison is marg_pass_windows.check_against_oracle."""
import helpers as H
from helpers import abi, synth
import marg_pass_windows as MW

SHAPES = ("prior", "loop", "second_new", "no_prior")

# (W, Wcap, work-items): 256 = the LDS variant's workgroup (pose matrices up to W = 12), 512 = the global-matrix variant's
WCAP_CASES = [(3, 10, 256), (6, 7, 256), (6, 10, 256), (9, 10, 256), (9, 12, 256), (11, 12, 256), (6, 20, 512), (14, 20, 512)]

_oracle = None
_cache = {}


def oracle():
    global _oracle
    if _oracle is None:
        _oracle = H.oracle_backend()
    return _oracle


def window(W, shape, F=40):
    """(window, (oracle's solved window, its stats)) of size W and the given shape with F landmarks generated."""
    key = (W, shape, F)
    if key not in _cache:
        osolve, opre = oracle()
        cfg = abi.default_config(window_size=W)
        pre = lambda *a: abi.preintegrate_with(opre, cfg, *a)
        seed = 40 + W
        if shape == "prior":
            w = MW.chained_window(cfg, pre, osolve, seed, W=W, n_features=F)
        elif shape == "loop":
            w = MW.chained_window(cfg, pre, osolve, seed + 1, W=W, n_features=F, with_loop=F // 4)
            assert (w.factor_target == W + 1).any()
        elif shape == "second_new":
            w = window(W, "prior", F)[0].copy()
            w.marginalization_flag = abi.VIO_MARGIN_SECOND_NEW
        else:
            w = synth.make_window(cfg, pre, seed=3000 + seed, n_features=F, W=W)
            assert w.prior is None
        assert w.W == W and 30 <= w.n_features <= 60, (W, shape, w.n_features)
        if shape != "loop":
            assert not (w.factor_target == W + 1).any()
        _cache[key] = (w, MW.expectations(cfg, osolve, {"w": w})["w"])
    return _cache[key]


def launcher_fcap(cfg, F):
    """The landmark capacity vio_backend_upload gives a batch whose landmark maximum is F (25 % headroom, rounded up to 64s)."""
    return max(F, min(cfg.max_features, (F + F // 4 + 63) // 64 * 64))


def caps(Wcap=0, Fcap=0, Mcap=0, Ncap=0, Flds=0, loop_cap=0):
    """The `caps` argument of simt_solve_window_caps (0: the window's own)."""
    return [Wcap, Fcap, Mcap, Ncap, Flds, loop_cap]
