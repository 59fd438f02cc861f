"""Shared by tests/test_cauchy_on_demand.py (SIMT emulator) and tests/test_cauchy_on_demand_gpu.py: a large window whose trust
region binds, and what "binds" looks like in an iteration trace."""
import numpy as np

import helpers as H
from helpers import abi, synth

# A W = 20 window whose trust region binds twice: synth.make_window(window_size = 20, seed = 12, n_features = 40,
# perturb_scale = 20). Found by solving seeds 1 .. 12 at perturb_scale 8 and 20 with the CPU oracle and looking for a radius
# that triples exactly (an accepted step of norm == radius: only a step cut back to the region has it): at perturb_scale 8 none
# binds, at 20 all do at iteration 1, and seed 12 alone binds again on a REUSED step: iterations 6-8 reject the same
# Gauss-Newton step (equal step norms, the radius halves), iteration 9 takes a shorter step from the same linearization -- cut
# back to the region --, and iteration 10 triples the radius again. Both situations in which the on-demand path runs, on the
# general (W > 12) path.
BIND_W20 = dict(seed=12, n_features=40, W=20, perturb_scale=20.0)


def bind_w20_window():
    """(cfg, window, the CPU oracle's solution, the oracle's stats)"""
    cfg = abi.default_config(window_size=20)
    osolve, opre = H.oracle_backend()
    w = synth.make_window(cfg, lambda *a: abi.preintegrate_with(opre, cfg, *a), **BIND_W20)
    ref, rs = H.solve_with(osolve, cfg, w)
    return cfg, w, ref, rs


def tripled(radius):
    """Iterations whose radius is 3 x the previous one: an accepted step that ended ON the trust region's boundary."""
    r = np.asarray(radius, float)
    return [k for k in range(1, len(r)) if abs(r[k] - 3.0 * r[k - 1]) <= 1e-12 * r[k]]


def assert_binds_both_ways(rs):
    """The trace binds right after a solve (iteration 1) and on a reused step after rejections."""
    n = rs["iterations"] + 1
    fl, sn = [int(x) for x in rs["it_flags"]][:n], np.asarray(rs["it_step_norm"])[:n]
    assert tripled(np.asarray(rs["it_radius"])[:n])[0] == 1
    reused_cut = [k for k in range(2, len(fl)) if fl[k - 1] == 1 and fl[k - 2] == 1 and sn[k - 1] == sn[k - 2] and sn[k] < 0.99 * sn[k - 1]]
    assert reused_cut, (fl, sn)
