"""Windows for the tests of a solve's set-up (csrc/solver_core.h: the head of solve_window -- state load, slot records --,
build_gram_pieces, setup_imu_info, setup_prior). Shared by tests/test_setup_phases.py (SIMT emulator) and
tests/test_setup_phases_gpu.py (device).

What can go wrong there is a matter of sizes, so the windows are the smallest that put each size on an edge:
  * the prior's size n against the 16-column tiles and the 8-step operand batches of H0 = J0^T J0, whose accumulators are
    scattered straight into the reduced matrix: window A's landmarks hosted at frame 0 cut to targets <= m leave a prior of
    n = 15 + 6 m columns (speed-bias and pose of the new frame 0, m - 1 more poses, the extrinsic pose); no prior at all; the prior
    a MARGIN_SECOND_NEW solve leaves;
  * the factor and slot counts against the workgroup size and the batched slot-record fill: one factor, 255 / 256 / 257 factors,
    slot counts just below, at and just past 256 (a bucket starts on an even slot, so the count is even), the full window
    (four trips of 256 work-items) and a window of more than 1024 factors (a second batch of four trips).
Nothing is hard-coded: every candidate's layout is read from the emulator build (tests/emul/simt_setup_info.cpp: the pack / carve
code of the kernel source). The expectation of every window is the CPU oracle's solve, computed once per process."""
import ctypes as C

import numpy as np

import helpers as H
from helpers import abi, synth
import marg_pass_windows as MW

_info_lib = None


def setup_info(cfg, w, nthreads=256, variant=-1, order=0):
    """dict(M, nslots, npairs, prior_n, prior_nb, lds, nstage, staged) for window `w` as the emulator (and the launcher's rule) lays
    it out; order even: buckets aligned to the staging chunk (what the device packs)."""
    global _info_lib
    if _info_lib is None:
        _info_lib = H.build_emul_lib("simt_setup_info.cpp", "libvio_simt_setup_info.so", "VIO_SIMT")
        _info_lib.simt_setup_info.argtypes = [C.POINTER(abi.VioConfig), C.POINTER(abi.VioWindow), C.c_int, C.c_int, C.c_int,
                                              C.POINTER(C.c_int), C.c_int]
    out = (C.c_int * 8)()
    rc = _info_lib.simt_setup_info(C.byref(cfg), C.byref(w.struct()), nthreads, variant, order, out, 8)
    assert rc == abi.VIO_OK, rc
    d = dict(zip(("M", "nslots", "npairs", "prior_n", "prior_nb", "lds", "nstage", "threads"), [int(x) for x in out]))
    d["staged"] = d["prior_n"] ** 2 <= d["nstage"]
    return d


def first_factors(w, count):
    """A copy of `w` with its first `count` factors (the factors come grouped by ascending landmark, so a prefix stays grouped);
    the landmarks that keep a factor are renumbered."""
    keep = np.arange(w.n_factors) < count
    feats = np.unique(w.factor_feature[keep])
    renum = -np.ones(w.n_features, int)
    renum[feats] = np.arange(len(feats))
    return abi.Window(w.W, w.pose, w.speed_bias, w.ex_pose, w.inv_depth[feats], w.factor_host[keep], w.factor_target[keep],
                      renum[w.factor_feature[keep]], w.pts_i[keep], w.pts_j[keep], w.preint,
                      w.prior.copy() if w.prior is not None else None, w.marginalization_flag, w.loop_frame)


def prior_window(cfg, pre, osolve, seed, m, W=None, n_features=150):
    """Window B of a sequence whose window A had its landmarks hosted at frame 0 cut to the targets <= m: B carries a prior of
    15 + 6 m columns (MW.chained_window with the cut)."""
    a = synth.make_window(cfg, pre, seed=1000 + seed, traj_seed=seed, frame_offset=0, n_features=n_features, W=W)
    a = MW.edit_window(a, None, lambda q: m)
    a, _ = H.solve_with(osolve, cfg, a)
    assert a.next_prior.n == 15 + 6 * m, (a.next_prior.n, m)
    b = synth.make_window(cfg, pre, seed=2000 + seed, traj_seed=seed, frame_offset=1, n_features=n_features, W=W)
    b.prior = a.next_prior.copy()
    return b


def second_new_window(cfg, pre, osolve, seed, W=None, n_features=150):
    """A window that carries the prior a MARGIN_SECOND_NEW solve leaves (that solve's own prior comes from a MARGIN_OLD solve)."""
    b = MW.chained_window(cfg, pre, osolve, seed, W=W, n_features=n_features)
    b.marginalization_flag = abi.VIO_MARGIN_SECOND_NEW
    b, _ = H.solve_with(osolve, cfg, b)
    assert b.next_prior.n > 0
    c = synth.make_window(cfg, pre, seed=4000 + seed, traj_seed=seed, frame_offset=1, n_features=n_features, W=W)
    c.prior = b.next_prior.copy()
    return c


def find_prefix(cfg, base, want, lo=1):
    """The shortest prefix of base's factors (at least `lo`) whose layout satisfies want(info)."""
    for count in range(lo, base.n_factors + 1):
        e = first_factors(base, count)
        if want(setup_info(cfg, e)):
            return e
    raise AssertionError("no such prefix of this window: pick another seed")


PRIOR_M = (1, 3, 8, 10)  # n = 21, 33, 63, 75


def build_windows(cfg, pre, osolve, W=None, n_features=150, seed=42, prior_m=PRIOR_M, sizes=True):
    """{name: window}. prior_m: the cuts of window A (the last one must be W: the uncut window, `full`); sizes = False: without the
    factor / slot count cases around the workgroup size."""
    ws = {}
    for m in prior_m[:-1]:
        ws["prior_m%d" % m] = prior_window(cfg, pre, osolve, seed, m, W=W, n_features=n_features)
    base = MW.chained_window(cfg, pre, osolve, seed, W=W, n_features=n_features)
    assert base.W == prior_m[-1] and base.prior.n == 15 + 6 * base.W
    ws["full"] = base
    nop = synth.make_window(cfg, pre, seed=3000 + seed, n_features=n_features, W=W)
    assert nop.prior is None
    ws["no_prior"] = nop
    ws["prior_second_new"] = second_new_window(cfg, pre, osolve, seed, W=W, n_features=n_features)
    ws["one_factor"] = first_factors(base, 1)
    if sizes:
        for count in (255, 256, 257):
            ws["factors_%d" % count] = first_factors(base, count)
        # slots: a bucket starts on an even slot and does not straddle a staging chunk, so the count moves in steps of two or more:
        # the last prefix below the workgroup size, the one that meets it, the first one past it
        exact = find_prefix(cfg, base, lambda i: i["nslots"] == 256, lo=100)
        ws["slots_below"], ws["slots_exact"] = first_factors(base, exact.n_factors - 1), exact
        ws["slots_above"] = find_prefix(cfg, base, lambda i: i["nslots"] > 256, lo=exact.n_factors)
    return ws


def many_factors_window(cfg, pre, osolve, seed=42, n_features=200):
    """More than 1024 factors: the slot-record fill of 256 work-items takes a second batch of four trips (the lean LDS layout)."""
    w = MW.chained_window(cfg, pre, osolve, seed, n_features=n_features)
    assert w.n_factors > 1024, w.n_factors
    return w
