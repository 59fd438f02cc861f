"""Windows for the tests of the marginalization's factor pass (csrc/marg_core.h: the projection factors hosted at frame 0 are
evaluated into a staging area chunk by chunk and multiplied bucket by bucket, a bucket staying with one wave across the chunks it
spans). Shared by tests/test_marg_factor_pass.py (SIMT emulator) and tests/test_marg_factor_pass_gpu.py (device).

The windows are synth.make_window outputs whose landmarks hosted at frame 0 are kept, dropped or cut short so that the slot ranges
the pass walks hit the places where a range can go wrong. Nothing is hard-coded: the staging chunk and the slot layout of every
candidate are read from the emulator build (tests/emul/simt_marg_info.cpp: the pack / carve code of the kernel source).
The expectation of every window is the CPU oracle's solve (H.oracle_backend()), computed once per process."""
import ctypes as C

import numpy as np

import helpers as H
from helpers import abi, synth

TOL_STATE = 1e-6  # tests/test_backend_gpu.py: TOL
TOL_PRIOR = 1e-5  # tests/test_backend_gpu.py: TOL_PRIOR

_info_lib = None


def marg_info(cfg, w, nthreads=256, variant=-1, order=1):
    """dict(CH=staging chunk in slots, S0=slots the pass walks, buckets=[(s0, s1, t)] of the buckets hosted at frame 0, lds=matrix in
    LDS) for window `w` as the emulator (and the launcher's rule) lays it out; order odd: buckets not aligned to the solver's chunks."""
    global _info_lib
    if _info_lib is None:
        _info_lib = H.build_emul_lib("simt_marg_info.cpp", "libvio_simt_marg_info.so", "VIO_SIMT")
        _info_lib.simt_marg_info.argtypes = [C.POINTER(abi.VioConfig), C.POINTER(abi.VioWindow), C.c_int, C.c_int, C.c_int,
                                             C.POINTER(C.c_int), C.c_int]
    cap = 4 + 3 * 64
    out = (C.c_int * cap)()
    rc = _info_lib.simt_marg_info(C.byref(cfg), C.byref(w.struct()), nthreads, variant, order, out, cap)
    assert rc == abi.VIO_OK, rc
    nb = (cap - 4) // 3
    buckets = [(out[4 + 3 * i], out[5 + 3 * i], out[6 + 3 * i]) for i in range(nb) if out[5 + 3 * i] > out[4 + 3 * i]]
    return dict(CH=out[0], S0=out[1], nb0=out[2], lds=out[3], buckets=[b for b in buckets if b[2] != w.W + 1])


def _ranges(w):
    """factor range [lo, hi) of every landmark (the factors come grouped by ascending landmark)"""
    return np.searchsorted(w.factor_feature, np.arange(w.n_features + 1))


def host0_tracks(w):
    """[(feature, last target)] of the landmarks hosted at frame 0, in feature order (window targets only)."""
    out, r = [], _ranges(w)
    for f in range(w.n_features):
        if r[f + 1] > r[f] and w.factor_host[r[f]] == 0:
            t = w.factor_target[r[f]:r[f + 1]]
            out.append((f, int(t[t <= w.W].max()) if (t <= w.W).any() else 0))
    return out


def edit_window(w, keep_host0=None, tmax=None):
    """A copy of `w` with the landmarks hosted at frame 0 edited: only the first `keep_host0` of them stay (None: all), and the
    j-th one keeps the factors whose target is <= tmax(j) (None: all of them). Landmarks hosted elsewhere stay as they are. A
    landmark left without a factor leaves the window; the landmarks are renumbered."""
    keep = np.zeros(w.n_factors, bool)
    j, r = 0, _ranges(w)
    for f in range(w.n_features):
        k = np.arange(r[f], r[f + 1])
        if not len(k):
            continue
        if w.factor_host[k[0]] != 0:
            keep[k] = True
            continue
        if keep_host0 is None or j < keep_host0:
            keep[k] = True if tmax is None else w.factor_target[k] <= tmax(j)
        j += 1
    feats = np.unique(w.factor_feature[keep])
    renum = -np.ones(w.n_features, int)
    renum[feats] = np.arange(len(feats))
    e = abi.Window(w.W, w.pose, w.speed_bias, w.ex_pose, w.inv_depth[feats], w.factor_host[keep], w.factor_target[keep],
                   renum[w.factor_feature[keep]], w.pts_i[keep], w.pts_j[keep], w.preint,
                   w.prior.copy() if w.prior is not None else None, w.marginalization_flag, w.loop_frame)
    return e


def chained_window(cfg, pre, osolve, seed, W=None, n_features=150, with_loop=0):
    """Window B of a sequence carrying the prior that the oracle's MARGIN_OLD solve of window A leaves (bench.steady_state_windows)."""
    a = synth.make_window(cfg, pre, seed=1000 + seed, traj_seed=seed, frame_offset=0, n_features=n_features, W=W)
    a, _ = H.solve_with(osolve, cfg, a)
    assert a.next_prior.n > 0
    b = synth.make_window(cfg, pre, seed=2000 + seed, traj_seed=seed, frame_offset=1, n_features=n_features, W=W, with_loop=with_loop)
    b.prior = a.next_prior.copy()
    return b


def two_bucket(w, k, j):
    """The first k landmarks hosted at frame 0, cut to the targets 1 and 2; the last j of them to target 1 alone."""
    return edit_window(w, k, lambda q: 1 if q >= k - j else 2)


def find_two_bucket(cfg, w, want):
    """The first (k, j) whose two_bucket window satisfies want(info); info = marg_info of that window. (k, j) is worked out from
    the track lengths -- bucket (0, 1) takes the slots [0, k), bucket (0, 2) starts on the next even slot -- and then checked on
    the layout the emulator build really gives."""
    tr = host0_tracks(w)
    for k in range(2, len(tr) + 1):
        ch = marg_info(cfg, two_bucket(w, k, 0))["CH"]
        for j in range(0, k):
            n2 = sum(1 for _, t in tr[:k - j] if t >= 2)
            s0 = (k + 1) & ~1
            if n2 == 0 or not want(dict(CH=ch, buckets=[(0, k, 1), (s0, s0 + n2, 2)])):
                continue
            e = two_bucket(w, k, j)
            inf = marg_info(cfg, e)
            if want(inf):
                return e, inf
    raise AssertionError("no such window among the edits of this seed: pick another seed")


def build_windows(cfg, pre, osolve, W=None, n_features=150, seed=42, with_loop=20, full=True):
    """{name: window}: the cases of the factor pass for one window size. full = False: the cases that need no more landmarks hosted at frame 0
    than any window has (the W = 6 and W = 20 sets: their staging chunks are larger than two buckets of a 150-landmark window)."""
    base = chained_window(cfg, pre, osolve, seed, W=W, n_features=n_features)
    ws = {"full": base}
    ws["s0_zero"] = edit_window(base, 0)                                   # no landmark hosted at frame 0
    ws["one_factor"] = edit_window(base, 1, lambda q: 1)                   # the odd tail alone
    ws["bucket_odd"] = edit_window(base, 7, lambda q: 1)                   # a single bucket (0, 1)
    ws["bucket_even"] = edit_window(base, 8, lambda q: 1)
    ch = marg_info(cfg, base)["CH"]
    if not full:
        return ws
    # a bucket that straddles a chunk boundary and ends in an odd tail behind it. (Buckets start on even slots and the chunk is even,
    # so a boundary never falls between the two factors of a step: what can go wrong is the tail of the part behind the boundary.)
    ws["straddle_odd"], inf = find_two_bucket(
        cfg, base, lambda i: len(i["buckets"]) == 2 and i["buckets"][1][0] < i["CH"] < i["buckets"][1][1] and (i["buckets"][1][1] - i["CH"]) % 2 == 1)
    ws["bucket_long"] = edit_window(base, min(45, ch - 3), lambda q: 1)    # longer than one Gram piece (kGramPiece = 30 slots)
    # the last slot in use at the chunk size, one short of it and one past it
    for name, d in (("chunk_minus1", -1), ("chunk_exact", 0), ("chunk_plus1", 1)):
        ws[name], inf = find_two_bucket(cfg, base, lambda i, d=d: len(i["buckets"]) == 2 and i["buckets"][1][1] == i["CH"] + d)
    ws["with_loop"] = chained_window(cfg, pre, osolve, seed + 1, W=W, n_features=n_features, with_loop=with_loop)
    assert (ws["with_loop"].factor_target == ws["with_loop"].W + 1).any()
    nop = synth.make_window(cfg, pre, seed=3000 + seed, n_features=n_features, W=W)  # no prior
    assert nop.prior is None
    ws["no_prior"] = nop
    sn = base.copy()
    sn.marginalization_flag = abi.VIO_MARGIN_SECOND_NEW
    ws["second_new"] = sn
    return ws


def expectations(cfg, osolve, ws):
    """{name: (oracle's solved window, its stats)}; every window must leave a prior with finite H and b."""
    out = {}
    for name, w in ws.items():
        ref, rs = H.solve_with(osolve, cfg, w)
        assert ref.next_prior.n > 0, name
        Hr, br, _ = ref.next_prior.canonical()
        assert np.isfinite(Hr).all() and np.isfinite(br).all(), name
        out[name] = (ref, rs)
    return out


def check_against_oracle(got, gs, ref, rs, report=None):
    Hr, br, xr = ref.next_prior.canonical()
    Hg, bg, xg = got.next_prior.canonical() if got.next_prior.n > 0 else (np.zeros((0, 0)), np.zeros(0), [])
    figs = dict(n=(got.next_prior.n, ref.next_prior.n), pose=H.pose_relerr(got.pose, ref.pose),
                sb=H.relerr(got.speed_bias, ref.speed_bias), depth=H.relerr(got.inv_depth, ref.inv_depth),
                H=H.relerr(Hg, Hr) if Hg.shape == Hr.shape else float("inf"), b=H.relerr(bg, br) if bg.shape == br.shape else float("inf"),
                iters=(gs["iterations"], rs["iterations"]))
    if report is not None:
        print("%-14s %s" % (report, " ".join("%s=%s" % (k, ("%.2e" % v) if isinstance(v, float) else v) for k, v in figs.items())))
    assert got.next_prior.n == ref.next_prior.n
    assert sorted((k, i) for k, i, _, _ in got.next_prior.blocks()) == sorted((k, i) for k, i, _, _ in ref.next_prior.blocks())
    assert [(k, i) for k, i, _ in xg] == [(k, i) for k, i, _ in xr]
    assert figs["H"] < TOL_PRIOR and figs["b"] < TOL_PRIOR
    for (_, _, a), (_, _, b) in zip(xg, xr):
        assert np.abs(a - b).max() < TOL_STATE
    assert figs["pose"] < TOL_STATE and figs["sb"] < TOL_STATE and figs["depth"] < TOL_STATE
    assert gs["iterations"] == rs["iterations"] and gs["termination"] == rs["termination"]
    assert list(gs["it_flags"]) == list(rs["it_flags"])
