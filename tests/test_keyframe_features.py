"""KeyFrame::buildKeyFrameFeatures (VINS_ios/loop/keyframe.cpp:128-155) through its three layers: vio_features_keyframe on the
host-side list against a numpy restatement written here; the fourth pass of the device store (store_keyframe, csrc/
store_core.h) on the wave64 SIMT emulator against that host function, bit for bit; vio_estimator_keyframe_features on
resident sequences (GPU), which must give what the host function gives on the fetched list and leave the sequences
resident; and the chain keyframe_features -> LoopDetector.connect -> set_relocalization."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import helpers as H
from helpers import abi, pkg, synth

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
import replay_synthetic as RS  # noqa: E402

_ip, _dp, _fp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float)
FIRST, REACH, FEW, KEPT = 1, 2, 3, 0


# ---- lists ------------------------------------------------------------------------------------------------------------------
def verdict(n_obs, start, W):
    """:133 and :136 as written."""
    if not (n_obs >= 2 and start < W - 2):
        return FIRST
    if not (start + n_obs >= W - 1 and n_obs >= 3):
        return REACH if not start + n_obs >= W - 1 else FEW
    return KEPT


def points_for(rows, rng):
    """Observations of every landmark: FeaturePerFrame::point is (x / z, y / z, 1); some z are not 1 so that the divisions
    of :141-144 are real ones."""
    n = int(sum(r[2] for r in rows))
    pts = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.45, 0.45, n), np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.8, 1.25, n))], 1)
    return pts


def hand_list(W, rng):
    """(id, start_frame, n_obs, used_num, solve_flag, is_outlier, fixed, estimated_depth); used_num deliberately stale."""
    rows = [
        (3, 0, 1, 7, 0, 0, 0, 4.0),                # n_obs 1
        (5, 0, 2, 0, 1, 0, 0, 6.5),                # n_obs 2 at start 0: does not reach frame W - 2
        (6, W - 2, 2, 0, 0, 0, 0, -1.0),           # start W - 2: not of the solved window
        (8, W - 3, 2, 9, 1, 0, 0, 3.25),           # start W - 3 with 2 observations: reaches, but fewer than three
        (9, 0, 3, 0, 1, 0, 0, 8.0),                # three observations that end before frame W - 2
        (11, 0, W - 1, 1, 1, 0, 1, 5.5),           # the boundary start + n = W - 1: kept, its measurement is its last observation
        (12, 0, W + 1, 0, 1, 0, 1, 2.75),          # seen in every frame
        (14, W - 4, 3, 0, 1, 0, 0, 7.125),         # start W - 4 with 3 observations: the measurement is its last one
        (15, 1, W - 2, 0, 0, 0, 0, -1.0),          # kept with the depth of a landmark never triangulated
        (17, 0, W, 3, 2, 1, 0, -3.7),              # kept with a negative depth and solve_flag 2: the reference tests neither
        (21, W - 1, 1, 0, 0, 0, 0, -1.0),
        (22, W, 1, 0, 0, 0, 0, -1.0),
    ]
    return rows, points_for(rows, rng)


def grown_list(W, n_keep, n_drop, rng):
    """n_keep qualifying landmarks and n_drop others in random list order, ascending ids."""
    kinds = rng.permutation(np.array([1] * n_keep + [0] * n_drop))
    rows = []
    for i, k in enumerate(kinds):
        if k:
            s = int(rng.integers(0, W - 2))
            n = int(rng.integers(max(3, W - 1 - s), W + 1 - s + 1))
        else:
            which = int(rng.integers(0, 3))
            if which == 0:
                s, n = int(rng.integers(W - 2, W + 1)), 1
            elif which == 1:
                s = int(rng.integers(0, W - 3))
                n = int(rng.integers(1, W - 1 - s))                        # start + n < W - 1
            else:
                s, n = W - 3, 2
            n = min(n, W + 1 - s)
        rows.append((100 + 2 * i, s, n, 0, int(rng.integers(0, 3)), 0, 0, float(rng.choice([-1.0, rng.uniform(0.5, 15.0), -rng.uniform(0.5, 4.0)]))))
        assert (verdict(n, s, W) == KEPT) == bool(k)
    return rows, points_for(rows, rng)


def states(W, rng):
    P = W + 1
    Rs = np.array([synth.rotvec_to_rot(rng.normal(0, 0.4, 3)) for _ in range(P)])
    Ps = rng.uniform(-8, 8, (P, 3))
    ric = synth.rotvec_to_rot(np.array([0.02, -0.03, 1.55]))
    tic = np.array([0.02, -0.04, 0.01])
    return Ps, Rs, tic, ric


def restate(rows, pts, W, cfg, Ps, Rs, tic, ric):
    """buildKeyFrameFeatures in numpy -> ids, px, norm, cloud, verdicts."""
    ids, px, norm, cloud, seen = [], [], [], [], []
    o = 0
    for (fid, s, n, _, _, _, _, depth) in rows:
        p = pts[o:o + n]
        o += n
        v = verdict(n, s, W)
        seen.append(v)
        if v != KEPT:
            continue
        m = p[W - 2 - s]
        px.append((np.float32(cfg.fx * m[0] / m[2] + cfg.cx), np.float32(cfg.fy * m[1] / m[2] + cfg.cy)))
        norm.append((np.float32(m[0] / m[2]), np.float32(m[1] / m[2])))
        ids.append(fid)
        cloud.append(Rs[s] @ (ric @ (p[0] * depth) + tic) + Ps[s])
    return (np.array(ids, np.int32), np.array(px, np.float32).reshape(-1, 2), np.array(norm, np.float32).reshape(-1, 2),
            np.array(cloud).reshape(-1, 3), seen)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the host function against the restatement -----------------------------------------------------------------------------
@pytest.mark.parametrize("W", [5, 10])
def test_host_function_matches_the_restatement(W):
    rng = np.random.default_rng(300 + W)
    cfg = abi.default_config(window_size=W)
    Ps, Rs, tic, ric = states(W, rng)
    rows, pts = hand_list(W, rng)
    want = restate(rows, pts, W, cfg, Ps, Rs, tic, ric)
    assert {FIRST, REACH, FEW, KEPT} <= set(want[4])                    # each of the four outcomes of the predicate occurs
    kept_depths = [r[7] for r, v in zip(rows, want[4]) if v == KEPT]
    assert -1.0 in kept_depths and min(kept_depths) < -1.0
    fm = pkg.window.FeatureManager(W)
    fm.load(rows, pts)
    before, pts_before = fm.dump()
    rc, n, ids, px, norm, cloud = fm.keyframe(cfg, Ps, Rs, tic, ric)
    assert rc == abi.VIO_OK and n == len(want[0]) > 0
    assert same_bits(ids, want[0]) and same_bits(px, want[1]) and same_bits(norm, want[2])
    # about twenty roundings of 1.1e-16 on magnitudes of order ten
    assert (np.abs(cloud - want[3]) <= 1e-12 * np.maximum(1.0, np.abs(want[3]))).all()
    after, pts_after = fm.dump()
    assert np.array_equal(after[:, 3], after[:, 2]) and not np.array_equal(before[:, 3], before[:, 2])   # used_num = n_obs
    keep = [0, 1, 2, 4, 5, 6, 7]
    assert same_bits(after[:, keep], before[:, keep]) and same_bits(pts_after, pts_before)            # nothing else moved
    # VIO_ECAP reports -(needed); the first cap entries are there
    rc, m, ids2, px2, _, cloud2 = fm.keyframe(cfg, Ps, Rs, tic, ric, cap=n - 2)
    assert rc == abi.VIO_ECAP and m == -n and same_bits(ids2, ids[:n - 2]) and same_bits(px2, px[:n - 2]) and same_bits(cloud2, cloud[:n - 2])
    rc, m, ids2, _, _, _ = fm.keyframe(cfg, Ps, Rs, tic, ric, cap=0)
    assert rc == abi.VIO_ECAP and m == -n and len(ids2) == 0
    fm.close()


# ---- 2. pass 4 of store_core.h on the SIMT emulator ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emul():
    l = H.build_emul_lib("simt_keyframe.cpp", "libvio_simt_keyframe.so", "VIO_SIMT")
    l.simt_store_keyframe.argtypes = [C.c_int] * 4 + [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, C.c_int, _ip, _fp, _fp, _dp, _ip]
    return l


def run_emulated(emul, W, Lcap, bank, rows, pts, cfg, Ps, Rs, tic, ric, cap, order):
    info = (abi.VioFeatureInfo * max(len(rows), 1))()
    for f, r in zip(info, rows):
        f.id, f.start_frame, f.n_obs, f.used_num, f.solve_flag, f.is_outlier, f.fixed = (int(x) for x in r[:7])
        f.estimated_depth = float(r[7])
    c = max(cap, 1)
    ids = np.full(c + 1, -7, np.int32)                                # poisoned: what is not written stays recognisable
    px, norm, cloud = np.full((c + 1, 2), np.nan, np.float32), np.full((c + 1, 2), np.nan, np.float32), np.full((c + 1, 3), np.nan)
    count = np.full(1, -12345, np.int32)
    a = [np.ascontiguousarray(x, np.float64) for x in (pts, Ps, Rs, tic, ric, [cfg.fx, cfg.fy, cfg.cx, cfg.cy])]
    rc = emul.simt_store_keyframe(W, Lcap, bank, len(rows), C.cast(info, C.c_void_p), *[x.ctypes.data_as(_dp) for x in a], cap, order,
                                  ids.ctypes.data_as(_ip), px.ctypes.data_as(_fp), norm.ctypes.data_as(_fp), cloud.ctypes.data_as(_dp),
                                  count.ctypes.data_as(_ip))
    assert rc == 0
    k = min(abs(int(count[0])), cap)
    assert (ids[k:] == -7).all() and np.isnan(px[k:]).all() and np.isnan(norm[k:]).all() and np.isnan(cloud[k:]).all()   # nothing behind the row's end
    return int(count[0]), ids[:k], px[:k], norm[:k], cloud[:k]


EMUL_CASES = [  # W, qualifying, others, Lcap, bank, lane order
    (5, 0, 40, 1024, 0, 0), (10, 1, 30, 1024, 1, 1), (10, 63, 50, 1024, 0, 2), (5, 64, 20, 1024, 1, 3), (10, 65, 90, 1024, 0, 1),
    (10, 257, 60, 1024, 1, 2),      # more than one trip of the 256 work-items over the list
    (5, 257, 43, 300, 0, 3),        # a slot at Lcap
    (10, 300, 340, 640, 1, 0),      # three trips, the last one full, at Lcap
]


@pytest.mark.parametrize("W,n_keep,n_drop,Lcap,bank,order", EMUL_CASES)
def test_store_pass_matches_the_host_function_bit_for_bit(emul, W, n_keep, n_drop, Lcap, bank, order):
    rng = np.random.default_rng(1000 * W + n_keep)
    cfg = abi.default_config(window_size=W)
    Ps, Rs, tic, ric = states(W, rng)
    rows, pts = grown_list(W, n_keep, n_drop, rng)
    fm = pkg.window.FeatureManager(W)
    fm.load(rows, pts)
    rc, n, ids, px, norm, cloud = fm.keyframe(cfg, Ps, Rs, tic, ric, cap=Lcap)
    assert rc == abi.VIO_OK and n == n_keep
    got = run_emulated(emul, W, Lcap, bank, rows, pts, cfg, Ps, Rs, tic, ric, Lcap, order)
    assert got[0] == n
    assert same_bits(got[1], ids) and same_bits(got[2], px) and same_bits(got[3], norm) and same_bits(got[4], cloud)
    if n_keep > 2:                                                     # a row too short: -(needed), the first cap entries
        got = run_emulated(emul, W, Lcap, bank, rows, pts, cfg, Ps, Rs, tic, ric, n_keep - 2, order)
        assert got[0] == -n and same_bits(got[1], ids[:n - 2]) and same_bits(got[4], cloud[:n - 2])
    fm.close()


@pytest.mark.parametrize("W", [5, 10])
def test_store_pass_on_the_hand_built_lists(emul, W):
    rng = np.random.default_rng(300 + W)                               # the lists of test 1
    cfg = abi.default_config(window_size=W)
    Ps, Rs, tic, ric = states(W, rng)
    rows, pts = hand_list(W, rng)
    fm = pkg.window.FeatureManager(W)
    fm.load(rows, pts)
    rc, n, ids, px, norm, cloud = fm.keyframe(cfg, Ps, Rs, tic, ric)
    for order in (0, 1, 2):
        got = run_emulated(emul, W, 64, order & 1, rows, pts, cfg, Ps, Rs, tic, ric, 64, order)
        assert got[0] == n and same_bits(got[1], ids) and same_bits(got[2], px) and same_bits(got[3], norm) and same_bits(got[4], cloud)
    fm.close()


# ---- 3. argument errors; no device ------------------------------------------------------------------------------------------
def test_argument_errors():
    lib = abi.load_product()
    W = 5
    cfg = abi.default_config(window_size=W)
    rng = np.random.default_rng(1)
    Ps, Rs, tic, ric = states(W, rng)
    fm = pkg.window.FeatureManager(W)
    a = [np.ascontiguousarray(x, np.float64) for x in (Ps, Rs, tic, ric)]
    p = [x.ctypes.data_as(_dp) for x in a]
    ids, px, cloud, n = np.zeros(4, np.int32), np.zeros((4, 2), np.float32), np.zeros((4, 3)), C.c_int32(77)
    ok = (ids.ctypes.data_as(_ip), px.ctypes.data_as(_fp), px.ctypes.data_as(_fp), cloud.ctypes.data_as(_dp), C.byref(n))
    f = lib.vio_features_keyframe
    assert f(None, C.byref(cfg), *p, 4, *ok) == abi.VIO_EINVAL
    assert f(fm._h, None, *p, 4, *ok) == abi.VIO_EINVAL
    assert f(fm._h, C.byref(cfg), None, *p[1:], 4, *ok) == abi.VIO_EINVAL
    assert f(fm._h, C.byref(cfg), *p, -1, *ok) == abi.VIO_EINVAL
    assert f(fm._h, C.byref(cfg), *p, 4, None, *ok[1:]) == abi.VIO_EINVAL
    assert f(fm._h, C.byref(cfg), *p, 4, *ok[:4], None) == abi.VIO_EINVAL
    assert n.value == 77
    assert f(fm._h, C.byref(cfg), *p, 4, *ok) == abi.VIO_OK and n.value == 0      # an empty list
    fm.close()
    est = pkg.estimator.Estimator(cfg, tic, ric, n_seq=3)
    g = lib.vio_estimator_keyframe_features
    seq, cnt = np.array([0, 2, 1], np.int32), np.full(3, 55, np.int32)
    outs = (ids.ctypes.data_as(_ip), px.ctypes.data_as(_fp), px.ctypes.data_as(_fp), cloud.ctypes.data_as(_dp))
    sp, cp = seq.ctypes.data_as(_ip), cnt.ctypes.data_as(_ip)
    assert g(None, 3, sp, 1, *outs, cp) == abi.VIO_EINVAL
    assert g(est._h, 3, None, 1, *outs, cp) == abi.VIO_EINVAL
    assert g(est._h, 3, sp, -1, *outs, cp) == abi.VIO_EINVAL
    assert g(est._h, 3, sp, 1, None, *outs[1:], cp) == abi.VIO_EINVAL
    assert g(est._h, 3, sp, 1, *outs, None) == abi.VIO_EINVAL
    assert g(est._h, 4, sp, 1, *outs, cp) == abi.VIO_EINVAL             # more sequences than there are
    for bad in ([0, 0, 1], [0, 3, 1], [0, -1, 1]):                      # a sequence twice; outside [0, n_seq)
        b = np.array(bad, np.int32)
        assert g(est._h, 3, b.ctypes.data_as(_ip), 1, *outs, cp) == abi.VIO_EINVAL
    assert (cnt == 55).all()
    assert g(est._h, 3, sp, 1, *outs, cp) == abi.VIO_OK and (cnt == -1).all()   # no sequence has a full NON_LINEAR window yet
    est.close()


def test_keyframe_features_without_a_device(tmp_path):
    """No device is needed while no sequence is resident (none can be without one): the call answers count = -1 for
    sequences that are still filling instead of failing."""
    script = tmp_path / "nodev.py"
    script.write_text(textwrap.dedent("""
        import importlib, sys
        import numpy as np
        sys.path.insert(0, %r)
        pkg = importlib.import_module("vins-mobile_amd")
        cfg = pkg.abi.default_config(window_size=5)
        est = pkg.estimator.Estimator(cfg, np.zeros(3), np.eye(3), n_seq=2)
        rc, out = est.keyframe_features([1, 0], stride=8)
        assert rc == pkg.abi.VIO_OK and [o[0] for o in out] == [-1, -1], (rc, out)
        est.close()
        print("answered")
    """ % H.ROOT))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "answered" in r.stdout, r.stdout + r.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def host_view(est, cfg, world, seq=0):
    """(c): the list comes back to the host, vio_features_keyframe on it with get_window()'s states."""
    fm = est.features(seq)
    w = est.window(seq)
    rec, _ = fm.dump()
    return fm.keyframe(cfg, w["Ps"], w["Rs"], world.tic, world.ric), len(rec)


def same_keyframe(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("W,seed", [(5, 33), (10, 5)])
def test_resident_sequences_give_what_the_fetched_list_gives(W, seed):
    """At every keyframe (a) keyframe_features, (b) still resident, (c) the list fetched and vio_features_keyframe on it:
    two views of one state through single-source arithmetic, bit-equal. A twin that only ever makes call (a) follows an
    estimator that never makes it (the window kernel's sums are not reproducible to the bit: poses to the 1e-5 of
    test_resident_sequences_give_what_the_host_side_list_gives, decisions and counts exactly) and stays resident throughout;
    at the very end its own (a) is checked against (c) too, many bank flips after its list went to the device."""
    cfg = abi.default_config(window_size=W)
    main, twin, plain = (RS.EstimatorLoop(cfg, seed=seed, init_noise=1.0) for _ in range(3))
    for lp in (main, twin, plain):
        lp.est.set_resident(True)
    keyframes = with_points = kept = dropped = 0
    for _ in range(40):
        a, b, c = main.step(), twin.step(), plain.step()
        assert b.action == c.action and b.marginalization_flag == c.marginalization_flag and b.n_factors == c.n_factors
        assert b.n_features == c.n_features
        if b.action == abi.VIO_FRAME_SOLVED:
            assert b.stats.iterations == c.stats.iterations
            assert np.abs(twin.history[-1][1] - plain.history[-1][1]).max() < 1e-5
        if b.action == abi.VIO_FRAME_SOLVED and b.marginalization_flag == abi.VIO_MARGIN_OLD:
            rc, (tw,) = twin.est.keyframe_features([0])               # the twin: (a) and nothing else
            assert rc == abi.VIO_OK and tw[0] >= 0 and twin.est.status().resident == 1
        if a.action != abi.VIO_FRAME_SOLVED or a.marginalization_flag != abi.VIO_MARGIN_OLD:
            continue
        rc, (got,) = main.est.keyframe_features([0])                  # (a)
        assert rc == abi.VIO_OK and got[0] >= 0
        assert main.est.status().resident == 1                         # (b)
        (rc2, n, *want), n_list = host_view(main.est, cfg, main.world)  # (c)
        assert rc2 == abi.VIO_OK and n == got[0] and same_keyframe(got[1:], want)
        keyframes += 1
        with_points += n > 0
        kept += n
        dropped += n_list - n
    print("W %d: %d keyframes, %d with points, %d kept, %d dropped" % (W, keyframes, with_points, kept, dropped))
    assert keyframes >= 5 and with_points >= 1 and kept > 0 and dropped > 0
    assert twin.est.status().resident == 1
    rc, (tw,) = twin.est.keyframe_features([0])
    (rc2, n, *want), _ = host_view(twin.est, cfg, twin.world)
    assert rc == rc2 == abi.VIO_OK and tw[0] == n > 0 and same_keyframe(tw[1:], want)
    for lp in (main, twin, plain):
        lp.close()


class _SeqView:
    """Routes a feeder's single-sequence calls to sequence q of a shared estimator."""

    def __init__(self, est, q):
        self.est, self.q = est, q

    def process_imu(self, dt, a, w):
        self.est.process_imu(dt, a, w, seq=self.q)

    def set_initial_state(self, *a):
        self.est.set_initial_state(*a, seq=self.q)

    def close(self):
        pass


@pytest.mark.gpu
def test_batch_of_four_sequences():
    """Two resident sequences, one held on the host-side list by a capacity fallback (a relocalization frame with more matched
    ids than a store slot takes keeps its sequence off the device while the frame is in the window), one still filling."""
    cfg = abi.default_config(window_size=6)
    W, nq = cfg.window_size, 4
    worlds = [RS.SyntheticWorld(cfg, 40 + q) for q in range(nq)]
    est = pkg.estimator.Estimator(cfg, worlds[0].tic, worlds[0].ric, n_seq=nq)
    est.set_resident(True)
    feeders = [RS.EstimatorLoop(cfg, seed=40 + q, init_noise=1.0, world=worlds[q]) for q in range(nq)]
    for f, q in zip(feeders, range(nq)):
        f.est.close()
        f.est = _SeqView(est, q)
    start = [0, 0, 0, 14]
    for call in range(18):
        obs, hdr, act = [], [], []
        for q in range(nq):
            k = call - start[q]
            if k < 0:
                obs.append(([], [])), hdr.append(0.0), act.append(0)
            else:
                obs.append(feeders[q].feed_until_image()), hdr.append(worlds[q].time(k)), act.append(1)
        if call == 16:
            assert [est.status(q).resident for q in range(nq)] == [1, 1, 1, 0]
            # 300 ids no landmark has, matched to the newest frame: no factor comes of it, but the list stays on the host
            est.set_relocalization(est.window(2)["headers"][W], np.zeros(3), [0, 0, 0, 1], 10 ** 6 + np.arange(300), np.zeros((300, 2)), seq=2)
        res = est.process_images(obs, hdr, act)
    assert [r.action for r in res[:3]] == [abi.VIO_FRAME_SOLVED] * 3 and res[3].action == abi.VIO_FRAME_FILLING
    assert res[2].n_loop_factors == 0
    assert [est.status(q).resident for q in range(nq)] == [1, 1, 0, 0]   # sequence 2 was solved on the host-side list and stays there
    order = [3, 1, 2, 0]
    rc, batch = est.keyframe_features(order, stride=512)
    assert rc == abi.VIO_OK
    assert [est.status(q).resident for q in range(nq)] == [1, 1, 0, 0]  # nobody moved
    by_seq = dict(zip(order, batch))
    assert by_seq[3][0] == -1 and len(by_seq[3][1]) == 0
    for q in (0, 1, 2):
        rc, (single,) = est.keyframe_features([q], stride=512)
        assert rc == abi.VIO_OK and single[0] == by_seq[q][0] > 2 and same_keyframe(single[1:], by_seq[q][1:]), q
    (rc, n, *want), _ = host_view(est, cfg, worlds[2], 2)
    assert n == by_seq[2][0] and same_keyframe(by_seq[2][1:], want)
    (rc, n, *want), _ = host_view(est, cfg, worlds[0], 0)              # (sequence 0 leaves the device for this look)
    assert n == by_seq[0][0] and same_keyframe(by_seq[0][1:], want)
    # a stride too small for some (all of them; only the longest): -(needed) for those, the others are filled
    counts = [by_seq[q][0] for q in (0, 1, 2)]
    for stride in (min(counts) - 1, max(counts) - 1):
        short = [q for q in (0, 1, 2) if by_seq[q][0] > stride]
        rc, part = est.keyframe_features(order, stride=stride)
        assert rc == abi.VIO_ECAP
        for q, r in zip(order, part):
            if q == 3:
                assert r[0] == -1
            elif q in short:
                assert r[0] == -by_seq[q][0] and same_keyframe(r[1:], [x[:stride] for x in by_seq[q][1:]])
            else:
                assert r[0] == by_seq[q][0] and same_keyframe(r[1:], by_seq[q][1:])
    est.close()


@pytest.mark.gpu
def test_chain_keyframe_features_connect_relocalization():
    """Plumbing of the three calls: the ids of keyframe_features label the window points of a synthetic keyframe pair in the
    loop detector, connect's kept_ids / kept_old_norm go to set_relocalization with that frame's header, and the next solved
    frame carries relocalization factors, at most one per kept match. Types and orders, not accuracy."""
    from test_loop_detector import VOC_SEED, vocabulary
    cfg = abi.default_config(window_size=10)
    W = cfg.window_size
    lp = RS.EstimatorLoop(cfg, seed=5, init_noise=1.0)
    lp.est.set_resident(True)
    for _ in range(60):
        r = lp.step()
        if r.action == abi.VIO_FRAME_SOLVED and r.marginalization_flag == abi.VIO_MARGIN_OLD and lp.k > W + 8:
            rc, (kf,) = lp.est.keyframe_features([0])
            if kf[0] >= 30:
                break
    n, ids, px, norm, cloud = kf
    assert rc == abi.VIO_OK and n >= 30 and lp.est.status().resident == 1
    w = lp.est.window()
    # the old keyframe: the cloud seen from a camera a little beside the one of window frame W - 2
    world = lp.world
    Rb, Pb = w["Rs"][W - 2], w["Ps"][W - 2] + w["Rs"][W - 2] @ np.array([0.25, 0.06, 0.02])
    Rc, tc = Rb @ world.ric, Pb + Rb @ world.tic
    Xc = (cloud - tc) @ Rc
    front = Xc[:, 2] > 0.2
    old_keys = np.where(front[:, None], np.stack([cfg.fx * Xc[:, 0] / Xc[:, 2] + cfg.cx, cfg.fy * Xc[:, 1] / Xc[:, 2] + cfg.cy], 1),
                        [[5.0, 5.0]]).astype(np.float32)
    rng = np.random.default_rng(3)
    desc = rng.integers(0, 2 ** 63, (n, 4), dtype=np.int64).astype(np.uint64)       # one random descriptor per landmark
    fast = (rng.uniform(0, 400, (9, 2)).astype(np.float32), rng.integers(0, 2 ** 63, (9, 4), dtype=np.int64).astype(np.uint64))
    voc = pkg.loop.BowVocabulary(vocabulary(VOC_SEED)[0])
    det = pkg.loop.LoopDetector(voc, pkg.loop.loop_detector_params(geom_check=3), n_sessions=1, max_entries=4, max_keypoints=1024)
    perm = rng.permutation(n)
    det.detect([0], [old_keys[perm]], [desc[perm]])
    det.detect([0], [np.concatenate([fast[0], px])], [np.concatenate([fast[1], desc])])
    c = det.connect(cfg, [0], [1], [0], [n], ids=[ids])[0]
    assert c["ransac_ran"] == 1 and c["n_kept"] > 22 and c["connected"] == 1
    assert np.array_equal(c["matched_old_pts"], old_keys)              # every window point found its own landmark
    assert np.array_equal(c["kept_ids"], ids[c["kept_index"]])
    o = np.argsort(c["kept_ids"])                                      # set_relocalization takes ascending ids
    q = synth.rot_to_quat(Rb)
    lp.est.set_relocalization(w["headers"][W - 2], Pb, q, c["kept_ids"][o], c["kept_old_norm"][o])
    for _ in range(4):
        r = lp.step()
        if r.action == abi.VIO_FRAME_SOLVED:
            break
    print("kept %d of %d, relocalization factors %d" % (c["n_kept"], n, r.n_loop_factors))
    assert r.action == abi.VIO_FRAME_SOLVED and 0 < r.n_loop_factors <= c["n_kept"]
    det.close(), voc.close(), lp.close()
