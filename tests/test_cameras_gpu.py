"""Per-sequence cameras on the device: a context whose sequences carry the made-up cameras A, B, C of camera_cases.py against
the same product in a homogeneous context created with that camera -- today's tested behaviour, so no tolerance is invented:
bit equality where the project demands it (front end, landmark store, descriptors and matching), the project's 1e-6 where window
solves share a launch (tests/test_estimator.py: the window kernel's LDS atomics make its sums not bit-reproducible)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import camera_cases as CC
import helpers as H
from helpers import abi, pkg, synth

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
import replay_synthetic as RS  # noqa: E402

pytestmark = pytest.mark.gpu
fe = pkg.frontend
NAMES = "ABC"
TOL, TOL_PRIOR = 1e-6, 1e-5      # tests/test_backend_gpu.py


# ---- 1. front end -------------------------------------------------------------------------------------------------------------
FE_KW = dict(max_corners=60, min_dist=12, image_rows=250, image_cols=333, freq=2)
FE_T = 6


@pytest.fixture(scope="module")
def fe_case():
    """Three streams and, per stream, what a one-sequence context whose cfg carries that stream's camera publishes and tracks."""
    base = abi.default_config(**FE_KW)
    cfgs = [CC.camera(n, base)[0] for n in NAMES]
    streams = [synth.make_image_stream(170 + s, FE_T, rows=FE_KW["image_rows"], cols=FE_KW["image_cols"])[0] for s in range(3)]
    want = []
    for s in range(3):
        one = fe.FeatureTracker(cfgs[s], n_seq=1)
        rec = []
        for f in range(FE_T):
            ids, xyz = one.read_images(streams[s][f][None], f % base.freq == 0)[0]
            rec.append((ids.copy(), xyz.copy(), one.state(0)))
        one.close()
        want.append(rec)
    return base, cfgs, streams, want


def _same_frame(got_obs, got_state, want, where):
    ids, xyz, state = want
    assert np.array_equal(got_obs[0], ids), where
    assert np.array_equal(got_obs[1], xyz), where
    for g, w in zip(got_state, state):
        assert np.array_equal(g, w), where


def test_frontend_mixed_cameras_equal_homogeneous_contexts(fe_case):
    base, cfgs, streams, want = fe_case
    cams = [CC.vio_camera(n, base) for n in NAMES]
    trk = fe.FeatureTracker(base, n_seq=3)
    for q in range(3):   # after create: cfg's intrinsics
        c = trk.get_camera(q)
        assert (c.fx, c.fy, c.cx, c.cy) == (base.fx, base.fy, base.cx, base.cy)
    order = [2, 0, 1]
    assert trk.set_cameras(order, [cams[q] for q in order]) == abi.VIO_OK
    for q in range(3):
        c = trk.get_camera(q)
        assert (c.fx, c.fy, c.cx, c.cy) == (cfgs[q].fx, cfgs[q].fy, cfgs[q].cx, cfgs[q].cy)
    n_pub = 0
    for f in range(FE_T):
        got = trk.read_images(np.stack([streams[s][f] for s in range(3)]), f % base.freq == 0)
        for s in range(3):
            _same_frame(got[s], trk.state(s), want[s][f], (f, s))
            n_pub += len(got[s][0])
    assert n_pub > 3 * 3 * FE_KW["max_corners"] // 4
    # the three sequences did publish different numbers for the same kind of pixels: the cameras are not interchangeable
    assert not np.array_equal(want[0][0][1][:5], want[1][0][1][:5])
    trk.close()


def test_frontend_subset_route_indexes_cameras_by_sequence(fe_case):
    base, cfgs, streams, want = fe_case
    cams = [CC.vio_camera(n, base) for n in NAMES]
    trk = fe.FeatureTracker(base, n_seq=3)
    assert trk.set_cameras([2, 0, 1], [cams[2], cams[0], cams[1]]) == abi.VIO_OK
    for f in range(FE_T):
        pub = f % base.freq == 0
        for seqs in ([2, 0], [1]):
            got = trk.read_subset(seqs, np.stack([streams[s][f] for s in seqs]), [pub] * len(seqs))
            for i, s in enumerate(seqs):
                _same_frame(got[i], trk.state(s), want[s][f], (f, s))
    # the camera survives vio_frontend_reset
    trk.reset([1])
    c = trk.get_camera(1)
    assert (c.fx, c.fy, c.cx, c.cy) == (cfgs[1].fx, cfgs[1].fy, cfgs[1].cx, cfgs[1].cy)
    got = trk.read_subset([1], streams[1][0][None], [True])
    _same_frame(got[0], trk.state(1), want[1][0], "after reset")
    trk.close()


def test_frontend_camera_set_between_two_steps_changes_only_what_is_published(fe_case):
    """The same pixels through three one-sequence trackers: camera A throughout, camera B throughout, and A with camera B set
    between frames 1 and 2. Every frame publishes."""
    base, cfgs, streams, _ = fe_case
    ta, tb, sw = fe.FeatureTracker(cfgs[0], n_seq=1), fe.FeatureTracker(cfgs[1], n_seq=1), fe.FeatureTracker(base, n_seq=1)
    for f in range(4):
        if f == 2:
            assert sw.set_cameras([0], [CC.vio_camera("B", base)]) == abi.VIO_OK
        (ids_a, xyz_a), (ids_b, xyz_b) = ta.read_images(streams[0][f][None], True)[0], tb.read_images(streams[0][f][None], True)[0]
        ids, xyz = sw.read_images(streams[0][f][None], True)[0]
        for g, wa, wb in zip(sw.state(0), ta.state(0), tb.state(0)):   # the tracker's pixel state never depends on the camera
            assert np.array_equal(g, wa) and np.array_equal(g, wb), f
        assert len(ids) > 10 and np.array_equal(ids, ids_a) and np.array_equal(ids, ids_b) and not np.array_equal(xyz_a, xyz_b)
        assert np.array_equal(xyz, xyz_a if f < 2 else xyz_b), f
    ta.close(), tb.close(), sw.close()


def test_frontend_set_cameras_refusals():
    base = abi.default_config(**FE_KW)
    trk = fe.FeatureTracker(base, n_seq=3)
    A, B = CC.vio_camera("A", base), CC.vio_camera("B", base)
    assert trk.set_cameras([0, 3], [A, B]) == abi.VIO_EINVAL and trk.set_cameras([-1], [A]) == abi.VIO_EINVAL
    assert trk.set_cameras([1, 1], [A, B]) == abi.VIO_EINVAL
    for field, value in (("fx", 0.0), ("fy", 0.0), ("fx", float("nan")), ("fy", float("inf"))):
        bad = CC.vio_camera("B", base)
        setattr(bad, field, value)
        assert trk.set_cameras([1, 2], [B, bad]) == abi.VIO_EINVAL
    for q in range(3):   # a refused call changed no camera
        assert trk.get_camera(q).fx == base.fx
    assert trk.lib.vio_frontend_get_camera(trk._h, 3, C.byref(abi.VioCamera())) == abi.VIO_EINVAL
    # between a submit and its collect
    frames = synth.make_image_stream(3, 1, rows=FE_KW["image_rows"], cols=FE_KW["image_cols"])[0]
    trk.submit(np.stack([frames[0]] * 3), True)
    assert trk.set_cameras([1], [B]) == abi.VIO_ESTATE
    trk.collect()
    assert trk.set_cameras([1], [B]) == abi.VIO_OK and trk.get_camera(1).fx == B.fx and trk.get_camera(0).fx == base.fx
    trk.close()


# ---- 2. window solves of different cameras in one launch ------------------------------------------------------------------------
WIN_NAMES = ["win_small_w4", "win_tiny_w4_f3", "win_c2_easy", "win_small_w4"]
WIN_CAMS = "ABCB"


def _as_golden(w, st):
    """An oracle-solved window in the form helpers.check_solution reads a golden fixture in."""
    d = dict(ref_raw_pose=w.raw_pose, ref_raw_speed_bias=w.raw_speed_bias, ref_raw_inv_depth=w.raw_inv_depth, ref_pose=w.pose,
             ref_speed_bias=w.speed_bias, ref_inv_depth=w.inv_depth, ref_loop_pose=w.loop_pose, ref_iterations=st["iterations"],
             ref_termination=st["termination"], ref_it_flags=st["it_flags"], ref_it_cost=st["it_cost"], ref_it_radius=st["it_radius"],
             ref_final_cost=st["final_cost"], ref_next_prior_n=np.int32(w.next_prior.n))
    if w.next_prior.n > 0:
        d.update(w.next_prior.to_npz_dict("ref_next_prior_"))
    return d


def test_window_solves_of_four_cameras_share_a_launch():
    loaded = [H.load_golden_window(n) for n in WIN_NAMES]
    cfg_be = loaded[2][0]   # the W = 10 fixture's configuration takes every window of the batch
    assert all(c.window_size <= cfg_be.window_size and c.fx == cfg_be.fx for c, _, _ in loaded)
    solver = pkg.backend.WindowSolver(cfg_be, max_batch=4)
    # NULL: vio_backend_solve_windows, on the goldens as today
    got = [w.copy() for _, w, _ in loaded]
    rc, stats = solver.solve_cam(got, None)
    assert rc == abi.VIO_OK
    for g, s, (_, _, d) in zip(got, stats, loaded):
        H.check_solution(g, s, d, tol=TOL, tol_prior=TOL_PRIOR)
    # one camera per window: sqrt_info in the parallel array, the extrinsic in the window
    osolve, _ = H.oracle_backend()
    ws, refs, si = [], [], []
    for (cfg, w, _), name in zip(loaded, WIN_CAMS):
        cam_cfg = CC.camera(name, cfg)[0]
        w = w.copy()
        w.ex_pose[:] = CC.ex_pose(name)
        refs.append(H.solve_with(osolve, cam_cfg, w))
        ws.append(w), si.append(cam_cfg.fx / 1.5)
    rc, stats = solver.solve_cam(ws, si)
    assert rc == abi.VIO_OK
    for g, s, (rw, rs) in zip(ws, stats, refs):
        H.check_solution(g, s, _as_golden(rw, rs), tol=TOL, tol_prior=TOL_PRIOR)
    # the cameras matter: window 0 and window 3 are the same fixture under A and B
    assert H.relerr(ws[0].pose, ws[3].pose) > 1e-5
    # an entry that is not finite and > 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert solver.solve_cam([w.copy() for _, w, _ in loaded], [si[0], bad, si[2], si[3]])[0] == abi.VIO_EINVAL
    assert solver.upload_cam([w.copy() for _, w, _ in loaded], si) == abi.VIO_OK
    solver.close()


def test_pnp_window_solves_of_two_cameras_share_a_launch():
    import test_pnp as TP
    cfg = abi.default_config()
    cases = TP.CASES[:2]
    ws = [TP.make_window(cfg, *c) for c in cases]
    solver = pkg.pnp.PnpSolver(cfg, max_batch=2)
    got = [w.copy() for w in ws]
    rc, stats = solver.solve_cam(got, None)     # NULL: vio_pnp_solve_windows, against the recorded reference as today
    assert rc == abi.VIO_OK
    for c, w, g, s in zip(cases, ws, got, stats):
        TP.check(g, s, *TP.reference(cfg, c[0], w))
    # cameras A and C: each window against solvers that take sqrt_info from the cfg they are called with, which carries that
    # window's camera -- the kernel's source run on the host (tests/emul/emul_pnp.cpp, held to the reference by tests/test_pnp.py),
    # the reference itself where it was built, and a homogeneous device context of that camera
    emul = H.build_emul_lib("emul_pnp.cpp", "libvio_emul_pnp.so", "VIO_EMUL")
    emul.emul_pnp_solve.argtypes = None
    cpu = [emul.emul_pnp_solve]
    ref_lib = H.ref_lib_or_none()
    if ref_lib is not None and hasattr(ref_lib, "ref_pnp_solve"):
        ref_lib.ref_pnp_solve.argtypes = None
        cpu.append(ref_lib.ref_pnp_solve)
    mixed, si, want = [], [], []
    for w, name in zip(ws, "AC"):
        cam_cfg = CC.camera(name, cfg)[0]
        w = w.copy()
        w.ex_pose = CC.ex_pose(name)
        refs = [pkg.pnp.solve_with(fn, cam_cfg, w) for fn in cpu]
        one = pkg.pnp.PnpSolver(cam_cfg, max_batch=1)
        ref = w.copy()
        refs.append((ref, one.solve([ref])[0]))
        one.close()
        want.append(refs), mixed.append(w), si.append(cam_cfg.fx / 1.5)
    rc, stats = solver.solve_cam(mixed, si)
    assert rc == abi.VIO_OK
    for g, s, refs in zip(mixed, stats, want):
        for ref, rs in refs:
            TP.check(g, s, ref, rs)
    assert H.pose_relerr(mixed[1].pose, got[1].pose) > 1e-7     # camera C is not the context's camera
    assert solver.solve_cam([w.copy() for w in ws], [si[0], 0.0])[0] == abi.VIO_EINVAL
    solver.close()


# ---- 3. / 5. estimator, one launch ------------------------------------------------------------------------------------------
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


EST_W, EST_STEPS, EST_START = 6, 24, [0, 3, 5]


def _world(q, cfg_q, seed0=20):
    return RS.SyntheticWorld(cfg_q, seed0 + q, ex=CC.ex_pose(NAMES[q]))


def _single(q, base, self_init=False, init_device=0, resident=None, seed0=20):
    cfg_q = CC.camera(NAMES[q], base)[0]
    s = RS.EstimatorLoop(cfg_q, seed=seed0 + q, init_noise=0.0 if self_init else 1.0, world=_world(q, cfg_q, seed0), self_init=self_init)
    if self_init:
        s.est.set_init_device(init_device)
    if resident is not None:
        s.est.set_resident(resident)
    acts, first = [], None
    for _ in range(EST_STEPS):
        r = s.step()
        acts.append(r.action)
        if first is None and r.action == abi.VIO_FRAME_SOLVED:
            first = {k: np.array(v, copy=True) for k, v in s.est.window().items()}
    return s, acts, first


def _mixed(base, resident, self_init=False, init_device=0, seed0=20):
    """Three sequences with cameras A, B, C in one estimator created with camera A, started EST_START calls apart.
    -> (estimator, newest positions per solved frame, iteration counts, actions, first solved windows)"""
    cfgs = [CC.camera(n, base)[0] for n in NAMES]
    worlds = [_world(q, cfgs[q], seed0) for q in range(3)]
    _, ticA, ricA = CC.camera("A", base)
    est = pkg.estimator.Estimator(base, ticA, ricA, n_seq=3)
    est.set_resident(resident)
    if self_init:
        est.enable_initialization(2)
        est.set_init_device(init_device)
    for q in (2, 1):   # (sequence 0 keeps the context's camera without a call)
        assert est.set_camera(CC.vio_camera(NAMES[q], base), seq=q) == abi.VIO_OK
    feeders = [RS.EstimatorLoop(cfgs[q], seed=seed0 + q, init_noise=0.0 if self_init else 1.0, world=worlds[q], self_init=self_init)
               for q in range(3)]
    for q, f in enumerate(feeders):
        f.est.close()
        f.est = _SeqView(est, q)
    got, iters, acts, first = [[] for _ in range(3)], [[] for _ in range(3)], [[] for _ in range(3)], [None] * 3
    for call in range(EST_STEPS + max(EST_START)):
        obs, hdr, act = [], [], []
        for q in range(3):
            k = call - EST_START[q]
            if k < 0 or k >= EST_STEPS:
                obs.append(([], [])), hdr.append(0.0), act.append(0)
                continue
            obs.append(feeders[q].feed_until_image()), hdr.append(worlds[q].time(k)), act.append(1)
        res = est.process_images(obs, hdr, act)
        for q in range(3):
            if not act[q]:
                continue
            acts[q].append(res[q].action)
            if res[q].action == abi.VIO_FRAME_SOLVED:
                got[q].append(est.window(q)["Ps"][EST_W].copy()), iters[q].append(res[q].stats.iterations)
                if first[q] is None:
                    first[q] = {k: np.array(v, copy=True) for k, v in est.window(q).items()}
    return est, got, iters, acts, first, worlds


@pytest.fixture(scope="module")
def est_case():
    base = abi.default_config(window_size=EST_W)
    singles = [_single(q, base) for q in range(3)]
    mixed = {r: _mixed(base, r) for r in (1, 0)}
    yield base, singles, mixed
    for s, _, _ in singles:
        s.close()
    for m in mixed.values():
        m[0].close()


@pytest.mark.parametrize("resident", [1, 0])
def test_estimator_sequences_with_their_own_cameras_equal_single_estimators(est_case, resident):
    base, singles, mixed = est_case
    est, got, iters, acts, _, _ = mixed[resident]
    for q in range(3):
        s, sacts, _ = singles[q]
        want = np.array([h[1] for h in s.history])
        assert acts[q] == sacts
        assert len(want) > 10 and len(got[q]) == len(want)
        diff = float(np.abs(np.array(got[q]) - want).max())
        print("resident %d, sequence %d (camera %s): newest positions differ by %.3g" % (resident, q, NAMES[q], diff))
        assert diff < 1e-6
        assert iters[q] == [h[3].stats.iterations for h in s.history]
        assert est.status(q).resident == resident
        assert CC.same_camera(est.get_camera(q), CC.vio_camera(NAMES[q], base))
    # a sequence that holds a window refuses a camera
    assert est.set_camera(CC.vio_camera("A", base), seq=1) == abi.VIO_ESTATE
    # the worlds are different enough for a wrong camera to show: the single estimators do not agree with each other
    assert np.abs(np.array(singles[0][0].history[-1][1]) - np.array(singles[1][0].history[-1][1])).max() > 1e-3


@pytest.mark.parametrize("init_device", [0, 2])
def test_estimator_start_up_reads_the_sequence_extrinsic(init_device):
    """The start-up (solveInitial: gyroscope hint, alignment with tic, re-triangulation) of three sequences with their own
    cameras in one estimator: the actions of every frame and the first solved window are the single estimators'."""
    base = abi.default_config(window_size=EST_W)
    singles = [_single(q, base, self_init=True, init_device=init_device) for q in range(3)]
    est, _, _, acts, first, _ = _mixed(base, 1, self_init=True, init_device=init_device)
    solved = 0
    for q in range(3):
        s, sacts, sfirst = singles[q]
        assert acts[q] == sacts, q
        assert (first[q] is None) == (sfirst is None)
        if sfirst is not None:
            solved += 1
            for k in ("Ps", "Rs", "Vs", "Bas", "Bgs"):
                d = float(np.abs(first[q][k] - sfirst[k]).max())
                assert d < 1e-6, (q, k, d)
    print("init_device %d: %d of 3 sequences initialised within %d frames" % (init_device, solved, EST_STEPS))
    assert solved == 3   # every sequence's start-up ran to its first solved window: the comparison above is not an empty one
    est.close()
    for s, _, _ in singles:
        s.close()


def test_keyframe_features_take_the_sequence_camera(est_case):
    base, singles, mixed = est_case
    res_est, host_est = mixed[1][0], mixed[0][0]
    assert [res_est.status(q).resident for q in range(3)] == [1, 1, 1] and [host_est.status(q).resident for q in range(3)] == [0, 0, 0]
    order = [1, 2, 0]
    rc, on_dev = res_est.keyframe_features(order, stride=512)
    rc2, on_host = host_est.keyframe_features(order, stride=512)
    assert rc == rc2 == abi.VIO_OK
    assert [res_est.status(q).resident for q in range(3)] == [1, 1, 1]     # served on the device, nobody moved
    for q, d, h in zip(order, on_dev, on_host):
        cfg_q = CC.camera(NAMES[q], base)[0]
        # against the set_resident(0) twin: ids, px and norm come from the observations alone, which both estimators were fed
        # bit for bit; cloud is made of the solved states and depths, which agree between two estimators to the solver's 1e-6 (LDS
        # atomics), so that one is bit for bit only against the host-side list of the SAME estimator, further down
        assert d[0] == h[0] > 2 and np.array_equal(d[1], h[1])
        for a, b in zip(d[2:4], h[2:4]):
            assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint8), b.view(np.uint8)), q
        assert H.relerr(d[4], h[4]) < 1e-6, q
        ids, px, norm, cloud = d[1:]
        want_px = np.stack([cfg_q.fx * norm[:, 0].astype(np.float64) + cfg_q.cx, cfg_q.fy * norm[:, 1].astype(np.float64) + cfg_q.cy], 1)
        # px and norm are float32 roundings of the same double point: a few 1e-5 px apart at these magnitudes; the cameras
        # are 4 px and more apart
        print("sequence %d: px against fx * norm + cx in numpy, largest difference %.3g px" % (q, np.abs(px - want_px).max()))
        assert np.abs(px - want_px).max() < 1e-3, q
        if q != 0:
            wrong = np.stack([base.fx * norm[:, 0].astype(np.float64) + base.cx, base.fy * norm[:, 1].astype(np.float64) + base.cy], 1)
            assert np.abs(px - wrong).max() > 1.0
    # bit for bit: the resident pass against the host-side list of the same estimator (the list comes back for the look)
    for q in order:
        rc, (dev,) = res_est.keyframe_features([q], stride=512)
        res_est.features(q)                                                   # demotes the sequence
        assert res_est.status(q).resident == 0
        rc2, (hst,) = res_est.keyframe_features([q], stride=512)
        assert rc == rc2 == abi.VIO_OK and dev[0] == hst[0] > 2
        for a, b in zip(dev[1:], hst[1:]):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), q


# ---- 4. estimator, two back-end groups ------------------------------------------------------------------------------------------
def _record(cfg_q, name, seed, W, steps):
    """One replay recorded once: per frame the IMU samples, image_msg, the header; the initial window at frame W."""
    world = RS.SyntheticWorld(cfg_q, seed, ex=CC.ex_pose(name))
    rng = np.random.default_rng(seed + 99)
    frames, init = [], []
    for k in range(steps):
        imu = [world.imu(world.time(0))] if k == 0 else world.imu_interval(k)
        if k <= W:
            Pt, Rt, Vt = world.truth(k)
            init.append((world.time(k), Pt + rng.normal(0, 0.01, 3), Rt @ synth.rotvec_to_rot(rng.normal(0, 0.005, 3)), Vt + rng.normal(0, 0.02, 3)))
        frames.append((imu, world.observe(k), world.time(k)))
    return world, frames, init


def _feed(est, seqs_of, records, W, steps, watch):
    """Feeds record r to the sequences seqs_of[r]; -> per watched sequence the newest positions and iteration counts."""
    n_seq = est.n_seq
    rec_of = {q: r for r, qs in enumerate(seqs_of) for q in qs}
    out = {q: ([], []) for q in watch}
    for k in range(steps):
        per = max(len(records[r][1][k][0]) for r in range(len(records)))
        dt, acc, gyr, ns = np.zeros((n_seq, per)), np.zeros((n_seq, per, 3)), np.zeros((n_seq, per, 3)), np.zeros(n_seq, np.int32)
        for q in range(n_seq):
            world, frames, _ = records[rec_of[q]]
            imu = frames[k][0]
            ns[q], dt[q, :len(imu)] = len(imu), world.dt
            acc[q, :len(imu)], gyr[q, :len(imu)] = [s[0] for s in imu], [s[1] for s in imu]
        est.process_imu_batch(ns, dt, acc, gyr)
        if k == W:
            for q in range(n_seq):
                world, _, init = records[rec_of[q]]
                est.set_initial_state([i[0] for i in init], [i[1] for i in init], [i[2] for i in init], [i[3] for i in init],
                                      [world.ba] * (W + 1), [world.bg] * (W + 1), seq=q)
        res = est.process_images([records[rec_of[q]][1][k][1] for q in range(n_seq)], [records[rec_of[q]][1][k][2] for q in range(n_seq)])
        for q in watch:
            if res[q].action == abi.VIO_FRAME_SOLVED:
                out[q][0].append(est.window(q)["Ps"][W].copy()), out[q][1].append(res[q].stats.iterations)
    return out


def test_estimator_cameras_across_two_backend_groups():
    """64 sequences on the host-side lists form two back-end groups of 32: camera B on sequences 3 and 40, A elsewhere. Sequence
    40 is window 8 of the second group's launch: an index by window in place of by sequence gives it sequence 8's camera."""
    W, steps, n_seq = 4, 12, 64
    base = abi.default_config(window_size=W)
    cfgB = CC.camera("B", base)[0]
    records = [_record(base, "A", 61, W, steps), _record(cfgB, "B", 62, W, steps)]
    on_b = [3, 40]
    want = []
    for r, (cfg_r, name) in enumerate(((base, "A"), (cfgB, "B"))):
        _, tic, ric = CC.camera(name, base)
        one = pkg.estimator.Estimator(cfg_r, tic, ric, n_seq=1)
        one.set_resident(0)
        want.append(_feed(one, [[0]] if r == 0 else [[], [0]], records, W, steps, [0])[0])
        one.close()
    _, ticA, ricA = CC.camera("A", base)
    est = pkg.estimator.Estimator(base, ticA, ricA, n_seq=n_seq)
    est.set_resident(0)
    for q in on_b:
        assert est.set_camera(CC.vio_camera("B", base), seq=q) == abi.VIO_OK
    watch = [3, 35, 40, 8]
    got = _feed(est, [[q for q in range(n_seq) if q not in on_b], on_b], records, W, steps, watch)
    for q in watch:
        ps, it = want[1 if q in on_b else 0]
        assert len(ps) >= steps - W - 1 and len(got[q][0]) == len(ps)
        diff = float(np.abs(np.array(got[q][0]) - np.array(ps)).max())
        print("sequence %d: newest positions differ by %.3g" % (q, diff))
        assert diff < 1e-6, q
        assert got[q][1] == it, q
    assert np.abs(np.array(want[0][0][-1]) - np.array(want[1][0][-1])).max() > 1e-3    # the two replays are not one
    est.close()


# ---- 6. loop connect ------------------------------------------------------------------------------------------------------------
def test_loop_connect_normalises_with_the_session_camera():
    import loop_keyframe_cases as KC
    import test_loop_keyframes as TLK
    rig = TLK.Rig(KC.SHAPES[1])
    try:
        base = rig.cfg
        cfgs = {n: CC.camera(n, base)[0] for n in "AB"}
        of_session = {0: "A", 2: "B"}   # session 1 has no camera: it uses the cfg of the call

        def run(det, cfg):
            rig.cfg = cfg
            try:
                return [rig.three_calls(det, call) for call in rig.calls]
            finally:
                rig.cfg = base

        today = run(rig.detector(), base)                     # no set_cameras: today's outputs
        homog = {n: run(rig.detector(), cfgs[n]) for n in "AB"}
        mixed_det = rig.detector()
        assert mixed_det.get_camera(0)[0] == abi.VIO_ESTATE
        assert mixed_det.set_cameras([2, 0], [CC.vio_camera("B", base), CC.vio_camera("A", base)]) == abi.VIO_OK
        assert mixed_det.get_camera(2)[1].fx == cfgs["B"].fx and mixed_det.get_camera(1)[0] == abi.VIO_ESTATE
        # the call's cfg is camera C's: no session with a camera may use it
        cfgC = CC.camera("C", base)[0]
        mixed = run(mixed_det, cfgC)
        withC = run(rig.detector(), cfgC)
        ran = {0: 0, 1: 0, 2: 0}
        for call, got, *refs in zip(rig.calls, mixed, today, homog["A"], homog["B"], withC):
            by = dict(zip(("today", "A", "B", "C"), refs))
            for i, (s, _) in enumerate(call):
                want = by[of_session.get(s, "C")][i]
                TLK.same_keyframe(got[i], want, ("mixed", s))
                c = got[i]["connection"]
                if c is not None and c["ransac_ran"]:
                    ran[s] += 1
                    # today's float arithmetic: (pt - (cx, cy)) / (fx, fy) in float, widened
                    cf = cfgs[of_session[s]] if s in of_session else cfgC
                    p = c["matched_old_pts"][c["kept_index"]]
                    norm = np.stack([(p[:, 0] - np.float32(cf.cx)) / np.float32(cf.fx), (p[:, 1] - np.float32(cf.cy)) / np.float32(cf.fy)], 1)
                    assert norm.dtype == np.float32 and np.array_equal(c["kept_old_norm"], norm.astype(np.float64))
                    if s in of_session:
                        assert not np.array_equal(c["kept_old_norm"], by["C"][i]["connection"]["kept_old_norm"])
        assert ran[0] >= 1 and ran[2] >= 1, ran
        # refusals
        A = CC.vio_camera("A", base)
        assert mixed_det.set_cameras([0, 0], [A, A]) == abi.VIO_EINVAL and mixed_det.set_cameras([3], [A]) == abi.VIO_EINVAL
        bad = CC.vio_camera("A", base)
        bad.fx = 0.0
        assert mixed_det.set_cameras([1], [bad]) == abi.VIO_EINVAL and mixed_det.get_camera(1)[0] == abi.VIO_ESTATE
    finally:
        rig.close()


# ---- 7. PnP tracker -------------------------------------------------------------------------------------------------------------
def test_pnp_tracker_sequences_with_their_own_cameras():
    """The scenario of tests/test_pnp.py::test_pnp_tracker_for_three_sequences_is_three_trackers_for_one with two sequences,
    cameras A and C, and its bound between copies inside one batch (1e-9)."""
    import test_pnp as TP
    base = abi.default_config()
    names = "AC"
    scs = []
    for q, n in enumerate(names):
        cfg_q, tic, ric = CC.camera(n, base)
        sc = TP._Scene(cfg_q, 4 + q)
        sc.tic, sc.ric = tic, ric     # the scene's camera: features() and the trackers below read these
        scs.append(sc)
    _, ticA, ricA = CC.camera("A", base)
    one = pkg.pnp.PnpTracker(base, ticA, ricA, n_seq=2, pnp_size=6)
    assert one.set_camera(CC.vio_camera("C", base), seq=1) == abi.VIO_OK
    each = [pkg.pnp.PnpTracker(sc.cfg, sc.tic, sc.ric, n_seq=1, pnp_size=6) for sc in scs]
    n_solved, worst = np.zeros(2, int), 0.0
    for k in range(12):
        for q, sc in enumerate(scs):
            for dt, a, w in ([(0.0,) + sc.imu(sc.t(0))] if k == 0 else sc.imu_interval(k)):
                one.process_imu(dt, a, w, seq=q), each[q].process_imu(dt, a, w)
            if k >= 2 and (k + q) % 3 == 2:
                j = k - 2
                init = (sc.t(j), sc.ba, sc.bg, sc.traj.pos(sc.t(j)) + sc.rng.normal(0, 0.005, 3), sc.traj.rot(sc.t(j)),
                        sc.traj.vel(sc.t(j)) + sc.rng.normal(0, 0.01, 3))
                one.set_init(*init, seq=q), each[q].set_init(*init)
        feats = [sc.features(k, n=80 + 20 * q) for q, sc in enumerate(scs)]
        hdrs = [sc.t(k) for sc in scs]
        P, R, solved = one.process_images(feats, hdrs, use_pnp=True)
        for q in range(2):
            Pq, Rq, sq = each[q].process_images([feats[q]], [hdrs[q]], use_pnp=True)
            assert solved[q] == sq[0] == (1 if k >= 6 else 0)
            worst = max(worst, np.abs(P[q] - Pq[0]).max(), np.abs(R[q] - Rq[0]).max())
        n_solved += solved
    print("two cameras in one tracker against one tracker each: largest difference %.2e" % worst)
    assert list(n_solved) == [6, 6] and worst < 1e-9
    for q in range(2):
        a, b = one.window(seq=q), each[q].window()
        assert max(np.abs(a[key] - b[key]).max() for key in ("Ps", "Rs", "Vs")) < 1e-9
    assert one.set_camera(CC.vio_camera("A", base), seq=1) == abi.VIO_ESTATE
    one.close()
    for t in each:
        t.close()
