"""The motion-only window of the front-end (vinsPnP::solve_ceres, VINS_ios/vins_pnp.cpp:264-341).

Checker: the REAL reference factor classes (IMUFactorPnP, PerspectiveFactor) under the vendored Ceres, assembled exactly
as vins_pnp.cpp does (oracle/ref_harness.cpp::ref_pnp_solve; vins_pnp.cpp itself needs an OpenCV header) — live where
oracle/_ref exists, else through tests/golden/pnp_windows.npz. CPU: the kernel's source compiled for the host
(tests/emul/emul_pnp.cpp, -DVIO_EMUL). GPU: the HIP kernel through the C ABI.

CASES take only accepted steps. EDGE_CASES add what the trust-region loop does otherwise -- rejected steps (the radius
halved and the cached Gauss-Newton / Cauchy pair reused, up to three times in a row; a solve whose last iteration is a
rejection returns the last accepted iterate), an exit through the parameter tolerance before the iteration limit -- and
the ends of the shape range: 2 and 8 frames, 9 to 72 unknowns, no factor to over 3000, frames without a feature.
Not covered: the invalid-step exit (HandleInvalidStep, termination 2, flags 0). None of the windows tried, which the
reference itself reproduces to 1e-8 under a 1e-13 change of its inputs, reaches it, and non-finite inputs are not
constructed to force it. Neither is a solve that meets the function tolerance exactly at its threshold (a solved window
solved a third time): the reference's own route depends on the last bits there."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
from helpers import abi, pkg, synth

GOLDEN = os.path.join(H.ROOT, "tests", "golden", "pnp_windows.npz")
TOL = 1e-6

# (seed, frames, features per frame, fixed frames, perturbation scale)
CASES = [(1, 7, 60, (0,), 1.0), (2, 7, 150, (0,), 3.0), (3, 7, 25, (0, 1), 1.0), (4, 5, 80, (), 1.0), (5, 7, 8, (2,), 6.0),
         (6, 7, 100, (0, 1, 2, 3, 4, 5, 6), 1.0), (7, 3, 40, (0,), 10.0)]


def make_window(cfg, seed, n, feats, fixed, perturb):
    rng = np.random.default_rng(seed)
    traj = synth.Trajectory(rng)
    t0 = rng.uniform(0, 20)
    ex = synth.ex_pose_default()
    ric, tic = synth.quat_to_rot(ex[3:]), ex[:3]
    g = np.array([0, 0, cfg.gravity])
    ba, bg = rng.normal(0, 0.02, 3), rng.normal(0, 0.002, 3)
    fdt, per = 1.0 / 30, 4
    dt = fdt / per

    def imu(t):
        R = traj.rot(t)
        return R.T @ (traj.acc(t) + g) + ba + rng.normal(0, 0.02, 3), traj.omega_body(t) + bg + rng.normal(0, 0.002, 3)

    pose, speed, pre = [], [], []
    last = imu(t0)
    for k in range(n):
        t = t0 + k * fdt
        P, R, V = traj.pos(t), traj.rot(t), traj.vel(t)
        if k in fixed:
            Pn, Rn, Vn = P, R, V
        else:
            Pn = P + rng.normal(0, 0.004 * perturb, 3)
            Rn = R @ synth.rotvec_to_rot(rng.normal(0, 0.003 * perturb, 3))
            Vn = V + rng.normal(0, 0.02 * perturb, 3)
        pose.append(np.concatenate([Pn, synth.rot_to_quat(Rn)])), speed.append(Vn)
        if k > 0:
            samples = [imu(t - fdt + (s + 1) * dt) for s in range(per)]
            pre.append(pkg.backend.preintegrate(cfg, last[0], last[1], ba, bg, np.full(per, dt), np.array([s[0] for s in samples]),
                                                np.array([s[1] for s in samples])))
            last = samples[-1]
    # landmarks in front of the middle camera, "solved" by the back-end to within a centimetre or two
    tm = t0 + (n // 2) * fdt
    Rm, Pm = traj.rot(tm) @ ric, traj.pos(tm) + traj.rot(tm) @ tic
    z = rng.uniform(3, 10, feats)
    Xw = np.column_stack([rng.uniform(-0.4, 0.4, feats) * z, rng.uniform(-0.5, 0.5, feats) * z, z]) @ Rm.T + Pm
    track = rng.integers(2, 40, feats)
    start, obs, pos, tn = [0], [], [], []
    for k in range(n):
        t = t0 + k * fdt
        Rc, Pc = traj.rot(t) @ ric, traj.pos(t) + traj.rot(t) @ tic
        for j in range(feats):
            if rng.random() < 0.1:
                continue
            c = Rc.T @ (Xw[j] - Pc)
            obs.append(c[:2] / c[2] + rng.normal(0, 0.7 / cfg.fx, 2))
            pos.append(Xw[j] + rng.normal(0, 0.01, 3))
            tn.append(track[j])
        start.append(len(obs))
    fx = np.zeros(n, np.uint8)
    fx[list(fixed)] = 1
    return pkg.pnp.PnpWindow(np.array(pose), np.array(speed), np.tile(np.concatenate([ba, bg]), (n, 1)), fx, ex, np.array(pre), start,
                             np.array(obs), np.array(pos), np.array(tn))


# ---------------------------------------------------------------------------------------------------------------------
# edge windows: make_window plus small edits. name -> builder(cfg)
def hard_start(cfg, seed, n, fixed, feats=40):
    """A start the first Gauss-Newton steps overshoot from: every free frame's rotation turned by about a radian."""
    w = make_window(cfg, seed, n, feats, fixed, 3.0)
    rng = np.random.default_rng(1000 + seed)
    for k in range(n):
        if k not in fixed:
            R = synth.quat_to_rot(w.pose[k, 3:]) @ synth.rotvec_to_rot(rng.normal(0, 1.0, 3))
            w.pose[k, 3:] = synth.rot_to_quat(R)
    return w


def with_features(w, keep):
    """The window with only the factors keep(frame, index within the frame) selects."""
    idx = [m for k in range(w.n) for j, m in enumerate(range(w.feat_start[k], w.feat_start[k + 1])) if keep(k, j)]
    start = [0] + [sum(1 for m in idx if m < w.feat_start[k + 1]) for k in range(w.n)]
    return pkg.pnp.PnpWindow(w.pose, w.speed, w.bias, w.fixed, w.ex_pose, w.preint, start, w.observation[idx], w.position[idx],
                             w.track_num[idx])


def with_tracks(w):
    w.track_num[0::7], w.track_num[3::7] = 0, 300   # weight 0 (a factor without effect) and thirty times the usual
    return w


EDGE_CASES = {
    # rejected steps (flags 1): two and three in a row, a last iteration that is one, seven and eight frames
    "rej_s40": lambda cfg: hard_start(cfg, 40, 4, (0,)),
    "rej_s44": lambda cfg: hard_start(cfg, 44, 4, (0,)),
    "rej_s51_n7": lambda cfg: hard_start(cfg, 51, 7, (0,)),
    "rej_s46_n7": lambda cfg: hard_start(cfg, 46, 7, (0,)),
    "rej_s40_n8": lambda cfg: hard_start(cfg, 40, 8, (0,)),
    # IMU factors only: converges before the iteration limit
    "imu_only": lambda cfg: with_features(make_window(cfg, 60, 7, 30, (0,), 1.0), lambda k, j: False),
    # shapes
    "n8_free": lambda cfg: make_window(cfg, 61, 8, 40, (), 1.0),
    "n8_fixed34": lambda cfg: make_window(cfg, 62, 8, 30, (3, 4), 2.0),
    "n7_free": lambda cfg: make_window(cfg, 63, 7, 50, (), 1.0),
    "n2_fixed0": lambda cfg: make_window(cfg, 64, 2, 25, (0,), 2.0),
    "n2_free": lambda cfg: make_window(cfg, 65, 2, 20, (), 1.0),
    "fixed0246": lambda cfg: make_window(cfg, 66, 7, 35, (0, 2, 4, 6), 2.0),
    "fixed_last": lambda cfg: make_window(cfg, 67, 7, 45, (6,), 1.0),
    "empty_middle": lambda cfg: with_features(make_window(cfg, 68, 7, 30, (0,), 1.0), lambda k, j: k != 3),
    "empty_ends": lambda cfg: with_features(make_window(cfg, 69, 6, 40, (1,), 1.0), lambda k, j: 0 < k < 5),
    "last_only": lambda cfg: with_features(make_window(cfg, 70, 7, 60, (0,), 1.0), lambda k, j: k == 6),
    "one_each": lambda cfg: with_features(make_window(cfg, 71, 7, 20, (0,), 1.0), lambda k, j: j == 0),
    "tracks_0_300": lambda cfg: with_tracks(make_window(cfg, 72, 7, 40, (0,), 1.0)),
    "large_m": lambda cfg: make_window(cfg, 73, 8, 450, (0,), 1.0),
}
REJECTED = [k for k in EDGE_CASES if k.startswith("rej_")]
STAT_KEYS = ("initial_cost", "final_cost", "iterations", "it_cost", "it_flags")
EDGE_STAT_KEYS = STAT_KEYS + ("termination", "num_successful_steps", "num_unsuccessful_steps", "it_radius", "it_step_norm")


def reference(cfg, seed, w):
    """seed: the seed of a CASES row, or the name of an edge window."""
    lib = H.ref_lib_or_none()
    if lib is not None and hasattr(lib, "ref_pnp_solve"):
        lib.ref_pnp_solve.argtypes = None
        return pkg.pnp.solve_with(lib.ref_pnp_solve, cfg, w)
    d = np.load(GOLDEN)
    pre = "e_%s_" % seed if isinstance(seed, str) else "c%d_" % seed
    out = w.copy()
    out.pose, out.speed = d[pre + "pose"], d[pre + "speed"]
    st = {k: d[pre + k] for k in EDGE_STAT_KEYS if pre + k in d.files}
    return out, st


def check(got, gs, ref, rs, tol=TOL):
    assert gs["iterations"] == int(rs["iterations"]) and list(gs["it_flags"]) == list(rs["it_flags"])
    assert H.relerr(np.array(gs["it_cost"]), np.array(rs["it_cost"])) < 1e-6
    assert abs(gs["initial_cost"] - float(rs["initial_cost"])) <= 1e-9 * float(rs["initial_cost"])
    assert H.pose_relerr(got.pose, ref.pose) < tol and H.relerr(got.speed, ref.speed) < tol


def check_route(got, gs, ref, rs, tol=TOL):
    """check() plus the way there: how the solve ended, its step counts, the trust-region radius and the step norm of
    every iteration, and the final cost on the scale of the initial one (the IMU-only window ends at 1e-21)."""
    check(got, gs, ref, rs, tol)
    assert gs["termination"] == int(rs["termination"])
    assert gs["num_successful_steps"] == int(rs["num_successful_steps"])
    assert gs["num_unsuccessful_steps"] == int(rs["num_unsuccessful_steps"])
    assert H.relerr(gs["it_radius"], rs["it_radius"]) < tol and H.relerr(gs["it_step_norm"], rs["it_step_norm"]) < tol
    assert abs(gs["final_cost"] - float(rs["final_cost"])) <= 1e-9 * float(rs["initial_cost"])


def pnp_unknowns(w):
    return 9 * int((w.fixed == 0).sum())


def edge_windows(cfg):
    return {name: build(cfg) for name, build in EDGE_CASES.items()}


@pytest.fixture(scope="module")
def emul():
    lib = H.build_emul_lib("emul_pnp.cpp", "libvio_emul_pnp.so", "VIO_EMUL")
    lib.emul_pnp_solve.argtypes = None
    return lib


@pytest.mark.parametrize("seed,n,feats,fixed,perturb", CASES)
def test_kernel_source_on_host_matches_the_reference(seed, n, feats, fixed, perturb, emul):
    cfg = abi.default_config()
    w = make_window(cfg, seed, n, feats, fixed, perturb)
    ref, rs = reference(cfg, seed, w)
    got, gs = pkg.pnp.solve_with(emul.emul_pnp_solve, cfg, w)
    check_route(got, gs, ref, rs)
    if len(fixed) < n:
        assert rs["final_cost"] < rs["initial_cost"]
    for k in fixed:   # constant blocks come back untouched (up to the quaternion round trip)
        assert np.abs(got.pose[k] - w.pose[k]).max() < 1e-12 and np.array_equal(got.speed[k], w.speed[k])


@pytest.fixture(scope="module")
def edges():
    """The edge windows with the reference's result for each, computed once: name -> (window, solved window, stats).
    Tests copy what they solve."""
    cfg = abi.default_config()
    return {name: (w,) + reference(cfg, name, w) for name, w in edge_windows(cfg).items()}


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_kernel_source_on_host_matches_the_reference_on_the_edge_windows(name, emul, edges):
    w, ref, rs = edges[name]
    got, gs = pkg.pnp.solve_with(emul.emul_pnp_solve, abi.default_config(), w)
    check_route(got, gs, ref, rs)
    for k in np.flatnonzero(w.fixed):
        assert np.abs(got.pose[k] - w.pose[k]).max() < 1e-12 and np.array_equal(got.speed[k], w.speed[k])


def test_the_recorded_edge_windows_cover_rejection_early_exit_and_the_shape_limits():
    """On the fixture alone (the shapes from the regenerated inputs): the table must not lose its edges when a window
    is replaced."""
    d = np.load(GOLDEN)
    ws = edge_windows(abi.default_config())
    assert {k[2:-5] for k in d.files if k.startswith("e_") and k.endswith("_pose")} == set(ws)
    flags = {name: "".join(str(int(f)) for f in d["e_%s_it_flags" % name]) for name in ws}
    for name, w in ws.items():
        assert d["e_%s_pose" % name].shape == (w.n, 7) and len(flags[name]) == int(d["e_%s_iterations" % name])
        assert int(d["e_%s_num_unsuccessful_steps" % name]) == flags[name].count("1")
        assert int(d["e_%s_termination" % name]) != 2 and "0" not in flags[name] and "2" not in flags[name]   # (module docstring)
    assert sum("1" in f for f in flags.values()) >= 4
    assert all("1" in flags[name] for name in REJECTED)
    assert any("11" in f for f in flags.values())                      # the cached Gauss-Newton / Cauchy pair is reused
    assert any(f.endswith("1") for f in flags.values())                # the result is the last ACCEPTED iterate
    assert any("1" in flags[name] and ws[name].n >= 7 for name in ws)
    assert any(int(d["e_%s_termination" % name]) == 1 and 0 < len(flags[name]) < 6 for name in ws)
    unknowns = {name: pnp_unknowns(w) for name, w in ws.items()}
    assert max(unknowns.values()) == 72 and 63 in unknowns.values() and 9 in unknowns.values()
    factors = [int(w.feat_start[-1]) for w in ws.values()]
    assert min(factors) == 0 and max(factors) > 3000


def test_the_edge_windows_are_well_conditioned_in_the_reference():
    """A condition on the inputs, not on the code under test: the reference, given observations, landmark positions and
    speeds changed by a relative 1e-13, must take the same route and land within 1e-8 (100 x under TOL) of its own
    result. A window that does not is no test case (the hard start with no frame fixed moves by 2e-6) and is replaced.
    Measured: at most 4e-11 on the rejected-step windows, 3e-11 on the others."""
    lib = H.ref_lib_or_none()
    if lib is None or not hasattr(lib, "ref_pnp_solve"):
        pytest.skip("oracle/_ref not built here (needs /root/reference)")
    lib.ref_pnp_solve.argtypes = None
    cfg = abi.default_config()
    for name, w in edge_windows(cfg).items():
        ref, rs = pkg.pnp.solve_with(lib.ref_pnp_solve, cfg, w)
        rng = np.random.default_rng(7)
        for _ in range(3):
            p = w.copy()
            for a in (p.observation, p.position, p.speed):
                a *= 1 + rng.uniform(-1e-13, 1e-13, a.shape)
            out, st = pkg.pnp.solve_with(lib.ref_pnp_solve, cfg, p)
            moved = max(H.pose_relerr(out.pose, ref.pose), H.relerr(out.speed, ref.speed))
            print("%s: %s moved %.1e" % (name, list(st["it_flags"]), moved))
            assert list(st["it_flags"]) == list(rs["it_flags"]) and st["termination"] == rs["termination"], name
            assert moved <= 1e-8, (name, moved)


@pytest.mark.gpu
def test_device_kernel_matches_the_reference_in_one_ragged_launch():
    cfg = abi.default_config()
    ws = [make_window(cfg, *c) for c in CASES]
    solver = pkg.pnp.PnpSolver(cfg, max_batch=len(ws))
    got = [w.copy() for w in ws]
    stats = solver.solve(got)
    for c, w, g, s in zip(CASES, ws, got, stats):
        ref, rs = reference(cfg, c[0], w)
        check(g, s, ref, rs)
    ms, k = solver.kernel_ms()
    assert k == 1 and ms > 0
    solver.close()


@pytest.mark.gpu
def test_device_kernel_full_batch_and_errors():
    cfg = abi.default_config()
    base = make_window(cfg, 2, 7, 150, (0,), 3.0)
    solver = pkg.pnp.PnpSolver(cfg, max_batch=256)
    ws = [base.copy() for _ in range(256)]
    stats = solver.solve(ws)
    ref, rs = reference(cfg, 2, base)
    for g, s in zip(ws[::37], stats[::37]):
        check(g, s, ref, rs)
    assert all(np.abs(w.pose - ws[0].pose).max() < 1e-9 for w in ws)
    ms, _ = solver.kernel_ms()
    print("256 PnP windows (7 frames, ~950 factors): %.3f ms" % ms)
    with pytest.raises(RuntimeError):
        solver.solve([base.copy() for _ in range(257)])
    solver.close()


def solve_on(solver, ws):
    got = [w.copy() for w in ws]
    return got, solver.solve(got)


def solve_fresh(cfg, ws):
    solver = pkg.pnp.PnpSolver(cfg, max_batch=len(ws))
    out = solve_on(solver, ws)
    solver.close()
    return out


@pytest.fixture(scope="module")
def ragged(edges):
    """Every edge window and every CASES row, 8 frames beside 2 and over 3000 factors beside none, solved in one launch
    on a context of its own: (keys, windows, reference results, solved windows, stats)."""
    cfg = abi.default_config()
    keys = list(EDGE_CASES) + [c[0] for c in CASES]
    ws = [edges[k][0] for k in EDGE_CASES] + [make_window(cfg, *c) for c in CASES]
    refs = [edges[k][1:] for k in EDGE_CASES] + [reference(cfg, c[0], w) for c, w in zip(CASES, ws[len(EDGE_CASES):])]
    assert len(ws) <= 40
    return (keys, ws, refs) + solve_fresh(cfg, ws)


def same_route(gs, hs):
    return (gs["iterations"] == hs["iterations"] and list(gs["it_flags"]) == list(hs["it_flags"]) and gs["termination"] == hs["termination"]
            and gs["num_successful_steps"] == hs["num_successful_steps"] and gs["num_unsuccessful_steps"] == hs["num_unsuccessful_steps"])


@pytest.mark.gpu
def test_device_kernel_matches_the_reference_on_edge_windows_and_cases_in_one_ragged_launch(ragged):
    keys, ws, refs, got, stats = ragged
    assert max(w.n for w in ws) == 8 and min(w.n for w in ws) == 2
    for key, w, (ref, rs), g, s in zip(keys, ws, refs, got, stats):
        print(key, list(s["it_flags"]), "%.1e" % max(H.pose_relerr(g.pose, ref.pose), H.relerr(g.speed, ref.speed)))
        check_route(g, s, ref, rs)
        for k in np.flatnonzero(w.fixed):
            assert np.abs(g.pose[k] - w.pose[k]).max() < 1e-12 and np.array_equal(g.speed[k], w.speed[k])


@pytest.mark.gpu
def test_one_context_across_batches_of_different_shapes(ragged):
    """The context keeps its device buffers between calls and pads every window to the batch's frame and factor counts:
    a large batch, a batch of the two-frame and the factor-free windows only (smaller strides, a smaller LDS request),
    the large batch again. Each result is what a context of its own gives, and what the reference gives."""
    cfg = abi.default_config()
    keys, ws, refs, fresh, fstats = ragged
    small = [i for i, (k, w) in enumerate(zip(keys, ws)) if w.n == 2 or w.feat_start[-1] == 0]
    assert len(small) == 3
    sfresh, sfstats = solve_fresh(cfg, [ws[i] for i in small])
    solver = pkg.pnp.PnpSolver(cfg, max_batch=len(ws))
    rounds = [(range(len(ws)), fresh, fstats), (small, sfresh, sfstats), (range(len(ws)), fresh, fstats)]
    for idx, want, wstats in rounds:
        got, stats = solve_on(solver, [ws[i] for i in idx])
        for i, g, s, f, fs in zip(idx, got, stats, want, wstats):
            assert same_route(s, fs), keys[i]
            assert H.pose_relerr(g.pose, f.pose) < TOL and H.relerr(g.speed, f.speed) < TOL, keys[i]
            check_route(g, s, *refs[i])
    solver.close()


@pytest.mark.gpu
def test_rejected_step_windows_alone_and_inside_the_batch(ragged):
    """(LDS atomics reorder the sums of the normal equations, so equality to the bit is not asked.)"""
    cfg = abi.default_config()
    keys, ws, refs, got, stats = ragged
    for name in REJECTED:
        i = keys.index(name)
        (alone,), (astats,) = solve_fresh(cfg, [ws[i]])
        assert "1" in "".join(str(f) for f in astats["it_flags"])
        assert same_route(astats, stats[i]), name
        assert H.pose_relerr(alone.pose, got[i].pose) < TOL and H.relerr(alone.speed, got[i].speed) < TOL, name


# ---------------------------------------------------------------------------------------------------------------------
# the vinsPnP object around the solve (vio_pnp_tracker_*)
class _Scene:
    """30 Hz camera, 120 Hz IMU, a landmark cloud with known positions: what the tracker + the back-end feed solveVinsPnP."""

    def __init__(self, cfg, seed):
        self.cfg, rng = cfg, np.random.default_rng(seed)
        self.rng = rng
        self.traj = synth.Trajectory(rng)
        self.t0 = rng.uniform(0, 20)
        ex = synth.ex_pose_default()
        self.ric, self.tic = synth.quat_to_rot(ex[3:]), ex[:3]
        self.g = np.array([0, 0, cfg.gravity])
        self.ba, self.bg = rng.normal(0, 0.02, 3), rng.normal(0, 0.002, 3)
        self.fdt, self.per = 1.0 / 30, 4
        self.lm = np.column_stack([rng.uniform(-9, 9, 3000), rng.uniform(-9, 9, 3000), rng.uniform(-11, -4, 3000)])

    def t(self, k):
        return self.t0 + k * self.fdt

    def imu(self, t):
        R = self.traj.rot(t)
        return (R.T @ (self.traj.acc(t) + self.g) + self.ba + self.rng.normal(0, 0.02, 3),
                self.traj.omega_body(t) + self.bg + self.rng.normal(0, 0.002, 3))

    def imu_interval(self, k):
        dt = self.fdt / self.per
        return [(dt,) + self.imu(self.t(k - 1) + (s + 1) * dt) for s in range(self.per)]

    def features(self, k, n=120):
        P, R = self.traj.pos(self.t(k)), self.traj.rot(self.t(k))
        Rc, Pc = R @ self.ric, P + R @ self.tic
        pc = (self.lm - Pc) @ Rc
        vis = np.flatnonzero((pc[:, 2] > 0.5) & (np.abs(pc[:, 0]) < 0.4 * pc[:, 2]) & (np.abs(pc[:, 1]) < 0.55 * pc[:, 2]))[:n]
        return [(int(i), pc[i, :2] / pc[i, 2] + self.rng.normal(0, 0.5 / self.cfg.fx, 2), self.lm[i] + self.rng.normal(0, 0.01, 3),
                 int(5 + i % 20)) for i in vis]


def test_pnp_tracker_bookkeeping_without_a_solve():
    """Window filling, updateFeatures, setInit, IMU propagation and the slide with use_pnp = false never reach the
    device (feature_tracker.cpp:151 passes use_pnp through; the default is off)."""
    cfg = abi.default_config()
    sc = _Scene(cfg, 3)
    tr = pkg.pnp.PnpTracker(cfg, sc.tic, sc.ric, pnp_size=6)
    hdrs = []
    for k in range(10):
        for dt, a, w in ([(0.0,) + sc.imu(sc.t(0))] if k == 0 else sc.imu_interval(k)):
            tr.process_imu(dt, a, w)
        if k == 4:   # the back-end's result for frame 2 arrives: it becomes the constant of the window
            P, R, V = sc.traj.pos(sc.t(2)), sc.traj.rot(sc.t(2)), sc.traj.vel(sc.t(2))
            tr.set_init(sc.t(2), sc.ba, sc.bg, P, R, V)
            w = tr.window()
            assert list(w["find_solved"]) == [0, 0, 1, 0, 0, 0, 0] and np.array_equal(w["Ps"][2], P) and np.array_equal(w["Vs"][2], V)
        _, _, solved = tr.process_images([sc.features(k)], [sc.t(k)], use_pnp=False)
        assert solved[0] == 0
        hdrs.append(sc.t(k))
        w = tr.window()
        assert w["frame_count"] == min(k + 1, 6)
    w = tr.window()
    assert list(w["headers"][:6]) == hdrs[4:10]                      # four slides: frames 4..9 remain (+ the copy in slot 6)
    assert list(w["find_solved"]) == [0] * 7                         # frame 2 (the solved one) has left the window
    assert np.array_equal(w["Ps"][6], w["Ps"][5]) and np.array_equal(w["Rs"][6], w["Rs"][5])   # the slide seeds the next frame
    tr.close()


@pytest.mark.gpu
def test_pnp_tracker_follows_the_truth_between_backend_results():
    """solveVinsPnP as readImage runs it: IMU samples since the last frame, the landmarks the back-end has solved with
    their current observations, and every third frame the back-end's newest state (two frames late) through setInit."""
    cfg = abi.default_config()
    sc = _Scene(cfg, 4)
    tr = pkg.pnp.PnpTracker(cfg, sc.tic, sc.ric, pnp_size=6)
    errs, n_solved = [], 0
    for k in range(60):
        for dt, a, w in ([(0.0,) + sc.imu(sc.t(0))] if k == 0 else sc.imu_interval(k)):
            tr.process_imu(dt, a, w)
        if k >= 2 and k % 3 == 2:
            j = k - 2
            tr.set_init(sc.t(j), sc.ba, sc.bg, sc.traj.pos(sc.t(j)) + sc.rng.normal(0, 0.005, 3), sc.traj.rot(sc.t(j)),
                        sc.traj.vel(sc.t(j)) + sc.rng.normal(0, 0.01, 3))
        P, R, solved = tr.process_images([sc.features(k)], [sc.t(k)], use_pnp=True)
        n_solved += int(solved[0])
        if solved[0]:
            # P / R = the second-newest slot after the slide = the frame just solved
            errs.append(np.linalg.norm(P[0] - sc.traj.pos(sc.t(k))))
            assert np.abs(R[0] - sc.traj.rot(sc.t(k))).max() < 0.01
    assert n_solved == 60 - 6
    errs = np.array(errs)
    assert np.sqrt((errs ** 2).mean()) < 0.03 and errs.max() < 0.08, (np.sqrt((errs ** 2).mean()), errs.max())
    tr.close()


@pytest.mark.gpu
def test_pnp_tracker_for_three_sequences_is_three_trackers_for_one():
    """Three sequences in one tracker (their solves share a launch, padded to the largest) against three trackers of one
    sequence fed the same calls: back-end results arriving at different frames per sequence, and the middle sequence
    without a frame for two frames while the others go on, so the launch shrinks to two windows and the solved windows
    no longer sit at their sequence's index. The 1e-9 is the bound between copies inside one batch
    (test_device_kernel_full_batch_and_errors); measured on an MI355X: 7e-18."""
    cfg = abi.default_config()
    scs = [_Scene(cfg, seed) for seed in (4, 5, 6)]
    one = pkg.pnp.PnpTracker(cfg, scs[0].tic, scs[0].ric, n_seq=3, pnp_size=6)
    each = [pkg.pnp.PnpTracker(cfg, sc.tic, sc.ric, n_seq=1, pnp_size=6) for sc in scs]
    n_solved, worst = np.zeros(3, int), 0.0
    for k in range(15):
        active = [1, 0 if k in (9, 10) else 1, 1]
        for q, sc in enumerate(scs):
            for dt, a, w in ([(0.0,) + sc.imu(sc.t(0))] if k == 0 else sc.imu_interval(k)):
                one.process_imu(dt, a, w, seq=q), each[q].process_imu(dt, a, w)
            if k >= 2 and (k + q) % 3 == 2:
                j = k - 2
                init = (sc.t(j), sc.ba, sc.bg, sc.traj.pos(sc.t(j)) + sc.rng.normal(0, 0.005, 3), sc.traj.rot(sc.t(j)),
                        sc.traj.vel(sc.t(j)) + sc.rng.normal(0, 0.01, 3))
                one.set_init(*init, seq=q), each[q].set_init(*init)
        feats = [sc.features(k, n=80 + 20 * q) if active[q] else [] for q, sc in enumerate(scs)]
        hdrs = [sc.t(k) for sc in scs]
        P, R, solved = one.process_images(feats, hdrs, use_pnp=True, active=active)
        for q in range(3):
            Pq, Rq, sq = each[q].process_images([feats[q]], [hdrs[q]], use_pnp=True, active=[active[q]])
            assert solved[q] == sq[0] == (1 if k >= 6 and active[q] else 0)
            worst = max(worst, np.abs(P[q] - Pq[0]).max(), np.abs(R[q] - Rq[0]).max())
        n_solved += solved
    print("three sequences in one tracker against one each: largest difference %.2e" % worst)
    assert list(n_solved) == [9, 7, 9]
    assert worst < 1e-9
    for q in range(3):   # and the windows they are left with
        a, b = one.window(seq=q), each[q].window()
        assert a["frame_count"] == b["frame_count"] and np.array_equal(a["find_solved"], b["find_solved"])
        assert np.array_equal(a["headers"], b["headers"])
        assert max(np.abs(a[key] - b[key]).max() for key in ("Ps", "Rs", "Vs")) < 1e-9
    one.close()
    for t in each:
        t.close()


def test_solved_features_are_joined_with_the_tracker_points_by_id():
    cfg = abi.default_config()
    lib = abi.load_product()
    ids = np.array([3, 4, 7, 9, 12, 15, 20], np.int32)                 # tracker: ascending ids
    pts = np.array([[10 * i + 0.25, 20 * i + 0.5] for i in range(7)], np.float32)
    solved = (abi.VioPnpFeature * 5)()
    for k, (fid, tn) in enumerate([(1, 5), (4, 6), (9, 7), (13, 8), (20, 9)]):   # back-end: ascending ids, some lost by the tracker
        solved[k].id, solved[k].track_num = fid, tn
        solved[k].position[:] = [fid * 1.0, fid * 2.0, fid * 3.0]
    out, n = (abi.VioPnpFeature * 8)(), C.c_int32()
    rc = lib.vio_pnp_match_features(C.byref(cfg), ids.ctypes.data_as(C.POINTER(C.c_int32)), pts.ctypes.data_as(C.POINTER(C.c_float)), 7,
                                    solved, 5, out, 8, C.byref(n))
    assert rc == 0 and n.value == 3
    assert [out[i].id for i in range(3)] == [4, 9, 20] and [out[i].track_num for i in range(3)] == [6, 7, 9]
    for o, row in zip(out[:3], (1, 3, 6)):
        assert abs(o.observation[0] - (float(pts[row, 0]) - cfg.cx) / cfg.fx) < 1e-15
        assert abs(o.observation[1] - (float(pts[row, 1]) - cfg.cy) / cfg.fy) < 1e-15
        assert list(o.position) == [o.id * 1.0, o.id * 2.0, o.id * 3.0]
    assert lib.vio_pnp_match_features(C.byref(cfg), ids.ctypes.data_as(C.POINTER(C.c_int32)), pts.ctypes.data_as(C.POINTER(C.c_float)), 7,
                                      solved, 5, out, 2, C.byref(n)) == abi.VIO_ECAP
