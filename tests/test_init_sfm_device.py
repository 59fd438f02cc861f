"""Estimator start-up on the device (vio_init_sfm_*, csrc/init_core.h / vio_init_sfm.hip): the relative pose fit, the PnP
chain and the triangulations of GlobalSFM::construct, its bundle adjustment, the inversion and the PnP of the frames
outside the window, for a batch of problems in one call.

Reference: the host route in the product library -- vio_init_relative_pose, vio_init_sfm, vio_init_pnp, and for the state
ahead of the bundle adjustment the chain of inital_sfm.cpp:117-227 driven from here over vio_init_pnp and
vio_init_triangulate_point (the library does not export that intermediate state). CPU: the kernel source on the SIMT
emulator (tests/emul/simt_init.cpp), which has to give the host route's bits up to the bundle adjustment. GPU: the same
scenes through vio_init_sfm_solve.

Observed on the MI355X (test_gpu_scenes_follow_the_host_route): see that test's docstring."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import helpers as H
from helpers import abi

init_sfm = H.pkg.init_sfm
synth = H.pkg.synth
_dp, _ip, _u8 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
OK, FAIL_RELATIVE, FAIL_CHAIN, FAIL_BA, FAIL_PNP = range(5)


def _p(a, ty=_dp):
    return a.ctypes.data_as(ty)


@functools.lru_cache(maxsize=None)
def _emul():
    lib = H.build_emul_lib("simt_init.cpp", "libsimt_init.so", "VIO_SIMT")
    lib.simt_init_sfm_solve.argtypes = [C.POINTER(abi.VioInitSfmProblem), C.c_int, C.POINTER(abi.VioSolveStats), C.c_int, C.c_int]
    lib.simt_init_head_state.argtypes = [C.c_int, _dp, _dp, _dp]
    lib.simt_init_fit_sign.argtypes = [C.c_int]
    return lib


# ---------------------------------------------------------------------------------------------------------------------
# scenes
def _scene(seed, F=11, l=1, n_both=60, n_head=40, n_tail=40, n_single=5, kind="3d", pix_noise=0.5, n_extra=0, extra_pts=None,
           thin=None, pair=False, relative=False):
    """A camera on a smooth trajectory (0.1 s between frames) and a landmark list in random order: n_both landmarks seen in
    every frame (the correspondences of frames l and F-1), n_head seen in frames 0 .. F-2, n_tail in frames l+1 .. F-1,
    n_single seen once. kind: 3d / plane (tilted) / far (beyond 50 baselines). thin = (frame, k): only k of the landmarks
    that have a position when the chain reaches `frame` are seen there. pair: one more landmark seen in two non-adjacent
    frames only, which no pair of construct's steps 1-3 covers. Extra frames sit half-way between window frames. relative: the
    problem brings its relative pose (the truth), as on the five-point route; else it is fitted."""
    rng = np.random.default_rng(seed)
    traj = synth.Trajectory(rng)
    t0 = rng.uniform(0, 20)
    ex = synth.ex_pose_default()
    ric, tic = synth.quat_to_rot(ex[3:]), ex[:3]
    pose = lambda t: (traj.rot(t) @ ric, traj.pos(t) + traj.rot(t) @ tic)
    cams = [pose(t0 + 0.1 * k) for k in range(F)]
    n = n_both + n_head + n_tail + n_single + (1 if pair else 0)
    z = {"3d": rng.uniform(4, 11, n), "plane": np.full(n, 6.0), "far": rng.uniform(400, 800, n)}[kind]
    xyc = rng.uniform(-0.45, 0.45, (n, 2))
    Xc = np.column_stack([xyc * z[:, None], z])
    if kind == "plane":
        Xc[:, 2] += 0.3 * Xc[:, 0]
    Rm, pm = cams[F // 2]
    Xw = Xc @ Rm.T + pm
    sig = pix_noise / 460.0
    span = [(0, F)] * n_both + [(0, F - 1)] * n_head + [(l + 1, F)] * n_tail
    frames = [list(range(a, b)) for a, b in span] + [[int(rng.integers(0, F))] for _ in range(n_single)]
    if pair:
        frames.append([l + 1, F - 2] if F - 2 > l + 2 else [0, F - 1])
    if thin is not None:                      # landmarks seen in `frame`: keep it for k of them
        f, k = thin
        seen = [j for j in range(n) if f in frames[j] and len(frames[j]) >= 2]
        for j in seen[k:]:
            frames[j] = [g for g in frames[j] if g != f]
    order = rng.permutation(n)
    start, fr, xy = [0], [], []
    for j in order:
        for k in frames[j]:
            R, p = cams[k]
            c = R.T @ (Xw[j] - p)
            fr.append(k), xy.append((c[0] / c[2] + rng.normal(0, sig), c[1] / c[2] + rng.normal(0, sig)))
        start.append(len(fr))
    extras = []
    for e in range(n_extra):
        k = (l + 1 + 2 * e) % (F - 1)
        R, p = pose(t0 + 0.1 * k + 0.05)
        where = np.argsort(order)             # list index of landmark j
        tracked = np.array([where[j] for j in range(n) if len(frames[j]) >= 2])
        idx = rng.permutation(tracked)[:extra_pts[e] if extra_pts else 50]
        if not extra_pts:                     # and two landmarks seen once: not tracked, skipped
            idx = np.concatenate([idx[:20], [where[j] for j in range(n) if len(frames[j]) < 2][:2], idx[20:]])
        c = (Xw[order[idx]] - p) @ R
        extras.append((k + 1, idx, c[:, :2] / c[:, 2:3] + rng.normal(0, sig, (len(idx), 2))))
    Ra, pa = cams[l]
    Rb, pb = cams[F - 1]
    return dict(F=F, l=l, start=np.array(start, np.int32), fr=np.array(fr, np.int32), xy=np.array(xy).reshape(-1, 2), extras=extras,
                R_true=Ra.T @ Rb, t_true=Ra.T @ (pb - pa), seed=seed,
                relative=((Ra.T @ Rb).ravel(), Ra.T @ (pb - pa) / np.linalg.norm(pb - pa)) if relative else None)


def _problem(sc, relative=None, hint=None):
    return init_sfm.SfmProblem(sc["F"], sc["l"], sc["start"], sc["fr"], sc["xy"], relative=relative or sc["relative"], hint=hint,
                               extras=sc["extras"])


def _hint(sc, deg=1.5):
    return sc["R_true"] @ synth.rotvec_to_rot(np.random.default_rng(sc["seed"]).normal(0, np.radians(deg) / np.sqrt(3), 3))


def _permuted(sc, rng):
    """The same scene with its landmark list in another order (and the extra frames' indices following)."""
    n = len(sc["start"]) - 1
    perm = rng.permutation(n)
    inv = np.empty(n, int)
    inv[perm] = np.arange(n)
    start, fr, xy = [0], [], []
    for j in perm:
        a, b = sc["start"][j], sc["start"][j + 1]
        fr.extend(sc["fr"][a:b]), xy.extend(sc["xy"][a:b])
        start.append(len(fr))
    out = dict(sc)
    out.update(start=np.array(start, np.int32), fr=np.array(fr, np.int32), xy=np.array(xy).reshape(-1, 2),
               extras=[(g, inv[idx].astype(np.int32), x) for g, idx, x in sc["extras"]])
    return out, perm


# ---------------------------------------------------------------------------------------------------------------------
# the host route
def _mat3vec(A, v):  # vio_math.h mat3vec, operation for operation
    return [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]


def _q_to_R(x, y, z, w):  # vio_math.h qtoR
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def _R_to_q(R):  # vio_math.h RtoQ -> (w, x, y, z)
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return (w, (R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t)
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = math.sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0)
    v = [0.0, 0.0, 0.0]
    v[i] = 0.5 * t
    t = 0.5 / t
    w = (R[k][j] - R[j][k]) * t
    v[j], v[k] = (R[j][i] + R[i][j]) * t, (R[k][i] + R[i][k]) * t
    return (w, v[0], v[1], v[2])


def _correspondences(sc):
    a, b = [], []
    for j in range(len(sc["start"]) - 1):
        s, e = sc["start"][j], sc["start"][j + 1]
        f = list(sc["fr"][s:e])
        if sc["l"] in f and sc["F"] - 1 in f:
            a.append(sc["xy"][s + f.index(sc["l"])]), b.append(sc["xy"][s + f.index(sc["F"] - 1)])
    return np.array(a).reshape(-1, 2), np.array(b).reshape(-1, 2)


def _host_relative(sc, hint=None):
    xy0, xy1 = _correspondences(sc)
    R, t, inl, ok = np.zeros(9), np.zeros(3), C.c_int32(), C.c_int32()
    h = None if hint is None else np.ascontiguousarray(hint, np.float64)
    rc = abi.load_product().vio_init_relative_pose(_p(xy0), _p(xy1), len(xy0), None if h is None else _p(h), _p(R), _p(t), C.byref(inl),
                                                   C.byref(ok))
    assert rc == 0
    return R, t, inl.value, ok.value, len(xy0)


def _host_pnp(p3, p2, R, t):
    p3, p2 = np.ascontiguousarray(p3, np.float64), np.ascontiguousarray(p2, np.float64)
    R, t, ok = np.array(R, np.float64).reshape(9).copy(), np.array(t, np.float64).copy(), C.c_int32()
    assert abi.load_product().vio_init_pnp(_p(p3), _p(p2), len(p3), _p(R), _p(t), C.byref(ok)) == 0
    return ok.value, R.reshape(3, 3), t


def _host_tri(P0, P1, x0, x1):
    out = np.zeros(3)
    a = [np.ascontiguousarray(v, np.float64) for v in (P0, P1, x0, x1)]
    assert abi.load_product().vio_init_triangulate_point(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(out)) == 0
    return out


def _host_chain(sc, Rrel, trel):
    """GlobalSFM::construct up to its bundle adjustment (inital_sfm.cpp:117-227) over the library's PnP and triangulation.
    -> (ok, cq [F][4] w x y z, ct [F][3], X [n][3], state [n])"""
    F, l, last = sc["F"], sc["l"], sc["F"] - 1
    n = len(sc["start"]) - 1
    obs = [{int(sc["fr"][k]): sc["xy"][k] for k in range(sc["start"][j], sc["start"][j + 1])} for j in range(n)]
    lists = [[int(sc["fr"][k]) for k in range(sc["start"][j], sc["start"][j + 1])] for j in range(n)]
    Rc, tc, X, state = [None] * F, [None] * F, np.zeros((n, 3)), np.zeros(n, bool)
    Rrel = np.asarray(Rrel).reshape(3, 3)
    Rc[l], tc[l] = np.eye(3), np.zeros(3)
    Rc[last] = Rrel.T.copy()
    tc[last] = np.array([-v for v in _mat3vec(Rc[last], trel)])
    P = lambda i: np.hstack([Rc[i], tc[i].reshape(3, 1)])

    def two(f0, f1):
        for j in range(n):
            if not state[j] and f0 in obs[j] and f1 in obs[j]:
                X[j], state[j] = _host_tri(P(f0), P(f1), obs[j][f0], obs[j][f1]), True

    def pnp(i, src):
        js = [j for j in range(n) if state[j] and i in obs[j]]
        if len(js) < 15:
            return False
        ok, R, t = _host_pnp(X[js], np.array([obs[j][i] for j in js]), Rc[src], tc[src])
        if ok:
            Rc[i], tc[i] = R, t
        return bool(ok)

    for i in range(l, last):
        if i > l:
            Rc[i], tc[i] = Rc[i - 1].copy(), tc[i - 1].copy()
            if not pnp(i, i - 1):
                return False, None, None, X, state
        two(i, last)
    for i in range(l + 1, last):
        two(l, i)
    for i in range(l - 1, -1, -1):
        Rc[i], tc[i] = Rc[i + 1].copy(), tc[i + 1].copy()
        pnp(i, i + 1)
        two(i, l)
    for j in range(n):
        if not state[j] and len(lists[j]) >= 2:
            f0, f1 = lists[j][0], lists[j][-1]
            a, b = sc["start"][j], sc["start"][j + 1] - 1
            X[j], state[j] = _host_tri(P(f0), P(f1), sc["xy"][a], sc["xy"][b]), True
    return True, np.array([_R_to_q(Rc[i]) for i in range(F)]), np.array(tc), X, state


def _host_sfm(sc, Rrel, trel):
    F, n = sc["F"], len(sc["start"]) - 1
    q, T, pts, pok, ok = np.zeros((F, 4)), np.zeros((F, 3)), np.zeros((n, 3)), np.zeros(n, np.uint8), C.c_int32()
    rc = abi.load_product().vio_init_sfm(F, sc["l"], _p(np.ascontiguousarray(Rrel, np.float64)), _p(np.ascontiguousarray(trel, np.float64)), n,
                                         _p(sc["start"], _ip), _p(sc["fr"], _ip), _p(sc["xy"]), _p(q), _p(T), _p(pts), _p(pok, _u8), C.byref(ok))
    assert rc == 0
    return ok.value, q, T, pts, pok


def _host_ba_stats(sc, cq, ct, X, state):
    cq, ct, X = cq.copy(), ct.copy(), X.copy()
    st, ok = abi.VioSolveStats(), C.c_int32(-1)
    okf = np.ascontiguousarray(state, np.uint8)
    rc = abi.load_product().vio_init_bundle_adjust(sc["F"], sc["l"], _p(cq), _p(ct), len(X), _p(X), _p(okf, _u8), _p(sc["start"], _ip),
                                                   _p(sc["fr"], _ip), _p(sc["xy"]), C.byref(st), C.byref(ok))
    assert rc == 0
    return ok.value, st.iterations, st.termination, list(st.it_flags[:st.iterations])


def _host_extra(sc, e, q, T, pts, pok):
    """The PnP of extra frame e as solveInitial runs it (VINS.cpp:926-1003) on the given window poses and landmarks."""
    g, idx, xy = sc["extras"][e]
    keep = [k for k, j in enumerate(idx) if pok[j]]
    if len(keep) < 6:
        return None
    Rq = _q_to_R(*q[g])
    R0 = Rq.T.copy()
    t0 = np.array([-v for v in _mat3vec(R0, T[g])])
    return _host_pnp(pts[idx[keep]], xy[keep], R0, t0)


def _run_emul(problems, order=0, stages=3):
    ps = [p.copy() for p in problems]
    rc, st = init_sfm.solve_with(lambda arr, n, s: _emul().simt_init_sfm_solve(arr, n, s, order, stages), ps)
    assert rc == 0
    heads, signs = [], []
    for b, p in enumerate(ps):
        cq, ct, X = np.zeros((p.frame_num, 4)), np.zeros((p.frame_num, 3)), np.zeros((max(p.n_features, 1), 3))
        heads.append((cq, ct, X) if _emul().simt_init_head_state(b, _p(cq), _p(ct), _p(X)) == 0 else None)
        signs.append(_emul().simt_init_fit_sign(b))
    return ps, st, heads, signs


def _check_head(sc, p, head, hint=None):
    """The emulator's (or any exact route's) head of one problem against the host route, bit for bit."""
    if sc["relative"] is None:
        R, t, inl, ok, ncorr = _host_relative(sc, hint)
        assert p.inliers == inl
        if ncorr >= 9:
            assert np.array_equal(p.relative_R, R) and np.array_equal(p.relative_T, t)
        if not ok:
            assert p.status == FAIL_RELATIVE and head is None
            return FAIL_RELATIVE
    else:
        R, t = sc["relative"]
    cok, cq, ct, X, state = _host_chain(sc, R, t)
    if not cok:
        assert p.status == FAIL_CHAIN and head is None
        return FAIL_CHAIN
    assert p.status not in (FAIL_RELATIVE, FAIL_CHAIN) and head is not None
    assert np.array_equal(head[0], cq) and np.array_equal(head[1], ct)
    two = np.diff(sc["start"]) >= 2
    assert np.array_equal(state, two)
    assert np.array_equal(head[2][: len(two)][two], X[two])
    return OK


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the ctypes mirror
def test_problem_struct_layout_matches_the_header(tmp_path):
    import os
    import subprocess
    fields = ["relative_mode", "R_hint", "n_extra", "extra_xy", "status", "relative_R", "q", "point_ok", "extra_T"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vio_amd.h"\nint main(){printf("%zu", sizeof(VioInitSfmProblem));\n'
                   + "".join('printf(" %%zu", offsetof(VioInitSfmProblem, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(H.ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.VioInitSfmProblem)] + [getattr(abi.VioInitSfmProblem, f).offset for f in fields]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the emulator
FIT_SCENES = {
    "n9": dict(seed=21, n_both=9), "n8": dict(seed=22, n_both=8), "n21": dict(seed=23, n_both=21), "n63": dict(seed=24, n_both=63),
    "n64": dict(seed=25, n_both=64), "n65": dict(seed=26, n_both=65), "n257": dict(seed=27, n_both=257, n_head=10, n_tail=10),
    "plane": dict(seed=4, kind="plane"), "plane_hint": dict(seed=8, kind="plane", hint=True),
    "plane_hint_decides": dict(seed=3, kind="plane", hint=True), "far": dict(seed=31, kind="far", pix_noise=0.05),
    "3d_a": dict(seed=1), "3d_b": dict(seed=2), "3d_c": dict(seed=5),
}


@functools.lru_cache(maxsize=None)
def _fit_scene(name):
    kw = dict(FIT_SCENES[name])
    hint = kw.pop("hint", False)
    sc = _scene(**kw)
    return sc, (_hint(sc) if hint else None)


@pytest.mark.parametrize("name", sorted(FIT_SCENES))
def test_head_gives_the_host_routes_bits(name):
    sc, hint = _fit_scene(name)
    outs = []
    for order in (0, 1, 2):
        ps, _, heads, signs = _run_emul([_problem(sc, hint=hint)], order, stages=1)
        outs.append((_check_head(sc, ps[0], heads[0], hint), signs[0]))
    assert outs[0] == outs[1] == outs[2]
    if name == "n8":
        assert outs[0][0] == FAIL_RELATIVE and ps[0].inliers == 0 and not ps[0].relative_R.any()
    if name == "far":
        assert outs[0][0] == FAIL_RELATIVE and ps[0].inliers <= 10
    if name == "plane_hint_decides":   # without the hint the fit lands on the plane's other solution
        R0 = _host_relative(sc)[0]
        assert np.abs(R0 - ps[0].relative_R).max() > 1e-3


def test_the_scenes_cover_both_signs_of_the_cheirality_vote():
    signs = {_run_emul([_problem(_fit_scene(k)[0], hint=_fit_scene(k)[1])], 0, stages=1)[3][0] for k in ("3d_a", "3d_b", "3d_c", "n21", "n63", "n64")}
    assert signs == {1, -1}


CHAIN_SCENES = {
    "f3_l0": dict(seed=41, relative=True, F=3, l=0), "f3_l1": dict(seed=42, relative=True, F=3, l=1), "f11_l0": dict(seed=43, relative=True, l=0), "f11_l1": dict(seed=44, relative=True, l=1),
    "f11_l9": dict(seed=45, relative=True, l=9), "f16": dict(seed=46, relative=True, F=16, l=3), "f17": dict(seed=47, relative=True, F=17, l=3),
    "fwd14": dict(seed=48, relative=True, l=1, thin=(3, 14)), "fwd15": dict(seed=49, relative=True, l=1, thin=(3, 15)), "back14": dict(seed=50, relative=True, l=3, thin=(1, 14)),
    "pair": dict(seed=51, relative=True, l=1, pair=True, n_single=9),
}


@functools.lru_cache(maxsize=None)
def _chain_scene(name):
    return _scene(**CHAIN_SCENES[name])


@pytest.mark.parametrize("name", sorted(CHAIN_SCENES))
def test_chain_edges_give_the_host_routes_bits(name):
    sc = _chain_scene(name)
    got = [_check_head(sc, *(lambda r: (r[0][0], r[2][0]))(_run_emul([_problem(sc)], order, stages=1))) for order in (0, 2)]
    assert got[0] == got[1] == (FAIL_CHAIN if name == "fwd14" else OK)


def _compare_final(p, sc, Rrel, trel, st):
    """A whole call against host vio_init_sfm + vio_init_bundle_adjust's trace + vio_init_pnp."""
    ok, q, T, pts, pok = _host_sfm(sc, Rrel, trel)
    cok, cq, ct, X, state = _host_chain(sc, Rrel, trel)
    assert cok
    bok, its, term, flags = _host_ba_stats(sc, cq, ct, X, state)
    assert bok == ok
    assert (st["iterations"], st["termination"]) == (its, term) and list(st["it_flags"][:its]) == flags
    n = len(pok)
    assert np.array_equal(p.point_ok[:n], pok)
    if not ok:
        assert p.status == FAIL_BA
        return
    assert np.abs(p.q - q).max() < 1e-9 and np.abs(p.T - T).max() < 1e-9
    m = pok.astype(bool)
    assert np.abs(p.points[:n][m] - pts[m]).max() < 1e-8 * max(1.0, np.abs(pts[m]).max())
    want = OK
    for e in range(len(sc["extras"])):
        ref = _host_extra(sc, e, p.q, p.T, p.points, p.point_ok)   # the same landmarks: bit for bit
        if ref is None or not ref[0]:
            want = FAIL_PNP if want == OK else want
        if ref is not None:
            assert np.array_equal(p.extra_R[e].reshape(3, 3), ref[1]) and np.array_equal(p.extra_T[e], ref[2])
    assert p.status == want


WHOLE_SCENES = {"w11": dict(seed=61, l=1, n_extra=3), "w11_pnp5": dict(seed=62, l=2, n_extra=3, extra_pts=[50, 5, 50]),
                "w11_pnp6": dict(seed=63, l=0, n_extra=2, extra_pts=[6, 40]), "w17": dict(seed=64, F=17, l=4, n_extra=1),
                "w8": dict(seed=66, F=8, l=2, n_extra=1)}


@functools.lru_cache(maxsize=None)
def _whole_scene(name):
    return _scene(**WHOLE_SCENES[name])


@pytest.mark.parametrize("name", sorted(WHOLE_SCENES))
def test_whole_call_on_the_emulator(name):
    sc = _whole_scene(name)
    R, t, _, ok, _ = _host_relative(sc)
    assert ok
    ps, st, _, _ = _run_emul([_problem(sc)], 0)
    _compare_final(ps[0], sc, R, t, st[0])
    if name == "w11_pnp5":
        assert ps[0].status == FAIL_PNP
    if name == "w11":   # the five-point route: the relative pose is an input
        ps0, st0, _, _ = _run_emul([_problem(sc, relative=(R, t))], 0)
        for a in ("q", "T", "points", "extra_R", "extra_T"):
            assert np.array_equal(getattr(ps0[0], a), getattr(ps[0], a))
        assert ps0[0].status == ps[0].status == OK


# a relative pose far from the truth: the chain goes through, the bundle adjustment does not converge in its 50 iterations
_BAD_RELATIVE = (synth.rotvec_to_rot(np.array([0.0, 0.6, 0.0])).ravel(), np.array([0.0, 0.0, -1.0]))


def _mixed_batch():
    """Seven problems: two that succeed (one of 17 frames), and failures in each of the four ways."""
    return [_problem(_whole_scene("w11")), _problem(_fit_scene("n8")[0]), _problem(_chain_scene("fwd14")), _problem(_whole_scene("w11_pnp5")),
            _problem(_whole_scene("w17")), _problem(_fit_scene("far")[0]), _problem(_whole_scene("w11"), relative=_BAD_RELATIVE)]


def _bits(p, st):
    return (p.status, p.inliers, p.relative_R.tobytes(), p.relative_T.tobytes(), p.q.tobytes(), p.T.tobytes(), p.points.tobytes(),
            p.point_ok.tobytes(), p.extra_R.tobytes(), p.extra_T.tobytes(), st["iterations"], st["termination"], st["final_cost"])


def test_a_mixed_batch_equals_its_single_problem_runs():
    probs = _mixed_batch()
    single = [_bits(*(lambda r: (r[0][0], r[1][0]))(_run_emul([p], 0))) for p in probs]
    assert {s[0] for s in single} == {OK, FAIL_RELATIVE, FAIL_CHAIN, FAIL_BA, FAIL_PNP}
    for order in (list(range(7)), [6, 3, 5, 0, 2, 4, 1]):
        ps, st, _, _ = _run_emul([probs[i] for i in order], 0)
        for k, i in enumerate(order):
            assert _bits(ps[k], st[k]) == single[i], (order, k)


def test_a_failed_bundle_adjustment_is_reported():
    """The chain goes through, the bundle adjustment's verdict and trace are the host's."""
    sc = _whole_scene("w11")
    ps, st, _, _ = _run_emul([_problem(sc, relative=_BAD_RELATIVE)], 0)
    assert ps[0].status == FAIL_BA and not ps[0].q.any() and ps[0].point_ok.any()
    _compare_final(ps[0], sc, *_BAD_RELATIVE, st[0])


# ---------------------------------------------------------------------------------------------------------------------
# fixture guard: the scenes of the GPU test are ones whose decisions do not hang on rounding
GPU_SCENES = [("fit", k) for k in sorted(FIT_SCENES)] + [("chain", k) for k in sorted(CHAIN_SCENES)] + [("whole", k) for k in sorted(WHOLE_SCENES)]


def _gpu_scene(kind, name):
    return _fit_scene(name) if kind == "fit" else ((_chain_scene if kind == "chain" else _whole_scene)(name), None)


def _host_head(sc, hint):
    if sc["relative"] is None:
        R, t, inl, ok, _ = _host_relative(sc, hint)
        if not ok:
            return dict(status=FAIL_RELATIVE, inliers=inl, R=R, t=t)
    else:
        (R, t), inl = sc["relative"], -1
    cok, cq, ct, X, state = _host_chain(sc, R, t)
    return dict(status=OK if cok else FAIL_CHAIN, inliers=inl, R=R, t=t, cq=cq, ct=ct, X=X)


@functools.lru_cache(maxsize=None)
def _spread(kind, name):
    """(stable, largest difference of relative pose / state ahead of the bundle adjustment) over 8 seeded permutations of
    the landmark list, on the host route."""
    sc, hint = _gpu_scene(kind, name)
    base = _host_head(sc, hint)
    rng = np.random.default_rng(1000 + sc["seed"])
    stable, spread = True, 0.0
    for _ in range(8):
        sp, perm = _permuted(sc, rng)
        got = _host_head(sp, hint)
        same = got["status"] == base["status"] and got["inliers"] == base["inliers"] and np.abs(got["R"] - base["R"]).max() < 1e-3
        stable = stable and same
        if not same:
            continue
        spread = max(spread, np.abs(got["R"] - base["R"]).max(), np.abs(got["t"] - base["t"]).max())
        if base["status"] == OK:
            two = np.diff(sc["start"]) >= 2
            spread = max(spread, np.abs(got["cq"] - base["cq"]).max(), np.abs(got["ct"] - base["ct"]).max(),
                         np.abs(got["X"][np.argsort(perm)][two] - base["X"][two]).max())
    return stable, float(spread)


def test_the_gpu_scenes_keep_their_decisions_under_reordering():
    unstable = [s for s in GPU_SCENES if not _spread(*s)[0]]
    assert len(unstable) * 8 <= len(GPU_SCENES), unstable


# ---------------------------------------------------------------------------------------------------------------------
# GPU
@pytest.fixture(scope="module")
def solver():
    s = init_sfm.SfmSolver(16, 17, 400, 4000, 4)
    yield s
    s.close()


@pytest.mark.gpu
def test_gpu_scenes_follow_the_host_route(solver):
    """Decisions equal the host route's; relative pose and the state ahead of the bundle adjustment within 100 x the
    reordering spread of the scene (floor 1e-12); final poses and points within the bundle adjustment's bar. The ratio
    observed / spread is printed per scene.

    Observed on an MI355X: 29 of the 30 scenes bit-equal to the host route up to the bundle adjustment (the device calls
    correctly rounded sin / cos / acos, the host the C library, which rounds the other way for about 0.04 % of arguments);
    fit/3d_a differs by 2.5e-8 at a spread of 7.1e-8: ratio 0.36, the largest."""
    worst = 0.0
    for kind, name in GPU_SCENES:
        stable, spread = _spread(kind, name)
        if not stable:
            continue
        sc, hint = _gpu_scene(kind, name)
        p = _problem(sc, hint=hint)
        st = solver.solve([p])[0]
        ref = _host_head(sc, hint)
        bound = max(100 * spread, 1e-12)
        diff = 0.0
        if sc["relative"] is None:
            assert p.inliers == ref["inliers"], (kind, name)
        if sc["relative"] is None and len(_correspondences(sc)[0]) >= 9:
            diff = max(np.abs(p.relative_R - ref["R"]).max(), np.abs(p.relative_T - ref["t"]).max())
        rc, cq, ct, X = solver.head_state(0, p)
        if ref["status"] != OK:
            assert p.status == ref["status"] and rc == abi.VIO_ESTATE, (kind, name)
        else:
            assert rc == 0 and p.status not in (FAIL_RELATIVE, FAIL_CHAIN), (kind, name)
            two = np.diff(sc["start"]) >= 2
            diff = max(diff, np.abs(cq - ref["cq"]).max(), np.abs(ct - ref["ct"]).max(), np.abs(X[: len(two)][two] - ref["X"][two]).max())
            _compare_final(p, sc, ref["R"], ref["t"], st)
        print("%s/%s: spread %.3g, device - host %.3g, ratio %.3g%s" % (kind, name, spread, diff, diff / max(spread, 1e-300),
                                                                        " (bit-equal)" if diff == 0 else ""))
        assert diff <= bound, (kind, name, diff, bound)
        worst = max(worst, diff / max(spread, 1e-18))
    print("largest device - host difference over spread: %.3g" % worst)


@pytest.mark.gpu
def test_gpu_results_do_not_depend_on_slot_batch_or_run(solver):
    probs = _mixed_batch()
    p0 = probs[0].copy()
    a = _bits(p0, solver.solve([p0])[0])
    p1 = probs[0].copy()
    assert _bits(p1, solver.solve([p1])[0]) == a
    single = []
    for p in probs:
        q = p.copy()
        single.append(_bits(q, solver.solve([q])[0]))
    assert {s[0] for s in single} == {OK, FAIL_RELATIVE, FAIL_CHAIN, FAIL_BA, FAIL_PNP}
    for order in ([0, 1, 2, 3, 4, 5, 6, 1, 2], [2, 1, 6, 5, 4, 3, 2, 1, 0]):
        ps = [probs[i].copy() for i in order]
        st = solver.solve(ps)
        for k, i in enumerate(order):
            assert _bits(ps[k], st[k]) == single[i], (order, k)


@pytest.mark.gpu
def test_gpu_arguments_and_capacities():
    lib = abi.load_product()
    sc = _whole_scene("w11")
    s = init_sfm.SfmSolver(2, 11, 400, 4000, 4)
    try:
        def untouched(ps):
            return all(not p.q.any() and not p.T.any() and not p.points.any() and not p.point_ok.any() and not p.extra_R.any()
                       and p.status == -1 for p in ps)

        ps = [_problem(sc) for _ in range(3)]
        assert s.solve_rc(ps)[0] == abi.VIO_ECAP and untouched(ps)                       # n > max_batch
        assert s.solve_rc([_problem(_whole_scene("w17"))])[0] == abi.VIO_ECAP            # frames
        for args in ((2, 11, 100, 4000, 4), (2, 11, 400, 500, 4), (2, 11, 400, 4000, 2)):  # landmarks, observations, extra frames
            small = init_sfm.SfmSolver(*args)
            ps = [_problem(sc), _problem(sc)]
            assert small.solve_rc(ps)[0] == abi.VIO_ECAP and untouched(ps)
            small.close()
        dup = dict(sc)
        dup["fr"] = sc["fr"].copy()
        j = int(np.argmax(np.diff(sc["start"]) >= 2))
        dup["fr"][sc["start"][j] + 1] = dup["fr"][sc["start"][j]]
        ps = [_problem(sc), _problem(dup)]
        assert s.solve_rc(ps)[0] == abi.VIO_ECAP and untouched(ps)                       # a landmark twice in one frame
        desc = dict(sc)
        desc["start"] = sc["start"].copy()
        desc["start"][5] = desc["start"][6] + 1
        ps = [_problem(sc), _problem(desc)]
        assert s.solve_rc(ps)[0] == abi.VIO_EINVAL and untouched(ps)                     # descending feat_start
        arr = (abi.VioInitSfmProblem * 1)()
        p = _problem(sc)
        p.fill_struct(arr[0])
        arr[0].obs_xy = None
        assert lib.vio_init_sfm_solve(s._h, arr, 1, None) == abi.VIO_EINVAL and untouched([p])
        assert lib.vio_init_sfm_solve(s._h, None, 1, None) == abi.VIO_EINVAL
        assert lib.vio_init_sfm_solve(s._h, None, 0, None) == abi.VIO_OK
        h = C.c_void_p()
        assert lib.vio_init_sfm_create(1, abi.VIO_INIT_BA_MAX_FRAMES + 1, 10, 100, 1, C.byref(h)) == abi.VIO_ECAP
        s.kernel_ms()
        p = _problem(sc)                                                                  # the context still works
        s.solve([p])
        assert p.status == OK and s.device() >= 0
        ms, launches = s.kernel_ms()
        assert launches == 3 and all(m > 0 for m in ms)
    finally:
        s.close()
