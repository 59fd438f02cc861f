#!/usr/bin/env python3
"""Records bundle adjustments of 17 to 32 frames (tests/test_init_ba_large.py: the large layout of the batched kernel, the
host solver beyond 11 frames) from the reference's solver stack (oracle/_ref: vendored Ceres 1.12 + Eigen 3.3.0,
ref_sfm_bundle_adjust of oracle/ref_sfm_harness.cpp) into tests/golden/init_sfm_large.npz. The cases are built the way
make_init_sfm_edges_golden.py builds its own: a scene of F frames, poses disturbed in frame l's gauge, landmarks triangulated
from them with the reference's triangulation.

A candidate is recorded only if the reference converges on it (termination 1, ok, at least three successful steps), if it
took under 150 ms (the harness stops Ceres after 0.3 s of wall time: a trace cut by that limit depends on the machine and
must never become a fixture), and if the relative decrease of every valid step lies at least 0.05 away from the 1e-3
threshold, so that no other summation order can flip an accept / reject decision. Run where oracle/_ref exists:
    make -C oracle ref && python tests/golden/make_init_sfm_large_golden.py"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as H
import test_initial_sfm as T
import test_initial_cpu as TC

OUT = os.path.join(ROOT, "tests", "golden", "init_sfm_large.npz")
MAX_SECONDS, RHO_MARGIN = 0.150, 0.05
lib = H.ref_lib_or_none()
assert lib is not None and hasattr(lib, "ref_sfm_bundle_adjust"), "build oracle/_ref first"
lib.ref_sfm_triangulate_point.restype = None
tri = T.triangulate_with(lib.ref_sfm_triangulate_point)
synth = TC.synth


def build(seed, F, l, n_points, rough=1.0, depth=1.0, n_ok=None, keep=None):
    """A scene of F frames; keep(j, obs) -> the observations of landmark j that stay; n_ok: at most that many point_ok
    landmarks; depth: factor on the triangulated landmarks."""
    sc = TC._scene(seed, n_frames=F, n_points=n_points)
    rng = np.random.default_rng(7000 + seed)
    Rl, pl = sc["Rwc"][l], sc["pwc"][l]
    far = F - 1 if l != F - 1 else 0            # (l = F - 1: the scale comes from the first frame instead of the last)
    s = 1.0 / np.linalg.norm(sc["pwc"][far] - pl)
    cq, ct, P = np.zeros((F, 4)), np.zeros((F, 3)), np.zeros((F, 12))
    for k in range(F):
        Rcw = (Rl.T @ sc["Rwc"][k]).T
        tcw = -Rcw @ (Rl.T @ (sc["pwc"][k] - pl) * s)
        if k != l:
            Rcw = synth.rotvec_to_rot(rng.normal(0, np.radians(1.0 * rough) / np.sqrt(3), 3)) @ Rcw
        if k != l and k != F - 1:
            tcw = tcw + rng.normal(0, 0.03 * rough, 3)
        q = synth.rot_to_quat(Rcw)
        cq[k] = (q[3], q[0], q[1], q[2])
        ct[k] = tcw
        P[k] = np.column_stack([Rcw, tcw]).ravel()
    start, fr, xy = [0], [], []
    for j, o in enumerate(sc["obs"]):
        if keep is not None:
            o = keep(j, o)
        for (k, x, y) in o:
            fr.append(k), xy.append((x, y))
        start.append(len(fr))
    start, fr, xy = np.array(start, np.int32), np.array(fr, np.int32), np.array(xy).reshape(-1, 2)
    n = len(sc["obs"])
    pts, ok = np.zeros((n, 3)), np.zeros(n, np.uint8)
    for j in range(n):
        a, b = start[j], start[j + 1] - 1
        if b > a and (n_ok is None or ok.sum() < n_ok):
            pts[j] = depth * tri(P[fr[a]], P[fr[b]], xy[a], xy[b])
            ok[j] = 1
    return dict(F=F, l=l, cq=cq, ct=ct, pts=pts, ok=ok, start=start, fr=fr, xy=xy)


def rho_margin(r):
    """Distance of the closest valid step's relative decrease from the accept threshold."""
    d = [abs(float(r["it_rho"][k]) - 1e-3) for k in range(1, int(r["iterations"])) if int(r["it_flags"][k]) & 1]
    return min(d) if d else np.inf


def record(out, name, c, want=None):
    t0 = time.perf_counter()
    r = T.run_ba(lib.ref_sfm_bundle_adjust, c, False)
    dt = time.perf_counter() - t0
    nobs = int(sum(c["start"][j + 1] - c["start"][j] for j in range(len(c["ok"])) if c["ok"][j]))
    print("%-10s F %2d l %2d points %3d/%3d obs %4d: %5.1f ms iterations %2d termination %d ok/bad %d/%d flags[1] %d rho margin %.3f cost %.3e -> %.3e"
          % (name, c["F"], c["l"], int(c["ok"].sum()), len(c["ok"]), nobs, 1e3 * dt, r["iterations"], r["termination"], r["n_ok"], r["n_bad"],
             int(r["it_flags"][1]), rho_margin(r), r["initial_cost"], r["final_cost"]))
    if not (r["ok"] == 1 and r["termination"] == 1 and r["n_ok"] >= 3 and dt < MAX_SECONDS and rho_margin(r) >= RHO_MARGIN):
        return False
    if want is not None and not want(c, r):
        return False
    for k, v in c.items():
        out["%s_in_%s" % (name, k)] = np.asarray(v)
    for k, v in r.items():
        out["%s_out_%s" % (name, k)] = np.asarray(v)
    return True


def first_of(out, name, candidates, want=None):
    for c in candidates:
        if record(out, name, c, want):
            return
    raise SystemExit("no candidate of %s qualified on the reference" % name)


def thinned(j, o):
    """A landmark keeps its first, its last and every second observation in between: 257 landmarks of 17 frames stay far
    under 4000 observations, and the file small."""
    return o if len(o) < 4 else o[:-1:2] + [o[-1]]


def short(c, r):
    """The emulator of the CPU tests runs 512 fibers per iteration of a 186-column problem: traces of at most 16 iterations."""
    return r["iterations"] <= 16


N_BIG = 60    # landmarks of the 31- and 32-frame cases: as many as keep the file the size of the other init_sfm fixtures
out = {}
seeds = range(60, 100)
first_of(out, "f17", (build(s, 17, 3, 60) for s in seeds))
first_of(out, "f21", (build(s, 21, 4, 90) for s in seeds), want=lambda c, r: r["n_bad"] > 0)
first_of(out, "f31", (build(s, 31, 5, N_BIG) for s in seeds), want=short)
# l = F - 1: one constant translation only, nc = 186. Wanted with a rejected first step: undisturbed depths give one on few
# seeds and then take longer than MAX_SECONDS, so the triangulated depths are scaled as for the edges' first_rejected.
first_of(out, "f32_last", (build(s, 32, 31, N_BIG, depth=d) for d in (1.0, 0.5, 0.35, 2.0, 3.0) for s in seeds),
         want=lambda c, r: int(r["it_flags"][1]) == 1 and short(c, r))
first_of(out, "f32_far", (build(s, 32, 6, N_BIG, rough=3.0, depth=0.5) for s in seeds), want=short)
first_of(out, "f17_np257", (build(s, 17, 3, 280, n_ok=257, keep=thinned) for s in seeds), want=lambda c, r: int(c["ok"].sum()) == 257)
names = [k[:-len("_out_n_bad")] for k in out if k.endswith("_out_n_bad")]
assert sum(int(out[n + "_out_n_bad"]) > 0 for n in names) >= 2, "fewer than two recorded cases hold a rejected step"
assert any(int(out[n + "_out_it_flags"][1]) == 1 for n in names), "no recorded case holds a rejected first step"
np.savez_compressed(OUT, **out)
print("wrote", OUT, len(out), "arrays", os.path.getsize(OUT), "bytes")
