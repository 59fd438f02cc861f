#!/usr/bin/env python3
"""Records the shape edges of the batched bundle adjustment (tests/test_init_ba.py) from the reference's solver stack
(oracle/_ref: vendored Ceres 1.12 + Eigen 3.3.0, ref_sfm_bundle_adjust of oracle/ref_sfm_harness.cpp) into
tests/golden/init_sfm_edges.npz. The cases are built the way test_initial_sfm.make_case builds its own (disturbed poses in
frame l's gauge, landmarks triangulated from them), with the frame set, the gauge frame, the observation lists and the
point_ok flags chosen per case. A case on which Ceres does not converge is not recorded. Run where oracle/_ref exists:
    make -C oracle ref && python tests/golden/make_init_sfm_edges_golden.py"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers as H
import test_initial_sfm as T
import test_initial_cpu as TC

OUT = os.path.join(ROOT, "tests", "golden", "init_sfm_edges.npz")
lib = H.ref_lib_or_none()
assert lib is not None and hasattr(lib, "ref_sfm_bundle_adjust"), "build oracle/_ref first"
lib.ref_sfm_triangulate_point.restype = None
tri = T.triangulate_with(lib.ref_sfm_triangulate_point)
synth = TC.synth


def build(seed, frames, l, n_points, rough=1.0, keep=None, ok_rule=None, n_ok=None, depth=1.0):
    """frames: the frames of an 11-frame scene that make up the window; keep(j, obs) -> the observations of landmark j that stay;
    ok_rule(j) -> point_ok of a landmark that could be triangulated; n_ok: at most that many point_ok landmarks; depth: factor on the
    triangulated landmarks (a start whose first Gauss-Newton-like step overshoots)."""
    sc = TC._scene(seed, n_points=n_points)
    rng = np.random.default_rng(5000 + seed)
    F = len(frames)
    Rl, pl = sc["Rwc"][frames[l]], sc["pwc"][frames[l]]
    s = 1.0 / np.linalg.norm(sc["pwc"][frames[F - 1]] - pl)
    cq, ct, P = np.zeros((F, 4)), np.zeros((F, 3)), np.zeros((F, 12))
    for k in range(F):
        Rcw = (Rl.T @ sc["Rwc"][frames[k]]).T
        tcw = -Rcw @ (Rl.T @ (sc["pwc"][frames[k]] - pl) * s)
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
        o = [(frames.index(k), x, y) for (k, x, y) in o if k in frames]
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
        if b > a and (ok_rule is None or ok_rule(j)) and (n_ok is None or ok.sum() < n_ok):
            pts[j] = depth * tri(P[fr[a]], P[fr[b]], xy[a], xy[b])
            ok[j] = 1
    return dict(F=F, l=l, cq=cq, ct=ct, pts=pts, ok=ok, start=start, fr=fr, xy=xy)


def record(out, name, c, want=None):
    r = T.run_ba(lib.ref_sfm_bundle_adjust, c, False)
    print("%-15s F %2d l %d points %3d/%3d obs %4d: iterations %2d termination %d ok/bad %d/%d flags[1] %d cost %.3e -> %.3e"
          % (name, c["F"], c["l"], int(c["ok"].sum()), len(c["ok"]), len(c["fr"]), r["iterations"], r["termination"], r["n_ok"], r["n_bad"],
             int(r["it_flags"][1]), r["initial_cost"], r["final_cost"]))
    if not (r["ok"] == 1 and r["termination"] == 1 and r["n_ok"] >= 3) or (want is not None and not want(r)):
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
    raise SystemExit("no candidate of %s converged on the reference" % name)


out = {}
seeds = range(60, 90)
first_of(out, "f3_l0", (build(s, [0, 5, 10], 0, 40) for s in seeds))
first_of(out, "f3_l1", (build(s, [0, 5, 10], 1, 40) for s in seeds))
# every second landmark keeps its first and last observation only. (With EVERY landmark cut to two observations the problem is
# nearly rank-deficient and amplifies rounding: init::bundle_adjust itself ends 1e-7 from Ceres there, iteration for iteration
# the same route. Such a problem says nothing about a kernel at the 1e-9 bar and is not recorded.)
first_of(out, "two_obs", (build(s, list(range(11)), 3, 90, keep=lambda j, o: [o[0], o[-1]] if len(o) >= 2 and j % 2 else o) for s in seeds))


def only_consts(l, F):
    return lambda j, o: [x for x in o if x[0] in (l, F - 1)] if j % 9 == 4 else o


first_of(out, "const_only", (build(s, list(range(11)), 2, 90, keep=only_consts(2, 11)) for s in seeds))
first_of(out, "interleaved", (build(s, list(range(11)), 1, 90, ok_rule=lambda j: j % 3 != 1) for s in seeds))
first_of(out, "np255", (build(s, [0, 3, 7, 10], 1, 300, n_ok=255) for s in seeds))
first_of(out, "np257", (build(s, [0, 3, 7, 10], 2, 300, n_ok=257) for s in seeds))
first_of(out, "first_rejected", (build(s, list(range(11)), 2, 60, rough=r, depth=d) for d in (0.5, 0.35, 2.0, 3.0) for r in (1.0, 3.0) for s in seeds),
         want=lambda r: int(r["it_flags"][1]) == 1)
refs = [k[:-len("_out_n_bad")] for k in out if k.endswith("_out_n_bad")]
assert any(int(out[n + "_out_n_bad"]) > 0 for n in refs), "no recorded case holds a rejected step"
assert any(np.any(out[n + "_in_ok"] == 0) for n in refs), "no recorded case holds point_ok = 0 entries"
np.savez_compressed(OUT, **out)
print("wrote", OUT, len(out), "arrays", os.path.getsize(OUT), "bytes")
