"""findFundamentalMat on its rare paths. fundamental_ransac_block (csrc/fe_ransac.h) restates the sequential
RANSAC / LMedS registrators with speculation (rounds of 8, 16, 16, ... hypotheses, subsets drawn as if checkSubset
passed, a multiply-high modulo, a 16-lane elimination); the named inputs of ransac_cases.py each force one of the paths
that restatement can get wrong, and the oracle's trace (OracleRansacTrace) proves which path a case took.

CPU part: the trace assertions, the oracle's own 7-point solver against a 50-digit reference, and the margin that keeps
the adaptive iteration bound independent of the device's pow / log.
GPU part: every case, byte for byte, through vio_fundamental_ransac and through track_update_kernel (all three CAP
instantiations, with and without the publish pass). ransac_batch_kernel calls the same block routine and is reachable
only through the loop detector; its tests are in test_loop_detector.py."""
import numpy as np
import pytest

import helpers as H
import ransac_cases as RC
from helpers import abi, pkg

CFG = RC.CFG


@pytest.fixture(scope="module")
def traces():
    return {name: H.oracle_ransac_trace(CFG, p1, p2) for name, (p1, p2) in RC.CASES.items()}


def bits(mask, lo, hi):
    return bin((mask >> lo) & ((1 << (hi - lo)) - 1)).count("1")


# ---- the trace: every case takes the path it is named for ---------------------------------------------------------
def test_trace_does_not_change_the_result(traces):
    for name, (p1, p2) in RC.CASES.items():
        assert np.array_equal(traces[name][0], H.oracle_ransac(CFG, p1, p2)), name


def test_lattice_redraws_in_three_rounds(traces):
    m, t = traces["lattice"]
    assert t["lmeds"] == 0 and t["iterations"] > 24 and t["subset_failed"] == 0
    rm = t["redraw_mask"]
    assert t["first_redraw_iteration"] == 0 and rm & 1             # the speculative draw is wrong from the first subset on
    assert bits(rm, 1, 8) >= 2                                      # again inside the first round of 8
    assert bits(rm, 8, 24) >= 2 and bits(rm, 24, 40) >= 1           # and in the rounds of 16 after it
    assert t["niters_lowered"] >= 2 and 7 < m.sum() < len(m)


def test_lattice_no_geometry_follows_the_subset_sequence(traces):
    m, t = traces["lattice_no_geometry"]
    assert t["iterations"] == 1000 and t["subset_redraws"] > 1000 and bits(t["redraw_mask"], 0, 64) >= 24
    assert t["first_redraw_iteration"] < 8 and 8 <= m.sum() <= 11


def test_late_better_hides_a_better_model_behind_the_end_of_the_scan(traces):
    """With a confidence close to 1 the same subsets are scanned further: the model the sequential run at 0.99 never sees
    is the next hypothesis of the same round of 8."""
    m, t = traces["late_better"]
    k = t["iterations"]
    assert 1 < k < 8 and t["last_best_iteration"] < k - 1
    sure = abi.default_config()
    sure.f_confidence = 0.9999999
    m2, t2 = H.oracle_ransac_trace(sure, *RC.CASES["late_better"])
    assert k <= t2["last_best_iteration"] < 8 and t2["max_good"] > t["max_good"] and not np.array_equal(m, m2)


def test_many_to_one_is_reported_collinear(traces):
    m, t = traces["many_to_one_6"]   # seven points out of six values: every subset holds two equal points
    assert len(np.unique(RC.CASES["many_to_one_6"][1], axis=0)) == 6
    assert t["subset_failed"] == 1 and t["subset_failed_iteration"] == 0 and t["subset_redraws"] == 10000 and m.all()
    m, t = traces["many_to_one_9"]
    assert len(np.unique(RC.CASES["many_to_one_9"][1], axis=0)) == 9
    assert t["subset_failed"] == 0 and t["iterations"] == 1000 and t["subset_redraws"] > 10 * t["iterations"]
    assert bits(t["redraw_mask"], 0, 64) >= 48                      # (nearly) every hypothesis of every round is redrawn
    assert 7 < m.sum() < len(m)
    for name in ("many_to_one_6", "many_to_one_9"):   # the other way round (equal points in image 1), as the tracker test feeds them
        p1, p2 = RC.CASES[name]
        t2 = H.oracle_ransac_trace(CFG, p2, p1)[1]
        assert t2["subset_redraws"] == traces[name][1]["subset_redraws"] and t2["subset_failed"] == traces[name][1]["subset_failed"]


def test_line_fails_at_the_first_subset(traces):
    m, t = traces["line"]
    assert t["subset_failed"] == 1 and t["subset_failed_iteration"] == 0 and t["iterations"] == 0 and m.all()


@pytest.mark.parametrize("n", RC.NO_GEOMETRY_N)
def test_no_geometry_runs_long(traces, n):
    m, t = traces["no_geometry_%d" % n]
    assert t["lmeds"] == 0 and t["iterations"] >= 300 and t["subset_redraws"] == 0   # tens of rounds
    assert t["best_updates"] >= 2 and 8 <= m.sum() <= 11
    # the bound only moves below 1000 when more than 0.517 n pairs agree (0.517^7 = 1 - 0.01^(1/1000)): with 8..11 chance
    # inliers that is n = 15 alone, where it is lowered twice; from n = 20 on the call runs its full 1000 hypotheses
    if n == 15:
        assert t["niters_lowered"] >= 2 and t["niters"] < 1000
    else:
        assert t["iterations"] == 1000


@pytest.mark.parametrize("k", RC.BOUNDARY_K)
def test_boundary_ends_at_k(traces, k):
    m, t = traces["boundary_%d" % k]
    assert t["lmeds"] == 0 and t["iterations"] == k and t["niters_lowered"] >= 1 and 7 < m.sum() < len(m)


def test_boundary_covers_both_ways_a_scan_ends(traces):
    """The scan ends either because the bound was already k when hypothesis k came up, or because hypothesis k - 1 itself
    lowered the bound to k or less; both happen at a round's last hypothesis and at the first one of the next round."""
    by_update = {k for k in RC.BOUNDARY_K if traces["boundary_%d" % k][1]["last_best_iteration"] == k - 1}
    assert by_update & {8, 24, 40} and by_update & {7, 9, 23, 25, 39, 41}
    assert set(RC.BOUNDARY_K) - by_update


def test_every_count_spans_lmeds_and_ransac():
    seen = set()
    for n in (8, 9, 13, 14, 15, 16, 320, 4099):
        p1, p2 = RC.every_count(n)
        m, t = H.oracle_ransac_trace(CFG, p1, p2)
        assert t["lmeds"] == (n < 15) and t["iterations"] > 0 and 7 <= m.sum() <= n
        seen.add((t["lmeds"], n & 1))
    assert len(seen) == 4 and RC.EVERY_COUNT_N[:313] == tuple(range(8, 321)) and RC.EVERY_COUNT_N[313:] == (511, 512, 513, 1000, 4099)


def test_static_and_shift_reach_the_degenerate_solver_branches(traces):
    for name in ("static", "static_12"):
        m, t = traces[name]
        assert t["zero_pivots"] == t["iterations"] == t["cubic_none"] > 0 and t["models"] == 0 and m.all()
    m, t = traces["static_perturbed"]    # RANSAC sizes: quadratic, 0 = 0 and F[8] = 0 models within 16 hypotheses
    assert t["lmeds"] == 0 and t["cubic_quadratic"] > 0 and t["cubic_none"] > 0 and t["models_f8_zero"] > 0 and t["iterations"] > 8
    m, t = traces["shift"]
    assert t["lmeds"] == 0 and m.all()
    for name in ("shift_9", "shift_14"):  # LMedS sizes (both median parities) scan all 300 hypotheses
        m, t = traces[name]
        assert t["lmeds"] == 1 and t["iterations"] == 300 and t["cubic_quadratic"] > 0


def test_zoom_reaches_nan_errors(traces):
    m, t = traces["zoom_about_a_point"]
    p1, p2 = RC.CASES["zoom_about_a_point"]
    assert t["lmeds"] == 0 and m.all() and (p1 == p2).all(axis=1).sum() == 1   # the centre is one of the pairs
    assert t["nan_errors"] == 0   # (RANSAC accepts the first model of a homography: the centre's error is 0 / finite there)
    for n in (10, 11, 13, 14):
        m, t = traces["zoom_small_%d" % n]
        assert t["lmeds"] == 1 and len(m) == n and t["iterations"] == 300
        assert t["nan_errors"] > 0 and t["models_f8_zero"] > 0 and t["cubic_quadratic"] > 0
        # the device returns a NaN error with the sign bit set: that is only right while the host never makes another
        assert t["nan_errors_positive"] == 0
    assert traces["zoom_small_14"][1]["nan_errors"] == 1            # a single NaN among 14 errors: its place in the sort
    assert traces["zoom_small_10"][1]["nan_errors"] % 10 == 0       # whole models of NaN (0 / 0 roots of the quadratic)
    assert traces["zoom_small_11"][1]["cubic_linear"] > 0 and traces["zoom_small_13"][1]["cubic_linear"] > 0


def test_extremes(traces):
    for kind in ("large", "negative", "subpixel"):
        m, t = traces["extremes_" + kind]
        assert t["iterations"] >= 1 and t["best_updates"] >= 1 and 7 < m.sum() <= len(m)
    assert RC.CASES["extremes_large"][0].min() > 1e4 and RC.CASES["extremes_negative"][0].max() < 0
    p1, p2 = RC.CASES["extremes_subpixel"]
    d = np.abs(p2 - p1)
    assert d.max() < 0.05 and (d * 1024 == np.round(d * 1024)).all() and d.max() > 0


def test_union_reaches_every_counter(traces):
    total = {}
    for _, t in traces.values():
        for k, v in t.items():
            total[k] = total.get(k, 0) + (v if k not in ("first_redraw_iteration", "subset_failed_iteration", "last_best_iteration")
                                          else (v >= 0))
    # nan_errors_positive must stay 0 (see test_zoom_reaches_nan_errors); everything else is reached, all five branches of
    # the cubic included
    for k, v in total.items():
        assert (v == 0) if k == "nan_errors_positive" else (v > 0), k


# ---- the oracle's 7-point solver against 50 digits --------------------------------------------------------------
# Worst deviation of oracle_run7point from the 50-digit models over the kept subsets, as measured: 5.43e-13 (unit
# Frobenius norm, sign aligned); the worst of x2' F x1 / (|x2| |F| |x1|) and det F / |F|^3 is 1.04e-18. The conditioning of
# the 7x9 null space and of the cubic's roots differs by orders of magnitude between subsets, hence 10 times the worst.
SOLVER_TOL = 5.43e-12
N_SUBSETS = 200


def reference_7point(mp, ms1, ms2):
    """-> (list of 3x3 real models of unit norm, separation of the cubic's roots) at 50 digits: null space of the 7x9
    system by SVD, roots of det(l F1 + (1 - l) F2). The separation is the smallest distance between two of the three
    complex roots relative to their size: it vanishes with the discriminant, and the number of real roots is ill-posed
    where it does."""
    A = mp.matrix(7, 9)
    for i in range(7):
        x0, y0, x1, y1 = (mp.mpf(float(v)) for v in (ms1[i, 0], ms1[i, 1], ms2[i, 0], ms2[i, 1]))
        for j, v in enumerate((x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, mp.mpf(1))):
            A[i, j] = v
    _, _, V = mp.svd_r(A, full_matrices=True, compute_uv=True)
    F1, F2 = mp.matrix(3, 3), mp.matrix(3, 3)
    for j in range(9):
        F1[j // 3, j % 3], F2[j // 3, j % 3] = V[7, j], V[8, j]
    # det(l F1 + (1 - l) F2) is a cubic in l: interpolate it through four points
    xs = [mp.mpf(-1), mp.mpf(0), mp.mpf(1), mp.mpf(2)]
    ys = [mp.det(x * F1 + (1 - x) * F2) for x in xs]
    Vm = mp.matrix([[x ** 3, x ** 2, x, 1] for x in xs])
    a, b, c, d = mp.lu_solve(Vm, mp.matrix(ys))
    roots = mp.polyroots([a, b, c, d], maxsteps=200, extraprec=100)
    sep = min(abs(roots[i] - roots[j]) for i, j in ((0, 1), (0, 2), (1, 2))) / (1 + max(abs(r) for r in roots))
    models = []
    for r in roots:
        if abs(mp.im(r)) > mp.mpf(10) ** -30 * (1 + abs(r)):
            continue
        F = mp.re(r) * F1 + (1 - mp.re(r)) * F2
        M = np.array([[float(F[i, j]) for j in range(3)] for i in range(3)])
        models.append(M / np.linalg.norm(M))
    return models, float(sep)


def test_run7point_against_50_digits():
    from mpmath import mp
    mp.dps = 50
    rng = np.random.default_rng(2024)
    worst, worst_res, set_aside = 0.0, 0.0, 0
    for _ in range(N_SUBSETS):
        ms1 = rng.uniform([0, 0], [480, 640], (7, 2)).astype(np.float32)
        ms2 = rng.uniform([0, 0], [480, 640], (7, 2)).astype(np.float32)
        ref, sep = reference_7point(mp, ms1, ms2)
        if sep < 1e-4:            # the number of real roots is ill-posed: two of them (nearly) coincide
            set_aside += 1
            continue
        got = H.oracle_run7point(ms1, ms2)
        assert len(got) == len(ref) and len(got) in (1, 3)
        h1, h2 = np.column_stack([ms1, np.ones(7)]).astype(float), np.column_stack([ms2, np.ones(7)]).astype(float)
        for F in got:
            F = F / np.linalg.norm(F)
            dev = min(min(np.linalg.norm(F - R), np.linalg.norm(F + R)) for R in ref)
            worst = max(worst, dev)
            res = np.abs(np.einsum("ij,jk,ik->i", h2, F, h1)) / (np.linalg.norm(h1, axis=1) * np.linalg.norm(h2, axis=1))
            worst_res = max(worst_res, res.max(), abs(np.linalg.det(F)))
            assert dev < SOLVER_TOL and res.max() < SOLVER_TOL and abs(np.linalg.det(F)) < SOLVER_TOL
        # every reference model is found, none twice
        for R in ref:
            assert sum(min(np.linalg.norm(F / np.linalg.norm(F) - R), np.linalg.norm(F / np.linalg.norm(F) + R)) < SOLVER_TOL
                       for F in got) >= 1
    print("run7point: worst deviation %.3g, worst residual %.3g, %d of %d set aside" % (worst, worst_res, set_aside, N_SUBSETS))
    assert set_aside <= N_SUBSETS // 10


# ---- the adaptive bound --------------------------------------------------------------------------------------------
def test_adaptive_bound_is_far_from_a_rounding_tie():
    """RANSACUpdateNumIters rounds log(1 - p) / log(1 - (good / count)^7) to the nearest integer. The device's pow and
    log differ from the host's by a few ulp (1e-14 of a quotient below 1000), so the rounded bound is the same on both as
    long as the quotient stays away from a half-integer: here by more than 1e-9 for every count in 15..4099 and every
    good in 7..count. Quotients of 1000 and more are never rounded (the function returns its max_iters argument, at
    most 1000, when the quotient is not below it), and neither is good == count (returns 0). A quotient within rounding of
    the current bound itself gives that bound on either branch."""
    closest = (1.0, 0, 0)
    num = np.log(1.0 - 0.99)
    for count in range(15, 4100):
        good = np.arange(7, count, dtype=np.float64)
        ep = (count - good) / count
        denom = 1.0 - np.power(1.0 - ep, 7)
        with np.errstate(divide="ignore"):
            q = num / np.log(denom)   # (denom rounds to 1 for the smallest good / count: log 0 -> the quotient is -inf)
        dist = np.where(np.isfinite(q) & (q < 1001.0), np.abs(q - np.floor(q) - 0.5), 1.0)
        i = int(np.argmin(dist))
        if dist[i] < closest[0]:
            closest = (float(dist[i]), count, i + 7)
    print("adaptive bound: closest to a half-integer %.3g at (count, good) = (%d, %d)" % closest)
    assert closest[0] > 1e-9


# ---- the device ----------------------------------------------------------------------------------------------------
def _fe():
    return pkg.frontend


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_case_on_device(name):
    p1, p2 = RC.CASES[name]
    got, ref = _fe().fundamental_ransac(CFG, p1, p2), H.oracle_ransac(CFG, p1, p2)
    assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes()


@pytest.mark.gpu
def test_every_count_on_device():
    """The multiply-high modulo at every divisor 8..320 and a few beyond, both median parities of LMedS."""
    bad = []
    for n in RC.EVERY_COUNT_N:
        p1, p2 = RC.every_count(n)
        if _fe().fundamental_ransac(CFG, p1, p2).tobytes() != H.oracle_ransac(CFG, p1, p2).tobytes():
            bad.append(n)
    assert bad == []


TRACK_CASES = ("lattice", "many_to_one_6", "many_to_one_9", "line", "no_geometry_30", "no_geometry_150", "boundary_8",
               "boundary_24", "boundary_40")


def track_inputs(name):
    """cur -> forw of a case. setMask keeps one point per pixel neighbourhood even at MIN_DIST 1, so where image 2 holds
    equal points (many_to_one) the pair is fed the other way round: the equal points are then cur's, forw is spread."""
    cur, forw = RC.CASES[name]
    if name.startswith("many_to_one"):
        cur, forw = forw, cur
    return cur, forw


def test_track_inputs_are_spread():
    cfg = abi.default_config(max_corners=150, min_dist=1)
    for name in TRACK_CASES:
        cur, forw = track_inputs(name)
        r = np.rint(forw).astype(int)
        assert (r[:, 0] >= 1).all() and (r[:, 0] < cfg.image_cols - 1).all() and (r[:, 1] >= 1).all() and (r[:, 1] < cfg.image_rows - 1).all()
        d = np.abs(r[:, None, :] - r[None, :, :]).max(axis=2) + 10 * np.eye(len(r), dtype=int)
        assert d.min() >= 2, name   # no two forw points inside one another's filled circle of radius 1
        assert len(cur) <= 150


@pytest.mark.gpu
@pytest.mark.parametrize("name", TRACK_CASES)
def test_case_through_track_update(name):
    """The same routine inside track_update_kernel: points come from LDS (PackedPts), RansacShared sits elsewhere in LDS
    for each of the three CAP instantiations (max_corners 150, 256, 300), once without and once with the publish pass
    (a second F-test, over pre -> forw, on the survivors of the first)."""
    from test_track_update_gpu import assert_same, run_both
    cur, forw = track_inputs(name)
    n = len(cur)
    ids, cnt = np.arange(500, 500 + n), np.full(n, 2)
    ref_mask = H.oracle_ransac(CFG, cur, forw)
    for cap in (150, 256, 300):
        cfg = abi.default_config(max_corners=cap, min_dist=1)
        for publish in (0, 1):
            g, r = run_both(cfg, cur, cur, forw, ids, cnt, np.ones(n, np.uint8), publish=bool(publish))
            assert_same(g, r)
            if not publish:   # nothing but the first F-test removes a track here
                assert g[1].tolist() == ids[ref_mask != 0].tolist()
