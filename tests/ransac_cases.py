"""Named inputs of findFundamentalMat, one for every rare path of the device routine (fundamental_ransac_block restates a
strictly sequential algorithm with speculation: rounds of 8, 16, 16, ... hypotheses, subsets drawn as if checkSubset
always passed, a multiply-high modulo, a 16-lane elimination). Every case is a deterministic (name, p1, p2) in float32,
generated here; which path a case takes is asserted from the oracle's trace in test_ransac_paths.py, so a case that
stops taking its path fails there instead of silently testing something else.

    CASES[name] -> (p1, p2)          everything except every_count
    EVERY_COUNT_N, every_count(n)    one scene cut to n pairs
    BOUNDARY_K                       the hypothesis counts the boundary_k cases end at
"""
import numpy as np

import helpers as H
from helpers import abi

CFG = abi.default_config()


def _f32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 2)


def two_view(rng, n, shift, n_out=0, out_lo=8.0, out_hi=40.0):
    """n points of a 3D scene seen from two camera positions; the first n_out pairs of a fixed permutation are gross
    outliers (image 2 moved by out_lo..out_hi px)."""
    z = rng.uniform(3, 9, n)
    x = rng.uniform(-0.35, 0.35, n) * z
    y = rng.uniform(-0.5, 0.5, n) * z
    a = np.column_stack([CFG.fx * x / z + CFG.cx, CFG.fy * y / z + CFG.cy])
    b = np.column_stack([CFG.fx * (x - shift[0]) / (z - shift[2]) + CFG.cx, CFG.fy * (y - shift[1]) / (z - shift[2]) + CFG.cy])
    bad = rng.permutation(n)[:n_out]
    b[bad] += rng.uniform(out_lo, out_hi, (n_out, 2)) * rng.choice([-1.0, 1.0], (n_out, 2))
    return _f32(a), _f32(b)


def _lattice(seed=94):
    """6x5 integer lattice, parallax along x that depends on a per-point depth, then 26 gross outliers: many 7-subsets of
    a lattice hold three points of one row, column or diagonal, so checkSubset throws them away. (The seed is one at
    which the oracle redraws at hypothesis 0, again inside the first round of 8 and in the second and third rounds.)"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(6), np.arange(5))
    p1 = np.column_stack([60.0 + 60.0 * gx.ravel(), 100.0 + 90.0 * gy.ravel()])
    depth = rng.uniform(2.0, 8.0, len(p1))
    p2 = p1 + np.column_stack([48.0 / depth, np.zeros(len(p1))])
    o1 = rng.uniform(30, 450, (26, 2))
    o2 = rng.uniform(30, 450, (26, 2))
    order = rng.permutation(len(p1) + 26)
    return _f32(np.vstack([p1, o1])[order]), _f32(np.vstack([p2, o2])[order])


def _lattice_no_geometry():
    """A 6x6 lattice in image 1 against independent uniform points in image 2: redraws in (nearly) every round of a call
    that runs its full 1000 hypotheses, and a winner with 8..10 chance inliers, so the mask follows the exact sequence
    of subsets (a lattice with a real geometry gives the same mask from almost any sequence)."""
    rng = np.random.default_rng(1)
    gx, gy = np.meshgrid(np.arange(6), np.arange(6))
    p1 = np.column_stack([60.0 + 60.0 * gx.ravel(), 60.0 + 90.0 * gy.ravel()])[rng.permutation(36)]
    return _f32(p1), _f32(rng.uniform([10, 10], [470, 630], (36, 2)))


def _late_better():
    """A scene whose scan ends at hypothesis 5, inside the first round, while hypothesis 5 itself (drawn, solved and
    scored with the round, but never scanned by the sequential algorithm) has more inliers than the winner."""
    return two_view(np.random.default_rng(9000 + 1771), 40, (0.25, 0.05, 0.1), n_out=3)


def _many_to_one(distinct):
    """40 current points matched to `distinct` old points (the loop path's searchByDes does that): equal points, which
    haveCollinearPoints reports through its zero differences."""
    rng = np.random.default_rng(100 + distinct)
    p1, p2 = two_view(rng, 40, (0.3, 0.05, 0.1))
    return p1, _f32(p2[rng.integers(0, distinct, 40) if distinct < 40 else np.arange(40)])


def _line():
    i = np.arange(20.0)
    p1 = np.column_stack([40.0 + 17.0 * i, 60.0 + 23.0 * i])
    p2 = np.column_stack([44.0 + 17.0 * i + 0.25 * i * i, 60.0 + 23.0 * i])
    return _f32(p1), _f32(p2)


def _no_geometry(n):
    rng = np.random.default_rng(1000 + n)
    return _f32(rng.uniform([10, 10], [470, 630], (n, 2))), _f32(rng.uniform([10, 10], [470, 630], (n, 2)))


def _static(n=40):
    """p2 == p1 (a still camera): the columns x2 y1 and y2 x1 of the 7x9 system are equal, so the elimination meets an
    exact zero pivot, the null space is not the one run7Point expects and every cubic is 0 = 0: no model at all."""
    rng = np.random.default_rng(7)
    p1 = _f32(rng.uniform([10, 10], [460, 630], (n, 2)))
    return p1, p1.copy()


def _shift(n=40):
    """p2 == p1 + (2, 0) on whole pixels: a homography, so every subset's system has rank 6 in exact arithmetic."""
    rng = np.random.default_rng(8)
    p1 = np.unique(rng.integers(3, 110, (n + 8, 2)) * 4.0, axis=0)
    p1 = p1[rng.permutation(len(p1))][:n]
    return _f32(p1), _f32(p1 + [2.0, 0.0])


def _static_perturbed(seed=0):
    """Whole-pixel points, two thirds of them still and every third moved by up to 3 px: subsets with many still points
    give cubics whose leading coefficients vanish exactly."""
    rng = np.random.default_rng(seed)
    p1 = np.unique(rng.integers(0, 64, (40, 2)) * 4.0, axis=0)
    p1 = p1[rng.permutation(len(p1))]
    p2 = p1.copy()
    p2[::3] += rng.integers(-3, 4, (len(p2[::3]), 2))
    return _f32(p1), _f32(p2)


def _zoom_small(seed, n, n_out):
    """LMedS sizes of the zoom: n pairs p2 = c + 2 (p1 - c) on power-of-two offsets from c, and n_out pairs whose
    image-2 point is c itself. A model whose epipole is exactly c has the error max(0 * inf, .) = NaN there."""
    rng = np.random.default_rng(seed)
    c = np.array([128.0, 128.0])
    p1 = np.unique(c + rng.choice([-1.0, 1.0], (n, 2)) * 2.0 ** rng.integers(0, 7, (n, 2)), axis=0)
    o1 = c + rng.choice([-1.0, 1.0], (n_out, 2)) * 2.0 ** rng.integers(0, 7, (n_out, 2))
    a, b = np.vstack([p1, o1]), np.vstack([c + 2.0 * (p1 - c), np.tile(c, (n_out, 1))])
    order = rng.permutation(len(a))
    return _f32(a[order]), _f32(b[order])


def _zoom_about_a_point():
    """p2 = c + 2 (p1 - c) on power-of-two coordinates, c itself one of the pairs: every F of this map has both epipoles
    on c, and the arithmetic is exact enough for the epipolar line through c to vanish exactly (0 * inf)."""
    rng = np.random.default_rng(3)
    c = np.array([128.0, 256.0])
    e = rng.integers(0, 7, (24, 2))
    s = rng.choice([-1.0, 1.0], (24, 2))
    p1 = c + s * 2.0 ** e
    p1 = np.unique(p1, axis=0)
    p1 = p1[rng.permutation(len(p1))]
    p1 = np.vstack([p1[:5], c, p1[5:]])
    return _f32(p1), _f32(c + 2.0 * (p1 - c))


def _extremes(kind):
    rng = np.random.default_rng(17)
    p1, p2 = two_view(rng, 60, (0.25, 0.05, 0.1), n_out=12)
    if kind == "large":
        return _f32(p1 + np.float32([1.0e4, 1.2e4])), _f32(p2 + np.float32([1.0e4, 1.2e4]))
    if kind == "negative":
        return _f32(p1 - np.float32([700, 900])), _f32(p2 - np.float32([700, 900]))
    q = np.round(p1)   # whole pixels, motion of a few 2^-10 px
    return _f32(q), _f32(q + np.round((p2 - p1) * 0.25) * 2.0 ** -10)


BOUNDARY_K = (7, 8, 9, 23, 24, 25, 39, 40, 41)


def _boundary_search():
    """two_view scenes whose outlier count and seed are searched with the oracle's trace until the run ends after
    exactly k hypotheses: the last of a round, the first of the next and their neighbours (rounds of 8, 16, 16)."""
    want, found = set(BOUNDARY_K), {}
    for seed in range(400):
        for n_out in range(2, 17):
            p1, p2 = two_view(np.random.default_rng(5000 + 17 * seed + n_out), 40, (0.25, 0.05, 0.1), n_out=n_out)
            k = H.oracle_ransac_trace(CFG, p1, p2)[1]["iterations"]
            if k in want and k not in found:
                found[k] = (p1, p2)
                if len(found) == len(want):
                    return found
    raise RuntimeError("boundary_k: no scene found for iterations in %s" % sorted(want - set(found)))


CASES = {
    "lattice": _lattice(),
    "lattice_no_geometry": _lattice_no_geometry(),
    "late_better": _late_better(),
    "many_to_one_6": _many_to_one(6),
    "many_to_one_9": _many_to_one(9),
    "line": _line(),
    "static": _static(40),
    "static_12": _static(12),
    "static_perturbed": _static_perturbed(),
    "shift": _shift(40),
    "shift_9": _shift(9),
    "shift_14": _shift(14),
    "zoom_about_a_point": _zoom_about_a_point(),
    "zoom_small_10": _zoom_small(273, 9, 1),
    "zoom_small_11": _zoom_small(119, 9, 2),
    "zoom_small_13": _zoom_small(112, 12, 1),
    "zoom_small_14": _zoom_small(169, 12, 2),
    "extremes_large": _extremes("large"),
    "extremes_negative": _extremes("negative"),
    "extremes_subpixel": _extremes("subpixel"),
}
NO_GEOMETRY_N = (15, 20, 30, 60, 150)
for _n in NO_GEOMETRY_N:
    CASES["no_geometry_%d" % _n] = _no_geometry(_n)
for _k, _v in sorted(_boundary_search().items()):
    CASES["boundary_%d" % _k] = _v

EVERY_COUNT_N = tuple(range(8, 321)) + (511, 512, 513, 1000, 4099)
_EVERY = two_view(np.random.default_rng(23), 4099, (0.25, 0.05, 0.1), n_out=4099 // 5)


def every_count(n):
    return _EVERY[0][:n], _EVERY[1][:n]
