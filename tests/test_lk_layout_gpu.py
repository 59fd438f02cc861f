"""lk_track_kernel after the change of its window layout (lk_layout.h: which lane owns which window pixel, the LDS row strides)
and with its error pass behind a template parameter: bit-exact against the CPU oracle, on images where every window pixel
carries its own value, at the image borders and corners (the border staging path at every level), with J staged again inside a
level, and through the tracker's step path (the kernel variant without the error pass)."""
import numpy as np
import pytest

import helpers as H
from helpers import abi, synth, pkg

pytestmark = pytest.mark.gpu
fe = pkg.frontend

ROWS, COLS = 120, 160


def texture_pair(seed, rows, cols, dx, dy):
    """Smoothed noise (structures about ten pixels wide, which LK can follow) plus fine per-pixel noise, so that no two window
    pixels are alike; the second frame is the same field moved by (dx, dy), sampled bilinearly. A flat square sits in both."""
    rng = np.random.default_rng(seed)
    pad = 16
    f = rng.uniform(0.0, 1.0, (rows + 2 * pad, cols + 2 * pad))
    fine = f.copy()
    k = np.ones(9) / 9
    for _ in range(3):
        f = np.apply_along_axis(np.convolve, 0, f, k, "same")
        f = np.apply_along_axis(np.convolve, 1, f, k, "same")
    core = f[pad:-pad, pad:-pad]
    f = np.clip((f - core.min()) / (core.max() - core.min()) * 215.0 + 40.0 * fine, 0, 255)

    def sample(oy, ox):
        iy, ix = int(np.floor(oy)), int(np.floor(ox))
        b, a = oy - iy, ox - ix

        def w(y, x):
            return f[pad + y:pad + y + rows, pad + x:pad + x + cols]
        return (1 - b) * ((1 - a) * w(iy, ix) + a * w(iy, ix + 1)) + b * ((1 - a) * w(iy + 1, ix) + a * w(iy + 1, ix + 1))
    img0, img1 = np.rint(sample(0, 0)).astype(np.uint8), np.rint(sample(-dy, -dx)).astype(np.uint8)
    for im in (img0, img1):
        im[FLAT[1] - 20:FLAT[1] + 20, FLAT[0] - 20:FLAT[0] + 20] = 128
    return np.ascontiguousarray(img0), np.ascontiguousarray(img1)


FLAT = (60, 60)  # (x, y) centre of the flat square: the 21 x 21 window and its Scharr halo see one value


def points(rows, cols):
    """48 sub-pixel starts at 160 x 120 (fewer on a narrower image): a grid over the interior, two within 12 px of each border, one within 12 px of both borders at
    each corner, one outside the image, one in the flat square."""
    rng = np.random.default_rng(5)
    gy, gx = np.meshgrid(np.linspace(16, rows - 17, 5), np.linspace(16, cols - 17, 6), indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-0.5, 0.5, (30, 2))
    grid = grid[np.abs(grid - np.array(FLAT)).max(1) > 34]  # (clear of the flat square: window + 3 px of motion)
    w, h = cols - 1.0, rows - 1.0
    border = [[1.3, 40.6], [9.7, 88.2], [w - 2.4, 33.3], [w - 11.2, 97.8],       # left, right
              [47.5, 0.4], [120.1, 10.9], [52.8, h - 0.7], [131.6, h - 11.4],    # top, bottom
              [3.2, 4.7], [w - 5.6, 2.1], [6.9, h - 3.3], [w - 1.8, h - 7.5]]    # corners
    more = [[100.25, 30.5], [110.75, 70.125], [30.5, 100.875], [140.375, 60.625], [90.0, 50.0], [100.5, 95.5]]
    special = [[-30.0, 50.0], [float(FLAT[0]) + 0.3, float(FLAT[1]) - 0.2]]
    extra = rng.uniform([14, 14], [cols - 15, rows - 15], (48, 2))
    extra = extra[np.abs(extra - np.array(FLAT)).max(1) > 34]
    pts = np.vstack([grid, border, more, special])
    pts = np.vstack([pts, extra[:48 - len(pts)]])
    pts = pts[(pts[:, 0] < cols + 20) & (pts[:, 1] < rows + 20)]
    return np.ascontiguousarray(pts, np.float32)


def check_klt(cfg, img0, img1, pts):
    got, gst, gerr = fe.klt_track(cfg, img0, img1, pts)
    ref, rst, rerr = H.oracle_klt(cfg, img0, img1, pts)
    assert np.array_equal(gst, rst), np.flatnonzero(gst != rst)
    ok = rst > 0
    assert np.array_equal(got[ok], ref[ok]), np.abs(got[ok] - ref[ok]).max()
    assert np.array_equal(gerr[ok], rerr[ok])
    return ref, rst


def test_klt_noise_texture_borders_and_corners():
    """The single-call entry (the kernel WITH the error pass): pts, status and err."""
    img0, img1 = texture_pair(11, ROWS, COLS, 0.6, 1.4)
    cfg = abi.default_config(max_corners=64, min_dist=8, image_rows=ROWS, image_cols=COLS)
    pts = points(ROWS, COLS)
    assert len(pts) == 48
    ref, rst = check_klt(cfg, img0, img1, pts)
    assert rst.sum() >= 36
    out, flat = np.flatnonzero(pts[:, 0] < 0)[0], np.flatnonzero((pts == np.float32([FLAT[0] + 0.3, FLAT[1] - 0.2])).all(1))[0]
    assert rst[out] == 0 and rst[flat] == 0
    near = (np.minimum(pts[:, 0], COLS - 1 - pts[:, 0]) < 12) | (np.minimum(pts[:, 1], ROWS - 1 - pts[:, 1]) < 12)
    near &= pts[:, 0] >= 0
    assert near.sum() >= 12 and rst[near].sum() >= 6   # the border staging path is taken and its results are compared
    inner = (rst > 0) & ~near
    assert np.abs(ref[inner] - pts[inner] - np.float32([0.6, 1.4])).max() < 0.5   # the oracle follows the motion


@pytest.mark.parametrize("rows,cols,lk_levels,shift", [
    (120, 96, 3, (5.3, -2.2)),    # two levels hold a 21 x 21 window: 2.6 px at the top level, the rest at level 0
    (120, 160, 0, (5.4, -3.6)),   # one level: all of the shift inside level 0, past the 3 px margin of the staged J region
])
def test_klt_shift_stages_j_again_inside_a_level(rows, cols, lk_levels, shift):
    img0, img1 = texture_pair(11, rows, cols, *shift)
    cfg = abi.default_config(max_corners=64, min_dist=8, image_rows=rows, image_cols=cols, lk_levels=lk_levels)
    pts = points(rows, cols)
    assert len(pts) >= 40
    ref, rst = check_klt(cfg, img0, img1, pts)
    moved = np.abs(ref - pts).max(1)[rst > 0]
    assert (moved > 4.5).sum() >= 20, moved   # tracked over the shift
    # (at one level every such point has left the J region staged at its start, which reaches 3 px either way)


def test_tracker_step_path_matches_oracle():
    """readImage through the step path (the kernel WITHOUT the error pass): 3 sequences x 4 frames, a feature capacity that
    is no multiple of the four features of a workgroup."""
    cfg = abi.default_config(max_corners=37, min_dist=8, image_rows=ROWS, image_cols=COLS)
    S, T = 3, 4
    streams = [synth.make_image_stream(40 + s, T, rows=ROWS, cols=COLS)[0] for s in range(S)]
    trk = fe.FeatureTracker(cfg, n_seq=S)
    oracles = [H.OracleTracker(cfg) for _ in range(S)]
    tracked = 0
    for f in range(T):
        publish = f % 2 == 0
        got = trk.read_images(np.stack([streams[s][f] for s in range(S)]), publish)
        for s in range(S):
            rids, rxyz = oracles[s].read_image(streams[s][f], publish)
            gids, gxyz = got[s]
            assert np.array_equal(gids, rids), (f, s)
            assert np.array_equal(gxyz, rxyz), (f, s)
            gp, gi, gc = trk.state(s)
            rp, ri, rc = oracles[s].state()
            assert np.array_equal(gi, ri) and np.array_equal(gc, rc), (f, s)
            assert np.array_equal(gp, rp), (f, s, np.abs(gp - rp).max())
            tracked += int((rc > 1).sum())
    assert tracked > 10 * S   # features did survive LK between frames: the comparison is of tracked points
    trk.close()
    for o in oracles:
        o.close()
