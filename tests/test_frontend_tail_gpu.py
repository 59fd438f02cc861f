"""The two one-workgroup-per-sequence kernels behind the throughput kernels of the front end, at the sizes where their
block-wide scans, ballots and index lists change path:
    track_update_kernel    status / border filter, the two F-tests, setMask  (through vio_frontend_set_tracks / _update_tracks)
    corner_select_kernel   threshold pass, greedy rounds, updateID, image_msg (through FeatureTracker against OracleTracker)
Everything is compared bit for bit with the oracle."""
import numpy as np
import pytest

import helpers as H
from helpers import abi, synth, pkg
from test_track_update_gpu import assert_same, run_both, two_view_points

pytestmark = pytest.mark.gpu
fe = pkg.frontend


def fields(cfg, n, seed, outliers=True):
    """Tracker fields of n tracks over three views of one scene. With `outliers`, an eighth of the tracks jumps between cur and
    forw (the first F-test rejects them) and another eighth drifted over the publish baseline only (the second does)."""
    rng = np.random.default_rng(seed)
    pre, forw = two_view_points(rng, cfg, n, (0.25, 0.05, 0.1))
    cur, _ = two_view_points(np.random.default_rng(seed), cfg, n, (0.1, 0.02, 0.04))
    if outliers and n >= 16:
        k = n // 8
        bad = rng.choice(n, 2 * k, replace=False)
        cur[bad[:k]] += rng.uniform(8, 25, (k, 2)).astype(np.float32) * rng.choice([-1, 1], (k, 2))
        pre[bad[k:]] += rng.uniform(8, 25, (k, 2)).astype(np.float32) * rng.choice([-1, 1], (k, 2))
    ids = np.arange(100, 100 + n)
    cnt = rng.integers(1, 9, n)
    return pre, cur, forw, ids, cnt


# (max_corners, n): the RANSAC threshold (8), the LMedS / RANSAC switch (15), ballot and `inside` word boundaries (64), the usual
# capacity, the 256-slot layout full, and the 512-slot instantiation
SIZES = [(150, 0), (150, 1), (150, 7), (150, 8), (150, 14), (150, 15), (150, 63), (150, 64), (150, 65), (150, 150), (256, 256),
         (300, 257), (300, 300)]


@pytest.mark.parametrize("publish", [0, 1])
@pytest.mark.parametrize("cap,n", SIZES)
def test_track_update_sizes(cap, n, publish):
    cfg = abi.default_config(max_corners=cap, min_dist=10)
    pre, cur, forw, ids, cnt = fields(cfg, n, 1000 + n)
    g, r = run_both(cfg, pre, cur, forw, ids, cnt, np.ones(n, np.uint8), publish=bool(publish))
    assert_same(g, r)
    if n >= 64:   # both F-tests had something to reject, and most tracks pass them
        assert n // 2 < len(r[1]) <= n - (n // 8 if not publish else 0) + 2


@pytest.mark.parametrize("publish", [0, 1])
def test_track_update_nothing_survives_the_first_filter(publish):
    cfg = abi.default_config(max_corners=150, min_dist=10)
    n = 90
    pre, cur, forw, ids, cnt = fields(cfg, n, 7)
    g, r = run_both(cfg, pre, cur, forw, ids, cnt, np.zeros(n, np.uint8), publish=bool(publish))   # every track lost by LK
    assert_same(g, r)
    assert len(g[1]) == 0
    out = forw.copy()                                                                                # every track outside the border
    out[: n // 2, 0] = np.linspace(-30, 0.4, n // 2)
    out[n // 2:, 1] = np.linspace(cfg.image_rows - 0.6, cfg.image_rows + 40, n - n // 2)
    g, r = run_both(cfg, pre, cur, out, ids, cnt, np.ones(n, np.uint8), publish=bool(publish))
    assert_same(g, r)
    assert len(g[1]) == 0


def test_track_update_second_f_test_skipped():
    """The first F-test leaves fewer than 8 tracks: rejectWithF does not run on what is left, setMask does."""
    cfg = abi.default_config(max_corners=150, min_dist=10)
    n = 8
    rng = np.random.default_rng(3)
    pre, cur, forw, ids, cnt = fields(cfg, n, 3, outliers=False)
    cur[5:] = rng.uniform(40, 400, (n - 5, 2)).astype(np.float32)   # three tracks with no geometry at all between cur and forw
    g0, r0 = run_both(cfg, pre, cur, forw, ids, cnt, np.ones(n, np.uint8), publish=False)
    assert_same(g0, r0)
    assert 0 < len(r0[1]) < 8
    g1, r1 = run_both(cfg, pre, cur, forw, ids, cnt, np.ones(n, np.uint8), publish=True)
    assert_same(g1, r1)
    assert 0 < len(r1[1]) <= len(r0[1])


@pytest.mark.parametrize("cap,n", [(150, 65), (150, 150), (300, 300)])
def test_track_update_equal_counts(cap, n):
    """Equal track_cnt throughout: the rank is the index order, and clusters make setMask drop tracks."""
    cfg = abi.default_config(max_corners=cap, min_dist=30)
    pre, cur, forw, ids, cnt = fields(cfg, n, 2000 + n)
    g, r = run_both(cfg, pre, cur, forw, ids, np.full(n, 3), np.ones(n, np.uint8), publish=True)
    assert_same(g, r)
    assert 8 < len(r[1]) < n and (g[2] == 4).all()


def jump_stream(seed_a, seed_b, T, cut, rows, cols):
    """A stream that changes scene at frame `cut`: most tracks are lost there, so the next publish frame mixes kept and new ids."""
    a = synth.make_image_stream(seed_a, T, rows=rows, cols=cols)[0]
    b = synth.make_image_stream(seed_b, T, rows=rows, cols=cols)[0]
    return [a[f] if f < cut else b[f] for f in range(T)]


@pytest.mark.parametrize("rows,cols,corners,min_dist", [
    (97, 61, 12, 8),      # the still sequence keeps its 12 slots full: its later frames need no corner
    (97, 61, 150, 8),     # more corners wanted than the small image has candidates, on every frame
    (97, 61, 40, 0),      # MIN_DIST 0: only the corner taken is suppressed
    (250, 333, 60, 12),
    (250, 333, 60, 0),
])
def test_corner_select_ids_points_observations(rows, cols, corners, min_dist):
    """Three sequences with different numbers of surviving tracks: a still one, a moving one, one that changes scene. Ids, points,
    counts and observations equal the oracle's on every frame; new ids continue each sequence's own counter.

    Case 97-61-12-8, frame 4, sequence 2 (the frame behind the scene change) sends eleven correspondences through the LMedS
    branch of the F-test: every 7-point model fits its own seven points to rounding error, so the median each model is ranked by
    is rounding noise (5e-29 against 2e-28 px^2 for the two best) and the winner hangs on the last bit of the cubic's roots. With
    the device library's acos / cos / pow the device kept tracks 8, 17, 23 where the oracle keeps 13, 20, 21; the branch now takes
    the roots from correctly rounded functions (vio_exact_math.h)."""
    cfg = abi.default_config(max_corners=corners, min_dist=min_dist, image_rows=rows, image_cols=cols)
    S, T = 3, 5
    moving = synth.make_image_stream(81, T, rows=rows, cols=cols)[0]
    streams = [[moving[0]] * T, synth.make_image_stream(82, T, rows=rows, cols=cols)[0], jump_stream(83, 84, T, 3, rows, cols)]
    trk = fe.FeatureTracker(cfg, n_seq=S)
    oracles = [H.OracleTracker(cfg) for _ in range(S)]
    next_id, seen, kept_and_new = [0] * S, [set() for _ in range(S)], False
    for f in range(T):
        publish = f != 2
        got = trk.read_images(np.stack([streams[s][f] for s in range(S)]), publish)
        survivors = []
        for s in range(S):
            rids, rxyz = oracles[s].read_image(streams[s][f], publish)
            gids, gxyz = got[s]
            assert np.array_equal(gids, rids), (f, s)
            assert np.array_equal(gxyz, rxyz), (f, s)
            gp, gi, gc = trk.state(s)
            rp, ri, rc = oracles[s].state()
            assert np.array_equal(gi, ri) and np.array_equal(gc, rc) and np.array_equal(gp, rp), (f, s)
            if not publish:
                continue
            new = [i for i in gi.tolist() if i not in seen[s]]
            assert new == list(range(next_id[s], next_id[s] + len(new))), (f, s)   # updateID: index order, no gap in n_id
            survivors.append(len(gi) - len(new))
            kept_and_new |= 0 < len(new) < len(gi)
            if f == 0:
                assert len(new) == len(gi) > 0                                      # first frame: every id is new
            if s == 0 and f >= 2:                                                   # the still sequence: no corner needed (or none to be had)
                assert not new and (len(gi) == corners or corners == 150)
            next_id[s] += len(new)
            seen[s].update(new)
        if f == 3:                                                                  # behind the scene change
            assert len(set(survivors)) > 1, survivors
    assert kept_and_new
    if corners == 150:
        assert all(len(trk.state(s)[1]) < corners for s in range(S))              # never enough candidates
    trk.close()
    for o in oracles:
        o.close()
