"""goodFeaturesToTrack on the device at the edges the smooth textures never reach (detect_cases.py; that the inputs are those
edges is asserted on the CPU in test_detect_edges.py): plateaus of equal eigenvalues that overflow the candidate lists, the
switch between the selection's LDS list and its in-place path, disc rows of the mask that fill a whole 64-lane word.
Everything is compared bit for bit with the CPU oracle."""
import ctypes as C
import re

import numpy as np
import pytest

import helpers as H
import detect_cases as D
from helpers import abi, pkg

pytestmark = pytest.mark.gpu
fe = pkg.frontend


def report(name, got, ref):
    """The figures of one comparison, printed before anything is asserted."""
    n = min(len(got), len(ref))
    diff = np.nonzero((got[:n] != ref[:n]).any(axis=1))[0]
    first = int(diff[0]) if len(diff) else (n if len(got) != len(ref) else -1)
    line = "%s: device %d picks, oracle %d; first differing pick %d" % (name, len(got), len(ref), first)
    if 0 <= first < n:
        line += " (device %s, oracle %s)" % (got[first].tolist(), ref[first].tolist())
    print(line)


_ref_cache = {}


def plateau_ref(name, masked, max_corners, min_dist):
    key = (name, masked, max_corners, min_dist)
    if key not in _ref_cache:
        img = D.PLATEAU_IMAGES[name]()
        mask = D.column_mask(*img.shape) if masked else None
        cfg = D.config(img.shape[0], img.shape[1], max_corners, min_dist)
        _ref_cache[key] = (cfg, img, mask, H.oracle_good_features(cfg, img, mask, max_corners))
    return _ref_cache[key]


@pytest.mark.parametrize("masked", [False, True], ids=["whole", "columns100to180"])
@pytest.mark.parametrize("max_corners,min_dist", D.PLATEAU_PARAMS)
@pytest.mark.parametrize("name", sorted(D.PLATEAU_IMAGES))
def test_plateau_images(name, max_corners, min_dist, masked):
    """Every pixel of a plateau is a candidate (23 184 on the 2x2 checkerboard, 7 616 in one block that lists 1 984 and 8 064
    in one strip whose segment holds 2 048): the device keeps them all, breaks the ties by raster index like the oracle's
    stable sort, and two calls agree."""
    cfg, img, mask, ref = plateau_ref(name, masked, max_corners, min_dist)
    got = fe.good_features(cfg, img, mask, max_corners)
    again = fe.good_features(cfg, img, mask, max_corners)
    report("%s %s max_corners %d min_dist %d" % (name, "masked" if masked else "whole", max_corners, min_dist), got, ref)
    print("  second call %s" % ("identical" if np.array_equal(got, again) else "DIFFERS"))
    assert len(ref) > 0
    assert np.array_equal(got, ref)
    assert np.array_equal(again, got)


def run_tracker(cfg, streams, publish_at):
    """Device tracker and one oracle per sequence over the streams: observations, ids, points and track counts equal on every
    frame. -> per frame, per sequence the number of features."""
    S, T = len(streams), len(streams[0])
    trk = fe.FeatureTracker(cfg, n_seq=S)
    oracles = [H.OracleTracker(cfg) for _ in range(S)]
    counts = []
    try:
        for f in range(T):
            publish = f in publish_at
            got = trk.read_images(np.stack([streams[s][f] for s in range(S)]), publish)
            counts.append([])
            for s in range(S):
                rids, rxyz = oracles[s].read_image(streams[s][f], publish)
                gids, gxyz = got[s]
                gp, gi, gc = trk.state(s)
                rp, ri, rc = oracles[s].state()
                print("frame %d sequence %d: device %d features, oracle %d" % (f, s, len(gi), len(ri)))
                assert np.array_equal(gids, rids), (f, s)
                assert np.array_equal(gxyz, rxyz), (f, s)
                assert np.array_equal(gi, ri) and np.array_equal(gc, rc) and np.array_equal(gp, rp), (f, s)
                counts[-1].append(len(gi))
    finally:
        trk.close()
        for o in oracles:
            o.close()
    return counts


def test_plateaus_through_the_tracker():
    """detect_kernel<false>: two still scenes whose lists overflow, cold start on frame 0, detection under the discs of what
    survived on frame 2."""
    rows, cols = D.TRACKER_PLATEAU_SHAPE
    scenes = [D.TRACKER_PLATEAU_SCENES[k]() for k in ("mixed", "checker2")]
    cfg = D.config(rows, cols, 60, 10)
    counts = run_tracker(cfg, [[img] * 3 for img in scenes], publish_at=(0, 2))
    assert all(n > 0 for n in counts[0])


def redone(err):
    """Sequence-frames the context redid from a full-size list, from the line VIO_AMD_REDO_REPORT=1 makes it print when it is closed."""
    m = re.search(r"detector: (\d+) sequence-frames redone", err)
    assert m, err
    return int(m.group(1))


def test_more_overflowing_sequences_than_redo_lists(monkeypatch, capfd):
    """Seven sequences of one tracker, six of them overflowing: the full-size lists are taken in turn, the ordinary sequence
    between them goes the ordinary way, and every sequence equals its oracle on every frame. The context's own count says that
    the six were redone (on the cold start at least; frame 2 detects only where tracks were lost) and nothing else was."""
    monkeypatch.setenv("VIO_AMD_REDO_REPORT", "1")
    rows, cols = D.TRACKER_PLATEAU_SHAPE
    cfg = D.config(rows, cols, 60, 10)
    counts = run_tracker(cfg, [[img] * 3 for img in D.turn_scenes()], publish_at=(0, 2))
    n = redone(capfd.readouterr().err)
    print("redone: %d sequence-frames" % n)
    assert all(c > 0 for c in counts[0])
    assert D.TURN_SEQUENCES - 1 <= n <= 2 * (D.TURN_SEQUENCES - 1)
    run_tracker(cfg, [[D.texture(rows, cols, seed=7)] * 3], publish_at=(0, 2))
    assert redone(capfd.readouterr().err) == 0   # an ordinary sequence alone: never


@pytest.mark.parametrize("max_corners,min_dist", [(150, 5), (512, 0)])
def test_plateau_odd_shape(max_corners, min_dist):
    """A plateau frame wider than one tile of the redo, with a rest tile and a rest strip (500 columns, more than the other
    cases here, because one tile of the redo is 480 wide)."""
    rows, cols = D.ODD_PLATEAU_SHAPE
    img = D.checker(rows, cols, 2)
    cfg = D.config(rows, cols, max_corners, min_dist)
    ref = H.oracle_good_features(cfg, img, None, max_corners)
    got = fe.good_features(cfg, img, None, max_corners)
    report("checker2 100x500 max_corners %d min_dist %d" % (max_corners, min_dist), got, ref)
    assert len(ref) > 100
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("min_dist", [0, 1, 30, 70])
def test_in_place_path_small_shape(min_dist):
    """More survivors than the selection's LDS list at 352 x 480: MIN_DIST 0 kills the corner alone, 70 reaches five strips
    (a second trip of the four-strip rescan)."""
    rows, cols = D.NOISE_BIG
    img = D.noise(rows, cols)
    cfg = D.config(rows, cols, 300, min_dist)
    ref = H.oracle_good_features(cfg, img, None, 300)
    got = fe.good_features(cfg, img, None, 300)
    report("noise 352x480 min_dist %d" % min_dist, got, ref)
    assert len(ref) > (20 if min_dist == 70 else 100)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("min_dist", [0, 12])
@pytest.mark.parametrize("k", D.BOUNDARY_COUNTS)
def test_lds_list_boundary(k, min_dist):
    """Exactly 8 191, 8 192 and 8 193 survivors: the last sizes of the LDS list and the first of the in-place path."""
    rows, cols = D.NOISE_BOUNDARY
    img = D.noise(rows, cols)
    cfg = D.config(rows, cols, 300, min_dist, quality_level=D.quality_for_survivors(img, k))
    ref = H.oracle_good_features(cfg, img, None, 300)
    got = fe.good_features(cfg, img, None, 300)
    report("noise 256x512, %d survivors, min_dist %d" % (k, min_dist), got, ref)
    assert len(ref) > 100
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("min_dist", sorted(D.DISC_SEEDS))
def test_disc_mask_word_edges(min_dist):
    """Disc rows wider than a wave's 64 columns (`l1 - l0 == 63`), discs over the image border and over the block edge, up to
    kMaxRadius, on a stream that changes scene so that publish frames mix kept and new corners."""
    rows, cols = D.DISC_SHAPE
    T, cut = 5, 3
    stream = D.jump_stream(*D.DISC_SEEDS[min_dist], T, cut, rows, cols)
    counts = run_tracker(D.config(rows, cols, 60, min_dist), [stream], publish_at=(0, 1, 3, 4))
    assert counts[0][0] > 0


def test_good_features_strided_views():
    """Image and mask are views into wider arrays: stride > cols."""
    rows, cols, stride = 96, 256, 300
    wide_img = np.full((rows, stride), 77, np.uint8)
    wide_mask = np.full((rows, stride), 255, np.uint8)
    img = D.texture(rows, cols)
    mask = np.zeros((rows, cols), np.uint8)
    mask[10:80, 30:200] = 255
    wide_img[:, :cols], wide_mask[:, :cols] = img, mask
    cfg = D.config(rows, cols, 80, 10)
    ref = H.oracle_good_features(cfg, img, mask, 80)
    lib = abi.load_product()
    u8p = C.POINTER(C.c_uint8)
    corners, n = np.zeros((80, 2), np.float32), C.c_int32()
    rc = lib.vio_good_features(C.byref(cfg), wide_img.ctypes.data_as(u8p), wide_mask.ctypes.data_as(u8p), rows, cols, stride, 80,
                               corners.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n))
    assert rc == abi.VIO_OK, rc
    report("strided views", corners[: n.value], ref)
    assert len(ref) > 20
    assert np.array_equal(corners[: n.value], ref)


def test_negative_masked_maximum():
    """mask = (eig < 0) on the ramp image: the masked maximum is negative and nothing is a corner."""
    img = D.ramp()
    mask = (H.oracle_min_eigen_map(img) < 0).astype(np.uint8) * 255
    cfg = D.config(96, 256, 50, 10)
    assert len(H.oracle_good_features(cfg, img, mask, 50)) == 0
    assert len(fe.good_features(cfg, img, mask, 50)) == 0
