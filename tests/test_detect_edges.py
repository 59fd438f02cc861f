"""The inputs of test_detect_edges_gpu.py are the edges they are named for (CPU oracle alone, no device): if a constant of
the detector or a generator changes so that a case stops overflowing a list, stops crossing the LDS / in-place switch
or stops filling a mask word, it fails here."""
import numpy as np
import pytest

import helpers as H
import detect_cases as D


def test_constants():
    assert D.CAND_LDS == 1984 and D.BLOCK_W == 240 and D.seg_cap(256) == 2048 and D.SEL_LDS == 8192


def test_candidates_helper_is_the_oracle_rule():
    """detector_candidates + the quality threshold, taken in (value, raster) order, is oracle_good_features at MIN_DIST 0."""
    img = D.texture(96, 256)
    cfg = D.config(96, 256, 512, 0)
    eig = H.oracle_min_eigen_map(img)
    keep = H.detector_candidates(img) & (eig > D.threshold(eig, None, cfg.quality_level))
    ys, xs = np.nonzero(keep)
    order = np.argsort(-eig[ys, xs].astype(np.float64), kind="stable")[:512]  # (nonzero is raster order)
    ref = H.oracle_good_features(cfg, img, None, 512)
    assert np.array_equal(ref, np.column_stack([xs[order], ys[order]]).astype(np.float32))


@pytest.mark.parametrize("name", sorted(D.PLATEAU_IMAGES))
def test_plateau_images_overflow_both_lists(name):
    img = D.PLATEAU_IMAGES[name]()
    assert img.shape == D.PLATEAU_SHAPE
    cand = H.detector_candidates(img)
    assert D.worst_block(cand) > D.CAND_LDS
    assert D.worst_strip(cand) > D.seg_cap(img.shape[1])
    n = D.survivors(img, None, 0.01)
    if name == "checker3":
        assert 0 < n <= D.SEL_LDS   # LDS path of the selection
    else:
        assert n > D.SEL_LDS        # in-place path, a sea of equal keys
    # with the column mask the candidates come from a region narrower than a block, and it still overflows
    m = D.column_mask(*img.shape)
    assert m[:, 100:181].all() and not m[:, :100].any() and not m[:, 181:].any()
    cm = H.detector_candidates(img, m)
    if name != "checker3":
        assert D.worst_block(cm) > D.CAND_LDS and D.worst_strip(cm) > D.seg_cap(img.shape[1])
    assert not cm[:, :100].any() and not cm[:, 181:].any() and cm.any()


def test_texture_alone_does_not_overflow():
    cand = H.detector_candidates(D.texture(96, 256))
    assert D.worst_block(cand) < D.CAND_LDS // 4 and D.worst_strip(cand) < D.seg_cap(256) // 4


def test_mixed_first_pick_is_late_in_its_strip():
    """The oracle's first corner of the mixed image lies in row 30 of its strip: the block's list is full long before."""
    ref = H.oracle_good_features(D.config(96, 256, 40, 10), D.mixed(), None, 40)
    assert ref[0].tolist() == [1.0, 94.0] and 94 % D.DET_R == 30


@pytest.mark.parametrize("name", sorted(D.TRACKER_PLATEAU_SCENES))
def test_tracker_plateau_scenes_overflow(name):
    img = D.TRACKER_PLATEAU_SCENES[name]()
    assert img.shape == D.TRACKER_PLATEAU_SHAPE
    cand = H.detector_candidates(img)
    assert D.worst_block(cand) > D.CAND_LDS and D.worst_strip(cand) > D.seg_cap(img.shape[1])


def test_corner_block_scene_overflows_its_block():
    img = D.corner_block(*D.TRACKER_PLATEAU_SHAPE)
    cand = H.detector_candidates(img)
    assert int(cand[:D.DET_R, :D.BLOCK_W].sum()) > D.CAND_LDS
    assert int(cand[:D.DET_R].sum()) > D.seg_cap(img.shape[1])


def test_odd_plateau_shape_overflows_and_leaves_rests():
    rows, cols = D.ODD_PLATEAU_SHAPE
    assert cols > D.REDO_W and cols % D.REDO_W and cols % D.BLOCK_W and rows % D.DET_R
    cand = H.detector_candidates(D.checker(rows, cols, 2))
    assert D.worst_block(cand) > D.CAND_LDS and D.worst_strip(cand) > D.seg_cap(cols)
    assert cand[rows - rows % D.DET_R:].any() and cand[:, D.REDO_W:].any()   # candidates in the rest strip and the rest tile


def test_turn_scenes_outnumber_the_redo_lists():
    scenes = D.turn_scenes()
    assert len(scenes) == D.TURN_SEQUENCES
    over = []
    for img in scenes:
        cand = H.detector_candidates(img)
        over.append(D.worst_block(cand) > D.CAND_LDS or D.worst_strip(cand) > D.seg_cap(img.shape[1]))
    assert over == [True, True, True, False, True, True, True]
    assert sum(over) > D.REDO_LISTS
    assert any(over[k] and over[k + D.REDO_LISTS] for k in range(len(over) - D.REDO_LISTS))   # two of them share a list


def test_noise_takes_the_in_place_path():
    assert D.survivors(D.noise(*D.NOISE_BIG), None, 0.01) > D.SEL_LDS
    assert D.survivors(D.noise(*D.NOISE_BOUNDARY), None, 0.01) > D.SEL_LDS + 1
    # MIN_DIST 70 reaches five strips: the suppression takes a second trip of four
    assert (2 * 70) // D.DET_R + 1 >= 5


@pytest.mark.parametrize("k", D.BOUNDARY_COUNTS)
def test_noise_boundary_survivor_counts(k):
    img = D.noise(*D.NOISE_BOUNDARY)
    q = D.quality_for_survivors(img, k)
    assert q is not None and 0.0 < q < 1.0
    assert D.survivors(img, None, q) == k
    cand = H.detector_candidates(img)  # the lists themselves do not overflow: the ordinary path is under test
    assert D.worst_block(cand) <= D.CAND_LDS and D.worst_strip(cand) <= D.seg_cap(img.shape[1])


def test_ramp_masked_maximum_is_negative():
    eig = H.oracle_min_eigen_map(D.ramp())
    neg = eig < 0
    assert int(neg.sum()) == 633 and eig[neg].max() < 0
    cfg = D.config(96, 256, 50, 10)
    assert len(H.oracle_good_features(cfg, D.ramp(), neg.astype(np.uint8) * 255, 50)) == 0


def disc_sequence_facts(min_dist):
    """Oracle tracker over the scene-change stream -> (full-word discs, centre near an image edge, centre near x = 240) over
    the publish frames that detect under discs."""
    rows, cols = D.DISC_SHAPE
    T, cut = 5, 3
    stream = D.jump_stream(*D.DISC_SEEDS[min_dist], T, cut, rows, cols)
    trk = H.OracleTracker(D.config(rows, cols, 60, min_dist))
    hits, at_image, at_block = [], False, False
    for f in range(T):
        publish = f != 2
        trk.read_image(stream[f], publish)
        if publish and f > 0:
            pts, _, cnt = trk.state()
            centres = D.disc_centres(pts, cnt)
            if len(centres):
                hits += D.full_word_discs(centres, min_dist, rows, cols)
                a, b = D.disc_edge_conditions(centres, min_dist, rows, cols)
                at_image, at_block = at_image or a, at_block or b
    trk.close()
    return hits, at_image, at_block


@pytest.mark.parametrize("min_dist", sorted(D.DISC_SEEDS))
def test_disc_rows_fill_a_whole_mask_word(min_dist):
    assert min_dist <= D.MAX_RADIUS
    hits, at_image, at_block = disc_sequence_facts(min_dist)
    assert hits, "no disc row covers a whole wave word"
    if min_dist == 32:  # the one radius at which only two centre columns per wave do it
        assert all(x0 + 29 <= cx <= x0 + 30 for cx, _, x0 in hits)
    assert at_image and at_block
