"""The valid region of a pre-step slot on the device: one launch for a batch that mixes slots without a lens, every lens model
and sourced slots, bit for bit the host entry vio_lens_model_valid_region (whose own yardstick is tests/test_region_cpu.py).
And the front end's region of interest per sequence (vio_frontend_set_regions), bit for bit region_cases.RegionTracker, which
tests/test_region_cpu.py holds against the oracle tracker."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import detect_cases as D
import helpers as H
import lens_model_cases as MC
import region_cases as RC
from device_buffers import Hip
from helpers import abi, pkg, synth
from test_frontend_subset_gpu import N_SEQ, assert_same, schedule

pytestmark = pytest.mark.gpu

ROWS, COLS = 72, 100        # two tiles of 64 across and down, both partial


def host_masks(margin):
    """{case name: the host entry's mask} for the eight slots of region_cases.cases (a slot without a lens: all 255)."""
    return {name: np.full((ROWS, COLS), 255, np.uint8) if lens is None else abi.lens_model_valid_region(lens, src, ROWS, COLS, margin)
            for name, lens, src in RC.cases(ROWS, COLS)}


def context():
    """Slots 0 .. 5: lens_model_cases.mixed_lenses (slot 1 through set_lenses); 6, 7: the sourced Brown-Conrady and fisheye."""
    cases = RC.cases(ROWS, COLS)
    pp = pkg.frontend.Preprocessor(ROWS, COLS, max_frames=len(cases) + 1)      # the last slot stays empty
    assert pp.set_lenses([1], [MC.mixed_lenses(ROWS, COLS)[1]]) == abi.VIO_OK
    assert pp.set_lens_models([2, 3, 4, 5, 6, 7], [l for _, l, _ in cases[2:]]) == abi.VIO_OK
    assert pp.set_sources([6, 7], [s for _, _, s in cases[6:]]) == abi.VIO_OK
    return pp, [name for name, _, _ in cases]


@pytest.mark.parametrize("margin", [0, 10])
def test_valid_regions_host_route_equals_the_host_entry(margin):
    pp, names = context()
    want = host_masks(margin)
    slots = [5, 0, 7, 3, 1, 8, 6, 2, 4]                     # entry i of the call is slot slots[i], in any order
    rc, masks = pp.valid_regions(slots, margin)
    assert rc == abi.VIO_OK
    for i, s in enumerate(slots):
        w = want[names[s]] if s < 8 else np.full((ROWS, COLS), 255, np.uint8)
        assert np.array_equal(masks[i], w), (s, int((masks[i] != w).sum()))
    assert 0 < int((masks[0] == 0).sum()) < ROWS * COLS and 0 < int((masks[2] == 0).sum()) < ROWS * COLS
    if margin == 0:
        assert int((masks[0] == 0).sum()) == abi.lens_model_coverage(MC.fisheye_clamped(ROWS, COLS), ROWS, COLS)
    pp.close()


@pytest.mark.parametrize("margin", [0, 10])
def test_valid_regions_resident_route_on_a_caller_stream(margin):
    pp, names = context()
    want = host_masks(margin)
    h = Hip()
    stream = C.c_void_p()
    assert h.hip.hipStreamCreate(C.byref(stream)) == 0
    n = 8
    d_masks = h.upload(np.full((n + 1, ROWS, COLS), 7, np.uint8))
    assert pp.valid_regions_resident(range(n), margin, d_masks.value, stream=stream.value) == abi.VIO_OK
    pp.sync()
    got = h.download(d_masks, np.zeros((n + 1, ROWS, COLS), np.uint8))
    for s in range(n):
        assert np.array_equal(got[s], want[names[s]]), (s, int((got[s] != want[names[s]]).sum()))
    assert (got[n] == 7).all()                               # nothing behind the call's n masks is written
    h.hip.hipFree(d_masks), h.hip.hipStreamDestroy(stream)
    pp.close()


def test_valid_regions_argument_errors_write_nothing():
    pp, _ = context()
    lib = abi.load_product()
    masks = np.full((2, ROWS, COLS), 7, np.uint8)
    mp = masks.ctypes.data_as(C.POINTER(C.c_uint8))

    def call(slots, margin, out=mp, handle=None):
        a = (C.c_int32 * max(len(slots), 1))(*slots)
        return lib.vio_preprocess_valid_regions(pp._h if handle is None else handle, len(slots), a, margin, out)
    assert call([0, 9], 0) == abi.VIO_EINVAL and call([-1], 0) == abi.VIO_EINVAL          # a slot out of range
    assert call([5, 5], 0) == abi.VIO_EINVAL                                              # named twice
    assert call([5], -1) == abi.VIO_EINVAL and call([5], 33) == abi.VIO_EINVAL            # the margin
    assert call([5], 0, out=None) == abi.VIO_EINVAL
    assert lib.vio_preprocess_valid_regions(pp._h, 1, None, 0, mp) == abi.VIO_EINVAL
    assert lib.vio_preprocess_valid_regions(None, 0, None, 0, mp) == abi.VIO_EINVAL
    assert lib.vio_preprocess_valid_regions_resident(pp._h, 1, None, 0, C.c_void_p(16), None) == abi.VIO_EINVAL
    assert lib.vio_preprocess_valid_regions_resident(pp._h, 1, (C.c_int32 * 1)(5), 0, None, None) == abi.VIO_EINVAL
    assert (masks == 7).all()
    assert call([5, 4], 32) == abi.VIO_OK and 0 < int((masks[0] == 0).sum()) and (masks[1] == 255).all()
    pp.close()


# ---- the front end's region of interest ------------------------------------------------------------------------------------
# 70 x 260: two detector workgroups across (260 > 240), every wave's 64-column window across a 64-bit word boundary (the waves
# are 60 columns apart), two full strips of 32 rows and a partial one
FE_ROWS, FE_COLS, FE_FRAMES, FE_RING = 70, 260, 12, 12
FeatureTracker = pkg.frontend.FeatureTracker


def fe_config():
    return abi.default_config(max_corners=40, min_dist=10, image_rows=FE_ROWS, image_cols=FE_COLS)


def fe_regions():
    """The regions of the five sequences: ring, holes, word edges, none, nothing usable."""
    return [RC.ring(FE_ROWS, FE_COLS, FE_RING), RC.holes(FE_ROWS, FE_COLS), RC.word_edges(FE_ROWS, FE_COLS), None,
            RC.none_usable(FE_ROWS, FE_COLS)]


def set_all(trk, regions):
    have = [s for s, r in enumerate(regions) if r is not None]
    assert trk.set_regions(have, np.stack([regions[s] for s in have])) == abi.VIO_OK


@functools.lru_cache(maxsize=None)
def lockstep_reference():
    """Five streams of 12 frames, publish on every third, each through its own RegionTracker, once: (frames [T][S], per frame and
    sequence (ids, xyz, state), what the region dropped per sequence)."""
    cfg, regions = fe_config(), fe_regions()
    frames = np.stack([synth.make_image_stream(40 + s, FE_FRAMES, rows=FE_ROWS, cols=FE_COLS)[0] for s in range(5)], axis=1)
    trackers = [RC.RegionTracker(cfg, r) for r in regions]
    want = []
    for f in range(FE_FRAMES):
        row = []
        for s, t in enumerate(trackers):
            ids, xyz = t.read_image(frames[f][s], f % 3 == 0)
            row.append((ids, xyz, t.state()))
        want.append(row)
    return frames, want, [sum(e["dropped"] for e in t.log) for t in trackers]


def test_five_sequences_with_different_regions_in_one_context():
    cfg, regions = fe_config(), fe_regions()
    frames, want, dropped = lockstep_reference()
    print("tracks the regions dropped, per sequence:", dropped)
    assert dropped[0] > 0 and dropped[3] == 0                 # the ring took tracks: the greedy pass's region bit is exercised
    trk = FeatureTracker(cfg, n_seq=5)
    set_all(trk, regions)
    single = [FeatureTracker(cfg, n_seq=1) for _ in range(5)]
    for s, r in enumerate(regions):
        if r is not None:
            assert single[s].set_regions([0], r[None]) == abi.VIO_OK
    oracle = H.OracleTracker(cfg)
    for f in range(FE_FRAMES):
        pub = f % 3 == 0
        got = trk.read_images(frames[f], pub)
        for s in range(5):
            ids, xyz, state = want[f][s]
            what = "frame %d sequence %d" % (f, s)
            assert_same(got[s], (ids, xyz), what + ": observations")
            assert_same(trk.state(s), state, what + ": state")
            single[s].read_images(frames[f][s:s + 1], pub)
            assert_same(trk.pnp_points(s), single[s].pnp_points(0), what + ": pnp_points")
        assert_same(got[3], oracle.read_image(frames[f][3], pub), "frame %d: the sequence without a region" % f)
        assert_same(trk.state(3), oracle.state(), "frame %d: the sequence without a region, state" % f)
        assert len(got[4][0]) == 0                              # nothing usable: nothing published, and the call returned
        if pub:
            for s in range(3):                                   # no published feature on a 0 pixel
                p = np.rint(trk.state(s)[0]).astype(int)
                assert len(p) > 0 and (regions[s][p[:, 1], p[:, 0]] == 255).all(), (f, s)
    oracle.close()
    trk.close()
    for t in single:
        t.close()


TICKS, CHANGE_TICK = 12, 6


def subset_regions(tick):
    """Regions on sequences 0, 1 and 3; sequence 0's changes ahead of tick CHANGE_TICK."""
    first = RC.ring(FE_ROWS, FE_COLS, FE_RING) if tick < CHANGE_TICK else RC.word_edges(FE_ROWS, FE_COLS)
    return {0: first, 1: RC.holes(FE_ROWS, FE_COLS), 3: RC.ring(FE_ROWS, FE_COLS, 20)}


@functools.lru_cache(maxsize=None)
def subset_reference():
    """test_frontend_subset_gpu's schedule through one RegionTracker per sequence, once: (frames [sequence][tick], per tick
    {sequence: (ids, xyz, state)})."""
    cfg = fe_config()
    frames = [synth.make_image_stream(40 + s, TICKS, rows=FE_ROWS, cols=FE_COLS)[0] for s in range(N_SEQ)]
    trackers = [RC.RegionTracker(cfg, subset_regions(0).get(s)) for s in range(N_SEQ)]
    per_tick = []
    for t, (resets, call) in enumerate(schedule(TICKS)):
        if t == CHANGE_TICK:
            trackers[0].set_region(subset_regions(t)[0])
        for s in resets:                                         # a fresh tracker; the sequence's region survives
            trackers[s] = RC.RegionTracker(cfg, subset_regions(t).get(s))
        want = {}
        for s, pub in call:
            ids, xyz = trackers[s].read_image(frames[s][t], pub)
            want[s] = (ids, xyz, trackers[s].state())
        per_tick.append(want)
    return frames, per_tick


@pytest.mark.parametrize("route", ["host", "device"])
def test_regions_through_read_subset(route):
    cfg = fe_config()
    frames, per_tick = subset_reference()
    trk = FeatureTracker(cfg, n_seq=N_SEQ)
    regions = subset_regions(0)
    assert trk.set_regions(sorted(regions), np.stack([regions[s] for s in sorted(regions)])) == abi.VIO_OK
    host = np.zeros((N_SEQ, FE_ROWS, FE_COLS), np.uint8)
    h, slots, px = Hip(), 7, FE_ROWS * FE_COLS
    dev = h.upload(np.zeros((slots, FE_ROWS, FE_COLS), np.uint8)) if route == "device" else None
    published = 0
    for t, (resets, call) in enumerate(schedule(TICKS)):
        if t == CHANGE_TICK:                                     # between two ticks: acts from the next publish frame on
            assert trk.set_regions([0], subset_regions(t)[0][None]) == abi.VIO_OK
        if resets:
            trk.reset(resets)
            for s in resets:
                mask, is_set, _ = trk.region(s)
                assert is_set and np.array_equal(mask, subset_regions(t)[s])
        if t % 2 == 1:
            call = call[::-1]
        seqs, flags = [s for s, _ in call], [1 if p else 0 for _, p in call]
        for i, s in enumerate(seqs):
            host[i] = frames[s][t]
        if route == "device":
            index = [(3 * i + 2) % slots for i in range(len(seqs))]
            for i, k in enumerate(index):
                assert h.hip.hipMemcpy(dev.value + k * px, host[i].ctypes.data, px, 1) == 0
            got = trk.read_subset(seqs, dev.value, flags, index)
        else:
            got = trk.read_subset(seqs, host.copy(), flags)
        for i, (s, pub) in enumerate(call):
            ids, xyz, state = per_tick[t][s]
            what = "%s tick %d sequence %d (publish %d)" % (route, t, s, pub)
            assert_same(got[i], (ids, xyz), what + ": observations")
            assert_same(trk.state(s), state, what + ": state")
            published += len(ids)
    assert published > 0
    if dev is not None:
        h.hip.hipFree(dev)
    trk.close()


def test_redo_path_honours_the_region(monkeypatch, capfd):
    """The 2 x 2 checkerboard of test_redo_path_inside_a_subset: every pixel of the plateau is a candidate, the lists overflow,
    and the sequence is redone from the full-size list -- whose detector pass reads the same mask words."""
    monkeypatch.setenv("VIO_AMD_REDO_REPORT", "1")
    rows, cols = D.TRACKER_PLATEAU_SHAPE
    cfg = D.config(rows, cols, 60, 10)
    scenes = [D.checker(rows, cols, 2), D.texture(rows, cols, seed=7)]
    region = RC.ring(rows, cols, FE_RING)
    trk = FeatureTracker(cfg, n_seq=2)
    assert trk.set_regions([0], region[None]) == abi.VIO_OK
    want = [RC.RegionTracker(cfg, region), RC.RegionTracker(cfg)]
    for f in range(2):
        got = trk.read_subset([1, 0], np.stack([scenes[1], scenes[0]]), [1, 1])
        for i, s in enumerate([1, 0]):
            ids, xyz = want[s].read_image(scenes[s], True)
            assert_same(got[i], (ids, xyz), "frame %d sequence %d: observations" % (f, s))
            assert_same(trk.state(s), want[s].state(), "frame %d sequence %d: state" % (f, s))
    p = np.rint(trk.state(0)[0]).astype(int)
    assert len(p) > 0 and (region[p[:, 1], p[:, 0]] == 255).all()
    capfd.readouterr()
    trk.close()
    m = re.search(r"detector: (\d+) sequence-frames redone", capfd.readouterr().err)
    assert m, "no redo report"
    print("redone: %s sequence-frames" % m.group(1))
    assert int(m.group(1)) >= 1


def test_lens_to_valid_region_to_tracker_on_the_device():
    """A fisheye slot of the pre-step: its valid region at margin 12 goes from valid_regions_resident straight into
    set_regions(masks_on_device = 1); the frames are rectified by run_resident and tracked by read_subset where they lie."""
    cfg, margin = fe_config(), 12
    lens = MC.fisheye_clamped(FE_ROWS, FE_COLS)
    raw = synth.make_image_stream(45, FE_FRAMES, rows=FE_ROWS, cols=FE_COLS)[0]
    # the host's restatement: rectified gray, the oracle's CLAHE of it, the valid region
    frames = [H.oracle_preprocess(MC.rectify(f, lens))[1] for f in raw]
    inside = RC.inside(lens, None, FE_ROWS, FE_COLS)
    mask = RC.valid_region(lens, None, FE_ROWS, FE_COLS, margin)
    assert int((~inside).sum()) == abi.lens_model_coverage(lens, FE_ROWS, FE_COLS) and 0 < int((mask == 255).sum()) < inside.sum()
    want = RC.RegionTracker(cfg, mask)
    h = Hip()
    pp = pkg.frontend.Preprocessor(FE_ROWS, FE_COLS, max_frames=1)
    assert pp.set_lens_models([0], [lens]) == abi.VIO_OK
    d_mask = h.upload(np.zeros((1, FE_ROWS, FE_COLS), np.uint8))
    d_raw, d_eq = h.upload(raw[0]), h.upload(np.zeros((1, FE_ROWS, FE_COLS), np.uint8))
    assert pp.valid_regions_resident([0], margin, d_mask.value) == abi.VIO_OK
    trk = FeatureTracker(cfg, n_seq=1)
    assert trk.set_regions([0], d_mask.value, mask_index=[0]) == abi.VIO_OK     # (waits for the device: the mask is complete)
    got_mask, is_set, n_usable = trk.region(0)
    assert is_set and np.array_equal(got_mask, mask) and n_usable == int((mask == 255).sum())
    published = 0
    for f in range(FE_FRAMES):
        pub = f % 3 == 0
        assert h.hip.hipMemcpy(d_raw, raw[f].ctypes.data, raw[f].nbytes, 1) == 0
        pp.run_resident(d_raw.value, 1, 1, d_eq.value)
        pp.sync()
        got = trk.read_subset([0], d_eq.value, [1 if pub else 0], [0])
        ids, xyz = want.read_image(frames[f], pub)
        assert_same(got[0], (ids, xyz), "frame %d: observations" % f)
        assert_same(trk.state(0), want.state(), "frame %d: state" % f)
        if pub:
            for x, y in np.rint(trk.state(0)[0]).astype(int):
                assert inside[max(0, y - margin):y + margin + 1, max(0, x - margin):x + margin + 1].all(), (f, x, y)
            published += len(ids)
    print("usable pixels", n_usable, "published observations", published)
    assert published > 0
    for d in (d_mask, d_raw, d_eq):
        h.hip.hipFree(d)
    trk.close(), pp.close()


def test_regions_contract():
    cfg, regions = fe_config(), fe_regions()
    frames, _, _ = lockstep_reference()
    trk, fresh = FeatureTracker(cfg, n_seq=5), FeatureTracker(cfg, n_seq=5)
    lib, ip = trk.lib, C.POINTER(C.c_int32)
    set_all(trk, regions)

    def table():
        return [trk.region(s) for s in range(5)]

    def same_table(a, b):
        return all(np.array_equal(x[0], y[0]) and x[1:] == y[1:] for x, y in zip(a, b))
    t0 = table()
    for s, r in enumerate(regions):                              # bytes in, 0 / 255 and the count out
        mask, is_set, n = t0[s]
        assert is_set == (r is not None) and np.array_equal(mask, RC.all_usable(FE_ROWS, FE_COLS) if r is None else r)
        assert n == int((mask == 255).sum())
    odd = np.where(regions[1] != 0, 3, 0).astype(np.uint8)       # any nonzero byte is usable
    assert trk.set_regions([1], odd[None]) == abi.VIO_OK and same_table(table(), t0)
    # VIO_EINVAL leaves every region as it was
    two = np.stack([regions[2], regions[2]])
    assert trk.set_regions([0, 0], two) == abi.VIO_EINVAL and trk.set_regions([0, 5], two) == abi.VIO_EINVAL
    assert trk.set_regions([-1], two[:1]) == abi.VIO_EINVAL
    assert trk.set_regions([2, 0], two, mask_index=[0, -1]) == abi.VIO_EINVAL
    assert trk.set_regions([0, 0], None) == abi.VIO_EINVAL
    assert lib.vio_frontend_set_regions(trk._h, 1, None, C.c_void_p(two.ctypes.data), 0, None) == abi.VIO_EINVAL
    assert lib.vio_frontend_set_regions(None, 0, None, None, 0, None) == abi.VIO_EINVAL
    assert lib.vio_frontend_get_region(trk._h, 5, None, C.byref(C.c_int32()), C.byref(C.c_int64())) == abi.VIO_EINVAL
    assert same_table(table(), t0)
    # VIO_ESTATE between a submit and its collect
    trk.submit(frames[0], 1)
    assert trk.set_regions([0], two[:1]) == abi.VIO_ESTATE
    assert lib.vio_frontend_get_region(trk._h, 0, None, C.byref(C.c_int32()), C.byref(C.c_int64())) == abi.VIO_ESTATE
    trk.collect()
    assert same_table(table(), t0)
    # every region cleared: a fresh context's results from here on
    trk.reset()
    assert same_table(table(), t0)                               # (a reset leaves the regions)
    assert trk.set_regions([0, 1, 2, 3, 4], None) == abi.VIO_OK
    assert all(not is_set and n == FE_ROWS * FE_COLS and (mask == 255).all() for mask, is_set, n in table())
    for f in range(4):
        got, want = trk.read_images(frames[f], f % 3 == 0), fresh.read_images(frames[f], f % 3 == 0)
        for s in range(5):
            assert_same(got[s], want[s], "cleared: frame %d sequence %d" % (f, s))
            assert_same(trk.state(s), fresh.state(s), "cleared: frame %d sequence %d state" % (f, s))
    assert all(len(trk.state(s)[1]) > 0 for s in range(5))
    trk.close(), fresh.close()
