"""Lens models inside the image pre-step on the device (VioLensModel: Brown-Conrady, rational, fisheye): one launch serves a batch
that mixes slots without a lens and slots of every model. gray_out equals the numpy restatement (lens_model_cases.py) bit for
bit -- which is also what decides that the device's double sqrt rounds like the host's -- and the equalized frame is the oracle's
CLAHE of that gray; the old setter, and a context that sets nothing, give what they always gave."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import lens_cases as LC
import lens_model_cases as MC
import source_cases as SC
from device_buffers import Hip
from helpers import abi, pkg

pytestmark = pytest.mark.gpu

# 72 x 100 is no multiple of the 8 x 8 grid (reflect extension, byte stores of the apply pass); 64 x 96 is (dword stores)
SHAPES = [(72, 100, False), (72, 100, True), (64, 96, True)]

_want = {}


def expected(rows, cols, rgba):
    """(gray, equalized) of the six-slot mixed batch, computed once per shape and never written to."""
    key = (rows, cols, rgba)
    if key not in _want:
        g = MC.mixed_expected_gray(rows, cols, rgba)
        e = np.stack([H.oracle_preprocess(np.ascontiguousarray(x))[1] for x in g])
        e.flags.writeable = False
        _want[key] = (g, e)
    return _want[key]


def set_mixed(pp, rows, cols):
    """slot 0: no lens, 1: lens C through set_lenses, 2 .. 5: Brown, rational, fisheye inside, fisheye clamped as models."""
    lenses = MC.mixed_lenses(rows, cols)
    assert pp.set_lenses([1], [lenses[1]]) == abi.VIO_OK
    assert pp.set_lens_models([2, 3, 4, 5], lenses[2:]) == abi.VIO_OK
    return lenses


def check(got, want, what):
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("rows,cols,rgba", SHAPES)
def test_mixed_batch_host_route(rows, cols, rgba):
    frames = MC.mixed_frames(rows, cols, rgba)
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=6)
    lenses = set_mixed(pp, rows, cols)
    pp.kernel_ms()
    gray, eq = pp.run(frames)
    assert pp.kernel_ms()[1] == 1                           # one launch of the gray pass and one of the apply pass
    wg, we = expected(rows, cols, rgba)
    check(gray, wg, "gray")
    check(eq, we, "equalized")
    assert 0 < MC.n_outside(lenses[5], rows, cols) < rows * cols / 2 and MC.n_outside(lenses[4], rows, cols) == 0
    for k in range(1, 6):
        assert (wg[k] != LC.gray_of(frames[k])).mean() > 0.5   # every lens moved its frame
    pp.close()


@pytest.mark.parametrize("rows,cols,rgba", SHAPES)
def test_mixed_batch_resident_route_on_a_caller_stream(rows, cols, rgba):
    frames = MC.mixed_frames(rows, cols, rgba)
    h = Hip()
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=6)
    set_mixed(pp, rows, cols)
    stream = C.c_void_p()
    assert h.hip.hipStreamCreate(C.byref(stream)) == 0
    d_in, d_eq = h.upload(frames), h.upload(np.zeros((6, rows, cols), np.uint8))
    pp.run_resident(d_in.value, 4 if rgba else 1, 6, d_eq.value, stream=stream.value)
    pp.sync()
    eq = h.download(d_eq, np.zeros((6, rows, cols), np.uint8))
    check(eq, expected(rows, cols, rgba)[1], "equalized")
    h.hip.hipFree(d_in), h.hip.hipFree(d_eq), h.hip.hipStreamDestroy(stream)
    pp.close()


def source_batch(rows, cols):
    """[(source, lens model or None)]: an area-average slot without a lens, the inside fisheye over an RGBA frame of twice the
    output size (s = 2), the rational lens over a gray frame of 2.25 times the size with padded rows (s = 3), the clamped fisheye
    over video-range NV12 luma of the output's size (s = 1)."""
    area = abi.make_source(abi.VIO_PIXEL_GRAY8, 200, 301, stride=304, crop=(7, 5, 217, 173))
    rgba2 = abi.make_source(abi.VIO_PIXEL_RGBA8, 2 * rows, 2 * cols)
    gray = abi.make_source(abi.VIO_PIXEL_GRAY8, 162, 225, stride=228)
    nv12 = abi.make_source(abi.VIO_PIXEL_NV12, rows, cols, stride=cols + 12, range=1)
    return [(area, None), (rgba2, MC.for_frame(MC.fisheye_in(rows, cols), rgba2, rows, cols)),
            (gray, MC.for_frame(MC.rational(rows, cols), gray, rows, cols)),
            (nv12, MC.for_frame(MC.fisheye_clamped(rows, cols), nv12, rows, cols))]


_src_want = {}


def source_case(rows, cols):
    """(batch, planes, gray, equalized), computed once and never written to."""
    if (rows, cols) not in _src_want:
        batch = source_batch(rows, cols)
        planes = [SC.random_plane(29 * k + cols, s) for k, (s, _) in enumerate(batch)]
        for s, l in batch[1:]:                                # bit-exactness is a fair demand: no sample near a rounding tie
            assert MC.tie_distance(l, s.rows, s.cols, rows, cols, SC.sample_offsets(SC.samples_per_axis(s, rows, cols))) > 1e-10
        g = np.stack([SC.expected_gray(b, s, None, rows, cols) if l is None else MC.rectify_source(b, s, l, rows, cols)
                      for b, (s, l) in zip(planes, batch)])
        e = np.stack([H.oracle_preprocess(np.ascontiguousarray(x))[1] for x in g])
        g.flags.writeable = e.flags.writeable = False
        _src_want[(rows, cols)] = (batch, planes, g, e)
    return _src_want[(rows, cols)]


def source_context(rows, cols):
    batch = source_case(rows, cols)[0]
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=len(batch))
    assert [SC.samples_per_axis(s, rows, cols) for s, _ in batch[1:]] == [2, 3, 1]
    assert pp.set_sources(range(len(batch)), [s for s, _ in batch]) == abi.VIO_OK
    assert pp.set_lens_models([1, 2, 3], [l for _, l in batch[1:]]) == abi.VIO_OK
    return pp


def test_run_frames_with_sources_of_mixed_size_and_format():
    rows, cols = 72, 100
    _, planes, wg, we = source_case(rows, cols)
    pp = source_context(rows, cols)
    pp.kernel_ms()
    rc, gray, eq = pp.run_frames(planes)
    assert rc == abi.VIO_OK and pp.kernel_ms()[1] == 1
    check(gray, wg, "gray")
    check(eq, we, "equalized")
    pp.close()


def test_run_frames_resident_with_sources_of_mixed_size_and_format():
    rows, cols = 72, 100
    _, planes, _, we = source_case(rows, cols)
    h, pp = Hip(), source_context(rows, cols)
    stream = C.c_void_p()
    assert h.hip.hipStreamCreate(C.byref(stream)) == 0
    d_in = [h.upload(p) for p in planes]
    d_eq = h.upload(np.zeros((len(planes), rows, cols), np.uint8))
    assert pp.run_frames_resident([d.value for d in d_in], d_eq.value, stream=stream.value) == abi.VIO_OK
    pp.sync()
    check(h.download(d_eq, np.zeros((len(planes), rows, cols), np.uint8)), we, "equalized")
    for d in d_in + [d_eq]:
        h.hip.hipFree(d)
    h.hip.hipStreamDestroy(stream)
    pp.close()


def test_the_two_setters_write_one_table():
    rows, cols, rgba = 72, 100, True
    frames = MC.mixed_frames(rows, cols, rgba)
    wg, we = expected(rows, cols, rgba)
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=6)
    lenses = set_mixed(pp, rows, cols)
    lib = abi.load_product()
    # what each getter reads
    assert pp.get_lens(0) is None and pp.get_lens_model(0) is None
    assert bytes(pp.get_lens(1)) == bytes(lenses[1])
    assert bytes(pp.get_lens_model(1)) == bytes(abi.lens_model_of(lenses[1]))          # a slot set by set_lenses, as a model
    assert bytes(pp.get_lens(2)) == bytes(LC.lens_a(rows, cols))                       # a Brown model, as a VioLens
    for k in (3, 4, 5):
        assert bytes(pp.get_lens_model(k)) == bytes(lenses[k])
        keep, is_set = LC.identity_lens(rows, cols), C.c_int32(7)
        before = bytes(keep)
        assert lib.vio_preprocess_get_lens(pp._h, k, C.byref(keep), C.byref(is_set)) == abi.VIO_ESTATE
        assert bytes(keep) == before and is_set.value == 7                             # out is left alone
    # the fisheye of slot 4 replaced by a VioLens, and back
    assert pp.set_lenses([4], [LC.lens_c(rows, cols)]) == abi.VIO_OK
    assert bytes(pp.get_lens(4)) == bytes(LC.lens_c(rows, cols)) and pp.get_lens_model(4).model == abi.VIO_LENS_BROWN
    gray, eq = pp.run(frames)
    assert np.array_equal(gray[4], LC.rectify(frames[4], LC.lens_c(rows, cols)))
    check(gray[:4], wg[:4], "gray, slots 0 .. 3")
    check(gray[5:], wg[5:], "gray, slot 5")
    assert pp.set_lens_models([4], [lenses[4]]) == abi.VIO_OK
    gray, eq = pp.run(frames)
    check(gray, wg, "gray")
    check(eq, we, "equalized")
    # clearing through either setter: a fisheye slot through set_lenses, a set_lenses slot through set_lens_models
    assert pp.set_lenses([5], None) == abi.VIO_OK and pp.set_lens_models([1], None) == abi.VIO_OK
    assert pp.get_lens_model(5) is None and pp.get_lens(5) is None and pp.get_lens(1) is None
    gray, eq = pp.run(frames)
    for k in (1, 5):
        g0, e0 = H.oracle_preprocess(frames[k])
        assert np.array_equal(gray[k], g0) and np.array_equal(eq[k], e0)
    check(gray[2:5], wg[2:5], "gray, slots 2 .. 4")
    # no fisheye left in the table, then no lens at all: the kernels without those routes
    assert pp.set_lens_models([4], None) == abi.VIO_OK
    gray, eq = pp.run(frames)
    check(gray[2:4], wg[2:4], "gray, slots 2, 3")
    check(eq[2:4], we[2:4], "equalized, slots 2, 3")
    assert pp.set_lens_models([2, 3], None) == abi.VIO_OK
    gray, eq = pp.run(frames)
    for k in range(6):
        g0, e0 = H.oracle_preprocess(frames[k])
        assert np.array_equal(gray[k], g0) and np.array_equal(eq[k], e0)
    pp.close()


def test_argument_errors_change_nothing():
    rows, cols, rgba = 64, 96, True
    frames = MC.mixed_frames(rows, cols, rgba)
    wg, we = expected(rows, cols, rgba)
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=6)
    lenses = set_mixed(pp, rows, cols)
    table = [None if pp.get_lens_model(k) is None else bytes(pp.get_lens_model(k)) for k in range(6)]
    good = MC.rational(rows, cols)

    def variant(of, **kw):
        m = abi.VioLensModel.from_buffer_copy(bytes(of))
        for k, v in kw.items():
            if k.startswith("k"):
                m.k[int(k[1:])] = v
            else:
                setattr(m, k, v)
        return m
    bad = [variant(good, model=3), variant(good, model=-1), variant(good, reserved=1),
           variant(lenses[4], k4=1e-3), variant(lenses[4], k7=-2.0),            # a fisheye has four coefficients
           variant(lenses[2], k5=0.1), variant(lenses[2], k7=1e-9)]             # Brown-Conrady five
    for field in ("fx", "fy", "cx", "cy", "rect_fx", "rect_fy", "rect_cx", "rect_cy") + tuple("k%d" % i for i in range(8)):
        bad += [variant(good, **{field: float("nan")}), variant(good, **{field: float("inf")})]
    for field in ("fx", "fy", "rect_fx", "rect_fy"):
        bad += [variant(good, **{field: 0.0}), variant(good, **{field: -50.0})]
    for m in bad:
        assert pp.set_lens_models([0, 4], [good, m]) == abi.VIO_EINVAL           # the valid entry ahead of it is not applied
    assert pp.set_lens_models([0, 0], [good, good]) == abi.VIO_EINVAL            # a slot named twice
    assert pp.set_lens_models([6], [good]) == abi.VIO_EINVAL and pp.set_lens_models([-1], [good]) == abi.VIO_EINVAL
    assert pp.set_lens_models([4, 4], None) == abi.VIO_EINVAL and pp.set_lens_models([6], None) == abi.VIO_EINVAL
    lib = abi.load_product()
    assert lib.vio_preprocess_set_lens_models(None, 0, None, None) == abi.VIO_EINVAL
    assert lib.vio_preprocess_set_lens_models(pp._h, 1, None, None) == abi.VIO_EINVAL
    assert lib.vio_preprocess_get_lens_model(pp._h, 6, C.byref(abi.VioLensModel()), C.byref(C.c_int32())) == abi.VIO_EINVAL
    # nothing of all that took: the table reads as before and the batch computes as before
    assert table == [None if pp.get_lens_model(k) is None else bytes(pp.get_lens_model(k)) for k in range(6)]
    gray, eq = pp.run(frames)
    check(gray, wg, "gray")
    check(eq, we, "equalized")
    pp.close()


def test_contexts_that_use_the_old_setter_or_none_compute_what_they_always_did():
    """Passes before lens models existed, by design: lens_cases.py's restatement, not this change's."""
    rows, cols, rgba = 72, 100, True
    frames = np.stack([LC.random_frame(11 * k + rows, rows, cols, rgba) for k in range(3)])
    old = pkg.frontend.Preprocessor(rows, cols, max_frames=3)
    assert old.set_lenses([0, 2], [LC.lens_a(rows, cols), LC.lens_c(rows, cols)]) == abi.VIO_OK
    gray, eq = old.run(frames)
    want = [LC.rectify(frames[0], LC.lens_a(rows, cols)), LC.gray_of(frames[1]).astype(np.uint8), LC.rectify(frames[2], LC.lens_c(rows, cols))]
    for k in range(3):
        assert np.array_equal(gray[k], want[k]) and np.array_equal(eq[k], H.oracle_preprocess(want[k])[1]), k
    old.close()
    none = pkg.frontend.Preprocessor(rows, cols, max_frames=3)
    gray, eq = none.run(frames)
    for k in range(3):
        g0, e0 = H.oracle_preprocess(frames[k])
        assert np.array_equal(gray[k], g0) and np.array_equal(eq[k], e0) and none.get_lens(k) is None
    none.close()
