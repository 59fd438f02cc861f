"""Native-size source frames in the image pre-step on the device: every slot's frame is taken where it lies, in its own size,
stride, format and range, and scaled (or rectified) to the context's rows x cols inside the gray pass. gray_out equals the numpy
restatement (source_cases.py) bit for bit, the equalized frame is the oracle's CLAHE of that gray, and the old entries compute
what they always did."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import lens_cases as LC
import source_cases as SC
from device_buffers import Hip
from helpers import abi, pkg

pytestmark = pytest.mark.gpu

# 72 x 100 is no multiple of the 8 x 8 grid (reflect extension, byte stores of the apply pass); 64 x 96 is (dword stores)
SHAPES = [(72, 100), (64, 96)]

_eq = {}


def expected(rows, cols, second=False):
    """(gray, equalized) of the mixed batch (second: of its second set of planes), computed once and never written to."""
    key = (rows, cols, second)
    if key not in _eq:
        if second:
            g = np.stack([SC.expected_gray(b, s, l, rows, cols) for b, (s, l) in zip(second_planes(rows, cols), SC.mixed_batch(rows, cols))])
        else:
            g = SC.mixed_expected(rows, cols)
        e = np.stack([H.oracle_preprocess(np.ascontiguousarray(x))[1] for x in g])
        e.flags.writeable = False
        _eq[key] = (g, e)
    return _eq[key]


def second_planes(rows, cols):
    return [SC.random_plane(1000 + 13 * k + rows, src) for k, (src, _) in enumerate(SC.mixed_batch(rows, cols))]


def context(rows, cols):
    batch = SC.mixed_batch(rows, cols)
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=len(batch))
    assert pp.set_sources(range(len(batch)), [s for s, _ in batch]) == abi.VIO_OK
    lensed = [k for k, (_, l) in enumerate(batch) if l is not None]
    assert pp.set_lenses(lensed, [batch[k][1] for k in lensed]) == abi.VIO_OK
    return pp


def check(got, want, what):
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_mixed_batch_host_route(rows, cols):
    pp = context(rows, cols)
    pp.kernel_ms()
    rc, gray, eq = pp.run_frames(SC.mixed_planes(rows, cols))
    assert rc == abi.VIO_OK
    wg, we = expected(rows, cols)
    check(gray, wg, "gray")
    check(eq, we, "equalized")
    assert pp.kernel_ms()[1] == 1                           # one launch of the gray pass and one of the apply pass
    rc, none, eq = pp.run_frames(SC.mixed_planes(rows, cols), want_gray=False)
    assert rc == abi.VIO_OK and none is None
    check(eq, we, "equalized without gray_out")
    pp.close()


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_mixed_batch_resident_route_on_a_caller_stream(rows, cols):
    h, pp = Hip(), context(rows, cols)
    planes = SC.mixed_planes(rows, cols)
    n = len(planes)
    stream = C.c_void_p()
    assert h.hip.hipStreamCreate(C.byref(stream)) == 0
    d_in = [h.upload(p) for p in planes]                    # six allocations of their own
    d_eq = h.upload(np.zeros((n, rows, cols), np.uint8))
    ptrs = [d.value for d in d_in]
    assert pp.run_frames_resident([ptrs[0] + 2] + ptrs[1:], d_eq.value, stream=stream.value) == abi.VIO_EINVAL   # RGBA, 2 bytes off
    pp.kernel_ms()
    assert pp.run_frames_resident(ptrs, d_eq.value, stream=stream.value) == abi.VIO_OK
    pp.sync()
    assert pp.kernel_ms()[1] == 1
    eq = h.download(d_eq, np.zeros((n, rows, cols), np.uint8))
    check(eq, expected(rows, cols)[1], "equalized")
    for d in d_in + [d_eq]:
        h.hip.hipFree(d)
    h.hip.hipStreamDestroy(stream)
    pp.close()


def test_two_resident_calls_back_to_back_keep_their_own_frame_tables():
    rows, cols = 72, 100
    h, pp = Hip(), context(rows, cols)
    first, second = SC.mixed_planes(rows, cols), second_planes(rows, cols)
    n = len(first)
    stream = C.c_void_p()
    assert h.hip.hipStreamCreate(C.byref(stream)) == 0
    d_a, d_b = [h.upload(p) for p in first], [h.upload(p) for p in second]
    out_a, out_b = h.upload(np.zeros((n, rows, cols), np.uint8)), h.upload(np.zeros((n, rows, cols), np.uint8))
    assert pp.run_frames_resident([d.value for d in d_a], out_a.value, stream=stream.value) == abi.VIO_OK
    assert pp.run_frames_resident([d.value for d in d_b], out_b.value, stream=stream.value) == abi.VIO_OK   # no sync in between
    pp.sync()
    check(h.download(out_a, np.zeros((n, rows, cols), np.uint8)), expected(rows, cols)[1], "first call")
    check(h.download(out_b, np.zeros((n, rows, cols), np.uint8)), expected(rows, cols, second=True)[1], "second call")
    assert not np.array_equal(expected(rows, cols)[1], expected(rows, cols, second=True)[1])
    for d in d_a + d_b + [out_a, out_b]:
        h.hip.hipFree(d)
    h.hip.hipStreamDestroy(stream)
    pp.close()


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_identity_sources_give_what_run_gives_and_run_is_untouched(rows, cols):
    rgba = np.stack([LC.random_frame(7 * k + rows, rows, cols, True) for k in range(3)])
    gray = np.stack([LC.random_frame(9 * k + cols, rows, cols, False) for k in range(3)])
    plain = pkg.frontend.Preprocessor(rows, cols, max_frames=3)
    want_rgba, want_gray = plain.run(rgba), plain.run(gray)
    plain.close()
    check(want_rgba[0], [H.oracle_preprocess(f)[0] for f in rgba], "run itself")
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=3)
    assert pp.run_frames(list(rgba))[0] == abi.VIO_ESTATE                       # no slot holds a source
    assert pp.set_sources([0, 1], [abi.make_source(abi.VIO_PIXEL_RGBA8, rows, cols)] * 2) == abi.VIO_OK
    assert pp.run_frames(list(rgba))[0] == abi.VIO_ESTATE                       # slot 2 holds none
    h = Hip()
    d = h.upload(rgba)
    assert pp.run_frames_resident([d.value] * 3, d.value) == abi.VIO_ESTATE
    h.hip.hipFree(d)
    rc, g, e = pp.run_frames(list(rgba[:2]))                                    # ... and a call that stays below it runs
    assert rc == abi.VIO_OK
    check(g, want_rgba[0][:2], "gray of 2 frames"), check(e, want_rgba[1][:2], "equalized of 2 frames")
    assert pp.set_sources([2], [abi.make_source(abi.VIO_PIXEL_RGBA8, rows, cols)]) == abi.VIO_OK
    rc, g, e = pp.run_frames(list(rgba))
    assert rc == abi.VIO_OK
    check(g, want_rgba[0], "identity RGBA gray"), check(e, want_rgba[1], "identity RGBA equalized")
    # the old entry on a context that holds sources: frames of rows x cols with `channels`, as ever
    g, e = pp.run(gray)
    check(g, want_gray[0], "run, gray"), check(e, want_gray[1], "run, equalized")
    g, e = pp.run(rgba)
    check(g, want_rgba[0], "run, RGBA gray"), check(e, want_rgba[1], "run, RGBA equalized")
    assert pp.set_sources([0, 1, 2], [abi.make_source(abi.VIO_PIXEL_GRAY8, rows, cols)] * 3) == abi.VIO_OK
    rc, g, e = pp.run_frames(list(gray))
    assert rc == abi.VIO_OK
    check(g, want_gray[0], "identity gray"), check(e, want_gray[1], "identity gray equalized")
    pp.close()


def test_clearing_and_replacing():
    rows, cols = 72, 100
    pp, planes, batch = context(rows, cols), SC.mixed_planes(rows, cols), SC.mixed_batch(rows, cols)
    wg, we = expected(rows, cols)
    # clear slot 1: a call that reaches it is refused, a shorter one still runs; the other slots keep their sources
    assert pp.set_sources([1], None) == abi.VIO_OK and pp.get_source(1) is None
    assert pp.run_frames(planes)[0] == abi.VIO_ESTATE
    rc, g, _ = pp.run_frames(planes[:1])
    assert rc == abi.VIO_OK and np.array_equal(g[0], wg[0])
    # set twice with different values: the second holds
    assert pp.set_sources([1], [abi.make_source(abi.VIO_PIXEL_RGBA8, 162, 225)]) == abi.VIO_OK
    rc, g, _ = pp.run_frames(planes)
    assert rc == abi.VIO_OK and not np.array_equal(g[1], wg[1])                # read as RGBA, R and B change places
    assert pp.set_sources([1], [batch[1][0]]) == abi.VIO_OK
    rc, g, e = pp.run_frames(planes)
    assert rc == abi.VIO_OK
    check(g, wg, "gray"), check(e, we, "equalized")
    # clearing a lens leaves the source: slot 4 is then the area average of its crop
    assert pp.set_lenses([4], None) == abi.VIO_OK
    rc, g, _ = pp.run_frames(planes)
    assert rc == abi.VIO_OK and np.array_equal(g[4], SC.expected_gray(planes[4], batch[4][0], None, rows, cols))
    assert np.array_equal(g[5], wg[5])
    pp.close()


def test_argument_errors_change_nothing():
    rows, cols = 64, 96
    pp, planes, batch = context(rows, cols), SC.mixed_planes(rows, cols), SC.mixed_batch(rows, cols)
    n, other = len(batch), abi.make_source(abi.VIO_PIXEL_GRAY8, rows, cols)
    assert pp.set_sources([n], [other]) == abi.VIO_EINVAL and pp.set_sources([-1], [other]) == abi.VIO_EINVAL
    assert pp.set_sources([1, n], [other, other]) == abi.VIO_EINVAL            # the valid entry ahead of it is not applied
    assert pp.set_sources([1, 1], [other, other]) == abi.VIO_EINVAL            # a slot named twice
    assert pp.set_sources([0, 0], None) == abi.VIO_EINVAL and pp.set_sources([n], None) == abi.VIO_EINVAL
    for field, value in (("format", 7), ("range", 2), ("rows", 0), ("cols", 20000), ("stride", cols - 1), ("crop_x", 1),
                         ("crop_cols", cols - 1), ("crop_rows", rows + 1)):
        bad = abi.VioSource.from_buffer_copy(bytes(other))
        setattr(bad, field, value)
        assert pp.set_sources([1, 0], [other, bad]) == abi.VIO_EINVAL, (field, value)
    lib = abi.load_product()
    assert lib.vio_preprocess_set_sources(None, 0, None, None) == abi.VIO_EINVAL
    assert lib.vio_preprocess_set_sources(pp._h, 1, None, None) == abi.VIO_EINVAL
    assert lib.vio_preprocess_get_source(pp._h, n, C.byref(abi.VioSource()), C.byref(C.c_int32())) == abi.VIO_EINVAL
    assert lib.vio_preprocess_run_frames(pp._h, None, n, None, None) == abi.VIO_EINVAL
    assert pp.run_frames(planes + planes[:1])[0] == abi.VIO_ECAP
    # nothing of all that took: the table reads as before and the batch computes as before
    for k in range(n):
        assert bytes(pp.get_source(k)) == bytes(batch[k][0]), k
    rc, g, e = pp.run_frames(planes)
    assert rc == abi.VIO_OK
    check(g, expected(rows, cols)[0], "gray"), check(e, expected(rows, cols)[1], "equalized")
    pp.close()


def test_nv12_luma_plane_alone_is_enough():
    """The buffer ends with the last byte of plane 0 (rows * stride bytes, no chroma plane behind it), at the very end of an
    array the test owns; the host route must not read past it."""
    rows, cols = 72, 100
    src = abi.make_source(abi.VIO_PIXEL_NV12, 144, 200, stride=208, crop=(0, 0, 200, 144), range=1)
    plane = SC.random_plane(5, src)
    holder = np.zeros(1 << 16, np.uint8)
    holder[-plane.size:] = plane
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=1)
    assert pp.set_sources([0], [src]) == abi.VIO_OK
    rc, g, e = pp.run_frames([holder[-plane.size:]])
    assert rc == abi.VIO_OK
    want = SC.expected_gray(plane, src, None, rows, cols)
    assert np.array_equal(g[0], want) and np.array_equal(e[0], H.oracle_preprocess(want)[1])
    pp.close()
