"""Lens rectification inside the image pre-step on the device: the frames of a slot that holds a lens are rectified while they
are converted to gray. gray_out equals the numpy restatement (lens_cases.py) bit for bit and the equalized frame is the oracle's
CLAHE of that rectified gray; slots without a lens, and a context that never set one, give what they always gave."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import lens_cases as LC
from helpers import abi, pkg

pytestmark = pytest.mark.gpu

# 72 x 100 is no multiple of the 8 x 8 grid (reflect extension, byte stores of the apply pass); 64 x 96 is (dword stores)
SHAPES = [(72, 100, False), (72, 100, True), (64, 96, True)]


def batch(rows, cols, rgba):
    return np.stack([LC.random_frame(11 * k + rows, rows, cols, rgba) for k in range(3)])


def mixed(rows, cols):
    """slot 0: lens A, slot 1: none, slot 2: lens C"""
    return [0, 2], [LC.lens_a(rows, cols), LC.lens_c(rows, cols)]


_want = {}


def expected(rows, cols, rgba):
    """(gray, equalized) of the mixed batch, computed once per shape and never written to."""
    key = (rows, cols, rgba)
    if key not in _want:
        frames = batch(rows, cols, rgba)
        gray = [LC.rectify(frames[0], LC.lens_a(rows, cols)), LC.gray_of(frames[1]).astype(np.uint8),
                LC.rectify(frames[2], LC.lens_c(rows, cols))]
        eq = [H.oracle_preprocess(g)[1] for g in gray]
        assert np.array_equal(H.oracle_preprocess(frames[1])[0], gray[1])
        g, e = np.stack(gray), np.stack(eq)
        g.flags.writeable = e.flags.writeable = False
        _want[key] = (g, e)
    return _want[key]


@pytest.mark.parametrize("rows,cols,rgba", SHAPES)
def test_mixed_batch_host_route(rows, cols, rgba):
    frames = batch(rows, cols, rgba)
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=3)
    slots, lenses = mixed(rows, cols)
    assert pp.set_lenses(slots, lenses) == abi.VIO_OK
    gray, eq = pp.run(frames)
    wg, we = expected(rows, cols, rgba)
    for k in range(3):
        assert np.array_equal(gray[k], wg[k]), (k, int((gray[k] != wg[k]).sum()))
        assert np.array_equal(eq[k], we[k]), (k, int((eq[k] != we[k]).sum()))
    assert LC.n_outside(lenses[1], rows, cols) > 0 and (wg[0] != LC.gray_of(frames[0])).mean() > 0.5
    got = pp.get_lens(0)
    assert bytes(got) == bytes(lenses[0]) and pp.get_lens(1) is None and bytes(pp.get_lens(2)) == bytes(lenses[1])
    pp.close()


class Hip:
    def __init__(self):
        hip = C.CDLL("libamdhip64.so")                       # the runtime libvio_amd.so is linked against
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        hip.hipStreamDestroy.argtypes = [C.c_void_p]
        self.hip = hip

    def upload(self, a):
        d = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(d), a.nbytes) == 0 and self.hip.hipMemcpy(d, a.ctypes.data, a.nbytes, 1) == 0
        return d

    def download(self, d, a):
        assert self.hip.hipMemcpy(a.ctypes.data, d, a.nbytes, 2) == 0
        return a


@pytest.mark.parametrize("rows,cols,rgba", SHAPES)
def test_mixed_batch_resident_route_on_a_caller_stream(rows, cols, rgba):
    frames = batch(rows, cols, rgba)
    h = Hip()
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=3)
    assert pp.set_lenses(*mixed(rows, cols)) == abi.VIO_OK
    stream = C.c_void_p()
    assert h.hip.hipStreamCreate(C.byref(stream)) == 0
    d_in, d_eq = h.upload(frames), h.upload(np.zeros((3, rows, cols), np.uint8))
    pp.run_resident(d_in.value, 4 if rgba else 1, 3, d_eq.value, stream=stream.value)
    pp.sync()
    eq = h.download(d_eq, np.zeros((3, rows, cols), np.uint8))
    we = expected(rows, cols, rgba)[1]
    for k in range(3):
        assert np.array_equal(eq[k], we[k]), (k, int((eq[k] != we[k]).sum()))
    h.hip.hipFree(d_in), h.hip.hipFree(d_eq), h.hip.hipStreamDestroy(stream)
    pp.close()


def test_clearing_and_replacing():
    rows, cols, rgba = 72, 100, True
    frames = batch(rows, cols, rgba)
    wg, we = expected(rows, cols, rgba)
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=3)
    assert pp.set_lenses(*mixed(rows, cols)) == abi.VIO_OK
    assert np.array_equal(pp.run(frames)[0][0], wg[0])
    # clear lens A: slot 0 is the raw gray again, slot 2 keeps its lens
    assert pp.set_lenses([0], None) == abi.VIO_OK and pp.get_lens(0) is None
    gray, eq = pp.run(frames)
    g0, e0 = H.oracle_preprocess(frames[0])
    assert np.array_equal(gray[0], g0) and np.array_equal(eq[0], e0)
    assert np.array_equal(gray[2], wg[2]) and np.array_equal(eq[2], we[2])
    # set twice with different values: the second holds (lens C in slot 0, then lens A)
    assert pp.set_lenses([0], [LC.lens_c(rows, cols)]) == abi.VIO_OK
    assert pp.set_lenses([0], [LC.lens_a(rows, cols)]) == abi.VIO_OK
    gray, eq = pp.run(frames)
    assert np.array_equal(gray[0], wg[0]) and np.array_equal(eq[0], we[0])
    # clearing every slot brings the context back to the kernel without lenses
    assert pp.set_lenses([0, 1, 2], None) == abi.VIO_OK
    gray, eq = pp.run(frames)
    for k in range(3):
        g0, e0 = H.oracle_preprocess(frames[k])
        assert np.array_equal(gray[k], g0) and np.array_equal(eq[k], e0)
    pp.close()


def test_a_context_without_lenses_gives_what_it_always_gave():
    """The inputs of test_preprocess.py's 136 x 100 case, and what that test expects of them."""
    from test_preprocess import _scene
    rows, cols = 136, 100
    rng = np.random.default_rng(rows + cols)
    frames = np.stack([_scene(rng, rows, cols, False) for _ in range(3)])
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=3)
    gray, eq = pp.run(frames)
    for k in range(3):
        g0, e0 = H.oracle_preprocess(frames[k])
        assert np.array_equal(gray[k], g0) and np.array_equal(eq[k], e0)
        assert pp.get_lens(k) is None
    pp.close()


def test_argument_errors_change_nothing():
    rows, cols, rgba = 64, 96, True
    frames = batch(rows, cols, rgba)
    wg, we = expected(rows, cols, rgba)
    pp = pkg.frontend.Preprocessor(rows, cols, max_frames=3)
    slots, lenses = mixed(rows, cols)
    assert pp.set_lenses(slots, lenses) == abi.VIO_OK
    A, Cc = lenses
    other = LC.identity_lens(rows, cols)
    assert pp.set_lenses([3], [other]) == abi.VIO_EINVAL and pp.set_lenses([-1], [other]) == abi.VIO_EINVAL
    assert pp.set_lenses([1, 3], [other, other]) == abi.VIO_EINVAL            # the valid entry ahead of it is not applied
    assert pp.set_lenses([1, 1], [other, other]) == abi.VIO_EINVAL            # a slot named twice
    assert pp.set_lenses([0, 0], None) == abi.VIO_EINVAL and pp.set_lenses([3], None) == abi.VIO_EINVAL
    for field in [k for k, _ in abi.VioLens._fields_]:
        for value in (float("nan"), float("inf")):
            bad = abi.VioLens.from_buffer_copy(bytes(other))
            setattr(bad, field, value)
            assert pp.set_lenses([1, 0], [other, bad]) == abi.VIO_EINVAL, (field, value)
    for field in ("fx", "fy", "rect_fx", "rect_fy"):
        for value in (0.0, -50.0):
            bad = abi.VioLens.from_buffer_copy(bytes(other))
            setattr(bad, field, value)
            assert pp.set_lenses([0], [bad]) == abi.VIO_EINVAL, (field, value)
    lib = abi.load_product()
    assert lib.vio_preprocess_set_lenses(None, 0, None, None) == abi.VIO_EINVAL
    assert lib.vio_preprocess_set_lenses(pp._h, 1, None, None) == abi.VIO_EINVAL
    assert lib.vio_preprocess_get_lens(pp._h, 3, C.byref(abi.VioLens()), C.byref(C.c_int32())) == abi.VIO_EINVAL
    # nothing of all that took: the table reads as before and the batch computes as before
    assert bytes(pp.get_lens(0)) == bytes(A) and pp.get_lens(1) is None and bytes(pp.get_lens(2)) == bytes(Cc)
    gray, eq = pp.run(frames)
    for k in range(3):
        assert np.array_equal(gray[k], wg[k]) and np.array_equal(eq[k], we[k])
    pp.close()
