"""Native-size source frames of the image pre-step, the parts that need no device: the new symbols, the per-pixel functions of
csrc/pre_source.h (the text the kernel compiles) as a stand-alone host program against the numpy restatement (source_cases.py),
what identity sources reduce to, the geometry of the scaling against vio_source_camera, vio_source_check and vio_source_camera."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import lens_cases as LC
import source_cases as SC
from helpers import abi

NEW_SYMBOLS = ["vio_source_check", "vio_source_camera", "vio_preprocess_set_sources", "vio_preprocess_get_source",
               "vio_preprocess_run_frames", "vio_preprocess_run_frames_resident"]


def test_the_new_symbols_are_in_the_header_the_library_and_abi_py():
    txt = open(os.path.join(H.ROOT, "include", "vio_amd.h")).read()
    lib = abi.load_product()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s      # bound in abi.load_product
    assert "typedef struct VioSource" in txt
    assert C.sizeof(abi.VioSource) == 9 * 4 and abi.VioSource.stride.offset == 16 and abi.VioSource.crop_rows.offset == 32
    for name in ("VIO_PIXEL_GRAY8", "VIO_PIXEL_RGBA8", "VIO_PIXEL_BGRA8", "VIO_PIXEL_NV12"):
        assert re.search(r"#define %s\s+%d\b" % (name, getattr(abi, name)), txt), name


@pytest.fixture(scope="module")
def scale_program():
    """tests/emul/source_scale: pre_source.h with a main of its own, built for the host without contraction."""
    csrc, inc = os.path.join(H.ROOT, "vins-mobile_amd", "csrc"), os.path.join(H.ROOT, "include")
    exe, src = os.path.join(H.EMUL_DIR, "source_scale"), os.path.join(H.EMUL_DIR, "source_scale_main.cpp")
    deps = [src, os.path.join(csrc, "pre_source.h"), os.path.join(csrc, "pre_rectify.h"), os.path.join(inc, "vio_amd.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + inc, "-I" + csrc, "-o", exe, src])
    return exe


def run_program(exe, tmp_path, plane, src, lens, rows, cols):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([rows, cols, lens is not None, 0], np.int32).tobytes())
        f.write(bytes(src))
        f.write(bytes(lens if lens is not None else abi.VioLens()))
        f.write(np.ascontiguousarray(plane, np.uint8).tobytes())
    subprocess.check_call([exe, fin, fout])
    return np.fromfile(fout, np.uint8).reshape(rows, cols)


# the six slots at 72 x 100, the first two also at 64 x 96
HEADER_CASES = [(72, 100, k) for k in range(6)] + [(64, 96, 0), (64, 96, 1)]


@pytest.mark.parametrize("rows,cols,k", HEADER_CASES)
def test_shared_header_on_the_host_equals_the_restatement_bit_for_bit(rows, cols, k, scale_program, tmp_path):
    src, lens = SC.mixed_batch(rows, cols)[k]
    plane = SC.mixed_planes(rows, cols)[k]
    assert abi.source_check(src, rows, cols) == abi.VIO_OK
    got = run_program(scale_program, tmp_path, plane, src, lens, rows, cols)
    want = SC.mixed_expected(rows, cols)[k]
    assert np.array_equal(got, want), int((got != want).sum())
    assert len(np.unique(want)) > 30                       # an image, not a constant


def test_the_cases_are_the_ratios_they_are_meant_to_be():
    rows, cols = 72, 100
    D = []
    for src, _ in SC.mixed_batch(rows, cols)[:4]:
        D.append(SC.weights(src.crop_cols, cols)[1] * SC.weights(src.crop_rows, rows)[1])
    assert D == [4, 81, 37541, 1]
    assert [SC.samples_per_axis(s, rows, cols) for s, _ in SC.mixed_batch(rows, cols)[4:]] == [2, 3]


@pytest.mark.parametrize("rows,cols", [(72, 100), (64, 96)])
def test_no_sample_coordinate_of_the_lensed_inputs_is_near_a_rounding_tie(rows, cols):
    """As in test_lens_cpu.py: bit-exactness between the restatement and the C++ is a fair demand only while no 32 u sits on
    a tie within the double rounding of the formula (about 1e-13)."""
    for src, lens in SC.mixed_batch(rows, cols)[4:]:
        d = SC.tie_distance(src, lens, rows, cols)
        print("closest approach to a tie:", d)
        assert d > 1e-10


@pytest.mark.parametrize("rows,cols", [(72, 100), (64, 96)])
def test_identity_sources_are_the_gray_of_today(rows, cols, scale_program, tmp_path):
    rgba = LC.random_frame(3, rows, cols, True)
    gray = LC.random_frame(4, rows, cols, False)
    bgra = np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])
    want_rgba = LC.gray_of(rgba).astype(np.uint8)
    cases = [(abi.make_source(abi.VIO_PIXEL_RGBA8, rows, cols), rgba, want_rgba),
             (abi.make_source(abi.VIO_PIXEL_BGRA8, rows, cols), bgra, want_rgba),
             (abi.make_source(abi.VIO_PIXEL_GRAY8, rows, cols), gray, gray),
             (abi.make_source(abi.VIO_PIXEL_NV12, rows, cols), gray, gray),
             (abi.make_source(abi.VIO_PIXEL_NV12, rows, cols, range=1), gray, SC.video_range(gray.astype(np.int64)).astype(np.uint8)),
             (abi.make_source(abi.VIO_PIXEL_GRAY8, rows, cols, range=1), gray, SC.video_range(gray.astype(np.int64)).astype(np.uint8))]
    for src, frame, want in cases:
        assert np.array_equal(SC.expected_gray(frame.ravel(), src, None, rows, cols), want)
        assert np.array_equal(run_program(scale_program, tmp_path, frame, src, None, rows, cols), want)
    # the range map itself: 16 -> 0, 235 -> 255, and saturating outside
    y = np.arange(256, dtype=np.int64)
    m = SC.video_range(y)
    assert m[0] == m[16] == 0 and m[235] == m[255] == 255 and m[126] == 128 and (np.diff(m) >= 0).all()
    # a lens in an identity-size slot (s = 1) is lens_cases.rectify
    for frame, src in ((rgba, cases[0][0]), (gray, cases[2][0])):
        for lens in (LC.lens_a(rows, cols), LC.lens_c(rows, cols)):
            assert SC.samples_per_axis(src, rows, cols) == 1
            want = LC.rectify(frame, lens)
            assert np.array_equal(SC.expected_gray(frame.ravel(), src, lens, rows, cols), want)
            assert np.array_equal(run_program(scale_program, tmp_path, frame, src, lens, rows, cols), want)


def ramp_plane(src, a, b, c):
    """a * u + b * v + c over the delivered frame, rounded to 8 bits, as a GRAY8 plane of src's stride."""
    v, u = np.mgrid[0:src.rows, 0:src.cols].astype(np.float64)
    plane = np.zeros((src.rows, src.stride), np.uint8)
    plane[:, :src.cols] = np.rint(a * u + b * v + c)
    return plane.ravel()


def output_centres(src, rows, cols):
    """Where vio_source_camera puts the output pixel centres in the delivered frame: x = fx' u + cx' inverted."""
    fx, fy, cx, cy = abi.source_camera(src, rows, cols, 1.0, 1.0, 0.0, 0.0)
    return (np.arange(cols, dtype=np.float64)[None, :] - cx) / fx, (np.arange(rows, dtype=np.float64)[:, None] - cy) / fy


RAMP_CASES = [(72, 100, abi.make_source(abi.VIO_PIXEL_GRAY8, 144, 200)),
              (72, 100, abi.make_source(abi.VIO_PIXEL_GRAY8, 162, 225)),
              (72, 100, abi.make_source(abi.VIO_PIXEL_GRAY8, 200, 301, stride=304, crop=(7, 5, 217, 173))),
              (64, 96, abi.make_source(abi.VIO_PIXEL_GRAY8, 144, 200)),
              (480, 640, abi.make_source(abi.VIO_PIXEL_GRAY8, 1080, 1920, crop=(240, 0, 1440, 1080))),
              (480, 640, abi.make_source(abi.VIO_PIXEL_GRAY8, 2159, 3839))]


@pytest.mark.parametrize("rows,cols,src", RAMP_CASES)
def test_the_area_average_of_a_ramp_is_the_ramp_at_the_mapped_pixel_centre(rows, cols, src, scale_program, tmp_path):
    """The area average of a linear ramp over an output pixel's footprint is the ramp at the footprint's centre, which is where
    vio_source_camera's mapping puts the output pixel centre. Rounding the ramp to bytes at the source size moves every source
    pixel, hence their weighted mean, by at most 0.5; the final division rounds by at most 0.5: 1 gray level in all."""
    assert abi.source_check(src, rows, cols) == abi.VIO_OK
    a, b, c = 200.0 / src.cols, 40.0 / src.rows, 7.3
    plane = ramp_plane(src, a, b, c)
    got = run_program(scale_program, tmp_path, plane, src, None, rows, cols)         # csrc/pre_source.h itself ...
    assert np.array_equal(got, SC.expected_gray(plane, src, None, rows, cols))      # ... which is the restatement here too
    got = got.astype(np.float64)
    u, v = output_centres(src, rows, cols)
    err = np.abs(got - (a * u + b * v + c)).max()
    print("max error (gray levels):", err)
    assert err <= 1.0


@pytest.mark.parametrize("rows,cols,srows,scols", [(72, 100, 144, 200), (72, 100, 162, 225), (64, 96, 144, 200), (72, 100, 72, 100)])
def test_a_ramp_through_an_undistorted_lens_lands_where_the_camera_mapping_says(rows, cols, srows, scols, scale_program, tmp_path):
    """A lens without distortion whose rect_* are vio_source_camera's of its raw pinhole samples the delivered frame at the
    affine image of (x + dx, y + dy); the s * s offsets are symmetric about 0, so on a linear ramp their mean is the ramp at the
    mapped pixel centre. What the arithmetic adds, in gray levels, with g = |a| + |b| the ramp's slope per source pixel:
      0.5      the ramp rounded to bytes (a bilinear sample is a convex combination of four such bytes, exact on a linear ramp)
      g / 64   the sample position rounded to 1/32 pixel, at most 1/64 on each axis
      0.5      the rounding of each blend, (.. + 512) >> 10
      0.5      the rounding of the mean (none with s = 1, where the mean is the sample)
      g * e    samples clamped at the frame's edge: the outermost sample lies k (s - 1) / (2 s) source pixels from the centre and
               the centre of pixel 0 lies (k - 1) / 2 from the edge, k the scale; e is by how much the first exceeds the second."""
    src = abi.make_source(abi.VIO_PIXEL_GRAY8, srows, scols)
    raw = (0.9 * scols, 0.95 * scols, scols / 2 - 2.2, srows / 2 + 1.4)
    lens = abi.make_lens(*raw, rect=abi.source_camera(src, rows, cols, *raw))
    a, b, c = 200.0 / scols, 40.0 / srows, 7.3
    plane = ramp_plane(src, a, b, c)
    got = run_program(scale_program, tmp_path, plane, src, lens, rows, cols)
    assert np.array_equal(got, SC.expected_gray(plane, src, lens, rows, cols))
    got = got.astype(np.float64)
    u, v = output_centres(src, rows, cols)
    s, g = SC.samples_per_axis(src, rows, cols), a + b
    e = max(0.0, max(k * (s - 1) / (2 * s) - (k - 1) / 2 for k in (scols / cols, srows / rows)))
    bound = 0.5 + g / 64 + 0.5 + (0.5 if s > 1 else 0.0) + g * e
    err = np.abs(got - (a * u + b * v + c)).max()
    print("s = %d, max error %.3f, bound %.3f" % (s, err, bound))
    assert err <= bound


def changed(src, **kw):
    out = abi.VioSource.from_buffer_copy(bytes(src))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def test_source_check_refuses_what_the_header_lists():
    rows, cols, ok, bad = 72, 100, abi.VIO_OK, abi.VIO_EINVAL
    rgba = abi.make_source(abi.VIO_PIXEL_RGBA8, 144, 200)
    gray = abi.make_source(abi.VIO_PIXEL_GRAY8, 200, 301, stride=304, crop=(7, 5, 217, 173))
    assert abi.source_check(rgba, rows, cols) == ok and abi.source_check(gray, rows, cols) == ok
    assert abi.load_product().vio_source_check(None, rows, cols) == bad
    for fmt in (0, 2, 3, 6, 11, 13, -1):
        assert abi.source_check(changed(gray, format=fmt), rows, cols) == bad, fmt
    for fmt in (abi.VIO_PIXEL_GRAY8, abi.VIO_PIXEL_NV12):
        assert abi.source_check(changed(gray, format=fmt, range=1), rows, cols) == ok
        assert abi.source_check(changed(gray, format=fmt, range=2), rows, cols) == bad
        assert abi.source_check(changed(gray, format=fmt, range=-1), rows, cols) == bad
    for fmt in (abi.VIO_PIXEL_RGBA8, abi.VIO_PIXEL_BGRA8):
        assert abi.source_check(changed(rgba, format=fmt), rows, cols) == ok
        assert abi.source_check(changed(rgba, format=fmt, range=1), rows, cols) == bad
    # the size of the frame
    assert abi.source_check(changed(gray, rows=0), rows, cols) == bad and abi.source_check(changed(gray, cols=0), rows, cols) == bad
    assert abi.source_check(abi.make_source(abi.VIO_PIXEL_GRAY8, 16384, 200), 16384 // 4, cols) == ok
    assert abi.source_check(abi.make_source(abi.VIO_PIXEL_GRAY8, 16385, 200), 16385 // 4, cols) == bad
    assert abi.source_check(abi.make_source(abi.VIO_PIXEL_GRAY8, 144, 16384), rows, 16384 // 4) == ok
    assert abi.source_check(abi.make_source(abi.VIO_PIXEL_GRAY8, 144, 16385), rows, 16385 // 4) == bad
    # the stride
    assert abi.source_check(changed(gray, stride=301), rows, cols) == ok and abi.source_check(changed(gray, stride=300), rows, cols) == bad
    assert abi.source_check(changed(rgba, stride=800), rows, cols) == ok and abi.source_check(changed(rgba, stride=796), rows, cols) == bad
    assert abi.source_check(changed(rgba, stride=804), rows, cols) == ok and abi.source_check(changed(rgba, stride=802), rows, cols) == bad
    # the crop lies inside the frame
    assert abi.source_check(changed(gray, crop_x=301 - 217), rows, cols) == ok
    assert abi.source_check(changed(gray, crop_x=301 - 217 + 1), rows, cols) == bad
    assert abi.source_check(changed(gray, crop_y=200 - 173), rows, cols) == ok
    assert abi.source_check(changed(gray, crop_y=200 - 173 + 1), rows, cols) == bad
    assert abi.source_check(changed(gray, crop_x=-1), rows, cols) == bad and abi.source_check(changed(gray, crop_y=-1), rows, cols) == bad
    assert abi.source_check(changed(gray, crop_cols=0), rows, cols) == bad and abi.source_check(changed(gray, crop_rows=0), rows, cols) == bad
    # no upscaling, at most 8 x
    assert abi.source_check(changed(gray, crop_cols=100, crop_rows=72), rows, cols) == ok
    assert abi.source_check(changed(gray, crop_cols=99), rows, cols) == bad and abi.source_check(changed(gray, crop_rows=71), rows, cols) == bad
    wide = abi.make_source(abi.VIO_PIXEL_GRAY8, 600, 900)
    assert abi.source_check(changed(wide, crop_cols=800, crop_rows=576), rows, cols) == ok
    assert abi.source_check(changed(wide, crop_cols=801, crop_rows=576), rows, cols) == bad
    assert abi.source_check(changed(wide, crop_cols=800, crop_rows=577), rows, cols) == bad
    # 255 * cw * ch < 2^32 (2^32 / 255 = 16843009.003): coprime pairs at a 2100 x 2100 output, just below and just above
    big = abi.make_source(abi.VIO_PIXEL_GRAY8, 8000, 8000)
    for cw, ch, want in ((3779, 4457, ok), (2489, 6767, bad)):
        assert np.gcd(cw, 2100) == 1 and np.gcd(ch, 2100) == 1
        assert (255 * cw * ch < 2 ** 32) == (want == ok)
        assert abi.source_check(changed(big, crop_cols=cw, crop_rows=ch), 2100, 2100) == want, (cw, ch)
    assert 255 * 3779 * 4457 > 2 ** 32 - 2000 and 255 * 2489 * 6767 < 2 ** 32 + 20000


def test_source_camera_is_the_formula_and_the_identity_for_an_identity_source():
    rows, cols = 72, 100
    pin = (161.3, 164.9, 98.7, 71.2)
    for src, _ in SC.mixed_batch(rows, cols)[:4]:
        got, want = abi.source_camera(src, rows, cols, *pin), SC.camera(src, rows, cols, *pin)
        assert np.allclose(got, want, rtol=1e-14, atol=1e-12), (got, want)
    ident = abi.make_source(abi.VIO_PIXEL_RGBA8, rows, cols)
    assert abi.source_camera(ident, rows, cols, *pin) == pin
    # half the size: the focal length halves and pixel centres map to pixel centres
    half = abi.make_source(abi.VIO_PIXEL_RGBA8, 2 * rows, 2 * cols)
    assert np.allclose(abi.source_camera(half, rows, cols, 100.0, 100.0, 0.5, 0.5), (50.0, 50.0, 0.0, 0.0), atol=1e-14)
    lib, out = abi.load_product(), (C.c_double * 4)()
    assert lib.vio_source_camera(C.byref(changed(ident, crop_cols=cols - 1)), rows, cols, (C.c_double * 4)(*pin), out) == abi.VIO_EINVAL
    assert lib.vio_source_camera(None, rows, cols, (C.c_double * 4)(*pin), out) == abi.VIO_EINVAL
