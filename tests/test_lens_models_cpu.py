"""Lens models of the image pre-step (VioLensModel: Brown-Conrady, rational, fisheye), the parts that need no device: the new
symbols, the per-pixel functions of csrc/pre_rectify.h and pre_source.h (the text the kernels compile) as a stand-alone host
program against the numpy restatement (lens_model_cases.py), lens_atan against numpy.arctan, the host entries
vio_lens_model_*, and how well the specified fisheye arithmetic rectifies a known scene."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import lens_cases as LC
import lens_model_cases as MC
import source_cases as SC
from helpers import abi

NEW_SYMBOLS = ["vio_preprocess_set_lens_models", "vio_preprocess_get_lens_model", "vio_lens_model_distort_points",
               "vio_lens_model_undistort_points", "vio_lens_model_coverage"]
SHAPES = [(72, 100), (64, 96)]
MODELS = ["brown_model", "rational", "fisheye_in", "fisheye_clamped"]


def build_program(name):
    """tests/emul/<name>: the shared headers with a main of their own, built for the host without contraction."""
    csrc, inc = os.path.join(H.ROOT, "vins-mobile_amd", "csrc"), os.path.join(H.ROOT, "include")
    exe, src = os.path.join(H.EMUL_DIR, name), os.path.join(H.EMUL_DIR, name + "_main.cpp")
    deps = [src, os.path.join(csrc, "pre_rectify.h"), os.path.join(csrc, "pre_source.h"), os.path.join(inc, "vio_amd.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + inc, "-I" + csrc, "-o", exe, src])
    return exe


@pytest.fixture(scope="module")
def model_program():
    return build_program("lens_model")


@pytest.fixture(scope="module")
def old_program():
    return build_program("lens_rectify")


def run_model(exe, tmp_path, frame, lens, rows=None, cols=None, source=None):
    """The host program on a rows x cols frame (gray or RGBA), or on plane 0 of a delivered frame described by `source`."""
    frame = np.ascontiguousarray(frame, np.uint8)
    if source is None:
        rows, cols = frame.shape[:2]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([rows, cols, 4 if frame.ndim == 3 else 1, 0 if source is None else 1], np.int32).tobytes())
        f.write(bytes(lens))
        if source is not None:
            f.write(bytes(source))
        f.write(frame.tobytes())
    subprocess.check_call([exe, "rectify", fin, fout])
    return np.fromfile(fout, np.uint8).reshape(rows, cols)


def run_old(exe, tmp_path, frame, lens):
    frame = np.ascontiguousarray(frame, np.uint8)
    rows, cols = frame.shape[:2]
    fin, fout = str(tmp_path / "old_in.bin"), str(tmp_path / "old_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([rows, cols, 4 if frame.ndim == 3 else 1, 0], np.int32).tobytes())
        f.write(bytes(lens))
        f.write(frame.tobytes())
    subprocess.check_call([exe, fin, fout])
    return np.fromfile(fout, np.uint8).reshape(rows, cols)


def test_the_new_symbols_are_in_the_header_the_library_and_abi_py(model_program):
    txt = open(os.path.join(H.ROOT, "include", "vio_amd.h")).read()
    lib = abi.load_product()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s      # bound in abi.load_product
    assert "typedef struct VioLensModel" in txt
    for name, value in (("BROWN", 0), ("RATIONAL", 1), ("FISHEYE", 2)):
        assert re.search(r"#define\s+VIO_LENS_%s\s+%d\b" % (name, value), txt) and getattr(abi, "VIO_LENS_" + name) == value
    # the header as a compiler lays it out == abi.py
    size, o_fx, o_k, o_rect = (int(x) for x in subprocess.check_output([model_program, "layout"]).split())
    M = abi.VioLensModel
    assert (size, o_fx, o_k, o_rect) == (C.sizeof(M), M.fx.offset, M.k.offset, M.rect_fx.offset) == (136, 8, 40, 104)


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("which", MODELS)
def test_shared_header_on_the_host_equals_the_restatement_bit_for_bit(rows, cols, which, model_program, tmp_path):
    lens = getattr(MC, which)(rows, cols)
    for rgba in (False, True):
        frame = LC.random_frame(rows + cols + rgba, rows, cols, rgba)
        got = run_model(model_program, tmp_path, frame, lens)
        want = MC.rectify(frame, lens)
        assert np.array_equal(got, want), (rgba, int((got != want).sum()))
        assert (want != LC.gray_of(frame)).mean() > 0.5        # the lens moved the frame: not a comparison of two copies


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_no_source_coordinate_of_these_inputs_is_near_a_rounding_tie(rows, cols):
    """As test_lens_cpu.py: bit-exactness between two correct implementations is a fair demand only while no 32 u sits on a tie
    within the double rounding of the formula (about 1e-13)."""
    for which in MODELS:
        d = MC.tie_distance(getattr(MC, which)(rows, cols), rows, cols, rows, cols)
        print(which, "closest approach to a tie:", d)
        assert d > 1e-10
    src, lens = supersampled_case(rows, cols)
    d = MC.tie_distance(lens, src.rows, src.cols, rows, cols, SC.sample_offsets(2))
    print("supersampled fisheye, closest approach to a tie:", d)
    assert d > 1e-10


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_brown_and_rational_without_a_divisor_give_the_bytes_of_the_same_vio_lens(rows, cols, model_program, old_program, tmp_path):
    for old in (LC.lens_a(rows, cols), LC.lens_c(rows, cols)):
        brown = abi.lens_model_of(old)
        rat = abi.lens_model_of(old)
        rat.model = abi.VIO_LENS_RATIONAL
        for rgba in (False, True):
            frame = LC.random_frame(3 + rgba, rows, cols, rgba)
            want = run_old(old_program, tmp_path, frame, old)
            assert np.array_equal(want, LC.rectify(frame, old))
            for m in (brown, rat):
                assert np.array_equal(run_model(model_program, tmp_path, frame, m), want), m.model
                assert np.array_equal(MC.rectify(frame, m), want), m.model


def scene(x, y):
    return 128 + 50 * np.sin(2.2 * x + 0.3) * np.cos(1.7 * y - 0.2) + 30 * np.sin(1.1 * x - 1.4 * y)


def equidistant_rays(f, cx, cy, u, v):
    """Raw pixel of an ideal equidistant camera (distance from the centre = f * theta) -> the ray's normalized point."""
    xd, yd = (u - cx) / f, (v - cy) / f
    th = np.hypot(xd, yd)
    s = np.where(th == 0, 1.0, np.tan(th) / np.where(th == 0, 1.0, th))
    return xd * s, yd * s


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_a_fisheye_without_coefficients_is_the_equidistant_map(rows, cols):
    """A smooth scene on the normalized plane, drawn through u = f theta x / r (libm, not the code under test) and rounded to a
    byte, rectified by the restatement with k = 0 and rect_* = the raw intrinsics, against the same scene sampled by that
    pinhole. The bound, as in test_lens_cpu.py's known-scene test, is the restatement's own and is derived, not measured:
      0.5   the raw frame's rounding (the blend is a convex combination of raw values)
    + (max |g_uu| + max |g_vv|) / 8   bilinear interpolation of the raw scene g(u, v) inside one pixel cell
    + (max |g_u| + max |g_v|) / 64    the source coordinate's rounding to 1/32 pixel (at most 1/64 off per axis)
    + 0.5   the one rounding of the integer blend
    with the derivatives of g taken by central differences of the analytic raw scene on a quarter-pixel grid (2 % added for
    what lies between the grid points), over the disc of the raw frame that the rectified image samples: beyond it, towards the
    raw corners, theta nears pi / 2, the scene is compressed without limit, and no output pixel looks there. Printed: the bound
    and the measured error."""
    f, cx, cy = 0.45 * cols, cols / 2 - 1.3, rows / 2 + 0.7
    lens = abi.make_lens_model(abi.VIO_LENS_FISHEYE, f, f, cx, cy)
    assert (lens.rect_fx, lens.rect_fy, lens.rect_cx, lens.rect_cy) == (f, f, cx, cy)
    vv, uu = np.mgrid[0:rows, 0:cols].astype(np.float64)
    raw = np.clip(np.rint(scene(*equidistant_rays(f, cx, cy, uu, vv))), 0, 255).astype(np.uint8)
    assert MC.n_outside(lens, rows, cols) == 0
    xn = (uu - lens.rect_cx) / lens.rect_fx
    yn = (vv - lens.rect_cy) / lens.rect_fy
    h = 0.25
    gv, gu = np.mgrid[-1:rows + h:h, -1:cols + h:h]
    g = scene(*equidistant_rays(f, cx, cy, gu, gv))
    used = np.hypot(gu - cx, gv - cy) <= f * np.arctan(np.hypot(xn, yn).max()) + 2.0     # the disc the output samples, + a cell

    def worst(d, at):
        return np.abs(d)[at].max()
    g_u, g_v = worst(g[:, 2:] - g[:, :-2], used[:, 1:-1]) / (2 * h), worst(g[2:, :] - g[:-2, :], used[1:-1, :]) / (2 * h)
    g_uu = worst(g[:, 2:] - 2 * g[:, 1:-1] + g[:, :-2], used[:, 1:-1]) / h ** 2
    g_vv = worst(g[2:, :] - 2 * g[1:-1, :] + g[:-2, :], used[1:-1, :]) / h ** 2
    bound = 0.5 + 1.02 * ((g_uu + g_vv) / 8 + (g_u + g_v) / 64) + 0.5
    want = scene(xn, yn)
    err = np.abs(MC.rectify(raw, lens).astype(np.float64) - want).max()
    print("bound %.3f grey levels, max error %.3f" % (bound, err))
    assert bound < 3.0                                              # the scene is smooth enough for the bound to say something
    assert err <= bound
    assert np.abs(raw.astype(np.float64) - want).max() > 10        # unrectified, the raw frame is far off


def atan_grid():
    """[0, 64] densely, the breakpoints of the reduction and their neighbours on both sides, and the smallest arguments."""
    b = np.array(MC.ATAN_BREAKS)
    near = np.concatenate([b, np.nextafter(b, 0), np.nextafter(b, 100), np.nextafter(np.nextafter(b, 0), 0)])
    rng = np.random.default_rng(9)
    return np.concatenate([np.linspace(0.0, 64.0, 400001), rng.uniform(0, 3, 200000), near, [0.0, 5e-324, 1e-300, 1e-9, 64.0]])


def test_atan_stays_within_4_ulp_of_numpy_arctan(model_program, tmp_path):
    x = atan_grid()
    ours, ref = MC.atan(x), np.arctan(x)
    ulp = np.abs(ours - ref) / np.spacing(ref)
    print("max distance from numpy.arctan: %.2f ulp at x = %r" % (ulp.max(), x[ulp.argmax()]))
    assert ulp.max() <= 4
    # the header's function on the host == the restatement, bit for bit
    fin, fout = str(tmp_path / "x.bin"), str(tmp_path / "atan.bin")
    x.tofile(fin)
    subprocess.check_call([model_program, "atan", fin, fout])
    got = np.fromfile(fout, np.float64)
    assert got.shape == ours.shape and np.array_equal(got.view(np.uint64), ours.view(np.uint64))


def rect_grid(lens, rows, cols):
    """The normalized points of the rectified image's pixel grid: the lens's field of view."""
    xn = (np.arange(cols, dtype=np.float64)[None, :] - lens.rect_cx) / lens.rect_fx + np.zeros((rows, 1))
    yn = (np.arange(rows, dtype=np.float64)[:, None] - lens.rect_cy) / lens.rect_fy + np.zeros((1, cols))
    return np.stack([xn.ravel(), yn.ravel()], axis=1)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_distort_points_is_the_formula(rows, cols):
    for which in MODELS:
        lens = getattr(MC, which)(rows, cols)
        p = rect_grid(lens, rows, cols)
        uv = abi.lens_model_distort_points(lens, p)
        u, v = MC.distort(lens, p[:, 0], p[:, 1])
        assert np.array_equal(uv[:, 0], u) and np.array_equal(uv[:, 1], v), which    # the library is built without contraction
    # a Brown-Conrady record is vio_lens_distort_points of the VioLens it stands for
    old = LC.lens_a(rows, cols)
    p = rect_grid(old, rows, cols)
    assert np.array_equal(abi.lens_model_distort_points(abi.lens_model_of(old), p), abi.lens_distort_points(old, p))


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_undistort_points_inverts_distort_points_over_the_field_of_view(rows, cols):
    """Rational: the fixed-point iteration of vio_lens_undistort_points, and its error budget (test_lens_cpu.py). Fisheye:
    Newton on theta converges quadratically, so a step below 1e-12 leaves theta exact to rounding; tan(theta) magnifies that by
    1 / cos^2(theta) <= 11 at the widest ray of these lenses (r = 3.05): far inside 1e-9."""
    for which in ("rational", "fisheye_in", "fisheye_clamped", "brown_model"):
        lens = getattr(MC, which)(rows, cols)
        p = rect_grid(lens, rows, cols)
        back, ok = abi.lens_model_undistort_points(lens, abi.lens_model_distort_points(lens, p))
        print(which, "max error", np.abs(back - p).max())
        assert np.abs(back - p).max() <= 1e-9, which
        assert ok.dtype == np.uint8 and (ok == 1).all(), which
    # a fisheye pixel further than f * pi / 2 from the centre is a ray from behind the image plane: no pinhole image
    lens = MC.fisheye_in(rows, cols)
    flat = abi.make_lens_model(abi.VIO_LENS_FISHEYE, lens.fx, lens.fx, lens.cx, lens.cy)
    far = lens.fx * np.pi / 2
    _, ok = abi.lens_model_undistort_points(flat, [[lens.cx, lens.cy], [lens.cx + far - 1.0, lens.cy], [lens.cx + far + 1.0, lens.cy],
                                                   [lens.cx, lens.cy - 2 * far]])
    assert list(ok) == [1, 1, 0, 0]
    # ... and the rational iteration says so when 50 rounds do not do it (test_lens_cpu.py's strong pincushion)
    strong = abi.make_lens_model(abi.VIO_LENS_RATIONAL, 100.0, 100.0, 50.0, 50.0, (2.0,))
    _, ok = abi.lens_model_undistort_points(strong, [[50.0, 50.0], [400.0, 380.0]])
    assert list(ok) == [1, 0]


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_coverage_equals_the_restatements_count(rows, cols):
    for which in MODELS:
        lens = getattr(MC, which)(rows, cols)
        n = abi.lens_model_coverage(lens, rows, cols)
        print(which, "outside:", n, n / (rows * cols))
        assert n == MC.n_outside(lens, rows, cols), which
        if which == "fisheye_clamped":                        # some, but fewer than half: the clamp path is a real share
            assert 0 < n < rows * cols / 2
        else:
            assert n == 0
    old = LC.lens_c(rows, cols)
    assert abi.lens_model_coverage(abi.lens_model_of(old), rows, cols) == abi.lens_coverage(old, rows, cols)


def test_the_host_entries_refuse_what_the_setter_refuses():
    lib, good = abi.load_product(), MC.fisheye_in(72, 100)
    n = C.c_int64()
    xy = (C.c_double * 2)(0.1, 0.2)
    out = (C.c_double * 2)()

    def variant(**kw):
        m = abi.VioLensModel.from_buffer_copy(bytes(good))
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    for bad in (variant(model=3), variant(model=-1), variant(reserved=1)):
        assert lib.vio_lens_model_coverage(C.byref(bad), 72, 100, C.byref(n)) == abi.VIO_EINVAL
        assert lib.vio_lens_model_distort_points(C.byref(bad), xy, 1, out) == abi.VIO_EINVAL
        assert lib.vio_lens_model_undistort_points(C.byref(bad), xy, 1, out, None) == abi.VIO_EINVAL
    stray = variant()
    stray.k[4] = 1e-3                                        # a fisheye has four coefficients
    assert lib.vio_lens_model_coverage(C.byref(stray), 72, 100, C.byref(n)) == abi.VIO_EINVAL
    assert lib.vio_lens_model_coverage(C.byref(variant(fx=float("nan"))), 72, 100, C.byref(n)) == abi.VIO_EINVAL
    assert lib.vio_lens_model_undistort_points(C.byref(variant(fx=0.0)), xy, 1, out, None) == abi.VIO_EINVAL
    assert lib.vio_lens_model_coverage(C.byref(good), 72, 100, C.byref(n)) == abi.VIO_OK


def supersampled_case(rows, cols):
    """An RGBA source of twice the output size (s = 2) and the inside fisheye, its raw intrinsics those of the delivered frame."""
    src = abi.make_source(abi.VIO_PIXEL_RGBA8, 2 * rows, 2 * cols)
    return src, MC.for_frame(MC.fisheye_in(rows, cols), src, rows, cols)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_supersampled_fisheye_on_the_host_equals_the_restatement(rows, cols, model_program, tmp_path):
    src, lens = supersampled_case(rows, cols)
    assert SC.samples_per_axis(src, rows, cols) == 2 and abi.source_check(src, rows, cols) == abi.VIO_OK
    plane = SC.random_plane(rows, src)
    got = run_model(model_program, tmp_path, plane, lens, rows, cols, source=src)
    want = MC.rectify_source(plane, src, lens, rows, cols)
    assert np.array_equal(got, want), int((got != want).sum())
    # video-range NV12 luma through the clamped fisheye, s = 1: the range map at each neighbour
    nv12 = abi.make_source(abi.VIO_PIXEL_NV12, rows, cols, stride=cols + 12, range=1)
    plane = SC.random_plane(cols, nv12)
    lens = MC.fisheye_clamped(rows, cols)
    got = run_model(model_program, tmp_path, plane, lens, rows, cols, source=nv12)
    assert np.array_equal(got, MC.rectify_source(plane, nv12, lens, rows, cols))
