"""Lens rectification of the image pre-step, the parts that need no device: the new symbols, the per-pixel function of
csrc/pre_rectify.h (the text the kernel compiles) as a stand-alone host program against the numpy restatement of the arithmetic
(lens_cases.py), the host entries vio_lens_*, and how well the specified arithmetic itself rectifies a known scene."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import lens_cases as LC
from helpers import abi

NEW_SYMBOLS = ["vio_preprocess_set_lenses", "vio_preprocess_get_lens", "vio_lens_distort_points", "vio_lens_undistort_points",
               "vio_lens_coverage"]
SHAPES = [(72, 100), (64, 96)]


def test_the_new_symbols_are_in_the_header_the_library_and_abi_py():
    txt = open(os.path.join(H.ROOT, "include", "vio_amd.h")).read()
    lib = abi.load_product()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s      # bound in abi.load_product
    assert "typedef struct VioLens" in txt
    assert C.sizeof(abi.VioLens) == 13 * 8 and abi.VioLens.k1.offset == 32 and abi.VioLens.rect_fx.offset == 72


@pytest.fixture(scope="module")
def rectify_program():
    """tests/emul/lens_rectify: pre_rectify.h with a main of its own, built for the host without contraction."""
    csrc, inc = os.path.join(H.ROOT, "vins-mobile_amd", "csrc"), os.path.join(H.ROOT, "include")
    exe, src = os.path.join(H.EMUL_DIR, "lens_rectify"), os.path.join(H.EMUL_DIR, "lens_rectify_main.cpp")
    deps = [src, os.path.join(csrc, "pre_rectify.h"), os.path.join(inc, "vio_amd.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + inc, "-I" + csrc, "-o", exe, src])
    return exe


def run_program(exe, tmp_path, frame, lens):
    frame = np.ascontiguousarray(frame, np.uint8)
    rows, cols = frame.shape[:2]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([rows, cols, 4 if frame.ndim == 3 else 1, 0], np.int32).tobytes())
        f.write(bytes(lens))
        f.write(frame.tobytes())
    subprocess.check_call([exe, fin, fout])
    return np.fromfile(fout, np.uint8).reshape(rows, cols)


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("which", ["A", "C"])
def test_shared_header_on_the_host_equals_the_restatement_bit_for_bit(rows, cols, which, rectify_program, tmp_path):
    lens = (LC.lens_a if which == "A" else LC.lens_c)(rows, cols)
    frame = LC.random_frame(rows + cols, rows, cols, rgba=False)
    got = run_program(rectify_program, tmp_path, frame, lens)
    want = LC.rectify(frame, lens)
    assert np.array_equal(got, want), int((got != want).sum())
    assert (want != frame).mean() > 0.5                    # the lens moved the frame: not a comparison of two copies
    # RGBA goes through the same function: the gray of each of the four neighbours, then the blend
    rgba = LC.random_frame(rows * cols, rows, cols, rgba=True)
    assert np.array_equal(run_program(rectify_program, tmp_path, rgba, lens), LC.rectify(rgba, lens))


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_no_source_coordinate_of_these_inputs_is_near_a_rounding_tie(rows, cols):
    """Bit-exactness between two correct implementations is a fair demand only while no 32 u sits on a tie within the double
    rounding of the formula (about 1e-13)."""
    for lens in (LC.lens_a(rows, cols), LC.lens_c(rows, cols)):
        d = LC.tie_distance(lens, rows, cols)
        print("closest approach to a tie:", d)
        assert d > 1e-10


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_identity_lens_returns_the_frame(rows, cols, rectify_program, tmp_path):
    lens = LC.identity_lens(rows, cols)
    for rgba in (False, True):
        frame = LC.random_frame(5, rows, cols, rgba)
        assert np.array_equal(LC.rectify(frame, lens), LC.gray_of(frame).astype(np.uint8))
        assert np.array_equal(run_program(rectify_program, tmp_path, frame, lens), LC.gray_of(frame).astype(np.uint8))


def rect_grid(lens, rows, cols):
    """The normalized points of the rectified image's pixel grid: lens A's field of view."""
    xn = (np.arange(cols, dtype=np.float64)[None, :] - lens.rect_cx) / lens.rect_fx + np.zeros((rows, 1))
    yn = (np.arange(rows, dtype=np.float64)[:, None] - lens.rect_cy) / lens.rect_fy + np.zeros((1, cols))
    return np.stack([xn.ravel(), yn.ravel()], axis=1)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_distort_points_is_the_formula(rows, cols):
    for lens in (LC.lens_a(rows, cols), LC.lens_c(rows, cols)):
        p = rect_grid(lens, rows, cols)
        uv = abi.lens_distort_points(lens, p)
        u, v = LC.distort(lens, p[:, 0], p[:, 1])
        assert np.allclose(uv[:, 0], u, rtol=1e-12, atol=0) and np.allclose(uv[:, 1], v, rtol=1e-12, atol=0)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_undistort_points_inverts_distort_points_over_the_field_of_view(rows, cols):
    """x <- x + (x_d - D(x)) contracts by |1 - D'|, at most about 0.5 per round at lens A's corners: 50 rounds are far more than
    the 1e-12 step needs, and a step below 1e-12 at that rate leaves an error of the same order, well inside 1e-9."""
    lens = LC.lens_a(rows, cols)
    p = rect_grid(lens, rows, cols)
    back, ok = abi.lens_undistort_points(lens, abi.lens_distort_points(lens, p))
    print("max error", np.abs(back - p).max())
    assert np.abs(back - p).max() <= 1e-9
    assert ok.dtype == np.uint8 and (ok == 1).all()
    # ... and says so when 50 rounds do not do it: a pincushion point far outside, where the forward model no longer contracts
    strong = abi.make_lens(100.0, 100.0, 50.0, 50.0, (2.0, 0.0, 0.0, 0.0, 0.0))
    _, ok = abi.lens_undistort_points(strong, [[50.0, 50.0], [400.0, 380.0]])
    assert list(ok) == [1, 0]


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_coverage_counts_the_clamped_pixels(rows, cols):
    a, c = LC.lens_a(rows, cols), LC.lens_c(rows, cols)
    assert abi.lens_coverage(a, rows, cols) == LC.n_outside(a, rows, cols) == 0
    n = abi.lens_coverage(c, rows, cols)
    print("lens C outside:", n, n / (rows * cols))
    assert n == LC.n_outside(c, rows, cols)
    # the count itself is pinned by the equality above; this only says that the clamp path is a real share of the frame:
    # a pincushion of k1 = 0.35 pushes a band along all four edges outside, about a fifth of the pixels (21.7 % and 20.7 % here)
    assert 0.15 <= n / (rows * cols) <= 0.25


def scene(x, y):
    return 128 + 60 * np.sin(7 * x + 0.3) * np.cos(5 * y - 0.2) + 40 * np.sin(3 * x - 4 * y)


@pytest.mark.parametrize("rows,cols", SHAPES + [(640, 480)])
def test_the_specified_arithmetic_rectifies_a_known_scene_to_within_the_bilinear_bound(rows, cols):
    """A smooth scene on the normalized plane, seen through lens A (raw pixel -> vio_lens_undistort_points -> scene, rounded to
    a byte), rectified by the restatement, against the same scene sampled by the rectified pinhole. Measured: 0.98 grey levels at
    72 x 100, 0.97 at 64 x 96, 0.96 at 640 x 480 (half a level from the raw frame's rounding, the rest bilinear interpolation and
    the final rounding). 1.5 is the bound of the restatement, not a device tolerance: the device equals the restatement."""
    lens = LC.lens_a(rows, cols)
    vv, uu = np.mgrid[0:rows, 0:cols].astype(np.float64)
    xn, ok = abi.lens_undistort_points(lens, np.stack([uu.ravel(), vv.ravel()], axis=1))
    assert ok.all()
    raw = np.clip(np.rint(scene(xn[:, 0], xn[:, 1])), 0, 255).astype(np.uint8).reshape(rows, cols)
    assert LC.n_outside(lens, rows, cols) == 0
    p = rect_grid(lens, rows, cols)
    want = scene(p[:, 0], p[:, 1]).reshape(rows, cols)
    err = np.abs(LC.rectify(raw, lens).astype(np.float64) - want).max()
    print("max error (grey levels):", err)
    assert err <= 1.5
    assert np.abs(raw.astype(np.float64) - want).max() > 10        # unrectified, the raw frame is far off
