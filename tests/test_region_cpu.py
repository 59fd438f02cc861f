"""The valid region of a pre-step slot, the parts that need no device: the host entry vio_lens_model_valid_region against the
numpy restatement (region_cases.py), its count against vio_lens_model_coverage, its argument errors, the new symbols, and the
shared header (csrc/pre_source.h, the text the kernel compiles) as a stand-alone program under AddressSanitizer and UBSan
against the library's bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import lens_model_cases as MC
import region_cases as RC
from helpers import abi

NEW_SYMBOLS = ["vio_preprocess_valid_regions", "vio_preprocess_valid_regions_resident", "vio_lens_model_valid_region"]


def test_the_new_symbols_are_in_the_header_the_library_and_abi_py():
    txt = open(os.path.join(H.ROOT, "include", "vio_amd.h")).read()
    lib = abi.load_product()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s      # bound in abi.load_product


ROWS, COLS, FRAMES, RING = 70, 260, 12, 12


def tracker_config():
    return abi.default_config(max_corners=40, min_dist=10, image_rows=ROWS, image_cols=COLS)


def run_tracker(trk, frames):
    """12 frames, publish on every third -> [(ids, xyz, state)] per frame."""
    out = []
    for f in range(FRAMES):
        ids, xyz = trk.read_image(frames[f], f % 3 == 0)
        out.append((ids, xyz) + tuple(trk.state()))
    return out


def assert_runs_equal(got, want, what):
    for f, (g, w) in enumerate(zip(got, want)):
        for a, b in zip(g, w):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (what, f)


def test_region_tracker_without_a_region_is_the_oracle_tracker():
    """The yardstick of the GPU tests against the oracle it restates: ids, xyz and state(), bit for bit."""
    cfg = tracker_config()
    frames = H.synth.make_image_stream(31, FRAMES, rows=ROWS, cols=COLS)[0]
    oracle = H.OracleTracker(cfg)
    want = run_tracker(oracle, frames)
    oracle.close()
    assert sum(len(w[0]) for w in want) > 0 and any(len(w[2]) < cfg.max_corners for w in want)
    assert_runs_equal(run_tracker(RC.RegionTracker(cfg), frames), want, "no region")
    assert_runs_equal(run_tracker(RC.RegionTracker(cfg, RC.all_usable(ROWS, COLS)), frames), want, "all usable")


def test_region_tracker_with_a_ring_differs_the_way_a_region_should():
    cfg = tracker_config()
    frames = H.synth.make_image_stream(31, FRAMES, rows=ROWS, cols=COLS)[0]
    region = RC.ring(ROWS, COLS, RING)
    oracle, masked = H.OracleTracker(cfg), RC.RegionTracker(cfg, region)
    want, got = run_tracker(oracle, frames), run_tracker(masked, frames)
    oracle.close()
    print("per publish frame:", [{k: v for k, v in e.items() if k != "points"} for e in masked.log])
    assert any(not np.array_equal(g[1], w[1]) for g, w in zip(got, want))
    assert sum(e["dropped"] for e in masked.log) >= 1                      # a track slid onto the ring and was not kept
    assert sum(e.get("absent", 0) for e in masked.log) >= 1                # a corner of the unmasked detector is not there
    for e in masked.log:                                                   # no published feature lies on a 0 pixel
        p = np.rint(e["points"]).astype(int)
        assert (region[p[:, 1], p[:, 0]] == 255).all()
    n_masked, n_plain = sum(len(g[0]) for g in got), sum(len(w[0]) for w in want)
    print("observations: masked", n_masked, "unmasked", n_plain)
    assert 2 * n_masked >= n_plain > 0


@pytest.mark.parametrize("rows,cols", RC.SHAPES)
@pytest.mark.parametrize("margin", RC.MARGINS)
def test_host_entry_equals_the_restatement_bit_for_bit(rows, cols, margin):
    want = RC.expected(rows, cols, margin)
    for name, lens, src in RC.cases(rows, cols):
        if lens is None:                                     # a slot without a lens: no host entry to ask, all 255 by definition
            assert (want[name] == 255).all()
            continue
        got = abi.lens_model_valid_region(lens, src, rows, cols, margin)
        zeros = int((got == 0).sum())
        print(name, "margin", margin, "zeros:", zeros, "of", rows * cols)
        assert np.array_equal(got, want[name]), (name, int((got != want[name]).sum()))
        assert set(np.unique(got)) <= {0, 255}
        if margin == 0 and src is None:                      # the complement of what the coverage entry counts
            assert zeros == abi.lens_model_coverage(lens, rows, cols) == MC.n_outside(lens, rows, cols), name
    # the inputs say something: the clamped fisheye (slot 5) has an outside, fewer than half the pixels; the inside one (4) none
    m0 = RC.expected(rows, cols, 0)
    assert 0 < int((m0["mixed5"] == 0).sum()) < rows * cols / 2 and (m0["mixed4"] == 255).all()
    assert 0 < int((m0["sourced1"] == 0).sum()) < rows * cols / 2
    if margin:                                               # the erosion took more, and only took
        for name in ("mixed5", "sourced1"):
            assert (want[name] <= m0[name]).all() and int((want[name] == 0).sum()) > int((m0[name] == 0).sum()), name


def test_a_margin_reaches_in_from_the_outside_pixels_only():
    """The image border is no outside: with every pixel inside, any margin leaves the mask all 255; one outside pixel in a
    corner takes the (margin + 1)^2 pixels within reach of it."""
    rows, cols = 20, 30
    assert (RC.erode(np.ones((rows, cols), bool), 7)).all()
    ok = np.ones((rows, cols), bool)
    ok[0, 0] = False
    assert int((~RC.erode(ok, 3)).sum()) == 16
    lens = MC.fisheye_in(72, 100)
    assert (abi.lens_model_valid_region(lens, None, 72, 100, 32) == 255).all()


def test_argument_errors_return_einval_and_write_nothing():
    lib, good = abi.load_product(), MC.fisheye_clamped(72, 100)
    mask = np.full((72, 100), 7, np.uint8)
    mp = mask.ctypes.data_as(C.POINTER(C.c_uint8))
    src = abi.make_source(abi.VIO_PIXEL_RGBA8, 144, 200)

    def variant(**kw):
        m = abi.VioLensModel.from_buffer_copy(bytes(good))
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    call = lib.vio_lens_model_valid_region
    assert call(None, None, 72, 100, 0, mp) == abi.VIO_EINVAL
    assert call(C.byref(good), None, 72, 100, 0, None) == abi.VIO_EINVAL
    for margin in (-1, 33):
        assert call(C.byref(good), None, 72, 100, margin, mp) == abi.VIO_EINVAL
    assert call(C.byref(good), None, 0, 100, 0, mp) == abi.VIO_EINVAL and call(C.byref(good), None, 72, 0, 0, mp) == abi.VIO_EINVAL
    for bad in (variant(model=3), variant(reserved=1), variant(fx=float("nan")), variant(rect_fx=0.0)):
        assert call(C.byref(bad), None, 72, 100, 0, mp) == abi.VIO_EINVAL
    small = abi.make_source(abi.VIO_PIXEL_RGBA8, 36, 50)     # no upscaling: vio_source_check refuses it
    assert call(C.byref(good), C.byref(small), 72, 100, 0, mp) == abi.VIO_EINVAL
    assert (mask == 7).all()
    assert call(C.byref(good), C.byref(src), 72, 100, 32, mp) == abi.VIO_OK and set(np.unique(mask)) <= {0, 255}


def test_shared_header_as_a_sanitized_program_gives_the_librarys_bytes(tmp_path):
    """Address and undefined-behaviour sanitizers on the header's host text, in a program of its own (nothing is loaded into
    this process under a sanitizer)."""
    csrc, inc = os.path.join(H.ROOT, "vins-mobile_amd", "csrc"), os.path.join(H.ROOT, "include")
    exe = str(tmp_path / "valid_region")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + inc, "-I" + csrc, "-o", exe,
                           os.path.join(H.EMUL_DIR, "valid_region_main.cpp")])
    fin, want = str(tmp_path / "cases.bin"), []
    with open(fin, "wb") as f:
        for rows, cols in RC.SHAPES:
            for margin in RC.MARGINS:
                for name, lens, src in RC.cases(rows, cols):
                    if lens is None:
                        continue
                    f.write(np.array([rows, cols, margin, 0 if src is None else 1], np.int32).tobytes() + bytes(lens))
                    if src is not None:
                        f.write(bytes(src))
                    want.append(RC.checksum(abi.lens_model_valid_region(lens, src, rows, cols, margin)))
    out = subprocess.run([exe, fin], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(want) == len(RC.SHAPES) * len(RC.MARGINS) * 7 and got == want
