"""Per-sequence cameras in the landmark store, without a device: the sources of the store passes that read a camera (store_ingest
with its triangulation, store_keyframe; csrc/store_core.h) on the wave64 SIMT emulator for three slots that hold the made-up
cameras C, A, B -- slot order is not camera order --, each slot's record and each job's intrinsics selected the way the kernels of
vio_store.hip select them (store::slot_camera, store::job_intrinsics), from NaN-poisoned buffers. Every slot must equal, bit for
bit, the host-side list driven with that slot's camera (vio_features_triangulate, vio_features_keyframe). Test-only build
(tests/emul/simt_cameras.cpp)."""
import ctypes as C

import numpy as np
import pytest

import camera_cases as CC
import helpers as H

SLOT_CAMERAS = "CAB"


@pytest.fixture(scope="module")
def lib():
    l = H.build_emul_lib("simt_cameras.cpp", "libvio_simt_cameras.so", "VIO_SIMT")
    l.simt_cameras.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_char_p, C.c_int, C.POINTER(C.c_longlong)]
    return l


def camera_table(names):
    rows = []
    for n in names:
        cfg, tic, ric = CC.camera(n)
        rows.append(np.concatenate([[cfg.fx, cfg.fy, cfg.cx, cfg.cy], tic, ric.ravel()]))
    return np.ascontiguousarray(rows, np.float64)


def run(lib, seed, W, order, names, jobs, shift=0):
    cams, jobs = camera_table(names), np.ascontiguousarray(jobs, np.int32)
    buf, stats = C.create_string_buffer(8192), (C.c_longlong * 6)()
    bad = lib.simt_cameras(seed, W, order, shift, cams.ctypes.data_as(C.POINTER(C.c_double)), jobs.ctypes.data_as(C.POINTER(C.c_int)), buf, 8192, stats)
    return bad, buf.value.decode(), list(stats)


# (seed, window size, lane order of the emulator, slot of keyframe job 0, 1, 2)
CASES = [(1, 10, 0, (2, 0, 1)), (2, 6, 1, (1, 2, 0)), (3, 10, 3, (0, 1, 2))]


@pytest.mark.parametrize("seed,W,order,jobs", CASES)
def test_store_passes_of_three_slots_equal_the_host_list_with_each_slots_camera(seed, W, order, jobs, lib):
    bad, msg, stats = run(lib, seed, W, order, SLOT_CAMERAS, jobs)
    assert bad == 0, msg
    for s in range(3):   # not a comparison of empty lists: triangulated depths and keyframe features in every slot
        assert stats[2 * s] > 20 and stats[2 * s + 1] > 20, stats


@pytest.mark.parametrize("shift", [1, 2])
def test_the_comparison_sees_a_record_taken_from_another_slot(shift, lib):
    """The store side reads the record of slot (s + shift) % 3 and the intrinsics row of job (j + shift) % 3: the wrong index the
    test above exists for. Depths and keyframe features must then differ; with three identical cameras the same fault shows
    nothing, which is why the cameras differ in every field."""
    bad, msg, _ = run(lib, 1, 10, 0, SLOT_CAMERAS, (2, 0, 1), shift=shift)
    assert bad > 0 and "depth" in msg
    bad, msg, _ = run(lib, 1, 10, 0, "BBB", (2, 0, 1), shift=shift)
    assert bad == 0, msg
    a = camera_table(SLOT_CAMERAS)
    for f in range(7):    # fx fy cx cy and tic: three different values each
        assert len(set(a[:, f])) == 3, f
    assert len({tuple(r[7:]) for r in a}) == 3
