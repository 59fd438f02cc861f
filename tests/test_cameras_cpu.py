"""Per-sequence cameras, the parts that need no device: the new symbols, and the set / get contract of the contexts that can be
created without one (the estimator and the PnP tracker). The cameras are made up (camera_cases.py)."""
import ctypes as C
import os
import re

import numpy as np

import camera_cases as CC
import helpers as H
from helpers import abi, pkg

NEW_SYMBOLS = ["vio_camera_from_config", "vio_frontend_set_cameras", "vio_frontend_get_camera", "vio_estimator_set_camera",
               "vio_estimator_get_camera", "vio_pnp_tracker_set_camera", "vio_pnp_tracker_get_camera", "vio_loop_detector_set_cameras",
               "vio_loop_detector_get_camera", "vio_backend_solve_windows_cam", "vio_backend_upload_cam", "vio_pnp_solve_windows_cam"]


def obs_grid(n, shift=0.0, first_id=0):
    ids = list(range(first_id, first_id + n))
    xyz = [[-0.4 + 0.8 * (i % 12) / 11 + shift, -0.3 + 0.6 * (i // 12) / 11, 1.0] for i in range(n)]
    return ids, xyz


def test_the_new_symbols_are_in_the_header_and_the_library():
    txt = open(os.path.join(H.ROOT, "include", "vio_amd.h")).read()
    lib = abi.load_product()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, txt), s
        assert hasattr(lib, s), s
    assert "typedef struct VioCamera" in txt
    # the struct is what the header says: four intrinsics, tic, ric
    assert C.sizeof(abi.VioCamera) == 16 * 8 and abi.VioCamera.tic.offset == 32 and abi.VioCamera.ric.offset == 56


def test_camera_from_config_takes_the_intrinsics_of_cfg_and_the_given_extrinsic():
    cfg, tic, ric = CC.camera("B")
    c = abi.camera_from_config(cfg, tic, ric)
    assert (c.fx, c.fy, c.cx, c.cy) == (cfg.fx, cfg.fy, cfg.cx, cfg.cy)
    assert np.array_equal(np.array(c.tic[:]), tic) and np.array_equal(np.array(c.ric[:]).reshape(3, 3), ric)
    c = abi.camera_from_config(cfg)
    assert list(c.tic) == [0, 0, 0] and list(c.ric) == [1, 0, 0, 0, 1, 0, 0, 0, 1]


def _bad_cameras():
    out = []
    for field, value in (("fx", 0.0), ("fy", 0.0), ("fx", float("nan")), ("fy", float("inf")), ("cx", float("nan"))):
        c = CC.vio_camera("B")
        setattr(c, field, value)
        out.append(c)
    return out


def _negative_fx():
    """sqrt_info = fx / 1.5 weighs the residuals of the window solves: the estimator and the PnP tracker take no fx <= 0."""
    c = CC.vio_camera("B")
    c.fx = -c.fx
    return c


def _bad_extrinsics():
    out = []
    _, tic, ric = CC.camera("B")
    cfg = CC.camera("B")[0]
    out.append(abi.make_camera(cfg.fx, cfg.fy, cfg.cx, cfg.cy, tic, ric @ np.diag([1.0, 1.0, -1.0])))   # determinant -1
    out.append(abi.make_camera(cfg.fx, cfg.fy, cfg.cx, cfg.cy, tic, ric * 1.001))                        # not orthonormal
    out.append(abi.make_camera(cfg.fx, cfg.fy, cfg.cx, cfg.cy, [0, float("nan"), 0], ric))
    return out


def test_estimator_camera_contract():
    cfg, tic, ric = CC.camera("A")
    cfg.window_size = 4
    est = pkg.estimator.Estimator(cfg, tic, ric, n_seq=3)
    A, B, Cc = CC.vio_camera("A", cfg), CC.vio_camera("B", cfg), CC.vio_camera("C", cfg)
    for q in range(3):  # after create: cfg with the creation tic / ric
        assert CC.same_camera(est.get_camera(q), A)
    assert est.set_camera(B, seq=1) == abi.VIO_OK and est.set_camera(Cc, seq=2) == abi.VIO_OK
    assert CC.same_camera(est.get_camera(0), A) and CC.same_camera(est.get_camera(1), B) and CC.same_camera(est.get_camera(2), Cc)
    # argument errors change nothing
    for bad in _bad_cameras() + _bad_extrinsics() + [_negative_fx()]:
        assert est.set_camera(bad, seq=1) == abi.VIO_EINVAL
    assert est.set_camera(B, seq=3) == abi.VIO_EINVAL and est.set_camera(B, seq=-1) == abi.VIO_EINVAL
    lib = abi.load_product()
    assert lib.vio_estimator_set_camera(est._h, 0, None) == abi.VIO_EINVAL
    assert lib.vio_estimator_get_camera(est._h, 3, C.byref(abi.VioCamera())) == abi.VIO_EINVAL
    assert CC.same_camera(est.get_camera(1), B)
    # a sequence that holds a frame refuses; the others do not care
    est.process_imu(0.01, [0, 0, 9.8], [0, 0, 0], seq=1)
    assert est.set_camera(Cc, seq=1) == abi.VIO_OK          # IMU samples alone are no frame
    assert est.set_camera(B, seq=1) == abi.VIO_OK
    assert est.process_image(*obs_grid(60), 1.0, seq=1).action == abi.VIO_FRAME_FILLING
    assert est.status(1).frame_count == 1
    assert est.set_camera(Cc, seq=1) == abi.VIO_ESTATE and CC.same_camera(est.get_camera(1), B)
    assert est.set_camera(B, seq=0) == abi.VIO_OK
    # the camera survives vio_estimator_clear, which makes the sequence settable again
    est.clear(1)
    assert est.status(1).frame_count == 0 and CC.same_camera(est.get_camera(1), B)
    assert est.set_camera(Cc, seq=1) == abi.VIO_OK and CC.same_camera(est.get_camera(1), Cc)
    # ... and the clearState inside process_image (a full INITIAL window that tracks too little: VIO_FRAME_RESET)
    for k in range(4):
        est.process_imu(0.01, [0, 0, 9.8], [0, 0, 0], seq=2)
        assert est.process_image(*obs_grid(50, shift=0.02 * k), float(k), seq=2).action == abi.VIO_FRAME_FILLING
    assert est.process_image(*obs_grid(50, first_id=1000), 4.0, seq=2).action == abi.VIO_FRAME_RESET
    assert est.status(2).frame_count == 0 and CC.same_camera(est.get_camera(2), Cc)
    est.close()


def test_pnp_tracker_camera_contract():
    cfg, tic, ric = CC.camera("A")
    tr = pkg.pnp.PnpTracker(cfg, tic, ric, n_seq=2, pnp_size=3)
    A, B, Cc = CC.vio_camera("A"), CC.vio_camera("B"), CC.vio_camera("C")
    assert CC.same_camera(tr.get_camera(0), A) and CC.same_camera(tr.get_camera(1), A)
    assert tr.set_camera(Cc, seq=1) == abi.VIO_OK
    assert CC.same_camera(tr.get_camera(0), A) and CC.same_camera(tr.get_camera(1), Cc)
    for bad in _bad_cameras() + _bad_extrinsics() + [_negative_fx()]:
        assert tr.set_camera(bad, seq=1) == abi.VIO_EINVAL
    assert tr.set_camera(B, seq=2) == abi.VIO_EINVAL and tr.set_camera(B, seq=-1) == abi.VIO_EINVAL
    assert CC.same_camera(tr.get_camera(1), Cc)
    # a frame in the window: refused until the sequence is cleared; the camera outlives the clear
    tr.process_imu(0.0, [0, 0, 9.8], [0, 0, 0], seq=1)
    feats = [[], [(7, (0.1, 0.2), (1.0, 2.0, 5.0), 3)]]
    _, _, solved = tr.process_images(feats, [0.0, 1.0], use_pnp=False, active=[0, 1])
    assert list(solved) == [0, 0] and tr.window(1)["frame_count"] == 1
    assert tr.set_camera(B, seq=1) == abi.VIO_ESTATE and CC.same_camera(tr.get_camera(1), Cc)
    assert tr.set_camera(B, seq=0) == abi.VIO_OK
    tr.clear(1)
    assert CC.same_camera(tr.get_camera(1), Cc) and tr.set_camera(B, seq=1) == abi.VIO_OK
    tr.close()


def test_window_filling_and_initial_slides_with_a_camera_equal_the_stand_alone_store():
    """Sequence 1 of a two-sequence estimator carries camera B (sequence 0 the context's): filling its window and the
    INITIAL-phase slides give what the stand-alone landmark store gives when it is driven the way processImage drives it,
    and what the same frames give in sequence 0 -- nothing of this phase may depend on the camera being set."""
    cfg, tic, ric = CC.camera("A")
    cfg.window_size = 5
    W = cfg.window_size
    est = pkg.estimator.Estimator(cfg, tic, ric, n_seq=2)
    assert est.set_camera(CC.vio_camera("B", cfg), seq=1) == abi.VIO_OK
    fm = pkg.window.FeatureManager(W)
    fc = 0
    for k in range(W + 4):
        for q in range(2):
            est.process_imu(0.01, [0, 0, 9.8], [0, 0, 0.1], seq=q)
        ids, xyz = obs_grid(80, shift=0.03 * k)
        res = est.process_images([(ids, xyz), (ids, xyz)], [10.0 + k] * 2)
        enough, _, _ = fm.add_check_parallax(fc, ids, xyz)
        for q in range(2):
            assert res[q].action == (abi.VIO_FRAME_FILLING if k < W else abi.VIO_FRAME_WAIT_INIT)
            assert res[q].marginalization_flag == (abi.VIO_MARGIN_OLD if enough else abi.VIO_MARGIN_SECOND_NEW)
        if fc < W:
            fc += 1
        elif enough:
            fm.remove_back()
        else:
            fm.remove_front(fc)
    want = fm.dump()
    for q in range(2):
        got = est.features(q).dump()
        assert got[0].shape == want[0].shape and len(got[0]) > 50 and np.array_equal(got[0][:, :3], want[0][:, :3])
        assert np.array_equal(got[1], want[1])
        assert list(est.window(q)["headers"][:W]) == [10.0 + k for k in range(4, W + 4)]
    assert CC.same_camera(est.get_camera(1), CC.vio_camera("B", cfg))
    est.close(), fm.close()
