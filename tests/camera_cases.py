"""Three made-up cameras that differ in every field, shared by the per-sequence camera tests (test_cameras_*.py).

A is the default configuration with the default extrinsic; B and C move every intrinsic by a few per cent / pixels and the
extrinsic by centimetres and degrees. None of them is a camera of a real device."""
import numpy as np

from helpers import abi, synth


def _rot(axis, deg):
    v = np.zeros(3)
    v[axis] = np.deg2rad(deg)
    return synth.rotvec_to_rot(v)


def camera(name, cfg=None):
    """-> (cfg carrying the camera's intrinsics, tic [3], ric [3, 3]); cfg: the configuration the other fields come from."""
    base = cfg if cfg is not None else abi.default_config()
    c = abi.VioConfig.from_buffer_copy(base)
    ex = synth.ex_pose_default()
    tic, ric = ex[:3].copy(), synth.quat_to_rot(ex[3:])
    if name == "B":
        c.fx, c.fy, c.cx, c.cy = base.fx * 1.04, base.fy * 0.97, base.cx + 5.0, base.cy - 7.0
        tic, ric = tic + np.array([0.01, -0.02, 0.015]), ric @ _rot(2, 3.0)
    elif name == "C":
        c.fx, c.fy, c.cx, c.cy = base.fx * 0.93, base.fy * 1.02, base.cx - 4.0, base.cy + 6.0
        tic, ric = tic + np.array([-0.015, 0.01, -0.01]), ric @ _rot(1, -2.0)
    else:
        assert name == "A"
    return c, tic, ric


def vio_camera(name, cfg=None):
    c, tic, ric = camera(name, cfg)
    return abi.make_camera(c.fx, c.fy, c.cx, c.cy, tic, ric)


def ex_pose(name):
    """para_Ex_Pose [7] of the camera: tic, then ric as x y z w."""
    _, tic, ric = camera(name)
    return np.concatenate([tic, synth.rot_to_quat(ric)])


def same_camera(a, b):
    """Two abi.VioCamera, field by field, bit for bit."""
    return (a.fx, a.fy, a.cx, a.cy, list(a.tic), list(a.ric)) == (b.fx, b.fy, b.cx, b.cy, list(b.tic), list(b.ric))
