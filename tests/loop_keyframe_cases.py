"""Sessions of keyframe IMAGES for the loop thread's keyframe step (vio_loop_detector_keyframes = vio_brief_extract +
vio_loop_detector_detect + vio_loop_detector_connect). Shared by the CPU and GPU tests of tests/test_loop_keyframes.py.

A session is a camera that slides over one large textured scene (test_brief.make_image's generator at scene size): keyframe
i is the crop at offset track[i], so a revisit of a place is the same scene shifted by a few pixels -- a pure image shift is
a valid epipolar geometry (F = [t]x), which is what the detector's and the connection's RANSAC test. The first lap moves by
a quarter image per keyframe (neighbours overlap, entries more than `dislocal` apart do not), the second lap revisits the
first places with an offset of 2..5 pixels. The window points of a keyframe are the session's fixed scene points that fall
inside the crop (ids = their scene index), so the same id is the same scene point in every keyframe that sees it.
One keyframe per batch is FLAT with no window points: no corners, n_keys == 0.

Detector: the synthetic vocabulary of tests/test_loop_detector.py (test_dbow.make_vocabulary), dislocal 3, so that sessions
of 8 to 12 keyframes reach the geometric check. MIN_LOOP_NUM is lowered to 8 so that a connection of a few dozen window points
can be `connected`. CAP is the extractor's and the detector's max_keypoints: a few crops have more FAST corners than
CAP - n_window, which is the cut case.

The expectation of a case on the CPU is the restatement alone: test_brief.oracle_extract per keyframe, then the Detector
class of tests/test_loop_detector.py."""
import functools

import numpy as np

import helpers as H
import test_brief as TB
import test_loop_detector as LD

synth = H.pkg.synth

SHAPES = [(120, 160), (97, 131)]
DISLOCAL = 3
MIN_LOOP_NUM = 8
FAST_THRESHOLD = 20
CAP = {(120, 160): 416, (97, 131): 288}   # max_keypoints of extractor and detector: a few keyframes of each shape are cut
N_POINTS = 150                  # scene points per session
DETECTOR = dict(dislocal=DISLOCAL)
# per session of a batch: (keyframes in the first lap, first place revisited, revisits, index of the flat keyframe or None)
SESSIONS = [(7, 0, 4, None), (6, 1, 3, 8), (7, 0, 2, None)]


def scene(seed, rows, cols, laps):
    """The scene a session's camera slides over: make_image's texture, boxes and speckle at the size the track needs."""
    rng = np.random.default_rng(seed)
    R, C = rows + 16, cols + (cols // 4) * laps + 16
    img = synth.make_texture(rng, R, C)
    img = np.clip(img + 25.0 * (rng.random((R, C)) < 0.01) * rng.standard_normal((R, C)) * 4, 0, 255)
    for _ in range(C // 40):                                         # flat boxes: strong corners at their vertices
        y, x = int(rng.integers(0, R - 20)), int(rng.integers(0, C - 30))
        img[y:y + int(rng.integers(6, 20)), x:x + int(rng.integers(8, 30))] = float(rng.choice([15, 230]))
    return np.ascontiguousarray(img, np.uint8)


@functools.lru_cache(maxsize=None)
def session(shape, sid):
    """-> list of (image [rows][cols] uint8, window points float32 [k][2], ids int32 [k]) in keyframe order."""
    rows, cols = shape
    n1, first, n2, flat = SESSIONS[sid]
    seed = 1000 * rows + 10 * sid
    big = scene(seed, rows, cols, n1)
    rng = np.random.default_rng(seed + 1)
    pts = rng.uniform([4, 4], [big.shape[1] - 4, big.shape[0] - 4], (N_POINTS, 2)).round(2)
    step = cols // 4
    track = [(step * i, 5) for i in range(n1)]
    track += [(step * (first + j) + 2 + (j + sid) % 4, 5 + 1 + (j % 3)) for j in range(n2)]
    out = []
    for ox, oy in track:
        img = np.ascontiguousarray(big[oy:oy + rows, ox:ox + cols])
        p = pts - np.array([ox, oy], np.float64)
        vis = (p[:, 0] >= 2) & (p[:, 0] < cols - 2) & (p[:, 1] >= 2) & (p[:, 1] < rows - 2)
        out.append((img, p[vis].astype(np.float32), np.nonzero(vis)[0].astype(np.int32)))
    if flat is not None:
        out.insert(flat, (np.full((rows, cols), 128, np.uint8), np.zeros((0, 2), np.float32), np.zeros(0, np.int32)))
    return out


def batch(shape):
    return [session(shape, sid) for sid in range(len(SESSIONS))]


def calls(shape):
    """The batch keyframe by keyframe: per call the list of (session id, keyframe index); sessions end at different calls."""
    ses = batch(shape)
    return [[(s, i) for s in range(len(ses)) if i < len(ses[s])] for i in range(max(len(x) for x in ses))]


def stride(shape):
    return max(len(w) for s in batch(shape) for _, w, _ in s)


@functools.lru_cache(maxsize=None)
def extracted(shape, sid):
    """oracle_extract of every keyframe of a session at capacity CAP[shape] -> list of (rc, keys, descriptors, n_fast)."""
    pat = TB.pattern()
    return [TB.oracle_extract(img, w, pat, thr=FAST_THRESHOLD, cap=CAP[shape]) for img, w, _ in session(shape, sid)]


@functools.lru_cache(maxsize=None)
def restated(shape, sid):
    """The restated Detector over the oracle's extraction -> list of (detection dict, cur_pts, old_pts)."""
    det = LD.Detector(LD.vocabulary(LD.VOC_SEED)[2], **DETECTOR)
    return [det.detect(k, d) for _, k, d, _ in extracted(shape, sid)]
