#!/usr/bin/env python3
"""Wall time of the loop thread's keyframe step for 1 / 64 / 512 sessions per call, three routes over the same keyframes:

  device frames   one vio_loop_detector_keyframes, the frames in a device buffer (what vio_preprocess_run_resident leaves)
  host frames     one vio_loop_detector_keyframes, the frames in host memory (pageable)
  three calls     vio_brief_extract, then vio_loop_detector_detect, then vio_loop_detector_connect for the detected
                  sessions, every buffer allocated beforehand: the time inside the three C calls. Packing the keys and
                  descriptors back to back for detect is the caller's work on this route; its numpy time is printed
                  beside the line and not counted

640x480 frames; every session slides over one textured scene: 8 keyframes a quarter image apart, then revisits of the
first places shifted by a few pixels (a pure shift is a valid epipolar geometry), so the timed calls reach the geometric
check, detect loops and run the connection. Vocabulary 10^5 words (k 10, L 5) as tools/loop_detector_timing.py, ~150 window
points and ~1700 descriptors per keyframe (FAST threshold 60 on this texture), max_keypoints 2048, dislocal 3.
Each route has its own detector; the three are timed alternately in one process, 2 calls of warm-up, then --reps calls:
median with the minimum beside it. Needs a gfx950 device; writes profiles/loop_keyframes_timing.txt.

    python tools/loop_keyframes_timing.py [--reps 5] [--sessions 1,64,512] [--out profiles/loop_keyframes_timing.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROWS, COLS, STEP, LAP = 480, 640, 160, 8
CAP, FAST_THRESHOLD, N_POINTS, STRIDE = 2048, 60, 450, 256
_i32p, _fp, _u8p, _u64p, _dp = (C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64),
                                C.POINTER(C.c_double))


def line(name, v):
    return "%-58s %9.3f ms   (median of %d; min %.3f)" % (name, float(np.median(v)), len(v), min(v))


def make_scene(pkg, rng):
    R, Cc = ROWS + 16, COLS + STEP * LAP + 16
    img = pkg.synth.make_texture(rng, R, Cc)
    img = np.clip(img + 25.0 * (rng.random((R, Cc)) < 0.01) * rng.standard_normal((R, Cc)) * 4, 0, 255)
    pts = rng.uniform([4, 4], [Cc - 4, R - 4], (N_POINTS, 2)).round(2)
    return np.ascontiguousarray(img, np.uint8), pts


_visible = {}


def keyframe(big, pts, entry, s, frames, wp, nw, ids):
    """Keyframe `entry` of session s into row s of the call's arrays: the first lap, then the revisits."""
    ox, oy = (STEP * entry, 5) if entry < LAP else (STEP * (entry - LAP) + 2 + s % 4, 6 + s % 3)
    frames[s] = big[oy:oy + ROWS, ox:ox + COLS]
    if (ox, oy) not in _visible:
        q = pts - np.array([ox, oy], np.float64)
        vis = np.nonzero((q[:, 0] >= 2) & (q[:, 0] < COLS - 2) & (q[:, 1] >= 2) & (q[:, 1] < ROWS - 2))[0][:STRIDE]
        _visible[(ox, oy)] = (q[vis].astype(np.float32), vis.astype(np.int32))
    w, vis = _visible[(ox, oy)]
    nw[s], wp[s, :len(vis)], ids[s, :len(vis)] = len(vis), w, vis


class Buffers:
    """Everything a route writes, allocated once."""

    def __init__(self, loop, S, K):
        self.out = (loop.VioLoopKeyframe * S)()
        self.det, self.con = (loop.VioLoopDetection * S)(), (loop.VioLoopConnection * S)()
        self.status, self.pts = np.zeros((S, STRIDE), np.uint8), np.zeros((S, STRIDE, 2), np.float32)
        self.kidx, self.kids, self.norm = np.zeros((S, STRIDE), np.int32), np.zeros((S, STRIDE), np.int32), np.zeros((S, STRIDE, 2))
        self.cur, self.old = np.zeros((S, K, 2), np.float32), np.zeros((S, K, 2), np.float32)
        self.kp, self.desc = np.zeros((S, K, 2), np.float32), np.zeros((S, K, 4), np.uint64)
        self.nf, self.nk = np.zeros(S, np.int32), np.zeros(S, np.int32)
        self.pk, self.pd = np.zeros((S * K, 2), np.float32), np.zeros((S * K, 4), np.uint64)
        self.sel = [np.zeros(S, np.int32) for _ in range(4)]
        self.sel_ids = np.zeros((S, STRIDE), np.int32)


def p(a, t):
    return a.ctypes.data_as(t)


def fused(lib, det, ex, cfg, S, ses, frames, on_device, wp, nw, ids, B):
    t = time.perf_counter()
    rc = lib.vio_loop_detector_keyframes(det._h, ex._h, C.byref(cfg), 22, S, p(ses, _i32p), C.c_void_p(frames), on_device, None, p(wp, _fp),
                                         p(nw, _i32p), p(ids, _i32p), STRIDE, FAST_THRESHOLD, B.out, p(B.status, _u8p), p(B.pts, _fp),
                                         p(B.kidx, _i32p), p(B.kids, _i32p), p(B.norm, _dp), p(B.cur, _fp), p(B.old, _fp), CAP)
    dt = time.perf_counter() - t
    assert rc == 0, rc
    return dt, [B.out[q].detection.status for q in range(S)], sum(B.out[q].connection.connected for q in range(S))


def three_calls(lib, det, ex, cfg, S, ses, frames, wp, nw, ids, B):
    """-> (seconds inside the three C calls, statuses, connected, seconds of numpy packing between them: not counted)."""
    t = time.perf_counter()
    rc = lib.vio_brief_extract(ex._h, p(frames, _u8p), S, p(wp, _fp), p(nw, _i32p), STRIDE, FAST_THRESHOLD, p(B.kp, _fp), p(B.desc, _u64p),
                               p(B.nf, _i32p), p(B.nk, _i32p))
    dt = time.perf_counter() - t
    assert rc in (0, -4), rc                                            # (VIO_ECAP: a FAST list was cut, the outputs are valid)
    t = time.perf_counter()
    o = 0
    for q in range(S):                                                  # detect takes the keyframes back to back
        n = int(B.nk[q])
        B.pk[o:o + n], B.pd[o:o + n] = B.kp[q, :n], B.desc[q, :n]
        o += n
    pack = time.perf_counter() - t
    t = time.perf_counter()
    rc = lib.vio_loop_detector_detect(det._h, S, p(ses, _i32p), p(B.nk, _i32p), p(B.pk, _fp), p(B.pd, _u64p), B.det, p(B.cur, _fp),
                                      p(B.old, _fp), CAP)
    dt += time.perf_counter() - t
    assert rc == 0, rc
    hit = [q for q in range(S) if B.det[q].status == 0]
    connected = 0
    if hit:
        m = len(hit)
        s_, c_, o_, w_ = B.sel
        for i, q in enumerate(hit):
            s_[i], c_[i], o_[i], w_[i], B.sel_ids[i] = ses[q], B.det[q].query, B.det[q].match, nw[q], ids[q]
        t = time.perf_counter()
        rc = lib.vio_loop_detector_connect(det._h, C.byref(cfg), 22, m, p(s_, _i32p), p(c_, _i32p), p(o_, _i32p), p(w_, _i32p),
                                           p(B.sel_ids, _i32p), STRIDE, B.con, p(B.status, _u8p), p(B.pts, _fp), p(B.kidx, _i32p),
                                           p(B.kids, _i32p), p(B.norm, _dp))
        dt += time.perf_counter() - t
        assert rc == 0, rc
        connected = sum(B.con[i].connected for i in range(m))
    return dt, [B.det[q].status for q in range(S)], connected, pack


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sessions", default="1,64,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_keyframes_timing.txt"))
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime has to be the one the library binds)
    import importlib
    pkg = importlib.import_module("vins-mobile_amd")
    from loop_detector_timing import make_vocabulary
    loop, abi = pkg.loop, pkg.abi
    prop = torch.cuda.get_device_properties(0)
    out = ["the loop thread's keyframe step: tools/loop_keyframes_timing.py on one %s (%s, %d CUs), wall time in ms per call"
           % (prop.name, getattr(prop, "gcnArchName", "?").split(":")[0], prop.multi_processor_count),
           "640x480 frames, FAST threshold %d, max_keypoints %d, vocabulary k 10 L 5, dislocal 3, %d first-lap keyframes per session"
           % (FAST_THRESHOLD, CAP, LAP)]
    rng = np.random.default_rng(7)
    blob, _ = make_vocabulary(10, 5, rng)
    voc = loop.BowVocabulary(blob)
    big, pts = make_scene(pkg, rng)
    d = np.load(os.path.join(ROOT, "tests", "golden", "brief_pattern.npz"))
    pat = (d["x1"], d["y1"], d["x2"], d["y2"])
    cfg = abi.default_config(image_rows=ROWS, image_cols=COLS)
    warm, total = 2, LAP + 2 + a.reps
    for S in [int(x) for x in a.sessions.split(",")]:
        lib = loop.bind_loop_detector(loop.bind_brief(abi.load_product()))
        ex = loop.BriefExtractor(ROWS, COLS, pat, max_frames=S, max_keypoints=CAP)
        P = loop.loop_detector_params(1.0, dislocal=3)
        dets = [loop.LoopDetector(voc, P, n_sessions=S, max_entries=total, max_keypoints=CAP) for _ in range(3)]
        bufs = [Buffers(loop, S, CAP) for _ in range(3)]
        ses = np.arange(S, dtype=np.int32)
        frames = np.zeros((S, ROWS, COLS), np.uint8)
        wp, nw, ids = np.zeros((S, STRIDE, 2), np.float32), np.zeros(S, np.int32), np.zeros((S, STRIDE), np.int32)
        times, hist, conn, keys, packs = [[], [], []], {}, 0, [], []
        for e in range(total):
            for s in range(S):
                keyframe(big, pts, e, s, frames, wp, nw, ids)
            dev = loop.DeviceFrames(frames)
            r0 = fused(lib, dets[0], ex, cfg, S, ses, dev.ptr, 1, wp, nw, ids, bufs[0])
            r1 = fused(lib, dets[1], ex, cfg, S, ses, frames.ctypes.data, 0, wp, nw, ids, bufs[1])
            r2 = three_calls(lib, dets[2], ex, cfg, S, ses, frames, wp, nw, ids, bufs[2])
            dev.close()
            assert r0[1] == r1[1] == r2[1] and r0[2] == r1[2] == r2[2], (e, r0[1:], r1[1:], r2[1:3])
            if e >= LAP + warm:
                for i, r in enumerate((r0, r1, r2)):
                    times[i].append(r[0] * 1e3)
                for st in r0[1]:
                    hist[loop.LOOP_STATUS[st]] = hist.get(loop.LOOP_STATUS[st], 0) + 1
                conn += r0[2]
                packs.append(r2[3] * 1e3)
                keys.append(float(np.mean([bufs[0].out[q].n_keys for q in range(S)])))
        out.append("%d sessions per call: %.0f descriptors and %.0f window points per keyframe; timed calls: %s, %d connected"
                   % (S, np.mean(keys), float(nw.mean()), hist, conn))
        out.append(line("  one vio_loop_detector_keyframes, device frames", times[0]))
        out.append(line("  one vio_loop_detector_keyframes, host frames", times[1]))
        out.append(line("  vio_brief_extract + detect + connect", times[2]) + "   + %.3f ms of packing in numpy" % float(np.median(packs)))
        print("\n".join(out[-4:]), flush=True)
        for x in dets:
            x.close()
        ex.close()
    voc.close()
    text = "\n".join(out) + "\n"
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
