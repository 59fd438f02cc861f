#!/usr/bin/env python3
"""Wall time of the two per-keyframe steps of the loop thread that work on resident data, next to the routes a caller had
before them. Needs a gfx950 device; writes profiles/loop_connect_timing.txt (median of --reps with the minimum beside it).

  connection   1 / 64 / 512 sessions through one vio_loop_detector_connect (150 window descriptors against an old keyframe
               of 600, both read from the detector's slabs) against the same pairs through vio_loop_find_connection one
               by one (descriptors and keypoints of both keyframes uploaded per pair).
  features     512 resident sequences through one vio_estimator_keyframe_features against vio_estimator_features +
               vio_features_keyframe per sequence, and the wall time of the process_images call that follows either: that
               is where the second route pays for taking every list off the device.

    python tools/loop_connect_timing.py [--reps 5] [--sequences 512] [--out profiles/loop_connect_timing.txt]
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


def line(name, v, unit="ms"):
    return "%-58s %9.3f %s   (median of %d; min %.3f)" % (name, float(np.median(v)), unit, len(v), min(v))


def time_connect(pkg, reps, out):
    from loop_detector_timing import make_keyframes, make_vocabulary
    loop, abi = pkg.loop, pkg.abi
    rng = np.random.default_rng(7)
    blob, leaves = make_vocabulary(10, 4, rng)
    voc = loop.BowVocabulary(blob)
    n_old, n_win, n_fast, pool = 600, 150, 7, 16
    keys, desc, keys2, desc2 = make_keyframes(leaves, pool, n_old, rng)
    cfg = abi.default_config()
    matcher = loop.Matcher()
    out.append("connection: %d window descriptors against an old keyframe of %d" % (n_win, n_old))
    for S in (1, 64, 512):
        det = loop.LoopDetector(voc, loop.loop_detector_params(geom_check=3), n_sessions=S, max_entries=2, max_keypoints=n_old)
        ses = list(range(S))
        kf = [s % pool for s in ses]
        det.detect(ses, [keys[i] for i in kf], [desc[i] for i in kf])
        det.detect(ses, [keys2[i][:n_fast + n_win] for i in kf], [desc2[i][:n_fast + n_win] for i in kf])
        ids = [np.arange(n_win, dtype=np.int32)] * S
        t_batch, t_single, kept = [], [], 0
        for r in range(reps + 2):
            t = time.perf_counter()
            res = det.connect(cfg, ses, [1] * S, [0] * S, [n_win] * S, ids=ids)
            a = time.perf_counter() - t
            t = time.perf_counter()
            for i in kf:
                w = matcher.find_connection(cfg, desc2[i][n_fast:n_fast + n_win], keys2[i][n_fast:n_fast + n_win], desc[i], keys[i])
            b = time.perf_counter() - t
            if r >= 2:
                t_batch.append(a * 1e3), t_single.append(b * 1e3)
            kept = sum(x["n_kept"] for x in res)
            assert res[-1]["n_kept"] == w[3]
        out.append(line("%3d sessions, one vio_loop_detector_connect" % S, t_batch) + "   %.1f kept per pair" % (kept / S))
        out.append(line("%3d x vio_loop_find_connection" % S, t_single))
        det.close()
    matcher.close(), voc.close()


def time_features(pkg, reps, n_seq, out):
    import replay_synthetic as RS
    abi = pkg.abi
    cfg = abi.default_config()
    W = cfg.window_size
    world = RS.SyntheticWorld(cfg, 5)
    est = pkg.estimator.Estimator(cfg, world.tic, world.ric, n_seq=n_seq)
    est.set_resident(True)
    rng = np.random.default_rng(104)
    init, state = [], {}

    def frame(k):
        """One published frame of every sequence (all of them see the same world)."""
        samples = [world.imu(world.time(0))] if k == 0 else world.imu_interval(k)
        m = len(samples)
        dt = np.full((n_seq, m), world.dt)
        acc = np.tile(np.array([s[0] for s in samples])[None], (n_seq, 1, 1))
        gyr = np.tile(np.array([s[1] for s in samples])[None], (n_seq, 1, 1))
        est.process_imu_batch([m] * n_seq, dt, acc, gyr)
        if k <= W:
            Pt, Rt, Vt = world.truth(k)
            init.append((world.time(k), Pt + rng.normal(0, 0.01, 3), Rt, Vt + rng.normal(0, 0.02, 3)))
            if k == W:
                for q in range(n_seq):
                    est.set_initial_state([i[0] for i in init], [i[1] for i in init], [i[2] for i in init], [i[3] for i in init],
                                          [world.ba] * (W + 1), [world.bg] * (W + 1), seq=q)
        ids, xyz = world.observe(k)
        n = len(ids)
        row = (abi.VioObs * max(n, 1))()
        est._pack_obs(ids, xyz, row, 0)
        obs = (abi.VioObs * (max(n, 1) * n_seq))()
        for q in range(n_seq):
            C.memmove(C.byref(obs, q * max(n, 1) * C.sizeof(abi.VioObs)), row, n * C.sizeof(abi.VioObs))
        cnt = np.full(n_seq, n, np.int32)
        hdr = np.full(n_seq, world.time(k))
        res = (abi.VioFrameResult * n_seq)()
        t = time.perf_counter()
        rc = est.lib.vio_estimator_process_images(est._h, obs, cnt.ctypes.data_as(C.POINTER(C.c_int32)), max(n, 1),
                                                  hdr.ctypes.data_as(C.POINTER(C.c_double)), None, res)
        state["ms"] = (time.perf_counter() - t) * 1e3
        assert rc == 0, rc
        return res

    k = 0
    for _ in range(W + 8):
        res = frame(k)
        k += 1
    assert all(r.action == abi.VIO_FRAME_SOLVED for r in res) and all(est.status(q).resident for q in range(n_seq))
    seqs = list(range(n_seq))
    # the batched call on output arrays that exist already, as a server would hold them: the C call is what is timed
    stride = 256
    sq = np.arange(n_seq, dtype=np.int32)
    o_ids, o_px, o_norm = np.zeros((n_seq, stride), np.int32), np.ones((n_seq, stride, 2), np.float32), np.ones((n_seq, stride, 2), np.float32)
    o_cloud, o_count = np.ones((n_seq, stride, 3)), np.zeros(n_seq, np.int32)
    ip, fp, dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    t_batch, t_next_batch, t_single, t_next_single, t_plain = [], [], [], [], []
    for r in range(-1, reps):                                          # (r = -1: a call that is not timed, like the two of the connection)
        t = time.perf_counter()
        rc = est.lib.vio_estimator_keyframe_features(est._h, n_seq, sq.ctypes.data_as(ip), stride, o_ids.ctypes.data_as(ip), o_px.ctypes.data_as(fp),
                                                     o_norm.ctypes.data_as(fp), o_cloud.ctypes.data_as(dp), o_count.ctypes.data_as(ip))
        if r >= 0:
            t_batch.append((time.perf_counter() - t) * 1e3)
        assert rc == 0 and (o_count > 0).all() and all(est.status(q).resident for q in (0, n_seq - 1))
        if r < 0:
            continue
        frame(k)
        k += 1
        t_next_batch.append(state["ms"])
        frame(k)
        k += 1
        t_plain.append(state["ms"])
        t = time.perf_counter()
        for q in seqs:
            w = est.window(q)
            est.features(q).keyframe(cfg, w["Ps"], w["Rs"], world.tic, world.ric, cap=stride)
        t_single.append((time.perf_counter() - t) * 1e3)
        frame(k)
        k += 1
        t_next_single.append(state["ms"])
        frame(k)                                                       # (every list is back on the device after this one)
        k += 1
    out.append("features: %d resident sequences, window size %d, %d points per keyframe" % (n_seq, W, int(o_count[0])))
    out.append("  samples of the batched call: " + " ".join("%.3f" % x for x in t_batch))
    out.append(line("one vio_estimator_keyframe_features", t_batch))
    out.append(line("    the process_images call after it", t_next_batch))
    out.append(line("%d x (vio_estimator_features + vio_features_keyframe)" % n_seq, t_single))
    out.append(line("    the process_images call after it", t_next_single))
    out.append(line("a process_images call with neither before it", t_plain))
    est.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sequences", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_connect_timing.txt"))
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime has to be the one the library binds)
    import importlib
    pkg = importlib.import_module("vins-mobile_amd")
    prop = torch.cuda.get_device_properties(0)
    out = ["loop closure on resident data: tools/loop_connect_timing.py on one %s (%s, %d CUs), wall time in ms"
           % (prop.name, getattr(prop, "gcnArchName", "?").split(":")[0], prop.multi_processor_count)]
    time_connect(pkg, a.reps, out)
    time_features(pkg, a.reps, a.sequences, out)
    text = "\n".join(out) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
