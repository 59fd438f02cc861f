#!/usr/bin/env python3
"""Time of one batched vio_loop_detector_detect call (the newest keyframe of every session, ~1000 descriptors each)
against databases of a few thousand entries, next to the route a caller had before the detector existed for the part of
the work that route can do: per session, one after the other, vio_vocabulary_transform + vio_bow_database_query +
vio_bow_database_add. Both routes see the same keyframes and the same database contents, are warmed up first and are
timed alternately in the same process: wall time around calls that end in a stream synchronise, median of --reps.
Needs a gfx950 device. Prints one line per route and a JSON summary line.

    python tools/loop_detector_timing.py [--sessions 64] [--entries 2000] [--desc 1000] [--levels 5] [--reps 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_vocabulary(k, L, rng):
    """A complete k-ary tree in the app's binary layout (loop/VocabularyBinary.hpp), breadth-first ids; a child is its parent
    with 24 bits flipped; leaves carry idf-like weights. -> bytes, leaf descriptors uint64 [k^L][4]."""
    n_nodes = sum(k ** l for l in range(1, L + 1))
    desc = np.zeros((n_nodes + 1, 4), np.uint64)
    desc[0] = rng.integers(0, 2 ** 63, 4, dtype=np.int64).astype(np.uint64)
    parent = (np.arange(1, n_nodes + 1) - 1) // k
    lo = 1
    for lev in range(1, L + 1):
        hi = lo + k ** lev
        d = desc[parent[lo - 1:hi - 1]].copy()
        for _ in range(24):
            b = rng.integers(0, 256, hi - lo)
            d[np.arange(hi - lo), b >> 6] ^= np.uint64(1) << (b & 63).astype(np.uint64)
        desc[lo:hi] = d
        lo = hi
    first_leaf = n_nodes + 1 - k ** L
    rec = np.zeros(n_nodes, np.dtype([("nid", "<i4"), ("pid", "<i4"), ("w", "<f8"), ("d", "<u8", 4)]))
    rec["nid"], rec["pid"], rec["d"] = np.arange(1, n_nodes + 1), parent, desc[1:]
    rec["w"][first_leaf - 1:] = rng.uniform(0.5, 9.0, k ** L)
    words = np.zeros(k ** L, np.dtype([("nid", "<i4"), ("wid", "<i4")]))
    words["nid"], words["wid"] = np.arange(first_leaf, n_nodes + 1), rng.permutation(k ** L)
    hdr = np.array([k, L, 0, 0, n_nodes, k ** L], "<i4")
    return hdr.tobytes() + rec.tobytes() + words.tobytes(), desc[first_leaf:]


def flip_bits(d, n, rng):
    d = d.copy()
    idx = np.indices(d.shape[:-1])
    for _ in range(n):
        b = rng.integers(0, 256, d.shape[:-1])
        np.bitwise_xor.at(d, (*idx, b >> 6), np.uint64(1) << (b & 63).astype(np.uint64))
    return d


def make_keyframes(leaves, n_kf, n_desc, rng):
    """n_kf places of n_desc landmarks near random leaves (10 bits flipped) with 3D points at depths 4..12 m. -> the first
    visit (keys, descriptors) and a second visit from a pose displaced sideways and rotated a little: 4 more bits
    flipped per descriptor, <= 0.3 px of noise, feature order shuffled."""
    d = flip_bits(leaves[rng.integers(0, len(leaves), (n_kf, n_desc))], 10, rng)
    xyz = np.stack([rng.uniform(-1.8, 1.8, (n_kf, n_desc)), rng.uniform(-1, 1, (n_kf, n_desc)), rng.uniform(4, 12, (n_kf, n_desc))], -1)

    def view(t, yaw, roll):
        cy, sy, cz, sz = np.cos(yaw), np.sin(yaw), np.cos(roll), np.sin(roll)
        R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        pc = (xyz - np.array(t)) @ R
        uv = 460.0 * pc[..., :2] / pc[..., 2:3] + np.array([320.0, 240.0])
        return (uv + rng.uniform(-0.3, 0.3, uv.shape)).astype(np.float32)
    keys_a, keys_b, d_b = view([0, 0, 0], 0.0, 0.0), view([0.35, 0.06, 0.15], 0.04, 0.02), flip_bits(d, 4, rng)
    for f in range(n_kf):
        perm = rng.permutation(n_desc)
        keys_b[f], d_b[f] = keys_b[f][perm], d_b[f][perm]
    return keys_a, d, keys_b, d_b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=64)
    ap.add_argument("--entries", type=int, default=2000, help="database entries per session before the timed calls")
    ap.add_argument("--desc", type=int, default=1000)
    ap.add_argument("--levels", type=int, default=5, help="vocabulary depth (k = 10)")
    ap.add_argument("--pool", type=int, default=192, help="distinct keyframes the databases are filled from")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime has to be the one the library binds)
    import importlib
    pkg = importlib.import_module("vins-mobile_amd")
    loop = pkg.loop
    rng = np.random.default_rng(a.seed)
    blob, leaves = make_vocabulary(10, a.levels, rng)
    voc = loop.BowVocabulary(blob)
    S, total = a.sessions, a.entries + a.warmup + a.reps
    keys, desc, keys2, desc2 = make_keyframes(leaves, a.pool, a.desc, rng)   # the databases hold first visits, the timed calls revisit
    pick = lambda s, e: (s * 37 + e * 11) % a.pool                      # keyframe of session s at entry e
    det = loop.LoopDetector(voc, loop.loop_detector_params(), n_sessions=S, max_entries=total, max_keypoints=a.desc)
    dbs = [loop.BowDatabase(voc, max_entries=total, max_total_words=total * a.desc) for _ in range(S)]
    bows = [(t[2], t[3]) for t in voc.transform(list(desc))]
    t0 = time.perf_counter()
    ses = list(range(S))
    for e in range(a.entries):                                          # the same contents on both sides
        kf = [pick(s, e) for s in ses]
        det.detect(ses, [keys[i] for i in kf], [desc[i] for i in kf])
        for s in ses:
            dbs[s].add(*bows[kf[s]])
    print("filled %d sessions x %d entries in %.1f s" % (S, a.entries, time.perf_counter() - t0), flush=True)
    dislocal = det.params.dislocal
    t_det, t_dev, t_base, hist = [], [], [], {}
    for r in range(a.warmup + a.reps):
        e = a.entries + r
        kf = [pick(s, e) for s in ses]
        t = time.perf_counter()
        res = det.detect(ses, [keys2[i] for i in kf], [desc2[i] for i in kf])
        dt_det, dev = time.perf_counter() - t, det.kernel_ms()
        t = time.perf_counter()
        for s in ses:                                                   # the route without the detector, session by session
            _, _, bw, bv = voc.transform([desc2[kf[s]]])[0]
            dbs[s].query([(bw, bv)], [e - dislocal], 50)
            dbs[s].add(bw, bv)
        dt_base = time.perf_counter() - t
        if r >= a.warmup:
            t_det.append(dt_det * 1e3), t_dev.append(dev), t_base.append(dt_base * 1e3)
            for q, _, _ in res:
                hist[loop.LOOP_STATUS[q["status"]]] = hist.get(loop.LOOP_STATUS[q["status"]], 0) + 1
    med = lambda v: float(np.median(v))
    print("batched detect   : %8.3f ms per call (min %.3f max %.3f), device %.3f ms, %.0f keyframes/s" %
          (med(t_det), min(t_det), max(t_det), med(t_dev), S / med(t_det) * 1e3))
    print("per-session route: %8.3f ms per %d x (transform + query + add) (min %.3f max %.3f), %.0f keyframes/s" %
          (med(t_base), S, min(t_base), max(t_base), S / med(t_base) * 1e3))
    print("statuses of the timed calls:", hist)
    print(json.dumps(dict(sessions=S, entries=a.entries, desc=a.desc, levels=a.levels, reps=a.reps, detect_ms=med(t_det),
                          detect_device_ms=med(t_dev), per_session_route_ms=med(t_base))))
    det.close()
    for d in dbs:
        d.close()
    voc.close()


if __name__ == "__main__":
    main()
