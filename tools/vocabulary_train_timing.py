#!/usr/bin/env python3
"""Times vocabulary training on both routes at k = 10: vio_vocabulary_train (csrc/vio_voc_train.hip, level-synchronous on the
device) against a plain C++ restatement of the same semantics with the same random stream (tools/vocabulary_train_host_route.cpp,
built on first use) on ONE thread and on the threads the box grants (16 at most), for (L = 4, 10^5 descriptors in 200 images)
and (L = 6, 10^6 descriptors in 2 000 images). The descriptors lie near the leaves of a tests/test_dbow.py::make_vocabulary-style
tree (every child = its parent with 24 bits flipped, a descriptor = a random leaf with 10 bits flipped). Both routes must give
the same file, byte for byte; the table has the median of --repeat runs with the minimum beside it, the device's launches and
iterations, and its time per pass (seeding / iterations / regrouping / weights, from events on the training's stream).
    python tools/vocabulary_train_timing.py [--repeat 5] > profiles/vocabulary_train_timing.txt"""
import argparse
import ctypes as C
import importlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("vins-mobile_amd")
abi, loop = pkg.abi, pkg.loop
from init_sfm_timing import host_width  # noqa: E402  (the threads the box grants: one definition for the timing tools)

_i32p, _u64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
STAT_KEYS = ("n_nodes", "n_words", "capped_nodes", "empty_clusters", "short_nodes", "iterations_max")
SIZES = ((4, 100_000, 200), (6, 1_000_000, 2_000))   # (L, descriptors, images)


def driver():
    """tools/libvocabulary_train_host_route.so, built with g++ when missing or older than its source."""
    src, so = os.path.join(ROOT, "tools", "vocabulary_train_host_route.cpp"), os.path.join(ROOT, "tools", "libvocabulary_train_host_route.so")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-mpopcnt", "-I" + os.path.join(ROOT, "include"), "-o", so,
                               src])
    d = C.CDLL(so)
    d.vocabulary_train_host_route_run.restype = C.c_double
    d.vocabulary_train_host_route_run.argtypes = [C.POINTER(loop.VioVocabularyTrainParams), C.c_int32, _i32p, _u64p, C.c_int32, C.c_char_p,
                                                  C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(loop.VioVocabularyTrainStats)]
    return d


def _pack(descs):
    n_desc = np.array([len(d) for d in descs], np.int32)
    desc = np.ascontiguousarray(np.concatenate([np.asarray(d, np.uint64).reshape(-1, 4) for d in descs] + [np.zeros((0, 4), np.uint64)]))
    return n_desc, desc


def host_route(descs, threads=1, k=10, L=6, weighting=0, max_iterations=None, seed=0):
    """-> (file bytes, stats dict, milliseconds) of the host route"""
    p = loop.VioVocabularyTrainParams()
    loop.bind_bow(abi.load_product()).vio_vocabulary_train_params_default(C.byref(p))
    p.k, p.L, p.weighting, p.seed = k, L, weighting, seed
    if max_iterations is not None:
        p.max_iterations = max_iterations
    n_desc, desc = _pack(descs)
    cap = 24 + 56 * sum(min(k ** l, k * len(desc)) for l in range(1, L + 1))   # a level has at most k^l nodes, k per split node
    blob, nb, st = C.create_string_buffer(cap), C.c_size_t(0), loop.VioVocabularyTrainStats()
    ms = driver().vocabulary_train_host_route_run(C.byref(p), len(n_desc), n_desc.ctypes.data_as(_i32p), desc.ctypes.data_as(_u64p), threads,
                                                  blob, cap, C.byref(nb), C.byref(st))
    assert ms >= 0, "the host route refused its arguments or the file did not fit"
    stats = {f: (list(st.iterations_max) if f == "iterations_max" else getattr(st, f)) for f in STAT_KEYS}
    return blob.raw[:nb.value], stats, ms


def synthetic(k, L, n, n_images, seed=1, flips=24, noise=10):
    """n descriptors near the leaves of a k-ary tree of depth L, dealt to n_images images in order"""
    rng = np.random.default_rng(seed)

    def flipped(d, count):
        d = d.copy()
        rows = np.arange(len(d))
        for _ in range(count):
            b = rng.integers(0, 256, len(d))
            d[rows, b >> 6] ^= np.uint64(1) << (b & 63).astype(np.uint64)
        return d
    level = rng.integers(0, 2 ** 63, (1, 4), dtype=np.int64).astype(np.uint64)
    for _ in range(L):
        level = flipped(np.repeat(level, k, axis=0), flips)
    d = flipped(level[rng.integers(0, len(level), n)], noise)
    per = n // n_images
    return [d[i * per:(i + 1) * per if i < n_images - 1 else n] for i in range(n_images)]


def measure(descs, k, L, repeat=5, width=None, seed=0):
    """-> dict of the table's row"""
    width = width or min(16, host_width())
    kw = dict(k=k, L=L, seed=seed)
    voc, stats = loop.BowVocabulary.train(descs, **kw)   # warm-up: code objects, buffers' first touch
    want = voc.serialize()
    voc.close()
    dev, passes = [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        voc, stats = loop.BowVocabulary.train(descs, **kw)
        dev.append(1e3 * (time.perf_counter() - t0))
        passes.append(stats["pass_ms"])
        assert voc.serialize() == want, "two runs with one seed differ"
        voc.close()
    one, pool = [], []
    for _ in range(repeat):
        b1, s1, ms1 = host_route(descs, threads=1, **kw)
        bp, sp, msp = host_route(descs, threads=width, **kw)
        assert b1 == want and bp == want, "the host route's file differs from the device's"
        one.append(ms1), pool.append(msp)
    return dict(n=sum(len(d) for d in descs), L=L, stats=stats, width=width, dev=(float(np.median(dev)), min(dev)),
                one=(float(np.median(one)), min(one)), pool=(float(np.median(pool)), min(pool)),
                passes=[float(np.median([p[i] for p in passes])) for i in range(4)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--sizes", type=str, default="")   # e.g. 3:6000:40 for a quick look
    args = ap.parse_args()
    import torch  # noqa: F401  (HIP runtime first)
    sizes = [tuple(int(x) for x in s.split(":")) for s in args.sizes.split(",")] if args.sizes else SIZES
    print("vocabulary training, k = 10, TF_IDF, default cap: vio_vocabulary_train (whole call: upload, levels, weights, the vocabulary) against "
          "tools/vocabulary_train_host_route.cpp on one thread and on a pool; same seed, the three files are equal byte for byte")
    print("%-4s %-10s %-8s %-9s %-22s %-24s %-24s %-9s %-9s" % ("L", "desc", "nodes", "launches", "device ms (min)", "host 1 thread ms (min)",
                                                            "host pool ms (min)", "1 / dev", "pool / dev"))
    rows = []
    for L, n, n_images in sizes:
        r = measure(synthetic(10, L, n, n_images), 10, L, repeat=args.repeat)
        rows.append(r)
        print("%-4d %-10d %-8d %-9d %-22s %-24s %-24s %-9.1f %-9.1f" % (
            L, r["n"], r["stats"]["n_nodes"], r["stats"]["launches"], "%.1f (%.1f)" % r["dev"], "%.1f (%.1f)" % r["one"],
            "%.1f (%.1f) x%d" % (r["pool"] + (r["width"],)), r["one"][0] / r["dev"][0], r["pool"][0] / r["dev"][0]))
    for r in rows:
        print("L %d, %d descriptors: iterations_max per level %s, capped %d, short %d, empty clusters %d; device passes, median ms: seeding %.2f, "
              "iterations %.2f, regrouping %.2f, weights %.2f" % ((r["L"], r["n"], r["stats"]["iterations_max"][:r["L"]], r["stats"]["capped_nodes"],
                                                               r["stats"]["short_nodes"], r["stats"]["empty_clusters"]) + tuple(r["passes"])))
    print("(medians of %d runs after one warm-up; a pass's time runs from its first launch to the next pass's first launch on the stream, the "
          "host's part in between included)" % args.repeat)


if __name__ == "__main__":
    main()
