"""Inputs of the vocabulary-training tests (tests/test_vocabulary_train.py on the CPU, tests/test_vocabulary_train_gpu.py on the
device) and their models (tests/voc_train_model.py), each computed once per process. Every case is the smallest shape at
which one pass of csrc/voc_train_core.h can go wrong; a block is 256 positions, a wave 64."""
import functools

import numpy as np

import voc_train_model as VM


def random_descriptors(rng, n):
    return rng.integers(0, 2 ** 63, (n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4)).astype(np.uint64)


def flip(d, bits):
    d = d.copy()
    for b in bits:
        d[int(b) >> 6] ^= np.uint64(1) << np.uint64(int(b) & 63)
    return d


def near_leaves(rng, k, L, n, flips=24, noise=10):
    """n descriptors near the leaves of a tests/test_dbow.py::make_vocabulary-style tree: every child = its parent with
    `flips` random bits flipped, a descriptor = a random leaf with `noise` random bits flipped."""
    level = [random_descriptors(rng, 1)[0]]
    for _ in range(L):
        level = [flip(p, rng.integers(0, 256, flips)) for p in level for _ in range(k)]
    return np.array([flip(level[int(rng.integers(0, len(level)))], rng.integers(0, 256, noise)) for _ in range(n)], np.uint64)


def split(d, sizes):
    out, o = [], 0
    for s in sizes:
        out.append(d[o:o + s])
        o += s
    assert o == len(d)
    return out


def _small():
    rng = np.random.default_rng(3)
    return split(random_descriptors(rng, 40), [9, 11, 0, 13, 7])


def _trivial_root():
    return [random_descriptors(np.random.default_rng(4), 7)]


def _mid():
    rng = np.random.default_rng(5)
    return split(near_leaves(rng, 10, 3, 6000), [150] * 40)


def _edge(n):
    return [random_descriptors(np.random.default_rng(100 + n), n)]


def _cross():
    rng = np.random.default_rng(6)
    return split(random_descriptors(rng, 800), [300, 300, 200])


def _dups():
    rng = np.random.default_rng(7)
    base = random_descriptors(rng, 4)
    return split(base[rng.integers(0, 4, 300)], [100, 120, 80])


def _ties():
    """descriptors that differ only in bits 0-7, 60-67 and 248-255: distance ties, exact-half majorities, word boundaries"""
    rng = np.random.default_rng(8)
    base = random_descriptors(rng, 1)[0]
    where = list(range(0, 8)) + list(range(60, 68)) + list(range(248, 256))
    out = [flip(base, [b for b in where if rng.random() < 0.5]) for _ in range(96)]
    return split(np.array(out, np.uint64), [32, 32, 32])


def _empty():
    rng = np.random.default_rng(2)
    d = np.zeros((30, 4), np.uint64)
    for i in range(30):
        for b in rng.choice(256, 3, replace=False):
            d[i, int(b) >> 6] |= np.uint64(1) << np.uint64(int(b) & 63)
    return split(d, [10, 10, 10])


# name -> (descriptors per image, keyword arguments of the training)
CASES = {
    "small": (_small, dict(k=3, L=2)),
    "trivial_root": (_trivial_root, dict(k=10, L=2)),
    "mid_tfidf": (_mid, dict(k=10, L=3, weighting=0)),
    "mid_idf": (_mid, dict(k=10, L=3, weighting=2)),
    "mid_seeds_only": (_mid, dict(k=10, L=3, max_iterations=0)),
    "mid_one_pass": (_mid, dict(k=10, L=3, max_iterations=1)),
    "cross": (_cross, dict(k=4, L=3, seed=5)),
    "dups": (_dups, dict(k=10, L=3, seed=1)),
    "ties": (_ties, dict(k=4, L=2, seed=2)),
    "empty": (_empty, dict(k=4, L=2, seed=6)),
}
for _n in (63, 64, 65, 255, 256, 257, 513):
    CASES["edge_%d" % _n] = (functools.partial(_edge, _n), dict(k=4, L=1, seed=_n))
CAPPED = ("mid_seeds_only", "mid_one_pass")          # the only cases the cap may stop
SMALL = [c for c in CASES if not c.startswith("mid")]  # what the SIMT emulator runs


@functools.lru_cache(maxsize=None)
def descriptors(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def model(name):
    return VM.Model(descriptors(name), **CASES[name][1])
