"""Vocabulary training without a device: the numpy model (tests/voc_train_model.py, written from the text of
include/vio_amd.h) against brute-force properties recomputed with Python integers and against the oracle's vocabulary; the
per-workgroup bodies of csrc/voc_train_core.h on the SIMT emulator (tests/emul/simt_voc_train.cpp) against the model, bit
for bit; the host route of tools/vocabulary_train_timing.py against the model; the refusals that need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import helpers as H
import voc_train_cases as VC
import voc_train_model as VM
from helpers import abi, pkg

loop = pkg.loop
_i32p, _u64p = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
STAT_KEYS = ("n_nodes", "n_words", "capped_nodes", "empty_clusters", "short_nodes", "iterations_max")


def ints(desc):
    """uint64 [n][4] -> Python integers of 256 bits"""
    return [sum(int(w) << (64 * j) for j, w in enumerate(d)) for d in np.asarray(desc, np.uint64).reshape(-1, 4)]


def popcount(x):
    return bin(x).count("1")


def node_int(m, nid):
    return ints(VM.from_bits(m.node_bits[nid]))[0]


@pytest.mark.parametrize("name", ["mid_seeds_only", "cross", "dups", "ties"])
def test_kmeanspp_picks_follow_the_prefix_rule(name):
    """max_iterations = 0: the children of a node are its k-means++ centres. Every centre is a member of the node, the first
    is floor(u n), every later one is the first index whose running sum of min_dists reaches cut; seeding stops below k
    exactly when the sum is 0."""
    m = VM.Model(VC.descriptors(name), **dict(VC.CASES[name][1], max_iterations=0))
    all_ints = ints(m.desc)
    assert m.runs
    for nid, run in list(m.runs.items())[:40]:
        mem = [all_ints[i] for i in run["members"]]
        n, key, seeds = len(mem), run["key"], run["seeds"]
        u = (VM.draw(key, 0) >> 11) * 2.0 ** -53
        assert 0.0 <= u < 1.0 and seeds[0] == min(n - 1, int(u * n))
        md = [popcount(x ^ mem[seeds[0]]) for x in mem]
        for j in range(1, m.k):
            total = sum(md)
            if total == 0:
                assert len(seeds) == j
                break
            factor = ((VM.draw(key, j) >> 11) + 1) * 2.0 ** -53
            assert 0.0 < factor <= 1.0
            cut, run_sum, pick = factor * float(total), 0, None
            for i, d in enumerate(md):
                run_sum += d
                if float(run_sum) >= cut:
                    pick = i
                    break
            assert pick is not None and seeds[j] == pick and md[pick] > 0
            md = [min(a, popcount(x ^ mem[pick])) for a, x in zip(md, mem)]
        else:
            assert len(seeds) == m.k
        assert [node_int(m, c) for c in m.children[nid]] == [mem[s] for s in seeds]     # centres are members
        assert m.runs[nid]["capped"] and m.runs[nid]["iterations"] == 0
    assert m.capped_nodes == len(m.runs)


@pytest.mark.parametrize("name", ["small", "cross", "ties", "empty", "dups", "edge_257", "mid_tfidf"])
def test_fixed_point_of_every_node_that_converged(name):
    m = VC.model(name)
    all_ints = ints(m.desc)
    assert m.capped_nodes == 0 and max(m.iterations_max) <= VM.DEFAULT_ITERATIONS // 2
    for nid, run in list(m.runs.items())[:60]:
        centres = [node_int(m, c) for c in m.children[nid]]
        groups = [[all_ints[i] for i in m.members[c]] for c in m.children[nid]]
        assert sum(len(g) for g in groups) == len(run["members"])
        for c, g in enumerate(groups):
            want = 0
            for b in range(256):
                if sum((x >> b) & 1 for x in g) > len(g) // 2:
                    want |= 1 << b
            assert centres[c] == want                        # (an empty group: the all-zero descriptor)
            for x in g:
                dist = [popcount(x ^ y) for y in centres]
                assert dist.index(min(dist)) == c            # nearest, first on ties
        # groups keep list order
        for c in m.children[nid]:
            pos = {int(i): p for p, i in enumerate(run["members"])}
            order = [pos[int(i)] for i in m.members[c]]
            assert order == sorted(order)


def test_every_case_but_the_capped_ones_converges_within_half_the_default_cap():
    for name in VC.CASES:
        m = VC.model(name)
        if name in VC.CAPPED:
            assert m.capped_nodes > 0
        else:
            assert m.capped_nodes == 0 and max(m.iterations_max) <= VM.DEFAULT_ITERATIONS // 2, name
    assert VC.model("empty").empty_clusters >= 1 and VC.model("dups").short_nodes >= 1


@pytest.mark.parametrize("name", ["small", "cross", "mid_tfidf", "empty"])
def test_ids_in_creation_order_words_in_leaf_order(name):
    m = VC.model(name)
    hdr, nodes, words = VM.parse_blob(m.blob())
    assert hdr[:4] == (m.k, m.L, 0, m.weighting) and list(nodes["id"]) == list(range(1, hdr[4] + 1))
    kids = {}
    for nid, pid in zip(nodes["id"], nodes["pid"]):
        assert pid < nid
        kids.setdefault(int(pid), []).append(int(nid))
    expect, counter = {}, [1]

    def visit(p):   # the reference's recursion: all children of a node, then the subtrees in order
        for c in kids.get(p, []):
            expect[c] = counter[0]
            counter[0] += 1
        for c in kids.get(p, []):
            if c in kids:
                visit(c)
    visit(0)
    assert all(expect[i] == i for i in range(1, hdr[4] + 1))
    leaves = [int(i) for i in nodes["id"] if int(i) not in kids]
    assert list(words["nid"]) == leaves and list(words["wid"]) == list(range(len(leaves)))
    assert all(w == 0.0 for i, w in zip(nodes["id"], nodes["w"]) if int(i) in kids)    # inner nodes: weight 0


@pytest.mark.parametrize("name", ["small", "cross", "ties", "mid_tfidf", "mid_idf", "mid_one_pass"])
def test_oracle_transform_gives_every_training_descriptor_its_leaf(name):
    """The model's file loads in the oracle's vocabulary, and the oracle's descent of a training descriptor ends in the leaf
    the training put it in, with the weight log(NDocs / Ni) of the model's own count."""
    import math
    from test_dbow import OracleVoc
    m = VC.model(name)
    ov = OracleVoc(m.blob())
    try:
        w, ww = ov.transform(m.desc)
        assert np.array_equal(w, m.training_leaf) and np.array_equal(w, m.words)
        ni = np.zeros(m.n_words, int)
        for g in range(m.n_docs):
            ni[np.unique(w[m.image == g])] += 1
        assert np.array_equal(ni, m.ni) and ni.min() >= (0 if m.empty_clusters else 1)
        assert list(ww) == [math.log(m.n_docs / ni[x]) for x in w]
    finally:
        ov.lib.oracle_voc_destroy(ov.h)
    assert len(VC.descriptors("small")[2]) == 0 and VC.model("small").n_docs == 5      # NDocs counts the empty image


# ---- the kernels' bodies on the SIMT emulator -------------------------------------------------------------------------------
def emul_train(descs, order=0, **kw):
    lib = H.build_emul_lib("simt_voc_train.cpp", "libvio_simt_voc_train.so", "VIO_SIMT")
    p = loop.VioVocabularyTrainParams(kw["k"], kw["L"], kw.get("weighting", 0), kw.get("max_iterations", VM.DEFAULT_ITERATIONS), kw.get("seed", 0))
    nd = np.array([len(d) for d in descs], np.int32)
    desc = np.ascontiguousarray(np.concatenate([np.asarray(d, np.uint64).reshape(-1, 4) for d in descs]))
    cap, words = 1 << 20, 1 << 14
    blob, nb, ni, st = C.create_string_buffer(cap), C.c_size_t(0), np.zeros(words, np.int32), loop.VioVocabularyTrainStats()
    rc = lib.simt_voc_train(C.byref(p), len(descs), nd.ctypes.data_as(_i32p), desc.ctypes.data_as(_u64p), order, blob, C.c_size_t(cap),
                            C.byref(nb), ni.ctypes.data_as(_i32p), words, C.byref(st))
    assert rc == 0, rc
    stats = {k: (list(st.iterations_max) if k == "iterations_max" else getattr(st, k)) for k in STAT_KEYS + ("launches",)}
    return blob.raw[:nb.value], ni[:st.n_words].copy(), stats


@pytest.mark.parametrize("name", VC.SMALL)
def test_emulated_kernels_equal_the_model(name):
    m = VC.model(name)
    kw = VC.CASES[name][1]
    blob, ni, stats = emul_train(VC.descriptors(name), **kw)
    assert {k: stats[k] for k in STAT_KEYS} == m.stats()
    assert blob == m.blob() and np.array_equal(ni, m.ni)
    assert stats["launches"] <= 2 + 5 * sum(kw["k"] + stats["iterations_max"][l] for l in range(kw["L"]))


@pytest.mark.parametrize("order", [1, 2, 5])
def test_emulated_kernels_do_not_depend_on_lane_order(order):
    """lanes of a wave run in reverse / shuffled order between two rendezvous points: a missing barrier shows"""
    for name in ("cross", "ties", "edge_257"):
        blob, ni, _ = emul_train(VC.descriptors(name), order=order, **VC.CASES[name][1])
        assert blob == VC.model(name).blob() and np.array_equal(ni, VC.model(name).ni)


# ---- the host route of the timing tool ---------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", [1, 3])
def test_host_route_equals_the_model(threads):
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import vocabulary_train_timing as VT
    m = VC.model("mid_tfidf")
    blob, stats, ms = VT.host_route(VC.descriptors("mid_tfidf"), threads=threads, **VC.CASES["mid_tfidf"][1])
    assert ms > 0 and blob == m.blob()
    assert {k: stats[k] for k in STAT_KEYS} == m.stats()


# ---- refusals that need no device ------------------------------------------------------------------------------------
def train_rc_with_counts(counts, **kw):
    """vio_vocabulary_train's return code for images of the given sizes (the limits are checked before a descriptor is read)"""
    lib = loop.bind_bow(abi.load_product())
    p = loop.VioVocabularyTrainParams()
    lib.vio_vocabulary_train_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    nd = np.array(counts, np.int32)
    desc = np.zeros((max(1, min(int(max(counts)), 64)), 4), np.uint64)
    h = C.c_void_p()
    return lib.vio_vocabulary_train(C.byref(p), len(nd), nd.ctypes.data_as(_i32p), desc.ctypes.data_as(_u64p), C.byref(h), None)


def test_defaults_and_refusals():
    lib = loop.bind_bow(abi.load_product())
    p = loop.VioVocabularyTrainParams()
    lib.vio_vocabulary_train_params_default(C.byref(p))
    assert (p.k, p.L, p.weighting, p.max_iterations, p.seed) == (10, 6, 0, VM.DEFAULT_ITERATIONS, 0)
    for kw in (dict(k=1), dict(k=33), dict(L=0), dict(L=11), dict(weighting=-1), dict(weighting=4), dict(max_iterations=-1),
               dict(max_iterations=4097)):
        assert train_rc_with_counts([20], **kw) == abi.VIO_EINVAL, kw
    assert train_rc_with_counts([0, 0, 0]) == abi.VIO_EINVAL        # no descriptor at all
    assert train_rc_with_counts([5, -1]) == abi.VIO_EINVAL
    assert train_rc_with_counts([(1 << 22) + 1]) == abi.VIO_ECAP
    assert train_rc_with_counts([(1 << 16) + 1]) == abi.VIO_ECAP
    n = C.c_size_t(0)
    assert lib.vio_vocabulary_serialize(None, None, 0, C.byref(n)) == abi.VIO_EINVAL
    assert lib.vio_vocabulary_save(None, b"x") == abi.VIO_EINVAL
    assert lib.vio_vocabulary_train(None, 1, None, None, None, None) == abi.VIO_EINVAL
