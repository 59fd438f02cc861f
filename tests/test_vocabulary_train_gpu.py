"""vio_vocabulary_train on the device (csrc/vio_voc_train.hip, voc_train_core.h) against the numpy model written from the
header's text (tests/voc_train_model.py): the serialized bytes are equal -- tree, descriptors, ids, words and weights -- and
so are the stats, at the smallest shapes where each pass can go wrong (tests/voc_train_cases.py). Then what does not need
the model: the training descriptors transform to their training leaves, a database of the training images finds each
image itself, serialization round trips, determinism, the launch bound, refusals."""
import struct

import numpy as np
import pytest

import voc_train_cases as VC
import voc_train_model as VM
from helpers import pkg

loop = pkg.loop
pytestmark = pytest.mark.gpu
STAT_KEYS = ("n_nodes", "n_words", "capped_nodes", "empty_clusters", "short_nodes", "iterations_max")
_trained = {}


def trained(name):
    """(bytes, stats) of the device's training of a case, once per process"""
    if name not in _trained:
        voc, stats = loop.BowVocabulary.train(VC.descriptors(name), **VC.CASES[name][1])
        try:
            _trained[name] = (voc.serialize(), stats)
        finally:
            voc.close()
    return _trained[name]


@pytest.mark.parametrize("name", list(VC.CASES))
def test_device_equals_model(name):
    m = VC.model(name)
    got, stats = trained(name)
    want = m.blob()
    print(name, {k: stats[k] for k in STAT_KEYS}, "launches", stats["launches"], "kernel_ms %.3f" % stats["kernel_ms"])
    assert {k: stats[k] for k in STAT_KEYS} == m.stats()
    assert stats["n_descriptors"] == len(m.desc)
    if got != want:
        # both sides call the same libm: the weights are expected to be equal bit for bit. Should only they differ, 1 ulp is
        # allowed on the weights alone and what differed is printed; everything else stays bit for bit.
        (gh, gn, gw), (wh, wn, ww) = VM.parse_blob(got), VM.parse_blob(want)
        assert gh == wh and np.array_equal(gw, ww)
        assert np.array_equal(gn["id"], wn["id"]) and np.array_equal(gn["pid"], wn["pid"]) and np.array_equal(gn["d"], wn["d"])
        bad = np.flatnonzero(gn["w"] != wn["w"])
        print("weights differ at nodes", gn["id"][bad][:10], gn["w"][bad][:10], wn["w"][bad][:10])
        assert np.all(np.abs(gn["w"][bad] - wn["w"][bad]) <= np.spacing(np.abs(wn["w"][bad])))
    if name in VC.CAPPED:
        assert stats["capped_nodes"] > 0
    else:
        assert stats["capped_nodes"] == 0
    if name == "dups":
        assert stats["short_nodes"] >= 1
    if name == "empty":
        assert m.empty_clusters >= 1 and stats["empty_clusters"] >= 1   # (the model did see one: the case cannot rot silently)


@pytest.mark.parametrize("name", ["small", "mid_tfidf", "cross", "ties", "edge_257"])
def test_training_descriptors_reach_their_training_leaves(name):
    """Independent of the model: the group a descriptor ends in is the leaf the ordinary descent gives it (the last
    association is computed with the last centres), so the words of a leaf's members are one word, and words in id order
    are the leaves in creation order."""
    descs = VC.descriptors(name)
    voc, stats = loop.BowVocabulary.train(descs, **VC.CASES[name][1])
    try:
        words = np.concatenate([t[0] for t in voc.transform(descs)])
        _, nodes, wrec = VM.parse_blob(voc.serialize())
        assert np.array_equal(wrec["wid"], np.arange(len(wrec))) and np.all(np.diff(wrec["nid"]) > 0)
        # descend by hand from the file: children of a node in id order, nearest first
        kids = {}
        for nid, pid in zip(nodes["id"], nodes["pid"]):
            kids.setdefault(int(pid), []).append(int(nid))
        bits = VM.to_bits(nodes["d"])
        wid = {int(n): int(w) for n, w in zip(wrec["nid"], wrec["wid"])}
        dbits = VM.to_bits(np.concatenate(descs))
        for i in range(0, len(dbits), max(1, len(dbits) // 200)):
            node = 0
            while node in kids:
                ch = kids[node]
                node = ch[int(np.argmin([(dbits[i] != bits[c - 1]).sum() for c in ch]))]
            assert wid[node] == words[i]
        # every word is the leaf of at least one training descriptor unless its group was empty
        assert len(np.unique(words)) == stats["n_words"] - stats["empty_clusters"]
    finally:
        voc.close()


def test_database_of_the_training_images_finds_each_image():
    descs = VC.descriptors("mid_tfidf")
    voc, _ = loop.BowVocabulary.train(descs, **VC.CASES["mid_tfidf"][1])
    db = loop.BowDatabase(voc, max_entries=len(descs), max_total_words=len(descs) * 256)
    try:
        bows = [(t[2], t[3]) for t in voc.transform(descs)]
        for e, (w, v) in enumerate(bows):
            assert len(w) > 0 and db.add(w, v) == e
        for e, (ent, sc) in enumerate(db.query(bows, [-1] * len(bows), max_results=1)):
            assert ent[0] == e and sc[0] >= 1 - 1e-12
    finally:
        db.close()
        voc.close()


def _same_transform(a, b, descs):
    for (w1, ww1, bw1, bv1), (w2, ww2, bw2, bv2) in zip(a.transform(descs), b.transform(descs)):
        assert np.array_equal(w1, w2) and np.array_equal(ww1, ww2) and np.array_equal(bw1, bw2) and np.array_equal(bv1, bv2)


def test_serialization_round_trips(tmp_path):
    from test_dbow import make_vocabulary
    descs = VC.descriptors("cross")
    voc, _ = loop.BowVocabulary.train(descs, **VC.CASES["cross"][1])
    blob = voc.serialize()
    path = tmp_path / "trained.bin"
    voc.save(path)
    assert path.read_bytes() == blob
    again, loaded = loop.BowVocabulary(blob=blob), loop.BowVocabulary(path=str(path))
    shuffled, _ = make_vocabulary(4, 3, seed=12)
    other = loop.BowVocabulary(blob=shuffled)
    back = loop.BowVocabulary(blob=other.serialize())
    try:
        assert voc.info() == again.info() == loaded.info()
        _same_transform(voc, again, descs), _same_transform(voc, loaded, descs)
        assert again.serialize() == blob
        assert other.info() == back.info()
        _same_transform(other, back, descs)
        n = pkg.loop.C.c_size_t(0)
        assert voc.lib.vio_vocabulary_serialize(voc._h, None, 0, pkg.loop.C.byref(n)) == 0 and n.value == len(blob)
        small = pkg.loop.C.create_string_buffer(16)
        assert voc.lib.vio_vocabulary_serialize(voc._h, small, 16, pkg.loop.C.byref(n)) == pkg.abi.VIO_ECAP and n.value == len(blob)
    finally:
        for v in (voc, again, loaded, other, back):
            v.close()


def test_same_seed_same_bytes_other_seed_other_bytes():
    descs, kw = VC.descriptors("cross"), dict(VC.CASES["cross"][1])
    first, _ = trained("cross")
    voc, _ = loop.BowVocabulary.train(descs, **kw)
    kw["seed"] = kw["seed"] + 1
    voc2, _ = loop.BowVocabulary.train(descs, **kw)
    try:
        assert voc.serialize() == first
        assert voc2.serialize() != first
    finally:
        voc.close(), voc2.close()


def test_launches_within_the_headers_bound():
    """include/vio_amd.h: launches <= 2 + 5 * sum over levels of (k + iterations_max[level])"""
    _, stats = trained("mid_tfidf")
    k, L = VC.CASES["mid_tfidf"][1]["k"], VC.CASES["mid_tfidf"][1]["L"]
    # (the tree of this case has 992 nodes, not the 10 + 100 + 1 000 of a full one: k-medians leaves some level-2 groups
    # with no more than k members, which get one child per member, and two clusters end empty)
    assert stats["n_nodes"] == VC.model("mid_tfidf").n_nodes > 900 and max(stats["iterations_max"]) > 0
    assert 0 < stats["launches"] <= 2 + 5 * sum(k + stats["iterations_max"][l] for l in range(L))


def test_rows_of_the_timing_table():
    """tools/vocabulary_train_timing.py: a row is measured only if the device's file and the host route's files (one thread
    and a pool) are equal byte for byte; the times are finite, medians not below their minima."""
    import os
    import sys
    import helpers as H
    sys.path.insert(0, os.path.join(H.ROOT, "tools"))
    import vocabulary_train_timing as VT
    r = VT.measure(VC.descriptors("cross"), 4, 3, repeat=1, width=2, seed=5)
    assert r["n"] == 800 and r["stats"]["n_nodes"] == VC.model("cross").n_nodes
    for key in ("dev", "one", "pool"):
        assert np.isfinite(r[key]).all() and r[key][0] >= r[key][1] > 0
    assert len(r["passes"]) == 4 and all(p >= 0 for p in r["passes"]) and sum(r["passes"]) > 0
    d = VT.synthetic(10, 2, 1000, 7)
    assert [len(x) for x in d] == [142] * 6 + [148] and len(np.unique(np.concatenate(d), axis=0)) > 900


def test_refusals():
    d = [VC.random_descriptors(np.random.default_rng(1), 20)]
    for kw in (dict(k=1, L=2), dict(k=33, L=2), dict(k=4, L=0), dict(k=4, L=11), dict(k=4, L=2, weighting=4), dict(k=4, L=2, max_iterations=-1),
               dict(k=4, L=2, max_iterations=4097)):
        with pytest.raises(RuntimeError, match="rc=-1"):
            loop.BowVocabulary.train(d, **kw)
    with pytest.raises(RuntimeError, match="rc=-1"):
        loop.BowVocabulary.train([np.zeros((0, 4), np.uint64)] * 3, k=4, L=2)       # no descriptor at all
    from test_vocabulary_train import train_rc_with_counts
    assert train_rc_with_counts([(1 << 22) + 1]) == pkg.abi.VIO_ECAP                  # more descriptors than the limit
    assert train_rc_with_counts([(1 << 16) + 1]) == pkg.abi.VIO_ECAP                  # more in one image than the limit
    assert train_rc_with_counts([5, -1]) == pkg.abi.VIO_EINVAL
    voc, stats = loop.BowVocabulary.train(d, k=20, L=6)                             # the largest tree the issue names
    voc.close()
    assert stats["n_words"] == 20
