"""The loop detector (csrc/vio_loop_detector.hip): TemplatedLoopDetector::detectLoop (VINS_ios/loop/TemplatedLoopDetector.h
:668-877) for n sessions per call, against a restatement written here in plain Python / numpy, line by line after the
reference and sharing no code with the product: tree descent and BowVector in numpy (cross-checked below against
oracle_voc_transform / oracle_voc_bow), L1 scores as ordered Python float sums, islands / temporal window /
neighbour-ratio matching as plain loops, the RANSAC by oracle_fundamental_ransac (old points first).
PARITY UNPINNED like the rest of DBoW2 here: DLoopDetector needs OpenCV and boost, which the image does not have.
Every comparison is exact: integers and index lists equal, doubles bit-identical, kept point pairs identical and in order.
Where a database query returns equal scores the product orders them by ascending entry id (vio_amd.h); so does the
restatement (the reference's std::sort leaves that order open)."""
import collections
import ctypes as C
import functools
import os
import struct
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import helpers as H
from helpers import pkg
from test_dbow import OracleVoc, make_vocabulary

loop, abi = pkg.loop, pkg.abi
VK, VL = 10, 4
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
STATUS = loop.LOOP_STATUS
ALPHA, MIN_NSS = float(np.float32(0.3)), float(np.float32(0.005))   # float members widened to double


def as_bytes(d):
    """uint64 [n][4] descriptors -> uint8 [n][32]: bit i = bit (i & 63) of word i >> 6 = bit (i & 7) of byte i >> 3."""
    return np.ascontiguousarray(d, "<u8").reshape(-1, 4).view(np.uint8).reshape(-1, 32)


def ham(a, b):
    return int(POP[a ^ b].sum())


# ---- the restatement ------------------------------------------------------------------------------------------------------
class Voc:
    """TemplatedVocabulary from the file's bytes (loadBin: children in file order)."""

    def __init__(self, blob):
        self.k, self.L, _, self.weighting, n_nodes, n_words = struct.unpack("<6i", blob[:24])
        self.desc = np.zeros((n_nodes + 1, 32), np.uint8)
        self.weight = np.zeros(n_nodes + 1)
        children = collections.defaultdict(list)
        for i in range(n_nodes):
            o = 24 + 48 * i
            nid, pid, w = struct.unpack("<iid", blob[o:o + 16])
            self.desc[nid] = np.frombuffer(blob[o + 16:o + 48], np.uint8)
            self.weight[nid] = w
            children[pid].append(nid)
        self.word = np.full(n_nodes + 1, -1, np.int64)
        for i in range(n_words):
            nid, wid = struct.unpack("<ii", blob[24 + 48 * n_nodes + 8 * i:][:8])
            self.word[nid] = wid
        # a complete k-ary tree (what make_vocabulary writes): the descent below takes all features down level by level
        assert all(len(c) == self.k for c in children.values()) and len(children) == sum(self.k ** l for l in range(self.L))
        self.children = np.zeros((n_nodes + 1, self.k), np.int64)
        for p, c in children.items():
            self.children[p] = c

    def transform(self, f, levelsup):
        """transform(feature, id, w, &nid, levelsup) :1212-1254 for every row of f -> node-level word id, weight, nid."""
        n = len(f)
        node = np.zeros(n, np.int64)
        nid_level = self.L - levelsup
        nid = np.zeros(n, np.int64)                                   # `if(nid_level <= 0) *nid = 0`
        for level in range(1, self.L + 1):
            cand = self.children[node]                                # [n][k]
            dist = POP[f[:, None, :] ^ self.desc[cand]].sum(-1)
            node = cand[np.arange(n), dist.argmin(1)]                 # first minimum: `d < best_d`
            if level == nid_level:
                nid = node.copy()
        return self.word[node], self.weight[node], nid

    def bow_fv(self, f, levelsup):
        """transform(features, v, fv, levelsup) :1121-1189 (TF_IDF, L1) -> BowVector dict, FeatureVector dict."""
        assert self.weighting == 0
        v, fv = {}, {}
        if len(f):
            word, w, nid = self.transform(f, levelsup)
            for i in range(len(f)):
                if w[i] > 0:
                    wi = int(word[i])
                    v[wi] = v[wi] + float(w[i]) if wi in v else float(w[i])     # addWeight
                    fv.setdefault(int(nid[i]), []).append(i)                      # addFeature
        norm = 0.0
        for wi in sorted(v):                                           # BowVector::normalize(L1) over the std::map
            norm += abs(v[wi])
        if norm > 0.0:
            for wi in v:
                v[wi] /= norm
        return v, fv


def l1_score(a, b):
    """L1Scoring::score, ScoringObject.cpp:23-68."""
    s = 0.0
    for w in sorted(set(a) & set(b)):
        s += abs(a[w] - b[w]) - abs(a[w]) - abs(b[w])
    return -s / 2.0


def compute_islands(q, max_gap, min_group):
    """computeIslands :891-965. q: [(id, score)] in descending score order -> [(first, last, score, best_entry, best_score)]."""
    if len(q) == 1:
        return [(q[0][0], q[0][0], q[0][1], q[0][0], q[0][1])]
    out = []
    if not q:
        return out
    q = sorted(q, key=lambda r: r[0])
    first = last = q[0][0]
    i_first = i_last = 0
    best_score, best_entry = q[0][1], q[0][0]

    def island():
        s = 0.0
        for i in range(i_first, i_last + 1):                           # calculateIslandScore
            s += q[i][1]
        return (first, last, s, best_entry, best_score)
    for idx in range(1, len(q)):
        e, sc = q[idx]
        if e - last < max_gap:
            last, i_last = e, idx
            if sc > best_score:
                best_score, best_entry = sc, e
        else:
            if last - first + 1 >= min_group:
                out.append(island())
            first = last = e
            i_first = i_last = idx
            best_score, best_entry = sc, e
    if last - first + 1 >= min_group:
        out.append(island())
    return out


def best_island(islands):
    """std::max_element with tIsland::operator< (score): the first of the largest."""
    best = islands[0]
    for i in islands[1:]:
        if best[2] < i[2]:
            best = i
    return best


def neighratio(A, iA, B, iB, ratio):
    """getMatches_neighratio :1164-1223 (A = the OLD entry's descriptors)."""
    mA, mB = [], []
    for a in iA:
        bj, d1, d2 = -1, 1e9, 1e9
        for j, b in enumerate(iB):
            d = float(ham(A[a], B[b]))
            if d < d1:
                bj, d2, d1 = j, d1, d
            elif d < d2:
                d2 = d
        if d2 != 0.0 and d1 / d2 <= ratio:                             # (0 / 0 is NaN in C++: `<=` is false)
            ib = iB[bj]
            if ib not in mB:
                mB.append(ib), mA.append(a)
            else:
                p = mB.index(ib)
                if d1 < float(ham(A[mA[p]], B[ib])):
                    mA[p] = a
    return mA, mB


def temporal_fit(a1, a2, b1, b2, max_dist):
    """updateTemporalWindow :995-1008."""
    fit = (b1 <= a1 <= b2) or (a1 <= b1 <= a2)
    if not fit:
        fit = max(a1 - b2, b1 - a2) <= max_dist
    return fit


class Detector:
    """TemplatedLoopDetector with Parameters(height, width) + set(1) unless overridden."""

    def __init__(self, voc, **over):
        self.voc = voc
        self.P = dict(use_nss=1, k=1, geom_check=1, di_levels=2, dislocal=20, max_db_results=50, min_matches_per_group=1,
                      max_intragroup_gap=3, max_distance_between_groups=3, max_distance_between_queries=2, min_Fpoints=12,
                      max_neighbor_ratio=0.6, min_inliers=20)
        self.P.update(over)
        self.cfg = abi.default_config(f_threshold=1.0, f_confidence=0.99)
        self.db, self.fv, self.descs, self.keys = [], [], [], []
        self.last_bow, self.win_n, self.win_island, self.win_q = {}, 0, None, -1

    def size(self):
        return len(self.db)

    def clear(self):
        self.db, self.fv, self.descs, self.keys = [], [], [], []
        self.win_n = 0

    def erase(self, entries):
        for e in entries:                                              # delete_entry, TemplatedDatabase.h:476-499
            self.db[e], self.fv[e] = {}, {}

    def detect(self, keys, desc):
        P = self.P
        f = as_bytes(desc)
        keys = np.asarray(keys, np.float32).reshape(-1, 2)
        eid = len(self.db)
        bv, fv = self.voc.bow_fv(f, P["di_levels"])
        r = dict(status=1, query=eid, match=-1, ns_factor=1.0, n_results=0, n_after_cut=0, island_first=-1, island_last=-1,
                 island_best_entry=-1, island_score=0.0, island_best_score=0.0, consistent_entries=0, n_di_matches=0, n_inliers=0)
        cur_pts = old_pts = np.zeros((0, 2), np.float32)
        if eid > P["dislocal"]:
            r["status"], cur_pts, old_pts = self._decide(r, eid, bv, fv, f, keys)
        r["consistent_entries"] = self.win_n
        self.db.append(bv), self.fv.append(fv), self.descs.append(f), self.keys.append(keys)
        if P["use_nss"] and eid + 1 > P["dislocal"]:
            self.last_bow = bv
        return r, cur_pts, old_pts

    def _decide(self, r, eid, bv, fv, f, keys):
        P, none = self.P, np.zeros((0, 2), np.float32)
        max_id = eid - P["dislocal"]
        q = [(e, l1_score(bv, self.db[e])) for e in range(min(max_id, len(self.db))) if set(bv) & set(self.db[e])]
        q.sort(key=lambda t: (-t[1], t[0]))
        if P["max_db_results"] > 0:
            q = q[:P["max_db_results"]]
        r["n_results"] = len(q)
        if not q:
            return 2, none, none
        if P["use_nss"]:
            r["ns_factor"] = l1_score(bv, self.last_bow)
            if not r["ns_factor"] >= MIN_NSS:
                return 3, none, none
        thr = ALPHA * r["ns_factor"]
        cut = len(q)
        for i, t in enumerate(q):                                      # removeLowScores: lower_bound with Result::geq
            if not t[1] >= thr:
                cut = i
                break
        q = q[:cut]
        r["n_after_cut"] = len(q)
        if not q:
            return 4, none, none
        r["match"] = q[0][0]
        islands = compute_islands(q, P["max_intragroup_gap"], P["min_matches_per_group"])
        if not islands:
            return 5, none, none
        isl = best_island(islands)
        if self.win_n == 0 or eid - self.win_q > P["max_distance_between_queries"]:
            self.win_n = 1
        else:
            fit = temporal_fit(self.win_island[0], self.win_island[1], isl[0], isl[1], P["max_distance_between_groups"])
            self.win_n = self.win_n + 1 if fit else 1
        self.win_island, self.win_q = isl, eid
        r["island_first"], r["island_last"], r["island_score"], r["island_best_entry"], r["island_best_score"] = isl
        r["match"] = isl[3]
        if not self.win_n > P["k"]:
            return 6, none, none
        if P["geom_check"] == 3:
            return 0, none, none
        old = isl[3]                                                   # isGeometricallyConsistent_DI :1056-1144
        i_old, i_cur = [], []
        for node in sorted(set(self.fv[old]) & set(fv)):
            a, b = neighratio(self.descs[old], self.fv[old][node], f, fv[node], P["max_neighbor_ratio"])
            i_old += a
            i_cur += b
        r["n_di_matches"] = len(i_old)
        if len(i_old) >= P["min_Fpoints"] and len(i_old) >= 8:         # checkFoundamental :1031-1053
            po, pc = self.keys[old][i_old], keys[i_cur]
            mask = H.oracle_ransac(self.cfg, po, pc)                   # findFundamentalMat(old, cur, FM_RANSAC, 1.0, 0.99)
            r["n_inliers"] = int(mask.sum())
            if r["n_inliers"] > P["min_inliers"]:
                return 0, pc[mask != 0], po[mask != 0]
        return 7, none, none


# ---- the synthetic sessions --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vocabulary(seed):
    blob, desc = make_vocabulary(VK, VL, seed)
    return blob, desc, Voc(blob)


class World:
    """Landmarks near leaves of the vocabulary with fixed 3D points; place p sees landmarks [step p, step p + see) plus
    `distract` unrepeatable distractors, from a pinhole camera that moves along x (depths spread over 4..12 m). Lap 1 is
    displaced sideways and rotated a little against lap 0, so the two views of a place differ by a real epipolar
    geometry; pixel noise <= 0.3 px keeps true pairs inside RANSAC's 1 px."""

    def __init__(self, voc_seed, seed, step=60, see=200, distract=60, n_places=200):
        self.rng = np.random.default_rng(seed)
        self.desc = vocabulary(voc_seed)[1]
        self.step, self.see, self.distract = step, see, distract
        n_inner = sum(VK ** l for l in range(VL))
        self.leaves = np.arange(n_inner, n_inner + VK ** VL)
        n_lm = n_places * step + see
        self.lmk = np.array([self.flip(self.desc[int(self.rng.choice(self.leaves))], 10) for _ in range(n_lm)], np.uint64)
        r = self.rng
        self.xyz = np.stack([np.arange(n_lm) / step + r.uniform(-0.2, 0.2, n_lm), r.uniform(-1, 1, n_lm), r.uniform(4, 12, n_lm)], 1)

    def flip(self, d, n):
        d = d.copy()
        for b in self.rng.integers(0, 256, n):
            d[b >> 6] ^= np.uint64(1) << np.uint64(b & 63)
        return d

    def project(self, ids, p, lap):
        t = np.array([p + self.see / (2.0 * self.step), 0.0, 0.0])
        R = np.eye(3)
        if lap:
            t = t + np.array([0.35, 0.06, 0.15])
            cy, sy, cz, sz = np.cos(0.04), np.sin(0.04), np.cos(0.02), np.sin(0.02)
            R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        pc = (self.xyz[ids] - t) @ R                                   # R^T (P - t)
        uv = 460.0 * pc[:, :2] / pc[:, 2:3] + np.array([320.0, 240.0])
        return uv + self.rng.uniform(-0.3, 0.3, uv.shape)

    def observe(self, p, lap=0, blank=False):
        ids = [] if blank else list(range(p * self.step, p * self.step + self.see))
        f = [self.flip(self.lmk[i], 4) for i in ids]
        uv = self.project(np.array(ids, np.int64), p, lap) if ids else np.zeros((0, 2))
        nd = self.distract if not blank else self.see + self.distract
        f += [self.flip(self.desc[int(self.rng.choice(self.leaves))], 10) for _ in range(nd)]
        uv = np.concatenate([uv, self.rng.uniform([0, 0], [640, 480], (nd, 2))])
        perm = self.rng.permutation(len(f))
        return uv[perm].astype(np.float32), np.array(f, np.uint64)[perm]

    def mixed(self, a, b, lap):
        (ka, fa), (kb, fb) = self.observe(a, lap), self.observe(b, lap)
        h = (self.see + self.distract) // 2
        return np.concatenate([ka[:h], kb[:h]]), np.concatenate([fa[:h], fb[:h]])


EMPTY = (np.zeros((0, 2), np.float32), np.zeros((0, 4), np.uint64))
VOC_SEED = 5


@functools.lru_cache(maxsize=None)
def scenario(which):
    """-> (frames [(keys, desc)], detector parameters overridden)."""
    w = World(VOC_SEED, 100 + which)
    if which == 1:      # two laps: places 0..59, three distractor frames, places 5..17, one distractor frame, places 18..30
        fr = [w.observe(p) for p in range(60)] + [w.observe(0, blank=True) for _ in range(3)]
        fr += [w.observe(p, 1) for p in range(5, 18)] + [w.observe(0, blank=True)] + [w.observe(p, 1) for p in range(18, 31)]
        return fr, {}
    if which == 2:      # an empty keyframe in the second lap
        fr = [w.observe(p) for p in range(40)] + [w.observe(5, 1), w.observe(6, 1), EMPTY] + [w.observe(p, 1) for p in (7, 8, 9)]
        return fr, {}
    if which == 3:      # groups: no overlap between neighbours, then half of place 0 + half of place 40
        fr = [w.observe(p) for p in range(0, 180, 4)] + [w.mixed(0, 40, 1) for _ in range(3)]
        return fr, dict(min_matches_per_group=2)
    raise ValueError(which)


ERASED = list(range(5, 18))


@functools.lru_cache(maxsize=None)
def restated(which, erase=False):
    frames, over = scenario(which)
    det = Detector(vocabulary(VOC_SEED)[2], **over)
    out = []
    for i, (k, d) in enumerate(frames):
        if erase and i == 60:
            det.erase(ERASED), det.erase([9])
        out.append(det.detect(k, d))
    return out, det.size()


def same(got, want, where):
    rg, cg, og = got
    rw, cw, ow = want
    for f in rw:
        if isinstance(rw[f], float):
            assert struct.pack("<d", rg[f]) == struct.pack("<d", rw[f]), (where, f, rg[f], rw[f], rg, rw)
        else:
            assert rg[f] == rw[f], (where, f, rg, rw)
    assert cg.dtype == cw.dtype == np.float32 and np.array_equal(cg, cw) and np.array_equal(og, ow), (where, rg)


# ---- CPU: the restatement against hand-worked cases; the interface without a device ----------------------------------------
def test_islands_hand_worked():
    # one result: its island, whatever min_matches_per_group says (:896-901)
    assert compute_islands([(7, 0.25)], 3, 5) == [(7, 7, 0.25, 7, 0.25)]
    # a gap exactly equal to max_intragroup_gap splits (`id - last < gap`): 5, 8 with gap 3 -> two islands
    assert compute_islands([(8, 0.5), (5, 0.25)], 3, 1) == [(5, 5, 0.25, 5, 0.25), (8, 8, 0.5, 8, 0.5)]
    assert compute_islands([(7, 0.5), (5, 0.25)], 3, 1) == [(5, 7, 0.75, 7, 0.5)]
    # length test: islands 5..6 (length 2) and 20 (length 1) with min_matches_per_group 2
    assert compute_islands([(20, 0.9), (6, 0.5), (5, 0.5)], 3, 2) == [(5, 6, 1.0, 5, 0.5)]   # best entry: first strictly larger
    assert compute_islands([(20, 0.9), (30, 0.5)], 3, 2) == []
    # the score is summed in ascending id order
    q = [(3, 0.1), (1, 1e16), (2, -1e16)]
    assert compute_islands(sorted(q, key=lambda r: -r[1]), 3, 1)[0][2] == (1e16 + -1e16) + 0.1
    # two islands of equal score: the first one wins
    isl = compute_islands([(1, 0.5), (10, 0.5)], 3, 1)
    assert best_island(isl) == (1, 1, 0.5, 1, 0.5)
    assert best_island([(1, 1, 0.5, 1, 0.5), (10, 10, 0.75, 10, 0.75), (20, 20, 0.75, 20, 0.75)])[0] == 10


def test_temporal_window_hand_worked():
    assert temporal_fit(10, 12, 11, 15, 3) and temporal_fit(10, 12, 5, 10, 3)     # overlap either way
    assert temporal_fit(10, 12, 15, 16, 3) and not temporal_fit(10, 12, 16, 17, 3)  # gap 3 fits, 4 does not
    assert temporal_fit(10, 12, 5, 7, 3) and not temporal_fit(10, 12, 4, 6, 3)


def test_neighratio_hand_worked():
    def d(*bits):
        v = np.zeros(32, np.uint8)
        for b in bits:
            v[b >> 3] |= 1 << (b & 7)
        return v
    far = d(*range(100, 200))
    # claim replacement: old 0 and old 2 both pick cur 1; old 2 is strictly closer and takes old 0's POSITION in the list
    A = [d(0, 1), d(50, 51, 52), d(0)]
    B = [d(50, 51, 52, 53), d(), far]
    assert neighratio(A, [0, 1, 2], B, [0, 1, 2], 0.6) == ([2, 1], [1, 0])
    # an equal distance does not replace (`best_dist_1 < d`)
    assert neighratio([d(0, 1), d(2, 3)], [0, 1], [d(), far], [0, 1], 0.6) == ([0], [0])
    # ties between candidates keep the first (`d < best_dist_1`), and the tie makes d1 / d2 = 1 > ratio: no match
    assert neighratio([d(0)], [0], [d(), d(0, 1)], [0, 1], 0.6) == ([], [])
    # 0 / 0: two exact copies -> NaN, no match; one exact copy and one far -> 0 / d2 = 0 matches
    assert neighratio([d(5)], [0], [d(5), d(5)], [0, 1], 0.6) == ([], [])
    assert neighratio([d(5)], [0], [d(5), far], [0, 1], 0.6) == ([0], [0])
    # one candidate alone: d / 1e9 matches
    assert neighratio([d(5)], [0], [far], [0], 0.6) == ([0], [0])
    # the outer loop runs over the first (old) list: the second output follows its order
    assert neighratio([d(9), d(5)], [0, 1], [d(5), far, d(9)], [0, 1, 2], 0.6) == ([0, 1], [2, 0])


def test_restated_transform_matches_oracle():
    blob, _, voc = vocabulary(VOC_SEED)
    ov = OracleVoc(blob)
    frames, _ = scenario(2)
    for k, dsc in frames[:3] + [frames[42]]:
        w, ww = ov.transform(dsc) if len(dsc) else (np.zeros(0, np.int32), np.zeros(0))
        rw, rww, nid = voc.transform(as_bytes(dsc), 2) if len(dsc) else (w, ww, w)
        assert np.array_equal(w, rw) and np.array_equal(ww, rww)
        bw, bv = ov.bow(dsc)
        v, fv = voc.bow_fv(as_bytes(dsc), 2)
        assert list(bw) == sorted(v) and [struct.pack("<d", x) for x in bv] == [struct.pack("<d", v[i]) for i in sorted(v)]
        # FeatureVector: every kept feature once, under its ancestor at level L - 2 (breadth-first ids: parent = (n - 1) // k)
        n_inner = sum(VK ** l for l in range(VL))
        leaf = {int(voc.word[n]): n for n in range(n_inner, n_inner + VK ** VL)}
        for node, idx in fv.items():
            assert idx == sorted(idx)
            for i in idx:
                n = leaf[int(w[i])]
                assert ((n - 1) // VK - 1) // VK == node and ww[i] > 0
        assert sum(len(i) for i in fv.values()) == int((ww > 0).sum())
    v0, fv0 = voc.bow_fv(as_bytes(frames[0][1]), VL)                  # di_levels = L: everything under the root
    assert list(fv0) == [0]


def test_scenarios_reach_every_status():
    """The condition on the inputs: over scenarios 1-3 every DetectionStatus occurs, with at least 20 LOOP_DETECTED in 1."""
    hist = [collections.Counter(STATUS[r["status"]] for r, _, _ in restated(s)[0]) for s in (1, 2, 3)]
    print(hist)
    assert hist[0]["LOOP_DETECTED"] >= 20
    assert set(hist[0]) | set(hist[1]) | set(hist[2]) == set(STATUS)
    assert "NO_DB_RESULTS" in hist[1] and "LOW_NSS_FACTOR" in hist[1] and "NO_GROUPS" in hist[2]
    det = [(r, c, o) for r, c, o in restated(1)[0] if r["status"] == 0]
    assert all(len(c) == len(o) == r["n_inliers"] > 20 and r["n_di_matches"] >= 12 for r, c, o in det)
    # erasing the first lap's entries 5..17 changes the second lap
    assert [r["status"] for r, _, _ in restated(1, True)[0]] != [r["status"] for r, _, _ in restated(1)[0]]
    assert restated(1, True)[1] == restated(1)[1] == len(scenario(1)[0])


def test_symbols_and_default_parameters():
    lib = loop.bind_loop_detector(abi.load_product())
    for s in ("params_default", "create", "destroy", "get_device", "detect", "erase", "clear", "size", "kernel_ms"):
        assert hasattr(lib, "vio_loop_detector_" + s), s
    p = loop.loop_detector_params(1.0)
    want = dict(use_nss=1, k=1, geom_check=1, di_levels=2, dislocal=20, max_db_results=50, min_matches_per_group=1,
                max_intragroup_gap=3, max_distance_between_groups=3, max_distance_between_queries=2, min_Fpoints=12,
                max_neighbor_ratio=0.6, f_threshold=1.0, f_confidence=0.99, min_inliers=20)
    assert {k: getattr(p, k) for k in want} == want
    assert p.alpha == float(np.float32(0.3)) and p.min_nss_factor == float(np.float32(0.005))
    p2 = loop.loop_detector_params(2.0)
    want.update(dislocal=40, max_db_results=100, min_matches_per_group=2, max_intragroup_gap=6, max_distance_between_groups=6,
                max_distance_between_queries=4)
    assert {k: getattr(p2, k) for k in want} == want and p2.alpha == p.alpha and p2.min_nss_factor == p.min_nss_factor
    p15 = loop.loop_detector_params(1.5)                               # products truncated to int
    assert (p15.dislocal, p15.max_db_results, p15.min_matches_per_group, p15.max_intragroup_gap) == (30, 75, 1, 4)


def test_create_refuses_without_device(tmp_path):
    script = tmp_path / "nodev.py"
    script.write_text(textwrap.dedent("""
        import ctypes as C, importlib, sys
        sys.path.insert(0, %r)
        pkg = importlib.import_module("vins-mobile_amd")
        lib = pkg.loop.bind_loop_detector(pkg.abi.load_product())
        p = pkg.loop.loop_detector_params()
        h = C.c_void_p()
        rc = lib.vio_loop_detector_create(None, C.byref(p), 4, 64, 512, C.byref(h))
        assert rc == pkg.abi.VIO_ENODEV and not h.value, rc
        print("refused")
    """ % H.ROOT))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dvoc():
    v = loop.BowVocabulary(vocabulary(VOC_SEED)[0])
    yield v
    v.close()


def run_product(dvoc, which, erase=False):
    frames, over = scenario(which)
    det = loop.LoopDetector(dvoc, loop.loop_detector_params(1.0, **over), n_sessions=1, max_entries=len(frames), max_keypoints=512)
    try:
        out = []
        for i, (k, d) in enumerate(frames):
            if erase and i == 60:
                det.erase(0, ERASED), det.erase(0, [9])
            out.append(det.detect([0], [k], [d])[0])
            assert det.kernel_ms() > 0.0
        return out, det.size(0)
    finally:
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", [1, 2, 3])
def test_sessions_match_restatement(dvoc, which):
    got, size = run_product(dvoc, which)
    want, wsize = restated(which)
    print(collections.Counter(STATUS[r["status"]] for r, _, _ in got))
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, (which, i))
    assert size == wsize == len(got)
    if which == 1:
        assert sum(r["status"] == 0 for r, _, _ in got) >= 20


@pytest.mark.gpu
def test_erase_matches_restatement(dvoc):
    got, size = run_product(dvoc, 1, erase=True)
    want, wsize = restated(1, True)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, ("erase", i))
    assert size == wsize == len(got)                                   # ids are not reused, size keeps counting
    plain = restated(1)[0]
    assert [r["status"] for r, _, _ in got] != [r["status"] for r, _, _ in plain]
    assert not any(r["match"] in ERASED for r, _, _ in got[60:])       # an erased entry is no query result any more


def small_session(sid):
    """Session `sid` of the batch test: its own world (seed 42 + sid) over the shared vocabulary, a first lap of its own
    length and a second lap that revisits part of it."""
    w = World(VOC_SEED, 42 + sid, step=24, see=80, distract=20, n_places=40)
    n1, a, n2 = 24 + sid % 5, sid % 4, 4 + sid % 7
    return [w.observe(p) for p in range(n1)] + [w.observe(p, 1) for p in range(a, a + n2)]


@pytest.mark.gpu
def test_batch_equals_independent_detectors(dvoc):
    n_ses = 64
    routes = [small_session(s) for s in range(n_ses)]
    P = loop.loop_detector_params()
    alone = []
    for s in range(n_ses):
        det = loop.LoopDetector(dvoc, P, n_sessions=1, max_entries=40, max_keypoints=128)
        alone.append([det.detect([0], [k], [d])[0] for k, d in routes[s]])
        det.close()
    det = loop.LoopDetector(dvoc, P, n_sessions=n_ses, max_entries=40, max_keypoints=128)
    try:
        nxt, call, batched = [0] * n_ses, 0, [[] for _ in range(n_ses)]
        while any(nxt[s] < len(routes[s]) for s in range(n_ses)):
            ses = [s for s in range(n_ses) if nxt[s] < len(routes[s]) and (call + s) % 5 != 0]   # some sit a call out
            ses = ses[::-1] if call % 2 else ses                                                   # in any order
            call += 1
            if not ses:
                continue
            res = det.detect(ses, [routes[s][nxt[s]][0] for s in ses], [routes[s][nxt[s]][1] for s in ses])
            for s, r in zip(ses, res):
                batched[s].append(r)
                nxt[s] += 1
        for s in range(n_ses):
            assert len(batched[s]) == len(alone[s]) == det.size(s)
            for i, (g, w) in enumerate(zip(batched[s], alone[s])):
                same(g, w, (s, i))
        hist = collections.Counter(STATUS[r["status"]] for s in range(n_ses) for r, _, _ in batched[s])
        print(hist)
        assert hist["LOOP_DETECTED"] > 0 and hist["CLOSE_MATCHES_ONLY"] == 21 * n_ses
    finally:
        det.close()


@pytest.mark.gpu
def test_refusals_and_clear(dvoc):
    frames, _ = scenario(2)
    with pytest.raises(loop.LoopDetectorError) as e:
        loop.LoopDetector(dvoc, loop.loop_detector_params(geom_check=2))
    assert e.value.rc == abi.VIO_EINVAL
    for bad in (dict(geom_check=0), dict(di_levels=VL + 1), dict(di_levels=-1)):
        with pytest.raises(loop.LoopDetectorError) as e:
            loop.LoopDetector(dvoc, loop.loop_detector_params(**bad))
        assert e.value.rc == abi.VIO_EINVAL
    det = loop.LoopDetector(dvoc, None, n_sessions=2, max_entries=len(frames), max_keypoints=300)
    try:
        dev = np.zeros(1, np.int32)
        dvoc.lib.vio_vocabulary_get_device(dvoc._h, dev.ctypes.data_as(C.POINTER(C.c_int32)))
        assert det.device() == int(dev[0])                             # bound to the vocabulary's device
        (k, d), (k1, d1) = frames[0], frames[1]
        with pytest.raises(loop.LoopDetectorError) as e:
            det.detect([1, 1], [k, k1], [d, d1])                       # a session twice in one call
        assert e.value.rc == abi.VIO_EINVAL
        with pytest.raises(loop.LoopDetectorError) as e:               # too many keypoints, next to a keyframe that would fit
            det.detect([0, 1], [k, np.concatenate([k, k])], [d, np.concatenate([d, d])])
        assert e.value.rc == abi.VIO_ECAP
        with pytest.raises(loop.LoopDetectorError) as e:
            det.erase(0, [0])                                          # no such entry
        assert e.value.rc == abi.VIO_EINVAL
        assert det.size(0) == det.size(1) == 0                         # nothing half-applied
        # session 1 runs part of the route, is cleared, and then gives what a fresh detector gives
        for k, d in frames[:30]:
            det.detect([1], [k], [d])
        assert det.size(1) == 30 and det.size(0) == 0
        det.clear(1)
        assert det.size(1) == 0
        want, _ = restated(2)
        for i, (k, d) in enumerate(frames):
            same(det.detect([1], [k], [d])[0], want[i], ("after clear", i))
        with pytest.raises(loop.LoopDetectorError) as e:               # the session is full
            det.detect([1], [k], [d])
        assert e.value.rc == abi.VIO_ECAP and det.size(1) == len(frames)
    finally:
        det.close()
