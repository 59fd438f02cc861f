"""numpy model of vio_vocabulary_train, written from the text of include/vio_amd.h (not from the kernels): the reference's
recursion (HKmeansStep, node after node, depth first), k-means++ with the header's random stream, the iteration cap,
creation-order ids, words over the leaves, Ni through the ordinary descent, math.log for the weights, the file layout of
loop/VocabularyBinary.hpp. Test infrastructure only."""
import math
import struct

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
DEFAULT_ITERATIONS = 128


def mix(x):
    x = (x + GOLDEN) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def child_key(key, c):
    return mix(key ^ (c + 1))


def draw(key, j):
    return mix((key + j * GOLDEN) & M64)


def first_centre(key, n):
    return min(n - 1, int(math.floor(((draw(key, 0) >> 11) * 2.0 ** -53) * float(n))))


def cut_of(key, m, total):
    return (((draw(key, m) >> 11) + 1) * 2.0 ** -53) * float(total)


def to_bits(desc):
    """uint64 [n][4] -> uint8 [n][256], bit i = word i >> 6, bit i & 63"""
    d = np.ascontiguousarray(desc, "<u8").reshape(-1, 4)
    return np.unpackbits(d.view(np.uint8).reshape(-1, 32), axis=1, bitorder="little")


def from_bits(bits):
    return np.packbits(np.asarray(bits, np.uint8).reshape(-1, 256), axis=1, bitorder="little").view("<u8").reshape(-1, 4)


def distances(bits, centres):
    """Hamming distances [n][c] (int64)"""
    b, c = bits.astype(np.int32), centres.astype(np.int32)
    return (b.sum(1)[:, None] + c.sum(1)[None, :] - 2 * (b @ c.T)).astype(np.int64)


def nearest(bits, centres):
    return np.argmin(distances(bits, centres), axis=1)   # the FIRST minimum


def mean_value(bits):
    """FBrief::meanValue: bit set iff more than floor(N / 2) members have it; an empty group gives zeros"""
    if len(bits) == 0:
        return np.zeros(256, np.uint8)
    return (bits.sum(0, dtype=np.int64) > len(bits) // 2).astype(np.uint8)


class Model:
    def __init__(self, desc_list, k, L, weighting=0, max_iterations=DEFAULT_ITERATIONS, seed=0):
        self.k, self.L, self.weighting, self.max_iterations, self.seed = k, L, weighting, max_iterations, seed
        self.desc_list = [np.asarray(d, np.uint64).reshape(-1, 4) for d in desc_list]
        self.desc = np.concatenate(self.desc_list + [np.zeros((0, 4), np.uint64)])
        self.image = np.concatenate([np.full(len(d), g, np.int64) for g, d in enumerate(self.desc_list)] + [np.zeros(0, np.int64)])
        self.bits = to_bits(self.desc)
        n = len(self.desc)
        assert n > 0
        # node id -> record; ids are handed out in creation order
        self.parent, self.level, self.node_bits, self.members, self.children = [0], [0], [np.zeros(256, np.uint8)], [np.arange(n)], [[]]
        self.runs = {}     # node id -> dict(seeds, iterations, capped, members) of every node that ran k-means
        self.capped_nodes = self.empty_clusters = self.short_nodes = 0
        self.iterations_max = [0] * 16
        self._step(0, np.arange(n), 1, mix(seed))
        self.n_nodes = len(self.parent) - 1
        self.word_node = [i for i in range(1, len(self.parent)) if not self.children[i]]
        self.node_word = {nid: w for w, nid in enumerate(self.word_node)}
        self.n_words = len(self.word_node)
        self.training_leaf = np.zeros(n, np.int64)    # word of the leaf whose group holds the descriptor
        for w, nid in enumerate(self.word_node):
            self.training_leaf[self.members[nid]] = w
        self.words = self.transform(self.bits)
        self.n_docs = len(self.desc_list)
        self.ni = np.zeros(self.n_words, np.int64)
        for g in range(self.n_docs):
            self.ni[np.unique(self.words[self.image == g])] += 1
        if weighting in (1, 3):
            self.word_weight = [1.0] * self.n_words
        else:
            self.word_weight = [math.log(self.n_docs / int(c)) if c > 0 else 0.0 for c in self.ni]

    def _step(self, parent, members, level, key):
        k, n = self.k, len(members)
        if n == 0:
            return
        bits = self.bits[members]
        if n <= k:
            centres, assoc = bits.copy(), np.arange(n)
        else:
            seeds = [first_centre(key, n)]
            md = distances(bits, bits[seeds[-1:]])[:, 0]
            while len(seeds) < k:
                total = int(md.sum())
                if total == 0:
                    break
                cut = cut_of(key, len(seeds), total)
                seeds.append(int(np.argmax(np.cumsum(md).astype(np.float64) >= cut)))
                md = np.minimum(md, distances(bits, bits[seeds[-1:]])[:, 0])
            centres = bits[seeds].copy()
            assoc = nearest(bits, centres)
            passes, capped = 0, True
            while passes < self.max_iterations:
                centres = np.array([mean_value(bits[assoc == c]) for c in range(len(seeds))])
                passes += 1
                new = nearest(bits, centres)
                same = np.array_equal(new, assoc)
                assoc = new
                if same:
                    capped = False
                    break
            self.runs[parent] = dict(seeds=seeds, iterations=passes, capped=capped, members=members, key=key)
            self.capped_nodes += capped
            self.short_nodes += len(seeds) < k
            self.iterations_max[level - 1] = max(self.iterations_max[level - 1], passes)
            self.empty_clusters += sum(int((assoc == c).sum() == 0) for c in range(len(seeds)))
        first = len(self.parent)
        for c in range(len(centres)):
            self.parent.append(parent), self.level.append(level), self.node_bits.append(centres[c]), self.children.append([])
            self.members.append(members[assoc == c])
            self.children[parent].append(first + c)
        if level < self.L:
            for c in range(len(centres)):
                if len(self.members[first + c]) > 1:
                    self._step(first + c, self.members[first + c], level + 1, child_key(key, c))

    def transform(self, bits):
        """the ordinary descent: word id of every descriptor"""
        out = np.zeros(len(bits), np.int64)
        todo = [(0, np.arange(len(bits)))]
        while todo:
            node, sel = todo.pop()
            if len(sel) == 0:
                continue
            ch = self.children[node]
            if not ch:
                out[sel] = self.node_word[node]
                continue
            pick = nearest(bits[sel], np.array([self.node_bits[c] for c in ch]))
            for j, c in enumerate(ch):
                todo.append((c, sel[pick == j]))
        return out

    def blob(self):
        nn = self.n_nodes
        rec = np.zeros(nn, dtype=[("id", "<i4"), ("pid", "<i4"), ("w", "<f8"), ("d", "<u8", 4)])
        rec["id"] = np.arange(1, nn + 1)
        rec["pid"] = self.parent[1:]
        rec["d"] = from_bits(np.array(self.node_bits[1:]))
        for w, nid in enumerate(self.word_node):
            rec["w"][nid - 1] = self.word_weight[w]
        words = np.zeros(self.n_words, dtype=[("nid", "<i4"), ("wid", "<i4")])
        words["nid"], words["wid"] = self.word_node, np.arange(self.n_words)
        return struct.pack("<6i", self.k, self.L, 0, self.weighting, nn, self.n_words) + rec.tobytes() + words.tobytes()

    def stats(self):
        return dict(n_nodes=self.n_nodes, n_words=self.n_words, capped_nodes=self.capped_nodes, empty_clusters=self.empty_clusters,
                    short_nodes=self.short_nodes, iterations_max=list(self.iterations_max))


def parse_blob(blob):
    """-> (header tuple, node records, word records) as numpy structured arrays"""
    hdr = struct.unpack("<6i", blob[:24])
    nodes = np.frombuffer(blob, dtype=[("id", "<i4"), ("pid", "<i4"), ("w", "<f8"), ("d", "<u8", 4)], count=hdr[4], offset=24)
    words = np.frombuffer(blob, dtype=[("nid", "<i4"), ("wid", "<i4")], count=hdr[5], offset=24 + 48 * hdr[4])
    return hdr, nodes, words
