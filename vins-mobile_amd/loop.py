"""Host-side mirror of the loop-closure producer's descriptor side: KeyFrame::searchByDes / findConnectionWithOldFrame
(VINS_ios/loop/keyframe.cpp:161-187, 267-273), descriptor extraction, the bag-of-words query and the loop detector
(TemplatedLoopDetector::detectLoop). Plumbing over csrc/vio_loop.hip, vio_brief.hip, vio_bow.hip and vio_loop_detector.hip for
tests and tools; no compute here."""
import ctypes as C

import numpy as np

from . import abi

_u64p, _i32p, _fp, _u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_uint8)


def bind(lib, prefix="vio"):
    if prefix == "vio":
        lib.vio_matcher_create.argtypes = [C.POINTER(C.c_void_p)]
        lib.vio_matcher_destroy.argtypes = [C.c_void_p]
        lib.vio_matcher_search_by_des.argtypes = [C.c_void_p, C.c_int32, _i32p, _i32p, _u64p, _u64p, _i32p, _i32p]
        lib.vio_loop_find_connection.argtypes = [C.c_void_p, C.POINTER(abi.VioConfig), C.c_int32, _u64p, _fp, C.c_int32, _u64p,
                                                 _fp, _fp, _fp, _u8p, _i32p]
    return lib


class Matcher:
    def __init__(self):
        self.lib = bind(abi.load_product())
        self._h = C.c_void_p()
        rc = self.lib.vio_matcher_create(C.byref(self._h))
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_matcher_create failed rc=%d (a gfx950 device is required)" % rc)

    def close(self):
        if self._h:
            self.lib.vio_matcher_destroy(self._h)
            self._h = C.c_void_p()

    def search_by_des(self, cur_list, old_list):
        """cur_list / old_list: per pair uint64 arrays [n][4]. Returns per pair (best_index, best_dist)."""
        n_cur = np.array([len(c) for c in cur_list], np.int32)
        n_old = np.array([len(o) for o in old_list], np.int32)
        cur = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint64).reshape(-1, 4) for c in cur_list] + [np.zeros((0, 4), np.uint64)]))
        old = np.ascontiguousarray(np.concatenate([np.asarray(o, np.uint64).reshape(-1, 4) for o in old_list] + [np.zeros((0, 4), np.uint64)]))
        idx = np.zeros(max(1, int(n_cur.sum())), np.int32)
        dist = np.zeros_like(idx)
        rc = self.lib.vio_matcher_search_by_des(self._h, len(cur_list), n_cur.ctypes.data_as(_i32p), n_old.ctypes.data_as(_i32p),
                                                cur.ctypes.data_as(_u64p), old.ctypes.data_as(_u64p), idx.ctypes.data_as(_i32p),
                                                dist.ctypes.data_as(_i32p))
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_matcher_search_by_des failed rc=%d" % rc)
        out, o = [], 0
        for n in n_cur:
            out.append((idx[o:o + n].copy(), dist[o:o + n].copy()))
            o += n
        return out

    def find_connection(self, cfg, cur_desc, cur_pts, old_desc, old_pts):
        cur_desc = np.ascontiguousarray(cur_desc, np.uint64).reshape(-1, 4)
        old_desc = np.ascontiguousarray(old_desc, np.uint64).reshape(-1, 4)
        cur_pts = np.ascontiguousarray(cur_pts, np.float32).reshape(-1, 2)
        old_pts = np.ascontiguousarray(old_pts, np.float32).reshape(-1, 2)
        n = len(cur_desc)
        mo, mn = np.zeros((max(n, 1), 2), np.float32), np.zeros((max(n, 1), 2), np.float32)
        status, k = np.zeros(max(n, 1), np.uint8), C.c_int32()
        rc = self.lib.vio_loop_find_connection(self._h, C.byref(cfg), n, cur_desc.ctypes.data_as(_u64p), cur_pts.ctypes.data_as(_fp),
                                               len(old_desc), old_desc.ctypes.data_as(_u64p), old_pts.ctypes.data_as(_fp),
                                               mo.ctypes.data_as(_fp), mn.ctypes.data_as(_fp), status.ctypes.data_as(_u8p), C.byref(k))
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_loop_find_connection failed rc=%d" % rc)
        return mo[:n], mn[:n], status[:n], k.value


# ---- keyframe descriptor extraction: BriefExtractor::operator() (loop/keyframe.cpp:375-409) -----------------------------
def bind_brief(lib):
    lib.vio_brief_load_pattern.argtypes = [C.c_char_p, _i32p, _i32p, _i32p, _i32p, C.c_int32, _i32p]
    lib.vio_brief_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _i32p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.vio_brief_destroy.argtypes = [C.c_void_p]
    lib.vio_brief_get_device.argtypes = [C.c_void_p, _i32p]
    lib.vio_brief_extract.argtypes = [C.c_void_p, _u8p, C.c_int32, _fp, _i32p, C.c_int32, C.c_int32, _fp, _u64p, _i32p, _i32p]
    lib.vio_brief_extract_device.argtypes = [C.c_void_p, C.c_void_p, _i32p, C.c_int32, _fp, _i32p, C.c_int32, C.c_int32, _fp, _u64p, _i32p,
                                             _i32p]
    return lib


class DeviceFrames:
    """A caller-owned device buffer of packed frames (what vio_preprocess_run_resident leaves behind): hipMalloc + one
    upload, through the HIP runtime the library is linked against. `.ptr` is what the *_device entries take."""

    def __init__(self, frames):
        frames = np.ascontiguousarray(frames, np.uint8)
        hip = self.hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        p = C.c_void_p()
        if hip.hipMalloc(C.byref(p), max(1, frames.nbytes)) != 0:
            raise RuntimeError("hipMalloc failed")
        self.ptr, self.nbytes = p.value, frames.nbytes
        if frames.nbytes and hip.hipMemcpy(p, frames.ctypes.data, frames.nbytes, 1) != 0:   # hipMemcpyHostToDevice
            self.close()
            raise RuntimeError("hipMemcpy failed")

    def close(self):
        if self.ptr:
            self.hip.hipFree(C.c_void_p(self.ptr))
            self.ptr = None


def _window_arrays(window_pts, n, stride=None):
    """per frame float [k][2] -> (n_window [n], points [n][stride][2], stride)"""
    nw = np.array([len(w) for w in window_pts], np.int32)
    assert len(nw) == n
    if stride is None:
        stride = max(1, int(nw.max()) if n else 1)
    wp = np.zeros((n, stride, 2), np.float32)
    for f, w in enumerate(window_pts):
        if len(w):   # (a given stride below a frame's count is the library's to refuse: n_window says what was asked)
            wp[f, :min(len(w), stride)] = np.asarray(w, np.float32).reshape(-1, 2)[:stride]
    return nw, wp, stride


def load_pattern(path, cap=256):
    """-> (x1, y1, x2, y2) int32 arrays from an OpenCV FileStorage YAML file (Resources/brief_pattern.yml). Host code only."""
    lib = bind_brief(abi.load_product())
    arr = [np.zeros(cap, np.int32) for _ in range(4)]
    n = C.c_int32(0)
    rc = lib.vio_brief_load_pattern(str(path).encode(), *[a.ctypes.data_as(_i32p) for a in arr], cap, C.byref(n))
    if rc != abi.VIO_OK:
        raise RuntimeError("vio_brief_load_pattern failed rc=%d" % rc)
    return tuple(a[:n.value].copy() for a in arr)


class BriefExtractor:
    """FAST corners + window points -> BRIEF descriptors for a batch of keyframes (csrc/vio_brief.hip)."""

    def __init__(self, rows, cols, pattern, max_frames=1, max_keypoints=4096):
        self.lib = bind_brief(abi.load_product())
        self.rows, self.cols, self.max_frames, self.cap = rows, cols, max_frames, max_keypoints
        pat = [np.ascontiguousarray(p, np.int32) for p in pattern]
        self._h = C.c_void_p()
        rc = self.lib.vio_brief_create(rows, cols, max_frames, max_keypoints, *[p.ctypes.data_as(_i32p) for p in pat], len(pat[0]),
                                       C.byref(self._h))
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_brief_create failed rc=%d (a gfx950 device is required)" % rc)

    def close(self):
        if self._h:
            self.lib.vio_brief_destroy(self._h)
            self._h = C.c_void_p()

    def extract(self, frames, window_pts, fast_threshold=20, allow_cut=False):
        """frames: [n][rows][cols] uint8; window_pts: per frame float arrays [k][2]. Returns per frame
        (keypoints [m][2], descriptors [m][4] uint64, n_fast)."""
        frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, self.rows, self.cols)
        n = len(frames)
        nw = np.array([len(w) for w in window_pts], np.int32)
        stride = max(1, int(nw.max()) if n else 1)
        wp = np.zeros((n, stride, 2), np.float32)
        for f, w in enumerate(window_pts):
            if len(w):
                wp[f, :len(w)] = np.asarray(w, np.float32).reshape(-1, 2)
        kp = np.zeros((n, self.cap, 2), np.float32)
        desc = np.zeros((n, self.cap, 4), np.uint64)
        nf, nk = np.zeros(n, np.int32), np.zeros(n, np.int32)
        rc = self.lib.vio_brief_extract(self._h, frames.ctypes.data_as(_u8p), n, wp.ctypes.data_as(_fp), nw.ctypes.data_as(_i32p), stride,
                                        fast_threshold, kp.ctypes.data_as(_fp), desc.ctypes.data_as(_u64p), nf.ctypes.data_as(_i32p),
                                        nk.ctypes.data_as(_i32p))
        if rc != abi.VIO_OK and not (allow_cut and rc == abi.VIO_ECAP):
            raise RuntimeError("vio_brief_extract failed rc=%d" % rc)
        return [(kp[f, :nk[f]].copy(), desc[f, :nk[f]].copy(), int(nf[f])) for f in range(n)]

    def extract_device(self, d_frames, n, window_pts, frame_index=None, fast_threshold=20, counts_only=False):
        """vio_brief_extract_device: d_frames = device pointer (int) of packed frames, frame f = slot frame_index[f].
        -> (rc, per frame (keypoints, descriptors, n_fast)), or (rc, n_fast [n], n_keypoints [n]) with counts_only."""
        nw, wp, stride = _window_arrays(window_pts, n)
        fi = None if frame_index is None else np.ascontiguousarray(frame_index, np.int32)
        kp = None if counts_only else np.zeros((n, self.cap, 2), np.float32)
        desc = None if counts_only else np.zeros((n, self.cap, 4), np.uint64)
        nf, nk = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        rc = self.lib.vio_brief_extract_device(self._h, C.c_void_p(d_frames), None if fi is None else fi.ctypes.data_as(_i32p), n,
                                               wp.ctypes.data_as(_fp), nw.ctypes.data_as(_i32p), stride, fast_threshold,
                                               None if counts_only else kp.ctypes.data_as(_fp),
                                               None if counts_only else desc.ctypes.data_as(_u64p), nf.ctypes.data_as(_i32p),
                                               nk.ctypes.data_as(_i32p))
        if counts_only or rc not in (abi.VIO_OK, abi.VIO_ECAP):
            return rc, nf, nk
        return rc, [(kp[f, :nk[f]].copy(), desc[f, :nk[f]].copy(), int(nf[f])) for f in range(n)]


# ---- bag-of-words query (DBoW2: csrc/vio_bow.hip) ---------------------------------------------------------------------
_f64p = C.POINTER(C.c_double)


def make_vocabulary_blob(k, L, scoring, weighting, nodes, words):
    """Bytes of a vocabulary in the app's binary layout (loop/VocabularyBinary.hpp): nodes = iterable of
    (node_id, parent_id, weight, desc[4] uint64), words = iterable of (node_id, word_id)."""
    import struct
    nodes, words = list(nodes), list(words)
    out = [struct.pack("<6i", k, L, scoring, weighting, len(nodes), len(words))]
    for nid, pid, w, d in nodes:
        out.append(struct.pack("<iid4Q", nid, pid, w, *[int(x) for x in d]))
    for nid, wid in words:
        out.append(struct.pack("<ii", nid, wid))
    return b"".join(out)


class VioVocabularyTrainParams(C.Structure):  # include/vio_amd.h
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("weighting", C.c_int32), ("max_iterations", C.c_int32), ("seed", C.c_uint64)]


class VioVocabularyTrainStats(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("n_descriptors", "n_nodes", "n_words", "capped_nodes", "empty_clusters", "short_nodes", "launches")] + \
               [("iterations_max", C.c_int32 * 16), ("kernel_ms", C.c_double), ("pass_ms", C.c_double * 4)]


def bind_bow(lib):
    vp = C.c_void_p
    lib.vio_vocabulary_train_params_default.argtypes = [C.POINTER(VioVocabularyTrainParams)]
    lib.vio_vocabulary_train_params_default.restype = None
    lib.vio_vocabulary_train.argtypes = [C.POINTER(VioVocabularyTrainParams), C.c_int32, _i32p, _u64p, C.POINTER(vp),
                                         C.POINTER(VioVocabularyTrainStats)]
    lib.vio_vocabulary_serialize.argtypes = [vp, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.vio_vocabulary_save.argtypes = [vp, C.c_char_p]
    lib.vio_vocabulary_create.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(vp)]
    lib.vio_vocabulary_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.vio_vocabulary_destroy.argtypes = [vp]
    lib.vio_vocabulary_destroy.restype = None
    lib.vio_vocabulary_info.argtypes = [vp, _i32p]
    lib.vio_vocabulary_get_device.argtypes = [vp, _i32p]
    lib.vio_vocabulary_transform.argtypes = [vp, C.c_int32, _i32p, _u64p, _i32p, _f64p, _i32p, _i32p, _f64p, C.c_int32]
    lib.vio_bow_database_create.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(vp)]
    lib.vio_bow_database_destroy.argtypes = [vp]
    lib.vio_bow_database_destroy.restype = None
    lib.vio_bow_database_size.argtypes = [vp, _i32p]
    lib.vio_bow_database_add.argtypes = [vp, C.c_int32, _i32p, _f64p, _i32p]
    lib.vio_bow_database_query.argtypes = [vp, C.c_int32, _i32p, _i32p, _f64p, C.c_int32, _i32p, C.c_int32, _i32p, _i32p, _f64p, C.c_int32]
    return lib


class BowVocabulary:
    """TemplatedVocabulary<FBrief> on the device: transform() for batches of keyframes; train() makes one from descriptors
    (TemplatedVocabulary::create), serialize() / save() write the app's file."""

    def __init__(self, blob=None, path=None, _handle=None):
        self.lib = bind_bow(abi.load_product())
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
            return
        rc = self.lib.vio_vocabulary_load(path.encode(), C.byref(self._h)) if path else \
            self.lib.vio_vocabulary_create(blob, len(blob), C.byref(self._h))
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_vocabulary_create failed rc=%d" % rc)

    def close(self):
        if self._h:
            self.lib.vio_vocabulary_destroy(self._h)
            self._h = C.c_void_p()

    @classmethod
    def train(cls, desc_list, k=None, L=None, weighting=None, max_iterations=None, seed=None):
        """vio_vocabulary_train on per image uint64 [n][4] descriptors -> (vocabulary, stats dict). Arguments left None keep
        vio_vocabulary_train_params_default's values."""
        lib = bind_bow(abi.load_product())
        p = VioVocabularyTrainParams()
        lib.vio_vocabulary_train_params_default(C.byref(p))
        for name, val in (("k", k), ("L", L), ("weighting", weighting), ("max_iterations", max_iterations), ("seed", seed)):
            if val is not None:
                setattr(p, name, val)
        n_desc = np.array([len(d) for d in desc_list], np.int32)
        desc = np.ascontiguousarray(np.concatenate([np.asarray(d, np.uint64).reshape(-1, 4) for d in desc_list] + [np.zeros((0, 4), np.uint64)]))
        h, st = C.c_void_p(), VioVocabularyTrainStats()
        rc = lib.vio_vocabulary_train(C.byref(p), len(desc_list), n_desc.ctypes.data_as(_i32p), desc.ctypes.data_as(_u64p), C.byref(h),
                                      C.byref(st))
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_vocabulary_train failed rc=%d" % rc)
        stats = {f: getattr(st, f) for f, _ in VioVocabularyTrainStats._fields_}
        stats["iterations_max"], stats["pass_ms"] = list(st.iterations_max), list(st.pass_ms)
        return cls(_handle=h), stats

    def serialize(self):
        """The vocabulary's file (loop/VocabularyBinary.hpp) as bytes."""
        n = C.c_size_t(0)
        rc = self.lib.vio_vocabulary_serialize(self._h, None, 0, C.byref(n))
        buf = C.create_string_buffer(max(1, n.value))
        rc = rc or self.lib.vio_vocabulary_serialize(self._h, buf, n.value, C.byref(n))
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_vocabulary_serialize failed rc=%d" % rc)
        return buf.raw[:n.value]

    def save(self, path):
        rc = self.lib.vio_vocabulary_save(self._h, str(path).encode())
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_vocabulary_save failed rc=%d" % rc)

    def info(self):
        a = np.zeros(6, np.int32)
        self.lib.vio_vocabulary_info(self._h, a.ctypes.data_as(_i32p))
        return dict(zip(("k", "L", "scoring", "weighting", "nodes", "words"), [int(x) for x in a]))

    def transform(self, desc_list, bow_stride=None):
        """desc_list: per keyframe uint64 [n][4]. -> per keyframe (word_id[n], word_weight[n], bow_word[m], bow_value[m])."""
        n_desc = np.array([len(d) for d in desc_list], np.int32)
        desc = np.ascontiguousarray(np.concatenate([np.asarray(d, np.uint64).reshape(-1, 4) for d in desc_list] + [np.zeros((0, 4), np.uint64)]))
        total = int(n_desc.sum())
        stride = int(bow_stride or max(1, int(n_desc.max())))
        wid, ww = np.zeros(max(1, total), np.int32), np.zeros(max(1, total), np.float64)
        bc = np.zeros(len(desc_list), np.int32)
        bw, bv = np.zeros((len(desc_list), stride), np.int32), np.zeros((len(desc_list), stride), np.float64)
        rc = self.lib.vio_vocabulary_transform(self._h, len(desc_list), n_desc.ctypes.data_as(_i32p), desc.ctypes.data_as(_u64p),
                                               wid.ctypes.data_as(_i32p), ww.ctypes.data_as(_f64p), bc.ctypes.data_as(_i32p),
                                               bw.ctypes.data_as(_i32p), bv.ctypes.data_as(_f64p), stride)
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_vocabulary_transform failed rc=%d (bow_count %s)" % (rc, bc))
        out, o = [], 0
        for f, n in enumerate(n_desc):
            out.append((wid[o:o + n].copy(), ww[o:o + n].copy(), bw[f, :bc[f]].copy(), bv[f, :bc[f]].copy()))
            o += n
        return out


class BowDatabase:
    """TemplatedDatabase<FBrief>: add(BowVector), query(BowVector, max_results, max_id) for batches of queries."""

    def __init__(self, voc, max_entries=4096, max_total_words=1 << 22):
        self.voc, self.lib = voc, voc.lib
        self._h = C.c_void_p()
        rc = self.lib.vio_bow_database_create(voc._h, max_entries, max_total_words, C.byref(self._h))
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_bow_database_create failed rc=%d" % rc)

    def close(self):
        if self._h:
            self.lib.vio_bow_database_destroy(self._h)
            self._h = C.c_void_p()

    def add(self, word, value):
        word, value = np.ascontiguousarray(word, np.int32), np.ascontiguousarray(value, np.float64)
        e = C.c_int32(-1)
        rc = self.lib.vio_bow_database_add(self._h, len(word), word.ctypes.data_as(_i32p), value.ctypes.data_as(_f64p), C.byref(e))
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_bow_database_add failed rc=%d" % rc)
        return e.value

    def query(self, bows, max_id, max_results=0):
        """bows: per query (word[m], value[m]); max_id: per query. -> per query (entry[r], score[r]), best first."""
        nq = len(bows)
        stride = max(1, max(len(b[0]) for b in bows))
        bc = np.array([len(b[0]) for b in bows], np.int32)
        bw, bv = np.zeros((nq, stride), np.int32), np.zeros((nq, stride), np.float64)
        for q, (w_, v_) in enumerate(bows):
            bw[q, :len(w_)], bv[q, :len(v_)] = w_, v_
        mid = np.ascontiguousarray(max_id, np.int32)
        n = C.c_int32(0)
        self.lib.vio_bow_database_size(self._h, C.byref(n))
        rs = max(1, n.value)
        nr = np.zeros(nq, np.int32)
        ent, sc = np.zeros((nq, rs), np.int32), np.zeros((nq, rs), np.float64)
        rc = self.lib.vio_bow_database_query(self._h, nq, bc.ctypes.data_as(_i32p), bw.ctypes.data_as(_i32p), bv.ctypes.data_as(_f64p), stride,
                                             mid.ctypes.data_as(_i32p), max_results, nr.ctypes.data_as(_i32p), ent.ctypes.data_as(_i32p),
                                             sc.ctypes.data_as(_f64p), rs)
        if rc != abi.VIO_OK:
            raise RuntimeError("vio_bow_database_query failed rc=%d" % rc)
        return [(ent[q, :nr[q]].copy(), sc[q, :nr[q]].copy()) for q in range(nq)]


# ---- the loop detector (DLoopDetector's detectLoop for n sessions: csrc/vio_loop_detector.hip) --------------------------
class VioLoopDetectorParams(C.Structure):
    _fields_ = [("use_nss", C.c_int32), ("alpha", C.c_float), ("k", C.c_int32), ("geom_check", C.c_int32), ("di_levels", C.c_int32),
                ("dislocal", C.c_int32), ("max_db_results", C.c_int32), ("min_nss_factor", C.c_float),
                ("min_matches_per_group", C.c_int32), ("max_intragroup_gap", C.c_int32), ("max_distance_between_groups", C.c_int32),
                ("max_distance_between_queries", C.c_int32), ("min_Fpoints", C.c_int32), ("max_neighbor_ratio", C.c_double),
                ("f_threshold", C.c_double), ("f_confidence", C.c_double), ("min_inliers", C.c_int32)]


class VioLoopDetection(C.Structure):
    _fields_ = [("status", C.c_int32), ("query", C.c_int32), ("match", C.c_int32), ("ns_factor", C.c_double), ("n_results", C.c_int32),
                ("n_after_cut", C.c_int32), ("island_first", C.c_int32), ("island_last", C.c_int32), ("island_best_entry", C.c_int32),
                ("island_score", C.c_double), ("island_best_score", C.c_double), ("consistent_entries", C.c_int32),
                ("n_di_matches", C.c_int32), ("n_inliers", C.c_int32)]


class VioLoopConnection(C.Structure):
    _fields_ = [("n_window", C.c_int32), ("ransac_ran", C.c_int32), ("n_kept", C.c_int32), ("connected", C.c_int32)]


class VioLoopKeyframe(C.Structure):
    _fields_ = [("detection", VioLoopDetection), ("connection", VioLoopConnection), ("n_fast", C.c_int32), ("n_keys", C.c_int32),
                ("fast_cut", C.c_int32)]


LOOP_STATUS = ("LOOP_DETECTED", "CLOSE_MATCHES_ONLY", "NO_DB_RESULTS", "LOW_NSS_FACTOR", "LOW_SCORES", "NO_GROUPS",
               "NO_TEMPORAL_CONSISTENCY", "NO_GEOMETRICAL_CONSISTENCY")   # DetectionStatus, TemplatedLoopDetector.h:46-64


def bind_loop_detector(lib):
    vp, pp, dp = C.c_void_p, C.POINTER(VioLoopDetectorParams), C.POINTER(VioLoopDetection)
    lib.vio_loop_detector_params_default.argtypes = [pp, C.c_float]
    lib.vio_loop_detector_params_default.restype = None
    lib.vio_loop_detector_create.argtypes = [vp, pp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    lib.vio_loop_detector_destroy.argtypes = [vp]
    lib.vio_loop_detector_destroy.restype = None
    lib.vio_loop_detector_get_device.argtypes = [vp, _i32p]
    lib.vio_loop_detector_detect.argtypes = [vp, C.c_int32, _i32p, _i32p, _fp, _u64p, dp, _fp, _fp, C.c_int32]
    lib.vio_loop_detector_erase.argtypes = [vp, C.c_int32, C.c_int32, _i32p]
    lib.vio_loop_detector_clear.argtypes = [vp, C.c_int32]
    lib.vio_loop_detector_size.argtypes = [vp, C.c_int32, _i32p]
    lib.vio_loop_detector_kernel_ms.argtypes = [vp, _fp]
    lib.vio_loop_detector_connect.argtypes = [vp, C.POINTER(abi.VioConfig), C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_int32,
                                              C.POINTER(VioLoopConnection), _u8p, _fp, _i32p, _i32p, C.POINTER(C.c_double)]
    lib.vio_loop_detector_keyframes.argtypes = [vp, vp, C.POINTER(abi.VioConfig), C.c_int32, C.c_int32, _i32p, vp, C.c_int32, _i32p, _fp, _i32p,
                                                _i32p, C.c_int32, C.c_int32, C.POINTER(VioLoopKeyframe), _u8p, _fp, _i32p, _i32p,
                                                C.POINTER(C.c_double), _fp, _fp, C.c_int32]
    lib.vio_loop_detector_set_cameras.argtypes = [vp, C.c_int32, _i32p, C.POINTER(abi.VioCamera)]
    lib.vio_loop_detector_get_camera.argtypes = [vp, C.c_int32, C.POINTER(abi.VioCamera)]
    return lib


def loop_detector_params(frequency=1.0, **over):
    """What the app constructs (Parameters(height, width) + set(frequency)), with fields overridden by keyword."""
    lib = bind_loop_detector(abi.load_product())
    p = VioLoopDetectorParams()
    lib.vio_loop_detector_params_default(C.byref(p), frequency)
    for k, v in over.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


class LoopDetectorError(RuntimeError):
    def __init__(self, what, rc):
        RuntimeError.__init__(self, "%s failed rc=%d" % (what, rc))
        self.rc = rc


class LoopDetector:
    """TemplatedLoopDetector<FBrief> for n_sessions sessions that share a vocabulary; detect() takes the newest keyframe
    of any subset of them."""

    def __init__(self, voc, params=None, n_sessions=1, max_entries=256, max_keypoints=1024):
        self.voc, self.lib = voc, bind_loop_detector(voc.lib)
        self.params = params if params is not None else loop_detector_params()
        self.n_sessions, self.max_keypoints = n_sessions, max_keypoints
        self._h = C.c_void_p()
        rc = self.lib.vio_loop_detector_create(voc._h, C.byref(self.params), n_sessions, max_entries, max_keypoints, C.byref(self._h))
        if rc != abi.VIO_OK:
            raise LoopDetectorError("vio_loop_detector_create", rc)

    def close(self):
        if self._h:
            self.lib.vio_loop_detector_destroy(self._h)
            self._h = C.c_void_p()

    def detect(self, sessions, keys_list, desc_list):
        """sessions: ids; keys_list / desc_list: per keyframe float [m][2] pixels, uint64 [m][4].
        -> per keyframe (dict of the VioLoopDetection fields, cur_pts [n_inliers][2], old_pts [n_inliers][2])."""
        n = len(sessions)
        ses = np.ascontiguousarray(sessions, np.int32)
        nk = np.array([len(d_) for d_ in desc_list], np.int32)
        keys = np.ascontiguousarray(np.concatenate([np.asarray(k_, np.float32).reshape(-1, 2) for k_ in keys_list] + [np.zeros((0, 2), np.float32)]))
        desc = np.ascontiguousarray(np.concatenate([np.asarray(d_, np.uint64).reshape(-1, 4) for d_ in desc_list] + [np.zeros((0, 4), np.uint64)]))
        assert len(keys) == len(desc)
        out = (VioLoopDetection * n)()
        stride = self.max_keypoints
        cur, old = np.zeros((n, stride, 2), np.float32), np.zeros((n, stride, 2), np.float32)
        rc = self.lib.vio_loop_detector_detect(self._h, n, ses.ctypes.data_as(_i32p), nk.ctypes.data_as(_i32p), keys.ctypes.data_as(_fp),
                                               desc.ctypes.data_as(_u64p), out, cur.ctypes.data_as(_fp), old.ctypes.data_as(_fp), stride)
        if rc != abi.VIO_OK:
            raise LoopDetectorError("vio_loop_detector_detect", rc)
        res = []
        for q in range(n):
            r = {f: getattr(out[q], f) for f, _ in VioLoopDetection._fields_}
            m = r["n_inliers"] if r["status"] == 0 else 0
            res.append((r, cur[q, :m].copy(), old[q, :m].copy()))
        return res

    def set_cameras(self, sessions, cams):
        """vio_loop_detector_set_cameras: session sessions[i] normalises with the intrinsics of cams[i] (abi.VioCamera) in
        connect() and keyframes(), in place of the cfg of the call. -> rc."""
        ses = np.ascontiguousarray(sessions, np.int32).reshape(-1)
        arr = (abi.VioCamera * max(len(cams), 1))(*cams)
        return self.lib.vio_loop_detector_set_cameras(self._h, len(ses), ses.ctypes.data_as(_i32p), arr)

    def get_camera(self, session):
        """-> (rc, abi.VioCamera); rc VIO_ESTATE: the session has none and uses the cfg of every call."""
        out = abi.VioCamera()
        return self.lib.vio_loop_detector_get_camera(self._h, session, C.byref(out)), out

    def connect(self, cfg, sessions, cur_entries, old_entries, n_window, ids=None, min_loop_num=22, stride=None, out=None):
        """findConnectionWithOldFrame for one (current, old) pair of entries per session, read from the detector's slabs.
        ids: per pair the feature ids of its window points (or None). -> per pair a dict of the VioLoopConnection fields
        plus status [n_window], matched_old_pts [n_window][2] (None without a connection), kept_index / kept_ids
        [n_kept], kept_old_norm [n_kept][2] (empty unless ransac_ran). out: the five raw arrays to fill (tests)."""
        n = len(sessions)
        ses, cur, old = (np.ascontiguousarray(a, np.int32) for a in (sessions, cur_entries, old_entries))
        nw = np.ascontiguousarray(n_window, np.int32)
        if stride is None:
            stride = max(1, int(nw.max()) if n else 1)
        idp = None
        if ids is not None:
            idp = np.zeros((n, stride), np.int32)
            for i, a in enumerate(ids):
                idp[i, :min(len(a), stride)] = np.asarray(a, np.int32)[:stride]
        res = (VioLoopConnection * max(n, 1))()
        if out is None:
            out = (np.zeros((n, stride), np.uint8), np.zeros((n, stride, 2), np.float32), np.zeros((n, stride), np.int32),
                   np.zeros((n, stride), np.int32), np.zeros((n, stride, 2), np.float64))
        status, pts, kidx, kids, norm = out
        rc = self.lib.vio_loop_detector_connect(self._h, C.byref(cfg), min_loop_num, n, ses.ctypes.data_as(_i32p), cur.ctypes.data_as(_i32p),
                                                old.ctypes.data_as(_i32p), nw.ctypes.data_as(_i32p),
                                                idp.ctypes.data_as(_i32p) if idp is not None else None, stride, res,
                                                status.ctypes.data_as(_u8p), pts.ctypes.data_as(_fp), kidx.ctypes.data_as(_i32p),
                                                kids.ctypes.data_as(_i32p), norm.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != abi.VIO_OK:
            raise LoopDetectorError("vio_loop_detector_connect", rc)
        got = []
        for i in range(n):
            r = {f: getattr(res[i], f) for f, _ in VioLoopConnection._fields_}
            m, k = r["n_window"], r["n_kept"]
            r["status"] = status[i, :m].copy()
            r["matched_old_pts"] = pts[i, :m].copy() if (r["ransac_ran"] or (m < 8 and k == m)) else None
            r["kept_index"] = kidx[i, :k].copy()
            r["kept_ids"] = kids[i, :k].copy() if ids is not None else None
            r["kept_old_norm"] = norm[i, :k].copy() if r["ransac_ran"] else np.zeros((0, 2))
            got.append(r)
        return got

    def keyframes(self, brief, cfg, sessions, frames, window_pts, ids=None, frame_index=None, on_device=False, min_loop_num=22,
                  fast_threshold=20, stride=None):
        """vio_loop_detector_keyframes: extraction (brief: a BriefExtractor), detect and connect for the newest keyframe of
        `sessions`. frames: a device pointer (int) with on_device, else a uint8 array of packed frames; frame i of the
        call is slot frame_index[i]. -> per keyframe a dict: detection (as detect()'s dict), cur_pts, old_pts, connection
        (as connect()'s dict; None unless the loop was detected), n_fast, n_keys, fast_cut, rows_written (the call wrote
        the keyframe's connection struct or its status / matched / kept rows)."""
        n = len(sessions)
        ses = np.ascontiguousarray(sessions, np.int32)
        nw, wp, stride = _window_arrays(window_pts, n, stride)
        fi = None if frame_index is None else np.ascontiguousarray(frame_index, np.int32)
        idp = None
        if ids is not None:
            idp = np.zeros((n, stride), np.int32)
            for i, a in enumerate(ids):
                idp[i, :min(len(a), stride)] = np.asarray(a, np.int32)[:stride]
        out = (VioLoopKeyframe * max(n, 1))()
        status, pts = np.zeros((n, stride), np.uint8), np.zeros((n, stride, 2), np.float32)
        kidx, kids, norm = np.zeros((n, stride), np.int32), np.zeros((n, stride), np.int32), np.zeros((n, stride, 2), np.float64)
        ps = self.max_keypoints
        cur, old = np.zeros((n, ps, 2), np.float32), np.zeros((n, ps, 2), np.float32)
        fptr = C.c_void_p(frames) if on_device else C.c_void_p(frames.ctypes.data)
        rc = self.lib.vio_loop_detector_keyframes(self._h, brief._h, C.byref(cfg), min_loop_num, n, ses.ctypes.data_as(_i32p), fptr,
                                                  1 if on_device else 0, None if fi is None else fi.ctypes.data_as(_i32p),
                                                  wp.ctypes.data_as(_fp), nw.ctypes.data_as(_i32p),
                                                  idp.ctypes.data_as(_i32p) if idp is not None else None, stride, fast_threshold, out,
                                                  status.ctypes.data_as(_u8p), pts.ctypes.data_as(_fp), kidx.ctypes.data_as(_i32p),
                                                  kids.ctypes.data_as(_i32p), norm.ctypes.data_as(C.POINTER(C.c_double)),
                                                  cur.ctypes.data_as(_fp), old.ctypes.data_as(_fp), ps)
        if rc != abi.VIO_OK:
            raise LoopDetectorError("vio_loop_detector_keyframes", rc)
        got = []
        for q in range(n):
            r = {f: getattr(out[q].detection, f) for f, _ in VioLoopDetection._fields_}
            m = r["n_inliers"] if r["status"] == 0 else 0
            k = dict(detection=r, cur_pts=cur[q, :m].copy(), old_pts=old[q, :m].copy(), connection=None, n_fast=out[q].n_fast,
                     n_keys=out[q].n_keys, fast_cut=out[q].fast_cut)
            c = {f: getattr(out[q].connection, f) for f, _ in VioLoopConnection._fields_}
            if r["status"] == 0:
                mw, nk = c["n_window"], c["n_kept"]
                c["status"] = status[q, :mw].copy()
                c["matched_old_pts"] = pts[q, :mw].copy() if (c["ransac_ran"] or (mw < 8 and nk == mw)) else None
                c["kept_index"] = kidx[q, :nk].copy()
                c["kept_ids"] = kids[q, :nk].copy() if ids is not None else None
                c["kept_old_norm"] = norm[q, :nk].copy() if c["ransac_ran"] else np.zeros((0, 2))
                k["connection"] = c
            # (the rows went in zeroed: a call that leaves a row alone leaves it zero)
            k["rows_written"] = bool(any(c[f] for f, _ in VioLoopConnection._fields_) or status[q].any() or kidx[q].any() or kids[q].any()
                                     or norm[q].any() or pts[q].any())
            got.append(k)
        return got

    def erase(self, session, entries):
        e = np.ascontiguousarray(entries, np.int32)
        rc = self.lib.vio_loop_detector_erase(self._h, session, len(e), e.ctypes.data_as(_i32p))
        if rc != abi.VIO_OK:
            raise LoopDetectorError("vio_loop_detector_erase", rc)

    def clear(self, session):
        rc = self.lib.vio_loop_detector_clear(self._h, session)
        if rc != abi.VIO_OK:
            raise LoopDetectorError("vio_loop_detector_clear", rc)

    def size(self, session):
        n = C.c_int32(-1)
        rc = self.lib.vio_loop_detector_size(self._h, session, C.byref(n))
        if rc != abi.VIO_OK:
            raise LoopDetectorError("vio_loop_detector_size", rc)
        return n.value

    def device(self):
        dev = C.c_int32(-1)
        rc = self.lib.vio_loop_detector_get_device(self._h, C.byref(dev))
        if rc != abi.VIO_OK:
            raise LoopDetectorError("vio_loop_detector_get_device", rc)
        return dev.value

    def kernel_ms(self):
        ms = C.c_float(0)
        rc = self.lib.vio_loop_detector_kernel_ms(self._h, C.byref(ms))
        if rc != abi.VIO_OK:
            raise LoopDetectorError("vio_loop_detector_kernel_ms", rc)
        return ms.value
