"""vio_loop_detector_connect (csrc/vio_loop_detector.hip): KeyFrame::findConnectionWithOldFrame (VINS_ios/loop/keyframe.cpp
:267-273) for one (current, old) pair of entries per session, read from the detector's device slabs, against
vio_loop_find_connection fed from the host with the very arrays the entries were filled with. Every comparison is exact.
The detector sits on the small synthetic vocabulary of test_loop_detector.py with geom_check = 3 (filling is cheap) and eight
entries per session; a current keyframe is N_FAST "FAST corners" followed by its window points, so the window descriptors
are the last n_window of the entry, as BriefExtractor leaves them."""
import ctypes as C
import itertools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import helpers as H
from helpers import pkg
from test_loop_detector import POP, VOC_SEED, World, as_bytes, vocabulary

loop, abi = pkg.loop, pkg.abi
K = 600                                              # max_keypoints: more than one LDS staging round of 512
N_FAST = 7
N_WINDOW = (0, 5, 8, 14, 15, 64, 65, 150, 257)       # keep all | LMedS 8..14 | plain RANSAC from 15 | wave / workgroup edges
N_OLD = (1, 63, 64, 65, 513, K)
PATTERN = 0xA5


def test_symbol_struct_and_null_arguments():
    lib = loop.bind_loop_detector(abi.load_product())
    assert hasattr(lib, "vio_loop_detector_connect")
    assert C.sizeof(loop.VioLoopConnection) == 16
    cfg = abi.default_config()
    one = np.zeros(1, np.int32)
    ip = one.ctypes.data_as(C.POINTER(C.c_int32))
    out = (loop.VioLoopConnection * 1)()
    st = np.zeros(1, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    nm = np.zeros(2).ctypes.data_as(C.POINTER(C.c_double))
    # no detector exists without a device (vio_loop_detector_create answers VIO_ENODEV): a null one is an argument error
    assert lib.vio_loop_detector_connect(None, C.byref(cfg), 22, 1, ip, ip, ip, ip, None, 1, out, st, None, ip, None, nm) == abi.VIO_EINVAL


def test_connect_refuses_without_device(tmp_path):
    script = tmp_path / "nodev.py"
    script.write_text(textwrap.dedent("""
        import ctypes as C, importlib, sys
        import numpy as np
        sys.path.insert(0, %r)
        pkg = importlib.import_module("vins-mobile_amd")
        lib = pkg.loop.bind_loop_detector(pkg.abi.load_product())
        p = pkg.loop.loop_detector_params()
        h = C.c_void_p()
        rc = lib.vio_loop_detector_create(None, C.byref(p), 4, 8, 512, C.byref(h))
        assert rc == pkg.abi.VIO_ENODEV and not h.value, rc
        cfg = pkg.abi.default_config()
        i = np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
        out = (pkg.loop.VioLoopConnection * 1)()
        st = np.zeros(1, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
        nm = np.zeros(2).ctypes.data_as(C.POINTER(C.c_double))
        rc = lib.vio_loop_detector_connect(h, C.byref(cfg), 22, 1, i, i, i, i, None, 1, out, st, None, i, None, nm)
        assert rc == pkg.abi.VIO_EINVAL, rc
        print("refused")
    """ % H.ROOT))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr


# ---- GPU ---------------------------------------------------------------------------------------------------------------
class Bed:
    """One detector; session s holds entry 0 = old keyframe, entry 1 = current keyframe of pair s (session `triple` a third
    entry). What went into detect() is kept for the host-fed yardstick."""

    def __init__(self):
        self.cfg = abi.default_config()
        w = World(VOC_SEED, 7, step=60, see=400, distract=200, n_places=4)   # 2/3 of a view repeat in the other lap
        rng = np.random.default_rng(11)
        self.pairs = []                                  # (old keys, old desc, cur keys, cur desc, n_window)
        for s, (nw, no) in enumerate(itertools.product(N_WINDOW, N_OLD)):
            (ko, fo), (kc, fc) = w.observe(s % 3, 0), w.observe(s % 3, 1)
            self.pairs.append((ko[:no], fo[:no], kc[:N_FAST + nw], fc[:N_FAST + nw], nw))
        # duplicate old descriptors with different keys: the first index wins
        (ko, fo), (kc, fc) = w.observe(1, 0), w.observe(1, 1)
        self.dup = len(self.pairs)
        self.pairs.append((np.concatenate([ko[:80], ko[80:160]]), np.concatenate([fo[:80], fo[:80]]), kc[:N_FAST + 40], fc[:N_FAST + 40], 40))
        # the only old descriptor is the complement of query 3: distance 256, no connection
        self.compl = len(self.pairs)
        self.pairs.append((ko[:1], ~fc[N_FAST + 3][None, :], kc[:N_FAST + 10], fc[:N_FAST + 10], 10))
        # three entries, for erase
        self.triple = len(self.pairs)
        self.pairs.append((ko[:100], fo[:100], kc[:N_FAST + 30], fc[:N_FAST + 30], 30))
        self.third = w.observe(2, 1)
        self.third = (self.third[0][:N_FAST + 20], self.third[1][:N_FAST + 20])
        self.ids = [(1000 * s + 3 * np.arange(p[4]) + rng.integers(0, 3, p[4])).astype(np.int32) for s, p in enumerate(self.pairs)]
        self.voc = loop.BowVocabulary(vocabulary(VOC_SEED)[0])
        S = len(self.pairs)
        self.det = loop.LoopDetector(self.voc, loop.loop_detector_params(geom_check=3), n_sessions=S, max_entries=8, max_keypoints=K)
        self.det.detect(list(range(S)), [p[0] for p in self.pairs], [p[1] for p in self.pairs])
        self.det.detect(list(range(S)), [p[2] for p in self.pairs], [p[3] for p in self.pairs])
        self.det.detect([self.triple], [self.third[0]], [self.third[1]])
        self.matcher = loop.Matcher()
        self._want = {}

    def want(self, s):
        """vio_loop_find_connection on the arrays session s was filled with (computed once)."""
        if s not in self._want:
            ko, fo, kc, fc, nw = self.pairs[s]
            n = len(fc)
            q, o = as_bytes(fc[n - nw:]), as_bytes(fo)
            every = nw == 0 or bool((POP[q[:, None, :] ^ o[None, :, :]].sum(-1).min(1) < 256).all())   # every query found a match
            self._want[s] = self.matcher.find_connection(self.cfg, fc[n - nw:], kc[n - nw:], fo, ko) + (every,)
        return self._want[s]

    def close(self):
        self.matcher.close(), self.det.close(), self.voc.close()


@pytest.fixture(scope="module")
def bed():
    b = Bed()
    yield b
    b.close()


def check_pair(bed, s, r, m):
    """Result r of connect (min_loop_num m) for session s against the host-fed yardstick."""
    mo, mn, status, k, connection = bed.want(s)
    nw = bed.pairs[s][4]
    if not connection:
        assert k == 0 and not status.any()
    assert r["n_window"] == nw and r["n_kept"] == k and np.array_equal(r["status"], status), s
    assert r["ransac_ran"] == (1 if nw >= 8 and connection else 0), s
    assert r["connected"] == (1 if r["ransac_ran"] and k > m else 0), (s, m)
    kept = np.nonzero(status)[0]
    assert np.array_equal(r["kept_index"], kept) and np.array_equal(r["kept_ids"], bed.ids[s][kept]), s
    if connection:
        assert np.array_equal(r["matched_old_pts"].view(np.uint32), mo.view(np.uint32)), s
    if r["ransac_ran"]:
        assert np.array_equal(r["kept_old_norm"].view(np.uint64), mn[kept].astype(np.float64).view(np.uint64)), s
    else:
        assert len(r["kept_old_norm"]) == 0


@pytest.mark.gpu
def test_connect_equals_find_connection_fed_from_the_host(bed):
    n_grid = len(N_WINDOW) * len(N_OLD)
    seen_kept = seen_dropped = seen_conn = seen_unconn = 0
    for s in range(n_grid):
        nw = bed.pairs[s][4]
        k = bed.want(s)[3]
        for m in (22, k - 1, k):                     # MIN_LOOP_NUM, and just below and just at n_kept
            r = bed.det.connect(bed.cfg, [s], [1], [0], [nw], ids=[bed.ids[s]], min_loop_num=m)[0]
            check_pair(bed, s, r, m)
        assert r["connected"] == 0                    # (m == n_kept: `>` is strict)
        if nw >= 8:
            seen_kept += int(r["status"].sum())
            seen_dropped += int((r["status"] == 0).sum())
            c22 = k > 22
            seen_conn += c22
            seen_unconn += not c22
        else:
            assert r["connected"] == 0 and r["n_kept"] == nw and r["status"].all()
    # the data has true pairs the RANSAC keeps and outliers it rejects; some pairs connect at MIN_LOOP_NUM, some do not
    print("kept %d dropped %d connected %d not connected %d" % (seen_kept, seen_dropped, seen_conn, seen_unconn))
    assert seen_kept > 0 and seen_dropped > 0 and seen_conn > 0 and seen_unconn > 0


@pytest.mark.gpu
def test_duplicate_old_descriptors_and_a_complement(bed):
    s = bed.dup
    ko, fo, kc, fc, nw = bed.pairs[s]
    r = bed.det.connect(bed.cfg, [s], [1], [0], [nw], ids=[bed.ids[s]])[0]
    check_pair(bed, s, r, 22)
    q, o = as_bytes(fc[N_FAST:]), as_bytes(fo)
    first = POP[q[:, None, :] ^ o[None, :, :]].sum(-1).argmin(1)     # argmin: the first of equal distances
    assert (first < 80).all()                                        # (every descriptor is there twice: never the copy)
    assert np.array_equal(r["matched_old_pts"], ko[first])
    s = bed.compl
    nw = bed.pairs[s][4]
    r = bed.det.connect(bed.cfg, [s], [1], [0], [nw], ids=[bed.ids[s]])[0]
    check_pair(bed, s, r, 22)
    assert r["n_kept"] == 0 and r["ransac_ran"] == 0 and r["connected"] == 0 and not r["status"].any()
    assert r["matched_old_pts"] is None


def raw_outputs(n, stride):
    return (np.full((n, stride), PATTERN, np.uint8), np.full((n, stride, 2), np.float32(-7.5)), np.full((n, stride), -77, np.int32),
            np.full((n, stride), -78, np.int32), np.full((n, stride, 2), -9.25))


@pytest.mark.gpu
def test_batch_equals_singles(bed):
    # nine sessions, mixed shapes, n_window 0 and 5 in the middle of the batch, in no particular order
    grid = list(itertools.product(N_WINDOW, N_OLD))
    pick = [grid.index(g) for g in ((257, K), (14, 63), (150, 513), (0, 64), (5, 1), (65, 65), (8, K), (64, 1), (15, 513))]
    nws = [bed.pairs[s][4] for s in pick]
    stride = 260
    outs = []
    for rep in range(2):
        o = raw_outputs(len(pick), stride)
        res = bed.det.connect(bed.cfg, pick, [1] * 9, [0] * 9, nws, ids=[bed.ids[s] for s in pick], stride=stride, out=o)
        outs.append((o, res))
    for a, b in zip(outs[0][0], outs[1][0]):
        assert a.tobytes() == b.tobytes()                            # two calls in a row give the same bytes
    o, res = outs[0]
    for i, s in enumerate(pick):
        check_pair(bed, s, res[i], 22)
        o1 = raw_outputs(1, stride)
        bed.det.connect(bed.cfg, [s], [1], [0], [nws[i]], ids=[bed.ids[s]], stride=stride, out=o1)
        for a, b in zip(o, o1):
            assert a[i].tobytes() == b[0].tobytes(), (s, i)          # every row equals the session's own n = 1 call
        # and what lies behind a row's valid part is the caller's
        assert (o[0][i, nws[i]:] == PATTERN).all() and (o[2][i, res[i]["n_kept"]:] == -77).all()


@pytest.mark.gpu
def test_refusals_erase_and_clear(bed):
    det, cfg = bed.det, bed.cfg
    a, b, t = 0 * len(N_OLD) + 5, 7 * len(N_OLD) + 5, bed.triple     # (n_window 0, K old), (150, K old), the three-entry session
    nwb = bed.pairs[b][4]
    assert det.size(a) == 2 and det.size(t) == 3

    def refused(ses, cur, old, nw, stride=300):
        o = raw_outputs(len(ses), stride)
        want = [x.copy() for x in o]
        with pytest.raises(loop.LoopDetectorError) as e:
            det.connect(cfg, ses, cur, old, nw, ids=[np.zeros(max(n, 0), np.int32) for n in nw], stride=stride, out=o)
        assert e.value.rc == abi.VIO_EINVAL, (ses, cur, old, nw)
        for x, y in zip(o, want):
            assert x.tobytes() == y.tobytes()                        # nothing written

    refused([b, b], [1, 1], [0, 0], [nwb, nwb])                      # a session twice
    refused([b, len(bed.pairs)], [1, 1], [0, 0], [nwb, 1])           # no such session
    refused([a, b], [1, 2], [0, 0], [0, nwb])                        # current entry outside [0, size), behind a good pair
    refused([b], [-1], [0], [nwb])
    refused([b], [1], [-1], [nwb])
    refused([b], [1], [1], [nwb])                                    # old_entry >= cur_entry
    refused([b], [0], [1], [1])
    refused([b], [1], [0], [nwb], stride=nwb - 1)                    # n_window > stride
    refused([b], [1], [0], [N_FAST + nwb + 1], stride=400)           # more than the current entry's keys
    refused([b], [1], [0], [-1])
    # the three-entry session: (2, 0) and (2, 1) work; erase entry 0; (2, 0) and (1, 0) are refused, (2, 1) still works
    nw3 = 20
    ids3 = [np.arange(nw3, dtype=np.int32)]
    before = [det.connect(cfg, [t], [2], [o], [nw3], ids=ids3)[0] for o in (0, 1)]
    kc, fc = bed.third
    for o, r in zip((0, 1), before):
        ko, fo = bed.pairs[t][0 + 2 * o], bed.pairs[t][1 + 2 * o]
        mo, mn, status, k = bed.matcher.find_connection(cfg, fc[-nw3:], kc[-nw3:], fo, ko)
        assert np.array_equal(r["status"], status) and r["n_kept"] == k and np.array_equal(r["matched_old_pts"], mo)
    det.erase(t, [0])
    refused([t], [2], [0], [nw3])
    refused([t], [1], [0], [nw3])
    after = det.connect(cfg, [t], [2], [1], [nw3], ids=ids3)[0]
    for f in before[1]:
        assert np.array_equal(after[f], before[1][f]), f
    check_pair(bed, b, det.connect(cfg, [b], [1], [0], [nwb], ids=[bed.ids[b]])[0], 22)   # other sessions are as they were
    det.erase(t, [2])                                                  # ... and an erased CURRENT entry is refused as well
    refused([t], [2], [1], [nw3])
    det.clear(t)
    assert det.size(t) == 0
    refused([t], [2], [1], [nw3])
    refused([t], [1], [0], [0])
