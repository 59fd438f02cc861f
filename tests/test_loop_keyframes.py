"""The loop thread's keyframe step from device-resident frames (csrc/vio_brief.hip, vio_brief_pack.hip, vio_loop_detector.hip):
vio_brief_extract_device = vio_brief_extract on the same pixels, and vio_loop_detector_keyframes = vio_brief_extract, then
vio_loop_detector_detect, then vio_loop_detector_connect for the sessions that detected -- every output and the detector's
state afterwards bit for bit (integers equal, floats and doubles by their bytes). Inputs: tests/loop_keyframe_cases.py.
On the CPU the cases are shown not to be vacuous with the restatements alone (oracle_extract of tests/test_brief.py, the
Detector of tests/test_loop_detector.py)."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers as H
import loop_keyframe_cases as KC
import test_brief as TB
import test_loop_detector as LD

pkg = H.pkg
loop, abi = pkg.loop, pkg.abi


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_case_sessions_are_not_vacuous():
    """A condition on the inputs, met by the restatements alone: loops are detected on consecutive keyframes, several other
    decisions occur, one keyframe has no descriptor at all and some FAST lists are cut at the capacity."""
    seen = collections.Counter()
    for shape in KC.SHAPES:
        twice, empty, cut = 0, 0, 0
        for sid in range(len(KC.SESSIONS)):
            ex, res, ses = KC.extracted(shape, sid), KC.restated(shape, sid), KC.session(shape, sid)
            status = [r["status"] for r, _, _ in res]
            seen.update(LD.STATUS[s] for s in status)
            twice += status.count(0) >= 2
            for (rc, keys, desc, n_fast), (img, w, ids) in zip(ex, ses):
                assert rc in (abi.VIO_OK, abi.VIO_ECAP) and len(keys) == len(desc) and len(w) == len(ids)
                assert (rc == abi.VIO_ECAP) == (n_fast > KC.CAP[shape] - len(w))
                assert np.array_equal(keys[len(keys) - len(w):], w)          # the window points close the list, cut or not
                empty += len(keys) == 0
                cut += n_fast > KC.CAP[shape] - len(w)
            for r, cur, old in res:
                if r["status"] == 0:
                    assert len(cur) == r["n_inliers"] > 20
        print(shape, "sessions with two detections", twice, "empty keyframes", empty, "cut keyframes", cut)
        assert twice >= 1 and empty == 1 and cut >= 1
        assert len({len(s) for s in KC.batch(shape)}) == len(KC.SESSIONS)      # sessions of different lengths
        assert max(len(w) for s in KC.batch(shape) for _, w, _ in s) > KC.MIN_LOOP_NUM
    print(dict(seen))
    assert len(seen) >= 4 and seen["LOOP_DETECTED"] >= 2 and seen["NO_DB_RESULTS"] >= 1


def test_entries_are_exported_declared_and_mirrored():
    lib = loop.bind_loop_detector(loop.bind_brief(abi.load_product()))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "vio_amd.h")).read(), flags=re.S)
    for name in ("vio_brief_extract_device", "vio_loop_detector_keyframes"):
        assert hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, txt), name
        assert getattr(lib, name).argtypes, name
    assert len(lib.vio_brief_extract_device.argtypes) == 12 and len(lib.vio_loop_detector_keyframes.argtypes) == 23
    assert "typedef struct VioLoopKeyframe" in txt
    names = [f for f, _ in loop.VioLoopKeyframe._fields_]
    assert names == ["detection", "connection", "n_fast", "n_keys", "fast_cut"]
    # C layout: two structs of 8-byte alignment (80 + 16 bytes), three ints, padded to 8
    assert C.sizeof(loop.VioLoopDetection) == 80 and loop.VioLoopKeyframe.connection.offset == 80
    assert loop.VioLoopKeyframe.n_fast.offset == 96 and C.sizeof(loop.VioLoopKeyframe) == 112


def test_null_arguments_are_refused_without_a_device(tmp_path):
    lib = loop.bind_loop_detector(loop.bind_brief(abi.load_product()))
    cfg = abi.default_config()
    one = np.zeros(8, np.int32)
    ip = one.ctypes.data_as(C.POINTER(C.c_int32))
    img = np.zeros(64, np.uint8)
    fp = np.zeros(8, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert lib.vio_brief_extract_device(None, C.c_void_p(img.ctypes.data), None, 1, fp, ip, 1, 20, None, None, ip, ip) == abi.VIO_EINVAL
    out = (loop.VioLoopKeyframe * 1)()
    st = np.zeros(8, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    nm = np.zeros(16, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.vio_loop_detector_keyframes(None, None, C.byref(cfg), 22, 1, ip, C.c_void_p(img.ctypes.data), 0, None, fp, ip, None, 1, 20, out,
                                         st, None, ip, None, nm, None, None, 0)
    assert rc == abi.VIO_EINVAL
    # the struct layout the header gives, against the mirror
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vio_amd.h"\nint main(){printf("%zu %zu %zu\\n",'
                   "sizeof(VioLoopKeyframe),offsetof(VioLoopKeyframe,connection),offsetof(VioLoopKeyframe,fast_cut));return 0;}\n")
    import subprocess
    subprocess.check_call(["gcc", "-I" + os.path.join(H.ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert got == [C.sizeof(loop.VioLoopKeyframe), loop.VioLoopKeyframe.connection.offset, loop.VioLoopKeyframe.fast_cut.offset]


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def same_bytes(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def same_extraction(got, want, what):
    assert len(got) == len(want), what
    for f, ((gk, gd, gn), (wk, wd, wn)) in enumerate(zip(got, want)):
        assert gn == wn, (what, f, gn, wn)
        same_bytes(gk, wk, (what, f, "keypoints")), same_bytes(gd, wd, (what, f, "descriptors"))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", KC.SHAPES)
def test_device_extraction_equals_host_extraction(shape):
    rows, cols = shape
    pat = TB.pattern()
    ses = KC.session(shape, 1)                                       # (its keyframe 8 is the flat one)
    ring = np.stack([ses[i][0] for i in (0, 3, 8, 6, 9)])            # the caller's buffer: 5 slots
    order = [4, 0, 0, 3, 2, 1]                                       # permuted, slot 0 twice, runs of one and of two slots
    wpts = [ses[0][1], np.zeros((0, 2), np.float32), ses[3][1], ses[6][1][:9], np.zeros((0, 2), np.float32), ses[9][1]]
    dev = loop.DeviceFrames(ring)
    big = loop.BriefExtractor(rows, cols, pat, max_frames=6, max_keypoints=2048)
    small = loop.BriefExtractor(rows, cols, pat, max_frames=6, max_keypoints=KC.CAP[shape] // 2)
    try:
        want = big.extract(ring[order], wpts, KC.FAST_THRESHOLD)
        rc, got = big.extract_device(dev.ptr, len(order), wpts, order, KC.FAST_THRESHOLD)
        assert rc == abi.VIO_OK
        same_extraction(got, want, "permuted")
        assert [len(k) - nf for k, _, nf in got] == [len(w) for w in wpts] and got[4][2] == 0 and len(got[4][0]) == 0
        # frame_index NULL = slots 0..n-1
        rc, got = big.extract_device(dev.ptr, 5, [wpts[1]] * 5, None, KC.FAST_THRESHOLD)
        assert rc == abi.VIO_OK
        same_extraction(got, big.extract(ring, [wpts[1]] * 5, KC.FAST_THRESHOLD), "in order")
        # NULL outputs: the counts alone
        rc, nf, nk = big.extract_device(dev.ptr, len(order), wpts, order, KC.FAST_THRESHOLD, counts_only=True)
        assert rc == abi.VIO_OK and list(nf) == [w[2] for w in want] and list(nk) == [len(w[0]) for w in want]
        # the cut: the FAST list ends at cap - n_window, the window points are kept, VIO_ECAP after valid outputs
        want = small.extract(ring[order], wpts, KC.FAST_THRESHOLD, allow_cut=True)
        rc, got = small.extract_device(dev.ptr, len(order), wpts, order, KC.FAST_THRESHOLD)
        assert rc == abi.VIO_ECAP
        same_extraction(got, want, "cut")
        assert len(got[0][0]) == small.cap and got[0][2] > small.cap and np.array_equal(got[0][0][small.cap - len(wpts[0]):], wpts[0])
        rc, nf, nk = small.extract_device(dev.ptr, len(order), wpts, order, KC.FAST_THRESHOLD, counts_only=True)
        assert rc == abi.VIO_ECAP and list(nf) == [w[2] for w in want] and list(nk) == [len(w[0]) for w in want]
        # refusals, each in a call that would otherwise end at VIO_ECAP (too many frames), so that no kernel can see the pointer
        # whatever the check says: a host pointer, a slot behind the end of the buffer, a negative slot
        host = np.ascontiguousarray(ring[[0] * 7])
        empty = [wpts[1]] * 7
        assert big.extract_device(dev.ptr, 7, empty, [0] * 7, counts_only=True)[0] == abi.VIO_ECAP      # 7 frames > max_frames
        assert big.extract_device(host.ctypes.data, 7, empty, [0] * 7, counts_only=True)[0] == abi.VIO_EINVAL
        assert big.extract_device(dev.ptr, 7, empty, [0] * 6 + [5], counts_only=True)[0] == abi.VIO_EINVAL   # slot 5 of 5
        assert big.extract_device(dev.ptr, 7, empty, [0] * 6 + [-1], counts_only=True)[0] == abi.VIO_EINVAL
    finally:
        big.close(), small.close(), dev.close()


class Rig:
    """One extractor, one buffer of device frames and the batch of KC.calls(shape); detectors are made per route."""

    def __init__(self, shape):
        self.shape, (self.rows, self.cols) = shape, shape
        self.voc = loop.BowVocabulary(LD.vocabulary(LD.VOC_SEED)[0])
        self.ses = KC.batch(shape)
        self.calls = KC.calls(shape)
        self.stride = KC.stride(shape)
        self.cap = KC.CAP[shape]
        self.cfg = abi.default_config(image_rows=self.rows, image_cols=self.cols, cx=self.cols / 2.0, cy=self.rows / 2.0)
        self.ex = loop.BriefExtractor(self.rows, self.cols, TB.pattern(), max_frames=len(self.ses), max_keypoints=self.cap)
        # the caller's buffer: every keyframe of the batch, session after session
        self.slot, frames = {}, []
        for s, kfs in enumerate(self.ses):
            for i, (img, _, _) in enumerate(kfs):
                self.slot[(s, i)] = len(frames)
                frames.append(img)
        self.frames = np.stack(frames)
        self.dev = loop.DeviceFrames(self.frames)
        self.open = []

    def detector(self, extra=2):
        d = loop.LoopDetector(self.voc, loop.loop_detector_params(1.0, **KC.DETECTOR), n_sessions=len(self.ses),
                              max_entries=max(len(s) for s in self.ses) + extra, max_keypoints=self.cap)
        self.open.append(d)
        return d

    def close(self):
        for d in self.open:
            d.close()
        self.ex.close(), self.dev.close(), self.voc.close()

    def three_calls(self, det, call):
        """Today's route for one call of the batch, in the result format of LoopDetector.keyframes."""
        imgs = np.stack([self.ses[s][i][0] for s, i in call])
        wpts, ids = [self.ses[s][i][1] for s, i in call], [self.ses[s][i][2] for s, i in call]
        ex = self.ex.extract(imgs, wpts, KC.FAST_THRESHOLD, allow_cut=True)
        sessions = [s for s, _ in call]
        dets = det.detect(sessions, [e[0] for e in ex], [e[1] for e in ex])
        out = [dict(detection=r, cur_pts=c, old_pts=o, connection=None, n_fast=e[2], n_keys=len(e[0]),
                    fast_cut=int(e[2] > self.cap - len(w)), rows_written=False) for (r, c, o), e, w in zip(dets, ex, wpts)]
        hit = [q for q, (r, _, _) in enumerate(dets) if r["status"] == 0]
        if hit:
            con = det.connect(self.cfg, [sessions[q] for q in hit], [dets[q][0]["query"] for q in hit], [dets[q][0]["match"] for q in hit],
                              [len(wpts[q]) for q in hit], [ids[q] for q in hit], KC.MIN_LOOP_NUM, self.stride)
            for q, c in zip(hit, con):
                out[q]["connection"], out[q]["rows_written"] = c, True
        return out

    def one_call(self, det, call, frames=None, reverse=False):
        call = call[::-1] if reverse else call
        wpts, ids = [self.ses[s][i][1] for s, i in call], [self.ses[s][i][2] for s, i in call]
        index = [self.slot[k] for k in call]
        src, on_device = (self.dev.ptr, True) if frames is None else (frames, False)   # (host frames: the same slots)
        out = det.keyframes(self.ex, self.cfg, [s for s, _ in call], src, wpts, ids, index, on_device, KC.MIN_LOOP_NUM, KC.FAST_THRESHOLD,
                            self.stride)
        return out[::-1] if reverse else out


def same_connection(gc, wc, where):
    assert sorted(gc) == sorted(wc)
    for f in wc:
        if isinstance(wc[f], np.ndarray):
            same_bytes(gc[f], wc[f], (where, f))
        else:
            assert gc[f] is wc[f] is None or gc[f] == wc[f], (where, f, gc[f], wc[f])


def same_keyframe(got, want, where):
    LD.same((got["detection"], got["cur_pts"], got["old_pts"]), (want["detection"], want["cur_pts"], want["old_pts"]), where)
    for f in ("n_fast", "n_keys", "fast_cut", "rows_written"):
        assert got[f] == want[f], (where, f, got[f], want[f])
    gc, wc = got["connection"], want["connection"]
    assert (gc is None) == (wc is None) == (want["detection"]["status"] != 0), where
    if wc is not None:
        same_connection(gc, wc, where)


@pytest.fixture(scope="module", params=KC.SHAPES, ids=lambda s: "%dx%d" % s)
def twins(request):
    """The batch driven through today's three calls on one detector and through vio_loop_detector_keyframes with device
    frames on its twin; both detectors stay open for the tests of their state."""
    rig = Rig(request.param)
    try:
        rig.old, rig.new = rig.detector(), rig.detector()
        rig.want = [rig.three_calls(rig.old, call) for call in rig.calls]
        rig.got = [rig.one_call(rig.new, call) for call in rig.calls]
        yield rig
    finally:
        rig.close()


@pytest.mark.gpu
def test_keyframe_step_equals_the_three_calls(twins):
    hist = collections.Counter()
    ran = connected = cut = empty = 0
    for c, (call, got, want) in enumerate(zip(twins.calls, twins.got, twins.want)):
        assert len(got) == len(want) == len(call)
        for (s, i), g, w in zip(call, got, want):
            same_keyframe(g, w, (twins.shape, "call", c, "session", s))
            hist[LD.STATUS[w["detection"]["status"]]] += 1
            cut, empty = cut + w["fast_cut"], empty + (w["n_keys"] == 0)
            if w["connection"] is not None:
                ran, connected = ran + w["connection"]["ransac_ran"], connected + w["connection"]["connected"]
                assert w["connection"]["n_window"] == len(twins.ses[s][i][1])
    print(twins.shape, dict(hist), "ransac ran", ran, "connected", connected, "cut", cut, "empty", empty)
    # asserted on the three-call route: the comparison above is not one of empty results
    assert hist["LOOP_DETECTED"] >= 2 and ran >= 1 and connected >= 1 and cut >= 1 and empty == 1 and len(hist) >= 4
    # ... and that route is the restatement's: same decisions (the device detector against the Python one)
    for s in range(len(twins.ses)):
        want = [r["status"] for r, _, _ in KC.restated(twins.shape, s)]
        assert [w["detection"]["status"] for call, res in zip(twins.calls, twins.want) for (s2, _), w in zip(call, res) if s2 == s] == want


@pytest.mark.gpu
def test_detector_state_is_the_same_afterwards(twins):
    n_ses = len(twins.ses)
    for s in range(n_ses):
        assert twins.old.size(s) == twins.new.size(s) == len(twins.ses[s])
    # an earlier (current, old) pair per session, read from the slabs: the stored keys and descriptors are the same
    cur = [len(twins.ses[s]) - 1 for s in range(n_ses)]
    old = [s % 3 for s in range(n_ses)]
    nw = [len(twins.ses[s][cur[s]][1]) for s in range(n_ses)]
    ids = [twins.ses[s][cur[s]][2] for s in range(n_ses)]
    a = twins.old.connect(twins.cfg, list(range(n_ses)), cur, old, nw, ids, KC.MIN_LOOP_NUM, twins.stride)
    b = twins.new.connect(twins.cfg, list(range(n_ses)), cur, old, nw, ids, KC.MIN_LOOP_NUM, twins.stride)
    for s, (x, y) in enumerate(zip(a, b)):
        same_connection(y, x, ("state connect", s))
    assert any(x["ransac_ran"] for x in a)
    # one plain detect with the same host keys and descriptors: database, direct index and temporal window are the same
    again = [KC.extracted(twins.shape, s)[1] for s in range(n_ses)]   # (the revisit of place 1 once more)
    ra = twins.old.detect(list(range(n_ses)), [e[1] for e in again], [e[2] for e in again])
    rb = twins.new.detect(list(range(n_ses)), [e[1] for e in again], [e[2] for e in again])
    for s, (x, y) in enumerate(zip(ra, rb)):
        LD.same(y, x, ("state detect", s))
    assert any(r["n_results"] > 0 for r, _, _ in ra)
    for s in range(n_ses):
        assert twins.old.size(s) == twins.new.size(s) == len(twins.ses[s]) + 1


@pytest.mark.gpu
def test_host_frames_give_the_same_results(twins):
    """frames_on_device = 0, the frames indexed the same way: once from pageable memory, once from a registered range; every
    other call with its sessions in reverse order."""
    lib = abi.load_product()
    for registered in (False, True):
        frames = twins.frames.copy()
        det = twins.detector()
        if registered:
            assert lib.vio_host_register(C.c_void_p(frames.ctypes.data), frames.nbytes) == abi.VIO_OK
        try:
            for c, call in enumerate(twins.calls):
                got = twins.one_call(det, call, frames, reverse=c % 2 == 1)
                for (s, _), g, w in zip(call, got, twins.got[c]):
                    same_keyframe(g, w, (twins.shape, "registered" if registered else "pageable", c, s))
        finally:
            if registered:
                assert lib.vio_host_unregister(C.c_void_p(frames.ctypes.data)) == abi.VIO_OK


@pytest.mark.gpu
def test_refusals_launch_nothing_and_change_nothing(twins):
    rig = twins
    det = rig.detector(extra=-6)                                      # sessions of 3..5 entries at most: soon full
    E = max(len(s) for s in rig.ses) - 6
    sizes = lambda: [det.size(s) for s in range(len(rig.ses))]

    def refused(rc, call, **kw):
        before = sizes()
        with pytest.raises(loop.LoopDetectorError) as e:
            kw.setdefault("det", det)
            d = kw.pop("det")
            wpts, ids = [rig.ses[s][i][1] for s, i in call], [rig.ses[s][i][2] for s, i in call]
            d.keyframes(kw.pop("ex", rig.ex), kw.pop("cfg", rig.cfg), [s for s, _ in call], kw.pop("frames", rig.dev.ptr), wpts, ids,
                        [rig.slot[k] for k in call], kw.pop("on_device", True), KC.MIN_LOOP_NUM, KC.FAST_THRESHOLD, kw.pop("stride", rig.stride))
        assert e.value.rc == rc and sizes() == before, (e.value.rc, rc)

    for i in range(E):                                                # fill session 0 alone
        rig.one_call(det, [(0, i)])
    assert sizes() == [E, 0, 0]
    first = rig.calls[0]
    refused(abi.VIO_ECAP, first)                                      # session 0 is full: sessions 1 and 2 of the call stay empty
    # A host pointer announced as device memory, in the call that has just been refused for capacity: VIO_EINVAL can only come
    # from the pointer check, and without that check the call would still end at VIO_ECAP before any launch.
    refused(abi.VIO_EINVAL, first, frames=rig.frames.ctypes.data)
    refused(abi.VIO_EINVAL, [(1, 0), (1, 1)])                         # a session twice
    refused(abi.VIO_EINVAL, [(1, 0), (2, 0)], stride=3)               # n_window > stride
    refused(abi.VIO_EINVAL, [(1, 0)], cfg=abi.default_config(image_rows=rig.rows + 1, image_cols=rig.cols))
    pat = TB.pattern()
    wide = loop.BriefExtractor(rig.rows, rig.cols, pat, max_frames=3, max_keypoints=rig.cap + 1)
    narrow = loop.BriefExtractor(rig.rows, rig.cols, pat, max_frames=1, max_keypoints=rig.cap)
    try:
        refused(abi.VIO_EINVAL, [(1, 0)], ex=wide)                    # the extractor holds more keypoints than the detector
        refused(abi.VIO_ECAP, [(1, 0), (2, 0)], ex=narrow)            # n above max_frames
    finally:
        wide.close(), narrow.close()
    # and the detector still works: the next keyframes of sessions 1 and 2 are what the twins got
    got = rig.one_call(det, [(1, 0), (2, 0)])
    for g, w in zip(got, rig.got[0][1:]):
        same_keyframe(g, w, "after the refusals")
    assert sizes() == [E, 1, 1]
