"""Front end: frames for a subset of a context's sequences, per-sequence publish, reset (vio_frontend_submit_subset /
collect_subset / read_subset / reset / in_step). Everything is compared bit for bit: ids, xyz, state() against the CPU oracle
tracker (one object per sequence, fed only that sequence's frames and flags), pnp_points() against n_seq = 1 product contexts
fed the same."""
import ctypes as C
import functools

import numpy as np
import pytest

import detect_cases as D
import helpers as H
from helpers import abi, pkg, synth

pytestmark = pytest.mark.gpu
FeatureTracker = pkg.frontend.FeatureTracker
N_SEQ = 5
EMPTY_TICK = 4


def schedule(ticks):
    """-> per tick: (sequences to reset ahead of the call, [(sequence, publish)] of the call in ascending sequence order).
    0: every tick, publishes every third frame of its own. 1: every second tick (so its current bank is the opposite of
    sequence 0's), publishes its odd frames. 2: first frame at tick 5. 3: three ticks, a pause, reset at tick 7, frames again
    from tick 9 (its frame count starts over). 4: never. Tick EMPTY_TICK: no camera delivers, the call has n = 0."""
    own = [0] * N_SEQ
    out = []
    for t in range(ticks):
        resets = [3] if t == 7 else []
        if t == 7:
            own[3] = 0
        call = []
        if t != EMPTY_TICK:
            takes = {0: True, 1: t % 2 == 0, 2: t >= 5, 3: t < 3 or t >= 9, 4: False}
            flag = {0: lambda k: k % 3 == 0, 1: lambda k: k % 2 == 1, 2: lambda k: k % 2 == 0, 3: lambda k: k % 2 == 0}
            for s in range(N_SEQ):
                if takes[s]:
                    call.append((s, flag[s](own[s])))
                    own[s] += 1
        out.append((resets, call))
    return out


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what


@functools.lru_cache(maxsize=None)
def reference(rows, cols, corners, min_dist, ticks):
    """The schedule through the references, once per geometry: per tick {sequence: (obs ids, obs xyz, state, pnp_points)} of
    the called sequences; the frames [sequence][tick]."""
    cfg = abi.default_config(max_corners=corners, min_dist=min_dist, image_rows=rows, image_cols=cols)
    frames = [synth.make_image_stream(40 + s, ticks, rows=rows, cols=cols)[0] for s in range(N_SEQ)]
    oracle = [H.OracleTracker(cfg) for _ in range(N_SEQ)]
    single = [FeatureTracker(cfg, n_seq=1) for _ in range(N_SEQ)]
    per_tick = []
    for t, (resets, call) in enumerate(schedule(ticks)):
        for s in resets:  # a fresh FeatureTracker: ids from 0 again
            oracle[s].close(), single[s].close()
            oracle[s], single[s] = H.OracleTracker(cfg), FeatureTracker(cfg, n_seq=1)
        want = {}
        for s, pub in call:
            ids, xyz = oracle[s].read_image(frames[s][t], pub)
            single[s].read_images(frames[s][t:t + 1], pub)
            want[s] = (ids, xyz, oracle[s].state(), single[s].pnp_points(0))
        per_tick.append(want)
    for o, g in zip(oracle, single):
        o.close(), g.close()
    return cfg, frames, per_tick


def run_schedule(rows, cols, corners, min_dist, ticks, route):
    cfg, frames, per_tick = reference(rows, cols, corners, min_dist, ticks)
    trk = FeatureTracker(cfg, n_seq=N_SEQ)
    host = np.zeros((N_SEQ, rows, cols), np.uint8)  # the frames of a call, back to back in call order
    slots, px, dev = 7, rows * cols, C.c_void_p()
    if route == "device":  # packed [slots][rows][cols] device memory of the caller's
        hip = C.CDLL("libamdhip64.so")                       # the runtime libvio_amd.so is linked against
        hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        assert hip.hipMalloc(C.byref(dev), slots * px) == 0
    if route == "registered":
        trk.register_host(host)
    last = {s: (trk.state(s), trk.pnp_points(s)) for s in range(N_SEQ)}
    assert all(len(st[1]) == 0 and len(pp[1]) == 0 for st, pp in last.values())
    try:
        for t, (resets, call) in enumerate(schedule(ticks)):
            if resets:
                trk.reset(resets)
                for s in resets:
                    st, pp = trk.state(s), trk.pnp_points(s)
                    assert len(st[1]) == 0 and len(pp[1]) == 0
                    last[s] = (st, pp)
            if t % 2 == 1:
                call = call[::-1]  # seq[] descending on odd ticks
            seqs = [s for s, _ in call]
            flags = [1 if p else 0 for _, p in call]
            index = None
            for i, s in enumerate(seqs):
                host[i] = frames[s][t]
            if route == "device":
                index = [(3 * i + 2) % slots for i in range(len(seqs))]  # scattered slots: 2 5 1 4 0
                for i, k in enumerate(index):  # (a synchronous copy: the frames are complete before the call)
                    assert hip.hipMemcpy(dev.value + k * px, host[i].ctypes.data, px, 1) == 0   # hipMemcpyHostToDevice
                got = trk.read_subset(seqs, dev.value, flags, index)
            else:
                got = trk.read_subset(seqs, host if route == "registered" else host.copy(), flags)
            assert len(got) == len(seqs)
            for i, (s, pub) in enumerate(call):  # rows of out_obs follow the call's order
                ids, xyz, state, pnp = per_tick[t][s]
                what = "%s tick %d sequence %d (call position %d, publish %d)" % (route, t, s, i, pub)
                print(what, "observations", len(got[i][0]), "oracle", len(ids), "state", len(state[1]), "pnp", len(pnp[1]))
                assert_same(got[i], (ids, xyz), what + ": observations")
                last[s] = (trk.state(s), trk.pnp_points(s))
                assert_same(last[s][0], state, what + ": state")
                assert_same(last[s][1], pnp, what + ": pnp_points")
            for s in set(range(N_SEQ)) - set(seqs):  # not called: not touched
                what = "%s tick %d sequence %d (not called)" % (route, t, s)
                assert_same(trk.state(s), last[s][0], what + ": state")
                assert_same(trk.pnp_points(s), last[s][1], what + ": pnp_points")
        assert len(trk.state(4)[1]) == 0
        published = sum(len(per_tick[t][s][0]) for t in range(ticks) for s in per_tick[t])
        assert published > 0 and not trk.in_step()
    finally:
        if route == "registered":
            trk.unregister_host(host)
        trk.close()
        if route == "device":
            hip.hipFree(dev)


@pytest.mark.parametrize("route", ["host", "registered", "device"])
def test_schedule_odd_geometry(route):
    """250 x 333 / 60 corners / min_dist 12, 14 ticks: the byte-wise pyramid path and partial strips, through all three
    frame routes. Sequences 0 and 1 sit in opposite banks from tick 2 on: one shared bank index cannot pass."""
    run_schedule(250, 333, 60, 12, 14, route)


def test_schedule_fused_pyramid():
    """480 x 640 / 150 corners, six ticks: level 0 and level 1 from one read of the frame (dword rows)."""
    run_schedule(480, 640, 150, 30, 6, "host")


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)])
def test_subset_of_all_equals_read_images(order):
    """seq = all sequences and one flag for all: the lock-step call of a second context, frame by frame; again permuted."""
    rows, cols, S, T = 97, 61, 3, 4
    cfg = abi.default_config(max_corners=20, min_dist=8, image_rows=rows, image_cols=cols)
    frames = np.stack([synth.make_image_stream(70 + s, T, rows=rows, cols=cols)[0] for s in range(S)], axis=1)  # [T][S]
    a, b = FeatureTracker(cfg, n_seq=S), FeatureTracker(cfg, n_seq=S)
    total = 0
    for t in range(T):
        pub = t % 2 == 0
        want = a.read_images(frames[t], pub)
        got = b.read_subset(list(order), frames[t][list(order)], pub)
        assert b.in_step()
        for i, s in enumerate(order):
            assert_same(got[i], want[s], "frame %d sequence %d: observations" % (t, s))
            assert_same(b.state(s), a.state(s), "frame %d sequence %d: state" % (t, s))
            assert_same(b.pnp_points(s), a.pnp_points(s), "frame %d sequence %d: pnp_points" % (t, s))
            total += len(want[s][0])
    assert total > 0
    a.close(), b.close()


def test_redo_path_inside_a_subset(monkeypatch, capfd):
    """The tracker plateau scenes (six of the seven overflow the detector's lists: more than the kRedoSlots = 4 full-size
    lists), five overflowing ones published in one call next to two sequences that do not publish and one sequence that is
    not in the call at all. The context's own count says that the redo workgroups did the work."""
    import re
    monkeypatch.setenv("VIO_AMD_REDO_REPORT", "1")
    rows, cols = D.TRACKER_PLATEAU_SHAPE
    cfg = D.config(rows, cols, 60, 10)
    scenes = D.turn_scenes()
    S = D.TURN_SEQUENCES + 1
    assert S == 8 and D.REDO_LISTS == 4
    scenes.append(D.texture(rows, cols, seed=8))
    trk = FeatureTracker(cfg, n_seq=S)
    oracle = [H.OracleTracker(cfg) for _ in range(S)]
    # frame 0: everyone but sequence 7 sees a first image; 0 1 2 4 5 overflow and publish, 3 (ordinary) and 6 do not publish
    # frame 1: sequence 7 joins and publishes, 5 stays out; 6 publishes now (cold start: overflows), 3 as well
    plan = [([6, 0, 3, 1, 2, 4, 5], {0: 1, 1: 1, 2: 1, 4: 1, 5: 1, 3: 0, 6: 0}),
            ([7, 6, 4, 3, 2, 1, 0], {7: 1, 6: 1, 3: 1, 4: 0, 2: 0, 1: 1, 0: 1})]
    untouched = {0: 7, 1: 5}
    for f, (seqs, pub) in enumerate(plan):
        before = trk.state(untouched[f])
        got = trk.read_subset(seqs, np.stack([scenes[s] for s in seqs]), [pub[s] for s in seqs])
        for i, s in enumerate(seqs):
            want = oracle[s].read_image(scenes[s], bool(pub[s]))
            print("frame", f, "sequence", s, "publish", pub[s], "observations", len(got[i][0]), "oracle", len(want[0]))
            assert_same(got[i], want, "frame %d sequence %d: observations" % (f, s))
            assert_same(trk.state(s), oracle[s].state(), "frame %d sequence %d: state" % (f, s))
        assert_same(trk.state(untouched[f]), before, "frame %d: the sequence outside the call" % f)
    assert all(len(trk.state(s)[1]) > 0 for s in (0, 1, 2, 4, 5))
    for o in oracle:
        o.close()
    capfd.readouterr()
    trk.close()
    m = re.search(r"detector: (\d+) sequence-frames redone", capfd.readouterr().err)
    assert m, "no redo report"
    print("redone: %s sequence-frames" % m.group(1))
    # frame 0: the five published plateau scenes; frame 1: sequence 6's cold start, and sequences 0 and 1 where they lost tracks
    assert 6 <= int(m.group(1)) <= 8


def test_contract():
    rows, cols, S = 97, 61, 3
    cfg = abi.default_config(max_corners=20, min_dist=8, image_rows=rows, image_cols=cols)
    frames = np.stack([synth.make_image_stream(80 + s, 3, rows=rows, cols=cols)[0] for s in range(S)], axis=1)  # [T][S]
    trk, fresh = FeatureTracker(cfg, n_seq=S), FeatureTracker(cfg, n_seq=S)
    lib, ip, u8p = trk.lib, C.POINTER(C.c_int32), C.POINTER(C.c_uint8)

    def rc_of(fn):
        with pytest.raises(pkg.frontend.TrackerError) as e:
            fn()
        return e.value.rc

    def snapshot():
        return [trk.state(s) + trk.pnp_points(s) for s in range(S)]

    def same(a, b):
        return all(len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y)) for x, y in zip(a, b))

    assert trk.in_step()
    trk.read_subset([0, 1, 2], frames[0], 1)
    assert trk.in_step()
    s0 = snapshot()
    assert all(len(st[1]) > 0 for st in s0)
    # bad arguments: VIO_EINVAL, no sequence changed, nothing in flight afterwards
    assert rc_of(lambda: trk.submit_subset([1, 1], frames[1][:2], 1)) == abi.VIO_EINVAL          # duplicate
    assert rc_of(lambda: trk.submit_subset([0, 3], frames[1][:2], 1)) == abi.VIO_EINVAL          # out of range
    assert rc_of(lambda: trk.submit_subset([-1], frames[1][:1], 1)) == abi.VIO_EINVAL
    assert rc_of(lambda: trk.submit_subset([0], frames[1][:1, :-1], 1)) == abi.VIO_EINVAL        # wrong size
    seqs = np.array([0, 1], np.int32)
    f1 = np.ascontiguousarray(frames[1][:2])
    assert lib.vio_frontend_submit_subset(trk._h, 2, seqs.ctypes.data_as(ip), C.c_void_p(f1.ctypes.data), 0, None, rows, cols, cols,
                                          None) == abi.VIO_EINVAL                                # publish == NULL
    assert lib.vio_frontend_submit_subset(trk._h, 4, seqs.ctypes.data_as(ip), C.c_void_p(f1.ctypes.data), 0, None, rows, cols, cols,
                                          f1.ctypes.data_as(u8p)) == abi.VIO_EINVAL              # n > n_seq
    assert rc_of(lambda: trk.reset([2, 2])) == abi.VIO_EINVAL
    assert rc_of(trk.collect_subset) == abi.VIO_ESTATE   # nothing in flight
    assert same(snapshot(), s0) and trk.in_step()
    # n == 0: VIO_OK, nothing launched, nothing changed
    assert trk.read_subset([], frames[1][:0], []) == []
    assert same(snapshot(), s0)
    # one frame in flight, and each submit has its own collect
    trk.submit_subset([1], frames[1][1:2], 0)
    assert rc_of(lambda: trk.submit_subset([0], frames[1][:1], 0)) == abi.VIO_ESTATE
    assert rc_of(lambda: trk.submit(frames[1], 0)) == abi.VIO_ESTATE
    assert rc_of(trk.collect) == abi.VIO_ESTATE          # mixed collect: the frame stays in flight
    assert rc_of(lambda: trk.reset([0])) == abi.VIO_ESTATE
    assert [len(ids) for ids, _ in trk.collect_subset()] == [0]
    assert not trk.in_step()
    # out of phase: every lock-step entry point refuses
    assert rc_of(lambda: trk.read_images(frames[2], 1)) == abi.VIO_ESTATE
    assert rc_of(lambda: trk.submit(frames[2], 1)) == abi.VIO_ESTATE
    assert rc_of(lambda: trk.submit(frames[2], 1, asynchronous=True)) == abi.VIO_ESTATE
    trk.upload_frames(frames)
    assert rc_of(lambda: trk.step(0, 1)) == abi.VIO_ESTATE
    s1 = snapshot()
    assert same(s1[:1] + s1[2:], s0[:1] + s0[2:]) and not same(s1[1:2], s0[1:2])
    # a lock-step submit is collected by collect, not by collect_subset
    trk.reset([1])
    assert not trk.in_step()                             # sequence 1 has no image, the others do
    trk.reset()
    assert trk.in_step()
    assert all(len(trk.state(s)[1]) == 0 and len(trk.pnp_points(s)[1]) == 0 for s in range(S))
    trk.submit(frames[0], 1)
    assert rc_of(trk.collect_subset) == abi.VIO_ESTATE
    got = trk.collect()
    want = fresh.read_images(frames[0], 1)
    assert all(len(ids) > 0 and np.array_equal(ids, np.arange(len(ids))) for ids, _ in got)   # ids from 0 again
    for t in (1, 2):                                     # ... and the context is a fresh one: the same tracks from here on
        for s in range(S):
            assert_same(got[s], want[s], "after reset: sequence %d observations" % s)
            assert_same(trk.state(s), fresh.state(s), "after reset: sequence %d state" % s)
        got, want = trk.read_images(frames[t], t == 2), fresh.read_images(frames[t], t == 2)
    for s in range(S):
        assert_same(got[s], want[s], "after reset: sequence %d observations" % s)
        assert len(want[s][0]) > 0
    trk.close(), fresh.close()
