"""vio_estimator_set_init_device(est, 2): phase A of a starting sequence does the landmark dump, relativePose's scan and the
lists of the in-between frames on the host pool; relative pose fit, GlobalSFM::construct with its bundle adjustment and the
PnP of the in-between frames (VINS.cpp:833-1003) of all sequences that got this far in the call run in ONE
vio_init_sfm_solve; alignment and the first window follow on the pool. Compared with the host route (level 0, the default)
on the replays of test_estimator_init_device.py."""
import os
import sys

import numpy as np
import pytest

import helpers as H
from helpers import abi, pkg

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
import replay_synthetic as RS  # noqa: E402
from test_estimator import _SeqView  # noqa: E402

SEEDS = [1, 3, 4]
QUANTITIES = ["Ps", "Rs", "Vs", "Bas", "Bgs"]
_ROUTES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_routes():
    yield
    for r in _ROUTES.values():
        r[0].close()
    _ROUTES.clear()


def run_route(seed, level, steps=60, max_features=0, relpose=None):
    """One self-initialising replay (computed once per module); -> (loop, actions, window at the first VIO_FRAME_SOLVED
    frame, device-route count)."""
    key = (seed, int(level), steps, max_features, relpose)
    if key not in _ROUTES:
        cfg = abi.default_config(max_features=max_features) if max_features else abi.default_config()
        loop = RS.EstimatorLoop(cfg, seed=seed, self_init=True)
        if relpose is not None:
            loop.est.enable_initialization(relpose)
        loop.est.set_init_device(level)
        acts, first = [], None
        for _ in range(steps):
            r = loop.step()
            acts.append(r.action)
            if first is None and r.action == abi.VIO_FRAME_SOLVED:
                first = {k: np.array(v, copy=True) for k, v in loop.est.window().items()}
        _ROUTES[key] = (loop, acts, first, loop.est.status().init_device_count)
    return _ROUTES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_level_2_initialises_like_the_host_route(seed):
    """The host route's action list, at least one start-up on the device, the accuracy assertions of
    test_device_route_initialises_like_the_host_route, and the first solved window within the project's parity bar for
    solver states (1e-6, test_staggered_sequences_equal_single_sequences)."""
    cfg = abi.default_config()
    W = cfg.window_size
    loop, acts, first, count = run_route(seed, 2)
    _, acts0, first0, count0 = run_route(seed, 0)
    assert acts == acts0
    assert count >= 1 and count0 == 0
    assert acts[:W] == [abi.VIO_FRAME_FILLING] * W
    assert acts[W:].count(abi.VIO_FRAME_SOLVED) >= 48 and abi.VIO_FRAME_FAILURE not in acts
    e = loop.errors()
    assert np.sqrt((e ** 2).mean()) < 0.1 and e.max() < 0.2, (np.sqrt((e ** 2).mean()), e.max())
    w = loop.est.window()
    k = loop.history[-1][0]
    v_true = loop.world.truth(k)[2]
    assert abs(np.linalg.norm(w["Vs"][W]) - np.linalg.norm(v_true)) < 0.1 and abs(w["Vs"][W][2] - v_true[2]) < 0.1
    assert np.abs(w["Bgs"][W] - loop.world.bg).max() < 5e-3
    diff = {k: float(np.abs(first[k] - first0[k]).max()) for k in QUANTITIES}
    print("seed %d: first solved window, level 2 - host route:" % seed, diff)
    for k in QUANTITIES:
        assert diff[k] < 1e-6, (k, diff[k])


@pytest.mark.gpu
def test_five_point_route_passes_its_relative_pose_in():
    """enable_initialization(1): the relative pose is the host's five-point result, passed in (relative_mode 0). The action
    list is the host route's. The first solved window is compared with level 1, which runs the same bundle adjustment kernel
    behind the host's chain: the five-point pose of one minimal sample is a poor start, and this replay's bundle adjustment
    carries the 1e-9 between the device's and the host's summation orders to 1.6e-6 in Ps (level 2 against level 0; against
    level 1: 4e-11)."""
    _, acts, first, count = run_route(SEEDS[0], 2, relpose=1)
    _, acts0, _, count0 = run_route(SEEDS[0], 0, relpose=1)
    _, acts1, first1, _ = run_route(SEEDS[0], 1, relpose=1)
    assert acts == acts0 == acts1 and count0 == 0
    assert (first is None) == (first1 is None)
    if first is not None:
        assert count >= 1
        for k in QUANTITIES:
            d = float(np.abs(first[k] - first1[k]).max())
            print("five-point route, level 2 - level 1, %s: %.3g" % (k, d))
            assert d < 1e-6, k


@pytest.mark.gpu
def test_staggered_sequences_equal_single_sequences_at_level_2():
    """Three sequences in one estimator, two of which reach solveInitial in the same call (they share one
    vio_init_sfm_solve) and one four calls later, give what three single-sequence estimators give. The pattern of
    test_estimator_init_device.py::test_staggered_sequences_equal_single_sequences."""
    cfg = abi.default_config()
    W = cfg.window_size
    n_steps = 30
    start = [0, 0, 4]
    worlds = [RS.SyntheticWorld(cfg, s) for s in SEEDS]
    singles = []
    for q in range(3):
        s = RS.EstimatorLoop(cfg, seed=SEEDS[q], self_init=True)
        s.est.set_init_device(2)
        for _ in range(n_steps):
            s.step()
        singles.append(s)
    est = pkg.estimator.Estimator(cfg, worlds[0].tic, worlds[0].ric, n_seq=3)
    est.enable_initialization(True)
    est.set_init_device(2)
    feeders = [RS.EstimatorLoop(cfg, seed=SEEDS[q], self_init=True, world=worlds[q]) for q in range(3)]
    got, first_call = [[] for _ in range(3)], [None] * 3
    for call in range(n_steps + max(start)):
        obs, hdr, act = [], [], []
        for q in range(3):
            k = call - start[q]
            f = feeders[q]
            if k < 0 or k >= n_steps:
                obs.append(([], [])), hdr.append(0.0), act.append(0)
                continue
            f.est.close()
            f.est = _SeqView(est, q)
            obs.append(f.feed_until_image()), hdr.append(worlds[q].time(k)), act.append(1)
        res = est.process_images(obs, hdr, act)
        for q in range(3):
            if res[q].action == abi.VIO_FRAME_SOLVED:
                got[q].append(est.window(q)["Ps"][W].copy())
                if first_call[q] is None:
                    first_call[q] = call
    for q in range(3):
        want = np.array([h[1] for h in singles[q].history])
        assert len(want) > 10 and len(got[q]) == len(want)
        assert np.abs(np.array(got[q]) - want).max() < 1e-6   # (the window kernel's LDS atomics: sums are not bit-reproducible)
        assert est.status(q).init_device_count == singles[q].est.status().init_device_count >= 1
        assert first_call[q] - start[q] == singles[q].history[0][0]
    est.close()
    for s in singles:
        s.close()


@pytest.mark.gpu
def test_a_problem_beyond_the_capacity_takes_the_host_route_at_level_2():
    """cfg.max_features is the context's landmark capacity (see test_estimator_init_device.py): set to the landmark count of
    the first solved window it fits the window solves of the start-up but not the start-up's own problem."""
    seed = SEEDS[0]
    loop, acts, _, _ = run_route(seed, 0)
    nf0 = loop.history[0][3].n_features
    k0 = acts.index(abi.VIO_FRAME_SOLVED)
    _, acts_off, _, count_off = run_route(seed, 0, k0 + 3, nf0)
    _, acts_on, _, count_on = run_route(seed, 2, k0 + 3, nf0)
    assert acts_off == acts[:k0 + 3] and acts_off[k0:] == [abi.VIO_FRAME_SOLVED] * 3
    assert acts_on == acts_off and count_on == 0 and count_off == 0
    assert run_route(seed, 2)[3] >= 1                    # (the full capacity takes the device route)


@pytest.mark.gpu
def test_the_level_is_checked():
    cfg = abi.default_config()
    loop = RS.EstimatorLoop(cfg, seed=1, self_init=True)
    try:
        assert loop.est.lib.vio_estimator_set_init_device(loop.est._h, 3) == abi.VIO_EINVAL
        assert loop.est.lib.vio_estimator_set_init_device(loop.est._h, -1) == abi.VIO_EINVAL
        for level in (0, 1, 2):
            assert loop.est.lib.vio_estimator_set_init_device(loop.est._h, level) == abi.VIO_OK
    finally:
        loop.close()
