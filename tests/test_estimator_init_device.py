"""vio_estimator_set_init_device: the bundle adjustments of solveInitial (VINS.cpp:833-1145, inital_sfm.cpp:229-296) of
all sequences that reach it in one process_images call run in one vio_init_ba_solve launch, between two host halves of
phase A. Compared with the host route (switch off, the default) on the scenes of test_estimator_initialises_itself."""
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


def run_route(seed, device, steps=60, max_features=0):
    """One self-initialising replay (computed once per module); -> (loop, actions, window at the first VIO_FRAME_SOLVED
    frame, device-route count)."""
    key = (seed, bool(device), steps, max_features)
    if key not in _ROUTES:
        _ROUTES[key] = _run_route(*key)
    return _ROUTES[key]


def _run_route(seed, device, steps, max_features):
    cfg = abi.default_config(max_features=max_features) if max_features else abi.default_config()
    loop = RS.EstimatorLoop(cfg, seed=seed, self_init=True)
    loop.est.set_init_device(device)
    acts, first = [], None
    for _ in range(steps):
        r = loop.step()
        acts.append(r.action)
        if first is None and r.action == abi.VIO_FRAME_SOLVED:
            first = {k: np.array(v, copy=True) for k, v in loop.est.window().items()}
    count = loop.est.status().init_device_count
    return loop, acts, first, count


def state_difference(seed):
    """Largest absolute difference per window quantity at the first solved frame, device route against host route."""
    _, _, host, _ = run_route(seed, False)
    _, _, dev, _ = run_route(seed, True)
    return {k: float(np.abs(dev[k] - host[k]).max()) for k in QUANTITIES}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_device_route_initialises_like_the_host_route(seed):
    """The assertions of test_estimator_initialises_itself with the switch on, the host route's action list, and at least
    one bundle adjustment on the device."""
    cfg = abi.default_config()
    W = cfg.window_size
    loop, acts, _, count = run_route(seed, True)
    assert acts[:W] == [abi.VIO_FRAME_FILLING] * W
    assert acts[W:].count(abi.VIO_FRAME_SOLVED) >= 48 and abi.VIO_FRAME_FAILURE not in acts
    e = loop.errors()
    assert np.sqrt((e ** 2).mean()) < 0.1 and e.max() < 0.2, (np.sqrt((e ** 2).mean()), e.max())
    w = loop.est.window()
    k = loop.history[-1][0]
    v_true = loop.world.truth(k)[2]
    assert abs(np.linalg.norm(w["Vs"][W]) - np.linalg.norm(v_true)) < 0.1 and abs(w["Vs"][W][2] - v_true[2]) < 0.1
    assert np.abs(w["Bgs"][W] - loop.world.bg).max() < 5e-3
    assert acts == run_route(seed, False)[1]
    assert count >= 1 and run_route(seed, False)[3] == 0


# Largest |device route - host route| at the first VIO_FRAME_SOLVED frame, measured on an MI355X: the three scenes, six
# repetitions each (the test prints its own figures). The bundle adjustments agree to 1e-9 with the host's, but PnP of the
# in-between frames, the alignment and the first window solve (whose LDS atomics are not bit-reproducible: single
# repetitions ranged from a twentieth of these values to these values) sit behind them. The difference is not derivable;
# the assertion allows ten times what was observed.
OBSERVED = {"Ps": 1.12e-12, "Rs": 1.55e-12, "Vs": 1.42e-12, "Bas": 1.43e-11, "Bgs": 2.56e-14}


@pytest.mark.gpu
def test_first_solved_window_differs_from_the_host_route_by_rounding_only():
    worst = {k: max(state_difference(s)[k] for s in SEEDS) for k in QUANTITIES}
    print("observed state difference:", worst)
    for k in QUANTITIES:
        assert worst[k] <= 10 * OBSERVED[k], (k, worst[k], OBSERVED[k])


@pytest.mark.gpu
def test_staggered_sequences_equal_single_sequences():
    """Three sequences in one estimator, two of which reach solveInitial in the same call (their bundle adjustments share a
    launch) and one four calls later, give what three single-sequence estimators give, all on the device route. The pattern
    of test_estimator.py::test_batched_sequences_equal_single_sequences."""
    cfg = abi.default_config()
    W = cfg.window_size
    n_steps = 30
    start = [0, 0, 4]
    worlds = [RS.SyntheticWorld(cfg, s) for s in SEEDS]
    singles = []
    for q in range(3):
        s = RS.EstimatorLoop(cfg, seed=SEEDS[q], self_init=True)
        s.est.set_init_device(True)
        for _ in range(n_steps):
            s.step()
        singles.append(s)
    est = pkg.estimator.Estimator(cfg, worlds[0].tic, worlds[0].ric, n_seq=3)
    est.enable_initialization(True)
    est.set_init_device(True)
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
def test_a_problem_beyond_the_capacity_takes_the_host_route():
    """cfg.max_features is the bundle adjustment context's landmark capacity. Set to the landmark count of the first solved
    window (about 200 here) it fits the window solves of the start-up, but not the bundle adjustment, which also holds the
    landmarks that entered in the last two frames (feature_manager.cpp:239 keeps those out of the window). The replay ends
    three frames after the first solve: later windows outgrow that capacity on either route."""
    seed = SEEDS[0]
    loop, acts, _, _ = run_route(seed, False)
    nf0 = loop.history[0][3].n_features
    k0 = acts.index(abi.VIO_FRAME_SOLVED)
    _, acts_off, _, count_off = run_route(seed, False, k0 + 3, nf0)
    _, acts_on, _, count_on = run_route(seed, True, k0 + 3, nf0)
    assert acts_off == acts[:k0 + 3] and acts_off[k0:] == [abi.VIO_FRAME_SOLVED] * 3   # still initialises, on the same frame
    assert acts_on == acts_off and count_on == 0 and count_off == 0
    assert run_route(seed, True)[3] >= 1                 # (the full capacity takes the device route)
