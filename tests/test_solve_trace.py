"""csrc/solve_trace.h on the host: the iteration trace's writer against its reader, the step evaluator and the dogleg
combination that the three trust-region kernels share. The header is compiled into a stand-alone program
(tests/emul/solve_trace_check.cpp) that prints what each piece made of the numbers on its command line; what it should
have made of them is worked out here."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import helpers as H

EMUL_DIR = os.path.join(H.ROOT, "tests", "emul")
MAX_TRACE = 64
ARRAYS = ("it_cost", "it_radius", "it_step_norm", "it_relative_decrease", "it_gradient_max_norm", "it_flags")


@pytest.fixture(scope="module")
def prog():
    exe = os.path.join(EMUL_DIR, "solve_trace_check")
    csrc = os.path.join(H.ROOT, "vins-mobile_amd", "csrc")
    inc = os.path.join(H.ROOT, "include")
    srcs = [os.path.join(EMUL_DIR, "solve_trace_check.cpp"), os.path.join(csrc, "solve_trace.h"), os.path.join(csrc, "vio_math.h"),
            os.path.join(inc, "vio_amd.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + inc, "-I" + csrc, "-o", exe, srcs[0]])

    def run(*args):
        out = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], check=True, capture_output=True, text=True)
        return [line.split() for line in out.stdout.splitlines()]
    return run


def unpacked(prog, n_records, recorded):
    """N record calls, finish(recorded), unpack_solve_stats: (header, name -> the array's 64 slots)."""
    lines = prog("trace", n_records, recorded)
    assert lines[0] == ["guards", "1"]                     # nothing was written behind the raw arrays
    assert lines[1][0] == "header" and [l[0] for l in lines[2:]] == list(ARRAYS)
    header = [float(x) for x in lines[1][1:3]] + [int(x) for x in lines[1][3:]]
    return header, {l[0]: np.array([float(x) for x in l[1:]]) for l in lines[2:]}


def expected_arrays(n):
    """What solve_trace_check.cpp records at i = 0 .. n-1, zeros behind."""
    i = np.arange(MAX_TRACE, dtype=np.float64)
    full = dict(it_cost=100.0 - i, it_radius=1e4 / (1 + i), it_step_norm=0.25 * i, it_relative_decrease=0.5 + 0.125 * i,
                it_gradient_max_norm=1.0 / (1 + i), it_flags=(i % 2 == 0) * 1.0 + (i % 3 == 0) * 2.0)
    return {k: np.where(i < n, v, 0.0) for k, v in full.items()}


@pytest.mark.parametrize("n_records,recorded", [(0, 0), (3, 3), (65, 64), (5, 2)])
def test_writer_then_reader_round_trips_and_slots_past_iterations_are_zero(n_records, recorded, prog):
    """The raw arrays start as NaN / -1. (65, 64): a full trace, and the record call at index 64 is dropped. (5, 2):
    records behind `iterations` are not copied either."""
    header, got = unpacked(prog, n_records, recorded)
    assert header == [100.0, 36.5, recorded, 1, 7, 3]
    want = expected_arrays(recorded)
    for k in ARRAYS:
        assert got[k].shape == (MAX_TRACE,) and np.array_equal(got[k], want[k]), k


def test_negative_iterations_copy_nothing(prog):
    header, got = unpacked(prog, 3, -1)
    assert header == [100.0, 36.5, -1, 1, 7, 3]
    for k in ARRAYS:
        assert np.array_equal(got[k], np.zeros(MAX_TRACE)), k


class CeresStepEvaluator:
    """TrustRegionStepEvaluator of the vendored Ceres (internal/ceres/trust_region_step_evaluator.cc:38-107), line by
    line, with max_consecutive_nonmonotonic_steps = 0 (use_nonmonotonic_steps is off in all three solves)."""
    max_consecutive_nonmonotonic_steps = 0

    def __init__(self, initial_cost):
        self.minimum_cost = self.current_cost = self.reference_cost = self.candidate_cost = initial_cost
        self.accumulated_reference_model_cost_change = self.accumulated_candidate_model_cost_change = 0.0
        self.num_consecutive_nonmonotonic_steps = 0

    def step_quality(self, cost, model_cost_change):
        relative_decrease = (self.current_cost - cost) / model_cost_change
        historical_relative_decrease = (self.reference_cost - cost) / (self.accumulated_reference_model_cost_change + model_cost_change)
        return max(relative_decrease, historical_relative_decrease)

    def step_accepted(self, cost, model_cost_change):
        self.current_cost = cost
        self.accumulated_candidate_model_cost_change += model_cost_change
        self.accumulated_reference_model_cost_change += model_cost_change
        if self.current_cost < self.minimum_cost:
            self.minimum_cost = self.current_cost
            self.num_consecutive_nonmonotonic_steps = 0
            self.candidate_cost = self.current_cost
            self.accumulated_candidate_model_cost_change = 0.0
        else:
            self.num_consecutive_nonmonotonic_steps += 1
            if self.current_cost > self.candidate_cost:
                self.candidate_cost = self.current_cost
                self.accumulated_candidate_model_cost_change = 0.0
        if self.num_consecutive_nonmonotonic_steps == self.max_consecutive_nonmonotonic_steps:
            self.reference_cost = self.candidate_cost
            self.accumulated_reference_model_cost_change = self.accumulated_candidate_model_cost_change


def test_step_evaluator_follows_ceres_on_a_hand_written_cost_sequence(prog):
    """From cost 10: a decrease to 8 (a new minimum), an increase to 9 (above the candidate), a step to 7 (a new minimum
    again); rho of each from Ceres' formulas, by hand and through the class above.

    What the kernels carry moves the reference to the candidate at EVERY accepted step; Ceres, with no non-monotonic
    step allowed, does so only while every accepted step is a new minimum -- which it is in a solve: a step is accepted
    on rho > 1e-3 with a positive model cost change against a reference that is the current cost. After the increase
    the two differ in the reference (Ceres keeps 8 with 0.5 accumulated, the kernels have 9 with 0) and in nothing else,
    rho of the next step included; the new minimum brings them together again. The reference is compared where they
    agree."""
    steps = [(8.0, 2.5), (9.0, 0.5), (7.0, 1.25)]
    lines = prog("evaluator", 10.0, *[x for s in steps for x in s])
    assert len(lines) == len(steps)
    ev = CeresStepEvaluator(10.0)
    by_hand = [(10.0 - 8.0) / 2.5, (8.0 - 9.0) / 0.5, max((9.0 - 7.0) / 1.25, (8.0 - 7.0) / (0.5 + 1.25))]
    for k, ((cost, mcc), line) in enumerate(zip(steps, lines)):
        rho, minimum, current, reference, candidate, acc_reference, acc_candidate = [float(x) for x in line]
        assert rho == ev.step_quality(cost, mcc) == by_hand[k], (k, rho)
        ev.step_accepted(cost, mcc)
        assert (minimum, current, candidate, acc_candidate) == (ev.minimum_cost, ev.current_cost, ev.candidate_cost,
                                                                ev.accumulated_candidate_model_cost_change), k
        if k != 1:
            assert (reference, acc_reference) == (ev.reference_cost, ev.accumulated_reference_model_cost_change), k
    assert (minimum, current, reference, candidate, acc_reference, acc_candidate) == (7.0, 7.0, 7.0, 7.0, 0.0, 0.0)


def dogleg(prog, alpha, g, gn, radius):
    """g: the (scaled) gradient, gn: the Gauss-Newton step, as vectors; the helper sees their norms and inner product."""
    (line,) = prog("dogleg", float(alpha), float(np.linalg.norm(g)), float(np.linalg.norm(gn)), float(g @ gn), float(radius))
    return [float(x) for x in line]


def test_dogleg_combination_in_its_three_branches(prog):
    g, gn = np.array([3.0, 4.0]), np.array([-1.0, -2.5])
    gnn = float(np.linalg.norm(gn))
    # the Gauss-Newton step lies inside the region: it is the step
    assert dogleg(prog, 0.2, g, gn, 3.0) == [0.0, 1.0, gnn]
    assert dogleg(prog, 0.2, g, gn, gnn) == [0.0, 1.0, gnn]
    # the Cauchy point -alpha g lies outside: the gradient direction cut at the radius
    assert dogleg(prog, 0.2, g, gn, 0.8) == [-(0.8 / 5.0), 0.0, 0.8]
    assert dogleg(prog, 0.2, g, gn, 1.0) == [-(1.0 / 5.0), 0.0, 1.0]
    # between: a + beta (b - a), a = -alpha g, b = gn, on the boundary. Closed form: beta is the positive root of
    # |b - a|^2 beta^2 + 2 a.(b - a) beta + |a|^2 - radius^2 = 0. Both signs of a.(b - a), which the code treats apart.
    for alpha, gn_, radius in [(0.2, gn, 2.0), (0.2, np.array([0.5, -1.4]), 1.2)]:
        a, b = -alpha * g, gn_
        assert np.linalg.norm(a) < radius < np.linalg.norm(b)
        q2, q1, q0 = (b - a) @ (b - a), 2 * a @ (b - a), a @ a - radius * radius
        beta = (-q1 + math.sqrt(q1 * q1 - 4 * q2 * q0)) / (2 * q2)
        ca, cb, norm = dogleg(prog, alpha, g, gn_, radius)
        assert norm < 0                                                     # the caller takes it from the combined step
        assert abs(cb - beta) <= 1e-14 and abs(ca + alpha * (1 - beta)) <= 1e-14 and 0 < beta < 1
        assert abs(np.linalg.norm(ca * g + cb * gn_) - radius) <= 1e-14 * radius
    signs = [np.sign((-0.2 * g) @ (gn_ + 0.2 * g)) for gn_ in (gn, np.array([0.5, -1.4]))]
    assert sorted(signs) == [-1.0, 1.0]


# ---- device: the trace as a C caller of the ABI sees it -----------------------------------------------------------------
# One solve per context, the caller's VioSolveStats filled with 0xff bytes beforehand and read as it comes back (the
# wrappers' dictionaries are cut at `iterations`): the slots below `iterations` are what the context's own parity test
# asks for, the slots from there on are 0 in every array.
def garbage_stats(n=1):
    st = (H.abi.VioSolveStats * n)()
    C.memset(st, 0xff, C.sizeof(st))
    return st


def assert_slots_past_iterations_are_zero(st):
    n = st.iterations
    assert 0 < n < MAX_TRACE
    for k in ARRAYS:
        tail = np.array(getattr(st, k)[n:])
        assert tail.shape == (MAX_TRACE - n,) and np.all(tail == 0), (k, tail)
    assert np.all(np.array(st.it_radius[:n]) > 0)                                                # and the head is a trace


@pytest.mark.gpu
def test_pose_graph_trace_slots_past_iterations_are_zero():
    import test_posegraph as TPG
    d = np.load(TPG.GOLD)
    g, max_iterations = TPG.load_case(d, "small")                                  # the smallest graph of the fixture: 30 keyframes
    o = TPG.pg.PoseGraphOptimizer(max_nodes=32, max_edges=256, n_graphs=1)
    arr, st = (TPG.pg.VioPoseGraph * 1)(), garbage_stats()
    g.fill_struct(arr[0])
    rc = o.lib.vio_posegraph_optimize(o._h, arr, 1, max_iterations, st)
    o.close()
    assert rc == H.abi.VIO_OK
    assert_slots_past_iterations_are_zero(st[0])
    TPG.check_against_golden(d, "small", g, H.abi.stats_to_dict(st[0]), TPG.TOL_GPU)


@pytest.mark.gpu
def test_pnp_trace_slots_past_iterations_are_zero():
    import test_pnp as TP
    cfg = H.abi.default_config()
    name = "n2_fixed0"                                                             # two frames, one fixed: 9 unknowns
    w = TP.EDGE_CASES[name](cfg)
    assert TP.pnp_unknowns(w) == 9
    ref, rs = TP.reference(cfg, name, w)
    solver = H.pkg.pnp.PnpSolver(cfg, max_batch=1)
    got = w.copy()
    arr, st = (H.abi.VioPnpWindow * 1)(), garbage_stats()
    got.fill_struct(arr[0])
    rc = solver.lib.vio_pnp_solve_windows(solver._h, arr, 1, st)
    solver.close()
    assert rc == 0
    assert_slots_past_iterations_are_zero(st[0])
    TP.check_route(got, H.pkg.pnp.stats_dict(st[0]), ref, rs)


WINDOW = "win_tiny_w4_f3"


@pytest.mark.gpu
def test_window_back_end_trace_slots_past_iterations_are_zero():
    cfg, w, d = H.load_golden_window(WINDOW)
    solver = H.pkg.backend.WindowSolver(cfg, max_batch=1)
    got = w.copy()
    arr, st = solver._array([got]), garbage_stats()
    rc = solver.lib.vio_backend_solve_windows(solver._h, arr, 1, 0, st)
    solver.close()
    assert rc == H.abi.VIO_OK
    assert_slots_past_iterations_are_zero(st[0])
    H.check_solution(got, H.abi.stats_to_dict(st[0]), d, tol=1e-6, tol_prior=1e-5)   # (tests/test_backend_gpu.py::test_golden_window)


@pytest.mark.gpu
def test_window_back_end_trace_slots_with_poisoned_device_buffers():
    """The same solve with VIO_AMD_POISON=1: the device's trace arrays hold 0xff patterns wherever the kernel did not
    write. A process of its own: the switch is read once."""
    import sys
    env = dict(os.environ, VIO_AMD_POISON="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "test_window_back_end_trace_slots_past_iterations_are_zero", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
