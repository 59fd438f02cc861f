"""The batched bundle adjustment of estimator start-up (vio_init_ba_*, csrc/sfm_core.h / vio_sfm.hip): the closing "full BA"
of GlobalSFM::construct (inital_sfm.cpp:229-296) for n problems per launch.

CPU: the kernel's own source on the wave64 SIMT emulator (tests/emul/simt_sfm.cpp, 256 fibers per problem, NaN-poisoned
LDS and slabs) against the recordings of the vendored Ceres: tests/golden/init_sfm.npz (the cases of test_initial_sfm.py)
and tests/golden/init_sfm_edges.npz (shape edges, make_init_sfm_edges_golden.py), with the assertions and tolerances of
test_initial_sfm.py::_compare. GPU: the same recordings through vio_init_ba_solve, bit-for-bit determinism across slots,
batches and runs, capacities and arguments, context reuse."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import test_initial_sfm as T

abi = H.abi
init_ba = H.pkg.init_ba
EDGES = os.path.join(H.ROOT, "tests", "golden", "init_sfm_edges.npz")


@pytest.fixture(scope="module")
def emul():
    lib = H.build_emul_lib("simt_sfm.cpp", "libvio_simt_sfm.so", "VIO_SIMT")
    lib.simt_sfm_solve.argtypes = [C.POINTER(abi.VioInitBaProblem), C.c_int, C.POINTER(abi.VioSolveStats), C.c_int, C.c_int]
    return lib


def problem_of(c):
    return init_ba.BaProblem(int(c["F"]), int(c["l"]), c["cq"], c["ct"], c["pts"], c["ok"], c["start"], c["fr"], c["xy"])


def as_run_ba(p, s):
    """A solved problem and its stats in the layout of test_initial_sfm.run_ba."""
    return dict(cq=p.c_rotation, ct=p.c_translation, pts=p.points, ok=p.ok, iterations=s["iterations"], termination=s["termination"],
                initial_cost=s["initial_cost"], final_cost=s["final_cost"], n_ok=s["num_successful_steps"],
                n_bad=s["num_unsuccessful_steps"], it_cost=s["it_cost"], it_radius=s["it_radius"], it_flags=s["it_flags"],
                it_step_norm=s["it_step_norm"], it_gmax=s["it_gradient_max_norm"], it_rho=s["it_relative_decrease"])


def emul_solve(lib, cases, order=0, slab=0):
    ps = [problem_of(c) for c in cases]
    rc, st = init_ba.solve_with(lambda arr, n, s: lib.simt_sfm_solve(arr, n, s, order, slab), ps)
    assert rc == abi.VIO_OK, rc
    return [as_run_ba(p, s) for p, s in zip(ps, st)]


def compare_runaway(got, ref):
    """The assertions of test_initial_sfm.py::test_runaway_landmarks_end_the_same_way."""
    assert int(ref["iterations"]) == 51 and int(ref["termination"]) == 0 and int(ref["ok"]) == 1
    assert got["iterations"] == 51 and got["termination"] == 0 and got["ok"] == 1
    assert np.array_equal(got["it_flags"][:10], ref["it_flags"][:10])
    assert np.abs(got["it_cost"][:10] / ref["it_cost"][:10] - 1).max() < 1e-7
    assert np.abs(got["it_radius"][:10] / ref["it_radius"][:10] - 1).max() < 1e-5
    assert abs(got["final_cost"] / ref["final_cost"] - 1) < 1e-4
    assert np.abs(got["cq"] - ref["cq"]).max() < 1e-4 and np.abs(got["ct"] - ref["ct"]).max() < 1e-3


def edge_cases():
    d = np.load(EDGES)
    names = sorted({k.split("_in_")[0] for k in d.files if "_in_" in k})
    out = []
    for nm in names:
        c = {k[len(nm) + 4:]: d[k] for k in d.files if k.startswith(nm + "_in_")}
        ref = {k[len(nm) + 5:]: d[k] for k in d.files if k.startswith(nm + "_out_")}
        out.append((nm, c, ref))
    return out


EDGE_NAMES = ["f3_l0", "f3_l1", "two_obs", "const_only", "interleaved", "np255", "np257", "first_rejected"]


# ---- CPU: the kernel source on the SIMT emulator -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed,order,slab", [(21, 0, 0), (25, 1, 0), (43, 2, 1)])
def test_emulated_kernel_follows_the_reference_solver(seed, order, slab, emul):
    c, ref = T._golden_case(seed)
    got = emul_solve(emul, [c], order, slab)[0]
    assert ref["n_ok"] >= 3
    T._compare(got, ref)


def test_recorded_step_qualities_stay_far_from_the_accept_threshold():
    """A rejected step has rho <= 1e-3 and an accepted one rho > 1e-3 (min_relative_decrease). Over every recorded
    iteration of the cases compared flag for flag the closest ones are -0.051 below and +0.55 above: the 1e-9-level
    differences a different summation order brings cannot flip a decision."""
    below, above = [], []
    for seed in T.CASES:
        ref = T._golden_case(seed)[1]
        for k in range(1, int(ref["iterations"])):
            if int(ref["it_flags"][k]) & 1:   # a valid step: its rho was compared with the threshold
                (above if int(ref["it_flags"][k]) & 2 else below).append(float(ref["it_rho"][k]))
    assert below and above
    assert max(below) < -0.05 and min(above) > 0.5, (max(below), min(above))
    assert abs(max(below) - (-0.051)) < 1e-3 and abs(min(above) - 0.55) < 1e-2


def test_emulated_kernel_ends_the_runaway_case_the_same_way(emul):
    c, ref = T._golden_case(T.RUNAWAY)
    compare_runaway(emul_solve(emul, [c])[0], ref)


def test_edge_fixture_holds_the_cases_it_is_meant_to():
    cases = {nm: (c, ref) for nm, c, ref in edge_cases()}
    assert sorted(cases) == sorted(EDGE_NAMES)
    assert int(cases["f3_l0"][0]["F"]) == 3 and int(cases["f3_l0"][0]["l"]) == 0
    assert int(cases["f3_l1"][0]["F"]) == 3 and int(cases["f3_l1"][0]["l"]) == 1
    c = cases["two_obs"][0]
    assert np.count_nonzero(np.diff(c["start"])[c["ok"] != 0] == 2) >= np.count_nonzero(c["ok"]) // 3
    c = cases["const_only"][0]
    consts = {int(c["l"]), int(c["F"]) - 1}
    assert any(c["ok"][j] and set(c["fr"][c["start"][j]:c["start"][j + 1]].tolist()) == consts for j in range(len(c["ok"])))
    c = cases["interleaved"][0]
    assert 0 < np.count_nonzero(c["ok"] == 0) and np.any(np.diff(c["ok"].astype(int)) > 0) and np.any(np.diff(c["ok"].astype(int)) < 0)
    assert int(np.count_nonzero(cases["np255"][0]["ok"])) == 255 and int(np.count_nonzero(cases["np257"][0]["ok"])) == 257
    ref = cases["first_rejected"][1]
    assert int(ref["it_flags"][1]) == 1 and int(ref["n_bad"]) > 0     # iteration 1: a valid step that was not accepted
    assert any(int(r["n_bad"]) > 0 for _, r in cases.values()) and all(int(r["ok"]) == 1 for _, r in cases.values())


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_emulated_kernel_on_the_shape_edges(name, emul):
    nm, c, ref = [e for e in edge_cases() if e[0] == name][0]
    T._compare(emul_solve(emul, [c], order=1 if name in ("np255", "np257") else 2)[0], ref)


def test_emulated_kernel_is_independent_of_the_lane_order_and_of_where_the_landmarks_live(emul):
    """Lanes of a wave run one after the other between barriers in the emulator: forward, reverse and shuffled orders give
    the same bits only if no phase reads what another lane of the same phase writes. The LDS and the global-slab variant of
    the landmark state run the same arithmetic."""
    c, _ = T._golden_case(43)
    runs = [emul_solve(emul, [c], order, slab)[0] for order, slab in ((0, 0), (1, 0), (3, 1))]
    for r in runs[1:]:
        for k in runs[0]:
            assert np.array_equal(np.asarray(r[k]), np.asarray(runs[0][k])), k


def test_emulated_batch_handles_no_landmarks_and_checks_arguments(emul):
    c, _ = T._golden_case(21)
    none = dict(c, ok=np.zeros_like(c["ok"]))
    got = emul_solve(emul, [none])[0]
    want = T.run_ba(T._product().vio_init_bundle_adjust, none, True)
    assert got["iterations"] == want["iterations"] == 1 and got["termination"] == want["termination"] == 1 and got["ok"] == want["ok"] == 1
    assert np.array_equal(got["cq"], c["cq"]) and np.array_equal(got["pts"], c["pts"])
    bad = dict(c, fr=c["fr"].copy())
    bad["fr"][3] = 99
    for cs in ([bad], [dict(c, F=1, l=0)]):
        ps = [problem_of(x) for x in cs]
        rc, _ = init_ba.solve_with(lambda arr, n, s: emul.simt_sfm_solve(arr, n, s, 0, 0), ps)
        assert rc == abi.VIO_EINVAL


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
ALL_SEEDS = [43, T.RUNAWAY, 21, 25]     # the 10-iteration problem next to the 51-iteration one


@pytest.fixture(scope="module")
def solver():
    s = init_ba.BaSolver(8, 11, 300, 3000)
    yield s
    s.close()


def _check_goldens(ps, st, seeds):
    for p, s, seed in zip(ps, st, seeds):
        ref = T._golden_case(seed)[1]
        if seed == T.RUNAWAY:
            compare_runaway(as_run_ba(p, s), ref)
        else:
            T._compare(as_run_ba(p, s), ref)


@pytest.mark.gpu
def test_device_follows_the_reference_solver_in_one_launch(solver):
    ps = [problem_of(T._golden_case(s)[0]) for s in ALL_SEEDS]
    st = solver.solve(ps)
    _check_goldens(ps, st, ALL_SEEDS)
    ms, launches = solver.kernel_ms()
    assert launches == 1 and ms > 0
    assert solver.device() >= 0


@pytest.mark.gpu
def test_device_on_the_shape_edges(solver):
    edges = edge_cases()
    ps = [problem_of(c) for _, c, _ in edges]
    st = solver.solve(ps)
    for p, s, (_, _, ref) in zip(ps, st, edges):
        T._compare(as_run_ba(p, s), ref)


@pytest.mark.gpu
def test_device_results_do_not_depend_on_slot_batch_or_run(solver):
    cases = {s: T._golden_case(s)[0] for s in ALL_SEEDS}
    filler = problem_of(cases[25])

    def bits(p, s):
        r = as_run_ba(p, s)
        return {k: np.asarray(v).copy() for k, v in r.items()}

    for seed in ALL_SEEDS:
        runs = []
        p = problem_of(cases[seed])
        runs.append(bits(p, solver.solve([p])[0]))                        # alone
        p = problem_of(cases[seed])
        runs.append(bits(p, solver.solve([p])[0]))                        # twice in a row
        p = problem_of(cases[seed])
        runs.append(bits(p, solver.solve([p] + [filler.copy() for _ in range(3)])[0]))   # slot 0 of a batch
        p = problem_of(cases[seed])
        runs.append(bits(p, solver.solve([problem_of(cases[s]) for s in ALL_SEEDS] + [filler.copy() for _ in range(3)] + [p])[-1]))  # last of 8
        for r in runs[1:]:
            for k in runs[0]:
                assert r[k].tobytes() == runs[0][k].tobytes(), (seed, k)


@pytest.mark.gpu
def test_device_capacity_and_arguments(solver):
    lib = abi.load_product()
    c, _ = T._golden_case(43)
    small = init_ba.BaSolver(2, 11, int(np.count_nonzero(c["ok"])) - 1, 3000)
    try:
        p = problem_of(c)
        rc, _ = small.solve_rc([p])
        assert rc == abi.VIO_ECAP
        assert np.array_equal(p.c_rotation, c["cq"]) and np.array_equal(p.c_translation, c["ct"]) and np.array_equal(p.points, c["pts"])
        rc, _ = small.solve_rc([problem_of(c) for _ in range(3)])
        assert rc == abi.VIO_ECAP
    finally:
        small.close()
    bad = dict(c, fr=c["fr"].copy())
    bad["fr"][3] = 99
    assert solver.solve_rc([problem_of(c), problem_of(bad)])[0] == abi.VIO_EINVAL
    assert solver.solve_rc([problem_of(dict(c, F=1, l=0))])[0] == abi.VIO_EINVAL
    assert solver.solve_rc([])[0] == abi.VIO_OK
    h = C.c_void_p()
    assert lib.vio_init_ba_create(1, abi.VIO_INIT_BA_MAX_FRAMES + 1, 10, 100, C.byref(h)) == abi.VIO_ECAP
    none = dict(c, ok=np.zeros_like(c["ok"]))
    p = problem_of(none)
    s = solver.solve([p])[0]
    assert s["iterations"] == 1 and s["termination"] == 1 and p.ok == 1 and np.array_equal(p.points, c["pts"])


@pytest.mark.gpu
def test_device_context_is_reused_across_batch_sizes():
    s = init_ba.BaSolver(8, 11, 300, 3000)
    try:
        for seeds in ([21], ALL_SEEDS, [25, 43]):
            ps = [problem_of(T._golden_case(x)[0]) for x in seeds]
            _check_goldens(ps, s.solve(ps), seeds)
    finally:
        s.close()
