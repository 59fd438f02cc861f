"""The batched bundle adjustment beyond 16 frames (vio_init_ba_*, csrc/sfm_core.h: the large layout -- reduced camera matrix
packed in LDS, 512 work-items, diagonal camera blocks and landmarks in global slabs), up to VIO_INIT_BA_MAX_FRAMES = 32.

Expected values: tests/golden/init_sfm_large.npz, recorded by tests/golden/make_init_sfm_large_golden.py from the vendored
Ceres (oracle/_ref) at 17, 21, 31 and 32 frames, compared with test_initial_sfm._compare and its tolerances as they stand.
CPU: the kernel's own source on the SIMT emulator (tests/emul/simt_sfm_large.cpp: 512 fibers per problem, LDS of exactly the
large layout's byte count, LDS and slabs NaN-poisoned), the host solver on the same cases, the 11-frame goldens forced
through the large layout, lane orders, capacities. GPU: the recordings through vio_init_ba_solve, bit reproducibility
across the split of a mixed batch, capacities, context reuse. (No estimator test: the estimator's switch keeps its bound of
16 frames, see vio_estimator_set_init_device in include/vio_amd.h.)"""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import test_initial_sfm as T

abi = H.abi
init_ba = H.pkg.init_ba
LARGE = os.path.join(H.ROOT, "tests", "golden", "init_sfm_large.npz")
NAMES = ["f17", "f21", "f31", "f32_last", "f32_far", "f17_np257"]
FRAMES_L = {"f17": (17, 3), "f21": (21, 4), "f31": (31, 5), "f32_last": (32, 31), "f32_far": (32, 6), "f17_np257": (17, 3)}

_CASES = {}


def large_cases():
    """name -> (inputs, recorded reference run); loaded once, never modified."""
    if not _CASES:
        d = np.load(LARGE)
        for nm in sorted({k.split("_in_")[0] for k in d.files if "_in_" in k}):
            c = {k[len(nm) + 4:]: d[k] for k in d.files if k.startswith(nm + "_in_")}
            ref = {k[len(nm) + 5:]: d[k] for k in d.files if k.startswith(nm + "_out_")}
            _CASES[nm] = (c, ref)
    return _CASES


@pytest.fixture(scope="module")
def emul():
    lib = H.build_emul_lib("simt_sfm_large.cpp", "libvio_simt_sfm_large.so", "VIO_SIMT")
    lib.simt_sfm_large_solve.argtypes = [C.POINTER(abi.VioInitBaProblem), C.c_int, C.POINTER(abi.VioSolveStats), C.c_int, C.c_int]
    lib.simt_sfm_large_lds_bytes.argtypes, lib.simt_sfm_large_lds_bytes.restype = [C.c_int], C.c_long
    return lib


def problem_of(c):
    return init_ba.BaProblem(int(c["F"]), int(c["l"]), c["cq"], c["ct"], c["pts"], c["ok"], c["start"], c["fr"], c["xy"])


def as_run_ba(p, s):
    """A solved problem and its stats in the layout of test_initial_sfm.run_ba."""
    return dict(cq=p.c_rotation, ct=p.c_translation, pts=p.points, ok=p.ok, iterations=s["iterations"], termination=s["termination"],
                initial_cost=s["initial_cost"], final_cost=s["final_cost"], n_ok=s["num_successful_steps"],
                n_bad=s["num_unsuccessful_steps"], it_cost=s["it_cost"], it_radius=s["it_radius"], it_flags=s["it_flags"],
                it_step_norm=s["it_step_norm"], it_gmax=s["it_gradient_max_norm"], it_rho=s["it_relative_decrease"])


def emul_solve(lib, cases, order=0, force=0):
    ps = [problem_of(c) for c in cases]
    rc, st = init_ba.solve_with(lambda arr, n, s: lib.simt_sfm_large_solve(arr, n, s, order, force), ps)
    assert rc == abi.VIO_OK, rc
    return [as_run_ba(p, s) for p, s in zip(ps, st)]


def bits(r):
    return {k: np.asarray(v).copy().tobytes() for k, v in r.items()}


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_large_fixture_holds_the_cases_it_is_meant_to():
    cases = large_cases()
    assert sorted(cases) == sorted(NAMES)
    for nm, (F, l) in FRAMES_L.items():
        c, ref = cases[nm]
        assert (int(c["F"]), int(c["l"])) == (F, l), nm
        assert int(ref["termination"]) == 1 and int(ref["ok"]) == 1 and int(ref["n_ok"]) >= 3, nm
        assert int(np.count_nonzero(c["ok"])) <= 300 and int(np.diff(c["start"])[c["ok"] != 0].sum()) <= 4000, nm   # the GPU tests' context
    c = cases["f32_last"][0]       # l = F - 1: every other frame has both blocks free, 6 F - 6 columns
    assert 6 * (int(c["F"]) - 1) == 186 and int(c["l"]) == int(c["F"]) - 1
    assert int(np.count_nonzero(cases["f17_np257"][0]["ok"])) == 257
    assert sum(int(ref["n_bad"]) > 0 for _, ref in cases.values()) >= 2
    assert any(int(ref["it_flags"][1]) == 1 for _, ref in cases.values())     # iteration 1: a valid step that was not accepted


def test_large_recorded_step_qualities_stay_far_from_the_accept_threshold():
    """Every valid step's relative decrease lies at least 0.05 from min_relative_decrease = 1e-3, on either side: the
    1e-9-level differences another summation order brings cannot flip a decision (the margin test_init_ba.py asserts for the
    11-frame cases)."""
    for nm, (_, ref) in large_cases().items():
        rho = [float(ref["it_rho"][k]) for k in range(1, int(ref["iterations"])) if int(ref["it_flags"][k]) & 1]
        assert rho and min(abs(r - 1e-3) for r in rho) >= 0.05, (nm, rho)
        for k in range(1, int(ref["iterations"])):
            if int(ref["it_flags"][k]) & 1:
                assert (float(ref["it_rho"][k]) > 1e-3) == bool(int(ref["it_flags"][k]) & 2)


@pytest.mark.parametrize("name", NAMES)
def test_emulated_large_layout_follows_the_reference_solver(name, emul):
    c, ref = large_cases()[name]
    T._compare(emul_solve(emul, [c], order={"f17": 1, "f31": 2}.get(name, 0))[0], ref)


@pytest.mark.parametrize("name", NAMES)
def test_host_solver_follows_the_reference_solver_beyond_11_frames(name):
    c, ref = large_cases()[name]
    T._compare(T.run_ba(T._product().vio_init_bundle_adjust, c, True), ref)


@pytest.mark.parametrize("seed", T.CASES)
def test_11_frame_goldens_forced_through_the_large_layout(seed, emul):
    c, ref = T._golden_case(seed)
    T._compare(emul_solve(emul, [c], order=seed % 3, force=1)[0], ref)


def test_emulated_large_layout_is_independent_of_the_lane_order(emul):
    """Forward, reverse and shuffled lane orders give the same bits only if no phase reads what another lane of the same
    phase writes: the reductions' scratch on top of the reduced matrix and the camera blocks in global memory included."""
    c, _ = large_cases()["f21"]
    runs = [bits(emul_solve(emul, [c], order)[0]) for order in (0, 1, 3)]
    assert runs[1] == runs[0] and runs[2] == runs[0]


def test_emulated_mixed_batch_is_split_by_each_problems_own_frame_count(emul):
    """An 11-frame problem next to a 17-frame one runs the small layout (the bits of the unchanged driver of
    test_init_ba.py), the 17-frame one the bits it gives alone."""
    small_c, big_c = T._golden_case(21)[0], large_cases()["f17"][0]
    old = H.build_emul_lib("simt_sfm.cpp", "libvio_simt_sfm.so", "VIO_SIMT")
    old.simt_sfm_solve.argtypes = [C.POINTER(abi.VioInitBaProblem), C.c_int, C.POINTER(abi.VioSolveStats), C.c_int, C.c_int]
    p = problem_of(small_c)
    rc, st = init_ba.solve_with(lambda arr, n, s: old.simt_sfm_solve(arr, n, s, 0, 0), [p])
    assert rc == abi.VIO_OK
    mixed = emul_solve(emul, [big_c, small_c])
    assert bits(mixed[1]) == bits(as_run_ba(p, st[0]))
    assert bits(mixed[0]) == bits(emul_solve(emul, [big_c])[0])


def test_large_layout_lds_and_frame_capacity(emul):
    """The large layout's dynamic LDS at 32 frames is the sum DESIGN section 7 gives and fits one workgroup; check_problem
    accepts 32 frames and refuses 33 with VIO_ECAP before anything is written."""
    assert abi.VIO_INIT_BA_MAX_FRAMES == 32
    assert emul.simt_sfm_large_lds_bytes(32) == 139128 + 10416 + 5888 + 1504 <= 160 * 1024
    assert emul.simt_sfm_large_lds_bytes(31) < emul.simt_sfm_large_lds_bytes(32)
    F = 33
    c = dict(F=F, l=2, cq=np.tile([1.0, 0, 0, 0], (F, 1)), ct=np.zeros((F, 3)), pts=np.ones((2, 3)), ok=np.ones(2, np.uint8),
             start=np.array([0, 2, 4], np.int32), fr=np.array([0, 32, 1, 5], np.int32), xy=np.zeros((4, 2)))
    p = problem_of(c)
    rc, _ = init_ba.solve_with(lambda arr, n, s: emul.simt_sfm_large_solve(arr, n, s, 0, 0), [p])
    assert rc == abi.VIO_ECAP
    assert np.array_equal(p.c_rotation, c["cq"]) and np.array_equal(p.c_translation, c["ct"]) and np.array_equal(p.points, c["pts"])
    # ... and behind a good 32-frame problem of the same call: nothing of either is touched
    good = large_cases()["f32_last"][0]
    g = problem_of(good)
    rc, _ = init_ba.solve_with(lambda arr, n, s: emul.simt_sfm_large_solve(arr, n, s, 0, 0), [g, p])
    assert rc == abi.VIO_ECAP and np.array_equal(g.c_rotation, good["cq"]) and np.array_equal(g.points, good["pts"])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
SMALL_SEEDS = [21, 43]


@pytest.fixture(scope="module")
def solver():
    s = init_ba.BaSolver(8, 32, 300, 4000)
    yield s
    s.close()


def _check(ps, st, refs):
    for p, s, ref in zip(ps, st, refs):
        T._compare(as_run_ba(p, s), ref)


def _batch(names_or_seeds):
    """Problems and references of recorded cases: a name of NAMES, or a seed of the 11-frame goldens."""
    got = [large_cases()[x] if isinstance(x, str) else T._golden_case(x) for x in names_or_seeds]
    return [problem_of(c) for c, _ in got], [ref for _, ref in got]


@pytest.mark.gpu
def test_device_follows_the_reference_solver_beyond_16_frames_in_one_launch(solver):
    ps, refs = _batch(NAMES)
    st = solver.solve(ps)
    _check(ps, st, refs)
    ms, launches = solver.kernel_ms()
    assert launches == 1 and ms > 0


@pytest.mark.gpu
def test_device_results_do_not_depend_on_slot_batch_or_run_across_the_split(solver):
    cases = large_cases()

    def run(batch, slot):
        ps, _ = _batch(batch)
        st = solver.solve(ps)
        return bits(as_run_ba(ps[slot], st[slot]))

    alone = run(["f31"], 0)
    assert run(["f31"], 0) == alone                                           # twice in a row
    assert run(["f31", 21, 43, 25], 0) == alone                               # slot 0 of a batch that also holds 11-frame problems
    solver.kernel_ms()
    assert run([21, "f17", 43, 25, "f21", 21, 43, "f31"], 7) == alone         # the last slot of 8
    assert solver.kernel_ms()[1] == 2                                         # one launch per layout
    small_alone = run([43], 0)
    assert run([43, "f31"], 0) == small_alone and run(["f31", 43], 1) == small_alone
    assert cases["f31"][0]["F"] == 31


@pytest.mark.gpu
def test_device_frame_capacities(solver):
    lib = abi.load_product()
    h = C.c_void_p()
    assert lib.vio_init_ba_create(1, abi.VIO_INIT_BA_MAX_FRAMES + 1, 10, 100, C.byref(h)) == abi.VIO_ECAP
    assert abi.VIO_INIT_BA_MAX_FRAMES == 32 and solver.device() >= 0            # (the module's context was created with 32)
    c = large_cases()["f21"][0]
    small = init_ba.BaSolver(2, 16, 300, 4000)
    try:
        p, q = problem_of(c), problem_of(T._golden_case(21)[0])
        rc, _ = small.solve_rc([q, p])
        assert rc == abi.VIO_ECAP
        assert np.array_equal(p.c_rotation, c["cq"]) and np.array_equal(p.c_translation, c["ct"]) and np.array_equal(p.points, c["pts"])
        assert np.array_equal(q.c_rotation, T._golden_case(21)[0]["cq"]) and np.array_equal(q.points, T._golden_case(21)[0]["pts"])
    finally:
        small.close()


@pytest.mark.gpu
def test_device_context_is_reused_across_layouts():
    s = init_ba.BaSolver(8, 32, 300, 4000)
    try:
        for batch in (SMALL_SEEDS, ["f32_last", "f17"], [21, "f21", 43, "f32_far"], ["f17_np257"], [25]):
            ps, refs = _batch(batch)
            _check(ps, s.solve(ps), refs)
    finally:
        s.close()
