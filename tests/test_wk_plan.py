"""The window launcher's plan (vins-mobile_amd/csrc/wk_plan.h: plain host C++, no HIP): which windows of a batch run with the pose
matrix in LDS, in which order, at which instantiation, at half or a whole CU of LDS, at which cooperative width and grid. A
stand-alone program (tests/emul/wk_plan.cpp, built with g++ and AddressSanitizer + UndefinedBehaviorSanitizer linked in) answers
one case per line.

The expected answers are a RECORD: the same program, built against a verbatim copy of plan_layout / static_launch_ok / the width
arithmetic of vio_backend_launch as they stood in vio_backend.hip before the plan became a header, printed them. A launch decision
that moves shows here first, without a device."""
import os
import subprocess

import pytest

import capacity_cases as CC
import helpers as H
from helpers import abi

N_CUS = 256


def plan(W, loop, nfeat, peers=2, path="host", profile=0, forced=0, coop_ok=1, active=None, max_features=1000):
    """A `plan` line of the program: dims by the path's growth rule for max_factors 8192, 8 factors per landmark, Ncap = 6 W + 15."""
    act = "-1" if active is None else "%d %s" % (len(active), " ".join(map(str, active)))
    line = "plan %s %d 8192 %d %d %d %d %d %d %d %s %d %s" % (path, max_features, W, loop, N_CUS, peers, profile, forced, coop_ok, act,
                                                             len(nfeat), " ".join(map(str, nfeat)))
    return dict(line=line, W=W, loop=loop, nfeat=list(nfeat), active=list(range(len(nfeat))) if active is None else list(active))


IDENTITY = None  # order: every window in input order
# name: (case, "rc n_lds n_glb variant static_w lds_asp Flds lds_bytes need Flds_glb lds_bytes_glb chunk chunk_glb width grid", order)
# (widths are what the launch asks for, before the runtime's occupancy answer)
CASES = {
    "A": (plan(10, 0, [40, 50, 60, 30]), "0 4 0 3 1 1 60 81920 72272 0 0 256 0 1 0", [3, 0, 1, 2]),
    "B": (plan(10, 0, [186, 100]), "0 2 0 3 1 1 186 81920 81840 0 0 256 0 1 0", [1, 0]),
    # the fat layout one landmark past half a CU, not crowded: a whole CU
    "B1": (plan(10, 0, [187, 100]), "0 2 0 3 1 1 187 163840 82000 0 0 256 0 1 0", [1, 0]),
    "C": (plan(10, 0, [150, 200, 400, 1000]), "0 4 0 3 1 1 1000 163840 151712 0 0 256 0 1 0", [0, 1, 2, 3]),
    # crowded (windows x peers > CUs): the lean layout at half a CU
    "D": (plan(10, 0, [300] * 200), "0 200 0 4 1 0 300 81920 78752 0 0 220 0 1 0", IDENTITY),
    "D1": (plan(10, 0, [300] * 128), "0 128 0 3 1 1 300 163840 90512 0 0 256 0 1 0", IDENTITY),  # not crowded
    "D2": (plan(10, 0, [341] * 200), "0 200 0 3 1 1 341 163840 93696 0 0 256 0 1 0", IDENTITY),  # crowded, lean past half
    "E": (plan(10, 1, [40, 50]), "0 2 0 0 0 1 50 81920 76064 0 0 256 0 1 0", [0, 1]),            # relocalization pose: run-time W
    "F": (plan(12, 0, [60, 172, 173]), "0 3 0 0 0 1 173 163840 96384 0 0 256 0 1 0", [0, 1, 2]),
    "G": (plan(12, 1, [60, 50]), "0 0 2 0 0 1 50 163840 0 60 110320 512 512 4 32", [0, 1]),       # W = 12 with the pose: global matrix
    "H": (plan(13, 0, [60, 50, 40]), "0 0 3 0 0 1 40 163840 0 60 110832 512 512 4 32", [0, 1, 2]),
    "J": (plan(20, 0, [50] * 20), "0 0 20 0 0 1 50 163840 0 50 119408 512 512 2 48", IDENTITY),
    "K": (plan(30, 0, [50] * 20), "0 0 20 0 0 1 50 163840 0 50 132960 512 512 4 96", IDENTITY),
    "L": (plan(30, 0, [50] * 40), "0 0 40 0 0 1 50 163840 0 50 132960 512 512 2 80", IDENTITY),
    "M": (plan(30, 0, [50] * 72), "0 0 72 0 0 1 50 163840 0 50 132960 512 512 1 72", IDENTITY),
    "N": (plan(30, 0, [50] * 72, peers=1), "0 0 72 0 0 1 50 163840 0 50 132960 512 512 2 144", IDENTITY),
    "O": (plan(4, 0, [3, 40]), "0 2 0 0 0 1 40 81920 37936 0 0 114 0 1 0", [0, 1]),
    "P": (plan(30, 0, [1000]), "-4", []),                                                         # VIO_ECAP
    # the stage clock's accumulators cost LDS, and a profiled launch is never cooperative
    "A_prof": (plan(10, 0, [40, 50, 60, 30], profile=1), "0 4 0 3 1 1 60 81920 72784 0 0 256 0 1 0", [3, 0, 1, 2]),
    "K_prof": (plan(30, 0, [50] * 20, profile=1), "0 0 20 0 0 1 50 163840 0 50 133472 512 512 1 20", IDENTITY),
    "K_nocoop": (plan(30, 0, [50] * 20, coop_ok=0), "0 0 20 0 0 1 50 163840 0 50 132960 512 512 1 20", IDENTITY),
    # windows packed on the device: an active list that leaves windows out (one of them the largest), the other growth rule
    "resident": (plan(10, 0, [70, 0, 55, 70, 900, 12, 55], path="resident", active=[0, 2, 3, 5, 6]),
                 "0 5 0 3 1 1 70 81920 73024 0 0 256 0 1 0", [5, 2, 6, 0, 3]),
    "resident_loop": (plan(10, 1, [0, 80, 60, 80], path="resident", active=[3, 1, 2]), "0 3 0 0 0 1 80 81920 78352 0 0 256 0 1 0", [2, 3, 1]),
    # a forced width: taken inside the peers bound, ignored past it (72 x 4 and 40 x 4 workgroups on 128 CUs) and past kCoopMax
    "K_forced2": (plan(30, 0, [50] * 20, forced=2), "0 0 20 0 0 1 50 163840 0 50 132960 512 512 2 48", IDENTITY),
    "K_forced1": (plan(30, 0, [50] * 20, forced=1), "0 0 20 0 0 1 50 163840 0 50 132960 512 512 1 20", IDENTITY),
    "M_forced4": (plan(30, 0, [50] * 72, forced=4), "0 0 72 0 0 1 50 163840 0 50 132960 512 512 1 72", IDENTITY),
    "L_forced4": (plan(30, 0, [50] * 40, forced=4), "0 0 40 0 0 1 50 163840 0 50 132960 512 512 2 80", IDENTITY),
    "J_forced8": (plan(20, 0, [50] * 20, forced=8), "0 0 20 0 0 1 50 163840 0 50 119408 512 512 2 48", IDENTITY),
    "ties": (plan(10, 0, [1000, 30, 1000, 30, 20]), "0 5 0 3 1 1 1000 163840 151712 0 0 256 0 1 0", [4, 1, 3, 0, 2]),
    # the fat layout past a whole CU: the lean one on a whole CU
    "lean_whole": (plan(12, 0, [1000, 30, 1000, 20]), "0 4 0 1 0 0 1000 163840 152816 0 0 256 0 1 0", [3, 1, 0, 2]),
    # both launches: the windows past the LDS variant's reach follow in input order
    "split": (plan(12, 0, [1200, 30, 1010, 1200, 20], max_features=2000), "0 3 2 1 0 0 1010 163840 153648 1200 163840 256 262 4 32",
              [4, 1, 2, 0, 3]),
    "split_res": (plan(12, 0, [1200, 30, 1010, 1200, 20], max_features=2000, path="resident", active=[3, 4, 2]),
                  "0 2 1 1 0 0 1010 163840 153648 1200 163840 256 262 4 32", [4, 2, 3]),
}
FIELDS = "rc n_lds n_glb variant static_w lds_asp Flds lds_bytes need Flds_glb lds_bytes_glb chunk chunk_glb width grid".split()


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    """Lines in, lines out. The sanitizers are linked into the program: it runs as it is, with nothing preloaded."""
    exe = str(tmp_path_factory.mktemp("wk_plan") / "wk_plan")
    # (-Wno-unknown-pragmas, -Wno-psabi: the solver headers under wk_plan.h carry hipcc's `#pragma unroll`, and simt.h returns vectors)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-psabi", "-DVIO_SIMT",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(H.ROOT, "include"),
                           "-I" + os.path.join(H.ROOT, "vins-mobile_amd", "csrc"), "-I" + H.EMUL_DIR, "-o", exe,
                           os.path.join(H.EMUL_DIR, "wk_plan.cpp")])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-3000:]
        got = [ln for ln in out.stdout.split("\n") if ln]
        assert len(got) == len(lines)
        return got
    return run


@pytest.fixture(scope="module")
def answers(prog):
    return dict(zip(CASES, prog([c[0]["line"] for c in CASES.values()])))


def parse(line):
    head, order, traits = line.split("|")
    return dict(zip(FIELDS, map(int, head.split()))), [int(v) for v in order.split()], [int(v) for v in traits.split()]


@pytest.mark.parametrize("name", list(CASES))
def test_plan_equals_the_record_of_the_launcher_it_replaced(answers, name):
    case, head, order = CASES[name]
    if head == "-4":
        assert answers[name] == "%d" % abi.VIO_ECAP
        return
    got, got_order, _ = parse(answers[name])
    assert got == dict(zip(FIELDS, map(int, head.split())))
    assert got_order == (case["active"] if order is IDENTITY else order)


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][1] != "-4"])
def test_properties_of_a_plan(answers, name):
    case = CASES[name][0]
    g, order, traits = parse(answers[name])
    nfeat = case["nfeat"]
    assert sorted(order) == sorted(case["active"]) and g["n_lds"] + g["n_glb"] == len(order)
    lds, glb = order[:g["n_lds"]], order[g["n_lds"]:]
    # ascending landmark counts, ties in input order: the stable sort of the active list
    assert lds == sorted(lds, key=lambda b: (nfeat[b], case["active"].index(b)))
    assert glb == [b for b in case["active"] if b in glb]
    if lds:
        assert max(1, max(nfeat[b] for b in lds)) == g["Flds"]
        assert g["lds_bytes"] in (81920, 163840) and g["need"] <= g["lds_bytes"]
        # the instantiation is the one whose traits are the layout's: matrix in LDS, the coupling where the layout has it, W at
        # compile time exactly when the plan says so
        assert traits == [1, g["lds_asp"], 256, 10 if g["static_w"] else 0]
        assert g["static_w"] == int(case["W"] == 10 and not case["loop"])
    if glb:
        assert max(1, max(nfeat[b] for b in glb)) == g["Flds_glb"] and 81920 < g["lds_bytes_glb"] <= 163840
        assert g["grid"] == (g["n_glb"] if g["width"] == 1 else (g["n_glb"] + 7) // 8 * 8 * g["width"])
    else:
        assert (g["width"], g["grid"]) == (1, 0)


def test_landmarks_at_which_a_layout_leaves_half_a_cu(prog):
    """W = 10, the sizes the comment of the variant table quotes: fat / lean layout, without / with a relocalization pose."""
    assert prog(["walk 10 0 1", "walk 10 1 1", "walk 10 0 0", "walk 10 1 0"]) == ["186", "126", "340", "280"]


def test_capacity_model_of_the_case_tables(prog):
    """tests/capacity_cases.launcher_fcap restates the host-window path's landmark capacity in Python."""
    cfg = abi.default_config()
    Fs = [1, 51, 52, 64, 186, 800, 1000]
    got = prog(["fcap host %d %d %d" % (cfg.max_features, cfg.max_factors, F) for F in Fs])
    assert [int(v) for v in got] == [CC.launcher_fcap(cfg, F) for F in Fs] == [64, 64, 128, 128, 256, 1000, 1000]
    # windows packed on the device: 50 % headroom and a floor of 384 landmarks
    assert prog(["fcap resident 1000 8192 %d" % F for F in (1, 300, 800)]) == ["384", "512", "1000"]
