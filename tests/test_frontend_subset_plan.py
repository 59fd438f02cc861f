"""The planner of the front end's subset calls (vins-mobile_amd/csrc/fe_subset.h: plain host C++, no HIP) against a Python model of
the per-sequence phase: a stand-alone program (tests/emul/fe_subset_plan.cpp, built with g++) runs schedules of calls and
resets and prints the phase bits, the launch lists and the verdict on the arguments after every command."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fe_subset") / "fe_subset_plan")
    csrc = os.path.join(H.ROOT, "vins-mobile_amd", "csrc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + csrc, "-o", exe,
                           os.path.join(H.EMUL_DIR, "fe_subset_plan.cpp")])

    def run(n_seq, commands):
        out = subprocess.run([exe], input="%d\n%s\n" % (n_seq, "\n".join(commands)), check=True, capture_output=True, text=True)
        return [ln for ln in out.stdout.split("\n") if ln]
    return run


class Model:
    """FeatureTracker's phase per sequence (feature_tracker.cpp:165-170, :284): a sequence without an image takes its frame
    into its current bank (pre = cur = forw), one with an image into the other bank, which then is the current one."""

    def __init__(self, n_seq):
        self.bank, self.have = [0] * n_seq, [0] * n_seq

    def call(self, seq, publish, frame_index=None):
        prev = [self.bank[s] if self.have[s] else -1 for s in seq]
        forw = [1 - self.bank[s] if self.have[s] else self.bank[s] for s in seq]
        for s, f in zip(seq, forw):
            self.bank[s], self.have[s] = f, 1
        slot = list(frame_index) if frame_index is not None else list(range(len(seq)))
        return [list(seq), slot, prev, forw, [int(bool(p)) for p in publish], [i for i, p in enumerate(publish) if p]]

    def reset(self, seq=None):
        for s in (range(len(self.bank)) if seq is None else seq):
            self.bank[s] = self.have[s] = 0

    def in_step(self):
        return int(len(set(zip(self.bank, self.have))) == 1)

    def line(self, lists=None):
        txt = "ok %d %s %s" % (self.in_step(), " ".join(map(str, self.bank)), " ".join(map(str, self.have)))
        for row in lists or []:
            txt += " |" + "".join(" %d" % v for v in row)
        return txt


def call_cmd(seq, publish, frame_index=None):
    fi = list(frame_index) if frame_index is not None else []
    return "call %d %s %s %d %s" % (len(seq), " ".join(map(str, seq)), " ".join(map(str, publish)), len(fi), " ".join(map(str, fi)))


@pytest.mark.parametrize("n_seq,seed", [(1, 0), (5, 1), (5, 2), (17, 3), (64, 4)])
def test_phase_bits_and_lists_after_random_schedules(prog, n_seq, seed):
    rng = np.random.default_rng(seed)
    model, cmds, want = Model(n_seq), [], []
    for _ in range(120):
        kind = rng.integers(0, 10)
        if kind == 0:
            model.reset()
            cmds.append("reset -1")
            want.append(model.line())
        elif kind == 1:
            seq = list(rng.permutation(n_seq)[: rng.integers(0, n_seq + 1)])
            model.reset(seq)
            cmds.append("reset %d %s" % (len(seq), " ".join(map(str, seq))))
            want.append(model.line())
        else:
            n = int(rng.integers(0, n_seq + 1))
            seq = [int(s) for s in rng.permutation(n_seq)[:n]]
            publish = [int(p) for p in rng.integers(0, 2, n)]
            fi = [int(f) for f in rng.integers(0, 1000, n)] if rng.integers(0, 2) else None
            cmds.append(call_cmd(seq, publish, fi))
            want.append(model.line(model.call(seq, publish, fi)))
    assert prog(n_seq, cmds) == want


def test_issue_schedule_puts_sequences_in_opposite_banks(prog):
    """Sequence 0 every tick, sequence 1 every second tick: their current banks differ after tick 2, which one shared bank
    index cannot express."""
    got = prog(2, [call_cmd([0, 1], [1, 1]), call_cmd([0], [0]), call_cmd([1, 0], [0, 1])])
    assert got[0] == "ok 1 0 0 1 1 | 0 1 | 0 1 | -1 -1 | 0 0 | 1 1 | 0 1"
    assert got[1] == "ok 0 1 0 1 1 | 0 | 0 | 0 | 1 | 0 |"
    assert got[2] == "ok 0 0 1 1 1 | 1 0 | 0 1 | 0 1 | 1 0 | 0 1 | 1"


def test_rejections_leave_the_phase_alone(prog):
    first = call_cmd([0, 2], [1, 0])
    bad = ["call 2 1 1 0 0 0",          # duplicate
           "call 1 3 1 0",              # out of range
           "call 1 -1 1 0",             # negative
           "call 4 0 1 2 0 0 0 0 0 0",  # more entries than sequences (and a duplicate)
           "call 2 0 1 x x 0",          # publish == NULL with n > 0
           "call 2 0 1 1 1 2 0 -4",     # negative frame slot
           "reset 2 1 1", "reset 1 3"]
    got = prog(3, [first] + bad + ["call 0 0", "reset 0", first])
    state = "0 0 0 0 1 0 1"  # in_step, bank[3], have[3] behind the first call (a first frame stays in the current bank)
    assert got[0].startswith("ok " + state + " |")
    assert got[1:1 + len(bad)] == ["bad " + state] * len(bad)
    assert got[-3] == "ok " + state + " | | | | | |"   # n = 0: a valid call that plans nothing
    assert got[-2] == "ok " + state
    assert got[-1] == "ok 0 1 0 1 1 0 1 | 0 2 | 0 1 | 0 0 | 1 1 | 1 0 | 0"


def test_in_step_returns_with_a_reset_of_all(prog):
    got = prog(3, [call_cmd([0, 1, 2], [1, 1, 1]), call_cmd([1], [0]), "reset 1 1", "reset -1", call_cmd([2, 1, 0], [0, 0, 0])])
    assert [ln.split()[1] for ln in got] == ["1", "0", "0", "1", "1"]
