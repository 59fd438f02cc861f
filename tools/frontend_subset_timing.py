#!/usr/bin/env python3
"""frontend_subset_timing.py [--out profiles/frontend_subset_timing.txt] -- device time per front-end step of the lock-step call
(vio_frontend_step_resident) and of the subset call (vio_frontend_submit_subset, device frames) at n = 512, 256, 64 and 1 called
sequences, on one context of 512 sequences of 640 x 480 / 150 corners, every called sequence published on every step.

The arms alternate inside one process: every repetition runs each arm once, in an order that rotates, from a reset context
(vio_frontend_reset, so every arm tracks the same frames from the same start), WARM steps unmeasured and then STEPS measured. The
time is the context's own event pair around the step's launches (vio_frontend_kernel_ms); for the subset call that includes the
upload of the call's plan, and in neither arm the copy of the observations. The record states the mean and the spread (max - min
over the repetitions) of every arm, how n = 512 compares with lock-step, and whether the time falls with n."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, ROWS, COLS, CORNERS = 512, 480, 640, 150
T, WARM, STEPS, REPS = 4, 3, 10, 5
SUBSET_N = (512, 256, 64, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_subset_timing.txt"))
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("vins-mobile_amd")
    abi, synth = pkg.abi, pkg.synth
    cfg = abi.default_config(max_corners=CORNERS, min_dist=30, image_rows=ROWS, image_cols=COLS)
    base = [synth.make_image_stream(100 + k, T, rows=ROWS, cols=COLS)[0] for k in range(8)]  # eight scenes, tiled over the sequences
    frames = np.stack([base[s % 8] for s in range(S)], axis=1)  # [T][S][rows][cols]
    trk = pkg.frontend.FeatureTracker(cfg, n_seq=S)
    trk.upload_frames(frames)
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    px = ROWS * COLS
    order = [0, 1, 2, 3, 2, 1]  # the view moves back and forth: no jump where the frames run out

    def run(arm, steps):
        for k in range(steps):
            f = order[run.k % len(order)]
            run.k += 1
            if arm == "lock-step":
                trk.step(f, True)
            else:
                seqs = np.arange(arm, dtype=np.int32)
                trk.submit_subset(seqs, dev.data_ptr() + f * S * px, 1, seqs)  # slot = sequence
                trk.collect_subset()
        trk.sync()

    arms = ["lock-step"] + list(SUBSET_N)
    times = {a: [] for a in arms}
    for rep in range(REPS):
        for a in arms[rep % len(arms):] + arms[:rep % len(arms)]:
            trk.reset()
            run.k = 0
            run(a, WARM)
            trk.kernel_ms()
            run(a, STEPS)
            ms, n = trk.kernel_ms()
            assert n == STEPS, (a, n)
            times[a].append(ms)
    trk.close()
    name = lambda a: a if a == "lock-step" else "subset n = %d" % a
    mean = {a: float(np.mean(times[a])) for a in arms}
    spread = {a: float(np.max(times[a]) - np.min(times[a])) for a in arms}
    lines = ["%s on %s" % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             "%d sequences of %d x %d / %d corners, device-resident frames, every called sequence published on every step;" % (S, COLS, ROWS, CORNERS),
             "%d repetitions, arms alternating in one process, each from a reset context: %d warm-up steps, then the mean device time" % (REPS, WARM),
             "(ms) of %d steps. lock-step = vio_frontend_step_resident (level 0 read in place from the context's ring);" % STEPS,
             "subset = vio_frontend_submit_subset with frames_on_device (plan upload + kernels; level 0 copied into the pyramid).", "",
             "%-16s %s   %9s %9s" % ("arm", " ".join("%8s" % ("rep %d" % r) for r in range(REPS)), "mean", "spread")]
    for a in arms:
        lines.append("%-16s %s   %9.4f %9.4f" % (name(a), " ".join("%8.4f" % v for v in times[a]), mean[a], spread[a]))
    d = mean[512] - mean["lock-step"]
    lines += ["", "subset n = 512 against lock-step: %+.4f ms (%+.1f %%); spreads %.4f and %.4f ms" % (d, 100 * d / mean["lock-step"], spread[512], spread["lock-step"]),
              "time against n: " + ", ".join("n = %d: %.4f ms (%.2f us per called sequence)" % (n, mean[n], 1e3 * mean[n] / n) for n in SUBSET_N),
              "the time %s with n" % ("falls" if all(mean[SUBSET_N[i]] > mean[SUBSET_N[i + 1]] for i in range(len(SUBSET_N) - 1)) else "does NOT fall monotonically")]
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt)
    print(txt)


if __name__ == "__main__":
    main()
