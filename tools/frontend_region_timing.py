#!/usr/bin/env python3
"""frontend_region_timing.py [--out profiles/frontend_region_timing.txt] [--parent-json FILE ...] -- what the region of interest
(vio_frontend_set_regions) costs the front-end step, and what the valid region of a lens costs once.

Front end: one context of 512 sequences of 640 x 480 / 150 corners, device time of vio_frontend_step_resident from the context's
own event pair (vio_frontend_kernel_ms), every step published. Arms, alternating inside one process, every repetition each arm
once in an order that rotates, from a reset context, WARM steps unmeasured and then STEPS measured:
  none        no sequence holds a region: the kernels as they always were
  all-usable  a region of all 255 on every sequence: the pure cost of the REGION variants
  fisheye     the margin-12 valid region of a fisheye lens on every sequence
Against the parent commit: run this tool from a checkout of the parent with `--arms none --json FILE` (it measures the same
workload with that checkout's library; the parent has no regions, so only that arm exists there), in turn with runs of this
checkout, and hand the files to `--parent-json`: the record then states both means and spreads.
Per kernel (detect, corner_select, track_update): `--trace-arm ARM` runs that arm alone, STEPS steps, for a kernel trace
taken around the process (rocprofv3 --kernel-trace --stats -- python tools/frontend_region_timing.py --trace-arm ARM); the
record of such a trace is appended by hand under the table.

Valid regions: vio_preprocess_valid_regions_resident for 512 fisheye slots at 640 x 480, margin 12 (wall time around the call and
its synchronisation, the launch being the only work), against vio_lens_model_valid_region on one host thread for one slot."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, ROWS, COLS, CORNERS = 512, 480, 640, 150
T, WARM, STEPS, REPS = 4, 3, 10, 5
MARGIN = 12
ARMS = ("none", "all-usable", "fisheye")


def fisheye(abi):
    """A 120-degree-class fisheye rectified at a focal length short enough that corners and edges look outside the frame."""
    f = 0.45 * COLS
    return abi.make_lens_model(abi.VIO_LENS_FISHEYE, f, f, COLS / 2 - 1.3, ROWS / 2 + 0.7, (0.021, -0.0043, 0.0011, -0.0002),
                               (0.3 * COLS, 0.3 * COLS, COLS / 2 - 0.5, ROWS / 2 - 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_region_timing.txt"))
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--json", help="write the repetitions' times here and no record")
    ap.add_argument("--parent-json", nargs="*", default=[], help="files a parent checkout wrote with --arms none --json")
    ap.add_argument("--trace-arm", help="run this arm alone (for a kernel trace around the process)")
    args = ap.parse_args()
    arms = [args.trace_arm] if args.trace_arm else args.arms.split(",")
    import torch
    pkg = importlib.import_module("vins-mobile_amd")
    abi, synth = pkg.abi, pkg.synth
    cfg = abi.default_config(max_corners=CORNERS, min_dist=30, image_rows=ROWS, image_cols=COLS)
    base = [synth.make_image_stream(100 + k, T, rows=ROWS, cols=COLS)[0] for k in range(8)]  # eight scenes, tiled over the sequences
    frames = np.stack([base[s % 8] for s in range(S)], axis=1)  # [T][S][rows][cols]
    trk = pkg.frontend.FeatureTracker(cfg, n_seq=S)
    trk.upload_frames(frames)
    order = [0, 1, 2, 3, 2, 1]  # the view moves back and forth: no jump where the frames run out
    seqs = np.arange(S, dtype=np.int32)
    regions, usable = {}, {}
    if "all-usable" in arms:
        regions["all-usable"] = np.full((1, ROWS, COLS), 255, np.uint8)
    if "fisheye" in arms:
        regions["fisheye"] = abi.lens_model_valid_region(fisheye(abi), None, ROWS, COLS, MARGIN)[None]
    for a, m in regions.items():
        usable[a] = float((m != 0).mean())

    def select(arm):
        if arm == "none":
            if hasattr(trk, "set_regions"):
                assert trk.set_regions(seqs, None) == abi.VIO_OK
        else:  # one mask image for every sequence
            assert trk.set_regions(seqs, regions[arm], mask_index=np.zeros(S, np.int32)) == abi.VIO_OK

    def run(steps):
        for _ in range(steps):
            trk.step(order[run.k % len(order)], True)
            run.k += 1
        trk.sync()

    times = {a: [] for a in arms}
    for rep in range(1 if args.trace_arm else REPS):
        for a in arms[rep % len(arms):] + arms[:rep % len(arms)]:
            select(a)
            trk.reset()
            run.k = 0
            run(WARM)
            trk.kernel_ms()
            run(STEPS)
            ms, n = trk.kernel_ms()
            assert n == STEPS, (a, n)
            times[a].append(ms)
    trk.close()
    if args.trace_arm:
        print("ran %s: %d warm-up and %d measured steps, %.4f ms per step" % (args.trace_arm, WARM, STEPS, times[args.trace_arm][0]))
        return
    if args.json:
        json.dump(times, open(args.json, "w"))
        print(times)
        return
    mean = {a: float(np.mean(times[a])) for a in arms}
    spread = {a: float(np.max(times[a]) - np.min(times[a])) for a in arms}
    lines = ["%s on %s" % (os.path.basename(__file__), torch.cuda.get_device_name(0)),
             "%d sequences of %d x %d / %d corners, device-resident frames, every step published (vio_frontend_step_resident);" % (S, COLS, ROWS, CORNERS),
             "%d repetitions, arms alternating in one process, each from a reset context: %d warm-up steps, then the mean device time" % (REPS, WARM),
             "(ms) of %d steps. spread = max - min over the repetitions." % STEPS, "",
             "%-22s %s   %9s %9s" % ("arm", " ".join("%8s" % ("rep %d" % r) for r in range(REPS)), "mean", "spread")]
    for a in arms:
        note = "" if a == "none" else "   (%.1f %% of the pixels usable)" % (100 * usable[a])
        lines.append("%-22s %s   %9.4f %9.4f%s" % (a, " ".join("%8.4f" % v for v in times[a]), mean[a], spread[a], note))
    parent = [v for f in args.parent_json for v in json.load(open(f))["none"]]
    if parent:
        pm, ps = float(np.mean(parent)), float(np.max(parent) - np.min(parent))
        lines += ["%-22s %s   %9.4f %9.4f   (%d processes of the parent's checkout, run in turn with this one's)" %
                  ("parent commit, none", " ".join("%8.4f" % v for v in parent[:REPS]), pm, ps, len(args.parent_json)),
                  "", "no region against the parent: %+.4f ms (%+.2f %%); spreads %.4f (this) and %.4f ms (parent): %s the parent's spread" %
                  (mean["none"] - pm, 100 * (mean["none"] - pm) / pm, spread["none"], ps,
                   "inside" if abs(mean["none"] - pm) <= ps else "OUTSIDE")]
    else:
        lines += ["", "no region against the parent: not measured in this run (no --parent-json)"]
    for a in arms:
        if a != "none" and "none" in mean:
            d = mean[a] - mean["none"]
            lines.append("%s against none: %+.4f ms (%+.2f %% of the step)" % (a, d, 100 * d / mean["none"]))
    # the valid regions of 512 fisheye slots, once
    pp = pkg.frontend.Preprocessor(ROWS, COLS, max_frames=S)
    assert pp.set_lens_models(seqs, [fisheye(abi)] * S) == abi.VIO_OK
    d_masks = torch.zeros((S, ROWS, COLS), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dev_ms = []
    for _ in range(REPS + 1):
        t0 = time.perf_counter()
        assert pp.valid_regions_resident(seqs, MARGIN, d_masks.data_ptr()) == abi.VIO_OK
        pp.sync()
        dev_ms.append(1e3 * (time.perf_counter() - t0))
    dev_ms = dev_ms[1:]  # (the first call loads the kernel)
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        one = abi.lens_model_valid_region(fisheye(abi), None, ROWS, COLS, MARGIN)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(d_masks[0].cpu().numpy(), one)
    pp.close()
    lines += ["", "valid regions (a one-off cost per lens): vio_preprocess_valid_regions_resident, %d fisheye slots, margin %d:" % (S, MARGIN),
              "  device, call + wait: mean %.3f ms, spread %.3f ms over %d calls (%.2f us per slot)" %
              (np.mean(dev_ms), np.max(dev_ms) - np.min(dev_ms), len(dev_ms), 1e3 * np.mean(dev_ms) / S),
              "  host entry vio_lens_model_valid_region, one thread, ONE slot: mean %.1f ms, spread %.1f ms over %d calls (%d slots: %.1f s)" %
              (np.mean(host_ms), np.max(host_ms) - np.min(host_ms), len(host_ms), S, S * np.mean(host_ms) / 1e3)]
    txt = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt)
    print(txt)


if __name__ == "__main__":
    main()
