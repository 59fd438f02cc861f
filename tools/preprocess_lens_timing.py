#!/usr/bin/env python3
"""Device time of the image pre-step (vio_preprocess_run_resident, from vio_preprocess_kernel_ms) for 512 RGBA 640x480 frames
resident in device memory, with and without lens rectification:

  (a) the parent commit's library     --parent-lib PATH/libvio_amd.so, built from the commit before lenses existed (skipped,
                                      and said so, when the option is not given)
  (b) this library, no lens set       the kernel without the lens branch
  (c) this library, a lens in every slot
  (d) this library, a lens in every other slot (one launch: lens or no lens is chosen per frame)
  (p) the parent commit's library with that lens in every slot (when it has vio_preprocess_set_lenses)
and, with --model, the lens models of VioLensModel next to them in the same rounds:
  (e) a rational lens in every slot    (f) a fisheye lens in every slot
  (g) mixed: slot k holds no lens, the Brown-Conrady, the rational, the fisheye lens for k % 4 = 0, 1, 2, 3

One context per variant, all on the same input; 10 launches of warm-up each, then --rounds rounds in which the variants take
turns, --reps launches each (one event pair per launch): per variant the median over the rounds with the minimum and the maximum
beside it, the spread of (a) as the yardstick for (b) against (a), and the achieved bytes per second against the 7 * rows * cols
bytes per RGBA frame of the header comment of csrc/vio_preprocess.hip. The outputs are compared as well: (b) equals (a), the slots
of (d) equal (c)'s or (b)'s, those of (g) the variant's of their model. Needs a gfx950 device; writes
profiles/preprocess_lens_timing.txt, or profiles/preprocess_lens_models_timing.txt when --model names another model than brown.

    python tools/preprocess_lens_timing.py [--parent-lib PATH] [--model brown|rational|fisheye|mixed ...] [--frames 512]
                                           [--rounds 9] [--reps 40] [--reverse] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, COLS = 640, 480


def bind_parent(path):
    """The entries this tool calls, of a library that predates abi.py's lens bindings."""
    lib, vp, i32 = C.CDLL(path), C.c_void_p, C.c_int32
    lib.vio_preprocess_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    lib.vio_preprocess_destroy.argtypes, lib.vio_preprocess_destroy.restype = [vp], None
    lib.vio_preprocess_set_clahe.argtypes = [vp, C.c_double, i32, i32]
    lib.vio_preprocess_run_resident.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    lib.vio_preprocess_sync.argtypes = [vp]
    lib.vio_preprocess_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i32)]
    if hasattr(lib, "vio_preprocess_set_lenses"):
        lib.vio_preprocess_set_lenses.argtypes = [vp, i32, C.POINTER(i32), vp]
    return lib


def phone_lens(abi):
    """A phone-like barrel lens with tangential terms, rectified to a centred pinhole: no output pixel looks outside."""
    f = 0.8 * COLS
    return abi.make_lens(f, 1.02 * f, COLS / 2 - 1.3, ROWS / 2 + 0.7, (-0.28, 0.07, 1e-3, -5e-4, 0.0),
                         (f, 1.02 * f, COLS / 2 - 0.5, ROWS / 2 - 0.5))


def rational_lens(abi):
    """The phone lens's frame and pinhole with a wide rational model, the three coefficients of the divisor included."""
    f = 0.8 * COLS
    return abi.make_lens_model(abi.VIO_LENS_RATIONAL, f, 1.02 * f, COLS / 2 - 1.3, ROWS / 2 + 0.7,
                               (0.41, 0.093, 1e-3, -5e-4, 0.0071, 0.73, 0.21, 0.017), (f, 1.02 * f, COLS / 2 - 0.5, ROWS / 2 - 0.5))


def fisheye_lens(abi):
    """A 120-degree-class fisheye, f = 0.45 cols, rectified at its own focal length: no output pixel looks outside."""
    f = 0.45 * COLS
    return abi.make_lens_model(abi.VIO_LENS_FISHEYE, f, 1.02 * f, COLS / 2 - 1.3, ROWS / 2 + 0.7, (0.021, -0.0043, 0.0011, -0.0002),
                               (f, 1.02 * f, COLS / 2 - 0.5, ROWS / 2 - 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--model", nargs="+", default=["brown"], choices=["brown", "rational", "fisheye", "mixed"],
                    help="the lens models to time (brown: variants (c) and (d))")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--reverse", action="store_true", help="create and run the variants in the reverse order")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "preprocess_lens_timing.txt" if a.model == ["brown"] else "preprocess_lens_models_timing.txt")
    import torch  # (its HIP runtime has to be the one the library binds)
    import importlib
    pkg = importlib.import_module("vins-mobile_amd")
    abi, Pre, DeviceFrames = pkg.abi, pkg.frontend.Preprocessor, pkg.loop.DeviceFrames
    assert torch.cuda.is_available(), "needs a device"
    prop = torch.cuda.get_device_properties(0)
    N = a.frames
    rng = np.random.default_rng(3)
    some = []
    for _ in range(8):                                       # 8 different textured frames, repeated over the batch
        g = pkg.synth.make_texture(rng, ROWS, COLS).astype(np.float64)
        px = np.stack([g * 0.9 + rng.normal(0, 4, g.shape), g + rng.normal(0, 4, g.shape), g * 0.7 + rng.normal(0, 4, g.shape),
                       np.full_like(g, 255)], axis=-1)
        some.append(np.clip(px, 0, 255).astype(np.uint8))
    frames = np.stack([some[k % 8] for k in range(N)])
    d_in = DeviceFrames(frames)
    del frames
    lens = phone_lens(abi)
    assert abi.lens_coverage(lens, ROWS, COLS) == 0
    models = {"rational": rational_lens(abi), "fisheye": fisheye_lens(abi)}
    for m in models.values():
        assert abi.lens_model_coverage(m, ROWS, COLS) == 0

    def context(lib=None, old=None, model=None):
        """old: (slots, VioLens) for set_lenses; model: [(slots, VioLensModel)] for set_lens_models"""
        pp = Pre(ROWS, COLS, max_frames=N, lib=lib)
        if old:
            assert pp.set_lenses(old[0], [old[1]] * len(old[0])) == abi.VIO_OK
        for slots, m in model or []:
            assert pp.set_lens_models(slots, [m] * len(slots)) == abi.VIO_OK
        return pp

    every = np.arange(N)
    plan = []                                                # (label, how to make the context)
    if a.parent_lib:
        plan.append(("(a) parent commit", lambda: context(lib=bind_parent(a.parent_lib))))
        if hasattr(bind_parent(a.parent_lib), "vio_preprocess_set_lenses"):
            plan.append(("(p) parent commit, that lens", lambda: context(lib=bind_parent(a.parent_lib), old=(every, lens))))
    plan.append(("(b) no lens set", lambda: context()))
    if "brown" in a.model:
        plan.append(("(c) a lens in every slot", lambda: context(old=(every, lens))))
        plan.append(("(d) a lens in every other slot", lambda: context(old=(np.arange(0, N, 2), lens))))
    if "rational" in a.model:
        plan.append(("(e) a rational lens in every slot", lambda: context(model=[(every, models["rational"])])))
    if "fisheye" in a.model:
        plan.append(("(f) a fisheye lens in every slot", lambda: context(model=[(every, models["fisheye"])])))
    if "mixed" in a.model:
        plan.append(("(g) mixed: none/Brown/rat./fisheye", lambda: context(model=[
            (np.arange(1, N, 4), abi.lens_model_of(lens)), (np.arange(2, N, 4), models["rational"]), (np.arange(3, N, 4), models["fisheye"])])))
    # contexts are created, and take their turns, in this order (--reverse: the other way round; reported in the order above)
    order = list(range(len(plan)))[::-1] if a.reverse else list(range(len(plan)))
    made = {i: plan[i][1]() for i in order}
    variants = [(plan[i][0], made[i]) for i in range(len(plan))]
    outs = [DeviceFrames(np.zeros((N, ROWS, COLS), np.uint8)) for _ in variants]

    def launches(i, n):
        pp = variants[i][1]
        pp.kernel_ms()
        for _ in range(n):
            pp.run_resident(d_in.ptr, 4, N, outs[i].ptr)
            pp.sync()
        ms, k = pp.kernel_ms()
        assert k == n
        return ms

    for i in order:
        launches(i, 10)
    t = [[] for _ in variants]
    for _ in range(a.rounds):
        for i in order:
            t[i].append(launches(i, a.reps))
    # the outputs of the first 4 frames (slots 0 and 2 hold a lens in (d), 1 and 3 do not)
    head = []
    for o in outs:
        h = np.zeros((4, ROWS, COLS), np.uint8)
        assert o.hip.hipMemcpy(h.ctypes.data, C.c_void_p(o.ptr), h.nbytes, 2) == 0
        head.append(h)
    names = [v[0][:3] for v in variants]
    b, same = head[names.index("(b)")], []
    if "(c)" in names:
        cc, dd = head[names.index("(c)")], head[names.index("(d)")]
        same.append("(d) slots 0, 2 == (c): %s, slots 1, 3 == (b): %s; (c) differs from (b) in %.0f %% of the bytes"
                    % (np.array_equal(dd[0::2], cc[0::2]), np.array_equal(dd[1::2], b[1::2]), 100.0 * (cc != b).mean()))
    if "(p)" in names and "(c)" in names:
        same.append("(c) == (p): %s" % np.array_equal(head[names.index("(c)")], head[names.index("(p)")]))
    for tag in ("(e)", "(f)"):
        if tag in names:
            same.append("%s differs from (b) in %.0f %% of the bytes" % (tag, 100.0 * (head[names.index(tag)] != b).mean()))
    if "(g)" in names:
        gg = head[names.index("(g)")]
        same.append("(g) slot k == the variant of its model: " + ", ".join(
            "%d %s" % (k, np.array_equal(gg[k], head[names.index(tag)][k])) for k, tag in enumerate(("(b)", "(c)", "(e)", "(f)")) if tag in names))
    if a.parent_lib:
        same.insert(0, "(b) == (a): %s" % np.array_equal(b, head[0]))
    nbytes = 7.0 * ROWS * COLS * N
    out = ["image pre-step with lens rectification: tools/preprocess_lens_timing.py on one %s (%s, %d CUs)"
           % (prop.name, getattr(prop, "gcnArchName", "?").split(":")[0], prop.multi_processor_count),
           "%d RGBA %dx%d frames resident in device memory, one vio_preprocess_run_resident per launch, device time of the two kernels"
           % (N, ROWS, COLS),
           "from vio_preprocess_kernel_ms; 10 launches of warm-up, then %d rounds of %d launches per variant, the variants taking turns"
           % (a.rounds, a.reps) + (" in the reverse of the order below" if a.reverse else ""), ""]
    med = {}
    for (label, _), v in zip(variants, t):
        m = float(np.median(v))
        med[label[:3]] = (m, max(v) - min(v))
        out.append("%-36s %8.4f ms   (median of %d rounds; min %.4f, max %.4f, spread %.4f = %.1f %%)   %6.2f TB/s of 7*R*C bytes per frame"
                   % (label, m, len(v), min(v), max(v), max(v) - min(v), 100.0 * (max(v) - min(v)) / m, nbytes / (m * 1e-3) / 1e12))
    out.append("")
    if a.parent_lib:
        ma, sa = med["(a)"]
        out.append("(b) - (a) = %+.4f ms against a run-to-run spread of (a) of %.4f ms: %s"
                   % (med["(b)"][0] - ma, sa, "within the spread" if med["(b)"][0] - ma <= sa else "SLOWER than the spread explains"))
        if "(p)" in med and "(c)" in med:
            mp, sp = med["(p)"]
            out.append("(c) - (p) = %+.4f ms against a run-to-run spread of (p) of %.4f ms: %s"
                       % (med["(c)"][0] - mp, sp, "within the spread" if med["(c)"][0] - mp <= sp else "SLOWER than the spread explains"))
        out.append("   ".join("%s / (a) = %.3f" % (k, med[k][0] / ma) for k in ("(c)", "(d)", "(e)", "(f)", "(g)") if k in med))
    else:
        out.append("(a) not measured: no --parent-lib given")
    out.append("   ".join("%s / (b) = %.3f" % (k, med[k][0] / med["(b)"][0]) for k in ("(c)", "(d)", "(e)", "(f)", "(g)") if k in med))
    for k in ("(e)", "(f)", "(g)"):
        if k in med:
            out.append("%s - (b) = %+.4f ms per %d frames" % (k, med[k][0] - med["(b)"][0], N))
    out += same
    text = "\n".join(out) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    for (_, pp), o in zip(variants, outs):
        pp.close(), o.close()
    d_in.close()


if __name__ == "__main__":
    main()
