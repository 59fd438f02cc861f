#!/usr/bin/env python3
"""Device time of the image pre-step (vio_preprocess_run_resident, from vio_preprocess_kernel_ms) for 512 RGBA 640x480 frames
resident in device memory, with and without lens rectification:

  (a) the parent commit's library     --parent-lib PATH/libvio_amd.so, built from the commit before lenses existed (skipped,
                                      and said so, when the option is not given)
  (b) this library, no lens set       the kernel without the lens branch
  (c) this library, a lens in every slot
  (d) this library, a lens in every other slot (one launch: lens or no lens is chosen per frame)

One context per variant, all on the same input; 10 launches of warm-up each, then --rounds rounds in which the variants take
turns, --reps launches each (one event pair per launch): per variant the median over the rounds with the minimum and the maximum
beside it, the spread of (a) as the yardstick for (b) against (a), and the achieved bytes per second against the 7 * rows * cols
bytes per RGBA frame of the header comment of csrc/vio_preprocess.hip. The outputs are compared as well: (b) equals (a), the slots
of (d) equal (c)'s or (b)'s. Needs a gfx950 device; writes profiles/preprocess_lens_timing.txt.

    python tools/preprocess_lens_timing.py [--parent-lib PATH] [--frames 512] [--rounds 9] [--reps 40] [--out FILE]
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
    return lib


def phone_lens(abi):
    """A phone-like barrel lens with tangential terms, rectified to a centred pinhole: no output pixel looks outside."""
    f = 0.8 * COLS
    return abi.make_lens(f, 1.02 * f, COLS / 2 - 1.3, ROWS / 2 + 0.7, (-0.28, 0.07, 1e-3, -5e-4, 0.0),
                         (f, 1.02 * f, COLS / 2 - 0.5, ROWS / 2 - 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_lens_timing.txt"))
    a = ap.parse_args()
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
    variants = []                                            # (label, context, device output)
    if a.parent_lib:
        variants.append(("(a) parent commit", Pre(ROWS, COLS, max_frames=N, lib=bind_parent(a.parent_lib))))
    variants.append(("(b) no lens set", Pre(ROWS, COLS, max_frames=N)))
    c = Pre(ROWS, COLS, max_frames=N)
    assert c.set_lenses(np.arange(N), [lens] * N) == abi.VIO_OK
    variants.append(("(c) a lens in every slot", c))
    d = Pre(ROWS, COLS, max_frames=N)
    assert d.set_lenses(np.arange(0, N, 2), [lens] * len(range(0, N, 2))) == abi.VIO_OK
    variants.append(("(d) a lens in every other slot", d))
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

    for i in range(len(variants)):
        launches(i, 10)
    t = [[] for _ in variants]
    for _ in range(a.rounds):
        for i in range(len(variants)):
            t[i].append(launches(i, a.reps))
    # the outputs of the first 4 frames (slots 0 and 2 hold a lens in (d), 1 and 3 do not)
    head = []
    for o in outs:
        h = np.zeros((4, ROWS, COLS), np.uint8)
        assert o.hip.hipMemcpy(h.ctypes.data, C.c_void_p(o.ptr), h.nbytes, 2) == 0
        head.append(h)
    names = [v[0][:3] for v in variants]
    b, cc, dd = head[names.index("(b)")], head[names.index("(c)")], head[names.index("(d)")]
    same = ["(d) slots 0, 2 == (c): %s, slots 1, 3 == (b): %s; (c) differs from (b) in %.0f %% of the bytes"
            % (np.array_equal(dd[0::2], cc[0::2]), np.array_equal(dd[1::2], b[1::2]), 100.0 * (cc != b).mean())]
    if a.parent_lib:
        same.insert(0, "(b) == (a): %s" % np.array_equal(b, head[0]))
    nbytes = 7.0 * ROWS * COLS * N
    out = ["image pre-step with lens rectification: tools/preprocess_lens_timing.py on one %s (%s, %d CUs)"
           % (prop.name, getattr(prop, "gcnArchName", "?").split(":")[0], prop.multi_processor_count),
           "%d RGBA %dx%d frames resident in device memory, one vio_preprocess_run_resident per launch, device time of the two kernels"
           % (N, ROWS, COLS),
           "from vio_preprocess_kernel_ms; 10 launches of warm-up, then %d rounds of %d launches per variant, the variants taking turns"
           % (a.rounds, a.reps), ""]
    med = {}
    for (label, _), v in zip(variants, t):
        m = float(np.median(v))
        med[label[:3]] = (m, max(v) - min(v))
        out.append("%-32s %8.4f ms   (median of %d rounds; min %.4f, max %.4f, spread %.4f = %.1f %%)   %6.2f TB/s of 7*R*C bytes per frame"
                   % (label, m, len(v), min(v), max(v), max(v) - min(v), 100.0 * (max(v) - min(v)) / m, nbytes / (m * 1e-3) / 1e12))
    out.append("")
    if a.parent_lib:
        ma, sa = med["(a)"]
        out.append("(b) - (a) = %+.4f ms against a run-to-run spread of (a) of %.4f ms: %s"
                   % (med["(b)"][0] - ma, sa, "within the spread" if med["(b)"][0] - ma <= sa else "SLOWER than the spread explains"))
        out.append("(c) / (a) = %.3f   (d) / (a) = %.3f" % (med["(c)"][0] / ma, med["(d)"][0] / ma))
    else:
        out.append("(a) not measured: no --parent-lib given")
    out.append("(c) / (b) = %.3f   (d) / (b) = %.3f" % (med["(c)"][0] / med["(b)"][0], med["(d)"][0] / med["(b)"][0]))
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
