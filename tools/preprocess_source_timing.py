#!/usr/bin/env python3
"""Device time of the image pre-step (from vio_preprocess_kernel_ms) for 512 frames resident in device memory that become
640x480 (cols x rows) images, by where the frames come from:

  (a) vio_preprocess_run_resident on 640x480 RGBA                         the existing entry, the yardstick
  (b) vio_preprocess_run_frames_resident, identity sources, same frames   the new entry where it has nothing to scale
  (c) 1280x960 RGBA                                                       2 x on both axes
  (d) 1920x1080 NV12, video range, cropped to 1440x1080                   9/4 on both axes, luma plane only
  (e) a mix of (a), (c) and (d) in equal parts                            one launch, three sizes and two formats
  (f) (c) with a lens in every slot                                       supersampled rectification, s = 2

One context per variant; 10 launches of warm-up each, then --rounds rounds in which the variants take turns, --reps launches each
(one event pair per launch): per variant the median over the rounds with the minimum and the maximum beside it, and the achieved
bytes per second, counting per frame the crop's source bytes plus 3 * rows * cols (gray out, gray in, equalized out), beside the
6.29 TB/s a plain device copy reaches on this chip. (b) is compared with (a) against (a)'s run-to-run spread, and the outputs of
(a) and (b) are compared. Needs a gfx950 device; writes profiles/preprocess_source_timing.txt.

    python tools/preprocess_source_timing.py [--frames 512] [--rounds 9] [--reps 20] [--variants abcdef] [--out FILE]

--variants picks a subset (for a profiler run of one variant, say); the comparisons with (a) are printed when (a) is among them.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, COLS = 480, 640
COPY_TBS = 6.29


class DeviceBatch:
    """n frames of one size in one device allocation, filled by repeating a few distinct host frames."""

    def __init__(self, distinct, n):
        hip = self.hip = C.CDLL("libamdhip64.so")             # the runtime libvio_amd.so is linked against
        hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.frame_bytes = distinct[0].nbytes
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), self.frame_bytes * n) == 0
        self.ptr = p.value
        for k in range(n):
            f = distinct[k % len(distinct)]
            assert hip.hipMemcpy(C.c_void_p(self.frame(k)), f.ctypes.data, f.nbytes, 1) == 0   # hipMemcpyHostToDevice

    def frame(self, k):
        return self.ptr + k * self.frame_bytes

    def close(self):
        self.hip.hipFree(C.c_void_p(self.ptr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--variants", default="abcdef")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_source_timing.txt"))
    a = ap.parse_args()
    import torch  # (its HIP runtime has to be the one the library binds)
    import importlib
    pkg = importlib.import_module("vins-mobile_amd")
    abi, Pre, DeviceFrames = pkg.abi, pkg.frontend.Preprocessor, pkg.loop.DeviceFrames
    assert torch.cuda.is_available(), "needs a device"
    prop = torch.cuda.get_device_properties(0)
    N = a.frames
    rng = np.random.default_rng(3)

    def textured(rows, cols, rgba):
        """8 distinct frames: a texture made at the output size, enlarged by pixel repetition, with noise of its own."""
        out = []
        for _ in range(8):
            g = pkg.synth.make_texture(rng, ROWS, COLS).astype(np.float32)
            g = np.repeat(np.repeat(g, -(-rows // ROWS), axis=0), -(-cols // COLS), axis=1)[:rows, :cols]
            if rgba:
                px = np.stack([g * 0.9, g, g * 0.7, np.full_like(g, 255)], axis=-1) + rng.normal(0, 4, (rows, cols, 1)).astype(np.float32)
            else:
                px = 16 + g * (219.0 / 255.0) + rng.normal(0, 3, g.shape).astype(np.float32)
            out.append(np.clip(px, 0, 255).astype(np.uint8))
        return out

    small = DeviceBatch(textured(ROWS, COLS, True), N)
    big = DeviceBatch(textured(960, 1280, True), N)
    luma = DeviceBatch(textured(1080, 1920, False), N)           # plane 0 only: the chroma plane is never read
    s_small = abi.make_source(abi.VIO_PIXEL_RGBA8, ROWS, COLS)
    s_big = abi.make_source(abi.VIO_PIXEL_RGBA8, 960, 1280)
    s_luma = abi.make_source(abi.VIO_PIXEL_NV12, 1080, 1920, crop=(240, 0, 1440, 1080), range=1)
    f = 0.8 * 1280
    lens = abi.make_lens(f, 1.02 * f, 1280 / 2 - 2.1, 960 / 2 + 1.9, (-0.28, 0.07, 1e-3, -5e-4, 0.0),
                         abi.source_camera(s_big, ROWS, COLS, f, 1.02 * f, 1280 / 2 - 0.5, 960 / 2 - 0.5))
    out_bytes = 3.0 * ROWS * COLS

    def crop_bytes(s):
        return float(s.crop_rows * s.crop_cols * (4 if s.format in (abi.VIO_PIXEL_RGBA8, abi.VIO_PIXEL_BGRA8) else 1))

    variants = []                                            # (label, context, call, bytes per launch)

    def add(label, sources, ptrs, lenses=None):
        if label[1] not in a.variants:
            return
        pp = Pre(ROWS, COLS, max_frames=N)
        nbytes = N * out_bytes
        if sources is None:
            variants.append((label, pp, lambda o: pp.run_resident(small.ptr, 4, N, o), nbytes + N * crop_bytes(s_small)))
            return
        assert pp.set_sources(np.arange(N), sources) == abi.VIO_OK
        if lenses is not None:
            assert pp.set_lenses(np.arange(N), lenses) == abi.VIO_OK
        nbytes += sum(crop_bytes(s) for s in sources)

        def call(o):
            assert pp.run_frames_resident(ptrs, o) == abi.VIO_OK
        variants.append((label, pp, call, nbytes))

    add("(a) run_resident, 640x480 RGBA", None, None)
    add("(b) run_frames_resident, identity", [s_small] * N, [small.frame(k) for k in range(N)])
    add("(c) 1280x960 RGBA", [s_big] * N, [big.frame(k) for k in range(N)])
    add("(d) 1920x1080 NV12 -> 1440x1080", [s_luma] * N, [luma.frame(k) for k in range(N)])
    kinds = [(s_small, small), (s_big, big), (s_luma, luma)]
    add("(e) mix of (a), (c), (d)", [kinds[k % 3][0] for k in range(N)], [kinds[k % 3][1].frame(k) for k in range(N)])
    add("(f) (c) with a lens in every slot", [s_big] * N, [big.frame(k) for k in range(N)], [lens] * N)
    outs = [DeviceFrames(np.zeros((N, ROWS, COLS), np.uint8)) for _ in variants]

    def launches(i, n):
        _, pp, call, _ = variants[i]
        pp.kernel_ms()
        for _ in range(n):
            call(outs[i].ptr)
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
    out = ["image pre-step with native-size source frames: tools/preprocess_source_timing.py on one %s (%s, %d CUs)"
           % (prop.name, getattr(prop, "gcnArchName", "?").split(":")[0], prop.multi_processor_count),
           "%d frames resident in device memory -> %dx%d, one call per launch, device time of the two kernels from" % (N, COLS, ROWS),
           "vio_preprocess_kernel_ms; 10 launches of warm-up, then %d rounds of %d launches per variant, the variants taking turns."
           % (a.rounds, a.reps),
           "Bytes per frame: the crop's source bytes + 3 * rows * cols; a plain device copy on this chip reaches %.2f TB/s." % COPY_TBS, ""]
    med, rate = [], []
    for (label, _, _, nbytes), v in zip(variants, t):
        m = float(np.median(v))
        med.append(m), rate.append(nbytes / (m * 1e-3) / 1e12)
        out.append("%-36s %8.4f ms   (median of %d rounds; min %.4f, max %.4f, spread %.4f = %.1f %%)   %7.1f MB   %5.2f TB/s = %2.0f %% of a copy"
                   % (label, m, len(v), min(v), max(v), max(v) - min(v), 100.0 * (max(v) - min(v)) / m, nbytes / 1e6, rate[-1],
                      100.0 * rate[-1] / COPY_TBS))
    out.append("")
    names = [v[0][1] for v in variants]
    if "a" in names:
        ia = names.index("a")
        if "b" in names:
            ib, head = names.index("b"), []
            for o in (outs[ia], outs[ib]):
                h = np.zeros((4, ROWS, COLS), np.uint8)
                assert o.hip.hipMemcpy(h.ctypes.data, C.c_void_p(o.ptr), h.nbytes, 2) == 0
                head.append(h)
            spread_a = max(t[ia]) - min(t[ia])
            out.append("(b) - (a) = %+.4f ms against a run-to-run spread of (a) of %.4f ms: %s; first 4 frames (b) == (a): %s"
                       % (med[ib] - med[ia], spread_a, "within the spread" if abs(med[ib] - med[ia]) <= spread_a else "OUTSIDE the spread",
                          np.array_equal(head[0], head[1])))
        for i, c in enumerate(names):
            if c in "cdef":
                out.append("(%s): %.2f of (a)'s bytes per second%s" % (c, rate[i] / rate[ia], "   BELOW HALF" if rate[i] < 0.5 * rate[ia] else ""))
    text = "\n".join(out) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f_out:
        f_out.write(text)
    for (_, pp, _, _), o in zip(variants, outs):
        pp.close(), o.close()
    for b in (small, big, luma):
        b.close()


if __name__ == "__main__":
    main()
