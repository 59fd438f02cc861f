"""Lens models of the image pre-step (include/vio_amd.h, VioLensModel): the test lenses and the numpy restatement of the three
forward models that the lens-model tests share, lens_atan of csrc/pre_rectify.h mirrored operation for operation. Every numpy
expression below is one IEEE double operation per element, rounded on its own, in the order of the header; np.where is a
select and np.sqrt the correctly rounded square root."""
import numpy as np

import lens_cases as LC
import source_cases as SC
from helpers import abi

BROWN, RATIONAL, FISHEYE = abi.VIO_LENS_BROWN, abi.VIO_LENS_RATIONAL, abi.VIO_LENS_FISHEYE

ATAN_BREAKS = (0.4375, 0.6875, 1.1875, 2.4375)
ATAN_HI = (0.0, 4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00)
ATAN_A = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
          9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
          4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02)


def atan(x):
    """lens_atan for x >= 0 (an array of doubles)."""
    x = np.asarray(x, np.float64)
    b0, b1, b2, b3 = (x < b for b in ATAN_BREAKS)

    def pick(v0, v1, v2, v3, v4):
        return np.where(b0, v0, np.where(b1, v1, np.where(b2, v2, np.where(b3, v3, v4))))
    num = pick(x, (x + x) - 1.0, x - 1.0, x - 1.5, -1.0 + 0 * x)
    den = pick(1.0 + 0 * x, 2.0 + x, x + 1.0, 1.0 + 1.5 * x, x)
    hi = pick(*[h + 0 * x for h in ATAN_HI])
    a = ATAN_A
    t = num / den
    z = t * t
    w = z * z
    s1 = z * (a[0] + w * (a[2] + w * (a[4] + w * (a[6] + w * (a[8] + w * a[10])))))
    s2 = w * (a[1] + w * (a[3] + w * (a[5] + w * (a[7] + w * a[9]))))
    return hi + (t - t * (s1 + s2))


def distort(L, xn, yn):
    """The forward model of a VioLensModel: normalized undistorted coordinates -> raw pixel coordinates (not clamped)."""
    k = list(L.k)
    r2 = xn * xn + yn * yn
    if L.model == FISHEYE:
        r = np.sqrt(r2)
        th = atan(r)
        t2 = th * th
        thd = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(r2 == 0, 1.0, thd / r)
        return L.fx * (xn * s) + L.cx, L.fy * (yn * s) + L.cy
    radial = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))
    if L.model == RATIONAL:
        radial = radial / (1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7])))
    xd = (xn * radial + (2 * k[2]) * xn * yn) + k[3] * (r2 + (2 * xn) * xn)
    yd = (yn * radial + k[2] * (r2 + (2 * yn) * yn)) + ((2 * k[3]) * xn) * yn
    return L.fx * xd + L.cx, L.fy * yd + L.cy


def sample_source(L, rows, cols, dx=0.0, dy=0.0):
    """(u, v) [rows, cols]: where the sample at (x + dx, y + dy) of the output looks in the raw frame, before the clamp."""
    xn = ((np.arange(cols, dtype=np.float64) + dx)[None, :] - L.rect_cx) / L.rect_fx
    yn = ((np.arange(rows, dtype=np.float64) + dy)[:, None] - L.rect_cy) / L.rect_fy
    return distort(L, xn + 0 * yn, yn + 0 * xn)


def blend(g, u, v):
    """The shared tail: clamp, 1/32-pixel fixed point, integer bilinear blend of the int64 gray image g -> int64."""
    rows, cols = g.shape
    U = np.rint(np.clip(u, 0, cols - 1) * 32).astype(np.int64)
    V = np.rint(np.clip(v, 0, rows - 1) * 32).astype(np.int64)
    ix, ax, iy, ay = U >> 5, U & 31, V >> 5, V & 31
    x1, y1 = np.minimum(ix + 1, cols - 1), np.minimum(iy + 1, rows - 1)
    top = g[iy, ix] * (32 - ax) + g[iy, x1] * ax
    bot = g[y1, ix] * (32 - ax) + g[y1, x1] * ax
    return (top * (32 - ay) + bot * ay + 512) >> 10


def rectify(frame, L):
    """frame [rows, cols] gray or [rows, cols, 4] RGBA -> the rectified gray (uint8)."""
    g = LC.gray_of(frame)
    return blend(g, *sample_source(L, *g.shape)).astype(np.uint8)


def rectify_source(buf, src, L, rows, cols):
    """A slot that holds the source src and the lens L: the mean of s * s samples of the whole delivered frame in buf."""
    g = SC.gray_plane(buf, src)
    s = SC.samples_per_axis(src, rows, cols)
    total = np.zeros((rows, cols), np.int64)
    for dy in SC.sample_offsets(s):
        for dx in SC.sample_offsets(s):
            total += blend(g, *sample_source(L, rows, cols, dx, dy))
    return ((total + (s * s) // 2) // (s * s)).astype(np.uint8)


def n_outside(L, rows, cols):
    u, v = sample_source(L, rows, cols)
    return int(((u < 0) | (u > cols - 1) | (v < 0) | (v > rows - 1)).sum())


def tie_distance(L, n_rows, n_cols, rows, cols, offsets=(0.0,)):
    """How close 32 u or 32 v comes to a rounding tie over the rows x cols output (raw frame n_rows x n_cols)."""
    best = 1.0
    for dy in offsets:
        for dx in offsets:
            u, v = sample_source(L, rows, cols, dx, dy)
            for w, n in ((u, n_cols), (v, n_rows)):
                inside = (w > 0) & (w < n - 1)                   # a clamped coordinate is an integer: no tie
                best = min(best, np.abs((w[inside] * 32) % 1.0 - 0.5).min())
    return best


def fisheye_in(rows, cols):
    """A 120-degree-class fisheye, f = 0.45 cols, off-centre, rectified at its own focal length: theta < tan(theta), so every
    output pixel looks inside the raw frame."""
    f = 0.45 * cols
    return abi.make_lens_model(FISHEYE, f, 1.02 * f, cols / 2 - 1.3, rows / 2 + 0.7, (0.021, -0.0043, 0.0011, -0.0002),
                               (f, 1.02 * f, cols / 2 - 0.5, rows / 2 - 0.5))


def fisheye_clamped(rows, cols):
    """The same lens rectified at a shorter focal length: the rectified field of view is wider than the raw frame's, its corners
    and edges look outside (the clamp path), and r passes every breakpoint of lens_atan."""
    f = 0.45 * cols
    return abi.make_lens_model(FISHEYE, f, 1.02 * f, cols / 2 - 1.3, rows / 2 + 0.7, (0.021, -0.0043, 0.0011, -0.0002),
                               (0.2 * cols, 0.2 * cols, cols / 2 - 0.5, rows / 2 - 0.5))


def rational(rows, cols):
    """A wide rational lens: all eight coefficients, the three of the divisor included."""
    f = 0.8 * cols
    return abi.make_lens_model(RATIONAL, f, 1.02 * f, cols / 2 - 1.3, rows / 2 + 0.7,
                               (0.41, 0.093, 1e-3, -5e-4, 0.0071, 0.73, 0.21, 0.017), (f, 1.02 * f, cols / 2 - 0.5, rows / 2 - 0.5))


def brown_model(rows, cols):
    """lens_cases.lens_a as a VIO_LENS_BROWN record."""
    return abi.lens_model_of(LC.lens_a(rows, cols))


def for_frame(L, src, rows, cols):
    """A lens made for a rows x cols raw frame with its raw intrinsics rescaled to the delivered frame of src; rect_* stay those
    of the rows x cols output (source_cases.lens_for_frame for a model record)."""
    kx, ky = src.cols / cols, src.rows / rows
    return abi.make_lens_model(L.model, L.fx * kx, L.fy * ky, (L.cx + 0.5) * kx - 0.5, (L.cy + 0.5) * ky - 0.5, list(L.k),
                               (L.rect_fx, L.rect_fy, L.rect_cx, L.rect_cy))


# the six slots of the mixed batch: None, a VioLens (through set_lenses) or a VioLensModel (through set_lens_models)
def mixed_lenses(rows, cols):
    return [None, LC.lens_c(rows, cols), brown_model(rows, cols), rational(rows, cols), fisheye_in(rows, cols),
            fisheye_clamped(rows, cols)]


def mixed_frames(rows, cols, rgba):
    return np.stack([LC.random_frame(13 * k + cols, rows, cols, rgba) for k in range(6)])


def as_model(lens):
    return abi.lens_model_of(lens) if isinstance(lens, abi.VioLens) else lens


_want = {}


def mixed_expected_gray(rows, cols, rgba):
    """The gray images of mixed_frames under mixed_lenses, computed once per shape and never written to."""
    key = (rows, cols, rgba)
    if key not in _want:
        frames = mixed_frames(rows, cols, rgba)
        g = np.stack([LC.gray_of(f).astype(np.uint8) if l is None else rectify(f, as_model(l))
                      for f, l in zip(frames, mixed_lenses(rows, cols))])
        g.flags.writeable = False
        _want[key] = g
    return _want[key]
