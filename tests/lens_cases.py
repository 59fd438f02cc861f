"""Lenses, frames and the numpy restatement of the rectification arithmetic (include/vio_amd.h, VioLens) that the lens tests
share. Every numpy operation below is one IEEE double operation per element, rounded on its own, in the order of the header."""
import numpy as np

from helpers import abi


def lens_a(rows, cols):
    """A phone-like barrel lens, off-centre, with tangential terms; rectified to a centred pinhole of the same focal length."""
    f = 0.8 * cols
    return abi.make_lens(f, 1.02 * f, cols / 2 - 1.3, rows / 2 + 0.7, (-0.28, 0.07, 1e-3, -5e-4, 0.0),
                         (f, 1.02 * f, cols / 2 - 0.5, rows / 2 - 0.5))


def lens_c(rows, cols):
    """Pincushion, lens A's focal lengths, centred: the corners of the rectified image look outside the raw one (the clamp path)."""
    f = 0.8 * cols
    return abi.make_lens(f, 1.02 * f, cols / 2 - 0.5, rows / 2 - 0.5, (0.35, 0.1, 0.0, 0.0, 0.0))


def identity_lens(rows, cols):
    return abi.make_lens(0.8 * cols, 0.83 * cols, cols / 2 - 1.3, rows / 2 + 0.7)


def distort(L, xn, yn):
    """The forward model: normalized undistorted coordinates -> raw pixel coordinates (not clamped)."""
    r2 = xn * xn + yn * yn
    radial = 1 + r2 * (L.k1 + r2 * (L.k2 + r2 * L.k3))
    xd = (xn * radial + (2 * L.p1) * xn * yn) + L.p2 * (r2 + (2 * xn) * xn)
    yd = (yn * radial + L.p1 * (r2 + (2 * yn) * yn)) + ((2 * L.p2) * xn) * yn
    return L.fx * xd + L.cx, L.fy * yd + L.cy


def source(L, rows, cols):
    """(u, v) [rows, cols]: where output pixel (x, y) looks in the raw image, before the clamp."""
    xn = (np.arange(cols, dtype=np.float64)[None, :] - L.rect_cx) / L.rect_fx
    yn = (np.arange(rows, dtype=np.float64)[:, None] - L.rect_cy) / L.rect_fy
    return distort(L, xn + 0 * yn, yn + 0 * xn)          # (+ 0 * ...: broadcast to the full grid, exact)


def gray_of(frame):
    frame = np.asarray(frame)
    if frame.ndim == 2:
        return frame.astype(np.int64)
    r, g, b = (frame[..., k].astype(np.int64) for k in range(3))
    return (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14


def n_outside(L, rows, cols):
    u, v = source(L, rows, cols)
    return int(((u < 0) | (u > cols - 1) | (v < 0) | (v > rows - 1)).sum())


def rectify(frame, L):
    """frame [rows, cols] gray or [rows, cols, 4] RGBA -> the rectified gray (uint8)."""
    g = gray_of(frame)
    rows, cols = g.shape
    u, v = source(L, rows, cols)
    U = np.rint(np.clip(u, 0, cols - 1) * 32).astype(np.int64)      # np.rint: ties to even
    V = np.rint(np.clip(v, 0, rows - 1) * 32).astype(np.int64)
    ix, ax, iy, ay = U >> 5, U & 31, V >> 5, V & 31
    x1, y1 = np.minimum(ix + 1, cols - 1), np.minimum(iy + 1, rows - 1)
    top = g[iy, ix] * (32 - ax) + g[iy, x1] * ax
    bot = g[y1, ix] * (32 - ax) + g[y1, x1] * ax
    return ((top * (32 - ay) + bot * ay + 512) >> 10).astype(np.uint8)


def tie_distance(L, rows, cols):
    """How close 32 u or 32 v comes to a rounding tie (a fraction of exactly 1/2) over the frame."""
    u, v = source(L, rows, cols)
    d = [np.abs((np.clip(w, 0, n - 1) * 32) % 1.0 - 0.5) for w, n in ((u, cols), (v, rows))]
    inside = [(w > 0) & (w < n - 1) for w, n in ((u, cols), (v, rows))]    # a clamped coordinate is an integer: no tie
    return min(d[0][inside[0]].min(), d[1][inside[1]].min())


def random_frame(seed, rows, cols, rgba):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (rows, cols, 4) if rgba else (rows, cols), dtype=np.uint8)
