"""Source frames and the numpy restatement of the scaling arithmetic (include/vio_amd.h, VioSource) that the source tests share.
Integer work is done in int64 (the weighted sums in doubles, exactly), where nothing can wrap; the lens part is one IEEE double
operation per element, in the order of the header, as in lens_cases.py."""
import numpy as np

import lens_cases as LC
from helpers import abi

FOUR = (abi.VIO_PIXEL_RGBA8, abi.VIO_PIXEL_BGRA8)


def random_plane(seed, src):
    """rows * stride random bytes: plane 0 of a delivered frame, padding included (and nothing after it)."""
    return np.random.default_rng(seed).integers(0, 256, src.rows * src.stride, dtype=np.uint8)


def video_range(y):
    return np.minimum(255, ((np.maximum(y, 16) - 16) * 255 + 109) // 219)


def gray_plane(buf, src):
    """The gray of every pixel of the delivered frame, int64 [src.rows, src.cols]."""
    rows = np.asarray(buf)[:src.rows * src.stride].reshape(src.rows, src.stride)
    if src.format in FOUR:
        px = rows[:, :4 * src.cols].reshape(src.rows, src.cols, 4).astype(np.int64)
        r, b = (px[..., 0], px[..., 2]) if src.format == abi.VIO_PIXEL_RGBA8 else (px[..., 2], px[..., 0])
        return (r * 4899 + px[..., 1] * 9617 + b * 1868 + 8192) >> 14
    y = rows[:, :src.cols].astype(np.int64)
    return video_range(y) if src.range == 1 else y


def weights(n_src, n_out):
    """[n_out, n_src] int64: the overlap of output index x with source index j on an axis of n_src * o units, and c."""
    g = int(np.gcd(n_src, n_out))
    c, o = n_src // g, n_out // g
    x, j = np.arange(n_out, dtype=np.int64)[:, None], np.arange(n_src, dtype=np.int64)[None, :]
    w = np.minimum((j + 1) * o, (x + 1) * c) - np.maximum(j * o, x * c)
    w = np.maximum(w, 0)
    assert (w.sum(axis=1) == c).all()
    return w, c


def area_average(gray_crop, rows, cols):
    """The exact area average of an int64 gray image to rows x cols: (S + D // 2) // D."""
    wy, ch = weights(gray_crop.shape[0], rows)
    wx, cw = weights(gray_crop.shape[1], cols)
    D = cw * ch
    assert 255 * D < 2 ** 32
    # the products in doubles (the fast matrix product): every term and every partial sum is an integer below 2^32, so exact
    S = (wy.astype(np.float64) @ gray_crop.astype(np.float64) @ wx.T.astype(np.float64)).astype(np.int64)
    return ((S + D // 2) // D).astype(np.uint8)


def samples_per_axis(src, rows, cols):
    return min(4, max(-(-src.cols // cols), -(-src.rows // rows)))


def sample_offsets(s):
    return [np.float64(2 * i + 1 - s) / np.float64(2 * s) for i in range(s)]


def sample_source(L, rows, cols, dx, dy):
    """(u, v) [rows, cols]: where the sample at (x + dx, y + dy) looks in the delivered frame, before the clamp."""
    xn = ((np.arange(cols, dtype=np.float64) + dx)[None, :] - L.rect_cx) / L.rect_fx
    yn = ((np.arange(rows, dtype=np.float64) + dy)[:, None] - L.rect_cy) / L.rect_fy
    return LC.distort(L, xn + 0 * yn, yn + 0 * xn)


def rectify_source(gray_full, src, L, rows, cols):
    """The mean of s * s bilinear samples of the whole delivered frame through lens L."""
    s = samples_per_axis(src, rows, cols)
    total = np.zeros((rows, cols), np.int64)
    for dy in sample_offsets(s):
        for dx in sample_offsets(s):
            u, v = sample_source(L, rows, cols, dx, dy)
            U = np.rint(np.clip(u, 0, src.cols - 1) * 32).astype(np.int64)
            V = np.rint(np.clip(v, 0, src.rows - 1) * 32).astype(np.int64)
            ix, ax, iy, ay = U >> 5, U & 31, V >> 5, V & 31
            x1, y1 = np.minimum(ix + 1, src.cols - 1), np.minimum(iy + 1, src.rows - 1)
            top = gray_full[iy, ix] * (32 - ax) + gray_full[iy, x1] * ax
            bot = gray_full[y1, ix] * (32 - ax) + gray_full[y1, x1] * ax
            total += (top * (32 - ay) + bot * ay + 512) >> 10
    return ((total + (s * s) // 2) // (s * s)).astype(np.uint8)


def expected_gray(buf, src, lens, rows, cols):
    """What the pre-step makes of the frame in buf for a slot that holds src (and lens, or None)."""
    g = gray_plane(buf, src)
    if lens is not None:
        return rectify_source(g, src, lens, rows, cols)
    return area_average(g[src.crop_y:src.crop_y + src.crop_rows, src.crop_x:src.crop_x + src.crop_cols], rows, cols)


def tie_distance(src, L, rows, cols):
    """How close 32 u or 32 v of any sample comes to a rounding tie (lens_cases.tie_distance over the s * s samples)."""
    s, best = samples_per_axis(src, rows, cols), 1.0
    for dy in sample_offsets(s):
        for dx in sample_offsets(s):
            u, v = sample_source(L, rows, cols, dx, dy)
            for w, n in ((u, src.cols), (v, src.rows)):
                inside = (w > 0) & (w < n - 1)
                best = min(best, np.abs((w[inside] * 32) % 1.0 - 0.5).min())
    return best


def camera(src, rows, cols, fx, fy, cx, cy):
    """vio_source_camera's formula."""
    kx, ky = cols / src.crop_cols, rows / src.crop_rows
    return fx * kx, fy * ky, (cx - src.crop_x + 0.5) * kx - 0.5, (cy - src.crop_y + 0.5) * ky - 0.5


def lens_for_frame(lens, src, rows, cols):
    """A lens of lens_cases.py (made for a rows x cols frame) with its raw intrinsics rescaled to the delivered frame of src;
    rect_* stay those of the rows x cols output."""
    kx, ky = src.cols / cols, src.rows / rows
    return abi.make_lens(lens.fx * kx, lens.fy * ky, (lens.cx + 0.5) * kx - 0.5, (lens.cy + 0.5) * ky - 0.5,
                         (lens.k1, lens.k2, lens.p1, lens.p2, lens.k3), (lens.rect_fx, lens.rect_fy, lens.rect_cx, lens.rect_cy))


def mixed_batch(rows, cols):
    """The six slots of the issue for a rows x cols context: [(source, lens or None)]."""
    rgba = abi.make_source(abi.VIO_PIXEL_RGBA8, 144, 200)
    bgra = abi.make_source(abi.VIO_PIXEL_BGRA8, 162, 225)
    gray = abi.make_source(abi.VIO_PIXEL_GRAY8, 200, 301, stride=304, crop=(7, 5, 217, 173))
    nv12 = abi.make_source(abi.VIO_PIXEL_NV12, rows, cols, stride=112, range=1)
    gray_l = abi.make_source(abi.VIO_PIXEL_GRAY8, 162, 225)
    return [(rgba, None), (bgra, None), (gray, None), (nv12, None),
            (rgba, lens_for_frame(LC.lens_a(rows, cols), rgba, rows, cols)),
            (gray_l, lens_for_frame(LC.lens_c(rows, cols), gray_l, rows, cols))]


def mixed_planes(rows, cols):
    return [random_plane(17 * k + rows, src) for k, (src, _) in enumerate(mixed_batch(rows, cols))]


_want = {}


def mixed_expected(rows, cols):
    """The gray images of mixed_batch / mixed_planes, computed once per shape and never written to."""
    if (rows, cols) not in _want:
        g = np.stack([expected_gray(b, s, l, rows, cols) for b, (s, l) in zip(mixed_planes(rows, cols), mixed_batch(rows, cols))])
        g.flags.writeable = False
        _want[(rows, cols)] = g
    return _want[(rows, cols)]
