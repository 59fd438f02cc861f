"""The valid region of a pre-step slot (include/vio_amd.h, vio_lens_model_valid_region): the numpy restatement and the cases
that the region tests share. Built on lens_model_cases.py / source_cases.py: one IEEE double operation per element, in the
order of csrc/pre_source.h."""
import zlib

import numpy as np

import lens_model_cases as MC
import source_cases as SC
from helpers import abi

MARGINS = (0, 1, 10)
SHAPES = [(72, 100), (64, 96)]


def _in_frame(u, v, rows, cols):
    """!(lens_outside(u, cols) || lens_outside(v, rows)): a NaN compares false and is outside."""
    with np.errstate(invalid="ignore"):
        return (u >= 0) & (u <= cols - 1) & (v >= 0) & (v <= rows - 1)


def inside(L, src, rows, cols):
    """bool [rows, cols]: nothing the output pixel is made of was clamped. L None: a slot without a lens."""
    if L is None:
        return np.ones((rows, cols), bool)
    if src is None:
        return _in_frame(*MC.sample_source(L, rows, cols), rows, cols)
    s = SC.samples_per_axis(src, rows, cols)
    ok = np.ones((rows, cols), bool)
    for dy in SC.sample_offsets(s):
        for dx in SC.sample_offsets(s):
            ok &= _in_frame(*MC.sample_source(L, rows, cols, dx, dy), src.rows, src.cols)
    return ok


def erode(ok, margin):
    """Every pixel within `margin` (Chebyshev) is set; neighbours outside the image do not count."""
    rows, cols = ok.shape
    pad = np.ones((rows + 2 * margin, cols + 2 * margin), bool)
    pad[margin:margin + rows, margin:margin + cols] = ok
    out = np.ones((rows, cols), bool)
    for dy in range(2 * margin + 1):
        for dx in range(2 * margin + 1):
            out &= pad[dy:dy + rows, dx:dx + cols]
    return out


def valid_region(L, src, rows, cols, margin):
    """The restatement of vio_lens_model_valid_region -> uint8 [rows, cols] of 0 / 255."""
    return np.where(erode(inside(L, src, rows, cols), margin), 255, 0).astype(np.uint8)


def sourced_cases(rows, cols):
    """[(source, lens)]: a Brown-Conrady and a fisheye lens over an RGBA frame of twice the output's size (s = 2)."""
    src = abi.make_source(abi.VIO_PIXEL_RGBA8, 2 * rows, 2 * cols)
    assert SC.samples_per_axis(src, rows, cols) == 2
    return [(src, MC.for_frame(MC.as_model(MC.mixed_lenses(rows, cols)[1]), src, rows, cols)),
            (src, MC.for_frame(MC.fisheye_clamped(rows, cols), src, rows, cols))]


def cases(rows, cols):
    """[(name, lens model or None, source or None)]: the six slots of lens_model_cases.mixed_lenses, then the two sourced ones."""
    out = [("mixed%d" % k, None if l is None else MC.as_model(l), None) for k, l in enumerate(MC.mixed_lenses(rows, cols))]
    return out + [("sourced%d" % k, l, s) for k, (s, l) in enumerate(sourced_cases(rows, cols))]


_want = {}


def expected(rows, cols, margin):
    """{name: mask} of cases(rows, cols), computed once per (shape, margin) and never written to."""
    key = (rows, cols, margin)
    if key not in _want:
        _want[key] = {}
        for name, lens, src in cases(rows, cols):
            m = valid_region(lens, src, rows, cols, margin)
            m.flags.writeable = False
            _want[key][name] = m
    return _want[key]


# ---- the front end's region of interest (vio_frontend_set_regions) ---------------------------------------------------------
def ring(rows, cols, k):
    """The outer k pixels unusable."""
    m = np.zeros((rows, cols), np.uint8)
    m[k:rows - k, k:cols - k] = 255
    return m


def holes(rows, cols):
    """Left half: usable with isolated 1-pixel zeros on a 5 x 7 lattice; right half: unusable with isolated 1-pixel 255s on the
    same lattice -- a lone usable pixel becomes a corner only if it is the maximum of its own 3 x 3."""
    m = np.zeros((rows, cols), np.uint8)
    m[:, :cols // 2] = 255
    lattice = np.zeros((rows, cols), bool)
    lattice[2::5, 3::7] = True
    m[lattice] = 255 - m[lattice]
    return m


def word_edges(rows, cols):
    """Zeros exactly in columns 61 .. 65, 127 and 128: both sides of the first two 64-bit word boundaries."""
    m = np.full((rows, cols), 255, np.uint8)
    m[:, [61, 62, 63, 64, 65, 127, 128]] = 0
    return m


def none_usable(rows, cols):
    return np.zeros((rows, cols), np.uint8)


def all_usable(rows, cols):
    return np.full((rows, cols), 255, np.uint8)


def circle_halfwidths(radius):
    """cv::circle's filled midpoint raster (the oracle's circle_halfwidths): half-width of every row of the disc."""
    hw = [-1] * (2 * radius + 1)
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        hw[radius + dy], hw[radius - dy] = max(hw[radius + dy], dx), max(hw[radius - dy], dx)
        hw[radius + dx], hw[radius - dx] = max(hw[radius + dx], dy), max(hw[radius - dx], dy)
        dy += 1
        err += plus
        plus += 2
        mask = (1 if err <= 0 else 0) - 1
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    return hw


class RegionTracker:
    """readImage (oracle/vio_oracle_frontend.cpp: oracle_tracker_read_image, tracker_update_tracks) restated over the oracle's
    primitives -- oracle_klt_track, oracle_fundamental_ransac, oracle_good_features with a mask image -- with ONE change: on a
    publish frame the mask starts as `region` (0 / 255; None: all 255) instead of all 255. tests/test_region_cpu.py holds it
    against helpers.OracleTracker. Per publish frame it also records what the region did (self.log)."""

    def __init__(self, cfg, region=None):
        import helpers as H
        self.H, self.cfg = H, cfg
        self.rows, self.cols = cfg.image_rows, cfg.image_cols
        self.region = None if region is None else np.where(np.asarray(region) != 0, 255, 0).astype(np.uint8)
        self.hw = circle_halfwidths(cfg.min_dist)
        self.cur_img = None
        self.pre = np.zeros((0, 2), np.float32)
        self.cur = np.zeros((0, 2), np.float32)
        self.forw = np.zeros((0, 2), np.float32)
        self.ids, self.cnt = np.zeros(0, np.int32), np.zeros(0, np.int32)
        self.n_id = 0
        self.log = []      # per publish frame: dict(dropped, absent, points)

    def set_region(self, region):
        self.region = None if region is None else np.where(np.asarray(region) != 0, 255, 0).astype(np.uint8)

    def _reduce(self, keep):
        keep = np.asarray(keep, bool)
        self.pre, self.cur, self.forw = self.pre[keep], self.cur[keep], self.forw[keep]
        self.ids, self.cnt = self.ids[keep], self.cnt[keep]

    def _paint(self, mask, ix, iy):
        r = self.cfg.min_dist
        for dy in range(-r, r + 1):
            yy = iy + dy
            if 0 <= yy < self.rows:
                h = self.hw[r + dy]
                mask[yy, max(0, ix - h):min(self.cols - 1, ix + h) + 1] = 0

    def _update_tracks(self, status, publish):
        """-> (mask, the mask without the region) on a publish frame."""
        H, cfg = self.H, self.cfg
        if len(self.cur):
            ix, iy = np.rint(self.forw[:, 0]).astype(np.int64), np.rint(self.forw[:, 1]).astype(np.int64)
            inb = (1 <= ix) & (ix < self.cols - 1) & (1 <= iy) & (iy < self.rows - 1)
            self._reduce((status != 0) & inb)
            if len(self.forw) >= 8:
                self._reduce(H.oracle_ransac(cfg, self.cur, self.forw) != 0)
        if not publish:
            return None, None
        if len(self.forw) >= 8:
            self._reduce(H.oracle_ransac(cfg, self.pre, self.forw) != 0)
        self.cnt = self.cnt + 1
        mask = np.full((self.rows, self.cols), 255, np.uint8) if self.region is None else self.region.copy()
        plain = np.full((self.rows, self.cols), 255, np.uint8)
        kept, dropped = [], 0
        for i in np.argsort(-self.cnt.astype(np.int64), kind="stable"):
            ix, iy = int(np.rint(self.forw[i, 0])), int(np.rint(self.forw[i, 1]))
            dropped += self.region is not None and self.region[iy, ix] == 0
            if mask[iy, ix] == 255:
                kept.append(i)
                self._paint(mask, ix, iy)
                self._paint(plain, ix, iy)
        kept = np.array(kept, np.int64)
        self.forw, self.ids, self.cnt = self.forw[kept], self.ids[kept], self.cnt[kept]
        self.log.append({"dropped": int(dropped)})
        return mask, plain

    def read_image(self, img, publish):
        """-> (ids int32 [n], xyz float64 [n, 3]) like helpers.OracleTracker.read_image."""
        H, cfg = self.H, self.cfg
        img = np.ascontiguousarray(img, np.uint8)
        if self.cur_img is None:
            self.cur_img = img
        self.forw = np.zeros((0, 2), np.float32)
        mask = plain = None
        if len(self.cur):
            self.forw, status, _ = H.oracle_klt(cfg, self.cur_img, img, self.cur)
            mask, plain = self._update_tracks(status, publish)
        elif publish:
            mask, plain = self._update_tracks(np.zeros(0, np.uint8), True)
        if publish:
            n_max = cfg.max_corners - len(self.ids)
            if n_max > 0:
                new = H.oracle_good_features(cfg, img, mask, n_max).reshape(-1, 2)
                unmasked = H.oracle_good_features(cfg, img, plain, n_max).reshape(-1, 2)
                have = {tuple(p) for p in new.tolist()}
                self.log[-1]["absent"] = sum(tuple(p) not in have for p in unmasked.tolist())
                self.forw = np.concatenate([self.forw, new]).astype(np.float32)
                self.ids = np.concatenate([self.ids, np.full(len(new), -1, np.int32)])
                self.cnt = np.concatenate([self.cnt, np.ones(len(new), np.int32)])
            self.pre = self.forw.copy()
        self.cur_img, self.cur = img, self.forw.copy()
        if not publish:
            return np.zeros(0, np.int32), np.zeros((0, 3))
        fresh = self.ids == -1
        self.ids = self.ids.copy()
        self.ids[fresh] = self.n_id + np.arange(int(fresh.sum()), dtype=np.int32)
        self.n_id += int(fresh.sum())
        xyz = np.stack([(self.cur[:, 0].astype(np.float64) - cfg.cx) / cfg.fx, (self.cur[:, 1].astype(np.float64) - cfg.cy) / cfg.fy,
                        np.ones(len(self.cur))], axis=1).reshape(-1, 3)
        self.log[-1]["points"] = self.cur.copy()
        return self.ids.astype(np.int32), xyz

    def state(self):
        return self.cur.copy(), self.ids.astype(np.int32), self.cnt.astype(np.int32)

    def close(self):
        pass


def checksum(mask):
    """What tests/emul/valid_region_main.cpp prints for a mask: CRC-32 of its bytes and the number of zeros."""
    mask = np.ascontiguousarray(mask, np.uint8)
    return zlib.crc32(mask.tobytes()) & 0xffffffff, int((mask == 0).sum())
