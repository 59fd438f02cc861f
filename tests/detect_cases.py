"""Named inputs of the corner detector (detect_kernel + corner_select_kernel, fe_detect.h + fe_select.h), one for every edge the
smooth synthetic textures never reach: plateaus of equal eigenvalues (every pixel of a plateau is a candidate, so the
candidate lists sized for "one pixel in four" overflow), the switch of the selection from its LDS list to the in-place
path, and disc rows of the setMask raster that cover a whole 64-lane word. Every image is deterministic and generated
here; that a case really is the edge it is named for is asserted from the CPU oracle alone in test_detect_edges.py, so
a later change of a constant fails there instead of silently turning an edge test into an ordinary one.
"""
import numpy as np

import helpers as H
from helpers import abi, synth

# The constants of vins-mobile_amd/csrc/fe_detect.h and fe_select.h these cases are built around (duplicated on purpose):
DET_W = 60        # kDetW: output columns per wave                                  (constexpr int kDetW = 60)
DET_WAVES = 4     # kDetWaves: waves per workgroup, side by side                    (constexpr int kDetWaves = 4)
DET_R = 32        # kDetR: output rows per strip = one candidate segment            (constexpr int kDetR = 32)
SEL_LDS = 8192    # kSelLds: survivors the selection keeps in LDS; `s_cnt > kSelLds` takes the in-place path
MAX_RADIUS = 128  # kMaxRadius: largest MIN_DIST
BLOCK_W = DET_WAVES * DET_W                       # 240 columns per detector workgroup
CAND_LDS = DET_WAVES * DET_W * DET_R // 4 + 64    # kCandLds = 1984: a workgroup's own candidate list (detect_kernel)


def seg_cap(cols):
    """fe->seg_cap = kDetR * cols / 4 (vio_frontend_create): slots of one strip's segment of the ordinary candidate list."""
    return DET_R * cols // 4


# ---- images ------------------------------------------------------------------------------------------------
def checker(rows, cols, cell):
    y, x = np.mgrid[0:rows, 0:cols]
    return np.where(((y // cell) + (x // cell)) % 2 == 0, 0, 255).astype(np.uint8)


def texture(rows, cols, seed=5):
    """One frame of the smooth synthetic stream the other front-end tests use: every eigenvalue distinct."""
    return synth.make_image_stream(seed, 1, rows=rows, cols=cols)[0][0].copy()


def mixed(rows=96, cols=256):
    """2x2 checkerboard in columns 0..239 (one detector block wide), texture in the rest."""
    img = texture(rows, cols)
    img[:, :BLOCK_W] = checker(rows, BLOCK_W, 2)
    return img


def corner_block(rows, cols):
    """A trackable texture with a 2x2 checkerboard over one 240 x 32 detector block in the top left corner."""
    img = texture(rows, cols, seed=6)
    img[:DET_R, :BLOCK_W] = checker(DET_R, BLOCK_W, 2)
    return img


def turn_scenes():
    """TURN_SEQUENCES still scenes for one tracker: all but number 3 overflow the lists, so the redo lists are taken in turn
    (sequences k and k + REDO_LISTS share one) while an ordinary sequence runs next to them."""
    rows, cols = TRACKER_PLATEAU_SHAPE
    inv = 255 - checker(rows, cols, 2)
    return [mixed(), checker(rows, cols, 2), corner_block(rows, cols), texture(rows, cols, seed=7), checker(rows, cols, 3),
            np.roll(mixed(), 7, axis=0), inv]


def noise(rows, cols):
    return np.random.default_rng(11).integers(0, 256, (rows, cols), dtype=np.uint8)


def column_mask(rows, cols, lo=100, hi=180):
    m = np.zeros((rows, cols), np.uint8)
    m[:, lo:hi + 1] = 255
    return m


def ramp(rows=96, cols=256):
    """(3x + 5y) mod 256: the eigenvalue map is negative (rounding) on a few hundred pixels."""
    y, x = np.mgrid[0:rows, 0:cols]
    return ((3 * x + 5 * y) % 256).astype(np.uint8)


PLATEAU_SHAPE = (96, 256)
PLATEAU_IMAGES = {
    "checker2": lambda: checker(96, 256, 2),
    "checker3": lambda: checker(96, 256, 3),
    "mixed": mixed,
}
PLATEAU_PARAMS = [(40, 10), (150, 0), (512, 3)]  # (max_corners, min_dist)

# The redo of an overflowed sequence walks the frame in tiles of REDO_W columns x DET_R rows and owns REDO_LISTS full-size lists
# (corner_select_kernel: NW = kSelThreads / 64 = 8 waves side by side; constexpr int kRedoSlots = 4)
REDO_W = 8 * DET_W
REDO_LISTS = 4
ODD_PLATEAU_SHAPE = (100, 500)  # two tiles across with a 20-column rest, three strips and a 4-row rest
TURN_SEQUENCES = 7              # more overflowing sequences than lists, and one ordinary sequence among them

NOISE_BIG = (352, 480)       # in-place path at a small shape
NOISE_BOUNDARY = (256, 512)  # survivors tuned to 8191 / 8192 / 8193 by the quality level
BOUNDARY_COUNTS = (SEL_LDS - 1, SEL_LDS, SEL_LDS + 1)

TRACKER_PLATEAU_SHAPE = (96, 256)
TRACKER_PLATEAU_SCENES = {"mixed": mixed, "checker2": lambda: checker(96, 256, 2)}

DISC_SHAPE = (250, 333)
DISC_SEEDS = {32: (83, 84), 33: (83, 84), 64: (83, 84), 128: (83, 84)}  # min_dist -> jump_stream seeds (32 needs cx in [X0 + 29, X0 + 30])


# ---- what the oracle says about a case ------------------------------------------------------------------------
def worst_block(cand):
    """Most candidates in one 240-column x 32-row detector block."""
    rows, cols = cand.shape
    return max(int(cand[y:y + DET_R, x:x + BLOCK_W].sum()) for y in range(0, rows, DET_R) for x in range(0, cols, BLOCK_W))


def worst_strip(cand):
    return max(int(cand[y:y + DET_R].sum()) for y in range(0, cand.shape[0], DET_R))


def threshold(eig, mask, quality):
    """(float)((double)maxVal * qualityLevel) with the masked maximum, like the oracle and the device."""
    mx = eig[np.asarray(mask) != 0].max() if mask is not None else eig.max()
    return np.float32(np.float64(mx) * np.float64(quality))


def survivors(img, mask, quality):
    """Candidates above the quality threshold: what corner_select_kernel counts in s_cnt."""
    eig = H.oracle_min_eigen_map(img)
    return int((H.detector_candidates(img, mask) & (eig > threshold(eig, mask, quality))).sum())


def quality_for_survivors(img, k):
    """quality_level at which exactly k candidates survive: the threshold rounds back to v_lo, the largest candidate value
    below the k-th; None when the k-th and the next are equal."""
    eig = H.oracle_min_eigen_map(img)
    vals = np.sort(eig[H.detector_candidates(img)])[::-1]
    if k >= len(vals) or not vals[k] < vals[k - 1]:
        return None
    q = float(np.float64(vals[k]) / np.float64(eig.max()))
    return q if np.float32(np.float64(eig.max()) * np.float64(q)) == vals[k] else None


def jump_stream(seed_a, seed_b, T, cut, rows, cols):
    """A stream that changes scene at frame `cut` (test_frontend_tail_gpu.jump_stream)."""
    a = synth.make_image_stream(seed_a, T, rows=rows, cols=cols)[0]
    b = synth.make_image_stream(seed_b, T, rows=rows, cols=cols)[0]
    return [a[f] if f < cut else b[f] for f in range(T)]


def disc_centres(pts, cnt):
    """Centres of the discs a publish frame's detection ran under, from the tracker state behind that frame: the kept
    tracks (the new corners have track count 1), rounded like cv::circle's Point."""
    kept = pts[cnt > 1]
    return np.rint(kept).astype(int)  # (cvRound: half to even, as np.rint)


def full_word_discs(centres, radius, rows, cols):
    """Discs whose widest row (half-width = radius, at dy = 0) covers a whole wave word [X0 - 2, X0 + 61], X0 = 240 bx + 60 w:
    the `l1 - l0 == 63` branch of the mask raster."""
    hits = []
    for cx, cy in centres:
        if not 0 <= cy < rows:
            continue
        for x0 in range(0, cols, DET_W):
            if cx - radius <= x0 - 2 and cx + radius >= x0 + 61:
                hits.append((int(cx), int(cy), x0))
    return hits


def disc_edge_conditions(centres, radius, rows, cols):
    """-> (a centre within radius of an image edge, a centre within radius of the block edge x = 240)"""
    cx, cy = centres[:, 0], centres[:, 1]
    at_image = bool(((cx < radius) | (cy < radius) | (cx >= cols - radius) | (cy >= rows - radius)).any())
    at_block = bool((np.abs(cx - BLOCK_W) <= radius).any())
    return at_image, at_block


def config(rows, cols, max_corners, min_dist, **kw):
    return abi.default_config(max_corners=max_corners, min_dist=min_dist, image_rows=rows, image_cols=cols, **kw)
