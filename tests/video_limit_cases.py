"""Every input of tests/test_video_limits_cpu.py and tests/test_video_limits_gpu.py: the images, the point sets and the
parameter sets that take lk_pyr_down, lk_track, lk_compact (csrc/track_lk.hip, SPEC S61-S66) and corner_extrema, corner_rank,
corner_select (csrc/corners.hip, S67-S70) to the structural edges of the kernels.  The CPU file runs the restatements
(tests/lk_ref.c, tests/corner_ref.c) on these very arrays and asserts that each case reaches the edge it is named after; the
GPU file runs the same arrays on the device and compares bit for bit.  Every generator is deterministic (a seeded
np.random.default_rng; the images by integer arithmetic alone); images, restated pyramids and restated results are made once per process and must not be written to."""
import functools

import numpy as np

import corner_ref as K
import lk_ref as R

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)


def below(v):
    """The float32 just below v."""
    return np.nextafter(F32(v), F32(-np.inf))


def above(v):
    return np.nextafter(F32(v), F32(np.inf))


# ---- images ------------------------------------------------------------------------------------------------------------------

def noise_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def smooth_image(w, h, seed, cell=5):
    """Integer bilinear interpolation of a random grid of `cell` pixels a mesh: texture everywhere, gradients a tracker can use."""
    g = np.random.default_rng(seed).integers(0, 256, (h // cell + 2, w // cell + 2)).astype(np.int64)
    x, y = np.arange(w), np.arange(h)[:, None]
    x0, a, y0, b = x // cell, x % cell, y // cell, y % cell
    v = g[y0, x0] * (cell - a) * (cell - b) + g[y0, x0 + 1] * a * (cell - b) + g[y0 + 1, x0] * (cell - a) * b + g[y0 + 1, x0 + 1] * a * b
    return ((v + cell * cell // 2) // (cell * cell)).astype(np.uint8)


def octave_image(side):
    """Blocks of 4, 16, 64 and 256 pixels added up: structure at every level of an 8-level pyramid."""
    rng = np.random.default_rng(side)
    img = np.zeros((side, side), np.int32)
    for s in (4, 16, 64, 256):
        n = -(-side // s)
        img += np.repeat(np.repeat(rng.integers(0, 64, (n, n)), s, 0), s, 1)[:side, :side]
    return img.astype(np.uint8)


def moved(img, dx, dy):
    """The image rolled so that its content moves by (dx, dy)."""
    return np.roll(img, (dy, dx), axis=(0, 1))


SMALL_SHIFT, BIG_SHIFT = (2, -1), (5, -3)
PYR_SHAPES = [(31, 63), (32, 64), (33, 65), (34, 66), (47, 127), (48, 129), (63, 31), (65, 33)]          # (h, w)
PYR_LEVEL1 = [(16, 32), (16, 32), (17, 33), (17, 33), (24, 64), (24, 65), (32, 16), (33, 17)]
PYR_PAD = 5                                                                                                # row stride = w + 5


@functools.lru_cache(maxsize=None)
def frame(name):
    if name == "a64":
        return smooth_image(64, 48, 1)
    if name == "a131":
        return smooth_image(131, 97, 2)
    if name in ("b64", "b131"):
        return moved(frame("a" + name[1:]), *SMALL_SHIFT)
    if name == "n64":
        return noise_image(64, 48, 3)
    if name == "big":
        return octave_image(1921)
    if name == "bigroll":
        return moved(frame("big"), *BIG_SHIFT)
    if name == "big1920":
        return octave_image(1920)
    if name == "all255":
        return np.full((33, 65), 255, np.uint8)
    if name == "columns":
        return np.tile(np.array([0, 255], np.uint8), (33, 33))[:, :65].copy()
    if name.startswith("pyr"):
        h, w = PYR_SHAPES[int(name[3:])]
        return noise_image(w, h, 1000 * h + w)
    raise KeyError(name)


PYR_CASES = ["pyr%d" % i for i in range(len(PYR_SHAPES))] + ["all255", "columns"]


def padded(img, pad=PYR_PAD):
    """The image in a buffer whose rows are pad bytes longer, the padding filled with other bytes."""
    h, w = img.shape
    buf = noise_image(w + pad, h, 7 * h + w)
    buf[:, :w] = img
    return buf


@functools.lru_cache(maxsize=None)
def pyramid(name, max_level):
    return R.Pyramid(frame(name), max_level)


# ---- tracking cases -------------------------------------------------------------------------------------------------------------

class TrackCase:
    """One call of the tracker.  prm: (win_radius, max_level, max_iters, eps, min_eig, fb_thresh, flags), the argument order of
    both lk_ref.params and api.lk_params.  built: the max_level the two pyramids are created with."""

    def __init__(self, tag, a, b, built, pts, prm, init=None, **note):
        self.tag, self.a, self.b, self.built, self.prm = tag, a, b, built, tuple(prm)
        self.pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
        self.init = None if init is None else np.ascontiguousarray(init, F32).reshape(-1, 2)
        assert (self.init is not None) == bool(self.prm[6] & R.USE_INITIAL)
        self.note = note
        self._want = None

    def pyramids(self):
        return pyramid(self.a, self.built), pyramid(self.b, self.built)

    def want(self):
        """(out, status, err, fb) of the restatement, computed once."""
        if self._want is None:
            pa, pb = self.pyramids()
            self._want = R.track(pa, pb, self.pts, R.params(*self.prm), self.init)
        return self._want

    def __repr__(self):
        return self.tag


def interior_points(w, h, margin, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(margin, w - 1 - margin, n), rng.uniform(margin, h - 1 - margin, n)], 1).astype(F32)


def prm(r=3, max_level=0, max_iters=30, eps=0.01, min_eig=1e-4, fb_thresh=0.0, flags=0):
    return (r, max_level, max_iters, eps, min_eig, fb_thresh, flags)


@functools.lru_cache(maxsize=None)
def radius_cases():
    """Every radius once on each pair of frames, 16 points, 30 iterations, forward-backward on."""
    out = []
    for r in range(2, 16):
        out.append(TrackCase("radius %d, 64 x 48" % r, "a64", "b64", 3, interior_points(64, 48, r + 2, 16, r), prm(r, 3, fb_thresh=0.5)))
        out.append(TrackCase("radius %d, 131 x 97" % r, "a131", "b131", 7, interior_points(131, 97, r + 2, 16, 100 + r), prm(r, 7, fb_thresh=0.5)))
    return out


def border_points(level, wl, hl, lo, hi_off):
    """Four (accepted, refused) pairs, left, top, right, bottom, for a window that is accepted on level `level` (wl x hl) while
    lo <= coordinate < size - hi_off on that level; the other coordinate sits mid-image.  Rows: accepted, refused, ..."""
    s = float(1 << level)
    mx, my = F32(s * (wl // 2) + 0.25), F32(s * (hl // 2) + 0.75)
    return np.array([[F32(s * lo), my], [below(s * lo), my], [mx, F32(s * lo)], [mx, below(s * lo)],
                     [below(s * (wl - hi_off)), my], [F32(s * (wl - hi_off)), my], [mx, below(s * (hl - hi_off))], [mx, F32(s * (hl - hi_off))]], F32)


def inward(pts, d):
    """Each point moved d pixels towards the image centre along the axis on which it lies at the border."""
    out = pts.copy()
    for i, side in enumerate((0, 0, 1, 1, 0, 0, 1, 1)):
        out[i, side] += F32(d if i < 4 else -d)
    return out


@functools.lru_cache(maxsize=None)
def border_cases():
    """S62 at the last accepted and the first refused origin.  The template (2r + 3 samples from point - (r + 1)) is accepted
    while r + 1 <= coordinate < size - r - 2; the search window (2r + 1 samples from guess - r) while r <= coordinate <
    size - r - 1.  Template cases move the point itself; search cases keep the point 2 level-pixels inside and put the initial
    guess at the border, with one iteration, so that the guess tested is the one given.  note: kind, level, r."""
    out = []
    for r in (2, 7):
        # level 0 of the 64 x 48 frame, identical frames
        t = border_points(0, 64, 48, r + 1, r + 2)
        out.append(TrackCase("template border, level 0, r %d" % r, "a64", "a64", 0, t, prm(r, 0), kind="template", level=0, r=r))
        g = border_points(0, 64, 48, r, r + 1)
        out.append(TrackCase("search border, level 0, r %d" % r, "a64", "a64", 0, inward(g, 2.0), prm(r, 0, max_iters=1, flags=R.USE_INITIAL),
                             init=g, kind="search", level=0, r=r))
        # level 1 (66 x 49) of the 131 x 97 pair; the template case on the moved frame, so that a level that runs leaves a trace
        t = border_points(1, 66, 49, r + 1, r + 2)
        out.append(TrackCase("template border, level 1, r %d" % r, "a131", "b131", 1, t, prm(r, 1), kind="template", level=1, r=r))
        g = border_points(1, 66, 49, r, r + 1)
        out.append(TrackCase("search border, level 1, r %d" % r, "a131", "a131", 1, inward(g, 4.0),
                             prm(r, 1, max_iters=1, flags=R.USE_INITIAL), init=g, kind="search", level=1, r=r))
    return out


WEIGHT_R, WEIGHT_BASE = 3, 24.0
WEIGHT_CLASSES = ("w11 == 0", "w11 == 0, w01 and w10 > 0", "w11 == -1", "w00 == 16384", "w00 == 16384, a and b not 0", "all 4096")


def weight_class(wt, a, b):
    w00, w01, w10, w11 = (int(v) for v in wt)
    names = []
    if w11 == 0:
        names.append("w11 == 0")
        if w01 > 0 and w10 > 0:
            names.append("w11 == 0, w01 and w10 > 0")
    if w11 == -1:
        names.append("w11 == -1")
    if w00 == 16384:
        names.append("w00 == 16384")
        if a and b:
            names.append("w00 == 16384, a and b not 0")
    if w00 == w01 == w10 == w11 == 4096:
        names.append("all 4096")
    return names


def weights_of(x, y, r=WEIGHT_R, w=64, h=48):
    """The S62 weights of the template of point (x, y) on a w x h level, through the restatement."""
    ok, ix, iy, wt = R.window_origin(float(F32(x) - F32(r + 1)), float(F32(y) - F32(r + 1)), 2 * r + 3, w, h)
    assert ok
    return wt


@functools.lru_cache(maxsize=None)
def weight_points():
    """{class: (x, y)}: the first coordinates, scanning fractional parts of k 2^-15 and one float32 to either side for k < 48
    (and 1/2), whose template weights fall into each class of WEIGHT_CLASSES."""
    vals = []
    for k in list(range(48)) + [1 << 14]:
        v = F32(WEIGHT_BASE + k * 2.0 ** -15)
        vals += [v, above(v), below(v)]
    found = {}
    for x in vals:
        for y in vals:
            a, b = float(x) - np.floor(x), float(y) - np.floor(y)
            for name in weight_class(weights_of(x, y), a, b):
                found.setdefault(name, (x, y))
        if len(found) == len(WEIGHT_CLASSES):
            break
    return found


@functools.lru_cache(maxsize=None)
def weight_cases():
    """The points of weight_points() and a band of their neighbours, tracked into the moved frame: once from the point itself
    and once from an initial guess with the same fractional parts, so that both windows take the weights."""
    pts = np.array([xy for xy in weight_points().values()], F32)
    band = np.array([[F32(WEIGHT_BASE + k * 2.0 ** -15), above(WEIGHT_BASE + (k + 1) * 2.0 ** -15)] for k in range(24)], F32)
    pts = np.concatenate([pts, band, band[:, ::-1] + F32(8.0)])
    return [TrackCase("weights", "a64", "b64", 0, pts, prm(WEIGHT_R, 0)),
            TrackCase("weights, as initial guesses", "a64", "b64", 0, pts, prm(WEIGHT_R, 0, flags=R.USE_INITIAL), init=pts + F32(1.0))]


@functools.lru_cache(maxsize=None)
def level_cases():
    """prm.max_level and the pyramid's level count apart, in either direction: top = min(max_level, nlev - 1)."""
    pts = interior_points(131, 97, 8, 16, 5)
    out = [TrackCase("built 7 (3 levels), tracked with %d" % ml, "a131", "b131", 7, pts, prm(4, ml, fb_thresh=0.5)) for ml in (0, 1, 2)]
    out.append(TrackCase("built 0 (1 level), tracked with 7", "a131", "b131", 0, pts, prm(4, 7, fb_thresh=0.5)))
    return out


@functools.lru_cache(maxsize=None)
def eps_cases():
    pts = interior_points(131, 97, 8, 16, 6)
    return {"zero": TrackCase("eps 0, 100 iterations", "a131", "b131", 7, pts, prm(4, 7, max_iters=100, eps=0.0)),
            "large": TrackCase("eps 1e3", "a131", "b131", 0, pts, prm(4, 0, eps=1e3)),
            "usual": TrackCase("eps 0.01", "a131", "b131", 0, pts, prm(4, 0)),
            "one": TrackCase("one iteration", "a131", "b131", 0, pts, prm(4, 0, max_iters=1)),
            "identical": TrackCase("identical frames", "a131", "a131", 7, pts, prm(4, 7, fb_thresh=0.5))}


def edge_values(r):
    big = F32(1e6)
    return [big, -big, above(big), below(-big), F32(1e6 + r + 1), above(1e6 + r + 1), F32(-1e6 + r + 1), below(-1e6 + r + 1), F32(1e6 + r),
            above(1e6 + r), F32(-1e6 + r), below(-1e6 + r), INF, -INF, NAN]


@functools.lru_cache(maxsize=None)
def coordinate_cases():
    """Coordinates at and beyond the range test of S62 (|origin| <= 1e6), infinite and not a number, in x and in y apart; as
    points and as initial guesses of a point that tracks.  Row 0 is an ordinary point."""
    r = 3
    good = (F32(30.5), F32(20.25))
    rows = [good] + [(v, good[1]) for v in edge_values(r)] + [(good[0], v) for v in edge_values(r)]
    pts = np.array(rows, F32)
    out = []
    for built, ml in ((0, 0), (1, 1)):
        out.append(TrackCase("coordinates, max_level %d" % ml, "a64", "b64", built, pts, prm(r, ml, fb_thresh=0.5)))
        out.append(TrackCase("coordinates as initial guesses, max_level %d" % ml, "a64", "b64", built, np.tile(np.array(good, F32), (len(rows), 1)),
                             prm(r, ml, flags=R.USE_INITIAL), init=pts))
    return out


BIG_FIT7 = (896, 1024)          # at r = 6 the 15-wide template fits the 16 x 16 level 7 only at origin 0: 7 <= x / 128 < 8


@functools.lru_cache(maxsize=None)
def big_cases():
    """A dozen points through the 8 levels of the 1921 x 1921 pair: six inside the square in which the r = 6 template fits level
    7, six outside it, which join from a lower level."""
    rng = np.random.default_rng(8)
    inside = rng.uniform(BIG_FIT7[0] + 1, BIG_FIT7[1] - 1, (6, 2))
    outside = np.array([[300.5, 400.25], [1500.0, 200.75], [60.25, 1800.5], [1850.5, 1850.5], [960.0, 100.0], [1100.5, 960.25]])
    pts = np.concatenate([inside, outside]).astype(F32)
    return [TrackCase("1921 x 1921, 8 levels, r %d" % r, "big", "bigroll", 7, pts, prm(r, 7, fb_thresh=0.5)) for r in (2, 6)]


# ---- compaction cases -----------------------------------------------------------------------------------------------------------

COMPACT_CAPS = (1023, 1024, 1025, 2048, 2049)
COMPACT_PATTERNS = ("none first", "all first", "mix")
COMPACT_PRM = prm(2, 0)
LOST = (-50.0, -50.0)


@functools.lru_cache(maxsize=None)
def compact_case(cap, pattern):
    """cap points on the noise frame tracked into itself: a row is kept where it lies on the image, lost where it is LOST.
    'none first': rows 0 .. 1023 lost, a mix behind; 'all first': rows 0 .. 1023 kept, a mix behind; 'mix': a mix throughout whose
    kept rows include 1023 and 1024."""
    rng = np.random.default_rng(cap * 10 + COMPACT_PATTERNS.index(pattern))
    pts = interior_points(64, 48, 6, cap, cap)
    keep = rng.integers(0, 2, cap).astype(bool)
    if pattern == "none first":
        keep[:1024] = False
    elif pattern == "all first":
        keep[:1024] = True
    else:
        keep[1023:1025] = True
    if cap > 1024 and pattern != "mix":
        keep[1024] = True                                            # a kept row behind the first chunk, and a lost one
        keep[1025:1026] = False
    pts[~keep] = LOST
    case = TrackCase("compaction, cap %d, %s" % (cap, pattern), "n64", "n64", 0, pts, COMPACT_PRM)
    case.keep = keep
    return case


def compact_counts(cap):
    """Device counts: none, 1024, 1025 (clamped to cap), cap - 1 -> rows used."""
    return [(None, cap), (1024, min(1024, cap)), (1025, min(1025, cap)), (cap - 1, cap - 1)]


# ---- corner cases ---------------------------------------------------------------------------------------------------------------

GROUND, DOT, WEAK_DOT, PITCH = 40, 200, 120, 8


def dot_row(n, r=1, skip=0, amps=(DOT,)):
    """n dots on one row, PITCH apart, r + 4 from every border; the first `skip` positions are left empty."""
    m = r + 4
    img = np.full((max(16, 2 * m + 1), 2 * m + PITCH * (n - 1) + 1), GROUND, np.uint8)
    for i in range(skip, n):
        img[img.shape[0] // 2, m + PITCH * i] = amps[i % len(amps)]
    return img


def dot_grid(cols, rows, r=1):
    m = r + 4
    img = np.full((2 * m + PITCH * (rows - 1) + 1, 2 * m + PITCH * (cols - 1) + 1), GROUND, np.uint8)
    img[m::PITCH, m::PITCH][:rows, :cols] = DOT
    return img


RANK_COUNTS = (255, 256, 257, 511, 512, 513, 1024, 1025)
TILE_RADII = (1, 15)


def tile_shapes(r):
    """(w, h) around the 64 x 16 tile of corner_extrema: V = (w - 2r - 3) x (h - 2r - 3) one pixel, one tile, one tile and a pixel,
    two tiles, two and a pixel wide, and the same in height; sides below 16 raised to 16."""
    ws = [max(16, 2 * r + 3 + d) for d in (1, 64, 65, 128, 129)]
    hs = [max(16, 2 * r + 3 + d) for d in (1, 16, 17, 33)]
    shapes = [(w, h) for h in (hs[0], hs[2]) for w in ws] + [(w, h) for w in (ws[1], ws[2]) for h in hs]
    return sorted(set(shapes))


@functools.lru_cache(maxsize=None)
def corner_image(name):
    kind, _, arg = name.partition(":")
    if kind == "row":
        return dot_row(int(arg))
    if kind == "row-1":
        return dot_row(int(arg), skip=1)
    if kind == "two":
        return dot_row(int(arg), amps=(DOT, WEAK_DOT))
    if kind == "grid":
        return dot_grid(33, 32)
    if kind == "tile":
        w, h = (int(v) for v in arg.split("x"))
        return noise_image(w, h, 1000 * w + h)
    raise KeyError(name)


class CornerCase:
    """One call of the detector on corner_image(image).  rows, candidates: what the case is named after (None: not fixed)."""

    def __init__(self, tag, image, r=1, min_eig=1e-4, quality=0.0, min_dist=0.0, max_corners=4096, keep=None, rows=None, candidates=None):
        self.tag, self.image, self.r, self.min_eig, self.quality, self.min_dist = tag, image, r, min_eig, quality, min_dist
        self.max_corners, self.keep, self.rows, self.candidates = max_corners, keep, rows, candidates
        self._want = None

    def want(self):
        """(xy, score, number of candidates) of the restatement, computed once."""
        if self._want is None:
            self._want = K.detect(corner_image(self.image), self.r, self.min_eig, self.quality, self.min_dist, self.keep, self.max_corners)
        return self._want

    def __repr__(self):
        return self.tag


@functools.lru_cache(maxsize=None)
def tile_cases():
    return [CornerCase("tile %d x %d, r %d" % (w, h, r), "tile:%dx%d" % (w, h), r, 0.0, max_corners=8192) for r in TILE_RADII for w, h in tile_shapes(r)]


@functools.lru_cache(maxsize=None)
def rank_cases():
    """One row of n equal dots, no minimum distance: n candidates of one score come back in scan order."""
    return [CornerCase("%d dots" % n, "row:%d" % n, max_corners=n + 7, rows=n, candidates=n) for n in RANK_COUNTS]


def grid_keep():
    """Ten keep points on dots of the grid, spread over its rows."""
    return np.array([[5 + PITCH * (3 * i + 1), 5 + PITCH * (3 * i + 2)] for i in range(10)], F32)


@functools.lru_cache(maxsize=None)
def select_cases():
    out = [CornerCase("1025 dots, min_dist 8.5", "row:1025", min_dist=8.5, rows=513, candidates=1025),
           CornerCase("1024 dots from the second position, min_dist 8.5", "row-1:1025", min_dist=8.5, rows=512, candidates=1024),
           CornerCase("1025 dots, min_dist 16.5", "row:1025", min_dist=16.5, rows=342, candidates=1025)]
    # the limit at a chunk end (ranks 0 .. 511 hold 256 accepted dots, 0 .. 1023 hold 512), one before, one after, and mid-chunk
    for mc in (100, 255, 256, 257, 512, 513):
        out.append(CornerCase("1025 dots, min_dist 8.5, max_corners %d" % mc, "row:1025", min_dist=8.5, max_corners=mc, rows=min(mc, 513), candidates=1025))
    for mc in (100, 511, 512, 513, 1024):
        out.append(CornerCase("1025 dots, min_dist 0, max_corners %d" % mc, "row:1025", max_corners=mc, rows=mc, candidates=1025))
    for n in RANK_COUNTS[:-1]:
        out.append(CornerCase("%d dots, min_dist 8.5" % n, "row:%d" % n, min_dist=8.5, rows=(n + 1) // 2, candidates=n))
    out.append(CornerCase("600 strong + 600 weak dots, min_dist 8.5", "two:1200", min_dist=8.5, rows=600, candidates=1200))
    out.append(CornerCase("33 x 32 grid, min_dist 8.5", "grid", min_dist=8.5, rows=528, candidates=1056))
    out.append(CornerCase("33 x 32 grid, min_dist 8.5, keep points", "grid", min_dist=8.5, keep=grid_keep(), candidates=1056))
    return out
