"""ctypes loader of tests/describe_ref.c, the plain-C restatement of SPEC S71-S74 (oriented 256-bit descriptors of given points
on a pyramid level), an independent numpy statement of the same sections, and the inputs both describe test files use.  Built
once per process through tests/cref.py; the levels come from lk_ref.Pyramid."""
import ctypes as C

import numpy as np

import corner_ref as K
import cref
import features_bits_ref as B
import lk_ref as R

UPRIGHT = 1
TABLE_SHA256 = "a7b37474c61bbdefd170703b090df3e755d48c3fa3a905de128af1c4515ea2ab"      # int8 [37][256][4]
Q20_SHA256 = "f7878db41a53e8dfcc22e227be377a819a17223fde897421ef25d75dfe140741"        # C[0..35], S[0..35], little-endian int32

_L = None
_V, _I, _F = C.c_void_p, C.c_int, C.c_float


def lib():
    global _L
    if _L is None:
        _L = cref.load("describe_ref", {
            "describe_tables": [_V, _V],
            "describe_bin": [C.c_int32, C.c_int32],
            "describe_position": [_F, _F, _I, _I, _I, _V, _V],
            "describe_moments": [_V, _I, _I, _I, _V, _V],
            "describe_points": [_V, _I, _I, _I, _I, _V, _I, _V, _V, _V],
        })
    return _L


def tables():
    """(q20 (72,) int32 = C then S, steered (37, 256, 4) int8) of the C restatement."""
    q20, st = np.zeros(72, np.int32), np.zeros((37, 256, 4), np.int8)
    lib().describe_tables(cref.ptr(q20), cref.ptr(st))
    return q20, st


def bin_of(m10, m01):
    return lib().describe_bin(int(m10), int(m01))


def points_array(pts):
    return np.ascontiguousarray(pts, np.float32).reshape(-1, 2)


def describe(plane, level, pts, flags=0):
    """The C restatement on one level plane (h, w) u8: (desc (n, 32) u8, valid (n,) u8, bin (n,) u8)."""
    plane = np.ascontiguousarray(plane, np.uint8)
    pts = points_array(pts)
    n = pts.shape[0]
    desc, valid, bins = np.zeros((max(n, 1), 32), np.uint8), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    nv = lib().describe_points(cref.ptr(plane), plane.shape[1], plane.shape[0], level, 1 if flags & UPRIGHT else 0, cref.ptr(pts), n,
                               cref.ptr(desc), cref.ptr(valid), cref.ptr(bins))
    assert nv == int(valid[:n].sum())
    return desc[:n], valid[:n], bins[:n]


def describe_image(img, level, pts, flags=0, max_level=None):
    """describe() on level `level` of the pyramid of img."""
    pyr = R.Pyramid(img, level if max_level is None else max_level)
    assert level < pyr.n
    return describe(pyr.levels[level], level, pts, flags)


# ---- the numpy statement -----------------------------------------------------------------------------------------------------

def np_tables():
    """S72 / S73 in numpy: (q20 (72,) int32, steered (37, 256, 4) int8)."""
    b = np.arange(36)
    theta = (b + 0.5) / 36 * 2 * np.pi - np.pi
    cs, sn = np.cos(theta), np.sin(theta)
    q20 = np.concatenate([np.rint(1048576.0 * cs), np.rint(1048576.0 * sn)]).astype(np.int32)
    base = B.base_pattern()
    st = np.zeros((37, 256, 4), np.int8)
    st[36] = base
    f = base.astype(np.float64)
    for k in range(36):
        for p in (0, 2):
            x, y = f[:, p], f[:, p + 1]
            st[k, :, p] = np.rint(cs[k] * x - sn[k] * y).astype(np.int8)
            st[k, :, p + 1] = np.rint(sn[k] * x + cs[k] * y).astype(np.int8)
    return q20, st


_NP = {}


def np_bin(m10, m01):
    """S72 for arrays of moments: int64 dots, the first maximum."""
    if "q20" not in _NP:
        _NP["q20"], _NP["steer"] = np_tables()
    q = _NP["q20"].astype(np.int64)
    m10, m01 = np.atleast_1d(np.asarray(m10, np.int64)), np.atleast_1d(np.asarray(m01, np.int64))
    dots = m10[:, None] * q[None, :36] + m01[:, None] * q[None, 36:]
    return np.argmax(dots, axis=1)


def np_describe(plane, level, pts, flags=0):
    """S71-S74 in numpy, one point at a time."""
    if "q20" not in _NP:
        _NP["q20"], _NP["steer"] = np_tables()
    steer = _NP["steer"].astype(np.int64)
    plane = np.ascontiguousarray(plane, np.uint8)
    h, w = plane.shape
    I = plane.astype(np.int64)
    # 5 x 5 box sums of every pixel that has one: box[y - 2, x - 2]
    cum = np.zeros((h + 1, w + 1), np.int64)
    cum[1:, 1:] = I.cumsum(0).cumsum(1)
    box = cum[5:, 5:] - cum[:-5, 5:] - cum[5:, :-5] + cum[:-5, :-5]
    dy, dx = np.mgrid[-15:16, -15:16]
    disc = dx * dx + dy * dy <= 225
    assert disc.sum() == 709
    pts = points_array(pts)
    n = pts.shape[0]
    desc, valid, bins = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8), np.full(n, 255, np.uint8)
    scale = np.float32(1.0) / np.float32(1 << level)
    for k in range(n):
        x, y = pts[k]
        if not (np.isfinite(x) and np.isfinite(y)) or abs(x) > np.float32(1e6) or abs(y) > np.float32(1e6):
            continue
        cx, cy = int(np.rint(np.float32(x * scale))), int(np.rint(np.float32(y * scale)))
        if not (17 <= cx <= w - 18 and 17 <= cy <= h - 18):
            continue
        if flags & UPRIGHT:
            b = 36
        else:
            patch = I[cy - 15:cy + 16, cx - 15:cx + 16]
            b = int(np_bin((dx * patch)[disc].sum(), (dy * patch)[disc].sum())[0])
        t = steer[b]
        a1 = box[cy + t[:, 1] - 2, cx + t[:, 0] - 2]
        a2 = box[cy + t[:, 3] - 2, cx + t[:, 2] - 2]
        desc[k] = np.packbits(a1 < a2, bitorder="little")
        valid[k] = 1
        bins[k] = b
    return desc, valid, bins


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------

SMALL = ((35, 35), (36, 40), (67, 35))          # (w, h): one describable pixel; a 2 x 6 region; wider than high


def small_image(w, h):
    return K.random_image(w, h)


def constant_image(w=48, h=40):
    return np.full((h, w), 93, np.uint8)


def fixture_corners():
    """(first frame, its 344 corners (344, 2) f32)."""
    img = R.fixture()[0]
    return img, K.detect(img, 10, 1e-4, 0.01, 8.0, None, 500)[0]


def lattice(w, h):
    """Points of a w x h level-0 image that sit on and around every edge of S71: x.5 positions (17.5 -> 18, 16.5 -> 16, ties to
    even), centres 16 / 17 and w - 18 / w - 17, then negative, non-finite and > 1e6 coordinates."""
    def axis(n):
        return [15.0, 16.0, 16.5, 17.0, 17.4, 17.5, n - 18.5, n - 18.0, n - 17.5, n - 17.0, (n - 1) / 2.0]
    pts = [(x, y) for y in axis(h) for x in axis(w)]
    mx, my = (w - 1) / 2.0, (h - 1) / 2.0
    nan, inf = float("nan"), float("inf")
    pts += [(-5.0, my), (mx, -5.0), (-17.0, -17.0), (nan, my), (mx, nan), (inf, my), (mx, -inf), (1.5e6, my), (mx, -2e6), (1e6, my),
            (1000001.0, my), (mx, my)]
    return np.array(pts, np.float32)


def alternating(w, h, n=67):
    """n points, valid and invalid in turn, so every group of four consecutive points mixes both."""
    rng = np.random.default_rng(w * 100 + h)
    good = np.stack([rng.uniform(17, w - 18, n), rng.uniform(17, h - 18, n)], 1)
    bad = np.stack([rng.uniform(-30, 10, n), rng.uniform(0, h, n)], 1)
    pts = np.where((np.arange(n) % 2 == 0)[:, None], good, bad).astype(np.float32)
    pts[5] = (np.nan, 20.0)
    return pts


def _rot(deg):
    t = np.deg2rad(deg)
    return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])


def rotate_map(xy, shape, deg):
    """The true map of rotate_frame, fp64: rotation by deg about the image centre."""
    h, w = shape
    c = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    return (np.asarray(xy, np.float64) - c) @ _rot(deg).T + c


def rotate_frame(img, deg):
    """out(map(x)) = img(x) by fp64 bilinear resampling at the inverse map; source positions outside the frame give 0."""
    h, w = img.shape
    c = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    src = (np.stack([xs.ravel(), ys.ravel()], 1) - c) @ _rot(deg) + c
    sx, sy = src[:, 0], src[:, 1]
    inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    sxc, syc = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
    x0, y0 = np.minimum(np.floor(sxc).astype(np.int64), w - 2), np.minimum(np.floor(syc).astype(np.int64), h - 2)
    a, b = sxc - x0, syc - y0
    I = img.astype(np.float64)
    v = I[y0, x0] * (1 - a) * (1 - b) + I[y0, x0 + 1] * a * (1 - b) + I[y0 + 1, x0] * (1 - a) * b + I[y0 + 1, x0 + 1] * a * b
    return np.clip(np.rint(np.where(inside, v, 0.0)), 0, 255).astype(np.uint8).reshape(h, w)


_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(q, t):
    """(nq, nt) int32 distances of 32-byte rows."""
    return _POP[q[:, None, :] ^ t[None, :, :]].sum(axis=2)
