"""ctypes loader of tests/corner_ref.c, the plain-C restatement of SPEC S67-S70 (minimum-eigenvalue corners, ranking, greedy
minimum-distance selection), and the small images both corner test files use.  Built once per process through tests/cref.py."""
import ctypes as C

import numpy as np

import cref

_L = None
_V, _I, _F = C.c_void_p, C.c_int, C.c_float


def lib():
    global _L
    if _L is None:
        _L = cref.load("corner_ref", {
            "corner_in_v": [_I, _I, _I, _I, _I],
            "corner_response": [_V, _I, _I, _I, _I, _I],
            "corner_response_plane": [_V, _I, _I, _I, _V],
            "corner_candidates": [_V, _I, _I, _I, _F, _I, _V, _V],
            "corner_rank": [_I, _V, _V, _F, _V, _V],
            "corner_select": [_I, _I, _V, _V, _F, _V, _I, _I, _V, _V, _V],
            "corner_detect": [_V, _I, _I, _I, _F, _F, _F, _V, _I, _I, _V, _V, _V],
        }, {"corner_response": C.c_double})
    return _L


def _img(img):
    img = np.ascontiguousarray(img, np.uint8)
    assert img.ndim == 2
    return img


def in_v(shape, r, x, y):
    return bool(lib().corner_in_v(shape[1], shape[0], r, x, y))


def response(img, r, x, y):
    """e of S67 at one pixel of V (fp64)."""
    img = _img(img)
    assert in_v(img.shape, r, x, y)
    return lib().corner_response(cref.ptr(img), img.shape[1], img.shape[0], r, x, y)


def candidates(img, r, min_eig):
    """S68: (pos (n,) int32 = y * w + x in scan order, e (n,) fp64)."""
    img = _img(img)
    h, w = img.shape
    pos, e = np.zeros(w * h, np.int32), np.zeros(w * h, np.float64)
    n = lib().corner_candidates(cref.ptr(img), w, h, r, min_eig, w * h, cref.ptr(pos), cref.ptr(e))
    return pos[:n].copy(), e[:n].copy()


def rank(pos, e, quality=0.0):
    """S69: (rank_pos, rank_s fp32, kept = ranks that survive the quality cut)."""
    n = pos.shape[0]
    rpos, rs = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32)
    kept = lib().corner_rank(n, cref.ptr(np.ascontiguousarray(pos, np.int32)), cref.ptr(np.ascontiguousarray(e, np.float64)), quality,
                             cref.ptr(rpos), cref.ptr(rs))
    return rpos[:n], rs[:n], kept


def keep_array(keep):
    return np.zeros((0, 2), np.float32) if keep is None else np.ascontiguousarray(keep, np.float32).reshape(-1, 2)


def select(w, rpos, rs, n, min_dist, keep, max_corners):
    """S70 over the first n ranks: (xy (m, 2) f32, score (m,) f32, fate (n,) u8: 1 accepted, 2 rejected, 0 not walked)."""
    keep = keep_array(keep)
    xy, sc, fate = np.zeros((max(max_corners, 1), 2), np.float32), np.zeros(max(max_corners, 1), np.float32), np.zeros(max(n, 1), np.uint8)
    m = lib().corner_select(n, w, cref.ptr(np.ascontiguousarray(rpos, np.int32)), cref.ptr(np.ascontiguousarray(rs, np.float32)), min_dist,
                            cref.ptr(keep), keep.shape[0], max_corners, cref.ptr(xy), cref.ptr(sc), cref.ptr(fate))
    return xy[:m].copy(), sc[:m].copy(), fate[:n].copy()


def detect(img, r, min_eig=1e-4, quality=0.0, min_dist=0.0, keep=None, max_corners=1 << 20):
    """S67-S70: (xy (m, 2) f32, score (m,) f32, number of candidates)."""
    img = _img(img)
    h, w = img.shape
    keep = keep_array(keep)
    rows = max(min(max_corners, w * h), 1)
    xy, sc, nc = np.zeros((rows, 2), np.float32), np.zeros(rows, np.float32), C.c_int()
    m = lib().corner_detect(cref.ptr(img), w, h, r, min_eig, quality, min_dist, cref.ptr(keep), keep.shape[0], min(max_corners, rows),
                            cref.ptr(xy), cref.ptr(sc), C.addressof(nc))
    return xy[:m].copy(), sc[:m].copy(), nc.value


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------

def random_image(w, h):
    return np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)


def block_pattern(w=64, h=48, cell=8):
    """A checkerboard of cell x cell blocks of 40 and 200: its block sums repeat exactly, so whole sets of pixels carry the same
    fp64 response and the 3 x 3 rule meets exact ties."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx // cell) + (yy // cell)) % 2 == 0, 40, 200).astype(np.uint8)


def two_pixel_plateau(w=40, h=40):
    """Flat ground with one structure that is mirror-symmetric about the line between columns 19 and 20: the responses at
    (19, y) and (20, y) are equal, so the two strongest pixels form a two-pixel plateau."""
    img = np.full((h, w), 90, np.uint8)
    img[18:22, 18:22] = 200
    img[19:21, 19:21] = 30
    img[16, 19:21] = 140
    return img


def constant_image(w=40, h=40):
    return np.full((h, w), 93, np.uint8)
