"""ctypes loader of tests/warp_ref.c, the plain-C restatement of SPEC S75-S78 (image warp by a 3 x 3 or lifted 2 x 3 model with
integer bilinear sampling at 1/32 pixel; the point transform), an independent numpy statement of the same sections, and the
inputs both warp test files use.  Built once per process through tests/cref.py."""
import ctypes as C

import numpy as np

import cref

INVERT, REPLICATE, AFFINE = 1, 2, 4

_L = None
_V, _I = C.c_void_p, C.c_int


def lib():
    global _L
    if _L is None:
        _L = cref.load("warp_ref", {
            "warp_model": [_V, _I, _V],
            "warp_position": [_V, _I, _I, _V, _V],
            "warp_image": [_V, _I, _I, _I, _V, _I, _I, _V, _I, _I, _I, _V, _V],
            "warp_points": [_V, _I, _V, _I, _V],
        }, {"warp_points": None})
    return _L


def _model(M, flags):
    M = np.ascontiguousarray(M, np.float64).reshape(-1)
    assert M.size == (6 if flags & AFFINE else 9)
    return M


def model(M, flags=0):
    """(status, m (9,) f64): S75."""
    m = np.zeros(9)
    return lib().warp_model(cref.ptr(_model(M, flags)), flags, cref.ptr(m)), m


def position(m, x, y):
    """S76 for one pixel: (inside, qx, qy)."""
    qx, qy = C.c_int32(0), C.c_int32(0)
    m = np.ascontiguousarray(m, np.float64)
    ok = lib().warp_position(cref.ptr(m), x, y, C.addressof(qx), C.addressof(qy))
    return ok, qx.value, qy.value


def warp(src, M, flags=0, border=0, dw=None, dh=None, sw=None, dst=None, dstride=None):
    """The C restatement: (dst (dh, dstride) u8 with dw columns written, valid (dh, dw) u8, status, n_valid).  With sw given, src
    holds rows of src.shape[1] >= sw bytes; with dst given it is written in place (the bytes beyond dw stay)."""
    src = np.ascontiguousarray(src, np.uint8)
    sh, sstride = src.shape
    sw = sstride if sw is None else sw
    dw = sw if dw is None else dw
    dh = sh if dh is None else dh
    dstride = dw if dstride is None else dstride
    if dst is None:
        dst = np.zeros((dh, dstride), np.uint8)
    assert dst.shape == (dh, dstride) and dst.flags.c_contiguous
    valid, info = np.zeros((dh, dw), np.uint8), np.zeros(2, np.int32)
    st = lib().warp_image(cref.ptr(src), sw, sh, sstride, cref.ptr(_model(M, flags)), flags, border, cref.ptr(dst), dw, dh, dstride,
                          cref.ptr(valid), cref.ptr(info))
    assert st == info[0]
    return dst, valid, int(info[0]), int(info[1])


def points(M, pts, flags=0):
    """The C restatement of S78: (n, 2) f32."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    out = np.zeros_like(pts)
    lib().warp_points(cref.ptr(_model(M, flags)), flags, cref.ptr(pts), pts.shape[0], cref.ptr(out))
    return out


# ---- the numpy statement -----------------------------------------------------------------------------------------------------

def np_model(M, flags=0):
    """S75 in numpy: (status, m (9,) f64)."""
    M = _model(M, flags)
    a = np.concatenate([M, [0.0, 0.0, 1.0]]) if flags & AFFINE else M.copy()
    with np.errstate(all="ignore"):
        def cof(i, j, k, l):
            return a[i] * a[j] - a[k] * a[l]
        adj = np.array([cof(4, 8, 5, 7), cof(2, 7, 1, 8), cof(1, 5, 2, 4),
                        cof(5, 6, 3, 8), cof(0, 8, 2, 6), cof(2, 3, 0, 5),
                        cof(3, 7, 4, 6), cof(1, 6, 0, 7), cof(0, 4, 1, 3)])
        det = (a[0] * adj[0] + a[1] * adj[3]) + a[2] * adj[6]
    m = adj if flags & INVERT else a
    if not M.any():
        return 2, m
    if not np.isfinite(M).all() or det == 0.0 or not np.isfinite(det):
        return 1, m
    return 0, m


def np_positions(m, dw, dh):
    """S76 for the whole output: (inside (dh, dw) bool, qx, qy (dh, dw) int64)."""
    ys, xs = np.mgrid[0:dh, 0:dw].astype(np.float64)
    with np.errstate(all="ignore"):
        X = (m[0] * xs + m[1] * ys) + m[2]
        Y = (m[3] * xs + m[4] * ys) + m[5]
        W = (m[6] * xs + m[7] * ys) + m[8]
        r = 32.0 / W
        fx, fy = X * r, Y * r
        inside = (W != 0.0) & np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < 2.0 ** 30) & (np.abs(fy) < 2.0 ** 30)
    qx = np.rint(np.where(inside, fx, 0.0)).astype(np.int64)
    qy = np.rint(np.where(inside, fy, 0.0)).astype(np.int64)
    return inside, qx, qy


def np_warp(src, M, flags=0, border=0, dw=None, dh=None):
    """S75-S77 in numpy: (dst (dh, dw) u8, valid (dh, dw) u8, status, n_valid)."""
    src = np.ascontiguousarray(src, np.uint8)
    sh, sw = src.shape
    dw = sw if dw is None else dw
    dh = sh if dh is None else dh
    status, m = np_model(M, flags)
    if status:
        return np.full((dh, dw), border, np.uint8), np.zeros((dh, dw), np.uint8), status, 0
    inside, qx, qy = np_positions(m, dw, dh)
    x0, y0, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
    I = src.astype(np.int64)
    total = np.zeros((dh, dw), np.int64)
    valid = inside.copy()
    for j, wy in ((0, 32 - ay), (1, ay)):
        for i, wx in ((0, 32 - ax), (1, ax)):
            wgt = wx * wy
            xx, yy = x0 + i, y0 + j
            tap_in = (xx >= 0) & (xx < sw) & (yy >= 0) & (yy < sh)
            v = I[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)]
            if not flags & REPLICATE:
                v = np.where(tap_in, v, border)
            total += wgt * v
            valid &= tap_in | (wgt == 0)
    out = np.where(inside, (total + 512) >> 10, border)
    return out.astype(np.uint8), valid.astype(np.uint8), 0, int(valid.sum())


def np_points(M, pts, flags=0):
    """S78 in numpy: (n, 2) f32."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    status, m = np_model(M, flags)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        X = (m[0] * x + m[1] * y) + m[2]
        Y = (m[3] * x + m[4] * y) + m[5]
        W = (m[6] * x + m[7] * y) + m[8]
        qx, qy = X / W, Y / W
        bad = (W == 0.0) | ~np.isfinite(qx) | ~np.isfinite(qy) | (status != 0)
        out = np.stack([qx, qy], 1).astype(np.float32)
    out[bad] = np.nan
    return out


def same_floats(a, b):
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and (a[~nan].view(np.uint32) == b[~nan].view(np.uint32)).all()


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------

def random_source(w, h, seed=0):
    return np.random.default_rng(1000 * w + h + seed).integers(0, 256, (h, w), dtype=np.uint8)


def homography(seed):
    """Identity plus uniform noise: 0.05 on the 2 x 2 part, 8 px on the translation, 2e-4 on the last row."""
    rng = np.random.default_rng(7500 + seed)
    H = np.eye(3)
    H[:2, :2] += rng.uniform(-0.05, 0.05, (2, 2))
    H[:2, 2] += rng.uniform(-8.0, 8.0, 2)
    H[2] += rng.uniform(-2e-4, 2e-4, 3)
    return H


def smooth_source(w=160, h=120):
    """rint(127.5 + 100 sin(x / 7) cos(y / 9)): neighbours differ by at most 15 across and 11 down."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.rint(127.5 + 100.0 * np.sin(xs / 7.0) * np.cos(ys / 9.0)).astype(np.uint8)


def bilinear_fp64(img, sx, sy):
    """The fp64 bilinear resampling of lk_ref.frame_r / describe_ref.rotate_frame at given source positions:
    (values rounded to u8, inside = the position lies in [0, w - 1] x [0, h - 1])."""
    h, w = img.shape
    with np.errstate(all="ignore"):
        inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    sxc, syc = np.clip(np.where(inside, sx, 0.0), 0, w - 1), np.clip(np.where(inside, sy, 0.0), 0, h - 1)
    x0, y0 = np.minimum(np.floor(sxc).astype(np.int64), w - 2), np.minimum(np.floor(syc).astype(np.int64), h - 2)
    a, b = sxc - x0, syc - y0
    I = img.astype(np.float64)
    v = I[y0, x0] * (1 - a) * (1 - b) + I[y0, x0 + 1] * a * (1 - b) + I[y0 + 1, x0] * (1 - a) * b + I[y0 + 1, x0 + 1] * a * b
    return np.clip(np.rint(v), 0, 255).astype(np.uint8), inside


def quarter_turn(h_src):
    return np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, h_src - 1.0], [0.0, 0.0, 1.0]])


def translation(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])
