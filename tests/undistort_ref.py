"""ctypes loader of tests/undistort_ref.c, the plain-C restatement of SPEC S79-S83 (the 5-coefficient lens model, points through
it both ways, undistorting an image, the map and the remap), an independent numpy statement of the same sections, and the inputs
both undistort test files use.  Built once per process through tests/cref.py.

Everywhere: K and K_new are (fx, fy, cx, cy), lens is (k1, k2, p1, p2, k3) or None, R is 3 x 3 or None, K_new may be None."""
import ctypes as C

import numpy as np

import cref

REPLICATE = 2
INT32_MIN = -2 ** 31

_L = None
_V, _I, _D = C.c_void_p, C.c_int, C.c_double


def lib():
    global _L
    if _L is None:
        _L = cref.load("undistort_ref", {
            "und_forward": [_V, _V, _D, _D, _V],
            "und_source_position": [_V, _V, _V, _V, _D, _D, _V],
            "und_distort_points": [_V, _V, _V, _V, _V, _I, _V],
            "und_undistort_points": [_V, _V, _V, _V, _I, _D, _V, _I, _V],
            "und_position": [_V, _V, _V, _V, _I, _I, _V, _V],
            "und_map": [_V, _V, _V, _V, _I, _I, _V],
            "und_remap": [_V, _I, _I, _I, _V, _I, _I, _V, _I, _I, _I, _V],
            "und_image": [_V, _I, _I, _I, _V, _V, _V, _V, _I, _I, _V, _I, _I, _I, _V],
        }, {"und_forward": _D, "und_distort_points": None, "und_undistort_points": None, "und_map": None})
    return _L


def _vec(a, n):
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    assert a.size == n
    return a


def _model(K, lens, R, K_new):
    """The four arrays (kept alive by the caller) and their pointers, None -> NULL."""
    arrs = (_vec(K, 4), _vec(lens, 5), _vec(R, 9), _vec(K_new, 4))
    return arrs, [None if a is None else cref.ptr(a) for a in arrs]


def forward(K, lens, x, y):
    """S79 for one normalised point: (u, v, rad)."""
    arrs, p = _model(K, lens, None, None)
    uv = np.zeros(2)
    rad = lib().und_forward(p[0], p[1], x, y, cref.ptr(uv))
    return uv[0], uv[1], rad


def source_position(K, lens, R, K_new, u, v):
    """S80 unrounded for one ideal pixel: (ok, sx, sy)."""
    arrs, p = _model(K, lens, R, K_new)
    s = np.zeros(2)
    ok = lib().und_source_position(p[0], p[1], p[2], p[3], float(u), float(v), cref.ptr(s))
    return ok, s[0], s[1]


def source_positions(K, lens, R, K_new, dw, dh):
    """S80 unrounded for every output pixel: (ok (dh, dw) bool, sx, sy (dh, dw) f64)."""
    ok, sx, sy = np.zeros((dh, dw), bool), np.zeros((dh, dw)), np.zeros((dh, dw))
    for y in range(dh):
        for x in range(dw):
            ok[y, x], sx[y, x], sy[y, x] = source_position(K, lens, R, K_new, x, y)
    return ok, sx, sy


def _pts(pts):
    return np.ascontiguousarray(pts, np.float32).reshape(-1, 2)


def distort_points(K, lens, R, K_new, pts):
    """The C restatement of S80: (n, 2) f32."""
    arrs, p = _model(K, lens, R, K_new)
    pts = _pts(pts)
    out = np.zeros_like(pts)
    lib().und_distort_points(p[0], p[1], p[2], p[3], cref.ptr(pts), pts.shape[0], cref.ptr(out))
    return out


def undistort_points(K, lens, R, K_new, pts, iters=None, tol_px=None):
    """The C restatement of S81: (n, 2) f32; iters, tol_px default to ITERS, TOL_PX below."""
    iters, tol_px = ITERS if iters is None else iters, TOL_PX if tol_px is None else tol_px
    arrs, p = _model(K, lens, R, K_new)
    pts = _pts(pts)
    out = np.zeros_like(pts)
    lib().und_undistort_points(p[0], p[1], p[2], p[3], iters, tol_px, cref.ptr(pts), pts.shape[0], cref.ptr(out))
    return out


def position(K, lens, R, K_new, x, y):
    """S82 for one output pixel: (usable, qx, qy)."""
    arrs, p = _model(K, lens, R, K_new)
    qx, qy = C.c_int32(0), C.c_int32(0)
    ok = lib().und_position(p[0], p[1], p[2], p[3], x, y, C.addressof(qx), C.addressof(qy))
    return ok, qx.value, qy.value


def make_map(K, lens, R, K_new, dw, dh):
    """S83: (dh, dw, 2) int32."""
    arrs, p = _model(K, lens, R, K_new)
    m = np.zeros((dh, dw, 2), np.int32)
    lib().und_map(p[0], p[1], p[2], p[3], dw, dh, cref.ptr(m))
    return m


def _image_args(src, sw, dw, dh, dst, dstride):
    src = np.ascontiguousarray(src, np.uint8)
    sh, sstride = src.shape
    sw = sstride if sw is None else sw
    dw = sw if dw is None else dw
    dh = sh if dh is None else dh
    dstride = dw if dstride is None else dstride
    if dst is None:
        dst = np.zeros((dh, dstride), np.uint8)
    assert dst.shape == (dh, dstride) and dst.flags.c_contiguous
    return src, sw, sh, sstride, dw, dh, dst, dstride


def remap(src, m, flags=0, border=0, sw=None, dst=None, dstride=None):
    """The C restatement of S83: (dst (dh, dstride) u8 with dw columns written, valid (dh, dw) u8, n_valid)."""
    m = np.ascontiguousarray(m, np.int32)
    dh, dw = m.shape[:2]
    src, sw, sh, sstride, dw, dh, dst, dstride = _image_args(src, sw, dw, dh, dst, dstride)
    valid = np.zeros((dh, dw), np.uint8)
    n = lib().und_remap(cref.ptr(src), sw, sh, sstride, cref.ptr(m), int(bool(flags & REPLICATE)), border, cref.ptr(dst), dw, dh, dstride,
                        cref.ptr(valid))
    return dst, valid, n


def undistort(src, K, lens, R=None, K_new=None, flags=0, border=0, dw=None, dh=None, sw=None, dst=None, dstride=None):
    """The C restatement of S82 + S77 without a map: (dst (dh, dstride) u8 with dw columns written, valid (dh, dw) u8, n_valid).
    With sw given, src holds rows of src.shape[1] >= sw bytes; with dst given it is written in place (the bytes beyond dw stay)."""
    arrs, p = _model(K, lens, R, K_new)
    src, sw, sh, sstride, dw, dh, dst, dstride = _image_args(src, sw, dw, dh, dst, dstride)
    valid = np.zeros((dh, dw), np.uint8)
    n = lib().und_image(cref.ptr(src), sw, sh, sstride, p[0], p[1], p[2], p[3], int(bool(flags & REPLICATE)), border, cref.ptr(dst), dw, dh,
                        dstride, cref.ptr(valid))
    return dst, valid, n


# ---- the numpy statement -----------------------------------------------------------------------------------------------------

def np_forward_norm(lens, x, y):
    """S79 on normalised coordinates (arrays): (xd, yd, rad)."""
    k1, k2, p1, p2, k3 = (0.0,) * 5 if lens is None else [float(c) for c in lens]
    with np.errstate(all="ignore"):
        xx, yy = x * x, y * y
        r2 = xx + yy
        rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        dX = ((2.0 * p1) * x) * y + p2 * (r2 + 2.0 * xx)
        dY = p1 * (r2 + 2.0 * yy) + ((2.0 * p2) * x) * y
        return x * rad + dX, y * rad + dY, rad


def np_source(K, lens, R, K_new, u, v):
    """S80 in fp64 on arrays of ideal pixels: (ok, sx, sy)."""
    fx, fy, cx, cy = [float(c) for c in K]
    nfx, nfy, ncx, ncy = [float(c) for c in (K if K_new is None else K_new)]
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        x, y = (u - ncx) * (1.0 / nfx), (v - ncy) * (1.0 / nfy)
        ok = np.ones(x.shape, bool)
        if R is not None:
            r = np.asarray(R, np.float64).reshape(9)
            X = (r[0] * x + r[3] * y) + r[6]
            Y = (r[1] * x + r[4] * y) + r[7]
            Z = (r[2] * x + r[5] * y) + r[8]
            ok = Z > 0.0
            iz = 1.0 / Z
            x, y = X * iz, Y * iz
        xd, yd, rad = np_forward_norm(lens, x, y)
        sx, sy = fx * xd + cx, fy * yd + cy
        ok = ok & (rad > 0.0) & np.isfinite(sx) & np.isfinite(sy)
    return ok, sx, sy


def _nan_pairs(ok, a, b):
    with np.errstate(all="ignore"):
        out = np.stack([a, b], -1).astype(np.float32)
    out[~ok] = np.nan
    return out


def np_distort_points(K, lens, R, K_new, pts):
    pts = _pts(pts)
    return _nan_pairs(*np_source(K, lens, R, K_new, pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)))


def np_undistort_points(K, lens, R, K_new, pts, iters=None, tol_px=None):
    iters, tol_px = ITERS if iters is None else iters, TOL_PX if tol_px is None else tol_px
    pts = _pts(pts)
    fx, fy, cx, cy = [float(c) for c in K]
    nfx, nfy, ncx, ncy = [float(c) for c in (K if K_new is None else K_new)]
    k1, k2, p1, p2, k3 = (0.0,) * 5 if lens is None else [float(c) for c in lens]
    with np.errstate(all="ignore"):
        x0, y0 = (pts[:, 0].astype(np.float64) - cx) * (1.0 / fx), (pts[:, 1].astype(np.float64) - cy) * (1.0 / fy)
        x, y = x0, y0
        for _ in range(iters):
            xx, yy = x * x, y * y
            r2 = xx + yy
            ic = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dX = ((2.0 * p1) * x) * y + p2 * (r2 + 2.0 * xx)
            dY = p1 * (r2 + 2.0 * yy) + ((2.0 * p2) * x) * y
            x, y = (x0 - dX) * ic, (y0 - dY) * ic
        xd, yd, rad = np_forward_norm(lens, x, y)
        ex, ey = fx * (xd - x0), fy * (yd - y0)
        ok = (rad > 0.0) & (ex * ex + ey * ey <= tol_px * tol_px)
        if R is not None:
            r = np.asarray(R, np.float64).reshape(9)
            X = (r[0] * x + r[1] * y) + r[2]
            Y = (r[3] * x + r[4] * y) + r[5]
            Z = (r[6] * x + r[7] * y) + r[8]
            ok = ok & (Z > 0.0)
            iz = 1.0 / Z
            x, y = X * iz, Y * iz
        u, v = nfx * x + ncx, nfy * y + ncy
        ok = ok & np.isfinite(u) & np.isfinite(v)
    return _nan_pairs(ok, u, v)


def np_map(K, lens, R, K_new, dw, dh):
    """S82 / S83 in numpy: (dh, dw, 2) int32."""
    ys, xs = np.mgrid[0:dh, 0:dw].astype(np.float64)
    ok, sx, sy = np_source(K, lens, R, K_new, xs, ys)
    with np.errstate(all="ignore"):
        fx, fy = sx * 32.0, sy * 32.0
        ok = ok & (np.abs(fx) < 2.0 ** 30) & (np.abs(fy) < 2.0 ** 30)
    m = np.full((dh, dw, 2), INT32_MIN, np.int64)
    m[..., 0][ok] = np.rint(fx[ok]).astype(np.int64)
    m[..., 1][ok] = np.rint(fy[ok]).astype(np.int64)
    return m.astype(np.int32)


def np_remap(src, m, flags=0, border=0):
    """S83 / S77 in numpy: (dst (dh, dw) u8, valid (dh, dw) u8, n_valid)."""
    src = np.ascontiguousarray(src, np.uint8)
    sh, sw = src.shape
    m = np.asarray(m).astype(np.int64)
    qx, qy = m[..., 0], m[..., 1]
    use = ~((qx == INT32_MIN) & (qy == INT32_MIN))
    x0, y0, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
    I = src.astype(np.int64)
    total = np.zeros(qx.shape, np.int64)
    valid = use.copy()
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
    out = np.where(use, (total + 512) >> 10, border)
    return out.astype(np.uint8), valid.astype(np.uint8), int(valid.sum())


def np_undistort(src, K, lens, R=None, K_new=None, flags=0, border=0, dw=None, dh=None):
    src = np.ascontiguousarray(src, np.uint8)
    dw = src.shape[1] if dw is None else dw
    dh = src.shape[0] if dh is None else dh
    return np_remap(src, np_map(K, lens, R, K_new, dw, dh), flags, border)


def same_floats(a, b):
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and (a[~nan].view(np.uint32) == b[~nan].view(np.uint32)).all()


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------

SW, SH = 67, 35
CAM = (60.0, 60.0, 33.0, 17.0)                               # the camera of the 67 x 35 source
LENS = (-0.28, 0.07, 1e-3, -5e-4, 0.0)                       # moves the corners of that frame by more than two pixels
CAM_NEW = (48.0, 52.0, 40.5, 22.25)                          # another focal length and principal point
MODERATE = (-0.28, 0.07, 1e-3, -5e-4, 0.0)
ITERS, TOL_PX = 20, 1e-3                                     # rejects no point of the grids the tests use under MODERATE


def rotation(rx, ry, rz):
    """Rz(rz) Ry(ry) Rx(rx), degrees."""
    a, b, c = np.radians([rx, ry, rz])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


ROT = rotation(3.0, -2.0, 4.0)                               # a few degrees about each axis


def random_source(w=SW, h=SH, seed=0):
    return np.random.default_rng(7900 + 1000 * w + h + seed).integers(0, 256, (h, w), dtype=np.uint8)


def extreme_map():
    """A hand-made 3 x 6 map: the corners of int32 and the negative positions around a pixel edge, against ordinary rows."""
    big = 2 ** 31 - 1
    qx = [big, big - 31, -1, -32, -33, 40]
    m = np.zeros((3, 6, 2), np.int32)
    for r, qy in enumerate((64, big, -33)):
        m[r, :, 0] = qx
        m[r, :, 1] = qy
    m[2, 5] = (INT32_MIN, INT32_MIN)                          # the unusable pair
    m[1, 5] = (INT32_MIN, 64)                                 # not the pair: sampled, far outside
    m[0, 5] = (64, INT32_MIN)
    return m


def seeded_points(n, seed=0):
    """Pixels over and a little around the 67 x 35 frame; from 63 rows on, three non-finite rows and one far outside the field."""
    rng = np.random.default_rng(8100 + n + seed)
    pts = np.stack([rng.uniform(-3, SW + 3, n), rng.uniform(-3, SH + 3, n)], 1).astype(np.float32)
    if n >= 63:
        pts[7] = (np.nan, 3.0)
        pts[20] = (np.inf, -np.inf)
        pts[33] = (5.0, np.nan)
        pts[41] = (5000.0, -4000.0)
    return pts
