"""ctypes loader of tests/lk_ref.c, the plain-C restatement of SPEC S61-S66 (pyramidal Lucas-Kanade tracking), and the
test frames both tracking test files use.  Built once per process through tests/cref.py."""
import ctypes as C
import os

import numpy as np

import cref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
USE_INITIAL = 1


class Params(C.Structure):
    """lk_params, the layout of pm_lk_params."""
    _fields_ = [("win_radius", C.c_int32), ("max_level", C.c_int32), ("max_iters", C.c_int32), ("eps", C.c_float),
                ("min_eig", C.c_float), ("fb_thresh", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


def params(r=10, max_level=3, max_iters=30, eps=0.01, min_eig=1e-4, fb_thresh=0.0, flags=0):
    return Params(r, max_level, max_iters, eps, min_eig, fb_thresh, flags, 0)


_L = None
_V, _I = C.c_void_p, C.c_int


def lib():
    global _L
    if _L is None:
        _L = cref.load("lk_ref", {
            "lk_pyr_plan": [_I, _I, _I, _V, _V, _V],
            "lk_pyr_down": [_V, _I, _I, _V],
            "lk_pyr_build": [_V, _I, _I, _I, _I, _V, _V, _V, _V],
            "lk_window_origin": [C.c_float, C.c_float, _I, _I, _I, _V, _V, _V],
            "lk_sample_window": [_V, _I, _I, C.c_float, C.c_float, _I, _V],
            "lk_template": [_V, _I, _I, C.c_float, C.c_float, _I, C.c_float, _V, _V, _V, _V],
            "lk_track_point": [_V, _V, _V, _V, _V, _I, C.c_float, C.c_float, _I, C.c_float, C.c_float, _V, _V, _V],
            "lk_fb_check": [C.c_float, C.c_float, C.c_float, C.c_float, _I, C.c_float, _V],
            "lk_track": [_V, _V, _V, _V, _V, _I, _V, _I, _V, _V, _V, _V, _V, _V],
            "lk_gather": [_V, _V, _V, _I, _V, _V, _V],
        })
    return _L


class Pyramid:
    """The levels of one image: .levels (list of (h, w) u8 arrays, views of .buf), .lw, .lh, .off, .n."""

    def __init__(self, img, max_level):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        self.lw, self.lh, self.off = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, np.int64)
        n = lib().lk_pyr_plan(w, h, max_level, cref.ptr(self.lw), cref.ptr(self.lh), cref.ptr(self.off))
        total = int(self.off[n - 1] + int(self.lw[n - 1]) * int(self.lh[n - 1]))
        self.buf = np.zeros(total, np.uint8)
        assert lib().lk_pyr_build(cref.ptr(img), w, h, w, max_level, cref.ptr(self.buf), cref.ptr(self.lw), cref.ptr(self.lh),
                                  cref.ptr(self.off)) == n
        self.n = n
        self.levels = [self.buf[int(self.off[l]):int(self.off[l]) + int(self.lw[l]) * int(self.lh[l])].reshape(int(self.lh[l]), int(self.lw[l]))
                       for l in range(n)]


def pyr_down(img):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
    lib().lk_pyr_down(cref.ptr(img), w, h, cref.ptr(out))
    return out


def window_origin(px, py, n, w, h):
    """(inside, ix, iy, weights[4])."""
    ix, iy, wt = C.c_int32(-1), C.c_int32(-1), np.zeros(4, np.int32)
    ok = lib().lk_window_origin(px, py, n, w, h, C.addressof(ix), C.addressof(iy), cref.ptr(wt))
    return ok, ix.value, iy.value, wt


def sample_window(img, px, py, n):
    """(n, n) int16 samples, or None when the window leaves the level."""
    img = np.ascontiguousarray(img, np.uint8)
    out = np.zeros((n, n), np.int16)
    ok = lib().lk_sample_window(cref.ptr(img), img.shape[1], img.shape[0], px, py, n, cref.ptr(out))
    return out if ok else None


def template(img, px, py, r, min_eig):
    """(code, T (n+2, n+2), gx, gy (n, n), G = [Gxx, Gxy, Gyy, D, e]); code 0 usable, 1 left the level, 2 flat."""
    img = np.ascontiguousarray(img, np.uint8)
    n = 2 * r + 1
    T, gx, gy, G = np.zeros((n + 2, n + 2), np.int16), np.zeros((n, n), np.int16), np.zeros((n, n), np.int16), np.zeros(5)
    code = lib().lk_template(cref.ptr(img), img.shape[1], img.shape[0], px, py, r, min_eig, cref.ptr(T), cref.ptr(gx), cref.ptr(gy),
                             cref.ptr(G))
    return code, T, gx, gy, G


def track_point(pa, pb, pt, prm, init=None):
    """One point, one direction, no forward-backward rule: (status, out[2], err)."""
    out, err = np.zeros(2, np.float32), C.c_float()
    st = lib().lk_track_point(cref.ptr(pa.buf), cref.ptr(pb.buf), cref.ptr(pa.lw), cref.ptr(pa.lh), cref.ptr(pa.off), pa.n, float(pt[0]),
                              float(pt[1]), 0 if init is None else 1, 0.0 if init is None else float(init[0]),
                              0.0 if init is None else float(init[1]), C.byref(prm), cref.ptr(out), C.addressof(err))
    return st, out, err.value


def fb_check(pt, back, back_status, thresh):
    fb = C.c_float()
    st = lib().lk_fb_check(float(pt[0]), float(pt[1]), float(back[0]), float(back[1]), back_status, thresh, C.addressof(fb))
    return st, fb.value


def track(pa, pb, pts, prm, init=None):
    """The whole call: (out (n, 2) f32, status (n,) u8, err (n,) f32, fb (n,) f32)."""
    assert pa.n == pb.n and (pa.lw == pb.lw).all() and (pa.lh == pb.lh).all()
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = pts.shape[0]
    if init is not None:
        init = np.ascontiguousarray(init, np.float32).reshape(-1, 2)
    out, status = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
    err, fb = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lib().lk_track(cref.ptr(pa.buf), cref.ptr(pb.buf), cref.ptr(pa.lw), cref.ptr(pa.lh), cref.ptr(pa.off), pa.n, cref.ptr(pts), n,
                   None if init is None else cref.ptr(init), C.byref(prm), cref.ptr(out), cref.ptr(status), cref.ptr(err), cref.ptr(fb))
    return out, status, err, fb


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------

def read_pgm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P5"
        line = f.readline()
        while line.startswith(b"#"):
            line = f.readline()
        w, h = (int(v) for v in line.split())
        assert int(f.readline()) == 255
        return np.frombuffer(f.read(w * h), np.uint8).reshape(h, w).copy()


def fixture():
    """(first frame (330, 496) u8, the 240 keypoints (240, 2) f32)."""
    img = read_pgm(os.path.join(GOLD, "img01_half.pgm"))
    kp = np.load(os.path.join(GOLD, "img01_img02_half_features.npz"))["img01_kp"].astype(np.float32)
    return img, kp


def second_image():
    return read_pgm(os.path.join(GOLD, "img02_half.pgm"))


SHIFT = (3, -2)


def frame_s(img):
    """Frame S: the first frame moved by (+3, -2), zero-filled: S(x + 3, y - 2) = I(x, y)."""
    out = np.zeros_like(img)
    out[:-2, 3:] = img[2:, :-3]
    return out


ROT_DEG, ROT_T = 1.0, (7.25, -5.5)


def frame_r_map(xy, shape):
    """The true map of frame R, fp64: rotation by 1 degree about the image centre, then a shift of (7.25, -5.5)."""
    h, w = shape
    c = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    t = np.deg2rad(ROT_DEG)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    return (np.asarray(xy, np.float64) - c) @ R.T + c + np.array(ROT_T)


def frame_r(img):
    """Frame R: R(map(x)) = I(x), by fp64 bilinear resampling of I at the inverse map, the
    source coordinates clamped to the frame; rounded to u8."""
    h, w = img.shape
    c = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    t = np.deg2rad(ROT_DEG)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    q = np.stack([xs.ravel(), ys.ravel()], 1) - c - np.array(ROT_T)
    src = q @ R + c                                  # inverse rotation: R^T applied to row vectors
    sx, sy = src[:, 0], src[:, 1]
    sx, sy = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)          # outside the frame: the nearest border pixel
    x0, y0 = np.minimum(np.floor(sx).astype(np.int64), w - 2), np.minimum(np.floor(sy).astype(np.int64), h - 2)
    a, b = sx - x0, sy - y0
    I = img.astype(np.float64)
    v = (I[y0, x0] * (1 - a) * (1 - b) + I[y0, x0 + 1] * a * (1 - b) + I[y0 + 1, x0] * (1 - a) * b + I[y0 + 1, x0 + 1] * a * b)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8).reshape(h, w)


def fit_similarity(xy1, xy2):
    """Least-squares 4-DOF similarity xy2 ~ [a -b; b a] xy1 + t, fp64: returns the 2 x 3 matrix."""
    xy1, xy2 = np.asarray(xy1, np.float64), np.asarray(xy2, np.float64)
    n = xy1.shape[0]
    M = np.zeros((2 * n, 4))
    M[0::2] = np.stack([xy1[:, 0], -xy1[:, 1], np.ones(n), np.zeros(n)], 1)
    M[1::2] = np.stack([xy1[:, 1], xy1[:, 0], np.zeros(n), np.ones(n)], 1)
    a, b, tx, ty = np.linalg.lstsq(M, xy2.reshape(-1), rcond=None)[0]
    return np.array([[a, -b, tx], [b, a, ty]])


def corners(shape):
    h, w = shape
    return np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float64)
