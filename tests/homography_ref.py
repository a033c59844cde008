"""ctypes loader of tests/homography_ref.c, the plain-C restatement of docs/SPEC.md S19-S22 (robust homography).
Built on first use by cref.py; shared by test_homography_cpu.py and test_homography_gpu.py."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = cref.load("homography_ref", {
            "hr_run": [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int64, C.c_int64, C.c_float, C.c_void_p,
                       C.c_void_p, C.c_void_p],
            "hr_sample4": [C.c_uint64, C.c_uint64, C.c_int, C.c_void_p],
            "hr_solve4": [C.c_void_p] * 5,
            "hr_model": [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p],
            "hr_score": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p],
        }, {"hr_run": C.c_uint64})
    return _lib


def _f32(xy):
    return np.ascontiguousarray(xy, np.float32).reshape(-1, 2)


def sample4(seed, h, n):
    idx = np.zeros(4, np.int32)
    lib().hr_sample4(seed, h, n, _p(idx))
    return idx


def solve4(p1, p2):
    """p1, p2: 4 x 2 float64.  Returns (valid, H 3x3)."""
    p1 = np.asarray(p1, np.float64)
    p2 = np.asarray(p2, np.float64)
    cols = [np.ascontiguousarray(c) for c in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1])]
    H = np.zeros(9, np.float64)
    ok = lib().hr_solve4(*[_p(c) for c in cols], _p(H))
    return bool(ok), H.reshape(3, 3)


def model(xy1, xy2, seed, h):
    xy1, xy2 = _f32(xy1), _f32(xy2)
    H = np.zeros(9, np.float64)
    ok = lib().hr_model(_p(xy1), _p(xy2), xy1.shape[0], seed, h, _p(H))
    return bool(ok), H.reshape(3, 3)


def score(H, xy1, xy2, thresh_px):
    xy1, xy2 = _f32(xy1), _f32(xy2)
    n = xy1.shape[0]
    H = np.ascontiguousarray(H, np.float64).reshape(9)
    mask = np.zeros(max(n, 1), np.uint8)
    c = lib().hr_score(_p(H), _p(xy1), _p(xy2), n, thresh_px, _p(mask))
    return mask[:n], c


def run(xy1, xy2, iters, thresh_px, seed, hyp_begin=0):
    """Whole run over ids [hyp_begin, iters): (key, H 3x3, mask, n_inliers)."""
    xy1, xy2 = _f32(xy1), _f32(xy2)
    n = xy1.shape[0]
    H = np.zeros(9, np.float64)
    mask = np.zeros(max(n, 1), np.uint8)
    ninl = C.c_int()
    key = lib().hr_run(_p(xy1), _p(xy2), n, seed, hyp_begin, iters, thresh_px, _p(H), _p(mask), C.byref(ninl))
    return key, H.reshape(3, 3), mask[:n], ninl.value
