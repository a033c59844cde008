"""ctypes loader of tests/affine_ref.c, the plain-C restatement of docs/SPEC.md S26-S30 (robust 2D affine and
similarity estimation, least-squares refit on the inliers).  Built on first use by cref.py; shared by
test_affine_cpu.py and test_affine_gpu.py.  model: 0 = full, 1 = partial."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = cref.load("affine_ref", {
            "ar_run": [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int64, C.c_int64, C.c_float,
                       C.c_void_p, C.c_void_p, C.c_void_p],
            "ar_sample": [C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p],
            "ar_solve": [C.c_int] + [C.c_void_p] * 5,
            "ar_model": [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p],
            "ar_inlier": [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float],
            "ar_score": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p],
            "ar_refine": [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_void_p],
        }, {"ar_run": C.c_uint64})
    return _lib


def _f32(xy):
    return np.ascontiguousarray(xy, np.float32).reshape(-1, 2)


def min_pts(model):
    return 3 if model == 0 else 2


def sample(model, seed, h, n):
    idx = np.zeros(3, np.int32)
    lib().ar_sample(model, seed, h, n, _p(idx))
    return idx[:min_pts(model)]


def solve(model, p1, p2):
    """p1, p2: MIN_PTS x 2 float64.  Returns (valid, A 2x3)."""
    p1 = np.asarray(p1, np.float64)
    p2 = np.asarray(p2, np.float64)
    cols = [np.ascontiguousarray(c) for c in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1])]
    A = np.zeros(6, np.float64)
    ok = lib().ar_solve(model, *[_p(c) for c in cols], _p(A))
    return bool(ok), A.reshape(2, 3)


def model_of(model, xy1, xy2, seed, h):
    xy1, xy2 = _f32(xy1), _f32(xy2)
    A = np.zeros(6, np.float64)
    ok = lib().ar_model(model, _p(xy1), _p(xy2), xy1.shape[0], seed, h, _p(A))
    return bool(ok), A.reshape(2, 3)


def inlier(a32, x, y, xp, yp, thr2):
    a = np.ascontiguousarray(a32, np.float32).reshape(6)
    return bool(lib().ar_inlier(_p(a), x, y, xp, yp, thr2))


def score(A, xy1, xy2, thresh_px):
    xy1, xy2 = _f32(xy1), _f32(xy2)
    n = xy1.shape[0]
    A = np.ascontiguousarray(A, np.float64).reshape(6)
    mask = np.zeros(max(n, 1), np.uint8)
    c = lib().ar_score(_p(A), _p(xy1), _p(xy2), n, thresh_px, _p(mask))
    return mask[:n], c


def run(model, xy1, xy2, iters, thresh_px, seed, hyp_begin=0):
    """Whole run over ids [hyp_begin, iters): (key, A 2x3, mask, n_inliers)."""
    xy1, xy2 = _f32(xy1), _f32(xy2)
    n = xy1.shape[0]
    A = np.zeros(6, np.float64)
    mask = np.zeros(max(n, 1), np.uint8)
    ninl = C.c_int()
    key = lib().ar_run(model, _p(xy1), _p(xy2), n, seed, hyp_begin, iters, thresh_px, _p(A), _p(mask), C.byref(ninl))
    return key, A.reshape(2, 3), mask[:n], ninl.value


def refine(model, xy1, xy2, mask, A_in):
    """S30: (status, A_out 2x3, cost_in, cost_out, n_used)."""
    xy1, xy2 = _f32(xy1), _f32(xy2)
    mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
    Ain = np.ascontiguousarray(A_in, np.float64).reshape(6)
    A = np.zeros(6, np.float64)
    costs = np.zeros(2, np.float64)
    ints = np.zeros(2, np.int32)
    st = lib().ar_refine(model, _p(xy1), _p(xy2), xy1.shape[0], _p(mask), _p(Ain), _p(A), _p(costs), _p(ints))
    return st, A.reshape(2, 3), costs[0], costs[1], int(ints[0])
