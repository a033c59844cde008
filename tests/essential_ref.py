"""ctypes loader of tests/essential_ref.c, the plain-C restatement of docs/SPEC.md S31-S35 (camera normalisation,
5-sample, 5-point solve, RANSAC-E, pose recovery).  Built on first use by cref.py; shared by test_essential_cpu.py and
test_essential_gpu.py.  K is (fx, fy, cx, cy)."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = cref.load("essential_ref", {
            "er_k_valid": [C.c_void_p, C.c_float, C.c_void_p],
            "er_normalise": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
            "er_sample": [C.c_uint64, C.c_uint64, C.c_int, C.c_void_p],
            "er_constraints": [C.c_void_p] * 5,
            "er_gauss_jordan": [C.c_void_p],
            "er_bz": [C.c_void_p, C.c_void_p],
            "er_detpoly": [C.c_void_p, C.c_void_p],
            "er_roots": [C.c_void_p, C.c_void_p],
            "er_solve5": [C.c_void_p] * 7,
            "er_candidates": [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p],
            "er_score": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p],
            "er_run": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_float,
                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "er_decompose": [C.c_void_p] * 4,
            "er_triangulate": [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p],
            "er_cheiral": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double],
            "er_recover_pose": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
        }, {"er_run": C.c_uint64})
    return _lib


def _f32(xy):
    return np.ascontiguousarray(xy, np.float32).reshape(-1, 2)


def _k(K):
    return np.ascontiguousarray(K, np.float64).reshape(4)


def thr_n(K, thresh_px):
    """S31: (valid, normalised threshold as f32)."""
    t = np.zeros(1, np.float32)
    ok = lib().er_k_valid(_p(_k(K)), thresh_px, _p(t))
    return bool(ok), t[0]


def normalise(K, xy):
    xy = _f32(xy)
    out = np.zeros_like(xy)
    lib().er_normalise(_p(_k(K)), _p(xy), xy.shape[0], _p(out))
    return out


def sample(seed, h, n):
    idx = np.zeros(5, np.int32)
    lib().er_sample(seed, h, n, _p(idx))
    return idx


def constraints(N):
    """N: 4 x 9 null-space basis (X, Y, Z, W).  The 10 x 20 matrix."""
    N = [np.ascontiguousarray(r, np.float64) for r in np.asarray(N)]
    A = np.zeros((10, 20), np.float64)
    lib().er_constraints(*[_p(r) for r in N], _p(A))
    return A


def gauss_jordan(A):
    A = np.array(A, np.float64, order="C")
    ok = lib().er_gauss_jordan(_p(A))
    return bool(ok), A


def detpoly(A):
    A = np.ascontiguousarray(A, np.float64)
    B = np.zeros((3, 3, 5), np.float64)
    lib().er_bz(_p(A), _p(B))
    p = np.zeros(11, np.float64)
    lib().er_detpoly(_p(B), _p(p))
    return B, p


def roots(p):
    p = np.ascontiguousarray(p, np.float64)
    r = np.zeros(10, np.float64)
    m = lib().er_roots(_p(p), _p(r))
    return r[:m]


def solve5(p1, p2):
    """p1, p2: 5 x 2 normalised (f64).  (E 10 x 3 x 3, valid 10 bool, stage)."""
    p1 = np.asarray(p1, np.float64)
    p2 = np.asarray(p2, np.float64)
    cols = [np.ascontiguousarray(c) for c in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1])]
    E = np.zeros(90, np.float64)
    v = np.zeros(10, np.int32)
    st = np.zeros(1, np.int32)
    lib().er_solve5(*[_p(c) for c in cols], _p(E), _p(v), _p(st))
    return E.reshape(10, 3, 3), v.astype(bool), int(st[0])


def candidates(xy1, xy2, K, seed, h):
    """S32 + S33 of sample h on pixel coordinates: (E 10 x 9, valid 10 bool)."""
    x1n, x2n = normalise(K, xy1), normalise(K, xy2)
    E = np.zeros(90, np.float64)
    v = np.zeros(10, np.int32)
    lib().er_candidates(_p(x1n), _p(x2n), x1n.shape[0], seed, h, _p(E), _p(v))
    return E.reshape(10, 9), v.astype(bool)


def score(E, xy1n, xy2n, thr2):
    xy1n, xy2n = _f32(xy1n), _f32(xy2n)
    n = xy1n.shape[0]
    mask = np.zeros(max(n, 1), np.uint8)
    c = lib().er_score(_p(np.ascontiguousarray(E, np.float64).reshape(9)), _p(xy1n), _p(xy2n), n, thr2, _p(mask))
    return mask[:n], c


def run(xy1, xy2, K, iters, thresh_px, seed, hyp_begin=0):
    """Whole RANSAC-E over samples [hyp_begin, iters): (key, E 3x3, mask, n_inliers)."""
    xy1, xy2 = _f32(xy1), _f32(xy2)
    n = xy1.shape[0]
    scratch = np.zeros(4 * max(n, 1), np.float32)
    E = np.zeros(9, np.float64)
    mask = np.zeros(max(n, 1), np.uint8)
    c = np.zeros(1, np.int32)
    key = lib().er_run(_p(xy1), _p(xy2), n, _p(_k(K)), seed, hyp_begin, iters, thresh_px, _p(scratch), _p(E), _p(mask),
                       _p(c))
    return int(key), E.reshape(3, 3), mask[:n], int(c[0])


def decompose(E):
    E = np.ascontiguousarray(E, np.float64).reshape(9)
    R1, R2, t = np.zeros(9), np.zeros(9), np.zeros(3)
    ok = lib().er_decompose(_p(E), _p(R1), _p(R2), _p(t))
    return bool(ok), R1.reshape(3, 3), R2.reshape(3, 3), t


def triangulate(R, t, x1, y1, x2, y2):
    Q = np.zeros(4)
    lib().er_triangulate(_p(np.ascontiguousarray(R, np.float64).reshape(9)), _p(np.ascontiguousarray(t, np.float64)),
                         x1, y1, x2, y2, _p(Q))
    return Q


def cheiral(R, t, Q, dist=50.0):
    return bool(lib().er_cheiral(_p(np.ascontiguousarray(R, np.float64).reshape(9)),
                                 _p(np.ascontiguousarray(t, np.float64)), _p(np.ascontiguousarray(Q, np.float64)), dist))


def recover_pose(xy1, xy2, K, E, mask=None, dist=50.0):
    """S35: (n_good or -1, R 3x3, t, mask_out, points n x 4 f32, good counts of the 4 candidates)."""
    xy1, xy2 = _f32(xy1), _f32(xy2)
    n = xy1.shape[0]
    R, t = np.zeros(9), np.zeros(3)
    mo = np.zeros(max(n, 1), np.uint8)
    pts = np.zeros((max(n, 1), 4), np.float32)
    g = np.zeros(4, np.int32)
    mi = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    ng = lib().er_recover_pose(_p(xy1), _p(xy2), n, _p(_k(K)), _p(np.ascontiguousarray(E, np.float64).reshape(9)),
                               None if mi is None else _p(mi), dist, _p(R), _p(t), _p(mo), _p(pts), _p(g))
    return ng, R.reshape(3, 3), t, mo[:n], pts[:n], g
