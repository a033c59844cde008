"""ctypes loader of tests/align3d_ref.c, the plain-C restatement of docs/SPEC.md S97-S101 (3-sample, triad solve, distance
test, RANSAC over rigid / similarity transforms, Horn / Umeyama refit, the point transform).  Built on first use by cref.py;
shared by test_align3d_cpu.py and test_align3d_gpu.py.  A model is 13 doubles: R row-major, t, s, with x2 = s R x1 + t."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p

RIGID, SIMILARITY = 0, 1
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = cref.load("align3d_ref", {
            "ar_sample": [C.c_uint64, C.c_uint64, C.c_int, C.c_void_p],
            "ar_solve": [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
            "ar_model32": [C.c_void_p, C.c_void_p],
            "ar_score": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p],
            "ar_candidate": [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p],
            "ar_run": [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int64, C.c_int64, C.c_float, C.c_void_p,
                       C.c_void_p, C.c_void_p],
            "ar_horn": [C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "ar_refine": [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
            "ar_transform": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
        }, {"ar_run": C.c_uint64})
    return _lib


def _xyz(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _t(T):
    return np.ascontiguousarray(T, np.float64).reshape(13)


def pack(s, R, t):
    """(s, R 3 x 3, t 3) -> the 13 doubles."""
    return np.r_[np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3), float(s)]


def unpack(T):
    """The 13 doubles -> (s, R 3 x 3, t 3)."""
    T = np.asarray(T, np.float64).reshape(13)
    return float(T[12]), T[:9].reshape(3, 3).copy(), T[9:12].copy()


def sample(seed, h, n):
    idx = np.zeros(3, np.int32)
    lib().ar_sample(seed, h, n, _p(idx))
    return idx


def solve(model, a, b):
    """S98 on 3 rows of each frame: (T 13, valid)."""
    out = np.zeros(13)
    ok = lib().ar_solve(model, _p(_xyz(a)), _p(_xyz(b)), _p(out))
    return out, bool(ok)


def model32(T):
    P = np.zeros(12, np.float32)
    lib().ar_model32(_p(_t(T)), _p(P))
    return P.reshape(3, 4)


def score(T, xyz1, xyz2, thresh):
    xyz1, xyz2 = _xyz(xyz1), _xyz(xyz2)
    n = xyz1.shape[0]
    mask = np.zeros(max(n, 1), np.uint8)
    with np.errstate(over="ignore"):
        thr2 = np.float32(thresh) * np.float32(thresh)              # fp32, as the launch computes it (may be +inf)
    c = lib().ar_score(_p(_t(T)), _p(xyz1), _p(xyz2), n, thr2, _p(mask))
    return mask[:n], c


def candidate(model, xyz1, xyz2, seed, h):
    """S97 + S98 of sample h: (T 13, valid)."""
    xyz1, xyz2 = _xyz(xyz1), _xyz(xyz2)
    out = np.zeros(13)
    ok = lib().ar_candidate(model, _p(xyz1), _p(xyz2), xyz1.shape[0], seed, h, _p(out))
    return out, bool(ok)


def run(model, xyz1, xyz2, iters, thresh, seed, hyp_begin=0):
    """Whole run over samples [hyp_begin, iters): (key, T 13, mask, n_inliers)."""
    xyz1, xyz2 = _xyz(xyz1), _xyz(xyz2)
    n = xyz1.shape[0]
    T = np.zeros(13)
    mask = np.zeros(max(n, 1), np.uint8)
    c = np.zeros(1, np.int32)
    key = lib().ar_run(model, _p(xyz1), _p(xyz2), n, seed, hyp_begin, iters, thresh, _p(T), _p(mask), _p(c))
    return int(key), T, mask[:n], int(c[0])


def horn(model, S, qa, ca, cb):
    """S101 steps 3-6 on the moments: (T 13, determined, the four Jacobi eigenvalues)."""
    T, eig = np.zeros(13), np.zeros(4)
    ok = lib().ar_horn(model, _p(np.ascontiguousarray(S, np.float64)), float(qa), _p(np.ascontiguousarray(ca, np.float64)),
                       _p(np.ascontiguousarray(cb, np.float64)), _p(T), _p(eig))
    return T, bool(ok), eig


class Info:
    """S101's info, as pm_h_refine_info."""

    def __init__(self, costs, ints):
        self.cost_in, self.cost_out = float(costs[0]), float(costs[1])
        self.n_used, self.iters, self.status = int(ints[0]), int(ints[1]), int(ints[2])


def refine(model, xyz1, xyz2, mask, T_in):
    """S101: (T 13, Info)."""
    xyz1, xyz2 = _xyz(xyz1), _xyz(xyz2)
    n = xyz1.shape[0]
    m = np.ascontiguousarray(mask, np.uint8).reshape(-1)
    out = np.zeros(13)
    costs = np.zeros(2)
    ints = np.zeros(3, np.int32)
    lib().ar_refine(model, _p(xyz1), _p(xyz2), n, _p(m if n else np.zeros(1, np.uint8)), _p(_t(T_in)), _p(out), _p(costs),
                    _p(ints))
    return out, Info(costs, ints)


def transform(T, xyz):
    xyz = _xyz(xyz)
    out = np.zeros_like(xyz)
    lib().ar_transform(_p(_t(T)), _p(xyz), xyz.shape[0], _p(out))
    return out
