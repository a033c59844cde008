"""ctypes loader of tests/pnp_ref.c, the plain-C restatement of docs/SPEC.md S36-S39 (camera check, 3-sample, P3P solve,
reprojection test, RANSAC-PnP, LM refinement).  Built on first use by cref.py; shared by test_pnp_cpu.py and test_pnp_gpu.py.  K is
(fx, fy, cx, cy); a pose is 12 doubles, R row-major then t, with x_cam = R X + t."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = cref.load("pnp_ref", {
            "pr_k_valid": [C.c_void_p, C.c_float],
            "pr_sample": [C.c_uint64, C.c_uint64, C.c_int, C.c_void_p],
            "pr_roots": [C.c_void_p, C.c_void_p],
            "pr_p3p": [C.c_void_p] * 6,
            "pr_proj32": [C.c_void_p] * 3,
            "pr_score": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p],
            "pr_candidates": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p],
            "pr_run": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int64, C.c_int64, C.c_float, C.c_void_p,
                       C.c_void_p, C.c_void_p],
            "pr_refine": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                          C.c_void_p],
        }, {"pr_run": C.c_uint64})
    return _lib


def _k(K):
    return np.ascontiguousarray(K, np.float64).reshape(4)


def _xyz(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _uv(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 2)


def k_valid(K, thresh_px):
    return bool(lib().pr_k_valid(_p(_k(K)), thresh_px))


def sample(seed, h, n):
    idx = np.zeros(3, np.int32)
    lib().pr_sample(seed, h, n, _p(idx))
    return idx


def roots(p):
    """S33 step 6 at degree 4 on the ascending coefficients p."""
    p = np.ascontiguousarray(p, np.float64)
    r = np.zeros(4)
    m = lib().pr_roots(_p(p), _p(r))
    return r[:m]


def p3p(K, X, uv):
    """S38 on 3 points: (Rt 4 x 12, valid 4 bool, quartic coefficients ascending)."""
    out = np.zeros(48)
    v = np.zeros(4, np.int32)
    coef = np.zeros(5)
    lib().pr_p3p(_p(_k(K)), _p(_xyz(X)), _p(_uv(uv)), _p(out), _p(v), _p(coef))
    return out.reshape(4, 12), v.astype(bool), coef


def proj32(K, Rt):
    P = np.zeros(12, np.float32)
    lib().pr_proj32(_p(_k(K)), _p(np.ascontiguousarray(Rt, np.float64).reshape(12)), _p(P))
    return P.reshape(3, 4)


def score(K, Rt, xyz, uv, thresh_px):
    xyz, uv = _xyz(xyz), _uv(uv)
    n = xyz.shape[0]
    mask = np.zeros(max(n, 1), np.uint8)
    thr2 = np.float32(thresh_px) * np.float32(thresh_px)
    c = lib().pr_score(_p(_k(K)), _p(np.ascontiguousarray(Rt, np.float64).reshape(12)), _p(xyz), _p(uv), n, thr2, _p(mask))
    return mask[:n], c


def candidates(xyz, uv, K, seed, h):
    """S37 + S38 of sample h: (Rt 4 x 12, valid 4 bool)."""
    xyz, uv = _xyz(xyz), _uv(uv)
    out = np.zeros(48)
    v = np.zeros(4, np.int32)
    lib().pr_candidates(_p(_k(K)), _p(xyz), _p(uv), xyz.shape[0], seed, h, _p(out), _p(v))
    return out.reshape(4, 12), v.astype(bool)


def run(xyz, uv, K, iters, thresh_px, seed, hyp_begin=0):
    """Whole RANSAC-PnP over samples [hyp_begin, iters): (key, Rt 12, mask, n_inliers)."""
    xyz, uv = _xyz(xyz), _uv(uv)
    n = xyz.shape[0]
    Rt = np.zeros(12)
    mask = np.zeros(max(n, 1), np.uint8)
    c = np.zeros(1, np.int32)
    key = lib().pr_run(_p(_k(K)), _p(xyz), _p(uv), n, seed, hyp_begin, iters, thresh_px, _p(Rt), _p(mask), _p(c))
    return int(key), Rt, mask[:n], int(c[0])


class Info:
    """S40's info, as pm_h_refine_info."""

    def __init__(self, costs, ints):
        self.cost_in, self.cost_out = float(costs[0]), float(costs[1])
        self.n_used, self.iters, self.status = int(ints[0]), int(ints[1]), int(ints[2])


def refine(xyz, uv, K, mask, Rt_in, max_iters=20):
    """S40: (Rt 12, Info)."""
    xyz, uv = _xyz(xyz), _uv(uv)
    n = xyz.shape[0]
    m = np.ascontiguousarray(mask, np.uint8).reshape(-1)
    out = np.zeros(12)
    costs = np.zeros(2)
    ints = np.zeros(3, np.int32)
    lib().pr_refine(_p(_k(K)), _p(xyz), _p(uv), n, _p(m if n else np.zeros(1, np.uint8)),
                    _p(np.ascontiguousarray(Rt_in, np.float64).reshape(12)), max_iters, _p(out), _p(costs), _p(ints))
    return out, Info(costs, ints)
