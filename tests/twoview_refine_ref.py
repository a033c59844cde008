"""ctypes loader of tests/twoview_refine_ref.c, the plain-C restatement of docs/SPEC.md S43-S47 (refinement of the
fundamental matrix and of the calibrated relative pose on their inliers).  Built on first use by cref.py; shared by
test_twoview_refine_cpu.py and test_twoview_refine_gpu.py.  K is (fx, fy, cx, cy); a pose is R (3 x 3) and t (3)."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p


class Info(C.Structure):
    _fields_ = [("cost_in", C.c_double), ("cost_out", C.c_double), ("n_used", C.c_int32), ("iters", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32)]

    def as_tuple(self):
        return (self.cost_in, self.cost_out, self.n_used, self.iters, self.status)


_lib = None
_SIGS = {
    "tv_f_refine": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "tv_f_refit": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "tv_f_cost": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
    "tv_pose_refine": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                       C.c_void_p],
    "tv_pose_cost": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
}
_RES = {"tv_f_cost": C.c_double, "tv_pose_cost": C.c_double}


def lib():
    global _lib
    if _lib is None:
        _lib = cref.load("twoview_refine_ref", _SIGS, _RES)
    return _lib


def _args(xy1, xy2, mask):
    xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
    n = xy1.shape[0]
    m = np.ascontiguousarray(mask, np.uint8).reshape(-1)
    assert m.shape[0] >= n
    return xy1, xy2, n, (m if m.shape[0] else np.zeros(1, np.uint8))


def _k(K):
    return np.ascontiguousarray(K, np.float64).reshape(4)


def f_refine(xy1, xy2, mask, F_in, max_iters=10, L=None):
    """S43-S45: (F 3 x 3, Info)."""
    xy1, xy2, n, m = _args(xy1, xy2, mask)
    F = np.zeros(9)
    info = Info()
    (L or lib()).tv_f_refine(_p(xy1), _p(xy2), n, _p(m), _p(np.ascontiguousarray(F_in, np.float64).reshape(9)), max_iters,
                             _p(F), C.addressof(info))
    return F.reshape(3, 3), info


def f_refit(xy1, xy2, mask):
    """S44 alone: (ok, F 3 x 3)."""
    xy1, xy2, n, m = _args(xy1, xy2, mask)
    F = np.zeros(9)
    ok = lib().tv_f_refit(_p(xy1), _p(xy2), n, _p(m), _p(F))
    return bool(ok), F.reshape(3, 3)


def f_cost(xy1, xy2, mask, F):
    xy1, xy2, n, m = _args(xy1, xy2, mask)
    return lib().tv_f_cost(_p(xy1), _p(xy2), n, _p(m), _p(np.ascontiguousarray(F, np.float64).reshape(9)))


def _rt(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def pose_refine(xy1, xy2, K, mask, R_in, t_in, max_iters=10, L=None):
    """S46-S47: (R 3 x 3, t, E 3 x 3, Info)."""
    xy1, xy2, n, m = _args(xy1, xy2, mask)
    out, E = np.zeros(12), np.zeros(9)
    info = Info()
    (L or lib()).tv_pose_refine(_p(xy1), _p(xy2), n, _p(_k(K)), _p(m), _p(_rt(R_in, t_in)), max_iters, _p(out), _p(E),
                                C.addressof(info))
    return out[:9].reshape(3, 3).copy(), out[9:].copy(), E.reshape(3, 3), info


def pose_cost(xy1, xy2, K, mask, R, t):
    xy1, xy2, n, m = _args(xy1, xy2, mask)
    return lib().tv_pose_cost(_p(xy1), _p(xy2), n, _p(_k(K)), _p(m), _p(_rt(R, t)))
