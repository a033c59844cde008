"""ctypes loader of tests/homography_refine_ref.c, the plain-C restatement of docs/SPEC.md S23-S25 (refinement of the
robust homography on its inliers).  Built on first use by cref.py; shared by test_homography_refine_cpu.py and
test_homography_refine_gpu.py."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p

_lib = None


class Info(C.Structure):
    """pm_h_refine_info (include/pm.h)."""
    _fields_ = [("cost_in", C.c_double), ("cost_out", C.c_double), ("n_used", C.c_int32), ("iters", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32)]

    def as_tuple(self):
        return (self.cost_in, self.cost_out, self.n_used, self.iters, self.status)


def lib():
    global _lib
    if _lib is None:
        _lib = cref.load("homography_refine_ref", {
            "hrr_refine": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p],
            "hrr_refit": [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2,
            "hrr_cost": [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2,
        }, {"hrr_cost": C.c_double})
    return _lib


def _args(xy1, xy2, mask):
    xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
    mask = np.ascontiguousarray(mask, np.uint8).reshape(-1)
    assert mask.shape[0] == xy1.shape[0] == xy2.shape[0]
    return xy1, xy2, mask


def refine(xy1, xy2, mask, H_in, max_iters=10):
    """S23-S25: (H_out 3x3, Info)."""
    xy1, xy2, mask = _args(xy1, xy2, mask)
    Hin = np.ascontiguousarray(H_in, np.float64).reshape(9)
    H = np.zeros(9, np.float64)
    info = Info()
    lib().hrr_refine(_p(xy1), _p(xy2), xy1.shape[0], _p(mask), _p(Hin), max_iters, _p(H), C.byref(info))
    return H.reshape(3, 3), info


def refit(xy1, xy2, mask):
    """S23 alone: (valid, H 3x3)."""
    xy1, xy2, mask = _args(xy1, xy2, mask)
    H = np.zeros(9, np.float64)
    ok = lib().hrr_refit(_p(xy1), _p(xy2), xy1.shape[0], _p(mask), _p(H))
    return bool(ok), H.reshape(3, 3)


def cost(xy1, xy2, mask, H):
    """S24's cost (sum of squared forward transfer errors over the inliers) of a 9-vector, in the S23 order."""
    xy1, xy2, mask = _args(xy1, xy2, mask)
    h = np.ascontiguousarray(H, np.float64).reshape(9)
    return lib().hrr_cost(_p(xy1), _p(xy2), xy1.shape[0], _p(mask), _p(h))
