"""ctypes loader of tests/homography_refine_ref.c, the plain-C restatement of docs/SPEC.md S23-S25 (refinement of the
robust homography on its inliers).  Built on first use with the host C compiler into a temporary directory, as
homography_ref.py builds its library; shared by test_homography_refine_cpu.py and test_homography_refine_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "homography_refine_ref.c")
_lib = None
_tmp = None


class Info(C.Structure):
    """pm_h_refine_info (include/pm.h)."""
    _fields_ = [("cost_in", C.c_double), ("cost_out", C.c_double), ("n_used", C.c_int32), ("iters", C.c_int32),
                ("status", C.c_int32), ("reserved", C.c_int32)]

    def as_tuple(self):
        return (self.cost_in, self.cost_out, self.n_used, self.iters, self.status)


def lib():
    global _lib, _tmp
    if _lib is None:
        cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
        assert cc, "no host C compiler"
        _tmp = tempfile.TemporaryDirectory(prefix="homography_refine_ref_")
        so = os.path.join(_tmp.name, "libhomography_refine_ref.so")
        r = subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        L = C.CDLL(so)
        L.hrr_refine.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_void_p]
        L.hrr_refit.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2
        L.hrr_cost.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2
        L.hrr_cost.restype = C.c_double
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


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
