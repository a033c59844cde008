"""ctypes loader of tests/homography_ref.c, the plain-C restatement of docs/SPEC.md S19-S22 (robust homography).
Built on first use with the host C compiler into a temporary directory; shared by test_homography_cpu.py and
test_homography_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "homography_ref.c")
_lib = None
_tmp = None


def lib():
    global _lib, _tmp
    if _lib is None:
        cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
        assert cc, "no host C compiler"
        _tmp = tempfile.TemporaryDirectory(prefix="homography_ref_")
        so = os.path.join(_tmp.name, "libhomography_ref.so")
        r = subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        L = C.CDLL(so)
        L.hr_run.restype = C.c_uint64
        L.hr_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int64, C.c_int64, C.c_float, C.c_void_p,
                             C.c_void_p, C.c_void_p]
        L.hr_sample4.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
        L.hr_solve4.argtypes = [C.c_void_p] * 5
        L.hr_model.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
        L.hr_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


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
