"""ctypes loader of tests/guided_ref.c, the plain-C restatement of docs/SPEC.md S48-S50 (guided matching).  Built on first
use by cref.py; shared by test_guided_cpu.py and test_guided_gpu.py."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p

MATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
F_SAMPSON, F_SYM, H = 0, 1, 2
DESC_F32, DESC_U8, DESC_BINARY = 0, 1, 2

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = cref.load("guided_ref", {
            "gr_gate": [C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float],
            "gr_knn": [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                       C.c_float, C.c_int, C.c_void_p, C.c_void_p],
            "gr_match_guided": [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
        })
    return _lib


def _desc(desc, q, t):
    dtype = np.float32 if desc == DESC_F32 else np.uint8
    q = np.ascontiguousarray(q, dtype)
    t = np.ascontiguousarray(t, dtype).reshape(-1, q.shape[1])
    return q, t


def _kp(kp):
    return np.ascontiguousarray(kp, np.float32).reshape(-1, 2)


def _model(M):
    return np.ascontiguousarray(M, np.float64).reshape(9)


def gate_pairs(kind, M, tau, xy1, xy2):
    """gate(i, i) for every row of two equally long keypoint arrays (uint8 mask)."""
    xy1, xy2, M = _kp(xy1), _kp(xy2), _model(M)
    return np.array([lib().gr_gate(kind, _p(M), tau, *[float(v) for v in (a[0], a[1], b[0], b[1])])
                     for a, b in zip(xy1, xy2)], np.uint8)


def knn(desc, q, t, kp1, kp2, kind, M, tau, k):
    """S49: (records nq x k, n_admitted)."""
    q, t = _desc(desc, q, t)
    kp1, kp2, M = _kp(kp1), _kp(kp2), _model(M)
    assert kp1.shape[0] == q.shape[0] and kp2.shape[0] == t.shape[0]
    out = np.zeros((q.shape[0], k), MATCH_DTYPE)
    adm = np.zeros(max(q.shape[0], 1), np.int32)
    rc = lib().gr_knn(desc, _p(q), q.shape[0], _p(t), t.shape[0], q.shape[1], _p(kp1), _p(kp2), kind, _p(M), tau, k, _p(out),
                      _p(adm))
    assert rc == 0
    return out, adm[:q.shape[0]]


def match_guided(desc, q, t, kp1, kp2, kind, M, tau, ratio):
    """S50: (2-NN records nq x 2, survivors, xy1, xy2)."""
    q, t = _desc(desc, q, t)
    kp1, kp2, M = _kp(kp1), _kp(kp2), _model(M)
    nq = q.shape[0]
    rec = np.zeros((nq, 2), MATCH_DTYPE)
    good = np.zeros(max(nq, 1), MATCH_DTYPE)
    xy1 = np.zeros((max(nq, 1), 2), np.float32)
    xy2 = np.zeros((max(nq, 1), 2), np.float32)
    n = lib().gr_match_guided(desc, _p(q), nq, _p(t), t.shape[0], q.shape[1], _p(kp1), _p(kp2), kind, _p(M), tau, ratio,
                              _p(rec), _p(good), _p(xy1), _p(xy2))
    assert n >= 0
    return rec, good[:n].copy(), xy1[:n].copy(), xy2[:n].copy()
