"""ctypes loader of tests/vocab_ref.c, the plain-C restatement of docs/SPEC.md S102-S106 (visual vocabularies: stride
initialisation, assignment by the matcher's rule, rounded-mean / majority update, the training loop and its records, the
bag-of-words encoding).  Built on first use by cref.py; shared by test_vocab_cpu.py, test_vocab_gpu.py, vocab_cases.py
(with test_vocab_limits_cpu.py and test_vocab_limits_gpu.py) and tools/prof_vocab.py."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p

L2_U8, BITS = 0, 1
ITER_DTYPE = np.dtype([("n_changed", "<i4"), ("n_empty", "<i4"), ("n_moved", "<i4"), ("reserved", "<i4"), ("cost", "<u8")])
_lib = None


def lib():
    global _lib
    if _lib is None:
        v = C.c_void_p
        _lib = cref.load("vocab_ref", {
            "vr_init_stride": [v, C.c_int, C.c_int, C.c_int, v],
            "vr_assign": [C.c_int, C.c_int, v, C.c_int, v, C.c_int, v, v, v],
            "vr_update": [C.c_int, C.c_int, v, C.c_int, v, C.c_int, v, v, v],
            "vr_train": [C.c_int, C.c_int, v, C.c_int, v, C.c_int, C.c_int, v, v, v],
            "vr_encode": [C.c_int, C.c_int, v, C.c_int, v, C.c_int, C.c_int, C.c_int32, v, v, v],
        }, {fn: None for fn in ("vr_init_stride", "vr_assign", "vr_update", "vr_train", "vr_encode")})
    return _lib


def _rows(a):
    a = np.ascontiguousarray(a, np.uint8)
    assert a.ndim == 2
    return a


def init_stride(rows, K):
    rows = _rows(rows)
    words = np.zeros((K, rows.shape[1]), np.uint8)
    lib().vr_init_stride(_p(rows), rows.shape[0], rows.shape[1], K, _p(words))
    return words


def assign(kind, words, rows):
    """S103: (labels int32, the matcher's float distances, the integer distances)."""
    words, rows = _rows(words), _rows(rows)
    n = rows.shape[0]
    lab, d, di = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    lib().vr_assign(kind, rows.shape[1], _p(words), words.shape[0], _p(rows), n, _p(lab), _p(d), _p(di))
    return lab, d, di


def update(kind, words, rows, labels):
    """S104 on given labels: (new words, n_empty, n_moved)."""
    words, rows = _rows(words).copy(), _rows(rows)
    labels = np.ascontiguousarray(labels, np.int32)
    ne, nm = C.c_int32(), C.c_int32()
    lib().vr_update(kind, rows.shape[1], _p(words), words.shape[0], _p(rows), rows.shape[0], _p(labels), C.byref(ne), C.byref(nm))
    return words, ne.value, nm.value


def train(kind, words, rows, iters):
    """S105: (final words, labels of the last iteration, records (ITER_DTYPE), the words after every iteration)."""
    words, rows = _rows(words).copy(), _rows(rows)
    K, n = words.shape[0], rows.shape[0]
    labels = np.full(n, -9, np.int32)
    info = np.zeros(iters, ITER_DTYPE)
    after = np.zeros((iters, K, rows.shape[1]), np.uint8)
    lib().vr_train(kind, rows.shape[1], _p(words), K, _p(rows), n, iters, _p(labels), _p(info), _p(after))
    return words, labels, info, after


def encode(kind, words, rows, count=None):
    """S106: (words int32 n, dist float32 n, hist uint32 K); count None = no device count."""
    words, rows = _rows(words), _rows(rows)
    n, K = rows.shape[0], words.shape[0]
    w, d, h = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(K, np.uint32)
    lib().vr_encode(kind, rows.shape[1], _p(words), K, _p(rows), n, int(count is not None), 0 if count is None else int(count),
                    _p(w), _p(d), _p(h))
    return w, d, h
