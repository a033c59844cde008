"""CPU: the yardstick of the wide Hamming tests and the host padding helper.

tests/test_knn_hamming_wide_gpu.py compares the matcher with oracle.bf_knn_hamming on rows zero-padded to a multiple of 4
bytes (SPEC S51).  Here that yardstick is itself checked against a numpy unpackbits popcount on the UNPADDED rows, and
pm_pad_rows_u8 (include/pm.h) against numpy."""
import ctypes as C

import numpy as np
import pytest

from points_matching_amd import api


def pad4(a):
    """Rows zero-padded to the next multiple of 4 bytes."""
    a = np.ascontiguousarray(a, np.uint8)
    w = -(-a.shape[1] // 4) * 4
    out = np.zeros((a.shape[0], w), np.uint8)
    out[:, :a.shape[1]] = a
    return out


def popcount_knn(q, t, k):
    """(distance, trainIdx) of the k nearest rows by popcount(q XOR t), ties to the lower index (SPEC S2/S3)."""
    d = np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(axis=2).astype(np.int64)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d, order, axis=1), order


@pytest.mark.parametrize("nbytes", [1, 3, 30, 61, 64])
def test_yardstick_equals_numpy_popcount(oracle, nbytes):
    rng = np.random.default_rng(100 + nbytes)
    nq, nt, k = 37, 150, 3
    t = rng.integers(0, 256, (nt, nbytes), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, nbytes), dtype=np.uint8)
    q[:10] = t[rng.integers(0, nt, 10)]
    q[:10, 0] ^= np.uint8(1)
    t[140] = t[7]                                  # a planted tie: the lower index first
    q[11] = t[7]
    q[12] = ~t[9]                                  # the complement: distance = the bit count of the real bytes
    want_d, want_i = popcount_knn(q, t, k)
    got = oracle.bf_knn_hamming(pad4(q), pad4(t), k)
    assert (got["trainIdx"] == want_i).all()
    assert (got["distance"] == want_d.astype(np.float32)).all()
    assert got["distance"][11, 0] == 0
    if nbytes >= 30:                               # (shorter rows repeat by chance: the planted pair is not alone)
        assert list(got["trainIdx"][11, :2]) == [7, 140]
    assert popcount_knn(q[12:13], t[9:10], 1)[0][0, 0] == 8 * nbytes


@pytest.mark.parametrize("n,nbytes,dst", [(5, 61, 64), (3, 1, 4), (7, 30, 32), (4, 64, 64), (6, 3, 5)])
def test_pad_rows_u8_host(n, nbytes, dst):
    rng = np.random.default_rng(n + nbytes)
    src = rng.integers(1, 256, (n, nbytes), dtype=np.uint8)
    want = np.zeros((n, dst), np.uint8)
    want[:, :nbytes] = src
    assert (api.pad_rows_u8(src, dst) == want).all()
    # any source alignment: the same rows one byte into a buffer; the destination starts out non-zero
    raw = np.zeros(n * nbytes + 1, np.uint8)
    raw[1:] = src.reshape(-1)
    out = np.full((n, dst), 0xEE, np.uint8)
    rc = api.lib().pm_pad_rows_u8(C.c_void_p(raw.ctypes.data + 1), n, nbytes, out.ctypes.data_as(C.c_void_p), dst)
    assert rc == api.PM_OK and (out == want).all()


def test_pad_rows_u8_host_arguments():
    lib = api.lib()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.pm_pad_rows_u8(None, 0, 4, None, 4) == api.PM_OK            # n == 0: nothing is touched
    assert lib.pm_pad_rows_u8(None, 1, 4, p, 4) == api.PM_E_INVALID
    assert lib.pm_pad_rows_u8(p, 1, 4, None, 4) == api.PM_E_INVALID
    assert lib.pm_pad_rows_u8(p, 1, 0, p, 4) == api.PM_E_INVALID
    assert lib.pm_pad_rows_u8(p, 1, 8, p, 4) == api.PM_E_INVALID
    assert lib.pm_pad_rows_u8(p, -1, 4, p, 4) == api.PM_E_INVALID
