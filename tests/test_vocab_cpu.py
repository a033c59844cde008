"""CPU: visual vocabularies (docs/SPEC.md S102-S106) through the plain-C restatement tests/vocab_ref.c — against a numpy
model written independently here (broadcast distances, argmin, np.add.at), hand-made cases for every rule of S104, the
monotone cost, planted recovery on both row kinds — and the C ABI surface of libpm_hip.so: the prototypes, the exports and
the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vocab_ref as R
from points_matching_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (R.L2_U8, R.BITS)
ARITY = {"pm_vocab_create": 6, "pm_vocab_destroy": 1, "pm_vocab_set": 3, "pm_vocab_set_dev": 3, "pm_vocab_get": 3,
         "pm_vocab_init_stride_dev": 4, "pm_vocab_train_dev": 7, "pm_vocab_train": 7, "pm_vocab_assign_dev": 8,
         "pm_vocab_assign": 7}


# ---- the numpy model ---------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.unpackbits(np.ascontiguousarray(a, np.uint8), axis=-1, bitorder="little").astype(np.int64)


def np_dist(kind, rows, words):
    """(n, K) exact integer distances."""
    if kind == R.L2_U8:
        d = rows[:, None, :].astype(np.int64) - words[None, :, :].astype(np.int64)
        return (d * d).sum(-1)
    return (_bits(rows)[:, None, :] != _bits(words)[None, :, :]).sum(-1)


def np_train(kind, words, rows, iters):
    words = words.copy()
    K, n = words.shape[0], rows.shape[0]
    info, prev, lab = [], None, None
    for t in range(iters):
        d = np_dist(kind, rows, words)
        lab = d.argmin(1)                                   # the first minimum: the lowest word index
        cost = int(d[np.arange(n), lab].sum())
        n_changed = n if t == 0 else int((lab != prev).sum())
        cnt = np.bincount(lab, minlength=K).astype(np.int64)
        full = cnt > 0
        src = rows.astype(np.int64) if kind == R.L2_U8 else _bits(rows)
        acc = np.zeros((K, src.shape[1]), np.int64)
        np.add.at(acc, lab, src)
        new = words.copy()
        c = cnt[full][:, None]
        if kind == R.L2_U8:
            new[full] = ((2 * acc[full] + c) // (2 * c)).astype(np.uint8)
        else:
            new[full] = np.packbits((2 * acc[full] > c).astype(np.uint8), axis=-1, bitorder="little")
        n_moved = int((new != words).any(1).sum())
        info.append((n_changed, int((~full).sum()), n_moved, 0, cost))
        words, prev = new, lab
    return words, lab.astype(np.int32), np.array(info, R.ITER_DTYPE)


def _random(kind, n, nbytes, seed):
    rng = np.random.default_rng(seed)
    if kind == R.L2_U8:
        return rng.integers(0, 256, (n, nbytes)).astype(np.uint8)
    # bit rows with structure: a few prototypes with flipped bits, so that majorities are not all coin tosses
    proto = rng.integers(0, 256, (7, nbytes)).astype(np.uint8)
    flips = np.packbits((rng.random((n, nbytes * 8)) < 0.2).astype(np.uint8), axis=-1, bitorder="little")
    return proto[rng.integers(0, 7, n)] ^ flips


# ---- the restatement against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_restatement_equals_the_numpy_model(kind):
    rows = _random(kind, 300, 8, seed=11 + kind)
    w0 = R.init_stride(rows, 5)
    assert (w0 == rows[[0, 60, 120, 180, 240]]).all()
    words, labels, info, after = R.train(kind, w0, rows, 6)
    mw, ml, mi = np_train(kind, w0, rows, 6)
    assert (words == mw).all() and (labels == ml).all() and (after[-1] == words).all()
    for f in R.ITER_DTYPE.names:
        assert (info[f] == mi[f]).all(), f
    assert info["n_changed"][0] == 300 and (info["reserved"] == 0).all()
    lab, dist, di = R.assign(kind, words, rows)
    d = np_dist(kind, rows, words)
    assert (lab == d.argmin(1)).all() and (di == d.min(1)).all()
    want = np.sqrt(d.min(1).astype(np.float32)) if kind == R.L2_U8 else d.min(1).astype(np.float32)
    assert (dist.view(np.uint32) == want.astype(np.float32).view(np.uint32)).all()


def test_iters_zero_runs_nothing():
    rows = _random(R.L2_U8, 20, 4, seed=1)
    words, labels, info, _ = R.train(R.L2_U8, rows[:3], rows, 0)
    assert (words == rows[:3]).all() and (labels == -9).all() and info.size == 0


# ---- S104, rule by rule --------------------------------------------------------------------------------------------------------
def test_a_mean_on_one_half_rounds_up():
    rows = np.array([[10, 0, 255, 7], [11, 1, 254, 7], [200, 200, 200, 200]], np.uint8)
    words, ne, nm = R.update(R.L2_U8, np.array([[0, 0, 0, 0], [9, 9, 9, 9]], np.uint8), rows, [0, 0, 1])
    assert words.tolist() == [[11, 1, 255, 7], [200, 200, 200, 200]] and (ne, nm) == (0, 2)
    rows = np.array([[0], [0], [1], [1], [1], [2]], np.uint8).repeat(4, 1)     # mean 5 / 6: rounds to 1; and 2.5 -> 3
    assert R.update(R.L2_U8, np.zeros((1, 4), np.uint8), rows, [0] * 6)[0].tolist() == [[1, 1, 1, 1]]
    rows = np.array([[2], [3]], np.uint8).repeat(4, 1)
    assert R.update(R.L2_U8, np.zeros((1, 4), np.uint8), rows, [0, 0])[0].tolist() == [[3, 3, 3, 3]]


def test_an_even_bit_split_gives_zero():
    rows = np.array([[0b1111, 0, 0, 0x80], [0b0101, 0, 0, 0x80], [0b0011, 0xFF, 0, 0], [0b0001, 0xFF, 0, 0]], np.uint8)
    words, ne, nm = R.update(R.BITS, np.full((1, 4), 0xFF, np.uint8), rows, [0, 0, 0, 0])
    # bit 0: 4 of 4 -> 1; bit 1: 2 of 4 -> 0; bit 2: 2 of 4 -> 0; bit 3: 1 of 4 -> 0; byte 1 and the top bit of byte 3: 2 of 4 -> 0
    assert words.tolist() == [[0b0001, 0, 0, 0]] and (ne, nm) == (0, 1)
    words, _, _ = R.update(R.BITS, np.zeros((1, 4), np.uint8), rows[:3], [0, 0, 0])
    assert words.tolist() == [[0b0111, 0, 0, 0x80]]                             # 3 rows: 2 of 3 is a majority


@pytest.mark.parametrize("kind", KINDS)
def test_duplicate_initial_words_leave_the_higher_index_empty(kind):
    rows = _random(kind, 200, 8, seed=5)
    w0 = np.stack([rows[0], rows[7], rows[0], rows[30]])
    words, labels, info, after = R.train(kind, w0, rows, 3)
    assert info["n_empty"][0] >= 1 and (after[0][2] == w0[2]).all()             # word 2 got no row and kept its bytes
    lab0 = R.assign(kind, w0, rows)[0]
    assert not (lab0 == 2).any() and (lab0 == 0).any()


@pytest.mark.parametrize("kind", KINDS)
def test_fewer_rows_than_words_repeat_under_the_stride_rule(kind):
    rows = _random(kind, 3, 8, seed=6)
    w0 = R.init_stride(rows, 8)
    assert (w0 == rows[[0, 0, 0, 1, 1, 1, 2, 2]]).all()                          # floor(i * 3 / 8)
    words, labels, info, _ = R.train(kind, w0, rows, 2)
    assert labels.tolist() == [0, 3, 6] and info["n_empty"].tolist() == [5, 5] and info["n_moved"].tolist() == [0, 0]
    assert info["cost"].tolist() == [0, 0] and (words == w0).all()
    big = np.arange(5 * 4, dtype=np.uint8).reshape(5, 4)
    assert (R.init_stride(big, 5) == big).all() and (R.init_stride(big, 2) == big[[0, 2]]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_cost_never_rises(kind):
    """S104: the rounded mean minimises the summed squared distance per dimension over the integers and the majority bit
    the Hamming sum, and S103 moves a row only to a word that is not farther: no step of an iteration raises the cost.
    (Rows of 8 and 16 bytes: squared distances stay below 2^22, where the matcher's float order is the integer order.)"""
    for nbytes, seed in ((8, 21), (16, 22)):
        rows = _random(kind, 400, nbytes, seed=seed)
        info = R.train(kind, R.init_stride(rows, 9), rows, 12)[2]
        cost = info["cost"].astype(np.int64)
        assert (np.diff(cost) <= 0).all(), cost
        assert cost[0] > cost[-1]


def test_encoding_tails_and_histogram():
    rows = _random(R.L2_U8, 50, 8, seed=3)
    words = R.init_stride(rows, 6)
    lab = R.assign(R.L2_U8, words, rows)[0]
    for count, m in ((None, 50), (50, 50), (49, 49), (0, 0), (-1, 0), (57, 50)):
        w, d, h = R.encode(R.L2_U8, words, rows, count)
        assert (w[:m] == lab[:m]).all() and (w[m:] == -1).all() and np.isnan(d[m:]).all() and not np.isnan(d[:m]).any()
        assert (h == np.bincount(lab[:m], minlength=6)).all() and h.sum() == m


# ---- planted recovery ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_planted_recovery_l2(seed):
    rng = np.random.default_rng(seed)
    centres = rng.integers(30, 226, (8, 16))
    planted = rng.integers(0, 8, 3000)
    rows = np.clip(np.rint(centres[planted] + rng.normal(0, 6, (3000, 16))), 0, 255).astype(np.uint8)
    w0 = np.stack([rows[np.flatnonzero(planted == c)[0]] for c in range(8)])
    words, labels, info, _ = R.train(R.L2_U8, w0, rows, 3)
    assert info["n_changed"][1] == 0
    assert np.abs(words.astype(np.int64) - centres).max() <= 1
    assert (labels == planted).all()


@pytest.mark.parametrize("seed", range(5))
def test_planted_recovery_bits(seed):
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 256, (16, 32)).astype(np.uint8)
    planted = rng.integers(0, 16, 2000)
    flips = np.packbits((rng.random((2000, 256)) < 0.1).astype(np.uint8), axis=-1, bitorder="little")
    rows = centres[planted] ^ flips
    w0 = np.stack([rows[np.flatnonzero(planted == c)[0]] for c in range(16)])
    words, labels, info, _ = R.train(R.BITS, w0, rows, 3)
    assert (words == centres).all() and (labels == planted).all()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_prototypes_and_exports():
    hdr = open(os.path.join(ROOT, "include", "pm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = api.lib()
    for name, arity in ARITY.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == arity, name
        assert name in api.EXPORTS and hasattr(L, name), name
    assert re.search(r"#define\s+PM_VOCAB_L2_U8\s+0\b", code) and re.search(r"#define\s+PM_VOCAB_BITS\s+1\b", code)
    assert (api.PM_VOCAB_L2_U8, api.PM_VOCAB_BITS) == (0, 1) == (R.L2_U8, R.BITS)
    assert "typedef struct pm_vocab_iter { int32_t n_changed, n_empty, n_moved, reserved; uint64_t cost; } pm_vocab_iter;" in code
    assert api.VOCAB_ITER_DTYPE.itemsize == 24 and api.VOCAB_ITER_DTYPE == R.ITER_DTYPE
    r = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    syms = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    assert not [n for n in ARITY if n not in syms]


def test_refusals_without_a_device():
    L = api.lib()
    INV, UNS = api.PM_E_INVALID, api.PM_E_UNSUPPORTED
    h = C.c_void_p(7)
    d = C.c_void_p(256)                                       # never dereferenced: every call below is refused first

    def refused(rc, status, msg):
        return rc == status and msg in L.pm_last_error()

    def create(kind=0, nbytes=128, K=8, max_rows=1000, out=True):
        h.value = 7
        return L.pm_vocab_create(None, kind, nbytes, K, max_rows, C.byref(h) if out else None)

    assert refused(create(out=False), INV, b"null output")
    for kind in (-1, 2):
        assert refused(create(kind=kind), INV, b"PM_VOCAB_") and not h.value
    for kind, nbytes in ((0, 0), (0, -4), (0, 6), (0, 2), (0, 260), (0, 257), (1, 68), (1, 128), (1, 3), (1, 0)):
        assert refused(create(kind=kind, nbytes=nbytes), INV, b"bytes must be") and not h.value
    for K in (0, -1, 262145):
        assert refused(create(K=K), INV, b"1 <= K <= 262144")
    assert refused(create(max_rows=0), INV, b"max_rows >= 1") and refused(create(max_rows=-5), INV, b"max_rows >= 1")
    assert refused(create(max_rows=(1 << 24) + 1), UNS, b"2^24") and not h.value
    for kind, nbytes, K, mr in ((0, 4, 1, 1), (0, 256, 262144, 1 << 24), (1, 64, 262144, 1 << 24), (1, 4, 1, 1)):
        assert refused(create(kind, nbytes, K, mr), INV, b"ctx is null") and not h.value   # the limits themselves pass
    for iters in (-1, 1001):
        assert refused(L.pm_vocab_train_dev(None, None, d, 10, iters, None, None), INV, b"0 <= iters <= 1000")
        assert refused(L.pm_vocab_train(None, None, d, 10, iters, None, None), INV, b"0 <= iters <= 1000")
    for iters in (0, 1000):
        assert refused(L.pm_vocab_train_dev(None, None, d, 10, iters, None, None), INV, b"null argument")
        assert refused(L.pm_vocab_train(None, None, d, 10, iters, None, None), INV, b"null argument")
    assert refused(L.pm_vocab_assign_dev(None, None, d, 10, None, None, None, None), INV, b"null argument")
    assert refused(L.pm_vocab_assign(None, None, d, 10, None, None, None), INV, b"null argument")
    assert refused(L.pm_vocab_init_stride_dev(None, None, d, 10), INV, b"null argument")
    for fn in (L.pm_vocab_set, L.pm_vocab_set_dev, L.pm_vocab_get):
        assert refused(fn(None, None, d), INV, b"null argument")
    assert L.pm_vocab_destroy(None) == api.PM_OK
