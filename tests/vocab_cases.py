"""Deterministic inputs that drive the vocabulary kernels (docs/SPEC.md S102-S106) to their limits, and the restatement's
answers on them.  Plain numpy and tests/vocab_ref.c: no device.  test_vocab_limits_cpu.py asserts that every builder reaches
the regime it is named for; test_vocab_limits_gpu.py compares the device with the same cached answers, bit for bit.

  A  layout_case      every lane layout of vocab_update: u8 rows whose dword count does not divide 64 or leaves lanes idle,
                      bit rows with an odd dword count.
  B  float_tie_case   squared distances of 2^22 and more that share a float: S103 orders on sqrtf((float)D), so the lower
                      word index wins although its integer distance is the larger.
  C  big_k_case       K of 70 000 and 262 144: labels of 2^16 and more, almost every word empty.
  D  row_limit_case   n = max_rows = 2^24 rows on one word: a byte sum of 255 * 2^24, above 2^31."""
import functools

import numpy as np

import vocab_ref as R


def make_rows(kind, n, nbytes, seed, protos=40, sigma=20.0, flip=0.15):
    """Rows with cluster structure: prototypes plus noise of `sigma` (u8) or bits flipped with probability `flip`."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, protos, n)
    if kind == R.L2_U8:
        p = rng.integers(0, 256, (protos, nbytes))
        return np.clip(np.rint(p[lab] + rng.normal(0, sigma, (n, nbytes))), 0, 255).astype(np.uint8)
    p = rng.integers(0, 256, (protos, nbytes)).astype(np.uint8)
    return p[lab] ^ np.packbits((rng.random((n, nbytes * 8)) < flip).astype(np.uint8), axis=-1, bitorder="little")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- A: lane layouts -----------------------------------------------------------------------------------------------------------
LAYOUT_U8 = (12, 20, 68, 100, 132, 192, 252)
LAYOUT_BITS = (4, 12, 20, 36, 60)
LAYOUTS = [(R.L2_U8, b) for b in LAYOUT_U8] + [(R.BITS, b) for b in LAYOUT_BITS]
LAYOUT_K, LAYOUT_N, LAYOUT_ITERS = 37, 1500, 3


@functools.lru_cache(maxsize=None)
def layout_case(kind, nbytes):
    """(rows, the restatement's training from the stride start, its encoding of the rows with the trained words)."""
    rows = make_rows(kind, LAYOUT_N, nbytes, seed=300 + nbytes, protos=LAYOUT_K)
    full = R.train(kind, R.init_stride(rows, LAYOUT_K), rows, LAYOUT_ITERS)
    enc = R.encode(kind, full[0], rows)
    _frozen(rows, *full, *enc)
    return rows, full, enc


def u8_lane_groups(nbytes):
    """(rpi, S) of vocab_update<0>: rpi rows side by side in a wave-instruction, S sorted rows per lane group."""
    W = nbytes // 4
    rpi = 64 // W
    return rpi, (64 + rpi - 1) // rpi


def sorted_runs(labels, wave):
    """The runs of equal labels of wave `wave` in the kernel's sorted order (the key is label << 6 | lane, so equal labels
    keep their lane order): a list of (label, first sorted position, last sorted position)."""
    lab = np.sort(np.asarray(labels[64 * wave:64 * wave + 64]), kind="stable")
    cut = np.flatnonzero(np.diff(lab)) + 1
    first = np.concatenate(([0], cut))
    last = np.concatenate((cut, [lab.size])) - 1
    return [(int(lab[a]), int(a), int(b)) for a, b in zip(first, last)]


# ---- B: float-shared distances -------------------------------------------------------------------------------------------------
TIE_BYTES = (68, 128, 132, 192, 256)
TIE_K, TIE_N, TIE_ITERS = 64, 1000, 2
TIE_H = 2 * 255 * 255 + 1000
TIE_HOSTS = 3000                                            # ordinary rows around the planted ones in the embedded form


def four_squares(total):
    """Four values in 0..255 whose squares sum to `total`: the first hit, in row-major order of (a, b), whose rest is a sum
    of two squares itself."""
    sq = np.arange(256, dtype=np.int64) ** 2
    two = sq[:, None] + sq[None, :]
    is_two = np.zeros(int(two.max()) + 1, bool)
    is_two[two] = True
    rest = total - two
    ok = (rest >= 0) & (rest < is_two.size) & is_two[np.clip(rest, 0, is_two.size - 1)]
    assert ok.any(), total
    a, b = np.argwhere(ok)[0]
    c, d = np.argwhere(two == rest[a, b])[0]
    return [int(a), int(b), int(c), int(d)]


@functools.lru_cache(maxsize=None)
def tie_words(nbytes):
    words = np.full((TIE_K, nbytes), 255, np.uint8)
    for c in range(TIE_K):
        words[c, :4] = four_squares(TIE_H + (63 - c) % 8)
    return _frozen(words)[0]


def np_idist(rows, words):
    """(n, K) exact integer squared distances."""
    r, w = rows.astype(np.int64), words.astype(np.int64)
    return (r * r).sum(1)[:, None] + (w * w).sum(1)[None, :] - 2 * (r @ w.T)


@functools.lru_cache(maxsize=None)
def float_tie_case(nbytes, embedded=False):
    """(rows, words, positions of the planted rows, the restatement's training from the words, its encoding with them).
    A planted row is 0 in bytes 0..3 and uniform in [0, 32) elsewhere, every word 255 from byte 4 on, so D_c(row) =
    TIE_H + (63 - c) % 8 + shift(row): the integer minimum is at word 7, the float order decides among the words below it.
    `embedded`: the planted rows at random positions among TIE_HOSTS ordinary rows."""
    rng = np.random.default_rng(4000 + nbytes)
    planted = rng.integers(0, 32, (TIE_N, nbytes)).astype(np.uint8)
    planted[:, :4] = 0
    if embedded:
        rows = make_rows(R.L2_U8, TIE_HOSTS + TIE_N, nbytes, seed=4500 + nbytes)
        where = np.sort(rng.choice(TIE_HOSTS + TIE_N, TIE_N, replace=False))
        rows[where] = planted
    else:
        rows, where = planted, np.arange(TIE_N)
    words = tie_words(nbytes)
    full = R.train(R.L2_U8, words, rows, TIE_ITERS)
    enc = R.encode(R.L2_U8, words, rows)
    _frozen(rows, where, *full, *enc)
    return rows, words, where, full, enc


# ---- C: K at and above 2^16 ----------------------------------------------------------------------------------------------------
BIG_K = [(R.L2_U8, 4, 262144, 1000), (R.BITS, 4, 262144, 1000), (R.L2_U8, 12, 70000, 2000), (R.BITS, 12, 70000, 2000)]
BIG_K_ITERS, BIG_K_SHORT = 2, 7                             # the encoding runs with a device count of n - BIG_K_SHORT


@functools.lru_cache(maxsize=None)
def big_k_case(kind, nbytes, K, n):
    """(rows, words, the restatement's training from the words, its encoding of n - 7 rows with the trained words).  The
    words are K random rows; half of the rows are random too (their nearest word is anywhere in 0 .. K-1), the other half
    are copies of 40 words spread over the whole index range, word K - 1 among them, with one byte disturbed: runs of more
    than one row on labels of 2^16 and more."""
    rng = np.random.default_rng(5000 + nbytes + K)
    words = rng.integers(0, 256, (K, nbytes)).astype(np.uint8)
    rows = rng.integers(0, 256, (n, nbytes)).astype(np.uint8)
    pool = np.unique(np.concatenate(([K - 1, K - 2, 1 << 16, (1 << 16) - 1], rng.integers(0, K, 36))))
    near = rng.choice(n, n // 2, replace=False)
    rows[near] = words[pool[rng.integers(0, pool.size, near.size)]]
    rows[near, rng.integers(0, nbytes, near.size)] ^= (1 << rng.integers(0, 3, near.size)).astype(np.uint8)
    full = R.train(kind, words, rows, BIG_K_ITERS)
    enc = R.encode(kind, full[0], rows, n - BIG_K_SHORT)
    _frozen(rows, words, *full, *enc)
    return rows, words, full, enc


# ---- D: the row limit ----------------------------------------------------------------------------------------------------------
ROW_LIMIT_N, ROW_LIMIT_ITERS = 1 << 24, 2


def row_limit_rows():
    """2^24 rows of 4 bytes: 255 everywhere, byte 1 = 254 on every third row, byte 2 = 0 on rows 5, 12, 19, ...  Built on
    demand and not cached (64 MiB)."""
    rows = np.full((ROW_LIMIT_N, 4), 255, np.uint8)
    rows[::3, 1] = 254
    rows[5::7, 2] = 0
    return rows


ROW_LIMIT_WORDS = _frozen(np.array([[255] * 4, [0] * 4], np.uint8))[0]


@functools.lru_cache(maxsize=None)
def row_limit_ref(kind):
    """The restatement on row_limit_rows(): (final words, records, the words after every iteration, the histogram of the
    encoding with the final words, one period of its distances).  Every row takes word 0 in both iterations and in the
    encoding, and the rows repeat with period 21, so the per-row outputs are kept as what says so: all labels are 0 and
    the distances are np.resize(period, n)."""
    rows = row_limit_rows()
    words, labels, info, after = R.train(kind, ROW_LIMIT_WORDS, rows, ROW_LIMIT_ITERS)
    w, dist, hist = R.encode(kind, words, rows)
    assert not labels.any() and not w.any()
    period = dist[:21].copy()
    assert (dist.view(np.uint32) == np.resize(period, ROW_LIMIT_N).view(np.uint32)).all()
    return _frozen(words, info, after, hist, period)
