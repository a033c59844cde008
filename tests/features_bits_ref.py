"""Numpy restatement of the binary descriptor of the feature front end (docs/SPEC.md S58-S60), independent of the C++ and
HIP code: the 256 lattice tests, their steered int8 offsets, and the 32 packed bytes of a keypoint from its Gaussian level."""
import hashlib

import numpy as np

MASK = (1 << 64) - 1
SEED = 0x504D4249545331
R2 = (23, 28, 35)
# sha256 of the 1024 int8 values of base_pattern(), row-major (S58)
PATTERN_SHA256 = "a7eb670509bf4b2fa7132146c22402c25937f36f3ef474905bc24e636da4c11f"


def splitmix64(state):
    """One step: (new state, output)."""
    state = (state + 0x9E3779B97F4A7C15) & MASK
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return state, z ^ (z >> 31)


def base_pattern():
    """S58: (256, 4) int8 tests (x1, y1, x2, y2)."""
    state = SEED
    kept, seen = [], set()
    while len(kept) < 256:
        c = []
        for _ in range(4):
            v = 0
            for _ in range(3):
                state, z = splitmix64(state)
                v += (z >> 33) % 11 - 5
            c.append(v)
        x1, y1, x2, y2 = c
        if x1 * x1 + y1 * y1 > 225 or x2 * x2 + y2 * y2 > 225:
            continue
        if (x1, y1) == (x2, y2):
            continue
        if (x1, y1, x2, y2) in seen or (x2, y2, x1, y1) in seen:
            continue
        seen.add((x1, y1, x2, y2))
        kept.append(c)
    return np.array(kept, np.int8)


def pattern_sha256(base):
    return hashlib.sha256(np.ascontiguousarray(base, np.int8).tobytes()).hexdigest()


def steered(base, cos, sin):
    """S59: (3, 36, 256, 4) int8 offsets (dx1, dy1, dx2, dy2) from the 36 bin-centre cosines and sines (float64)."""
    out = np.zeros((3, 36, 256, 4), np.int8)
    b = base.astype(np.float64)
    for l in range(3):
        s = R2[l] / 15.0
        for k in range(36):
            cs, sn = np.float64(cos[k]), np.float64(sin[k])
            for p in (0, 2):
                x, y = b[:, p], b[:, p + 1]
                out[l, k, :, p] = np.rint(s * (cs * x - sn * y)).astype(np.int8)
                out[l, k, :, p + 1] = np.rint(s * (sn * x + cs * y)).astype(np.int8)
    return out


def describe(level, x, y, offsets):
    """S60: the 32 bytes of the keypoint at column x, row y of its Gaussian level; offsets: (256, 4) int8 of its level and bin."""
    o = offsets.astype(np.int64)
    a = level[y + o[:, 1], x + o[:, 0]]
    b = level[y + o[:, 3], x + o[:, 2]]
    return np.packbits(a < b, bitorder="little")


def hamming_2nn(q, t):
    """Brute-force Hamming 2-NN of u8 rows: (idx (n, 2), dist (n, 2)), ties to the lower train index."""
    pop = np.array([bin(i).count("1") for i in range(256)], np.int32)
    d = pop[q[:, None, :] ^ t[None, :, :]].sum(axis=2)
    idx = np.argsort(d, axis=1, kind="stable")[:, :2]
    return idx, np.take_along_axis(d, idx, axis=1)
