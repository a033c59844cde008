"""Plain numpy references for the stable compactions (no call into the library): the ratio rule (docs/SPEC.md S4), the
midpoint rule (main.cpp:49-69, as include/pm.h states it), the cross rule (cross_ref.py), the keypoint gather, and a
generator of k-NN records whose keep-vector is fixed BY CONSTRUCTION, not by running a rule.

Patterns (which rows survive):
  all             every row
  none            no row
  checker         blocks of 256 rows alternately all kept and all dropped (block 0 kept)
  last_only       only row nq - 1
  first_of_block  only the rows with i % 256 == 0
  half            a random half of the rows

make_records(nq, pattern, rng) returns a Records bundle: one forward list `fwd` (nq x k) and one reverse list `rev`
(nt = nq rows x 2) on which the ratio rule at RATIO, the cross rule with flags 0 and the cross rule with FWD | REV all
keep exactly `keep`; a 1-NN list `mid` on which the midpoint rule keeps exactly `keep`, with `mid_minmax` its
[minMatch, maxMatch]; keypoints kp1 (nq x 2) and kp2 (nt x 2).  Every queryIdx equals its row, every trainIdx is -1 or
in [0, nt).

Why the rows of `fwd` are kept or dropped (ratio rule, RATIO = 0.8, rhs = float32(RATIO) * d2 in float32):
  kept     d1 = the float32 just below rhs (one ulp), or d1 = 0, or d1 = rhs / 2, both neighbours present
  dropped  one reason per row, in turn:
           0  d1 == d2
           1  d1 = the float32 just above rhs (one ulp)
           2  second trainIdx = -1 with distance +inf (d1 finite: only the index test drops the row)
           3  first trainIdx = -1 (distances that would pass: only the index test drops the row)
           4  d1 = NaN
           5  d2 = NaN
           6  d1 == rhs exactly (the comparison is strict)
Cross rule on (fwd, rev): fwd[i, 0].trainIdx = perm[i] for a shuffled permutation perm (reason 3 rows: -1).  A kept row
i has rev[perm[i], 0].trainIdx = i and a reverse row that passes the ratio test; a dropped row's reverse record names
another query row or -1, so it fails the mutual test whatever the flags.
Midpoint rule on `mid` (min starts at 1, max at 0; cut = min + (max - min) / 2 in double; keep iff d < cut):
  some row kept, some dropped   first kept row d = -8 (the minimum), first dropped row d = 2 (the maximum): cut = -3.
                                kept: [-8, -4.5) or the float32 just below -3; dropped: 2, -3 (== cut, strict), NaN, 0,
                                [1, 2), the float32 just above -3
  every row kept                max stays at its start value 0, min = -8: cut = -4; all d in [-8, -4.5) or just below -4
  no row kept                   d = 0.5 or NaN: min = max = 0.5 (or 1 and 0 if all are NaN) and 0.5 < 0.5 fails
"""
from types import SimpleNamespace

import numpy as np

from cross_ref import cross_ref

MATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
PATTERNS = ("all", "none", "checker", "last_only", "first_of_block", "half")
RATIO = 0.8
BLOCK = 256
N_DROP_REASONS = 7


# ---- the rules -----------------------------------------------------------------------------------------------------------------

def ratio_keep(knn, ratio):
    """Boolean keep-vector of the ratio rule on (nq, k >= 2) records."""
    with np.errstate(invalid="ignore"):
        rhs = np.float32(ratio) * knn["distance"][:, 1].astype(np.float32)       # float32 product
        return (knn["trainIdx"][:, 0] >= 0) & (knn["trainIdx"][:, 1] >= 0) & (knn["distance"][:, 0] < rhs)


def ratio_rule(knn, ratio):
    return knn[ratio_keep(knn, ratio), 0].copy()


def midpoint_rule(m):
    """m: (n,) records.  Returns (survivors, minMatch, maxMatch) with the two values as Python floats (doubles)."""
    d = m["distance"].astype(np.float32)
    lo, hi = np.float32(1.0), np.float32(0.0)
    ok = ~np.isnan(d)                                                           # a NaN never wins a comparison
    if ok.any():
        lo, hi = min(lo, d[ok].min()), max(hi, d[ok].max())
    lo, hi = float(lo), float(hi)
    cut = lo + (hi - lo) / 2
    with np.errstate(invalid="ignore"):
        keep = d.astype(np.float64) < cut
    return m[keep].copy(), lo, hi


def cross_rule(fwd, rev, flags, ratio):
    return cross_ref(fwd, rev, flags, ratio)


def gather(kp1, kp2, good):
    return kp1[good["queryIdx"]], kp2[good["trainIdx"]]


# ---- the pattern generator ---------------------------------------------------------------------------------------------------

def keep_vector(nq, pattern, rng):
    i = np.arange(nq)
    if pattern == "all":
        return np.ones(nq, bool)
    if pattern == "none":
        return np.zeros(nq, bool)
    if pattern == "checker":
        return (i // BLOCK) % 2 == 0
    if pattern == "last_only":
        return i == nq - 1
    if pattern == "first_of_block":
        return i % BLOCK == 0
    if pattern == "half":
        keep = np.zeros(nq, bool)
        keep[rng.permutation(nq)[:nq // 2]] = True
        return keep
    raise ValueError(pattern)


def _up(x):
    return np.nextafter(x, np.float32(np.inf), dtype=np.float32)


def _down(x):
    return np.nextafter(x, np.float32(-np.inf), dtype=np.float32)


def _ratio_rows(n, keep, rng, ratio):
    """(d1, d2, first_present, second_present, reason) of n rows; reason = -1 on kept rows."""
    d2 = (rng.random(n, dtype=np.float32) * np.float32(1.5) + np.float32(0.5)).astype(np.float32)     # [0.5, 2)
    rhs = (np.float32(ratio) * d2).astype(np.float32)
    d1 = _down(rhs)
    style = rng.integers(0, 3, n)
    d1 = np.where(style == 1, np.float32(0.0), d1)
    d1 = np.where(style == 2, rhs * np.float32(0.5), d1).astype(np.float32)
    reason = np.full(n, -1)
    dropped = np.nonzero(~keep)[0]
    reason[dropped] = np.arange(dropped.size) % N_DROP_REASONS
    first = np.ones(n, bool)
    second = np.ones(n, bool)
    d1 = np.where(reason == 0, d2, d1)
    d1 = np.where(reason == 1, _up(rhs), d1)
    second[reason == 2] = False
    first[reason == 3] = False
    d1 = np.where(reason == 4, np.float32(np.nan), d1)
    d1 = np.where(reason == 6, rhs, d1).astype(np.float32)
    d2 = np.where(reason == 2, np.float32(np.inf), d2)
    d2 = np.where(reason == 5, np.float32(np.nan), d2).astype(np.float32)
    return d1, d2, first, second, reason


def _midpoint_distances(keep, rng):
    n = keep.size
    kept, dropped = np.nonzero(keep)[0], np.nonzero(~keep)[0]
    d = np.empty(n, np.float32)
    if kept.size == 0:
        d[:] = np.where(np.arange(n) % 3 == 2, np.float32(np.nan), np.float32(0.5))
        ok = ~np.isnan(d)
        return d, ([0.5, 0.5] if ok.any() else [1.0, 0.0])
    cut = np.float32(-3.0) if dropped.size else np.float32(-4.0)
    d[kept] = (rng.random(kept.size, dtype=np.float32) * np.float32(3.5) - np.float32(8.0)).astype(np.float32)
    d[kept] = np.minimum(d[kept], np.float32(-4.5))
    d[kept[1::5]] = _down(cut)
    d[kept[0]] = -8.0
    why = np.arange(dropped.size) % 6
    vals = np.select([why == 0, why == 1, why == 2, why == 3, why == 4],
                     [np.float32(2.0), np.float32(-3.0), np.float32(np.nan), np.float32(0.0),
                      rng.random(dropped.size, dtype=np.float32) + np.float32(1.0)], _up(np.float32(-3.0)))
    d[dropped] = vals.astype(np.float32)
    return d, [-8.0, 2.0 if dropped.size else 0.0]


def make_records(nq, pattern, rng, k=2, ratio=RATIO):
    keep = keep_vector(nq, pattern, rng)
    nt = nq
    rows = np.arange(nq, dtype=np.int32)
    perm = rng.permutation(nt).astype(np.int32)
    d1, d2, first, second, reason = _ratio_rows(nq, keep, rng, ratio)
    fwd = np.zeros((nq, k), MATCH_DTYPE)
    fwd["queryIdx"] = rows[:, None]
    fwd["trainIdx"][:, 0] = np.where(first, perm, -1)
    fwd["trainIdx"][:, 1] = np.where(second, np.roll(perm, 1), -1)
    fwd["distance"][:, 0] = d1
    fwd["distance"][:, 1] = d2
    for c in range(2, k):                                                       # further neighbours: never read by a rule
        fwd["trainIdx"][:, c] = np.roll(perm, c)
        fwd["distance"][:, c] = rng.random(nq, dtype=np.float32) + np.float32(3.0)
    # reverse list: row perm[i] belongs to query row i
    r1, r2, _, _, _ = _ratio_rows(nq, np.ones(nq, bool), rng, ratio)             # every reverse row passes the ratio test
    other = np.where(rows % 2 == 0, (rows + 1) % nq if nq > 1 else -1, -1).astype(np.int32)
    rev = np.zeros((nt, 2), MATCH_DTYPE)
    rev["queryIdx"] = np.arange(nt, dtype=np.int32)[:, None]
    rev["trainIdx"][perm, 0] = np.where(keep, rows, other)
    rev["trainIdx"][perm, 1] = (rows + 2) % nq
    rev["distance"][perm, 0] = r1
    rev["distance"][perm, 1] = r2
    mid = np.zeros(nq, MATCH_DTYPE)
    mid["queryIdx"] = rows
    mid["trainIdx"] = perm
    mid["distance"], mid_minmax = _midpoint_distances(keep, rng)
    kp1 = (rng.random((nq, 2), dtype=np.float32) * np.float32(900.0)).astype(np.float32)
    kp2 = (rng.random((nt, 2), dtype=np.float32) * np.float32(600.0)).astype(np.float32)
    return SimpleNamespace(nq=nq, nt=nt, k=k, ratio=ratio, pattern=pattern, keep=keep, fwd=fwd, rev=rev, mid=mid,
                           mid_minmax=mid_minmax, reason=reason, kp1=kp1, kp2=kp2)
