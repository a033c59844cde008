"""Cross-check rule of docs/SPEC.md S41, restated in numpy over two record arrays (no call into the library).

fwd: (nq, kf) pm_match records of the matcher on (q, t); rev: (nt, kr) records on (t, q).  Returns the surviving
forward first-neighbour records in query order.
"""
import numpy as np

RATIO_FWD, RATIO_REV = 1, 2


def _s4(rows, ratio):
    """SPEC S4 per row: both neighbours exist and d1 < ratio * d2 (one f32 multiply, strict)."""
    with np.errstate(invalid="ignore"):
        rhs = np.float32(ratio) * rows["distance"][:, 1].astype(np.float32)
    return (rows["trainIdx"][:, 0] >= 0) & (rows["trainIdx"][:, 1] >= 0) & (rows["distance"][:, 0] < rhs)


def cross_ref(fwd, rev, flags=0, ratio=0.8):
    nq, nt = fwd.shape[0], rev.shape[0]
    if nq == 0 or nt == 0:
        return fwd[:0, 0].copy()
    j = fwd["trainIdx"][:, 0]
    ok = (j >= 0) & (j < nt)
    js = np.where(ok, j, 0)
    ok &= rev["trainIdx"][js, 0] == np.arange(nq)
    if flags & RATIO_FWD:
        ok &= _s4(fwd, ratio)
    if flags & RATIO_REV:
        ok &= _s4(rev, ratio)[js]
    return fwd[ok, 0].copy()
