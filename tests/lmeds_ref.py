"""Independent fp64 reference for the scoring rule of docs/SPEC.md S15 (LMedS over 7-point models): pure numpy, written
from the textbook definitions, not from the oracle or the kernels.  Shared by test_lmeds_independent_cpu.py (the C
oracle standing in for the device) and test_lmeds_limits_gpu.py.

  residuals   symmetric epipolar distance max(d^2 / |l1|^2, d^2 / |l2|^2) with d = x2^T F x1, l2 = F x1 the line in
              image 2 and l1 = F^T x2 the line in image 1, by matrix products in float64 (no fma, no reciprocal);
              a residual that is not a number counts as +inf
  median      np.sort, v[n/2] for odd n and (v[n/2 - 1] + v[n/2]) / 2 for even n
  sigma, thr  2.5 * 1.4826 * (1 + 5 / (n - 7)) * sqrt(median), at least 0.001; thr = sigma^2
  mask        residual <= thr

The device rounds every residual to f32 before it sorts, so its median differs from this one by rounding only:
MEDIAN_RTOL = 2^-22 (2^-24 for the rounding of one residual, a factor 2 because an even n averages two of them, a
factor 2 of margin for the fused evaluation order).  A relative bound means nothing for an exact fit, where the
median is cancellation noise: it applies from MEDIAN_FLOOR = 1e-6 px^2 up.  The mask is compared outside the band
|e - thr| <= BAND_RTOL * thr, and the band may hold at most BAND_MAX_FRAC of the correspondences."""
import numpy as np

MEDIAN_RTOL = 2.0 ** -22
MEDIAN_FLOOR = 1e-6
BAND_RTOL = 1e-5
BAND_MAX_FRAC = 1e-3


def residuals(F, xy1, xy2):
    F = np.asarray(F, np.float64).reshape(3, 3)
    h1 = np.column_stack([np.asarray(xy1, np.float64), np.ones(len(xy1))])
    h2 = np.column_stack([np.asarray(xy2, np.float64), np.ones(len(xy2))])
    with np.errstate(all="ignore"):
        l2 = h1 @ F.T                                # rows: F x1
        l1 = h2 @ F                                  # rows: F^T x2
        d = (h2 * l2).sum(axis=1)                    # x2^T F x1
        e = np.maximum(d * d / (l1[:, 0] ** 2 + l1[:, 1] ** 2), d * d / (l2[:, 0] ** 2 + l2[:, 1] ** 2))
    return np.where(np.isnan(e), np.inf, e)          # (np.maximum propagates NaN)


def median(e):
    v = np.sort(np.asarray(e, np.float64))
    n = v.size
    if n & 1:
        return float(v[n // 2])
    with np.errstate(all="ignore"):
        return float((v[n // 2 - 1] + v[n // 2]) * 0.5)


def threshold(med, n):
    sigma = 2.5 * 1.4826 * (1.0 + 5.0 / (n - 7)) * np.sqrt(med)
    sigma = max(sigma, 0.001)
    return sigma * sigma


def strictly_below_upper_median(e):
    """Number of f32-rounded residuals strictly below v[n/2]: n/2 when v[n/2 - 1] < v[n/2], fewer when the two tie."""
    with np.errstate(over="ignore"):
        v = np.sort(np.asarray(e, np.float64).astype(np.float32))
    return int((v < v[v.size // 2]).sum())


def check_median(F, xy1, xy2, med):
    """Reported median against the fp64 one.  Returns (relative difference or None below the floor, fp64 median)."""
    ref = median(residuals(F, xy1, xy2))
    if not np.isfinite(ref):
        assert med == np.inf, (med, ref)
        return None, ref
    if ref < MEDIAN_FLOOR:
        assert med < 2.0 * MEDIAN_FLOOR, (med, ref)
        return None, ref
    rel = abs(med - ref) / ref
    assert rel <= MEDIAN_RTOL, (med, ref, rel)
    return rel, ref


def check_mask(F, xy1, xy2, mask, n_inliers):
    """Reported mask against fp64 residuals and the fp64 threshold, outside the border band.  Returns the band count."""
    e = residuals(F, xy1, xy2)
    return check_mask_at(F, xy1, xy2, mask, n_inliers, threshold(median(e), e.size), e)


def check_mask_at(F, xy1, xy2, mask, n_inliers, thr, e=None):
    """As check_mask for a given squared threshold (S16: thr = thresh_px^2)."""
    e = residuals(F, xy1, xy2) if e is None else e
    n = e.size
    with np.errstate(invalid="ignore"):
        band = np.abs(e - thr) <= BAND_RTOL * thr
    assert band.sum() <= BAND_MAX_FRAC * n, (int(band.sum()), n)
    want = e <= thr
    bad = np.nonzero((want != np.asarray(mask).astype(bool)) & ~band)[0]
    assert bad.size == 0, (bad[:5], e[bad[:5]], thr)
    assert abs(int(want.sum()) - int(n_inliers)) <= int(band.sum()) and int(n_inliers) == int(np.asarray(mask).sum())
    return int(band.sum())
