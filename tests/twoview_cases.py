"""The two input lists of the two-view refinement tests (test_twoview_refine_cpu.py and its sanitised child run), built on
the masks this repository's own C references produce: RANSAC-F of the oracle on synth.two_view, and RANSAC-E + pose
recovery of tests/essential_ref.c on synth.calibrated_view.  Cached per process."""
import functools

import numpy as np

import essential_ref as ER
from points_matching_amd import synth

F_LIST = [(2275, 1), (2275, 2), (2275, 3), (573, 4), (573, 5), (573, 6), (143, 7), (143, 8), (143, 9)]
POSE_LIST = [(seed, forward) for forward in (False, True) for seed in range(7, 13)]


def kv(K):
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


@functools.lru_cache(maxsize=None)
def f_case(n, seed):
    """synth.two_view(n, seed), RANSAC-F with 2000 hypotheses, 1.0 px, seed 11: (xy1, xy2, F_gt, truth, F0, mask)."""
    from oracle import pm_oracle
    pm_oracle.build()
    xy1, xy2, Fg, inl = synth.two_view(n, seed)
    rc, F0, mask, c, key = pm_oracle.ransac_fundamental(xy1, xy2, 2000, 1.0, 11)
    assert rc == 0 and c >= 8
    return xy1, xy2, Fg, inl, F0, mask


@functools.lru_cache(maxsize=None)
def pose_case(seed, forward):
    """synth.calibrated_view(2000, seed, outlier_frac=0.3, noise_px=0.5, forward), RANSAC-E with 1000 samples, 1.0 px,
    seed 11, then S35: (xy1, xy2, K, R_gt, t_gt, truth, R0, t0, pose mask)."""
    xy1, xy2, K, Rg, tg, X, inl = synth.calibrated_view(2000, seed=seed, outlier_frac=0.3, noise_px=0.5, forward=forward)
    k = kv(K)
    key, E, mask, c = ER.run(xy1, xy2, k, 1000, 1.0, 11)
    ng, R0, t0, pm, pts, g = ER.recover_pose(xy1, xy2, k, E, mask)
    assert key != 0 and ng >= 5
    return xy1, xy2, k, Rg, tg, inl, R0, t0, pm


def sampson_rms(F, x1, x2):
    """RMS Sampson distance (px) of F over the correspondences, in plain numpy fp64."""
    p1 = np.c_[x1, np.ones(len(x1))].astype(np.float64)
    p2 = np.c_[x2, np.ones(len(x2))].astype(np.float64)
    l, lt = p1 @ F.T, p2 @ F
    num = (p2 * l).sum(1)
    return np.sqrt(np.mean(num ** 2 / (l[:, 0] ** 2 + l[:, 1] ** 2 + lt[:, 0] ** 2 + lt[:, 1] ** 2)))


def rot_deg(Ra, Rb):
    """Angle of Ra^T Rb in degrees; the chord form keeps its resolution near zero, where arccos of the trace has none."""
    return np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(Ra - Rb) / (2.0 * np.sqrt(2.0)))))


def dir_deg(a, b):
    """Angle between two directions in degrees, by atan2 (resolution near zero)."""
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b)))
