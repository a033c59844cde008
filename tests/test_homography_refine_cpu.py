"""CPU: the restatement of docs/SPEC.md S23-S25 (tests/homography_refine_ref.c) — refinement of the robust homography
on its inliers — checked against an INDEPENDENT algorithm (numpy's SVD-based normalised least-squares DLT), against the
planted H of synth.planar_view, on its degenerate paths, plus the argument checks of the shipped entry points, which
need no device.  The restatement produces the GPU's bits (test_homography_refine_gpu.py), so the accuracy thresholds
here hold for the kernel's outputs too."""
import ctypes as C

import numpy as np

import homography_ref as R
import homography_refine_ref as RR
from points_matching_amd import api, synth


def _svd_dlt(x1, x2):
    """Hartley-normalised least-squares DLT by SVD (numpy), in the S20 output convention."""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)

    def T(x):
        c = x.mean(0)
        s = np.sqrt(2.0) / np.sqrt(((x - c) ** 2).sum(1)).mean()
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])

    T1, T2 = T(x1), T(x2)
    a = np.column_stack([x1, np.ones(len(x1))]) @ T1.T
    b = np.column_stack([x2, np.ones(len(x2))]) @ T2.T
    A = np.zeros((2 * len(a), 9))
    A[0::2, 0:3] = -a
    A[0::2, 6:9] = b[:, :1] * a
    A[1::2, 3:6] = -a
    A[1::2, 6:9] = b[:, 1:2] * a
    H = np.linalg.inv(T2) @ np.linalg.svd(A)[2][-1].reshape(3, 3) @ T1
    H /= np.linalg.norm(H)
    return -H if H[2, 2] < 0 else H


def _transfer(H, Hg, x):
    p = np.column_stack([x, np.ones(len(x))]).astype(np.float64)
    a, b = p @ H.T, p @ Hg.T
    return np.linalg.norm(a[:, :2] / a[:, 2:3] - b[:, :2] / b[:, 2:3], axis=1)


def test_refit_agrees_with_numpy_svd_dlt():
    for seed, noise, n in ((1, 0.0, 300), (2, 0.5, 2275), (3, 1.0, 900), (4, 0.5, 40)):
        x1, x2, _, inl = synth.planar_view(n, seed=seed, noise_px=noise, outlier_frac=0.3)
        ok, H = RR.refit(x1, x2, inl)
        assert ok
        Hs = _svd_dlt(x1[inl], x2[inl])
        assert np.abs(H - Hs).max() < 1e-9, (seed, np.abs(H - Hs).max())
        assert abs(np.linalg.norm(H) - 1.0) < 1e-15 and H[2, 2] >= 0


def test_refit_recovers_the_planted_homography_on_noiseless_data():
    # an affine map that is exact in float32 on integer points: nothing but the refit's own arithmetic is left
    rng = np.random.default_rng(7)
    x1 = rng.integers(0, 1000, (500, 2)).astype(np.float32)
    A = np.array([[0.75, 0.5, 16.0], [-0.25, 1.25, -8.0], [0.0, 0.0, 1.0]])
    x2 = (np.column_stack([x1, np.ones(500)]) @ A.T)[:, :2].astype(np.float32)
    ok, H = RR.refit(x1, x2, np.ones(500, np.uint8))
    assert ok and np.abs(H - A / np.linalg.norm(A)).max() < 1e-9
    # synth.planar_view with perspective: the float32 rounding of the points bounds what any estimator recovers
    x1, x2, Hg, inl = synth.planar_view(2275, seed=3, noise_px=0.0, outlier_frac=0.3)
    ok, H = RR.refit(x1, x2, inl)
    assert ok and np.abs(H - Hg).max() < 1e-7
    assert _transfer(H, Hg, x1[inl]).max() < 1e-3


def test_cost_never_increases_on_a_seeded_sweep():
    rng = np.random.default_rng(24)
    statuses = set()
    for case in range(40):
        n = int(rng.choice([6, 30, 300, 1200]))
        x1, x2, _, _ = synth.planar_view(n, seed=100 + case, noise_px=float(rng.uniform(0.0, 2.0)),
                                         outlier_frac=float(rng.uniform(0.0, 0.5)))
        key, Hr, m, c = R.run(x1, x2, 500, float(rng.uniform(0.5, 4.0)), case)
        if key == 0:
            continue
        for it in (0, 1, 10):
            H, info = RR.refine(x1, x2, m, Hr, it)
            statuses.add(info.status)
            assert info.cost_out <= info.cost_in, (case, it, info.as_tuple())
            assert info.n_used == c and 0 <= info.iters <= it
            assert info.cost_in == RR.cost(x1, x2, m, Hr)
            assert np.isfinite(H).all() and abs(np.linalg.norm(H) - 1.0) < 1e-14 and H[2, 2] >= 0
            if info.status == 1:
                assert (H.view(np.uint64) == Hr.view(np.uint64)).all() and info.cost_out == info.cost_in
    assert 0 in statuses


def test_refinement_is_far_more_accurate_than_the_minimal_solve():
    ratios = []
    for seed in range(6):
        x1, x2, Hg, inl = synth.planar_view(2275, seed=seed, noise_px=0.5, outlier_frac=0.3)
        key, Hr, m, c = R.run(x1, x2, 2000, 2.0, 0x5EED + seed)
        H, info = RR.refine(x1, x2, m, Hr, 10)
        assert info.status == 0 and info.cost_out < info.cost_in
        e0, e1 = _transfer(Hr, Hg, x1[inl]).mean(), _transfer(H, Hg, x1[inl]).mean()
        ratios.append(e0 / e1)
        assert e1 < 0.2, (seed, e0, e1)
    # this seed set: 5.2-8.4x (mean 7.2x) lower mean transfer error to H_gt than the winning 4-point solve
    # (0.37-0.65 px -> 0.05-0.11 px)
    assert min(ratios) > 3.0 and np.mean(ratios) > 5.0, ratios


def test_degenerate_paths():
    x1, x2, Hg, inl = synth.planar_view(600, seed=9, noise_px=0.5, outlier_frac=0.2)
    key, Hr, m, c = R.run(x1, x2, 500, 2.0, 9)
    # fewer than 4 inliers: H_in kept bit for bit
    few = np.zeros(600, np.uint8)
    few[[5, 77, 500]] = 1
    H, info = RR.refine(x1, x2, few, Hr, 10)
    assert info.status == 1 and info.n_used == 3 and info.iters == 0
    assert (H.view(np.uint64) == Hr.view(np.uint64)).all() and info.cost_out == info.cost_in > 0
    # no inliers at all
    H, info = RR.refine(x1, x2, np.zeros(600, np.uint8), Hr, 10)
    assert info.as_tuple() == (0.0, 0.0, 0, 0, 1) and (H == Hr).all()
    # a zero H (RANSAC found no model): status 2, H stays zero
    H, info = RR.refine(x1, x2, m, np.zeros((3, 3)), 10)
    assert info.as_tuple() == (0.0, 0.0, 0, 0, 2) and not H.any()
    # all inliers collinear in image 1: the refit is rank-deficient and may not beat H_in, but nothing breaks
    xs = np.linspace(10, 900, 200)
    c1 = np.column_stack([xs, 0.5 * xs + 20]).astype(np.float32)
    p = np.column_stack([c1, np.ones(200)]) @ Hg.T
    c2 = (p[:, :2] / p[:, 2:3]).astype(np.float32)
    for it in (0, 10):
        H, info = RR.refine(c1, c2, np.ones(200, np.uint8), Hg, it)
        assert info.n_used == 200 and info.cost_out <= info.cost_in and np.isfinite(H).all()
    # every inlier on one point: no Hartley normalisation, so no refit; with H_in[8] = 0, no LM either
    d1, d2 = x1.copy(), x2.copy()
    d1[:8], d2[:8] = d1[0], d2[0]
    one = np.zeros(600, np.uint8)
    one[:8] = 1
    H0 = np.array([[1.0, 0, 0], [0, 1.0, 0], [1e-3, 1e-3, 0.0]])
    H0 /= np.linalg.norm(H0)
    H, info = RR.refine(d1, d2, one, H0, 10)
    assert info.status == 1 and info.n_used == 8 and info.iters == 0 and (H == H0).all()


def test_max_iters_bounds_the_lm_passes():
    x1, x2, _, _ = synth.planar_view(1500, seed=12, noise_px=0.8, outlier_frac=0.3)
    key, Hr, m, c = R.run(x1, x2, 1000, 2.0, 12)
    costs = []
    for it in (0, 1, 2, 5, 10, 30):
        H, info = RR.refine(x1, x2, m, Hr, it)
        assert info.iters <= it
        costs.append(info.cost_out)
    assert all(b <= a for a, b in zip(costs, costs[1:])), costs      # more iterations never end higher
    assert costs[-1] < costs[0]


def test_library_rejects_bad_arguments_without_a_device():
    L = api.lib()
    xy = np.zeros((10, 2), np.float32)
    m = np.ones(10, np.uint8)
    H = np.eye(3).reshape(9).copy()
    Ho = np.zeros(9)

    def host(n=10, mask=m, it=10, Hin=H):
        return L.pm_homography_refine(None, api._p(xy), api._p(xy), n, api._p(mask), api._p(Hin), it, api._p(Ho), None)

    assert host(it=-1) == api.PM_E_INVALID and host(it=101) == api.PM_E_INVALID
    assert b"max_iters" in L.pm_last_error()
    assert host(mask=None) == api.PM_E_INVALID
    assert host(n=-1) == api.PM_E_INVALID
    assert host(n=3) == api.PM_E_TOO_FEW and (Ho == H).all()       # H_out = H_in
    assert host(Hin=None) == api.PM_E_INVALID
    assert host() == api.PM_E_INVALID and b"ctx" in L.pm_last_error()
    view = api.PointsView(1, 1, None, 1, 10, 0, 1, 0)
    d = C.c_void_p(16)                                           # never dereferenced: the calls fail before any launch
    assert L.pm_homography_refine_dev(None, C.byref(view), d, d, 10, d, None) == api.PM_E_INVALID
    assert L.pm_homography_refine_dev(None, C.byref(view), None, d, 10, d, d) == api.PM_E_INVALID
    assert L.pm_homography_refine_dev(None, None, d, d, 10, d, d) == api.PM_E_INVALID
    assert L.pm_homography_refine_dev(None, C.byref(view), d, d, 200, d, d) == api.PM_E_INVALID
    good = api.RansacParams(0, 10, 1, 2.0, api.PM_ERR_REPROJ)
    bad = api.RansacParams(0, 10, 1, 2.0, api.PM_ERR_SAMPSON)
    key, ninl = C.c_uint64(), C.c_int()
    info = api.HRefineInfo()

    def refined(prm=good, n=10, it=10):
        return L.pm_ransac_homography_refined(None, api._p(xy), api._p(xy), n, C.byref(prm), it, api._p(Ho), None,
                                              C.byref(ninl), C.byref(key), C.byref(info))

    assert refined(prm=bad) == api.PM_E_INVALID
    assert refined(it=-1) == api.PM_E_INVALID
    assert refined(n=3) == api.PM_E_TOO_FEW
    assert refined() == api.PM_E_INVALID and b"ctx" in L.pm_last_error()
    assert C.sizeof(api.HRefineInfo) == 32 == api.H_REFINE_INFO_DTYPE.itemsize
