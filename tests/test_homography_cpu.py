"""CPU: the restatement of docs/SPEC.md S19-S22 (tests/homography_ref.c) — robust homography — checked against the
SPEC's stream definitions and an INDEPENDENT algorithm (numpy's SVD-based normalised DLT), plus the argument checks of
the shipped entry points, which need no device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import homography_ref as R
from points_matching_amd import api, synth

M64 = (1 << 64) - 1


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def walk(seed, h, n, k, const):
    """S6's walk with k accepted indices on the stream keyed by `const` (S6: 0x9E37..., S13: 0x7F4A..., S19: 0x4A7C...)."""
    stream = mix64((seed ^ const) & M64) ^ mix64((h + 0xD1B54A32D192ED03) & M64)
    out = []
    for d in range(64):
        if len(out) == k:
            break
        c = ((mix64((stream + (d + 1) * 0x9E3779B97F4A7C15) & M64) >> 32) * n) >> 32
        if c not in out:
            out.append(c)
    c = 0
    while len(out) < k:
        if c not in out:
            out.append(c)
        c += 1
    return out


S6, S13, S19 = 0x9E3779B97F4A7C15, 0x7F4A7C159E3779B9, 0x4A7C159E3779B97F


def test_sampler_is_the_spec_walk_and_a_pure_function():
    rng = np.random.default_rng(19)
    for _ in range(400):
        seed, h, n = int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 32)), int(rng.integers(4, 5000))
        a = R.sample4(seed, h, n)
        assert list(a) == walk(seed, h, n, 4, S19)
        assert (R.sample4(seed, h, n) == a).all()
        assert len(set(a.tolist())) == 4 and a.min() >= 0 and a.max() < n
    for n in (4, 5, 6):                                # tiny n: the deterministic completion rule
        for h in range(200):
            a = R.sample4(7, h, n)
            assert sorted(a.tolist()) == sorted(set(a.tolist())) and a.max() < n
            assert list(a) == walk(7, h, n, 4, S19)


def test_sampler_stream_is_distinct_from_s6_and_s13():
    same6 = same13 = 0
    for h in range(2000):
        a = walk(0x5EED, h, 2275, 4, S19)
        same6 += a == walk(0x5EED, h, 2275, 8, S6)[:4]
        same13 += a == walk(0x5EED, h, 2275, 7, S13)[:4]
    assert same6 == 0 and same13 == 0


def np_dlt(p1, p2):
    """Textbook normalised 4-point DLT with numpy's LAPACK SVD.  x2 ~ H x1, unit Frobenius norm, H[2,2] >= 0."""
    def hartley(p):
        c = p.mean(axis=0)
        s = math.sqrt(2.0) / np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
        return (p - c) * s, np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    a, T1 = hartley(p1)
    b, T2 = hartley(p2)
    rows = []
    for (x, y), (u, v) in zip(a, b):
        rows.append([-x, -y, -1, 0, 0, 0, u * x, u * y, u])
        rows.append([0, 0, 0, -x, -y, -1, v * x, v * y, v])
    _, sv, Vt = np.linalg.svd(np.array(rows))
    H = np.linalg.inv(T2) @ Vt[-1].reshape(3, 3) @ T1
    H /= np.linalg.norm(H)
    return (-H if H[2, 2] < 0 else H), sv


def test_solver_agrees_with_numpy_svd_dlt_on_planar_data():
    worst, checked = 0.0, 0
    for seed in range(6):
        xy1, xy2, _, _ = synth.planar_view(400, seed=seed, outlier_frac=0.1, noise_px=0.5)
        for h in range(250):
            idx = R.sample4(0xABC, h, len(xy1))
            p1, p2 = xy1[idx].astype(np.float64), xy2[idx].astype(np.float64)
            ok, H = R.model(xy1, xy2, 0xABC, h)
            ok2, H2 = R.solve4(p1, p2)
            assert ok == ok2 and (H.view(np.uint64) == H2.view(np.uint64)).all()
            if not ok:
                continue
            H_np, sv = np_dlt(p1, p2)
            gap = sv[7] / sv[0]                        # the null vector is determined up to ~eps / gap
            if gap < 1e-5:
                continue
            err = min(np.linalg.norm(H - H_np), np.linalg.norm(H + H_np))
            assert err <= 5e-13 / gap + 1e-13, (seed, h, err, gap)
            assert abs(np.linalg.norm(H) - 1) < 1e-14 and H[2, 2] >= 0
            worst = max(worst, err)
            checked += 1
    assert checked >= 900                             # of 1500: samples with an outlier are often invalid
    assert worst < 1e-9


def test_planted_homography_is_recovered_from_clean_samples():
    xy1, xy2, H_gt, inl = synth.planar_view(300, seed=3, outlier_frac=0.0, noise_px=0.0)
    s, d = xy1.sum(axis=1), xy1[:, 0] - xy1[:, 1]
    idx = [s.argmin(), d.argmax(), s.argmax(), d.argmin()]          # four well-spread points
    ok, H = R.solve4(xy1[idx].astype(np.float64), xy2[idx].astype(np.float64))
    assert ok
    p = np.column_stack([xy1, np.ones(len(xy1))]) @ H.T
    assert np.abs(p[:, :2] / p[:, 2:3] - xy2).max() < 1e-2


def test_collinear_samples_are_invalid():
    rng = np.random.default_rng(5)
    for _ in range(200):
        p1 = rng.uniform(0, 900, (4, 2))
        p2 = rng.uniform(0, 600, (4, 2))
        k = rng.integers(0, 4)                         # make three points of one image collinear
        trip = [i for i in range(4) if i != k]
        t = rng.uniform(-1, 2)
        img = p1 if rng.integers(0, 2) else p2
        img[trip[2]] = img[trip[0]] + t * (img[trip[1]] - img[trip[0]])
        ok, H = R.solve4(p1.astype(np.float32).astype(np.float64), p2.astype(np.float32).astype(np.float64))
        assert not ok and not H.any()
    # every point on one line: no model at all
    x = np.linspace(10, 900, 50)
    line = np.column_stack([x, 0.5 * x + 3]).astype(np.float32)
    key, H, mask, c = R.run(line, line[::-1].copy(), 500, 2.0, 1)
    assert key == 0 and not H.any() and not mask.any() and c == 0


def test_orientation_flipped_samples_are_invalid_and_reflections_valid():
    sq = np.array([[0.0, 0.0], [100.0, 0.0], [100.0, 100.0], [0.0, 100.0]])
    ok, _ = R.solve4(sq, sq * 1.5 + 7)
    assert ok
    ok, _ = R.solve4(sq, sq[:, ::-1].copy())          # a mirror image: every triple flips, consistently
    assert ok
    crossed = sq[[0, 1, 3, 2]]                         # a "bow tie": two triples flip, two do not
    ok, H = R.solve4(sq, crossed)
    assert not ok and not H.any()


def test_inlier_test_matches_float64_reprojection_away_from_threshold():
    xy1, xy2, H_gt, _ = synth.planar_view(3000, seed=11, outlier_frac=0.3, noise_px=1.5)
    mask, c = R.score(H_gt, xy1, xy2, 2.0)
    p = np.column_stack([xy1, np.ones(len(xy1))]).astype(np.float64) @ H_gt.astype(np.float32).astype(np.float64).T
    e2 = ((p[:, :2] / p[:, 2:3] - xy2) ** 2).sum(axis=1)
    far = np.abs(e2 - 4.0) > 1e-3
    assert far.sum() > 2900
    assert (mask[far] == (e2[far] <= 4.0)).all() and c == mask.sum()
    # w == 0 is an outlier even when u = v = 0
    H0 = np.zeros((3, 3))
    m0, c0 = R.score(H0, xy1[:10], xy2[:10], 1e30)
    assert c0 == 0 and not m0.any()


def test_run_finds_the_planted_model():
    xy1, xy2, H_gt, inl = synth.planar_view(1000, seed=21, outlier_frac=0.3, noise_px=0.5)
    key, H, mask, c = R.run(xy1, xy2, 300, 2.0, 0x5EED)
    assert key and c == mask.sum() == api.ransac_key_inliers(key)
    assert (mask.astype(bool) & inl).sum() >= 0.9 * inl.sum() and (mask.astype(bool) & ~inl).sum() < 10


# ---- the shipped entry points reject bad arguments before they need a device -------------------------------------
def _call_host(n=10, kind=api.PM_ERR_REPROJ, xy=True, params=True, hb=0, he=100):
    xy1 = np.zeros((max(n, 1), 2), np.float32)
    prm = api.RansacParams(hb, he, 1, 2.0, kind)
    H = np.zeros(9)
    return api.lib().pm_ransac_homography(None, api._p(xy1) if xy else None, api._p(xy1) if xy else None, n,
                                          C.byref(prm) if params else None, api._p(H), None, None, None)


@pytest.mark.skipif(not os.path.exists(api.LIB_PATH), reason="libpm_hip.so not built")
def test_library_rejects_bad_arguments_without_a_device():
    L = api.lib()
    for s in ("pm_ransac_homography", "pm_ransac_homography_run_dev", "pm_ransac_homography_from_hyp"):
        assert hasattr(L, s), s
    assert _call_host(n=3) == api.PM_E_TOO_FEW
    assert _call_host(n=0) == api.PM_E_TOO_FEW
    assert _call_host(n=-1) == api.PM_E_INVALID
    assert _call_host(xy=False) == api.PM_E_INVALID
    assert _call_host(params=False) == api.PM_E_INVALID
    for kind in (api.PM_ERR_SAMPSON, api.PM_ERR_SYM_EPIPOLAR, 3, -1):
        assert _call_host(kind=kind) == api.PM_E_INVALID
        assert b"error_kind" in L.pm_last_error()
    assert _call_host(hb=5, he=5) == api.PM_E_INVALID            # empty range
    assert _call_host(hb=0, he=(1 << 32) + 1) == api.PM_E_INVALID
    assert _call_host() == api.PM_E_INVALID                      # all good but the null context
    assert b"ctx" in L.pm_last_error()
    # the F entry points keep refusing the new kind
    prm = api.RansacParams(0, 10, 1, 2.0, api.PM_ERR_REPROJ)
    xy = np.zeros((10, 2), np.float32)
    assert L.pm_ransac_fundamental(None, api._p(xy), api._p(xy), 10, C.byref(prm), None, None, None, None) == api.PM_E_INVALID
    # device form
    view = api.PointsView(1, 1, None, 1, 10, 0, 1, 0)
    good = api.RansacParams(0, 10, 1, 2.0, api.PM_ERR_REPROJ)
    bad = api.RansacParams(0, 10, 1, 2.0, api.PM_ERR_SAMPSON)
    d = C.c_void_p(16)                                           # never dereferenced: the calls fail before any launch
    assert L.pm_ransac_homography_run_dev(None, C.byref(view), C.byref(good), None, d, d, 10, d) == api.PM_E_INVALID
    assert L.pm_ransac_homography_run_dev(None, C.byref(view), C.byref(bad), d, d, d, 10, d) == api.PM_E_INVALID
    assert L.pm_ransac_homography_run_dev(None, None, C.byref(good), d, d, d, 10, d) == api.PM_E_INVALID
    assert L.pm_ransac_homography_run_dev(None, C.byref(view), C.byref(good), d, d, d, -1, d) == api.PM_E_INVALID
    # one hypothesis
    H = np.zeros(9)
    assert L.pm_ransac_homography_from_hyp(None, api._p(xy), api._p(xy), 10, C.byref(good), C.c_int64(-1), api._p(H),
                                           None, None) == api.PM_E_INVALID
    assert L.pm_ransac_homography_from_hyp(None, api._p(xy), api._p(xy), 3, C.byref(good), C.c_int64(0), api._p(H),
                                           None, None) == api.PM_E_TOO_FEW
    assert L.pm_ransac_homography_from_hyp(None, api._p(xy), api._p(xy), 10, C.byref(bad), C.c_int64(0), api._p(H),
                                           None, None) == api.PM_E_INVALID


def test_planar_view_is_consistent():
    xy1, xy2, H, inl = synth.planar_view(500, seed=4, outlier_frac=0.2, noise_px=0.0)
    assert xy1.dtype == xy2.dtype == np.float32 and xy1.shape == (500, 2)
    assert inl.sum() == 400 and abs(np.linalg.norm(H) - 1) < 1e-12 and H[2, 2] > 0
    p = np.column_stack([xy1[inl], np.ones(inl.sum())]) @ H.T
    assert np.abs(p[:, :2] / p[:, 2:3] - xy2[inl]).max() < 1e-3
    assert np.linalg.cond(H) < 1e7


def test_homography_wrappers_reject_mismatched_lengths_without_a_device():
    """The Python wrappers check the row counts before any call into the library (a shorter xy2 would be read past)."""
    ctx = api.Context.__new__(api.Context)            # no device: the check must come first
    ctx._h = C.c_void_p()
    xy1, xy2 = np.zeros((10, 2), np.float32), np.zeros((9, 2), np.float32)
    for call in (lambda: ctx.ransac_homography(xy1, xy2, 10, 2.0, 1),
                 lambda: ctx.ransac_homography_from_hyp(xy1, xy2, 0, 2.0, 1),
                 lambda: ctx.ransac_homography_refined(xy1, xy2, 10, 2.0, 1),
                 lambda: ctx.ransac_homography(xy2, xy1, 10, 2.0, 1),
                 lambda: ctx.homography_refine(xy1, xy2, np.ones(10, np.uint8), np.eye(3))):
        with pytest.raises(ValueError):
            call()
