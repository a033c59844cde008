"""CPU: 3-D to 3-D alignment (docs/SPEC.md S97-S101) through its plain-C restatement tests/align3d_ref.c — the minimal
triad solve on planted and degenerate samples, the Horn / Umeyama refit against an independent numpy statement (SVD Kabsch
with the reflection fix, float64), the refit's behaviour, the point transform — and the C ABI surface of libpm_hip.so: the
prototypes, the exports and every refusal that needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align3d_ref as R
from backend_cases import np_fit            # SVD Kabsch / Umeyama with the reflection fix, float64
from points_matching_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = 2.0 ** -52
MODELS = (R.RIGID, R.SIMILARITY)
NAMES = ("pm_ransac_align3d", "pm_ransac_align3d_from_hyp", "pm_ransac_align3d_run_dev", "pm_align3d_refine",
         "pm_align3d_refine_dev", "pm_estimate_align3d", "pm_transform_points3_dev", "pm_transform_points3",
         "pm_gather_align3d_dev")
ARITY = dict(zip(NAMES, (10, 10, 9, 9, 7, 12, 6, 5, 10)))


def _rot_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def _apply(T, x):
    s, Rm, t = R.unpack(T)
    return s * np.asarray(x, np.float64) @ Rm.T + t


# -- S97, S98: sample and minimal solve -------------------------------------------------------------------------------------
def test_sample_is_three_distinct_indices_and_a_pure_function():
    for n in (3, 4, 5, 100, 32768):
        seen = set()
        for h in list(range(200)) + [(1 << 32) - 1]:
            idx = R.sample(0x5EED, h, n)
            assert len(set(idx.tolist())) == 3 and idx.min() >= 0 and idx.max() < n
            assert (R.sample(0x5EED, h, n) == idx).all()
            seen.update(idx.tolist())
        assert n > 5 or seen == set(range(n))
    assert any((R.sample(1, h, 100) != R.sample(2, h, 100)).any() for h in range(8))


@pytest.mark.parametrize("model", MODELS)
def test_minimal_solve_recovers_a_planted_transform(model):
    # noise-free rows are exact in fp64 only up to their float32 rounding (2^-24 relative, coordinates below 16), which
    # a triad of side ~ 1 turns into an angle of a few 1e-6 rad: the bounds below are 100x that
    worst = 0.0
    for seed in range(20):
        x1, x2, s, Rg, tg, _ = synth.align3d_scene(200, seed=seed, model=model, outlier_frac=0.0, noise=0.0)
        for h in range(20):
            idx = R.sample(seed, h, 200)
            a = x1[idx].astype(np.float64)
            if np.linalg.norm(np.cross(a[1] - a[0], a[2] - a[0])) < 1.0:
                continue                                  # a thin triangle amplifies the rounding: not what is checked here
            T, ok = R.solve(model, x1[idx], x2[idx])
            assert ok
            sm, Rm, tm = R.unpack(T)
            assert _rot_deg(Rm, Rg) < 0.02 and abs(sm / s - 1.0) < 1e-4 and np.linalg.norm(tm - tg) < 5e-3
            assert (sm == 1.0) if model == R.RIGID else True
            worst = max(worst, _rot_deg(Rm, Rg))
    assert worst > 0.0


@pytest.mark.parametrize("model", MODELS)
def test_minimal_solve_gives_a_rotation_on_noisy_samples(model):
    # R = T2^T T1 of two triads orthonormal to a few ulp each: |R^T R - I| and |det R - 1| stay below 32 eps
    for seed in range(10):
        x1, x2, *_ = synth.align3d_scene(100, seed=seed, model=model, outlier_frac=0.5, noise=0.05)
        for h in range(50):
            T, ok = R.candidate(model, x1, x2, seed, h)
            assert ok
            s, Rm, _ = R.unpack(T)
            assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 32 * EPS64
            assert abs(np.linalg.det(Rm) - 1.0) <= 32 * EPS64
            assert s == 1.0 if model == R.RIGID else s > 0.0


@pytest.mark.parametrize("model", MODELS)
def test_degenerate_samples_are_invalid(model):
    a = np.array([[0, 0, 5], [1, 0, 5], [0, 1, 6]], np.float32)
    b = a + np.float32(1.0)
    assert R.solve(model, a, b)[1]
    for side in range(2):
        for bad in (np.array([[0, 0, 5], [0, 0, 5], [0, 1, 6]], np.float32),          # two points coincide
                    np.array([[0, 0, 5], [0, 1, 6], [0, 0, 5]], np.float32),
                    np.array([[0, 0, 5], [1, 1, 6], [2, 2, 7]], np.float32),          # collinear
                    np.array([[0, 0, 5], [1, np.nan, 5], [0, 1, 6]], np.float32),     # not finite
                    np.array([[0, 0, 5], [1, 0, 5], [0, np.inf, 6]], np.float32)):
            T, ok = R.solve(model, bad if side == 0 else a, b if side == 0 else bad)
            assert not ok and not T.any()
    x1 = np.tile(a[:1], (10, 1))
    assert not R.candidate(model, x1, x1, 1, 0)[1]
    assert not R.candidate(model, a[:2], b[:2], 1, 0)[1]                              # n < 3


# -- S99, S100 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_nan_rows_are_never_inliers_and_change_no_other_verdict(model):
    x1, x2, s, Rg, tg, inl = synth.align3d_scene(500, seed=3, model=model, outlier_frac=0.3, noise=0.01)
    T = R.pack(s, Rg, tg)
    m0, c0 = R.score(T, x1, x2, 0.1)
    assert c0 >= 0.99 * inl.sum()
    y1, y2 = x1.copy(), x2.copy()
    y1[::7, 1] = np.nan
    y2[3::11, 0] = np.inf
    y1[5::13, 2] = -np.inf
    bad = ~(np.isfinite(y1).all(axis=1) & np.isfinite(y2).all(axis=1))
    m1, c1 = R.score(T, y1, y2, 0.1)
    assert not m1[bad].any() and (m1[~bad] == m0[~bad]).all() and c1 == m1.sum()
    assert not R.score(T, y1, y2, 1e30)[0][bad].any()          # thr^2 overflows to +inf in fp32: still no inlier


def test_three_inliers_among_500_rows_is_deterministic():
    # 3 true correspondences among 500 rows: a sample hits them with probability ~5e-8, so 2000 samples will not; the
    # restatement still defines the outcome (most inliers, then lowest id), and defines it the same way every time
    x1, x2, *_ = synth.align3d_scene(500, seed=77, outlier_frac=0.994, noise=0.001)
    first = R.run(R.RIGID, x1, x2, 2000, 0.05, 5)
    again = R.run(R.RIGID, x1, x2, 2000, 0.05, 5)
    assert first[0] == again[0] and (first[1] == again[1]).all() and (first[2] == again[2]).all() and first[0] != 0


# -- S101 against numpy ---------------------------------------------------------------------------------------------------------
def _fit_scenes():
    """(name, model, xyz1, xyz2, mask): clean, noisy and near-planar inlier sets, offsets from the origin included."""
    out = []
    for model in MODELS:
        for seed in range(4):
            for name, noise in (("clean", 0.0), ("noisy", 0.05)):
                x1, x2, _, _, _, inl = synth.align3d_scene(800, seed=seed, model=model, outlier_frac=0.3, noise=noise)
                out.append((name, model, x1, x2, inl.astype(np.uint8)))
            x1, x2, s, Rg, tg, inl = synth.align3d_scene(800, seed=50 + seed, model=model, outlier_frac=0.0, noise=0.0)
            flat = x1.astype(np.float64)
            flat[:, 2] = 8.0 + 1e-3 * (flat[:, 2] - 8.0)              # a slab 4e-3 thick, 8 x 8 wide
            rng = np.random.default_rng(seed)
            y2 = s * flat @ Rg.T + tg + rng.normal(0, 1e-3, flat.shape)
            out.append(("planar", model, flat.astype(np.float32), y2.astype(np.float32), np.ones(800, np.uint8)))
    return out


# Predicted positions of S101's refit against numpy's SVD fit.  Both solve the same problem; each carries a few eps * cond
# of the rotation, with cond = s1 / (s2 + s3) of the cross-moment matrix's singular values (the eigenvalue gap of Horn's
# matrix is 2 (s2 + s3) against a top eigenvalue s1 + s2 + s3), times the extent of the data.  Measured worst over the
# scenes of _fit_scenes(), diff / (eps * cond * |x2|max): 14.2 (the 800-term sums on both sides are part of it) -- FIT_K is
# 18x above it, since a condition-number estimate is loose by such factors.
FIT_K = 256.0


def test_refit_against_numpy_kabsch_umeyama():
    worst = 0.0
    for name, model, x1, x2, mask in _fit_scenes():
        sel = mask.astype(bool)
        start, _ = np_fit(model, x1[sel][:3], x2[sel][:3])             # any start: the refit does not depend on it
        T, info = R.refine(model, x1, x2, mask, start)
        assert info.status == 0 and info.n_used == sel.sum(), name
        ref, S = np_fit(model, x1[sel], x2[sel])
        cond = S[0] / (S[1] + S[2])
        scale = np.abs(x2[sel]).max()
        diff = np.abs(_apply(T, x1[sel]) - _apply(ref, x1[sel])).max()
        print("%-7s model %d  cond %9.3g  diff / (eps cond scale) %.3g" % (name, model, cond, diff / (EPS64 * cond * scale)))
        assert diff <= FIT_K * EPS64 * cond * scale, (name, model, diff, cond)
        worst = max(worst, diff / (EPS64 * cond * scale))
        s, Rm, _ = R.unpack(T)
        assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 32 * EPS64 and abs(np.linalg.det(Rm) - 1.0) <= 32 * EPS64
        assert (s == 1.0) if model == R.RIGID else s > 0.0
    print("worst ratio %.3g" % worst)


# -- S101: behaviour -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_refit_never_raises_the_cost_and_is_idempotent(model):
    for seed in range(6):
        x1, x2, s, Rg, tg, inl = synth.align3d_scene(600, seed=seed, model=model, outlier_frac=0.4, noise=0.02, nan_frac=0.05)
        key, T0, mask, c = R.run(model, x1, x2, 300, 0.1, 9)
        assert key
        for start in (T0, R.pack(s, Rg, tg), R.pack(1.0, np.eye(3), np.zeros(3))):
            for m in (mask, inl.astype(np.uint8), np.ones(600, np.uint8)):
                T1, i1 = R.refine(model, x1, x2, m, start)
                assert i1.cost_out <= i1.cost_in and i1.iters == 0 and i1.status in (0, 1)
                usable = m.astype(bool) & np.isfinite(x1).all(axis=1) & np.isfinite(x2).all(axis=1)
                assert i1.n_used == usable.sum()
                if i1.status == 1:
                    assert (T1.view(np.uint64) == np.asarray(start).view(np.uint64)).all()
                T2, i2 = R.refine(model, x1, x2, m, T1)
                # the second refit sees the same moments: it returns the same model, or keeps its input when rounding
                # puts its cost a hair above
                assert np.abs(T2 - T1).max() <= 64 * EPS64 * max(1.0, np.abs(T1).max())
                assert i2.cost_out <= i2.cost_in


@pytest.mark.parametrize("model", MODELS)
def test_refit_keeps_the_input_when_the_rotation_is_not_determined(model):
    # rows k * (1, 2, -1) + (3, 0, 5) with integer k are EXACTLY collinear in float32, and so is their image under a
    # quarter turn about z, a doubling and an integer shift
    k = np.arange(40, dtype=np.float64)[:, None]
    a = k * np.array([1.0, 2.0, -1.0]) + np.array([3.0, 0.0, 5.0])
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    s = 2.0 if model == R.SIMILARITY else 1.0
    b = s * a @ Rz.T + np.array([1.0, -2.0, 4.0])
    start = R.pack(s, _rodrigues_x(0.3) @ Rz, np.array([0.5, 0.5, 0.5]))
    ones = np.ones(40, np.uint8)
    T, info = R.refine(model, a, b, ones, start)
    assert info.status == 1 and info.n_used == 40 and info.cost_out == info.cost_in
    assert (T.view(np.uint64) == start.view(np.uint64)).all()
    same = np.tile(a[:1], (40, 1))                                     # coincident rows
    T, info = R.refine(model, same, same, ones, start)
    assert info.status == 1 and (T.view(np.uint64) == start.view(np.uint64)).all()
    two = np.zeros(40, np.uint8)                                       # fewer than 3 usable inliers
    two[[3, 9]] = 1
    x1, x2, *_ = synth.align3d_scene(40, seed=1, model=model, outlier_frac=0.0)
    T, info = R.refine(model, x1, x2, two, start)
    assert info.status == 1 and info.n_used == 2 and (T.view(np.uint64) == start.view(np.uint64)).all()
    x1[[3, 9, 12]] = np.nan                                            # NaN rows are not usable
    two[12] = 1
    T, info = R.refine(model, x1, x2, two, start)
    assert info.status == 1 and info.n_used == 0
    T, info = R.refine(model, a, b, ones, np.zeros(13))                # the zero model
    assert info.status == 2 and not T.any() and info.n_used == 0


def _rodrigues_x(th):
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(th), -np.sin(th)], [0.0, np.sin(th), np.cos(th)]])


def test_jacobi_eigenvalues_match_lapack():
    # ten sweeps are past convergence on a 4 x 4 symmetric matrix: eigenvalues agree with LAPACK to a few eps * |N|
    rng = np.random.default_rng(4)
    for _ in range(50):
        S = rng.normal(size=9) * 10.0 ** rng.uniform(-3, 3)
        _, _, eig = R.horn(R.RIGID, np.r_[S, 1.0, 1.0], 1.0, np.zeros(3), np.zeros(3))
        Sxx, Syx, Szx, Sxy, Syy, Szy, Sxz, Syz, Szz = S
        N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx], [0, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                      [0, 0, -Sxx + Syy - Szz, Syz + Szy], [0, 0, 0, -Sxx - Syy + Szz]])
        N = N + np.triu(N, 1).T
        assert np.abs(np.sort(eig) - np.linalg.eigvalsh(N)).max() <= 32 * EPS64 * np.abs(N).max()


# -- the point transform -------------------------------------------------------------------------------------------------------
def test_transform_equals_numpy_fp64_after_one_rounding():
    rng = np.random.default_rng(8)
    x = rng.uniform(-50, 50, (2000, 3)).astype(np.float32)
    x[5] = np.nan
    x[17, 1] = np.inf
    for model in MODELS:
        _, _, s, Rg, tg, _ = synth.align3d_scene(3, seed=2, model=model)
        T = R.pack(s, Rg, tg)
        out = R.transform(T, x)
        M = s * Rg                                                     # the same products, each rounded once
        xd = x.astype(np.float64)
        ref = ((M[:, 0] * xd[:, :1] + M[:, 1] * xd[:, 1:2]) + M[:, 2] * xd[:, 2:3]) + tg
        ok = np.isfinite(x).all(axis=1)
        assert (out[ok] == ref[ok].astype(np.float32)).all()
        assert np.isnan(out[~ok]).all() and (~ok).sum() == 2
        assert (out[~ok].view(np.uint32) == 0x7FC00000).all()
        y = x.copy()
        R.lib().ar_transform(R._p(T), R._p(y), 2000, R._p(y))          # in place
        assert (y.view(np.uint32) == out.view(np.uint32)).all()


# -- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_exports():
    hdr = open(os.path.join(ROOT, "include", "pm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = api.lib()
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == ARITY[name], name
        assert name in api.EXPORTS and hasattr(L, name)
    assert "PM_ALIGN3D_RIGID = 0, PM_ALIGN3D_SIMILARITY = 1" in code
    assert (api.PM_ALIGN3D_RIGID, api.PM_ALIGN3D_SIMILARITY) == (0, 1)
    assert C.sizeof(api.XyzView) == 32


def test_every_refusal_without_a_device():
    L = api.lib()
    INV, FEW = api.PM_E_INVALID, api.PM_E_TOO_FEW
    ref = lambda s: C.byref(s) if s is not None else None
    x1, x2, *_ = synth.align3d_scene(10, seed=1)
    T, mask = np.zeros(13), np.zeros(10, np.uint8)
    ninl, key, info = C.c_int(), C.c_uint64(), api.HRefineInfo()
    good = api.RansacParams(0, 10, 1, 0.1, api.PM_ERR_REPROJ)
    empty = api.RansacParams(5, 5, 1, 0.1, api.PM_ERR_REPROJ)
    top = api.RansacParams(0, (1 << 32) + 1, 1, 0.1, api.PM_ERR_REPROJ)
    wide = api.RansacParams(0, 1 << 32, 1, 0.1, api.PM_ERR_REPROJ)
    kind = api.RansacParams(0, 10, 1, 0.1, api.PM_ERR_SAMPSON)
    thr0 = api.RansacParams(0, 10, 1, 0.0, api.PM_ERR_REPROJ)
    thrinf = api.RansacParams(0, 10, 1, float("inf"), api.PM_ERR_REPROJ)
    thrnan = api.RansacParams(0, 10, 1, float("nan"), api.PM_ERR_REPROJ)

    def refused(rc, status, msg):
        return rc == status and msg in L.pm_last_error()

    def poison(n=10):
        T[:] = 7.0
        mask[:] = 7
        ninl.value, key.value = 7, 7
        info.status, info.n_used, info.cost_in = 7, 7, 7.0

    def zeroed(with_info=False, n=10):
        return (not T.any() and not mask[:n].any() and ninl.value == 0 and key.value == 0 and
                (not with_info or (info.status == 2 and info.n_used == 0)))

    # ---- pm_ransac_align3d / pm_estimate_align3d: model, params, threshold, arrays, n, ctx; outputs reset on refusal
    def run(model=0, prm=good, n=10, pts=True, t=T, est=False):
        poison()
        a, b = (api._p(x1), api._p(x2)) if pts else (None, None)
        if est:
            return L.pm_estimate_align3d(None, model, a, b, n, ref(prm), 1, api._p(t), api._p(mask), C.byref(ninl), C.byref(key),
                                         C.byref(info))
        return L.pm_ransac_align3d(None, model, a, b, n, ref(prm), api._p(t), api._p(mask), C.byref(ninl), C.byref(key))

    for est in (False, True):
        assert refused(run(model=2, est=est), INV, b"PM_ALIGN3D_") and refused(run(model=-1, est=est), INV, b"PM_ALIGN3D_")
        assert zeroed(est)
        assert refused(run(prm=None, est=est), INV, b"params is null") and zeroed(est)
        assert refused(run(prm=empty, est=est), INV, b"sample ids must") and refused(run(prm=top, est=est), INV, b"sample ids must")
        assert refused(run(prm=wide, est=est), INV, b"split the range")
        assert refused(run(prm=kind, est=est), INV, b"error_kind") and zeroed(est)
        for bad in (thr0, thrinf, thrnan):
            assert refused(run(prm=bad, est=est), INV, b"thresh_px") and zeroed(est)
        assert refused(run(pts=False, est=est), INV, b"bad point arrays") and refused(run(n=-1, est=est), INV, b"bad point arrays")
        for n in (0, 2):
            assert refused(run(n=n, est=est), FEW, b"need at least 3") and zeroed(est, n)
        assert refused(run(t=None, est=est), INV, b"null T") and not mask.any() and ninl.value == 0 and key.value == 0
        assert refused(run(model=1, n=3, est=est), INV, b"ctx is null") and zeroed(est, 3)

    # ---- pm_ransac_align3d_from_hyp: the id, then as above (p's own range is ignored)
    def hyp(h=0, model=0, prm=good, n=10, t=T):
        poison()
        return L.pm_ransac_align3d_from_hyp(None, model, api._p(x1), api._p(x2), n, ref(prm), C.c_int64(h), api._p(t),
                                            api._p(mask), C.byref(ninl))

    assert refused(hyp(h=-1), INV, b"hypothesis id") and refused(hyp(h=1 << 32), INV, b"hypothesis id") and not T.any()
    assert refused(hyp(prm=None), INV, b"params is null") and refused(hyp(model=5), INV, b"PM_ALIGN3D_")
    assert refused(hyp(prm=thr0), INV, b"thresh_px") and refused(hyp(prm=kind), INV, b"error_kind")
    assert refused(hyp(n=2), FEW, b"need at least 3") and refused(hyp(t=None), INV, b"null T")
    assert refused(hyp(h=(1 << 32) - 1, prm=empty), INV, b"ctx is null") and not T.any() and ninl.value == 0

    # ---- pm_ransac_align3d_run_dev: outputs, mask_len, model, params, view, ctx
    view = api.XyzView(1, 1, None, 10, 0)
    d = C.c_void_p(16)                                           # never dereferenced: the calls fail before any launch

    def dev(v=view, model=0, prm=good, outs=(d, d, d, d), mask_len=10):
        return L.pm_ransac_align3d_run_dev(None, model, ref(v), ref(prm), outs[0], outs[1], outs[2], mask_len, outs[3])

    for i in range(4):
        assert refused(dev(outs=tuple(None if j == i else d for j in range(4))), INV, b"null argument")
    assert refused(dev(mask_len=-1), INV, b"mask_len") and refused(dev(model=2), INV, b"PM_ALIGN3D_")
    assert refused(dev(prm=None), INV, b"params is null") and refused(dev(prm=empty), INV, b"sample ids must")
    assert refused(dev(prm=kind), INV, b"error_kind") and refused(dev(prm=thr0), INV, b"thresh_px")
    for v in (None, api.XyzView(None, 1, None, 10, 0), api.XyzView(1, None, None, 10, 0), api.XyzView(1, 1, None, 0, 0)):
        assert refused(dev(v=v), INV, b"need a view")
    assert refused(dev(), INV, b"ctx is null") and refused(dev(mask_len=0, model=1), INV, b"ctx is null")

    # ---- pm_align3d_refine: T_in / T_out before everything (nothing written), then model, arrays, n, ctx
    Tin = R.pack(1.0, np.eye(3), np.array([1.0, 2.0, 3.0]))

    def refine(model=0, mi=mask, t_in=Tin, t_out=T, n=10, pts=True):
        poison()
        a, b = (api._p(x1), api._p(x2)) if pts else (None, None)
        return L.pm_align3d_refine(None, model, a, b, n, api._p(mi), api._p(t_in), api._p(t_out), C.byref(info))

    def passed_through():
        return (T == Tin).all() and info.status == 1 and info.n_used == 0 and info.cost_in == 0.0

    for kw in ({"t_in": None}, {"t_out": None}):
        assert refused(refine(**kw), INV, b"null T") and info.status == 7 and (T == 7.0).all()
    assert refused(refine(model=3), INV, b"PM_ALIGN3D_") and passed_through()
    assert refused(refine(mi=None), INV, b"bad point or mask arrays") and passed_through()
    assert refused(refine(pts=False), INV, b"bad point or mask arrays") and refused(refine(n=-1), INV, b"bad point or mask")
    assert refused(refine(n=2), FEW, b"need at least 3") and passed_through()
    assert refused(refine(n=3), INV, b"ctx is null") and passed_through()

    # ---- pm_align3d_refine_dev: pointers (info optional), model, view, ctx
    def refd(v=view, model=0, args=(d, d, d), inf=None):
        return L.pm_align3d_refine_dev(None, model, ref(v), args[0], args[1], args[2], inf)

    for i in range(3):
        assert refused(refd(args=tuple(None if j == i else d for j in range(3))), INV, b"null argument")
    assert refused(refd(model=2), INV, b"PM_ALIGN3D_")
    assert refused(refd(v=None), INV, b"need a view") and refused(refd(v=api.XyzView(1, 1, None, 0, 0)), INV, b"need a view")
    assert refused(refd(), INV, b"ctx is null") and refused(refd(inf=d, model=1), INV, b"ctx is null")

    # ---- pm_transform_points3[_dev]: ctx first, as pm_transform_points; with a context the pointer and size checks
    assert refused(L.pm_transform_points3_dev(None, d, d, None, 10, d), INV, b"ctx is null")
    assert refused(L.pm_transform_points3(None, api._p(Tin), api._p(x1), 10, api._p(x1)), INV, b"ctx is null")

    # ---- pm_gather_align3d_dev: pointers (the count is optional), sizes, ctx
    def gather(args=(d, d, d, d, d, d), cap=10, n1=5, n2=5):
        mt, cnt, t1, t2, o1, o2 = args
        return L.pm_gather_align3d_dev(None, mt, cnt, cap, t1, n1, t2, n2, o1, o2)

    for i in (0, 2, 3, 4, 5):
        assert refused(gather(args=tuple(None if j == i else d for j in range(6))), INV, b"null argument")
    assert refused(gather(cap=0), INV, b"need cap >= 1")
    assert refused(gather(n1=-1), INV, b"need cap >= 1") and refused(gather(n2=-1), INV, b"need cap >= 1")
    assert refused(gather(args=(d, None, d, d, d, d), n1=0, n2=0), INV, b"ctx is null")
    assert refused(gather(), INV, b"ctx is null")
