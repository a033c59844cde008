"""The affine restatement (tests/affine_ref.c: SPEC S26-S30) against DIFFERENT algorithms at hard geometry
(synth.affine_view_wide: images up to 16000 px, any rotation, scale 0.25-4, anisotropy, shear, reflection, coordinates
offset by up to 1e5 px): numpy.linalg.solve on the minimal 6 x 6 / 4 x 4 systems, a numpy statement of the S27 sample
rule, float64 forward residuals for the S28 mask, numpy.linalg.lstsq, Umeyama's SVD closed form and scipy's MINPACK LM
for the S30 refit, and a numpy statement of the refit's relative-det rule.  The GPU suites compare the HIP kernels with
the restatement bit for bit, so these tests anchor that chain; the helpers here are shared with
tests/test_affine_independent_gpu.py, which checks the kernels against the same references directly."""
import ctypes as C

import numpy as np
import pytest

import affine_ref as R
from points_matching_amd import api, synth

FULL, PARTIAL = api.PM_AFFINE_FULL, api.PM_AFFINE_PARTIAL
MODELS = (FULL, PARTIAL)
FLT_EPS = 2.0 ** -23          # S27's collinearity constant, and twice the fp32 unit roundoff
EPS64 = 2.0 ** -52
DET_REL = 1e-12               # S30: the full refit needs det > DET_REL * (Sxx * Syy)

# (width, height, angle, scale, aniso, shear, reflect, offset, noise_px, outlier_frac); aniso, shear and reflect apply to
# the full model only.  None: drawn by the generator.  Mild (affine_view-like) to hard.
WIDE_CASES = [
    (1000, 660, 0.1, 1.0, 1.1, 0.05, False, (0, 0), 0.5, 0.3),
    (1000, 700, None, 0.25, None, None, False, (0, 0), 0.3, 0.3),
    (4000, 3000, None, 4.0, 3.0, 0.3, True, (0, 0), 0.7, 0.3),
    (4000, 3000, 3.1, None, None, -0.3, False, (2e4, 1e4), 0.7, 0.4),
    (8000, 6000, -1.6, 0.5, 2.0, None, True, (-5e4, 3e4), 0.5, 0.2),
    (16000, 12000, None, 2.0, None, None, False, (0, 0), 1.0, 0.3),
    (16000, 12000, None, None, 2.5, 0.2, True, (1e5, -6e4), 1.0, 0.3),
]


def wide_view(n, seed, case, model):
    W, H, ang, sc, k, sh, refl, off, noise, out = case
    if model == PARTIAL:
        k, sh, refl = 1.0, 0.0, False
    return synth.affine_view_wide(n, seed=seed, width=W, height=H, angle=ang, scale=sc, aniso=k, shear=sh,
                                  reflect=refl, offset=off, noise_px=noise, outlier_frac=out, partial=model == PARTIAL)


def thresh_for(case, A):
    """3.5 sigma of an inlier's forward residual: image-1 noise is magnified by up to the largest singular value."""
    s = np.linalg.svd(np.asarray(A)[:, :2], compute_uv=False)[0]
    return float(max(1.5, 3.5 * case[8] * np.sqrt(1.0 + s * s)))


def _bits_equal(a, b):
    return (np.asarray(a, np.float64).view(np.uint64) == np.asarray(b, np.float64).view(np.uint64)).all()


# ---- numpy statements of the same operations ---------------------------------------------------------------------
def minimal_system(model, p1, p2):
    """The minimal system of S27: 6 x 6 (full, unknowns a0..a5) or 4 x 4 (partial, unknowns a, b, tx, ty)."""
    M, r = [], []
    for (x, y), (u, v) in zip(p1, p2):
        if model == FULL:
            M += [[x, y, 1, 0, 0, 0], [0, 0, 0, x, y, 1]]
        else:
            M += [[x, -y, 1, 0], [y, x, 0, 1]]
        r += [u, v]
    return np.array(M, np.float64), np.array(r, np.float64)


def np_minimal(model, p1, p2):
    """(A by LAPACK, cond(M)).  A's error is a few eps * cond(M) relative to |A|; Cramer's rule on the differences
    (S27) is at least as accurate, so the two differ by that much at most."""
    M, r = minimal_system(model, p1, p2)
    s = np.linalg.solve(M, r)
    A = s.reshape(2, 3) if model == FULL else np.array([[s[0], -s[1], s[2]], [s[1], s[0], s[3]]])
    return A, np.linalg.cond(M)


def np_sample_rule(model, p1, p2):
    """S27's validity rule restated: (valid, clear).  Full: no collinear triple in EITHER image by FLT_EPSILON times the
    l1 spread; partial: the pair distinct in BOTH images; any non-finite coordinate is invalid.  clear: the full check
    is far from its threshold compared with the rounding of det, so rounding cannot flip the verdict."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    if not (np.isfinite(p1).all() and np.isfinite(p2).all()):
        return False, True
    if model == PARTIAL:
        return bool((p1[1] != p1[0]).any() and (p2[1] != p2[0]).any()), True
    valid, clear = True, True
    for p in (p1, p2):
        d1, d2 = p[1] - p[0], p[2] - p[0]
        prods = np.array([d1[0] * d2[1], d1[1] * d2[0]])
        det = prods[0] - prods[1]
        thr = FLT_EPS * np.abs(np.concatenate([d1, d2])).sum()
        valid &= bool(abs(det) > thr)
        clear &= bool(abs(abs(det) - thr) > 8 * EPS64 * np.abs(prods).sum() + 1e-9 * thr)
    return valid, clear


def residual64(A, xy1, xy2):
    """Forward residual distance ||x2 - A x1|| in float64 and the fp32 rounding band of S28 around it.

    S28 rounds u = fmaf(a0, x, fmaf(a1, y, a2)) twice: |err u| <= 2^-23 U, U = |a0 x| + |a1 y| + |a2| (first order; V
    alike), du = u - xp adds one rounding of |du|, and the squares and the sum a few 2^-24 of d^2.  So the verdict can
    differ from the exact one only when d lies within err = 2^-23 (U + V + |du| + |dv|) of thr, plus a few 2^-24 thr
    (thr2 itself is rounded to f32).  The band used is 4 err + 1e-3 thr."""
    A = np.asarray(A, np.float64).reshape(2, 3)
    x, y = xy1[:, 0].astype(np.float64), xy1[:, 1].astype(np.float64)
    xp, yp = xy2[:, 0].astype(np.float64), xy2[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        u = A[0, 0] * x + A[0, 1] * y + A[0, 2]
        v = A[1, 0] * x + A[1, 1] * y + A[1, 2]
        d = np.hypot(u - xp, v - yp)
        U = np.abs(A[0, 0] * x) + np.abs(A[0, 1] * y) + np.abs(A[0, 2])
        V = np.abs(A[1, 0] * x) + np.abs(A[1, 1] * y) + np.abs(A[1, 2])
        err = 4.0 * FLT_EPS * (U + V + np.abs(u - xp) + np.abs(v - yp))
    return d, err


def check_mask_vs_float64(A, xy1, xy2, thr, mask, what=""):
    """S28 verdicts of A32 = (float)A against float64 forward residuals of the same A32, outside the rounding band.
    Non-finite rows must be outliers.  Returns the number of points checked."""
    A32 = np.asarray(A, np.float64).astype(np.float32).astype(np.float64)
    d, err = residual64(A32, xy1, xy2)
    band = 1e-3 * thr + err
    m = np.asarray(mask).astype(bool)
    finite = np.isfinite(xy1).all(axis=1) & np.isfinite(xy2).all(axis=1)
    assert not m[~finite].any(), (what, "non-finite row is an inlier", np.nonzero(m & ~finite)[0][:5])
    ok = finite & np.isfinite(d) & np.isfinite(band) & (np.abs(d - thr) > band)
    bad = np.nonzero(ok & ((d <= thr) != m))[0]
    assert bad.size == 0, (what, bad[:5], d[bad[:5]], band[bad[:5]], m[bad[:5]])
    return int(ok.sum())


def lstsq_fit(model, p1, p2):
    """numpy.linalg.lstsq on the uncentred design matrix: (A, cond of the design matrix)."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    if model == FULL:
        M = np.column_stack([p1, np.ones(len(p1))])
        return np.linalg.lstsq(M, p2, rcond=None)[0].T, np.linalg.cond(M)
    M = np.zeros((2 * len(p1), 4))
    M[0::2] = np.column_stack([p1[:, 0], -p1[:, 1], np.ones(len(p1)), np.zeros(len(p1))])
    M[1::2] = np.column_stack([p1[:, 1], p1[:, 0], np.zeros(len(p1)), np.ones(len(p1))])
    s = np.linalg.lstsq(M, p2.reshape(-1), rcond=None)[0]
    return np.array([[s[0], -s[1], s[2]], [s[1], s[0], s[3]]]), np.linalg.cond(M)


def umeyama(p1, p2):
    """Umeyama's closed form (SVD of the cross-covariance) for the least-squares similarity x2 = c R x1 + t, R a rotation.
    {c R, c >= 0} is exactly {[a -b; b a]}, so its minimiser is S30's partial refit."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    m1, m2 = p1.mean(axis=0), p2.mean(axis=0)
    q1, q2 = p1 - m1, p2 - m2
    U, D, Vt = np.linalg.svd(q2.T @ q1 / len(p1))
    S = np.diag([1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    Rm = U @ S @ Vt
    c = np.trace(np.diag(D) @ S) / (q1 * q1).sum(axis=1).mean()
    return np.column_stack([c * Rm, m2 - c * Rm @ m1])


def positions(A, p1):
    return np.column_stack([np.asarray(p1, np.float64), np.ones(len(p1))]) @ np.asarray(A).reshape(2, 3).T


# Predicted positions of S30's refit against lstsq on the uncentred data: lstsq's error is a few eps * cond(M) * |x2|
# (cond grows as the offset squared over the spread); S30's centred normal equations are the more accurate of the two.
# Measured worst over WIDE_CASES, diff / (eps * cond * |x2|max): 0.14 (full), 4.3 (partial): 350x and 11x margins.
LSTSQ_K = 50.0
# The same against Umeyama with the centred data's cond and |x2 - mean| (SVD vs normal equations): measured 0.019, 26x.
UMEYAMA_K = 0.5
LM_REL = 1e-9                 # relative cost agreement with scipy's optimum
# Minimal solves against LAPACK, relative to |A|max: measured worst err / (eps * cond(M)) 0.0046 (full), 0.019
# (partial): 100x and 27x margins.
SOLVE_K = 0.5


def check_refit_vs_lstsq(model, xy1, xy2, mask, A, what=""):
    m = np.asarray(mask).astype(bool)
    p1, p2 = xy1[m].astype(np.float64), xy2[m].astype(np.float64)
    ref, cond = lstsq_fit(model, p1, p2)
    diff = np.abs(positions(A, p1) - positions(ref, p1)).max()
    tol = LSTSQ_K * EPS64 * cond * np.abs(p2).max()
    assert diff <= tol, (what, "lstsq", diff, tol)
    if model == PARTIAL:
        U = umeyama(p1, p2)
        q1 = p1 - p1.mean(axis=0)
        cond_c = np.linalg.cond(np.column_stack([q1, np.ones(len(q1))]))
        diff_u = np.abs(positions(A, p1) - positions(U, p1)).max()
        tol_u = UMEYAMA_K * EPS64 * (cond_c * np.abs(p2 - p2.mean(axis=0)).max() + np.abs(p2).max())
        assert diff_u <= tol_u, (what, "umeyama", diff_u, tol_u)
        assert A[0, 0] == A[1, 1] and A[0, 1] == -A[1, 0], what
    return diff / (EPS64 * cond * np.abs(p2).max())


def forward_cost(model, xy1, xy2, mask, A):
    m = np.asarray(mask).astype(bool)
    r = positions(A, xy1[m]) - xy2[m].astype(np.float64)
    return float((r * r).sum())


def scipy_minimum(model, xy1, xy2, mask, A_in):
    """MINPACK LM (scipy) on the forward residual from A_in, tight tolerances: the minimum cost."""
    from scipy.optimize import least_squares
    m = np.asarray(mask).astype(bool)
    p1, p2 = xy1[m].astype(np.float64), xy2[m].astype(np.float64)
    A_in = np.asarray(A_in, np.float64).reshape(2, 3)

    def unpack(z):
        if model == FULL:
            return z.reshape(2, 3)
        return np.array([[z[0], -z[1], z[2]], [z[1], z[0], z[3]]])
    z0 = A_in.reshape(6) if model == FULL else np.array([A_in[0, 0], A_in[1, 0], A_in[0, 2], A_in[1, 2]])
    r = least_squares(lambda z: (positions(unpack(z), p1) - p2).reshape(-1), z0, method="lm", x_scale="jac",
                      xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return 2.0 * r.cost


def check_refit_optimal(model, xy1, xy2, mask, A_in, cost_out, what=""):
    cs = scipy_minimum(model, xy1, xy2, mask, A_in)
    assert abs(cost_out - cs) <= LM_REL * cs + 1e-18, (what, cost_out, cs, cost_out / cs - 1)


def np_det_rule(p1):
    """S30's full-refit rule det > 1e-12 (Sxx Syy) restated with the SVD of the centred image-1 inliers:
    det = (s1 s2)^2.  (valid, clear); clear: the ratio is at least 5 % away from 1e-12."""
    q = np.asarray(p1, np.float64)
    q = q - q.mean(axis=0)
    s = np.linalg.svd(q, compute_uv=False)
    ratio = (s[0] * s[1]) ** 2 / ((q[:, 0] ** 2).sum() * (q[:, 1] ** 2).sum())
    return bool(ratio > DET_REL), bool(abs(ratio / DET_REL - 1.0) > 0.05), ratio


def strip_spread(ratio, width_px, angle=0.4):
    """The spread that puts a strip's det / (Sxx Syy) near ratio * 1e-12: for uniform spreads that quotient is
    (spread^2 / 3) / (L^2 / 12) / (cos^2 sin^2)."""
    return width_px * abs(np.sin(angle) * np.cos(angle)) * np.sqrt(ratio * DET_REL / 4.0)


def strip(n, seed, width_px, spread, angle=0.4, origin=(300.0, 200.0)):
    """Inliers in a thin strip: a `width_px` segment at `angle`, perpendicular spread `spread` px (f32 rounding adds
    about 2^-24 |x| of its own)."""
    rng = np.random.default_rng([seed, 0x57])
    t = rng.uniform(0, width_px, n)
    e = rng.uniform(-spread, spread, n)
    d, nrm = np.array([np.cos(angle), np.sin(angle)]), np.array([-np.sin(angle), np.cos(angle)])
    return (np.asarray(origin) + t[:, None] * d + e[:, None] * nrm).astype(np.float32)


NONFINITE = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, 1e-42, -0.0], np.float32)


def poisoned_rows(xy1, xy2, frac, seed, ids=()):
    """Copies of (xy1, xy2) with `frac` of the rows (and the rows `ids`) given one coordinate from NONFINITE (NaN, +-Inf,
    +-1e30, 3e38, a subnormal, -0.0), in either image.  Returns (a, b, poisoned rows, non-finite rows)."""
    rng = np.random.default_rng([seed, 0xBAD])
    a, b = xy1.copy(), xy2.copy()
    rows = np.unique(np.concatenate([rng.permutation(len(a))[:int(round(frac * len(a)))], np.asarray(ids, int)]))
    for j, r in enumerate(rows):
        c = rng.integers(4)
        (a if c < 2 else b)[r, c % 2] = NONFINITE[j % len(NONFINITE)]
    bad = np.zeros(len(a), bool)
    bad[rows] = True
    nonfin = ~(np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1))
    return a, b, bad, nonfin


# thresh_px edges: (thresh_px, admits anything).  thr2 = thresh_px^2 in f32: 2e19 overflows to inf, 1e-20 is subnormal.
THRESH_EDGES = [(0.0, False), (float("nan"), False), (float("inf"), False), (-float("inf"), False), (2e19, False),
                (-2.5, True), (1e-20, True), (1.8e19, True)]


# ---- the generator -----------------------------------------------------------------------------------------------
def test_affine_view_wide_geometry():
    for ci, case in enumerate(WIDE_CASES):
        for model in MODELS:
            xy1, xy2, A, inl = wide_view(3000, ci, case[:8] + (0.0, 0.25), model)
            assert xy1.shape == xy2.shape == (3000, 2) and xy1.dtype == xy2.dtype == np.float32 and inl.sum() == 2250
            W, H, off = case[0], case[1], case[7]
            assert (xy1.min(axis=0) >= np.array(off) - 1).all() and (xy1.max(axis=0) <= np.array(off) + [W, H] + 1).all()
            r = positions(A, xy1) - xy2
            d = np.hypot(r[:, 0], r[:, 1])
            assert d[inl].max() < 1e-4 * max(np.abs(xy2).max(), 1.0) and np.median(d[~inl]) > 10
            s = np.linalg.svd(A[:, :2], compute_uv=False)
            assert 0.25 * 0.99 <= np.sqrt(s[0] * s[1]) <= 4 * 1.01, (ci, s)
            if model == PARTIAL:
                assert abs(A[0, 0] - A[1, 1]) < 1e-15 * s[0] and abs(A[0, 1] + A[1, 0]) < 1e-15 * s[0]
            elif case[6]:
                assert np.linalg.det(A[:, :2]) < 0
            if model == FULL and case[4] is not None and case[4] >= 2:
                assert s[0] / s[1] > 1.5, (ci, s)
    a = synth.affine_view(50, seed=3)
    b = synth.affine_view(50, seed=3)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    with pytest.raises(ValueError):
        synth.affine_view_wide(10, partial=True, reflect=True)


# ---- S27 at hard geometry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("ci", range(len(WIDE_CASES)))
def test_restated_minimal_solve_matches_numpy(model, ci):
    case = WIDE_CASES[ci]
    xy1, xy2, _, _ = wide_view(400, 10 + ci, case, model)
    seed, checked, worst = 0x77 + ci, 0, 0.0
    for h in range(300):
        idx = R.sample(model, seed, h, 400)
        ok, A = R.model_of(model, xy1, xy2, seed, h)
        p1, p2 = xy1[idx].astype(np.float64), xy2[idx].astype(np.float64)
        valid, clear = np_sample_rule(model, p1, p2)
        if clear:
            assert ok == valid, (ci, h)
        if not ok:
            assert not A.any()
            continue
        An, cond = np_minimal(model, p1, p2)
        err = np.abs(A - An).max() / np.abs(An).max()
        assert err <= SOLVE_K * EPS64 * cond, (ci, h, err, cond)
        worst = max(worst, err / (EPS64 * cond))
        if model == PARTIAL:
            assert A[0, 0] == A[1, 1] and A[0, 1] == -A[1, 0]
        checked += 1
    assert checked >= 280, checked


@pytest.mark.parametrize("model", MODELS)
def test_restated_sample_rule_matches_numpy_statement(model):
    """Random, planted-degenerate (in image 1 only, image 2 only, both), coincident and NaN samples."""
    rng = np.random.default_rng(27 + model)
    k = R.min_pts(model)
    counts = dict(valid=0, invalid=0, clear=0)
    for it in range(3000):
        scale = 10.0 ** rng.uniform(-2, 5)
        p1 = rng.uniform(-1, 1, (k, 2)) * scale + rng.choice([0.0, 1e4, 1e5])
        p2 = rng.uniform(-1, 1, (k, 2)) * scale * rng.uniform(0.25, 4)
        kind = it % 6
        for img, p in ((1, p1), (2, p2)):
            if kind == img or kind == 3:                 # degenerate in that image (3: both)
                if model == FULL:                        # near-collinear third point, tiny off-line distance
                    p[2] = p[0] + rng.uniform(-2, 2) * (p[1] - p[0]) + rng.normal(0, 1) * 10.0 ** rng.uniform(-12, 0)
                else:
                    p[1] = p[0]
        if kind == 4:
            (p1 if rng.integers(2) else p2)[rng.integers(k), rng.integers(2)] = np.nan
        p1, p2 = p1.astype(np.float32).astype(np.float64), p2.astype(np.float32).astype(np.float64)
        ok, A = R.solve(model, p1, p2)
        valid, clear = np_sample_rule(model, p1, p2)
        if clear:
            counts["clear"] += 1
            assert ok == valid, (it, kind, p1, p2)
        counts["valid" if ok else "invalid"] += 1
        if not ok:
            assert not A.any()
    assert counts["clear"] >= 2900 and counts["valid"] >= 800 and counts["invalid"] >= 800, counts


# ---- S28 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("W", [1000, 4000, 16000])
@pytest.mark.parametrize("offset", [(0.0, 0.0), (1e5, -4e4)])
def test_restated_mask_matches_float64_residual(model, W, offset):
    case = (W, int(0.75 * W), None, None, None, None, False, offset, 0.5 + W / 8000.0, 0.3)
    xy1, xy2, Ag, inl = wide_view(4000, W, case, model)
    thr = thresh_for(case, Ag)
    checked, models = 0, 0
    for k, A in enumerate([Ag] + [R.model_of(model, xy1, xy2, 5, h)[1] for h in range(40)]):
        if not A.any():
            continue
        mask, c = R.score(A, xy1, xy2, thr)
        assert c == mask.sum()
        checked += check_mask_vs_float64(A, xy1, xy2, thr, mask, (W, offset, k))
        models += 1
    assert models >= 35 and checked >= 0.95 * 4000 * models, (models, checked)          # band: 0.1-2 % of points


# ---- S30 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("ci", range(len(WIDE_CASES)))
def test_restated_refit_matches_lstsq_umeyama_and_scipy(model, ci):
    case = WIDE_CASES[ci]
    xy1, xy2, Ag, inl = wide_view(2000, 40 + ci, case, model)
    thr = thresh_for(case, Ag)
    key, A0, mask, c = R.run(model, xy1, xy2, 300, thr, 0x99 + ci)
    assert key and c >= 0.6 * inl.sum()
    st, A, cin, cout, nu = R.refine(model, xy1, xy2, mask, A0)
    assert st == 0 and nu == c and cout <= cin
    check_refit_vs_lstsq(model, xy1, xy2, mask, A, (ci, model))
    assert abs(forward_cost(model, xy1, xy2, mask, A) - cout) <= 1e-9 * cout
    check_refit_optimal(model, xy1, xy2, mask, A0, cout, (ci, model))
    # idempotence: the refit of the refit is itself, bit for bit, and ties are accepted
    st2, A2, cin2, cout2, nu2 = R.refine(model, xy1, xy2, mask, A)
    assert st2 == 0 and _bits_equal(A2, A) and cin2 == cout2 == cout and nu2 == nu


@pytest.mark.parametrize("spread_ratio", [1e-3, 0.3, 0.8, 1.25, 3.0, 1e3])
def test_restated_near_degenerate_refit_follows_the_det_rule(spread_ratio):
    """Inliers in a thin strip, spread chosen so that det / (Sxx Syy) lands on either side of 1e-12: the full refit runs
    exactly when the numpy statement says so (a rejected refit returns A_in bit for bit); the partial one always runs."""
    n, L = 600, 4000.0
    p1 = strip(n, int(spread_ratio * 1000), L, strip_spread(spread_ratio, L))
    A_gt = np.array([[0.9, -0.2, 31.0], [0.25, 1.1, -12.0]])
    p2 = positions(A_gt, p1).astype(np.float32)
    A_in = A_gt + [[1e-3, -2e-3, 3.0], [2e-3, 1e-3, -4.0]]          # far worse than any least-squares fit
    ones = np.ones(n, np.uint8)
    valid, clear, ratio = np_det_rule(p1)
    st, A, cin, cout, nu = R.refine(FULL, p1, p2, ones, A_in)
    assert clear, ratio
    if valid:
        assert st == 0 and cout < cin, (ratio, st)
    else:
        assert st == 1 and _bits_equal(A, A_in) and cout == cin, (ratio, st)
    st, A, cin, cout, nu = R.refine(PARTIAL, p1, p2, ones, A_in)
    assert st == 0 and A[0, 0] == A[1, 1] and A[0, 1] == -A[1, 0]
    U = umeyama(p1, p2)
    assert np.abs(positions(A, p1) - positions(U, p1)).max() <= 1e-6
    check_refit_optimal(PARTIAL, p1, p2, ones, A_in, cout, spread_ratio)


def test_near_degenerate_strip_brackets_the_rule():
    """The strips above really sit on both sides of the rule, close to it."""
    got = {}
    for r in (0.3, 0.8, 1.25, 3.0):
        L = 4000.0
        got[r] = np_det_rule(strip(600, int(r * 1000), L, strip_spread(r, L)))[2] / DET_REL
    assert 0.1 < got[0.3] < got[0.8] < 0.95 and 1.05 < got[1.25] < got[3.0] < 10.0, got


@pytest.mark.parametrize("model", MODELS)
def test_restated_refit_on_collinear_and_nonfinite_inliers(model):
    x = np.linspace(5, 3950, 300)
    l1 = np.column_stack([x, 0.3 * x + 11]).astype(np.float32)
    A_gt = np.array([[0.8, 0.1, 3.0], [-0.1, 0.8, 20.0]])
    l2 = positions(A_gt, l1).astype(np.float32)
    A_in = A_gt + 1e-3
    st, A, cin, cout, nu = R.refine(model, l1, l2, np.ones(300, np.uint8), A_in)
    if model == FULL:
        assert st == 1 and _bits_equal(A, A_in)                # det is exactly 0 up to rounding: below the rule
    else:
        assert st == 0 and cout < cin
    # a NaN or Inf row inside the mask: every sum is NaN, the refit is rejected and A_in comes back bit for bit
    xy1, xy2, Ag, _ = wide_view(500, 3, WIDE_CASES[3], model)
    for v in (np.nan, np.inf, -np.inf):
        for c in range(4):
            a, b = xy1.copy(), xy2.copy()
            (a if c < 2 else b)[17, c % 2] = v
            st, A, cin, cout, nu = R.refine(model, a, b, np.ones(500, np.uint8), Ag)
            assert st == 1 and _bits_equal(A, Ag) and nu == 500, (v, c)


# ---- non-finite rows and thresholds ------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_restated_nonfinite_rows_and_samples(model):
    xy1, xy2, Ag, inl = wide_view(2000, 9, WIDE_CASES[2], model)
    thr = thresh_for(WIDE_CASES[2], Ag)
    sampled = np.concatenate([R.sample(model, 0x51, h, 2000) for h in range(40)])
    a, b, bad, nonfin = poisoned_rows(xy1, xy2, 0.05, 9, ids=sampled)
    for v in NONFINITE[:3]:
        for c in range(4):
            p, q = xy1.copy(), xy2.copy()
            (p if c < 2 else q)[:, c % 2] = v
            assert R.score(Ag, p, q, thr)[1] == 0, (v, c)
    invalid = 0
    for h in range(400):
        idx = R.sample(model, 0x51, h, 2000)
        ok, A = R.model_of(model, a, b, 0x51, h)
        valid, clear = np_sample_rule(model, a[idx], b[idx])
        if clear:
            assert ok == valid, h
        if nonfin[idx].any():
            assert not ok and not A.any(), h
            invalid += 1
    assert invalid >= 20, invalid
    key, A, mask, c = R.run(model, a, b, 600, thr, 0x51)
    assert key and not mask[nonfin].any() and c == mask.sum()
    check_mask_vs_float64(A, a, b, thr, mask, model)
    st, Ar, cin, cout, nu = R.refine(model, a, b, mask, A)
    assert st == 0 and np.isfinite(Ar).all() and np.isfinite([cin, cout]).all()


@pytest.mark.parametrize("model", MODELS)
def test_restated_threshold_edges(model):
    xy1, xy2, Ag, inl = wide_view(1500, 12, WIDE_CASES[0], model)
    # a few rows exactly on the model (residual 0) and a few with residuals around 1e-20 px near the origin
    A32 = Ag.astype(np.float32)
    xy1[:4] = 0.0
    xy2[:4] = A32[:, 2]                                   # u = fmaf(a0, 0, fmaf(a1, 0, a2)) = a2 exactly
    xy2[4:8] = A32[:, 2] + np.float32(3e-20)
    thr2_of = lambda t: np.float32(t) * np.float32(t)
    with np.errstate(over="ignore", invalid="ignore"):
        for t, admits in THRESH_EDGES:
            mask, c = R.score(Ag, xy1, xy2, t)
            assert (c > 0) == admits and c == mask.sum(), (t, c)
            key, A, m2, c2 = R.run(model, xy1, xy2, 200, t, 0x7)
            assert key and (api.ransac_key_inliers(key) > 0) == admits and c2 == m2.sum(), t
            if not admits:                                # every valid model counts 0: the lowest valid id wins
                assert not m2.any() and api.ransac_key_hyp(key) == min(
                    h for h in range(200) if R.model_of(model, xy1, xy2, 0x7, h)[0]), t
            t2 = thr2_of(t)
            if admits and np.isfinite(t2) and t2 > 1e-30:
                check_mask_vs_float64(Ag, xy1, xy2, float(np.sqrt(np.float64(t2))), mask, t)
            if admits and t2 < 1e-30:                     # subnormal thr2: only the exact rows
                assert mask[:4].all() and not mask[4:].any(), t
        m_neg, _ = R.score(Ag, xy1, xy2, -2.5)
        m_pos, _ = R.score(Ag, xy1, xy2, 2.5)
        assert (m_neg == m_pos).all()                     # thr2 = tau * tau: the sign of tau does not matter


# ---- wrappers ----------------------------------------------------------------------------------------------------
def test_affine_wrappers_reject_mismatched_lengths_without_a_device():
    """The Python wrappers check the row counts before any call into the library (a shorter xy2 would be read past)."""
    ctx = api.Context.__new__(api.Context)            # no device: the check must come first
    ctx._h = C.c_void_p()
    xy1, xy2 = np.zeros((10, 2), np.float32), np.zeros((9, 2), np.float32)
    for model in MODELS:
        for call in (lambda: ctx.ransac_affine(xy1, xy2, 10, 2.0, 1, model=model),
                     lambda: ctx.ransac_affine_from_hyp(xy1, xy2, 0, 2.0, 1, model=model),
                     lambda: ctx.estimate_affine(xy1, xy2, 10, 2.0, 1, model=model),
                     lambda: ctx.ransac_affine(xy2, xy1, 10, 2.0, 1, model=model),
                     lambda: ctx.affine_refine(xy1, xy2, np.ones(10, np.uint8), np.eye(2, 3), model=model)):
            with pytest.raises(ValueError):
                call()
