"""CPU: the restatement of docs/SPEC.md S26-S30 (tests/affine_ref.c) — robust 2D affine / similarity estimation and the
least-squares refit — checked against the SPEC's stream definitions and INDEPENDENT algorithms (numpy.linalg.solve on
the minimal systems, numpy.linalg.lstsq on the inliers, S21's homography test on [A; 0 0 1]), plus the argument checks
of the shipped entry points, which need no device."""
import ctypes as C

import numpy as np
import pytest

import affine_ref as R
import homography_ref as HR
from points_matching_amd import api, synth

M64 = (1 << 64) - 1
FULL, PARTIAL = api.PM_AFFINE_FULL, api.PM_AFFINE_PARTIAL
MODELS = (FULL, PARTIAL)


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def walk(seed, h, n, k, const):
    """S6's walk with k accepted indices on the stream keyed by `const`."""
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
S26 = {FULL: 0x79B97F4A7C159E37, PARTIAL: 0x7C159E3779B97F4A}


@pytest.mark.parametrize("model", MODELS)
def test_sampler_is_the_spec_walk_and_a_pure_function(model):
    k = R.min_pts(model)
    rng = np.random.default_rng(26 + model)
    for _ in range(400):
        seed, h, n = int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 32)), int(rng.integers(k, 5000))
        a = R.sample(model, seed, h, n)
        assert list(a) == walk(seed, h, n, k, S26[model])
        assert (R.sample(model, seed, h, n) == a).all()
        assert len(set(a.tolist())) == k and a.min() >= 0 and a.max() < n
    for n in (k, k + 1, k + 2):                        # tiny n: the deterministic completion rule
        for h in range(200):
            a = R.sample(model, 7, h, n)
            assert len(set(a.tolist())) == k and a.max() < n
            assert list(a) == walk(7, h, n, k, S26[model])


def test_sampler_streams_are_distinct_from_each_other_and_s6_s13_s19():
    same = dict.fromkeys(("full-partial", "S6", "S13", "S19"), 0)
    for h in range(2000):
        f = walk(0x5EED, h, 2275, 3, S26[FULL])
        p = walk(0x5EED, h, 2275, 2, S26[PARTIAL])
        same["full-partial"] += f[:2] == p
        for name, c in (("S6", S6), ("S13", S13), ("S19", S19)):
            o = walk(0x5EED, h, 2275, 3, c)
            same[name] += (f == o) + (p == o[:2])
    assert not any(same.values()), same


def np_solve(model, p1, p2):
    """The minimal system solved by LAPACK: 6 x 6 (full) or 4 x 4 (partial, unknowns a, b, tx, ty)."""
    M, r = [], []
    for (x, y), (u, v) in zip(p1, p2):
        if model == FULL:
            M += [[x, y, 1, 0, 0, 0], [0, 0, 0, x, y, 1]]
        else:
            M += [[x, -y, 1, 0], [y, x, 0, 1]]
        r += [u, v]
    s = np.linalg.solve(np.array(M, np.float64), np.array(r, np.float64))
    if model == FULL:
        return s.reshape(2, 3)
    return np.array([[s[0], -s[1], s[2]], [s[1], s[0], s[3]]])


@pytest.mark.parametrize("model", MODELS)
def test_minimal_solve_recovers_planted_model_and_agrees_with_numpy(model):
    k = R.min_pts(model)
    for seed in range(300):
        _, _, A_gt, _ = synth.affine_view(4, seed=seed, partial=model == PARTIAL)
        rng = np.random.default_rng(seed)
        p1 = rng.uniform([0, 0], [993, 660], (k, 2))
        p2 = p1 @ A_gt[:, :2].T + A_gt[:, 2]
        ok, A = R.solve(model, p1, p2)
        assert ok, seed
        scale = np.abs(A_gt).max()
        assert np.abs(A - A_gt).max() <= 1e-9 * scale, (seed, A, A_gt)
        assert np.abs(A - np_solve(model, p1, p2)).max() <= 1e-9 * scale
        if model == PARTIAL:                           # the similarity form holds exactly
            assert A[0, 0] == A[1, 1] and A[0, 1] == -A[1, 0]


def test_collinear_triples_and_coincident_pairs_are_invalid_in_either_image():
    good = np.array([[10.0, 20.0], [300.0, 40.0], [120.0, 400.0]])
    line = np.array([[10.0, 20.0], [110.0, 70.0], [310.0, 170.0]])           # exactly collinear
    assert R.solve(FULL, good, good * 1.1 + 3)[0]
    assert not R.solve(FULL, line, good)[0]
    assert not R.solve(FULL, good, line)[0]
    assert not R.solve(FULL, line + 1e-9, good)[0]                           # collinear within FLT_EPSILON
    nan = good.copy()
    nan[1, 0] = np.nan
    assert not R.solve(FULL, nan, good)[0] and not R.solve(FULL, good, nan)[0]
    assert not R.solve(FULL, good, np.repeat(good[:1], 3, axis=0))[0]        # all three coincide in image 2
    mirror = good * np.array([-1.0, 1.0]) + [700, 0]                         # a reflection is a valid affine map
    ok, A = R.solve(FULL, good, mirror)
    assert ok and np.linalg.det(A[:, :2]) < 0
    pair = good[:2]
    assert R.solve(PARTIAL, pair, pair * 0.9 + 5)[0]
    same = np.repeat(pair[:1], 2, axis=0)
    assert not R.solve(PARTIAL, same, pair)[0] and not R.solve(PARTIAL, pair, same)[0]
    assert not R.solve(PARTIAL, nan[:2], pair)[0] and not R.solve(PARTIAL, pair, nan[:2])[0]
    # invalid samples leave A = 0
    assert not R.solve(FULL, line, good)[1].any() and not R.solve(PARTIAL, same, pair)[1].any()


def test_inlier_test_matches_float64_and_s21_bit_for_bit():
    rng = np.random.default_rng(28)
    _, _, A, _ = synth.affine_view(4, seed=3)
    a32 = A.astype(np.float32)
    h32 = np.concatenate([a32.reshape(6), np.float32([0, 0, 1])]).astype(np.float32)
    thr = 1.5
    agree = 0
    for _ in range(4000):
        x, y = rng.uniform(-50, 1050, 2).astype(np.float32)
        u, v = (a32.astype(np.float64) @ np.array([x, y, 1.0]))
        off = rng.uniform(0, 2 * thr) * np.exp(1j * rng.uniform(0, 2 * np.pi))
        xp, yp = np.float32(u + off.real), np.float32(v + off.imag)
        d2 = (np.float64(xp) - u) ** 2 + (np.float64(yp) - v) ** 2
        got = R.inlier(a32, x, y, xp, yp, np.float32(thr * thr))
        if abs(d2 - thr * thr) > 1e-3:
            assert got == (d2 <= thr * thr)
            agree += 1
        # S28 is S21 on [A; 0 0 1] for every input
        assert got == bool(HR.lib().hr_inlier(HR._p(h32), C.c_float(x), C.c_float(y), C.c_float(xp), C.c_float(yp),
                                               C.c_float(thr * thr)))
    assert agree > 3500
    specials = [np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, 3e38]
    for x in specials:
        for t2 in (2.25, 0.0, np.inf, np.nan, 1e-44):
            for args in ((x, 5.0, 5.0, 5.0), (5.0, x, 5.0, 5.0), (5.0, 5.0, x, 5.0), (5.0, 5.0, 5.0, x)):
                got = R.inlier(a32, *[C.c_float(v) for v in args], C.c_float(t2))
                ref = bool(HR.lib().hr_inlier(HR._p(h32), *[C.c_float(v) for v in args], C.c_float(t2)))
                assert got == ref, (args, t2)
                if not np.isfinite(x) or not np.isfinite(t2) or t2 == 0.0:
                    assert not got, (args, t2)


def lstsq_fit(model, p1, p2):
    if model == FULL:
        M = np.column_stack([p1, np.ones(len(p1))])
        return np.linalg.lstsq(M, p2, rcond=None)[0].T
    rows = np.zeros((2 * len(p1), 4))
    rows[0::2] = np.column_stack([p1[:, 0], -p1[:, 1], np.ones(len(p1)), np.zeros(len(p1))])
    rows[1::2] = np.column_stack([p1[:, 1], p1[:, 0], np.zeros(len(p1)), np.ones(len(p1))])
    s = np.linalg.lstsq(rows, p2.reshape(-1), rcond=None)[0]
    return np.array([[s[0], -s[1], s[2]], [s[1], s[0], s[3]]])


@pytest.mark.parametrize("model", MODELS)
def test_refit_equals_numpy_lstsq_on_the_inliers(model):
    for seed in range(20):
        n = (50, 700, 2275)[seed % 3]
        xy1, xy2, A_gt, inl = synth.affine_view(n, seed=seed, outlier_frac=0.3, noise_px=0.7, partial=model == PARTIAL)
        key, A, mask, c = R.run(model, xy1, xy2, 500, 2.0, seed)
        assert key != 0
        st, Ar, cin, cout, nu = R.refine(model, xy1, xy2, mask, A)
        m = mask.astype(bool)
        ref = lstsq_fit(model, xy1[m].astype(np.float64), xy2[m].astype(np.float64))
        assert st == 0 and nu == c == m.sum()
        assert np.abs(Ar - ref).max() <= 1e-10 * np.abs(ref).max(), (seed, Ar, ref)
        assert cout <= cin
        p = np.column_stack([xy1[m], np.ones(m.sum())]).astype(np.float64)
        assert abs(cout - ((p @ Ar.T - xy2[m]) ** 2).sum()) <= 1e-9 * cout


@pytest.mark.parametrize("model", MODELS)
def test_cost_never_increases_on_a_seeded_sweep(model):
    rng = np.random.default_rng(30 + model)
    for seed in range(60):
        n = int(rng.integers(2, 400))
        xy1, xy2, A_gt, _ = synth.affine_view(n, seed=seed, outlier_frac=rng.uniform(0, 0.6), noise_px=rng.uniform(0, 3),
                                              partial=model == PARTIAL)
        mask = (rng.uniform(size=n) < rng.uniform(0.05, 1.0)).astype(np.uint8)
        A_in = A_gt + rng.normal(0, 0.01, (2, 3)) * [[1, 1, 100], [1, 1, 100]]
        st, A, cin, cout, nu = R.refine(model, xy1, xy2, mask, A_in)
        assert st in (0, 1) and cout <= cin and nu == mask.sum()
        if st == 1:
            assert (A.view(np.uint64) == A_in.view(np.uint64)).all()


@pytest.mark.parametrize("model", MODELS)
def test_degenerate_paths(model):
    xy1, xy2, A_gt, _ = synth.affine_view(40, seed=1, outlier_frac=0.0, noise_px=0.3, partial=model == PARTIAL)
    ones = np.ones(40, np.uint8)
    st, A, cin, cout, nu = R.refine(model, xy1, xy2, ones, np.zeros((2, 3)))
    assert st == 2 and not A.any() and cin == cout == 0.0 and nu == 0
    st, A, *_ = R.refine(model, xy1, xy2, ones, -np.zeros((2, 3)))                  # either sign of zero
    assert st == 2
    few = np.zeros(40, np.uint8)
    few[:R.min_pts(model) - 1] = 1
    st, A, cin, cout, nu = R.refine(model, xy1, xy2, few, A_gt)
    assert st == 1 and (A == A_gt).all() and cin == cout and nu == R.min_pts(model) - 1
    st, A, cin, cout, nu = R.refine(model, xy1, xy2, np.zeros(40, np.uint8), A_gt)
    assert st == 1 and nu == 0 and cin == 0.0
    # all inliers on one line: the full normal system is singular; the partial one is not
    x = np.linspace(5, 950, 40)
    l1 = np.column_stack([x, 0.3 * x + 11]).astype(np.float32)
    l2 = np.column_stack([0.8 * x + 3, 0.24 * x + 20]).astype(np.float32)
    st, A, cin, cout, nu = R.refine(model, l1, l2, ones, A_gt)
    assert st in (0, 1) and cout <= cin
    if model == FULL:
        assert st == 1 and (A == A_gt).all()
    # coincident inliers: no spread at all
    st, A, *_ = R.refine(model, np.repeat(xy1[:1], 40, 0), np.repeat(xy2[:1], 40, 0), ones, A_gt)
    assert st == 1 and (A == A_gt).all()
    # the exact least-squares solution is its own refit: the same bits at the same cost, and the tie is accepted
    st, A0, *_ = R.refine(model, xy1, xy2, ones, A_gt)
    st2, A1, cin, cout, _ = R.refine(model, xy1, xy2, ones, A0)
    assert st2 == 0 and (A1.view(np.uint64) == A0.view(np.uint64)).all() and cin == cout


@pytest.mark.parametrize("model", MODELS)
def test_run_finds_the_planted_model(model):
    xy1, xy2, A_gt, inl = synth.affine_view(800, seed=9, outlier_frac=0.45, noise_px=0.3, partial=model == PARTIAL)
    key, A, mask, c = R.run(model, xy1, xy2, 300, 3.0, 0xA1)
    assert key != 0 and api.ransac_key_inliers(key) == c == mask.sum()
    assert (mask.astype(bool) & inl).sum() >= 0.95 * inl.sum()
    st, Ar, *_ = R.refine(model, xy1, xy2, mask, A)
    p = np.column_stack([xy1[inl], np.ones(inl.sum())]).astype(np.float64)
    rms = lambda M: np.sqrt((((p @ M.T) - (p @ A_gt.T)) ** 2).sum(axis=1).mean())
    assert st == 0 and rms(Ar) < 0.08 and rms(Ar) < 0.5 * rms(A), (rms(Ar), rms(A))


def test_affine_view_is_consistent():
    for partial in (False, True):
        xy1, xy2, A, inl = synth.affine_view(500, seed=4, outlier_frac=0.3, noise_px=0.0, partial=partial)
        assert xy1.dtype == xy2.dtype == np.float32 and A.shape == (2, 3) and inl.sum() == 350
        r = np.column_stack([xy1, np.ones(500)]).astype(np.float64) @ A.T - xy2
        assert np.abs(r[inl]).max() < 1e-3 and np.abs(r[~inl]).max() > 10
        if partial:
            assert abs(A[0, 0] - A[1, 1]) < 1e-15 and abs(A[0, 1] + A[1, 0]) < 1e-15


@pytest.mark.parametrize("model", MODELS)
def test_library_rejects_bad_arguments_without_a_device(model):
    L = api.lib()
    k = R.min_pts(model)
    xy = np.zeros((10, 2), np.float32)
    m = np.ones(10, np.uint8)
    A = np.zeros(6)
    good = api.RansacParams(0, 10, 1, 2.0, api.PM_ERR_REPROJ)
    bad = api.RansacParams(0, 10, 1, 2.0, api.PM_ERR_SAMPSON)
    empty = api.RansacParams(5, 5, 1, 2.0, api.PM_ERR_REPROJ)
    key, ninl = C.c_uint64(), C.c_int()
    info = api.HRefineInfo()

    def run(mdl=model, prm=good, n=10, pts=True):
        A[:] = 7.0
        return L.pm_ransac_affine(None, mdl, api._p(xy) if pts else None, api._p(xy) if pts else None, n,
                                  C.byref(prm) if prm is not None else None, api._p(A), None, C.byref(ninl), C.byref(key))

    for mdl in (2, -1):
        assert run(mdl=mdl) == api.PM_E_INVALID and b"model" in L.pm_last_error() and not A.any()
    assert run(prm=bad) == api.PM_E_INVALID and b"error_kind" in L.pm_last_error()
    assert run(prm=empty) == api.PM_E_INVALID
    assert run(prm=None) == api.PM_E_INVALID
    assert run(pts=False) == api.PM_E_INVALID
    assert run(n=-1) == api.PM_E_INVALID
    assert run(n=k - 1) == api.PM_E_TOO_FEW and not A.any()
    assert run(n=k) == api.PM_E_INVALID and b"ctx" in L.pm_last_error()        # ctx last: everything else passed

    def hyp(mdl=model, prm=good, h=0, n=10):
        return L.pm_ransac_affine_from_hyp(None, mdl, api._p(xy), api._p(xy), n, C.byref(prm), C.c_int64(h), api._p(A),
                                           None, None)

    assert hyp(mdl=2) == api.PM_E_INVALID and hyp(mdl=-1) == api.PM_E_INVALID
    assert hyp(h=-1) == api.PM_E_INVALID and hyp(h=1 << 32) == api.PM_E_INVALID
    assert hyp(prm=bad) == api.PM_E_INVALID
    assert hyp(n=k - 1) == api.PM_E_TOO_FEW
    assert hyp() == api.PM_E_INVALID and b"ctx" in L.pm_last_error()

    view = api.PointsView(1, 1, None, 1, 10, 0, 1, 0)
    d = C.c_void_p(16)                                           # never dereferenced: the calls fail before any launch

    def dev(mdl=model, v=view, prm=good, outs=(d, d, d, d), mask_len=10):
        return L.pm_ransac_affine_run_dev(None, mdl, C.byref(v) if v is not None else None, C.byref(prm), outs[0],
                                          outs[1], outs[2], mask_len, outs[3])

    assert dev(mdl=2) == api.PM_E_INVALID and dev(mdl=-1) == api.PM_E_INVALID
    assert dev(prm=bad) == api.PM_E_INVALID and dev(prm=empty) == api.PM_E_INVALID
    assert dev(v=None) == api.PM_E_INVALID
    assert dev(v=api.PointsView(1, 1, None, 0, 10, 0, 1, 0)) == api.PM_E_INVALID
    assert dev(outs=(None, d, d, d)) == api.PM_E_INVALID and dev(outs=(d, d, None, d)) == api.PM_E_INVALID
    assert dev(mask_len=-1) == api.PM_E_INVALID
    assert dev() == api.PM_E_INVALID and b"ctx" in L.pm_last_error()

    Ain = np.array([1.0, 0, 0, 0, 1, 0])

    def ref(mdl=model, n=10, mask=m, a_in=Ain):
        A[:] = 7.0
        return L.pm_affine_refine(None, mdl, api._p(xy), api._p(xy), n, api._p(mask) if mask is not None else None,
                                  api._p(a_in) if a_in is not None else None, api._p(A), C.byref(info))

    assert ref(mdl=2) == api.PM_E_INVALID and ref(mdl=-1) == api.PM_E_INVALID
    assert ref(mask=None) == api.PM_E_INVALID and ref(a_in=None) == api.PM_E_INVALID
    assert ref(n=-1) == api.PM_E_INVALID
    assert ref(n=k - 1) == api.PM_E_TOO_FEW and (A == Ain).all() and info.status == 1        # A_out = A_in
    assert ref() == api.PM_E_INVALID and b"ctx" in L.pm_last_error()

    def refd(mdl=model, v=view, mask=d):
        return L.pm_affine_refine_dev(None, mdl, C.byref(v) if v is not None else None, mask, d, d, None)

    assert refd(mdl=2) == api.PM_E_INVALID and refd(mdl=-1) == api.PM_E_INVALID
    assert refd(mask=None) == api.PM_E_INVALID and refd(v=None) == api.PM_E_INVALID
    assert refd() == api.PM_E_INVALID and b"ctx" in L.pm_last_error()

    def est(mdl=model, prm=good, n=10, refine=1):
        return L.pm_estimate_affine(None, mdl, api._p(xy), api._p(xy), n, C.byref(prm), refine, api._p(A), None,
                                    C.byref(ninl), C.byref(key), C.byref(info))

    assert est(mdl=2) == api.PM_E_INVALID and est(mdl=-1) == api.PM_E_INVALID
    assert est(prm=bad) == api.PM_E_INVALID and est(prm=empty) == api.PM_E_INVALID
    assert est(n=k - 1) == api.PM_E_TOO_FEW and info.status == 2
    assert est(refine=0) == api.PM_E_INVALID and b"ctx" in L.pm_last_error()
    assert est() == api.PM_E_INVALID and b"ctx" in L.pm_last_error()
