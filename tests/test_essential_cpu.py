"""CPU: the C restatement of docs/SPEC.md S31-S35 (tests/essential_ref.c) against independent numpy references: the
true E among the 5-point candidates, the epipolar and cubic constraints, the Gauss-Jordan reduction and the real-root
count against numpy's linear solve and companion-matrix roots, the decomposition against np.linalg.svd, the
triangulation against the SVD DLT and the cheirality counts, plus a mutation check (a Gauss-Jordan without its pivot
swap is caught by the same comparison), plus the argument checks of the shipped entry points, which need no device."""
import ctypes as C

import numpy as np

import essential_ref as R
from points_matching_amd import api, synth


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def _rot(rng, s=0.3):
    w = rng.normal(size=3) * s
    th = np.linalg.norm(w)
    k = _skew(w / th)
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * k @ k


def _sample(rng):
    Rt = _rot(rng)
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = np.c_[rng.uniform(-1, 1, (5, 2)), rng.uniform(2, 6, 5)]
    X2 = X @ Rt.T + t
    E = _skew(t) @ Rt
    return X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:], E / np.linalg.norm(E), Rt, t


def _nullspace(p1, p2):
    # rows [x2x1 x2y1 x2 y2x1 y2y1 y2 x1 y1 1]; the basis of numpy's SVD, not the restatement's Householder one
    A = np.c_[p2[:, 0] * p1[:, 0], p2[:, 0] * p1[:, 1], p2[:, 0], p2[:, 1] * p1[:, 0], p2[:, 1] * p1[:, 1], p2[:, 1],
              p1[:, 0], p1[:, 1], np.ones(5)]
    return np.linalg.svd(A)[2][5:]


def test_true_essential_among_candidates():
    rng = np.random.default_rng(1)
    hit = 0
    for _ in range(1000):
        p1, p2, Et, _, _ = _sample(rng)
        E, v, _ = R.solve5(p1, p2)
        err = [min(np.abs(E[j] - Et).max(), np.abs(E[j] + Et).max()) / np.abs(Et).max() for j in range(10) if v[j]]
        hit += bool(err) and min(err) < 1e-8
    assert hit >= 990


def test_candidates_satisfy_epipolar_and_cubic_constraints():
    # every candidate to 1e-9 but the ill-conditioned few (a root next to another one, a back-substitution with a small
    # pivot): 99% within 1e-9, all within 1e-6
    rng = np.random.default_rng(2)
    worst = []
    for _ in range(300):
        p1, p2, _, _, _ = _sample(rng)
        E, v, _ = R.solve5(p1, p2)
        h1, h2 = np.c_[p1, np.ones(5)], np.c_[p2, np.ones(5)]
        for j in np.nonzero(v)[0]:
            e = E[j]
            assert abs(np.linalg.norm(e) - 1) < 1e-12
            f = e.reshape(-1)
            assert f[np.argmax(np.abs(f))] > 0                 # sign rule: first entry of largest magnitude positive
            worst.append(max(np.abs(np.einsum("ni,ij,nj->n", h2, e, h1)).max(), abs(np.linalg.det(e)),
                             np.abs(2 * e @ e.T @ e - np.trace(e @ e.T) * e).max()))
    worst = np.array(worst)
    assert len(worst) > 900
    assert (worst < 1e-9).mean() >= 0.99 and worst.max() < 1e-6


# -- an independent expansion of the constraints: polynomials as {(ex, ey, ez): coefficient} --------------------------
MONO = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
        (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def _pmul(a, b):
    o = {}
    for ka, va in a.items():
        for kb, vb in b.items():
            k = (ka[0] + kb[0], ka[1] + kb[1], ka[2] + kb[2])
            o[k] = o.get(k, 0.0) + va * vb
    return o


def _padd(a, b, s=1.0):
    o = dict(a)
    for k, v in b.items():
        o[k] = o.get(k, 0.0) + s * v
    return o


def _numpy_matrix(N):
    E = [[{(1, 0, 0): N[0][3 * i + j], (0, 1, 0): N[1][3 * i + j], (0, 0, 1): N[2][3 * i + j], (0, 0, 0): N[3][3 * i + j]}
          for j in range(3)] for i in range(3)]
    det = {}
    for (a, b, c), s in (((0, 1, 2), 1), ((1, 2, 0), 1), ((2, 0, 1), 1), ((0, 2, 1), -1), ((2, 1, 0), -1), ((1, 0, 2), -1)):
        det = _padd(det, _pmul(_pmul(E[0][a], E[1][b]), E[2][c]), s)
    EEt = [[_padd(_padd(_pmul(E[i][0], E[j][0]), _pmul(E[i][1], E[j][1])), _pmul(E[i][2], E[j][2])) for j in range(3)]
           for i in range(3)]
    tr = _padd(_padd(EEt[0][0], EEt[1][1]), EEt[2][2])
    rows = [det]
    for i in range(3):
        for j in range(3):
            r = {}
            for k in range(3):
                r = _padd(r, _pmul(EEt[i][k], E[k][j]), 2.0)
            rows.append(_padd(r, _pmul(tr, E[i][j]), -1.0))
    return np.array([[r.get(m, 0.0) for m in MONO] for r in rows])


def _gj_python(A, swap=True):
    A = A.copy()
    for j in range(10):
        p = j + int(np.argmax(np.abs(A[j:, j]))) if swap else j
        A[[j, p]] = A[[p, j]]
        A[j] = A[j] / A[j, j]
        for r in range(10):
            if r != j:
                A[r] -= A[r, j] * A[j]
    return A


def test_reduction_and_root_count_match_numpy():
    rng = np.random.default_rng(3)
    agree = close = 0
    for _ in range(300):
        p1, p2, _, _, _ = _sample(rng)
        N = _nullspace(p1, p2)
        A = R.constraints(N)
        An = _numpy_matrix(N)
        ok, G = R.gauss_jordan(A)
        assert ok
        ref = np.linalg.solve(An[:, :10], An[:, 10:])          # independent: rows scaled / ordered differently
        assert np.abs(G[:, 10:] - ref).max() < 1e-7 * max(1.0, np.abs(ref).max())
        B, p = R.detpoly(G)
        ours = R.roots(p)
        rr = np.roots(p[::-1])
        d = np.abs(rr[:, None] - rr[None, :]) + np.eye(len(rr))
        if d.min() < 1e-4 * max(1.0, np.abs(rr).max()):      # two roots within the gap: the count may differ
            close += 1
            continue
        real = np.sort(rr[np.abs(rr.imag) < 1e-6 * np.maximum(1.0, np.abs(rr))].real)
        assert len(ours) == len(real)
        assert np.allclose(ours, real, rtol=1e-7, atol=1e-9)
        agree += 1
    assert agree >= 290


def test_pivot_rule_is_needed():
    # a zero leading entry: the restatement pivots and matches numpy; the same elimination without the swap (mutant)
    # divides by zero, and the comparison above catches it
    rng = np.random.default_rng(5)
    A = rng.normal(size=(10, 20))
    A[0, 0] = 0.0
    ok, G = R.gauss_jordan(A)
    assert ok
    ref = np.linalg.solve(A[:, :10], A[:, 10:])
    assert np.abs(G[:, 10:] - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())
    with np.errstate(all="ignore"):
        mut = _gj_python(A, swap=False)
    assert not (np.isfinite(mut).all() and np.abs(mut[:, 10:] - ref).max() < 1e-9 * max(1.0, np.abs(ref).max()))
    assert np.abs(_gj_python(A)[:, 10:] - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())
    assert not R.gauss_jordan(np.zeros((10, 20)))[0]


def _np_decompose(E):
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])
    return U @ W @ Vt, U @ W.T @ Vt, U[:, 2]


def test_decomposition_matches_numpy_svd():
    rng = np.random.default_rng(4)
    for _ in range(300):
        _, _, Et, _, _ = _sample(rng)
        ok, R1, R2, t = R.decompose(Et)
        assert ok
        N1, N2, tn = _np_decompose(Et)
        for Rm in (R1, R2):
            assert abs(np.linalg.det(Rm) - 1) < 1e-12 and np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-12
        assert min(np.abs(t - tn).max(), np.abs(t + tn).max()) < 1e-12
        pairs = min(max(np.abs(R1 - N1).max(), np.abs(R2 - N2).max()), max(np.abs(R1 - N2).max(), np.abs(R2 - N1).max()))
        assert pairs < 1e-12
    assert not R.decompose(np.zeros(9))[0]
    # mutant: W as a reflection ([[0 1 0] [1 0 0] [0 0 1]]) gives det -1 "rotations" that the checks above reject
    U, _, Vt = np.linalg.svd(Et)
    Wm = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1.0]])
    M1 = (U if np.linalg.det(U) > 0 else -U) @ Wm @ (Vt if np.linalg.det(Vt) > 0 else -Vt)
    assert abs(np.linalg.det(M1) - 1) > 1e-3 and np.abs(M1 - R1).max() > 1e-3 and np.abs(M1 - R2).max() > 1e-3
    assert not R.decompose(np.diag([1.0, 0, 0]))[0]


def test_triangulation_and_cheirality_match_numpy():
    xy1, xy2, K, Rg, tg, X, inl = synth.calibrated_view(400, seed=9, outlier_frac=0.2)
    k = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    x1n, x2n = R.normalise(k, xy1).astype(np.float64), R.normalise(k, xy2).astype(np.float64)
    E = _skew(tg) @ Rg
    ok, R1, R2, t = R.decompose(E / np.linalg.norm(E))
    assert ok
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    good = np.zeros(4, int)
    band = 0
    for i in range(400):
        for c, (Rm, tv) in enumerate(cands):
            Q = R.triangulate(Rm, tv, *x1n[i], *x2n[i])
            P0 = np.c_[np.eye(3), np.zeros(3)]
            P1 = np.c_[Rm, tv]
            A = np.array([x1n[i, 0] * P0[2] - P0[0], x1n[i, 1] * P0[2] - P0[1], x2n[i, 0] * P1[2] - P1[0],
                          x2n[i, 1] * P1[2] - P1[1]])
            q = np.linalg.svd(A)[2][-1]
            assert abs(abs(Q @ q) - 1) < 1e-9
            Xh = q[:3] / q[3]
            z2 = (Rm @ Xh + tv)[2]
            ref = q[2] * q[3] > 0 and Xh[2] < 50 and 0 < z2 < 50
            near = min(abs(Xh[2]), abs(Xh[2] - 50), abs(z2), abs(z2 - 50)) < 1e-9 * max(1.0, abs(Xh[2]))
            got = R.cheiral(Rm, tv, Q)
            if got != ref:
                assert near
                band += 1
            good[c] += got
    assert band <= 2
    ng, Rr, tr, mo, pts, g = R.recover_pose(xy1, xy2, k, E / np.linalg.norm(E))
    assert (g == good).all() and ng == good.max()
    assert np.abs(Rr - Rg).max() < 1e-9 and np.abs(tr - tg).max() < 1e-9
    assert mo[inl].mean() > 0.98


def test_sampler_and_camera_rules():
    for h in range(200):
        idx = R.sample(7, h, 9)
        assert len(set(idx.tolist())) == 5 and idx.min() >= 0 and idx.max() < 9
    assert (R.sample(7, 3, 5) == R.sample(7, 3, 5)).all()
    assert sorted(R.sample(1, 0, 5).tolist()) == [0, 1, 2, 3, 4]
    assert R.thr_n((800.0, 900.0, 1.0, 2.0), 1.0) == (True, np.float32(1.0 / 850.0))
    for bad in ((0.0, 1.0, 0.0, 0.0), (1.0, -1.0, 0.0, 0.0), (1.0, 1.0, np.nan, 0.0), (1.0, 1.0, 0.0, np.inf)):
        assert not R.thr_n(bad, 1.0)[0]
    assert not R.thr_n((800.0, 800.0, 0.0, 0.0), 0.0)[0]


def test_run_recovers_pose_on_cpu():
    xy1, xy2, K, Rg, tg, X, inl = synth.calibrated_view(600, seed=21, outlier_frac=0.3)
    k = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    key, E, mask, c = R.run(xy1, xy2, k, 300, 1.0, 5)
    assert key and c == mask.sum() >= 0.8 * inl.sum()
    assert (key >> 32) == c and (0xFFFFFFFF - (key & 0xFFFFFFFF)) // 10 < 300
    ng, Rr, tr, mo, _, _ = R.recover_pose(xy1, xy2, k, E, mask)
    assert ng >= 0.95 * c
    assert np.degrees(np.arccos(np.clip((np.trace(Rr.T @ Rg) - 1) / 2, -1, 1))) < 0.5
    assert np.degrees(np.arccos(np.clip(tr @ tg, -1, 1))) < 3.0


def test_library_rejects_bad_arguments_without_a_device():
    """Every check of the six entry points, tripped alone and in pairs that pin the order, with ctx = NULL: the checks
    all sit before the ctx check.  Messages are matched on the text after PM_REQUIRE's function-name prefix."""
    L = api.lib()
    INV, FEW = api.PM_E_INVALID, api.PM_E_TOO_FEW
    xy = np.zeros((10, 2), np.float32)
    m = np.ones(10, np.uint8)
    cam = api.Camera(800.0, 800.0, 320.0, 240.0)
    cam0, caminf = api.Camera(0.0, 800.0, 320.0, 240.0), api.Camera(800.0, 800.0, float("inf"), 240.0)
    good = api.RansacParams(0, 10, 1, 1.0, api.PM_ERR_SAMPSON)
    kind = api.RansacParams(0, 10, 1, 1.0, api.PM_ERR_REPROJ)
    empty = api.RansacParams(5, 5, 1, 1.0, api.PM_ERR_SAMPSON)
    neg = api.RansacParams(-1, 5, 1, 1.0, api.PM_ERR_SAMPSON)
    high = api.RansacParams(0, (1 << 32) // 10 + 1, 1, 1.0, api.PM_ERR_SAMPSON)
    wide = api.RansacParams(0, ((1 << 31) - 1) // 10 + 1, 1, 1.0, api.PM_ERR_SAMPSON)
    thr0 = api.RansacParams(0, 10, 1, 0.0, api.PM_ERR_SAMPSON)
    thrnan = api.RansacParams(0, 10, 1, float("nan"), api.PM_ERR_SAMPSON)
    E, Rm, t = np.zeros(9), np.zeros(9), np.zeros(3)
    E90, counts = np.zeros(90), np.zeros(10, np.int32)
    mask, pts4 = np.zeros(10, np.uint8), np.zeros((10, 4), np.float32)
    key, ninl, ng, nm = C.c_uint64(), C.c_int(), C.c_int(), C.c_int()
    Ein = np.array([0.0, -1, 0, 1, 0, 0, 0, 0, 0])
    nz = [10]

    def ref(p):
        return C.byref(p) if p is not None else None

    def refused(rc, status, frag):
        msg = L.pm_last_error()
        assert rc == status and frag in msg, (rc, msg)
        return True

    def poison(n):
        nz[0] = max(n, 0)                                        # the mask and the points are zeroed over n entries
        for a in (E, Rm, t, E90, pts4):
            a[...] = 7.0
        counts[:] = 7
        mask[:] = 7
        key.value, ninl.value, ng.value, nm.value = 7, 7, 7, 7

    # ---- pm_ransac_essential: params, K, point arrays, n < 5, ctx
    def run(prm=good, k=cam, n=10, pts=True):
        poison(n)
        return L.pm_ransac_essential(None, api._p(xy) if pts else None, api._p(xy) if pts else None, n, ref(k), ref(prm),
                                     api._p(E), api._p(mask), C.byref(ninl), C.byref(key))

    def run_zeroed():
        return not E.any() and not mask[:nz[0]].any() and (mask[nz[0]:] == 7).all() and ninl.value == 0 and key.value == 0

    assert refused(run(prm=None), INV, b"params is null") and run_zeroed()
    for prm in (empty, neg, high):
        assert refused(run(prm=prm), INV, b"sample ids must") and run_zeroed()
    assert refused(run(prm=wide), INV, b"split the range")
    assert refused(run(prm=kind), INV, b"error_kind") and run_zeroed()
    assert refused(run(k=None), INV, b"K is null") and run_zeroed()
    assert refused(run(k=cam0), INV, b"K needs") and refused(run(k=caminf), INV, b"K needs")
    assert refused(run(prm=thr0), INV, b"normalised threshold") and refused(run(prm=thrnan), INV, b"normalised threshold")
    assert refused(run(pts=False), INV, b"bad point arrays") and refused(run(n=-1), INV, b"bad point arrays")
    assert refused(run(n=4), FEW, b"need at least 5") and run_zeroed()
    assert refused(run(n=0), FEW, b"need at least 5") and refused(run(n=0, pts=False), FEW, b"need at least 5")
    # the order: params (null, range, kind), K (null, values, threshold), point arrays, n < 5, ctx
    assert refused(run(prm=None, k=None), INV, b"params is null")
    assert refused(run(prm=wide, k=None), INV, b"split the range")
    assert refused(run(prm=kind, k=cam0), INV, b"error_kind")
    assert refused(run(prm=thr0, k=cam0), INV, b"K needs")
    assert refused(run(prm=thr0, pts=False), INV, b"normalised threshold")
    assert refused(run(pts=False, n=4), INV, b"bad point arrays")
    assert refused(run(n=5), INV, b"ctx is null") and run_zeroed()      # ctx last: everything else passed

    # ---- pm_ransac_essential_from_hyp: hyp, params, then as above with the candidates' outputs before the point arrays
    def hyp(prm=good, h=0, k=cam, n=10, pts=True, e=E90, cnt=counts):
        poison(n)
        return L.pm_ransac_essential_from_hyp(None, api._p(xy) if pts else None, api._p(xy) if pts else None, n, ref(k),
                                              ref(prm), C.c_int64(h), api._p(e), api._p(cnt), C.byref(nm))

    def hyp_zeroed():
        return not E90.any() and (counts == -1).all() and nm.value == 0

    for h in (-1, (1 << 32) // 10):
        assert refused(hyp(h=h), INV, b"sample id must") and hyp_zeroed()
    assert refused(hyp(prm=None), INV, b"params is null") and hyp_zeroed()
    assert refused(hyp(prm=kind), INV, b"error_kind") and hyp_zeroed()
    assert refused(hyp(k=None), INV, b"K is null") and refused(hyp(k=cam0), INV, b"K needs")
    assert refused(hyp(prm=thr0), INV, b"normalised threshold")
    assert refused(hyp(e=None), INV, b"null E or counts") and (counts == -1).all() and nm.value == 0
    assert refused(hyp(cnt=None), INV, b"null E or counts") and not E90.any()
    assert refused(hyp(pts=False), INV, b"bad point arrays")
    assert refused(hyp(n=4), FEW, b"need at least 5") and hyp_zeroed()
    assert refused(hyp(h=-1, prm=None), INV, b"sample id must")
    assert refused(hyp(prm=None, k=None), INV, b"params is null")
    assert refused(hyp(prm=kind, k=None), INV, b"error_kind")
    assert refused(hyp(k=cam0, e=None), INV, b"K needs")
    assert refused(hyp(e=None, pts=False), INV, b"null E or counts")
    assert refused(hyp(pts=False, n=4), INV, b"bad point arrays")
    assert refused(hyp(prm=empty, h=(1 << 32) // 10 - 1, n=5), INV, b"ctx is null") and hyp_zeroed()   # p's own range is unused

    # ---- pm_ransac_essential_run_dev: outputs, mask_len, params, K, view, ctx
    view = api.PointsView(1, 1, None, 1, 10, 0, 1, 0)
    d = C.c_void_p(16)                                           # never dereferenced: the calls fail before any launch

    def dev(v=view, k=cam, prm=good, outs=(d, d, d, d), mask_len=10):
        return L.pm_ransac_essential_run_dev(None, ref(v), ref(k), ref(prm), outs[0], outs[1], outs[2], mask_len, outs[3])

    for i in range(4):
        assert refused(dev(outs=tuple(None if j == i else d for j in range(4))), INV, b"null argument")
    assert refused(dev(mask_len=-1), INV, b"mask_len")
    assert refused(dev(prm=None), INV, b"params is null")
    assert refused(dev(prm=empty), INV, b"sample ids must") and refused(dev(prm=high), INV, b"sample ids must")
    assert refused(dev(prm=wide), INV, b"split the range")
    assert refused(dev(prm=kind), INV, b"error_kind")
    assert refused(dev(k=None), INV, b"K is null") and refused(dev(k=cam0), INV, b"K needs")
    assert refused(dev(prm=thr0), INV, b"normalised threshold")
    assert refused(dev(v=None), INV, b"null correspondence view")
    assert refused(dev(v=api.PointsView(None, 1, None, 1, 10, 0, 1, 0)), INV, b"null correspondence view")
    assert refused(dev(v=api.PointsView(1, 1, None, 0, 10, 0, 1, 0)), INV, b"need 1 <= parts")
    assert refused(dev(v=api.PointsView(1, 1, None, 1, 0, 0, 1, 0)), INV, b"need 1 <= parts")
    assert refused(dev(v=api.PointsView(1, 1, None, 2, 10, 19, 1, 0)), INV, b"pitch_xy smaller")
    assert refused(dev(outs=(None, d, d, d), mask_len=-1), INV, b"null argument")
    assert refused(dev(mask_len=-1, prm=None), INV, b"mask_len")
    assert refused(dev(prm=kind, k=None), INV, b"error_kind")
    assert refused(dev(prm=thr0, v=None), INV, b"normalised threshold")
    assert refused(dev(mask_len=0), INV, b"ctx is null")
    assert refused(dev(), INV, b"ctx is null")

    # ---- pm_recover_pose: K, E, dist, point arrays (mask_in may be null), n < 5, ctx
    def pose(k=cam, e=Ein, mi=m, dist=50.0, n=10, pts=True, p4=pts4):
        poison(n)
        return L.pm_recover_pose(None, api._p(xy) if pts else None, api._p(xy) if pts else None, n, ref(k), api._p(e),
                                 api._p(mi), C.c_double(dist), api._p(Rm), api._p(t), api._p(mask), C.byref(ng), api._p(p4))

    def pose_zeroed():
        return (not Rm.any() and not t.any() and not mask[:nz[0]].any() and ng.value == 0 and not pts4[:nz[0]].any() and
                (pts4[nz[0]:] == 7).all())

    assert refused(pose(k=None), INV, b"K is null") and pose_zeroed()
    assert refused(pose(k=cam0), INV, b"K needs") and refused(pose(k=caminf), INV, b"K needs")
    assert refused(pose(e=None), INV, b"null E") and pose_zeroed()
    for dist in (0.0, -1.0, float("nan")):
        assert refused(pose(dist=dist), INV, b"dist must") and pose_zeroed()
    assert refused(pose(pts=False), INV, b"bad point arrays") and refused(pose(n=-1), INV, b"bad point arrays")
    assert refused(pose(n=4), FEW, b"need at least 5") and pose_zeroed()
    assert refused(pose(k=cam0, dist=0.0), INV, b"K needs")
    assert refused(pose(k=None, e=None), INV, b"K is null")
    assert refused(pose(e=None, dist=0.0), INV, b"null E")
    assert refused(pose(dist=0.0, n=4), INV, b"dist must")
    assert refused(pose(dist=0.0, pts=False), INV, b"dist must")
    assert refused(pose(pts=False, n=4), INV, b"bad point arrays")
    assert refused(pose(mi=None, p4=None), INV, b"ctx is null")         # the input mask and the points are optional
    assert refused(pose(n=5), INV, b"ctx is null") and pose_zeroed()

    # ---- pm_recover_pose_dev: required pointers (mask_in and points4 optional), K, dist, view, ctx
    def posed(v=view, k=cam, args=(d, d, d, d, d, d, d), dist=50.0):
        e, mi, r, tt, mo, g, p4 = args
        return L.pm_recover_pose_dev(None, ref(v), ref(k), e, mi, C.c_double(dist), r, tt, mo, g, p4)

    for i in (0, 2, 3, 4, 5):
        assert refused(posed(args=tuple(None if j == i else d for j in range(7))), INV, b"null argument")
    assert refused(posed(k=None), INV, b"K is null") and refused(posed(k=cam0), INV, b"K needs")
    assert refused(posed(dist=0.0), INV, b"dist must")
    assert refused(posed(v=None), INV, b"null correspondence view")
    assert refused(posed(v=api.PointsView(1, 1, None, 65, 10, 20, 1, 0)), INV, b"need 1 <= parts")
    assert refused(posed(args=(None, d, d, d, d, d, d), k=None), INV, b"null argument")
    assert refused(posed(k=cam0, dist=0.0), INV, b"K needs")
    assert refused(posed(dist=0.0, v=None), INV, b"dist must")
    assert refused(posed(args=(d, None, d, d, d, d, None)), INV, b"ctx is null")
    assert refused(posed(), INV, b"ctx is null")

    # ---- pm_estimate_pose: params, K, dist, point arrays, n < 5, ctx
    def est(prm=good, k=cam, dist=50.0, n=10, pts=True):
        poison(n)
        return L.pm_estimate_pose(None, api._p(xy) if pts else None, api._p(xy) if pts else None, n, ref(k), ref(prm),
                                  C.c_double(dist), api._p(E), api._p(Rm), api._p(t), api._p(mask), C.byref(ninl),
                                  C.byref(ng), C.byref(key))

    def est_zeroed():
        return run_zeroed() and not Rm.any() and not t.any() and ng.value == 0

    assert refused(est(prm=None), INV, b"params is null") and est_zeroed()
    assert refused(est(prm=empty), INV, b"sample ids must") and refused(est(prm=wide), INV, b"split the range")
    assert refused(est(prm=kind), INV, b"error_kind")
    assert refused(est(k=None), INV, b"K is null") and refused(est(k=cam0), INV, b"K needs") and est_zeroed()
    assert refused(est(prm=thr0), INV, b"normalised threshold")
    assert refused(est(dist=0.0), INV, b"dist must") and est_zeroed()
    assert refused(est(pts=False), INV, b"bad point arrays")
    assert refused(est(n=4), FEW, b"need at least 5") and est_zeroed()
    assert refused(est(prm=kind, k=cam0), INV, b"error_kind")
    assert refused(est(k=cam0, dist=0.0), INV, b"K needs")
    assert refused(est(prm=thr0, dist=0.0), INV, b"normalised threshold")
    assert refused(est(dist=0.0, n=4), INV, b"dist must")
    assert refused(est(pts=False, n=4), INV, b"bad point arrays")
    assert refused(est(n=5), INV, b"ctx is null") and est_zeroed()
