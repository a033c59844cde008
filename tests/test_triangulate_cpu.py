"""CPU: the plain-C restatement of triangulation (tests/triangulate_ref.c, docs/SPEC.md S93-S96) against numpy — its linear
point against the SVD null vector, cost ordering, zero-row invariance, every per-point status by a constructed input, the
gates against an independent float64 evaluation, the numpy reference alone on the recovery scenes of the GPU file, the
re-refinement rule — and the surface of pm_triangulate* (prototypes, exports, every PM_E_INVALID without a device)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import triangulate_ref as T
from points_matching_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K0 = np.array([800.0, 800.0, 320.0, 240.0])                 # principal point exact in f32
EYE = np.r_[np.eye(3).reshape(-1), np.zeros(3)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def _pose(Rm, c):
    """The pose of a camera with rotation Rm at centre c."""
    return np.r_[np.asarray(Rm, np.float64).reshape(-1), -np.asarray(Rm) @ np.asarray(c, np.float64)]


def _pix(K, Rt, X):
    return T.project(K, Rt, np.atleast_2d(np.asarray(X, np.float64)))[0].astype(np.float32)


@pytest.mark.parametrize("n_views", [2, 3, 5, 8])
def test_linear_point_reprojects_like_the_svd_null_vector(n_views):
    # largest difference observed over these 16 scenes (4 seeds x 4 view counts, 200 points each): 2.52e-5 px — the f32
    # rounding of S31's normalised coordinates (2^-24 * 800 px = 4.8e-5 px), which the float64 SVD does not make.  Bound: 10 x.
    worst = 0.0
    for seed in range(4):
        K, uv, Rt, X, _ = T.scene(200, n_views, seed, noise_px=0.5)
        r = T.run(K, uv, Rt, max_reproj_px=1e6, max_cos_parallax=1.0, max_iters=0)
        assert (r.status == T.OK).all()
        obs = T.observed(K, uv)
        Xs = np.array([q[:3] / q[3] for q in (T.np_linear(K, uv, Rt, i, obs) for i in range(200))])
        for v in range(n_views):
            worst = max(worst, np.abs(T.project(K, Rt[v], Xs)[0] - T.project(K, Rt[v], r.xyz64)[0]).max())
    print("n_views %d: linear vs SVD %.3g px" % (n_views, worst))
    assert worst <= 2.6e-4, worst


@pytest.mark.parametrize("n_views", [2, 3, 5, 8])
def test_refined_cost_never_above_linear_cost(n_views):
    K, uv, Rt, X, _ = T.scene(600, n_views, 21, blank_frac=0.1, swap_every=9)
    r = T.run(K, uv, Rt, max_reproj_px=1e6, max_cos_parallax=1.0, max_iters=10)
    seen = np.isfinite(r.cost_lin) | np.isinf(r.cost_lin)
    assert seen.sum() > 450 and (r.cost_fin[seen] <= r.cost_lin[seen]).all()
    assert (r.cost_fin[seen] < r.cost_lin[seen]).sum() > 300                      # and LM does move the noisy ones
    r0 = T.run(K, uv, Rt, max_reproj_px=1e6, max_cos_parallax=1.0, max_iters=0)
    assert (_bits(r0.cost_lin[seen]) == _bits(r.cost_lin[seen])).all() and (r0.iters == 0).all()
    # a point LM did not move is the linear point bit for bit
    kept = seen & (_bits(r.cost_fin) == _bits(r.cost_lin))
    assert kept.any() and (_bits(r.xyz64[kept]) == _bits(r0.xyz64[kept])).all()


@pytest.mark.parametrize("max_iters", [0, 10])
def test_zero_rows_change_no_bit(max_iters):
    """A point seen only in views {1, 3} of a 5-view call has the bits of the 2-view call with those two views."""
    K, uv, Rt, X, _ = T.scene(300, 5, 31, first_identity=False)
    blank = np.full_like(uv[0], np.nan)
    r5 = T.run(K, [blank, uv[1], blank, uv[3], blank], Rt, max_iters=max_iters)
    r2 = T.run(K, [uv[1], uv[3]], [Rt[1], Rt[3]], max_iters=max_iters)
    assert (r2.status == T.OK).sum() > 250
    for k in ("xyz", "points4", "err2", "xyz64", "cost_lin", "cost_fin"):
        assert (_bits(getattr(r5, k)) == _bits(getattr(r2, k))).all(), k
    assert (r5.status == r2.status).all() and (r5.iters == r2.iters).all() and r5.n_good == r2.n_good
    # and the rows of the blanked views are zero, the others the 2-view call's
    A5, A2 = T.rows(K, [blank, uv[1], blank, uv[3], blank], Rt, 7), T.rows(K, [uv[1], uv[3]], [Rt[1], Rt[3]], 7)
    assert not A5[[0, 1, 4, 5, 8, 9]].any() and (A5[[2, 3, 6, 7]] == A2).all()


def test_every_status_is_reached_by_a_constructed_input():
    X = np.array([0.4, -0.3, 8.0])
    side = _pose(np.eye(3), [1.0, 0.0, 0.0])
    nan2 = np.full((1, 2), np.nan, np.float32)
    # one observation only
    r = T.run(K0, [_pix(K0, None, X), nan2, nan2], [None, side, side])
    assert r.status[0] == T.FEW_VIEWS and np.isnan(r.xyz).all() and np.isnan(r.err2).all() and r.n_good == 0
    # a point at infinity: the principal ray of two cameras that look the same way from different centres
    pp = np.array([[320.0, 240.0]], np.float32)
    r = T.run(K0, [pp, pp], [None, side])
    assert r.status[0] == T.DEGENERATE and r.points4[0, 3] == 0.0 and np.isnan(r.xyz).all()
    # a point behind both cameras (its pixels are those of the mirrored point in front)
    B = np.array([0.4, -0.3, -8.0])
    r = T.run(K0, [_pix(K0, None, B), _pix(K0, side, B)], [None, side])
    assert r.status[0] == T.DEPTH and r.xyz64[0, 2] < 0 and np.isnan(r.xyz).all()
    # two cameras at the same centre, max_cos_parallax 0.9998: the linear system has no depth (its null vector is the common
    # centre, which the depth gate refuses) ...
    turn = _pose(T._rot(np.array([0.0, 0.05, 0.0])), [0.0, 0.0, 0.0])
    r = T.run(K0, [_pix(K0, None, X), _pix(K0, turn, X)], [None, turn], max_cos_parallax=0.9998)
    assert r.status[0] == T.DEPTH
    # ... from a given start the point stays on the ray and fails the parallax gate; so does the linear point of two centres
    # 1 mm apart at depth 8 (cos = 1 - 8e-9)
    r = T.run(K0, [_pix(K0, None, X), _pix(K0, turn, X)], [None, turn], max_cos_parallax=0.9998, flags=T.USE_INITIAL, xyz0=[X])
    assert r.status[0] == T.PARALLAX
    near = _pose(T._rot(np.array([0.0, 0.05, 0.0])), [1e-3, 0.0, 0.0])
    r = T.run(K0, [_pix(K0, None, X), _pix(K0, near, X)], [None, near], max_cos_parallax=0.9998)
    assert r.status[0] == T.PARALLAX and abs(r.xyz64[0, 2] - 8.0) < 0.5
    assert T.run(K0, [_pix(K0, None, X), _pix(K0, near, X)], [None, near], max_cos_parallax=1.0).status[0] == T.OK
    # a pixel moved by 20 px in one of three views
    up = _pose(np.eye(3), [0.0, 1.0, 0.0])
    uv = [_pix(K0, None, X), _pix(K0, side, X), _pix(K0, up, X)]
    assert T.run(K0, uv, [None, side, up]).status[0] == T.OK
    uv[1] = uv[1] + np.float32([20.0, 0.0])
    r = T.run(K0, uv, [None, side, up], max_reproj_px=3.0)
    assert r.status[0] == T.REPROJ and np.isnan(r.xyz).all() and np.isnan(r.err2).all()
    # a non-finite start under PM_TRI_USE_INITIAL
    uv[1] = _pix(K0, side, X)
    r = T.run(K0, uv, [None, side, up], flags=T.USE_INITIAL, xyz0=[[np.nan, 0.0, 1.0]])
    assert r.status[0] == T.DEGENERATE


@pytest.mark.parametrize("n_views,max_cos,max_depth,seed", [(2, 0.9985, 10.0, 3), (3, 0.9998, np.inf, 4), (5, 0.997, 11.0, 5),
                                                           (8, 0.9998, 9.0, 6), (4, 1.0, np.inf, 7)])
def test_statuses_equal_an_independent_float64_evaluation(n_views, max_cos, max_depth, seed):
    K, uv, Rt, X, _ = T.scene(400, n_views, seed, blank_frac=0.1, swap_every=7)
    r = T.run(K, uv, Rt, 3.0, max_cos, max_depth, 10)
    obs = T.observed(K, uv)
    assert ((obs.sum(0) < 2) == (r.status == T.FEW_VIEWS)).all() and not (r.status == T.DEGENERATE).any()
    ev = r.status != T.FEW_VIEWS
    st, margin = T.np_gates(K, [u[ev] for u in uv], Rt, r.xyz64[ev], obs[:, ev], 3.0, max_cos, max_depth)
    assert margin.min() > 1e-6, margin.min()                    # no point within 1e-6 relative of a threshold
    assert (st == r.status[ev]).all()
    assert r.n_good == (r.status == T.OK).sum() and (np.isnan(r.xyz).all(1) == (r.status != T.OK)).all()
    e, _ = T.np_errors(K, uv, Rt, r.xyz64, obs)
    ok = r.status == T.OK
    assert np.allclose(r.err2[ok], np.nanmax(e[:, ok], 0), rtol=1e-6) and np.isnan(r.err2[~ok]).all()
    assert len(np.unique(r.status)) >= 3


@pytest.mark.parametrize("seed", T.RECOVERY["seeds"])
def test_numpy_reference_alone_separates_the_recovery_scenes(seed):
    """The GPU file's recovery test asserts: every untouched track PM_TRI_OK, every touched one not.  The numpy reference
    (SVD start, damped steps, float64 gates) alone meets both on these seeds, away from every threshold; the restatement agrees."""
    K, uv, Rt, X, touched = T.recovery_scene(seed)
    Xn, st, margin = T.np_pipeline(K, uv, Rt, T.RECOVERY["max_reproj_px"], T.RECOVERY["max_cos_parallax"], np.inf)
    assert touched.sum() == 30 and (st[~touched] == T.OK).all() and (st[touched] != T.OK).all()
    assert margin.min() > 1e-6
    e, _ = T.np_errors(K, uv, Rt, Xn, T.observed(K, uv))
    worst = np.sqrt(np.nanmax(e, 0))
    print("seed %d: untouched <= %.2f px, touched >= %.1f px" % (seed, worst[~touched].max(), worst[touched].min()))
    r = T.run(K, uv, Rt, T.RECOVERY["max_reproj_px"], T.RECOVERY["max_cos_parallax"], np.inf, 10)
    assert (r.status == st).all() and np.abs(r.xyz64[st == T.OK] - Xn[st == T.OK]).max() < 1e-6


@pytest.mark.parametrize("n_views", [2, 5])
def test_second_pass_over_its_own_output_keeps_settled_rows(n_views):
    """On clean tracks (no pixel noise: LM's stop is sharp, see triangulate_ref.settled) nearly every row is settled, LM still
    takes steps from the f32-rounded start, and the f32 output comes back bit for bit.  With 0.5 px noise the same rule holds
    on the few rows it admits (measured here: 6 of 2046 and 3 of 2500 PM_TRI_OK rows outside it change their last bits)."""
    K, uv, Rt, X, _ = T.clean_scene(n_views)
    r = T.run(K, uv, Rt, max_iters=100)
    s = T.settled(r, 100, n_views)
    r2 = T.run(K, uv, Rt, max_iters=100, flags=T.USE_INITIAL, xyz0=r.xyz)
    assert s.sum() > 1900 and (r2.status[s] == T.OK).all() and (r2.cost_fin[s] < r2.cost_lin[s]).sum() > 1900
    assert (_bits(r2.xyz[s]) == _bits(r.xyz[s])).all()
    assert not r2.points4.any()                                # not written under PM_TRI_USE_INITIAL
    Kn, uvn, Rtn, Xn, _ = T.scene(2500, n_views, 40 + n_views, blank_frac=0.1)
    rn = T.run(Kn, uvn, Rtn, max_iters=100)
    sn = T.settled(rn, 100, n_views)
    rn2 = T.run(Kn, uvn, Rtn, max_iters=100, flags=T.USE_INITIAL, xyz0=rn.xyz)
    assert (_bits(rn2.xyz[sn]) == _bits(rn.xyz[sn])).all()
    # no step at all (max_iters 0): every PM_TRI_OK row comes back bit for bit
    r3 = T.run(Kn, uvn, Rtn, max_iters=0, flags=T.USE_INITIAL, xyz0=rn.xyz)
    ok = r3.status == T.OK
    assert ok.sum() > 1500 and (_bits(r3.xyz[ok]) == _bits(rn.xyz[ok])).all()


# ---- the surface ------------------------------------------------------------------------------------------------------------

ARITY = {"pm_triangulate_dev": 9, "pm_triangulate": 12}


def test_surface():
    hdr = open(os.path.join(ROOT, "include", "pm.h")).read()
    for name, arity in ARITY.items():
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == arity, name
        assert name in api.EXPORTS
    r = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    syms = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    assert not [n for n in ARITY if n not in syms]
    assert re.search(r"#define PM_TRI_MAX_VIEWS\s+8\b", hdr) and re.search(r"#define PM_TRI_USE_INITIAL\s+1\b", hdr)
    assert api.PM_TRI_MAX_VIEWS == T.lib().tr_max_views() == 8 and api.PM_TRI_USE_INITIAL == T.USE_INITIAL == T.lib().tr_use_initial()
    m = re.search(r"enum \{ (PM_TRI_OK[^}]*) \};", hdr)
    names = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(",")))
    assert names == {"PM_TRI_OK": T.OK, "PM_TRI_FEW_VIEWS": T.FEW_VIEWS, "PM_TRI_DEGENERATE": T.DEGENERATE, "PM_TRI_DEPTH": T.DEPTH,
                     "PM_TRI_PARALLAX": T.PARALLAX, "PM_TRI_REPROJ": T.REPROJ}
    assert all(getattr(api, k) == v for k, v in names.items())
    assert C.sizeof(api.TriViews) == 8 * 8 * 2 + 8 + 8 and C.sizeof(api.TriParams) == 32
    assert api.TriViews.count.offset == 128 and api.TriViews.n_views.offset == 136 and api.TriParams.max_iters.offset == 24
    p = api.tri_params()
    assert (p.max_reproj_px, p.max_cos_parallax, p.max_depth, p.max_iters, p.flags) == (3.0, 0.9998, float("inf"), 10, 0)
    v = api.tri_views([16, 32, 48], [None, 64, 0], 7, 80)
    assert (v.uv[1], v.uv[3], v.Rt[0], v.Rt[1], v.Rt[2], v.count, v.n_views, v.cap) == (32, None, None, 64, None, 80, 3, 7)
    for method in ("triangulate_dev", "triangulate"):
        assert callable(getattr(api.Context, method))


def test_library_rejects_bad_arguments_without_a_device():
    """Every PM_E_INVALID of the two forms, tripped alone with ctx = NULL (the argument checks sit before the ctx check, as
    in the other estimator calls), and the outputs untouched after each."""
    L = api.lib()
    n = 6
    uv = [np.zeros((n, 2), np.float32) for _ in range(3)]
    pose = EYE.copy()
    xyz, st, p4, e2 = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros((n, 4), np.float32), np.zeros(n, np.float32)
    ng = C.c_int()
    cam = api.Camera(800.0, 800.0, 320.0, 240.0)
    inf = float("inf")

    def poison():
        for a in (xyz, st, p4, e2):
            a[...] = 7
        ng.value = 7

    def untouched():
        return all((a == 7).all() for a in (xyz, st, p4, e2)) and ng.value == 7

    def refused(rc, frag):
        msg = L.pm_last_error()
        assert rc == api.PM_E_INVALID and frag in msg, (rc, msg)
        return untouched()

    def ref(x):
        return C.byref(x) if x is not None else None

    def host(k=cam, prm=api.tri_params(), nv=3, npts=n, views=True, poses=True, out=True, stat=True, hole=False):
        poison()
        up = (C.c_void_p * 8)(*[api._p(u) for u in uv])
        if hole:
            up[1] = None
        rp = (C.c_void_p * 8)(None, api._p(pose), api._p(pose))
        return L.pm_triangulate(None, up if views else None, rp if poses else None, nv, npts, ref(k), ref(prm),
                                api._p(xyz) if out else None, api._p(st) if stat else None, api._p(p4), api._p(e2), C.byref(ng))

    def dev(k=cam, prm=api.tri_params(), nv=3, cap=n, views=True, out=True, stat=True, hole=False):
        poison()                                                 # host arrays stand in: nothing may be touched before the refusal
        v = api.tri_views([u.ctypes.data for u in uv[:min(max(nv, 0), 3)]], [None, pose.ctypes.data, pose.ctypes.data][:min(max(nv, 0), 3)], cap)
        v.n_views = nv
        if hole:
            v.uv[1] = None
        return L.pm_triangulate_dev(None, ref(v) if views else None, ref(k), ref(prm), api._p(xyz) if out else None,
                                    api._p(st) if stat else None, api._p(p4), api._p(e2), C.byref(ng))

    for call in (host, dev):
        assert refused(call(views=False), b"null pointer")
        assert refused(call(out=False), b"null pointer") and refused(call(stat=False), b"null pointer")
        assert refused(call(k=None), b"null pointer") and refused(call(prm=None), b"null pointer")
        for nv in (-1, 0, 1, 9):
            assert refused(call(nv=nv), b"n_views outside [2, 8]")
        assert refused(call(hole=True), b"a view's uv is null")
        for bad in (api.Camera(800.0, -1.0, 320.0, 240.0), api.Camera(0.0, 800.0, 320.0, 240.0),
                    api.Camera(800.0, 800.0, 320.0, float("nan")), api.Camera(inf, 800.0, 320.0, 240.0)):
            assert refused(call(k=bad), b"K needs finite values")
        for v in (0.0, -1.0, inf, float("nan")):
            assert refused(call(prm=api.tri_params(max_reproj_px=v)), b"max_reproj_px")
        for v in (-1.0, 1.0000001, -2.0, float("nan")):
            assert refused(call(prm=api.tri_params(max_cos_parallax=v)), b"max_cos_parallax")
        for v in (0.0, -3.0, float("nan")):
            assert refused(call(prm=api.tri_params(max_depth=v)), b"max_depth")
        for v in (-1, 101):
            assert refused(call(prm=api.tri_params(max_iters=v)), b"max_iters")
        for v in (2, 3, -1):
            assert refused(call(prm=api.tri_params(flags=v)), b"unknown flag")
        # everything valid: only the context is missing
        assert refused(call(), b"ctx is null")
        assert refused(call(prm=api.tri_params(max_cos_parallax=1.0, max_depth=inf, max_iters=0, flags=1)), b"ctx is null")
    assert refused(host(poses=False), b"null pointer")
    assert refused(host(npts=-1), b"cap or n < 0") and refused(dev(cap=-1), b"cap or n < 0")
