"""ctypes loader of tests/triangulate_ref.c, the plain-C restatement of docs/SPEC.md S93-S96 (triangulation from 2 .. 8
posed views: observations, linear DLT, LM over the point, gates), plus the numpy scenes and the independent float64 numpy
evaluation the two test files share.  Built on first use by cref.py.  K is (fx, fy, cx, cy); a pose is 12 doubles, R
row-major then t, with x_cam = R X + t, or None for [I|0]."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p

OK, FEW_VIEWS, DEGENERATE, DEPTH, PARALLAX, REPROJ = range(6)
USE_INITIAL = 1
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = cref.load("triangulate_ref", {
            "tr_max_views": [], "tr_use_initial": [],
            "tr_rows": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p],
            "tr_run": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8,
        })
    return _lib


def _views(uv, Rt):
    uv = [np.ascontiguousarray(u, np.float32).reshape(-1, 2) for u in uv]
    poses = [None if r is None else np.ascontiguousarray(r, np.float64).reshape(12) for r in Rt]
    assert len(uv) == len(poses) and all(u.shape[0] == uv[0].shape[0] for u in uv)
    up = (C.c_void_p * len(uv))(*[_p(u) for u in uv])
    rp = (C.c_void_p * len(uv))(*[(_p(r) if r is not None else None) for r in poses])
    return uv, poses, up, rp


def rows(K, uv, Rt, i):
    """The 2V x 4 DLT system of point i (S94)."""
    uv, poses, up, rp = _views(uv, Rt)
    A = np.zeros((2 * len(uv), 4))
    lib().tr_rows(_p(np.ascontiguousarray(K, np.float64).reshape(4)), up, rp, len(uv), i, _p(A))
    return A


class Result:
    pass


def run(K, uv, Rt, max_reproj_px=3.0, max_cos_parallax=0.9998, max_depth=np.inf, max_iters=10, flags=0, xyz0=None):
    """S93-S96 over all points: a Result with xyz (n, 3) f32, status, points4 (n, 4) f32, err2 f32, n_good, and the extras
    cost_lin, cost_fin (float64), iters (LM passes at trial points) and xyz64 (the final point before the f32 rounding)."""
    uv, poses, up, rp = _views(uv, Rt)
    n = uv[0].shape[0]
    m = max(n, 1)
    r = Result()
    r.xyz = np.zeros((m, 3), np.float32)
    if xyz0 is not None:
        r.xyz[:n] = np.asarray(xyz0, np.float32).reshape(-1, 3)
    r.status, r.points4, r.err2 = np.zeros(m, np.uint8), np.zeros((m, 4), np.float32), np.zeros(m, np.float32)
    r.cost_lin, r.cost_fin, r.iters, r.xyz64 = np.zeros(m), np.zeros(m), np.zeros(m, np.int32), np.zeros((m, 3))
    prm = np.array([max_reproj_px, max_cos_parallax, max_depth], np.float64)
    r.n_good = lib().tr_run(_p(np.ascontiguousarray(K, np.float64).reshape(4)), up, rp, len(uv), n, _p(prm), max_iters, flags,
                            _p(r.xyz), _p(r.status), _p(r.points4), _p(r.err2), _p(r.cost_lin), _p(r.cost_fin), _p(r.iters),
                            _p(r.xyz64))
    for k in ("xyz", "status", "points4", "err2", "cost_lin", "cost_fin", "iters", "xyz64"):
        setattr(r, k, getattr(r, k)[:n])
    return r


# ---- scenes (numpy only, in the style of synth.pnp_scene) ---------------------------------------------------------------

def _rot(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(K, Rt, X):
    """float64 pixels and depths of world points X (n, 3) under the pose Rt (12 doubles or None)."""
    Rm, t = (np.eye(3), np.zeros(3)) if Rt is None else (np.asarray(Rt[:9]).reshape(3, 3), np.asarray(Rt[9:]))
    with np.errstate(invalid="ignore", divide="ignore"):
        Xc = X @ Rm.T + t
        return np.c_[K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], Xc[:, 2]


def scene(n, n_views, seed, noise_px=0.5, blank_frac=0.0, swap_every=0, first_identity=True, width=993, height=660):
    """n world points at depths 4-12 in front of camera 0, seen by n_views cameras that sit up to ~1.5 units to the side and
    turn up to ~6 degrees, plus N(0, noise_px) on every pixel.  blank_frac of the observations become NaN rows (not seen);
    with swap_every = k, every k-th track has the pixel of one view (not view 0) replaced by a uniform-random one.
    Returns K (4), uv (list of (n, 2) f32), Rt (list of 12 doubles; the first is None with first_identity), X (n, 3) and the
    boolean flags of the swapped tracks."""
    rng = np.random.default_rng([seed, 0x7A1])
    K = np.array([rng.uniform(700, 900), rng.uniform(750, 950), width / 2.0 + rng.uniform(-40, 40), height / 2.0 + rng.uniform(-30, 30)])
    px = rng.uniform([0.1 * width, 0.1 * height], [0.9 * width, 0.9 * height], (n, 2))
    z = rng.uniform(4.0, 12.0, n)
    X = np.c_[(px[:, 0] - K[2]) / K[0] * z, (px[:, 1] - K[3]) / K[1] * z, z]
    Rt = [None if first_identity else np.r_[np.eye(3).reshape(-1), np.zeros(3)]]
    for v in range(1, n_views):
        w = rng.normal(size=3)
        w *= rng.uniform(0.02, 0.1) / np.linalg.norm(w)
        a = 2 * np.pi * (v + rng.uniform(-0.3, 0.3)) / max(n_views - 1, 1)
        c = np.array([np.cos(a), 0.6 * np.sin(a), rng.uniform(-0.15, 0.15)]) * rng.uniform(0.8, 1.5)
        if n_views == 2:
            c = np.array([1.0, rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)])
        Rm = _rot(w)
        Rt.append(np.r_[Rm.reshape(-1), -Rm @ c])
    uv = []
    for v in range(n_views):
        p, _ = project(K, Rt[v], X)
        uv.append(p + rng.normal(0, noise_px, (n, 2)))
    swapped = np.zeros(n, bool)
    if swap_every:
        swapped[::swap_every] = True
        for i in np.nonzero(swapped)[0]:
            uv[1 + rng.integers(0, n_views - 1)][i] = rng.uniform([0, 0], [width, height])
    if blank_frac:
        for v in range(n_views):
            uv[v][rng.random(n) < blank_frac] = np.nan
    return K, [np.ascontiguousarray(u.astype(np.float32)) for u in uv], Rt, X, swapped


# ---- independent float64 numpy evaluation ----------------------------------------------------------------------------------

def observed(K, uv):
    """(n_views, n) bool: S93's rule in float64 (the f32 rounding of S31 cannot move a pixel across 2^20 focal lengths here)."""
    out = []
    for u in uv:
        xn = np.c_[(u[:, 0].astype(np.float64) - K[2]) / K[0], (u[:, 1].astype(np.float64) - K[3]) / K[1]]
        with np.errstate(invalid="ignore"):
            out.append(np.isfinite(xn).all(1) & (np.abs(xn) <= 2.0 ** 20).all(1))
    return np.array(out)


def np_linear(K, uv, Rt, i, obs):
    """The SVD null vector of point i's rows over its observing views, from float64 normalised pixels."""
    A = []
    for v in np.nonzero(obs[:, i])[0]:
        P = np.c_[np.eye(3), np.zeros(3)] if Rt[v] is None else np.c_[np.asarray(Rt[v][:9]).reshape(3, 3), np.asarray(Rt[v][9:])]
        x = (float(uv[v][i, 0]) - K[2]) / K[0]
        y = (float(uv[v][i, 1]) - K[3]) / K[1]
        A += [x * P[2] - P[0], y * P[2] - P[1]]
    return np.linalg.svd(np.array(A))[2][-1]


def np_errors(K, uv, Rt, X, obs):
    """Per view and point: squared pixel error and depth at X (n, 3), float64; NaN where the view does not observe."""
    e, z = np.full(obs.shape, np.nan), np.full(obs.shape, np.nan)
    for v in range(len(uv)):
        p, d = project(K, Rt[v], X)
        r = p - uv[v].astype(np.float64)
        e[v], z[v] = np.where(obs[v], (r * r).sum(1), np.nan), np.where(obs[v], d, np.nan)
    return e, z


def np_min_cos(Rt, X, obs):
    """Smallest cosine between the rays X - C_v of two observing views, per point (1 where there is no pair)."""
    n = X.shape[0]
    rays = []
    for r in Rt:
        c = np.zeros(3) if r is None else -np.asarray(r[:9]).reshape(3, 3).T @ np.asarray(r[9:])
        d = X - c
        rays.append(d / np.linalg.norm(d, axis=1, keepdims=True))
    out = np.ones(n)
    for a in range(len(Rt)):
        for b in range(a + 1, len(Rt)):
            both = obs[a] & obs[b]
            out = np.where(both, np.minimum(out, (rays[a] * rays[b]).sum(1)), out)
    return out


def np_gates(K, uv, Rt, X, obs, max_reproj_px, max_cos_parallax, max_depth):
    """Statuses DEPTH / PARALLAX / REPROJ / OK of the points X by S96's order, float64, and each gate's margin: the
    smallest relative distance of a tested quantity to its threshold (for the tests' "no point near a threshold")."""
    e, z = np_errors(K, uv, Rt, X, obs)
    with np.errstate(invalid="ignore"):
        zmin, zmax, emax = np.nanmin(z, 0), np.nanmax(z, 0), np.nanmax(e, 0)
    mc = np_min_cos(Rt, X, obs)
    st = np.full(X.shape[0], OK)
    st[~(emax <= max_reproj_px ** 2)] = REPROJ
    if max_cos_parallax < 1:
        st[~(mc < max_cos_parallax)] = PARALLAX
    st[~((zmin > 0) & (zmax < max_depth))] = DEPTH
    margin = np.minimum(np.abs(emax / max_reproj_px ** 2 - 1), np.abs(zmin) / np.maximum(zmax, 1e-300))
    if np.isfinite(max_depth):
        margin = np.minimum(margin, np.abs(zmax / max_depth - 1))
    if max_cos_parallax < 1:
        margin = np.minimum(margin, np.abs(mc - max_cos_parallax) / abs(max_cos_parallax))
    return st, margin


def np_refine(K, uv, Rt, X0, obs_i, i, iters=30):
    """Damped Gauss-Newton over one point in float64 numpy (numeric structure independent of S95: full numpy solves,
    lambda on the diagonal), accept-only."""
    views = np.nonzero(obs_i)[0]

    def res(X):
        r, J = [], []
        for v in views:
            Rm, t = (np.eye(3), np.zeros(3)) if Rt[v] is None else (np.asarray(Rt[v][:9]).reshape(3, 3), np.asarray(Rt[v][9:]))
            xc = Rm @ X + t
            if not xc[2] > 0:
                return None, None
            r += [K[0] * xc[0] / xc[2] + K[2] - float(uv[v][i, 0]), K[1] * xc[1] / xc[2] + K[3] - float(uv[v][i, 1])]
            J += [K[0] * (Rm[0] - xc[0] / xc[2] * Rm[2]) / xc[2], K[1] * (Rm[1] - xc[1] / xc[2] * Rm[2]) / xc[2]]
        return np.array(r), np.array(J)

    X = np.array(X0, np.float64)
    r, J = res(X)
    if r is None:
        return X
    lam = 1e-3
    for _ in range(iters):
        H = J.T @ J
        try:
            d = np.linalg.solve(H + lam * np.diag(np.diag(H)), -J.T @ r)
        except np.linalg.LinAlgError:
            break
        rt, Jt = res(X + d)
        if rt is not None and rt @ rt < r @ r:
            X, r, J, lam = X + d, rt, Jt, lam / 10
        else:
            lam *= 10
    return X


def np_pipeline(K, uv, Rt, max_reproj_px, max_cos_parallax, max_depth):
    """The numpy reference alone: SVD start, damped steps, gates.  Returns (X (n, 3), status, margin)."""
    obs = observed(K, uv)
    n = uv[0].shape[0]
    X = np.zeros((n, 3))
    for i in range(n):
        q = np_linear(K, uv, Rt, i, obs)
        X[i] = np_refine(K, uv, Rt, q[:3] / q[3], obs[:, i], i)
    st, margin = np_gates(K, uv, Rt, X, obs, max_reproj_px, max_cos_parallax, max_depth)
    return X, st, margin


# the recovery test of both files: 5 views, 0.5 px noise, every tenth track with one view's pixel replaced
RECOVERY = dict(n=300, n_views=5, seeds=(0, 1), max_reproj_px=3.0, max_cos_parallax=0.9998)


def recovery_scene(seed):
    return scene(RECOVERY["n"], RECOVERY["n_views"], seed, noise_px=0.5, swap_every=10)


def clean_scene(n_views):
    """2500 tracks without pixel noise (f32 rounding of the pixels only), ~10 % of the observations blanked: the scene of the
    second-pass tests."""
    return scene(2500, n_views, 60 + n_views, noise_px=0.0, blank_frac=0.1)


def settled(r, max_iters, n_views):
    """Rows of a run whose re-refinement from their own f32 output must reproduce that output bit for bit (the
    PM_TRI_USE_INITIAL tests): PM_TRI_OK, LM stopped by itself, and every coordinate of the final fp64 point further from the
    nearest f32 rounding boundary than the noise of LM's stop.  Why a margin at all: the second pass starts up to half an f32
    spacing off the optimum, moves back to it and stops where the cost no longer changes in fp64 — a point that differs from
    the first pass's by the noise of that stop, not by zero.  The noise, for the scenes of scene(): a residual is the
    difference of two pixel-sized numbers (below 1024, fp64 spacing 2^-43), so it carries up to dr = 4 * 2^-43 of rounding;
    the cost c = sum r^2 over 2V residuals then moves by up to dc = 2 sqrt(2V c) dr (Cauchy-Schwarz) without the point
    moving, and LM cannot tell points apart whose costs differ by less: it stops within d, H d^2 / 2 = dc.  Along the ray
    the curvature is lowest, H >= (f b / z^2)^2 >= (700 * 0.8 / 144)^2 ~ 15 px^2/unit^2 from one other view; across it
    H >= 2 (f / z)^2 >= 6800.  So |dZ| <= sqrt(2 dc / 15) and |dX_j| <= |X_j / Z| |dZ| + sqrt(2 dc / 6800).  A bound, not an
    estimate: on tracks with 0.5 px noise it leaves few rows, on clean tracks (c ~ 1e-9 px^2) nearly all."""
    x = r.xyz64
    f = x.astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dc = 2.0 * np.sqrt(2 * n_views * r.cost_fin) * 4 * 2.0 ** -43
        dz = np.sqrt(2 * dc / 15.0)
        m = np.abs(x / x[:, 2:3]) * dz[:, None] + np.sqrt(2 * dc / 6800.0)[:, None]
        sp = np.spacing(np.abs(f).astype(np.float32)).astype(np.float64)
        away = (0.5 * sp - np.abs(x - f) > m).all(1)
    return (r.status == OK) & (r.iters < max_iters) & away
