"""ctypes loader of tests/ba_ref.c, the plain-C restatement of docs/SPEC.md S113-S117 (local bundle adjustment: joint
Levenberg-Marquardt over free poses and points through the Schur complement), plus the perturbed scenes and the independent
dense numpy solver the two test files share.  Built on first use by cref.py.  Scenes and conventions are those of
triangulate_ref.py: K is (fx, fy, cx, cy); a pose is 12 doubles, R row-major then t, x_cam = R X + t, or None for [I|0]."""
import ctypes as C

import numpy as np

import cref
import triangulate_ref as T
from cref import ptr as _p

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = cref.load("ba_ref", {
            "ba_max_views": [],
            "ba_run": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_uint] + [C.c_void_p] * 6,
        }, {"ba_run": None})
    return _lib


class Result:
    pass


def run(K, uv, Rt, xyz, fixed_mask=1, max_iters=10, gate_px=0.0):
    """S113-S117 over all rows of xyz (n, 3) f32: a Result with Rt (V, 12), xyz (n, 3) f32, used (n) u8, cost_in, cost_out,
    n_points, n_obs, iters, accepted, status, and xyz64, the final fp64 points (the f32 row's value for an unused row)."""
    uv = [np.ascontiguousarray(u, np.float32).reshape(-1, 2) for u in uv]
    poses = [None if r is None else np.ascontiguousarray(r, np.float64).reshape(12) for r in Rt]
    n, V = uv[0].shape[0], len(uv)
    assert len(poses) == V and all(u.shape[0] == n for u in uv)
    up = (C.c_void_p * V)(*[_p(u) for u in uv])
    rp = (C.c_void_p * V)(*[(_p(r) if r is not None else None) for r in poses])
    m = max(n, 1)
    r = Result()
    r.Rt = np.zeros((V, 12))
    r.xyz = np.zeros((m, 3), np.float32)
    r.xyz[:n] = np.asarray(xyz, np.float32).reshape(-1, 3)[:n]
    r.used, r.xyz64 = np.zeros(m, np.uint8), np.zeros((m, 3))
    cost, info = np.zeros(2), np.zeros(5, np.int32)
    lib().ba_run(_p(np.ascontiguousarray(K, np.float64).reshape(4)), up, rp, V, n, float(gate_px), int(max_iters), int(fixed_mask),
                 _p(r.Rt), _p(r.xyz), _p(r.used), _p(cost), _p(info), _p(r.xyz64))
    r.xyz, r.used, r.xyz64 = r.xyz[:n], r.used[:n], r.xyz64[:n]
    r.cost_in, r.cost_out = float(cost[0]), float(cost[1])
    r.n_points, r.n_obs, r.iters, r.accepted, r.status = (int(x) for x in info)
    return r


# ---- scenes ---------------------------------------------------------------------------------------------------------------

def perturbed(n, n_views, seed, fixed_mask=1, angle_deg=0.5, t_sigma=0.02, x_sigma=0.05, noise_px=0.5, blank_frac=0.1,
              swap_every=0):
    """A scene of triangulate_ref.scene() and a start for it: every free pose turned by angle_deg about a random axis (on the
    left) and its t shifted by N(0, t_sigma), every point shifted by N(0, x_sigma) and rounded to f32.  Returns K, uv, the true
    poses, the start poses, the start rows (n, 3) f32 and the true points."""
    K, uv, Rt, X, _ = T.scene(n, n_views, seed, noise_px=noise_px, blank_frac=blank_frac, swap_every=swap_every)
    rng = np.random.default_rng([seed, 0xBA])
    Rt0 = []
    for v, r in enumerate(Rt):
        if (fixed_mask >> v) & 1:
            Rt0.append(r)
            continue
        r = np.r_[np.eye(3).reshape(-1), np.zeros(3)] if r is None else r
        w = rng.normal(size=3)
        w *= np.radians(angle_deg) / np.linalg.norm(w)
        Rm = T._rot(w) @ r[:9].reshape(3, 3)
        Rt0.append(np.r_[Rm.reshape(-1), r[9:] + rng.normal(0, t_sigma, 3)])
    xyz0 = (X + rng.normal(0, x_sigma, X.shape)).astype(np.float32)
    return K, uv, Rt, Rt0, xyz0, X


def rot_err_deg(a, b):
    """Angle between the rotations of two poses (None: identity), degrees."""
    Ra = np.eye(3) if a is None else np.asarray(a[:9]).reshape(3, 3)
    Rb = np.eye(3) if b is None else np.asarray(b[:9]).reshape(3, 3)
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def t_dir_err_deg(a, b):
    ta, tb = np.asarray(a[9:]), np.asarray(b[9:])
    return np.degrees(np.arccos(np.clip(ta @ tb / (np.linalg.norm(ta) * np.linalg.norm(tb)), -1, 1)))


# ---- independent float64 numpy evaluation -----------------------------------------------------------------------------------

def _pose(r):
    return (np.eye(3), np.zeros(3)) if r is None else (np.asarray(r[:9], np.float64).reshape(3, 3), np.asarray(r[9:], np.float64))


def np_used(K, uv, Rt, xyz, gate_px=0.0):
    """The used set of S113 by a float64 numpy evaluation: bit v of byte i."""
    X = np.asarray(xyz, np.float32).astype(np.float64)
    obs = T.observed(K, uv)
    e, z = T.np_errors(K, uv, Rt, X, obs)
    with np.errstate(invalid="ignore"):
        ok = obs & np.isfinite(X).all(1)[None, :] & (z > 0) & np.isfinite(z)
        if gate_px > 0:
            ok &= e <= gate_px ** 2
    ok &= ok.sum(0) >= 2
    return (ok * (1 << np.arange(len(uv)))[:, None]).sum(0).astype(np.uint8), e


def np_cost(K, uv, Rt, X, used):
    """Sum of squared pixel errors over the used observations at the poses Rt and points X (n, 3), float64."""
    total = 0.0
    for v in range(len(uv)):
        m = ((used >> v) & 1).astype(bool)
        p, _ = T.project(K, Rt[v], X[m])
        total += float(((p - uv[v][m].astype(np.float64)) ** 2).sum())
    return total


def _skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def np_dense(K, uv, Rt0, X0, used, fixed_mask, iters=200):
    """Dense damped Gauss-Newton over every free pose and every used point at once, float64 numpy: the full stacked Jacobian,
    np.linalg.lstsq on [J; sqrt(mu) I] (additive damping, a step accepted only if the cost falls), the rotation updated by the
    exact exponential.  Shares nothing with the Schur form.  Returns (poses, X, cost)."""
    V = len(uv)
    free = [v for v in range(V) if not (fixed_mask >> v) & 1]
    pts = np.nonzero(used)[0]
    col = {int(i): 6 * len(free) + 3 * k for k, i in enumerate(pts)}
    obs = [(v, int(i)) for v in range(V) for i in pts if (used[i] >> v) & 1]
    poses = [_pose(r) for r in Rt0]
    X = np.array(X0, np.float64)

    def res(poses, X, jac):
        r = np.zeros(2 * len(obs))
        J = np.zeros((2 * len(obs), 6 * len(free) + 3 * len(pts))) if jac else None
        for k, (v, i) in enumerate(obs):
            Rm, t = poses[v]
            Y = Rm @ X[i]
            x = Y + t
            if not x[2] > 0:
                return None, None
            r[2 * k] = K[0] * x[0] / x[2] + K[2] - float(uv[v][i, 0])
            r[2 * k + 1] = K[1] * x[1] / x[2] + K[3] - float(uv[v][i, 1])
            if jac:
                Jp = np.array([[K[0] / x[2], 0, -K[0] * x[0] / x[2] ** 2], [0, K[1] / x[2], -K[1] * x[1] / x[2] ** 2]])
                if v in free:
                    a = 6 * free.index(v)
                    J[2 * k:2 * k + 2, a:a + 3] = -Jp @ _skew(Y)
                    J[2 * k:2 * k + 2, a + 3:a + 6] = Jp
                J[2 * k:2 * k + 2, col[i]:col[i] + 3] = Jp @ Rm
        return r, J

    r, J = res(poses, X, True)
    cost, mu, small = float(r @ r), 1e-3 * float((J * J).sum(0).max()), 0
    for _ in range(iters):
        A = np.vstack([J, np.sqrt(mu) * np.eye(J.shape[1])])
        try:
            d = np.linalg.lstsq(A, np.r_[-r, np.zeros(J.shape[1])], rcond=None)[0]
        except np.linalg.LinAlgError:                       # LAPACK gives up at a huge mu, after the last gain: the end
            break
        trial = list(poses)
        for a, v in enumerate(free):
            trial[v] = (T._rot(d[6 * a:6 * a + 3]) @ poses[v][0], poses[v][1] + d[6 * a + 3:6 * a + 6])
        Xt = X.copy()
        Xt[pts] += d[6 * len(free):].reshape(-1, 3)
        rt, _ = res(trial, Xt, False)
        if rt is not None and float(rt @ rt) < cost:
            gain = cost - float(rt @ rt)
            poses, X = trial, Xt
            r, J = res(poses, X, True)
            cost, mu = float(r @ r), mu / 10
            small = small + 1 if gain <= 1e-13 * cost else 0
            if small >= 3:
                break
        else:
            mu *= 10
            if mu > 1e30:
                break
    return [np.r_[Rm.reshape(-1), t] for Rm, t in poses], X, cost
