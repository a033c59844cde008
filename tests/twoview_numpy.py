"""An implementation of the two-view refinements written separately from tests/twoview_refine_ref.c, in plain numpy: the
SVD 8-point refit with SVD rank-2 projection, and Levenberg-Marquardt with a central finite-difference Jacobian on the
same costs (sum of squared Sampson distances), for F over (U, V, sigma) with Rodrigues rotations and for the pose over
(R, t) with a Rodrigues rotation and a null-space basis of t.  No formula is shared with the restatement beyond the cost
itself.  Used by test_twoview_refine_cpu.py."""
import numpy as np


def _h(x):
    return np.c_[np.asarray(x, np.float64), np.ones(len(x))]


def sampson(F, p1, p2):
    """Signed Sampson distances of homogeneous points (n x 3 each)."""
    l, lt = p1 @ F.T, p2 @ F
    return (p2 * l).sum(1) / np.sqrt(l[:, 0] ** 2 + l[:, 1] ** 2 + lt[:, 0] ** 2 + lt[:, 1] ** 2)


def _hartley(x):
    c = x.mean(0)
    s = np.sqrt(2.0) / np.linalg.norm(x - c, axis=1).mean()
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def unit_f(F):
    F = F / np.linalg.norm(F)
    return -F if F[2, 2] < 0 else F


def refit8(xy1, xy2, mask):
    """Normalised least-squares 8-point over the inliers, rank 2 by SVD, unit norm, F[2,2] >= 0."""
    m = np.asarray(mask).astype(bool)
    x1, x2 = np.asarray(xy1, np.float64)[m], np.asarray(xy2, np.float64)[m]
    T1, T2 = _hartley(x1), _hartley(x2)
    a, b = _h(x1) @ T1.T, _h(x2) @ T2.T
    A = np.c_[b[:, 0:1] * a, b[:, 1:2] * a, a]
    Fn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    U, S, Vt = np.linalg.svd(Fn)
    Fn = U @ np.diag([S[0], S[1], 0.0]) @ Vt
    return unit_f(T2.T @ Fn @ T1)


def _rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def _lm(res, retract, state, npar, iters=300, h=1e-6):
    lam = 1e-3
    r = res(state)
    c = r @ r
    for _ in range(iters):
        J = np.empty((len(r), npar))
        for k in range(npar):
            e = np.zeros(npar)
            e[k] = h
            J[:, k] = (res(retract(state, e)) - res(retract(state, -e))) / (2 * h)
        A, g = J.T @ J, J.T @ r
        moved = False
        for _ in range(30):
            d = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
            s2 = retract(state, d)
            r2 = res(s2)
            if r2 @ r2 < c:
                state, r, c, lam, moved = s2, r2, r2 @ r2, lam / 10, True
                break
            lam *= 10
        if not moved or np.abs(d).max() < 1e-13:
            break
    return state, c


def f_lm(xy1, xy2, mask, F0):
    """LM on the pixel Sampson cost from F0 over rank-2 matrices: (F unit norm, cost)."""
    m = np.asarray(mask).astype(bool)
    x1, x2 = np.asarray(xy1, np.float64)[m], np.asarray(xy2, np.float64)[m]
    T1, T2 = _hartley(x1), _hartley(x2)
    p1, p2 = _h(x1), _h(x2)
    U, S, Vt = np.linalg.svd(np.linalg.inv(T2).T @ F0 @ np.linalg.inv(T1))

    def F_of(s):
        U, V, sg = s
        return T2.T @ (U @ np.diag([1.0, sg, 0.0]) @ V.T) @ T1

    def retract(s, d):
        U, V, sg = s
        return (U @ _rodrigues(d[:3]), V @ _rodrigues(d[3:6]), sg + d[6])

    s, c = _lm(lambda s: sampson(F_of(s), p1, p2), retract, (U, Vt.T, S[1] / S[0]), 7)
    return unit_f(F_of(s)), c


def essential(R, t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R


def pose_lm(xy1, xy2, K, mask, R0, t0):
    """LM on the Sampson cost of [t]x R over the S31-normalised points (f32 rounding included), scaled to px^2:
    (R, t unit, cost)."""
    fx, fy, cx, cy = K
    m = np.asarray(mask).astype(bool)

    def nrm(x):
        x = np.asarray(x, np.float32).astype(np.float64)[m]
        return np.c_[((x[:, 0] - cx) / fx).astype(np.float32), ((x[:, 1] - cy) / fy).astype(np.float32)].astype(np.float64)

    p1, p2 = _h(nrm(xy1)), _h(nrm(xy2))
    f = 0.5 * (fx + fy)

    def retract(s, d):
        R, t = s
        B = np.linalg.svd(t.reshape(1, 3))[2][1:].T
        t2 = t + B @ d[3:]
        return (_rodrigues(d[:3]) @ R, t2 / np.linalg.norm(t2))

    s, c = _lm(lambda s: f * sampson(essential(*s), p1, p2), retract, (np.asarray(R0, np.float64), t0 / np.linalg.norm(t0)), 5)
    return s[0], s[1], c
