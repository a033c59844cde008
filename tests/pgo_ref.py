"""ctypes loader of tests/pgo_ref.c, the plain-C restatement of docs/SPEC.md S118-S123 (pose-graph optimisation over SE(3) /
Sim(3) nodes and the map-point move behind it), plus the graphs and the independent dense numpy solver the two test files
share.  Built on first use by cref.py.  A pose is 13 doubles, R row-major, t, s: x_i = s R X + t (world to frame i); an edge
measurement takes frame a to frame b."""
import ctypes as C

import numpy as np

import cref
from cref import ptr as _p

SIM3, RIGID = 1, 0
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = cref.load("pgo_ref", {
            "pgo_edge": [C.c_int] + [C.c_void_p] * 7,
            "pgo_run": [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_double] + [C.c_void_p] * 4,
            "pgo_move": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
        }, {"pgo_run": None, "pgo_move": None})
    return _lib


class Result:
    pass


def edge(model, A, B, Z, w):
    """S119 of one edge: (ok, r (P), Ja (P, P), Jb (P, P)); rows are residual components."""
    P = 7 if model == SIM3 else 6
    r, Ja, Jb = np.zeros(P), np.zeros((P, P)), np.zeros((P, P))
    a = [np.ascontiguousarray(v, np.float64) for v in (A, B, Z, w)]
    ok = lib().pgo_edge(model, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(r), _p(Ja), _p(Jb))
    return bool(ok), r, Ja, Jb


def run(model, pose, fixed, ab, Z, w, max_iters=10, cg_iters=50, cg_tol=1e-6, n_edges=None):
    """S118-S122 over the first n_edges (default: all) edges: a Result with pose (N, 13), used (E) u8 (zero beyond n_edges),
    cost_in, cost_out, n_edges_used, n_nodes_free, iters, accepted, cg_total, status."""
    pose = np.ascontiguousarray(pose, np.float64).reshape(-1, 13)
    fixed = np.ascontiguousarray(fixed, np.uint8)
    ab = np.ascontiguousarray(ab, np.int32).reshape(-1, 2)
    Z = np.ascontiguousarray(Z, np.float64).reshape(-1, 13)
    w = np.ascontiguousarray(w, np.float64).reshape(-1, 3)
    N, E = pose.shape[0], ab.shape[0] if n_edges is None else int(n_edges)
    assert fixed.shape[0] == N and Z.shape[0] >= E and w.shape[0] >= E and ab.shape[0] >= E
    r = Result()
    r.pose = np.zeros((N, 13))
    r.used = np.zeros(max(ab.shape[0], 1), np.uint8)
    cost, info = np.zeros(2), np.zeros(6, np.int32)
    lib().pgo_run(model, _p(pose), N, _p(fixed), _p(ab), _p(Z), _p(w), E, int(max_iters), int(cg_iters), float(cg_tol), _p(r.pose),
                  _p(r.used), _p(cost), _p(info))
    r.used = r.used[:ab.shape[0]]
    r.cost_in, r.cost_out = float(cost[0]), float(cost[1])
    r.n_edges_used, r.n_nodes_free, r.iters, r.accepted, r.cg_total, r.status = (int(v) for v in info)
    return r


def move(pose_old, pose_new, anchor, xyz):
    """S123: rows (n, 3) f32 moved with their anchor node -> (n, 3) f32."""
    po = np.ascontiguousarray(pose_old, np.float64).reshape(-1, 13)
    pn = np.ascontiguousarray(pose_new, np.float64).reshape(-1, 13)
    anchor = np.ascontiguousarray(anchor, np.int32)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros((max(xyz.shape[0], 1), 3), np.float32)
    lib().pgo_move(_p(po), _p(pn), po.shape[0], _p(anchor), _p(xyz), xyz.shape[0], _p(out))
    return out[:xyz.shape[0]]


# ---- poses and graphs -------------------------------------------------------------------------------------------------------

def rot(w):
    """Rodrigues: the rotation by |w| radians about w."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def pose13(R, t, s=1.0):
    return np.r_[np.asarray(R, np.float64).reshape(-1), np.asarray(t, np.float64), float(s)]


def parts(T):
    T = np.asarray(T, np.float64)
    return T[:9].reshape(3, 3), T[9:12], T[12]


def compose(Z, A):
    """The pose Z o A: first A, then Z."""
    Rz, tz, sz = parts(Z)
    Ra, ta, sa = parts(A)
    return pose13(Rz @ Ra, sz * (Rz @ ta) + tz, sz * sa)


def between(A, B):
    """The measurement that takes frame a to frame b: B o A^-1."""
    Ra, ta, sa = parts(A)
    Rb, tb, sb = parts(B)
    R, s = Rb @ Ra.T, sb / sa
    return pose13(R, tb - s * (R @ ta), s)


def random_pose(rng, max_deg=180.0, scale=(1.0, 1.0), t_sigma=2.0):
    w = rng.normal(size=3)
    w *= np.radians(rng.uniform(0, max_deg)) / np.linalg.norm(w)
    return pose13(rot(w), rng.normal(0, t_sigma, 3), rng.uniform(*scale))


def ring_truth(n, model, seed, radius=10.0):
    """n keyframes on a circle looking inwards, with a slowly varying scale in the similarity model."""
    rng = np.random.default_rng([seed, 0x960])
    out = []
    for i in range(n):
        th = 2 * np.pi * i / n
        R = rot([0, 0, th]) @ rot(rng.normal(0, 0.05, 3))
        c = np.array([radius * np.cos(th), radius * np.sin(th), 0.3 * np.sin(3 * th)])
        s = 1.0 if model == RIGID else float(np.exp(rng.normal(0, 0.05)))
        out.append(pose13(R, -s * (R @ c), s))
    return np.array(out)


def noisy(Z, rng, deg, rel):
    """A measurement with a rotation error of deg degrees, a relative translation error and (s != 1 kept) scale error rel."""
    R, t, s = parts(Z)
    w = rng.normal(size=3)
    w *= np.radians(deg) / np.linalg.norm(w)
    return pose13(rot(w) @ R, t * (1 + rng.normal(0, rel, 3)) + rng.normal(0, rel, 3), s)


def chain_graph(n, n_loops, model, seed, deg=0.5, rel=0.01, weighted=True):
    """A chain of n nodes plus n_loops loop edges; noisy measurements; the start composes the chain's measurements from the
    held node 0.  Returns truth, start (n, 13), fixed (n) u8, ab (E, 2) i32, Z (E, 13), w (E, 3)."""
    rng = np.random.default_rng([seed, 0x961])
    truth = ring_truth(n, model, seed)
    ab = [(i, i + 1) for i in range(n - 1)]
    while len(ab) < n - 1 + n_loops:
        a, b = sorted(rng.choice(n, 2, replace=False))
        if b - a >= 2 and (a, b) not in ab:
            ab.append((int(a), int(b)))
    Z = []
    for a, b in ab:
        z = noisy(between(truth[a], truth[b]), rng, deg, rel)
        if model == SIM3:
            z[12] *= float(np.exp(rng.normal(0, rel)))
        Z.append(z)
    Z = np.array(Z)
    start = [truth[0]]
    for i in range(n - 1):
        start.append(compose(Z[i], start[-1]))
    start = np.array(start)
    if model == RIGID:
        start[:, 12] = 1.0
        Z[:, 12] = 1.0
    w = rng.uniform(0.5, 2.0, (len(ab), 3)) if weighted else np.ones((len(ab), 3))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return truth, start, fixed, np.array(ab, np.int32), Z, w


def graph(n, n_edges, model, seed, deg=0.5, rel=0.01, shuffle=False):
    """chain_graph's layout with n_edges edges in all (n_edges >= n - 1): the extra ones join random pairs a != b in either
    direction, duplicates allowed.  shuffle permutes the edge ids, so that incidence order is not arrival order."""
    rng = np.random.default_rng([seed, 0x962])
    truth = ring_truth(n, model, seed)
    ab = [(i, i + 1) for i in range(n - 1)]
    while len(ab) < n_edges:
        a, b = rng.choice(n, 2, replace=False)
        ab.append((int(a), int(b)))
    ab = np.array(ab, np.int32).reshape(-1, 2)
    Z = np.array([noisy(between(truth[a], truth[b]), rng, deg, rel) for a, b in ab])
    if model == SIM3:
        Z[:, 12] *= np.exp(rng.normal(0, rel, len(ab)))
    start = [truth[0]]
    for i in range(n - 1):
        start.append(compose(Z[i], start[-1]))
    start = np.array(start)
    if model == RIGID:
        start[:, 12] = 1.0
        Z[:, 12] = 1.0
    w = rng.uniform(0.5, 2.0, (len(ab), 3))
    if shuffle:
        order = rng.permutation(len(ab))
        ab, Z, w = ab[order], Z[order], w[order]
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return truth, start, fixed, ab, Z, w


def rules_graph(model, seed=3):
    """A graph of 41 nodes and 90 edges with one edge or node for every rule of S118's used set, and the used bytes those
    rules give: held nodes 17 and 18 in the middle (the edge between them has both ends held), node indices out of range, a
    self loop, a NaN in a measurement, an infinite weight, a zero and a negative measured scale, a measurement half a turn
    off, a zero-weight edge (used), a node with a NaN and a node with a negative scale (none of their edges is used), and node
    40, free, with no edge at all.  Returns start, fixed, ab, Z, w, expected."""
    _, start, fixed, ab, Z, w = graph(40, 90, model, seed)
    start = np.vstack([start, start[:1]])
    fixed = np.r_[fixed, np.uint8(0)]
    fixed[[17, 18]] = 1
    ab[45], ab[46], ab[47] = (-1, 3), (3, 41), (7, 7)
    Z[48, 4] = np.nan
    w[49, 1] = np.inf
    Z[50, 12], Z[51, 12] = 0.0, -1.0
    a, b = ab[52]
    R, t, s = parts(between(start[a], start[b]))
    Z[52] = pose13(rot([0.0, np.pi, 0.0]) @ R, t, s)
    w[53] = 0.0
    start[30, 3] = np.nan
    start[33, 12] = -1.0
    expected = np.ones(len(ab), np.uint8)
    expected[[45, 46, 47, 48, 49, 50, 51, 52]] = 0
    for e, (a, b) in enumerate(ab):
        if a in (30, 33) or b in (30, 33) or (0 <= a < 41 and 0 <= b < 41 and fixed[a] and fixed[b]):
            expected[e] = 0
    return start, fixed, ab, Z, w, expected


def exact_graph(model):
    """12 nodes whose poses (axis permutations, small integer t, scales that are powers of two) and 15 measurements are exact
    in fp64: every residual at the start is 0.0.  Returns start, fixed, ab, Z, w."""
    perm = [np.eye(3), np.eye(3)[[1, 2, 0]], np.eye(3)[[2, 0, 1]]]
    pose = np.array([pose13(perm[i % 3], [i, 2 * i - 5, 3 - i], 1.0 if model == RIGID else 2.0 ** (i % 3 - 1)) for i in range(12)])
    ab = np.array([(i, i + 1) for i in range(11)] + [(11, 0), (3, 8), (9, 2), (5, 0)], np.int32)
    Z = np.array([between(pose[a], pose[b]) for a, b in ab])
    fixed = np.zeros(12, np.uint8)
    fixed[0] = 1
    return pose, fixed, ab, Z, np.ones((15, 3))


# ---- independent float64 numpy evaluation -----------------------------------------------------------------------------------

def np_residual(model, pose, ab, Z, w):
    """The stacked residual of every edge, (E, 7) or (E, 6): its own statement of S119, vectorised over the edges."""
    pose, Z, w = np.asarray(pose, np.float64), np.asarray(Z, np.float64), np.asarray(w, np.float64)
    a, b = np.asarray(ab)[:, 0], np.asarray(ab)[:, 1]
    Ra, Rb, Rz = (v[:, :9].reshape(-1, 3, 3) for v in (pose[a], pose[b], Z))
    RD = np.einsum("eij,ekj->eik", Rb, Ra)
    sD = pose[b, 12] / pose[a, 12]
    tD = pose[b, 9:12] - sD[:, None] * np.einsum("eij,ej->ei", RD, pose[a, 9:12])
    Er = np.einsum("eji,ejk->eik", Rz, RD)
    cos = (np.trace(Er, axis1=1, axis2=2) - 1) / 2
    vee = np.stack([Er[:, 2, 1] - Er[:, 1, 2], Er[:, 0, 2] - Er[:, 2, 0], Er[:, 1, 0] - Er[:, 0, 1]], 1)
    out = [w[:, :1] * vee / (1 + cos)[:, None], w[:, 1:2] * (tD - Z[:, 9:12])]
    if model == SIM3:
        out.append((w[:, 2] * np.sinh(np.log(sD / Z[:, 12])))[:, None])
    return np.concatenate(out, 1)


def np_update(model, T, d):
    """S121 step 6 on one pose in numpy: R' = Cayley(d[:3] / 2) R, t' = t + d[3:6], s' = s (1 + d[6]) in the similarity model."""
    R, t, s = parts(T)
    h = np.asarray(d[:3], np.float64) / 2
    Kx = np.array([[0, -h[2], h[1]], [h[2], 0, -h[0]], [-h[1], h[0], 0]])
    Cm = ((1 - h @ h) * np.eye(3) + 2 * np.outer(h, h) + 2 * Kx) / (1 + h @ h)
    return pose13(Cm @ R, t + d[3:6], s * (1 + d[6]) if model == SIM3 else s)


def np_apply(model, pose, free, d):
    """pose with the local step d (len(free), 7 or 6) applied: exact exponential on the left, t + dt, s * exp(ds)."""
    out = np.array(pose, np.float64)
    for k, i in enumerate(free):
        R, t, s = parts(pose[i])
        out[i] = pose13(rot(d[k, :3]) @ R, t + d[k, 3:6], s * (np.exp(d[k, 6]) if model == SIM3 else 1.0))
    return out


def np_dense(model, pose, fixed, ab, Z, w, iters=60, h=1e-6):
    """Dense Gauss-Newton over every free node at once: the stacked residual above, its Jacobian by central differences,
    np.linalg.lstsq, iterated until the step vanishes (a step is halved while the cost does not fall).  Shares nothing with
    the restatement but the problem.  Returns (pose, cost)."""
    P = 7 if model == SIM3 else 6
    free = [i for i in range(len(pose)) if not fixed[i]]
    pose = np.array(pose, np.float64)
    r = np_residual(model, pose, ab, Z, w).reshape(-1)
    cost = float(r @ r)
    for _ in range(iters):
        J = np.zeros((r.size, P * len(free)))
        for k, i in enumerate(free):
            for j in range(P):
                d = np.zeros((1, P))
                d[0, j] = h
                rp = np_residual(model, np_apply(model, pose, [i], d), ab, Z, w).reshape(-1)
                rm = np_residual(model, np_apply(model, pose, [i], -d), ab, Z, w).reshape(-1)
                J[:, P * k + j] = (rp - rm) / (2 * h)
        d = np.linalg.lstsq(J, -r, rcond=None)[0].reshape(len(free), P)
        moved = False
        for _ in range(30):
            trial = np_apply(model, pose, free, d)
            rt = np_residual(model, trial, ab, Z, w).reshape(-1)
            if float(rt @ rt) < cost:
                pose, r, cost, moved = trial, rt, float(rt @ rt), True
                break
            d = d / 2
        if not moved or np.abs(d).max() < 1e-13:
            break
    return pose, cost


def pose_err(A, B):
    """(rotation angle in degrees, |t_a - t_b|, |s_a / s_b - 1|) between two poses."""
    Ra, ta, sa = parts(A)
    Rb, tb, sb = parts(B)
    D = Ra.T @ Rb
    sin = np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2
    ang = np.degrees(np.arctan2(sin, (np.trace(D) - 1) / 2))     # exact near zero, where arccos is not
    return ang, float(np.linalg.norm(ta - tb)), abs(sa / sb - 1)
