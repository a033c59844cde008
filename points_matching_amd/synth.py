"""Deterministic synthetic inputs for the BASELINE configs.

The reference ships no usable inputs for its own path (main.cpp:14-15 reads img1.bmp/img2.bmp,
which are missing), so every workload is generated here from a seed:
  * SIFT-like descriptors: integer-valued floats in [0,255]   (what OpenCV SIFT emits)
  * SURF-like descriptors: unit-L2-norm general floats         (what main.cpp:37-40 emits)
  * ORB-like descriptors : 256-bit packed binary
  * two-view geometry with a known F_gt, inlier noise and gross outliers
"""
import numpy as np


def _planted(rng, nq, nt, frac):
    """Planted ground truth: query i < n_pl is a noisy copy of train row perm[i]."""
    n_pl = int(round(frac * min(nq, nt)))
    src = rng.permutation(nt)[:n_pl]
    return n_pl, src


def sift_like(nq, nt, dim=128, seed=0xC2, planted=0.5, sigma=0.05):
    """|N(0,1)| -> L2-normalise -> clip 0.2 -> renormalise -> x512 -> round -> saturate [0,255]."""
    rng = np.random.default_rng(seed)

    def quant(x):
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
        x = np.minimum(x, 0.2)
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
        return np.clip(np.rint(x * 512.0), 0, 255).astype(np.float32)

    t_raw = np.abs(rng.standard_normal((nt, dim)))
    q_raw = np.abs(rng.standard_normal((nq, dim)))
    n_pl, src = _planted(rng, nq, nt, planted)
    if n_pl:
        base = t_raw[src] / np.linalg.norm(t_raw[src], axis=1, keepdims=True)
        q_raw[:n_pl] = np.abs(base + sigma * rng.standard_normal((n_pl, dim)))
    truth = np.full(nq, -1, np.int32)
    truth[:n_pl] = src
    return quant(q_raw), quant(t_raw), truth


def surf_like(nq, nt, dim=128, seed=0xC2, planted=0.5, sigma=0.05):
    """N(0,1)^dim, L2-normalised: general (non-integer) floats."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((nt, dim))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    q = rng.standard_normal((nq, dim))
    n_pl, src = _planted(rng, nq, nt, planted)
    if n_pl:
        q[:n_pl] = t[src] + sigma * rng.standard_normal((n_pl, dim))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    truth = np.full(nq, -1, np.int32)
    truth[:n_pl] = src
    return q.astype(np.float32), t.astype(np.float32), truth


def orb_like(nq, nt, nbytes=32, seed=0xC4, planted=0.5, flip=0.1):
    """iid Bernoulli(1/2) bits; planted copies flip each bit with probability `flip`."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (nt, nbytes), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, nbytes), dtype=np.uint8)
    n_pl, src = _planted(rng, nq, nt, planted)
    if n_pl:
        flips = (rng.random((n_pl, nbytes * 8)) < flip)
        q[:n_pl] = t[src] ^ np.packbits(flips, axis=1)
    truth = np.full(nq, -1, np.int32)
    truth[:n_pl] = src
    return q, t, truth


def two_view(n, seed=0xC3, outlier_frac=0.3, noise_px=0.5, width=993, height=660, focal=1000.0):
    """3-D points in z in [4,12] seen by two 1000-px-focal cameras (baseline 1, small rotation).

    Returns xy1, xy2 (n x 2 float32 pixels), F_gt (3x3 float64, x2^T F x1 = 0, unit Frobenius
    norm) and the boolean ground-truth inlier flags.  Image size = img01/img02 (993 x 660).
    """
    rng = np.random.default_rng(seed)
    K = np.array([[focal, 0, width / 2.0], [0, focal, height / 2.0], [0, 0, 1.0]])
    ang = rng.uniform(-0.08, 0.08, 3)
    cx, cy, cz = np.cos(ang)
    sx, sy, sz = np.sin(ang)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    t = np.array([1.0, 0.05, 0.02])
    t /= np.linalg.norm(t)
    z = rng.uniform(4.0, 12.0, n)
    X = np.stack([rng.uniform(-0.45, 0.45, n) * z * width / focal,
                  rng.uniform(-0.45, 0.45, n) * z * height / focal, z], axis=1)
    x1 = (K @ X.T).T
    x1 = x1[:, :2] / x1[:, 2:3]
    X2 = (R @ X.T).T + t
    x2 = (K @ X2.T).T
    x2 = x2[:, :2] / x2[:, 2:3]
    x1 = x1 + rng.normal(0, noise_px, x1.shape)
    x2 = x2 + rng.normal(0, noise_px, x2.shape)
    inl = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.permutation(n)[:n_out]
        inl[bad] = False
        x1[bad] = rng.uniform([0, 0], [width, height], (n_out, 2))
        x2[bad] = rng.uniform([0, 0], [width, height], (n_out, 2))
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Kinv = np.linalg.inv(K)
    F = Kinv.T @ tx @ R @ Kinv
    F /= np.linalg.norm(F)
    if F[2, 2] < 0:
        F = -F
    return np.ascontiguousarray(x1.astype(np.float32)), np.ascontiguousarray(x2.astype(np.float32)), F, inl


def _sift_quant(x):
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    x = np.minimum(x, 0.2)
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return np.clip(np.rint(x * 512.0), 0, 255).astype(np.float32)


def pair_workload(nq=8192, nt=8192, dim=128, seed=0xC3, rank=0, planted=0.28, outlier_frac=0.3,
                  noise_px=0.5, sigma=0.05, kind="sift", width=993, height=660, focal=1000.0):
    """One image pair of BASELINE config C3/C4: descriptors + keypoints + geometry.

    The train image (descriptors `t`, keypoints `kp2`, 3-D scene, cameras) depends on `seed`
    only; the query image depends on (seed, rank), so the ranks of a multi-GPU run hold
    different query-row shards of one global problem against a replicated train set.
    A fraction `planted` of the query rows are noisy copies of distinct train rows; their
    keypoints are true projections of the same 3-D point (+N(0, noise_px)), except that
    `outlier_frac` of them get a uniform-random image-1 position (false matches that survive
    the ratio test).  kind: "sift" (integer-valued floats), "surf" (unit-norm floats), "orb"
    (dim = bytes per descriptor, uint8).
    """
    rt = np.random.default_rng([seed, 0])
    rq = np.random.default_rng([seed, 1, rank])
    # scene + cameras (train-side, rank-independent)
    K = np.array([[focal, 0, width / 2.0], [0, focal, height / 2.0], [0, 0, 1.0]])
    ang = rt.uniform(-0.08, 0.08, 3)
    ca, cb, cc = np.cos(ang)
    sa, sb, sc = np.sin(ang)
    R = (np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
         @ np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]))
    tv = np.array([1.0, 0.05, 0.02])
    tv /= np.linalg.norm(tv)
    z = rt.uniform(4.0, 12.0, nt)
    X = np.stack([rt.uniform(-0.45, 0.45, nt) * z * width / focal,
                  rt.uniform(-0.45, 0.45, nt) * z * height / focal, z], axis=1)
    p2 = (K @ ((R @ X.T).T + tv).T).T
    kp2 = (p2[:, :2] / p2[:, 2:3] + rt.normal(0, noise_px, (nt, 2))).astype(np.float32)
    tx = np.array([[0, -tv[2], tv[1]], [tv[2], 0, -tv[0]], [-tv[1], tv[0], 0]])
    Kinv = np.linalg.inv(K)
    F = Kinv.T @ tx @ R @ Kinv
    F /= np.linalg.norm(F)
    if F[2, 2] < 0:
        F = -F
    # descriptors
    n_pl = int(round(planted * min(nq, nt)))
    src = rq.permutation(nt)[:n_pl]
    if kind == "orb":
        t = rt.integers(0, 256, (nt, dim), dtype=np.uint8)
        q = rq.integers(0, 256, (nq, dim), dtype=np.uint8)
        flips = rq.random((n_pl, dim * 8)) < 0.1
        q[:n_pl] = t[src] ^ np.packbits(flips, axis=1)
    elif kind == "sift":
        t_raw = np.abs(rt.standard_normal((nt, dim)))
        q_raw = np.abs(rq.standard_normal((nq, dim)))
        base = t_raw[src] / np.linalg.norm(t_raw[src], axis=1, keepdims=True)
        q_raw[:n_pl] = np.abs(base + sigma * rq.standard_normal((n_pl, dim)))
        t, q = _sift_quant(t_raw), _sift_quant(q_raw)
    else:
        t = rt.standard_normal((nt, dim))
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        q = rq.standard_normal((nq, dim))
        q[:n_pl] = t[src] + sigma * rq.standard_normal((n_pl, dim))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        t, q = t.astype(np.float32), q.astype(np.float32)
    # query keypoints
    kp1 = rq.uniform([0, 0], [width, height], (nq, 2))
    p1 = (K @ X[src].T).T
    kp1[:n_pl] = p1[:, :2] / p1[:, 2:3] + rq.normal(0, noise_px, (n_pl, 2))
    true_inlier = np.zeros(nq, bool)
    true_inlier[:n_pl] = True
    n_bad = int(round(outlier_frac * n_pl))
    bad = rq.permutation(n_pl)[:n_bad]
    kp1[bad] = rq.uniform([0, 0], [width, height], (n_bad, 2))
    true_inlier[bad] = False
    # shuffle the query rows so planted rows are not a prefix
    perm = rq.permutation(nq)
    truth = np.full(nq, -1, np.int32)
    truth[:n_pl] = src
    # every array C-contiguous: the device entry points take raw pointers
    return {"q": np.ascontiguousarray(q[perm]), "t": np.ascontiguousarray(t),
            "kp1": np.ascontiguousarray(kp1[perm].astype(np.float32)), "kp2": np.ascontiguousarray(kp2),
            "truth": truth[perm], "true_inlier": true_inlier[perm], "F_gt": F}


def planar_view(n, seed=0xC5, outlier_frac=0.3, noise_px=0.5, width=993, height=660):
    """Correspondences of a planar scene (or a pure camera rotation): image-2 points are image-1 points mapped by a known,
    well-conditioned homography (rotation up to 6 degrees, scale 0.9-1.1, shift up to 40 px, mild perspective about
    the image centre), plus N(0, noise_px) in both images; `outlier_frac` of the pairs get uniform-random image-2
    positions.

    Returns xy1, xy2 (n x 2 float32 pixels), H_gt (3x3 float64, x2 ~ H x1, unit Frobenius norm, H[2,2] > 0) and the
    boolean ground-truth inlier flags.
    """
    rng = np.random.default_rng([seed, 0x4817])
    a = rng.uniform(-0.1, 0.1)
    sc = rng.uniform(0.9, 1.1)
    A = np.array([[sc * np.cos(a), -sc * np.sin(a), rng.uniform(-40, 40)],
                  [sc * np.sin(a), sc * np.cos(a), rng.uniform(-40, 40)],
                  [rng.uniform(-1e-4, 1e-4), rng.uniform(-1e-4, 1e-4), 1.0]])
    C = np.array([[1.0, 0, width / 2.0], [0, 1.0, height / 2.0], [0, 0, 1.0]])
    H = C @ A @ np.linalg.inv(C)
    H /= np.linalg.norm(H)
    if H[2, 2] < 0:
        H = -H
    x1 = rng.uniform([0, 0], [width, height], (n, 2))
    p = np.column_stack([x1, np.ones(n)]) @ H.T
    x2 = p[:, :2] / p[:, 2:3]
    x1 = x1 + rng.normal(0, noise_px, x1.shape)
    x2 = x2 + rng.normal(0, noise_px, x2.shape)
    inl = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.permutation(n)[:n_out]
        inl[bad] = False
        x2[bad] = rng.uniform([0, 0], [width, height], (n_out, 2))
    return np.ascontiguousarray(x1.astype(np.float32)), np.ascontiguousarray(x2.astype(np.float32)), H, inl


def calibrated_view(n, seed=0xE5, K=None, R=None, t=None, outlier_frac=0.3, noise_px=0.5, planar=False, forward=False,
                    width=993, height=660):
    """Correspondences of a calibrated two-view scene (visual odometry, SfM, a stereo rig): 3-D points seen by one
    pinhole camera K at [I|0] and at [R|t], plus N(0, noise_px) in both images; `outlier_frac` of the pairs get
    uniform-random image-2 positions.  Defaults: K with fx != fy and an off-centre principal point; R a rotation up to
    ~6 degrees; t a unit sideways baseline, or (`forward`) mostly along the optical axis.  `planar`: the points lie on
    one tilted plane.  Points are kept in front of both cameras.

    Returns xy1, xy2 (n x 2 float32 pixels), K (3 x 3), R (3 x 3), t (unit 3-vector; x2 ~ K (R X + t)), X (n x 3 points
    in camera-1 coordinates) and the boolean ground-truth inlier flags.
    """
    rng = np.random.default_rng([seed, 0xE55E])
    if K is None:
        K = np.array([[rng.uniform(700, 900), 0, width / 2.0 + rng.uniform(-40, 40)],
                      [0, rng.uniform(750, 950), height / 2.0 + rng.uniform(-30, 30)], [0, 0, 1.0]])
    K = np.asarray(K, np.float64)
    if R is None:
        w = rng.normal(size=3)
        w *= rng.uniform(0.03, 0.1) / np.linalg.norm(w)
        th = np.linalg.norm(w)
        k = w / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    R = np.asarray(R, np.float64)
    if t is None:
        t = np.array([0.2, 0.05, -1.0]) if forward else np.array([1.0, rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)])
    t = np.asarray(t, np.float64) / np.linalg.norm(t)
    Ki = np.linalg.inv(K)
    X = np.zeros((0, 3))
    while X.shape[0] < n:
        m = 2 * n
        px = rng.uniform([0, 0], [width, height], (m, 2))
        ray = np.c_[px, np.ones(m)] @ Ki.T
        if planar:
            nrm = np.array([0.1, -0.2, 1.0])
            d = 8.0
            z = d / (ray @ nrm)
        else:
            z = rng.uniform(4.0, 12.0, m)
        P = ray * z[:, None]
        P2 = P @ R.T + t
        P = P[(P[:, 2] > 0.5) & (P2[:, 2] > 0.5)]
        X = np.r_[X, P]
    X = X[:n]
    x1 = X @ K.T
    x1 = x1[:, :2] / x1[:, 2:3]
    x2 = (X @ R.T + t) @ K.T
    x2 = x2[:, :2] / x2[:, 2:3]
    x1 = x1 + rng.normal(0, noise_px, x1.shape)
    x2 = x2 + rng.normal(0, noise_px, x2.shape)
    inl = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.permutation(n)[:n_out]
        inl[bad] = False
        x2[bad] = rng.uniform([0, 0], [width, height], (n_out, 2))
    return (np.ascontiguousarray(x1.astype(np.float32)), np.ascontiguousarray(x2.astype(np.float32)), K, R, t, X, inl)


def pnp_scene(n, seed=0x9F, K=None, outlier_frac=0.3, noise_px=0.5, width=993, height=660):
    """2D-3D correspondences of one calibrated frame against a known map (visual odometry / SfM localisation): world
    points in front of the camera seen by pinhole K at pose x_cam = R X + t, plus N(0, noise_px) on the pixels;
    `outlier_frac` of the pixels are replaced by uniform-random image positions.  Defaults: K with fx != fy and an
    off-centre principal point, R a rotation up to ~30 degrees, t up to ~2 units, depths 4-12.

    Returns xyz (n x 3 float32 world points), uv (n x 2 float32 pixels), K (3 x 3), R (3 x 3), t (3) and the boolean
    ground-truth inlier flags.
    """
    rng = np.random.default_rng([seed, 0x9A9F])
    if K is None:
        K = np.array([[rng.uniform(700, 900), 0, width / 2.0 + rng.uniform(-40, 40)],
                      [0, rng.uniform(750, 950), height / 2.0 + rng.uniform(-30, 30)], [0, 0, 1.0]])
    K = np.asarray(K, np.float64)
    w = rng.normal(size=3)
    w *= rng.uniform(0.1, 0.5) / np.linalg.norm(w)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.uniform(-2.0, 2.0, 3)
    px = rng.uniform([0, 0], [width, height], (n, 2))
    Xc = np.c_[px, np.ones(n)] @ np.linalg.inv(K).T * rng.uniform(4.0, 12.0, n)[:, None]
    X = (Xc - t) @ R                                           # world = R^T (x_cam - t)
    uv = Xc @ K.T
    uv = uv[:, :2] / uv[:, 2:3] + rng.normal(0, noise_px, (n, 2))
    inl = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.permutation(n)[:n_out]
        inl[bad] = False
        uv[bad] = rng.uniform([0, 0], [width, height], (n_out, 2))
    return np.ascontiguousarray(X.astype(np.float32)), np.ascontiguousarray(uv.astype(np.float32)), K, R, t, inl


def affine_view(n, seed=0xA5, outlier_frac=0.3, noise_px=0.5, partial=False, width=993, height=660):
    """Correspondences of a 2D affine scene (a document scan, an aerial mosaic tile, a stabilised video frame): image-2
    points are image-1 points mapped by a known affine map about the image centre, plus N(0, noise_px) in both images;
    `outlier_frac` of the pairs get uniform-random image-2 positions.  The map is a rotation up to 10 degrees, scale
    0.85-1.15 and a shift up to 40 px; unless `partial`, also anisotropic scale (0.9-1.1 per axis) and shear up to 0.1,
    so that only the full 6-DOF model explains it.  `partial`: a similarity (rotation, uniform scale, translation).

    Returns xy1, xy2 (n x 2 float32 pixels), A_gt (2 x 3 float64, x2 = A [x1 y1 1]^T) and the boolean ground-truth inlier
    flags.
    """
    rng = np.random.default_rng([seed, 0xAFF1])
    a = rng.uniform(-0.175, 0.175)
    sc = rng.uniform(0.85, 1.15)
    R = sc * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    if not partial:
        R = R @ np.array([[rng.uniform(0.9, 1.1), rng.uniform(-0.1, 0.1)], [0.0, rng.uniform(0.9, 1.1)]])
    c = np.array([width / 2.0, height / 2.0])
    t = c + rng.uniform(-40, 40, 2) - R @ c
    A = np.column_stack([R, t])
    x1 = rng.uniform([0, 0], [width, height], (n, 2))
    x2 = x1 @ R.T + t
    x1 = x1 + rng.normal(0, noise_px, x1.shape)
    x2 = x2 + rng.normal(0, noise_px, x2.shape)
    inl = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.permutation(n)[:n_out]
        inl[bad] = False
        x2[bad] = rng.uniform([0, 0], [width, height], (n_out, 2))
    return np.ascontiguousarray(x1.astype(np.float32)), np.ascontiguousarray(x2.astype(np.float32)), A, inl


def planar_view_wide(n, seed=0, width=4000, height=3000, angle=None, persp=0.8, pp_offset=(0.0, 0.0), noise_px=0.5,
                     outlier_frac=0.3, w_min=0.05):
    """planar_view at hard geometry: images up to 16000 px wide, any rotation, strong perspective.

    Built about the principal point c1 = image centre + pp_offset: x2 - c2 ~ A (x1 - c1), A = [[s R, t], [g, h, 1]] with
    R a rotation by `angle` radians (None: uniform in [-pi, pi)), s in [0.7, 1.4], |t| up to width / 20 and the
    perspective row (g, h) of random direction scaled so that |g dx + h dy| reaches `persp` at the farthest image
    corner: the true w = 1 + g dx + h dy spans about [1 - persp, 1 + persp] over image 1 (0.8: 0.2 to 1.8, a 9x
    change of scale).  Pairs whose true w is at or below `w_min` (behind or at the vanishing line) are redrawn.  Image-2
    points may lie far outside the image; outliers are uniform over the bounding box of the true image-2 points.

    Returns xy1, xy2 (n x 2 float32 pixels), H_gt (3x3 float64, x2 ~ H x1, unit Frobenius norm, H[2,2] > 0) and the
    boolean ground-truth inlier flags, as planar_view does.
    """
    rng = np.random.default_rng([seed, 0x4818])
    a = rng.uniform(-np.pi, np.pi) if angle is None else float(angle)
    sc = rng.uniform(0.7, 1.4)
    c1 = np.array([width / 2.0 + pp_offset[0], height / 2.0 + pp_offset[1]])
    c2 = np.array([width / 2.0, height / 2.0])
    corners = np.array([[0, 0], [width, 0], [0, height], [width, height]], np.float64) - c1
    d = rng.normal(size=2)
    d /= np.linalg.norm(d)
    g = d * (persp / np.abs(corners @ d).max())
    A = np.array([[sc * np.cos(a), -sc * np.sin(a), rng.uniform(-width / 20.0, width / 20.0)],
                  [sc * np.sin(a), sc * np.cos(a), rng.uniform(-width / 20.0, width / 20.0)],
                  [g[0], g[1], 1.0]])
    C1 = np.array([[1.0, 0, -c1[0]], [0, 1.0, -c1[1]], [0, 0, 1.0]])
    C2 = np.array([[1.0, 0, c2[0]], [0, 1.0, c2[1]], [0, 0, 1.0]])
    H = C2 @ A @ C1
    x1 = np.zeros((0, 2))
    while x1.shape[0] < n:
        c = rng.uniform([0, 0], [width, height], (2 * n + 16, 2))
        x1 = np.concatenate([x1, c[(c - c1) @ g + 1.0 > w_min]])
    x1 = x1[:n]
    p = np.column_stack([x1, np.ones(n)]) @ H.T
    x2 = p[:, :2] / p[:, 2:3]
    H = H / np.linalg.norm(H)
    if H[2, 2] < 0:
        H = -H
    x1 = x1 + rng.normal(0, noise_px, x1.shape)
    x2 = x2 + rng.normal(0, noise_px, x2.shape)
    inl = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.permutation(n)[:n_out]
        inl[bad] = False
        x2[bad] = rng.uniform(x2[inl].min(axis=0), x2[inl].max(axis=0), (n_out, 2))
    return np.ascontiguousarray(x1.astype(np.float32)), np.ascontiguousarray(x2.astype(np.float32)), H, inl


def affine_view_wide(n, seed=0, width=4000, height=3000, angle=None, scale=None, aniso=None, shear=None, reflect=False,
                     offset=(0.0, 0.0), noise_px=0.5, outlier_frac=0.3, partial=False):
    """affine_view at hard geometry: images up to 16000 px wide, any rotation, scale 0.25-4, far from the origin.

    x2 - c2 = M (x1 - c1) + t, with c1 = c2 = image centre + `offset` (mosaic or tile coordinates: 1e4-1e5 px puts
    every coordinate far from the origin), |t| up to width / 20 and M = s R(angle) for `partial`.  Otherwise
    M = s R(angle) diag(sqrt(k), 1 / sqrt(k)) [[1, shear], [0, 1]] R(beta) diag(1, -1 if reflect else 1): anisotropy
    k (singular-value ratio about k for small shear), shear and a reflection.  None draws: angle and beta uniform in
    [-pi, pi), s log-uniform in [0.25, 4], k uniform in [1, 3], shear uniform in [-0.3, 0.3].  Both images get
    N(0, noise_px); `outlier_frac` of the pairs get image-2 points uniform over the bounding box of the true ones.

    Returns xy1, xy2 (n x 2 float32 pixels), A_gt (2 x 3 float64, x2 = A [x1 y1 1]^T) and the boolean ground-truth inlier
    flags, as affine_view does.
    """
    if partial and (reflect or (aniso not in (None, 1.0)) or (shear not in (None, 0.0))):
        raise ValueError("a similarity has no anisotropy, shear or reflection")
    rng = np.random.default_rng([seed, 0xAFF2])
    a = rng.uniform(-np.pi, np.pi) if angle is None else float(angle)
    s = float(np.exp(rng.uniform(np.log(0.25), np.log(4.0)))) if scale is None else float(scale)

    def rot(t):
        return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])

    M = s * rot(a)
    if not partial:
        k = rng.uniform(1.0, 3.0) if aniso is None else float(aniso)
        sh = rng.uniform(-0.3, 0.3) if shear is None else float(shear)
        beta = rng.uniform(-np.pi, np.pi)
        M = M @ np.diag([np.sqrt(k), 1.0 / np.sqrt(k)]) @ np.array([[1.0, sh], [0.0, 1.0]]) @ rot(beta)
        if reflect:
            M = M @ np.diag([1.0, -1.0])
    c = np.array([width / 2.0 + offset[0], height / 2.0 + offset[1]])
    t = c + rng.uniform(-width / 20.0, width / 20.0, 2) - M @ c
    A = np.column_stack([M, t])
    x1 = rng.uniform([offset[0], offset[1]], [offset[0] + width, offset[1] + height], (n, 2))
    x2 = x1 @ M.T + t
    x1 = x1 + rng.normal(0, noise_px, x1.shape)
    x2 = x2 + rng.normal(0, noise_px, x2.shape)
    inl = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.permutation(n)[:n_out]
        inl[bad] = False
        x2[bad] = rng.uniform(x2[inl].min(axis=0), x2[inl].max(axis=0), (n_out, 2))
    return np.ascontiguousarray(x1.astype(np.float32)), np.ascontiguousarray(x2.astype(np.float32)), A, inl


def _rodrigues(axis, th):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _wide_camera(width, height, focal, aspect, pp_offset):
    """K with fx = focal, fy = focal / aspect and the principal point pp_offset (fractions of the size) off-centre."""
    return np.array([[focal, 0, width * (0.5 + pp_offset[0])], [0, focal / aspect, height * (0.5 + pp_offset[1])],
                     [0, 0, 1.0]])


def _log_uniform(rng, lo, hi, m):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), m))


def calibrated_view_wide(n, seed=0, width=4000, height=3000, focal=3000.0, aspect=1.0, pp_offset=(0.0, 0.0), angle=None,
                         depth=(4.0, 12.0), forward=False, plane_frac=0.0, noise_px=0.5, outlier_frac=0.3):
    """calibrated_view at hard geometry: images up to 16000 px wide, narrow and wide fields, any rotation up to 60
    degrees, near-pure rotation, forward motion, depth ranges of 1:1000, a dominant plane.

    K has fx = `focal`, fy = focal / `aspect` and the principal point `pp_offset` (fractions of the image size) off the
    centre.  R is a rotation by `angle` radians (None: uniform in [0, pi / 3]) about a random axis.  t is a unit
    baseline: sideways with random y and z parts, or (`forward`) mostly along the optical axis, so that the epipoles lie
    inside the images.  The depths of the points in camera 1 are log-uniform over `depth`, in baselines: (100, 100) is a
    baseline over depth of 1e-2, (0.5, 500) a depth ratio of 1:1000.  `plane_frac` of the points lie on one tilted plane
    through the middle (geometric mean) of the depth range, the rest off it.  A point is kept if it is at least 0.1
    baselines in front of both cameras and projects inside both images; ValueError if the two fields barely overlap.
    Both images get N(0, noise_px); `outlier_frac` of the pairs get uniform-random image-2 positions.

    Returns xy1, xy2 (n x 2 float32 pixels), K (3 x 3), R (3 x 3), t (unit 3-vector; x2 ~ K (R X + t)), X (n x 3 points
    in camera-1 coordinates) and the boolean ground-truth inlier flags, as calibrated_view does.
    """
    rng = np.random.default_rng([seed, 0xE55F])
    K = _wide_camera(width, height, focal, aspect, pp_offset)
    Ki = np.linalg.inv(K)
    axis = rng.normal(size=3)
    th = rng.uniform(0.0, np.pi / 3) if angle is None else float(angle)
    R = _rodrigues(axis, th)
    t = (np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), -1.0]) if forward else
         np.array([1.0, rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)]))
    t /= np.linalg.norm(t)
    nrm = np.array([0.15, -0.2, 1.0])
    d_plane = np.sqrt(depth[0] * depth[1])
    X = np.zeros((0, 3))
    on = np.zeros(0, bool)
    for _ in range(200):
        if X.shape[0] >= n:
            break
        m = 4 * n + 64
        ray = np.c_[rng.uniform([0, 0], [width, height], (m, 2)), np.ones(m)] @ Ki.T
        z = _log_uniform(rng, depth[0], depth[1], m)
        flat = rng.random(m) < plane_frac
        z = np.where(flat, d_plane / (ray @ nrm), z)
        P = ray * z[:, None]
        P2 = P @ R.T + t
        p2 = P2 @ K.T
        with np.errstate(all="ignore"):
            p2 = p2[:, :2] / p2[:, 2:3]
        ok = ((P[:, 2] > 0.1) & (P2[:, 2] > 0.1) & (p2[:, 0] > 0) & (p2[:, 0] < width) & (p2[:, 1] > 0) &
              (p2[:, 1] < height))
        X = np.r_[X, P[ok]]
        on = np.r_[on, flat[ok]]
    if X.shape[0] < n:
        raise ValueError("the two fields of view barely overlap: no scene")
    X = X[:n]
    x1 = X @ K.T
    x1 = x1[:, :2] / x1[:, 2:3]
    x2 = (X @ R.T + t) @ K.T
    x2 = x2[:, :2] / x2[:, 2:3]
    x1 = x1 + rng.normal(0, noise_px, x1.shape)
    x2 = x2 + rng.normal(0, noise_px, x2.shape)
    inl = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.permutation(n)[:n_out]
        inl[bad] = False
        x2[bad] = rng.uniform([0, 0], [width, height], (n_out, 2))
    return (np.ascontiguousarray(x1.astype(np.float32)), np.ascontiguousarray(x2.astype(np.float32)), K, R, t, X, inl)


def pnp_scene_wide(n, seed=0, width=4000, height=3000, focal=3000.0, aspect=1.0, pp_offset=(0.0, 0.0), angle=None,
                   offset=0.0, depth=(4.0, 12.0), thickness=None, collinear_frac=0.0, behind_frac=0.0, noise_px=0.5,
                   outlier_frac=0.3):
    """pnp_scene at hard geometry: any rotation, map coordinates far from the origin, depths of 1:1000, a near-planar
    map, narrow and wide fields, collinear map points, outliers behind the camera.

    K as calibrated_view_wide.  R is a rotation by `angle` radians (None: uniform in [0, pi]) about a random axis; the
    camera sits up to 2 units from the map's own origin, and the whole map is shifted by a vector of length `offset`
    (1e3-1e4: the float32 world coordinates then carry 6e-5 to 1e-3 units of rounding).  Camera-frame depths are
    log-uniform over `depth`; with `thickness` the points lie within thickness * depth of one tilted plane at the
    middle of the depth range instead.  `collinear_frac` of the points (inliers) are moved onto one line through two of
    the map's points, A + k d with A and d on a grid of 2^-10 units and integer k, so that they are EXACTLY collinear in
    float32 (needs offset = 0).  `outlier_frac` of the pixels are uniform-random image positions; `behind_frac` of those
    outliers instead keep their true pixel and get the world point mirrored through the camera centre, which projects
    onto that pixel from behind (w < 0).

    Returns xyz (n x 3 float32 world points), uv (n x 2 float32 pixels), K (3 x 3), R (3 x 3), t (3; x_cam = R X + t) and
    the boolean ground-truth inlier flags, as pnp_scene does.
    """
    if collinear_frac and offset:
        raise ValueError("exactly collinear points need offset = 0")
    rng = np.random.default_rng([seed, 0x9AA0])
    K = _wide_camera(width, height, focal, aspect, pp_offset)
    Ki = np.linalg.inv(K)
    axis = rng.normal(size=3)
    th = rng.uniform(0.0, np.pi) if angle is None else float(angle)
    R = _rodrigues(axis, th)
    t0 = rng.uniform(-2.0, 2.0, 3)
    ray = np.c_[rng.uniform([0, 0], [width, height], (n, 2)), np.ones(n)] @ Ki.T
    if thickness is None:
        z = _log_uniform(rng, depth[0], depth[1], n)
    else:
        nrm = np.array([0.15, -0.2, 1.0])
        d_plane = np.sqrt(depth[0] * depth[1])
        z = d_plane * (1.0 + thickness * rng.uniform(-0.5, 0.5, n)) / (ray @ nrm)
    Xc = ray * z[:, None]
    Xw = (Xc - t0) @ R                                          # world = R^T (x_cam - t0)
    inl = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    order = rng.permutation(n)
    bad = order[:n_out]
    inl[bad] = False
    n_col = int(round(collinear_frac * n))
    if n_col:
        rows = order[n_out:n_out + n_col]
        g = 2.0 ** -10
        A = np.rint(Xw[rows[0]] / g) * g
        d = np.rint((Xw[rows[1]] - A) / 512.0 / g) * g
        Xw[rows] = A + rng.integers(0, 513, n_col)[:, None] * d
    shift = rng.normal(size=3)
    shift *= offset / np.linalg.norm(shift)
    Xw = Xw + shift
    t = t0 - R @ shift
    X32 = Xw.astype(np.float32)
    Xc = X32.astype(np.float64) @ R.T + t                      # pixels of the float32 map points
    uv = Xc @ K.T
    uv = uv[:, :2] / uv[:, 2:3] + rng.normal(0, noise_px, (n, 2))
    if n_out:
        n_beh = int(round(behind_frac * n_out))
        uv[bad[n_beh:]] = rng.uniform([0, 0], [width, height], (n_out - n_beh, 2))
        mirrored = (-Xc[bad[:n_beh]] - t) @ R                   # R X + t = -x_cam
        X32[bad[:n_beh]] = mirrored.astype(np.float32)
    return np.ascontiguousarray(X32), np.ascontiguousarray(uv.astype(np.float32)), K, R, t, inl


def align3d_scene(n, seed=0xA3D, model=0, outlier_frac=0.3, noise=0.01, nan_frac=0.0):
    """3D-3D correspondences of the same tracks in two frames (stereo odometry between two rig poses, two monocular maps
    of different gauge): rows of frame 1 uniform in a box of +-4 units at depths 4-12, frame 2 = s R x1 + t plus
    N(0, noise) on both sides.  R is a rotation of 0.1-0.6 rad about a random axis, t up to 2 units per axis, s = 1 for
    `model` 0 (rigid) and 0.5-2 (log-uniform) for `model` 1 (similarity).  `outlier_frac` of the frame-2 rows are
    replaced by uniform-random positions in the frame-2 box; `nan_frac` of the rows (outliers first) get a NaN row in
    one of the two arrays, the way pm_stereo_points_dev and pm_triangulate_dev mark a missing point.

    Returns xyz1, xyz2 (n x 3 float32), the planted (s, R, t) and the boolean ground-truth inlier flags (False for
    outliers and NaN rows).
    """
    rng = np.random.default_rng([seed, 0xA13D])
    R = _rodrigues(rng.normal(size=3), rng.uniform(0.1, 0.6))
    t = rng.uniform(-2.0, 2.0, 3)
    s = 1.0 if model == 0 else float(np.exp(rng.uniform(np.log(0.5), np.log(2.0))))
    X1 = np.c_[rng.uniform(-4.0, 4.0, (n, 2)), rng.uniform(4.0, 12.0, n)]
    X2 = s * X1 @ R.T + t
    lo, hi = X2.min(axis=0) if n else np.zeros(3), X2.max(axis=0) if n else np.ones(3)
    x1 = X1 + rng.normal(0, noise, (n, 3))
    x2 = X2 + rng.normal(0, noise, (n, 3))
    inl = np.ones(n, bool)
    order = rng.permutation(n)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = order[:n_out]
        inl[bad] = False
        x2[bad] = rng.uniform(lo, hi, (n_out, 3))
    n_nan = int(round(nan_frac * n))
    if n_nan:
        rows = order[:n_nan]
        inl[rows] = False
        side = rng.integers(0, 2, n_nan).astype(bool)
        x1[rows[side]] = np.nan
        x2[rows[~side]] = np.nan
    return np.ascontiguousarray(x1.astype(np.float32)), np.ascontiguousarray(x2.astype(np.float32)), s, R, t, inl


def multiview_scene_wide(n, n_views, seed=0, width=4000, height=3000, focal=3000.0, aspect=1.0, pp_offset=(0.0, 0.0),
                         offset=0.0, world_rot=False, angle=0.1, baseline=0.25, depth=(4.0, 12.0), forward=False,
                         noise_px=0.5, blank_frac=0.0, swap_every=0, first_identity=False):
    """Tracks of n map points over n_views posed views at hard geometry (the scenes of the triangulation and bundle
    adjustment tests): a map far from the origin, any world frame, turns up to 60 degrees between views, small
    parallax, depths of 1:1000, narrow and wide fields, motion along the optical axis.

    K as calibrated_view_wide.  The points are drawn in the frame of view 0: a uniform pixel and a depth log-uniform over
    `depth`.  View v > 0 sits `baseline` times depth[0] (the nearest depth) from view 0, sideways on a ring, or
    (`forward`) on view 0's optical axis towards the points, and is turned by `angle` * v / (n_views - 1) radians about an
    axis 0.3 off the optical axis (mostly roll, so that the points stay in front).  A point is kept if every view sees it
    at least 0.1 * depth[0] in front and within one image size of the image; ValueError if that leaves too few.  Then the
    world frame: with `world_rot` a uniform-random rotation of the whole scene, and a shift of all points and camera
    centres by a vector of length `offset`, so that |t| ~ offset.  Every pixel gets N(0, noise_px); `blank_frac` of the
    observations become NaN rows; with swap_every = k, every k-th track has the pixel of one view (not view 0) replaced
    by a uniform-random one.  `first_identity` gives view 0 the pose None and needs offset = 0 and no world_rot.

    Returns K (fx, fy, cx, cy), uv (a list of (n, 2) f32), Rt (a list of 12 doubles, R row-major then t, x_cam = R X + t;
    None for view 0 with first_identity), X (n x 3 float64 world points) and the boolean flags of the swapped tracks.
    """
    if first_identity and (offset or world_rot):
        raise ValueError("a None pose for view 0 needs offset = 0 and no world rotation")
    rng = np.random.default_rng([seed, 0x3D1E])
    Km = _wide_camera(width, height, focal, aspect, pp_offset)
    K = np.array([Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2]])
    Ki = np.linalg.inv(Km)
    spread = baseline * depth[0]
    Rv, cv = [np.eye(3)], [np.zeros(3)]
    for v in range(1, n_views):
        a = 2 * np.pi * (v + rng.uniform(-0.3, 0.3)) / max(n_views - 1, 1)
        if forward:
            c = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 1.0]) * spread * v / (n_views - 1)
        else:
            c = np.array([np.cos(a), 0.6 * np.sin(a), rng.uniform(-0.15, 0.15)]) * spread * rng.uniform(0.7, 1.0)
        axis = np.array([0.3 * rng.normal(), 0.3 * rng.normal(), 1.0])
        Rv.append(_rodrigues(axis, angle * v / (n_views - 1)))
        cv.append(c)
    X0 = np.zeros((0, 3))
    for _ in range(200):
        if X0.shape[0] >= n:
            break
        m = 4 * n + 64
        ray = np.c_[rng.uniform([0, 0], [width, height], (m, 2)), np.ones(m)] @ Ki.T
        P = ray * _log_uniform(rng, depth[0], depth[1], m)[:, None]
        ok = np.ones(m, bool)
        for Rm, c in zip(Rv, cv):
            Pc = (P - c) @ Rm.T
            with np.errstate(all="ignore"):
                p = Pc @ Km.T
                p = p[:, :2] / p[:, 2:3]
            ok &= ((Pc[:, 2] > 0.1 * depth[0]) & (p[:, 0] > -width) & (p[:, 0] < 2 * width) & (p[:, 1] > -height) &
                   (p[:, 1] < 2 * height))
        X0 = np.r_[X0, P[ok]]
    if X0.shape[0] < n:
        raise ValueError("the fields of view barely overlap: no scene")
    X0 = X0[:n]
    Rw = _rodrigues(rng.normal(size=3), rng.uniform(0.0, np.pi)) if world_rot else np.eye(3)
    shift = rng.normal(size=3)
    shift *= offset / np.linalg.norm(shift)
    X = X0 @ Rw.T + shift
    Rt = []
    for v, (Rm, c) in enumerate(zip(Rv, cv)):
        Rv_w = Rm @ Rw.T
        Rt.append(None if (v == 0 and first_identity) else np.r_[Rv_w.reshape(-1), -Rv_w @ (Rw @ c + shift)])
    uv = []
    for Rm, c in zip(Rv, cv):
        Pc = (X0 - c) @ Rm.T
        p = Pc @ Km.T
        uv.append(p[:, :2] / p[:, 2:3] + rng.normal(0, noise_px, (n, 2)))
    swapped = np.zeros(n, bool)
    if swap_every:
        swapped[::swap_every] = True
        for i in np.nonzero(swapped)[0]:
            uv[1 + rng.integers(0, n_views - 1)][i] = rng.uniform([0, 0], [width, height])
    if blank_frac:
        for v in range(n_views):
            uv[v][rng.random(n) < blank_frac] = np.nan
    return K, [np.ascontiguousarray(u.astype(np.float32)) for u in uv], Rt, X, swapped


def align3d_scene_wide(n, seed=0, model=0, offset=0.0, scale=None, angle=None, span=8.0, flat=1.0, line=1.0, noise=0.01,
                       outlier_frac=0.3, nan_frac=0.0):
    """align3d_scene at hard geometry: frames far from the origin, scales of 1e-3 .. 1e3, rotations of exactly pi or of
    1e-6 rad, flat, thin and collinear clouds, clouds 1e-3 units wide.

    Frame-1 rows are uniform in a cube of side `span` about the origin, its third axis shrunk by `flat` and its second and
    third by `line` (1e-4: a slab or a needle that thin), the cube then turned by a random rotation.  With flat = 0 or
    line = 0 the rows are A + j d1 + k d2 (or A + k d) with A, d1, d2 on a grid of 2^-10 units and integer j, k, so that
    they are EXACTLY coplanar (collinear) in float32; that needs offset = 0 and span = 8.  The rows are then shifted by a
    vector of length `offset`, which frame 2 = s R x1 + t inherits.  R is a rotation by `angle` radians (None: uniform in
    [0, pi]) about a random axis, t up to span / 4 per axis, s = 1 for `model` 0; for `model` 1 `scale`, or log-uniform in
    [0.5, 2] when None.  Frame 1 gets N(0, noise), frame 2 N(0, s * noise) (the same relative noise); `outlier_frac` of
    the frame-2 rows become uniform-random positions in the frame-2 box; `nan_frac` as in align3d_scene.

    Returns xyz1, xyz2 (n x 3 float32), the planted (s, R, t) and the boolean ground-truth inlier flags, as
    align3d_scene does.  With flat = 0 or line = 0 frame 1 carries no noise (it would leave the plane).
    """
    exact = flat == 0 or line == 0
    if exact and (offset or span != 8.0):
        raise ValueError("exactly coplanar or collinear rows need offset = 0 and span = 8")
    rng = np.random.default_rng([seed, 0xA13E])
    R = _rodrigues(rng.normal(size=3), rng.uniform(0.0, np.pi) if angle is None else float(angle))
    t = rng.uniform(-span / 4.0, span / 4.0, 3)
    s = 1.0 if model == 0 else (float(np.exp(rng.uniform(np.log(0.5), np.log(2.0)))) if scale is None else float(scale))
    att = _rodrigues(rng.normal(size=3), rng.uniform(0.0, np.pi))
    if exact:
        g = 2.0 ** -10
        A = np.rint(rng.uniform(-1.0, 1.0, 3) / g) * g
        d1 = np.rint(att[:, 0] * span / 1024.0 / g) * g
        d2 = np.rint(att[:, 1] * span / 1024.0 / g) * g
        j = rng.integers(-512, 513, n)[:, None]
        k = rng.integers(-512, 513, n)[:, None]
        X1 = A + j * d1 + (0 if line == 0 else 1) * k * d2
    else:
        X1 = rng.uniform(-span / 2.0, span / 2.0, (n, 3)) * np.array([1.0, line, line * flat])
        X1 = X1 @ att.T
    shift = rng.normal(size=3)
    shift *= offset / np.linalg.norm(shift)
    X1 = X1 + shift
    X2 = s * X1 @ R.T + t
    lo, hi = X2.min(axis=0) if n else np.zeros(3), X2.max(axis=0) if n else np.ones(3)
    hi = np.maximum(hi, lo + s * span / 8.0)                   # a flat cloud still has outliers off its plane
    x1 = X1 + (0.0 if exact else rng.normal(0, noise, (n, 3)))
    x2 = X2 + rng.normal(0, s * noise, (n, 3))
    inl = np.ones(n, bool)
    order = rng.permutation(n)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = order[:n_out]
        inl[bad] = False
        x2[bad] = rng.uniform(lo, hi, (n_out, 3))
    n_nan = int(round(nan_frac * n))
    if n_nan:
        rows = order[:n_nan]
        inl[rows] = False
        side = rng.integers(0, 2, n_nan).astype(bool)
        x1[rows[side]] = np.nan
        x2[rows[~side]] = np.nan
    return np.ascontiguousarray(x1.astype(np.float32)), np.ascontiguousarray(x2.astype(np.float32)), s, R, t, inl
