"""Inputs shared by test_guided_cpu.py and test_guided_gpu.py (docs/SPEC.md S48-S50): the shape grid with keypoints of a
synthetic scene plus uniform clutter, the batch-boundary scene, the tie scene and the repeated-texture scene."""
import numpy as np

from points_matching_amd import synth
import guided_ref as GR

NQS = (1, 5, 17, 67)
NTS = (1, 63, 64, 65, 200)
KS = (1, 2, 4)
KINDS = (GR.F_SAMPSON, GR.F_SYM, GR.H)
TAUS = {GR.F_SAMPSON: (3.0, 30.0), GR.F_SYM: (3.0, 30.0), GR.H: (3.0, 100.0)}    # px: a tight gate and a loose one
# name -> (descriptor type, row width): S1 with and without a tail, the u8 word and 16-byte paths, two Hamming widths
DESCS = {"f32_128": (GR.DESC_F32, 128), "f32_64": (GR.DESC_F32, 64), "f32_20": (GR.DESC_F32, 20),
         "u8_128": (GR.DESC_U8, 128), "u8_32": (GR.DESC_U8, 32), "ham_32": (GR.DESC_BINARY, 32), "ham_8": (GR.DESC_BINARY, 8)}


def descriptors(desc, width, nq, nt, seed):
    rng = np.random.default_rng([seed, desc, width, nq, nt])
    if desc == GR.DESC_F32:
        return rng.standard_normal((nq, width)).astype(np.float32), rng.standard_normal((nt, width)).astype(np.float32)
    return rng.integers(0, 256, (nq, width), dtype=np.uint8), rng.integers(0, 256, (nt, width), dtype=np.uint8)


def geometry(kind, nq, nt, seed=5):
    """(kp1, kp2, M): the first nq / nt points of a two-view (F) or planar (H) scene of max(nq, nt) correspondences, 30 %
    of them uniform clutter in both images.  Query i and train row i see the same 3-D point unless one is clutter."""
    n = max(nq, nt)
    if kind == GR.H:
        xy1, xy2, M, _ = synth.planar_view(n, seed=seed + n, outlier_frac=0.3)
    else:
        xy1, xy2, M, _ = synth.two_view(n, seed=seed + n, outlier_frac=0.3)
    return np.ascontiguousarray(xy1[:nq]), np.ascontiguousarray(xy2[:nt]), np.ascontiguousarray(M, np.float64)


def grid_cases(kind):
    for nq in NQS:
        for nt in NTS:
            kp1, kp2, M = geometry(kind, nq, nt)
            for tau in TAUS[kind]:
                yield nq, nt, kp1, kp2, M, tau


def batch_scene(seed=9):
    """H = identity, tau = 0.5: query c (c = 0 .. 130) sits alone at (20 c, 100) and exactly c train keypoints lie within
    0.1 px of it, so every admitted count from 0 to 130 occurs; the 8515 train rows are shuffled, so the admitted rows
    of a query are spread over the whole sweep.  Returns (kp1, kp2, H, tau, expected counts)."""
    rng = np.random.default_rng(seed)
    counts = np.arange(131)
    kp1 = np.stack([20.0 * counts, np.full(131, 100.0)], axis=1).astype(np.float32)
    owner = np.repeat(counts, counts)
    kp2 = kp1[owner] + rng.uniform(-0.1, 0.1, (owner.size, 2)).astype(np.float32)
    perm = rng.permutation(owner.size)
    return kp1, np.ascontiguousarray(kp2[perm].astype(np.float32)), np.eye(3), 0.5, counts.astype(np.int32)


def tie_scene(desc, width):
    """One admitted set (H = identity, every keypoint at one spot) of 200 train rows, six of which — rows 3, 64, 70, 71,
    140 and 199 — carry the same descriptor, the nearest one of both queries.  Returns (q, t, kp1, kp2, H, tau, copies)."""
    q, t = descriptors(desc, width, 2, 200, seed=77)
    copies = [3, 64, 70, 71, 140, 199]
    if desc == GR.DESC_F32:
        t[copies] = q[0] + np.float32(0.001)
        q[1] = q[0] + np.float32(0.002)
    else:
        t[copies] = q[0]
        t[copies, 0] ^= 1
        q[1] = q[0]
        q[1, 1] ^= 2
    kp1 = np.full((2, 2), 50.0, np.float32)
    kp2 = np.full((200, 2), 50.0, np.float32)
    return q, t, kp1, kp2, np.eye(3), 1.0, copies


def texture_scene(n=512, copies=2, dim=64, sigma=0.02, seed=21):
    """Repeated texture: n true correspondences of a two-view scene (no clutter); every train descriptor has `copies`
    look-alikes elsewhere in image 2, 40-120 px off the epipolar line of its query.  Train rows 0 .. n-1 are the true
    matches (truth[i] = i), the look-alikes follow.  Returns a dict q, t, kp1, kp2, F, truth."""
    rng = np.random.default_rng(seed)
    xy1, xy2, F, _ = synth.two_view(n, seed=seed, outlier_frac=0.0, noise_px=0.3)
    base = rng.standard_normal((n, dim))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    q = base + sigma * rng.standard_normal((n, dim))
    t = [base + sigma * rng.standard_normal((n, dim))]
    kp2 = [xy2]
    lines = (F @ np.concatenate([xy1.astype(np.float64), np.ones((n, 1))], axis=1).T).T
    normal = lines[:, :2] / np.linalg.norm(lines[:, :2], axis=1, keepdims=True)
    for _ in range(copies):
        t.append(base + sigma * rng.standard_normal((n, dim)))
        off = rng.uniform(40.0, 120.0, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
        kp2.append(xy2 + off * normal)
    return {"q": np.ascontiguousarray(q, np.float32), "t": np.ascontiguousarray(np.concatenate(t), np.float32),
            "kp1": np.ascontiguousarray(xy1, np.float32), "kp2": np.ascontiguousarray(np.concatenate(kp2), np.float32),
            "F": np.ascontiguousarray(F, np.float64), "truth": np.arange(n, dtype=np.int32)}
