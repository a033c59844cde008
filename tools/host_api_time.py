"""Wall time of the host-pointer entry points (what a drop-in caller of main.cpp:46 / :95-98 pays per call, copies,
allocations and the call's own synchronisation included): the matcher and RANSAC-F on the matcher's workloads, then
every host-pointer form of csrc/estimators.cpp at 2275 correspondences (config C3's size) for 1000 and 10 000 samples,
and the second steps alone on the masks those produce.  One line per form: median and min per call after warm-up, over
enough calls that the timed window lasts a second or more.

    python tools/host_api_time.py [substring ...]      (only the forms whose name contains one of the substrings)"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import points_matching_amd as pm
from points_matching_amd import synth

ONLY = sys.argv[1:]
WINDOW_S, WARMUP = 1.0, 50


def timed(name, fn, note=""):
    """Every call is timed on its own (each ends in its own synchronise inside the library)."""
    if ONLY and not any(s in name for s in ONLY):
        return
    for _ in range(WARMUP):
        fn()
    t0 = time.perf_counter()
    for _ in range(20):
        fn()
    calls = max(100, int(1.2 * WINDOW_S * 20 / (time.perf_counter() - t0)))
    dt = np.empty(calls)
    for i in range(calls):
        t0 = time.perf_counter()
        fn()
        dt[i] = time.perf_counter() - t0
    print("%-44s median %9.1f us  min %9.1f us  (%d calls, %.2f s)%s" %
          (name, np.median(dt) * 1e6, dt.min() * 1e6, calls, dt.sum(), note), flush=True)


ctx = pm.Context(0)
for (nq, nt) in ((2048, 2048), (8192, 8192)):
    w = synth.pair_workload(nq, nt, 128, seed=1, kind="sift")
    timed("bf_knn_l2 %dx%d" % (nq, nt), lambda: ctx.bf_knn_l2(w["q"], w["t"], 2, pm.api.PM_KNN_HINT_INTEGER),
          "  copies: %.1f MB in, %.2f MB out" % ((nq + nt) * 512 / 1e6, nq * 32 / 1e6))
    knn = ctx.bf_knn_l2(w["q"], w["t"], 2, pm.api.PM_KNN_HINT_INTEGER)
    good = pm.api.filter_ratio(knn, 0.8)
    x1, x2 = w["kp1"][good["queryIdx"]], w["kp2"][good["trainIdx"]]
    timed("ransac_fundamental n=%d 10000" % x1.shape[0], lambda: ctx.ransac_fundamental(x1, x2, 10000, 1.0, 5))

# ---- the estimators: RANSAC + second step in one call, then the second step alone on that call's model and mask
N, SEED = 2275, 5
FULL, PARTIAL = pm.api.PM_AFFINE_FULL, pm.api.PM_AFFINE_PARTIAL
h1, h2 = synth.planar_view(N, seed=0xC3, outlier_frac=0.3, noise_px=0.5)[:2]
af1, af2 = synth.affine_view(N, seed=0xC3, outlier_frac=0.3, noise_px=0.5)[:2]
ap1, ap2 = synth.affine_view(N, seed=0xC3, outlier_frac=0.3, noise_px=0.5, partial=True)[:2]
e1, e2, Ke = synth.calibrated_view(N, seed=0xC3, outlier_frac=0.3, noise_px=0.5)[:3]
xyz, uv, Kp = synth.pnp_scene(N, seed=0xC3, outlier_frac=0.3, noise_px=0.5)[:3]
Ke, Kp = pm.api._camera(Ke), pm.api._camera(Kp)
for hyps in (1000, 10000):
    timed("ransac_homography_refined %d" % hyps, lambda: ctx.ransac_homography_refined(h1, h2, hyps, 3.0, SEED))
    timed("estimate_affine full %d" % hyps, lambda: ctx.estimate_affine(af1, af2, hyps, 3.0, SEED, model=FULL))
    timed("estimate_affine partial %d" % hyps, lambda: ctx.estimate_affine(ap1, ap2, hyps, 3.0, SEED, model=PARTIAL))
    timed("estimate_pose %d" % hyps, lambda: ctx.estimate_pose(e1, e2, Ke, hyps, 1.0, SEED))
    timed("solve_pnp_ransac %d" % hyps, lambda: ctx.solve_pnp_ransac(xyz, uv, Kp, hyps, 8.0, SEED))

rc, Hm, hmask = ctx.ransac_homography(h1, h2, 1000, 3.0, SEED)[:3]
assert rc == pm.api.PM_OK
timed("homography_refine", lambda: ctx.homography_refine(h1, h2, hmask, Hm))
for tag, model, a1, a2 in (("full", FULL, af1, af2), ("partial", PARTIAL, ap1, ap2)):
    rc, Am, amask = ctx.estimate_affine(a1, a2, 1000, 3.0, SEED, model=model, refine=False)[:3]
    assert rc == pm.api.PM_OK
    timed("affine_refine %s" % tag, lambda: ctx.affine_refine(a1, a2, amask, Am, model=model))
rc, Em, emask = ctx.ransac_essential(e1, e2, Ke, 1000, 1.0, SEED)[:3]
assert rc == pm.api.PM_OK
timed("recover_pose", lambda: ctx.recover_pose(e1, e2, Ke, Em, emask))
timed("recover_pose points", lambda: ctx.recover_pose(e1, e2, Ke, Em, emask, points=True))
rc, Rm, tm, pmask = ctx.ransac_pnp(xyz, uv, Kp, 1000, 8.0, SEED)[:4]
assert rc == pm.api.PM_OK
timed("pnp_refine", lambda: ctx.pnp_refine(xyz, uv, Kp, pmask, Rm, tm))
