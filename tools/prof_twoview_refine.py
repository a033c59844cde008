"""Kernel times of the two-view refinements, from pm_ctx_timing_get (hipEvents around each launch): fundamental_refine
(pm_fundamental_refine_dev on RANSAC-F's mask), pose_refine (pm_pose_refine_dev on the pose mask of pm_estimate_pose) and,
in the same session for comparison, homography_refine (pm_homography_refine_dev on RANSAC-H's mask), each with
max_iters = 10 at 2275 and 9175 correspondences.  One JSON line per size; run it in a process of its own, under a time
limit:
    timeout -k 10 300 python3 tools/prof_twoview_refine.py [reps max_iters n1 n2 ...]      (default: 20 10 2275 9175)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import points_matching_amd as pm  # noqa: E402
from points_matching_amd import api, synth  # noqa: E402

WARMUP = 3
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
sizes = [int(a) for a in sys.argv[3:]] or [2275, 9175]
dev = torch.device("cuda", 0)
ctx = pm.Context(0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


for n in sizes:
    out = {"n": n, "reps": reps, "max_iters": iters}
    info = torch.zeros(32, dtype=torch.uint8, device=dev)
    runs = {}
    # F on RANSAC-F's mask
    xy1, xy2, _, _ = synth.two_view(n, 0xC3)
    rc, F0, mask, c, key = ctx.ransac_fundamental(xy1, xy2, 2000, 1.0, 11)
    f1, f2, fm, fF, fo = up(xy1), up(xy2), up(mask), up(F0.reshape(9)), torch.zeros(9, dtype=torch.float64, device=dev)
    fv = api.PointsView(f1.data_ptr(), f2.data_ptr(), 0, 1, n, 0, 1, 0)
    runs["fundamental_refine"] = lambda: ctx.fundamental_refine_dev(fv, fm.data_ptr(), fF.data_ptr(), iters, fo.data_ptr(), info.data_ptr())
    out["fundamental_inliers"] = c
    # the pose on the pose mask
    p1, p2, K, _, _, _, _ = synth.calibrated_view(n, seed=0xC3, outlier_frac=0.3, noise_px=0.5)
    cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    rc, E0, R0, t0, pmask, c, ng, key = ctx.estimate_pose(p1, p2, cam, 1000, 1.0, 11)
    q1, q2, qm, qi = up(p1), up(p2), up(pmask), up(np.concatenate([R0.reshape(9), t0]))
    qo, qe = torch.zeros(12, dtype=torch.float64, device=dev), torch.zeros(9, dtype=torch.float64, device=dev)
    pv = api.PointsView(q1.data_ptr(), q2.data_ptr(), 0, 1, n, 0, 1, 0)
    runs["pose_refine"] = lambda: ctx.pose_refine_dev(pv, cam, qm.data_ptr(), qi.data_ptr(), iters, qo.data_ptr(), qe.data_ptr(), info.data_ptr())
    out["pose_inliers"] = ng
    # H on RANSAC-H's mask
    h1, h2, _, _ = synth.planar_view(n, seed=0xC3, outlier_frac=0.3, noise_px=0.5)
    rc, H0, hmask, c, key = ctx.ransac_homography(h1, h2, 2000, 1.0, 11)
    g1, g2, gm, gH, go = up(h1), up(h2), up(hmask), up(H0.reshape(9)), torch.zeros(9, dtype=torch.float64, device=dev)
    hv = api.PointsView(g1.data_ptr(), g2.data_ptr(), 0, 1, n, 0, 1, 0)
    runs["homography_refine"] = lambda: ctx.homography_refine_dev(hv, gm.data_ptr(), gH.data_ptr(), iters, go.data_ptr(), info.data_ptr())
    out["homography_inliers"] = c
    for name, run in runs.items():
        ctx.timing_enable(False)
        for _ in range(WARMUP):
            run()
        ctx.synchronize()
        ctx.timing_reset()
        ctx.timing_enable(True)
        for _ in range(reps):
            run()
        ctx.synchronize()
        ms, launches = ctx.timing_get(name)
        out[name + "_us"] = round(ms * 1e3, 2)                    # pm_ctx_timing_get: mean per launch
        out[name + "_launches"] = launches
        out[name + "_lm_passes"] = int(info.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]["iters"])
        ctx.timing_enable(False)
    print(json.dumps(out), flush=True)
ctx.close()
