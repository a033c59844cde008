"""Kernel time of the refinement of the robust homography (pm_homography_refine_dev: S23 refit + S24 LM, one launch of
one workgroup) after a RANSAC-H run on the same correspondences, from pm_ctx_timing_get (hipEvents around the launch).
One JSON line per size; run it in a process of its own, under a time limit (and under rocprofv3 --kernel-trace --stats
for the profiler's own figure):
    timeout -k 10 300 python3 tools/prof_homography_refine.py [max_iters reps n1 n2 ...]   (default: 10 50 2275 32768)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import points_matching_amd as pm  # noqa: E402
from points_matching_amd import api, synth  # noqa: E402

max_iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
sizes = [int(a) for a in sys.argv[3:]] or [2275, 32768]
HYPS = 10000
WARMUP = 5
dev = torch.device("cuda", 0)
ctx = pm.Context(0)
for n in sizes:
    x1, x2, _, _ = synth.planar_view(n, seed=0xC3, outlier_frac=0.3, noise_px=0.5)
    d1, d2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
    dn = torch.tensor([n], dtype=torch.int32, device=dev)
    d_key = torch.zeros(1, dtype=torch.int64, device=dev)
    d_H = torch.zeros(9, dtype=torch.float64, device=dev)
    d_Hr = torch.zeros(9, dtype=torch.float64, device=dev)
    d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_ninl = torch.zeros(1, dtype=torch.int32, device=dev)
    d_info = torch.zeros(32, dtype=torch.uint8, device=dev)
    view = api.PointsView(d1.data_ptr(), d2.data_ptr(), dn.data_ptr(), 1, n, 0, 1, 0)
    ctx.ransac_homography_run_dev(view, 0, HYPS, 1.0, 0x5EED, d_key.data_ptr(), d_H.data_ptr(), d_mask.data_ptr(), n,
                                  d_ninl.data_ptr())

    def run():
        ctx.homography_refine_dev(view, d_mask.data_ptr(), d_H.data_ptr(), max_iters, d_Hr.data_ptr(), d_info.data_ptr())

    ctx.timing_enable(False)
    for _ in range(WARMUP):
        run()
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    for _ in range(reps):
        run()
    ctx.synchronize()
    ms, launches = ctx.timing_get("homography_refine")
    ctx.timing_enable(False)
    info = d_info.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]
    print(json.dumps({"n": n, "max_iters": max_iters, "reps": reps, "inliers": int(d_ninl.item()),
                      "lm_iters": int(info["iters"]), "status": int(info["status"]),
                      "cost_in": float(info["cost_in"]), "cost_out": float(info["cost_out"]),
                      "refine_us": round(ms * 1e3, 2) if launches else None, "launches": launches}), flush=True)
ctx.close()
