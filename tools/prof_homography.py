"""Kernel time of the one-launch RANSAC-H kernel (pm_ransac_homography_run_dev) next to the one-launch RANSAC-F kernel
(pm_ransac_run_dev) on the same correspondences and hypothesis count, from pm_ctx_timing_get (hipEvents around the
launch).  One JSON line per size; run it in a process of its own, under a time limit:
    timeout -k 10 300 python3 tools/prof_homography.py [hyps reps n1 n2 ...]      (default: 10000 50 2275 512 32768)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import points_matching_amd as pm  # noqa: E402
from points_matching_amd import api, synth  # noqa: E402

hyps = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
sizes = [int(a) for a in sys.argv[3:]] or [2275, 512, 32768]
WARMUP = 5
dev = torch.device("cuda", 0)
ctx = pm.Context(0)
for n in sizes:
    x1, x2, _, _ = synth.planar_view(n, seed=0xC3, outlier_frac=0.3, noise_px=0.5)
    d1, d2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
    dn = torch.tensor([n], dtype=torch.int32, device=dev)
    d_key = torch.zeros(1, dtype=torch.int64, device=dev)
    d_M = torch.zeros(9, dtype=torch.float64, device=dev)
    d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_ninl = torch.zeros(1, dtype=torch.int32, device=dev)
    view = api.PointsView(d1.data_ptr(), d2.data_ptr(), dn.data_ptr(), 1, n, 0, 1, 0)

    def run_h():
        ctx.ransac_homography_run_dev(view, 0, hyps, 1.0, 0x5EED, d_key.data_ptr(), d_M.data_ptr(), d_mask.data_ptr(), n,
                                      d_ninl.data_ptr())

    def run_f():
        ctx.ransac_run_dev(d1.data_ptr(), d2.data_ptr(), n, dn.data_ptr(), 0, hyps, 1.0, 0x5EED, d_key.data_ptr(),
                           d_M.data_ptr(), d_mask.data_ptr(), d_ninl.data_ptr())

    out = {"n": n, "hyps": hyps, "reps": reps}
    for name, kernel, fn in (("H", "ransac_h_fused", run_h), ("F", "ransac_fused", run_f)):
        ctx.timing_enable(False)
        for _ in range(WARMUP):
            fn()
        ctx.synchronize()
        ctx.timing_reset()
        ctx.timing_enable(True)
        for _ in range(reps):
            fn()
        ctx.synchronize()
        ms, launches = ctx.timing_get(kernel)
        ctx.timing_enable(False)
        out[name + "_kernel"] = kernel
        out[name + "_us"] = round(ms * 1e3, 2) if launches else None
        out[name + "_launches"] = launches
        out[name + "_inliers"] = int(d_ninl.item())
    print(json.dumps(out), flush=True)
ctx.close()
