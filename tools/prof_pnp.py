"""Kernel times of absolute pose, from pm_ctx_timing_get (hipEvents around each launch): the P3P solve launch
(pnp_solve) and the scoring launch (ransac_p_fused) of pm_ransac_pnp_run_dev and the refinement (pnp_refine, 20 LM
iterations at most) of pm_pnp_refine_dev on RANSAC's mask, at 2275 correspondences (config C3's size) for 1000 samples
and 10 000.  One JSON line per sample count; run it in a process of its own, under a time limit:
    timeout -k 10 300 python3 tools/prof_pnp.py [n reps hyps1 hyps2 ...]      (default: 2275 20 1000 10000)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import points_matching_amd as pm  # noqa: E402
from points_matching_amd import api, synth  # noqa: E402

WARMUP = 3
n = int(sys.argv[1]) if len(sys.argv) > 1 else 2275
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
counts = [int(a) for a in sys.argv[3:]] or [1000, 10000]
dev = torch.device("cuda", 0)
ctx = pm.Context(0)

xyz, uv, K, _, _, _ = synth.pnp_scene(n, seed=0xC3, outlier_frac=0.3, noise_px=0.5)
cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
dx, du = torch.from_numpy(xyz).to(dev), torch.from_numpy(uv).to(dev)
dn = torch.tensor([n], dtype=torch.int32, device=dev)
d_key = torch.zeros(1, dtype=torch.int64, device=dev)
d_Rt = torch.zeros(12, dtype=torch.float64, device=dev)
d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
d_ninl = torch.zeros(1, dtype=torch.int32, device=dev)
d_Rt2 = torch.zeros(12, dtype=torch.float64, device=dev)
view = api.PnpView(dx.data_ptr(), du.data_ptr(), dn.data_ptr(), n, 0)

for hyps in counts:
    def run():
        ctx.ransac_pnp_run_dev(view, cam, 0, hyps, 2.0, 0x5EED, d_key.data_ptr(), d_Rt.data_ptr(), d_mask.data_ptr(), n,
                               d_ninl.data_ptr())
        ctx.pnp_refine_dev(view, cam, d_mask.data_ptr(), d_Rt.data_ptr(), 20, d_Rt2.data_ptr())

    ctx.timing_enable(False)
    for _ in range(WARMUP):
        run()
    ctx.synchronize()
    ctx.timing_reset()
    ctx.timing_enable(True)
    for _ in range(reps):
        run()
    ctx.synchronize()
    out = {"n": n, "samples": hyps, "reps": reps}
    for k in ("pnp_solve", "ransac_p_fused", "pnp_refine"):
        ms, launches = ctx.timing_get(k)
        out[k + "_us"] = round(ms * 1e3, 2)                       # pm_ctx_timing_get: mean per launch
        out[k + "_launches"] = launches
    ctx.timing_enable(False)
    out["inliers"] = int(d_ninl.item())
    print(json.dumps(out), flush=True)
ctx.close()
