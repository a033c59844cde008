"""Kernel times of robust affine estimation, from pm_ctx_timing_get (hipEvents around each launch): the one-launch
RANSAC-A kernel (pm_ransac_affine_run_dev) for both models next to the one-launch RANSAC-H kernel
(pm_ransac_homography_run_dev) on the same correspondences and hypothesis count, and the least-squares refit
(pm_affine_refine_dev) on every correspondence as an inlier.  One JSON line per size; run it in a process of its own,
under a time limit:
    timeout -k 10 300 python3 tools/prof_affine.py [hyps reps n1 n2 ...]      (default: 10000 50 512 2275 32768)
Under `rocprofv3 --kernel-trace --stats -d DIR -o affine --output-format csv -- python3 tools/prof_affine.py`, the trace
gives the kernel-only durations; `--summarize` (CPU only) turns it into one JSON object of per-size medians:
    python3 tools/prof_affine.py --summarize DIR/affine_kernel_trace.csv [reps n1 n2 ...]"""
import csv
import json
import os
import statistics
import sys

import numpy as np

WARMUP = 5
KERNELS = (("ransac_a_full", "AModel<0>"), ("ransac_a_partial", "AModel<1>"), ("ransac_h", "HModel"),
           ("affine_refine_full", "affine_refine<0>"), ("affine_refine_partial", "affine_refine<1>"))


def summarize(trace, reps, sizes):
    """Median / min kernel duration (us) per kernel and size: each kernel's launches come in size order, WARMUP + reps
    per size; the warm-up launches are dropped."""
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    out = {"source": "rocprofv3 --kernel-trace", "reps": reps, "warmup": WARMUP, "us": {}}
    for name, tag in KERNELS:
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0 for r in rows if tag in r["Kernel_Name"]]
        assert len(d) == (WARMUP + reps) * len(sizes), (name, len(d))
        per = {}
        for i, n in enumerate(sizes):
            chunk = d[i * (WARMUP + reps) + WARMUP:(i + 1) * (WARMUP + reps)]
            per[str(n)] = {"median": round(statistics.median(chunk), 2), "min": round(min(chunk), 2)}
        out["us"][name] = per
    return out


if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
    reps_ = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    print(json.dumps(summarize(sys.argv[2], reps_, [int(a) for a in sys.argv[4:]] or [512, 2275, 32768]), indent=1))
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import points_matching_amd as pm  # noqa: E402
from points_matching_amd import api, synth  # noqa: E402

hyps = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
sizes = [int(a) for a in sys.argv[3:]] or [512, 2275, 32768]
MODELS = (("full", api.PM_AFFINE_FULL), ("partial", api.PM_AFFINE_PARTIAL))
dev = torch.device("cuda", 0)
ctx = pm.Context(0)


def timed(kernel, fn):
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
    return (round(ms * 1e3, 2) if launches else None), launches


for n in sizes:
    x1, x2, _, _ = synth.affine_view(n, seed=0xC3, outlier_frac=0.3, noise_px=0.5)
    d1, d2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
    dn = torch.tensor([n], dtype=torch.int32, device=dev)
    d_key = torch.zeros(1, dtype=torch.int64, device=dev)
    d_M = torch.zeros(9, dtype=torch.float64, device=dev)
    d_A = torch.zeros(6, dtype=torch.float64, device=dev)
    d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_all = torch.ones(n, dtype=torch.uint8, device=dev)
    d_ninl = torch.zeros(1, dtype=torch.int32, device=dev)
    view = api.PointsView(d1.data_ptr(), d2.data_ptr(), dn.data_ptr(), 1, n, 0, 1, 0)
    out = {"n": n, "hyps": hyps, "reps": reps}
    for name, model in MODELS:
        def run_a(model=model):
            ctx.ransac_affine_run_dev(view, 0, hyps, 1.0, 0x5EED, d_key.data_ptr(), d_M.data_ptr(), d_mask.data_ptr(), n,
                                      d_ninl.data_ptr(), model=model)

        def refit(model=model):
            ctx.affine_refine_dev(view, d_all.data_ptr(), d_M.data_ptr(), d_A.data_ptr(), model=model)

        out["A_" + name + "_us"], out["A_" + name + "_launches"] = timed("ransac_a_fused", run_a)
        out["A_" + name + "_inliers"] = int(d_ninl.item())
        out["refit_" + name + "_us"], out["refit_" + name + "_launches"] = timed("affine_refine", refit)

    def run_h():
        ctx.ransac_homography_run_dev(view, 0, hyps, 1.0, 0x5EED, d_key.data_ptr(), d_M.data_ptr(), d_mask.data_ptr(), n,
                                      d_ninl.data_ptr())

    out["H_us"], out["H_launches"] = timed("ransac_h_fused", run_h)
    out["H_inliers"] = int(d_ninl.item())
    print(json.dumps(out), flush=True)
ctx.close()
