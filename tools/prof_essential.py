"""Kernel times of calibrated relative pose, from pm_ctx_timing_get (hipEvents around each launch): the 5-point solve
launch (essential_solve), the scoring launch (ransac_e_fused) of pm_ransac_essential_run_dev and the one-workgroup pose
recovery (recover_pose) of pm_recover_pose_dev on RANSAC's mask, at 2275 correspondences (config C3) for 1000 samples
(OpenCV's default maxIters [recalled]) and 10 000.  One JSON line per sample count; run it in a process of its own,
under a time limit:
    timeout -k 10 300 python3 tools/prof_essential.py [n reps hyps1 hyps2 ...]      (default: 2275 20 1000 10000)
Under `rocprofv3 --kernel-trace --stats -d DIR -o essential --output-format csv -- python3 tools/prof_essential.py`,
the trace gives the kernel-only durations; `--summarize` (CPU only) turns it into one JSON object of per-count medians:
    python3 tools/prof_essential.py --summarize DIR/essential_kernel_trace.csv [reps hyps1 hyps2 ...]"""
import csv
import json
import os
import statistics
import sys

WARMUP = 3
KERNELS = (("essential_solve", "essential_solve"), ("ransac_e_fused", "EModel"), ("recover_pose", "recover_pose_kernel"))


def summarize(trace, reps, counts):
    """Median / min kernel duration (us) per kernel and sample count: each kernel's launches come in count order,
    WARMUP + reps per count; the warm-up launches are dropped."""
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    out = {"source": "rocprofv3 --kernel-trace", "reps": reps, "warmup": WARMUP, "us": {}}
    for name, tag in KERNELS:
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0 for r in rows if tag in r["Kernel_Name"]]
        assert len(d) == (WARMUP + reps) * len(counts), (name, len(d))
        per = {}
        for i, h in enumerate(counts):
            chunk = d[i * (WARMUP + reps) + WARMUP:(i + 1) * (WARMUP + reps)]
            per[str(h)] = {"median": round(statistics.median(chunk), 2), "min": round(min(chunk), 2)}
        out["us"][name] = per
    return out


if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
    reps_ = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    print(json.dumps(summarize(sys.argv[2], reps_, [int(a) for a in sys.argv[4:]] or [1000, 10000]), indent=1))
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import points_matching_amd as pm  # noqa: E402
from points_matching_amd import api, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2275
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
counts = [int(a) for a in sys.argv[3:]] or [1000, 10000]
dev = torch.device("cuda", 0)
ctx = pm.Context(0)

x1, x2, K, _, _, _, _ = synth.calibrated_view(n, seed=0xC3, outlier_frac=0.3, noise_px=0.5)
cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
d1, d2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
dn = torch.tensor([n], dtype=torch.int32, device=dev)
d_key = torch.zeros(1, dtype=torch.int64, device=dev)
d_E = torch.zeros(9, dtype=torch.float64, device=dev)
d_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
d_ninl = torch.zeros(1, dtype=torch.int32, device=dev)
d_R, d_t = torch.zeros(9, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
d_pm = torch.zeros(n, dtype=torch.uint8, device=dev)
d_ng = torch.zeros(1, dtype=torch.int32, device=dev)
view = api.PointsView(d1.data_ptr(), d2.data_ptr(), dn.data_ptr(), 1, n, 0, 1, 0)

for hyps in counts:
    def run():
        ctx.ransac_essential_run_dev(view, cam, 0, hyps, 1.0, 0x5EED, d_key.data_ptr(), d_E.data_ptr(), d_mask.data_ptr(),
                                     n, d_ninl.data_ptr())
        ctx.recover_pose_dev(view, cam, d_E.data_ptr(), d_mask.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), d_pm.data_ptr(),
                             d_ng.data_ptr())

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
    for k in ("essential_solve", "ransac_e_fused", "recover_pose"):
        ms, launches = ctx.timing_get(k)
        out[k + "_us"] = round(ms * 1e3, 2)
        out[k + "_launches"] = launches
    ctx.timing_enable(False)
    out["inliers"] = int(d_ninl.item())
    out["n_good"] = int(d_ng.item())
    print(json.dumps(out), flush=True)
ctx.close()
