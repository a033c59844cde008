"""A/B of the u8 two-buffer coarse kernel's super-tile sizes (PM_OPT_KNN_SUPERTILE 1 / 2 / 3 = 1 / 2 / 4 tiles per LDS
buffer and per barrier): hipEvent mean of the coarse launch, three alternating rounds, SIFT-like data with the u8 hint.
    python tools/sweep_supertile.py [n ...]          (default: 8192 32768, square shapes)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import points_matching_amd as pm  # noqa: E402
from points_matching_amd import synth  # noqa: E402

TIMERS = {1: "knn_l2_mfma_u8", 2: "knn_l2_mfma_u8_s2", 3: "knn_l2_mfma_u8_s4"}
sizes = [int(a) for a in sys.argv[1:]] or [8192, 32768]
dev = torch.device("cuda", 0)
ctx = pm.Context(0)
for n in sizes:
    w = synth.pair_workload(n, n, 128, seed=0xC3, kind="sift")
    d_q, d_t = torch.from_numpy(w["q"]).to(dev), torch.from_numpy(w["t"]).to(dev)
    d_out = torch.empty((n, 2, 4), dtype=torch.int32, device=dev)

    def run(reps):
        for _ in range(reps):
            ctx.bf_knn_l2_dev(d_q.data_ptr(), n, d_t.data_ptr(), n, 128, 2, d_out.data_ptr(), pm.api.PM_KNN_HINT_U8)

    res, ref = {}, None
    for rnd in range(3):
        for s in (1, 2, 3):
            ctx.set_option(pm.api.PM_OPT_KNN_SUPERTILE, s)
            run(5)
            ctx.synchronize()
            ctx.timing_enable(True)
            ctx.timing_reset()
            run(40 if n <= 8192 else 10)
            us = ctx.timing_get(TIMERS[s])[0] * 1e3
            ctx.timing_enable(False)
            out = d_out.cpu().numpy()
            ref = out if ref is None else ref
            res.setdefault(s, []).append(us)
            print("n %d round %d option %d coarse %.2f us same-as-first %s" % (n, rnd, s, us, bool((out == ref).all())), flush=True)
    for s, v in res.items():
        print("n %d option %d: median %.2f min %.2f" % (n, s, float(np.median(v)), min(v)), flush=True)
ctx.set_option(pm.api.PM_OPT_KNN_SUPERTILE, 0)
