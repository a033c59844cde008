"""3-D to 3-D alignment on one MI355X (docs/SPEC.md S97-S101): a first measurement, no threshold.

    python tools/prof_align3d.py [--reps 20] [--warmup 3] [--out profiles/align3d_timing.json]

In one session, one process, 2275 and 32768 rows, 10 000 samples, both models, on synth.align3d_scene (30 % outliers, 1 % NaN
rows):
  * align3d_solve, ransac_align3d_fused and align3d_refine by the context's timer (one event pair per launch,
    pm_ctx_timing_get), five alternating rounds over all cases, the median of the rounds and the rounds themselves;
  * pm_ransac_pnp_run_dev (pnp_solve + ransac_p_fused) at the same sizes and sample count on synth.pnp_scene, in the same
    rounds, as the yardstick: 4 candidates per sample against 1, 5 operand planes against 6;
  * whether the device results equal the plain-C restatement tests/align3d_ref.c (at 2275 rows; 32768 rows x 10 000 samples
    is left to the test suite's shorter runs).
Counters were not collected.  No GPU, no numbers: the tool fails without a device."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ROUNDS = 5
SIZES = (2275, 32768)
SAMPLES = 10000
THRESH = 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align3d_timing.json"))
    a = ap.parse_args()
    import torch
    import points_matching_amd as pm
    from points_matching_amd import api, synth
    import align3d_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("prof_align3d: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    R.lib()
    cases = []
    for n in SIZES:
        for model in (api.PM_ALIGN3D_RIGID, api.PM_ALIGN3D_SIMILARITY):
            out = dict(k=torch.zeros(1, dtype=torch.int64, device=dev), T=torch.zeros(13, dtype=torch.float64, device=dev),
                       m=torch.zeros(n, dtype=torch.uint8, device=dev), c=torch.zeros(1, dtype=torch.int32, device=dev),
                       T2=torch.zeros(13, dtype=torch.float64, device=dev), info=torch.zeros(32, dtype=torch.uint8, device=dev))
            x1, x2, *_ = synth.align3d_scene(n, seed=n + model, model=model, outlier_frac=0.3, noise=0.01, nan_frac=0.01)
            d1, d2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
            view = api.XyzView(d1.data_ptr(), d2.data_ptr(), None, n, 0)

            def call(view=view, out=out, model=model, n=n):
                ctx.ransac_align3d_run_dev(view, 0, SAMPLES, THRESH, 7, out["k"].data_ptr(), out["T"].data_ptr(), out["m"].data_ptr(), n,
                                           out["c"].data_ptr(), model=model)
                ctx.align3d_refine_dev(view, out["m"].data_ptr(), out["T"].data_ptr(), out["T2"].data_ptr(), out["info"].data_ptr(),
                                       model=model)
            cases.append(dict(family="align3d", rows=n, model=model, call=call, keep=(d1, d2, view, out), scene=(x1, x2),
                              timers=("align3d_solve", "ransac_align3d_fused", "align3d_refine"), rounds=[]))
        xyz, uv, Kg, *_ = synth.pnp_scene(n, seed=n, outlier_frac=0.3)
        K = (Kg[0, 0], Kg[1, 1], Kg[0, 2], Kg[1, 2])
        dx, du = torch.from_numpy(xyz).to(dev), torch.from_numpy(uv).to(dev)
        pview = api.PnpView(dx.data_ptr(), du.data_ptr(), None, n, 0)
        pout = dict(k=torch.zeros(1, dtype=torch.int64, device=dev), Rt=torch.zeros(12, dtype=torch.float64, device=dev),
                    m=torch.zeros(n, dtype=torch.uint8, device=dev), c=torch.zeros(1, dtype=torch.int32, device=dev))

        def pcall(pview=pview, pout=pout, K=K, n=n):
            ctx.ransac_pnp_run_dev(pview, K, 0, SAMPLES, 2.0, 7, pout["k"].data_ptr(), pout["Rt"].data_ptr(), pout["m"].data_ptr(), n,
                                   pout["c"].data_ptr())
        cases.append(dict(family="pnp", rows=n, model=None, call=pcall, keep=(dx, du, pview, pout), scene=None,
                          timers=("pnp_solve", "ransac_p_fused"), rounds=[]))
    torch.cuda.synchronize()
    for c in cases:
        for _ in range(a.warmup):
            c["call"]()
    ctx.synchronize()
    for _ in range(ROUNDS):                                      # alternate: every case sees every round
        for c in cases:
            ctx.timing_enable(True)
            ctx.timing_reset()
            for _ in range(a.reps):
                c["call"]()
            ctx.synchronize()
            row = {}
            for name in c["timers"]:
                ms, launches = ctx.timing_get(name)
                assert launches == a.reps, (name, launches)
                row[name] = ms
            c["rounds"].append(row)
            ctx.timing_enable(False)
    recs = []
    for c in cases:
        rec = {"family": c["family"], "rows": c["rows"], "samples": SAMPLES}
        if c["family"] == "align3d":
            rec["model"] = "similarity" if c["model"] else "rigid"
        for name in c["timers"]:
            vals = [r[name] for r in c["rounds"]]
            rec[name + "_ms_median_of_rounds"] = round(float(np.median(vals)), 5)
            rec[name + "_rounds_ms"] = [round(v, 5) for v in vals]
        if c["family"] == "align3d":
            out = c["keep"][3]
            rec["inliers"] = int(out["c"].item())
            if c["rows"] == SIZES[0]:
                x1, x2 = c["scene"]
                kr, Tr, mr, cr = R.run(c["model"], x1, x2, SAMPLES, THRESH, 7)
                ref, ri = R.refine(c["model"], x1, x2, mr, Tr)
                rec["device_equals_restatement"] = bool(
                    (int(out["k"].item()) & ((1 << 64) - 1)) == kr and (out["m"].cpu().numpy() == mr).all() and
                    (out["T"].cpu().numpy().view(np.uint64) == Tr.view(np.uint64)).all() and
                    (out["T2"].cpu().numpy().view(np.uint64) == ref.view(np.uint64)).all())
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    res = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "rounds": ROUNDS,
           "timer": "pm_ctx_timing_get: one event pair per launch, mean per launch; the median of the rounds is reported",
           "scene": "synth.align3d_scene: 30 % outliers, noise 0.01, 1 % NaN rows, threshold 0.1; synth.pnp_scene: 30 % outliers, 2 px",
           "cases": recs,
           "not_measured": ["hardware counters", "the host forms (staging dominates)", "the calls inside a captured graph",
                            "pm_transform_points3_dev and pm_gather_align3d_dev (one thread per row, bandwidth-bound)"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
