"""Local bundle adjustment on one MI355X (docs/SPEC.md S113-S117): a first measurement, no threshold.

    python tools/prof_ba.py --resources     # no GPU needed: compiles csrc/bundle_adjust.hip and prints the compiler's remark
    python tools/prof_ba.py [--reps 10] [--warmup 3] [--out profiles/ba_timing.json]

In one session, one process, on the perturbed scenes of tests/ba_ref.py (0.5 px noise, ~10 % of the observations blanked, free
poses turned by 0.5 degrees and shifted by N(0, 0.02), points shifted by N(0, 0.05)), 500 / 2 000 / 8 000 points, 3 and 8 views,
view 0 held:
  * pm_bundle_adjust_dev at max_iters 0 and 10 by the context's timer (one event pair per launch), five alternating rounds over
    all cases, the median of the rounds; the time per iteration is (t10 - t0) / the trial evaluations the call reports; the map
    rows are put back before every launch, outside the event pair;
  * whether poses, rows, used bytes and the info record equal the restatement tests/ba_ref.c, and its time on one CPU thread;
  * the alternation a caller has without this call, on the same scene and stream: per round pm_pnp_refine_dev (2 iterations) for
    every free view on its used observations, then pm_triangulate_dev under PM_TRI_USE_INITIAL (2 iterations, gates wide open);
    each round timed by an event pair, and after each round the cost over the bundle adjustment's used set by a float64 numpy
    evaluation.  Reported: the cost after the rounds that fit into the stream time of the 10-iteration call, and the trajectory.
Counters were not collected.  No GPU, no numbers: the timing mode fails without a device."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ROUNDS = 5
SIZES = (500, 2000, 8000)
VIEWS = (3, 8)
ALT_ROUNDS = 40


def resources():
    from points_matching_amd import build as B
    src = os.path.join(B.CSRC, "bundle_adjust.hip")
    r = subprocess.run([B.HIPCC] + B.FLAGS + B.EXTRA["bundle_adjust.hip"] + ["-x", "hip", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    for ln in r.stderr.splitlines():
        if "remark:" in ln:
            print(ln.split("remark:", 1)[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").rstrip())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_timing.json"))
    a = ap.parse_args()
    if a.resources:
        return resources()
    import torch
    import points_matching_amd as pm
    from points_matching_amd import api
    import ba_ref as B
    if not torch.cuda.is_available():
        raise SystemExit("prof_ba: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    B.lib()
    cases = []
    for n in SIZES:
        for V in VIEWS:
            K, uv, Rt, Rt0, xyz0, X = B.perturbed(n, V, 70 + V, 1)
            d = dict(uv=[torch.from_numpy(u).to(dev) for u in uv],
                     P=torch.from_numpy(np.array([np.zeros(12) if r is None else r for r in Rt0])).to(dev),
                     out=torch.zeros((V, 12), dtype=torch.float64, device=dev), start=torch.from_numpy(xyz0).to(dev),
                     xyz=torch.from_numpy(xyz0.copy()).to(dev), used=torch.zeros(n, dtype=torch.uint8, device=dev),
                     info=torch.zeros(40, dtype=torch.uint8, device=dev),
                     work=torch.zeros(api.bundle_adjust_workspace(V, n), dtype=torch.uint8, device=dev))
            d["views"] = api.tri_views([u.data_ptr() for u in d["uv"]],
                                       [None if r is None else d["P"].data_ptr() + 96 * v for v, r in enumerate(Rt0)], n)
            torch.cuda.synchronize()
            for it in (0, 10):
                def call(d=d, K=K, prm=api.ba_params(1, it)):
                    d["xyz"].copy_(d["start"])
                    ctx.bundle_adjust_dev(d["views"], K, prm, d["out"].data_ptr(), d["xyz"].data_ptr(), d["used"].data_ptr(),
                                          d["work"].data_ptr(), d["work"].numel(), d["info"].data_ptr())
                cases.append(dict(n=n, V=V, it=it, call=call, d=d, scene=(K, uv, Rt0, xyz0), rounds=[]))
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
            ms, launches = ctx.timing_get("bundle_adjust")
            assert launches == a.reps, launches
            c["rounds"].append(ms)
            ctx.timing_enable(False)
    recs = []
    for c0, c10 in zip(cases[0::2], cases[1::2]):
        n, V, d = c10["n"], c10["V"], c10["d"]
        K, uv, Rt0, xyz0 = c10["scene"]
        c10["call"]()
        ctx.synchronize()
        t0 = time.perf_counter()
        ref = B.run(K, uv, Rt0, xyz0, 1, 10)
        cpu_s = time.perf_counter() - t0
        info = d["info"].cpu().numpy().view(api.BA_INFO_DTYPE)[0]
        same = bool((d["out"].cpu().numpy().view(np.uint64) == ref.Rt.view(np.uint64)).all() and
                    (d["xyz"].cpu().numpy().view(np.uint32) == ref.xyz.view(np.uint32)).all() and
                    (d["used"].cpu().numpy() == ref.used).all() and
                    (float(info["cost_in"]), float(info["cost_out"]), int(info["iters"]), int(info["accepted"]), int(info["status"])) ==
                    (ref.cost_in, ref.cost_out, ref.iters, ref.accepted, ref.status))
        ms0, ms10 = float(np.median(c0["rounds"])), float(np.median(c10["rounds"]))
        # ---- the alternation on the same scene and stream
        masks = [torch.from_numpy(((ref.used >> v) & 1).astype(np.uint8)).to(dev) for v in range(V)]
        P = torch.from_numpy(np.array([np.zeros(12) if r is None else r for r in Rt0])).to(dev)
        xyz = torch.from_numpy(xyz0.copy()).to(dev)
        status = torch.zeros(n, dtype=torch.uint8, device=dev)
        views = api.tri_views([u.data_ptr() for u in d["uv"]], [None if r is None else P.data_ptr() + 96 * v for v, r in enumerate(Rt0)], n)
        tri = api.tri_params(1e6, 1.0, float("inf"), 2, api.PM_TRI_USE_INITIAL)

        def alt_round():
            for v in range(1, V):
                ctx.pnp_refine_dev(api.PnpView(xyz.data_ptr(), d["uv"][v].data_ptr(), None, n, 0), K, masks[v].data_ptr(),
                                   P.data_ptr() + 96 * v, 2, P.data_ptr() + 96 * v)
            ctx.triangulate_dev(views, K, tri, xyz.data_ptr(), status.data_ptr())

        for _ in range(a.warmup):                                # warm the two kernels on scratch copies of the state
            alt_round()
        ctx.synchronize()
        P.copy_(torch.from_numpy(np.array([np.zeros(12) if r is None else r for r in Rt0])).to(dev))
        xyz.copy_(torch.from_numpy(xyz0).to(dev))
        torch.cuda.synchronize()
        traj, total = [], 0.0
        for r in range(ALT_ROUNDS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            alt_round()
            e1.record(st)
            torch.cuda.synchronize()
            total += e0.elapsed_time(e1)
            poses = [None if Rt0[v] is None else P[v].cpu().numpy() for v in range(V)]
            rows = xyz.cpu().numpy().astype(np.float64)
            lost = int(np.isnan(rows[ref.used != 0]).any(1).sum())
            keep = np.where(np.isnan(rows).any(1), 0, ref.used).astype(np.uint8)
            traj.append((round(total, 4), round(B.np_cost(K, uv, poses, np.nan_to_num(rows), keep), 3), lost))
        fit = [t for t in traj if t[0] <= ms10]
        rec = {"points": n, "n_views": V, "used_points": ref.n_points, "used_observations": ref.n_obs,
               "ms_max_iters_0": round(ms0, 4), "ms_max_iters_10": round(ms10, 4), "rounds_ms_0": [round(v, 4) for v in c0["rounds"]],
               "rounds_ms_10": [round(v, 4) for v in c10["rounds"]], "trial_evaluations": ref.iters, "accepted": ref.accepted,
               "ms_per_iteration": round((ms10 - ms0) / max(ref.iters, 1), 4), "cost_in": ref.cost_in, "cost_out": ref.cost_out,
               "restatement_one_cpu_thread_ms": round(cpu_s * 1e3, 2), "device_equals_restatement": same,
               "alternation_rounds_within_ms10": len(fit), "alternation_cost_within_ms10": fit[-1][1] if fit else None,
               "alternation_ms_per_round": round(total / ALT_ROUNDS, 4),
               "alternation_trajectory_ms_cost_lost_points": traj}
        recs.append(rec)
        print(json.dumps({k: v for k, v in rec.items() if k != "alternation_trajectory_ms_cost_lost_points"}), flush=True)
    res = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "rounds": ROUNDS,
           "timer": "pm_ctx_timing_get: one event pair per launch, mean per launch; the median of the rounds is reported.  "
                    "The alternation: one torch event pair per round on the same stream, a single pass of %d rounds" % ALT_ROUNDS,
           "scene": "tests/ba_ref.py perturbed(): 0.5 px noise, ~10 % blanked, free poses 0.5 degrees and N(0, 0.02) off, points "
                    "N(0, 0.05) off, view 0 held, gate off",
           "alternation": "per round: pm_pnp_refine_dev (2 iterations) for each free view on the used observations, then "
                          "pm_triangulate_dev under PM_TRI_USE_INITIAL (2 iterations, max_reproj_px 1e6, parallax test off); its cost is "
                          "a float64 numpy evaluation over the bundle adjustment's used set (points it turned to NaN are left out and counted)",
           "cases": recs,
           "not_measured": ["hardware counters", "pm_bundle_adjust (the host form: staging dominates)", "2, 4-7 views", "gate_px > 0",
                            "two held poses", "the call inside a captured graph", "other alternation schedules than 2 + 2 iterations"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
