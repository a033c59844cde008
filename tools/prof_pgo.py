"""Pose-graph optimisation on one MI355X (docs/SPEC.md S118-S123): a first measurement, no threshold.

    python tools/prof_pgo.py --resources     # no GPU needed: compiles csrc/pose_graph.hip and prints the compiler's remark
    python tools/prof_pgo.py [--reps 3] [--warmup 1] [--sizes 100,1000,10000] [--out profiles/pgo_timing.json]

In one session, one process, on the graphs of tests/pgo_ref.py graph() (a chain of keyframes on a ring plus random loop edges,
about 3 edges per node, measurements 0.1 degrees / 0.2 % off, the start composed along the chain, node 0 held), 100 / 1 000 /
10 000 nodes, both models:
  * pm_pose_graph_optimize_dev by the context's timer (one event pair per launch) at max_iters 0, at max_iters 10 with
    cg_iters 50 (the defaults) and at max_iters 10 with cg_iters 1, alternating rounds over all cases, the median of the rounds;
    the time per Levenberg-Marquardt step is (t(10, 50) - t(0)) / the trial evaluations the call reports, the time per
    conjugate-gradient iteration (t(10, 50) - t(10, 1)) / the difference of the two calls' cg_total (the two calls take
    different paths, so this is an estimate);
  * whether poses, used bytes and the info record equal the restatement tests/pgo_ref.c, and its time on one CPU thread.
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
ROUNDS = 3
SIZES = (100, 1000, 10000)
CONFIGS = ((0, 50), (10, 50), (10, 1))           # (max_iters, cg_iters)


def resources():
    from points_matching_amd import build as B
    src = os.path.join(B.CSRC, "pose_graph.hip")
    r = subprocess.run([B.HIPCC] + B.FLAGS + B.EXTRA["pose_graph.hip"] + ["-x", "hip", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    for ln in r.stderr.splitlines():
        if "remark:" in ln:
            print(ln.split("remark:", 1)[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").rstrip())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES), help="node counts, comma-separated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgo_timing.json"))
    a = ap.parse_args()
    if a.resources:
        return resources()
    import torch
    import points_matching_amd as pm
    from points_matching_amd import api
    import pgo_ref as G
    if not torch.cuda.is_available():
        raise SystemExit("prof_pgo: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    G.lib()
    cases = []
    for n in (int(v) for v in a.sizes.split(",")):
        for model in (api.PM_PGO_RIGID, api.PM_PGO_SIM3):
            g = G.graph(n, 3 * n, model, 30, deg=0.1, rel=0.002)[1:]
            pose, fixed, ab, Z, w = g
            d = dict(g=[torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in g],
                     out=torch.zeros((n, 13), dtype=torch.float64, device=dev), used=torch.zeros(len(ab), dtype=torch.uint8, device=dev),
                     info=torch.zeros(40, dtype=torch.uint8, device=dev),
                     work=torch.zeros(api.pose_graph_workspace(n, len(ab), model), dtype=torch.uint8, device=dev))
            torch.cuda.synchronize()
            print("graph of %d nodes, %d edges, model %d ready" % (n, len(ab), model), flush=True)
            for it, cg in CONFIGS:
                def call(d=d, n=n, E=len(ab), prm=api.pgo_params(model, it, cg)):
                    t = d["g"]
                    ctx.pose_graph_optimize_dev(t[0].data_ptr(), n, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                                None, E, prm, d["out"].data_ptr(), d["used"].data_ptr(), d["work"].data_ptr(),
                                                d["work"].numel(), d["info"].data_ptr())
                cases.append(dict(n=n, model=model, it=it, cg=cg, call=call, d=d, g=g, rounds=[]))
    for c in cases:
        for _ in range(a.warmup):
            c["call"]()
        ctx.synchronize()
    print("warm", flush=True)
    for r in range(ROUNDS):                                      # alternate: every case sees every round
        for c in cases:
            ctx.timing_enable(True)
            ctx.timing_reset()
            for _ in range(a.reps):
                c["call"]()
            ctx.synchronize()
            ms, launches = ctx.timing_get("pose_graph")
            assert launches == a.reps, launches
            c["rounds"].append(ms)
            ctx.timing_enable(False)
        print("round %d done" % r, flush=True)
    recs = []
    for c0, c50, c1 in zip(cases[0::3], cases[1::3], cases[2::3]):
        n, model, d = c50["n"], c50["model"], c50["d"]
        out = {}
        for c in (c50, c1):
            c["call"]()
            ctx.synchronize()
            t0 = time.perf_counter()
            ref = G.run(model, *c["g"], c["it"], c["cg"])
            cpu_s = time.perf_counter() - t0
            info = d["info"].cpu().numpy().view(api.PGO_INFO_DTYPE)[0]
            same = bool((d["out"].cpu().numpy().view(np.uint64) == ref.pose.view(np.uint64)).all() and
                        (d["used"].cpu().numpy() == ref.used).all() and
                        (float(info["cost_in"]), float(info["cost_out"]), int(info["n_edges_used"]), int(info["n_nodes_free"]),
                         int(info["iters"]), int(info["accepted"]), int(info["cg_total"]), int(info["status"])) ==
                        (ref.cost_in, ref.cost_out, ref.n_edges_used, ref.n_nodes_free, ref.iters, ref.accepted, ref.cg_total, ref.status))
            out[c["cg"]] = (ref, cpu_s, same)
        ref, cpu_s, same = out[50]
        ms0, ms50, ms1 = (float(np.median(c["rounds"])) for c in (c0, c50, c1))
        rec = {"nodes": n, "edges": len(c50["g"][2]), "model": "SIM3" if model == api.PM_PGO_SIM3 else "RIGID",
               "edges_used": ref.n_edges_used, "ms_max_iters_0": round(ms0, 4), "ms_max_iters_10_cg_50": round(ms50, 4),
               "ms_max_iters_10_cg_1": round(ms1, 4), "rounds_ms_0": [round(v, 4) for v in c0["rounds"]],
               "rounds_ms_10_cg_50": [round(v, 4) for v in c50["rounds"]], "rounds_ms_10_cg_1": [round(v, 4) for v in c1["rounds"]],
               "trial_evaluations": ref.iters, "accepted": ref.accepted, "cg_iterations_taken": ref.cg_total,
               "cg_iterations_taken_at_cg_1": out[1][0].cg_total,
               "ms_per_lm_step": round((ms50 - ms0) / max(ref.iters, 1), 4),
               "ms_per_cg_iteration": round((ms50 - ms1) / max(ref.cg_total - out[1][0].cg_total, 1), 5),
               "cost_in": ref.cost_in, "cost_out": ref.cost_out, "restatement_one_cpu_thread_ms": round(cpu_s * 1e3, 2),
               "device_equals_restatement": bool(same and out[1][2])}
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    res = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "rounds": ROUNDS,
           "timer": "pm_ctx_timing_get: one event pair per launch, mean per launch; the median of the rounds is reported",
           "graphs": "tests/pgo_ref.py graph(n, 3 n, model, 30, deg=0.1, rel=0.002): a chain on a ring plus 2 n + 1 random loop edges, "
                     "the start composed along the chain, node 0 held; max_iters 10, cg_iters 50, cg_tol 1e-6 unless stated",
           "cases": recs,
           "not_measured": ["hardware counters", "pm_pose_graph_optimize (the host form: staging dominates)", "pm_pgo_move_points_dev",
                            "hub nodes", "the call inside a captured graph", "a multi-workgroup conjugate gradient"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
