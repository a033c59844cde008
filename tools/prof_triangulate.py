"""Triangulation on one MI355X (docs/SPEC.md S93-S96): a first measurement, no threshold.

    python tools/prof_triangulate.py --resources      # no GPU needed: compiles csrc/triangulate.hip and writes the registers,
                                                      # LDS and scratch of every instantiation to profiles/triangulate_kernel_resources.txt
    python tools/prof_triangulate.py [--reps 20] [--warmup 3] [--out profiles/triangulate_timing.json]

In one session, one process, on the scenes of tests/triangulate_ref.py (0.5 px noise, ~10 % of the observations blanked), 2 000
and 200 000 points, 2, 4 and 8 views, max_iters 0 and 5:
  * pm_triangulate_dev by the context's timer (one event pair per launch, pm_ctx_timing_get), five alternating rounds over all
    cases, the median of the rounds and the rounds themselves; points per second and the bytes the launch moves (pixels in, xyz,
    status, points4, err2 out) with the GB/s that implies;
  * the plain-C restatement tests/triangulate_ref.c on one CPU thread on the same rows, and whether the device outputs equal it;
  * VGPRs, AGPRs, LDS and scratch per instantiation, from profiles/triangulate_kernel_resources.txt.
Counters were not collected.  No GPU, no numbers: the timing mode fails without a device."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RES = os.path.join(ROOT, "profiles", "triangulate_kernel_resources.txt")
ROUNDS = 5
SIZES = (2000, 200000)
VIEWS = (2, 4, 8)
ITERS = (0, 5)
KEYS = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def write_resources():
    from points_matching_amd import build as B
    src = os.path.join(B.CSRC, "triangulate.hip")
    cmd = [B.HIPCC] + B.FLAGS + B.EXTRA["triangulate.hip"] + ["-x", "hip", "-c", src, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    lines = [ln.split("remark:", 1)[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").rstrip()
             for ln in r.stderr.splitlines() if "remark:" in ln]
    os.makedirs(os.path.dirname(RES), exist_ok=True)
    with open(RES, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(RES)


def read_resources():
    """{n_views: {key: int}} from the compiler's remarks."""
    out, cur = {}, None
    for ln in open(RES):
        m = re.search(r"Function Name: .*triangulate_kernelILi(\d)E", ln)
        if m:
            cur = out.setdefault(int(m.group(1)), {})
            continue
        for k in KEYS:
            if cur is not None and ln.strip().startswith(k + ":"):
                cur[k] = int(ln.split(":")[1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate_timing.json"))
    a = ap.parse_args()
    if a.resources:
        return write_resources()
    import torch
    import points_matching_amd as pm
    from points_matching_amd import api
    import triangulate_ref as T
    if not torch.cuda.is_available():
        raise SystemExit("prof_triangulate: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    T.lib()
    cases = []
    for n in SIZES:
        for V in VIEWS:
            K, uv, Rt, X, _ = T.scene(n, V, 70 + V, blank_frac=0.1)
            d_uv = [torch.from_numpy(u).to(dev) for u in uv]
            d_Rt = [None if r is None else torch.from_numpy(np.ascontiguousarray(r)).to(dev) for r in Rt]
            out = dict(xyz=torch.zeros((n, 3), dtype=torch.float32, device=dev), status=torch.zeros(n, dtype=torch.uint8, device=dev),
                       p4=torch.zeros((n, 4), dtype=torch.float32, device=dev), e2=torch.zeros(n, dtype=torch.float32, device=dev),
                       ng=torch.zeros(1, dtype=torch.int32, device=dev))
            views = api.tri_views([u.data_ptr() for u in d_uv], [None if r is None else r.data_ptr() for r in d_Rt], n)
            torch.cuda.synchronize()
            for it in ITERS:
                prm = api.tri_params(3.0, 0.9998, float("inf"), it)

                def call(views=views, prm=prm, out=out, K=K):
                    ctx.triangulate_dev(views, K, prm, out["xyz"].data_ptr(), out["status"].data_ptr(), out["p4"].data_ptr(),
                                        out["e2"].data_ptr(), out["ng"].data_ptr())
                cases.append(dict(n=n, n_views=V, max_iters=it, call=call, keep=(d_uv, d_Rt, out, views), scene=(K, uv, Rt), rounds=[]))
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
            ms, launches = ctx.timing_get("triangulate")
            assert launches == a.reps, launches
            c["rounds"].append(ms)
            ctx.timing_enable(False)
    res_by_v = read_resources() if os.path.exists(RES) else {}
    recs = []
    for c in cases:
        n, V, it = c["n"], c["n_views"], c["max_iters"]
        K, uv, Rt = c["scene"]
        c["call"]()
        ctx.synchronize()
        out = c["keep"][2]
        t0 = time.perf_counter()
        ref = T.run(K, uv, Rt, 3.0, 0.9998, np.inf, it)
        cpu_s = time.perf_counter() - t0
        same = bool((out["xyz"].cpu().numpy().view(np.uint32) == ref.xyz.view(np.uint32)).all() and
                    (out["status"].cpu().numpy() == ref.status).all() and
                    (out["p4"].cpu().numpy().view(np.uint32) == ref.points4.view(np.uint32)).all() and
                    (out["e2"].cpu().numpy().view(np.uint32) == ref.err2.view(np.uint32)).all() and int(out["ng"].item()) == ref.n_good)
        med = float(np.median(c["rounds"]))
        moved = n * (8 * V + 12 + 1 + 16 + 4)
        rec = {"points": n, "n_views": V, "max_iters": it, "ms_median_of_rounds": round(med, 5), "rounds_ms": [round(v, 5) for v in c["rounds"]],
               "points_per_s": round(n / (med * 1e-3)), "bytes_moved": moved, "GB_per_s": round(moved / (med * 1e-3) / 1e9, 2),
               "lm_trial_passes_mean": round(float(ref.iters.mean()), 2), "ok_rows": int(ref.n_good),
               "restatement_one_cpu_thread_ms": round(cpu_s * 1e3, 3), "device_equals_restatement": same}
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    res = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "rounds": ROUNDS,
           "timer": "pm_ctx_timing_get: one event pair per launch, mean per launch; the median of the rounds is reported",
           "scene": "tests/triangulate_ref.py scene(): 0.5 px noise, ~10 % of the observations blanked, max_reproj_px 3, max_cos_parallax 0.9998",
           "cases": recs, "kernel_resources_per_view_count": {str(k): v for k, v in sorted(res_by_v.items())},
           "not_measured": ["hardware counters", "pm_triangulate (the host form: staging dominates)", "3, 5, 6 and 7 views",
                            "PM_TRI_USE_INITIAL", "the call inside a captured graph"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
