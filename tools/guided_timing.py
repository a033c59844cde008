"""Guided matching against the unguided matcher on one MI355X (docs/SPEC.md S48-S50, DESIGN.md "Guided k-NN").

    python tools/guided_timing.py [--n 8192] [--tau 3] [--reps 30] [--warmup 5] [--out profiles/guided_timing.json]

Scene: synth.pair_workload(n, n, 128, kind="sift") as u8 rows, true F, Sampson gate.  In one session it records
  * the mean admitted fraction (mean of n_admitted / nt over the queries);
  * the "knn_guided" kernel time from pm_ctx_timing_get (event pairs around the launch, mean over the repetitions after
    warm-up) for k = 2, and the same with tau = 1e-3 px, which admits almost nothing: the gate sweep alone.  Their
    difference is what the distance phase and the top-k cost;
  * the device time of the whole calls by event pairs around them, guided one-call form and pm_bf_knn_l2_u8_ratio_dev
    (the yardstick) alternating on the same inputs: median and quartiles.
No GPU, no numbers: the script fails without a device."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import points_matching_amd as pm  # noqa: E402
from points_matching_amd import api, synth  # noqa: E402


def stats(us):
    us = np.sort(np.asarray(us))
    return {"median": round(float(np.median(us)), 2), "p25": round(float(np.percentile(us, 25)), 2),
            "p75": round(float(np.percentile(us, 75)), 2), "min": round(float(us[0]), 2), "max": round(float(us[-1]), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--tau", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_timing.json"))
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 repetitions"
    if not torch.cuda.is_available():
        raise SystemExit("guided_timing: no GPU")
    n = a.n
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    w = synth.pair_workload(n, n, 128, seed=3, kind="sift")
    q8, t8 = w["q"].astype(np.uint8), w["t"].astype(np.uint8)
    d_q, d_t = torch.from_numpy(q8).to(dev), torch.from_numpy(t8).to(dev)
    d_kp1, d_kp2 = torch.from_numpy(w["kp1"]).to(dev), torch.from_numpy(w["kp2"]).to(dev)
    d_F = torch.from_numpy(np.ascontiguousarray(w["F_gt"], np.float64).reshape(9)).to(dev)
    knn = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    knn_u = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    adm = torch.zeros(n, dtype=torch.int32, device=dev)
    good = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    xy1 = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    xy2 = torch.zeros((n, 2), dtype=torch.float32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def guided_knn(tau):
        ctx.bf_knn_guided_l2_u8_dev(d_q.data_ptr(), n, d_t.data_ptr(), n, 128, d_kp1.data_ptr(), d_kp2.data_ptr(),
                                    api.PM_GUIDE_F_SAMPSON, d_F.data_ptr(), tau, 2, knn.data_ptr(), adm.data_ptr())

    def guided_call():
        ctx.bf_match_guided_l2_u8_dev(d_q.data_ptr(), n, d_t.data_ptr(), n, 128, d_kp1.data_ptr(), d_kp2.data_ptr(),
                                      api.PM_GUIDE_F_SAMPSON, d_F.data_ptr(), a.tau, 0.8, knn.data_ptr(), good.data_ptr(),
                                      xy1.data_ptr(), xy2.data_ptr(), cnt.data_ptr())

    def plain_call():
        ctx.bf_knn_l2_u8_ratio_dev(d_q.data_ptr(), n, d_t.data_ptr(), n, 128, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(),
                                   knn_u.data_ptr(), good.data_ptr(), xy1.data_ptr(), xy2.data_ptr(), cnt.data_ptr())

    res = {"n": n, "dim": 128, "desc": "u8", "gate": "F, Sampson", "tau_px": a.tau, "reps": a.reps, "warmup": a.warmup, "unit": "us"}
    # kernel time from pm_ctx_timing_get: the full gate, then the gate that admits almost nothing
    for label, tau in (("knn_guided", a.tau), ("knn_guided_gate_only", 1e-3)):
        for _ in range(a.warmup):
            guided_knn(tau)
        ctx.synchronize()
        ctx.timing_enable(True)
        ctx.timing_reset()
        for _ in range(a.reps):
            guided_knn(tau)
        ms, launches = ctx.timing_get("knn_guided")
        ctx.timing_enable(False)
        assert launches == a.reps
        frac = float(adm.cpu().numpy().astype(np.float64).mean() / n)
        res[label] = {"kernel_mean_us": round(ms * 1e3, 2), "launches": launches, "mean_admitted_fraction": round(frac, 6),
                      "mean_admitted_rows": round(frac * n, 2)}
    res["distance_phase_and_topk_us"] = round(res["knn_guided"]["kernel_mean_us"] - res["knn_guided_gate_only"]["kernel_mean_us"], 2)
    # whole calls, alternating
    calls = {"guided_one_call": guided_call, "unguided_u8_ratio": plain_call}
    times = {k: [] for k in calls}
    survivors = {}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            torch.cuda.synchronize()
            if rep >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
            g = good[:int(cnt[0])].cpu().numpy().view(pm.MATCH_DTYPE).reshape(-1)
            survivors[name] = {"kept": int(g.size), "correct": int((g["trainIdx"] == w["truth"][g["queryIdx"]]).sum())}
    for name in calls:
        res[name] = dict(stats(times[name]), **survivors[name])
    res["guided_over_unguided_median"] = round(res["guided_one_call"]["median"] / res["unguided_u8_ratio"]["median"], 3)
    text = json.dumps(res)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
