"""Semi-global matching on one MI355X (docs/SPEC.md S89-S92): a first measurement, no threshold.

    python tools/prof_sgm.py [--reps 10] [--warmup 2] [--out profiles/sgm_timing.json]

In one session, one process, on the synthetic rectified pairs of tools/prof_stereo.py, 640 x 480 with 64 disparities and
1920 x 1080 with 128, p1 = 4, p2 = 24, uniqueness 10:
  * pm_stereo_sgm_dev with 4 and with 8 paths and pm_stereo_bm_dev at radius 4, by the context's timers (one event pair per
    launch, pm_ctx_timing_get).  The three are taken in rounds, one after the other, so that they share whatever else the
    machine is doing; per kernel the time per map (mean per launch x launches per map), the median of the rounds and the
    rounds themselves;
  * the bytes of S the passes move per map (the first pass writes the volume, the last one reads it, every other pass reads and
    writes it) and the GB/s the time of the path passes implies;
  * the plain-C restatement tests/sgm_ref.c on one CPU thread in the same session and whether the device map equals it.  The
    restatement is brute force, so for 1920 x 1080 both run once more on a band of 64 computed rows cut out of the pair (paths do
    not stop at a band's edge, so the band is matched as an image of its own, on the device as well).
Counters were not collected.  No GPU, no numbers: the script fails without a device."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import points_matching_amd as pm  # noqa: E402
from points_matching_amd import api  # noqa: E402
import sgm_ref as G  # noqa: E402
from prof_stereo import synthetic_pair  # noqa: E402

ROUNDS = 5
P1, P2, UNIQ = 4, 24, 10
CASES = [(640, 480, 64), (1920, 1080, 128)]
BAND = 64                                                        # computed rows of the band the restatement runs on at 1920 x 1080
KERNELS = ("sgm_census", "sgm_path", "sgm_path_winner")


def timed(ctx, names, fn, reps):
    """Per name: mean ms per launch x launches per call."""
    ctx.timing_enable(True)
    ctx.timing_reset()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    out = {}
    for name in names:
        ms, launches = ctx.timing_get(name)
        assert launches and launches % reps == 0, (name, launches)
        out[name] = ms * (launches // reps)
    ctx.timing_enable(False)
    return out


def device_map(ctx, dev, left, right, prm):
    h, w = left.shape
    d_l, d_r = torch.from_numpy(np.ascontiguousarray(left)).to(dev), torch.from_numpy(np.ascontiguousarray(right)).to(dev)
    d_m = torch.zeros((h, w), dtype=torch.int16, device=dev)
    d_info = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.stereo_sgm_dev(d_l.data_ptr(), d_r.data_ptr(), w, h, w, w, prm, d_m.data_ptr(), w, d_info.data_ptr())
    ctx.synchronize()
    return d_m.cpu().numpy(), int(d_info[1].item())


def measure(ctx, dev, w, h, D, a):
    left, right = synthetic_pair(w, h, D)
    d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    d_m = torch.zeros((h, w), dtype=torch.int16, device=dev)
    d_info = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    prm = {p: api.sgm_params(D, P1, P2, p, 0, UNIQ) for p in (4, 8)}
    bm = api.stereo_params(D, 4, 0, UNIQ)
    calls = {
        "sgm_4_paths": (KERNELS, lambda: ctx.stereo_sgm_dev(d_l.data_ptr(), d_r.data_ptr(), w, h, w, w, prm[4], d_m.data_ptr(), w, d_info.data_ptr())),
        "sgm_8_paths": (KERNELS, lambda: ctx.stereo_sgm_dev(d_l.data_ptr(), d_r.data_ptr(), w, h, w, w, prm[8], d_m.data_ptr(), w, d_info.data_ptr())),
        "stereo_bm_radius_4": (("stereo_bm",), lambda: ctx.stereo_bm_dev(d_l.data_ptr(), d_r.data_ptr(), w, h, w, w, bm, d_m.data_ptr(), w,
                                                                          d_info.data_ptr())),
    }
    for _, fn in calls.values():
        for _ in range(a.warmup):
            fn()
    ctx.synchronize()
    per_round = {k: [] for k in calls}
    for _ in range(ROUNDS):                                      # alternate: every call sees every round
        for k, (names, fn) in calls.items():
            per_round[k].append(timed(ctx, names, fn, a.reps))
    x0, x1, y0, y1 = G.computed_rect(w, h, 0, D)
    pixels = (x1 - x0 + 1) * (y1 - y0 + 1)
    out = {}
    for k, (names, fn) in calls.items():
        rec = {}
        for name in names:
            rounds = [r[name] for r in per_round[k]]
            rec[name] = {"ms_per_map_median_of_rounds": round(float(np.median(rounds)), 5), "rounds_ms": [round(v, 5) for v in rounds]}
        totals = [sum(r.values()) for r in per_round[k]]
        rec["all_kernels_ms_per_map"] = {"median_of_rounds": round(float(np.median(totals)), 5), "rounds_ms": [round(v, 5) for v in totals]}
        if k.startswith("sgm"):
            paths = int(k.split("_")[1])
            s_bytes = pixels * D * 2 * (2 * paths - 2)               # one write, paths - 2 read-add-writes, one read
            path_ms = [r["sgm_path"] + r["sgm_path_winner"] for r in per_round[k]]
            rec["s_volume_bytes"] = pixels * D * 2
            rec["s_traffic_bytes_per_map"] = s_bytes
            rec["s_traffic_GB_per_s"] = round(s_bytes / (float(np.median(path_ms)) * 1e-3) / 1e9, 1)
            rec["path_steps_per_map"] = pixels * paths
        out[k] = rec
    # equality with the restatement in the same session
    equal, cpu = {}, {}
    full = w * h <= 640 * 480
    cl, cr = (left, right) if full else (left[h // 2 - BAND // 2 - 3:h // 2 + BAND // 2 + 3], right[h // 2 - BAND // 2 - 3:h // 2 + BAND // 2 + 3])
    for p in (4, 8):
        got, n = device_map(ctx, dev, cl, cr, prm[p])
        t0 = time.perf_counter()
        want, n_want = G.sgm(cl, cr, 0, D, P1, P2, p, UNIQ)
        cpu["sgm_%d_paths" % p] = round(time.perf_counter() - t0, 3)
        equal["sgm_%d_paths" % p] = bool((got == want).all() and n == n_want)
    return {"width": w, "height": h, "num_disp": D, "p1": P1, "p2": P2, "uniqueness": UNIQ, "computed_pixels": pixels, "calls": out,
            "restatement_one_cpu_thread": {"image": [cl.shape[1], cl.shape[0]], "seconds": cpu},
            "device_equals_restatement": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_sgm: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    G.lib()
    res = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "rounds": ROUNDS,
           "timer": "pm_ctx_timing_get: one event pair per launch; per kernel the mean per launch x launches per map, the median of the rounds is reported",
           "cases": [], "not_measured": ["hardware counters", "pm_stereo_sgm (the host form: staging dominates)"]}
    for w, h, D in CASES:
        res["cases"].append(measure(ctx, dev, w, h, D, a))
        print(json.dumps(res["cases"][-1]), flush=True)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
