"""Dense stereo on one MI355X (docs/SPEC.md S85-S87): a first measurement, no threshold.

    python tools/prof_stereo.py [--reps 20] [--warmup 3] [--out profiles/stereo_timing.json]

In one session, one process, on synthetic rectified pairs (a smoothed seeded texture, the right image the left one shifted by a
disparity that ramps over the frame, +-3 noise) of 496 x 330 with 64 disparities, 640 x 480 with 64 and with 128, and
1920 x 1080 with 128, each at radius 4 and radius 10, uniqueness 10:
  * stereo_bm (left map), stereo_bm with PM_STEREO_FROM_RIGHT, stereo_lr_check and stereo_points (2000 points) by the context's
    timers (one event pair per launch, pm_ctx_timing_get); the kernels are taken in rounds, one after the other, so that they
    share whatever else the machine is doing; the median of the rounds and the rounds themselves are reported;
  * next to each block-matching time the costs per second: computed pixels x disparities / time (a cost is one window sum);
  * the plain-C restatement tests/stereo_ref.c on one CPU thread in the same session, its time and its costs per second, and
    whether the device map, the checked map and the points equal it.  The restatement is brute force (every cost a double loop
    over its window), so on 1920 x 1080 it runs on a band of 64 computed rows and the device rows of that band are compared.
A variant without LDS was not built, so there is nothing to compare against; counters were not collected.  No GPU, no numbers: the
script fails without a device."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import points_matching_amd as pm  # noqa: E402
from points_matching_amd import api  # noqa: E402
import stereo_ref as S  # noqa: E402

ROUNDS = 5
UNIQ = 10
CASES = [(496, 330, 64), (640, 480, 64), (640, 480, 128), (1920, 1080, 128)]
BAND = 64                                                        # computed rows the restatement runs on at 1920 x 1080


def synthetic_pair(w, h, D):
    """A smoothed seeded texture; right(x - d(x, y)) = left(x) with d ramping from D / 8 to 3 D / 4 over the frame; +-3 noise."""
    rng = np.random.default_rng(w * 7 + h)
    t = rng.integers(0, 256, (h + 1, w + D + 1)).astype(np.int64)
    wide = (t[:-1, :-1] + t[:-1, 1:] + t[1:, :-1] + t[1:, 1:] + 2) >> 2
    left = wide[:, :w].astype(np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    d = (D // 8 + (xs * 5 // w + ys * 3 // h) * (D * 5 // 64)).astype(np.int64)          # piecewise constant: 8 x 4 planes
    right = np.take_along_axis(wide, np.clip(xs + d, 0, w + D - 1), axis=1)                # right(x) = wide(x + d): left(x + d)
    right = np.clip(right + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)
    return left, right


def timed(ctx, name, fn, reps):
    ctx.timing_enable(True)
    ctx.timing_reset()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    ms, launches = ctx.timing_get(name)
    ctx.timing_enable(False)
    assert launches == reps, (name, launches)
    return ms


def measure(ctx, dev, w, h, D, r, a):
    left, right = synthetic_pair(w, h, D)
    K, base = (0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0), 0.12
    rng = np.random.default_rng(D + r)
    pts = np.stack([rng.uniform(0, w, 2000), rng.uniform(0, h, 2000)], 1).astype(np.float32)
    d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    d_lm, d_rm = torch.zeros((h, w), dtype=torch.int16, device=dev), torch.zeros((h, w), dtype=torch.int16, device=dev)
    d_keep = torch.zeros((h, w), dtype=torch.int16, device=dev)
    d_info = torch.zeros((3, 2), dtype=torch.int32, device=dev)
    d_pts = torch.from_numpy(pts).to(dev)
    d_xyz = torch.zeros((2000, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    pl, pr = api.stereo_params(D, r, 0, UNIQ), api.stereo_params(D, r, 0, UNIQ, api.PM_STEREO_FROM_RIGHT)
    calls = {
        "stereo_bm": ("stereo_bm", lambda: ctx.stereo_bm_dev(d_l.data_ptr(), d_r.data_ptr(), w, h, w, w, pl, d_lm.data_ptr(), w, d_info[0].data_ptr())),
        "stereo_bm_from_right": ("stereo_bm", lambda: ctx.stereo_bm_dev(d_l.data_ptr(), d_r.data_ptr(), w, h, w, w, pr, d_rm.data_ptr(), w,
                                                                        d_info[1].data_ptr())),
        "stereo_lr_check": ("stereo_lr_check", lambda: ctx.stereo_lr_check_dev(d_lm.data_ptr(), d_rm.data_ptr(), w, h, w, w, 16, d_info[2].data_ptr())),
        "stereo_points": ("stereo_points", lambda: ctx.stereo_points_dev(d_lm.data_ptr(), w, h, w, K, base, None, d_pts.data_ptr(), None, 2000,
                                                                         d_xyz.data_ptr())),
    }
    for _, fn in calls.values():
        for _ in range(a.warmup):
            fn()
    ctx.synchronize()
    per_round = {k: [] for k in calls}
    for _ in range(ROUNDS):                                      # alternate: every kernel sees every round
        for k, (name, fn) in calls.items():
            per_round[k].append(timed(ctx, name, fn, a.reps))
    x0, x1 = S.computed_columns(w, 0, D, r)
    costs = max(x1 - x0 + 1, 0) * max(h - 2 * r, 0) * D
    out = {}
    for k, (name, fn) in calls.items():
        ms = float(np.median(per_round[k]))
        out[k] = {"kernel": name, "mean_ms_median_of_rounds": round(ms, 5), "rounds_ms": [round(v, 5) for v in per_round[k]]}
        if name == "stereo_bm":
            out[k]["costs"] = costs
            out[k]["Gcosts_per_s"] = round(costs / (ms * 1e-3) / 1e9, 2)
    # what was timed, once more in order, against the restatement
    calls["stereo_bm"][1]()
    calls["stereo_bm_from_right"][1]()
    ctx.synchronize()
    d_keep.copy_(d_lm)
    calls["stereo_lr_check"][1]()
    calls["stereo_points"][1]()
    ctx.synchronize()
    lm, rm, checked, info = d_keep.cpu().numpy(), d_rm.cpu().numpy(), d_lm.cpu().numpy(), d_info.cpu().numpy()
    y0, y1 = (0, h) if w * h <= 640 * 480 else (h // 2 - BAND // 2 - r, h // 2 + BAND // 2 + r)
    t0 = time.perf_counter()
    ref_l, _ = S.bm(left[y0:y1], right[y0:y1], 0, D, r, UNIQ)
    cpu_s = time.perf_counter() - t0
    ref_r, _ = S.bm(left[y0:y1], right[y0:y1], 0, D, r, UNIQ, S.FROM_RIGHT)
    ref_c, _ = S.lr_check(ref_l, ref_r, 16)
    rows = slice(y0 + r, y1 - r) if (y0, y1) != (0, h) else slice(0, h)
    band = slice(r, y1 - y0 - r) if (y0, y1) != (0, h) else slice(0, h)
    cpu_costs = max(x1 - x0 + 1, 0) * (y1 - y0 - 2 * r) * D
    equal = {"left_map": bool((lm[rows] == ref_l[band]).all()), "right_map": bool((rm[rows] == ref_r[band]).all()),
             "checked_map": bool((checked[rows] == ref_c[band]).all())}
    if (y0, y1) == (0, h):
        equal["counts"] = bool(info[:, 1].tolist() == [int((ref_l != S.INVALID).sum()), int((ref_r != S.INVALID).sum()), int((ref_c != S.INVALID).sum())])
        equal["points"] = bool(S.same_floats(d_xyz.cpu().numpy(), S.points(ref_c, K, base, None, pts)))
    else:
        equal["points"] = bool(S.same_floats(d_xyz.cpu().numpy(), S.points(checked, K, base, None, pts)))          # on the device's own map
    return {"width": w, "height": h, "num_disp": D, "radius": r, "uniqueness": UNIQ, "valid_left": int(info[0, 1]), "valid_after_check": int(info[2, 1]),
            "kernels": out,
            "restatement_one_cpu_thread": {"rows": [y0, y1], "seconds_left_map": round(cpu_s, 3), "costs": cpu_costs,
                                           "Gcosts_per_s": round(cpu_costs / cpu_s / 1e9, 4)},
            "device_equals_restatement": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_stereo: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    S.lib()
    res = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "rounds": ROUNDS,
           "timer": "pm_ctx_timing_get: one event pair per launch, mean over reps; the median of the rounds is reported",
           "cases": [], "not_measured": ["a variant without LDS (not built)", "hardware counters", "pm_stereo_bm (the host form: staging dominates)"]}
    for w, h, D in CASES:
        for r in (4, 10):
            res["cases"].append(measure(ctx, dev, w, h, D, r, a))
            print(json.dumps(res["cases"][-1]), flush=True)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
