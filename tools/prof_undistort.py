"""Lens undistortion on one MI355X (docs/SPEC.md S79-S83): a first measurement, no threshold.

    python tools/prof_undistort.py [--reps 50] [--warmup 5] [--out profiles/undistort_timing.json]

In one session, one process, on the 496 x 330 fixture tests/golden/img01_half.pgm and on a synthetic 3840 x 2160 frame, each
undistorted onto an output of its own size under a moderate lens (k1 = -0.28, k2 = 0.07, p1 = 1e-3, p2 = -5e-4, k3 = 0) and a
camera whose focal length is 0.8 of the frame's width:
  * undistort_bilinear (the fused form), undistort_map and remap_q5 (the two-launch form), and warp_bilinear by a near-identity
    homography, all by the context's timers (one event pair per launch, pm_ctx_timing_get), valid mask and info written;
    the four are taken in rounds, one after the other, so that they share whatever else the machine is doing;
  * the fused form again with a rectifying rotation of a few degrees (the R branch), and with a zero lens (the branch without the
    polynomial);
  * next to each time the bytes the call must move (source + output; the map adds 8 bytes per pixel written or read) over the
    time, and whether the device bytes equal the plain-C restatement tests/undistort_ref.c;
  * undistort_points at 240 and 100 000 points (20 rounds).
An LDS-staged source window, colour images and frames larger than 3840 x 2160 are NOT measured here.  No GPU, no numbers: the
script fails without a device."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import points_matching_amd as pm  # noqa: E402
from points_matching_amd import api  # noqa: E402
import lk_ref  # noqa: E402
import undistort_ref as U  # noqa: E402

LENS = U.MODERATE
ROUNDS = 5


def synthetic_frame(w=3840, h=2160):
    """Smooth structure plus seeded noise: nothing a cache could compress away, nothing that depends on a file."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 127.5 + 90.0 * np.sin(xs / 37.0) * np.cos(ys / 29.0)
    noise = np.random.default_rng(2160).integers(-20, 21, (h, w))
    return np.clip(np.rint(base + noise), 0, 255).astype(np.uint8)


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


def measure_frame(ctx, dev, img, a):
    h, w = img.shape
    K = (0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0)
    s = w / 496.0
    H = np.array([[1.02, 0.015, -6.0 * s], [-0.02, 0.99, 4.0 * s], [4e-5 / s, -3e-5 / s, 1.0]])
    d_src = torch.from_numpy(img).to(dev)
    d_dst = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    d_val = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    d_info = torch.zeros(2, dtype=torch.int32, device=dev)
    d_map = torch.zeros((h, w, 2), dtype=torch.int32, device=dev)
    d_M = torch.from_numpy(H.reshape(-1).copy()).to(dev)
    prm = api.warp_params(0, 0)
    tail = (d_dst.data_ptr(), w, h, w, d_val.data_ptr(), d_info.data_ptr())
    torch.cuda.synchronize()
    px = w * h
    calls = {
        "undistort_bilinear": ("undistort_bilinear", lambda: ctx.undistort_dev(d_src.data_ptr(), w, h, w, K, LENS, None, None, prm, *tail), 2 * px),
        "undistort_map": ("undistort_map", lambda: ctx.undistort_map_dev(K, LENS, None, None, w, h, d_map.data_ptr()), 8 * px),
        "remap_q5": ("remap_q5", lambda: ctx.remap_dev(d_src.data_ptr(), w, h, w, d_map.data_ptr(), prm, *tail), 10 * px),
        "warp_bilinear_near_identity": ("warp_bilinear", lambda: ctx.warp_dev(d_src.data_ptr(), w, h, w, d_M.data_ptr(), prm, *tail), 2 * px),
        "undistort_bilinear_with_R": ("undistort_bilinear", lambda: ctx.undistort_dev(d_src.data_ptr(), w, h, w, K, LENS, U.ROT, None, prm, *tail), 2 * px),
        "undistort_bilinear_zero_lens": ("undistort_bilinear", lambda: ctx.undistort_dev(d_src.data_ptr(), w, h, w, K, None, None, None, prm, *tail), 2 * px),
    }
    for _, fn, _ in calls.values():
        for _ in range(a.warmup):
            fn()
    ctx.synchronize()
    per_round = {k: [] for k in calls}
    for _ in range(ROUNDS):                                      # alternate: every kernel sees every round
        for k, (name, fn, _) in calls.items():
            per_round[k].append(timed(ctx, name, fn, a.reps))
    out = {}
    for k, (name, fn, moved) in calls.items():
        ms = float(np.median(per_round[k]))
        out[k] = {"kernel": name, "mean_ms_median_of_rounds": round(ms, 5), "rounds_ms": [round(v, 5) for v in per_round[k]],
                  "bytes_moved": moved, "GBs": round(moved / (ms * 1e-3) / 1e9, 1)}
    # correctness of what was timed: fused and map + remap against the restatement
    want = U.undistort(img, K, LENS)
    calls["undistort_bilinear"][1]()
    ctx.synchronize()
    fused = (d_dst.cpu().numpy() == want[0]).all() and (d_val.cpu().numpy() == want[1]).all() and int(d_info.cpu().numpy()[1]) == want[2]
    d_dst.zero_()
    torch.cuda.synchronize()
    calls["undistort_map"][1]()
    calls["remap_q5"][1]()
    ctx.synchronize()
    two = (d_dst.cpu().numpy() == want[0]).all() and (d_val.cpu().numpy() == want[1]).all() and int(d_info.cpu().numpy()[1]) == want[2]
    f, m, r = (out[k]["mean_ms_median_of_rounds"] for k in ("undistort_bilinear", "undistort_map", "remap_q5"))
    return {"width": w, "height": h, "camera": list(K), "lens": list(LENS), "valid_pixels": want[2], "kernels": out,
            "fused_ms": f, "map_plus_remap_ms": round(m + r, 5), "remap_alone_ms": r,
            "faster_per_frame_with_a_fixed_map": "remap_q5" if r < f else "undistort_bilinear",
            "fused_equals_restatement": bool(fused), "map_plus_remap_equals_restatement": bool(two)}


def measure_points(ctx, dev, n, a):
    rng = np.random.default_rng(n)
    w, h = 3840, 2160
    K = (0.8 * w, 0.8 * w, (w - 1) / 2.0, (h - 1) / 2.0)
    pts = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1).astype(np.float32)
    d_pts = torch.from_numpy(pts).to(dev)
    d_out = torch.zeros_like(d_pts)
    torch.cuda.synchronize()

    def call():
        ctx.undistort_points_dev(K, LENS, None, None, U.ITERS, U.TOL_PX, d_pts.data_ptr(), None, n, d_out.data_ptr())

    for _ in range(a.warmup):
        call()
    ctx.synchronize()
    ms = [timed(ctx, "undistort_points", call, a.reps) for _ in range(ROUNDS)]
    want = U.undistort_points(K, LENS, None, None, pts)
    got = d_out.cpu().numpy()
    return {"points": n, "iters": U.ITERS, "tol_px": U.TOL_PX, "undistort_points_mean_ms_median_of_rounds": round(float(np.median(ms)), 5),
            "rounds_ms": [round(v, 5) for v in ms], "rejected": int(np.isnan(got).any(axis=1).sum()),
            "device_equals_restatement": bool(U.same_floats(got, want))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_undistort: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    U.lib()
    res = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "rounds": ROUNDS,
           "timer": "pm_ctx_timing_get: one event pair per launch, mean over reps; the median of the rounds is reported",
           "frames": {"fixture_496x330": measure_frame(ctx, dev, lk_ref.fixture()[0], a),
                      "synthetic_3840x2160": measure_frame(ctx, dev, synthetic_frame(), a)},
           "points": [measure_points(ctx, dev, 240, a), measure_points(ctx, dev, 100000, a)],
           "not_measured": ["an LDS-staged source window", "frames larger than 3840 x 2160"]}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
