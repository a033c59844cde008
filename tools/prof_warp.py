"""Image warp by H or A and the point transform on one MI355X (docs/SPEC.md S75-S78): a first measurement, no threshold.

    python tools/prof_warp.py [--reps 50] [--warmup 5] [--out profiles/warp_timing.json] [--alignment profiles/warp_alignment.txt]

In one session, one process:
  * warp_bilinear by the context's timers (one event pair per launch, pm_ctx_timing_get) on the 496 x 330 fixture
    tests/golden/img01_half.pgm and on a synthetic 3840 x 2160 frame, each warped onto an output of its own size by a mild
    homography, by an affine on the division-free branch (last row exactly (0, 0, 1)), and by the homography under
    PM_WARP_INVERT; valid mask and info written.  Next to each time: (source bytes + output bytes) / time, the HBM figures of
    the hardware notes to read it against (a frame of this size lives in the caches, so this is a rate, not a share of HBM),
    whether the device bytes equal the plain-C restatement tests/warp_ref.c, and that restatement's time on one CPU thread;
  * warp_points at 240 and 100 000 points;
  * the alignment chain (two pyramids, corners, track + gather, similarity RANSAC, refit, warp with PM_WARP_AFFINE) on the
    fixture and its copy turned by 3 degrees: both mean absolute grey differences over the valid pixels, written to the
    alignment file, and the chain's time by an event pair.
Larger frames, strong perspective and an LDS-staged source window are NOT measured here.  No GPU, no numbers: the script fails
without a device."""
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
import describe_ref  # noqa: E402
import lk_ref  # noqa: E402
import warp_ref  # noqa: E402

HBM_PEAK_TBS, HBM_ACHIEVABLE_TBS = 8.0, 6.3          # the hardware notes' figures for the MI355X


def stats(v):
    v = np.sort(np.asarray(v))
    return {"median": round(float(np.median(v)), 4), "p25": round(float(np.percentile(v, 25)), 4),
            "p75": round(float(np.percentile(v, 75)), 4), "min": round(float(v[0]), 4), "max": round(float(v[-1]), 4)}


def synthetic_frame(w=3840, h=2160):
    """Smooth structure plus seeded noise: nothing a cache could compress away, nothing that depends on a file."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 127.5 + 90.0 * np.sin(xs / 37.0) * np.cos(ys / 29.0)
    noise = np.random.default_rng(2160).integers(-20, 21, (h, w))
    return np.clip(np.rint(base + noise), 0, 255).astype(np.uint8)


def models(w, h):
    """A mild homography scaled to the frame, and an affine with the exact last row (0, 0, 1)."""
    s = w / 496.0
    H = np.array([[1.02, 0.015, -6.0 * s], [-0.02, 0.99, 4.0 * s], [4e-5 / s, -3e-5 / s, 1.0]])
    A = np.array([[0.998, -0.05, 9.0 * s], [0.05, 0.998, -7.0 * s]])
    return (("homography", H, 0), ("affine_unit_last_row", A, api.PM_WARP_AFFINE), ("homography_inverted", H, api.PM_WARP_INVERT))


def kernel_ms(ctx, name, fn, a):
    """Mean time of the named kernel over a.reps calls after a.warmup, by the context's own event pairs."""
    for _ in range(a.warmup):
        fn()
    ctx.synchronize()
    ctx.timing_enable(True)
    ctx.timing_reset()
    for _ in range(a.reps):
        fn()
    ctx.synchronize()
    ms, launches = ctx.timing_get(name)
    ctx.timing_enable(False)
    assert launches == a.reps, (name, launches)
    return ms


def measure_frame(ctx, dev, img, a):
    h, w = img.shape
    d_src = torch.from_numpy(img).to(dev)
    d_dst = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    d_val = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    d_info = torch.zeros(2, dtype=torch.int32, device=dev)
    out = {}
    for name, M, flags in models(w, h):
        d_M = torch.from_numpy(np.ascontiguousarray(M, np.float64).reshape(-1)).to(dev)
        prm = api.warp_params(flags, 0)
        torch.cuda.synchronize()

        def call():
            ctx.warp_dev(d_src.data_ptr(), w, h, w, d_M.data_ptr(), prm, d_dst.data_ptr(), w, h, w, d_val.data_ptr(), d_info.data_ptr())

        ms = kernel_ms(ctx, "warp_bilinear", call, a)
        t0 = time.perf_counter()
        want = warp_ref.warp(img, M, flags, 0)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        info = d_info.cpu().numpy()
        same = (d_dst.cpu().numpy() == want[0]).all() and (d_val.cpu().numpy() == want[1]).all() and (int(info[0]), int(info[1])) == want[2:]
        moved = 2 * w * h                                          # source bytes + output bytes (the mask's bytes are not counted)
        out[name] = {"warp_bilinear_mean_ms": round(ms, 5), "source_plus_output_bytes": moved,
                     "source_plus_output_GBs": round(moved / (ms * 1e-3) / 1e9, 1), "valid_pixels": int(info[1]),
                     "device_equals_restatement": bool(same), "c_restatement_one_thread_ms": round(cpu_ms, 2)}
    return {"width": w, "height": h, "models": out}


def measure_points(ctx, dev, n, a):
    rng = np.random.default_rng(n)
    pts = np.stack([rng.uniform(0, 3840, n), rng.uniform(0, 2160, n)], 1).astype(np.float32)
    H = models(3840, 2160)[0][1]
    d_pts = torch.from_numpy(pts).to(dev)
    d_out = torch.zeros_like(d_pts)
    d_M = torch.from_numpy(H.reshape(-1).copy()).to(dev)
    torch.cuda.synchronize()
    ms = kernel_ms(ctx, "warp_points", lambda: ctx.transform_points_dev(d_M.data_ptr(), 0, d_pts.data_ptr(), None, n, d_out.data_ptr()), a)
    same = warp_ref.same_floats(d_out.cpu().numpy(), warp_ref.points(H, pts))
    return {"points": n, "warp_points_mean_ms": round(ms, 5), "device_equals_restatement": bool(same)}


def alignment(ctx, dev, st, a, path):
    img1 = lk_ref.fixture()[0]
    img2 = describe_ref.rotate_frame(img1, 3)
    h, w = img1.shape
    cap = 512
    d_img1, d_img2 = torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev)
    d_kp = torch.zeros((cap, 2), dtype=torch.float32, device=dev)
    d_xy1, d_xy2 = torch.zeros_like(d_kp), torch.zeros_like(d_kp)
    d_n, d_cnt, d_ninl = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(3))
    d_key = torch.zeros(1, dtype=torch.int64, device=dev)
    d_A, d_Ar = torch.zeros(6, dtype=torch.float64, device=dev), torch.zeros(6, dtype=torch.float64, device=dev)
    d_mask = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_dst, d_val = torch.zeros((h, w), dtype=torch.uint8, device=dev), torch.zeros((h, w), dtype=torch.uint8, device=dev)
    d_info = torch.zeros(2, dtype=torch.int32, device=dev)
    p1, p2 = ctx.pyramid(w, h, 3), ctx.pyramid(w, h, 3)
    view = api.PointsView(d_xy1.data_ptr(), d_xy2.data_ptr(), d_cnt.data_ptr(), 1, cap, 0, 1, 0)
    cprm, lk, wprm = api.corner_params(), api.lk_params(10, 3, fb_thresh=0.5), api.warp_params(api.PM_WARP_AFFINE, 0)
    torch.cuda.synchronize()

    def chain():
        p1.build_dev(d_img1.data_ptr())
        p2.build_dev(d_img2.data_ptr())
        ctx.corners_dev(p1, cprm, cap, d_kp.data_ptr(), d_n.data_ptr())
        ctx.track_lk_gather_dev(p1, p2, d_kp.data_ptr(), d_n.data_ptr(), cap, lk, d_xy1.data_ptr(), d_xy2.data_ptr(), d_cnt.data_ptr())
        ctx.ransac_affine_run_dev(view, 0, 500, 2.0, 0x5EED, d_key.data_ptr(), d_A.data_ptr(), d_mask.data_ptr(), cap, d_ninl.data_ptr(),
                                  model=api.PM_AFFINE_PARTIAL)
        ctx.affine_refine_dev(view, d_mask.data_ptr(), d_A.data_ptr(), d_Ar.data_ptr(), None, model=api.PM_AFFINE_PARTIAL)
        ctx.warp_dev(d_img2.data_ptr(), w, h, w, d_Ar.data_ptr(), wprm, d_dst.data_ptr(), w, h, w, d_val.data_ptr(), d_info.data_ptr())

    ms = []
    for rep in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        chain()
        e1.record(st)
        torch.cuda.synchronize()
        if rep >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    dst, v = d_dst.cpu().numpy(), d_val.cpu().numpy() == 1
    A = d_Ar.cpu().numpy()
    want = warp_ref.warp(img2, A, api.PM_WARP_AFFINE, 0)
    same = (dst == want[0]).all() and ((d_val.cpu().numpy()) == want[1]).all()
    before = float(np.abs(img2.astype(np.int32) - img1.astype(np.int32))[v].mean())
    after = float(np.abs(dst.astype(np.int32) - img1.astype(np.int32))[v].mean())
    res = {"frame": "tests/golden/img01_half.pgm against its copy turned by 3 degrees", "model": "similarity, refitted",
           "tracked": int(d_cnt.item()), "inliers": int(d_ninl.item()), "valid_pixels": int(v.sum()),
           "mean_abs_diff_before": round(before, 4), "mean_abs_diff_after": round(after, 4), "device_equals_restatement": bool(same),
           "chain_event_ms": stats(ms), "A": [float(x) for x in A]}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("alignment chain: pyramids, corners, track + gather, similarity RANSAC (500 hypotheses, 2 px), refit, warp\n")
        f.write("frame 1: tests/golden/img01_half.pgm (%d x %d); frame 2: frame 1 turned by 3 degrees about its centre\n" % (w, h))
        f.write("tracked %d, inliers %d, valid pixels %d of %d\n" % (res["tracked"], res["inliers"], res["valid_pixels"], w * h))
        f.write("mean absolute grey difference to frame 1 over the valid pixels: unwarped %.4f, warped %.4f\n" % (before, after))
        f.write("chain time by an event pair, ms: %s\n" % json.dumps(res["chain_event_ms"]))
    ctx.synchronize()
    p1.close()
    p2.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_timing.json"))
    ap.add_argument("--alignment", default=os.path.join(ROOT, "profiles", "warp_alignment.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_warp: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    warp_ref.lib()                                      # built before anything is timed against it
    res = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "timer": "pm_ctx_timing_get: one event pair per launch, mean over reps",
           "hbm_TBs_to_read_against": {"peak": HBM_PEAK_TBS, "achievable": HBM_ACHIEVABLE_TBS},
           "frames": {"fixture_496x330": measure_frame(ctx, dev, lk_ref.fixture()[0], a),
                      "synthetic_3840x2160": measure_frame(ctx, dev, synthetic_frame(), a)},
           "points": [measure_points(ctx, dev, 240, a), measure_points(ctx, dev, 100000, a)],
           "alignment_chain": alignment(ctx, dev, st, a, a.alignment),
           "not_measured": ["frames larger than 3840 x 2160", "strong perspective", "an LDS-staged source window"]}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    ctx.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
