"""Sparse Lucas-Kanade tracking on one MI355X (docs/SPEC.md S61-S66): a first measurement, no threshold.

    python tools/prof_track.py [--reps 50] [--warmup 5] [--out profiles/track_timing.json]

Input: the 496 x 330 fixture tests/golden/img01_half.pgm as the previous frame, frame R of the tests (1 degree rotation plus a
shift of (7.25, -5.5), made by tests/lk_ref.py) as the next frame, and the keypoints pm_detect_describe_dev finds on the
previous frame with max_kp 4000.  Parameters: win_radius 10, max_level 3, 30 iterations, eps 0.01, forward-backward
threshold 0.5 px (so both directions run).  In one session:
  * the _dev chain of a video step: pm_pyramid_build_dev of ONE frame (the next one; the previous frame's pyramid exists),
    then pm_track_lk_gather_dev (track + compaction).  Device time by an event pair on the context's stream around the
    chain, and wall clock around the chain including the final synchronisation (median, quartiles, min, max);
  * the per-kernel means and launch counts of lk_pyr_down, lk_track, lk_compact from pm_ctx_timing_get, in a pass of
    their own (the event pairs around every launch serialise the stream: their sum is an upper bound of the chain);
  * the plain-C restatement tests/lk_ref.c on the same input, one thread: pyramid of the next frame + tracking;
  * what the descriptor route costs for the same pair: pm_detect_describe_dev on the next frame and
    pm_bf_knn_l2_u8_ratio_dev between the two frames' rows, each by event pairs.
No GPU, no numbers: the script fails without a device."""
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
import lk_ref  # noqa: E402

KERNELS = ("lk_pyr_down", "lk_track", "lk_compact")
MAX_KP = 4000


def stats(v):
    v = np.sort(np.asarray(v))
    return {"median": round(float(np.median(v)), 4), "p25": round(float(np.percentile(v, 25)), 4),
            "p75": round(float(np.percentile(v, 75)), 4), "min": round(float(v[0]), 4), "max": round(float(v[-1]), 4)}


def event_ms(st, fn, a):
    out = []
    for rep in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize()
        if rep >= a.warmup:
            out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_track: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    img1 = lk_ref.fixture()[0]
    img2 = lk_ref.frame_r(img1)
    h, w = img1.shape
    prm = api.lk_params(10, 3, 30, 0.01, 1e-4, 0.5)
    d_img = [torch.from_numpy(im).to(dev) for im in (img1, img2)]
    d_kp = [torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev) for _ in range(2)]
    d_u8 = [torch.zeros((MAX_KP, 128), dtype=torch.uint8, device=dev) for _ in range(2)]
    d_n = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2)]
    d_xy1 = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
    d_xy2 = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def detect(i):
        ctx.detect_describe_dev(d_img[i].data_ptr(), w, h, w, MAX_KP, d_kp[i].data_ptr(), d_u8[i].data_ptr(), 0, 0, d_n[i].data_ptr())

    detect(0)
    detect(1)
    ctx.synchronize()
    n1, n2 = int(d_n[0].item()), int(d_n[1].item())
    p1, p2 = ctx.pyramid(w, h, 3), ctx.pyramid(w, h, 3)
    p1.build_dev(d_img[0].data_ptr())
    ctx.synchronize()

    def chain():
        p2.build_dev(d_img[1].data_ptr())
        ctx.track_lk_gather_dev(p1, p2, d_kp[0].data_ptr(), d_n[0].data_ptr(), MAX_KP, prm, d_xy1.data_ptr(), d_xy2.data_ptr(), d_cnt.data_ptr())

    chain_ms = event_ms(st, chain, a)
    tracked = int(d_cnt.item())
    wall = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        chain()
        ctx.synchronize()
        t1 = time.perf_counter()
        if rep >= a.warmup:
            wall.append((t1 - t0) * 1e3)
    ctx.timing_enable(True)
    ctx.timing_reset()
    for _ in range(a.reps):
        chain()
    ctx.synchronize()
    kern = {}
    for k in KERNELS:
        ms, launches = ctx.timing_get(k)
        kern[k] = {"mean_ms": round(ms, 5), "launches_per_call": launches / a.reps, "ms_per_call": round(ms * launches / a.reps, 5)}
    ctx.timing_enable(False)

    # the plain-C restatement, one thread, same frames, points and parameters
    kp = d_kp[0][:n1].cpu().numpy()
    ra = lk_ref.Pyramid(img1, 3)
    ref_pyr, ref_track = [], []
    for _ in range(7):
        t0 = time.perf_counter()
        rb = lk_ref.Pyramid(img2, 3)
        t1 = time.perf_counter()
        out, status, _, _ = lk_ref.track(ra, rb, kp, lk_ref.params(10, 3, 30, 0.01, 1e-4, 0.5))
        t2 = time.perf_counter()
        ref_pyr.append((t1 - t0) * 1e3)
        ref_track.append((t2 - t1) * 1e3)
    same = int((status == 1).sum()) == tracked and \
        (d_xy2[:tracked].cpu().numpy().view(np.uint32) == out[status == 1].view(np.uint32)).all()

    # the descriptor route for the same pair: detection of the next frame + the matcher
    feat_ms = event_ms(st, lambda: detect(1), a)
    d_knn = torch.zeros((MAX_KP, 8), dtype=torch.int32, device=dev)
    d_good = torch.zeros((MAX_KP, 4), dtype=torch.int32, device=dev)
    d_ng = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    match_ms = event_ms(st, lambda: ctx.bf_knn_l2_u8_ratio_dev(d_u8[0].data_ptr(), n1, d_u8[1].data_ptr(), n2, 128, 0.8, d_kp[0].data_ptr(),
                                                               d_kp[1].data_ptr(), d_knn.data_ptr(), d_good.data_ptr(), d_xy1.data_ptr(),
                                                               d_xy2.data_ptr(), d_ng.data_ptr()), a)
    res = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "width": w, "height": h, "max_kp": MAX_KP,
           "params": {"win_radius": 10, "max_level": 3, "max_iters": 30, "eps": 0.01, "min_eig": 1e-4, "fb_thresh": 0.5},
           "points": n1, "tracked": tracked, "device_equals_restatement": bool(same),
           "chain_build_track_gather_event_ms": stats(chain_ms), "chain_build_track_gather_wall_ms": stats(wall),
           "kernels": kern, "kernel_sum_ms_per_call": round(sum(v["ms_per_call"] for v in kern.values()), 5),
           "c_restatement_one_thread_ms": {"pyramid": stats(ref_pyr), "track": stats(ref_track)},
           "descriptor_route_same_pair": {"keypoints_next_frame": n2, "good_matches": int(d_ng.item()),
                                          "detect_describe_dev_next_frame_event_ms": stats(feat_ms),
                                          "bf_knn_l2_u8_ratio_dev_event_ms": stats(match_ms)}}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    ctx.synchronize()
    p1.close()
    p2.close()
    ctx.close()


if __name__ == "__main__":
    main()
