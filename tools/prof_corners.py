"""Minimum-eigenvalue corners on one MI355X (docs/SPEC.md S67-S70): a first measurement, no threshold.

    python tools/prof_corners.py [--reps 50] [--warmup 5] [--out profiles/corners_timing.json]

Input: the 496 x 330 fixture tests/golden/img01_half.pgm as the previous frame and frame R of the tests (made by
tests/lk_ref.py) as the next frame.  Corner parameters: block_radius 10, min_eig 1e-4, quality 0.01, min_dist 8, 500 corners.
Tracking parameters: win_radius 10, max_level 3, 30 iterations, eps 0.01, forward-backward threshold 0.5 px.  In one session:
  * pm_corners_dev on the previous frame's pyramid: device time by an event pair on the context's stream around the call, and
    wall clock around the call including the final synchronisation (median, quartiles, min, max);
  * the per-kernel means of corner_extrema, corner_rank, corner_select from pm_ctx_timing_get, in a pass of their own (one
    event pair per launch; the launches are dependent, so the sum is close to the call);
  * pm_corners_replenish_dev on the next frame's pyramid after a track of the corners found (fewer than 500 here) into it (the survivors are restored from a
    device copy before every repetition; that copy is inside the event pair and is timed alone as well);
  * the figures to read these against: pm_detect_describe_dev on the previous frame, and pyramid of the next frame + track +
    gather of the corners;
  * the plain-C restatement tests/corner_ref.c on the same input, one thread, and whether the device rows equal it.
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
import corner_ref  # noqa: E402
import lk_ref  # noqa: E402

KERNELS = ("corner_extrema", "corner_rank", "corner_select")
CORNERS = 500
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corners_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_corners: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    img1 = lk_ref.fixture()[0]
    img2 = lk_ref.frame_r(img1)
    h, w = img1.shape
    cprm = api.corner_params(10, 1e-4, 0.01, 8.0)
    lk = api.lk_params(10, 3, 30, 0.01, 1e-4, 0.5)
    d_img = [torch.from_numpy(im).to(dev) for im in (img1, img2)]
    d_xy = torch.zeros((CORNERS, 2), dtype=torch.float32, device=dev)
    d_sc = torch.zeros(CORNERS, dtype=torch.float32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    d_xy1 = torch.zeros((CORNERS, 2), dtype=torch.float32, device=dev)
    d_xy2 = torch.zeros((CORNERS, 2), dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    d_new = torch.zeros(1, dtype=torch.int32, device=dev)
    d_kp = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
    d_u8 = torch.zeros((MAX_KP, 128), dtype=torch.uint8, device=dev)
    d_nkp = torch.zeros(1, dtype=torch.int32, device=dev)
    p1, p2 = ctx.pyramid(w, h, 3), ctx.pyramid(w, h, 3)
    torch.cuda.synchronize()
    p1.build_dev(d_img[0].data_ptr())
    p2.build_dev(d_img[1].data_ptr())
    ctx.synchronize()

    def corners():
        ctx.corners_dev(p1, cprm, CORNERS, d_xy.data_ptr(), d_n.data_ptr(), d_sc.data_ptr())

    corners_ms = event_ms(st, corners, a)
    found = int(d_n.item())
    wall = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        corners()
        ctx.synchronize()
        t1 = time.perf_counter()
        if rep >= a.warmup:
            wall.append((t1 - t0) * 1e3)
    ctx.timing_enable(True)
    ctx.timing_reset()
    for _ in range(a.reps):
        corners()
    ctx.synchronize()
    kern = {}
    for k in KERNELS:
        ms, launches = ctx.timing_get(k)
        kern[k] = {"mean_ms": round(ms, 5), "launches_per_call": launches / a.reps, "ms_per_call": round(ms * launches / a.reps, 5)}
    ctx.timing_enable(False)

    # the restatement, one thread, and parity of the rows
    ref_ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        want = corner_ref.detect(img1, 10, 1e-4, 0.01, 8.0, None, CORNERS)
        ref_ms.append((time.perf_counter() - t0) * 1e3)
    same = want[0].shape[0] == found and (d_xy[:found].cpu().numpy().view(np.uint32) == want[0].view(np.uint32)).all() and \
        (d_sc[:found].cpu().numpy().view(np.uint32) == want[1].view(np.uint32)).all()

    # track the corners into the next frame; replenish the survivors on its pyramid
    def chain():
        p2.build_dev(d_img[1].data_ptr())
        ctx.track_lk_gather_dev(p1, p2, d_xy.data_ptr(), d_n.data_ptr(), CORNERS, lk, d_xy1.data_ptr(), d_xy2.data_ptr(), d_cnt.data_ptr())

    chain_ms = event_ms(st, chain, a)
    tracked = int(d_cnt.item())
    surv_xy, surv_cnt = d_xy2.clone(), d_cnt.clone()
    torch.cuda.synchronize()

    def restore():
        d_xy2.copy_(surv_xy)
        d_cnt.copy_(surv_cnt)

    def replenish():
        restore()
        ctx.corners_replenish_dev(p2, cprm, d_xy2.data_ptr(), d_cnt.data_ptr(), CORNERS, CORNERS, None, d_new.data_ptr())

    restore_ms = event_ms(st, restore, a)
    rep_ms = event_ms(st, replenish, a)
    added, total = int(d_new.item()), int(d_cnt.item())
    want_r = corner_ref.detect(img2, 10, 1e-4, 0.01, 8.0, surv_xy[:tracked].cpu().numpy(), CORNERS - tracked)
    same_r = want_r[0].shape[0] == added and (d_xy2[tracked:total].cpu().numpy().view(np.uint32) == want_r[0].view(np.uint32)).all()

    # what the DoG + descriptor front end costs on the same frame
    feat_ms = event_ms(st, lambda: ctx.detect_describe_dev(d_img[0].data_ptr(), w, h, w, MAX_KP, d_kp.data_ptr(), d_u8.data_ptr(), 0, 0,
                                                           d_nkp.data_ptr()), a)
    res = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "width": w, "height": h,
           "corner_params": {"block_radius": 10, "min_eig": 1e-4, "quality": 0.01, "min_dist": 8.0, "max_corners": CORNERS},
           "candidates": int(want[2]), "corners": found, "device_equals_restatement": bool(same),
           "corners_dev_event_ms": stats(corners_ms), "corners_dev_wall_ms": stats(wall),
           "kernels": kern, "kernel_sum_ms_per_call": round(sum(v["ms_per_call"] for v in kern.values()), 5),
           "c_restatement_one_thread_ms": stats(ref_ms),
           "replenish": {"tracked": tracked, "added": added, "total": total, "candidates_next_frame": int(want_r[2]),
                         "device_equals_restatement": bool(same_r), "restore_plus_replenish_dev_event_ms": stats(rep_ms),
                         "restore_alone_event_ms": stats(restore_ms)},
           "to_read_against": {"detect_describe_dev_event_ms": stats(feat_ms), "dog_keypoints": int(d_nkp.item()),
                               "pyramid_track_gather_event_ms": stats(chain_ms)}}
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
