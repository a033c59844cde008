"""Oriented 256-bit descriptors of given points on one MI355X (docs/SPEC.md S71-S74): a first measurement, no threshold.

    python tools/prof_describe.py [--reps 50] [--warmup 5] [--out profiles/describe_points_timing.json]

Input: the 496 x 330 fixture tests/golden/img01_half.pgm and its 344 minimum-eigenvalue corners (block_radius 10, min_eig 1e-4,
quality 0.01, min_dist 8, up to 500 corners), described at level 0.  In one session, one process:
  * pm_describe_points_dev and pm_describe_points_gather_dev on the corners: device time by an event pair on the context's
    stream around the call (median, quartiles, min, max), and wall clock around the aligned call including the final
    synchronisation;
  * the per-kernel means of desc_points and desc_compact from pm_ctx_timing_get, in a pass of their own (one event pair per
    launch);
  * the whole chain per image: pyramid (level 0 only) + pm_corners_dev + pm_describe_points_gather_dev, by an event pair;
  * the figure to read it against: pm_detect_describe_bits_dev per image (DoG keypoints + their 256-bit descriptors);
  * whether the device rows equal the plain-C restatement tests/describe_ref.c.
Scaling with the point count is NOT measured here.  No GPU, no numbers: the script fails without a device."""
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

KERNELS = ("desc_points", "desc_compact")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "describe_points_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prof_describe: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    img, corners = describe_ref.fixture_corners()
    h, w = img.shape
    cprm = api.corner_params(10, 1e-4, 0.01, 8.0)
    dprm = api.describe_params(0)
    d_img = torch.from_numpy(img).to(dev)
    d_kp = torch.zeros((CORNERS, 2), dtype=torch.float32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    d_desc = torch.zeros((CORNERS, 32), dtype=torch.uint8, device=dev)
    d_valid = torch.zeros(CORNERS, dtype=torch.uint8, device=dev)
    d_bin = torch.zeros(CORNERS, dtype=torch.uint8, device=dev)
    d_xy = torch.zeros((CORNERS, 2), dtype=torch.float32, device=dev)
    d_gdesc = torch.zeros((CORNERS, 32), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    d_dkp = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
    d_dbits = torch.zeros((MAX_KP, 32), dtype=torch.uint8, device=dev)
    d_dn = torch.zeros(1, dtype=torch.int32, device=dev)
    pyr = ctx.pyramid(w, h, 0)
    torch.cuda.synchronize()
    pyr.build_dev(d_img.data_ptr())
    ctx.corners_dev(pyr, cprm, CORNERS, d_kp.data_ptr(), d_n.data_ptr())
    ctx.synchronize()
    found = int(d_n.item())

    def aligned():
        ctx.describe_points_dev(pyr, d_kp.data_ptr(), d_n.data_ptr(), CORNERS, dprm, d_desc.data_ptr(), d_valid.data_ptr(), d_bin.data_ptr())

    def gather():
        ctx.describe_points_gather_dev(pyr, d_kp.data_ptr(), d_n.data_ptr(), CORNERS, dprm, d_xy.data_ptr(), d_gdesc.data_ptr(), d_cnt.data_ptr())

    def chain():
        pyr.build_dev(d_img.data_ptr())
        ctx.corners_dev(pyr, cprm, CORNERS, d_kp.data_ptr(), d_n.data_ptr())
        gather()

    aligned_ms = event_ms(st, aligned, a)
    gather_ms = event_ms(st, gather, a)
    wall = []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aligned()
        ctx.synchronize()
        t1 = time.perf_counter()
        if rep >= a.warmup:
            wall.append((t1 - t0) * 1e3)
    ctx.timing_enable(True)
    ctx.timing_reset()
    for _ in range(a.reps):
        gather()
    ctx.synchronize()
    kern = {}
    for k in KERNELS:
        ms, launches = ctx.timing_get(k)
        kern[k] = {"mean_ms": round(ms, 5), "launches_per_call": launches / a.reps, "ms_per_call": round(ms * launches / a.reps, 5)}
    ctx.timing_enable(False)
    chain_ms = event_ms(st, chain, a)
    bits_ms = event_ms(st, lambda: ctx.detect_describe_bits_dev(d_img.data_ptr(), w, h, w, MAX_KP, d_dkp.data_ptr(), d_dbits.data_ptr(), 0,
                                                                 d_dn.data_ptr()), a)
    want = describe_ref.describe(img, 0, corners)
    valid = int(d_cnt.item())
    same = found == corners.shape[0] and (d_desc[:found].cpu().numpy() == want[0]).all() and \
        (d_valid[:found].cpu().numpy() == want[1]).all() and (d_bin[:found].cpu().numpy() == want[2]).all() and \
        valid == int(want[1].sum()) and (d_gdesc[:valid].cpu().numpy() == want[0][want[1] == 1]).all()
    res = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "width": w, "height": h, "level": 0,
           "corner_params": {"block_radius": 10, "min_eig": 1e-4, "quality": 0.01, "min_dist": 8.0, "max_corners": CORNERS},
           "points": found, "valid_rows": valid, "device_equals_restatement": bool(same),
           "describe_points_dev_event_ms": stats(aligned_ms), "describe_points_dev_wall_ms": stats(wall),
           "describe_points_gather_dev_event_ms": stats(gather_ms),
           "kernels": kern, "kernel_sum_ms_per_call": round(sum(v["ms_per_call"] for v in kern.values()), 5),
           "pyramid_corners_describe_per_image_event_ms": stats(chain_ms),
           "to_read_against": {"detect_describe_bits_dev_per_image_event_ms": stats(bits_ms), "dog_keypoints": int(d_dn.item())},
           "scaling_with_point_count": "not measured"}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    ctx.synchronize()
    pyr.close()
    ctx.close()


if __name__ == "__main__":
    main()
