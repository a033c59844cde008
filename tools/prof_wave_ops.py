"""The one-workgroup helper kernels that csrc/wave_ops.hpp's selection and rank helpers build (lk_compact, desc_compact,
feat_compact, feat_rank, corner_rank), timed against another build of the library on one MI355X.

    python tools/prof_wave_ops.py --parent-lib PATH/libpm_hip.so [--reps 100] [--warmup 10] [--out profiles/wave_ops_timing.json]

Three series in fresh processes, alternating the builds through PM_LIB_PATH: parent, head (the library in the tree), parent.
Each series times the call that launches the kernel, with the shapes of tools/prof_track.py, prof_describe.py,
prof_features.py and prof_corners.py (the 496 x 330 fixture, max_kp 4000, 500 corners), by an event pair on the context's
stream around the call (median and quartiles over --reps calls after --warmup), and in a pass of its own the kernel's mean
from pm_ctx_timing_get.  "within_parent_spread": the head's median does not exceed the slower parent series, i.e. it exceeds
neither parent series by more than the two differ.  No GPU, no numbers: the script fails without a device."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"track_lk_gather_dev": ("lk_compact",), "describe_points_gather_dev": ("desc_compact",),
         "detect_describe_dev": ("feat_rank", "feat_compact"), "corners_dev": ("corner_rank",)}
MAX_KP = 4000
CORNERS = 500


def series(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import points_matching_amd as pm
    from points_matching_amd import api
    import lk_ref
    if not torch.cuda.is_available():
        raise SystemExit("prof_wave_ops: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    img1 = lk_ref.fixture()[0]
    img2 = lk_ref.frame_r(img1)
    h, w = img1.shape
    d_img = [torch.from_numpy(im).to(dev) for im in (img1, img2)]
    d_kp = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
    d_u8 = torch.zeros((MAX_KP, 128), dtype=torch.uint8, device=dev)
    d_nkp = torch.zeros(1, dtype=torch.int32, device=dev)
    d_xy1 = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
    d_xy2 = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    d_cxy = torch.zeros((CORNERS, 2), dtype=torch.float32, device=dev)
    d_cn = torch.zeros(1, dtype=torch.int32, device=dev)
    d_gxy = torch.zeros((CORNERS, 2), dtype=torch.float32, device=dev)
    d_gdesc = torch.zeros((CORNERS, 32), dtype=torch.uint8, device=dev)
    d_gcnt = torch.zeros(1, dtype=torch.int32, device=dev)
    lk = api.lk_params(10, 3, 30, 0.01, 1e-4, 0.5)
    cprm = api.corner_params(10, 1e-4, 0.01, 8.0)
    dprm = api.describe_params(0)
    p1, p2, p0 = ctx.pyramid(w, h, 3), ctx.pyramid(w, h, 3), ctx.pyramid(w, h, 0)
    torch.cuda.synchronize()
    p1.build_dev(d_img[0].data_ptr())
    p2.build_dev(d_img[1].data_ptr())
    p0.build_dev(d_img[0].data_ptr())
    calls = {
        "detect_describe_dev": lambda: ctx.detect_describe_dev(d_img[0].data_ptr(), w, h, w, MAX_KP, d_kp.data_ptr(), d_u8.data_ptr(), 0, 0,
                                                               d_nkp.data_ptr()),
        "track_lk_gather_dev": lambda: ctx.track_lk_gather_dev(p1, p2, d_kp.data_ptr(), d_nkp.data_ptr(), MAX_KP, lk, d_xy1.data_ptr(),
                                                               d_xy2.data_ptr(), d_cnt.data_ptr()),
        "corners_dev": lambda: ctx.corners_dev(p0, cprm, CORNERS, d_cxy.data_ptr(), d_cn.data_ptr()),
        "describe_points_gather_dev": lambda: ctx.describe_points_gather_dev(p0, d_cxy.data_ptr(), d_cn.data_ptr(), CORNERS, dprm, d_gxy.data_ptr(),
                                                                             d_gdesc.data_ptr(), d_gcnt.data_ptr()),
    }
    res = {}
    for name, fn in calls.items():                      # in this order: the later calls read what the earlier ones found
        ms = []
        for rep in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        v = np.sort(np.asarray(ms))
        res[name] = {"median": round(float(np.median(v)), 5), "p25": round(float(np.percentile(v, 25)), 5),
                     "p75": round(float(np.percentile(v, 75)), 5), "min": round(float(v[0]), 5)}
        ctx.timing_enable(True)
        ctx.timing_reset()
        for _ in range(a.reps):
            fn()
        ctx.synchronize()
        res[name]["kernel_mean_ms"] = {k: round(ctx.timing_get(k)[0], 5) for k in CALLS[name]}
        ctx.timing_enable(False)
    res["rows"] = {"keypoints": int(d_nkp.item()), "tracked": int(d_cnt.item()), "corners": int(d_cn.item()), "described": int(d_gcnt.item())}
    ctx.synchronize()
    for p in (p0, p1, p2):
        p.close()
    ctx.close()
    print("SERIES " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_ops_timing.json"))
    ap.add_argument("--series", action="store_true", help="(internal) run one series with the library of PM_LIB_PATH")
    a = ap.parse_args()
    if a.series:
        return series(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("prof_wave_ops: --parent-lib must name the parent build of libpm_hip.so")
    out = {"unit": "ms", "reps": a.reps, "warmup": a.warmup, "order": ["parent_1", "head", "parent_2"], "series": {}}
    for tag in out["order"]:
        env = dict(os.environ)
        env.pop("PM_LIB_PATH", None)
        if tag != "head":
            env["PM_LIB_PATH"] = os.path.abspath(a.parent_lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--series", "--reps", str(a.reps), "--warmup", str(a.warmup)],
                           env=env, capture_output=True, text=True, timeout=240)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("SERIES ")]
        if r.returncode != 0 or not line:
            raise SystemExit("prof_wave_ops: series %s failed (%d)\n%s\n%s" % (tag, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
        out["series"][tag] = json.loads(line[0][7:])
        print(tag, json.dumps(out["series"][tag]), flush=True)
    out["calls"] = {}
    for name, kernels in CALLS.items():
        p1, hd, p2 = (out["series"][t][name]["median"] for t in out["order"])
        out["calls"][name] = {"kernels": list(kernels), "parent_1_median": p1, "head_median": hd, "parent_2_median": p2,
                              "parent_spread": round(abs(p1 - p2), 5), "head_minus_faster_parent": round(hd - min(p1, p2), 5),
                              "within_parent_spread": bool(hd <= max(p1, p2))}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
