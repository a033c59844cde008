"""The device feature front end against the host extractor on one MI355X (docs/SPEC.md S53-S57).

    python tools/prof_features.py [--reps 50] [--warmup 5] [--descriptor grad|bits|both] [--out profiles/features_timing.json]

Inputs: the two 496 x 330 fixtures tests/golden/img0{1,2}_half.pgm, max_kp 4000 (what pm_cli uses).  In one session:
  * pm_detect_describe_dev, device time by event pairs on the context's stream around each call (median, quartiles);
  * pm_detect_describe (host pointers, blocking: allocation, upload, run, download), wall clock around each call;
  * the per-kernel means and launch counts of one call from pm_ctx_timing_get, in a pass of their own (the event pairs
    around every launch serialise the stream, so their sum is an upper bound of the call's time);
  * the baseline: `pm_cli --features host --extract-only` on an image given as both --img1 and --img2, wall clock of the
    process over two extractions, best of three, halved (process start and PGM read included: a few ms);
  * keypoint counts, and whether the device's rows equal the blocking form's.
--descriptor bits measures the binary form (pm_detect_describe_bits[_dev], S58-S60) the same way; both measures the two forms
one after the other in one session and nests the figures of an image under "grad" and "bits" (default output file:
profiles/features_bits_timing.json).
No GPU, no numbers: the script fails without a device."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import points_matching_amd as pm  # noqa: E402
from points_matching_amd import build  # noqa: E402

KERNELS = {"grad": ("feat_blur", "feat_decimate", "feat_extrema", "feat_rank", "feat_describe", "feat_compact", "feat_gather"),
           "bits": ("feat_blur", "feat_decimate", "feat_extrema", "feat_rank", "feat_describe_bits", "feat_compact", "feat_gather_bits")}
MAX_KP = 4000


def read_pgm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P5"
        line = f.readline()
        while line.startswith(b"#"):
            line = f.readline()
        w, h = (int(v) for v in line.split())
        assert int(f.readline()) == 255
        return np.frombuffer(f.read(w * h), np.uint8).reshape(h, w).copy()


def stats(v):
    v = np.sort(np.asarray(v))
    return {"median": round(float(np.median(v)), 4), "p25": round(float(np.percentile(v, 25)), 4),
            "p75": round(float(np.percentile(v, 75)), 4), "min": round(float(v[0]), 4), "max": round(float(v[-1]), 4)}


def measure(ctx, st, dev, a, kind, img, d_img, path, host_bin):
    h, w = img.shape
    d_kp = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
    bits = kind == "bits"
    d_u8 = torch.zeros((MAX_KP, 32 if bits else 128), dtype=torch.uint8, device=dev)
    d_f = torch.zeros((MAX_KP, 128), dtype=torch.float32, device=dev)
    d_meta = torch.zeros((MAX_KP, 4), dtype=torch.float32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def call():
        if bits:
            ctx.detect_describe_bits_dev(d_img.data_ptr(), w, h, w, MAX_KP, d_kp.data_ptr(), d_u8.data_ptr(), d_meta.data_ptr(), d_n.data_ptr())
            return
        ctx.detect_describe_dev(d_img.data_ptr(), w, h, w, MAX_KP, d_kp.data_ptr(), d_u8.data_ptr(), d_f.data_ptr(),
                                d_meta.data_ptr(), d_n.data_ptr())

    dev_ms, wall_ms = [], []
    for rep in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        torch.cuda.synchronize()
        if rep >= a.warmup:
            dev_ms.append(e0.elapsed_time(e1))
    n = int(d_n.item())
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        if bits:
            kp_b, u8_b, meta_b = ctx.detect_describe_bits(img, MAX_KP)
        else:
            kp_b, u8_b, f_b, meta_b = ctx.detect_describe(img, MAX_KP)
        t1 = time.perf_counter()
        if rep >= a.warmup:
            wall_ms.append((t1 - t0) * 1e3)
    same = kp_b.shape[0] == n and (kp_b == d_kp[:n].cpu().numpy()).all() and (u8_b == d_u8[:n].cpu().numpy()).all()
    # per-kernel means, a pass of its own
    ctx.timing_enable(True)
    ctx.timing_reset()
    for _ in range(a.reps):
        call()
    kern = {}
    for k in KERNELS[kind]:
        ms, launches = ctx.timing_get(k)
        kern[k] = {"mean_ms": round(ms, 5), "launches_per_call": launches / a.reps, "ms_per_call": round(ms * launches / a.reps, 5)}
    ctx.timing_enable(False)
    # the host extractor: one process, the image twice
    host_wall = []
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(3):
            t0 = time.perf_counter()
            out = subprocess.run([host_bin, "--features", "host", "--img1", path, "--img2", path, "--extract-only", "--quiet", "--descriptor", kind,
                                  "--max-kp", str(MAX_KP), "--save-features", os.path.join(tmp, "f")], capture_output=True, text=True)
            t1 = time.perf_counter()
            assert out.returncode == 0, out.stderr
            host_wall.append((t1 - t0) * 1e3 / 2)
    host_ms = min(host_wall)
    dev_stat, wall_stat = stats(dev_ms), stats(wall_ms)
    return {
        "width": w, "height": h, "keypoints": n, "blocking_form_equals_dev_form": bool(same),
        "dev_form_event_ms": dev_stat, "blocking_form_wall_ms": wall_stat, "host_extractor_ms_per_image": round(host_ms, 3),
        "speedup_dev_form_over_host": round(host_ms / dev_stat["median"], 1),
        "speedup_blocking_form_over_host": round(host_ms / wall_stat["median"], 1),
        "kernels": kern, "kernel_sum_ms_per_call": round(sum(v["ms_per_call"] for v in kern.values()), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--descriptor", choices=("grad", "bits", "both"), default="grad")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "features_timing.json" if a.descriptor == "grad" else "features_bits_timing.json")
    kinds = ("grad", "bits") if a.descriptor == "both" else (a.descriptor,)
    if not torch.cuda.is_available():
        raise SystemExit("prof_features: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    paths = [os.path.join(ROOT, "tests", "golden", "img0%d_half.pgm" % i) for i in (1, 2)]
    res = {"max_kp": MAX_KP, "reps": a.reps, "warmup": a.warmup, "unit": "ms", "descriptor": a.descriptor, "images": {}}
    host_bin = build.build_host()
    for path in paths:
        name = os.path.basename(path)
        img = read_pgm(path)
        h, w = img.shape
        d_img = torch.from_numpy(img).to(dev)
        for kind in kinds:
            fig = measure(ctx, st, dev, a, kind, img, d_img, path, host_bin)
            if a.descriptor == "both":
                res["images"].setdefault(name, {})[kind] = fig
            else:
                res["images"][name] = fig
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
