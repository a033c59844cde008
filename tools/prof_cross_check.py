"""What one-call cross-check matching costs (docs/SPEC.md S42), timed with HIP events on the context's stream after
warm-up, at C3 (8192 x 8192 SIFT-128) and C2 (2048 x 2048), float rows with PM_KNN_HINT_U8.  Per size, alternating in one
process, `reps` runs each (median, quartiles, min, max in microseconds):
  (a) pm_bf_match_cross_l2_f32_dev with cross_flags = PM_CROSS_RATIO_FWD;
  (b) the same work through the older entry points: pm_bf_knn_l2_f32_dev(k = 2) + pm_bf_knn_l2_f32_dev(k = 1, arguments
      swapped) + pm_filter_ratio_gather_dev, same buffers (forward-ratio filter only: no reverse lookup);
  (c) pm_bf_knn_l2_ratio_dev alone: the forward-only filter the feature is an alternative to;
then the filter kernels by themselves from pm_ctx_timing_get, one launch per sample: "filter_cross_gather" inside (a) and
"filter_gather" inside (b), and the two filter entry points called alone on the records (a) left behind.
One JSON line per size; run it in a process of its own, under a time limit:
    timeout -k 10 300 python3 tools/prof_cross_check.py [reps n1 n2 ...]          (default: 30 8192 2048)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import points_matching_amd as pm  # noqa: E402
from points_matching_amd import api, synth  # noqa: E402

WARMUP = 5
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
sizes = [int(a) for a in sys.argv[2:]] or [8192, 2048]
assert reps >= 20, "median of at least 20 runs"
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
ctx = pm.Context(0)
ctx.set_stream(stream.cuda_stream)
HINT, RATIO, DIM = api.PM_KNN_HINT_U8, 0.8, 128


def stats(us):
    q = statistics.quantiles(us, n=4)
    return {"median": round(statistics.median(us), 2), "p25": round(q[0], 2), "p75": round(q[2], 2),
            "min": round(min(us), 2), "max": round(max(us), 2)}


def kernel_us(pairs):
    """Per-launch times of the named kernels, the (name, fn) pairs alternating; one launch of the kernel per fn()."""
    ctx.timing_enable(True)
    us = {name: [] for name, _ in pairs}
    for i in range(WARMUP + reps):
        for name, fn in pairs:
            ctx.timing_reset()
            fn()
            ms, launches = ctx.timing_get(name.split(":")[0])
            assert launches == 1, (name, launches)
            if i >= WARMUP:
                us[name].append(ms * 1e3)
    ctx.timing_enable(False)
    return {name: stats(v) for name, v in us.items()}


for n in sizes:
    w = synth.pair_workload(nq=n, nt=n, dim=DIM)
    with torch.cuda.stream(stream):
        d_q, d_t, d_kp1, d_kp2 = (torch.from_numpy(w[k]).to(dev) for k in ("q", "t", "kp1", "kp2"))
        d_fwd = torch.zeros((n, 8), dtype=torch.int32, device=dev)
        d_rev = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        d_good = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        d_xy1 = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        d_xy2 = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    stream.synchronize()
    q, t, kp1, kp2 = d_q.data_ptr(), d_t.data_ptr(), d_kp1.data_ptr(), d_kp2.data_ptr()
    fwd, rev, good, xy1, xy2, cnt = (x.data_ptr() for x in (d_fwd, d_rev, d_good, d_xy1, d_xy2, d_n))

    def run_a():
        ctx.bf_match_cross_l2_dev(q, n, t, n, DIM, HINT, api.PM_CROSS_RATIO_FWD, RATIO, kp1, kp2, fwd, rev, good, xy1, xy2, cnt)

    def run_b():
        ctx.bf_knn_l2_dev(q, n, t, n, DIM, 2, fwd, HINT)
        ctx.bf_knn_l2_dev(t, n, q, n, DIM, 1, rev, HINT)
        ctx.filter_ratio_gather_dev(fwd, n, 2, RATIO, kp1, kp2, good, xy1, xy2, cnt)

    def run_c():
        ctx.bf_knn_l2_ratio_dev(q, n, t, n, DIM, HINT, RATIO, kp1, kp2, fwd, good, xy1, xy2, cnt)

    forms = (("a_one_call_cross", run_a), ("b_three_calls", run_b), ("c_forward_ratio_only", run_c))
    survivors = {}
    for name, fn in forms:
        for _ in range(WARMUP):
            fn()
        ctx.synchronize()
        survivors[name] = int(d_n.item())
    times = {name: [] for name, _ in forms}
    for _ in range(reps):                                  # (a), (b), (c) alternate: drift hits all three alike
        for name, fn in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    out = {"n": n, "dim": DIM, "reps": reps, "warmup": WARMUP, "unit": "us", "survivors": survivors}
    for name, _ in forms:
        out[name] = stats(times[name])
    out["a_minus_b_median"] = round(out["a_one_call_cross"]["median"] - out["b_three_calls"]["median"], 2)
    out["a_over_c_median"] = round(out["a_one_call_cross"]["median"] / out["c_forward_ratio_only"]["median"], 3)

    def filter_cross():
        ctx.filter_cross_gather_dev(fwd, n, 2, rev, n, 1, api.PM_CROSS_RATIO_FWD, RATIO, kp1, kp2, good, xy1, xy2, cnt)

    def filter_ratio():
        ctx.filter_ratio_gather_dev(fwd, n, 2, RATIO, kp1, kp2, good, xy1, xy2, cnt)

    out["kernel_in_call"] = kernel_us((("filter_cross_gather:in (a)", run_a), ("filter_gather:in (b)", run_b)))
    run_a()                                                # fwd / rev hold the two k-NN lists
    out["kernel_alone"] = kernel_us((("filter_cross_gather:alone", filter_cross), ("filter_gather:alone", filter_ratio)))
    print(json.dumps(out), flush=True)
ctx.close()
