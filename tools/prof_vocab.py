"""Visual vocabularies on one MI355X (docs/SPEC.md S102-S106): a first measurement, no threshold.

    python tools/prof_vocab.py [--iters 3] [--warmup 1] [--out profiles/vocab_timing.json]

In one session and one process, by the context's timer (one event pair per launch, pm_ctx_timing_get), five alternating
rounds over all cases, the median of the rounds and the rounds themselves:
  * per training iteration the matcher call (the sum of its kernels' timers), vocab_update and vocab_finish, for 1 000 000
    rows of 128 bytes at K = 64, 4096 and 65536, 1 000 000 rows of 256 bits at K = 4096, and 3000 rows of 128 bytes at K = 64
    (the launch-latency end); the update's share of the three; the atomic bytes the update issued in the measured iteration
    (counted on the host from the labels: one flush per run of equal labels within a lane group's stretch of a wave's sorted
    rows) and the rate they reached, next to the bytes an ungrouped form would have issued;
  * the whole call between two events on the stream, as a check on the sum (it also holds the timer's own events, the stride
    start and the gaps between launches);
  * vocab_hist at 1000 and 100 000 rows (K = 4096);
  * whether the device outputs equal the plain-C restatement tests/vocab_ref.c on the small case.
Counters were not collected and the host forms were not timed.  No GPU, no numbers: the tool fails without a device."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ROUNDS = 5
MATCHER = ("knn_l2_prep", "knn_l2_mfma_f16", "knn_l2_mfma", "knn_l2_mfma_u8", "knn_l2_mfma_u8_s2", "knn_l2_mfma_u8_s4",
           "knn_l2_mfma_f16s", "knn_l2_refine", "knn_l2_exact", "knn_hamming_expand", "knn_hamming_mfma_i8", "knn_hamming_refine", "knn_hamming512_expand", "knn_hamming512_mfma_i8",
           "knn_hamming512_refine", "knn_hamming", "knn_hamming_merge", "pad_rows_u8")
TRAIN = [("l2", 128, 1000000, 64), ("l2", 128, 1000000, 4096), ("l2", 128, 1000000, 65536), ("bits", 32, 1000000, 4096),
         ("l2", 128, 3000, 64)]
HIST = [1000, 100000]


def device_rows(torch, dev, kind, n, nbytes, seed):
    """Clustered rows made on the device: 256 prototypes plus noise (u8) or 10 % flipped bits."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lab = torch.randint(0, 256, (n,), generator=g, device=dev)
    proto = torch.randint(0, 256, (256, nbytes), generator=g, device=dev, dtype=torch.int32)
    if kind == "l2":
        noise = (torch.randn((n, nbytes), generator=g, device=dev) * 12.0).round().to(torch.int32)
        return (proto[lab] + noise).clamp_(0, 255).to(torch.uint8).contiguous()
    flip = torch.zeros((n, nbytes), dtype=torch.int32, device=dev)
    for b in range(8):
        flip |= (torch.rand((n, nbytes), generator=g, device=dev) < 0.1).to(torch.int32) << b
    return (proto[lab] ^ flip).to(torch.uint8).contiguous()


def atomic_bytes(labels, kind, nbytes):
    """Bytes of atomic adds one vocab_update issues for these labels: per wave of 64 rows the labels are sorted and each lane
    group walks its stretch; a run of equal labels within a stretch is flushed once (the accumulators and one count)."""
    n = labels.shape[0]
    pad = (-n) % 64
    lab = np.concatenate([labels.astype(np.int64), np.full(pad, 1 << 40, np.int64) + np.arange(pad)]).reshape(-1, 64)
    lab.sort(axis=1)
    groups = 64 // (nbytes // 4) if kind == "l2" else 1
    stretch = -(-64 // groups)
    runs = 0
    for g in range(groups):
        s = lab[:, g * stretch:(g + 1) * stretch]
        real = s < (1 << 40)
        first = np.ones_like(real)
        first[:, 1:] = s[:, 1:] != s[:, :-1]
        runs += int((first & real).sum())
    per_flush = (nbytes if kind == "l2" else nbytes * 8) * 4 + 4
    return runs * per_flush, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocab_timing.json"))
    a = ap.parse_args()
    import torch
    import points_matching_amd as pm
    from points_matching_amd import api
    import vocab_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("prof_vocab: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    R.lib()
    cases = []
    for kind, nbytes, n, K in TRAIN:
        k = api.PM_VOCAB_L2_U8 if kind == "l2" else api.PM_VOCAB_BITS
        d_rows = device_rows(torch, dev, kind, n, nbytes, seed=n + K)
        voc = api.Vocab(ctx, k, nbytes, K, n)
        d_lab = torch.zeros(n, dtype=torch.int32, device=dev)
        d_info = torch.zeros(a.iters * 24, dtype=torch.uint8, device=dev)

        def call(voc=voc, d_rows=d_rows, n=n, d_lab=d_lab, d_info=d_info):
            voc.init_stride_dev(d_rows.data_ptr(), n)
            voc.train_dev(d_rows.data_ptr(), n, a.iters, d_lab.data_ptr(), d_info.data_ptr())
        cases.append(dict(what="train", kind=kind, kcode=k, bytes=nbytes, rows=n, K=K, call=call, voc=voc, keep=(d_rows, d_lab, d_info),
                          launches=a.iters, timers=("vocab_update", "vocab_finish"), rounds=[]))
    hist_rows = device_rows(torch, dev, "l2", max(HIST), 128, seed=5)
    hist_voc = api.Vocab(ctx, api.PM_VOCAB_L2_U8, 128, 4096, max(HIST))
    hist_voc.init_stride_dev(hist_rows.data_ptr(), max(HIST))
    d_hist = torch.zeros(4096, dtype=torch.int32, device=dev)
    d_words = torch.zeros(max(HIST), dtype=torch.int32, device=dev)
    for n in HIST:
        def hcall(n=n):
            hist_voc.assign_dev(hist_rows.data_ptr(), n, 0, d_words.data_ptr(), 0, d_hist.data_ptr())
        cases.append(dict(what="encode", kind="l2", bytes=128, rows=n, K=4096, call=hcall, launches=1, timers=("vocab_hist",), rounds=[]))
    torch.cuda.synchronize()
    for c in cases:
        for _ in range(a.warmup):
            c["call"]()
    ctx.synchronize()
    for _ in range(ROUNDS):                                      # alternate: every case sees every round
        for c in cases:
            ctx.timing_enable(True)
            ctx.timing_reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            c["call"]()
            e1.record(st)
            ctx.synchronize()
            row = {"call_by_events": e0.elapsed_time(e1)}        # the whole call (a training call: stride start + iterations)
            for name in c["timers"]:
                ms, launches = ctx.timing_get(name)
                assert launches == c["launches"], (name, launches)
                row[name] = ms
            total = 0.0
            for name in MATCHER:                                 # mean per launch x launches, per matcher call
                ms, launches = ctx.timing_get(name)
                total += ms * launches
            row["matcher"] = total / c["launches"]
            c["rounds"].append(row)
            ctx.timing_enable(False)
    recs = []
    for c in cases:
        rec = {k: c[k] for k in ("what", "kind", "bytes", "rows", "K")}
        med = {}
        for name in c["timers"] + ("matcher", "call_by_events"):
            vals = [r[name] for r in c["rounds"]]
            med[name] = float(np.median(vals))
            rec[name + "_ms_median_of_rounds"] = round(med[name], 5)
            rec[name + "_rounds_ms"] = [round(v, 5) for v in vals]
        if c["what"] == "train":
            d_rows, d_lab, d_info = c["keep"]
            it = med["matcher"] + med["vocab_update"] + med["vocab_finish"]
            rec["iteration_ms"] = round(it, 5)
            rec["update_share_of_iteration"] = round(med["vocab_update"] / it, 4)
            ab, runs = atomic_bytes(d_lab.cpu().numpy(), c["kind"], c["bytes"])
            per_row = (c["bytes"] if c["kind"] == "l2" else c["bytes"] * 8) * 4 + 4
            rec["atomic_flushes_last_iteration"] = runs
            rec["atomic_bytes_last_iteration"] = ab
            rec["atomic_bytes_ungrouped"] = c["rows"] * per_row
            rec["atomic_GB_per_s_at_mean_update_time"] = round(ab / (med["vocab_update"] * 1e-3) / 1e9, 2)
            rec["records"] = [[int(v) for v in r] for r in d_info.cpu().numpy().view(api.VOCAB_ITER_DTYPE).tolist()]
            if c["rows"] <= 3000:
                rows = d_rows.cpu().numpy()
                want = R.train(c["kcode"], R.init_stride(rows, c["K"]), rows, a.iters)
                rec["device_equals_restatement"] = bool(
                    (c["voc"].get() == want[0]).all() and (d_lab.cpu().numpy() == want[1]).all() and
                    d_info.cpu().numpy().view(api.VOCAB_ITER_DTYPE).tobytes() == want[2].tobytes())
                assert rec["device_equals_restatement"]
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    res = {"unit": "ms", "iterations_per_call": a.iters, "warmup": a.warmup, "rounds": ROUNDS,
           "timer": "pm_ctx_timing_get: one event pair per launch, mean per launch over the iterations of a call; matcher = the sum "
                    "of its kernels' timers per call of it; the median of the rounds is reported",
           "rows": "256 prototypes plus noise of sigma 12 (u8 rows) or 10 % flipped bits (bit rows), made on the device; stride start",
           "reference_rate": "1.3 TB/s of added bytes: the guide's figure for float atomics; the integer rate above is the first measured here",
           "cases": recs,
           "not_measured": ["hardware counters", "the host forms (staging dominates)", "vocab_init", "K above 65536", "rows of other widths"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    ctx.synchronize()
    for c in cases:
        if "voc" in c:
            c["voc"].close()
    hist_voc.close()
    ctx.close()


if __name__ == "__main__":
    main()
