"""The image database on one MI355X (docs/SPEC.md S107-S112): a first measurement, no threshold.

    python tools/prof_bowdb.py [--queries 10] [--warmup 2] [--out profiles/bowdb_timing.json]

In one session and one process, by the context's timer (one event pair per launch, pm_ctx_timing_get), five alternating
rounds over all cases, the median of the rounds and the rounds themselves:
  * databases of 10 000 and 100 000 images of 1000 rows each (about 1000 entries at K = 65536, fewer distinct words at
    K = 4096), K = 4096 and 65536, idf weights; built with pm_bowdb_add_dev from histograms made on the device;
  * per query bow_query_vec, bow_score, bow_top, and the whole call between two events on the stream; the entry bytes per
    second of bow_score (6 bytes per entry) next to the 6.3 TB/s stream figure;
  * bow_add per call, over the last 200 images of each database;
  * the plain-C restatement tests/bowdb_ref.c on one CPU thread, per query, on the same database (taken over from the
    device's dump), and whether every score and the selection of the device equal the restatement's (asserted).
Counters were not collected, the host forms were not timed, and every image has the same length.  No GPU, no numbers: the
tool fails without a device."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ROUNDS = 5
ROWS = 1000
TOP = 10
CASES = [(10000, 4096), (10000, 65536), (100000, 4096), (100000, 65536)]
TIMERS = ("bow_query_vec", "bow_score", "bow_top")
STREAM_TBS = 6.3


def device_hists(torch, dev, n, K, seed):
    """n histograms of ROWS rows: 70 % of the rows from 1500 words of the image's own, 30 % uniform."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    base = torch.randint(0, K, (n, 1), generator=g, device=dev)
    own = (base + torch.randint(0, 1500, (n, ROWS), generator=g, device=dev) * 7) % K
    uni = torch.randint(0, K, (n, ROWS), generator=g, device=dev)
    words = torch.where(torch.rand((n, ROWS), generator=g, device=dev) < 0.7, own, uni)
    h = torch.zeros((n, K), dtype=torch.int32, device=dev)
    h.scatter_add_(1, words, torch.ones_like(words, dtype=torch.int32))
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bowdb_timing.json"))
    a = ap.parse_args()
    import torch
    import points_matching_amd as pm
    from points_matching_amd import api
    import bowdb_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("prof_bowdb: no GPU")
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(st)
    ctx = pm.Context(0)
    ctx.set_stream(st.cuda_stream)
    R.lib()
    cases = []
    for n, K in CASES:
        db = api.BowDb(ctx, K, n, n * ROWS)
        d_id = torch.zeros(1, dtype=torch.int32, device=dev)
        batch = max(1, min(n, (1 << 28) // (4 * K)))
        done = 0
        add_ms = None
        while done < n:
            b = min(batch, n - done)
            h = device_hists(torch, dev, b, K, seed=K + done)
            torch.cuda.synchronize()
            for i in range(b):
                if done + i == n - 200:                          # the last 200 adds are timed
                    ctx.synchronize()
                    ctx.timing_enable(True)
                    ctx.timing_reset()
                db.add_dev(h[i].data_ptr(), d_id.data_ptr())
            ctx.synchronize()
            done += b
        add_ms, launches = ctx.timing_get("bow_add")
        assert launches == 200, launches
        ctx.timing_enable(False)
        assert int(d_id.cpu().numpy()[0]) == n - 1
        db.idf_dev()
        d_q = device_hists(torch, dev, a.queries, K, seed=7 * K + n)
        d_ids = torch.zeros((a.queries, TOP), dtype=torch.int32, device=dev)
        d_sc = torch.zeros((a.queries, TOP), dtype=torch.float64, device=dev)
        d_cnt = torch.zeros(a.queries, dtype=torch.int32, device=dev)
        d_all = torch.zeros((a.queries, n), dtype=torch.float64, device=dev)

        def call(db=db, d_q=d_q, d_ids=d_ids, d_sc=d_sc, d_cnt=d_cnt, d_all=d_all):
            for j in range(a.queries):
                db.query_dev(d_q[j].data_ptr(), TOP, 0, 0, d_ids[j].data_ptr(), d_sc[j].data_ptr(), d_cnt.data_ptr() + 4 * j, d_all[j].data_ptr())
        cases.append(dict(images=n, K=K, db=db, call=call, keep=(d_q, d_ids, d_sc, d_cnt, d_all), bow_add_ms=add_ms, rounds=[]))
    ctx.synchronize()
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
            row = {"query_by_events": e0.elapsed_time(e1) / a.queries}
            for name in TIMERS:
                ms, launches = ctx.timing_get(name)
                assert launches == a.queries, (name, launches)      # one event pair per query (bow_top: around both launches)
                row[name] = ms
            c["rounds"].append(row)
            ctx.timing_enable(False)
    recs = []
    for c in cases:
        n, K, db = c["images"], c["K"], c["db"]
        d_q, d_ids, d_sc, d_cnt, d_all = c["keep"]
        rec = {"images": n, "K": K, "bow_add_ms_per_call_last_200": round(c["bow_add_ms"], 5)}
        dump = db.get()
        rec["entries"] = dump["n_entries"]
        rec["entries_per_image"] = round(dump["n_entries"] / n, 1)
        for name in TIMERS + ("query_by_events",):
            vals = [r[name] for r in c["rounds"]]
            rec[name + "_ms_median_of_rounds"] = round(float(np.median(vals)), 5)
            rec[name + "_rounds_ms"] = [round(v, 5) for v in vals]
        score_s = rec["bow_score_ms_median_of_rounds"] * 1e-3
        rec["bow_score_entry_TB_per_s"] = round(dump["n_entries"] * 6 / score_s / 1e12, 3)
        rec["bow_score_share_of_stream_figure"] = round(rec["bow_score_entry_TB_per_s"] / STREAM_TBS, 3)
        rec["bow_score_ns_per_image"] = round(score_s * 1e9 / n, 2)
        ref = R.RefDb(K, n, max(dump["n_entries"], 1))
        ref.load(dump)
        q = d_q.cpu().numpy().view(np.uint32)
        ids, sc, cnt, every = d_ids.cpu().numpy(), d_sc.cpu().numpy(), d_cnt.cpu().numpy(), d_all.cpu().numpy()
        t0 = time.perf_counter()
        want = [ref.query(q[j], TOP) for j in range(a.queries)]
        rec["restatement_one_cpu_thread_ms_per_query"] = round((time.perf_counter() - t0) * 1e3 / a.queries, 3)
        ok = all((ids[j] == w[0]).all() and (sc[j].view(np.uint64) == w[1].view(np.uint64)).all() and cnt[j] == w[2] and
                 (every[j].view(np.uint64) == w[3].view(np.uint64)).all() for j, w in enumerate(want))
        rec["device_equals_restatement"] = bool(ok)
        rec["candidates_of_query_0"] = int((every[0] > 0).sum())
        assert ok
        ref.close()
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    res = {"unit": "ms", "queries_per_round": a.queries, "warmup": a.warmup, "rounds": ROUNDS, "top": TOP,
           "timer": "pm_ctx_timing_get: one event pair per kernel and query (bow_top: around both launches above 32768 images); "
                    "query_by_events: two events around the queries of a round, per query; the median of the rounds is reported",
           "images": "1000 rows each, 70 % from 1500 words of the image's own, 30 % uniform; idf weights; queries made the same way",
           "reference_rate": "6.3 TB/s: the achievable HBM stream figure; an entry is 6 bytes (u32 word, u16 tf)",
           "restatement": "tests/bowdb_ref.c, -O2, one thread, the database taken over from the device's dump",
           "cases": recs,
           "not_measured": ["hardware counters", "the host forms (staging dominates)", "images of very uneven length",
                            "pm_bowdb_idf_dev and bow_norms", "K above 65536"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    ctx.synchronize()
    for c in cases:
        c["db"].close()
    ctx.close()


if __name__ == "__main__":
    main()
