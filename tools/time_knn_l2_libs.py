"""Time the L2 matcher of two builds of the library against each other, in one sitting.

    python tools/time_knn_l2_libs.py <parent libpm_hip.so> <head libpm_hip.so> <out.json>

Fresh child processes, each bound to one library through PM_LIB_PATH, alternate parent, head, parent, head.  A child runs
every workload below and reports, per workload, samples of the library's own timers knn_l2_prep and knn_l2_refine and of
the call (stream time between two events), each sample the mean of CALLS calls.  Per timer the record holds the median of
each run, the pooled median of either side, the spread (the gap between the two parent runs) and whether the head's median
stays within parent + spread.  A child that fails ends the run: nothing more is started."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, SAMPLES = 10, 30
#            name                       nq    nt    dim  kind    flags fusion ratio-form
WORKLOADS = [("c3_sift_hint_u8",        8192, 8192, 128, "sift", 8,    0,     False),
             ("c3_sift_auto",           8192, 8192, 128, "sift", 0,    0,     False),
             ("c3_surf_auto",           8192, 8192, 128, "surf", 0,    0,     False),
             ("c3_surf_unit_norm",      8192, 8192, 128, "surf", 16,   0,     False),
             ("ratio_512_hint_u8",      512,  512,  128, "sift", 8,    0,     True),      # the fused u8 tail (default there)
             ("c3_ratio_integer_fused", 8192, 8192, 128, "sift", 4,    2,     True),      # the other fused tail
             # not asked for by the acceptance list: the one instantiation whose register count rose (knn_l2_prep16u<256, true>)
             ("extra_surf256_unit_norm", 8192, 8192, 256, "surf", 16,  0,     False),
             # ... and the one that grew most in instruction lines (knn_l2_prep16g<256, false>: general floats, dim % 4 != 0)
             ("extra_surf130_auto",     8192, 8192, 130, "surf", 0,    0,     False)]
TIMERS = ("knn_l2_prep", "knn_l2_refine", "call")


def child():
    sys.path.insert(0, ROOT)
    import torch
    import points_matching_amd as pm
    from points_matching_amd import synth
    from points_matching_amd.api import PM_OPT_FILTER_FUSION
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(s)
    ctx = pm.Context(0)
    ctx.set_stream(s.cuda_stream)
    out = {}
    for name, nq, nt, dim, kind, flags, fusion, ratio in WORKLOADS:
        w = synth.pair_workload(nq, nt, dim, seed=0xC3, kind=kind)
        d_q, d_t = torch.from_numpy(w["q"]).to(dev), torch.from_numpy(w["t"]).to(dev)
        d_kp1, d_kp2 = torch.from_numpy(w["kp1"]).to(dev), torch.from_numpy(w["kp2"]).to(dev)
        d_knn = torch.empty((nq, 2, 4), dtype=torch.int32, device=dev)
        d_good = torch.empty((nq, 4), dtype=torch.int32, device=dev)
        d_xy1, d_xy2 = torch.empty((nq, 2), device=dev), torch.empty((nq, 2), device=dev)
        d_n = torch.zeros((1,), dtype=torch.int32, device=dev)
        ctx.set_option(PM_OPT_FILTER_FUSION, fusion)

        def call():
            if ratio:
                ctx.bf_knn_l2_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, dim, flags, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(),
                                        d_knn.data_ptr(), d_good.data_ptr(), d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr())
            else:
                ctx.bf_knn_l2_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, dim, 2, d_knn.data_ptr(), flags)

        for _ in range(5):
            call()
        torch.cuda.synchronize()
        samples = {t: [] for t in TIMERS}
        for _ in range(SAMPLES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.timing_enable(False)
            e0.record(s)
            for _ in range(CALLS):
                call()
            e1.record(s)
            torch.cuda.synchronize()
            samples["call"].append(e0.elapsed_time(e1) * 1e3 / CALLS)
            ctx.timing_enable(True)                              # (the timers' own events stay out of the call time)
            ctx.timing_reset()
            for _ in range(CALLS):
                call()
            torch.cuda.synchronize()
            for t in TIMERS[:2]:
                ms, _ = ctx.timing_get(t)                          # already the mean per launch
                samples[t].append(ms * 1e3)
        ctx.timing_enable(False)
        ctx.set_option(PM_OPT_FILTER_FUSION, 0)
        out[name] = {"n_good": int(d_n.item()) if ratio else None,
                     "samples_us": {t: [round(float(v), 3) for v in samples[t]] for t in TIMERS}}
    print("RESULT " + json.dumps(out))


def median(v):
    v = sorted(v)
    return 0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2])


def main(parent, head, out_path):
    runs = []
    for side, lib in (("parent", parent), ("head", head), ("parent", parent), ("head", head)):
        env = dict(os.environ, PM_LIB_PATH=os.path.abspath(lib))
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child"], env=env,
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:], r.stderr[-4000:])
            raise SystemExit("child for %s ended with status %d: nothing more is started" % (side, r.returncode))
        runs.append((side, json.loads(line[0][7:])))
        print(side, "run done", flush=True)
    rec = {"calls_per_sample": CALLS, "samples_per_run": SAMPLES, "order": [s for s, _ in runs], "unit": "us", "workloads": {}}
    ok_all = True
    for name, *_ in WORKLOADS:
        w = {}
        for t in TIMERS:
            per_run = {"parent": [], "head": []}
            pooled = {"parent": [], "head": []}
            for side, res in runs:
                per_run[side].append(round(median(res[name]["samples_us"][t]), 3))
                pooled[side] += res[name]["samples_us"][t]
            spread = round(abs(per_run["parent"][0] - per_run["parent"][1]), 3)
            p, h = round(median(pooled["parent"]), 3), round(median(pooled["head"]), 3)
            within = h <= p + spread
            ok_all &= within or name.startswith("extra_")
            w[t] = {"parent_runs": per_run["parent"], "head_runs": per_run["head"], "parent": p, "head": h, "spread": spread,
                    "within": within}
            print("%-26s %-14s parent %9.3f head %9.3f spread %7.3f %s" % (name, t, p, h, spread, "ok" if within else "OVER"), flush=True)
        counts = {res[name]["n_good"] for _, res in runs}         # survivors of the ratio forms: one number for all four runs
        if len(counts) != 1:
            raise SystemExit("%s: the runs disagree on n_good: %s" % (name, counts))
        w["n_good"] = counts.pop()
        rec["workloads"][name] = w
    rec["all_within"] = ok_all
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0 if ok_all else 2           # (1: a child failed)


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child()
    else:
        sys.exit(main(*sys.argv[1:4]))
