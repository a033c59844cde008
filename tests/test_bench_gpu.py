"""GPU: bench.py's N > 1 code path with two ranks sharing this box's one GPU (gloo backend, --single-device): the
launcher branch, both exchanges (survivor blocks, 80-byte records) through the HIP entry points, weak and strong
scaling, checked by the bench's own oracle parity flag.  The driver's real multi-GPU run uses RCCL on N GPUs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, ranks=2):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
           "--sustain-seconds", "0"] + (["--gpus", "2", "--backend", "gloo", "--single-device"] if ranks == 2 else []) + extra
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def _load_dump(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_two_ranks_c3_shape(scaling, tmp_path):
    d = _run(["--nq", "2048", "--nt", "2048", "--hyps", "3000", "--scaling", scaling, "--dump-outputs", str(tmp_path)])
    assert d["n_gpus"] == 2 and d["parity"] == "ok" and d["scaling"] == scaling
    assert d["ransac"]["n_matches"] > 300 and d["ransac"]["inliers"] > 100
    assert "ransac_fused" in d["kernels_us"] and "ransac_finish" in d["kernels_us"]
    # the form of the timed region is the one the warm-up trial found faster (max over ranks); both are reported
    tr = d["step_form_trial"]
    piped = tr["pipelined_ms_per_step"] < tr["serial_ms_per_step"]
    assert d["step_form"].startswith("pipelined" if piped else "serial")
    assert d["ms_per_step"] == (d["ms_per_step_pipelined"] if piped else d["ms_per_step_serial"])
    assert d["ms_per_step_serial"] > 0 and d["ms_per_step_pipelined"] > 0
    assert "timing_note" in d["config"]                   # two processes on one GPU: not performance data
    assert d["collectives"]["ranks"] == 2 and d["collectives"]["allgather_records_us"] > 0
    # --dump-outputs on rank 0: the gathered correspondences, the mask over them and F agree with the JSON line
    o = _load_dump(str(tmp_path))
    assert o["xy1"].shape == o["xy2"].shape == (d["ransac"]["n_matches"], 2) and o["inlier_mask"].size == o["xy1"].shape[0]
    assert o["n_inliers"] == o["inlier_mask"].sum() == d["ransac"]["inliers"] and o["best_hyp"] == d["ransac"]["best_hyp"]
    assert o["F"].shape == (3, 3) and o["F"].dtype == np.float64


def test_two_ranks_c4_strong_shape():
    d = _run(["--workload", "c4", "--scaling", "strong", "--nq", "4096", "--nt", "4096", "--hyps", "5000"])
    assert d["n_gpus"] == 2 and d["parity"] == "ok" and d["scaling"] == "strong"


def test_dump_outputs_is_the_timed_step_bit_for_bit(tmp_path):
    """One rank, --dump-outputs: every array the timed step hands its caller (2-NN records, ratio survivors, gathered
    points, F, inlier mask, counts) equals the CPU oracle on the same seeded inputs, bit for bit; --steps is what ran."""
    from oracle import pm_oracle as O
    from points_matching_amd import synth
    nq, H = 1024, 1000
    d = _run(["--workload", "c2", "--nq", str(nq), "--nt", str(nq), "--hyps", str(H), "--steps", "4", "--headline-only",
              "--no-large", "--dump-outputs", str(tmp_path)], ranks=1)
    assert d["steps"] == 4 and d["n_gpus"] == 1 and d["parity"] == "ok"
    o = _load_dump(str(tmp_path))
    assert all(a.dtype in (np.float32, np.float64) for a in o.values())
    w = synth.pair_workload(nq, nq, 128, seed=0xC3, rank=0, kind="sift")
    knn = O.bf_knn_l2(w["q"], w["t"], 2)
    good = O.filter_ratio(knn, 0.8)
    for pre, m in (("knn", knn), ("good", good)):
        for f, name in (("queryIdx", "query_idx"), ("trainIdx", "train_idx"), ("imgIdx", "img_idx")):
            assert (o["%s_%s" % (pre, name)] == m[f]).all(), (pre, name)
        assert (o[pre + "_distance"].view(np.uint32) == m["distance"].view(np.uint32)).all(), pre
    xy1, xy2 = w["kp1"][good["queryIdx"]], w["kp2"][good["trainIdx"]]
    assert (o["xy1"].view(np.uint32) == xy1.view(np.uint32)).all() and (o["xy2"].view(np.uint32) == xy2.view(np.uint32)).all()
    rc, F, mask, ninl, key = O.ransac_fundamental(xy1, xy2, H, 1.0, 0x5EED)
    assert rc == 0 and o["n_matches"] == good.size == d["ransac"]["n_matches"]
    assert o["n_inliers"] == ninl == d["ransac"]["inliers"] and (o["inlier_mask"] == mask).all()
    assert o["best_hyp"] == 0xFFFFFFFF - (key & 0xFFFFFFFF) == d["ransac"]["best_hyp"]
    assert (o["F"].view(np.uint64) == F.view(np.uint64)).all()
