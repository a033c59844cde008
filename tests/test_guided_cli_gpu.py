"""GPU: pm_cli --guided TAU (docs/SPEC.md S48-S50 behind the host tool).  On the golden image pair and on its pinned
features the option adds exactly one stdout line — both match counts and both inlier counts, recomputed here through the
library — and changes nothing else; without it the output is the pinned fixture's."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from points_matching_amd import api, build, io

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LINE = re.compile(r"^guided matching: tau = 3 px, matches (\d+) -> (\d+), inliers (\d+) -> (\d+)$")


def _split(stdout):
    lines = stdout.splitlines()
    guided = [ln for ln in lines if ln.startswith("guided matching:")]
    return lines, guided, [ln for ln in lines if not ln.startswith("guided matching:")]


def test_guided_option_on_the_pinned_features(tmp_path, ctx):
    g = np.load(os.path.join(GOLD, "img_half_cli.npz"), allow_pickle=False)
    iters, seed = int(g["params"][0]), int(g["params"][1])
    d1, d2 = g["desc1"].astype(np.float32), g["desc2"].astype(np.float32)
    p = {}
    for name, arr in (("d1", d1), ("d2", d2), ("k1", g["kp1"]), ("k2", g["kp2"])):
        p[name] = str(tmp_path / (name + ".pmm"))
        io.save_pmm(p[name], arr)
    cmd = [build.HOST_BIN, "--desc1", p["d1"], "--desc2", p["d2"], "--kp1", p["k1"], "--kp2", p["k2"], "--filter", "ratio",
           "--ratio", "0.8", "--method", "ransac8", "--iters", str(iters), "--seed", str(seed), "--thresh", "1.0", "--f-scale", "unit",
           "--json"]
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    lines, none, _ = _split(plain.stdout)
    n = g["ratio_query"].size
    want = ["Good Matches are:"] + ["-- Good Match [%d] Keypoint 1: %d  -- Keypoint 2: %d  " % (i, g["ratio_query"][i], g["ratio_train"][i])
                                    for i in range(n)]
    js = json.loads(lines[-1])
    assert none == [] and lines[:n + 1] == want and js["matches"] == n and js["inliers"] == int(g["mask"].sum())
    assert (np.array(js["F"], np.float64).view(np.uint64) == g["F_bits"]).all()

    out = subprocess.run(cmd + ["--guided", "3"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    glines, guided, rest = _split(out.stdout)
    assert len(guided) == 1 and glines[-2] == guided[0]
    drop_ms = lambda s: re.sub(r'"ms": \{[^}]*\}', "", s)                    # wall-clock figures differ between two runs
    assert rest[:-1] == lines[:-1] and drop_ms(rest[-1]) == drop_ms(lines[-1])
    m = LINE.match(guided[0])
    assert m, guided[0]
    got = [int(v) for v in m.groups()]
    # the same two passes through the library
    F = g["F_bits"].view(np.float64)
    knn, _ = ctx.bf_knn_guided_l2(d1, d2, g["kp1"], g["kp2"], api.PM_GUIDE_F_SAMPSON, F, 3.0, 2)
    good = api.filter_ratio(knn, 0.8)
    rc, _, _, n_inl, _ = ctx.ransac_fundamental(g["kp1"][good["queryIdx"]], g["kp2"][good["trainIdx"]], iters, 1.0, seed)
    assert rc == api.PM_OK
    assert got == [n, good.size, int(g["mask"].sum()), n_inl]
    print(guided[0])
    assert got[1] >= 8 and got[3] >= 8


def test_guided_option_on_the_golden_image_pair():
    cmd = [build.HOST_BIN, "--img1", os.path.join(GOLD, "img01_half.pgm"), "--img2", os.path.join(GOLD, "img02_half.pgm"),
           "--filter", "ratio", "--method", "ransac8", "--iters", "2000", "--json", "--guided", "3"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines, guided, _ = _split(out.stdout)
    assert len(guided) == 1 and lines[-2] == guided[0] and lines[0] == "Good Matches are:"
    m = LINE.match(guided[0])
    assert m, guided[0]
    js = json.loads(lines[-1])
    assert int(m.group(1)) == js["matches"] and int(m.group(3)) == js["inliers"]
    print(guided[0])


def test_guided_option_usage_errors(tmp_path):
    w = {"q": np.zeros((8, 8), np.float32), "kp": np.zeros((8, 2), np.float32)}
    for name, arr in w.items():
        io.save_pmm(str(tmp_path / (name + ".pmm")), arr)
    files = ["--desc1", str(tmp_path / "q.pmm"), "--desc2", str(tmp_path / "q.pmm"), "--kp1", str(tmp_path / "kp.pmm"),
             "--kp2", str(tmp_path / "kp.pmm")]
    for extra in (["--guided", "0"], ["--guided", "-1"], ["--guided", "abc"],
                  ["--guided", "3", "--filter", "ratio", "--method", "ransac8", "--gpus", "2"],
                  ["--guided", "3", "--filter", "ratio", "--method", "ransac8", "--mgpu"]):
        out = subprocess.run([build.HOST_BIN] + files + extra, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "pm_cli:" in out.stderr and out.stdout == "", extra
