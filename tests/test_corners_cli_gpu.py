"""GPU: `pm_cli --matcher track --points corners` (minimum-eigenvalue corners of SPEC S67-S70 on image 1 in place of the DoG
keypoints, tracked into image 2, gathered, estimated) on the fixture frame and frame R; its counts against the API's; the
argument errors."""
import json
import os
import subprocess

import numpy as np
import pytest

import lk_ref as R
from points_matching_amd import api, build

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMG1 = os.path.join(GOLD, "img01_half.pgm")
MAX_KP = 512


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def api_counts(img1, img2, r, levels, fb, dist, quality, min_eig):
    """(corners found on image 1, rows gathered after tracking them into image 2)."""
    import torch
    import points_matching_amd as pm
    dev = torch.device("cuda", 0)
    h, w = img1.shape
    d1, d2 = torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev)
    d_kp = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    d_xy1 = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
    d_xy2 = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with pm.Context(0) as c:
        p1, p2 = c.pyramid(w, h, levels), c.pyramid(w, h, levels)
        try:
            p1.build_dev(d1.data_ptr())
            p2.build_dev(d2.data_ptr())
            c.corners_dev(p1, api.corner_params(r, min_eig, quality, dist), MAX_KP, d_kp.data_ptr(), d_n.data_ptr())
            c.track_lk_gather_dev(p1, p2, d_kp.data_ptr(), d_n.data_ptr(), MAX_KP, api.lk_params(r, levels, fb_thresh=fb), d_xy1.data_ptr(),
                                  d_xy2.data_ptr(), d_cnt.data_ptr())
            c.synchronize()
            return int(d_n.item()), int(d_cnt.item())
        finally:
            c.synchronize()
            p1.close()
            p2.close()


@pytest.mark.parametrize("extra,r,levels,fb,dist,quality,min_eig",
                         [([], 10, 3, 0.0, 8.0, 0.01, 1e-4),
                          (["--lk-radius", "7", "--lk-levels", "2", "--lk-fb", "0.5", "--corner-dist", "12.5", "--corner-quality", "0.05",
                            "--corner-min-eig", "2"], 7, 2, 0.5, 12.5, 0.05, 2.0)])
def test_cli_finds_corners_tracks_and_estimates(tmp_path, extra, r, levels, fb, dist, quality, min_eig):
    build.build_host()
    img1 = R.fixture()[0]
    img2 = R.frame_r(img1)
    p2 = str(tmp_path / "frame_r.pgm")
    write_pgm(p2, img2)
    run = subprocess.run([build.HOST_BIN, "--img1", IMG1, "--img2", p2, "--features", "device", "--matcher", "track", "--points", "corners",
                          "--method", "ransac8", "--max-kp", str(MAX_KP), "--json"] + extra, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    rep = json.loads(lines[-1])
    n_c, cnt = api_counts(img1, img2, r, levels, fb, dist, quality, min_eig)
    print("cli: n1 %d, matches %d, inliers %d; api: %d corners, %d gathered" % (rep["n1"], rep["matches"], rep["inliers"], n_c, cnt))
    assert rep["n1"] == n_c > 60 and rep["n2"] == 0
    assert rep["matches"] == cnt > 60
    assert rep["ransac_status"] == 0 and rep["inliers"] >= 8 and np.isfinite(rep["F"]).all()
    # the estimator output is the usual one: the match list, one residual line per match, the mean
    assert lines[0] == "Good Matches are:"
    assert sum(ln.startswith("result = ") for ln in lines) == cnt
    assert any(ln.startswith("The average value is") for ln in lines)


NEEDS, RANGE = "--points dog|corners needs --matcher track", "--corner-dist 0..1e6"


@pytest.mark.parametrize("args,message", [(["--matcher", "bf", "--points", "corners"], NEEDS), (["--points", "corners"], NEEDS),
                                          (["--matcher", "bf", "--points", "dog"], NEEDS), (["--matcher", "track", "--points", "harris"], NEEDS),
                                          (["--matcher", "track", "--corner-dist", "5"], NEEDS),
                                          (["--matcher", "track", "--points", "dog", "--corner-quality", "0.1"], NEEDS),
                                          (["--matcher", "track", "--points", "corners", "--corner-dist", "-1"], RANGE),
                                          (["--matcher", "track", "--points", "corners", "--corner-dist", "2e6"], RANGE),
                                          (["--matcher", "track", "--points", "corners", "--corner-quality", "1.5"], RANGE),
                                          (["--matcher", "track", "--points", "corners", "--corner-min-eig", "-2"], RANGE),
                                          (["--matcher", "track", "--points", "corners", "--corner-min-eig", "nan"], RANGE),
                                          (["--matcher", "track", "--points"], "--points needs a value")])
def test_cli_argument_errors(args, message):
    """Each case must be refused by the validation of the new options, with its message, not as an unknown option."""
    build.build_host()
    run = subprocess.run([build.HOST_BIN, "--img1", IMG1, "--img2", IMG1, "--features", "device"] + args, capture_output=True, text=True,
                         timeout=60)
    assert run.returncode == 2, (args, run.returncode, run.stderr)
    assert "pm_cli: " + message in run.stderr and run.stdout == "", (args, run.stderr)
