"""GPU: `pm_cli --features corners` (pyramid -> minimum-eigenvalue corners -> oriented 256-bit descriptors of SPEC S71-S74 on both
images, then the Hamming path of --features device --descriptor bits) on the fixture frame against frame R and against the
30-degree frame; its counts against the API chain's; the usage errors."""
import json
import os
import subprocess

import numpy as np
import pytest

import describe_ref as D
import lk_ref as R
from points_matching_amd import api, build

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMG1 = os.path.join(GOLD, "img01_half.pgm")
MAX_KP = 512


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def api_counts(imgs, dist, quality, min_eig):
    """Rows that corners + gather-describe at level 0 leave on each image."""
    import torch
    import points_matching_amd as pm
    dev = torch.device("cuda", 0)
    out = []
    with pm.Context(0) as c:
        for img in imgs:
            h, w = img.shape
            d_img = torch.from_numpy(img).to(dev)
            d_kp = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
            d_n = torch.zeros(1, dtype=torch.int32, device=dev)
            d_xy = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
            d_desc = torch.zeros((MAX_KP, 32), dtype=torch.uint8, device=dev)
            d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            p = c.pyramid(w, h, 0)
            try:
                p.build_dev(d_img.data_ptr())
                c.corners_dev(p, api.corner_params(10, min_eig, quality, dist), MAX_KP, d_kp.data_ptr(), d_n.data_ptr())
                c.describe_points_gather_dev(p, d_kp.data_ptr(), d_n.data_ptr(), MAX_KP, api.describe_params(), d_xy.data_ptr(),
                                             d_desc.data_ptr(), d_cnt.data_ptr())
                c.synchronize()
                out.append(int(d_cnt.item()))
            finally:
                c.synchronize()
                p.close()
    return out


@pytest.mark.parametrize("frame,extra,dist,quality,min_eig",
                         [("R", [], 8.0, 0.01, 1e-4), ("rot30", [], 8.0, 0.01, 1e-4),
                          ("R", ["--filter", "ratio", "--corner-dist", "6", "--corner-quality", "0.02", "--corner-min-eig", "1"], 6.0, 0.02, 1.0)])
def test_cli_describes_corners_matches_and_estimates(tmp_path, frame, extra, dist, quality, min_eig):
    build.build_host()
    img1 = R.fixture()[0]
    img2 = R.frame_r(img1) if frame == "R" else D.rotate_frame(img1, 30.0)
    p2 = str(tmp_path / "frame2.pgm")
    write_pgm(p2, img2)
    run = subprocess.run([build.HOST_BIN, "--img1", IMG1, "--img2", p2, "--features", "corners", "--method", "ransac8", "--max-kp", str(MAX_KP),
                          "--json"] + extra, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    rep = json.loads(lines[-1])
    n1, n2 = api_counts((img1, img2), dist, quality, min_eig)
    print("cli %s: n1 %d, n2 %d, matches %d, inliers %d; api: %d and %d rows" % (frame, rep["n1"], rep["n2"], rep["matches"], rep["inliers"], n1, n2))
    assert rep["n1"] == n1 and rep["n2"] == n2
    assert rep["matches"] > 60
    assert rep["ransac_status"] == 0 and rep["inliers"] >= 8 and np.isfinite(rep["F"]).all()
    assert lines[0] == "Good Matches are:" or lines[0].startswith("The Best Match")


@pytest.mark.parametrize("args,message", [(["--features", "corners", "--descriptor", "grad"], "--features corners describes by bits and takes no --descriptor grad"),
                                          (["--features", "corners", "--matcher", "track"], "--features corners takes --matcher bf only"),
                                          (["--features", "corners", "--matcher", "flann"], "--features corners takes --matcher bf only"),
                                          (["--features", "corners", "--points", "corners"], "--features corners takes no --points"),
                                          (["--features", "corners", "--points", "dog"], "--features corners takes no --points"),
                                          (["--features", "corners", "--corner-dist", "-1"], "--corner-dist 0..1e6"),
                                          (["--features", "harris"], "--features host|device")])
def test_cli_usage_errors(args, message):
    build.build_host()
    run = subprocess.run([build.HOST_BIN, "--img1", IMG1, "--img2", IMG1] + args, capture_output=True, text=True, timeout=60)
    assert run.returncode == 2, (args, run.returncode, run.stderr)
    assert "pm_cli: " + message in run.stderr and run.stdout == "", (args, run.stderr)


def test_cli_corners_need_images():
    build.build_host()
    run = subprocess.run([build.HOST_BIN, "--features", "corners", "--desc1", "a", "--desc2", "b", "--kp1", "c", "--kp2", "d"], capture_output=True,
                         text=True, timeout=60)
    assert run.returncode == 2 and "pm_cli: --features corners needs --img1 / --img2" in run.stderr and run.stdout == ""
