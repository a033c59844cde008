"""GPU: `pm_cli --align OUT.pgm [--align-model M]` (correspondences -> 2-D RANSAC + refinement -> pm_warp_dev of image 2 into the
frame of image 1, SPEC S75-S77) on the fixture frame and its copy turned by 3 degrees, through the tracking route: the PGM
against the same chain through the library, the report line, the usage errors; and that a run without --align still prints
what the pinned fixture tests/golden/img_half_cli.npz holds."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import describe_ref as D
import lk_ref as R
import warp_ref as W
from points_matching_amd import api, build, io

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMG1 = os.path.join(GOLD, "img01_half.pgm")
MAX_KP, ITERS, THRESH, SEED = 512, 500, 2.0, 24301


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


def library_chain(img1, img2, model):
    """corners (block radius 10) -> track (radius 10, 3 levels) -> RANSAC + refinement -> warp: (dst, valid, n_inliers, n_valid)."""
    import torch
    import points_matching_amd as pm
    dev = torch.device("cuda", 0)
    h, w = img1.shape
    with pm.Context(0) as c:
        d_img1, d_img2 = torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev)
        d_kp = torch.zeros((MAX_KP, 2), dtype=torch.float32, device=dev)
        d_xy1, d_xy2 = torch.zeros_like(d_kp), torch.zeros_like(d_kp)
        d_n, d_cnt, d_ninl = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(3))
        d_key = torch.zeros(1, dtype=torch.int64, device=dev)
        d_M, d_Mr = torch.zeros(9, dtype=torch.float64, device=dev), torch.zeros(9, dtype=torch.float64, device=dev)
        d_mask = torch.zeros(MAX_KP, dtype=torch.uint8, device=dev)
        d_dst, d_val = torch.zeros((h, w), dtype=torch.uint8, device=dev), torch.zeros((h, w), dtype=torch.uint8, device=dev)
        d_info = torch.zeros(2, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        p1, p2 = c.pyramid(w, h, 3), c.pyramid(w, h, 3)
        try:
            p1.build_dev(d_img1.data_ptr())
            p2.build_dev(d_img2.data_ptr())
            c.corners_dev(p1, api.corner_params(10, 1e-4, 0.01, 8.0), MAX_KP, d_kp.data_ptr(), d_n.data_ptr())
            c.track_lk_gather_dev(p1, p2, d_kp.data_ptr(), d_n.data_ptr(), MAX_KP, api.lk_params(10, 3), d_xy1.data_ptr(), d_xy2.data_ptr(),
                                  d_cnt.data_ptr())
            view = api.PointsView(d_xy1.data_ptr(), d_xy2.data_ptr(), d_cnt.data_ptr(), 1, MAX_KP, 0, 1, 0)
            if model == "homography":
                flags = 0
                c.ransac_homography_run_dev(view, 0, ITERS, THRESH, SEED, d_key.data_ptr(), d_M.data_ptr(), d_mask.data_ptr(), MAX_KP, d_ninl.data_ptr())
                c.homography_refine_dev(view, d_mask.data_ptr(), d_M.data_ptr(), 10, d_Mr.data_ptr(), None)
            else:
                flags = api.PM_WARP_AFFINE
                kind = api.PM_AFFINE_PARTIAL if model == "similarity" else api.PM_AFFINE_FULL
                c.ransac_affine_run_dev(view, 0, ITERS, THRESH, SEED, d_key.data_ptr(), d_M.data_ptr(), d_mask.data_ptr(), MAX_KP, d_ninl.data_ptr(),
                                        model=kind)
                c.affine_refine_dev(view, d_mask.data_ptr(), d_M.data_ptr(), d_Mr.data_ptr(), None, model=kind)
            c.warp_dev(d_img2.data_ptr(), w, h, w, d_Mr.data_ptr(), api.warp_params(flags, 0), d_dst.data_ptr(), w, h, w, d_val.data_ptr(),
                       d_info.data_ptr())
            c.synchronize()
            info = d_info.cpu().numpy()
            assert info[0] == 0
            return d_dst.cpu().numpy(), d_val.cpu().numpy(), int(d_ninl.item()), int(info[1])
        finally:
            c.synchronize()
            p1.close()
            p2.close()


@pytest.mark.parametrize("model", ["homography", "similarity"])
def test_cli_align_writes_the_library_warp_and_reports(tmp_path, model):
    build.build_host()
    img1 = R.fixture()[0]
    img2 = D.rotate_frame(img1, 3)
    p2, out = str(tmp_path / "frame2.pgm"), str(tmp_path / "aligned.pgm")
    write_pgm(p2, img2)
    run = subprocess.run([build.HOST_BIN, "--img1", IMG1, "--img2", p2, "--features", "device", "--matcher", "track", "--points", "corners",
                          "--max-kp", str(MAX_KP), "--iters", str(ITERS), "--thresh", str(THRESH), "--seed", str(SEED), "--align", out] +
                         (["--align-model", model] if model != "homography" else []), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    dst, valid, ninl, n_valid = library_chain(img1, img2, model)
    assert (R.read_pgm(out) == dst).all()
    lines = run.stdout.strip().splitlines()
    assert lines[0] == "Good Matches are:" and not [ln for ln in lines if ln.startswith("result =") or ln.startswith("The average")]
    m = re.fullmatch(r"align: model=(\w+) inliers=(\d+) valid=(\d+) mad_before=([0-9.]+) mad_after=([0-9.]+)", lines[-1])
    assert m, lines[-1]
    v = valid == 1
    before = np.abs(img2.astype(np.int32) - img1.astype(np.int32))[v].mean()
    after = np.abs(dst.astype(np.int32) - img1.astype(np.int32))[v].mean()
    print(lines[-1])
    assert m.group(1) == model and int(m.group(2)) == ninl and int(m.group(3)) == n_valid == int(v.sum())
    assert abs(float(m.group(4)) - before) <= 1e-4 and abs(float(m.group(5)) - after) <= 1e-4 and after < before


@pytest.mark.parametrize("args,message", [(["--align-model", "affine"], "--align-model needs --align OUT.pgm"),
                                          (["--align", "x.pgm", "--align-model", "rigid"], "--align-model homography|affine|similarity"),
                                          (["--align", "x.pgm", "--json"], "--align takes no --json"),
                                          (["--align", "x.pgm", "--guided", "2"], "--align takes no --json"),
                                          (["--align", "x.pgm", "--print-epilines"], "--align takes no --json")])
def test_cli_align_usage_errors(args, message):
    build.build_host()
    run = subprocess.run([build.HOST_BIN, "--img1", IMG1, "--img2", IMG1] + args, capture_output=True, text=True, timeout=60)
    assert run.returncode == 2, (args, run.returncode, run.stderr)
    assert "pm_cli: " + message in run.stderr and run.stdout == "", (args, run.stderr)


def test_cli_align_needs_images():
    build.build_host()
    run = subprocess.run([build.HOST_BIN, "--align", "x.pgm", "--desc1", "a", "--desc2", "b", "--kp1", "c", "--kp2", "d"], capture_output=True,
                         text=True, timeout=60)
    assert run.returncode == 2 and "pm_cli: --align needs --img1 / --img2" in run.stderr and run.stdout == ""


def test_cli_without_align_still_matches_the_pinned_fixture(tmp_path):
    """Part (1) of test_cli_gpu.test_cli_image_pair_pinned_to_its_fixture: the match list, inliers, winning hypothesis and F bits."""
    build.build_host()
    g = np.load(os.path.join(GOLD, "img_half_cli.npz"), allow_pickle=False)
    iters, seed = int(g["params"][0]), int(g["params"][1])
    p = {}
    for name, arr in (("d1", g["desc1"].astype(np.float32)), ("d2", g["desc2"].astype(np.float32)), ("k1", g["kp1"]), ("k2", g["kp2"])):
        p[name] = str(tmp_path / (name + ".pmm"))
        io.save_pmm(p[name], arr)
    out = subprocess.run([build.HOST_BIN, "--desc1", p["d1"], "--desc2", p["d2"], "--kp1", p["k1"], "--kp2", p["k2"], "--filter", "ratio",
                          "--ratio", "0.8", "--method", "ransac8", "--iters", str(iters), "--seed", str(seed), "--thresh", "1.0", "--f-scale", "unit",
                          "--json"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    n = g["ratio_query"].size
    want = ["Good Matches are:"] + ["-- Good Match [%d] Keypoint 1: %d  -- Keypoint 2: %d  " % (i, g["ratio_query"][i], g["ratio_train"][i])
                                    for i in range(n)]
    assert lines[:n + 1] == want and not [ln for ln in lines if ln.startswith("align:")]
    js = json.loads(lines[-1])
    key = int(g["key"][0])
    assert js["matches"] == n and js["inliers"] == int(g["mask"].sum()) == key >> 32
    assert js["best_hyp"] == 0xFFFFFFFF - (key & 0xFFFFFFFF) and js["ransac_status"] == 0
    assert (np.array(js["F"], np.float64).view(np.uint64) == g["F_bits"]).all()
