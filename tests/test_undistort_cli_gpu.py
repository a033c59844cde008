"""GPU: `pm_cli --undistort OUT.pgm --img1 IN.pgm --camera fx,fy,cx,cy --lens k1,k2,p1,p2,k3 [--new-camera fx,fy,cx,cy] [--json]`
(SPEC S79-S83) on the fixture frame: the PGM against api.Context.undistort byte for byte, the printed n_valid, the usage errors."""
import json
import os
import re
import subprocess

import pytest

import lk_ref as R
from points_matching_amd import build

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMG1 = os.path.join(GOLD, "img01_half.pgm")
CAMERA, LENS, NEW_CAMERA = "400,410.5,248,165", "-0.28,0.07,1e-3,-5e-4,0", "360,360,250.25,160"


def _numbers(text):
    return tuple(float(v) for v in text.split(","))


@pytest.mark.parametrize("new_camera,as_json", [(None, False), (NEW_CAMERA, True)])
def test_cli_undistort_writes_the_library_image_and_reports(tmp_path, new_camera, as_json):
    import points_matching_amd as pm
    build.build_host()
    out = str(tmp_path / "undistorted.pgm")
    run = subprocess.run([build.HOST_BIN, "--undistort", out, "--img1", IMG1, "--camera", CAMERA, "--lens", LENS] +
                         (["--new-camera", new_camera] if new_camera else []) + (["--json"] if as_json else []),
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    img = R.fixture()[0]
    with pm.Context(0) as c:
        dst, valid, n_valid = c.undistort(img, _numbers(CAMERA), _numbers(LENS), K_new=_numbers(new_camera) if new_camera else None)
    assert (R.read_pgm(out) == dst).all() and 0 < n_valid <= img.size and (dst != img).any()
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 1
    if as_json:
        assert json.loads(lines[0]) == {"undistort": {"width": img.shape[1], "height": img.shape[0], "n_valid": n_valid}}
    else:
        m = re.fullmatch(r"undistort: valid=(\d+)", lines[0])
        assert m and int(m.group(1)) == n_valid == int(valid.sum())


@pytest.mark.parametrize("args,message", [
    (["--camera", "400,410,248", "--lens", LENS], "--camera fx,fy,cx,cy (four numbers)"),
    (["--camera", "400,410,248,165,1", "--lens", LENS], "--camera fx,fy,cx,cy (four numbers)"),
    (["--camera", "400,abc,248,165", "--lens", LENS], "--camera fx,fy,cx,cy (four numbers)"),
    (["--camera", "400,410,nan,165", "--lens", LENS], "--camera fx,fy,cx,cy (four numbers)"),
    (["--camera", CAMERA, "--lens", "-0.28,0.07"], "--lens k1,k2,p1,p2,k3 (five numbers)"),
    (["--camera", CAMERA, "--lens", "-0.28;0.07;0;0;0"], "--lens k1,k2,p1,p2,k3 (five numbers)"),
    (["--camera", CAMERA, "--lens", LENS + ","], "--lens k1,k2,p1,p2,k3 (five numbers)"),
    (["--camera", CAMERA, "--lens", LENS, "--new-camera", "1,2"], "--new-camera fx,fy,cx,cy (four numbers)"),
    (["--camera", CAMERA], "--undistort needs --img1 IN.pgm --camera fx,fy,cx,cy --lens k1,k2,p1,p2,k3"),
    (["--lens", LENS], "--undistort needs --img1 IN.pgm --camera fx,fy,cx,cy --lens k1,k2,p1,p2,k3")])
def test_cli_undistort_usage_errors(tmp_path, args, message):
    build.build_host()
    out = str(tmp_path / "never.pgm")
    run = subprocess.run([build.HOST_BIN, "--undistort", out, "--img1", IMG1] + args, capture_output=True, text=True, timeout=60)
    assert run.returncode == 2, (args, run.returncode, run.stderr)
    assert "pm_cli: " + message in run.stderr and run.stdout == "" and not os.path.exists(out), (args, run.stderr)


def test_cli_undistort_bad_model_and_stray_options(tmp_path):
    build.build_host()
    out = str(tmp_path / "never.pgm")
    run = subprocess.run([build.HOST_BIN, "--undistort", out, "--img1", IMG1, "--camera", "0,410,248,165", "--lens", LENS], capture_output=True,
                         text=True, timeout=60)
    assert run.returncode != 0 and "K needs finite values" in run.stderr and not os.path.exists(out)          # PM_E_INVALID from the library
    run = subprocess.run([build.HOST_BIN, "--img1", IMG1, "--img2", IMG1, "--lens", LENS], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "pm_cli: --camera, --lens and --new-camera need --undistort OUT.pgm" in run.stderr and run.stdout == ""
