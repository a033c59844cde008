"""GPU: `pm_cli --stereo OUT.pgm --img1 L.pgm --img2 R.pgm --num-disp N [--min-disp M] [--radius R] [--uniqueness U]
[--lr-check T16] [--json]` (SPEC S88) on the two-plane scene written as PGMs: the decoded 16-bit map against the plain-C
restatement value for value, the printed n_valid, the error exits."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import stereo_ref as S
from points_matching_amd import build

pytestmark = pytest.mark.gpu


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img, np.uint8).tobytes())


def _read_pgm16(path):
    data = open(path, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n65535\n", data)
    assert m, data[:20]
    w, h = int(m.group(1)), int(m.group(2))
    body = data[m.end():]
    assert len(body) == 2 * w * h
    return np.frombuffer(body, ">u2").reshape(h, w).astype(np.int64)


@pytest.mark.parametrize("min_disp,lr,as_json", [(0, None, False), (-2, 16, True)])
def test_cli_stereo_writes_the_restatement_map_and_reports(tmp_path, min_disp, lr, as_json):
    build.build_host()
    left, right, _ = S.scene(1, True)
    l, r, out = str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "disp.pgm")
    _write_pgm(l, left)
    _write_pgm(r, right)
    run = subprocess.run([build.HOST_BIN, "--stereo", out, "--img1", l, "--img2", r, "--num-disp", "16", "--min-disp", str(min_disp), "--radius", "2",
                          "--uniqueness", "10"] + (["--lr-check", str(lr)] if lr is not None else []) + (["--json"] if as_json else []),
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    want, n = S.bm(left, right, min_disp, 16, 2, 10)
    if lr is not None:
        want, n = S.lr_check(want, S.bm(left, right, min_disp, 16, 2, 10, S.FROM_RIGHT)[0], lr)
    want = want.astype(np.int64)
    coded = np.where(want == S.INVALID, 0, want - 16 * min_disp + 1)
    got = _read_pgm16(out)
    assert (got == coded).all() and int((got != 0).sum()) == n and 0 < n < left.size
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 1
    if as_json:
        assert json.loads(lines[0]) == {"stereo": {"width": S.SCENE_W, "height": S.SCENE_H, "n_valid": n}}
    else:
        m = re.fullmatch(r"stereo: valid=(\d+)", lines[0])
        assert m and int(m.group(1)) == n


def test_cli_stereo_error_exits(tmp_path):
    build.build_host()
    left, right, _ = S.scene(1)
    l, r, small, out = str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm"), str(tmp_path / "small.pgm"), str(tmp_path / "never.pgm")
    _write_pgm(l, left)
    _write_pgm(r, right)
    _write_pgm(small, right[:, :-1])
    run = subprocess.run([build.HOST_BIN, "--stereo", out, "--img1", l, "--img2", small, "--num-disp", "16"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 1 and "--stereo needs two images of one size" in run.stderr and run.stdout == "" and not os.path.exists(out)
    run = subprocess.run([build.HOST_BIN, "--stereo", out, "--img1", l, "--img2", r], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "--stereo needs --img1 L.pgm --img2 R.pgm --num-disp N" in run.stderr and not os.path.exists(out)
    run = subprocess.run([build.HOST_BIN, "--stereo", out, "--img1", l, "--img2", r, "--num-disp", "16", "--radius", "11"], capture_output=True, text=True,
                         timeout=60)
    assert run.returncode == 1 and "radius outside [1, 10]" in run.stderr and not os.path.exists(out)          # PM_E_INVALID from the library
    for extra in (["--align", out], ["--guided", "2.0"], ["--epilines", out], ["--matcher", "track"], ["--features", "device"], ["--filter", "ratio"],
                  ["--undistort", out]):                             # a switch of another mode is refused, not ignored
        run = subprocess.run([build.HOST_BIN, "--stereo", out, "--img1", l, "--img2", r, "--num-disp", "16"] + extra, capture_output=True, text=True,
                             timeout=60)
        assert run.returncode == 2 and "pm_cli: --stereo " in run.stderr and run.stdout == "" and not os.path.exists(out), (extra, run.stderr)
    run = subprocess.run([build.HOST_BIN, "--img1", l, "--img2", r, "--num-disp", "16"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "need --stereo OUT.pgm" in run.stderr and run.stdout == ""
