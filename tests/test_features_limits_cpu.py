"""CPU: the reference and the inputs of tests/test_features_limits_gpu.py, pinned without a device, so that the GPU file
cannot pass on inputs that miss the paths it is there for.

The reference is the host extractor (host/pm_features.cpp, the specification of SPEC S53-S60) behind
tests/features_host_main.cpp, which takes contrast and edge_r where pm_cli fixes them.  Here: the driver equals pm_cli at the
defaults byte for byte; the large inputs select more than 1024 and more than 2048 rows; the small ones keep exactly the rows
the GPU file expects (none, one, two); the octave rule gives five octaves for 700x520 and no side below 32 anywhere (the
kernels' tiles and the 8-pixel scan border need none shorter than 17); the four non-default threshold pairs change the count."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import features_ref as R
from points_matching_amd import api, build, io


@pytest.mark.skipif(not os.path.exists(api.LIB_PATH), reason="pm_cli links libpm_hip.so, which is not built")
@pytest.mark.parametrize("kind", ["grad", "bits"])
def test_driver_equals_the_cli_at_the_defaults(tmp_path, kind):
    build.build_host()
    pgm = os.path.join(R.GOLD, "img01_half.pgm")
    pre = str(tmp_path / kind)
    out = subprocess.run([build.HOST_BIN, "--features", "host", "--descriptor", kind, "--img1", pgm, "--img2", pgm, "--extract-only",
                          "--save-features", pre, "--quiet"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    kp_c, rows_c = io.load_pmm(pre + "_kp1.pmm"), io.load_pmm(pre + "_desc1.pmm")
    kp, rows = R.run_host_driver(pgm, R.DEFAULT_MAX_KP, 0.03, 10.0, kind)          # pm_cli's --max-kp default is the extractor's
    assert kp.shape[0] == 240 and kp_c.dtype == kp.dtype and rows_c.dtype == rows.dtype == (np.float32 if kind == "grad" else np.uint8)
    assert kp_c.shape == kp.shape and kp_c.tobytes() == kp.tobytes()
    assert rows_c.shape == rows.shape and rows_c.tobytes() == rows.tobytes()
    # the cached form on the named input is the same run
    kp_n, rows_n = R.host_features("golden1", kind=kind)
    assert kp_n.tobytes() == kp.tobytes() and rows_n.tobytes() == rows.tobytes()


def test_large_inputs_are_the_bytes_of_the_blob_generator():
    """The two large inputs come from the windowed generator; the hashes are those of blobs(w, h, 11, w*h//60) itself."""
    for name in R.LARGE:
        assert hashlib.sha256(R.image(name).tobytes()).hexdigest() == R.LARGE_SHA256[name], name
    for name in ("97x131", "65x65", "33x40"):            # and on inputs small enough to run both
        w, h = (int(v) for v in name.split("x"))
        assert (R.blobs_windowed(w, h, 11, w * h // 60) == R.blobs(w, h, 11, w * h // 60)).all()


def test_large_inputs_select_more_than_one_and_two_compaction_rounds():
    """Rows the host keeps; the selection itself (what feat_compact scans, 1024 rows a round) is at least as long.  Both
    descriptor kinds keep the same keypoints here (the norm rule of the gradient form drops none)."""
    rows = {case: R.host_features(*case)[0].shape[0] for case in R.LARGE_CASES}
    print("rows of the large inputs:", rows)
    assert rows[("700x520", 4000)] > 2048                 # three rounds of feat_compact, nine workgroups of feat_rank
    assert rows[("640x480", 4000)] > 1024                 # two rounds
    assert rows[("700x520", 1025)] <= 1025 and rows[("700x520", 1024)] <= 1024 and rows[("700x520", 1023)] <= 1023
    assert rows[("700x520", 1023)] > 512                  # the cut cases still fill several workgroups
    assert rows == {("700x520", 4000): 2217, ("700x520", 1025): 874, ("700x520", 1024): 874, ("700x520", 1023): 873,
                    ("640x480", 4000): 1854, ("640x480", 1025): 855}
    for name, max_kp in R.LARGE_CASES:
        kp, _ = R.host_features(name, max_kp)
        kp_b, rows_b = R.host_features(name, max_kp, kind="bits")
        assert kp_b.tobytes() == kp.tobytes() and rows_b.shape == (kp.shape[0], 32)
    # a capped selection is a prefix of the full one, so its kept rows are a prefix of the kept rows
    full = R.host_features("700x520", 4000)
    for max_kp in (1025, 1024, 1023):
        kp, desc = R.host_features("700x520", max_kp)
        assert kp.tobytes() == full[0][:kp.shape[0]].tobytes() and desc.tobytes() == full[1][:kp.shape[0]].tobytes()
    # a row count that is no multiple of 8 (feat_gather_bits writes eight rows a workgroup)
    assert any(R.host_features(*case)[0].shape[0] % 8 for case in R.LARGE_CASES)


def test_max_kp_one():
    for name in ("97x131", "700x520"):
        for kind in ("grad", "bits"):
            n = R.host_features(name, 1, kind=kind)[0].shape[0]
            assert n in (0, 1)


@pytest.mark.parametrize("kind", ["grad", "bits"])
def test_small_inputs_keep_exactly_these_rows(kind):
    for name in R.NO_ROWS:
        w, h = (int(v) for v in name.split("x"))
        assert min(w, h) >= 32
        kp, rows = R.host_features(name, kind=kind)
        assert kp.shape == (0, 2) and rows.shape[0] == 0, name
    for name, n in R.FEW_ROWS:
        kp, rows = R.host_features(name, kind=kind)
        assert kp.shape == (n, 2) and rows.shape[0] == n, name


def test_border_skipped_inputs_do_have_candidates():
    """63x64 and 64x64 select candidates, and the border rule (r2 >= 23 on every side) drops each of them: a non-empty
    selection with no valid row.  Counted with the numpy restatement of the levels and of the scan."""
    for name in ("63x64", "64x64"):
        img = R.image(name)
        n_oct = len(R.plan_octaves(img.shape[1], img.shape[0]))
        assert n_oct == (1 if name == "63x64" else 2)
        cand = R.candidate_responses(R.NumpyLevels(img), n_oct)
        print("candidates of %s: %d" % (name, cand.size))
        assert cand.size >= 1, name
        assert R.host_features(name)[0].shape[0] == 0


def test_five_octave_input_has_one_candidate_per_octave():
    """"five": one candidate in each of the five octaves, so octave 4's pos_base, oct_off and geom record decide a result:
    its candidate is the strongest and cannot be kept on a 32x32 plane, so max_kp = 1 gives no row, and every further row of
    the selection adds one keypoint, octave 3's first."""
    img = R.image("five")
    assert R.plan_octaves(512, 512) == [(512, 512), (256, 256), (128, 128), (64, 64), (32, 32)]
    lev = R.NumpyLevels(img)

    class One:
        def __init__(self, o):
            self.o = o

        def detect_level(self, _, i):
            return lev.detect_level(self.o, i)

    per_octave = [R.candidate_responses(One(o), 1) for o in range(5)]
    assert [c.size for c in per_octave] == [1, 1, 1, 1, 1]
    resp = [float(c[0]) for c in per_octave]
    assert resp[4] > resp[3] > resp[0] > resp[1] > resp[2]
    for kind in ("grad", "bits"):
        for max_kp in (1, 2, 3, 4, 5, R.DEFAULT_MAX_KP):
            kp, rows = R.host_features("five", max_kp, kind=kind)
            assert kp.tolist() == [list(p) for p in R.FIVE_KEPT[:max(0, min(max_kp, 5) - 1)]], (kind, max_kp)


def test_octave_plan():
    assert R.plan_octaves(700, 520) == [(700, 520), (350, 260), (175, 130), (88, 65), (44, 33)]
    assert len(R.plan_octaves(640, 480)) == 4 and len(R.plan_octaves(512, 512)) == 5 and len(R.plan_octaves(511, 600)) == 4
    names = list(R.LARGE) + list(R.NO_ROWS) + [n for n, _ in R.FEW_ROWS] + [R.THRESHOLD_IMAGE, "31x32", "32x31"]
    for name in names:
        w, h = (int(v) for v in name.split("x"))
        if w < 32 or h < 32:                              # the small-image rule answers before any plan
            continue
        plan = R.plan_octaves(w, h)
        assert 1 <= len(plan) <= 5
        assert all(min(ow, oh) >= 32 for ow, oh in plan), (name, plan)
    assert [R.plan_octaves(w, 40)[0][0] for w in (32, 33)] == [32, 33] and len(R.plan_octaves(32, 32)) == 1


def test_thresholds_reach_the_extractor():
    """Each non-default pair must change the count, or the GPU file's threshold cases would pass with the arguments ignored.
    On 97x131 three of the four pairs do (29 rows at the defaults; 31, 28, 24 at (0.015, 10), (0.06, 10), (0.03, 3)).  The
    fourth cannot: the blobs are round, none of the image's extrema fails the edge test at 10 and passes it at 30, and
    (0.03, 30) selects the same 78 candidates and keeps the same 29 rows as the defaults.  So the four pairs also run on the
    golden1 photograph, where every one of them changes the count (240 rows at the defaults; 320, 111, 117, 263)."""
    for name, same in ((R.THRESHOLD_IMAGE, ((0.03, 30.0),)), (R.THRESHOLD_PHOTO, ())):
        base = R.host_features(name)[0].shape[0]
        counts = {}
        for contrast, edge_r in R.THRESHOLDS:
            for kind in ("grad", "bits"):
                n = R.host_features(name, contrast=contrast, edge_r=edge_r, kind=kind)[0].shape[0]
                assert n >= 1 and (n != base or (contrast, edge_r) in same), (name, contrast, edge_r, kind, n, base)
            counts[(contrast, edge_r)] = n
        print("%s: rows at the defaults %d; at the threshold pairs: %s" % (name, base, counts))
        assert counts[(0.015, 10.0)] > base > counts[(0.06, 10.0)] and counts[(0.03, 30.0)] >= base > counts[(0.03, 3.0)]
        # a negative contrast lets every extremum through that passes the edge test
        assert R.host_features(name, contrast=-1.0)[0].shape[0] > counts[(0.015, 10.0)]
    base = R.host_features(R.THRESHOLD_PHOTO)[0].shape[0]
    assert all(R.host_features(R.THRESHOLD_PHOTO, contrast=c, edge_r=e)[0].shape[0] != base for c, e in R.THRESHOLDS)
