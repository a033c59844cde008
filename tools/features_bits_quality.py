"""Matching quality of the binary descriptors (docs/SPEC.md S58-S60) against the 128-D gradient rows, on the CPU.

    python tools/features_bits_quality.py [--out profiles/features_bits_quality.txt]

The host extractor (`pm_cli --features host --extract-only --descriptor bits|grad`) describes the two 496 x 330 fixtures;
a numpy brute-force 2-NN (Hamming for the bits, squared L2 for the gradient rows), the ratio test at 0.8 in float32 and
the CPU oracle's RANSAC-F (2000 hypotheses, 1 px Sampson threshold, seed 0x5EED: the arguments of the device pipeline
tests) give good matches and inliers.  No GPU is used."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import features_bits_ref as ref  # noqa: E402
import pm_oracle  # noqa: E402
from points_matching_amd import build, io  # noqa: E402


def two_nn_l2(q, t):
    q, t = q.astype(np.int64), t.astype(np.int64)
    d = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2 * q @ t.T
    idx = np.argsort(d, axis=1, kind="stable")[:, :2]
    return idx, np.sqrt(np.take_along_axis(d, idx, axis=1).astype(np.float32))


def quality(kind, tmp):
    pre = os.path.join(tmp, kind)
    img = [os.path.join(ROOT, "tests", "golden", "img0%d_half.pgm" % i) for i in (1, 2)]
    out = subprocess.run([build.build_host(), "--features", "host", "--descriptor", kind, "--img1", img[0], "--img2", img[1],
                          "--extract-only", "--quiet", "--save-features", pre], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    d1, d2 = io.load_pmm(pre + "_desc1.pmm"), io.load_pmm(pre + "_desc2.pmm")
    k1, k2 = io.load_pmm(pre + "_kp1.pmm").reshape(-1, 2), io.load_pmm(pre + "_kp2.pmm").reshape(-1, 2)
    idx, dist = ref.hamming_2nn(d1, d2) if kind == "bits" else two_nn_l2(d1, d2)
    dist = dist.astype(np.float32)
    good = np.nonzero(dist[:, 0] < np.float32(0.8) * dist[:, 1])[0]
    rc, F, mask, n_inl, key = pm_oracle.ransac_fundamental(k1[good], k2[idx[good, 0]], 2000, 1.0, 0x5EED)
    set_bits = float(np.unpackbits(np.concatenate([d1, d2])).mean()) if kind == "bits" else None
    return d1.shape[0], d2.shape[0], good.size, n_inl, rc, set_bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_bits_quality.txt"))
    a = ap.parse_args()
    pm_oracle.build()
    lines = ["host extractor on tests/golden/img01_half.pgm, img02_half.pgm; numpy 2-NN, ratio 0.8, oracle RANSAC-F (2000 hypotheses, "
             "1 px, seed 0x5EED)", "descriptor  keypoints  good_matches  inliers  ransac_status"]
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ("grad", "bits"):
            n1, n2, good, inl, rc, share = quality(kind, tmp)
            lines.append("%-10s  %d / %d  %d  %d  %d" % (kind, n1, n2, good, inl, rc))
            if share is not None:
                lines.append("share of set bits: %.3f" % share)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
