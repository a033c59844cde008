"""CPU: the plain-C restatement of SPEC S61-S66 (tests/lk_ref.c) is pinned here, so that the GPU tests compare the kernels
against something that was itself checked; plus the ABI of the tracking entry points.

The figures quoted below as "prototype" are properties of the SPECIFICATION: they come from a numpy prototype of S61-S66 run
on a CPU, and they are checked here against the C restatement on the CPU.  They say nothing about a GPU run; the GPU tests
compare bit for bit against the restatement and have no tolerance.  A bound below is the prototype's worst figure times about
three (frame S), or the issue's stated bound (frame R); the restatement's own figures are printed before each assertion."""
import os
import re
import subprocess

import numpy as np
import pytest

import lk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pm_pyramid_create", "pm_pyramid_destroy", "pm_pyramid_build_dev", "pm_pyramid_level_get", "pm_track_lk_dev",
         "pm_track_lk_gather_dev", "pm_track_lk"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def fx():
    """The fixture frame, its keypoints and the pyramids (max_level 3) of the frames the tests track into; built once."""
    img, kp = R.fixture()
    d = {"img": img, "kp": kp, "p1": R.Pyramid(img, 3)}
    d["pS"] = R.Pyramid(R.frame_s(img), 3)
    d["pR"] = R.Pyramid(R.frame_r(img), 3)
    d["true_r"] = R.frame_r_map(kp, img.shape)
    return d


# ---- ABI -------------------------------------------------------------------------------------------------------------------

def test_abi_header_declares_and_library_exports_the_tracking_names():
    from points_matching_amd import api
    hdr = open(os.path.join(ROOT, "include", "pm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in api.EXPORTS, name
    assert "typedef struct pm_pyramid pm_pyramid;" in code and "pm_lk_params;" in code and "PM_LK_USE_INITIAL" in code
    r = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    syms = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    assert not [n for n in NAMES if n not in syms]
    assert tuple(f[0] for f in api.LkParams._fields_) == tuple(f[0] for f in R.Params._fields_)
    import ctypes
    assert ctypes.sizeof(api.LkParams) == 32


def test_restatement_is_not_part_of_the_library():
    pkg = os.path.join(ROOT, "points_matching_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".hip", ".cpp", ".hpp", ".h", ".py")):
                assert "lk_ref" not in open(os.path.join(d, f), errors="replace").read(), f


# ---- S61 -------------------------------------------------------------------------------------------------------------------

def pyr_down_np(img):
    """S61 in numpy: reflect-101 padding, the 25-tap integer sum at the even pixels, (s + 128) >> 8."""
    k = np.array([1, 4, 6, 4, 1], np.int64)
    p = np.pad(img.astype(np.int64), 2, mode="reflect")
    h, w = img.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    s = np.zeros((oh, ow), np.int64)
    for j in range(5):
        for i in range(5):
            s += k[i] * k[j] * p[j:j + 2 * oh:2, i:i + 2 * ow:2]
    return ((s + 128) >> 8).astype(np.uint8)


def plan_np(w, h, max_level):
    dims = [(w, h)]
    while len(dims) <= max_level and (dims[-1][0] + 1) // 2 >= 16 and (dims[-1][1] + 1) // 2 >= 16:
        dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
    return dims


@pytest.mark.parametrize("shape,max_level,levels", [((330, 496), 7, 5), ((330, 496), 3, 4), ((330, 496), 0, 1), ((16, 16), 7, 1),
                                                    ((31, 17), 7, 1), ((18, 33), 7, 1), ((35, 64), 7, 2), ((64, 33), 7, 2)])
def test_pyramid_equals_numpy(shape, max_level, levels):
    """(h, w) = (18, 33) is the issue's 33 x 18: it stops at one level, because the next would be 17 x 9."""
    if shape == (330, 496):
        img = R.fixture()[0]
    else:
        img = np.random.default_rng(shape[0] * 100 + shape[1]).integers(0, 256, shape, dtype=np.uint8)
    p = R.Pyramid(img, max_level)
    dims = plan_np(shape[1], shape[0], max_level)
    assert p.n == len(dims) == levels
    want = img
    for l in range(p.n):
        assert p.levels[l].shape == (dims[l][1], dims[l][0])
        assert (p.levels[l] == want).all(), l
        want = pyr_down_np(want)
    # one reduction of every small shape, whether or not the plan keeps it: edge columns and rows, odd and even sizes
    assert (R.pyr_down(img) == pyr_down_np(img)).all()


# ---- S62 -------------------------------------------------------------------------------------------------------------------

def test_sampling_weights_sum_and_sample_range():
    """64 x 64 fractional offsets: the weights sum to 16384 and every S lies in [0, 8160], on the extreme images too."""
    rng = np.random.default_rng(5)
    imgs = [np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8), rng.integers(0, 256, (8, 8), dtype=np.uint8),
            (rng.integers(0, 2, (8, 8)) * 255).astype(np.uint8)]
    for fy in range(64):
        for fx_ in range(64):
            px, py = 2.0 + fx_ / 64.0, 1.0 + fy / 64.0
            ok, ix, iy, wt = R.window_origin(px, py, 3, 8, 8)
            assert ok == 1 and (ix, iy) == (2, 1)
            assert int(wt.sum()) == 16384 and (wt >= 0).all()
            a, b = fx_ / 64.0, fy / 64.0
            assert wt.tolist() == [round((1 - a) * (1 - b) * 16384), round(a * (1 - b) * 16384), round((1 - a) * b * 16384),
                                   16384 - round((1 - a) * (1 - b) * 16384) - round(a * (1 - b) * 16384) - round((1 - a) * b * 16384)]
            for im in imgs:
                s = R.sample_window(im, px, py, 3)
                assert s.min() >= 0 and s.max() <= 8160
                q = im.astype(np.int64)
                want = (q[1:4, 2:5] * wt[0] + q[1:4, 3:6] * wt[1] + q[2:5, 2:5] * wt[2] + q[2:5, 3:6] * wt[3] + 256) >> 9
                assert (s == want).all()
    assert (R.sample_window(imgs[1], 2.5, 1.5, 3) == 8160).all()


def test_window_leaves_the_level():
    img = np.zeros((20, 24), np.uint8)
    n = 5
    assert R.sample_window(img, 0.0, 0.0, n) is not None
    assert R.sample_window(img, 18.0, 14.0, n) is not None          # ix + n = 23 = w - 1, iy + n = 19 = h - 1
    assert R.sample_window(img, 18.999, 14.999, n) is not None
    for px, py in ((-0.001, 3.0), (3.0, -0.001), (19.0, 3.0), (3.0, 15.0), (float("nan"), 3.0), (3.0, float("inf")), (1e30, 3.0),
                   (3.0, -1e30), (1.0000001e6, 3.0)):
        assert R.sample_window(img, px, py, n) is None, (px, py)


# ---- S63 - S65 on the frames -------------------------------------------------------------------------------------------------

def test_identity_frame_is_exact(fx):
    """Prototype: exact.  Every point status 1, out == pt bit for bit, err 0."""
    for r in (3, 10, 15):
        out, st, err, fb = R.track(fx["p1"], fx["p1"], fx["kp"], R.params(r, 3))
        assert (st == 1).all() and (bits(out) == bits(fx["kp"])).all() and (err == 0).all() and (fb == -1).all()


@pytest.mark.parametrize("r", [3, 10, 15])
def test_frame_s_is_tracked_within_a_tenth_of_a_pixel(fx, r):
    """Prototype maxima: 0.037, 0.0009, 0.0010 px for r = 3, 10, 15; the bound 0.1 px is about 3 times the worst."""
    out, st, err, fb = R.track(fx["p1"], fx["pS"], fx["kp"], R.params(r, 3))
    e = np.hypot(*(out.astype(np.float64) - fx["kp"] - np.array(R.SHIFT, np.float64)).T)
    print("frame S, r %d: statuses %s, max error %.5f px" % (r, np.bincount(st).tolist(), e.max()))
    assert (st == 1).all()
    assert e.max() <= 0.1


def test_frame_r_is_tracked_within_half_a_pixel(fx):
    """Prototype: every point status 1, max error 0.169 px, median 0.05; the least-squares similarity through the tracks
    maps the four corners within 0.014 px of the true map.  Bounds: 0.5 px per point, 0.1 px at the corners."""
    out, st, err, fb = R.track(fx["p1"], fx["pR"], fx["kp"], R.params(10, 3))
    e = np.hypot(*(out.astype(np.float64) - fx["true_r"]).T)
    A = R.fit_similarity(fx["kp"], out)
    c = R.corners(fx["img"].shape)
    ce = np.hypot(*(c @ A[:, :2].T + A[:, 2] - R.frame_r_map(c, fx["img"].shape)).T)
    print("frame R: statuses %s, max error %.4f, median %.4f, corner error %.4f px" % (np.bincount(st).tolist(), e.max(), np.median(e), ce.max()))
    assert (st == 1).all()
    assert e.max() <= 0.5
    assert ce.max() <= 0.1


def test_statuses(fx):
    prm = R.params(10, 3)
    flat = R.Pyramid(np.full((330, 496), 93, np.uint8), 3)
    out, st, err, fb = R.track(flat, flat, fx["kp"][:8], prm)
    assert (st == 3).all() and (bits(out) == bits(fx["kp"][:8])).all() and (err == -1).all()
    pts = np.array([[5, 5], [np.nan, 100], [100, np.nan], [1e30, 100], [100, -1e30], [np.inf, 100]], np.float32)
    out, st, err, fb = R.track(fx["p1"], fx["p1"], pts, prm)
    assert (st == 2).all() and (err == -1).all()
    assert (bits(out[0]) == bits(pts[0])).all() and (bits(out[3:]) == bits(pts[3:])).all()
    assert bits(out[1])[0] == 0x7FC00000 and bits(out[2])[1] == 0x7FC00000      # S65: a NaN is stored as the quiet NaN
    # a search window that leaves level 0: the initial guess points outside
    prm_i = R.params(10, 0, flags=R.USE_INITIAL)
    p0 = R.Pyramid(fx["img"], 0)
    out, st, err, fb = R.track(p0, p0, fx["kp"][:1], prm_i, init=np.array([[490.0, 100.0]], np.float32))
    assert st[0] == 2 and out[0].tolist() == [490.0, 100.0]


def eig_np(img, kp, r):
    """Smaller eigenvalue per pixel of the level-0 normal matrix at integer points, independently: central differences of
    32 * I, numpy's symmetric eigenvalue solver."""
    I = img.astype(np.float64) * 32
    n = 2 * r + 1
    out = []
    for x, y in kp.astype(np.int64):
        gx = I[y - r:y + r + 1, x - r + 1:x + r + 2] - I[y - r:y + r + 1, x - r - 1:x + r]
        gy = I[y - r + 1:y + r + 2, x - r:x + r + 1] - I[y - r - 1:y + r, x - r:x + r + 1]
        G = np.array([[(gx * gx).sum(), (gx * gy).sum()], [(gx * gy).sum(), (gy * gy).sum()]]) / (n * n * 4096.0)
        out.append(np.linalg.eigvalsh(G)[0])
    return np.array(out)


def test_min_eig_splits_the_points_as_numpy_says(fx):
    """min_eig = 20 grey-level^2: both classes occur (prototype), and the split is the independent eigenvalue's."""
    assert (fx["kp"] == np.rint(fx["kp"])).all()
    e = eig_np(fx["img"], fx["kp"], 10)
    print("eigenvalues: min %.3f, median %.3f, max %.3f; below 20: %d" % (e.min(), np.median(e), e.max(), (e < 20).sum()))
    assert np.abs(e - 20).min() > 1e-6
    out, st, err, fb = R.track(fx["p1"], fx["p1"], fx["kp"], R.params(10, 3, min_eig=20.0))
    assert (e < 20).any() and (e >= 20).any()
    assert (st == np.where(e >= 20, 1, 3)).all()
    code, T, gx, gy, G = R.template(fx["img"], float(fx["kp"][0, 0]), float(fx["kp"][0, 1]), 10, 1e-4)
    assert code == 0 and abs(G[4] - e[0]) <= 1e-9 * e[0]


# ---- S66 -------------------------------------------------------------------------------------------------------------------

def test_forward_backward(fx):
    """Prototype: with fb_thresh = 0.5 every point of frame R keeps status 1.  With 1e-3 the statuses are those the rule
    gives on the backward tracks, restated here in numpy from single-direction calls."""
    kp = fx["kp"]
    out, st, err, fb = R.track(fx["p1"], fx["pR"], kp, R.params(10, 3, fb_thresh=0.5))
    print("frame R, fb 0.5: statuses %s, max fb %.4f" % (np.bincount(st).tolist(), fb.max()))
    assert (st == 1).all() and (fb >= 0).all() and (fb <= 0.5).all()
    out_f = R.track(fx["p1"], fx["pR"], kp, R.params(10, 3))[0]
    assert (bits(out) == bits(out_f)).all()                      # the check changes statuses only
    thr = np.float32(1e-3)
    out, st, err, fb = R.track(fx["p1"], fx["pR"], kp, R.params(10, 3, fb_thresh=float(thr)))
    prm = R.params(10, 3)
    want_st, want_fb = [], []
    for i in range(kp.shape[0]):
        bs, back, _ = R.track_point(fx["pR"], fx["p1"], out_f[i], prm)
        ex, ey = back[0] - kp[i, 0], back[1] - kp[i, 1]                 # fp32
        keep = bs == 1 and float(ex) * float(ex) + float(ey) * float(ey) <= float(thr) * float(thr)
        want_st.append(1 if keep else 4)
        want_fb.append(np.sqrt(ex * ex + ey * ey, dtype=np.float32))
        assert R.fb_check(kp[i], back, bs, float(thr)) == (want_st[-1], float(want_fb[-1]))
    assert (st == np.array(want_st)).all() and (bits(fb) == bits(np.array(want_fb))).all()
    assert (st == 1).any() and (st == 4).any()


def test_wide_baseline_pair_runs(fx):
    """The real second image is a wide-baseline view: nothing usable is tracked; it only has to run and be repeatable."""
    p2 = R.Pyramid(R.second_image(), 3)
    a = R.track(fx["p1"], p2, fx["kp"], R.params(10, 3, fb_thresh=0.5))
    b = R.track(fx["p1"], p2, fx["kp"], R.params(10, 3, fb_thresh=0.5))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert set(np.unique(a[1]).tolist()) <= {1, 2, 3, 4}
