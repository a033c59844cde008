"""GPU: minimum-eigenvalue corners (pm_corners*, SPEC S67-S70) against the plain-C restatement tests/corner_ref.c, which
tests/test_corners_cpu.py pins on the CPU.  Every comparison is bit for bit and there is no tolerance anywhere: S67 makes the
sums exact integers, S69 makes the keys distinct and S70 defines the result by the serial loop.  With min_dist = 0,
quality = 0 and room for every candidate the output IS the ranked candidate list, so the detector needs no inspection entry
point."""
import gc

import numpy as np
import pytest

import corner_ref as K
import lk_ref as R
from points_matching_amd import api

pytestmark = pytest.mark.gpu
PATTERN_F = -7.5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import torch
    import points_matching_amd as pm
    c = pm.Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()
    gc.collect()


class Frames:
    """Images by name and their device pyramids, each built once."""

    def __init__(self, ctx):
        self.ctx = ctx
        img = R.fixture()[0]
        self.img = {"1": img, "S": R.frame_s(img), "R": R.frame_r(img), "block": K.block_pattern(), "pair": K.two_pixel_plateau(),
                    "flat": K.constant_image()}
        for w, h in ((67, 35), (130, 37), (64, 48), (16, 16)):
            self.img["%dx%d" % (w, h)] = K.random_image(w, h)
        self._dev, self._ref = {}, {}

    def dev(self, name, max_level=0):
        import torch
        if (name, max_level) not in self._dev:
            d_img = torch.from_numpy(self.img[name]).to("cuda:0")
            torch.cuda.synchronize()
            h, w = self.img[name].shape
            p = self.ctx.pyramid(w, h, max_level).build_dev(d_img.data_ptr())
            self.ctx.synchronize()
            self._dev[(name, max_level)] = p
        return self._dev[(name, max_level)]

    def ref(self, name, r, min_eig=1e-4, quality=0.0, min_dist=0.0, keep=None, max_corners=1 << 20):
        """The restatement's (xy, score, candidates), computed once per argument set."""
        key = (name, r, min_eig, quality, min_dist, None if keep is None else keep.tobytes(), max_corners)
        if key not in self._ref:
            self._ref[key] = K.detect(self.img[name], r, min_eig, quality, min_dist, keep, max_corners)
        return self._ref[key]

    def close(self):
        for p in self._dev.values():
            p.close()


@pytest.fixture(scope="module")
def fr(ctx):
    f = Frames(ctx)
    yield f
    ctx.synchronize()
    f.close()


def dev_corners(ctx, pyr, prm, max_corners, keep=None, n_keep=None, cap_keep=None, score=True):
    """pm_corners_dev on torch buffers pre-filled with a pattern -> (n, xy (max_corners, 2), score (max_corners,)).
    n_keep: None = no count pointer, else the value of the device count."""
    import torch
    dev = torch.device("cuda", 0)
    d_xy = torch.full((max_corners, 2), PATTERN_F, dtype=torch.float32, device=dev)
    d_sc = torch.full((max_corners,), PATTERN_F, dtype=torch.float32, device=dev)
    d_n = torch.full((1,), -9, dtype=torch.int32, device=dev)
    d_keep = torch.from_numpy(K.keep_array(keep)).to(dev) if keep is not None else None
    cap_keep = (0 if keep is None else K.keep_array(keep).shape[0]) if cap_keep is None else cap_keep
    d_nk = torch.tensor([n_keep], dtype=torch.int32, device=dev) if n_keep is not None else None
    torch.cuda.synchronize()
    ctx.corners_dev(pyr, prm, max_corners, d_xy.data_ptr(), d_n.data_ptr(), d_sc.data_ptr() if score else None,
                    d_keep.data_ptr() if d_keep is not None else None, d_nk.data_ptr() if d_nk is not None else None, cap_keep)
    ctx.synchronize()
    return int(d_n.item()), d_xy.cpu().numpy(), d_sc.cpu().numpy()


def assert_rows(tag, got, want):
    """got: (n, xy, score) of dev_corners; want: (xy, score, ...) of the restatement.  Rows behind n must hold the pattern."""
    n, xy, sc = got
    m = want[0].shape[0]
    same = n == m and (bits(xy[:m]) == bits(want[0])).all() and (bits(sc[:m]) == bits(want[1])).all()
    first = -1
    if n == m and not same:
        first = int(np.flatnonzero((bits(xy[:m]) != bits(want[0])).any(axis=1) | (bits(sc[:m]) != bits(want[1])))[0])
    print("%s: device %d rows, restatement %d, first differing row %d" % (tag, n, m, first))
    assert same, tag
    assert (xy[max(n, 0):] == PATTERN_F).all() and (sc[max(n, 0):] == PATTERN_F).all(), tag


# ---- S67 - S69: the whole ranked candidate list --------------------------------------------------------------------------------

@pytest.mark.parametrize("r,min_eig", [(1, 1.0), (10, 1.0), (15, 1.0), (1, 1e-4)])
def test_candidate_list_of_the_fixture(ctx, fr, r, min_eig):
    """(1, 1e-4): 8921 candidates, thousands of equal fp32 scores, so the position half of the key decides the order."""
    want = fr.ref("1", r, min_eig)
    assert want[0].shape[0] == want[2] > 500
    got = dev_corners(ctx, fr.dev("1"), api.corner_params(r, min_eig, 0.0, 0.0), 16384)
    assert_rows("fixture r %d min_eig %g" % (r, min_eig), got, want)


@pytest.mark.parametrize("name", ["67x35", "130x37", "64x48", "block", "pair", "flat"])
def test_small_shapes_and_plateaus(ctx, fr, name):
    """Sizes that are no multiple of the 64 x 16 tile, V narrower and lower than a tile (r = 15 leaves 2 rows of the 35), and
    the plateau images of the CPU file."""
    h, w = fr.img[name].shape
    for r in (1, 2, 4, 15):
        if w - 2 * r - 3 < 1 or h - 2 * r - 3 < 1:
            continue
        want = fr.ref(name, r, 0.0)
        got = dev_corners(ctx, fr.dev(name), api.corner_params(r, 0.0, 0.0, 0.0), 4096)
        assert_rows("%s r %d" % (name, r), got, want)
    assert name != "flat" or fr.ref(name, 2, 0.0)[2] == 0
    assert name != "pair" or fr.ref(name, 2, 0.0)[2] >= 1


def test_single_pixel_and_empty_valid_region(ctx, fr):
    want = fr.ref("16x16", 6, 0.0)
    assert want[2] == 1 and want[0].tolist() == [[7.0, 7.0]]
    assert_rows("16x16 r 6", dev_corners(ctx, fr.dev("16x16"), api.corner_params(6, 0.0, 0.0, 0.0), 8), want)
    got = dev_corners(ctx, fr.dev("16x16"), api.corner_params(7, 0.0, 0.0, 0.0), 8)
    assert got[0] == 0 and (got[1] == PATTERN_F).all()
    xy, sc = ctx.corners(fr.img["16x16"], 8, api.corner_params(7, 0.0, 0.0, 0.0))
    assert xy.shape == (0, 2)


def test_host_form_with_a_row_stride(ctx, fr):
    img = fr.img["130x37"]
    h, w = img.shape
    buf = np.random.default_rng(3).integers(0, 256, (h, w + 7), dtype=np.uint8)
    buf[:, :w] = img
    want = fr.ref("130x37", 3, 0.0, 0.0, 4.0, None, 100)
    xy, sc = ctx.corners(buf, 100, api.corner_params(3, 0.0, 0.0, 4.0), w=w)
    assert xy.shape == want[0].shape and (bits(xy) == bits(want[0])).all() and (bits(sc) == bits(want[1])).all()


# ---- S69 quality, S70 ------------------------------------------------------------------------------------------------------------

def keep_points(shape, n=40):
    h, w = shape
    rng = np.random.default_rng(11)
    keep = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1).astype(np.float32)
    keep[3] = (np.nan, 100.0)
    return keep


@pytest.mark.parametrize("min_dist,max_corners", [(5.0, 500), (10.0, 50)])
@pytest.mark.parametrize("r,min_eig", [(10, 1.0), (1, 1e-4)])
def test_selection(ctx, fr, min_dist, max_corners, r, min_eig):
    """(1, 1e-4) walks several chunks of the selection kernel; (10, 1.0) ends inside the first two."""
    keep = keep_points(fr.img["1"].shape)
    for kp in (None, keep):
        want = fr.ref("1", r, min_eig, 0.0, min_dist, kp, max_corners)
        got = dev_corners(ctx, fr.dev("1"), api.corner_params(r, min_eig, 0.0, min_dist), max_corners, kp)
        assert_rows("r %d min_dist %g max %d keep %s" % (r, min_dist, max_corners, kp is not None), got, want)
        assert kp is None or not (bits(want[0]) == bits(fr.ref("1", r, min_eig, 0.0, min_dist, None, max_corners)[0][:want[0].shape[0]])).all()


def test_keep_counts(ctx, fr):
    """A device keep count of -1 (none), below, at and above cap_keep (clamped); no count pointer (= cap_keep); no score pointer."""
    keep = keep_points(fr.img["1"].shape)
    prm = api.corner_params(10, 1.0, 0.0, 8.0)
    for n_keep, used in ((-1, 0), (0, 0), (17, 17), (40, 40), (47, 40), (None, 40)):
        want = fr.ref("1", 10, 1.0, 0.0, 8.0, keep[:used] if used else None, 300)
        got = dev_corners(ctx, fr.dev("1"), prm, 300, keep, n_keep)
        assert_rows("keep count %s" % n_keep, got, want)
    got = dev_corners(ctx, fr.dev("1"), prm, 300, keep, None, score=False)
    assert got[0] == want[0].shape[0] and (bits(got[1][:got[0]]) == bits(want[0])).all() and (got[2] == PATTERN_F).all()


@pytest.mark.parametrize("quality", [0.05, 1.0])
def test_quality(ctx, fr, quality):
    for min_dist in (0.0, 6.0):
        want = fr.ref("1", 10, 1.0, quality, min_dist, None, 1000)
        got = dev_corners(ctx, fr.dev("1"), api.corner_params(10, 1.0, quality, min_dist), 1000)
        assert_rows("quality %g min_dist %g" % (quality, min_dist), got, want)
        assert 1 <= want[0].shape[0] < want[2]


# ---- overflow --------------------------------------------------------------------------------------------------------------------

def test_overflow(ctx, fr):
    got = dev_corners(ctx, fr.dev("1"), api.corner_params(10, 1.0, 0.0, 8.0, capacity=16), 100)
    assert got[0] == -1 and (got[1] == PATTERN_F).all() and (got[2] == PATTERN_F).all()
    want = fr.ref("1", 10, 1.0, 0.0, 8.0, None, 100)
    xy, sc = ctx.corners(fr.img["1"], 100, api.corner_params(10, 1.0, 0.0, 8.0, capacity=16))
    assert xy.shape == want[0].shape and (bits(xy) == bits(want[0])).all() and (bits(sc) == bits(want[1])).all()


# ---- replenish -------------------------------------------------------------------------------------------------------------------

def dev_replenish(ctx, pyr, prm, pts, count, cap, target, score=True, n_new=True):
    import torch
    dev = torch.device("cuda", 0)
    buf = np.full((cap, 2), PATTERN_F, np.float32)
    buf[:pts.shape[0]] = pts
    d_pts = torch.from_numpy(buf).to(dev)
    d_cnt = torch.tensor([count], dtype=torch.int32, device=dev)
    d_sc = torch.full((cap,), PATTERN_F, dtype=torch.float32, device=dev)
    d_new = torch.full((1,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.corners_replenish_dev(pyr, prm, d_pts.data_ptr(), d_cnt.data_ptr(), cap, target, d_sc.data_ptr() if score else None,
                              d_new.data_ptr() if n_new else None)
    ctx.synchronize()
    return int(d_cnt.item()), int(d_new.item()), d_pts.cpu().numpy(), d_sc.cpu().numpy()


def test_replenish(ctx, fr):
    img = fr.img["1"]
    keep = keep_points(img.shape, 60)
    prm = api.corner_params(10, 1.0, 0.0, 8.0)
    # (count, cap, target): room to the target; bounded by cap; target below, at and above the count; counts to clamp
    for count, cap, target in ((60, 256, 200), (60, 100, 200), (60, 256, 60), (60, 256, 30), (60, 256, 61), (0, 64, 64), (-3, 64, 10),
                               (60, 60, 200), (90, 60, 200)):
        n = min(max(count, 0), cap)
        pts = keep[:n]                                               # (a count above cap: cap rows are the obstacles)
        room = max(min(target, cap) - n, 0)
        want = fr.ref("1", 10, 1.0, 0.0, 8.0, pts if n else None, room) if room else (np.zeros((0, 2), np.float32), np.zeros(0, np.float32))
        cnt, new, out, sc = dev_replenish(ctx, fr.dev("1"), prm, pts, count, cap, target)
        m = want[0].shape[0]
        print("replenish count %d cap %d target %d: %d new (restatement %d)" % (count, cap, target, new, m))
        assert new == m and cnt == n + m
        assert (bits(out[:n]) == bits(pts[:n])).all() and (bits(out[n:n + m]) == bits(want[0])).all() and (out[n + m:] == PATTERN_F).all()
        assert (sc[:n] == PATTERN_F).all() and (bits(sc[n:n + m]) == bits(want[1])).all() and (sc[n + m:] == PATTERN_F).all()
        if room and n:                                               # the same rows as pm_corners_dev with the same obstacles
            dn, dxy, dsc = dev_corners(ctx, fr.dev("1"), prm, room, pts[:n])
            assert dn == m and (bits(dxy[:m]) == bits(out[n:n + m])).all() and (bits(dsc[:m]) == bits(sc[n:n + m])).all()
    cnt, new, out, sc = dev_replenish(ctx, fr.dev("1"), prm, keep, 60, 256, 200, score=False, n_new=False)
    assert cnt == 60 + fr.ref("1", 10, 1.0, 0.0, 8.0, keep, 140)[0].shape[0] and new == -9 and (sc == PATTERN_F).all()
    # overflow: the count stays, no rows
    cnt, new, out, sc = dev_replenish(ctx, fr.dev("1"), api.corner_params(10, 1.0, 0.0, 8.0, capacity=16), keep, 60, 256, 200)
    assert cnt == 60 and new == -1 and (out[60:] == PATTERN_F).all() and (bits(out[:60]) == bits(keep)).all() and (sc == PATTERN_F).all()


# ---- the video chain ---------------------------------------------------------------------------------------------------------------

def test_video_chain_on_one_stream(fr):
    """pm_corners_dev (200, r 10, min_dist 8) -> pm_track_lk_gather_dev into frame S -> a device copy of the count ->
    pm_corners_replenish_dev on frame S's pyramid up to 200 -> pm_ransac_affine_run_dev on the tracked pairs; everything on one
    stream, one synchronisation at the end."""
    import torch
    import points_matching_amd as pm
    dev = torch.device("cuda", 0)
    img1, img2 = fr.img["1"], fr.img["S"]
    h, w = img1.shape
    CAP = 200
    st = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(st)
    c = pm.Context(0)
    c.set_stream(st.cuda_stream)
    p1 = p2 = None
    try:
        d_img1, d_img2 = torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev)
        d_kp = torch.zeros((CAP, 2), dtype=torch.float32, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        d_xy1 = torch.full((CAP, 2), PATTERN_F, dtype=torch.float32, device=dev)
        d_xy2 = torch.full((CAP, 2), PATTERN_F, dtype=torch.float32, device=dev)
        d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        d_total = torch.zeros(1, dtype=torch.int32, device=dev)
        d_new = torch.zeros(1, dtype=torch.int32, device=dev)
        d_key = torch.zeros(1, dtype=torch.int64, device=dev)
        d_A = torch.zeros(6, dtype=torch.float64, device=dev)
        d_mask = torch.zeros(CAP, dtype=torch.uint8, device=dev)
        d_ninl = torch.zeros(1, dtype=torch.int32, device=dev)
        p1, p2 = c.pyramid(w, h, 3), c.pyramid(w, h, 3)
        cprm = api.corner_params(10, 1e-4, 0.01, 8.0)
        lk = api.lk_params(10, 3, fb_thresh=0.5)
        torch.cuda.synchronize()
        p1.build_dev(d_img1.data_ptr())
        p2.build_dev(d_img2.data_ptr())
        c.corners_dev(p1, cprm, CAP, d_kp.data_ptr(), d_n.data_ptr())
        c.track_lk_gather_dev(p1, p2, d_kp.data_ptr(), d_n.data_ptr(), CAP, lk, d_xy1.data_ptr(), d_xy2.data_ptr(), d_cnt.data_ptr())
        d_total.copy_(d_cnt)                                          # on the same stream: the estimator keeps the tracked count
        c.corners_replenish_dev(p2, cprm, d_xy2.data_ptr(), d_total.data_ptr(), CAP, CAP, None, d_new.data_ptr())
        view = api.PointsView(d_xy1.data_ptr(), d_xy2.data_ptr(), d_cnt.data_ptr(), 1, CAP, 0, 1, 0)
        c.ransac_affine_run_dev(view, 0, 500, 2.0, 0x5EED, d_key.data_ptr(), d_A.data_ptr(), d_mask.data_ptr(), CAP, d_ninl.data_ptr(),
                                model=api.PM_AFFINE_PARTIAL)
        c.synchronize()
        n_kp, cnt, total, new, ninl = int(d_n.item()), int(d_cnt.item()), int(d_total.item()), int(d_new.item()), int(d_ninl.item())
        kp, xy1, xy2 = d_kp.cpu().numpy(), d_xy1.cpu().numpy(), d_xy2.cpu().numpy()
        A = d_A.cpu().numpy().reshape(2, 3)
        want_kp = K.detect(img1, 10, 1e-4, 0.01, 8.0, None, CAP)[0]
        assert n_kp == want_kp.shape[0] == CAP and (bits(kp) == bits(want_kp)).all()
        out, status, _, _ = R.track(R.Pyramid(img1, 3), R.Pyramid(img2, 3), kp, R.params(10, 3, fb_thresh=0.5))
        keep = status == 1
        assert cnt == keep.sum() and (bits(xy1[:cnt]) == bits(kp[keep])).all() and (bits(xy2[:cnt]) == bits(out[keep])).all()
        want = K.detect(img2, 10, 1e-4, 0.01, 8.0, xy2[:cnt], CAP - cnt)
        m = want[0].shape[0]
        good = int((np.hypot(*(xy2[:cnt].astype(np.float64) - xy1[:cnt] - np.array(R.SHIFT, np.float64)).T) <= 0.5).sum())
        print("chain: %d corners, %d tracked (%d within 0.5 px of the shift), %d new (restatement %d), total %d, %d inliers" %
              (n_kp, cnt, good, new, m, total, ninl))
        assert 0 < cnt < CAP, "the premise fails: frame S must lose some corners and keep some"
        assert new == m and total == cnt + m <= CAP                   # the count is the restatement's, 200 at the most
        assert (bits(xy2[cnt:total]) == bits(want[0])).all() and (xy2[total:] == PATTERN_F).all()
        assert good >= 0.9 * cnt, "the premise fails on the restatement's own tracks"
        assert ninl >= 0.95 * good and np.isfinite(A).all()
        assert np.abs(A[:, :2] - np.eye(2)).max() <= 0.01 and np.abs(A[:, 2] - np.array(R.SHIFT)).max() <= 0.5
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        for p in (p1, p2):
            if p is not None:
                p.close()
        c.close()
        gc.collect()


# ---- the tracker's contract ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r,m", [(3, 1.0), (10, 1.0), (10, 20.0), (15, 5.0)])
def test_corners_are_never_flat_for_the_tracker(ctx, fr, r, m):
    """Corners found at radius r with min_eig m, tracked with win_radius r and min_eig m (no forward-backward check): none
    has status 3, at one level and at four."""
    import torch
    dev = torch.device("cuda", 0)
    n, xy, _ = dev_corners(ctx, fr.dev("1"), api.corner_params(r, m, 0.0, 3.0), 2000)
    assert n > 50
    d_pts = torch.from_numpy(xy[:n].copy()).to(dev)
    for max_level in (0, 3):
        d_out = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.track_lk_dev(fr.dev("1", max_level), fr.dev("R", max_level), d_pts.data_ptr(), None, n, api.lk_params(r, max_level, min_eig=m),
                         d_out.data_ptr(), d_st.data_ptr())
        ctx.synchronize()
        st = d_st.cpu().numpy()
        print("r %d min_eig %g max_level %d: %d corners, statuses %s" % (r, m, max_level, n, np.bincount(st, minlength=5).tolist()))
        assert (st != 3).all() and (st == 1).sum() > 0


# ---- determinism, the host form, arguments, capture ------------------------------------------------------------------------------------

def test_two_runs_give_identical_bytes(ctx, fr):
    keep = keep_points(fr.img["1"].shape)
    for prm, rows in ((api.corner_params(1, 1e-4, 0.0, 0.0), 16384), (api.corner_params(10, 1.0, 0.0, 6.0), 400)):
        a = dev_corners(ctx, fr.dev("1"), prm, rows, keep)
        b = dev_corners(ctx, fr.dev("1"), prm, rows, keep)
        assert a[0] == b[0] > 0 and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_host_form_equals_the_device_form(ctx, fr):
    keep = keep_points(fr.img["1"].shape)
    prm = api.corner_params(10, 1.0, 0.05, 6.0)
    n, xy, sc = dev_corners(ctx, fr.dev("1"), prm, 400, keep)
    hxy, hsc = ctx.corners(fr.img["1"], 400, prm, keep)
    assert hxy.shape[0] == n > 0 and hxy.tobytes() == xy[:n].tobytes() and hsc.tobytes() == sc[:n].tobytes()


def test_argument_statuses(ctx, fr):
    import torch
    dev = torch.device("cuda", 0)
    pyr = fr.dev("1")
    d_xy = torch.zeros((8, 2), dtype=torch.float32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def call(prm=None, max_corners=8, xy=d_xy.data_ptr(), n=d_n.data_ptr(), keep=None, cap_keep=0):
        ctx.corners_dev(pyr, prm or api.corner_params(), max_corners, xy, n, None, keep, None, cap_keep)

    def rep(prm=None, pts=d_xy.data_ptr(), count=d_n.data_ptr(), cap=8, target=8):
        ctx.corners_replenish_dev(pyr, prm or api.corner_params(), pts, count, cap, target)

    nan, inf = float("nan"), float("inf")
    bad = [api.corner_params(block_radius=0), api.corner_params(block_radius=16), api.corner_params(min_eig=-1.0), api.corner_params(min_eig=nan),
           api.corner_params(min_eig=inf), api.corner_params(quality=-0.1), api.corner_params(quality=1.5), api.corner_params(quality=nan),
           api.corner_params(min_dist=-1.0), api.corner_params(min_dist=2e6), api.corner_params(min_dist=nan), api.corner_params(min_dist=inf),
           api.corner_params(capacity=-1), api.corner_params(capacity=(1 << 24) + 1)]
    flags, res = api.corner_params(), api.corner_params()
    flags.flags = 1
    res.reserved[1] = 1
    for prm in bad + [flags, res]:
        for f in (call, rep):
            with pytest.raises(api.PmError) as e:
                f(prm)
            assert e.value.status == api.PM_E_INVALID
    for f, kw in ((call, dict(xy=None)), (call, dict(n=None)), (call, dict(max_corners=-1)), (call, dict(cap_keep=4)), (call, dict(cap_keep=-1)),
                  (rep, dict(pts=None)), (rep, dict(count=None)), (rep, dict(cap=-1)), (rep, dict(target=-1))):
        with pytest.raises(api.PmError) as e:
            f(**kw)
        assert e.value.status == api.PM_E_INVALID, kw
    for f, kw in ((call, dict(max_corners=0)), (rep, dict(cap=0))):
        with pytest.raises(api.PmError) as e:
            f(**kw)
        assert e.value.status == api.PM_E_UNSUPPORTED, kw
    for kw in (dict(max_corners=-1), dict(max_corners=0), dict(prm=bad[0])):
        with pytest.raises(api.PmError) as e:
            ctx.corners(fr.img["1"], **kw)
        assert e.value.status == (api.PM_E_UNSUPPORTED if kw.get("max_corners") == 0 else api.PM_E_INVALID), kw
    d_n.fill_(0)
    torch.cuda.synchronize()
    call()
    rep(target=0)
    ctx.synchronize()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capturing_stream_is_refused(fr):
    """Refused first thing with PM_E_UNSUPPORTED: nothing is launched, and the context keeps working afterwards."""
    import torch
    import points_matching_amd as pm
    dev = torch.device("cuda", 0)
    img = fr.img["1"]
    h, w = img.shape
    st = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(st)
    c = pm.Context(0)
    c.set_stream(st.cuda_stream)
    pyr = None
    bufs = None
    try:
        d_img = torch.from_numpy(img).to(dev)
        d_xy = torch.full((100, 2), PATTERN_F, dtype=torch.float32, device=dev)
        d_n = torch.full((1,), -5, dtype=torch.int32, device=dev)
        d_cnt = torch.full((1,), 0, dtype=torch.int32, device=dev)
        bufs = (d_img, d_xy, d_n, d_cnt)
        torch.cuda.synchronize()
        pyr = c.pyramid(w, h, 0).build_dev(d_img.data_ptr())
        torch.cuda.synchronize()
        prm = api.corner_params(10, 1.0, 0.0, 8.0)
        calls = [lambda: c.corners_dev(pyr, prm, 100, d_xy.data_ptr(), d_n.data_ptr()),
                 lambda: c.corners_replenish_dev(pyr, prm, d_xy.data_ptr(), d_cnt.data_ptr(), 100, 100, None, d_n.data_ptr()),
                 lambda: c.corners(img, 100, prm)]
        gc.collect()
        for call in calls:
            g = torch.cuda.CUDAGraph()
            with pytest.raises(pm.PmError) as err:
                with torch.cuda.graph(g, stream=st, capture_error_mode="relaxed"):
                    call()
            assert err.value.status == api.PM_E_UNSUPPORTED and "capturing" in str(err.value)
            del g, err
            torch.cuda.set_stream(st)
            torch.cuda.synchronize()
        assert (d_xy == PATTERN_F).all() and int(d_n.item()) == -5 and int(d_cnt.item()) == 0
        calls[0]()
        torch.cuda.synchronize()
        want = fr.ref("1", 10, 1.0, 0.0, 8.0, None, 100)
        assert int(d_n.item()) == 100 and (bits(d_xy.cpu().numpy()) == bits(want[0])).all()
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        if pyr is not None:
            pyr.close()
        c.close()
        del bufs
        gc.collect()
