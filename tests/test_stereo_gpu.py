"""GPU: pm_stereo_bm[_dev], pm_stereo_lr_check_dev, pm_stereo_points[_dev] and pm_stereo_rectify (SPEC S84-S87) against the
plain-C restatement tests/stereo_ref.c, which tests/test_stereo_cpu.py pins on the CPU.  Disparities and counts are integers that
are a function of the inputs alone and the points are sequences of single fp64 operations: every comparison is bit for bit.
The block-matching kernel's tile is 64 columns x 4 rows per workgroup (one 64-pixel row segment per wave, a lane per
disparity, 64 disparities per register group): shapes are that tile exactly, one past it in each direction and images that hold
one computed pixel or none; disparity counts go around 64, 128 and up to 256."""
import gc

import numpy as np
import pytest

import stereo_ref as S
from points_matching_amd import api

pytestmark = pytest.mark.gpu
GUARD8, GUARD16 = 0xA5, 0x5A5A
INV = S.INVALID


@pytest.fixture(scope="module")
def ctx():
    import torch
    import points_matching_amd as pm
    c = pm.Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()
    gc.collect()


def _padded(img, stride, offset, fill):
    """img (h, w) as a flat buffer: offset bytes, rows of `stride`, 64 bytes behind; and the (h, stride) view of its rows."""
    h, w = img.shape
    buf = np.full(offset + h * stride + 64, fill, img.dtype)
    rows = buf[offset:offset + h * stride].reshape(h, stride)
    rows[:, :w] = img
    return buf, rows


def dev_bm(ctx, left, right, dmin, D, r, uniq=0, flags=0, lstride=None, rstride=None, dstride=None, loff=0, roff=0, doff=0, want_info=True):
    """pm_stereo_bm_dev on guarded torch buffers -> (whole disp buffer, status, n_valid) and the same three from the C
    restatement written into an equally guarded host buffer; also the (h, w) map."""
    import torch
    dev = torch.device("cuda", 0)
    h, w = left.shape
    lstride, rstride, dstride = lstride or w, rstride or w, dstride or w
    lbuf, lrows = _padded(left, lstride, loff, 201)
    rbuf, rrows = _padded(right, rstride, roff, 37)
    want = np.full(doff + h * dstride + 64, GUARD16, np.int16)
    _, n = S.bm(lrows, rrows, dmin, D, r, uniq, flags, w=w, disp=want[doff:doff + h * dstride].reshape(h, dstride), dstride=dstride)
    d_l, d_r = torch.from_numpy(lbuf).to(dev), torch.from_numpy(rbuf).to(dev)
    d_d = torch.full((want.size,), GUARD16, dtype=torch.int16, device=dev)
    d_info = torch.full((2,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.stereo_bm_dev(d_l.data_ptr() + loff, d_r.data_ptr() + roff, w, h, lstride, rstride, api.stereo_params(D, r, dmin, uniq, flags),
                      d_d.data_ptr() + 2 * doff, dstride, d_info.data_ptr() if want_info else None)
    ctx.synchronize()
    info = d_info.cpu().numpy()
    return (d_d.cpu().numpy(), int(info[0]), int(info[1])), (want, 0, n), want[doff:doff + h * dstride].reshape(h, dstride)[:, :w]


def check(ctx, left, right, dmin, D, r, uniq=0, flags=0, **kw):
    got, want, disp = dev_bm(ctx, left, right, dmin, D, r, uniq, flags, **kw)
    bad = int((got[0] != want[0]).sum())
    assert bad == 0, ("disp", left.shape, dmin, D, r, uniq, flags, kw, bad)
    assert got[1:] == want[1:], (left.shape, dmin, D, r, uniq, flags, got[1:], want[1:])
    return disp, want[2]


# ---- 1. shapes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, S.FROM_RIGHT])
def test_one_computed_pixel_and_none(ctx, flags):
    for r, dmin, D in ((1, 0, 1), (2, 0, 5), (3, -2, 4), (2, 3, 6), (10, 0, 3)):
        dmax = dmin + D - 1
        w1 = 2 * r + 1 + max(dmax, 0) - min(dmin, 0)                 # exactly one computed column
        h1 = 2 * r + 1
        for w, h, n in ((w1, h1, 1), (w1 - 1, h1, 0), (w1, h1 - 1, 0), (1, 1, 0)):
            if w < 1 or h < 1:
                continue
            left, right = S.random_pair(w, h, seed=r)
            disp, n_valid = check(ctx, left, right, dmin, D, r, 0, flags)
            assert n_valid == n and int((disp != INV).sum()) == n


@pytest.mark.parametrize("flags", [0, S.FROM_RIGHT])
@pytest.mark.parametrize("w,h", [(64, 4), (65, 5), (64, 5), (65, 4), (63, 3), (129, 9)])
def test_tile_and_one_past_it(ctx, w, h, flags):
    """Images of the 64 x 4 tile and one past it, radius 1 so that every tile holds computed pixels; then computed ranges that
    are the tile and one past it (the image larger by the margins)."""
    left, right = S.random_pair(w, h)
    for dmin, D in ((0, 1), (0, 4), (-2, 5)):
        check(ctx, left, right, dmin, D, 1, 10, flags)
    r, dmin, D = 2, 0, 6
    left, right = S.random_pair(w + 2 * r + D - 1, h + 2 * r, seed=1)          # computed pixels: w x h
    disp, n = check(ctx, left, right, dmin, D, r, 0, flags)
    assert n == w * h


@pytest.mark.parametrize("flags", [0, S.FROM_RIGHT])
def test_odd_strides_and_base_addresses(ctx, flags):
    left, right = S.random_pair(71, 13)
    for k, (ls, rs, ds, lo, ro, do) in enumerate(((71, 71, 71, 0, 0, 0), (73, 79, 75, 1, 3, 1), (77, 71, 83, 3, 2, 3), (72, 75, 71, 2, 1, 2))):
        got, want, disp = dev_bm(ctx, left, right, -3, 9, 2, 10, flags, lstride=ls, rstride=rs, dstride=ds, loff=lo, roff=ro, doff=do)
        assert (got[0] == want[0]).all() and got[1:] == want[1:], k
        assert (want[0][:do] == GUARD16).all() and (want[0][-64:] == GUARD16).all() and 0 < want[2] < 71 * 13
    got, want, _ = dev_bm(ctx, left, right, -3, 9, 2, 10, flags, want_info=False)
    assert (got[0] == want[0]).all() and got[1:] == (-9, -9)


# ---- 2. parameters ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, S.FROM_RIGHT])
@pytest.mark.parametrize("r", [1, 2, 10])
def test_radius_min_disp_uniqueness(ctx, r, flags):
    left, right, _ = S.scene(1, True)
    left, right = left[:2 * r + 8], right[:2 * r + 8]                # a few computed rows are enough: more than one tile row
    for dmin in (-7, 0, 5):
        for uniq in (0, 15, 99):
            disp, n = check(ctx, left, right, dmin, 12, r, uniq, flags)
            assert n > 0 or uniq == 99


@pytest.mark.parametrize("flags", [0, S.FROM_RIGHT])
@pytest.mark.parametrize("D", [1, 2, 3, 63, 64, 65, 127, 128, 129, 192, 193])
def test_disparity_counts_around_the_register_groups(ctx, D, flags):
    w = D + 70                                                       # 68 computed columns: two tiles
    rng = np.random.default_rng(D)
    base = rng.integers(0, 256, (9, w + 300)).astype(np.uint8)
    shift = max(D - 2, 0)                                            # the true disparity sits near the top of the range
    left, right = base[:, :w], base[:, shift:w + shift]              # right(x - shift) = left(x)
    for dmin, uniq in ((0, 0), (-7, 15), (5, 15)):
        disp, n = check(ctx, left, right, dmin, D, 2, uniq, flags)
    assert n > 0


@pytest.mark.parametrize("uniq", [0, 15])
@pytest.mark.parametrize("flags", [0, S.FROM_RIGHT])
@pytest.mark.parametrize("shift", [62, 63, 64, 65])
def test_winner_on_either_side_of_a_register_group_edge(ctx, shift, flags, uniq):
    """The winner at disparity index 62 .. 65 of 128: the parabola's neighbours k1 - 1 and k1 + 1 are lanes 63 and 0 of two
    different register groups (the sweep above puts k1 at 63 for D = 65 and never at 64).  test_sgm_gpu.py has the same for the
    winner's other caller."""
    D, r = 128, 2
    w = D + 77
    base = np.random.default_rng(640 + shift).integers(0, 256, (9, w + 300)).astype(np.uint8)
    left, right = base[:, :w], base[:, shift:w + shift]
    disp, n = check(ctx, left, right, 0, D, r, uniq, flags)
    x0, x1 = S.computed_columns(w, 0, D, r, flags)
    got = disp[r:9 - r, x0:x1 + 1].astype(np.int64)
    assert got.size == 370 == n and (((got + 8) >> 4) == shift).all()
    assert ((got & 15) != 0).any()                                    # sub-pixel parts: the neighbour reads took part


@pytest.mark.parametrize("flags", [0, S.FROM_RIGHT])
def test_256_disparities(ctx, flags):
    rng = np.random.default_rng(256)
    base = rng.integers(0, 256, (12, 600)).astype(np.uint8)
    for shift in (0, 100, 255):
        left, right = base[:, :300], base[:, shift:300 + shift]
        disp, n = check(ctx, left, right, 0, 256, 1, 10, flags)
        x0, x1 = S.computed_columns(300, 0, 256, 1, flags)
        assert x1 - x0 + 1 == 300 - 2 - 255 and (((disp[1:11, x0:x1 + 1].astype(np.int64) + 8) >> 4) == shift).all()
    check(ctx, base[:, :300], base[:, 300:], -200, 256, 1, 0, flags)          # unrelated images, a range on both sides of 0


# ---- 3. images -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, S.FROM_RIGHT])
def test_constant_image_every_tie(ctx, flags):
    img = np.full((12, 150), 93, np.uint8)
    for dmin, D, r, uniq in ((-2, 6, 1, 0), (-2, 6, 1, 99), (0, 70, 3, 15), (3, 130, 2, 50)):
        disp, n = check(ctx, img, img, dmin, D, r, uniq, flags)
        x0, x1 = S.computed_columns(150, dmin, D, r, flags)
        assert n == (x1 - x0 + 1) * (12 - 2 * r) and (disp[r:12 - r, x0:x1 + 1] == 16 * dmin).all()


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("r", [2, 4])
def test_two_plane_scene(ctx, r, noise):
    left, right, d_true = S.scene(1, noise)
    disp, n = check(ctx, left, right, 0, S.SCENE_D, r, S.SCENE_UNIQ)
    inner = S.interior(r)
    v = disp.astype(np.int64)
    assert (v[inner] != INV).all() and (np.abs(v[inner] - 16 * d_true[inner]) <= 8).all()
    check(ctx, left, right, 0, S.SCENE_D, r, S.SCENE_UNIQ, S.FROM_RIGHT)


def test_periodic_texture_rejects_more_than_half(ctx):
    left, right = S.periodic()
    for flags in (0, S.FROM_RIGHT):
        ref, n = S.bm(left, right, 0, 32, 2, 15, flags)
        x0, x1 = S.computed_columns(96, 0, 32, 2, flags)
        computed = (x1 - x0 + 1) * (24 - 4)
        assert n < computed / 2                                      # the restatement rejects more than half: the branch is exercised
        assert S.bm(left, right, 0, 32, 2, 0, flags)[1] == computed
        check(ctx, left, right, 0, 32, 2, 15, flags)


@pytest.mark.parametrize("flags", [0, S.FROM_RIGHT])
def test_maximal_cost(ctx, flags):
    """All 0 against all 255 at radius 10: every cost is 441 * 255, the first disparity wins, and any uniqueness above 0 rejects
    it (c2 = c1 > 0)."""
    a, b = np.zeros((25, 100), np.uint8), np.full((25, 100), 255, np.uint8)
    for uniq in (0, 1, 99):
        disp, n = check(ctx, a, b, 0, 70, 10, uniq, flags)
        assert n == (5 * (100 - 20 - 69) if uniq == 0 else 0) and (disp[disp != INV] == 0).all()
    half = a.copy()
    half[:, 50:] = 255                                               # costs from 0 to the maximum in one row
    check(ctx, half, b, -3, 40, 10, 15, flags)


# ---- 4. the left-right check -----------------------------------------------------------------------------------------------

def dev_lr(ctx, lm, rm, max_diff, lstride=None, rstride=None, loff=0, roff=0, want_info=True):
    import torch
    dev = torch.device("cuda", 0)
    h, w = lm.shape
    lstride, rstride = lstride or w, rstride or w
    lbuf, lrows = _padded(lm, lstride, loff, GUARD16)
    rbuf, rrows = _padded(rm, rstride, roff, 777)
    want, n = S.lr_check(lrows, rrows, max_diff, w=w)
    d_l, d_r = torch.from_numpy(lbuf).to(dev), torch.from_numpy(rbuf).to(dev)
    d_info = torch.full((2,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.stereo_lr_check_dev(d_l.data_ptr() + 2 * loff, d_r.data_ptr() + 2 * roff, w, h, lstride, rstride, max_diff, d_info.data_ptr() if want_info else None)
    ctx.synchronize()
    got = d_l.cpu().numpy()
    assert (got[:loff] == GUARD16).all() and (got[loff + h * lstride:] == GUARD16).all()
    assert (got[loff:loff + h * lstride].reshape(h, lstride) == want).all()          # the elements between the rows included
    assert (d_r.cpu().numpy() == rbuf).all()
    assert tuple(d_info.cpu().numpy()) == ((0, n) if want_info else (-9, -9))
    return want[:, :w], n


def test_lr_check_on_the_scene(ctx):
    left, right, d_true = S.scene(1)
    for r in (2, 4):
        lm = S.bm(left, right, 0, S.SCENE_D, r, S.SCENE_UNIQ)[0]
        rm = S.bm(left, right, 0, S.SCENE_D, r, S.SCENE_UNIQ, S.FROM_RIGHT)[0]
        for t, kw in ((16, {}), (0, dict(lstride=99, rstride=101, loff=1, roff=3)), (4, dict(want_info=False))):
            out, n = dev_lr(ctx, lm, rm, t, **kw)
        out, n = dev_lr(ctx, lm, rm, 16)
        assert (out[S.occluded_strip(r, core=True)] == INV).all() and 0 < n < int((lm != INV).sum())


def test_lr_check_hand_placed_values(ctx):
    lm = np.full((5, 67), INV, np.int16)
    rm = np.full((5, 67), 40, np.int16)
    lm[0, 0], lm[0, 66] = 16, -16                                    # xr = -1 and xr = w
    lm[1, 0], lm[1, 66] = 7, -8                                      # xr = x: inside
    lm[2, 3], lm[2, 4], lm[2, 5], lm[2, 6] = 45, 46, 35, 34          # |diff| = max_diff16 and one more, both signs
    lm[3, 65], lm[3, 64] = 40, 40
    rm[3, 63] = INV                                                  # 65 - floor(48 / 16) = 62 valid; 64 - 3 = 61 valid; none looks at 63
    lm[4, 20] = 24
    rm[4, 19] = INV                                                  # 20 - floor(32 / 16) = 18: valid
    out, n = dev_lr(ctx, lm, rm, 5)
    assert out[0, 0] == INV and out[0, 66] == INV and out[1, 0] == INV and out[1, 66] == INV          # |7 - 40| > 5
    assert list(out[2, 3:7]) == [45, INV, 35, INV] and out[3, 65] == 40 and out[3, 64] == 40
    out, n = dev_lr(ctx, lm, rm, 1000)
    assert out[0, 0] == INV and out[0, 66] == INV and out[1, 0] == 7 and out[1, 66] == -8 and out[4, 20] == 24
    lm[4, 20] = 23                                                   # 20 - floor(31 / 16) = 19: invalid
    assert dev_lr(ctx, lm, rm, 1000)[0][4, 20] == INV


# ---- 5. points -------------------------------------------------------------------------------------------------------------

K_RECT, BASE = (310.5, 305.25, 14.75, 9.5), 0.1203


def _point_map():
    rng = np.random.default_rng(77)
    disp = rng.integers(1, 400, (20, 30)).astype(np.int16)
    disp[3, 4], disp[5, 6], disp[7, 8] = INV, 0, -48
    return disp


def _points(n, seed=0):
    rng = np.random.default_rng(870 + n + seed)
    pts = np.stack([rng.uniform(-2, 32, n), rng.uniform(-2, 22, n)], 1).astype(np.float32)
    special = [(4.2, 2.8), (5.5, 5.0), (8.0, 7.49), (np.nan, 3.0), (3.0, np.inf), (-0.5, 0.0), (-0.51, 0.0), (29.49, 19.49), (29.5, 3.0), (3.0, 19.5)]
    if n >= 63:
        pts[:len(special)] = special
    return pts


def dev_points(ctx, disp, pts, R=None, cap=None, n=None, dstride=None, doff=0):
    import torch
    dev = torch.device("cuda", 0)
    h, w = disp.shape
    dstride = dstride or w
    dbuf, drows = _padded(disp, dstride, doff, 999)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    cap = pts.shape[0] if cap is None else cap
    host = np.full((cap, 2), 1.0, np.float32)
    host[:min(cap, pts.shape[0])] = pts[:cap]
    d_d, d_p = torch.from_numpy(dbuf).to(dev), torch.from_numpy(host).to(dev)
    d_x = torch.full((cap * 3 + 16,), -7.5, dtype=torch.float32, device=dev)
    d_n = None if n is None else torch.full((1,), n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.stereo_points_dev(d_d.data_ptr() + 2 * doff, w, h, dstride, K_RECT, BASE, R, d_p.data_ptr(), None if d_n is None else d_n.data_ptr(), cap,
                          d_x.data_ptr())
    ctx.synchronize()
    out = d_x.cpu().numpy()
    assert (out[cap * 3:] == -7.5).all()
    return out[:cap * 3].reshape(cap, 3)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_points_bit_for_bit(ctx, n):
    disp, pts = _point_map(), _points(n)
    R1 = S.rectify(*S.rig_pose(0))[1]
    for R in (None, R1, np.eye(3)):
        want = S.points(disp, K_RECT, BASE, R, pts)
        assert S.same_floats(dev_points(ctx, disp, pts, R), want), n
        assert S.same_floats(dev_points(ctx, disp, pts, R, dstride=37, doff=3), want), n
    if n >= 63:
        got = dev_points(ctx, disp, pts)
        assert np.isnan(got[[0, 1, 2, 3, 4, 6, 8, 9]]).all() and np.isfinite(got[[5, 7]]).all()
        assert (got[[0, 1, 2, 3, 4, 6, 8, 9]].view(np.uint32) == 0x7FC00000).all()


def test_points_count_protocol(ctx):
    disp, pts = _point_map(), _points(257)
    want = S.points(disp, K_RECT, BASE, None, pts)
    for n, rows in ((None, 257), (0, 0), (-1, 0), (170, 170), (257, 257), (1000, 257)):
        got = dev_points(ctx, disp, pts, n=n)
        assert S.same_floats(got[:rows], want[:rows]) and (got[rows:] == -7.5).all(), n          # rows beyond the count keep their bytes
    got = dev_points(ctx, disp, pts[:100], cap=300, n=100)
    assert S.same_floats(got[:100], want[:100]) and (got[100:] == -7.5).all()


# ---- 6. arguments, capture -------------------------------------------------------------------------------------------------

def test_argument_statuses(ctx):
    import torch
    dev = torch.device("cuda", 0)
    W, H = 40, 12
    left, right = S.random_pair(W, H)
    d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    d_d = torch.full((H * W,), GUARD16, dtype=torch.int16, device=dev)
    d_m = torch.full((H * W,), 48, dtype=torch.int16, device=dev)
    d_buf = torch.zeros(8 * W * H, dtype=torch.uint8, device=dev)
    d_pts = torch.full((8, 2), 3.0, dtype=torch.float32, device=dev)
    d_xyz = torch.full((8, 3), -7.5, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    nan, inf = float("nan"), float("inf")
    sp = api.stereo_params

    def bm(l=d_l.data_ptr(), r=d_r.data_ptr(), w=W, h=H, ls=W, rs=W, prm=sp(8, 2), d=d_d.data_ptr(), ds=W):
        ctx.stereo_bm_dev(l, r, w, h, ls, rs, prm, d, ds)

    def lr(l=d_d.data_ptr(), r=d_m.data_ptr(), w=W, h=H, ls=W, rs=W, t=16):
        ctx.stereo_lr_check_dev(l, r, w, h, ls, rs, t)

    def pt(d=d_m.data_ptr(), w=W, h=H, ds=W, K=K_RECT, b=BASE, R=None, p=d_pts.data_ptr(), cap=8, x=d_xyz.data_ptr()):
        ctx.stereo_points_dev(d, w, h, ds, K, b, R, p, None, cap, x)

    bad_reserved = sp(8, 2)
    bad_reserved.reserved[2] = 1
    bad_R = np.eye(3)
    bad_R[1, 2] = nan
    base = d_buf.data_ptr()
    invalid = [lambda: bm(l=0), lambda: bm(r=0), lambda: bm(prm=None), lambda: bm(d=0),
               lambda: bm(prm=sp(8, 0)), lambda: bm(prm=sp(8, 11)), lambda: bm(prm=sp(0, 2)), lambda: bm(prm=sp(257, 2)),
               lambda: bm(prm=sp(8, 2, -1025)), lambda: bm(prm=sp(8, 2, 1018)), lambda: bm(prm=sp(8, 2, 0, -1)), lambda: bm(prm=sp(8, 2, 0, 100)),
               lambda: bm(prm=sp(8, 2, 0, 0, 2)), lambda: bm(prm=sp(8, 2, 0, 0, 3)), lambda: bm(prm=bad_reserved),
               lambda: bm(w=0), lambda: bm(h=0), lambda: bm(h=-2), lambda: bm(ls=W - 1), lambda: bm(rs=W - 1), lambda: bm(ds=W - 1),
               lambda: bm(l=base, d=base), lambda: bm(l=base, d=base + W * H - 1), lambda: bm(r=base + 2 * W * H - 1, d=base),
               lambda: ctx.stereo_bm_dev(d_l.data_ptr(), d_r.data_ptr(), W, H, W, W, sp(8, 2), d_d.data_ptr(), W, d_d.data_ptr() + 64),          # info in the map
               lambda: ctx.stereo_bm_dev(d_l.data_ptr(), d_r.data_ptr(), W, H, W, W, sp(8, 2), d_d.data_ptr(), W, d_l.data_ptr() + W * H - 4),   # ... in an image
               lambda: ctx.stereo_bm_dev(d_l.data_ptr(), d_r.data_ptr(), W, H, W, W, sp(8, 2), d_d.data_ptr(), W, d_r.data_ptr()),
               lambda: ctx.stereo_lr_check_dev(d_d.data_ptr(), d_m.data_ptr(), W, H, W, W, 16, d_m.data_ptr() + 8),
               lambda: ctx.stereo_lr_check_dev(d_d.data_ptr(), d_m.data_ptr(), W, H, W, W, 16, d_d.data_ptr() + 2 * W * H - 4),
               lambda: pt(x=d_m.data_ptr()), lambda: pt(x=d_pts.data_ptr()), lambda: pt(x=d_pts.data_ptr() + 60), lambda: pt(d=base, x=base + 2 * W * H - 4),
               lambda: lr(l=0), lambda: lr(r=0), lambda: lr(t=-1), lambda: lr(w=0), lambda: lr(h=0), lambda: lr(ls=W - 1), lambda: lr(rs=W - 1),
               lambda: lr(l=base, r=base), lambda: lr(l=base, r=base + 2 * W * H - 2),
               lambda: pt(d=0), lambda: pt(p=0), lambda: pt(x=0), lambda: pt(K=(0.0, 300.0, 1.0, 1.0)), lambda: pt(K=(300.0, -1.0, 1.0, 1.0)),
               lambda: pt(K=(300.0, 300.0, nan, 1.0)), lambda: pt(K=(inf, 300.0, 1.0, 1.0)), lambda: pt(b=0.0), lambda: pt(b=-0.1), lambda: pt(b=nan),
               lambda: pt(b=inf), lambda: pt(R=bad_R), lambda: pt(w=0), lambda: pt(h=0), lambda: pt(ds=W - 1), lambda: pt(cap=-1)]
    for k, call in enumerate(invalid):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_INVALID, (k, str(e.value))
    unsupported = [lambda: bm(w=10001, h=10000, ls=10001, rs=10001, ds=10001), lambda: lr(w=10001, h=10000, ls=10001, rs=10001),
                   lambda: pt(w=10001, h=10000, ds=10001), lambda: pt(cap=0)]
    for k, call in enumerate(unsupported):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_UNSUPPORTED, (k, str(e.value))
    z = np.zeros((4, 2), np.float32)
    m = np.full((H, W), 48, np.int16)
    for call in (lambda: ctx.stereo_bm(left, right, sp(8, 0)), lambda: ctx.stereo_bm(left, right, sp(300, 2)),
                 lambda: ctx.stereo_bm(left, right, sp(8, 2, flags=api.PM_STEREO_FROM_RIGHT), lr_max_diff16=16),
                 lambda: ctx.stereo_points(m, (0.0, 1.0, 0.0, 0.0), BASE, z), lambda: ctx.stereo_points(m, K_RECT, -1.0, z),
                 lambda: ctx.stereo_points(m, K_RECT, BASE, z, R=bad_R)):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_INVALID
    # the host forms check the caller's own ranges before anything is staged
    import ctypes as C
    hb = np.zeros(4 * W * H + 64, np.uint8)
    hl, hr = hb[:W * H].reshape(H, W), hb[W * H:2 * W * H].reshape(H, W)
    info = api.StereoInfo()
    L, cp, prm8 = api.lib(), (lambda a: a.ctypes.data_as(C.c_void_p)), sp(8, 2)
    for disp_at, info_p in ((0, C.byref(info)), (W * H - 2, C.byref(info)), (2 * W * H - 2, C.byref(info)),
                            (2 * W * H, C.c_void_p(hb.ctypes.data + 8)), (2 * W * H, C.c_void_p(hb.ctypes.data + 2 * W * H + 16))):
        rc = L.pm_stereo_bm(ctx._h, cp(hl), cp(hr), W, H, W, W, C.byref(prm8), -1, C.c_void_p(hb.ctypes.data + disp_at), W, info_p)
        assert rc == api.PM_E_INVALID, (disp_at, rc)
    assert L.pm_stereo_bm(ctx._h, cp(hl), cp(hr), W, H, W, W, C.byref(prm8), -1, C.c_void_p(hb.ctypes.data + 2 * W * H), W, C.byref(info)) == api.PM_OK
    hx = np.zeros(64, np.float32)
    cam = api.Camera(*K_RECT)
    for pts_at, xyz_at in ((0, 0), (0, 4), (12, 0)):                 # 4 points: 8 floats of pts, 12 of xyz
        rc = L.pm_stereo_points(ctx._h, cp(m), W, H, W, C.byref(cam), C.c_double(BASE), None, C.c_void_p(hx.ctypes.data + 4 * pts_at), 4,
                                C.c_void_p(hx.ctypes.data + 4 * xyz_at))
        assert rc == (api.PM_OK if pts_at == 12 else api.PM_E_INVALID), (pts_at, xyz_at, rc)
    assert L.pm_stereo_points(ctx._h, cp(m), W, H, W, C.byref(cam), C.c_double(BASE), None, cp(hx), 4, cp(m)) == api.PM_E_INVALID
    with pytest.raises(api.PmError) as e:
        ctx.stereo_points(m, K_RECT, BASE, np.zeros((0, 2), np.float32))
    assert e.value.status == api.PM_E_UNSUPPORTED
    for R, t, want in ((np.eye(3), (0.0, -0.3, 0.0), api.PM_E_UNSUPPORTED), (np.eye(3), (0.0, 0.0, 0.0), api.PM_E_NO_MODEL)):
        rc, R1, R2, b, flag = api.stereo_rectify(R, t)
        assert rc == want and not R1.any() and not R2.any() and b == 0.0
    with pytest.raises(api.PmError) as e:
        api.stereo_rectify(np.eye(3), (nan, 0.0, 0.0))
    assert e.value.status == api.PM_E_INVALID
    ctx.synchronize()
    assert (d_d == GUARD16).all() and (d_m == 48).all() and (d_xyz == -7.5).all()          # nothing was launched
    bm(l=base, d=base + W * H + (W * H & 1))                                          # adjacent ranges are fine
    ctx.synchronize()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capturing_stream_is_refused():
    """Refused first thing with PM_E_UNSUPPORTED: nothing is cleared, allocated or launched, and the context keeps working."""
    import torch
    import points_matching_amd as pm
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(st)
    c = pm.Context(0)
    c.set_stream(st.cuda_stream)
    bufs = None
    try:
        W, H = 40, 12
        left, right = S.random_pair(W, H)
        d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
        d_d = torch.full((H, W), GUARD16, dtype=torch.int16, device=dev)
        d_m = torch.full((H, W), 48, dtype=torch.int16, device=dev)
        d_info = torch.full((2,), -5, dtype=torch.int32, device=dev)
        d_pts = torch.full((16, 2), 3.0, dtype=torch.float32, device=dev)
        d_xyz = torch.full((16, 3), -7.5, dtype=torch.float32, device=dev)
        bufs = (d_l, d_r, d_d, d_m, d_info, d_pts, d_xyz)
        torch.cuda.synchronize()
        prm = api.stereo_params(8, 2, 0, 10)
        calls = [lambda: c.stereo_bm_dev(d_l.data_ptr(), d_r.data_ptr(), W, H, W, W, prm, d_d.data_ptr(), W, d_info.data_ptr()),
                 lambda: c.stereo_lr_check_dev(d_d.data_ptr(), d_m.data_ptr(), W, H, W, W, 16, d_info.data_ptr()),
                 lambda: c.stereo_points_dev(d_m.data_ptr(), W, H, W, K_RECT, BASE, None, d_pts.data_ptr(), None, 16, d_xyz.data_ptr()),
                 lambda: c.stereo_bm(left, right, prm), lambda: c.stereo_bm(left, right, prm, lr_max_diff16=16),
                 lambda: c.stereo_points(np.full((H, W), 48, np.int16), K_RECT, BASE, np.zeros((4, 2), np.float32))]
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
        assert (d_d == GUARD16).all() and (d_info == -5).all() and (d_xyz == -7.5).all()
        calls[0]()
        torch.cuda.synchronize()
        want, n = S.bm(left, right, 0, 8, 2, 10)
        assert (d_d.cpu().numpy() == want).all() and tuple(d_info.cpu().numpy()) == (0, n)
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        c.close()
        del bufs


# ---- 7. host forms ---------------------------------------------------------------------------------------------------------

def test_host_forms_equal_the_device_forms(ctx):
    left, right, _ = S.scene(2, True)
    for r, uniq in ((2, 10), (4, 0)):
        for flags in (0, S.FROM_RIGHT):
            prm = api.stereo_params(S.SCENE_D, r, 0, uniq, flags)
            disp, n = ctx.stereo_bm(left, right, prm)
            got, want, _ = dev_bm(ctx, left, right, 0, S.SCENE_D, r, uniq, flags)
            assert (disp.reshape(-1) == got[0][:disp.size]).all() and n == got[2]
        lm = S.bm(left, right, 0, S.SCENE_D, r, uniq)[0]
        rm = S.bm(left, right, 0, S.SCENE_D, r, uniq, S.FROM_RIGHT)[0]
        for t in (0, 16):
            want, n_want = dev_lr(ctx, lm, rm, t)
            disp, n = ctx.stereo_bm(left, right, api.stereo_params(S.SCENE_D, r, 0, uniq), lr_max_diff16=t)
            assert (disp == want).all() and n == n_want
    padded_l = np.ascontiguousarray(np.pad(left, ((0, 0), (0, 5)), constant_values=9))
    padded_r = np.ascontiguousarray(np.pad(right, ((0, 0), (0, 5)), constant_values=200))
    dst = np.full((S.SCENE_H, S.SCENE_W + 7), GUARD16, np.int16)
    out, n = ctx.stereo_bm(padded_l, padded_r, api.stereo_params(S.SCENE_D, 2, 0, 10), 16, w=S.SCENE_W, disp=dst)
    want, n_want = S.lr_check(S.bm(left, right, 0, S.SCENE_D, 2, 10)[0], S.bm(left, right, 0, S.SCENE_D, 2, 10, S.FROM_RIGHT)[0], 16)
    assert out is dst and (dst[:, :S.SCENE_W] == want).all() and (dst[:, S.SCENE_W:] == GUARD16).all() and n == n_want
    disp, pts = _point_map(), _points(257)
    R1 = S.rectify(*S.rig_pose(0))[1]
    for R in (None, R1):
        assert S.same_floats(ctx.stereo_points(disp, K_RECT, BASE, pts, R), dev_points(ctx, disp, pts, R))
    rc, R1g, R2g, b, flag = api.stereo_rectify(*S.rig_pose(3, -1.0))
    ref = S.rectify(*S.rig_pose(3, -1.0))
    assert rc == api.PM_OK and S.bits_equal(R1g, ref[1]) and S.bits_equal(R2g, ref[2]) and b == ref[3] and flag == ref[4] == 1


# ---- 8. the chain ----------------------------------------------------------------------------------------------------------

def test_chain_rectify_match_depth_pnp_on_one_stream(ctx):
    """The two-plane scene as the images of a rig with a pure x baseline looking at two fronto-parallel planes: pm_stereo_rectify
    gives R1 = R2 = I, pm_undistort_dev (no lens) returns both images as they are, then pm_stereo_bm_dev twice,
    pm_stereo_lr_check_dev, a pyramid and pm_corners_dev on the rectified left image, pm_stereo_points_dev at the corners and
    pm_ransac_pnp_run_dev with the corner pixels as uv: one stream, one synchronisation.  Every stage equals its restatement; the
    depths are within half a pixel of disparity of the truth; the pose is the identity."""
    import torch
    import corner_ref
    import pnp_ref
    import undistort_ref as U
    dev = torch.device("cuda", 0)
    left, right, d_true = S.scene(1, True)
    H, W = left.shape
    K, b, r = (80.0, 80.0, 47.5, 23.5), 0.12, 2
    rc, R1, R2, base, flag = api.stereo_rectify(np.eye(3), (-b, 0.0, 0.0))
    assert rc == api.PM_OK and (R1 == np.eye(3)).all() and (R2 == np.eye(3)).all() and base == b and flag == 0
    CAP = 128
    d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    d_rl, d_rr = torch.zeros((H, W), dtype=torch.uint8, device=dev), torch.zeros((H, W), dtype=torch.uint8, device=dev)
    d_lm, d_rm = torch.zeros((H, W), dtype=torch.int16, device=dev), torch.zeros((H, W), dtype=torch.int16, device=dev)
    d_info = torch.zeros((3, 2), dtype=torch.int32, device=dev)
    d_xy = torch.full((CAP, 2), -7.5, dtype=torch.float32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    d_xyz = torch.full((CAP, 3), -7.5, dtype=torch.float32, device=dev)
    k = torch.zeros(1, dtype=torch.int64, device=dev)
    Rt = torch.zeros(12, dtype=torch.float64, device=dev)
    m = torch.zeros(CAP, dtype=torch.uint8, device=dev)
    c = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    prm, wp = api.stereo_params(S.SCENE_D, r, 0, S.SCENE_UNIQ), api.warp_params()
    cp = api.corner_params(3, 1.0, 0.01, 5.0)
    pyr = ctx.pyramid(W, H, 0)
    try:
        ctx.undistort_dev(d_l.data_ptr(), W, H, W, K, None, R1, K, wp, d_rl.data_ptr(), W, H, W)
        ctx.undistort_dev(d_r.data_ptr(), W, H, W, K, None, R2, K, wp, d_rr.data_ptr(), W, H, W)
        ctx.stereo_bm_dev(d_rl.data_ptr(), d_rr.data_ptr(), W, H, W, W, prm, d_lm.data_ptr(), W, d_info[0].data_ptr())
        ctx.stereo_bm_dev(d_rl.data_ptr(), d_rr.data_ptr(), W, H, W, W, api.stereo_params(S.SCENE_D, r, 0, S.SCENE_UNIQ, api.PM_STEREO_FROM_RIGHT),
                          d_rm.data_ptr(), W, d_info[1].data_ptr())
        ctx.stereo_lr_check_dev(d_lm.data_ptr(), d_rm.data_ptr(), W, H, W, W, 16, d_info[2].data_ptr())
        pyr.build_dev(d_rl.data_ptr())
        ctx.corners_dev(pyr, cp, CAP, d_xy.data_ptr(), d_n.data_ptr())
        ctx.stereo_points_dev(d_lm.data_ptr(), W, H, W, K, base, R1, d_xy.data_ptr(), d_n.data_ptr(), CAP, d_xyz.data_ptr())
        view = api.PnpView(d_xyz.data_ptr(), d_xy.data_ptr(), d_n.data_ptr(), CAP, 0)
        ctx.ransac_pnp_run_dev(view, K, 0, 100, 1.0, 5, k.data_ptr(), Rt.data_ptr(), m.data_ptr(), CAP, c.data_ptr())
        ctx.synchronize()
    finally:
        ctx.synchronize()
        pyr.close()
    # every stage against its restatement
    assert (d_rl.cpu().numpy() == U.undistort(left, K, None, R1, K)[0]).all() and (d_rl.cpu().numpy() == left).all()
    assert (d_rr.cpu().numpy() == right).all()
    lm0, n0 = S.bm(left, right, 0, S.SCENE_D, r, S.SCENE_UNIQ)
    rm, n1 = S.bm(left, right, 0, S.SCENE_D, r, S.SCENE_UNIQ, S.FROM_RIGHT)
    lm, n2 = S.lr_check(lm0, rm, 16)
    assert (d_lm.cpu().numpy() == lm).all() and (d_rm.cpu().numpy() == rm).all()
    assert d_info.cpu().numpy().tolist() == [[0, n0], [0, n1], [0, n2]]
    cxy = corner_ref.detect(left, 3, 1.0, 0.01, 5.0, None, CAP)[0]
    n = int(d_n.item())
    assert n == cxy.shape[0] and n >= 40 and (d_xy.cpu().numpy()[:n] == cxy).all()
    xyz = d_xyz.cpu().numpy()
    want = S.points(lm, K, base, R1, cxy)
    assert S.same_floats(xyz[:n], want) and (xyz[n:] == -7.5).all()
    finite = np.isfinite(want).all(1)
    assert 20 <= finite.sum() < n                                    # some corners sit where the check removed the disparity
    # the depths: half a pixel of disparity, carried to depth
    dt = d_true[cxy[:, 1].astype(int), cxy[:, 0].astype(int)].astype(np.float64)
    fb = K[0] * base                                                 # every finite row, the corners at the plane boundary included
    assert (np.abs(want[finite, 2] - fb / dt[finite]) <= fb * 0.5 / (dt[finite] * (dt[finite] - 0.5))).all()
    # the pose
    kr, Rtr, mr, cr = pnp_ref.run(want, cxy, K, 100, 1.0, 5)
    assert (int(k.item()) & ((1 << 64) - 1)) == kr and int(c.item()) == cr
    assert (np.ascontiguousarray(Rt.cpu().numpy()).view(np.uint64) == np.ascontiguousarray(Rtr, np.float64).view(np.uint64)).all()
    mask = m.cpu().numpy()
    assert (mask[:n] == mr).all() and not mask[n:].any()
    assert int(c.item()) >= finite.sum() and not mask[:n][~finite].any()          # NaN rows are never inliers
    Rm, t = Rtr[:9].reshape(3, 3), Rtr[9:]
    rot = float(np.degrees(np.arccos(np.clip((np.trace(Rm) - 1.0) / 2.0, -1.0, 1.0))))
    print("chain: %d corners, %d with depth, %d inliers, rotation %.2e deg, |t| %.2e" % (n, finite.sum(), int(c.item()), rot, np.linalg.norm(t)))
    assert rot < 0.1 and np.linalg.norm(t) < 0.01
