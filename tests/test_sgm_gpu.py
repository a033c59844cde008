"""GPU: pm_stereo_sgm[_dev] (SPEC S89-S92) against the plain-C restatement tests/sgm_ref.c, which tests/test_sgm_cpu.py pins on
the CPU.  Every quantity is an integer and a function of the inputs alone: every comparison is bit for bit, over the whole
guarded buffer, with n_valid and status.

The kernels' tiles.  sgm_census: a workgroup owns 64 columns x 4 rows of the IMAGE (staged with a margin of 4 columns and 3
rows): images of that tile exactly and one past it in each direction.  sgm_path: no tile in the image; a wave walks a path with a
lane per disparity, 64 disparities per register group, up to four groups: disparity counts at each group boundary and one to
either side, and true shifts whose winner and its two neighbours straddle lanes 63 | 64.  A horizontal pass has one wave per
computed row, a vertical or diagonal pass one per computed column, and a diagonal wave that leaves the rectangle's side enters
at the other side and restarts: rectangles one pixel wide or high (every step of some direction restarts) and 5 wide or high
(diagonal waves wrap many times, or barely)."""
import gc

import numpy as np
import pytest

import sgm_ref as G
import stereo_ref as S
from points_matching_amd import api

pytestmark = pytest.mark.gpu
GUARD16 = 0x5A5A
INV = S.INVALID
BOTH = [0, S.FROM_RIGHT]


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


def dev_sgm(ctx, left, right, dmin, D, p1=4, p2=24, paths=8, uniq=0, flags=0, lstride=None, rstride=None, dstride=None, loff=0, roff=0, doff=0,
            want_info=True):
    """pm_stereo_sgm_dev on guarded torch buffers -> (whole disp buffer, status, n_valid) and the same three from the C
    restatement written into an equally guarded host buffer; also the (h, w) map."""
    import torch
    dev = torch.device("cuda", 0)
    h, w = left.shape
    lstride, rstride, dstride = lstride or w, rstride or w, dstride or w
    lbuf, lrows = _padded(left, lstride, loff, 201)
    rbuf, rrows = _padded(right, rstride, roff, 37)
    want = np.full(doff + h * dstride + 64, GUARD16, np.int16)
    _, n = G.sgm(lrows, rrows, dmin, D, p1, p2, paths, uniq, flags, w=w, disp=want[doff:doff + h * dstride].reshape(h, dstride), dstride=dstride)
    d_l, d_r = torch.from_numpy(lbuf).to(dev), torch.from_numpy(rbuf).to(dev)
    d_d = torch.full((want.size,), GUARD16, dtype=torch.int16, device=dev)
    d_info = torch.full((2,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.stereo_sgm_dev(d_l.data_ptr() + loff, d_r.data_ptr() + roff, w, h, lstride, rstride, api.sgm_params(D, p1, p2, paths, dmin, uniq, flags),
                       d_d.data_ptr() + 2 * doff, dstride, d_info.data_ptr() if want_info else None)
    ctx.synchronize()
    info = d_info.cpu().numpy()
    return (d_d.cpu().numpy(), int(info[0]), int(info[1])), (want, 0, n), want[doff:doff + h * dstride].reshape(h, dstride)[:, :w]


def check(ctx, left, right, dmin, D, p1=4, p2=24, paths=8, uniq=0, flags=0, **kw):
    got, want, disp = dev_sgm(ctx, left, right, dmin, D, p1, p2, paths, uniq, flags, **kw)
    bad = int((got[0] != want[0]).sum())
    assert bad == 0, ("disp", left.shape, dmin, D, p1, p2, paths, uniq, flags, kw, bad)
    assert got[1:] == want[1:], (left.shape, dmin, D, p1, p2, paths, uniq, flags, got[1:], want[1:])
    return disp, want[2]


def rect_image(wc, hc, dmin, D, seed=0):
    """A random pair whose computed rectangle (left map) is wc x hc."""
    dmax = dmin + D - 1
    return S.random_pair(wc + 8 + max(dmax, 0) - min(dmin, 0), hc + 6, seed=seed)


# ---- 1. shapes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", BOTH)
def test_one_computed_pixel_and_none(ctx, flags):
    for dmin, D in ((0, 1), (0, 5), (-2, 4), (3, 6), (0, 70)):
        dmax = dmin + D - 1
        w1, h1 = 9 + max(dmax, 0) - min(dmin, 0), 7
        for w, h, n in ((w1, h1, 1), (w1 - 1, h1, 0), (w1, h1 - 1, 0), (1, 1, 0)):
            left, right = S.random_pair(w, h, seed=D)
            for paths in (4, 8):
                disp, n_valid = check(ctx, left, right, dmin, D, 4, 24, paths, 0, flags)
                assert n_valid == n and int((disp != INV).sum()) == n


@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("wc,hc", [(1, 40), (40, 1), (5, 40), (40, 5), (2, 2), (64, 3), (65, 3)])
def test_thin_rectangles(ctx, wc, hc, flags):
    """One pixel wide: every diagonal step leaves the side and restarts, the horizontal paths are one pixel long.  One pixel
    high: every vertical and diagonal path is one pixel long.  Five: the diagonal waves wrap eight times, or never reach the
    side before the rows end."""
    for dmin, D, uniq in ((0, 6, 0), (-3, 9, 15)):
        left, right = rect_image(wc, hc, dmin, D, seed=wc)          # S90: the right map's rectangle has the same size
        for paths in (4, 8):
            disp, n = check(ctx, left, right, dmin, D, 4, 24, paths, uniq, flags)
            x0, x1, y0, y1 = G.computed_rect(left.shape[1], left.shape[0], dmin, D, flags)
            assert (x1 - x0 + 1, y1 - y0 + 1) == (wc, hc) and (n == wc * hc or uniq)


@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("w,h", [(64, 8), (65, 9), (64, 9), (65, 8), (63, 7), (129, 13)])
def test_census_tile_and_one_past_it(ctx, w, h, flags):
    left, right = S.random_pair(w, h)
    for dmin, D in ((0, 1), (0, 4), (-2, 5)):
        check(ctx, left, right, dmin, D, 4, 24, 8, 10, flags)


@pytest.mark.parametrize("flags", BOTH)
def test_odd_strides_and_base_addresses(ctx, flags):
    left, right = S.random_pair(71, 13)
    for k, (ls, rs, ds, lo, ro, do) in enumerate(((71, 71, 71, 0, 0, 0), (73, 79, 75, 1, 3, 1), (77, 71, 83, 3, 2, 3), (72, 75, 71, 2, 1, 2))):
        got, want, disp = dev_sgm(ctx, left, right, -3, 9, 4, 24, 8, 10, flags, lstride=ls, rstride=rs, dstride=ds, loff=lo, roff=ro, doff=do)
        assert (got[0] == want[0]).all() and got[1:] == want[1:], k
        assert (want[0][:do] == GUARD16).all() and (want[0][-64:] == GUARD16).all() and 0 < want[2] < 71 * 13
    got, want, _ = dev_sgm(ctx, left, right, -3, 9, 4, 24, 8, 10, flags, want_info=False)
    assert (got[0] == want[0]).all() and got[1:] == (-9, -9)


# ---- 2. parameters ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("D", [1, 2, 3, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256])
def test_disparity_counts_around_the_lane_groups(ctx, D, flags):
    w = D + 77                                                       # 70 computed columns at dmin = 0
    rng = np.random.default_rng(D)
    base = rng.integers(0, 256, (9, w + 300)).astype(np.uint8)
    shift = max(D - 2, 0)                                            # the true disparity sits near the top of the range
    left, right = base[:, :w], base[:, shift:w + shift]              # right(x - shift) = left(x)
    for dmin, uniq in ((0, 0), (-7, 15), (5, 15)):
        disp, n = check(ctx, left, right, dmin, D, 4, 24, 8, uniq, flags)
    assert n > 0
    if D >= 3:
        x0, x1, y0, y1 = G.computed_rect(w, 9, 0, D, flags)
        top = check(ctx, left, right, 0, D, 4, 24, 8, 0, flags)[0][y0:y1 + 1, x0:x1 + 1].astype(np.int64)
        assert (((top + 8) >> 4) == shift).all()                     # the winner is where the test wants it


@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("shift", [62, 63, 64, 65])
def test_winner_and_neighbours_straddle_a_lane_group(ctx, shift, flags):
    w = 128 + 77
    base = np.random.default_rng(640 + shift).integers(0, 256, (9, w + 300)).astype(np.uint8)
    left, right = base[:, :w], base[:, shift:w + shift]
    for dmin, uniq, paths in ((0, 0, 8), (0, 15, 4), (-1, 15, 8)):
        disp, n = check(ctx, left, right, dmin, 128, 4, 24, paths, uniq, flags)
    x0, x1, y0, y1 = G.computed_rect(w, 9, -1, 128, flags)
    assert n > 0 and (((disp[y0:y1 + 1, x0:x1 + 1].astype(np.int64) + 8) >> 4) == shift).all()
    # smooth images: the neighbours of the winner cost little more, so the sub-pixel step reads both sides of the boundary
    ramp = ((np.arange(w + 300)[None, :] * 3 + np.arange(9)[:, None] * 5) % 251).astype(np.uint8)
    check(ctx, ramp[:, :w], ramp[:, shift:w + shift], 0, 128, 1, 2, 8, 0, flags)


@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("paths", [4, 8])
def test_penalties(ctx, paths, flags):
    left, right, _ = S.scene(1, True)
    left, right = left[:20], right[:20]
    for p1, p2 in G.PENALTIES:
        for dmin, uniq in ((0, 0), (-7, 15), (5, 99)):
            check(ctx, left, right, dmin, 16, p1, p2, paths, uniq, flags)


@pytest.mark.parametrize("flags", BOTH)
def test_constant_image_and_maximal_cost(ctx, flags):
    img = np.full((12, 150), 93, np.uint8)
    for dmin, D, uniq in ((-2, 6, 0), (-2, 6, 99), (0, 70, 15), (3, 130, 50)):
        disp, n = check(ctx, img, img, dmin, D, 1023, 1023, 8, uniq, flags)
        x0, x1, y0, y1 = G.computed_rect(150, 12, dmin, D, flags)
        assert n == (x1 - x0 + 1) * (y1 - y0 + 1) and (disp[y0:y1 + 1, x0:x1 + 1] == 16 * dmin).all()
    # a checkerboard against its inverse: every second disparity costs 31 bits, the others none, with the largest penalties
    hi = ((np.add.outer(np.arange(12), np.arange(150)) % 2) * 255).astype(np.uint8)
    check(ctx, hi, 255 - hi, 0, 70, 1023, 1023, 8, 15, flags)
    check(ctx, hi, 255 - hi, 0, 70, 0, 1023, 8, 0, flags)


# ---- 3. images -------------------------------------------------------------------------------------------------------------

def test_two_plane_scene(ctx):
    left, right, d_true = S.scene(1, True)
    inner = S.interior(4)
    for p1, p2, paths in ((4, 24, 4), (4, 24, 8), (8, 32, 8)):
        disp, n = check(ctx, left, right, 0, 16, p1, p2, paths)
        v = disp.astype(np.int64)
        assert n == 3066 and (v[inner] != INV).all() and (np.abs(v[inner] - 16 * d_true[inner]) <= 8).all()
    check(ctx, left, right, 0, 16, 4, 24, 8, 10, S.FROM_RIGHT)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_textureless_band_on_the_device_map(ctx, seed):
    left, right, mask = G.band_scene(seed)
    for p1, p2, paths in ((4, 24, 4), (4, 24, 8), (8, 32, 8)):
        disp, _ = check(ctx, left, right, 0, 16, p1, p2, paths)
        assert G.off_by_more_than_half(disp, mask, G.BAND_TRUE16) == 0
    disp, _ = check(ctx, left, right, 0, 16, 0, 0, 8)
    assert G.off_by_more_than_half(disp, mask, G.BAND_TRUE16) > 210
    bm, _ = ctx.stereo_bm(left, right, api.stereo_params(16, 4))
    assert G.off_by_more_than_half(bm, mask, G.BAND_TRUE16) > 210


def test_periodic_texture(ctx):
    left, right = S.periodic()
    for flags in BOTH:
        for uniq in (0, 15, 99):
            check(ctx, left, right, 0, 32, 4, 24, 8, uniq, flags)


# ---- 4. host form, chain, arena --------------------------------------------------------------------------------------------

def test_host_form_with_and_without_the_left_right_check(ctx):
    left, right, _ = S.scene(2, True)
    for paths, uniq in ((8, 10), (4, 0)):
        for flags in BOTH:
            disp, n = ctx.stereo_sgm(left, right, api.sgm_params(16, 4, 24, paths, 0, uniq, flags))
            want, n_want = G.sgm(left, right, 0, 16, 4, 24, paths, uniq, flags)
            assert (disp == want).all() and n == n_want
        lm = G.sgm(left, right, 0, 16, 4, 24, paths, uniq)[0]
        rm = G.sgm(left, right, 0, 16, 4, 24, paths, uniq, S.FROM_RIGHT)[0]
        for t in (0, 16):
            want, n_want = S.lr_check(lm, rm, t)
            disp, n = ctx.stereo_sgm(left, right, api.sgm_params(16, 4, 24, paths, 0, uniq), lr_max_diff16=t)
            assert (disp == want).all() and n == n_want and 0 < n < int((lm != INV).sum())
    padded_l = np.ascontiguousarray(np.pad(left, ((0, 0), (0, 5)), constant_values=9))
    padded_r = np.ascontiguousarray(np.pad(right, ((0, 0), (0, 5)), constant_values=200))
    dst = np.full((S.SCENE_H, S.SCENE_W + 7), GUARD16, np.int16)
    out, n = ctx.stereo_sgm(padded_l, padded_r, api.sgm_params(16, 4, 24, 8, 0, 10), 16, w=S.SCENE_W, disp=dst)
    want, n_want = S.lr_check(G.sgm(left, right, 0, 16, 4, 24, 8, 10)[0], G.sgm(left, right, 0, 16, 4, 24, 8, 10, S.FROM_RIGHT)[0], 16)
    assert out is dst and (dst[:, :S.SCENE_W] == want).all() and (dst[:, S.SCENE_W:] == GUARD16).all() and n == n_want


def test_chain_on_one_stream(ctx):
    """pm_stereo_sgm_dev left and right, pm_stereo_lr_check_dev and pm_stereo_points_dev enqueued on one stream, one
    synchronisation: every stage equals the restatement chain."""
    import torch
    dev = torch.device("cuda", 0)
    left, right, d_true = S.scene(1, True)
    H, W = left.shape
    K, base = (80.0, 80.0, 47.5, 23.5), 0.12
    ys, xs = np.mgrid[4:H - 4:5, 20:W - 6:7]
    pts = np.stack([xs.reshape(-1) + 0.25, ys.reshape(-1) - 0.25], 1).astype(np.float32)
    d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    d_lm, d_rm = torch.zeros((H, W), dtype=torch.int16, device=dev), torch.zeros((H, W), dtype=torch.int16, device=dev)
    d_info = torch.zeros((3, 2), dtype=torch.int32, device=dev)
    d_p = torch.from_numpy(pts).to(dev)
    d_xyz = torch.full((pts.shape[0], 3), -7.5, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.stereo_sgm_dev(d_l.data_ptr(), d_r.data_ptr(), W, H, W, W, api.sgm_params(16, 4, 24, 8, 0, 10), d_lm.data_ptr(), W, d_info[0].data_ptr())
    ctx.stereo_sgm_dev(d_l.data_ptr(), d_r.data_ptr(), W, H, W, W, api.sgm_params(16, 4, 24, 8, 0, 10, api.PM_STEREO_FROM_RIGHT), d_rm.data_ptr(), W,
                       d_info[1].data_ptr())
    ctx.stereo_lr_check_dev(d_lm.data_ptr(), d_rm.data_ptr(), W, H, W, W, 16, d_info[2].data_ptr())
    ctx.stereo_points_dev(d_lm.data_ptr(), W, H, W, K, base, None, d_p.data_ptr(), None, pts.shape[0], d_xyz.data_ptr())
    ctx.synchronize()
    lm0, n0 = G.sgm(left, right, 0, 16, 4, 24, 8, 10)
    rm, n1 = G.sgm(left, right, 0, 16, 4, 24, 8, 10, S.FROM_RIGHT)
    lm, n2 = S.lr_check(lm0, rm, 16)
    assert (d_lm.cpu().numpy() == lm).all() and (d_rm.cpu().numpy() == rm).all()
    assert d_info.cpu().numpy().tolist() == [[0, n0], [0, n1], [0, n2]] and 0 < n2 < n0
    want = S.points(lm, K, base, None, pts)
    assert S.same_floats(d_xyz.cpu().numpy(), want)
    finite = np.isfinite(want).all(1)
    dt = d_true[np.floor(pts[:, 1] + 0.5).astype(int), np.floor(pts[:, 0] + 0.5).astype(int)].astype(np.float64)
    fb = K[0] * base
    inner = S.interior(4)[np.floor(pts[:, 1] + 0.5).astype(int), np.floor(pts[:, 0] + 0.5).astype(int)] & finite
    assert inner.sum() >= 20 and (np.abs(want[inner, 2] - fb / dt[inner]) <= fb * 0.5 / (dt[inner] * (dt[inner] - 0.5))).all()


def test_arena_growth_larger_after_smaller(ctx):
    """A fresh context: its arena grows at the second call (and the first size runs again in the grown arena)."""
    import torch
    import points_matching_amd as pm
    c = pm.Context(0)
    try:
        small = S.random_pair(40, 12, seed=5)
        large = S.random_pair(400, 200, seed=6)                      # 1.2 MB of census words and 4.6 MB of sums: past the first MiB
        for left, right, D in ((small[0], small[1], 8), (large[0], large[1], 32), (small[0], small[1], 8)):
            check(c, left, right, 0, D, 4, 24, 8, 10)
    finally:
        torch.cuda.synchronize()
        c.close()


# ---- 5. arguments, capture -------------------------------------------------------------------------------------------------

def test_argument_statuses_leave_the_outputs_untouched(ctx):
    import ctypes as C
    import torch
    dev = torch.device("cuda", 0)
    W, H = 40, 12
    left, right = S.random_pair(W, H)
    d_l, d_r = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
    d_d = torch.full((H * W + 64,), GUARD16, dtype=torch.int16, device=dev)
    d_info = torch.full((2,), -9, dtype=torch.int32, device=dev)
    d_buf = torch.zeros(8 * W * H, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sp = api.sgm_params

    def sgm(l=d_l.data_ptr(), r=d_r.data_ptr(), w=W, h=H, ls=W, rs=W, prm=sp(8, 4, 24), d=d_d.data_ptr(), ds=W, info=d_info.data_ptr()):
        ctx.stereo_sgm_dev(l, r, w, h, ls, rs, prm, d, ds, info)

    bad_reserved = sp(8, 4, 24)
    bad_reserved.reserved = 1
    base = d_buf.data_ptr()
    invalid = [lambda: sgm(l=0), lambda: sgm(r=0), lambda: sgm(prm=None), lambda: sgm(d=0),
               lambda: sgm(prm=sp(0, 4, 24)), lambda: sgm(prm=sp(257, 4, 24)), lambda: sgm(prm=sp(8, 4, 24, 8, -1025)), lambda: sgm(prm=sp(8, 4, 24, 8, 1018)),
               lambda: sgm(prm=sp(8, -1, 24)), lambda: sgm(prm=sp(8, 25, 24)), lambda: sgm(prm=sp(8, 4, 1024)), lambda: sgm(prm=sp(8, 4, 24, 0)),
               lambda: sgm(prm=sp(8, 4, 24, 5)), lambda: sgm(prm=sp(8, 4, 24, 16)), lambda: sgm(prm=sp(8, 4, 24, 8, 0, -1)),
               lambda: sgm(prm=sp(8, 4, 24, 8, 0, 100)), lambda: sgm(prm=sp(8, 4, 24, 8, 0, 0, 2)), lambda: sgm(prm=sp(8, 4, 24, 8, 0, 0, 3)),
               lambda: sgm(prm=bad_reserved),
               lambda: sgm(w=0), lambda: sgm(h=0), lambda: sgm(h=-2), lambda: sgm(ls=W - 1), lambda: sgm(rs=W - 1), lambda: sgm(ds=W - 1),
               lambda: sgm(l=base, d=base), lambda: sgm(l=base, d=base + W * H - 1), lambda: sgm(r=base + 2 * W * H - 1, d=base),
               lambda: sgm(info=d_d.data_ptr() + 64), lambda: sgm(info=d_l.data_ptr() + W * H - 4), lambda: sgm(info=d_r.data_ptr())]
    for k, call in enumerate(invalid):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_INVALID, (k, str(e.value))
    unsupported = [lambda: sgm(w=10001, h=10000, ls=10001, rs=10001, ds=10001),
                   lambda: sgm(w=4096 + 8 + 63 + 1, h=4096 + 6, ls=4168, rs=4168, ds=4168, prm=sp(64, 4, 24, 8, -63))]          # 2^30 + 64 * 4096 sums
    for k, call in enumerate(unsupported):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_UNSUPPORTED, (k, str(e.value))
    for call in (lambda: ctx.stereo_sgm(left, right, sp(8, 30, 24)), lambda: ctx.stereo_sgm(left, right, sp(300, 4, 24)),
                 lambda: ctx.stereo_sgm(left, right, sp(8, 4, 24, flags=api.PM_STEREO_FROM_RIGHT), lr_max_diff16=16)):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_INVALID
    # the host form checks the caller's own ranges before anything is staged
    hb = np.full(4 * W * H + 64, 7, np.uint8)
    hl, hr = hb[:W * H].reshape(H, W), hb[W * H:2 * W * H].reshape(H, W)
    info = api.StereoInfo(-9, -9)
    L, cp, prm8 = api.lib(), (lambda a: a.ctypes.data_as(C.c_void_p)), sp(8, 4, 24)
    for disp_at, info_p in ((0, C.byref(info)), (W * H - 2, C.byref(info)), (2 * W * H - 2, C.byref(info)),
                            (2 * W * H, C.c_void_p(hb.ctypes.data + 8)), (2 * W * H, C.c_void_p(hb.ctypes.data + 2 * W * H + 16))):
        rc = L.pm_stereo_sgm(ctx._h, cp(hl), cp(hr), W, H, W, W, C.byref(prm8), -1, C.c_void_p(hb.ctypes.data + disp_at), W, info_p)
        assert rc == api.PM_E_INVALID, (disp_at, rc)
    assert (hb == 7).all() and (info.status, info.n_valid) == (-9, -9)
    ctx.synchronize()
    assert (d_d == GUARD16).all() and (d_info == -9).all()             # nothing was launched, nothing cleared
    sgm(l=base, d=base + W * H + (W * H & 1), info=None)               # adjacent ranges are fine
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
        d_info = torch.full((2,), -5, dtype=torch.int32, device=dev)
        bufs = (d_l, d_r, d_d, d_info)
        torch.cuda.synchronize()
        prm = api.sgm_params(8, 4, 24, 8, 0, 10)
        calls = [lambda: c.stereo_sgm_dev(d_l.data_ptr(), d_r.data_ptr(), W, H, W, W, prm, d_d.data_ptr(), W, d_info.data_ptr()),
                 lambda: c.stereo_sgm(left, right, prm), lambda: c.stereo_sgm(left, right, prm, lr_max_diff16=16)]
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
        assert (d_d == GUARD16).all() and (d_info == -5).all()
        calls[0]()
        torch.cuda.synchronize()
        want, n = G.sgm(left, right, 0, 8, 4, 24, 8, 10)
        assert (d_d.cpu().numpy() == want).all() and tuple(d_info.cpu().numpy()) == (0, n)
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        c.close()
        del bufs
