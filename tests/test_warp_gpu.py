"""GPU: pm_warp[_dev] and pm_transform_points[_dev] (SPEC S75-S78) against the plain-C restatement tests/warp_ref.c, which
tests/test_warp_cpu.py pins on the CPU.  The output, the valid mask and n_valid are integers that are a function of the inputs
alone, and the points are single fp64 expressions: every comparison is bit for bit, there is no tolerance anywhere.  Shapes are
the smallest that reach each edge of the kernel: fewer pixels than a thread's four, one 64 x 16 tile exactly, one past it in
both directions, odd strides and base addresses."""
import gc

import numpy as np
import pytest

import describe_ref as D
import lk_ref as R
import warp_ref as W
from points_matching_amd import api

pytestmark = pytest.mark.gpu
GUARD = 0xA5
SW, SH = 67, 35
BORDER = 77


@pytest.fixture(scope="module")
def ctx():
    import torch
    import points_matching_amd as pm
    c = pm.Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()
    gc.collect()


@pytest.fixture(scope="module")
def src():
    return W.random_source(SW, SH)


H0 = W.homography(2)


def dev_warp(ctx, src, M, flags=0, border=BORDER, dw=None, dh=None, dstride=None, offset=0, sw=None, want_valid=True, want_info=True):
    """pm_warp_dev on guarded torch buffers -> (whole dst buffer, whole valid buffer, status, n_valid) and the same four from
    the C restatement written into equally guarded host buffers."""
    import torch
    dev = torch.device("cuda", 0)
    src = np.ascontiguousarray(src, np.uint8)
    sh, sstride = src.shape
    sw = sstride if sw is None else sw
    dw = sw if dw is None else dw
    dh = sh if dh is None else dh
    dstride = dw if dstride is None else dstride
    M = np.ascontiguousarray(M, np.float64).reshape(-1)
    want_dst = np.full(offset + dh * dstride + 64, GUARD, np.uint8)
    want_val = np.full(offset + dh * dw + 64, GUARD, np.uint8)
    ref = W.warp(src, M, flags, border, dw, dh, sw, dst=want_dst[offset:offset + dh * dstride].reshape(dh, dstride), dstride=dstride)
    want_val[offset:offset + dh * dw] = ref[1].reshape(-1)
    d_src = torch.from_numpy(src).to(dev)
    d_M = torch.from_numpy(M).to(dev)
    d_dst = torch.full((want_dst.size,), GUARD, dtype=torch.uint8, device=dev)
    d_val = torch.full((want_val.size,), GUARD, dtype=torch.uint8, device=dev)
    d_info = torch.full((2,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.warp_dev(d_src.data_ptr(), sw, sh, sstride, d_M.data_ptr(), api.warp_params(flags, border), d_dst.data_ptr() + offset, dw, dh, dstride,
                 d_val.data_ptr() + offset if want_valid else None, d_info.data_ptr() if want_info else None)
    ctx.synchronize()
    info = d_info.cpu().numpy()
    return (d_dst.cpu().numpy(), d_val.cpu().numpy(), int(info[0]), int(info[1])), (want_dst, want_val, ref[2], ref[3])


def check(ctx, src, M, flags=0, **kw):
    got, want = dev_warp(ctx, src, M, flags, **kw)
    assert (got[0] == want[0]).all(), ("dst", flags, kw, int((got[0] != want[0]).sum()))
    assert (got[1] == want[1]).all(), ("valid", flags, kw, int((got[1] != want[1]).sum()))
    assert got[2:] == want[2:], (flags, kw, got[2:], want[2:])
    return want


# ---- 6. shapes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, W.REPLICATE])
@pytest.mark.parametrize("dw,dh,dstride", [(1, 1, 1), (3, 5, 3), (64, 16, 64), (65, 17, 65), (67, 35, 71)])
def test_output_shapes(ctx, src, dw, dh, dstride, flags):
    check(ctx, src, H0, flags, dw=dw, dh=dh, dstride=dstride)


@pytest.mark.parametrize("flags", [0, W.REPLICATE])
def test_odd_base_addresses_leave_the_surroundings_untouched(ctx, src, flags):
    for offset in (1, 2, 3):
        want = check(ctx, src, H0, flags, dstride=71, offset=offset)
        assert (want[0][:offset] == GUARD).all() and (want[0][-64:] == GUARD).all() and 0 < want[3] < SW * SH


def test_tiny_sources_and_other_output_sizes(ctx, src):
    one, two = np.array([[200]], np.uint8), np.array([[10, 250], [90, 170]], np.uint8)
    half = np.array([[0.25, 0, -0.4], [0, 0.25, -0.3], [0, 0, 1.0]])          # a 9 x 9 output over and around the source
    for flags in (0, W.REPLICATE):
        check(ctx, one, half, flags, dw=9, dh=9)
        check(ctx, two, half, flags, dw=9, dh=9)
        check(ctx, one, np.eye(3), flags)
        big = check(ctx, src, H0, flags, dw=150, dh=90)                         # larger than the source
        small = check(ctx, src, H0, flags, dw=30, dh=20)                        # smaller
        assert 0 < big[3] < 150 * 90 and small[3] > 0
    check(ctx, np.ascontiguousarray(np.pad(src, ((0, 0), (0, 6)))), H0, 0, sw=SW)          # a source stride of 73


def test_without_valid_or_info(ctx, src):
    got, want = dev_warp(ctx, src, H0, 0, want_valid=False, want_info=False)
    assert (got[0] == want[0]).all() and (got[1] == GUARD).all() and got[2:] == (-9, -9)


# ---- 7. models and positions -------------------------------------------------------------------------------------------------

def _unit_row(eps):
    M = W.homography(5).copy()
    M[2] = (0.0, 0.0, 1.0 + eps)
    return M


MODELS = {
    "identity": np.eye(3),
    "negative positions": W.translation(-5.3, -2.7),
    "ties": W.translation(0.5 / 32, 1.5 / 32),
    "ties, negative": W.translation(-3 - 0.5 / 32, -1 - 2.5 / 32),
    "half pixel": W.translation(0.5, 0.5),
    "quarter turn": W.quarter_turn(SH),
    "3e7 px away": W.translation(3e7, 0),
    "past 2^30": W.translation(4e7, -4e7),
    "W = 0 column": np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -10.0]]),
    "NaN": np.array([[1.0, 0, 0], [0, np.nan, 0], [0, 0, 1.0]]),
    "infinite": np.array([[1.0, 0, np.inf], [0, 1.0, 0], [0, 0, 1.0]]),
    "zero": np.zeros((3, 3)),
    "singular": np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]),
    "last row (0, 0, 1)": _unit_row(0.0),
    "last row (0, 0, 1 + 2^-52)": _unit_row(2.0 ** -52),
    "strong perspective": np.array([[1.0, 0.1, -3], [0.05, 1.0, 2], [0.01, -0.02, 1.0]]),
}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_models_and_positions(ctx, src, name):
    M = MODELS[name]
    for flags in (0, W.REPLICATE, W.INVERT, W.INVERT | W.REPLICATE):
        want = check(ctx, src, M, flags)
        if name in ("NaN", "infinite", "singular"):
            assert want[2] == 1 and want[3] == 0
        elif name == "zero":
            assert want[2] == 2 and want[3] == 0
        else:
            assert want[2] == 0
    if name == "quarter turn":
        check(ctx, src, M, 0, dw=SH, dh=SW)


def test_affine_models(ctx, src):
    A = W.homography(4)[:2]
    for flags in (W.AFFINE, W.AFFINE | W.INVERT, W.AFFINE | W.REPLICATE):
        a = check(ctx, src, A, flags)
        b = check(ctx, src, np.vstack([A, [0, 0, 1.0]]), flags & ~W.AFFINE)
        assert (a[0] == b[0]).all() and a[3] == b[3] > 0
    assert check(ctx, src, np.zeros(6), W.AFFINE)[2] == 2
    assert check(ctx, src, np.array([1.0, 2, 0, 2, 4, 0]), W.AFFINE | W.INVERT)[2] == 1


# ---- 8. arguments, capture ---------------------------------------------------------------------------------------------------

def test_argument_statuses(ctx, src):
    import torch
    dev = torch.device("cuda", 0)
    d_buf = torch.zeros(2 * SW * SH, dtype=torch.uint8, device=dev)
    d_src = torch.from_numpy(src).to(dev)
    d_dst = torch.full((SH * SW,), GUARD, dtype=torch.uint8, device=dev)
    d_M = torch.from_numpy(np.eye(3).reshape(-1)).to(dev)
    d_pts = torch.zeros((8, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def warp(s=d_src.data_ptr(), sw=SW, sh=SH, ss=SW, M=d_M.data_ptr(), prm=api.warp_params(), d=d_dst.data_ptr(), dw=SW, dh=SH, ds=SW):
        ctx.warp_dev(s, sw, sh, ss, M, prm, d, dw, dh, ds)

    def pts(M=d_M.data_ptr(), flags=0, p=d_pts.data_ptr(), cap=8, out=d_pts.data_ptr()):
        ctx.transform_points_dev(M, flags, p, None, cap, out)

    bad_reserved = api.warp_params()
    bad_reserved.reserved[1] = 1
    base = d_buf.data_ptr()
    invalid = [lambda: warp(s=0), lambda: warp(M=0), lambda: warp(prm=None), lambda: warp(d=0),
               lambda: warp(prm=api.warp_params(8)), lambda: warp(prm=api.warp_params(0, 256)), lambda: warp(prm=api.warp_params(0, -1)),
               lambda: warp(prm=bad_reserved), lambda: warp(sw=0), lambda: warp(sh=0), lambda: warp(dw=0), lambda: warp(dh=-1),
               lambda: warp(ss=SW - 1), lambda: warp(ds=SW - 1),
               lambda: warp(s=base, d=base),                                        # the same image
               lambda: warp(s=base, d=base + SW * SH - 1),                          # the last source byte is the first of dst
               lambda: warp(s=base + SW * SH - 1, d=base),
               lambda: pts(M=0), lambda: pts(p=0), lambda: pts(out=0), lambda: pts(flags=2), lambda: pts(flags=8), lambda: pts(cap=-1)]
    for k, call in enumerate(invalid):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_INVALID, (k, str(e.value))
    unsupported = [lambda: warp(sw=10001, sh=10000, ss=10001), lambda: warp(dw=10001, dh=10000, ds=10001), lambda: pts(cap=0)]
    for k, call in enumerate(unsupported):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_UNSUPPORTED, (k, str(e.value))
    for call in (lambda: ctx.warp(src, np.eye(3), api.warp_params(16)), lambda: ctx.warp(src, np.eye(3), api.warp_params(0, 300)),
                 lambda: ctx.transform_points(np.eye(3), np.zeros((4, 2), np.float32), 2)):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_INVALID
    with pytest.raises(api.PmError) as e:
        ctx.transform_points(np.eye(3), np.zeros((0, 2), np.float32))
    assert e.value.status == api.PM_E_UNSUPPORTED
    ctx.synchronize()
    assert (d_dst == GUARD).all()                                                    # nothing was launched
    warp(s=base, d=base + SW * SH)                                                   # adjacent ranges are fine
    warp()
    ctx.synchronize()
    assert (d_dst.cpu().numpy().reshape(SH, SW) == src).all()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capturing_stream_is_refused(src):
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
        d_src = torch.from_numpy(src).to(dev)
        d_M = torch.from_numpy(H0.reshape(-1).copy()).to(dev)
        d_dst = torch.full((SH, SW), GUARD, dtype=torch.uint8, device=dev)
        d_val = torch.full((SH, SW), GUARD, dtype=torch.uint8, device=dev)
        d_info = torch.full((2,), -5, dtype=torch.int32, device=dev)
        d_pts = torch.full((16, 2), -7.5, dtype=torch.float32, device=dev)
        bufs = (d_src, d_M, d_dst, d_val, d_info, d_pts)
        torch.cuda.synchronize()
        prm = api.warp_params(0, BORDER)
        calls = [lambda: c.warp_dev(d_src.data_ptr(), SW, SH, SW, d_M.data_ptr(), prm, d_dst.data_ptr(), SW, SH, SW, d_val.data_ptr(), d_info.data_ptr()),
                 lambda: c.transform_points_dev(d_M.data_ptr(), 0, d_pts.data_ptr(), None, 16, d_pts.data_ptr()),
                 lambda: c.warp(src, H0, prm),
                 lambda: c.transform_points(H0, np.zeros((4, 2), np.float32))]
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
        assert (d_dst == GUARD).all() and (d_val == GUARD).all() and (d_info == -5).all() and (d_pts == -7.5).all()
        calls[0]()
        torch.cuda.synchronize()
        want = W.warp(src, H0, 0, BORDER)
        assert (d_dst.cpu().numpy() == want[0]).all() and (d_val.cpu().numpy() == want[1]).all()
        assert tuple(d_info.cpu().numpy()) == want[2:]
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        c.close()
        del bufs


# ---- 9. points ---------------------------------------------------------------------------------------------------------------

def seeded_points(n):
    rng = np.random.default_rng(900 + n)
    pts = np.stack([rng.uniform(-50, 700, n), rng.uniform(-50, 500, n)], 1).astype(np.float32)
    if n >= 63:
        pts[7] = (np.nan, 3.0)
        pts[20] = (np.inf, -np.inf)
        pts[41] = (10.0, 4.0)          # W = 0 under the model of test_points_nan_rules
    return pts


def dev_points(ctx, M, pts, flags=0, cap=None, n=None, in_place=False):
    """pm_transform_points_dev on pattern-filled buffers -> out with cap rows.  n: None = no count pointer."""
    import torch
    dev = torch.device("cuda", 0)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    cap = pts.shape[0] if cap is None else cap
    host = np.full((cap, 2), -7.5, np.float32)
    host[:min(cap, pts.shape[0])] = pts[:cap]
    d_pts = torch.from_numpy(host).to(dev)
    d_out = d_pts if in_place else torch.full((cap, 2), -7.5, dtype=torch.float32, device=dev)
    d_M = torch.from_numpy(np.ascontiguousarray(M, np.float64).reshape(-1)).to(dev)
    d_n = None if n is None else torch.full((1,), n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.transform_points_dev(d_M.data_ptr(), flags, d_pts.data_ptr(), None if d_n is None else d_n.data_ptr(), cap, d_out.data_ptr())
    ctx.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_points_bit_for_bit(ctx, n):
    pts = seeded_points(n)
    H = W.homography(6)
    for M, flags in ((H, 0), (H, W.INVERT), (H[:2], W.AFFINE), (H[:2], W.AFFINE | W.INVERT)):
        want = W.points(M, pts, flags)
        assert W.same_floats(dev_points(ctx, M, pts, flags), want), (n, flags)
        assert W.same_floats(dev_points(ctx, M, pts, flags, in_place=True), want), (n, flags, "in place")


def test_points_nan_rules(ctx):
    pts = seeded_points(300)
    M = np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -10.0]])
    got = dev_points(ctx, M, pts)
    assert W.same_floats(got, W.points(M, pts)) and np.isnan(got[[7, 20, 41]]).all() and np.isfinite(got[0]).all()
    for M, flags in ((np.zeros((3, 3)), 0), (np.zeros(6), W.AFFINE), (MODELS["NaN"], 0), (MODELS["singular"], W.INVERT)):
        assert np.isnan(dev_points(ctx, M, pts, flags)).all()


def test_points_count_protocol(ctx):
    pts = seeded_points(300)
    H = W.homography(6)
    want = W.points(H, pts)
    for n, rows in ((None, 300), (0, 0), (-1, 0), (170, 170), (300, 300), (1000, 300)):
        for in_place in (False, True):
            got = dev_points(ctx, H, pts, n=n, in_place=in_place)
            assert W.same_floats(got[:rows], want[:rows]), (n, in_place)
            rest = pts[rows:] if in_place else np.full((300 - rows, 2), -7.5, np.float32)
            assert W.same_floats(got[rows:], rest), (n, in_place)          # rows beyond the count are untouched


def test_nan_points_as_initial_guesses_give_status_2(ctx):
    import torch
    dev = torch.device("cuda", 0)
    img, kp = R.fixture()
    h, w = img.shape
    pts = kp[:64].copy()
    d_img = torch.from_numpy(img).to(dev)
    d_pts = torch.from_numpy(pts).to(dev)
    d_init = torch.zeros((64, 2), dtype=torch.float32, device=dev)
    d_out = torch.zeros((64, 2), dtype=torch.float32, device=dev)
    d_st = torch.full((64,), 9, dtype=torch.uint8, device=dev)
    M = np.eye(3)
    M[2] = (1.0, 0.0, -float(pts[5, 0]))                                  # W = x - x5: zero for point 5 alone (or its column mates)
    d_M = torch.from_numpy(M.reshape(-1)).to(dev)
    torch.cuda.synchronize()
    pyr = ctx.pyramid(w, h, 2)
    try:
        pyr.build_dev(d_img.data_ptr())
        ctx.transform_points_dev(d_M.data_ptr(), 0, d_pts.data_ptr(), None, 64, d_init.data_ptr())
        ctx.track_lk_dev(pyr, pyr, d_pts.data_ptr(), None, 64, api.lk_params(10, 2, flags=api.PM_LK_USE_INITIAL), d_out.data_ptr(), d_st.data_ptr(),
                         dinit_ptr=d_init.data_ptr())
        ctx.synchronize()
        init, st = d_init.cpu().numpy(), d_st.cpu().numpy()
        nan = np.isnan(init).any(axis=1)
        assert W.same_floats(init, W.points(M, pts)) and nan[5] and not nan.all()
        assert (st[nan] == 2).all()
    finally:
        ctx.synchronize()
        pyr.close()


# ---- 10. host forms ------------------------------------------------------------------------------------------------------------

def test_host_forms_equal_the_device_forms(ctx, src):
    for M, flags in ((H0, 0), (H0, W.INVERT | W.REPLICATE), (H0[:2], W.AFFINE), (np.zeros((3, 3)), 0)):
        for dw, dh in ((SW, SH), (65, 17), (3, 5)):
            got, _ = dev_warp(ctx, src, M, flags, dw=dw, dh=dh)
            dst, valid, status, n_valid = ctx.warp(src, M, api.warp_params(flags, BORDER), dw, dh)
            assert (dst.reshape(-1) == got[0][:dw * dh]).all() and (valid.reshape(-1) == got[1][:dw * dh]).all()
            assert (status, n_valid) == got[2:]
    padded = np.ascontiguousarray(np.pad(src, ((0, 0), (0, 6))))
    assert (ctx.warp(padded, H0, api.warp_params(0, BORDER), sw=SW)[0] == W.warp(src, H0, 0, BORDER)[0]).all()
    pts = seeded_points(300)
    for M, flags in ((H0, 0), (H0, W.INVERT), (H0[:2], W.AFFINE)):
        assert W.same_floats(ctx.transform_points(M, pts, flags), dev_points(ctx, M, pts, flags))


# ---- 11. the chain -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["affine", "homography"])
def test_chain_track_estimate_refine_warp_on_one_stream(ctx, model):
    """pm_pyramid_build_dev x 2 -> pm_corners_dev -> pm_track_lk_gather_dev -> RANSAC + refinement -> pm_warp_dev of frame 2 by
    the model as it lies on the device, on the context's stream with one synchronisation at the end."""
    import torch
    dev = torch.device("cuda", 0)
    img1 = R.fixture()[0]
    img2 = D.rotate_frame(img1, 3)
    h, w = img1.shape
    cap = 512
    d_img1, d_img2 = torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev)
    d_kp = torch.zeros((cap, 2), dtype=torch.float32, device=dev)
    d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    d_xy1 = torch.zeros((cap, 2), dtype=torch.float32, device=dev)
    d_xy2 = torch.zeros((cap, 2), dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    d_key = torch.zeros(1, dtype=torch.int64, device=dev)
    d_M = torch.zeros(9, dtype=torch.float64, device=dev)
    d_Mr = torch.zeros(9, dtype=torch.float64, device=dev)
    d_mask = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_ninl = torch.zeros(1, dtype=torch.int32, device=dev)
    d_rinfo = torch.zeros(32, dtype=torch.uint8, device=dev)
    d_dst = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    d_val = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    d_info = torch.zeros(2, dtype=torch.int32, device=dev)
    p1, p2 = ctx.pyramid(w, h, 3), ctx.pyramid(w, h, 3)
    torch.cuda.synchronize()
    try:
        p1.build_dev(d_img1.data_ptr())
        p2.build_dev(d_img2.data_ptr())
        ctx.corners_dev(p1, api.corner_params(), cap, d_kp.data_ptr(), d_n.data_ptr())
        ctx.track_lk_gather_dev(p1, p2, d_kp.data_ptr(), d_n.data_ptr(), cap, api.lk_params(10, 3, fb_thresh=0.5), d_xy1.data_ptr(),
                                d_xy2.data_ptr(), d_cnt.data_ptr())
        view = api.PointsView(d_xy1.data_ptr(), d_xy2.data_ptr(), d_cnt.data_ptr(), 1, cap, 0, 1, 0)
        if model == "affine":
            flags = W.AFFINE
            ctx.ransac_affine_run_dev(view, 0, 500, 2.0, 0x5EED, d_key.data_ptr(), d_M.data_ptr(), d_mask.data_ptr(), cap, d_ninl.data_ptr(),
                                      model=api.PM_AFFINE_PARTIAL)
            ctx.affine_refine_dev(view, d_mask.data_ptr(), d_M.data_ptr(), d_Mr.data_ptr(), d_rinfo.data_ptr(), model=api.PM_AFFINE_PARTIAL)
        else:
            flags = 0
            ctx.ransac_homography_run_dev(view, 0, 500, 2.0, 0x5EED, d_key.data_ptr(), d_M.data_ptr(), d_mask.data_ptr(), cap, d_ninl.data_ptr())
            ctx.homography_refine_dev(view, d_mask.data_ptr(), d_M.data_ptr(), 10, d_Mr.data_ptr(), d_rinfo.data_ptr())
        ctx.warp_dev(d_img2.data_ptr(), w, h, w, d_Mr.data_ptr(), api.warp_params(flags, 0), d_dst.data_ptr(), w, h, w, d_val.data_ptr(),
                     d_info.data_ptr())
        ctx.synchronize()
        cnt, ninl = int(d_cnt.item()), int(d_ninl.item())
        M = d_Mr.cpu().numpy()[:6 if model == "affine" else 9]
        dst, valid, info = d_dst.cpu().numpy(), d_val.cpu().numpy(), d_info.cpu().numpy()
        want = W.warp(img2, M, flags, 0)
        assert (dst == want[0]).all() and (valid == want[1]).all() and (int(info[0]), int(info[1])) == want[2:] and want[2] == 0
        v = valid == 1
        assert v.sum() * 2 > v.size
        before = np.abs(img2.astype(np.int32) - img1.astype(np.int32))[v].mean()
        after = np.abs(dst.astype(np.int32) - img1.astype(np.int32))[v].mean()
        print("chain (%s): %d tracked, %d inliers, %d valid pixels, mean absolute difference %.3f -> %.3f" % (model, cnt, ninl, v.sum(), before, after))
        assert after < before
    finally:
        ctx.synchronize()
        p1.close()
        p2.close()
