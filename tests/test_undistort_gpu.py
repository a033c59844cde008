"""GPU: pm_undistort[_dev], pm_undistort_map_dev, pm_remap[_dev], pm_undistort_points[_dev] and pm_distort_points[_dev] (SPEC
S79-S83) against the plain-C restatement tests/undistort_ref.c, which tests/test_undistort_cpu.py pins on the CPU.  Bytes, masks,
counts and map entries are integers that are a function of the inputs alone, and the points are sequences of single fp64
operations: every comparison is bit for bit, there is no tolerance anywhere.  Shapes are the smallest that reach each edge of the
kernels: fewer pixels than a thread's four, one 64 x 16 tile exactly, one past it in both directions, odd strides and base
addresses; point counts around one wave and one workgroup."""
import gc

import numpy as np
import pytest

import undistort_ref as U
from points_matching_amd import api, synth

pytestmark = pytest.mark.gpu
GUARD = 0xA5
SW, SH = U.SW, U.SH
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
    return U.random_source()


def dev_undistort(ctx, src, lens=U.LENS, R=None, K_new=None, flags=0, border=BORDER, dw=None, dh=None, dstride=None, offset=0, sw=None,
                  want_valid=True, want_info=True, K=U.CAM, via_map=False):
    """pm_undistort_dev (or pm_undistort_map_dev + pm_remap_dev) on guarded torch buffers -> (whole dst buffer, whole valid buffer,
    status, n_valid) and the same four from the C restatement written into equally guarded host buffers."""
    import torch
    dev = torch.device("cuda", 0)
    src = np.ascontiguousarray(src, np.uint8)
    sh, sstride = src.shape
    sw = sstride if sw is None else sw
    dw = sw if dw is None else dw
    dh = sh if dh is None else dh
    dstride = dw if dstride is None else dstride
    want_dst = np.full(offset + dh * dstride + 64, GUARD, np.uint8)
    want_val = np.full(offset + dh * dw + 64, GUARD, np.uint8)
    ref = U.undistort(src, K, lens, R, K_new, flags, border, dw, dh, sw, dst=want_dst[offset:offset + dh * dstride].reshape(dh, dstride),
                      dstride=dstride)
    want_val[offset:offset + dh * dw] = ref[1].reshape(-1)
    d_src = torch.from_numpy(src).to(dev)
    d_dst = torch.full((want_dst.size,), GUARD, dtype=torch.uint8, device=dev)
    d_val = torch.full((want_val.size,), GUARD, dtype=torch.uint8, device=dev)
    d_info = torch.full((2,), -9, dtype=torch.int32, device=dev)
    d_map = torch.full((dh * dw * 2 + 16,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    prm = api.warp_params(flags, border)
    tail = (d_dst.data_ptr() + offset, dw, dh, dstride, d_val.data_ptr() + offset if want_valid else None, d_info.data_ptr() if want_info else None)
    if via_map:
        ctx.undistort_map_dev(K, lens, R, K_new, dw, dh, d_map.data_ptr())
        ctx.remap_dev(d_src.data_ptr(), sw, sh, sstride, d_map.data_ptr(), prm, *tail)
    else:
        ctx.undistort_dev(d_src.data_ptr(), sw, sh, sstride, K, lens, R, K_new, prm, *tail)
    ctx.synchronize()
    info = d_info.cpu().numpy()
    got = (d_dst.cpu().numpy(), d_val.cpu().numpy(), int(info[0]), int(info[1]))
    if via_map:
        m = d_map.cpu().numpy()
        assert (m[dh * dw * 2:] == 0x5A5A5A5A).all()
        assert (m[:dh * dw * 2].reshape(dh, dw, 2) == U.make_map(K, lens, R, K_new, dw, dh)).all()
    return got, (want_dst, want_val, 0, ref[2])


def check(ctx, src, **kw):
    got, want = dev_undistort(ctx, src, **kw)
    assert (got[0] == want[0]).all(), ("dst", kw, int((got[0] != want[0]).sum()))
    assert (got[1] == want[1]).all(), ("valid", kw, int((got[1] != want[1]).sum()))
    assert got[2:] == want[2:], (kw, got[2:], want[2:])
    return want


# ---- 1. shapes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, U.REPLICATE])
@pytest.mark.parametrize("dw,dh,dstride", [(1, 1, 1), (3, 5, 3), (64, 16, 64), (65, 17, 65), (67, 35, 71)])
def test_output_shapes(ctx, src, dw, dh, dstride, flags):
    check(ctx, src, flags=flags, dw=dw, dh=dh, dstride=dstride)
    check(ctx, src, flags=flags, dw=dw, dh=dh, dstride=dstride, via_map=True)


def test_the_lens_moves_the_corners_by_more_than_two_pixels():
    ok, sx, sy = U.source_position(U.CAM, U.LENS, None, None, 0, 0)
    assert ok and sx > 2.0 and sy > 1.0 and np.hypot(sx, sy) > 2.0


@pytest.mark.parametrize("flags", [0, U.REPLICATE])
def test_odd_base_addresses_leave_the_surroundings_untouched(ctx, src, flags):
    for offset in (1, 2, 3):
        for via_map in (False, True):
            want = check(ctx, src, R=U.ROT, flags=flags, dstride=71, offset=offset, via_map=via_map)          # the border is in play
            assert (want[0][:offset] == GUARD).all() and (want[0][-64:] == GUARD).all() and 0 < want[3] < SW * SH


def test_source_stride_above_width(ctx, src):
    padded = np.ascontiguousarray(np.pad(src, ((0, 0), (0, 6)), constant_values=201))          # a source stride of 73
    for flags in (0, U.REPLICATE):
        a = check(ctx, padded, flags=flags, sw=SW)
        b = check(ctx, src, flags=flags)
        assert (a[0] == b[0]).all() and a[3] == b[3]
        check(ctx, padded, flags=flags, sw=SW, via_map=True)


def test_without_valid_or_info(ctx, src):
    for via_map in (False, True):
        got, want = dev_undistort(ctx, src, want_valid=False, want_info=False, via_map=via_map)
        assert (got[0] == want[0]).all() and (got[1] == GUARD).all() and got[2:] == (-9, -9)


def test_tiny_sources(ctx):
    one, two = np.array([[200]], np.uint8), np.array([[10, 250], [90, 170]], np.uint8)
    K1, K2 = (4.0, 4.0, 0.0, 0.0), (4.0, 4.0, 0.5, 0.5)
    K9 = (16.0, 16.0, 4.0, 4.0)                                        # a 9 x 9 output over and around the source
    for flags in (0, U.REPLICATE):
        for via_map in (False, True):
            check(ctx, one, K=K1, K_new=K9, flags=flags, dw=9, dh=9, via_map=via_map)
            check(ctx, two, K=K2, K_new=K9, flags=flags, dw=9, dh=9, via_map=via_map)
            assert check(ctx, one, K=K1, lens=None, flags=flags, via_map=via_map)[3] == 1


# ---- 2. the wave-uniform branches ------------------------------------------------------------------------------------------

BRANCHES = {
    "zero lens": dict(lens=(0.0,) * 5),
    "negative-zero lens": dict(lens=(-0.0, 0.0, -0.0, 0.0, 0.0)),
    "lens = NULL": dict(lens=None),
    "lens = NULL, R": dict(lens=None, R=U.ROT),
    "R = NULL": dict(R=None),
    "R": dict(R=U.ROT),
    "R = identity given": dict(R=np.eye(3)),
    "K_new, other size": dict(K_new=U.CAM_NEW, dw=90, dh=50),
    "K_new and R, other size": dict(K_new=U.CAM_NEW, R=U.ROT, dw=50, dh=41),
    "zero lens, K_new": dict(lens=(0.0,) * 5, K_new=U.CAM_NEW, dw=90, dh=50),
    "rad <= 0": dict(lens=(-2.0, 0.0, 0.0, 0.0, 0.0), K_new=(30.0, 30.0, 33.0, 17.0)),
    "Z <= 0": dict(R=U.rotation(0.0, 80.0, 0.0), K_new=(30.0, 30.0, 33.0, 17.0)),
    "far away": dict(lens=None, K_new=(1e-9, 1e-9, 33.0, 17.0)),
    "k3 and tangential": dict(lens=(0.12, -0.05, 4e-3, -3e-3, 0.02)),
}


@pytest.mark.parametrize("name", sorted(BRANCHES))
def test_branches_against_the_one_restatement(ctx, src, name):
    for flags in (0, U.REPLICATE):
        fused = check(ctx, src, flags=flags, **BRANCHES[name])
        mapped = check(ctx, src, flags=flags, via_map=True, **BRANCHES[name])          # also: the map equals the restatement's
        assert (fused[0] == mapped[0]).all() and (fused[1] == mapped[1]).all() and fused[3] == mapped[3]
        if name in ("rad <= 0", "Z <= 0", "far away"):
            assert fused[3] < SW * SH
    if name.startswith(("zero lens", "negative-zero", "lens = NULL")) and "R" not in BRANCHES[name] and "K_new" not in BRANCHES[name]:
        assert (check(ctx, src, **BRANCHES[name])[0][:SW * SH].reshape(SH, SW) == src).all()


def test_fused_equals_map_then_remap_on_the_device(ctx, src):
    """Device against device: bytes, valid mask and n_valid of one launch and of the two."""
    for kw in (dict(), dict(R=U.ROT, K_new=U.CAM_NEW, dw=90, dh=50), BRANCHES["rad <= 0"], BRANCHES["Z <= 0"]):
        for flags in (0, U.REPLICATE):
            a, _ = dev_undistort(ctx, src, flags=flags, **kw)
            b, _ = dev_undistort(ctx, src, flags=flags, via_map=True, **kw)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2:] == b[2:]


def test_extreme_map_through_remap(ctx, src):
    import torch
    dev = torch.device("cuda", 0)
    m = U.extreme_map()
    dh, dw = m.shape[:2]
    d_src = torch.from_numpy(src).to(dev)
    d_map = torch.from_numpy(m).to(dev)
    for flags in (0, U.REPLICATE):
        want = U.remap(src, m, flags, 200)
        d_dst = torch.full((dh * dw + 64,), GUARD, dtype=torch.uint8, device=dev)
        d_val = torch.full((dh * dw + 64,), GUARD, dtype=torch.uint8, device=dev)
        d_info = torch.full((2,), -9, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.remap_dev(d_src.data_ptr(), SW, SH, SW, d_map.data_ptr(), api.warp_params(flags, 200), d_dst.data_ptr(), dw, dh, dw, d_val.data_ptr(),
                      d_info.data_ptr())
        ctx.synchronize()
        dst, val = d_dst.cpu().numpy(), d_val.cpu().numpy()
        assert (dst[:dh * dw].reshape(dh, dw) == want[0]).all() and (val[:dh * dw].reshape(dh, dw) == want[1]).all()
        assert (dst[dh * dw:] == GUARD).all() and (val[dh * dw:] == GUARD).all()
        assert tuple(d_info.cpu().numpy()) == (0, want[2]) and not want[1][:, :5].any()
        host = ctx.remap(src, m, api.warp_params(flags, 200))
        assert (host[0] == want[0]).all() and (host[1] == want[1]).all() and host[2] == want[2]


# ---- 3. points ---------------------------------------------------------------------------------------------------------------

def dev_points(ctx, pts, lens=U.LENS, R=None, K_new=None, cap=None, n=None, in_place=False, iters=U.ITERS, tol_px=U.TOL_PX, forward=False):
    """pm_undistort_points_dev (forward: pm_distort_points_dev) on pattern-filled buffers -> out with cap rows.  n: None = no
    count pointer."""
    import torch
    dev = torch.device("cuda", 0)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    cap = pts.shape[0] if cap is None else cap
    host = np.full((cap, 2), -7.5, np.float32)
    host[:min(cap, pts.shape[0])] = pts[:cap]
    d_pts = torch.from_numpy(host).to(dev)
    d_out = d_pts if in_place else torch.full((cap, 2), -7.5, dtype=torch.float32, device=dev)
    d_n = None if n is None else torch.full((1,), n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    dn = None if d_n is None else d_n.data_ptr()
    if forward:
        ctx.distort_points_dev(U.CAM, lens, R, K_new, d_pts.data_ptr(), dn, cap, d_out.data_ptr())
    else:
        ctx.undistort_points_dev(U.CAM, lens, R, K_new, iters, tol_px, d_pts.data_ptr(), dn, cap, d_out.data_ptr())
    ctx.synchronize()
    return d_out.cpu().numpy()


POINT_MODELS = [(U.LENS, None, None), (U.LENS, U.ROT, U.CAM_NEW), (None, None, None), (None, U.ROT, None), ((0.0,) * 5, None, U.CAM_NEW)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_points_bit_for_bit(ctx, n):
    pts = U.seeded_points(n)
    for lens, R, K_new in POINT_MODELS:
        for iters, tol in ((U.ITERS, U.TOL_PX), (1, 1e-3), (50, 1e-9)):
            want = U.undistort_points(U.CAM, lens, R, K_new, pts, iters, tol)
            assert U.same_floats(dev_points(ctx, pts, lens, R, K_new, iters=iters, tol_px=tol), want), (n, iters)
            assert U.same_floats(dev_points(ctx, pts, lens, R, K_new, iters=iters, tol_px=tol, in_place=True), want), (n, iters, "in place")
        want = U.distort_points(U.CAM, lens, R, K_new, pts)
        assert U.same_floats(dev_points(ctx, pts, lens, R, K_new, forward=True), want), n
        assert U.same_floats(dev_points(ctx, pts, lens, R, K_new, forward=True, in_place=True), want), (n, "in place")


def test_rejected_and_non_finite_rows_are_nan(ctx):
    pts = U.seeded_points(257)
    got = dev_points(ctx, pts)
    assert np.isnan(got[[7, 20, 33, 41]]).all() and np.isfinite(np.delete(got, [7, 20, 33, 41], axis=0)).all()
    one = dev_points(ctx, pts, iters=1)                                 # one round: the gate rejects what has not converged
    assert U.same_floats(one, U.undistort_points(U.CAM, U.LENS, None, None, pts, 1, U.TOL_PX))
    assert np.isnan(one).all(axis=1).sum() > np.isnan(got).all(axis=1).sum()
    fwd = dev_points(ctx, pts, forward=True)
    assert np.isnan(fwd[[7, 20, 33]]).all() and np.isfinite(fwd[0]).all()
    strong = dev_points(ctx, np.array([[93.0, 17.0], [63.0, 17.0]], np.float32), lens=(-2.0, 0.0, 0.0, 0.0, 0.0), forward=True)
    assert np.isnan(strong[0]).all() and np.isfinite(strong[1]).all()          # rad <= 0
    behind = dev_points(ctx, pts, lens=None, R=U.rotation(0.0, 100.0, 0.0))
    assert U.same_floats(behind, U.undistort_points(U.CAM, None, U.rotation(0.0, 100.0, 0.0), None, pts)) and np.isnan(behind).any()


def test_points_count_protocol(ctx):
    pts = U.seeded_points(257)
    for forward in (False, True):
        want = U.distort_points(U.CAM, U.LENS, None, None, pts) if forward else U.undistort_points(U.CAM, U.LENS, None, None, pts)
        for n, rows in ((None, 257), (0, 0), (-1, 0), (170, 170), (257, 257), (1000, 257)):
            for in_place in (False, True):
                got = dev_points(ctx, pts, n=n, in_place=in_place, forward=forward)
                assert U.same_floats(got[:rows], want[:rows]), (n, in_place)
                rest = pts[rows:] if in_place else np.full((257 - rows, 2), -7.5, np.float32)
                assert U.same_floats(got[rows:], rest), (n, in_place)          # rows beyond the count keep their bytes
        got = dev_points(ctx, pts[:100], cap=300, n=100, forward=forward)          # a count below a larger capacity
        assert U.same_floats(got[:100], want[:100]) and (got[100:] == -7.5).all()


def test_nan_points_as_initial_guesses_give_status_2(ctx):
    import torch
    import lk_ref as R
    dev = torch.device("cuda", 0)
    img, kp = R.fixture()
    h, w = img.shape
    pts = kp[:64].copy()
    pts[5] = (4.0 * w, -3.0 * h)                                         # far outside the field: rejected
    K = (0.8 * w, 0.8 * w, w / 2.0, h / 2.0)
    d_img = torch.from_numpy(img).to(dev)
    d_pts = torch.from_numpy(kp[:64].copy()).to(dev)
    d_init = torch.from_numpy(pts).to(dev)
    d_out = torch.zeros((64, 2), dtype=torch.float32, device=dev)
    d_st = torch.full((64,), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    pyr = ctx.pyramid(w, h, 2)
    try:
        pyr.build_dev(d_img.data_ptr())
        ctx.undistort_points_dev(K, U.MODERATE, None, None, U.ITERS, U.TOL_PX, d_init.data_ptr(), None, 64, d_init.data_ptr())
        ctx.track_lk_dev(pyr, pyr, d_pts.data_ptr(), None, 64, api.lk_params(10, 2, flags=api.PM_LK_USE_INITIAL), d_out.data_ptr(), d_st.data_ptr(),
                         dinit_ptr=d_init.data_ptr())
        ctx.synchronize()
        init, st = d_init.cpu().numpy(), d_st.cpu().numpy()
        nan = np.isnan(init).any(axis=1)
        assert U.same_floats(init, U.undistort_points(K, U.MODERATE, None, None, pts)) and nan[5] and not nan.all()
        assert (st[nan] == 2).all()
    finally:
        ctx.synchronize()
        pyr.close()


# ---- 4. arguments, capture ---------------------------------------------------------------------------------------------------

def test_argument_statuses(ctx, src):
    import torch
    dev = torch.device("cuda", 0)
    d_buf = torch.zeros(2 * SW * SH + SW * SH * 8, dtype=torch.uint8, device=dev)
    d_src = torch.from_numpy(src).to(dev)
    d_dst = torch.full((SH * SW,), GUARD, dtype=torch.uint8, device=dev)
    d_map = torch.full((SH * SW * 2 + 2,), GUARD, dtype=torch.int32, device=dev)
    d_pts = torch.full((8, 2), -7.5, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    nan, inf = float("nan"), float("inf")

    def und(s=d_src.data_ptr(), sw=SW, sh=SH, ss=SW, K=U.CAM, lens=U.LENS, R=None, Kn=None, prm=api.warp_params(), d=d_dst.data_ptr(), dw=SW, dh=SH,
            ds=SW):
        ctx.undistort_dev(s, sw, sh, ss, K, lens, R, Kn, prm, d, dw, dh, ds)

    def rmp(s=d_src.data_ptr(), sw=SW, sh=SH, ss=SW, m=d_map.data_ptr(), prm=api.warp_params(), d=d_dst.data_ptr(), dw=SW, dh=SH, ds=SW):
        ctx.remap_dev(s, sw, sh, ss, m, prm, d, dw, dh, ds)

    def mp(K=U.CAM, lens=U.LENS, R=None, Kn=None, dw=SW, dh=SH, m=d_map.data_ptr()):
        ctx.undistort_map_dev(K, lens, R, Kn, dw, dh, m)

    def upt(K=U.CAM, lens=U.LENS, R=None, Kn=None, iters=10, tol=1e-3, p=d_pts.data_ptr(), cap=8, out=d_pts.data_ptr()):
        ctx.undistort_points_dev(K, lens, R, Kn, iters, tol, p, None, cap, out)

    def dpt(K=U.CAM, lens=U.LENS, R=None, Kn=None, p=d_pts.data_ptr(), cap=8, out=d_pts.data_ptr()):
        ctx.distort_points_dev(K, lens, R, Kn, p, None, cap, out)

    bad_reserved = api.warp_params()
    bad_reserved.reserved[1] = 1
    bad_R = np.eye(3)
    bad_R[1, 2] = nan
    base = d_buf.data_ptr()
    mbase = (base + 2 * SW * SH + 7) & ~7
    invalid = [lambda: und(s=0), lambda: und(prm=None), lambda: und(d=0),
               lambda: und(prm=api.warp_params(1)), lambda: und(prm=api.warp_params(4)), lambda: und(prm=api.warp_params(8)),
               lambda: und(prm=api.warp_params(0, 256)), lambda: und(prm=api.warp_params(0, -1)), lambda: und(prm=bad_reserved),
               lambda: und(sw=0), lambda: und(sh=0), lambda: und(dw=0), lambda: und(dh=-1), lambda: und(ss=SW - 1), lambda: und(ds=SW - 1),
               lambda: und(s=base, d=base),                                        # the same image
               lambda: und(s=base, d=base + SW * SH - 1),                          # the last source byte is the first of dst
               lambda: und(s=base + SW * SH - 1, d=base),
               lambda: und(K=(0.0, 60.0, 33.0, 17.0)), lambda: und(K=(60.0, -1.0, 33.0, 17.0)), lambda: und(K=(60.0, 60.0, nan, 17.0)),
               lambda: und(K=(inf, 60.0, 33.0, 17.0)), lambda: und(Kn=(60.0, 0.0, 33.0, 17.0)), lambda: und(Kn=(60.0, 60.0, 33.0, inf)),
               lambda: und(lens=(nan, 0, 0, 0, 0)), lambda: und(lens=(0, 0, 0, 0, inf)), lambda: und(lens=(0, 0, -inf, 0, 0)), lambda: und(R=bad_R),
               lambda: rmp(s=0), lambda: rmp(m=0), lambda: rmp(prm=None), lambda: rmp(d=0), lambda: rmp(prm=api.warp_params(1)),
               lambda: rmp(prm=api.warp_params(0, 256)), lambda: rmp(prm=bad_reserved), lambda: rmp(sw=0), lambda: rmp(dh=0), lambda: rmp(ss=SW - 1),
               lambda: rmp(ds=SW - 1), lambda: rmp(s=base, d=base), lambda: rmp(s=base, d=base + SW * SH - 1),
               lambda: rmp(m=d_map.data_ptr() + 4),                                # not 8-byte aligned
               lambda: rmp(m=mbase, d=mbase + SW * SH * 8 - 1), lambda: rmp(m=mbase, d=mbase),          # map and dst overlap
               lambda: mp(m=0), lambda: mp(dw=0), lambda: mp(dh=-3), lambda: mp(m=d_map.data_ptr() + 4), lambda: mp(K=(60.0, 60.0, 33.0, nan)),
               lambda: mp(Kn=(-60.0, 60.0, 33.0, 17.0)), lambda: mp(lens=(0, nan, 0, 0, 0)), lambda: mp(R=bad_R),
               lambda: upt(p=0), lambda: upt(out=0), lambda: upt(cap=-1), lambda: upt(iters=0), lambda: upt(iters=51), lambda: upt(iters=-4),
               lambda: upt(tol=0.0), lambda: upt(tol=-1e-3), lambda: upt(tol=nan), lambda: upt(tol=inf), lambda: upt(K=(60.0, 0.0, 33.0, 17.0)),
               lambda: upt(Kn=(60.0, 60.0, nan, 17.0)), lambda: upt(lens=(0, 0, 0, nan, 0)), lambda: upt(R=bad_R),
               lambda: dpt(p=0), lambda: dpt(out=0), lambda: dpt(cap=-1), lambda: dpt(K=(0.0, 60.0, 33.0, 17.0)), lambda: dpt(Kn=(60.0, inf, 33.0, 17.0)),
               lambda: dpt(lens=(inf, 0, 0, 0, 0)), lambda: dpt(R=bad_R)]
    for k, call in enumerate(invalid):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_INVALID, (k, str(e.value))
    unsupported = [lambda: und(sw=10001, sh=10000, ss=10001), lambda: und(dw=10001, dh=10000, ds=10001), lambda: rmp(sw=10001, sh=10000, ss=10001),
                   lambda: rmp(dw=10001, dh=10000, ds=10001), lambda: mp(dw=10001, dh=10000), lambda: upt(cap=0), lambda: dpt(cap=0)]
    for k, call in enumerate(unsupported):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_UNSUPPORTED, (k, str(e.value))
    z = np.zeros((4, 2), np.float32)
    for call in (lambda: ctx.undistort(src, U.CAM, U.LENS, prm=api.warp_params(16)), lambda: ctx.undistort(src, U.CAM, U.LENS, prm=api.warp_params(0, 300)),
                 lambda: ctx.undistort(src, (0.0, 1.0, 0.0, 0.0), U.LENS), lambda: ctx.undistort(src, U.CAM, (nan, 0, 0, 0, 0)),
                 lambda: ctx.remap(src, U.extreme_map(), api.warp_params(1)),
                 lambda: ctx.undistort_points(U.CAM, U.LENS, z, iters=0), lambda: ctx.undistort_points(U.CAM, U.LENS, z, tol_px=0.0),
                 lambda: ctx.undistort_points(U.CAM, U.LENS, z, R=bad_R), lambda: ctx.distort_points(U.CAM, (0, 0, 0, 0, nan), z)):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_INVALID
    for call in (lambda: ctx.undistort_points(U.CAM, U.LENS, np.zeros((0, 2), np.float32)), lambda: ctx.distort_points(U.CAM, U.LENS, np.zeros((0, 2), np.float32))):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_UNSUPPORTED
    ctx.synchronize()
    assert (d_dst == GUARD).all() and (d_map == GUARD).all() and (d_pts == -7.5).all()          # nothing was launched
    und(s=base, d=base + SW * SH)                                                    # adjacent ranges are fine
    und(lens=None)
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
        d_dst = torch.full((SH, SW), GUARD, dtype=torch.uint8, device=dev)
        d_val = torch.full((SH, SW), GUARD, dtype=torch.uint8, device=dev)
        d_info = torch.full((2,), -5, dtype=torch.int32, device=dev)
        d_map = torch.full((SH, SW, 2), -5, dtype=torch.int32, device=dev)
        d_pts = torch.full((16, 2), -7.5, dtype=torch.float32, device=dev)
        bufs = (d_src, d_dst, d_val, d_info, d_map, d_pts)
        torch.cuda.synchronize()
        prm = api.warp_params(0, BORDER)
        z = np.zeros((4, 2), np.float32)
        calls = [lambda: c.undistort_dev(d_src.data_ptr(), SW, SH, SW, U.CAM, U.LENS, None, None, prm, d_dst.data_ptr(), SW, SH, SW, d_val.data_ptr(),
                                         d_info.data_ptr()),
                 lambda: c.undistort_map_dev(U.CAM, U.LENS, None, None, SW, SH, d_map.data_ptr()),
                 lambda: c.remap_dev(d_src.data_ptr(), SW, SH, SW, d_map.data_ptr(), prm, d_dst.data_ptr(), SW, SH, SW, d_val.data_ptr(), d_info.data_ptr()),
                 lambda: c.undistort_points_dev(U.CAM, U.LENS, None, None, U.ITERS, U.TOL_PX, d_pts.data_ptr(), None, 16, d_pts.data_ptr()),
                 lambda: c.distort_points_dev(U.CAM, U.LENS, None, None, d_pts.data_ptr(), None, 16, d_pts.data_ptr()),
                 lambda: c.undistort(src, U.CAM, U.LENS, prm=prm),
                 lambda: c.remap(src, U.extreme_map(), prm),
                 lambda: c.undistort_points(U.CAM, U.LENS, z),
                 lambda: c.distort_points(U.CAM, U.LENS, z)]
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
        assert (d_dst == GUARD).all() and (d_val == GUARD).all() and (d_info == -5).all() and (d_map == -5).all() and (d_pts == -7.5).all()
        calls[0]()
        torch.cuda.synchronize()
        want = U.undistort(src, U.CAM, U.LENS, None, None, 0, BORDER)
        assert (d_dst.cpu().numpy() == want[0]).all() and (d_val.cpu().numpy() == want[1]).all()
        assert tuple(d_info.cpu().numpy()) == (0, want[2])
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        c.close()
        del bufs


# ---- 5. host forms ------------------------------------------------------------------------------------------------------------

def test_host_forms_equal_the_device_forms(ctx, src):
    for kw in (dict(), dict(R=U.ROT, K_new=U.CAM_NEW), dict(lens=None), BRANCHES["rad <= 0"]):
        for flags in (0, U.REPLICATE):
            for dw, dh in ((SW, SH), (65, 17), (3, 5)):
                got, _ = dev_undistort(ctx, src, flags=flags, dw=dw, dh=dh, **kw)
                dst, valid, n_valid = ctx.undistort(src, U.CAM, kw.get("lens", U.LENS), kw.get("R"), kw.get("K_new"), api.warp_params(flags, BORDER), dw, dh)
                assert (dst.reshape(-1) == got[0][:dw * dh]).all() and (valid.reshape(-1) == got[1][:dw * dh]).all() and n_valid == got[3]
                m = U.make_map(U.CAM, kw.get("lens", U.LENS), kw.get("R"), kw.get("K_new"), dw, dh)
                r = ctx.remap(src, m, api.warp_params(flags, BORDER))
                assert (r[0] == dst).all() and (r[1] == valid).all() and r[2] == n_valid
    padded = np.ascontiguousarray(np.pad(src, ((0, 0), (0, 6))))
    assert (ctx.undistort(padded, U.CAM, U.LENS, prm=api.warp_params(0, BORDER), sw=SW)[0] == U.undistort(src, U.CAM, U.LENS, border=BORDER)[0]).all()
    pts = U.seeded_points(257)
    for lens, R, K_new in POINT_MODELS:
        assert U.same_floats(ctx.undistort_points(U.CAM, lens, pts, R, K_new, U.ITERS, U.TOL_PX), dev_points(ctx, pts, lens, R, K_new))
        assert U.same_floats(ctx.distort_points(U.CAM, lens, pts, R, K_new), dev_points(ctx, pts, lens, R, K_new, forward=True))


def test_host_form_returns_the_bytes_between_the_rows_unchanged(ctx, src):
    dst = np.full((SH, 71), GUARD, np.uint8)
    out, valid, n_valid = ctx.undistort(src, U.CAM, U.LENS, prm=api.warp_params(0, BORDER), dst=dst)
    want = U.undistort(src, U.CAM, U.LENS, border=BORDER)
    assert out is dst and (dst[:, :SW] == want[0]).all() and (dst[:, SW:] == GUARD).all() and (valid == want[1]).all() and n_valid == want[2]


# ---- 6. the chain --------------------------------------------------------------------------------------------------------------

CHAIN_LENS = (-0.25, 0.06, 8e-4, -5e-4, 0.0)
CHAIN = dict(seed=0, width=640, height=480, focal=420.0, noise_px=0.3, outlier_frac=0.2, angle=0.15)
CHAIN_HYP, CHAIN_THRESH, CHAIN_SEED = 200, 1.0, 0x5EED


def _rot_deg(A, B):
    return float(np.degrees(np.arccos(np.clip((np.trace(A @ B.T) - 1.0) / 2.0, -1.0, 1.0))))


def _bits_equal(a, b):
    return (np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64) == np.ascontiguousarray(b, np.float64).reshape(-1).view(np.uint64)).all()


def test_chain_undistort_essential_pose_on_one_stream(ctx):
    """300 correspondences of synth.calibrated_view_wide (640 x 480, focal 420, a rotation of 0.15 rad, 0.3 px noise, 20 %
    outliers), their pixels distorted by the numpy forward model (up to 47 px at the corners); the device count is written
    directly.  pm_undistort_points_dev in place on both arrays -> pm_ransac_essential_run_dev -> pm_recover_pose_dev on the
    context's stream, one synchronisation; against the host forms fed with the restatement's undistorted points, bit for bit.
    With the CPU restatements alone (tests/essential_ref.c, samples [0, 200), 1 px, seed 0x5EED) the rotation error against
    the truth is 0.0458 degrees on the undistorted points (239 inliers) and 1.3748 degrees on the raw distorted ones (110)."""
    import torch
    dev = torch.device("cuda", 0)
    xy1, xy2, K, Rg, tg, X, truth = synth.calibrated_view_wide(300, **CHAIN)
    Kc = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    d1, d2 = U.np_distort_points(Kc, CHAIN_LENS, None, None, xy1), U.np_distort_points(Kc, CHAIN_LENS, None, None, xy2)
    assert np.isfinite(d1).all() and np.isfinite(d2).all() and np.abs(d1 - xy1).max() > 10.0
    u1, u2 = U.undistort_points(Kc, CHAIN_LENS, None, None, d1), U.undistort_points(Kc, CHAIN_LENS, None, None, d2)
    assert np.isfinite(u1).all() and np.isfinite(u2).all()
    n, cap = 300, 320
    errs = {}
    for name, undo in (("undistorted", True), ("raw", False)):
        h1, h2 = np.full((cap, 2), -7.5, np.float32), np.full((cap, 2), -7.5, np.float32)
        h1[:n], h2[:n] = d1, d2
        d_xy1, d_xy2 = torch.from_numpy(h1).to(dev), torch.from_numpy(h2).to(dev)
        d_n = torch.full((1,), n, dtype=torch.int32, device=dev)
        k = torch.zeros(1, dtype=torch.int64, device=dev)
        E = torch.zeros(9, dtype=torch.float64, device=dev)
        m = torch.zeros(cap, dtype=torch.uint8, device=dev)
        c = torch.zeros(1, dtype=torch.int32, device=dev)
        Rd, td = torch.zeros(9, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
        mo = torch.zeros(cap, dtype=torch.uint8, device=dev)
        ng = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        if undo:
            ctx.undistort_points_dev(Kc, CHAIN_LENS, None, None, U.ITERS, U.TOL_PX, d_xy1.data_ptr(), d_n.data_ptr(), cap, d_xy1.data_ptr())
            ctx.undistort_points_dev(Kc, CHAIN_LENS, None, None, U.ITERS, U.TOL_PX, d_xy2.data_ptr(), d_n.data_ptr(), cap, d_xy2.data_ptr())
        view = api.PointsView(d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr(), 1, cap, 0, 1, 0)
        ctx.ransac_essential_run_dev(view, Kc, 0, CHAIN_HYP, CHAIN_THRESH, CHAIN_SEED, k.data_ptr(), E.data_ptr(), m.data_ptr(), cap, c.data_ptr())
        ctx.recover_pose_dev(view, Kc, E.data_ptr(), m.data_ptr(), Rd.data_ptr(), td.data_ptr(), mo.data_ptr(), ng.data_ptr())
        ctx.synchronize()
        a, b = (u1, u2) if undo else (d1, d2)
        g1, g2 = d_xy1.cpu().numpy(), d_xy2.cpu().numpy()
        assert U.same_floats(g1[:n], a) and U.same_floats(g2[:n], b) and (g1[n:] == -7.5).all() and (g2[n:] == -7.5).all()
        rc, Eh, mh, ch, kh = ctx.ransac_essential(a, b, Kc, CHAIN_HYP, CHAIN_THRESH, CHAIN_SEED)
        assert rc == api.PM_OK
        rc, Rh, th, moh, ngh, _ = ctx.recover_pose(a, b, Kc, Eh, mh)
        assert rc == api.PM_OK
        assert (int(k.item()) & ((1 << 64) - 1)) == kh and int(c.item()) == ch and int(ng.item()) == ngh
        assert _bits_equal(E.cpu().numpy(), Eh) and _bits_equal(Rd.cpu().numpy(), Rh) and _bits_equal(td.cpu().numpy(), th)
        assert (m.cpu().numpy()[:n] == mh).all() and (mo.cpu().numpy()[:n] == moh).all()
        errs[name] = _rot_deg(Rd.cpu().numpy().reshape(3, 3), Rg)
        print("chain (%s): %d inliers, %d in front, rotation error %.4f degrees" % (name, ch, ngh, errs[name]))
    assert errs["undistorted"] < errs["raw"]
