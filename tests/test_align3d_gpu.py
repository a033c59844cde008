"""GPU: 3-D to 3-D alignment (pm_ransac_align3d*, pm_align3d_refine*, pm_transform_points3*, pm_gather_align3d_dev;
docs/SPEC.md S97-S101) against the C restatement (tests/align3d_ref.c) bit for bit — single samples, whole runs at sizes
around the slot and LDS-tile boundaries, ids at the top of the 32-bit range, views with device-side counts and long
masks, NaN rows, the refit (host, device, in place), the point transform and the gather — plus recovery of planted
transforms, the refit's gain, every error status of the device forms, and two device chains with no host copy before the
final readback: two monocular maps of different gauge (triangulation -> similarity -> transform) and stereo odometry
(two disparity maps -> points -> rigid motion)."""
import ctypes as C

import numpy as np
import pytest

import align3d_ref as R
from points_matching_amd import api, synth

pytestmark = pytest.mark.gpu

TILE = 40 * 128          # correspondences per LDS tile of the scorer (ransac_align3d_fused.hip)
MODELS = (R.RIGID, R.SIMILARITY)
U64 = (1 << 64) - 1


def _bits_equal(a, b):
    return (np.asarray(a, np.float64).view(np.uint64) == np.asarray(b, np.float64).view(np.uint64)).all()


def _rot_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def _info_equal(info, ref):
    return (_bits_equal([info.cost_in, info.cost_out], [ref.cost_in, ref.cost_out]) and
            (info.n_used, info.iters, info.status) == (ref.n_used, ref.iters, ref.status))


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


# -- bit parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_from_hyp_bit_parity(ctx, model):
    x1, x2, *_ = synth.align3d_scene(200, seed=4, model=model, nan_frac=0.02)
    x1[5] = x1[6]                                     # duplicate and collinear triples among the samples
    x2[9:12] = x2[9]
    x1[20:60] = x1[20] + np.arange(40, dtype=np.float32)[:, None] * np.array([1.0, 2.0, -1.0], np.float32)
    valid = 0
    for h in range(1000):
        rc, T, mask, c = ctx.ransac_align3d_from_hyp(x1, x2, h, 0.1, 0x5EED, model=model)
        Tr, ok = R.candidate(model, x1, x2, 0x5EED, h)
        assert rc == (api.PM_OK if ok else api.PM_E_NO_MODEL), h
        assert _bits_equal(T, Tr), h
        mr, cr = R.score(Tr, x1, x2, 0.1) if ok else (np.zeros(200, np.uint8), 0)
        assert c == cr and (mask == mr).all(), h
        valid += ok
    assert 500 < valid < 1000


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n,iters", [(3, 50), (4, 50), (127, 200), (128, 200), (129, 200), (2275, 500), (TILE - 1, 100),
                                     (TILE, 100), (TILE + 1, 100), (2 * TILE + 1, 100), (32768, 40)])
def test_full_run_bit_parity(ctx, model, n, iters):
    x1, x2, *_ = synth.align3d_scene(n, seed=n, model=model, nan_frac=0.01 if n > 100 else 0.0)
    rc, T, mask, c, key = ctx.ransac_align3d(x1, x2, iters, 0.1, 0xE55, model=model)
    kr, Tr, mr, cr = R.run(model, x1, x2, iters, 0.1, 0xE55)
    assert rc == (api.PM_OK if kr else api.PM_E_NO_MODEL)
    assert key == kr and c == cr
    assert _bits_equal(T, Tr)
    assert (mask == mr).all()


@pytest.mark.parametrize("model", MODELS)
def test_ids_at_the_top_of_the_32_bit_range(ctx, model):
    x1, x2, *_ = synth.align3d_scene(300, seed=6, model=model)
    b, e = (1 << 32) - 150, 1 << 32
    rc, T, mask, c, key = ctx.ransac_align3d(x1, x2, e, 0.1, 21, model=model, hyp_begin=b)
    kr, Tr, mr, cr = R.run(model, x1, x2, e, 0.1, 21, hyp_begin=b)
    assert rc == api.PM_OK and key == kr and c == cr and _bits_equal(T, Tr) and (mask == mr).all()
    assert b <= api.ransac_key_hyp(key) < e
    rc, T1, m1, c1 = ctx.ransac_align3d_from_hyp(x1, x2, e - 1, 0.1, 21, model=model)
    # the one-sample run of the restatement, not the bare candidate: at id 2^32 - 1 a model without a single inlier has
    # key 0, which S100 (as S29) reads as "no model"
    k1, Tr1, mr1, cr1 = R.run(model, x1, x2, e, 0.1, 21, hyp_begin=e - 1)
    assert _bits_equal(T1, Tr1) and rc == (api.PM_OK if k1 else api.PM_E_NO_MODEL) and c1 == cr1 and (m1 == mr1).all()


@pytest.mark.parametrize("model", MODELS)
def test_view_with_device_count_mask_lengths_and_guard_bytes(ctx, model):
    torch, dev = _dev()
    cap, guard = 3000, 64
    x1, x2, *_ = synth.align3d_scene(cap, seed=31, model=model, nan_frac=0.01)
    d1, d2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
    for n in (2500, 2):                               # a device count below cap, and below 3
        dn = torch.tensor([n], dtype=torch.int32, device=dev)
        view = api.XyzView(d1.data_ptr(), d2.data_ptr(), dn.data_ptr(), cap, 0)
        kr, Tr, mr, cr = R.run(model, x1[:n], x2[:n], 300, 0.1, 77)
        assert bool(kr) == (n >= 3)
        for mask_len in (n - 1, n, cap + 7):
            k = torch.zeros(1, dtype=torch.int64, device=dev)
            T = torch.full((13,), 7.0, dtype=torch.float64, device=dev)
            m = torch.full((mask_len + guard,), 7, dtype=torch.uint8, device=dev)
            c = torch.full((1,), 99, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctx.ransac_align3d_run_dev(view, 0, 300, 0.1, 77, k.data_ptr(), T.data_ptr(), m.data_ptr(), mask_len, c.data_ptr(),
                                       model=model)
            ctx.synchronize()
            assert (int(k.item()) & U64) == kr and int(c.item()) == cr
            assert _bits_equal(T.cpu().numpy(), Tr)
            mm = m.cpu().numpy()
            w = min(mask_len, n)
            assert (mm[:w] == mr[:w]).all() and not mm[w:mask_len].any()
            assert (mm[mask_len:] == 7).all()                                     # guard bytes untouched


@pytest.mark.parametrize("model", MODELS)
def test_nan_rows_are_never_inliers_and_change_no_other_verdict(ctx, model):
    x1, x2, *_ = synth.align3d_scene(1000, seed=12, model=model, outlier_frac=0.2)
    h = next(h for h in range(100) if R.candidate(model, x1, x2, 3, h)[1] and R.score(R.candidate(model, x1, x2, 3, h)[0],
                                                                                   x1, x2, 0.1)[1] > 500)
    idx = set(R.sample(3, h, 1000).tolist())
    rc, T0, m0, c0 = ctx.ransac_align3d_from_hyp(x1, x2, h, 0.1, 3, model=model)
    y1, y2 = x1.copy(), x2.copy()
    rows = np.array([i for i in range(0, 1000, 7) if i not in idx])
    y1[rows[::3], 1] = np.nan
    y2[rows[1::3], 0] = np.inf
    y2[rows[2::3]] = np.nan
    rc, T1, m1, c1 = ctx.ransac_align3d_from_hyp(y1, y2, h, 0.1, 3, model=model)
    keep = np.ones(1000, bool)
    keep[rows] = False
    assert rc == api.PM_OK and _bits_equal(T0, T1)
    assert not m1[rows].any() and (m1[keep] == m0[keep]).all() and c1 == m1.sum() and m0[rows].any()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", [3, 50, 2275, 32768])
def test_refit_bit_parity_on_ransac_and_handmade_masks(ctx, model, n):
    x1, x2, s, Rg, tg, inl = synth.align3d_scene(n, seed=40 + n, model=model, outlier_frac=0.0 if n <= 50 else 0.3,
                                                 nan_frac=0.0 if n <= 50 else 0.02)
    kr, Tr, mr, cr = R.run(model, x1, x2, 300 if n < 32768 else 60, 0.1, 9)
    assert kr
    rng = np.random.default_rng(n)
    for mask in (mr, inl.astype(np.uint8), (rng.random(n) < 0.5).astype(np.uint8), np.ones(n, np.uint8)):
        for start in (Tr, R.pack(s, Rg, tg)):
            rc, T, info = ctx.align3d_refine(x1, x2, mask, start, model=model)
            ref, ri = R.refine(model, x1, x2, mask, start)
            assert rc == api.PM_OK
            assert _bits_equal(T, ref), (n, model)
            assert _info_equal(info, ri), (n, info.cost_in, info.cost_out, info.n_used, info.status, ri.__dict__)
            assert info.cost_out <= info.cost_in and info.iters == 0


@pytest.mark.parametrize("model", MODELS)
def test_refit_statuses_and_estimate_call(ctx, model):
    x1, x2, s, Rg, tg, inl = synth.align3d_scene(300, seed=77, model=model)
    Tg = R.pack(s, Rg, tg)
    rc, T, info = ctx.align3d_refine(x1, x2, inl, np.zeros(13), model=model)
    assert rc == api.PM_E_NO_MODEL and info.status == 2 and not T.any()
    rc, T, info = ctx.align3d_refine(x1[:2], x2[:2], inl[:2], Tg, model=model)
    assert rc == api.PM_E_TOO_FEW and (T == Tg).all()
    k = np.arange(40, dtype=np.float64)[:, None]                       # exactly collinear rows: status 1, the input bits
    a = k * np.array([1.0, 2.0, -1.0]) + np.array([3.0, 0.0, 5.0])
    rc, T, info = ctx.align3d_refine(a, a + 1.0, np.ones(40, np.uint8), Tg, model=model)
    ref, ri = R.refine(model, a, a + 1.0, np.ones(40, np.uint8), Tg)
    assert rc == api.PM_OK and info.status == 1 and _bits_equal(T, Tg) and _info_equal(info, ri)
    kr, Tr, mr, cr = R.run(model, x1, x2, 500, 0.1, 3)
    for refine in (False, True):
        rc, T, mask, c, key, info = ctx.estimate_align3d(x1, x2, 500, 0.1, 3, model=model, refine=refine)
        assert rc == api.PM_OK and key == kr and c == cr and (mask == mr).all()
        if refine:
            ref, ri = R.refine(model, x1, x2, mr, Tr)
            assert _bits_equal(T, ref) and _info_equal(info, ri) and info.status == 0
        else:
            assert _bits_equal(T, Tr) and info.status == 1 and info.n_used == 0
    same = np.tile(x1[:1], (100, 1))
    rc, T, mask, c, key, info = ctx.estimate_align3d(same, same, 100, 0.1, 1, model=model)
    assert rc == api.PM_E_NO_MODEL and key == 0 and not T.any() and not mask.any() and c == 0 and info.status == 2


@pytest.mark.parametrize("model", MODELS)
def test_refit_device_form_in_place_and_with_counts(ctx, model):
    torch, dev = _dev()
    cap, n = 3000, 2600
    x1, x2, *_ = synth.align3d_scene(cap, seed=91, model=model, nan_frac=0.01)
    kr, Tr, mr, cr = R.run(model, x1[:n], x2[:n], 300, 0.1, 4)
    ref, ri = R.refine(model, x1[:n], x2[:n], mr, Tr)
    d1, d2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
    dn = torch.tensor([n], dtype=torch.int32, device=dev)
    view = api.XyzView(d1.data_ptr(), d2.data_ptr(), dn.data_ptr(), cap, 0)
    dm = torch.from_numpy(np.r_[mr, np.ones(cap - n, np.uint8)]).to(dev)      # rows past the count are never read
    dT = torch.from_numpy(Tr.copy()).to(dev)
    dinfo = torch.zeros(32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.align3d_refine_dev(view, dm.data_ptr(), dT.data_ptr(), dT.data_ptr(), dinfo.data_ptr(), model=model)   # in place
    ctx.synchronize()
    info = dinfo.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]
    assert _bits_equal(dT.cpu().numpy(), ref)
    assert _bits_equal([info["cost_in"], info["cost_out"]], [ri.cost_in, ri.cost_out])
    assert (int(info["n_used"]), int(info["iters"]), int(info["status"])) == (ri.n_used, 0, ri.status)


def test_transform_points3_host_device_in_place_and_with_a_count(ctx):
    torch, dev = _dev()
    rng = np.random.default_rng(8)
    x = rng.uniform(-50, 50, (1000, 3)).astype(np.float32)
    x[5] = np.nan
    x[17, 1] = np.inf
    _, _, s, Rg, tg, _ = synth.align3d_scene(3, seed=2, model=R.SIMILARITY)
    T = R.pack(s, Rg, tg)
    ref = R.transform(T, x)
    out = ctx.transform_points3(T, x)
    assert (out.view(np.uint32) == ref.view(np.uint32)).all()
    dT = torch.from_numpy(T).to(dev)
    dx = torch.from_numpy(x).to(dev)
    dout = torch.full((1000, 3), 7.0, dtype=torch.float32, device=dev)
    dn = torch.tensor([700], dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.transform_points3_dev(dT.data_ptr(), dx.data_ptr(), dn.data_ptr(), 1000, dout.data_ptr())
    ctx.transform_points3_dev(dT.data_ptr(), dx.data_ptr(), None, 1000, dx.data_ptr())            # in place, no count
    ctx.synchronize()
    o = dout.cpu().numpy()
    assert (o[:700].view(np.uint32) == ref[:700].view(np.uint32)).all() and (o[700:] == 7.0).all()
    assert (dx.cpu().numpy().view(np.uint32) == ref.view(np.uint32)).all()


def test_gather_rows_and_nan_for_bad_indices(ctx):
    torch, dev = _dev()
    rng = np.random.default_rng(5)
    t1 = rng.uniform(-5, 5, (40, 3)).astype(np.float32)
    t2 = rng.uniform(-5, 5, (30, 3)).astype(np.float32)
    m = np.zeros(20, api.MATCH_DTYPE)
    m["queryIdx"] = rng.integers(0, 40, 20)
    m["trainIdx"] = rng.integers(0, 30, 20)
    m["queryIdx"][3], m["trainIdx"][7], m["trainIdx"][8], m["queryIdx"][9] = 40, -1, 30, -5
    dm = torch.from_numpy(m.view(np.uint8)).to(dev)
    d1, d2 = torch.from_numpy(t1).to(dev), torch.from_numpy(t2).to(dev)
    dcount = torch.tensor([12], dtype=torch.int32, device=dev)
    o1 = torch.full((20, 3), 7.0, dtype=torch.float32, device=dev)
    o2 = torch.full((20, 3), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.gather_align3d_dev(dm.data_ptr(), dcount.data_ptr(), 20, d1.data_ptr(), 40, d2.data_ptr(), 30, o1.data_ptr(), o2.data_ptr())
    ctx.synchronize()
    h1, h2 = o1.cpu().numpy(), o2.cpu().numpy()
    for i in range(12):
        q, t = m["queryIdx"][i], m["trainIdx"][i]
        assert (np.isnan(h1[i]).all() if not 0 <= q < 40 else (h1[i] == t1[q]).all()), i
        assert (np.isnan(h2[i]).all() if not 0 <= t < 30 else (h2[i] == t2[t]).all()), i
    assert (h1[12:] == 7.0).all() and (h2[12:] == 7.0).all()                    # rows past the count untouched


# -- planted recovery ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("seed", range(6))
def test_recovers_planted_transform_and_refit_is_closer(ctx, model, seed):
    # 50 % outliers; noise 0.01 per coordinate on both sides, so a true inlier's residual under the planted transform is
    # below 0.01 * sqrt(2) * (1 + s) * 4.5 sigma < 0.2 = the threshold at s <= 2
    x1, x2, s, Rg, tg, inl = synth.align3d_scene(2275, seed=seed, model=model, outlier_frac=0.5, noise=0.01)
    rc0, T0, mask0, c0, key0 = ctx.ransac_align3d(x1, x2, 2000, 0.2, 11, model=model)
    rc, T, mask, c, key, info = ctx.estimate_align3d(x1, x2, 2000, 0.2, 11, model=model, refine=True)
    kr, Tr, mr, cr = R.run(model, x1, x2, 2000, 0.2, 11)
    assert rc == rc0 == api.PM_OK and key == key0 == kr and (mask == mask0).all() and (mask == mr).all() and _bits_equal(T0, Tr)
    assert mask.astype(bool)[inl].all()                                    # every true inlier is in the mask
    assert info.status == 0 and info.cost_out < info.cost_in
    s0, R0, t0 = R.unpack(T0)
    s1, R1, t1 = R.unpack(T)
    assert _rot_deg(R1, Rg) < _rot_deg(R0, Rg)
    assert np.linalg.norm(t1 - tg) < np.linalg.norm(t0 - tg)
    if model == R.SIMILARITY:
        assert abs(s1 - s) < abs(s0 - s)
    else:
        assert s0 == 1.0 and s1 == 1.0


def test_three_inliers_among_500_rows_equals_the_restatement(ctx):
    x1, x2, *_ = synth.align3d_scene(500, seed=77, outlier_frac=0.994, noise=0.001)
    kr, Tr, mr, cr = R.run(R.RIGID, x1, x2, 2000, 0.05, 5)
    rc, T, mask, c, key = ctx.ransac_align3d(x1, x2, 2000, 0.05, 5)
    assert rc == api.PM_OK and key == kr and c == cr and _bits_equal(T, Tr) and (mask == mr).all()


# -- statuses ------------------------------------------------------------------------------------------------------------------
def test_statuses(ctx):
    torch, dev = _dev()
    x1, x2, *_ = synth.align3d_scene(100, seed=5)
    same = np.tile(x1[:1], (100, 1))
    rc, T, mask, c, key = ctx.ransac_align3d(same, x2, 100, 0.1, 1)
    assert rc == api.PM_E_NO_MODEL and key == 0 and not T.any() and not mask.any() and c == 0
    assert ctx.ransac_align3d(x1[:2], x2[:2], 100, 0.1, 1)[0] == api.PM_E_TOO_FEW
    for call in (lambda: ctx.ransac_align3d(x1, x2, 100, 0.0, 1), lambda: ctx.ransac_align3d(x1, x2, 100, float("inf"), 1),
                 lambda: ctx.ransac_align3d(x1, x2, (1 << 32) + 1, 0.1, 1, hyp_begin=(1 << 32) - 5),
                 lambda: ctx.ransac_align3d(x1, x2, 100, 0.1, 1, kind=api.PM_ERR_SAMPSON),
                 lambda: ctx.ransac_align3d(x1, x2, 100, 0.1, 1, model=2),
                 lambda: ctx.ransac_align3d_from_hyp(x1, x2, 1 << 32, 0.1, 1),
                 lambda: ctx.align3d_refine(x1, x2, np.ones(100, np.uint8), np.ones(13), model=7)):
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_INVALID
    L, h = api.lib(), ctx._h
    d1, d2 = torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev)
    dk, dT = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(13, dtype=torch.float64, device=dev)
    dm, dc = torch.zeros(100, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    view = api.XyzView(d1.data_ptr(), d2.data_ptr(), None, 100, 0)
    vp = C.byref(view)
    P = [C.c_void_p(t.data_ptr()) for t in (dk, dT, dm, dc)]
    INV = api.PM_E_INVALID
    prm = C.byref(api.RansacParams(0, 10, 1, 0.1, api.PM_ERR_REPROJ))
    assert L.pm_ransac_align3d_run_dev(h, 0, None, prm, *P[:3], 100, P[3]) == INV                 # null view
    for i in range(4):                                                                            # null outputs
        Q = [None if j == i else P[j] for j in range(4)]
        assert L.pm_ransac_align3d_run_dev(h, 0, vp, prm, Q[0], Q[1], Q[2], 100, Q[3]) == INV
    assert L.pm_ransac_align3d_run_dev(h, 0, vp, prm, *P[:3], -1, P[3]) == INV                    # mask_len
    assert L.pm_ransac_align3d_run_dev(h, 2, vp, prm, *P[:3], 100, P[3]) == INV                   # model
    assert L.pm_ransac_align3d_run_dev(h, 0, vp, None, *P[:3], 100, P[3]) == INV                  # params
    for bad in (api.RansacParams(0, 10, 1, 0.0, api.PM_ERR_REPROJ), api.RansacParams(0, 10, 1, 0.1, api.PM_ERR_SAMPSON),
                api.RansacParams(3, 3, 1, 0.1, api.PM_ERR_REPROJ), api.RansacParams(0, (1 << 32) + 1, 1, 0.1, api.PM_ERR_REPROJ)):
        assert L.pm_ransac_align3d_run_dev(h, 0, vp, C.byref(bad), *P[:3], 100, P[3]) == INV
    for bad in (api.XyzView(d1.data_ptr(), d2.data_ptr(), None, 0, 0), api.XyzView(None, d2.data_ptr(), None, 100, 0),
                api.XyzView(d1.data_ptr(), None, None, 100, 0)):
        assert L.pm_ransac_align3d_run_dev(h, 0, C.byref(bad), prm, *P[:3], 100, P[3]) == INV
        assert L.pm_align3d_refine_dev(h, 0, C.byref(bad), P[2], P[1], P[1], None) == INV
    assert L.pm_align3d_refine_dev(h, 0, None, P[2], P[1], P[1], None) == INV
    assert L.pm_align3d_refine_dev(h, 0, vp, None, P[1], P[1], None) == INV
    assert L.pm_align3d_refine_dev(h, 0, vp, P[2], None, P[1], None) == INV
    assert L.pm_align3d_refine_dev(h, 0, vp, P[2], P[1], None, None) == INV
    assert L.pm_align3d_refine_dev(h, 3, vp, P[2], P[1], P[1], None) == INV
    X = C.c_void_p(d1.data_ptr())
    assert L.pm_transform_points3_dev(h, None, X, None, 100, X) == INV
    assert L.pm_transform_points3_dev(h, P[1], None, None, 100, X) == INV
    assert L.pm_transform_points3_dev(h, P[1], X, None, 100, None) == INV
    assert L.pm_transform_points3_dev(h, P[1], X, None, -1, X) == INV
    assert L.pm_transform_points3_dev(h, P[1], X, None, 0, X) == api.PM_E_UNSUPPORTED
    assert L.pm_transform_points3(h, None, api._p(x1), 100, api._p(x1)) == INV
    assert L.pm_transform_points3(h, api._p(np.zeros(13)), api._p(x1), 0, api._p(x1)) == api.PM_E_UNSUPPORTED
    assert L.pm_gather_align3d_dev(h, None, P[3], 10, X, 1, X, 1, X, X) == INV
    assert L.pm_gather_align3d_dev(h, X, P[3], 0, X, 1, X, 1, X, X) == INV
    assert L.pm_gather_align3d_dev(h, X, P[3], 10, X, -1, X, 1, X, X) == INV
    # a zero input model on the device form is a data outcome: status 2 in the info, the call itself succeeds
    dinfo = torch.zeros(32, dtype=torch.uint8, device=dev)
    dm.fill_(1)
    ctx.align3d_refine_dev(view, dm.data_ptr(), dT.data_ptr(), dT.data_ptr(), dinfo.data_ptr())
    ctx.synchronize()
    assert int(dinfo.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]["status"]) == 2 and not dT.cpu().numpy().any()


# -- chains --------------------------------------------------------------------------------------------------------------------
def _look_at_pose(centre, yaw):
    """World -> camera pose (R, t) of a camera at `centre` turned by `yaw` about y."""
    Rm = np.array([[np.cos(yaw), 0.0, -np.sin(yaw)], [0.0, 1.0, 0.0], [np.sin(yaw), 0.0, np.cos(yaw)]])
    return Rm, -Rm @ np.asarray(centre, np.float64)


def test_chain_two_monocular_maps_of_different_gauge(ctx):
    torch, dev = _dev()
    n, fx, fy, cx, cy = 1500, 800.0, 820.0, 500.0, 330.0
    K = (fx, fy, cx, cy)
    rng = np.random.default_rng(21)
    X = np.c_[rng.uniform(-2.5, 2.5, (n, 2)), rng.uniform(5.0, 9.0, n)]
    poses = [_look_at_pose(c, y) for c, y in (((-0.8, 0.0, 0.0), 0.05), ((0.8, 0.1, 0.0), -0.05), ((-0.7, -0.1, 0.2), 0.03),
                                              ((0.9, 0.0, -0.1), -0.06))]
    # gauge B of the second map: x_B = s G x_W + g.  A camera x_cam = R x_W + t sees the same pixels from x_B under the pose
    # R' = R G^T, t' = s t - R' g (the whole camera frame scaled by s)
    s = 1.7
    G = synth._rodrigues([0.3, -1.0, 0.5], 0.4)
    g = np.array([0.7, -1.1, 2.0])
    XB = s * X @ G.T + g
    noise_px = 0.25                                                        # uniform in +-noise_px per pixel coordinate
    uv, Rt = [], []
    for k, (Rk, tk) in enumerate(poses):
        xc = X @ Rk.T + tk
        px = np.c_[fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy] + rng.uniform(-noise_px, noise_px, (n, 2))
        uv.append(px.astype(np.float32))
        if k < 2:
            Rt.append(np.r_[Rk.reshape(-1), tk])
        else:
            Rb = Rk @ G.T
            Rt.append(np.r_[Rb.reshape(-1), s * tk - Rb @ g])
    uv[1][::97] = np.nan                                                   # tracks lost in one view of a pair: NaN map rows
    uv[2][5::101] = np.nan
    # Triangulation noise, first order: a pixel error e in each of the two views of a pair (baseline b ~ 1.6, depth Z <= 9)
    # moves the point by at most Z^2 / (fx b) * 2 e = 0.032 in depth and Z / fx * e * sqrt(2) = 0.004 across; the two maps
    # together, in gauge B: s * 2 * 0.036 = 0.12.  The RANSAC threshold is twice that.
    bound = s * 2.0 * (81.0 / (fx * 1.6) * 2 * noise_px + 9.0 / fx * noise_px * np.sqrt(2.0))
    thr = 2.0 * bound
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        ctx.set_stream(st.cuda_stream)
        duv = [torch.from_numpy(u).to(dev) for u in uv]
        dRt = [torch.from_numpy(r).to(dev) for r in Rt]
        dA = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        dB = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        dsa = torch.zeros(n, dtype=torch.uint8, device=dev)
        dsb = torch.zeros(n, dtype=torch.uint8, device=dev)
        dk = torch.zeros(1, dtype=torch.int64, device=dev)
        dT = torch.zeros(13, dtype=torch.float64, device=dev)
        dT0 = torch.zeros(13, dtype=torch.float64, device=dev)
        dm = torch.zeros(n, dtype=torch.uint8, device=dev)
        dc = torch.zeros(1, dtype=torch.int32, device=dev)
        dinfo = torch.zeros(32, dtype=torch.uint8, device=dev)
        dAB = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        st.synchronize()
        prm = api.tri_params()
        ctx.triangulate_dev(api.tri_views([duv[0].data_ptr(), duv[1].data_ptr()], [dRt[0].data_ptr(), dRt[1].data_ptr()], n), K, prm,
                            dA.data_ptr(), dsa.data_ptr())
        ctx.triangulate_dev(api.tri_views([duv[2].data_ptr(), duv[3].data_ptr()], [dRt[2].data_ptr(), dRt[3].data_ptr()], n), K, prm,
                            dB.data_ptr(), dsb.data_ptr())
        view = api.XyzView(dA.data_ptr(), dB.data_ptr(), None, n, 0)
        ctx.ransac_align3d_run_dev(view, 0, 500, thr, 0xC0FFEE, dk.data_ptr(), dT0.data_ptr(), dm.data_ptr(), n, dc.data_ptr(),
                                   model=api.PM_ALIGN3D_SIMILARITY)
        ctx.align3d_refine_dev(view, dm.data_ptr(), dT0.data_ptr(), dT.data_ptr(), dinfo.data_ptr(), model=api.PM_ALIGN3D_SIMILARITY)
        ctx.transform_points3_dev(dT.data_ptr(), dA.data_ptr(), None, n, dAB.data_ptr())
        ctx.synchronize()
        ctx.set_stream(0)
    A, B, AB = dA.cpu().numpy(), dB.cpu().numpy(), dAB.cpu().numpy()
    T, T0 = dT.cpu().numpy(), dT0.cpu().numpy()
    info = dinfo.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]
    fin = np.isfinite(A).all(axis=1) & np.isfinite(B).all(axis=1)
    assert fin.sum() >= 0.95 * n and (~np.isfinite(A).all(axis=1)).sum() >= 15 and (~np.isfinite(B).all(axis=1)).sum() >= 14
    # the same calls from the host on the maps read back: the device chain computed exactly this
    rc, Th, mh, ch, kh, ih = ctx.estimate_align3d(A, B, 500, thr, 0xC0FFEE, model=api.PM_ALIGN3D_SIMILARITY)
    assert rc == api.PM_OK and (int(dk.item()) & U64) == kh and int(dc.item()) == ch and _bits_equal(T, Th)
    assert (dm.cpu().numpy() == mh).all() and int(info["status"]) == ih.status == 0
    assert (AB.view(np.uint32) == R.transform(T, A).view(np.uint32)).all() and np.isnan(AB[~np.isfinite(A).all(axis=1)]).all()
    d = np.linalg.norm(AB[fin].astype(np.float64) - B[fin], axis=1)
    s1, R1, t1 = R.unpack(T)
    print("finite rows %d, inliers %d, worst |T(A) - B| %.4f (first-order bound %.4f, threshold %.4f), scale %.6f vs %.6f" %
          (fin.sum(), ch, d.max(), bound, thr, s1, s))
    assert ch >= 0.99 * fin.sum() and d.max() <= thr
    # scale: one row alone would fix it to bound / extent of the map (0.12 / (1.7 * 5) = 1.4 %); the least-squares scale
    # over more than 1000 rows averages that down by sqrt(n) ~ 30 or more; 0.3 % leaves a factor 6 on top
    assert abs(s1 / s - 1.0) < 3e-3, (s1, s)
    assert _rot_deg(R1, G) < 0.5 and np.linalg.norm(t1 - g) < 0.2


def test_chain_stereo_odometry(ctx):
    torch, dev = _dev()
    w, h, fx, cx, cy, base = 1024, 768, 800.0, 512.0, 384.0, 0.5
    K = (fx, fx, cx, cy)
    rng = np.random.default_rng(33)
    zmax = 8.0
    P1 = np.c_[rng.uniform(-3.0, 3.0, 4000), rng.uniform(-2.0, 2.0, 4000), rng.uniform(3.5, zmax - 0.5, 4000)]
    Rm = synth._rodrigues([0.2, 1.0, -0.1], np.radians(3.0))
    tm = np.array([0.2, 0.05, 0.3])
    P2 = P1 @ Rm.T + tm                                                     # the rig's motion: x2 = R x1 + t

    def pixels(P):
        return np.rint(fx * P[:, 0] / P[:, 2] + cx).astype(np.int64), np.rint(fx * P[:, 1] / P[:, 2] + cy).astype(np.int64)

    (u1, v1), (u2, v2) = pixels(P1), pixels(P2)
    ok = (u1 >= 0) & (u1 < w) & (v1 >= 0) & (v1 < h) & (u2 >= 0) & (u2 < w) & (v2 >= 0) & (v2 < h) & (P2[:, 2] < zmax)
    for u, v in ((u1, v1), (u2, v2)):                                      # drop points that share a pixel in a frame
        _, first, counts = np.unique(v * w + u, return_index=True, return_counts=True)
        alone = np.zeros(len(u), bool)
        alone[first[counts == 1]] = True
        ok &= alone
    P1, P2, u1, v1, u2, v2 = P1[ok], P2[ok], u1[ok], v1[ok], u2[ok], v2[ok]
    n = len(P1)
    assert n >= 1500
    maps = []
    for P, u, v in ((P1, u1, v1), (P2, u2, v2)):
        dmap = np.full((h, w), api.PM_STEREO_INVALID, np.int16)
        dmap[v, u] = np.rint(16.0 * fx * base / P[:, 2]).astype(np.int16)
        maps.append(dmap)
    pts = [np.c_[u1, v1].astype(np.float32), np.c_[u2, v2].astype(np.float32)]
    pts[0][::50] = -5.0                                                    # lost tracks: outside the map, NaN rows
    # Threshold.  S87 reads Z = 16 fx B / v at the rounded pixel.  v is rounded to one 1/16-pixel step, so Z is off by at
    # most one step's worth, Z^2 / (16 fx B) = 0.01 at Z = 8 (half of it, strictly); the pixel is rounded by at most half a
    # pixel per axis, which moves X and Y by 0.5 Z / fx = 0.005 each.  One frame: sqrt(0.01^2 + 2 * 0.005^2) = 0.0122; the
    # residual compares two frames: 2 * 0.0122 = 0.0245.
    thr = 2.0 * np.sqrt((zmax * zmax / (16.0 * fx * base)) ** 2 + 2.0 * (0.5 * zmax / fx) ** 2)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        ctx.set_stream(st.cuda_stream)
        dmaps = [torch.from_numpy(m).to(dev) for m in maps]
        dpts = [torch.from_numpy(p).to(dev) for p in pts]
        dX = [torch.zeros((n, 3), dtype=torch.float32, device=dev) for _ in range(2)]
        dk = torch.zeros(1, dtype=torch.int64, device=dev)
        dT0 = torch.zeros(13, dtype=torch.float64, device=dev)
        dT = torch.zeros(13, dtype=torch.float64, device=dev)
        dm = torch.zeros(n, dtype=torch.uint8, device=dev)
        dc = torch.zeros(1, dtype=torch.int32, device=dev)
        dinfo = torch.zeros(32, dtype=torch.uint8, device=dev)
        st.synchronize()
        for i in range(2):
            ctx.stereo_points_dev(dmaps[i].data_ptr(), w, h, w, K, base, None, dpts[i].data_ptr(), None, n, dX[i].data_ptr())
        view = api.XyzView(dX[0].data_ptr(), dX[1].data_ptr(), None, n, 0)
        ctx.ransac_align3d_run_dev(view, 0, 500, float(thr), 7, dk.data_ptr(), dT0.data_ptr(), dm.data_ptr(), n, dc.data_ptr())
        ctx.align3d_refine_dev(view, dm.data_ptr(), dT0.data_ptr(), dT.data_ptr(), dinfo.data_ptr())
        ctx.synchronize()
        ctx.set_stream(0)
    X1, X2 = dX[0].cpu().numpy(), dX[1].cpu().numpy()
    T0, T = dT0.cpu().numpy(), dT.cpu().numpy()
    info = dinfo.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]
    fin = np.isfinite(X1).all(axis=1) & np.isfinite(X2).all(axis=1)
    assert np.isnan(X1[::50]).all() and fin.sum() == n - len(X1[::50])
    kr, Tr, mr, cr = R.run(R.RIGID, X1, X2, 500, float(thr), 7)
    ref, ri = R.refine(R.RIGID, X1, X2, mr, Tr)
    assert (int(dk.item()) & U64) == kr and int(dc.item()) == cr and _bits_equal(T0, Tr) and (dm.cpu().numpy() == mr).all()
    assert _bits_equal(T, ref) and int(info["status"]) == ri.status == 0
    s0, R0, t0 = R.unpack(T0)
    s1, R1, t1 = R.unpack(T)
    print("rows %d, inliers %d, threshold %.4f; rotation error %.5f -> %.5f deg, translation error %.5f -> %.5f" %
          (n, cr, thr, _rot_deg(R0, Rm), _rot_deg(R1, Rm), np.linalg.norm(t0 - tm), np.linalg.norm(t1 - tm)))
    assert s0 == 1.0 and s1 == 1.0 and cr >= 0.9 * fin.sum()
    assert _rot_deg(R1, Rm) < _rot_deg(R0, Rm) and np.linalg.norm(t1 - tm) < np.linalg.norm(t0 - tm)
