"""GPU: absolute camera pose (pm_ransac_pnp*, docs/SPEC.md S36-S39) against the C restatement (tests/pnp_ref.c) bit for
bit — every candidate slot and count of single samples, whole runs at sizes around the slot and LDS-tile boundaries,
views with device-side counts and long masks, the S40 refinement (host, device and in place) — plus recovery of a
planted pose, the refinement's gain, every error status, the device chain matcher -> ratio filter -> gather -> RANSAC-PnP
-> refinement with no host round trip, and a visual-odometry chain (relative pose and triangulated map, then PnP)."""
import numpy as np
import pytest

import pnp_ref as R
from points_matching_amd import api, synth

pytestmark = pytest.mark.gpu

TILE = 48 * 128          # correspondences per LDS tile of the PnP scorer (ransac_p_fused.hip)


def _bits_equal(a, b):
    return (np.asarray(a, np.float64).view(np.uint64) == np.asarray(b, np.float64).view(np.uint64)).all()


def _scene(n, seed, **kw):
    xyz, uv, K, Rg, tg, inl = synth.pnp_scene(n, seed=seed, **kw)
    return xyz, uv, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), Rg, tg, inl


def _rot_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def test_sample_candidates_bit_parity(ctx):
    xyz, uv, K, _, _, _ = _scene(200, seed=4)
    xyz[5] = xyz[6]                                   # degenerate samples among the ids
    xyz[9:12] = xyz[9]
    models = 0
    for h in range(1000):
        rc, Rt, counts, nm = ctx.ransac_pnp_from_hyp(xyz, uv, K, h, 4.0, 0x5EED)
        Rr, vr = R.candidates(xyz, uv, K, 0x5EED, h)
        assert rc == (api.PM_OK if vr.any() else api.PM_E_NO_MODEL)
        assert nm == vr.sum()
        assert _bits_equal(Rt, Rr), h
        for j in range(4):
            assert counts[j] == (R.score(K, Rr[j], xyz, uv, 4.0)[1] if vr[j] else -1), (h, j)
        models += nm
    assert models > 1200


@pytest.mark.parametrize("n,iters", [(4, 50), (5, 50), (127, 200), (128, 200), (129, 200), (2275, 500),
                                     (TILE - 1, 100), (TILE, 100), (TILE + 1, 100), (8193, 100), (32768, 40)])
def test_full_run_bit_parity(ctx, n, iters):
    xyz, uv, K, _, _, _ = _scene(n, seed=n)
    rc, Rm, t, mask, c, key = ctx.ransac_pnp(xyz, uv, K, iters, 2.0, 0xE55)
    kr, Rtr, mr, cr = R.run(xyz, uv, K, iters, 2.0, 0xE55)
    assert rc == (api.PM_OK if kr else api.PM_E_NO_MODEL)
    assert key == kr and c == cr
    assert _bits_equal(np.r_[Rm.reshape(-1), t], Rtr)
    assert (mask == mr).all()


def test_view_with_device_count_and_mask_lengths(ctx):
    import torch
    dev = torch.device("cuda", 0)
    cap = 3000
    xyz, uv, K, _, _, _ = _scene(cap, seed=31)
    dx, du = torch.from_numpy(xyz).to(dev), torch.from_numpy(uv).to(dev)
    for n in (2500, 3):                               # a device count below cap, and below 4
        dn = torch.tensor([n], dtype=torch.int32, device=dev)
        view = api.PnpView(dx.data_ptr(), du.data_ptr(), dn.data_ptr(), cap, 0)
        kr, Rtr, mr, cr = R.run(xyz[:n], uv[:n], K, 300, 2.0, 77)
        assert bool(kr) == (n >= 4)
        for mask_len in (n - 1, n, cap + 7):
            if mask_len < 0:
                continue
            k = torch.zeros(1, dtype=torch.int64, device=dev)
            Rt = torch.full((12,), 7.0, dtype=torch.float64, device=dev)
            m = torch.full((mask_len,), 7, dtype=torch.uint8, device=dev)
            c = torch.full((1,), 99, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctx.ransac_pnp_run_dev(view, K, 0, 300, 2.0, 77, k.data_ptr(), Rt.data_ptr(), m.data_ptr(), mask_len, c.data_ptr())
            ctx.synchronize()
            assert (int(k.item()) & ((1 << 64) - 1)) == kr and int(c.item()) == cr
            assert _bits_equal(Rt.cpu().numpy(), Rtr)
            mm = m.cpu().numpy()
            w = min(mask_len, n)
            assert (mm[:w] == mr[:w]).all() and not mm[w:].any()


@pytest.mark.parametrize("seed", range(6))
def test_recovers_planted_pose(ctx, seed):
    # 30 % outliers, 0.5 px noise, fx != fy, off-centre principal point; no refinement on the inliers (follow-up), so the
    # bounds are those of the minimal-sample winner.  The restatement on these six scenes (CPU): 99.8-100 % of the
    # inliers found, no outlier kept, R within 0.024-0.057 deg, t within 0.16-0.39 % of |t|
    xyz, uv, K, Rg, tg, inl = _scene(2275, seed=seed, outlier_frac=0.3, noise_px=0.5)
    rc, Rm, t, mask, c, key = ctx.ransac_pnp(xyz, uv, K, 1000, 2.0, 11)
    assert rc == api.PM_OK
    kr, Rtr, mr, cr = R.run(xyz, uv, K, 1000, 2.0, 11)
    assert key == kr and _bits_equal(np.r_[Rm.reshape(-1), t], Rtr) and (mask == mr).all()
    assert c >= 0.99 * inl.sum() and (mask.astype(bool) & ~inl).sum() <= 0.005 * inl.sum()
    assert _rot_deg(Rm, Rg) < 0.1, _rot_deg(Rm, Rg)
    assert np.linalg.norm(t - tg) < 0.01 * max(1.0, np.linalg.norm(tg)), (t, tg)


def test_statuses(ctx):
    xyz, uv, K, _, _, _ = _scene(100, seed=5)
    same = np.tile(xyz[:1], (100, 1))
    rc, Rm, t, mask, c, key = ctx.ransac_pnp(same, uv, K, 100, 2.0, 1)
    assert rc == api.PM_E_NO_MODEL and key == 0 and not Rm.any() and not t.any() and not mask.any()
    assert ctx.ransac_pnp(xyz[:3], uv[:3], K, 100, 2.0, 1)[0] == api.PM_E_TOO_FEW
    bad_calls = [lambda bad=bad: ctx.ransac_pnp(xyz, uv, bad, 100, 2.0, 1)
                 for bad in ((0.0, 800.0, 400.0, 300.0), (800.0, -1.0, 400.0, 300.0), (800.0, 800.0, np.nan, 300.0),
                             (800.0, 800.0, 400.0, np.inf))]
    bad_calls += [lambda: ctx.ransac_pnp(xyz, uv, K, 100, 0.0, 1),
                  lambda: ctx.ransac_pnp(xyz, uv, K, 100, float("inf"), 1),
                  lambda: ctx.ransac_pnp(xyz, uv, K, (1 << 32) // 4 + 1, 2.0, 1, hyp_begin=(1 << 32) // 4 - 5),
                  lambda: ctx.ransac_pnp(xyz, uv, K, 100, 2.0, 1, kind=api.PM_ERR_SAMPSON),
                  lambda: ctx.ransac_pnp_from_hyp(xyz, uv, K, (1 << 32) // 4, 2.0, 1)]
    for call in bad_calls:
        with pytest.raises(api.PmError) as e:
            call()
        assert e.value.status == api.PM_E_INVALID
    import ctypes as C
    L, h = api.lib(), ctx._h
    cam = C.byref(api.Camera(*K))
    prm = C.byref(api.RansacParams(0, 10, 1, 2.0, api.PM_ERR_REPROJ))
    x, u = api._p(np.ascontiguousarray(xyz)), api._p(np.ascontiguousarray(uv))
    buf = np.zeros(64)
    b, cnt = api._p(buf), api._p(np.zeros(4, np.int32))
    assert L.pm_ransac_pnp(h, x, u, 100, cam, None, b, b, None, None, None) == api.PM_E_INVALID        # null params
    assert L.pm_ransac_pnp(h, x, u, 100, None, prm, b, b, None, None, None) == api.PM_E_INVALID        # null K
    assert L.pm_ransac_pnp(h, None, u, 100, cam, prm, b, b, None, None, None) == api.PM_E_INVALID      # null points
    assert L.pm_ransac_pnp(h, x, None, 100, cam, prm, b, b, None, None, None) == api.PM_E_INVALID
    assert L.pm_ransac_pnp(h, x, u, -1, cam, prm, b, b, None, None, None) == api.PM_E_INVALID
    assert L.pm_ransac_pnp(None, x, u, 100, cam, prm, b, b, None, None, None) == api.PM_E_INVALID      # null ctx
    assert L.pm_ransac_pnp_from_hyp(h, x, u, 100, cam, prm, C.c_int64(0), None, cnt, None) == api.PM_E_INVALID
    assert L.pm_ransac_pnp_from_hyp(h, x, u, 100, cam, prm, C.c_int64(0), b, None, None) == api.PM_E_INVALID
    assert L.pm_ransac_pnp_from_hyp(h, x, u, 100, cam, prm, C.c_int64(-1), b, cnt, None) == api.PM_E_INVALID
    mk = api._p(np.ones(100, np.uint8))
    assert L.pm_pnp_refine(h, x, u, 100, cam, None, b, b, 20, b, b, None) == api.PM_E_INVALID          # null mask
    assert L.pm_pnp_refine(h, x, u, 100, cam, mk, None, b, 20, b, b, None) == api.PM_E_INVALID         # null R_in
    assert L.pm_pnp_refine(h, x, u, 100, cam, mk, b, b, 101, b, b, None) == api.PM_E_INVALID           # max_iters
    assert L.pm_pnp_refine(h, x, u, 100, cam, mk, b, b, -1, b, b, None) == api.PM_E_INVALID
    assert L.pm_solve_pnp_ransac(h, x, u, 100, cam, prm, 101, b, b, None, None, None, None) == api.PM_E_INVALID
    import torch
    dev = torch.device("cuda", 0)
    dx, du = torch.from_numpy(xyz).to(dev), torch.from_numpy(uv).to(dev)
    dk, dRt = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(12, dtype=torch.float64, device=dev)
    dm, dc = torch.zeros(100, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    view = api.PnpView(dx.data_ptr(), du.data_ptr(), None, 100, 0)
    vp = C.byref(view)
    P = [C.c_void_p(t.data_ptr()) for t in (dk, dRt, dm, dc)]
    assert L.pm_ransac_pnp_run_dev(h, None, cam, prm, *P[:3], 100, P[3]) == api.PM_E_INVALID         # null view
    assert L.pm_ransac_pnp_run_dev(h, vp, cam, prm, None, P[1], P[2], 100, P[3]) == api.PM_E_INVALID  # null outputs
    assert L.pm_ransac_pnp_run_dev(h, vp, cam, prm, P[0], None, P[2], 100, P[3]) == api.PM_E_INVALID
    assert L.pm_ransac_pnp_run_dev(h, vp, cam, prm, P[0], P[1], None, 100, P[3]) == api.PM_E_INVALID
    assert L.pm_ransac_pnp_run_dev(h, vp, cam, prm, P[0], P[1], P[2], 100, None) == api.PM_E_INVALID
    assert L.pm_ransac_pnp_run_dev(h, vp, cam, prm, *P[:3], -1, P[3]) == api.PM_E_INVALID             # mask_len
    bad_view = api.PnpView(dx.data_ptr(), du.data_ptr(), None, 0, 0)
    assert L.pm_ransac_pnp_run_dev(h, C.byref(bad_view), cam, prm, *P[:3], 100, P[3]) == api.PM_E_INVALID
    assert L.pm_pnp_refine_dev(h, vp, cam, None, P[1], 20, P[1], None) == api.PM_E_INVALID
    assert L.pm_pnp_refine_dev(h, vp, cam, P[2], P[1], 200, P[1], None) == api.PM_E_INVALID
    assert L.pm_gather_pnp_dev(h, None, P[3], 10, P[1], 1, P[1], 1, P[1], P[1]) == api.PM_E_INVALID
    assert L.pm_gather_pnp_dev(h, P[1], P[3], 0, P[1], 1, P[1], 1, P[1], P[1]) == api.PM_E_INVALID


# -- S40: the refinement on the inliers ------------------------------------------------------------------------------------
def _info_equal(info, ref):
    return (_bits_equal([info.cost_in, info.cost_out], [ref.cost_in, ref.cost_out]) and
            (info.n_used, info.iters, info.status) == (ref.n_used, ref.iters, ref.status))


@pytest.mark.parametrize("n", [4, 50, 2275, 32768])
def test_refine_bit_parity_on_ransac_and_handmade_masks(ctx, n):
    xyz, uv, K, _, _, inl = _scene(n, seed=40 + n, outlier_frac=0.0 if n <= 50 else 0.3)
    kr, Rtr, mr, cr = R.run(xyz, uv, K, 300 if n < 32768 else 60, 2.0, 9)
    assert kr
    rng = np.random.default_rng(n)
    masks = [mr, inl.astype(np.uint8), (rng.random(n) < 0.5).astype(np.uint8)]
    for mask in masks:
        for it in (0, 1, 20):
            rc, Rm, t, info = ctx.pnp_refine(xyz, uv, K, mask, Rtr[:9], Rtr[9:], it)
            ref, ri = R.refine(xyz, uv, K, mask, Rtr, it)
            assert rc == api.PM_OK
            assert _bits_equal(np.r_[Rm.reshape(-1), t], ref), (n, it)
            assert _info_equal(info, ri), (n, it, info.cost_in, info.cost_out, info.iters, info.status, ri.__dict__)
            assert info.cost_out <= info.cost_in


def test_refine_statuses_and_convenience_call(ctx):
    xyz, uv, K, Rg, tg, inl = _scene(300, seed=77)
    rc, Rm, t, info = ctx.pnp_refine(xyz, uv, K, inl, np.zeros(9), np.zeros(3))
    assert rc == api.PM_E_NO_MODEL and info.status == 2 and not Rm.any() and not t.any()
    rc, Rm, t, info = ctx.pnp_refine(xyz[:3], uv[:3], K, inl[:3], Rg, tg)
    assert rc == api.PM_E_TOO_FEW and (Rm == Rg).all() and (t == tg).all()
    rc, Rm, t, mask, c, key, info = ctx.solve_pnp_ransac(xyz, uv, K, 500, 2.0, 3, max_iters=20)
    kr, Rtr, mr, cr = R.run(xyz, uv, K, 500, 2.0, 3)
    ref, ri = R.refine(xyz, uv, K, mr, Rtr, 20)
    assert rc == api.PM_OK and key == kr and c == cr and (mask == mr).all()
    assert _bits_equal(np.r_[Rm.reshape(-1), t], ref) and _info_equal(info, ri)


def test_refine_device_form_in_place_and_with_counts(ctx):
    import torch
    dev = torch.device("cuda", 0)
    cap, n = 3000, 2600
    xyz, uv, K, _, _, _ = _scene(cap, seed=91)
    kr, Rtr, mr, cr = R.run(xyz[:n], uv[:n], K, 300, 2.0, 4)
    ref, ri = R.refine(xyz[:n], uv[:n], K, mr, Rtr, 20)
    dx, du = torch.from_numpy(xyz).to(dev), torch.from_numpy(uv).to(dev)
    dn = torch.tensor([n], dtype=torch.int32, device=dev)
    view = api.PnpView(dx.data_ptr(), du.data_ptr(), dn.data_ptr(), cap, 0)
    dm = torch.from_numpy(np.r_[mr, np.ones(cap - n, np.uint8)]).to(dev)      # rows past the count are never read
    dRt = torch.from_numpy(Rtr.copy()).to(dev)
    dinfo = torch.zeros(32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.pnp_refine_dev(view, K, dm.data_ptr(), dRt.data_ptr(), 20, dRt.data_ptr(), dinfo.data_ptr())   # in place
    ctx.synchronize()
    info = dinfo.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]
    assert _bits_equal(dRt.cpu().numpy(), ref)
    assert _bits_equal([info["cost_in"], info["cost_out"]], [ri.cost_in, ri.cost_out])
    assert (int(info["n_used"]), int(info["iters"]), int(info["status"])) == (ri.n_used, ri.iters, ri.status)


@pytest.mark.parametrize("seed", range(6))
def test_refined_pose_closer_than_minimal(ctx, seed):
    # the restatement on these scenes (CPU): minimal solve 0.024-0.057 deg / 0.16-0.41 % of |t| off the planted pose,
    # refined 0.001-0.007 deg / 0.010-0.054 % (4-15 LM iterations)
    xyz, uv, K, Rg, tg, inl = _scene(2275, seed=seed, outlier_frac=0.3, noise_px=0.5)
    rc0, R0, t0, mask0, c0, key0 = ctx.ransac_pnp(xyz, uv, K, 1000, 2.0, 11)
    rc, Rm, t, mask, c, key, info = ctx.solve_pnp_ransac(xyz, uv, K, 1000, 2.0, 11, max_iters=20)
    assert rc == rc0 == api.PM_OK and key == key0 and (mask == mask0).all()
    assert info.status == 0 and info.cost_out < info.cost_in
    e0 = _rot_deg(R0, Rg) + np.degrees(np.linalg.norm(t0 - tg) / np.linalg.norm(tg))
    e1 = _rot_deg(Rm, Rg) + np.degrees(np.linalg.norm(t - tg) / np.linalg.norm(tg))
    assert e1 < e0, (e0, e1)
    assert _rot_deg(Rm, Rg) < 0.015 and np.linalg.norm(t - tg) < 0.001 * np.linalg.norm(tg)


def test_gather_rows_and_nan_for_bad_indices(ctx):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    kp = rng.uniform(0, 600, (40, 2)).astype(np.float32)
    obj = rng.uniform(-5, 5, (30, 3)).astype(np.float32)
    m = np.zeros(20, api.MATCH_DTYPE)
    m["queryIdx"] = rng.integers(0, 40, 20)
    m["trainIdx"] = rng.integers(0, 30, 20)
    m["queryIdx"][3], m["trainIdx"][7], m["trainIdx"][8] = 40, -1, 30
    dm = torch.from_numpy(m.view(np.uint8)).to(dev)
    dkp, dobj = torch.from_numpy(kp).to(dev), torch.from_numpy(obj).to(dev)
    dcount = torch.tensor([12], dtype=torch.int32, device=dev)
    duv = torch.full((20, 2), 7.0, dtype=torch.float32, device=dev)
    dxyz = torch.full((20, 3), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.gather_pnp_dev(dm.data_ptr(), dcount.data_ptr(), 20, dkp.data_ptr(), 40, dobj.data_ptr(), 30, duv.data_ptr(),
                       dxyz.data_ptr())
    ctx.synchronize()
    uvh, xyzh = duv.cpu().numpy(), dxyz.cpu().numpy()
    for i in range(12):
        q, t = m["queryIdx"][i], m["trainIdx"][i]
        assert (np.isnan(uvh[i]).all() if not 0 <= q < 40 else (uvh[i] == kp[q]).all()), i
        assert (np.isnan(xyzh[i]).all() if not 0 <= t < 30 else (xyzh[i] == obj[t]).all()), i
    assert (uvh[12:] == 7.0).all() and (xyzh[12:] == 7.0).all()                  # rows past the count untouched


def test_chained_device_flow_without_host_copy(ctx):
    import torch
    dev = torch.device("cuda", 0)
    nq = nt = 1800
    w = synth.pair_workload(nq=nq, nt=nt, dim=128, seed=12, planted=0.6)
    xyz0, uv0, Kg, Rg, tg, _ = synth.pnp_scene(nq, seed=12, outlier_frac=0.0)
    K = (Kg[0, 0], Kg[1, 1], Kg[0, 2], Kg[1, 2])
    # the frame's keypoints are kp1; the map holds one 3-D point per train row, the planted ones seen at their query's
    # keypoint from the pose (Rg, tg), the rest random
    kp1 = w["kp1"].copy()
    rows = np.nonzero(w["truth"] >= 0)[0]
    obj = np.random.default_rng(12).uniform(-3, 3, (nt, 3)).astype(np.float32)
    obj[:, 2] += 8.0
    kp1[rows] = uv0[rows]
    obj[w["truth"][rows]] = xyz0[rows]
    q, t = w["q"].astype(np.uint8), w["t"].astype(np.uint8)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        ctx.set_stream(s.cuda_stream)
        d_q, d_t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
        d_kp1, d_kp2 = torch.from_numpy(kp1).to(dev), torch.from_numpy(w["kp2"]).to(dev)
        d_obj = torch.from_numpy(obj).to(dev)
        d_knn = torch.empty((nq, 2, 4), dtype=torch.int32, device=dev)
        d_good = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
        d_xy1 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
        d_xy2 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        d_uv = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
        d_xyz = torch.zeros((nq, 3), dtype=torch.float32, device=dev)
        k = torch.zeros(1, dtype=torch.int64, device=dev)
        Rt = torch.zeros(12, dtype=torch.float64, device=dev)
        m = torch.zeros(nq, dtype=torch.uint8, device=dev)
        c = torch.zeros(1, dtype=torch.int32, device=dev)
        dinfo = torch.zeros(32, dtype=torch.uint8, device=dev)
        s.synchronize()
        ctx.bf_knn_l2_u8_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 128, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(),
                                   d_knn.data_ptr(), d_good.data_ptr(), d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr())
        ctx.gather_pnp_dev(d_good.data_ptr(), d_n.data_ptr(), nq, d_kp1.data_ptr(), nq, d_obj.data_ptr(), nt,
                           d_uv.data_ptr(), d_xyz.data_ptr())
        view = api.PnpView(d_xyz.data_ptr(), d_uv.data_ptr(), d_n.data_ptr(), nq, 0)
        ctx.ransac_pnp_run_dev(view, K, 0, 500, 2.0, 0xC0FFEE, k.data_ptr(), Rt.data_ptr(), m.data_ptr(), nq, c.data_ptr())
        ctx.pnp_refine_dev(view, K, m.data_ptr(), Rt.data_ptr(), 20, Rt.data_ptr(), dinfo.data_ptr())
        ctx.synchronize()
        ctx.set_stream(0)
    n = int(d_n.item())
    assert n >= 400
    good = d_good.cpu().numpy()[:n].copy().view(api.MATCH_DTYPE).reshape(-1)
    xyz_h, uv_h = obj[good["trainIdx"]], kp1[good["queryIdx"]]
    assert (d_xyz.cpu().numpy()[:n] == xyz_h).all() and (d_uv.cpu().numpy()[:n] == uv_h).all()
    rc, Rh, th, mh, ch, kh, ih = ctx.solve_pnp_ransac(xyz_h, uv_h, K, 500, 2.0, 0xC0FFEE, max_iters=20)
    assert rc == api.PM_OK
    assert (int(k.item()) & ((1 << 64) - 1)) == kh and int(c.item()) == ch
    assert _bits_equal(Rt.cpu().numpy(), np.r_[Rh.reshape(-1), th])
    mm = m.cpu().numpy()
    assert (mm[:n] == mh).all() and not mm[n:].any()
    assert ch >= 0.5 * n and _rot_deg(Rh, Rg) < 0.1 and np.linalg.norm(th - tg) < 0.01 * max(1.0, np.linalg.norm(tg))


def test_visual_odometry_chain(ctx):
    # frames 0 / 1: relative pose and the triangulated map (pm_recover_pose's points4, in the map's scale |t01| = 1);
    # frame 2: located against that map by PnP, in the same scale
    xy0, xy1, Kg, R01, t01, X, inl = synth.calibrated_view(1500, seed=8, outlier_frac=0.2, noise_px=0.3)
    K = (Kg[0, 0], Kg[1, 1], Kg[0, 2], Kg[1, 2])
    rc, E, R1, t1, mask, ninl, ngood, key = ctx.estimate_pose(xy0, xy1, K, 1000, 1.0, 3)
    assert rc == api.PM_OK and ngood > 500
    rc, Rr, tr, mo, ng, pts = ctx.recover_pose(xy0, xy1, K, E, mask=mask, points=True)
    assert rc == api.PM_OK
    sel = mo.astype(bool)
    Xmap = (pts[sel, :3] / pts[sel, 3:4]).astype(np.float32)
    # frame 2: camera-0 coordinates -> frame 2 by a known pose; its pixels of the true points, with noise
    a = np.radians(4.0)
    R02 = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t02 = np.array([1.6, 0.1, -0.3])
    Xc = X[sel] @ R02.T + t02
    rng = np.random.default_rng(8)
    uv2 = (np.c_[K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]] + rng.normal(0, 0.3, (sel.sum(), 2)))
    rc, R2, t2, m2, c2, k2, info = ctx.solve_pnp_ransac(Xmap, uv2.astype(np.float32), K, 1000, 3.0, 5, max_iters=20)
    assert rc == api.PM_OK and c2 >= 0.9 * sel.sum()
    assert _rot_deg(R2, R02) < 0.5, _rot_deg(R2, R02)
    assert np.linalg.norm(t2 - t02) < 0.05 * np.linalg.norm(t02), (t2, t02)
