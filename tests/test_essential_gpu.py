"""GPU: calibrated relative pose (pm_ransac_essential*, pm_recover_pose*, pm_estimate_pose; docs/SPEC.md S31-S35) against
the C restatement (tests/essential_ref.c) bit for bit — every candidate of single samples, whole runs at several sizes,
views with device-side counts, mask lengths, pose recovery with its points — plus recovery of a planted pose, the
status rules and the chained device flow matcher -> ratio filter + gather -> RANSAC-E -> pose recovery with no host
round trip."""
import numpy as np
import pytest

import essential_ref as R
from points_matching_amd import api, synth

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    return (np.asarray(a, np.float64).view(np.uint64) == np.asarray(b, np.float64).view(np.uint64)).all()


def _kv(K):
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def _scene(n, seed, **kw):
    xy1, xy2, K, Rg, tg, X, inl = synth.calibrated_view(n, seed=seed, **kw)
    return xy1, xy2, _kv(K), Rg, tg, inl


def _rot_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def _dir_deg(a, b):
    return np.degrees(np.arccos(np.clip(np.dot(a, b) / np.linalg.norm(a) / np.linalg.norm(b), -1, 1)))


def test_sample_candidates_bit_parity(ctx):
    xy1, xy2, K, _, _, _ = _scene(200, seed=4, noise_px=0.7)
    xy1[5] = xy1[6]                                   # degenerate samples among the ids
    xy2[5] = xy2[6]
    xy1[9:12] = xy1[9]
    xy2[9:12] = xy2[9]
    thr = 1.5
    ok, tn = R.thr_n(K, thr)
    thr2 = np.float32(tn) * np.float32(tn)
    x1n, x2n = R.normalise(K, xy1), R.normalise(K, xy2)
    models = 0
    for h in range(1000):
        rc, E, counts, nm = ctx.ransac_essential_from_hyp(xy1, xy2, K, h, thr, 0x5EED)
        Er, vr = R.candidates(xy1, xy2, K, 0x5EED, h)
        assert rc == (api.PM_OK if vr.any() else api.PM_E_NO_MODEL)
        assert nm == vr.sum()
        assert _bits_equal(E.reshape(10, 9), Er), h
        for j in range(10):
            if vr[j]:
                assert counts[j] == R.score(Er[j], x1n, x2n, thr2)[1]
            else:
                assert counts[j] == -1
        models += nm
    assert models > 2000


@pytest.mark.parametrize("n,iters", [(5, 50), (6, 50), (127, 200), (128, 200), (129, 200), (2275, 500), (8193, 100),
                                     (32768, 40)])
def test_full_run_bit_parity(ctx, n, iters):
    xy1, xy2, K, _, _, _ = _scene(n, seed=n)
    rc, E, mask, c, key = ctx.ransac_essential(xy1, xy2, K, iters, 1.0, 0xE55)
    kr, Er, mr, cr = R.run(xy1, xy2, K, iters, 1.0, 0xE55)
    assert rc == (api.PM_OK if kr else api.PM_E_NO_MODEL)
    assert key == kr and c == cr
    assert _bits_equal(E, Er)
    assert (mask == mr).all()


def test_view_with_device_counts_and_mask_lengths(ctx):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(64)
    counts = np.minimum(rng.multinomial(9000 - 64 * 20, np.ones(64) / 64) + 20, 160)
    counts[3], counts[17] = 0, 160
    total = int(counts.sum())
    xy1, xy2, K, _, _, _ = _scene(total, seed=31)
    cap, pitch = 160, 2 * 160 + 32
    b1 = np.full((64, pitch), np.nan, np.float32)
    b2 = np.full((64, pitch), np.nan, np.float32)
    o = 0
    for p, c in enumerate(counts):
        b1[p, :2 * c] = xy1[o:o + c].reshape(-1)
        b2[p, :2 * c] = xy2[o:o + c].reshape(-1)
        o += c
    d1, d2 = torch.from_numpy(b1).to(dev), torch.from_numpy(b2).to(dev)
    dc = torch.tensor(counts.astype(np.int32), device=dev)
    view = api.PointsView(d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), 64, cap, pitch, 1, 0)
    kr, Er, mr, cr = R.run(xy1, xy2, K, 300, 1.0, 77)
    assert kr
    for mask_len in (total - 100, total, 64 * cap + 7):
        k = torch.zeros(1, dtype=torch.int64, device=dev)
        E = torch.full((9,), 7.0, dtype=torch.float64, device=dev)
        m = torch.full((mask_len,), 7, dtype=torch.uint8, device=dev)
        c = torch.full((1,), 99, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.ransac_essential_run_dev(view, K, 0, 300, 1.0, 77, k.data_ptr(), E.data_ptr(), m.data_ptr(), mask_len,
                                     c.data_ptr())
        ctx.synchronize()
        assert (int(k.item()) & ((1 << 64) - 1)) == kr and int(c.item()) == cr
        assert _bits_equal(E.cpu().numpy(), Er.reshape(-1))
        mm = m.cpu().numpy()
        w = min(mask_len, total)
        assert (mm[:w] == mr[:w]).all() and not mm[w:].any()
    # pose recovery over the same view, device-side
    Ed = torch.from_numpy(Er.reshape(-1).copy()).to(dev)
    mi = torch.from_numpy(np.r_[mr, np.zeros(64 * cap - total, np.uint8)]).to(dev)
    Rd, td = torch.zeros(9, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
    mo = torch.full((64 * cap,), 7, dtype=torch.uint8, device=dev)
    ng = torch.zeros(1, dtype=torch.int32, device=dev)
    pts = torch.zeros((64 * cap, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.recover_pose_dev(view, K, Ed.data_ptr(), mi.data_ptr(), Rd.data_ptr(), td.data_ptr(), mo.data_ptr(), ng.data_ptr(),
                         pts.data_ptr())
    ctx.synchronize()
    ngr, Rr, tr, mor, ptr_, _ = R.recover_pose(xy1, xy2, K, Er, mr)
    assert int(ng.item()) == ngr
    assert _bits_equal(Rd.cpu().numpy(), Rr.reshape(-1)) and _bits_equal(td.cpu().numpy(), tr)
    mo = mo.cpu().numpy()
    assert (mo[:total] == mor).all() and not mo[total:].any()
    assert (pts.cpu().numpy()[:total].view(np.uint32) == ptr_.view(np.uint32)).all()


@pytest.mark.parametrize("n", [6, 129, 2275, 8193])
def test_recover_pose_bit_parity(ctx, n):
    xy1, xy2, K, _, _, _ = _scene(n, seed=100 + n)
    kr, Er, mr, _ = R.run(xy1, xy2, K, 200, 1.0, 3)
    assert kr
    for mask in (mr, None):
        rc, Rg, tg, mo, ng, pts = ctx.recover_pose(xy1, xy2, K, Er, mask=mask, points=True)
        ngr, Rr, tr, mor, ptr_, _ = R.recover_pose(xy1, xy2, K, Er, mask)
        assert rc == api.PM_OK and ng == ngr
        assert _bits_equal(Rg, Rr) and _bits_equal(tg, tr)
        assert (mo == mor).all()
        assert (pts.view(np.uint32) == ptr_.view(np.uint32)).all()


@pytest.mark.parametrize("kind", ["generic", "forward", "planar"])
def test_recovers_planted_pose(ctx, kind):
    # 30% outliers, 0.5 px noise in both images, fx != fy, off-centre principal point; no refinement of E (out of scope),
    # so the bounds are those of the minimal-sample winner: measured 0.07 / 0.08 deg in R and 0.4 / 0.8 deg in t
    xy1, xy2, K, Rg, tg, inl = _scene(2000, seed=7, outlier_frac=0.3, noise_px=0.5, forward=kind == "forward",
                                      planar=kind == "planar")
    assert K[0] != K[1] and K[2] != 993 / 2
    rc, E, Rr, tr, mask, c, ng, key = ctx.estimate_pose(xy1, xy2, K, 1000, 1.0, 11)
    assert rc == api.PM_OK
    assert c >= 0.85 * inl.sum()
    kr, Er, mr, cr = R.run(xy1, xy2, K, 1000, 1.0, 11)
    assert key == kr and _bits_equal(E, Er) and (mr.astype(bool) & ~inl).sum() <= 0.02 * inl.sum()
    ngr, Rr2, tr2, mor, _, _ = R.recover_pose(xy1, xy2, K, Er, mr)
    assert ng == ngr and _bits_equal(Rr, Rr2) and _bits_equal(tr, tr2) and (mask == mor).all()
    if kind == "planar":
        return      # a plane admits two essential matrices that fit every point; which one wins is not the pose's business
    assert ng >= 0.95 * c
    assert (mask.astype(bool) & ~inl).sum() <= 0.02 * inl.sum()
    assert _rot_deg(Rr, Rg) < 0.25, _rot_deg(Rr, Rg)
    assert _dir_deg(tr, tg) < 2.0, _dir_deg(tr, tg)


def test_statuses(ctx):
    xy1, xy2, K, _, _, _ = _scene(100, seed=5)
    same = np.tile(xy1[:1], (100, 1))
    rc, E, mask, c, key = ctx.ransac_essential(same, same, K, 100, 1.0, 1)
    assert rc == api.PM_E_NO_MODEL and key == 0 and not E.any() and not mask.any()
    rc = ctx.ransac_essential(xy1[:4], xy2[:4], K, 100, 1.0, 1)[0]
    assert rc == api.PM_E_TOO_FEW
    for bad in ((0.0, 800.0, 400.0, 300.0), (800.0, -1.0, 400.0, 300.0), (800.0, 800.0, np.nan, 300.0),
                (800.0, 800.0, 400.0, np.inf)):
        with pytest.raises(api.PmError) as e:
            ctx.ransac_essential(xy1, xy2, bad, 100, 1.0, 1)
        assert e.value.status == api.PM_E_INVALID
    with pytest.raises(api.PmError) as e:
        ctx.ransac_essential(xy1, xy2, K, 100, 0.0, 1)
    assert e.value.status == api.PM_E_INVALID
    with pytest.raises(api.PmError) as e:
        ctx.ransac_essential(xy1, xy2, K, (1 << 32) // 10 + 1, 1.0, 1, hyp_begin=(1 << 32) // 10 - 5)
    assert e.value.status == api.PM_E_INVALID
    with pytest.raises(api.PmError) as e:
        ctx.ransac_essential(xy1, xy2, K, 100, 1.0, 1, kind=api.PM_ERR_SYM_EPIPOLAR)
    assert e.value.status == api.PM_E_INVALID
    rc, Rr, tr, mo, ng, _ = ctx.recover_pose(xy1, xy2, K, np.zeros(9))
    assert rc == api.PM_E_NO_MODEL and not Rr.any() and not tr.any() and not mo.any()


def test_chained_device_flow_without_host_copy(ctx):
    import torch
    dev = torch.device("cuda", 0)
    nq = nt = 1800
    w = synth.pair_workload(nq=nq, nt=nt, dim=128, seed=12, planted=0.6)
    _, _, Kg, Rg, tg, _, _ = synth.calibrated_view(4, seed=12)
    K = _kv(Kg)
    # make the scene a calibrated two-view one: every planted train keypoint is its query keypoint seen from [R|t]
    kp1, kp2 = w["kp1"], w["kp2"].copy()
    rows = np.nonzero(w["truth"] >= 0)[0]
    rng = np.random.default_rng(12)
    ray = np.column_stack([kp1[rows], np.ones(len(rows))]) @ np.linalg.inv(Kg).T
    X = ray * rng.uniform(4.0, 12.0, len(rows))[:, None]
    x2 = (X @ Rg.T + tg) @ Kg.T
    kp2[w["truth"][rows]] = (x2[:, :2] / x2[:, 2:3]).astype(np.float32)
    q, t = w["q"].astype(np.uint8), w["t"].astype(np.uint8)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        ctx.set_stream(s.cuda_stream)
        d_q, d_t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
        d_kp1, d_kp2 = torch.from_numpy(kp1).to(dev), torch.from_numpy(kp2).to(dev)
        d_knn = torch.empty((nq, 2, 4), dtype=torch.int32, device=dev)
        d_good = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
        d_xy1 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
        d_xy2 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        k = torch.zeros(1, dtype=torch.int64, device=dev)
        E = torch.zeros(9, dtype=torch.float64, device=dev)
        m = torch.zeros(nq, dtype=torch.uint8, device=dev)
        c = torch.zeros(1, dtype=torch.int32, device=dev)
        Rd, td = torch.zeros(9, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
        mo = torch.zeros(nq, dtype=torch.uint8, device=dev)
        ng = torch.zeros(1, dtype=torch.int32, device=dev)
        s.synchronize()
        ctx.bf_knn_l2_u8_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 128, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(),
                                   d_knn.data_ptr(), d_good.data_ptr(), d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr())
        view = api.PointsView(d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr(), 1, nq, 0, 1, 0)
        ctx.ransac_essential_run_dev(view, K, 0, 500, 1.0, 0xC0FFEE, k.data_ptr(), E.data_ptr(), m.data_ptr(), nq,
                                     c.data_ptr())
        ctx.recover_pose_dev(view, K, E.data_ptr(), m.data_ptr(), Rd.data_ptr(), td.data_ptr(), mo.data_ptr(),
                             ng.data_ptr())
        ctx.synchronize()
        ctx.set_stream(0)
    n = int(d_n.item())
    assert n >= 400
    xy1, xy2 = d_xy1.cpu().numpy()[:n].copy(), d_xy2.cpu().numpy()[:n].copy()
    rc, Eh, Rh, th, mh, ch, ngh, kh = ctx.estimate_pose(xy1, xy2, K, 500, 1.0, 0xC0FFEE)
    assert rc == api.PM_OK
    assert (int(k.item()) & ((1 << 64) - 1)) == kh and int(c.item()) == ch and int(ng.item()) == ngh
    assert _bits_equal(E.cpu().numpy(), Eh.reshape(-1))
    assert _bits_equal(Rd.cpu().numpy(), Rh.reshape(-1)) and _bits_equal(td.cpu().numpy(), th)
    mm = mo.cpu().numpy()
    assert (mm[:n] == mh).all() and not mm[n:].any()
    assert ch >= 0.5 * n
    assert _rot_deg(Rh, Rg) < 1.0 and _dir_deg(th, tg) < 3.0
