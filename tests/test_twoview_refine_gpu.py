"""GPU: refinement of the fundamental matrix and of the calibrated relative pose on their inliers (pm_fundamental_refine*,
pm_pose_refine*, docs/SPEC.md S43-S47) against the C restatement (tests/twoview_refine_ref.c) bit for bit — F / R / t / E
and every info field, RANSAC masks and hand-made ones, max_iters 0 / 1 / 10 / 100, the host form, the device form, in
place, views with several parts and device-side counts, masks longer than n — plus every status and error code of the
contracts in include/pm.h, the convenience calls against the two-call forms, and the two chained device flows with no
host round trip (the F one also under stream capture and replay).  The accuracy gain is tested on the restatement
(test_twoview_refine_cpu.py): the device equals it bit for bit."""
import numpy as np
import pytest

import twoview_refine_ref as TV
from points_matching_amd import api, synth

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    return (np.asarray(a, np.float64).view(np.uint64) == np.asarray(b, np.float64).view(np.uint64)).all()


def _info_equal(info, ref):
    return (_bits_equal([info.cost_in, info.cost_out], [ref.cost_in, ref.cost_out]) and
            (info.n_used, info.iters, info.status) == (ref.n_used, ref.iters, ref.status))


def _dev_info_equal(info, ref):
    return (_bits_equal([info["cost_in"], info["cost_out"]], [ref.cost_in, ref.cost_out]) and
            (int(info["n_used"]), int(info["iters"]), int(info["status"])) == (ref.n_used, ref.iters, ref.status))


def _kv(K):
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def _scene(n, seed, **kw):
    xy1, xy2, K, Rg, tg, X, inl = synth.calibrated_view(n, seed=seed, **kw)
    return xy1, xy2, _kv(K), Rg, tg, inl


def _check_f(ctx, xy1, xy2, mask, F_in, it):
    rc, F, info = ctx.fundamental_refine(xy1, xy2, mask, F_in, it)
    Fr, ir = TV.f_refine(xy1, xy2, mask, F_in, it)
    assert rc == (api.PM_E_NO_MODEL if ir.status == 2 else api.PM_OK)
    assert _bits_equal(F, Fr), (F, Fr)
    assert _info_equal(info, ir), (info.cost_in, info.cost_out, info.n_used, info.iters, info.status, ir.as_tuple())
    return F, info


def _check_pose(ctx, xy1, xy2, K, mask, R_in, t_in, it):
    rc, R, t, E, info = ctx.pose_refine(xy1, xy2, K, mask, R_in, t_in, it)
    Rr, tr, Er, ir = TV.pose_refine(xy1, xy2, K, mask, R_in, t_in, it)
    assert rc == (api.PM_E_NO_MODEL if ir.status == 2 else api.PM_OK)
    assert _bits_equal(R, Rr) and _bits_equal(t, tr) and _bits_equal(E, Er), (R, Rr, t, tr, E, Er)
    assert _info_equal(info, ir), (info.cost_in, info.cost_out, info.n_used, info.iters, info.status, ir.as_tuple())
    return R, t, E, info


def _dev_f(ctx, view, d_mask, d_Fin, it, d_Fout=None):
    import torch
    dev = torch.device("cuda", 0)
    d_info = torch.full((32,), 0xAB, dtype=torch.uint8, device=dev)
    if d_Fout is None:
        d_Fout = torch.full((9,), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.fundamental_refine_dev(view, d_mask.data_ptr(), d_Fin.data_ptr(), it, d_Fout.data_ptr(), d_info.data_ptr())
    ctx.synchronize()
    return d_Fout.cpu().numpy().reshape(3, 3), d_info.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]


def _dev_pose(ctx, view, K, d_mask, d_in, it, d_out=None):
    import torch
    dev = torch.device("cuda", 0)
    d_info = torch.full((32,), 0xAB, dtype=torch.uint8, device=dev)
    d_E = torch.full((9,), 7.0, dtype=torch.float64, device=dev)
    if d_out is None:
        d_out = torch.full((12,), 7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.pose_refine_dev(view, K, d_mask.data_ptr(), d_in.data_ptr(), it, d_out.data_ptr(), d_E.data_ptr(), d_info.data_ptr())
    ctx.synchronize()
    o = d_out.cpu().numpy()
    return o[:9].reshape(3, 3), o[9:], d_E.cpu().numpy().reshape(3, 3), d_info.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]


def _parts_view(xy1, xy2, counts, cap):
    """The correspondences split over len(counts) parts of capacity cap with NaN padding: (view, keep-alive tensors)."""
    import torch
    dev = torch.device("cuda", 0)
    pitch = 2 * cap + 64
    b1 = np.full((len(counts), pitch), np.nan, np.float32)
    b2 = np.full((len(counts), pitch), np.nan, np.float32)
    o = 0
    for p, k in enumerate(counts):
        b1[p, :2 * k] = xy1[o:o + k].reshape(-1)
        b2[p, :2 * k] = xy2[o:o + k].reshape(-1)
        o += k
    d1, d2 = torch.from_numpy(b1).to(dev), torch.from_numpy(b2).to(dev)
    dc = torch.tensor(counts, dtype=torch.int32, device=dev)
    return api.PointsView(d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), len(counts), cap, pitch, 1, 0), (d1, d2, dc)


# ---- the fundamental matrix ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 9, 511, 512, 513, 2275, 9175])
def test_f_bit_parity_on_ransac_masks(ctx, n):
    xy1, xy2, _, _ = synth.two_view(n, n, outlier_frac=0.0 if n <= 9 else 0.3)
    rc, F0, mask, c, key = ctx.ransac_fundamental(xy1, xy2, 2000, 1.0, 11)
    assert rc == api.PM_OK
    for it in (0, 1, 10, 100):
        F, info = _check_f(ctx, xy1, xy2, mask, F0, it)
        assert info.cost_out <= info.cost_in and info.n_used == c


def test_f_bit_parity_on_hand_made_masks(ctx):
    n = 2275
    xy1, xy2, _, inl = synth.two_view(n, 77, noise_px=0.7)
    rc, F0, mask, c, key = ctx.ransac_fundamental(xy1, xy2, 2000, 1.0, 5)
    masks = {"zero": np.zeros(n, np.uint8), "seven": np.zeros(n, np.uint8), "eight": np.zeros(n, np.uint8),
             "truth": inl.astype(np.uint8), "all": np.ones(n, np.uint8), "wrap": np.zeros(n, np.uint8),
             "tail": np.zeros(n, np.uint8)}
    good = np.nonzero(inl)[0]
    masks["seven"][good[:7]] = 1
    masks["eight"][good[:8]] = 1
    masks["wrap"][7::512] = 1                        # i >= P wraps onto the same partial
    masks["wrap"][good[100:120]] = 1
    masks["tail"][1800:] = inl[1800:]
    for name, m in masks.items():
        for it in (0, 1, 10):
            F, info = _check_f(ctx, xy1, xy2, m, F0, it)
            if name in ("zero", "seven"):
                assert info.status == 1 and info.iters == 0 and _bits_equal(F, F0), name
    # a zero F: status 2, PM_E_NO_MODEL
    F, info = _check_f(ctx, xy1, xy2, mask, np.zeros(9), 10)
    assert info.status == 2 and not F.any()


def test_f_view_with_device_counts_in_place_and_long_masks(ctx):
    import torch
    dev = torch.device("cuda", 0)
    xy1, xy2, _, inl = synth.two_view(2100, 31)
    rc, F0, mask, c, key = ctx.ransac_fundamental(xy1, xy2, 2000, 1.0, 77)
    tail = mask.copy()
    tail[:1700] = 0                                  # inliers only in the last part
    cap, counts = 1024, [700, 0, 1000, 400]
    view, keep = _parts_view(xy1, xy2, counts, cap)
    d_Fin = torch.from_numpy(F0.reshape(9).copy()).to(dev)
    for m in (mask, tail):
        dm = torch.ones(len(counts) * cap, dtype=torch.uint8, device=dev)      # longer than n, ones beyond it
        dm[:2100] = torch.from_numpy(m).to(dev)
        for it in (0, 10):
            F, info = _dev_f(ctx, view, dm, d_Fin, it)
            Fh, ih = TV.f_refine(xy1, xy2, m, F0, it)
            assert _bits_equal(F, Fh) and _dev_info_equal(info, ih)
    # one part with a device count below the capacity; in place (d_F_out == d_F_in)
    f1, f2 = torch.from_numpy(xy1).to(dev), torch.from_numpy(xy2).to(dev)
    dn = torch.tensor([1500], dtype=torch.int32, device=dev)
    v1 = api.PointsView(f1.data_ptr(), f2.data_ptr(), dn.data_ptr(), 1, 2100, 0, 1, 0)
    dm = torch.from_numpy(mask).to(dev)
    d_F = torch.from_numpy(F0.reshape(9).copy()).to(dev)
    F, info = _dev_f(ctx, v1, dm, d_F, 10, d_Fout=d_F)
    Fh, ih = TV.f_refine(xy1[:1500], xy2[:1500], mask[:1500], F0, 10)
    assert _bits_equal(F, Fh) and _dev_info_equal(info, ih) and ih.status == 0
    # a device count below 8: fewer than 8 inliers, F kept
    dn.fill_(7)
    d_F = torch.from_numpy(F0.reshape(9).copy()).to(dev)
    F, info = _dev_f(ctx, v1, dm, d_F, 10)
    assert int(info["status"]) == 1 and int(info["iters"]) == 0 and _bits_equal(F, F0)


def test_f_statuses_and_error_codes(ctx):
    import torch
    xy1, xy2, _, _ = synth.two_view(100, 5)
    rc, F0, mask, c, key = ctx.ransac_fundamental(xy1, xy2, 500, 1.0, 1)
    assert rc == api.PM_OK
    rc, F, info = ctx.fundamental_refine(xy1[:7], xy2[:7], mask[:7], F0, 10)
    assert rc == api.PM_E_TOO_FEW and _bits_equal(F, F0) and info.status == 1
    rc, F, info = ctx.fundamental_refine(xy1, xy2, mask, np.zeros(9), 10)
    assert rc == api.PM_E_NO_MODEL and info.status == 2 and not F.any()
    for bad in (-1, 101):
        with pytest.raises(api.PmError) as e:
            ctx.fundamental_refine(xy1, xy2, mask, F0, bad)
        assert e.value.status == api.PM_E_INVALID
        with pytest.raises(api.PmError) as e:
            ctx.ransac_fundamental_refined(xy1, xy2, 500, 1.0, 1, bad)
        assert e.value.status == api.PM_E_INVALID
    L = api.lib()
    out, inf = np.zeros(9), api.HRefineInfo()
    import ctypes as C
    p = api._p
    assert L.pm_fundamental_refine(ctx._h, None, p(xy2), 100, p(mask), p(F0.reshape(9)), 10, p(out), C.byref(inf)) == api.PM_E_INVALID
    assert L.pm_fundamental_refine(ctx._h, p(xy1), p(xy2), 100, None, p(F0.reshape(9)), 10, p(out), C.byref(inf)) == api.PM_E_INVALID
    assert L.pm_fundamental_refine(ctx._h, p(xy1), p(xy2), 100, p(mask), None, 10, p(out), C.byref(inf)) == api.PM_E_INVALID
    assert L.pm_fundamental_refine(None, p(xy1), p(xy2), 100, p(mask), p(F0.reshape(9)), 10, p(out), C.byref(inf)) == api.PM_E_INVALID
    dev = torch.device("cuda", 0)
    d = torch.zeros(64, dtype=torch.float64, device=dev)
    view = api.PointsView(d.data_ptr(), d.data_ptr(), 0, 1, 8, 0, 1, 0)
    for args in ((0, d.data_ptr(), 10, d.data_ptr()), (d.data_ptr(), 0, 10, d.data_ptr()), (d.data_ptr(), d.data_ptr(), 10, 0),
                 (d.data_ptr(), d.data_ptr(), 101, d.data_ptr())):
        with pytest.raises(api.PmError) as e:
            ctx.fundamental_refine_dev(view, *args)
        assert e.value.status == api.PM_E_INVALID
    with pytest.raises(api.PmError) as e:
        ctx.fundamental_refine_dev(api.PointsView(0, d.data_ptr(), 0, 1, 8, 0, 1, 0), d.data_ptr(), d.data_ptr(), 10, d.data_ptr())
    assert e.value.status == api.PM_E_INVALID
    # the convenience call: the RANSAC statuses, info status 2
    same = np.tile(xy1[:1], (100, 1))
    rc, F, m, c, key, info = ctx.ransac_fundamental_refined(same, same, 50, 1.0, 1, 10)
    assert rc == api.PM_E_NO_MODEL and key == 0 and not F.any() and not m.any() and info.status == 2
    assert ctx.ransac_fundamental_refined(xy1[:7], xy2[:7], 50, 1.0, 1, 10)[0] == api.PM_E_TOO_FEW
    with pytest.raises(api.PmError) as e:
        ctx.ransac_fundamental_refined(xy1, xy2, 50, 1.0, 1, 10, kind=api.PM_ERR_REPROJ)
    assert e.value.status == api.PM_E_INVALID
    with pytest.raises(api.PmError) as e:
        ctx.ransac_fundamental_refined(xy1, xy2, 0, 1.0, 1, 10)          # empty hypothesis range
    assert e.value.status == api.PM_E_INVALID


@pytest.mark.parametrize("kind", [api.PM_ERR_SAMPSON, api.PM_ERR_SYM_EPIPOLAR])
def test_f_convenience_call_equals_ransac_then_refine(ctx, kind):
    xy1, xy2, _, _ = synth.two_view(2275, 44)
    rc, F, mask, c, key, info = ctx.ransac_fundamental_refined(xy1, xy2, 3000, 1.0, 0x5EED, 10, kind=kind)
    rc0, F0, m0, c0, k0 = ctx.ransac_fundamental(xy1, xy2, 3000, 1.0, 0x5EED, kind=kind)
    rc1, F1, i1 = ctx.fundamental_refine(xy1, xy2, m0, F0, 10)
    assert rc == rc0 == rc1 == api.PM_OK and key == k0 and c == c0 and (mask == m0).all()
    assert _bits_equal(F, F1) and _info_equal(info, i1) and info.status == 0 and info.cost_out < info.cost_in


def _planted_pair(seed, Kg=None, Rg=None, tg=None):
    """A matcher workload whose planted train keypoints are the query keypoints seen from [R|t] (K None: a generic
    two-view scene through synth.two_view's cameras is not needed here; F fits any rigid scene)."""
    nq = nt = 1800
    w = synth.pair_workload(nq=nq, nt=nt, dim=128, seed=seed, planted=0.6)
    if Kg is None:
        return w, w["kp1"], w["kp2"]
    kp1, kp2 = w["kp1"], w["kp2"].copy()
    rows = np.nonzero(w["truth"] >= 0)[0]
    rng = np.random.default_rng(seed)
    ray = np.column_stack([kp1[rows], np.ones(len(rows))]) @ np.linalg.inv(Kg).T
    X = ray * rng.uniform(4.0, 12.0, len(rows))[:, None]
    x2 = (X @ Rg.T + tg) @ Kg.T
    kp2[w["truth"][rows]] = (x2[:, :2] / x2[:, 2:3]).astype(np.float32)
    return w, kp1, kp2


def test_f_chained_device_flow_without_host_copy_and_under_capture(ctx):
    """matcher -> ratio filter + gather -> pm_ransac_run_dev -> pm_fundamental_refine_dev on one stream with no host round
    trip; then RANSAC + refinement recorded into a graph and replayed (the matcher refuses a capturing stream)."""
    import gc
    import torch
    dev = torch.device("cuda", 0)
    nq = nt = 1800
    w, kp1, kp2 = _planted_pair(12)
    q, t = w["q"].astype(np.uint8), w["t"].astype(np.uint8)
    s = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(s)
    ctx.set_stream(s.cuda_stream)
    try:
        d_q, d_t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
        d_kp1, d_kp2 = torch.from_numpy(kp1).to(dev), torch.from_numpy(kp2).to(dev)
        d_knn = torch.empty((nq, 2, 4), dtype=torch.int32, device=dev)
        d_good = torch.zeros((nq, 4), dtype=torch.int32, device=dev)
        d_xy1 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
        d_xy2 = torch.zeros((nq, 2), dtype=torch.float32, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        k = torch.zeros(1, dtype=torch.int64, device=dev)
        F = torch.zeros(9, dtype=torch.float64, device=dev)
        m = torch.zeros(nq, dtype=torch.uint8, device=dev)
        c = torch.zeros(1, dtype=torch.int32, device=dev)
        Ff = torch.zeros(9, dtype=torch.float64, device=dev)
        inf = torch.zeros(32, dtype=torch.uint8, device=dev)
        s.synchronize()
        ctx.bf_knn_l2_u8_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 128, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(),
                                   d_knn.data_ptr(), d_good.data_ptr(), d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr())
        view = api.PointsView(d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr(), 1, nq, 0, 1, 0)

        def tail():
            ctx.ransac_run_dev(d_xy1.data_ptr(), d_xy2.data_ptr(), nq, d_n.data_ptr(), 0, 2000, 1.0, 0xC0FFEE, k.data_ptr(),
                               F.data_ptr(), m.data_ptr(), c.data_ptr())
            ctx.fundamental_refine_dev(view, m.data_ptr(), F.data_ptr(), 10, Ff.data_ptr(), inf.data_ptr())

        def result():
            torch.cuda.synchronize()
            return (int(k.item()), int(c.item()), F.cpu().numpy().tobytes(), Ff.cpu().numpy().tobytes(),
                    inf.cpu().numpy().tobytes(), m.cpu().numpy().tobytes())

        tail()
        base = result()
        n = int(d_n.item())
        assert n >= 400
        xy1, xy2 = d_xy1.cpu().numpy()[:n].copy(), d_xy2.cpu().numpy()[:n].copy()
        rc, Fh, mh, ch, kh, ih = ctx.ransac_fundamental_refined(xy1, xy2, 2000, 1.0, 0xC0FFEE, 10)
        assert rc == api.PM_OK and (base[0] & ((1 << 64) - 1)) == kh and base[1] == ch
        assert (m.cpu().numpy()[:n] == mh).all()
        info = inf.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]
        assert _bits_equal(Ff.cpu().numpy(), Fh.reshape(-1)) and _dev_info_equal(info, ih) and ih.status == 0
        # capture and replay
        k.zero_(); F.zero_(); Ff.zero_(); inf.zero_(); m.zero_(); c.zero_()
        gc.collect()                     # no finaliser of an earlier test's context (hipFree) inside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            tail()
        torch.cuda.set_stream(s)
        g.replay()
        assert result() == base
        del g
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        ctx.set_stream(0)


# ---- the relative pose --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [5, 6, 511, 512, 513, 2275, 9175])
def test_pose_bit_parity_on_pose_masks(ctx, n):
    xy1, xy2, K, Rg, tg, inl = _scene(n, seed=n, outlier_frac=0.0 if n <= 6 else 0.3, forward=bool(n & 1))
    if n <= 6:                                       # too few for a RANSAC worth the name: the true pose, every point
        R0, t0, pm, ng = Rg, tg, np.ones(n, np.uint8), n
    else:
        rc, E0, R0, t0, pm, c, ng, key = ctx.estimate_pose(xy1, xy2, K, 500, 1.0, 11)
        assert rc == api.PM_OK
    for it in (0, 1, 10, 100):
        R, t, E, info = _check_pose(ctx, xy1, xy2, K, pm, R0, t0, it)
        assert info.cost_out <= info.cost_in and info.n_used == ng
        if it == 0:
            assert info.status == 1 and _bits_equal(R, R0) and _bits_equal(t, t0)


def test_pose_bit_parity_on_hand_made_masks_and_poses(ctx):
    n = 2275
    xy1, xy2, K, Rg, tg, inl = _scene(n, seed=77, noise_px=0.7)
    rc, E0, R0, t0, pm, c, ng, key = ctx.estimate_pose(xy1, xy2, K, 500, 1.0, 5)
    masks = {"zero": np.zeros(n, np.uint8), "four": np.zeros(n, np.uint8), "five": np.zeros(n, np.uint8),
             "truth": inl.astype(np.uint8), "all": np.ones(n, np.uint8), "wrap": np.zeros(n, np.uint8)}
    good = np.nonzero(inl)[0]
    masks["four"][good[:4]] = 1
    masks["five"][good[:5]] = 1
    masks["wrap"][7::512] = 1
    masks["wrap"][good[100:140]] = 1
    for name, m in masks.items():
        for it in (0, 1, 10):
            R, t, E, info = _check_pose(ctx, xy1, xy2, K, m, R0, t0, it)
            if name in ("zero", "four"):
                assert info.status == 1 and info.iters == 0 and _bits_equal(R, R0) and _bits_equal(t, t0), name
    # the ground truth, a t that is not of unit length, a t of zero length, a zero pose
    _check_pose(ctx, xy1, xy2, K, pm, Rg, tg, 10)
    R, t, E, info = _check_pose(ctx, xy1, xy2, K, pm, R0, 3.5 * t0, 10)
    assert info.status == 0 and abs(np.linalg.norm(t) - 1) < 1e-15
    rc, R, t, E, info = ctx.pose_refine(xy1, xy2, K, pm, R0, np.zeros(3), 10)        # E = 0: the cost is not a number
    Rr, tr, Er, ir = TV.pose_refine(xy1, xy2, K, pm, R0, np.zeros(3), 10)
    assert rc == api.PM_OK and info.status == ir.status == 1 and info.iters == ir.iters == 0 and info.n_used == ir.n_used
    assert _bits_equal(R, R0) and not t.any() and not E.any() and _bits_equal(R, Rr) and not tr.any() and not Er.any()
    R, t, E, info = _check_pose(ctx, xy1, xy2, K, pm, np.zeros(9), np.zeros(3), 10)
    assert info.status == 2 and not R.any() and not t.any() and not E.any()


def test_pose_view_with_device_counts_in_place_and_long_masks(ctx):
    import torch
    dev = torch.device("cuda", 0)
    xy1, xy2, K, Rg, tg, inl = _scene(2100, seed=31)
    rc, E0, R0, t0, pm, c, ng, key = ctx.estimate_pose(xy1, xy2, K, 500, 1.0, 77)
    Rt0 = np.concatenate([R0.reshape(9), t0])
    tail = pm.copy()
    tail[:1700] = 0
    cap, counts = 1024, [700, 0, 1000, 400]
    view, keep = _parts_view(xy1, xy2, counts, cap)
    d_in = torch.from_numpy(Rt0.copy()).to(dev)
    for m in (pm, tail):
        dm = torch.ones(len(counts) * cap, dtype=torch.uint8, device=dev)
        dm[:2100] = torch.from_numpy(m).to(dev)
        for it in (0, 10):
            R, t, E, info = _dev_pose(ctx, view, K, dm, d_in, it)
            Rh, th, Eh, ih = TV.pose_refine(xy1, xy2, K, m, R0, t0, it)
            assert _bits_equal(R, Rh) and _bits_equal(t, th) and _bits_equal(E, Eh) and _dev_info_equal(info, ih)
    f1, f2 = torch.from_numpy(xy1).to(dev), torch.from_numpy(xy2).to(dev)
    dn = torch.tensor([1500], dtype=torch.int32, device=dev)
    v1 = api.PointsView(f1.data_ptr(), f2.data_ptr(), dn.data_ptr(), 1, 2100, 0, 1, 0)
    dm = torch.from_numpy(pm).to(dev)
    d_Rt = torch.from_numpy(Rt0.copy()).to(dev)
    R, t, E, info = _dev_pose(ctx, v1, K, dm, d_Rt, 10, d_out=d_Rt)
    Rh, th, Eh, ih = TV.pose_refine(xy1[:1500], xy2[:1500], K, pm[:1500], R0, t0, 10)
    assert _bits_equal(R, Rh) and _bits_equal(t, th) and _bits_equal(E, Eh) and _dev_info_equal(info, ih) and ih.status == 0
    dn.fill_(4)
    d_Rt = torch.from_numpy(Rt0.copy()).to(dev)
    R, t, E, info = _dev_pose(ctx, v1, K, dm, d_Rt, 10)
    assert int(info["status"]) == 1 and int(info["iters"]) == 0 and _bits_equal(R, R0) and _bits_equal(t, t0)
    # d_E_out and d_info may be null
    d_out = torch.zeros(12, dtype=torch.float64, device=dev)
    dn.fill_(1500)
    ctx.pose_refine_dev(v1, K, dm.data_ptr(), d_Rt.data_ptr(), 10, d_out.data_ptr())
    ctx.synchronize()
    assert _bits_equal(d_out.cpu().numpy(), np.concatenate([Rh.reshape(9), th]))


def test_pose_statuses_and_error_codes(ctx):
    import ctypes as C
    import torch
    xy1, xy2, K, Rg, tg, inl = _scene(100, seed=5)
    m = inl.astype(np.uint8)
    rc, R, t, E, info = ctx.pose_refine(xy1[:4], xy2[:4], K, m[:4], Rg, tg, 10)
    assert rc == api.PM_E_TOO_FEW and _bits_equal(R, Rg) and _bits_equal(t, tg) and info.status == 1
    rc, R, t, E, info = ctx.pose_refine(xy1, xy2, K, m, np.zeros(9), np.zeros(3), 10)
    assert rc == api.PM_E_NO_MODEL and info.status == 2 and not R.any() and not t.any() and not E.any()
    for bad in (-1, 101):
        with pytest.raises(api.PmError) as e:
            ctx.pose_refine(xy1, xy2, K, m, Rg, tg, bad)
        assert e.value.status == api.PM_E_INVALID
        with pytest.raises(api.PmError) as e:
            ctx.estimate_pose_refined(xy1, xy2, K, 100, 1.0, 1, bad)
        assert e.value.status == api.PM_E_INVALID
    for bad in ((0.0, 800.0, 400.0, 300.0), (800.0, -1.0, 400.0, 300.0), (800.0, 800.0, np.nan, 300.0),
                (800.0, 800.0, 400.0, np.inf)):
        with pytest.raises(api.PmError) as e:
            ctx.pose_refine(xy1, xy2, bad, m, Rg, tg, 10)
        assert e.value.status == api.PM_E_INVALID
        with pytest.raises(api.PmError) as e:
            ctx.estimate_pose_refined(xy1, xy2, bad, 100, 1.0, 1, 10)
        assert e.value.status == api.PM_E_INVALID
    L, p = api.lib(), api._p
    cam = api._camera(K)
    Rin, tin, Ro, to, inf = Rg.reshape(9).copy(), tg.copy(), np.zeros(9), np.zeros(3), api.HRefineInfo()

    def call(ctxh=ctx._h, a1=p(xy1), k=C.byref(cam), mk=p(m), r=p(Rin), tt=p(tin), ro=p(Ro)):
        return L.pm_pose_refine(ctxh, a1, p(xy2), 100, k, mk, r, tt, 10, ro, p(to), None, C.byref(inf))

    assert call() == api.PM_OK                       # E_out may be null
    assert call(ctxh=None) == api.PM_E_INVALID
    assert call(a1=None) == api.PM_E_INVALID
    assert call(k=None) == api.PM_E_INVALID
    assert call(mk=None) == api.PM_E_INVALID
    assert call(r=None) == api.PM_E_INVALID
    assert call(tt=None) == api.PM_E_INVALID
    assert call(ro=None) == api.PM_E_INVALID
    dev = torch.device("cuda", 0)
    d = torch.zeros(64, dtype=torch.float64, device=dev)
    view = api.PointsView(d.data_ptr(), d.data_ptr(), 0, 1, 8, 0, 1, 0)
    for args in ((0, d.data_ptr(), 10, d.data_ptr()), (d.data_ptr(), 0, 10, d.data_ptr()), (d.data_ptr(), d.data_ptr(), 10, 0),
                 (d.data_ptr(), d.data_ptr(), -1, d.data_ptr())):
        with pytest.raises(api.PmError) as e:
            ctx.pose_refine_dev(view, K, *args)
        assert e.value.status == api.PM_E_INVALID
    with pytest.raises(api.PmError) as e:
        ctx.pose_refine_dev(view, (0.0, 1.0, 1.0, 1.0), d.data_ptr(), d.data_ptr(), 10, d.data_ptr())
    assert e.value.status == api.PM_E_INVALID
    # the convenience call: the statuses of pm_estimate_pose, info status 2
    same = np.tile(xy1[:1], (100, 1))
    rc, E, R, t, mk, c, ng, key, info = ctx.estimate_pose_refined(same, same, K, 100, 1.0, 1, 10)
    assert rc == api.PM_E_NO_MODEL and key == 0 and not E.any() and not R.any() and not t.any() and info.status == 2
    assert ctx.estimate_pose_refined(xy1[:4], xy2[:4], K, 100, 1.0, 1, 10)[0] == api.PM_E_TOO_FEW


def test_pose_convenience_call_equals_estimate_then_refine(ctx):
    xy1, xy2, K, Rg, tg, inl = _scene(2275, seed=44)
    rc, E, R, t, mask, c, ng, key, info = ctx.estimate_pose_refined(xy1, xy2, K, 1000, 1.0, 0x5EED, 20)
    rc0, E0, R0, t0, m0, c0, ng0, k0 = ctx.estimate_pose(xy1, xy2, K, 1000, 1.0, 0x5EED)
    rc1, R1, t1, E1, i1 = ctx.pose_refine(xy1, xy2, K, m0, R0, t0, 20)
    assert rc == rc0 == rc1 == api.PM_OK and key == k0 and c == c0 and ng == ng0 and (mask == m0).all()
    assert _bits_equal(R, R1) and _bits_equal(t, t1) and _bits_equal(E, E1) and _info_equal(info, i1)
    assert info.status == 0 and info.cost_out < info.cost_in
    # pm_estimate_pose itself is unchanged by the third step: the same bits as the restatement's chain gives
    import essential_ref as ER
    kr, Er, mr, cr = ER.run(xy1, xy2, K, 1000, 1.0, 0x5EED)
    assert kr == k0 and _bits_equal(Er, E0)


def test_pose_chained_device_flow_without_host_copy(ctx):
    """matcher -> ratio filter + gather -> pm_ransac_essential_run_dev -> pm_recover_pose_dev -> pm_pose_refine_dev (in
    place on the 12 doubles pm_recover_pose_dev wrote) with no host round trip, against the host forms."""
    import torch
    dev = torch.device("cuda", 0)
    nq = nt = 1800
    _, _, Kg, Rg, tg, _, _ = synth.calibrated_view(4, seed=12)
    K = _kv(Kg)
    w, kp1, kp2 = _planted_pair(12, Kg, Rg, tg)
    q, t = w["q"].astype(np.uint8), w["t"].astype(np.uint8)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        ctx.set_stream(s.cuda_stream)
        try:
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
            Rt = torch.zeros(12, dtype=torch.float64, device=dev)
            Ef = torch.zeros(9, dtype=torch.float64, device=dev)
            mo = torch.zeros(nq, dtype=torch.uint8, device=dev)
            ng = torch.zeros(1, dtype=torch.int32, device=dev)
            inf = torch.zeros(32, dtype=torch.uint8, device=dev)
            s.synchronize()
            ctx.bf_knn_l2_u8_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 128, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(),
                                       d_knn.data_ptr(), d_good.data_ptr(), d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr())
            view = api.PointsView(d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr(), 1, nq, 0, 1, 0)
            ctx.ransac_essential_run_dev(view, K, 0, 500, 1.0, 0xC0FFEE, k.data_ptr(), E.data_ptr(), m.data_ptr(), nq,
                                         c.data_ptr())
            ctx.recover_pose_dev(view, K, E.data_ptr(), m.data_ptr(), Rt.data_ptr(), Rt.data_ptr() + 72, mo.data_ptr(),
                                 ng.data_ptr())
            ctx.pose_refine_dev(view, K, mo.data_ptr(), Rt.data_ptr(), 20, Rt.data_ptr(), Ef.data_ptr(), inf.data_ptr())
            ctx.synchronize()
        finally:
            ctx.set_stream(0)
    n = int(d_n.item())
    assert n >= 400
    xy1, xy2 = d_xy1.cpu().numpy()[:n].copy(), d_xy2.cpu().numpy()[:n].copy()
    rc, Eh, Rh, th, mh, ch, ngh, kh, ih = ctx.estimate_pose_refined(xy1, xy2, K, 500, 1.0, 0xC0FFEE, 20)
    assert rc == api.PM_OK
    assert (int(k.item()) & ((1 << 64) - 1)) == kh and int(c.item()) == ch and int(ng.item()) == ngh
    o = Rt.cpu().numpy()
    assert _bits_equal(o[:9], Rh.reshape(-1)) and _bits_equal(o[9:], th) and _bits_equal(Ef.cpu().numpy(), Eh.reshape(-1))
    info = inf.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]
    assert _dev_info_equal(info, ih) and ih.status == 0
    assert (mo.cpu().numpy()[:n] == mh).all()
