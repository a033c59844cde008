"""GPU: triangulation (pm_triangulate*, docs/SPEC.md S93-S96) against the C restatement (tests/triangulate_ref.c) bit for bit —
every output at the wave and workgroup edges for 2 .. 8 views with blanked observations and a device-side count, the host
form, PM_TRI_USE_INITIAL on a perturbed map and over its own output — plus agreement with pm_recover_pose_dev's points4,
recovery of clean tracks and rejection of spoilt ones, the chain relative pose -> triangulated map -> PnP of a third view on
one stream, capture and replay, and every PM_E_INVALID with the outputs untouched."""
import numpy as np
import pytest

import points_matching_amd as pm
import triangulate_ref as T
from points_matching_amd import api, synth

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 2500)     # the wave (64) and workgroup (256) edges, and more than one workgroup
GUARD = 7.0
_scenes = {}


def _scene(n_views):
    """One scene per view count, computed once: 2500 + 5 rows, ~10 % of the observations blanked, every 9th track spoilt."""
    if n_views not in _scenes:
        _scenes[n_views] = T.scene(SIZES[-1] + 5, n_views, 40 + n_views, blank_frac=0.1, swap_every=9)
    return _scenes[n_views]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


class _Dev:
    """The device side of one call: views, poses, outputs filled with guard values."""

    def __init__(self, uv, Rt, cap, count=None, xyz0=None):
        import torch
        self.torch, dev = torch, torch.device("cuda", 0)
        self.uv = [torch.from_numpy(np.ascontiguousarray(u[:cap])).to(dev) for u in uv]
        self.Rt = [None if r is None else torch.from_numpy(np.ascontiguousarray(r, np.float64)).to(dev) for r in Rt]
        self.count = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
        self.xyz = torch.full((cap, 3), GUARD, dtype=torch.float32, device=dev)
        if xyz0 is not None:
            self.xyz[:len(xyz0)] = torch.from_numpy(np.ascontiguousarray(xyz0, np.float32)).to(dev)
        self.status = torch.full((cap,), 7, dtype=torch.uint8, device=dev)
        self.points4 = torch.full((cap, 4), GUARD, dtype=torch.float32, device=dev)
        self.err2 = torch.full((cap,), GUARD, dtype=torch.float32, device=dev)
        self.n_good = torch.full((1,), -5, dtype=torch.int32, device=dev)
        self.views = api.tri_views([u.data_ptr() for u in self.uv], [None if r is None else r.data_ptr() for r in self.Rt], cap,
                                   None if self.count is None else self.count.data_ptr())
        torch.cuda.synchronize()

    def run(self, ctx, K, prm):
        ctx.triangulate_dev(self.views, K, prm, self.xyz.data_ptr(), self.status.data_ptr(), self.points4.data_ptr(),
                            self.err2.data_ptr(), self.n_good.data_ptr())
        ctx.synchronize()
        return (self.xyz.cpu().numpy(), self.status.cpu().numpy(), self.points4.cpu().numpy(), self.err2.cpu().numpy(),
                int(self.n_good.item()))


def _assert_parity(got, ref, n, initial=False):
    xyz, status, points4, err2, n_good = got
    assert (status[:n] == ref.status).all() and n_good == ref.n_good
    assert (_bits(xyz[:n]) == _bits(ref.xyz)).all() and (_bits(err2[:n]) == _bits(ref.err2)).all()
    if initial:
        assert (points4 == GUARD).all()                         # not written under PM_TRI_USE_INITIAL
    else:
        assert (_bits(points4[:n]) == _bits(ref.points4)).all() and (points4[n:] == GUARD).all()
    assert (xyz[n:] == GUARD).all() and (status[n:] == 7).all() and (err2[n:] == GUARD).all()   # rows past the count survive


@pytest.mark.parametrize("max_iters", [0, 10])
@pytest.mark.parametrize("n_views", [2, 3, 4, 5, 8])
def test_bit_parity_at_wave_and_workgroup_edges(ctx, n_views, max_iters):
    K, uv, Rt, X, _ = _scene(n_views)
    prm = api.tri_params(3.0, 0.9998, 11.0, max_iters)
    seen = set()
    for n in SIZES:
        cap = n + 5
        ref = T.run(K, [u[:n] for u in uv], Rt, 3.0, 0.9998, 11.0, max_iters)
        got = _Dev(uv, Rt, cap, count=n).run(ctx, K, prm)
        _assert_parity(got, ref, n)
        seen |= set(ref.status.tolist())
    assert {T.OK, T.DEPTH, T.REPROJ} <= seen and (n_views > 3 or T.FEW_VIEWS in seen)


@pytest.mark.parametrize("n_views", [6, 7])
def test_bit_parity_of_the_other_instantiations(ctx, n_views):
    """6 and 7 views have kernels of their own: one size past a workgroup each, linear only and refined."""
    K, uv, Rt, X, _ = _scene(n_views)
    n = 257
    for max_iters in (0, 10):
        ref = T.run(K, [u[:n] for u in uv], Rt, 3.0, 0.9998, 11.0, max_iters)
        _assert_parity(_Dev(uv, Rt, n + 5, count=n).run(ctx, K, api.tri_params(3.0, 0.9998, 11.0, max_iters)), ref, n)
        assert {T.OK, T.DEPTH, T.REPROJ} <= set(ref.status.tolist())


def test_host_form_and_null_count_and_optional_outputs(ctx):
    K, uv, Rt, X, _ = _scene(3)
    n = 1000
    ref = T.run(K, [u[:n] for u in uv], Rt, 2.5, 0.9999, np.inf, 10)
    xyz, status, p4, e2, ng = ctx.triangulate([u[:n] for u in uv], Rt, K, api.tri_params(2.5, 0.9999, float("inf"), 10))
    assert (status == ref.status).all() and ng == ref.n_good
    assert all((_bits(a) == _bits(b)).all() for a, b in ((xyz, ref.xyz), (p4, ref.points4), (e2, ref.err2)))
    d = _Dev(uv, Rt, n)                                          # count NULL: cap rows; the optional outputs NULL
    ctx.triangulate_dev(d.views, K, api.tri_params(2.5, 0.9999, float("inf"), 10), d.xyz.data_ptr(), d.status.data_ptr())
    ctx.synchronize()
    assert (_bits(d.xyz.cpu().numpy()) == _bits(ref.xyz)).all() and (d.status.cpu().numpy() == ref.status).all()
    assert (d.points4 == GUARD).all() and (d.err2 == GUARD).all() and int(d.n_good.item()) == -5
    # a count outside [0, cap] is clamped; 0 writes nothing but the count of good rows
    for count, rows in ((-3, 0), (0, 0), (n + 100, n)):
        d = _Dev(uv, Rt, n, count=count)
        got = d.run(ctx, K, api.tri_params(2.5, 0.9999, float("inf"), 10))
        assert got[4] == (ref.n_good if rows else 0) and (got[1][:rows] == ref.status[:rows]).all() and (got[1][rows:] == 7).all()
    assert ctx.triangulate([u[:0] for u in uv], Rt, K)[4] == 0


@pytest.mark.parametrize("n_views", [2, 5])
def test_use_initial_on_a_perturbed_map_and_over_its_own_output(ctx, n_views):
    K, uv, Rt, X, _ = _scene(n_views)
    n, cap = 2500, 2505
    rng = np.random.default_rng(3)
    xyz0 = (X[:n] + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
    xyz0[5], xyz0[77, 1], xyz0[300, 2] = np.nan, np.inf, -4.0    # no start, no start, a start behind the camera
    ref = T.run(K, [u[:n] for u in uv], Rt, 3.0, 0.9998, np.inf, 10, flags=T.USE_INITIAL, xyz0=xyz0)
    assert ref.status[5] == ref.status[77] == T.DEGENERATE or T.FEW_VIEWS in (ref.status[5], ref.status[77])
    got = _Dev(uv, Rt, cap, count=n, xyz0=xyz0).run(ctx, K, api.tri_params(3.0, 0.9998, float("inf"), 10, api.PM_TRI_USE_INITIAL))
    _assert_parity(got, ref, n, initial=True)
    # clean tracks: a full run, then a second pass over its own output in place; settled rows (triangulate_ref.settled, nearly
    # all of them here) keep every bit although LM takes steps from the f32-rounded start
    K, uv, Rt, X, _ = T.clean_scene(n_views)
    first = T.run(K, uv, Rt, 3.0, 0.9998, np.inf, 100)
    d = _Dev(uv, Rt, cap, count=n)
    one = d.run(ctx, K, api.tri_params(3.0, 0.9998, float("inf"), 100))
    _assert_parity(one, first, n)
    two = d.run(ctx, K, api.tri_params(3.0, 0.9998, float("inf"), 100, api.PM_TRI_USE_INITIAL))
    s = T.settled(first, 100, n_views)
    assert s.sum() > 1900 and (two[1][:n][s] == T.OK).all() and (_bits(two[0][:n][s]) == _bits(one[0][:n][s])).all()
    again = T.run(K, uv, Rt, 3.0, 0.9998, np.inf, 100, flags=T.USE_INITIAL, xyz0=one[0][:n])
    assert (_bits(two[0][:n]) == _bits(again.xyz)).all() and (two[1][:n] == again.status).all() and two[4] == again.n_good
    assert (again.cost_fin[s] < again.cost_lin[s]).sum() > 1900


def test_points4_equals_recover_pose_dev(ctx):
    """Two views, Rt[0] = NULL, Rt[1] the R, t pm_recover_pose_dev wrote, max_iters 0: the same arithmetic, so points4 equals
    that call's under == on every row."""
    import torch
    dev = torch.device("cuda", 0)
    n = 1500
    xy0, xy1, Kg, R01, t01, X, inl = synth.calibrated_view(n, seed=8, outlier_frac=0.2, noise_px=0.3)
    K = (Kg[0, 0], Kg[1, 1], Kg[0, 2], Kg[1, 2])
    rc, E, R1, t1, mask, ninl, ngood, key = ctx.estimate_pose(xy0, xy1, K, 1000, 1.0, 3)
    assert rc == api.PM_OK
    d0, d1 = torch.from_numpy(xy0).to(dev), torch.from_numpy(xy1).to(dev)
    dE, dm = torch.from_numpy(E.reshape(-1).copy()).to(dev), torch.from_numpy(mask).to(dev)
    Rt = torch.zeros(12, dtype=torch.float64, device=dev)
    mo, ng = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    p4r = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    xyz, st = torch.zeros((n, 3), dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    p4t = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    view = api.PointsView(d0.data_ptr(), d1.data_ptr(), None, 1, n, 0, 1, 0)
    ctx.recover_pose_dev(view, K, dE.data_ptr(), dm.data_ptr(), Rt.data_ptr(), Rt.data_ptr() + 72, mo.data_ptr(), ng.data_ptr(),
                         p4r.data_ptr())
    ctx.triangulate_dev(api.tri_views([d0.data_ptr(), d1.data_ptr()], [None, Rt.data_ptr()], n), K,
                        api.tri_params(3.0, 0.9998, 50.0, 0), xyz.data_ptr(), st.data_ptr(), p4t.data_ptr())
    ctx.synchronize()
    a, b = p4r.cpu().numpy(), p4t.cpu().numpy()
    assert np.isfinite(a).all() and (a == b).all()
    # and with max_depth = that call's dist the depth gate is its cheirality test: no RANSAC inlier it refused is kept here
    ok = st.cpu().numpy() == T.OK
    assert ok.sum() > 0.7 * n and not (ok & (mo.cpu().numpy() == 0) & (mask != 0)).any()


@pytest.mark.parametrize("seed", T.RECOVERY["seeds"])
def test_recovers_clean_tracks_and_rejects_spoilt_ones(ctx, seed):
    # tests/test_triangulate_cpu.py asserts that a float64 numpy reference alone meets both conditions on these seeds
    K, uv, Rt, X, touched = T.recovery_scene(seed)
    xyz, status, p4, e2, ng = ctx.triangulate(uv, Rt, K, api.tri_params(T.RECOVERY["max_reproj_px"], T.RECOVERY["max_cos_parallax"],
                                                                         float("inf"), 10))
    assert (status[~touched] == T.OK).all() and (status[touched] != T.OK).all() and ng == (~touched).sum()
    assert np.abs(xyz[~touched] - X[~touched]).max() < 0.25 and e2[~touched].max() <= 9.0


def _rot_deg(Ra, Rb):
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def test_chain_pose_map_pnp_on_one_stream(ctx):
    """calibrated view -> RANSAC-E -> pose recovery -> pose refinement (into the 12 doubles the triangulation reads as Rt[1])
    -> triangulation -> RANSAC-PnP + refinement of a third view against the NaN-bearing map, no host round trip.  The third
    pose against the truth at the tolerances of test_pnp_gpu.py's visual-odometry chain (|t01| = 1 is the scene's scale)."""
    import torch
    dev = torch.device("cuda", 0)
    n = 1500
    xy0, xy1, Kg, R01, t01, X, inl = synth.calibrated_view(n, seed=8, outlier_frac=0.2, noise_px=0.3)
    K = (Kg[0, 0], Kg[1, 1], Kg[0, 2], Kg[1, 2])
    a = np.radians(4.0)
    R02 = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t02 = np.array([1.6, 0.1, -0.3])
    Xc = X @ R02.T + t02
    uv2 = (np.c_[K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]] +
           np.random.default_rng(8).normal(0, 0.3, (n, 2))).astype(np.float32)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        ctx.set_stream(s.cuda_stream)
        try:
            d0, d1, d2 = (torch.from_numpy(x).to(dev) for x in (xy0, xy1, uv2))
            k, k2 = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
            E = torch.zeros(9, dtype=torch.float64, device=dev)
            m, mo, m2 = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(3))
            c, ng, c2, good = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(4))
            Rt, Rt2 = torch.zeros(12, dtype=torch.float64, device=dev), torch.zeros(12, dtype=torch.float64, device=dev)
            xyz = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            st = torch.zeros(n, dtype=torch.uint8, device=dev)
            s.synchronize()
            view = api.PointsView(d0.data_ptr(), d1.data_ptr(), None, 1, n, 0, 1, 0)
            ctx.ransac_essential_run_dev(view, K, 0, 1000, 1.0, 3, k.data_ptr(), E.data_ptr(), m.data_ptr(), n, c.data_ptr())
            ctx.recover_pose_dev(view, K, E.data_ptr(), m.data_ptr(), Rt.data_ptr(), Rt.data_ptr() + 72, mo.data_ptr(), ng.data_ptr())
            ctx.pose_refine_dev(view, K, mo.data_ptr(), Rt.data_ptr(), 20, Rt.data_ptr())
            ctx.triangulate_dev(api.tri_views([d0.data_ptr(), d1.data_ptr()], [None, Rt.data_ptr()], n), K,
                                api.tri_params(3.0, 0.9998, 50.0, 10), xyz.data_ptr(), st.data_ptr(), None, None, good.data_ptr())
            pv = api.PnpView(xyz.data_ptr(), d2.data_ptr(), None, n, 0)
            ctx.ransac_pnp_run_dev(pv, K, 0, 1000, 3.0, 5, k2.data_ptr(), Rt2.data_ptr(), m2.data_ptr(), n, c2.data_ptr())
            ctx.pnp_refine_dev(pv, K, m2.data_ptr(), Rt2.data_ptr(), 20, Rt2.data_ptr())
            ctx.synchronize()
        finally:
            ctx.set_stream(0)
    sth, xyzh, m2h = st.cpu().numpy(), xyz.cpu().numpy(), m2.cpu().numpy()
    ok = sth == T.OK
    assert int(good.item()) == ok.sum() > 0.7 * n and (np.isnan(xyzh).all(1) == ~ok).all()
    assert not m2h[~ok].any() and int(c2.item()) >= 0.9 * ok.sum()        # a NaN row is never a PnP inlier
    o = Rt2.cpu().numpy()
    R2, t2 = o[:9].reshape(3, 3), o[9:]
    assert _rot_deg(R2, R02) < 0.5, _rot_deg(R2, R02)
    assert np.linalg.norm(t2 - t02) < 0.05 * np.linalg.norm(t02), (t2, t02)


def test_capture_and_replay():
    import gc
    import torch
    dev = torch.device("cuda", 0)
    K, uv, Rt, X, _ = _scene(4)
    n = 700
    ref = T.run(K, [u[:n] for u in uv], Rt, 3.0, 0.9998, np.inf, 5)
    st = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(st)
    c = pm.Context(0)
    c.set_stream(st.cuda_stream)
    try:
        d = _Dev(uv, Rt, n)
        prm = api.tri_params(3.0, 0.9998, float("inf"), 5)
        gc.collect()                 # no finaliser of an earlier test's context (hipFree) inside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st, capture_error_mode="relaxed"):
            c.triangulate_dev(d.views, K, prm, d.xyz.data_ptr(), d.status.data_ptr(), d.points4.data_ptr(), d.err2.data_ptr(),
                              d.n_good.data_ptr())
        torch.cuda.set_stream(st)
        for _ in range(2):
            d.xyz.fill_(GUARD)
            d.n_good.fill_(-5)
            g.replay()
            torch.cuda.synchronize()
            assert int(d.n_good.item()) == ref.n_good and (_bits(d.xyz.cpu().numpy()) == _bits(ref.xyz)).all()
        del g
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        c.close()


def test_invalid_arguments_leave_the_outputs_untouched(ctx):
    K, uv, Rt, X, _ = _scene(3)
    n = 100
    d = _Dev(uv, Rt, n)
    good = api.tri_params()
    inf = float("inf")

    def refused(views=d.views, k=K, prm=good, xyz=True, status=True, host=False):
        with pytest.raises(pm.PmError) as e:
            if host:
                ctx.triangulate(*views, k, prm)
            else:
                ctx.triangulate_dev(views, k, prm, d.xyz.data_ptr() if xyz else None, d.status.data_ptr() if status else None,
                                    d.points4.data_ptr(), d.err2.data_ptr(), d.n_good.data_ptr())
        ctx.synchronize()
        assert e.value.status == api.PM_E_INVALID, e.value
        assert (d.xyz == GUARD).all() and (d.status == 7).all() and (d.points4 == GUARD).all() and (d.err2 == GUARD).all()
        assert int(d.n_good.item()) == -5
        return True

    def views(n_views=3, cap=n, hole=False):
        v = api.tri_views([u.data_ptr() for u in d.uv], [None if r is None else r.data_ptr() for r in d.Rt], cap)
        v.n_views = n_views
        if hole:
            v.uv[2] = None
        return v

    assert refused(xyz=False) and refused(status=False)
    for nv in (-1, 0, 1, 9):
        assert refused(views=views(n_views=nv))
    assert refused(views=views(cap=-1)) and refused(views=views(hole=True))
    for k in ((800.0, -1.0, 320.0, 240.0), (0.0, 800.0, 320.0, 240.0), (800.0, 800.0, float("nan"), 240.0), (inf, 800.0, 320.0, 240.0)):
        assert refused(k=k)
    bad = [api.tri_params(max_reproj_px=v) for v in (0.0, -1.0, inf, float("nan"))]
    bad += [api.tri_params(max_cos_parallax=v) for v in (-1.0, 1.0000001, float("nan"))]
    bad += [api.tri_params(max_depth=v) for v in (0.0, -3.0, float("nan"))]
    bad += [api.tri_params(max_iters=v) for v in (-1, 101)] + [api.tri_params(flags=v) for v in (2, 3, -1)]
    for prm in bad:
        assert refused(prm=prm)
        assert refused(views=([u[:n] for u in uv], Rt), prm=prm, host=True)
    assert refused(views=([u[:n] for u in uv[:1]], Rt[:1]), host=True)           # one view
    L = api.lib()
    assert L.pm_triangulate_dev(None, None, None, None, None, None, None, None, None) == api.PM_E_INVALID
    assert L.pm_triangulate(None, None, None, 3, n, None, None, None, None, None, None, None) == api.PM_E_INVALID
    # and the call still works
    ref = T.run(K, [u[:n] for u in uv], Rt)
    _assert_parity(d.run(ctx, K, good), ref, n)
