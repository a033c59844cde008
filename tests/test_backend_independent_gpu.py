"""GPU: the 3-D back end — triangulation (pm_triangulate*, SPEC S93-S96), 3-D alignment (pm_ransac_align3d*,
pm_align3d_refine*, pm_transform_points3*, S97-S101) and bundle adjustment (pm_bundle_adjust*, S113-S117) — at hard geometry:
every case of the three tables of tests/backend_cases.py (maps 1e4 units from the origin, turns of 60 and 180 degrees,
parallax of 1e-3, depths of 1:1000, 16000 px images, scales of 1e-3 .. 1e3, exactly flat and collinear clouds, non-finite
rows), through the device forms and the host forms.  Every output is first compared with the C restatement bit for bit
(doubles as u64, floats as u32, statuses, masks, counts, info records, guard values behind every buffer); then the
independent checks of tests/test_backend_independent_cpu.py run on the device's own output, with the same helpers and the
same tolerances.  No new kernel shapes: the wave and workgroup edges are test_triangulate_gpu.py's, test_align3d_gpu.py's
and test_bundle_adjust_gpu.py's.  The twin of tests/test_pose_independent_gpu.py for the back end."""
import numpy as np
import pytest

import align3d_ref as AR
import ba_ref as B
import backend_cases as BC
import triangulate_ref as T
from points_matching_amd import api
from test_bundle_adjust_gpu import _assert_parity as ba_parity
from test_bundle_adjust_gpu import _Dev as BaDev
from test_triangulate_gpu import _assert_parity as tri_parity
from test_triangulate_gpu import _Dev as TriDev

pytestmark = pytest.mark.gpu

TRI_RUNS = [(name, V) for name in BC.TRI_NAMES for V in BC.TRI_VIEWS]
ALIGN_RUNS = BC.ALIGN_RUNS
BA_RUNS = BC.BA_RUNS
PAD = 5                       # rows past the count, which no call may read into its result or write
U64 = (1 << 64) - 1


def _pad(a, fill):
    return np.r_[a, np.full((PAD,) + a.shape[1:], fill, a.dtype)]


def _same(a, b):
    return (BC.bits(np.ascontiguousarray(a)) == BC.bits(np.ascontiguousarray(b))).all()


# ---- triangulation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,V", TRI_RUNS)
def test_triangulation_at_hard_geometry(ctx, name, V):
    K, uv, Rt, _, _, _ = BC.tri_scene(name, V)
    g, n = BC.tri_gates(name), BC.TRI_N
    uvp = [_pad(u, np.nan) for u in uv]
    for initial in (False, True):
        x0 = BC.tri_start(name, V) if initial else None
        flags = api.PM_TRI_USE_INITIAL if initial else 0
        ref = T.run(K, uv, Rt, g[0], g[1], g[2], 100, flags=flags, xyz0=x0)
        prm = api.tri_params(g[0], g[1], float(g[2]), 100, flags)
        got = TriDev(uvp, Rt, n + PAD, count=n, xyz0=x0).run(ctx, K, prm)
        tri_parity(got, ref, n, initial=initial)
        xyz, status, p4, e2, ng = ctx.triangulate(uv, Rt, K, prm, xyz0=x0)                  # the host form
        assert (status == ref.status).all() and ng == ref.n_good and _same(xyz, ref.xyz) and _same(e2, ref.err2)
        assert _same(p4, ref.points4)
        # the independent checks on the device's own output (xyz64 never leaves the device: the restatement's, whose f32
        # rounding was just compared)
        out = BC.Out(xyz=got[0][:n], status=got[1][:n], points4=got[2][:n], err2=got[3][:n], n_good=got[4], xyz64=ref.xyz64)
        BC.tri_checks(name, V, out, initial=initial)


# ---- 3-D alignment ---------------------------------------------------------------------------------------------------------
def _align_dev(ctx, model, x1, x2, thresh, seed, mask_in, start):
    """pm_ransac_align3d_run_dev, pm_align3d_refine_dev and pm_transform_points3_dev on a view with a device-side count, every
    output poisoned and guarded: (key, T, mask, count), (T refit, info record), transformed rows."""
    import torch
    dev = torch.device("cuda", 0)
    n, cap, guard = len(x1), len(x1) + PAD, 64
    d1, d2 = torch.from_numpy(_pad(x1, 7.0)).to(dev), torch.from_numpy(_pad(x2, 7.0)).to(dev)
    dn = torch.tensor([n], dtype=torch.int32, device=dev)
    view = api.XyzView(d1.data_ptr(), d2.data_ptr(), dn.data_ptr(), cap, 0)
    k = torch.zeros(1, dtype=torch.int64, device=dev)
    Tw = torch.full((13 + 2,), 7.0, dtype=torch.float64, device=dev)
    m = torch.full((cap + guard,), 7, dtype=torch.uint8, device=dev)
    c = torch.full((1,), 99, dtype=torch.int32, device=dev)
    dm = torch.from_numpy(_pad(np.ascontiguousarray(mask_in, np.uint8), 1)).to(dev)      # rows past the count: never read
    dT = torch.from_numpy(np.r_[np.asarray(start, np.float64), 7.0, 7.0]).to(dev)
    dinfo = torch.full((32 + 8,), 0x55, dtype=torch.uint8, device=dev)
    dout = torch.full((cap, 3), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.ransac_align3d_run_dev(view, 0, BC.ALIGN_ITERS, thresh, seed, k.data_ptr(), Tw.data_ptr(), m.data_ptr(), cap, c.data_ptr(),
                               model=model)
    ctx.align3d_refine_dev(view, dm.data_ptr(), dT.data_ptr(), dT.data_ptr(), dinfo.data_ptr(), model=model)        # in place
    ctx.transform_points3_dev(dT.data_ptr(), d1.data_ptr(), dn.data_ptr(), cap, dout.data_ptr())
    ctx.synchronize()
    Th, mh, Tr, ih, oh = Tw.cpu().numpy(), m.cpu().numpy(), dT.cpu().numpy(), dinfo.cpu().numpy(), dout.cpu().numpy()
    assert (Th[13:] == 7.0).all() and (Tr[13:] == 7.0).all() and (ih[32:] == 0x55).all() and (oh[n:] == 7.0).all()
    assert not mh[n:cap].any() and (mh[cap:] == 7).all()
    return (int(k.item()) & U64, Th[:13], mh[:n], int(c.item())), (Tr[:13], ih[:32].view(api.H_REFINE_INFO_DTYPE)[0]), oh[:n]


@pytest.mark.parametrize("name,model", ALIGN_RUNS)
def test_alignment_at_hard_geometry(ctx, name, model):
    x1, x2, s, Rg, tg, inl = BC.align_scene(name, model)
    thresh, seed = BC.align_case(name)[2], 0x3D + model
    kr, Tr, mr, cr = AR.run(model, x1, x2, BC.ALIGN_ITERS, thresh, seed)
    start = Tr if kr else BC.align_start(name, model)
    mask_in = mr if kr else inl.astype(np.uint8)
    ref, ri = AR.refine(model, x1, x2, mask_in, start)
    # the host forms
    rc, Tw, mask, c, key = ctx.ransac_align3d(x1, x2, BC.ALIGN_ITERS, thresh, seed, model=model)
    assert rc == (api.PM_OK if kr else api.PM_E_NO_MODEL) and key == kr and c == cr and _same(Tw, Tr) and (mask == mr).all()
    rc, Tn, info = ctx.align3d_refine(x1, x2, mask_in, start, model=model)
    assert rc == api.PM_OK and _same(Tn, ref) and _same(np.array([info.cost_in, info.cost_out]), np.array([ri.cost_in, ri.cost_out]))
    assert (info.n_used, info.iters, info.status) == (ri.n_used, 0, ri.status)
    far = name in ("far-1e4", "scale-1e-3", "scale-1e3", "nonfinite")
    if far:
        moved = ctx.transform_points3(ref, x1)
        assert _same(moved, AR.transform(ref, x1))
    # the device forms
    (kd, Td, md, cd), (Trd, ird), od = _align_dev(ctx, model, x1, x2, thresh, seed, mask_in, start)
    assert kd == kr and cd == cr and _same(Td, Tr) and (md == mr).all()
    assert _same(Trd, ref) and _same(np.array([ird["cost_in"], ird["cost_out"]]), np.array([ri.cost_in, ri.cost_out]))
    assert (int(ird["n_used"]), int(ird["iters"]), int(ird["status"])) == (ri.n_used, 0, ri.status)
    assert _same(od, AR.transform(ref, x1))
    # the independent checks on the device's own output
    BC.check_align_run(name, model, kd, Td, md, cd)
    dinfo = AR.Info([ird["cost_in"], ird["cost_out"]], [ird["n_used"], ird["iters"], ird["status"]])
    m = BC.check_align_refit(name, model, mask_in, start, Trd, dinfo)
    assert m["checked"] == (name in BC.ALIGN_DETERMINED)
    BC.check_align_refit(name, model, mask_in, start, Tn, info)
    if far:
        BC.check_transform(Trd, x1, od, (name, model))
        BC.check_transform(ref, x1, moved, (name, model))
    # a refit from a start that is not the winner, on the planted inliers: host form, independent checks
    start2, mask2 = BC.align_start(name, model), inl.astype(np.uint8)
    rc, T2, info2 = ctx.align3d_refine(x1, x2, mask2, start2, model=model)
    ref2, ri2 = AR.refine(model, x1, x2, mask2, start2)
    assert _same(T2, ref2) and (info2.n_used, info2.status) == (ri2.n_used, ri2.status)
    BC.check_align_refit(name, model, mask2, start2, T2, info2)


# ---- bundle adjustment -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,V,mask", BA_RUNS)
def test_bundle_adjustment_at_hard_geometry(ctx, name, V, mask):
    K, uv, Rt0, xyz0, gate = BC.ba_scene(name, V, mask)
    n = BC.BA_N
    uvp, xp = [_pad(u, np.nan) for u in uv], _pad(xyz0, np.float32(7.0))
    runs = []
    for it in BC.BA_BUDGETS:
        ref = B.run(K, uv, Rt0, xyz0, mask, it, gate)
        prm = api.ba_params(mask, it, gate)
        d = BaDev(uvp, Rt0, xp, n + PAD, count=n, in_place=it == 30)
        out, xyz, used, info = d.run(ctx, K, prm)
        ba_parity((out, xyz, used, info), ref, n, d.xyz_in)
        ho, hx, hu, hi = ctx.bundle_adjust(uv, Rt0, K, xyz0, prm)                           # the host form
        ba_parity((ho, np.r_[hx, xp[n:]], np.r_[hu, np.full(PAD, 0xEE, np.uint8)], hi), ref, n, xp)
        runs.append(BC.Out(Rt=out, xyz=xyz[:n], used=used[:n], xyz64=ref.xyz64, cost_in=float(info["cost_in"]),
                           cost_out=float(info["cost_out"]), n_points=int(info["n_points"]), n_obs=int(info["n_obs"]),
                           status=int(info["status"])))
    BC.ba_checks(name, V, mask, runs)
