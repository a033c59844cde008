"""GPU: the HIP calibrated estimators — RANSAC-E (SPEC S31-S34), pose recovery (S35), RANSAC-PnP (S36-S39) and their
chains with the refinements — against DIFFERENT algorithms at hard geometry (synth.calibrated_view_wide,
synth.pnp_scene_wide; the references, case tables and tolerances of tests/test_pose_independent_cpu.py), plus the kernel
shapes the other suites do not reach: pinned ids per workgroup (every score_lds_ids<MODEL, 1..4> branch, the second pass
of a wave's live ballot, two solver waves, samples straddling workgroups, workgroups without a valid id), ids at the top
of the 32-bit range, LDS tile boundaries, 64-part views, capacities beyond one tile, short and long masks with guard
bytes, non-finite rows; each bit for bit against the C restatements as well.  The sampler indices come from
essential_ref.sample / pnp_ref.sample: they are spec data, not arithmetic.  The twin of
tests/test_homography_independent_gpu.py for E and PnP."""
import numpy as np
import pytest

import essential_ref as ER
import pnp_ref as PR
import twoview_refine_ref as TV
from points_matching_amd import api
from test_pose_independent_cpu import (E_BD, E_CASES, P_CASES, check_mask_vs_float64_reproj,
                                       check_mask_vs_float64_sampson, check_recover_pose, count64_reproj,
                                       count64_sampson, dir_deg, nonfinite_rows, nonfinite_rows3, p3p_case, pose_dists,
                                       recover_case, rot_deg, skew, solve5_case, unit_sign_e, wide_e, wide_p)

pytestmark = pytest.mark.gpu

RL_WAVES = 12            # waves per workgroup of ransac_fused_lds: wave w owns the workgroup's ids w, w + 12, ...
P_TILE = 48 * 128        # correspondences per LDS tile of the PnP scorer (ransac_p_fused.hip); E's is 8192

E_NAMES = [c[0] for c in E_CASES]
P_NAMES = [c[0] for c in P_CASES]


def ecase(name):
    return E_CASES[E_NAMES.index(name)]


def pcase(name):
    return P_CASES[P_NAMES.index(name)]


def _bits_equal(a, b):
    return (np.asarray(a, np.float64).view(np.uint64) == np.asarray(b, np.float64).view(np.uint64)).all()


def _rt(Rm, t):
    return np.r_[np.asarray(Rm, np.float64).reshape(-1), np.asarray(t, np.float64)]


def _run_dev(ctx, model, view, K, hb, he, thr, seed, mask_len, guard=256):
    """pm_ransac_{essential,pnp}_run_dev with every output poisoned; the mask buffer has `guard` sentinel bytes past
    mask_len, returned separately: (key, model doubles, mask, count, guard bytes)."""
    import torch
    dev = torch.device("cuda", 0)
    words = 9 if model == "E" else 12
    k = torch.zeros(1, dtype=torch.int64, device=dev)
    M = torch.full((words,), 7.0, dtype=torch.float64, device=dev)
    m = torch.full((mask_len + guard,), 7, dtype=torch.uint8, device=dev)
    c = torch.full((1,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    run = ctx.ransac_essential_run_dev if model == "E" else ctx.ransac_pnp_run_dev
    run(view, K, hb, he, thr, seed, k.data_ptr(), M.data_ptr(), m.data_ptr(), mask_len, c.data_ptr())
    ctx.synchronize()
    mm = m.cpu().numpy()
    return int(k.item()) & ((1 << 64) - 1), M.cpu().numpy(), mm[:mask_len], int(c.item()), mm[mask_len:]


def _check_e_run(ctx, xy1, xy2, K, iters, thr, seed, hyp_begin=0, what="", want=None):
    """Whole host run: bit parity with the restatement, and the winner's mask against float64."""
    rc, E, mask, c, key = ctx.ransac_essential(xy1, xy2, K, iters, thr, seed, hyp_begin)
    kr, Er, mr, cr = want or ER.run(xy1, xy2, K, iters, thr, seed, hyp_begin)
    assert key == kr, (what, hex(key), hex(kr))
    assert _bits_equal(E, Er) and (mask == mr).all() and c == cr, what
    if kr:
        assert rc == api.PM_OK and c == mask.sum()
        fin = np.isfinite(xy1).all(axis=1) & np.isfinite(xy2).all(axis=1)
        check_mask_vs_float64_sampson(E, K, xy1[fin], xy2[fin], thr, mask[fin], what)
    return key, E, mask, c


def _check_p_run(ctx, xyz, uv, K, iters, thr, seed, hyp_begin=0, what="", want=None):
    rc, Rm, t, mask, c, key = ctx.ransac_pnp(xyz, uv, K, iters, thr, seed, hyp_begin)
    kr, Rtr, mr, cr = want or PR.run(xyz, uv, K, iters, thr, seed, hyp_begin)
    assert key == kr, (what, hex(key), hex(kr))
    assert _bits_equal(_rt(Rm, t), Rtr) and (mask == mr).all() and c == cr, what
    if kr:
        assert rc == api.PM_OK and c == mask.sum()
        fin = np.isfinite(xyz).all(axis=1) & np.isfinite(uv).all(axis=1)
        check_mask_vs_float64_reproj(K, Rm, t, xyz[fin], uv[fin], thr, mask[fin], what)
    return key, Rm, t, mask, c


# ---- single samples ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["narrow-16000", "rot-60", "forward", "depth-1000"])
def test_single_samples_essential(ctx, name):
    """Every candidate of 300 ids: bits against the restatement, then the independent checks of the CPU file on the
    GPU's own output (unit norm, sign, residuals, cubic constraints, root count against numpy), and every count against
    the restatement's and, outside the band, float64's."""
    case = ecase(name)
    thr = case[2]
    state = {}

    def gpu_candidates(xy1, xy2, K, seed, h):
        if "x1n" not in state:
            ok, tn = ER.thr_n(K, thr)
            state.update(x1n=ER.normalise(K, xy1), x2n=ER.normalise(K, xy2), thr2=np.float32(tn) * np.float32(tn))
        rc, E, counts, nm = ctx.ransac_essential_from_hyp(xy1, xy2, K, h, thr, seed)
        Er, vr = ER.candidates(xy1, xy2, K, seed, h)
        assert rc == (api.PM_OK if vr.any() else api.PM_E_NO_MODEL) and nm == vr.sum(), (name, h)
        assert _bits_equal(E.reshape(10, 9), Er), (name, h)
        for j in range(10):
            if not vr[j]:
                assert counts[j] == -1, (name, h, j)
                continue
            assert counts[j] == ER.score(Er[j], state["x1n"], state["x2n"], state["thr2"])[1], (name, h, j)
            c64, nb = count64_sampson(E[j], K, xy1, xy2, thr)
            assert abs(counts[j] - c64) <= nb, (name, h, j, counts[j], c64, nb)
        return E.reshape(10, 9), vr

    nvalid, nclear, samples, _, _ = solve5_case(case, E_NAMES.index(name), candidates=gpu_candidates)
    assert nvalid >= samples and samples == 300


@pytest.mark.parametrize("name", ["rot-any", "offset-1e4", "depth-1000", "collinear-20"])
def test_single_samples_pnp(ctx, name):
    case = pcase(name)
    thr = case[2]

    def gpu_candidates(xyz, uv, K, seed, h):
        rc, Rt, counts, nm = ctx.ransac_pnp_from_hyp(xyz, uv, K, h, thr, seed)
        Rr, vr = PR.candidates(xyz, uv, K, seed, h)
        assert rc == (api.PM_OK if vr.any() else api.PM_E_NO_MODEL) and nm == vr.sum(), (name, h)
        assert _bits_equal(Rt, Rr), (name, h)
        for j in range(4):
            if not vr[j]:
                assert counts[j] == -1, (name, h, j)
                continue
            assert counts[j] == PR.score(K, Rr[j], xyz, uv, thr)[1], (name, h, j)
            c64, nb = count64_reproj(K, Rt[j], xyz, uv, thr)
            assert abs(counts[j] - c64) <= nb, (name, h, j, counts[j], c64, nb)
        return Rt, vr

    nvalid, nclear, samples, _, _ = p3p_case(case, P_NAMES.index(name), candidates=gpu_candidates)
    assert nvalid >= 0.5 * samples and samples == 300


# ---- pinned ids per workgroup ----------------------------------------------------------------------------------------
def wave_occupancy(valid, hb):
    """valid: the flags of a launch's model ids, in order.  Row b: the live ids of each of the 12 waves of workgroup b
    (ids [b hb, (b + 1) hb); wave w owns local ids w + 12 k)."""
    return np.array([[int(valid[h0:h0 + hb][w::RL_WAVES].sum()) for w in range(RL_WAVES)]
                     for h0 in range(0, len(valid), hb)])


def branches_reached(occ):
    """(the NH of every score_lds_ids call: 4 per full pass of a wave's live ballot, then the remainder; the most live
    ids in one wave; the number of workgroups without a live id)."""
    nh = set()
    for live in occ.reshape(-1):
        if live >= 4:
            nh.add(4)
        if live % 4:
            nh.add(int(live % 4))
    return nh, int(occ.max()), int((occ.sum(axis=1) == 0).sum())


def _e_valid_flags(xy1, xy2, K, seed, samples):
    """The restatement's valid flags of ids [0, 10 samples) (the points normalised once)."""
    x1n, x2n = ER.normalise(K, xy1), ER.normalise(K, xy2)
    E, v = np.zeros(90), np.zeros(10, np.int32)
    flags = np.zeros((samples, 10), bool)
    for h in range(samples):
        ER.lib().er_candidates(ER._p(x1n), ER._p(x2n), len(x1n), seed, h, ER._p(E), ER._p(v))
        flags[h] = v != 0
    return flags.reshape(-1)


def test_pinned_ids_per_workgroup_essential(ctx):
    """PM_OPT_RANSAC_WG_IDS over RANSAC-E: ids per workgroup below, at and above a sample's 10 slots (samples straddle
    workgroups), one and two solver waves, partial last workgroups.  At 128 ids per workgroup the restatement's valid
    flags reach every NH = 1..4, a wave with 5 or more live ids (a second pass) and a workgroup with no valid id."""
    case = ecase("rot-any")
    xy1, xy2, K, _, _, _, _ = wide_e(3000, 11, case)
    thr, seed = case[2], 0x9D
    valid = _e_valid_flags(xy1, xy2, K, seed, 1037)
    for hb in (127, 128):
        nh, most, empty = branches_reached(wave_occupancy(valid, hb))
        assert nh == {1, 2, 3, 4} and most >= 5, (hb, nh, most)
    assert branches_reached(wave_occupancy(valid, 128))[2] >= 1
    assert branches_reached(wave_occupancy(valid[:3330], 128))[2] >= 1
    want = {nh: ER.run(xy1, xy2, K, nh, thr, seed) for nh in (1037, 333)}
    try:
        for ids in (1, 9, 10, 11, 12, 13, 64, 65, 127, 128):
            ctx.set_option(api.PM_OPT_RANSAC_WG_IDS, ids)
            for nh in (1037, 333):
                rc, E, mask, c, key = ctx.ransac_essential(xy1, xy2, K, nh, thr, seed)
                kr, Er, mr, cr = want[nh]
                assert key == kr and _bits_equal(E, Er) and (mask == mr).all() and c == cr, (ids, nh)
    finally:
        ctx.set_option(api.PM_OPT_RANSAC_WG_IDS, 0)
    check_mask_vs_float64_sampson(want[1037][1], K, xy1, xy2, thr, want[1037][2])


def test_pinned_ids_per_workgroup_pnp(ctx):
    """The same over RANSAC-PnP (4 slots per sample).  Half of the map points carry a NaN, so that most samples have
    no candidate: at 127 and 128 ids per workgroup (32 samples) the restatement's valid flags then hold workgroups
    without a valid id next to waves with 5 or more live ones, and every NH = 1..4."""
    case = pcase("rot-any")
    xyz, uv, K, _, _, _ = wide_p(3000, 11, case)
    xyz[np.random.default_rng(5).permutation(3000)[:1500], 1] = np.nan
    thr, seed = case[2], 0xC4
    valid = np.concatenate([PR.candidates(xyz, uv, K, seed, h)[1] for h in range(1037)])
    for hb in (127, 128):
        for nh in (1037, 333):
            got, most, empty = branches_reached(wave_occupancy(valid[:4 * nh], hb))
            assert got == {1, 2, 3, 4} and most >= 5 and empty >= 1, (hb, nh, got, most, empty)
    want = {nh: PR.run(xyz, uv, K, nh, thr, seed) for nh in (1037, 333)}
    assert want[1037][0] and want[333][0]
    try:
        for ids in (1, 3, 4, 5, 12, 13, 64, 65, 127, 128):
            ctx.set_option(api.PM_OPT_RANSAC_WG_IDS, ids)
            for nh in (1037, 333):
                rc, Rm, t, mask, c, key = ctx.ransac_pnp(xyz, uv, K, nh, thr, seed)
                kr, Rtr, mr, cr = want[nh]
                assert key == kr and _bits_equal(_rt(Rm, t), Rtr) and (mask == mr).all() and c == cr, (ids, nh)
    finally:
        ctx.set_option(api.PM_OPT_RANSAC_WG_IDS, 0)
    fin = np.isfinite(xyz).all(axis=1)
    Rtw, mw = want[1037][1], want[1037][2]
    assert not mw[~fin].any()
    check_mask_vs_float64_reproj(K, Rtw[:9].reshape(3, 3), Rtw[9:], xyz[fin], uv[fin], thr, mw[fin])


# ---- ids at the top of the range -------------------------------------------------------------------------------------
def test_essential_ids_at_the_top_and_sharding_there(ctx):
    import torch
    dev = torch.device("cuda", 0)
    case = ecase("pp-offset")
    n = 2275
    xy1, xy2, K, _, _, _, _ = wide_e(n, 32, case)
    thr, top = case[2], (1 << 32) // 10
    key, E, mask, c = _check_e_run(ctx, xy1, xy2, K, top, thr, 0x32, hyp_begin=top - 500, what="top")
    assert key and api.ransac_key_hyp(key) >= 10 * (top - 500)
    f1, f2 = torch.from_numpy(xy1).to(dev), torch.from_numpy(xy2).to(dev)
    view = api.PointsView(f1.data_ptr(), f2.data_ptr(), None, 1, n, 0, 1, 0)
    for a in (top - 499, top - 250, top - 1):
        ka, Ea, _, _, _ = _run_dev(ctx, "E", view, K, top - 500, a, thr, 0x32, n)
        kb, Eb, _, _, _ = _run_dev(ctx, "E", view, K, a, top, thr, 0x32, n)
        assert max(ka, kb) == key, a
        assert _bits_equal(Ea if ka > kb else Eb, E.reshape(-1)), a


def test_pnp_ids_at_the_top_and_sharding_there(ctx):
    """Samples up to 2^30: the ids reach 2^32 - 1, whose key has a low word of 0."""
    import torch
    dev = torch.device("cuda", 0)
    case = pcase("depth-1000")
    n = 2275
    xyz, uv, K, _, _, _ = wide_p(n, 32, case)
    thr, top = case[2], 1 << 30
    key, Rm, t, mask, c = _check_p_run(ctx, xyz, uv, K, top, thr, 0x32, hyp_begin=top - 1000, what="top")
    assert key and api.ransac_key_hyp(key) >= 4 * (top - 1000)
    # the last sample alone: the winner is one of the last four ids
    k1, R1, t1, m1, c1 = _check_p_run(ctx, xyz, uv, K, top, thr, 0x32, hyp_begin=top - 1, what="last sample")
    vr = PR.candidates(xyz, uv, K, 0x32, top - 1)[1]
    assert bool(k1) == bool(vr.any())
    if k1:
        assert api.ransac_key_hyp(k1) >= 4 * (top - 1)
    dx, du = torch.from_numpy(xyz).to(dev), torch.from_numpy(uv).to(dev)
    view = api.PnpView(dx.data_ptr(), du.data_ptr(), None, n, 0)
    for a in (top - 999, top - 500, top - 1):
        ka, Ra, _, _, _ = _run_dev(ctx, "P", view, K, top - 1000, a, thr, 0x32, n)
        kb, Rb, mb, cb, _ = _run_dev(ctx, "P", view, K, a, top, thr, 0x32, n)
        assert max(ka, kb) == key, a
        assert _bits_equal(Ra if ka > kb else Rb, _rt(Rm, t)), a
        if a == top - 1:
            assert kb == k1 and _bits_equal(Rb, _rt(R1, t1)) and (mb == m1).all() and cb == c1


# ---- sizes around the slot and tile boundaries -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 127, 128, 129, 8191, 8192, 8193, 16385])
def test_essential_sizes_around_slot_and_tile_boundaries(ctx, n):
    case = ecase("rot-60")
    xy1, xy2, K, _, _, _, _ = wide_e(n, n, case, **({"outlier_frac": 0.0} if n == 5 else {}))
    _check_e_run(ctx, xy1, xy2, K, 300 if n > 8192 else 700, case[2], 0xE0, what=n)


@pytest.mark.parametrize("n", [4, 127, 128, 129, P_TILE - 1, P_TILE, P_TILE + 1, 2 * P_TILE + 1])
def test_pnp_sizes_around_slot_and_tile_boundaries(ctx, n):
    case = pcase("near-planar")
    xyz, uv, K, _, _, _ = wide_p(n, n, case, **({"outlier_frac": 0.0} if n == 4 else {}))
    _check_p_run(ctx, xyz, uv, K, 300 if n > P_TILE else 700, case[2], 0xE0, what=n)


# ---- views -------------------------------------------------------------------------------------------------------------
def _parts_view(torch, dev, xy1, xy2, counts, cap, pad=6):
    """`len(counts)` parts of `cap` slots, pitch 2 cap + pad floats, NaN padding; counts on the device."""
    pitch = 2 * cap + pad
    b1 = np.full((len(counts), pitch), np.nan, np.float32)
    b2 = np.full((len(counts), pitch), np.nan, np.float32)
    o = 0
    for p, k in enumerate(counts):
        b1[p, :2 * k] = xy1[o:o + k].reshape(-1)
        b2[p, :2 * k] = xy2[o:o + k].reshape(-1)
        o += k
    d1, d2 = torch.from_numpy(b1.reshape(-1)).to(dev), torch.from_numpy(b2.reshape(-1)).to(dev)
    dc = torch.tensor(counts, dtype=torch.int32, device=dev)
    return d1, d2, dc, pitch


def test_essential_64_part_view_uneven_counts_and_pose_recovery_with_points(ctx):
    import torch
    dev = torch.device("cuda", 0)
    cap, parts = 130, 64
    counts = [0 if p % 7 == 3 else (53 * p + 11) % 131 for p in range(parts)]
    n = sum(counts)
    case = ecase("forward")
    xy1, xy2, K, _, _, _, _ = wide_e(n, 640, case)
    thr = case[2]
    d1, d2, dc, pitch = _parts_view(torch, dev, xy1, xy2, counts, cap)
    view = api.PointsView(d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), parts, cap, pitch, 1, 0)
    key, E, mask, c, guard = _run_dev(ctx, "E", view, K, 0, 1500, thr, 0x40, parts * cap)
    kr, Er, mr, cr = ER.run(xy1, xy2, K, 1500, thr, 0x40)
    assert kr and key == kr and _bits_equal(E, Er.reshape(-1)) and c == cr
    assert (mask[:n] == mr).all() and not mask[n:].any() and (guard == 7).all()
    check_mask_vs_float64_sampson(Er, K, xy1, xy2, thr, mask[:n])
    # the pose recovery over the same view, points4 requested, every output poisoned, guard bytes behind the mask
    Ed = torch.from_numpy(Er.reshape(-1).copy()).to(dev)
    mi = torch.from_numpy(np.r_[mr, np.ones(parts * cap - n, np.uint8)]).to(dev)     # rows past the count are never read
    Rd = torch.full((9,), 7.0, dtype=torch.float64, device=dev)
    td = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    mo = torch.full((parts * cap + 256,), 7, dtype=torch.uint8, device=dev)
    ng = torch.full((1,), 99, dtype=torch.int32, device=dev)
    pts = torch.full((parts * cap + 64, 4), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.recover_pose_dev(view, K, Ed.data_ptr(), mi.data_ptr(), Rd.data_ptr(), td.data_ptr(), mo.data_ptr(), ng.data_ptr(),
                         pts.data_ptr())
    ctx.synchronize()
    ngr, Rr, tr, mor, ptr_, _ = ER.recover_pose(xy1, xy2, K, Er, mr)
    mo, pts = mo.cpu().numpy(), pts.cpu().numpy()
    assert int(ng.item()) == ngr and _bits_equal(Rd.cpu().numpy(), Rr.reshape(-1)) and _bits_equal(td.cpu().numpy(), tr)
    assert (mo[:n] == mor).all() and not mo[n:parts * cap].any() and (mo[parts * cap:] == 7).all()
    assert (pts[:n].view(np.uint32) == ptr_.view(np.uint32)).all() and (pts[parts * cap:] == 7.0).all()
    check_recover_pose(K, Er, xy1, xy2, mr, 50.0, (int(ng.item()), Rd.cpu().numpy().reshape(3, 3), td.cpu().numpy(),
                                                   mo[:n], pts[:n]), what="64 parts")


@pytest.mark.parametrize("count", [8000, 9000])
def test_essential_capacity_beyond_one_lds_tile(ctx, count):
    """cap 10000 > 8192 points per LDS tile with a device count below it: one tile (8000) or two (9000)."""
    import torch
    dev = torch.device("cuda", 0)
    cap = 10000
    case = ecase("depth-1000")
    xy1, xy2, K, _, _, _, _ = wide_e(cap, 10000, case)
    thr = case[2]
    f1, f2 = torch.from_numpy(xy1).to(dev), torch.from_numpy(xy2).to(dev)
    dn = torch.tensor([count], dtype=torch.int32, device=dev)
    view = api.PointsView(f1.data_ptr(), f2.data_ptr(), dn.data_ptr(), 1, cap, 0, 1, 0)
    key, E, mask, c, guard = _run_dev(ctx, "E", view, K, 0, 300, thr, 0x7E, cap)
    kr, Er, mr, cr = ER.run(xy1[:count], xy2[:count], K, 300, thr, 0x7E)
    assert kr and key == kr and _bits_equal(E, Er.reshape(-1)) and c == cr
    assert (mask[:count] == mr).all() and not mask[count:].any() and (guard == 7).all()
    check_mask_vs_float64_sampson(Er, K, xy1[:count], xy2[:count], thr, mask[:count])


@pytest.mark.parametrize("count", [6000, 6500])
def test_pnp_capacity_beyond_one_lds_tile(ctx, count):
    """cap 7000 > 6144 correspondences per LDS tile with a device count below it: one tile (6000) or two (6500)."""
    import torch
    dev = torch.device("cuda", 0)
    cap = 7000
    case = pcase("wide-field")
    xyz, uv, K, _, _, _ = wide_p(cap, 7000, case)
    thr = case[2]
    dx, du = torch.from_numpy(xyz).to(dev), torch.from_numpy(uv).to(dev)
    dn = torch.tensor([count], dtype=torch.int32, device=dev)
    view = api.PnpView(dx.data_ptr(), du.data_ptr(), dn.data_ptr(), cap, 0)
    key, Rt, mask, c, guard = _run_dev(ctx, "P", view, K, 0, 300, thr, 0x7E, cap)
    kr, Rtr, mr, cr = PR.run(xyz[:count], uv[:count], K, 300, thr, 0x7E)
    assert kr and key == kr and _bits_equal(Rt, Rtr) and c == cr
    assert (mask[:count] == mr).all() and not mask[count:].any() and (guard == 7).all()
    check_mask_vs_float64_reproj(K, Rtr[:9].reshape(3, 3), Rtr[9:], xyz[:count], uv[:count], thr, mask[:count])


# ---- mask lengths --------------------------------------------------------------------------------------------------------
MASK_LENS = (0, 1, 100, 2999, 3002, 3001 + 127, 3001 + 300)


def test_essential_mask_shorter_and_longer_than_n(ctx):
    import torch
    dev = torch.device("cuda", 0)
    n = 3001
    case = ecase("wide-field")
    xy1, xy2, K, _, _, _, _ = wide_e(n, 3001, case)
    thr = case[2]
    kr, Er, mr, cr = ER.run(xy1, xy2, K, 500, thr, 0x31)
    assert kr
    f1, f2 = torch.from_numpy(xy1).to(dev), torch.from_numpy(xy2).to(dev)
    view = api.PointsView(f1.data_ptr(), f2.data_ptr(), None, 1, n, 0, 1, 0)
    for mask_len in MASK_LENS:
        key, E, mask, c, guard = _run_dev(ctx, "E", view, K, 0, 500, thr, 0x31, mask_len)
        k = min(mask_len, n)
        assert key == kr and _bits_equal(E, Er.reshape(-1)) and c == cr, mask_len      # the count covers all n
        assert (mask[:k] == mr[:k]).all() and not mask[k:].any() and (guard == 7).all(), mask_len


def test_pnp_mask_shorter_and_longer_than_n(ctx):
    import torch
    dev = torch.device("cuda", 0)
    n = 3001
    case = pcase("offset-1e3")
    xyz, uv, K, _, _, _ = wide_p(n, 3001, case)
    thr = case[2]
    kr, Rtr, mr, cr = PR.run(xyz, uv, K, 500, thr, 0x31)
    assert kr
    dx, du = torch.from_numpy(xyz).to(dev), torch.from_numpy(uv).to(dev)
    view = api.PnpView(dx.data_ptr(), du.data_ptr(), None, n, 0)
    for mask_len in MASK_LENS:
        key, Rt, mask, c, guard = _run_dev(ctx, "P", view, K, 0, 500, thr, 0x31, mask_len)
        k = min(mask_len, n)
        assert key == kr and _bits_equal(Rt, Rtr) and c == cr, mask_len                # the count covers all n
        assert (mask[:k] == mr[:k]).all() and not mask[k:].any() and (guard == 7).all(), mask_len


# ---- non-finite input ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pp-offset", "rot-any"])
def test_essential_nonfinite_rows(ctx, name):
    """5 % of the rows carry a NaN, an infinity or +-1e30: bit parity, never inliers (S31 turns them into NaN), never
    good in the pose recovery, and the planted pose still found within the mild suite's bounds."""
    case = ecase(name)
    xy1, xy2, K, Rg, tg, _, inl = wide_e(3000, 900, case)
    a, b, bad = nonfinite_rows(xy1, xy2, 0.05, 3)
    thr = case[2]
    rc, E, mask, c, key = ctx.ransac_essential(a, b, K, 1000, thr, 0xF0)
    kr, Er, mr, cr = ER.run(a, b, K, 1000, thr, 0xF0)
    assert rc == api.PM_OK and key == kr and _bits_equal(E, Er) and (mask == mr).all() and c == cr
    assert not mask[bad].any()
    ok = ~bad
    check_mask_vs_float64_sampson(E, K, a[ok], b[ok], thr, mask[ok], name)
    for m_in in (mask, None):
        rc, Rr, tr, mo, ng, pts = ctx.recover_pose(a, b, K, E, mask=m_in, points=True)
        ngr, Rr2, tr2, mor, ptr_, _ = ER.recover_pose(a, b, K, E, m_in)
        assert rc == api.PM_OK and ng == ngr and _bits_equal(Rr, Rr2) and _bits_equal(tr, tr2) and (mo == mor).all()
        assert (pts.view(np.uint32) == ptr_.view(np.uint32)).all()
        assert not mo[bad].any()
    assert rot_deg(Rr, Rg) < 0.25 and dir_deg(tr, tg) < 2.0, (rot_deg(Rr, Rg), dir_deg(tr, tg))


@pytest.mark.parametrize("name", ["rot-any", "depth-1000"])
def test_pnp_nonfinite_rows(ctx, name):
    case = pcase(name)
    xyz, uv, K, Rg, tg, inl = wide_p(3000, 900, case)
    a, b, bad = nonfinite_rows3(xyz, uv, 0.05, 3)
    thr = case[2]
    rc, Rm, t, mask, c, key = ctx.ransac_pnp(a, b, K, 1000, thr, 0xF0)
    kr, Rtr, mr, cr = PR.run(a, b, K, 1000, thr, 0xF0)
    assert rc == api.PM_OK and key == kr and _bits_equal(_rt(Rm, t), Rtr) and (mask == mr).all() and c == cr
    assert not mask[bad].any()
    ok = ~bad
    check_mask_vs_float64_reproj(K, Rm, t, a[ok], b[ok], thr, mask[ok], name)
    assert rot_deg(Rm, Rg) < 0.1, rot_deg(Rm, Rg)
    assert np.linalg.norm(t - tg) < 0.01 * max(1.0, np.linalg.norm(tg)), (t, tg)
    rc, R2, t2, info = ctx.pnp_refine(a, b, K, mask, Rm, t, 20)
    ref, ri = PR.refine(a, b, K, mask, Rtr, 20)
    assert rc == api.PM_OK and _bits_equal(_rt(R2, t2), ref) and info.status == ri.status == 0
    assert np.isfinite(_rt(R2, t2)).all() and np.isfinite([info.cost_in, info.cost_out]).all()


# ---- pose recovery -------------------------------------------------------------------------------------------------------
def _gpu_recover(ctx):
    def recover(xy1, xy2, K, E, mask, dist):
        rc, Rr, tr, mo, ng, pts = ctx.recover_pose(xy1, xy2, K, E, mask=mask, dist=dist, points=True)
        ngr, Rr2, tr2, mor, ptr_, _ = ER.recover_pose(xy1, xy2, K, E, mask, dist)
        assert ng == max(ngr, 0) and _bits_equal(Rr, Rr2) and _bits_equal(tr, tr2) and (mo == mor).all(), dist
        assert (pts.view(np.uint32) == ptr_.view(np.uint32)).all(), dist
        return ng, Rr, tr, mo, pts
    return recover


@pytest.mark.parametrize("n", [5, 511, 512, 513, 1025])
def test_recover_pose_sizes_around_the_workgroup(ctx, n):
    """One workgroup of 512 threads runs the recovery: sizes around it, with no mask, a RANSAC mask and a mask of exactly
    one set byte; parity with the restatement, then numpy's SVD decomposition, triangulation and cheirality."""
    case = ecase("rot-any")
    xy1, xy2, K, Rg, tg, _, inl = wide_e(n, 70 + n, case, **({"outlier_frac": 0.0} if n == 5 else {}))
    kr, Er, mr, _ = ER.run(xy1, xy2, K, 200, case[2], 3)
    assert kr
    one = np.zeros(n, np.uint8)
    one[np.nonzero(mr)[0][-1]] = 1
    recover = _gpu_recover(ctx)
    for mask in (None, mr, one):
        got = recover(xy1, xy2, K, Er, mask, 50.0)
        check_recover_pose(K, Er, xy1, xy2, mask, 50.0, got, what=(n, None if mask is None else int(mask.sum())))
        if mask is one:
            assert got[0] <= 1


@pytest.mark.parametrize("dist", [1e-3, 50.0, 1e9])
def test_recover_pose_dist_on_the_depth_ratio_case(ctx, dist):
    case = ecase("depth-1000")
    xy1, xy2, K, Rg, tg, X, inl = wide_e(1500, 71, case)
    E = unit_sign_e(skew(tg) @ Rg)
    recover = _gpu_recover(ctx)
    m = inl.astype(np.uint8)
    got = recover(xy1, xy2, K, E, m, dist)
    check_recover_pose(K, E, xy1, xy2, m, dist, got, what=dist)
    near = inl & (X[:, 2] < 0.5 * dist) & ((X @ Rg.T + tg)[:, 2] < 0.5 * dist)
    far = inl & (X[:, 2] > 2.0 * dist)
    if dist == 1e-3:
        assert got[0] == 0
    else:
        assert got[3][near].mean() > 0.95 and (not far.any() or got[3][far].mean() < 0.05)
        assert np.abs(got[1] - Rg).max() < 1e-9 and np.abs(got[2] - tg).max() < 1e-9


@pytest.mark.parametrize("name", ["bd-1e-2", "bd-1e-3"])
def test_recover_pose_near_pure_rotation(ctx, name):
    """The four cheirality counts nearly tie: parity with the restatement always (inside recover_case's recover), numpy's
    choice where its best count leads by more than the banded points."""
    case = ecase(name)
    ndec, runs, _, _, _ = recover_case(case, E_NAMES.index(name), recover=_gpu_recover(ctx))
    assert runs == 6 and ndec >= 1


def test_recover_pose_nan_essential_on_the_device_form(ctx):
    """A NaN E through pm_recover_pose_dev with points4 requested: R, t, count, mask and points4[:n] all zero, the guard
    past the mask intact."""
    import torch
    dev = torch.device("cuda", 0)
    n = 700
    xy1, xy2, K, _, _, _, _ = wide_e(n, 72, ecase("rot-any"))
    f1, f2 = torch.from_numpy(xy1).to(dev), torch.from_numpy(xy2).to(dev)
    view = api.PointsView(f1.data_ptr(), f2.data_ptr(), None, 1, n, 0, 1, 0)
    E = np.full(9, 0.1)
    E[4] = np.nan
    Ed = torch.from_numpy(E).to(dev)
    Rd = torch.full((9,), 7.0, dtype=torch.float64, device=dev)
    td = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    mo = torch.full((n + 256,), 7, dtype=torch.uint8, device=dev)
    ng = torch.full((1,), 99, dtype=torch.int32, device=dev)
    pts = torch.full((n + 64, 4), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.recover_pose_dev(view, K, Ed.data_ptr(), None, Rd.data_ptr(), td.data_ptr(), mo.data_ptr(), ng.data_ptr(),
                         pts.data_ptr())
    ctx.synchronize()
    mo, pts = mo.cpu().numpy(), pts.cpu().numpy()
    assert not Rd.cpu().numpy().any() and not td.cpu().numpy().any() and int(ng.item()) == 0
    assert not mo[:n].any() and (mo[n:] == 7).all()
    assert not pts[:n].any() and (pts[n:] == 7.0).all()
    assert ER.recover_pose(xy1, xy2, K, E)[0] == -1


# ---- whole chains at hard geometry ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["narrow-16000", "rot-60"])
def test_estimate_pose_refined_at_hard_geometry(ctx, name):
    case = ecase(name)
    xy1, xy2, K, Rg, tg, _, inl = wide_e(2275, 80, case)
    thr = case[2]
    rc0, E0, R0, t0, m0, c0, ng0, k0 = ctx.estimate_pose(xy1, xy2, K, 1000, thr, 0x5EED)
    rc, E, Rm, t, mask, c, ng, key, info = ctx.estimate_pose_refined(xy1, xy2, K, 1000, thr, 0x5EED, 20)
    kr, Er, mr, cr = ER.run(xy1, xy2, K, 1000, thr, 0x5EED)
    ngr, Rr, tr, mor, _, _ = ER.recover_pose(xy1, xy2, K, Er, mr)
    assert rc0 == rc == api.PM_OK and key == k0 == kr and c == c0 == cr and ng == ng0 == ngr
    assert _bits_equal(E0, Er) and _bits_equal(R0, Rr) and _bits_equal(t0, tr) and (mask == mor).all() and (m0 == mor).all()
    R2, t2, E2, i2 = TV.pose_refine(xy1, xy2, K, mor, Rr, tr, 20)
    assert _bits_equal(Rm, R2) and _bits_equal(t, t2) and _bits_equal(E, E2)
    assert (info.n_used, info.iters, info.status) == (i2.n_used, i2.iters, i2.status) and info.status == 0
    check_mask_vs_float64_sampson(E0, K, xy1, xy2, thr, ER.run(xy1, xy2, K, 1000, thr, 0x5EED)[2], name)
    e0 = rot_deg(R0, Rg) + dir_deg(t0, tg)
    e1 = rot_deg(Rm, Rg) + dir_deg(t, tg)
    assert e1 <= e0, (e0, e1)
    assert ng >= 0.9 * c and c >= 0.85 * inl.sum()


@pytest.mark.parametrize("name", ["offset-1e3", "behind"])
def test_solve_pnp_ransac_at_hard_geometry(ctx, name):
    case = pcase(name)
    xyz, uv, K, Rg, tg, inl = wide_p(2275, 80, case)
    thr = case[2]
    rc0, R0, t0, m0, c0, k0 = ctx.ransac_pnp(xyz, uv, K, 1000, thr, 0x5EED)
    rc, Rm, t, mask, c, key, info = ctx.solve_pnp_ransac(xyz, uv, K, 1000, thr, 0x5EED, max_iters=20)
    kr, Rtr, mr, cr = PR.run(xyz, uv, K, 1000, thr, 0x5EED)
    ref, ri = PR.refine(xyz, uv, K, mr, Rtr, 20)
    assert rc0 == rc == api.PM_OK and key == k0 == kr and c == c0 == cr and (mask == mr).all() and (m0 == mr).all()
    assert _bits_equal(_rt(R0, t0), Rtr) and _bits_equal(_rt(Rm, t), ref)
    assert _bits_equal([info.cost_in, info.cost_out], [ri.cost_in, ri.cost_out])
    assert (info.n_used, info.iters, info.status) == (ri.n_used, ri.iters, ri.status) and info.status == 0
    check_mask_vs_float64_reproj(K, R0, t0, xyz, uv, thr, mask, name)
    e0 = rot_deg(R0, Rg) + np.degrees(np.linalg.norm(t0 - tg) / np.linalg.norm(tg))
    e1 = rot_deg(Rm, Rg) + np.degrees(np.linalg.norm(t - tg) / np.linalg.norm(tg))
    assert e1 <= e0, (e0, e1)
    assert c >= 0.99 * inl.sum() and not mask[~inl & (xyz.astype(np.float64) @ Rg[2] + tg[2] < 0)].any()
