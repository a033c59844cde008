"""GPU: the HIP robust homography (RANSAC-H, SPEC S19-S22) and its refinement (S23-S25) against DIFFERENT algorithms —
numpy SVD DLT, a numpy statement of the S20 sample rule, float64 transfer distances, scipy's MINPACK LM — at mild and
hard geometry (synth.planar_view_wide), plus the kernel shapes the other suites do not reach (LDS tile boundaries, pinned
ids per workgroup, ids near 2^32, 64-part views, short and long masks, non-finite rows), each bit for bit against the
C restatements as well.  The sampler indices come from homography_ref.sample4: they are spec data, not arithmetic.
The twin of tests/test_independent_gpu.py for F."""
import numpy as np
import pytest

import homography_ref as R
import homography_refine_ref as RR
from points_matching_amd import api, synth
from test_homography_independent_cpu import (REFIT_TOL, SOLVE4_TOL, WIDE_CASES, check_lm_optimal,
                                             check_mask_vs_float64, mean_transfer_between, nonfinite_rows, np_dlt,
                                             np_sample_rule, thresh_for, transfer64, wide_view)

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    return (np.asarray(a, np.float64).view(np.uint64) == np.asarray(b, np.float64).view(np.uint64)).all()


def _run_dev(ctx, view, hb, he, thr, seed, mask_len, guard=256):
    """run_dev with outputs poisoned; the mask buffer has `guard` sentinel bytes past mask_len, returned separately."""
    import torch
    dev = torch.device("cuda", 0)
    k = torch.zeros(1, dtype=torch.int64, device=dev)
    H = torch.full((9,), 7.0, dtype=torch.float64, device=dev)
    m = torch.full((mask_len + guard,), 7, dtype=torch.uint8, device=dev)
    c = torch.full((1,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.ransac_homography_run_dev(view, hb, he, thr, seed, k.data_ptr(), H.data_ptr(), m.data_ptr(), mask_len, c.data_ptr())
    ctx.synchronize()
    mm = m.cpu().numpy()
    return int(k.item()) & ((1 << 64) - 1), H.cpu().numpy().reshape(3, 3), mm[:mask_len], int(c.item()), mm[mask_len:]


def _check_run(ctx, xy1, xy2, iters, thr, seed, hyp_begin=0, what=""):
    """Whole host run: bit parity with the restatement, and the winner's mask against float64."""
    rc, H, mask, c, key = ctx.ransac_homography(xy1, xy2, iters, thr, seed, hyp_begin)
    kr, Hr, mr, cr = R.run(xy1, xy2, iters, thr, seed, hyp_begin)
    assert key == kr, (what, hex(key), hex(kr))
    assert _bits_equal(H, Hr) and (mask == mr).all() and c == cr, what
    if kr:
        assert rc == api.PM_OK and c == mask.sum()
        check_mask_vs_float64(H, xy1, xy2, thr, mask, what)
    return key, H, mask, c


def _hard_cases():
    return [WIDE_CASES[0], WIDE_CASES[2], WIDE_CASES[3], WIDE_CASES[5]]


# ---- single hypotheses ---------------------------------------------------------------------------------------------
def test_single_hypotheses_against_numpy(ctx):
    """H vs numpy SVD DLT of the 4 sampled points, unit norm and sign, validity vs the numpy sample rule, mask vs float64
    transfer distance: >= 1000 valid ids over mild and hard geometry."""
    valid = clear = 0
    for ci, case in enumerate(_hard_cases()):
        n = 500
        xy1, xy2, _, _ = wide_view(n, 200 + ci, case)
        thr, seed = thresh_for(case), 0xA11 + ci
        for h in range(700):
            rc, H, mask, c = ctx.ransac_homography_from_hyp(xy1, xy2, h, thr, seed)
            idx = R.sample4(seed, h, n)
            p1, p2 = xy1[idx].astype(np.float64), xy2[idx].astype(np.float64)
            ok_np, is_clear = np_sample_rule(p1, p2)
            ok = rc == api.PM_OK
            if is_clear:
                assert ok == ok_np, (ci, h, rc)
                clear += 1
            if not ok:
                assert rc == api.PM_E_NO_MODEL and not H.any() and not mask.any() and c == 0, (ci, h)
                continue
            assert abs(np.linalg.norm(H) - 1.0) < 1e-14 and H[2, 2] >= 0, (ci, h)
            Hn, S, _ = np_dlt(p1, p2)
            gap = S[7] / S[0]
            assert np.linalg.norm(H - Hn) <= SOLVE4_TOL / gap + 1e-14, (ci, h, np.linalg.norm(H - Hn), gap)
            assert c == mask.sum()
            check_mask_vs_float64(H, xy1, xy2, thr, mask, (ci, h))
            valid += 1
    assert valid >= 1000 and clear >= 2500, (valid, clear)


def test_winner_is_the_best_model_by_float64_count(ctx):
    """The run's winner has at least as many float64-counted inliers as every other id of the run, up to the points
    within the rounding band of either model."""
    case = WIDE_CASES[3]
    xy1, xy2, _, _ = wide_view(1500, 77, case)
    thr, seed = thresh_for(case), 0x3E
    rc, H, mask, c, key = ctx.ransac_homography(xy1, xy2, 300, thr, seed)
    assert rc == api.PM_OK

    def count64(M):
        d, _, err = transfer64(M.astype(np.float32).astype(np.float64), xy1, xy2)
        border = np.abs(d - thr) <= 1e-3 * thr + err
        return int((d <= thr).sum()), int(border.sum())
    cw, bw = count64(H)
    assert abs(cw - c) <= bw
    for h in range(300):
        rc_h, H_h, _, _ = ctx.ransac_homography_from_hyp(xy1, xy2, h, thr, seed)
        if rc_h != api.PM_OK:
            continue
        ch, bh = count64(H_h)
        assert ch <= cw + bw + bh, (h, ch, cw)


# ---- refinement ----------------------------------------------------------------------------------------------------
def test_refit_against_numpy_svd_dlt(ctx):
    """max_iters = 0 returns the S23 refit (when it is cheaper than the RANSAC model): vs numpy SVD over the GPU mask."""
    checked = 0
    for ci, case in enumerate(WIDE_CASES):
        xy1, xy2, _, _ = wide_view(2000, 300 + ci, case)
        rc, H0, mask, c, key = ctx.ransac_homography(xy1, xy2, 500, thresh_for(case), 0x5A + ci)
        assert rc == api.PM_OK
        rc, H, info = ctx.homography_refine(xy1, xy2, mask, H0, 0)
        Hr, ir = RR.refine(xy1, xy2, mask, H0, 0)
        assert _bits_equal(H, Hr) and info.status == ir.status
        if info.status != 0:                       # the RANSAC model was cheaper: H_in kept
            continue
        m = mask.astype(bool)
        Hn, S, _ = np_dlt(xy1[m], xy2[m])
        gap2 = (S[7] ** 2 - S[8] ** 2) / S[0] ** 2
        assert np.linalg.norm(H - Hn) <= REFIT_TOL / gap2, (ci, np.linalg.norm(H - Hn), gap2)
        checked += 1
    assert checked >= 4


@pytest.mark.parametrize("ci", range(len(WIDE_CASES)))
def test_lm_reaches_the_scipy_minimum(ctx, ci):
    case = WIDE_CASES[ci]
    xy1, xy2, _, _ = wide_view(2275, 400 + ci, case)
    rc, H0, mask, c, key = ctx.ransac_homography(xy1, xy2, 1000, thresh_for(case), 0x1F + ci)
    assert rc == api.PM_OK
    for it in (10, 100):
        rc, H, info = ctx.homography_refine(xy1, xy2, mask, H0, it)
        Hr, ir = RR.refine(xy1, xy2, mask, H0, it)
        assert _bits_equal(H, Hr) and info.status == 0 and info.cost_out <= info.cost_in
        check_lm_optimal(xy1, xy2, mask, H0, H, info.cost_out, (ci, it))


def _refine_both(ctx, xy1, xy2, mask, H_in, it, what):
    rc, H, info = ctx.homography_refine(xy1, xy2, mask, H_in, it)
    Hr, ir = RR.refine(xy1, xy2, mask, H_in, it)
    assert _bits_equal(H, Hr), what
    assert _bits_equal([info.cost_in, info.cost_out], [ir.cost_in, ir.cost_out]), what
    assert (info.n_used, info.iters, info.status) == (ir.n_used, ir.iters, ir.status), what
    return H, info


def test_refinement_edges(ctx):
    # 4 to 8 inliers (4: an exact fit, cost ~ 0)
    xy1, xy2, Hg, inl = synth.planar_view_wide(600, seed=5, width=4000, height=3000, outlier_frac=0.3, noise_px=0.8)
    good = np.nonzero(inl)[0]
    for k in range(4, 9):
        m = np.zeros(600, np.uint8)
        m[good[7 * k:7 * k + k]] = 1
        H, info = _refine_both(ctx, xy1, xy2, m, Hg, 10, k)
        assert info.n_used == k
        if info.iters:
            check_lm_optimal(xy1, xy2, m, Hg, H, info.cost_out, k)
    # n = 513 (one point wraps onto partial 0) and 2^20
    for n, it in ((513, 10), (1 << 20, 10)):
        xy1, xy2, _, _ = synth.planar_view_wide(n, seed=n, width=4000, height=3000, outlier_frac=0.3, noise_px=0.7)
        rc, H0, mask, c, key = ctx.ransac_homography(xy1, xy2, 200, 2.8, 0x44)
        assert rc == api.PM_OK
        H, info = _refine_both(ctx, xy1, xy2, mask, H0, it, n)
        assert info.status == 0
        check_lm_optimal(xy1, xy2, mask, H0, H, info.cost_out, n)
    # a start point with |H[8]| < 1e-8: no LM (S24), the refit or H_in comes back
    A = np.array([[0.9, 0.1, -1e-9], [-0.05, 1.1, 2e-9], [2e-4, 3e-4, 5e-9]])
    x1 = np.random.default_rng(3).uniform(100, 3000, (800, 2))
    p = np.column_stack([x1, np.ones(800)]) @ A.T
    xy1, xy2 = x1.astype(np.float32), (p[:, :2] / p[:, 2:3]).astype(np.float32)
    H_in = A / np.linalg.norm(A)
    H, info = _refine_both(ctx, xy1, xy2, np.ones(800, np.uint8), H_in, 10, "h8")
    assert info.iters == 0 and np.isfinite(H).all()


def test_refinement_on_a_64_part_view(ctx):
    import torch
    dev = torch.device("cuda", 0)
    cap, parts = 130, 64
    counts = [(37 * p) % 131 if p % 9 else 0 for p in range(parts)]
    n = sum(counts)
    xy1, xy2, _, _ = synth.planar_view_wide(n, seed=64, width=8000, height=6000, outlier_frac=0.3, noise_px=0.7)
    rc, H0, mask, c, key = ctx.ransac_homography(xy1, xy2, 400, 3.6, 0x64)
    assert rc == api.PM_OK
    d1, d2, dc, _ = _parts_view(torch, dev, xy1, xy2, counts, cap)
    view = api.PointsView(d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), parts, cap, 2 * cap + 6, 1, 0)
    dm = torch.zeros(parts * cap, dtype=torch.uint8, device=dev)
    dm[:n] = torch.from_numpy(mask).to(dev)
    d_Hin = torch.from_numpy(H0.reshape(9).copy()).to(dev)
    d_H = torch.full((9,), 7.0, dtype=torch.float64, device=dev)
    d_info = torch.zeros(32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.homography_refine_dev(view, dm.data_ptr(), d_Hin.data_ptr(), 10, d_H.data_ptr(), d_info.data_ptr())
    ctx.synchronize()
    H = d_H.cpu().numpy().reshape(3, 3)
    info = d_info.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0]
    Hr, ir = RR.refine(xy1, xy2, mask, H0, 10)
    assert _bits_equal(H, Hr) and _bits_equal([info["cost_out"]], [ir.cost_out]) and int(info["status"]) == ir.status == 0
    check_lm_optimal(xy1, xy2, mask, H0, H, float(info["cost_out"]), "64 parts")


# ---- kernel shapes -------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("n", [4, 127, 128, 129, 8191, 8192, 8193, 16385, 40000])
def test_sizes_around_slot_and_tile_boundaries(ctx, n):
    case = WIDE_CASES[2]
    xy1, xy2, _, _ = wide_view(n, n, case[:6] + (0.0 if n == 4 else 0.3,))
    _check_run(ctx, xy1, xy2, 300 if n > 8192 else 700, thresh_for(case), 0xE0, what=n)


def test_pinned_ids_per_workgroup(ctx):
    """PM_OPT_RANSAC_WG_IDS: one or two solver waves, partial last workgroups, every score_lds<HModel, 1..4> branch."""
    case = WIDE_CASES[3]
    xy1, xy2, _, _ = wide_view(3000, 11, case)
    thr = thresh_for(case)
    want = {nh: R.run(xy1, xy2, nh, thr, 0x9D) for nh in (1037, 333)}
    try:
        for ids in (1, 12, 13, 64, 65, 127, 128):
            ctx.set_option(api.PM_OPT_RANSAC_WG_IDS, ids)
            for nh in (1037, 333):
                rc, H, mask, c, key = ctx.ransac_homography(xy1, xy2, nh, thr, 0x9D)
                kr, Hr, mr, cr = want[nh]
                assert key == kr and _bits_equal(H, Hr) and (mask == mr).all() and c == cr, (ids, nh)
    finally:
        ctx.set_option(api.PM_OPT_RANSAC_WG_IDS, 0)
    check_mask_vs_float64(want[1037][1], xy1, xy2, thr, want[1037][2])


def test_ids_near_2_pow_32_and_sharding_there(ctx):
    import torch
    dev = torch.device("cuda", 0)
    case = WIDE_CASES[5]
    xy1, xy2, _, _ = wide_view(2275, 32, case)
    thr, top = thresh_for(case), 1 << 32
    key, H, mask, c = _check_run(ctx, xy1, xy2, top, thr, 0x32, hyp_begin=top - 5000, what="top")
    assert key and api.ransac_key_hyp(key) >= top - 5000
    f1, f2 = torch.from_numpy(xy1).to(dev), torch.from_numpy(xy2).to(dev)
    view = api.PointsView(f1.data_ptr(), f2.data_ptr(), None, 1, 2275, 0, 1, 0)
    for a in (top - 4999, top - 2500, top - 1):
        ka, Ha, _, _, _ = _run_dev(ctx, view, top - 5000, a, thr, 0x32, 2275)
        kb, Hb, _, _, _ = _run_dev(ctx, view, a, top, thr, 0x32, 2275)
        assert max(ka, kb) == key, a
        assert _bits_equal(Ha if ka > kb else Hb, H), a


def test_64_part_view_uneven_counts(ctx):
    import torch
    dev = torch.device("cuda", 0)
    cap, parts = 130, 64
    counts = [0 if p % 7 == 3 else (53 * p + 11) % 131 for p in range(parts)]
    n = sum(counts)
    xy1, xy2, _, _ = wide_view(n, 640, WIDE_CASES[4])
    thr = thresh_for(WIDE_CASES[4])
    d1, d2, dc, pitch = _parts_view(torch, dev, xy1, xy2, counts, cap)
    view = api.PointsView(d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), parts, cap, pitch, 1, 0)
    key, H, mask, c, guard = _run_dev(ctx, view, 0, 1500, thr, 0x40, parts * cap)
    kr, Hr, mr, cr = R.run(xy1, xy2, 1500, thr, 0x40)
    assert key == kr and _bits_equal(H, Hr) and c == cr and (mask[:n] == mr).all() and not mask[n:].any()
    assert (guard == 7).all()
    check_mask_vs_float64(H, xy1, xy2, thr, mask[:n])


@pytest.mark.parametrize("count", [8000, 9000])
def test_capacity_beyond_one_lds_tile(ctx, count):
    """cap 10000 > 8192 points per LDS tile with a device count below it: one tile (8000) or two (9000)."""
    import torch
    dev = torch.device("cuda", 0)
    cap = 10000
    xy1, xy2, _, _ = wide_view(cap, 10000, WIDE_CASES[2])
    thr = thresh_for(WIDE_CASES[2])
    f1, f2 = torch.from_numpy(xy1).to(dev), torch.from_numpy(xy2).to(dev)
    dn = torch.tensor([count], dtype=torch.int32, device=dev)
    view = api.PointsView(f1.data_ptr(), f2.data_ptr(), dn.data_ptr(), 1, cap, 0, 1, 0)
    key, H, mask, c, guard = _run_dev(ctx, view, 0, 600, thr, 0x7E, cap)
    kr, Hr, mr, cr = R.run(xy1[:count], xy2[:count], 600, thr, 0x7E)
    assert key == kr and _bits_equal(H, Hr) and c == cr and (mask[:count] == mr).all() and not mask[count:].any()
    assert (guard == 7).all()
    check_mask_vs_float64(H, xy1[:count], xy2[:count], thr, mask[:count])


def test_mask_shorter_and_longer_than_n(ctx):
    import torch
    dev = torch.device("cuda", 0)
    n = 3001
    xy1, xy2, _, _ = wide_view(n, 3001, WIDE_CASES[3])
    thr = thresh_for(WIDE_CASES[3])
    kr, Hr, mr, cr = R.run(xy1, xy2, 800, thr, 0x31)
    f1, f2 = torch.from_numpy(xy1).to(dev), torch.from_numpy(xy2).to(dev)
    view = api.PointsView(f1.data_ptr(), f2.data_ptr(), None, 1, n, 0, 1, 0)
    for mask_len in (0, 1, 100, 2999, n + 1, n + 127, n + 300):
        key, H, mask, c, guard = _run_dev(ctx, view, 0, 800, thr, 0x31, mask_len)
        k = min(mask_len, n)
        assert key == kr and _bits_equal(H, Hr) and c == cr, mask_len      # the count covers all n
        assert (mask[:k] == mr[:k]).all() and not mask[k:].any() and (guard == 7).all(), mask_len


# ---- non-finite input ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 3])
def test_nonfinite_rows(ctx, ci):
    """5 % of the rows carry a NaN, an infinity or +-1e30: bit parity, never inliers, the planted H still found, and
    the refinement on that mask stays finite."""
    case = WIDE_CASES[ci]
    xy1, xy2, Hg, inl = wide_view(3000, 900 + ci, case)
    a, b, bad = nonfinite_rows(xy1, xy2, 0.05, ci)
    thr = thresh_for(case)
    rc, H, mask, c, key = ctx.ransac_homography(a, b, 1500, thr, 0xF0 + ci)
    kr, Hr, mr, cr = R.run(a, b, 1500, thr, 0xF0 + ci)
    assert rc == api.PM_OK and key == kr and _bits_equal(H, Hr) and (mask == mr).all() and c == cr
    assert not mask[bad].any()
    ok = ~bad
    check_mask_vs_float64(H, a[ok], b[ok], thr, mask[ok], ci)
    assert mean_transfer_between(H, Hg, xy1, inl & ok) < thr          # (x1 noise is magnified up to ~9x here)
    H2, info = _refine_both(ctx, a, b, mask, H, 10, ci)
    assert np.isfinite(H2).all() and np.isfinite([info.cost_in, info.cost_out]).all() and info.status == 0
    assert mean_transfer_between(H2, Hg, xy1, inl & ok) < 0.5 * thr
