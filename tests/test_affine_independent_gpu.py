"""GPU: the HIP robust affine / similarity estimation (RANSAC-A, SPEC S26-S29) and its refit (S30) against DIFFERENT
algorithms — numpy.linalg.solve on the minimal systems, a numpy statement of the S27 sample rule, float64 forward
residuals, numpy.linalg.lstsq, Umeyama's SVD closed form, scipy's MINPACK LM and a numpy statement of the refit's det
rule — at mild and hard geometry (synth.affine_view_wide), plus the kernel shapes the other affine suites do not reach
(LDS slot and tile boundaries, pinned ids per workgroup, the id 2^32 - 1, short, long and empty masks with guard bytes,
capacities above one tile, device counts out of range, non-finite rows, threshold edges), each bit for bit against the
C restatement as well.  The sampler indices come from affine_ref.sample: they are spec data, not arithmetic.  The
twin of tests/test_homography_independent_gpu.py for the affine family; every case runs for both models."""
import numpy as np
import pytest

import affine_ref as R
from points_matching_amd import api
from test_affine_independent_cpu import (FULL, MODELS, PARTIAL, SOLVE_K, EPS64, THRESH_EDGES, WIDE_CASES,
                                         check_mask_vs_float64, check_refit_optimal, check_refit_vs_lstsq,
                                         forward_cost, np_det_rule, np_minimal, np_sample_rule, poisoned_rows, positions,
                                         residual64, strip, strip_spread, thresh_for, wide_view)
from test_homography_independent_gpu import _parts_view

pytestmark = pytest.mark.gpu
GUARD = 256


def _bits_equal(a, b):
    return (np.asarray(a, np.float64).view(np.uint64) == np.asarray(b, np.float64).view(np.uint64)).all()


def _same_costs(a, b):
    """Bit for bit, except that any NaN equals any NaN: a NaN's sign and payload are not specified (a NaN row makes the
    sums NaN, and the host and the device produce different default NaNs)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all()


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


def _flat_view(torch, dev, xy1, xy2, count=None, cap=None):
    """One part over device copies of (xy1, xy2); `count` (may be out of range) read on the device if given."""
    f1, f2 = torch.from_numpy(np.ascontiguousarray(xy1)).to(dev), torch.from_numpy(np.ascontiguousarray(xy2)).to(dev)
    dn = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    cap = len(xy1) if cap is None else cap
    view = api.PointsView(f1.data_ptr(), f2.data_ptr(), None if dn is None else dn.data_ptr(), 1, cap, 0, 1, 0)
    return view, (f1, f2, dn)


def _run_dev(ctx, model, view, hb, he, thr, seed, mask_len):
    """run_dev with poisoned outputs and GUARD sentinel bytes past mask_len: (key, A, mask, count, guard bytes)."""
    torch, dev = _dev()
    k = torch.zeros(1, dtype=torch.int64, device=dev)
    A = torch.full((8,), 7.0, dtype=torch.float64, device=dev)
    m = torch.full((mask_len + GUARD,), 7, dtype=torch.uint8, device=dev)
    c = torch.full((1,), 99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.ransac_affine_run_dev(view, hb, he, thr, seed, k.data_ptr(), A.data_ptr(), m.data_ptr(), mask_len, c.data_ptr(),
                              model=model)
    ctx.synchronize()
    a, mm = A.cpu().numpy(), m.cpu().numpy()
    assert (a[6:] == 7.0).all()                       # exactly 6 doubles are written
    return int(k.item()) & ((1 << 64) - 1), a[:6].reshape(2, 3), mm[:mask_len], int(c.item()), mm[mask_len:]


def _check_run(ctx, model, xy1, xy2, iters, thr, seed, hyp_begin=0, what=""):
    """Whole host run: key, A, mask and count bit for bit with the restatement, the mask against float64."""
    rc, A, mask, c, key = ctx.ransac_affine(xy1, xy2, iters, thr, seed, model=model, hyp_begin=hyp_begin)
    kr, Ar, mr, cr = R.run(model, xy1, xy2, iters, thr, seed, hyp_begin)
    assert key == kr, (what, hex(key), hex(kr))
    assert _bits_equal(A, Ar) and (mask == mr).all() and c == cr, what
    if kr:
        assert rc == api.PM_OK and c == mask.sum()
        t2 = np.float64(np.float32(thr)) ** 2
        if 1e-30 < t2 < np.finfo(np.float32).max:        # a threshold that admits anything, above the subnormals
            check_mask_vs_float64(A, xy1, xy2, abs(thr), mask, what)
    else:
        assert rc == api.PM_E_NO_MODEL and not A.any() and not mask.any()
    return key, A, mask, c


def _refit_both(ctx, model, xy1, xy2, mask, A_in, what=""):
    """Host refit: A, costs, n_used and status bit for bit with the restatement."""
    rc, A, info = ctx.affine_refine(xy1, xy2, mask, A_in, model=model)
    st, Ar, cin, cout, nu = R.refine(model, xy1, xy2, mask, A_in)
    assert rc == (api.PM_E_NO_MODEL if st == 2 else api.PM_OK), what
    assert _bits_equal(A, Ar), (what, A, Ar)
    assert _same_costs([info.cost_in, info.cost_out], [cin, cout]), what
    assert (info.status, info.n_used, info.iters) == (st, nu, 0), what
    return st, A, info


def _refit_dev(ctx, model, view, mask, A_in, alias=False, with_info=True):
    """Device refit over `view`: (A_out, info record or None).  alias: A_out is the A_in buffer itself."""
    torch, dev = _dev()
    dm = torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(dev)
    dA = torch.from_numpy(np.asarray(A_in, np.float64).reshape(6).copy()).to(dev)
    dAo = dA if alias else torch.full((6,), 7.0, dtype=torch.float64, device=dev)
    dinfo = torch.full((4,), 7.0, dtype=torch.float64, device=dev) if with_info else None
    torch.cuda.synchronize()
    ctx.affine_refine_dev(view, dm.data_ptr(), dA.data_ptr(), dAo.data_ptr(), dinfo.data_ptr() if with_info else None,
                          model=model)
    ctx.synchronize()
    info = dinfo.cpu().numpy().view(api.H_REFINE_INFO_DTYPE)[0] if with_info else None
    return dAo.cpu().numpy().reshape(2, 3), info


# ---- single hypotheses ---------------------------------------------------------------------------------------------
def _plant_image2_degenerate(model, xy2, seed, n, hs):
    """Make the samples of ids `hs` degenerate in image 2 ONLY: full — two of them an exactly collinear integer triple,
    one of them a coincident pair; partial — the pair coincident.  Ids whose samples overlap an earlier one are skipped.
    Returns the planted ids."""
    used, planted = set(), []
    for j, h in enumerate(hs):
        idx = [int(i) for i in R.sample(model, seed, h, n)]
        if used & set(idx):
            continue
        used |= set(idx)
        if model == FULL and j % 3:
            base = np.array([100.0 + 7 * j, 200.0 + 3 * j])
            for s, i in enumerate(idx):
                xy2[i] = base + s * np.array([200.0, 60.0])          # exactly collinear in f32 and f64
        else:
            xy2[idx[-1]] = xy2[idx[0]]
        planted.append(h)
    return planted


@pytest.mark.parametrize("model", MODELS)
def test_single_hypotheses_against_numpy(ctx, model):
    """A vs numpy.linalg.solve of the sampled points, validity vs the numpy S27 rule, mask vs float64 residuals: at
    least 1000 valid ids over mild and hard geometry; planted samples degenerate only in image 2 give PM_E_NO_MODEL."""
    valid = clear = planted_seen = 0
    for ci in (0, 2, 4, 6):
        case, n = WIDE_CASES[ci], 500
        xy1, xy2, Ag, _ = wide_view(n, 200 + ci, case, model)
        thr, seed = thresh_for(case, Ag), 0xA11 + ci
        planted = set(_plant_image2_degenerate(model, xy2, seed, n, range(1000, 1040)))
        assert len(planted) >= 15
        for h in list(range(330)) + sorted(planted):
            rc, A, mask, c = ctx.ransac_affine_from_hyp(xy1, xy2, h, thr, seed, model=model)
            idx = R.sample(model, seed, h, n)
            p1, p2 = xy1[idx].astype(np.float64), xy2[idx].astype(np.float64)
            ok_np, is_clear = np_sample_rule(model, p1, p2)
            ok = rc == api.PM_OK
            if h in planted:
                assert not ok_np and is_clear and R.solve(model, p1, p1 * 1.5 + 3)[0], (ci, h)   # image 1 alone is fine
                assert rc == api.PM_E_NO_MODEL and not A.any() and not mask.any() and c == 0, (ci, h, A)
                planted_seen += 1
                continue
            if is_clear:
                assert ok == ok_np, (ci, h, rc)
                clear += 1
            if not ok:
                assert rc == api.PM_E_NO_MODEL and not A.any() and not mask.any() and c == 0, (ci, h)
                continue
            An, cond = np_minimal(model, p1, p2)
            err = np.abs(A - An).max() / np.abs(An).max()
            assert err <= SOLVE_K * EPS64 * cond, (ci, h, err, cond)
            assert c == mask.sum()
            check_mask_vs_float64(A, xy1, xy2, thr, mask, (ci, h))
            valid += 1
    assert valid >= 1000 and clear >= 1250 and planted_seen >= 60, (valid, clear, planted_seen)


@pytest.mark.parametrize("model", MODELS)
def test_winner_is_the_best_model_by_float64_count(ctx, model):
    """The run's winner has at least as many float64-counted inliers as every other id of the run, up to the points
    within the rounding band of either model."""
    case = WIDE_CASES[6]
    xy1, xy2, Ag, _ = wide_view(1500, 77, case, model)
    thr, seed = thresh_for(case, Ag), 0x3E
    rc, A, mask, c, key = ctx.ransac_affine(xy1, xy2, 300, thr, seed, model=model)
    assert rc == api.PM_OK

    def count64(M):
        d, err = residual64(M.astype(np.float32).astype(np.float64), xy1, xy2)
        border = np.abs(d - thr) <= 1e-3 * thr + err
        return int((d <= thr).sum()), int(border.sum())
    cw, bw = count64(A)
    assert abs(cw - c) <= bw
    for h in range(300):
        rc_h, A_h, _, _ = ctx.ransac_affine_from_hyp(xy1, xy2, h, thr, seed, model=model)
        if rc_h != api.PM_OK:
            continue
        ch, bh = count64(A_h)
        assert ch <= cw + bw + bh, (h, ch, cw)


# ---- refit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_refit_at_wide_cases(ctx, model):
    """Bit parity with the restatement, lstsq (and Umeyama for the partial model), scipy's minimum, idempotence; the
    estimate call (RANSAC + refit, one synchronisation) gives the same bits."""
    for ci, case in enumerate(WIDE_CASES):
        xy1, xy2, Ag, _ = wide_view(2000, 300 + ci, case, model)
        thr, seed = thresh_for(case, Ag), 0x5A + ci
        rc, A0, mask, c, key = ctx.ransac_affine(xy1, xy2, 500, thr, seed, model=model)
        assert rc == api.PM_OK
        st, A, info = _refit_both(ctx, model, xy1, xy2, mask, A0, ci)
        assert st == 0 and info.cost_out <= info.cost_in and info.n_used == c
        check_refit_vs_lstsq(model, xy1, xy2, mask, A, ci)
        assert abs(forward_cost(model, xy1, xy2, mask, A) - info.cost_out) <= 1e-9 * info.cost_out
        check_refit_optimal(model, xy1, xy2, mask, A0, info.cost_out, ci)
        st2, A2, info2 = _refit_both(ctx, model, xy1, xy2, mask, A, ci)
        assert st2 == 0 and _bits_equal(A2, A) and info2.cost_in == info2.cost_out == info.cost_out
        rc, Ae, me, ce, ke, infoe = ctx.estimate_affine(xy1, xy2, 500, thr, seed, model=model)
        assert rc == api.PM_OK and ke == key and (me == mask).all() and _bits_equal(Ae, A) and infoe.status == 0


@pytest.mark.parametrize("model", MODELS)
def test_refit_edges(ctx, model):
    torch, dev = _dev()
    # collinear inliers: the full normal system is singular (status 1), the partial one is not (status 0)
    x = np.linspace(5, 3950, 300)
    l1 = np.column_stack([x, 0.3 * x + 11]).astype(np.float32)
    A_gt = np.array([[0.8, 0.1, 3.0], [-0.1, 0.8, 20.0]])
    l2 = positions(A_gt, l1).astype(np.float32)
    st, A, info = _refit_both(ctx, model, l1, l2, np.ones(300, np.uint8), A_gt + 1e-3, "line")
    assert st == (1 if model == FULL else 0)
    # the thin strip on both sides of the relative-det rule: the refit runs exactly when the numpy rule says so
    L, A_in = 4000.0, A_gt + [[1e-3, -2e-3, 3.0], [2e-3, 1e-3, -4.0]]
    for r in (0.01, 0.3, 0.8, 1.25, 3.0, 100.0):
        p1 = strip(600, int(r * 1000) + 1, L, strip_spread(r, L))
        p2 = positions(A_gt, p1).astype(np.float32)
        valid, clear, ratio = np_det_rule(p1)
        st, A, info = _refit_both(ctx, model, p1, p2, np.ones(600, np.uint8), A_in, r)
        assert clear
        if model == PARTIAL or valid:
            assert st == 0 and info.cost_out < info.cost_in, (r, ratio)
        else:
            assert st == 1 and _bits_equal(A, A_in), (r, ratio)
    # a NaN or Inf row inside the mask: cost_in is NaN or inf, status 1, A_out = A_in bit for bit
    xy1, xy2, Ag, _ = wide_view(700, 3, WIDE_CASES[3], model)
    for j, v in enumerate((np.nan, np.inf, -np.inf, np.nan)):
        a, b = xy1.copy(), xy2.copy()
        (a if j % 2 else b)[100 + j, j % 2] = v
        st, A, info = _refit_both(ctx, model, a, b, np.ones(700, np.uint8), Ag, v)
        assert st == 1 and _bits_equal(A, Ag) and not np.isfinite(info.cost_in) and _same_costs(info.cost_out, info.cost_in)
    # n around the 512 partials, and 32768: parity, idempotence; the device form with A_out aliasing A_in and no info
    for n in (511, 512, 513, 32768):
        xy1, xy2, Ag, _ = wide_view(n, n, WIDE_CASES[4], model)
        rc, A0, mask, c, key = ctx.ransac_affine(xy1, xy2, 300, thresh_for(WIDE_CASES[4], Ag), 0x44, model=model)
        assert rc == api.PM_OK
        st, A, info = _refit_both(ctx, model, xy1, xy2, mask, A0, n)
        assert st == 0
        st2, A2, info2 = _refit_both(ctx, model, xy1, xy2, mask, A, n)
        assert st2 == 0 and _bits_equal(A2, A) and info2.cost_in == info2.cost_out
        view, keep = _flat_view(torch, dev, xy1, xy2)
        Ad, di = _refit_dev(ctx, model, view, mask, A0, alias=True)
        assert _bits_equal(Ad, A) and int(di["status"]) == 0 and _bits_equal([di["cost_out"]], [info.cost_out]), n
        Ad, di = _refit_dev(ctx, model, view, mask, A0, with_info=False)
        assert _bits_equal(Ad, A) and di is None, n
    # a single-part view whose device count is 0, negative or above cap (clamped to [0, cap])
    n = 3000
    xy1, xy2, Ag, _ = wide_view(n, 30, WIDE_CASES[5], model)
    mask = (np.arange(n) % 4 != 1).astype(np.uint8)
    st_all, A_all, info_all = _refit_both(ctx, model, xy1, xy2, mask, Ag, "cap")
    for cnt in (0, -5, n + 1, 1 << 30):
        view, keep = _flat_view(torch, dev, xy1, xy2, count=cnt)
        Ad, di = _refit_dev(ctx, model, view, mask, Ag)
        if cnt <= 0:
            assert int(di["status"]) == 1 and int(di["n_used"]) == 0 and _bits_equal(Ad, Ag), cnt
        else:
            assert _bits_equal(Ad, A_all) and int(di["status"]) == st_all, cnt
            assert _bits_equal([di["cost_in"], di["cost_out"]], [info_all.cost_in, info_all.cost_out]), cnt
        key, A, m, c, guard = _run_dev(ctx, model, view, 0, 200, 2.0, 0x9, n)
        kr, Ar, mr, cr = R.run(model, xy1[:max(min(cnt, n), 0)], xy2[:max(min(cnt, n), 0)], 200, 2.0, 0x9)
        assert key == kr and _bits_equal(A, Ar) and c == cr and (guard == 7).all(), cnt
        k = max(min(cnt, n), 0)
        assert (m[:k] == mr[:k]).all() and not m[k:].any(), cnt


# ---- kernel shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", ["min", 127, 128, 129, 8191, 8192, 8193, 16385, 40000])
def test_sizes_around_slot_and_tile_boundaries(ctx, model, n):
    n = R.min_pts(model) if n == "min" else n
    case = WIDE_CASES[2]
    xy1, xy2, Ag, _ = wide_view(n, n, case[:9] + (0.0 if n < 5 else 0.3,), model)
    _check_run(ctx, model, xy1, xy2, 300 if n > 8192 else 700, thresh_for(case, Ag), 0xE0, what=n)


@pytest.mark.parametrize("model", MODELS)
def test_pinned_ids_per_workgroup(ctx, model):
    """PM_OPT_RANSAC_WG_IDS: one or two solver waves, partial last workgroups, every score_lds<AModel, 1..4> branch.  A
    value above 128 is refused by the option call and leaves the pinned value in force."""
    case = WIDE_CASES[3]
    xy1, xy2, Ag, _ = wide_view(3000, 11, case, model)
    thr = thresh_for(case, Ag)
    want = {nh: R.run(model, xy1, xy2, nh, thr, 0x9D) for nh in (1037, 333)}
    try:
        for ids in (1, 2, 12, 13, 63, 64, 65, 127, 128, 129):
            if ids > 128:
                with pytest.raises(api.PmError):
                    ctx.set_option(api.PM_OPT_RANSAC_WG_IDS, ids)
                assert ctx.get_option(api.PM_OPT_RANSAC_WG_IDS) == 128
            else:
                ctx.set_option(api.PM_OPT_RANSAC_WG_IDS, ids)
            for nh in (1037, 333):
                rc, A, mask, c, key = ctx.ransac_affine(xy1, xy2, nh, thr, 0x9D, model=model)
                kr, Ar, mr, cr = want[nh]
                assert key == kr and _bits_equal(A, Ar) and (mask == mr).all() and c == cr, (ids, nh)
    finally:
        ctx.set_option(api.PM_OPT_RANSAC_WG_IDS, 0)
    check_mask_vs_float64(want[1037][1], xy1, xy2, thr, want[1037][2])


@pytest.mark.parametrize("model", MODELS)
def test_the_last_id_and_masks_of_every_length(ctx, model):
    torch, dev = _dev()
    n = 3001
    xy1, xy2, Ag, _ = wide_view(n, 3001, WIDE_CASES[6], model)
    thr, top = thresh_for(WIDE_CASES[6], Ag), (1 << 32) - 1
    # the single id 2^32 - 1, alone and as the last id of a run
    rc, A, mask, c = ctx.ransac_affine_from_hyp(xy1, xy2, top, thr, 0x31, model=model)
    ok, Ar = R.model_of(model, xy1, xy2, 0x31, top)
    assert ok and rc == api.PM_OK and _bits_equal(A, Ar) and (mask == R.score(Ar, xy1, xy2, thr)[0]).all()
    key, A2, _, _ = _check_run(ctx, model, xy1, xy2, 1 << 32, thr, 0x31, hyp_begin=top, what="top")
    assert api.ransac_key_hyp(key) == top and _bits_equal(A2, A)
    _check_run(ctx, model, xy1, xy2, 1 << 32, thr, 0x31, hyp_begin=top - 700, what="top-700")
    # the flat device form with mask_len 0, shorter and longer than n: guard bytes past mask_len untouched
    kr, Ar, mr, cr = R.run(model, xy1, xy2, 800, thr, 0x31)
    view, keep = _flat_view(torch, dev, xy1, xy2)
    for mask_len in (0, 1, 100, 2999, n, n + 1, n + 127, n + 300):
        key, A, m, c, guard = _run_dev(ctx, model, view, 0, 800, thr, 0x31, mask_len)
        k = min(mask_len, n)
        assert key == kr and _bits_equal(A, Ar) and c == cr, mask_len          # the count covers all n
        assert (m[:k] == mr[:k]).all() and not m[k:].any() and (guard == 7).all(), mask_len


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("count", [8000, 9000])
def test_capacity_beyond_one_lds_tile(ctx, model, count):
    """cap 10000 > 8192 points per LDS tile with a device count below it: one tile (8000) or two (9000)."""
    torch, dev = _dev()
    cap = 10000
    xy1, xy2, Ag, _ = wide_view(cap, cap, WIDE_CASES[2], model)
    thr = thresh_for(WIDE_CASES[2], Ag)
    view, keep = _flat_view(torch, dev, xy1, xy2, count=count)
    key, A, mask, c, guard = _run_dev(ctx, model, view, 0, 600, thr, 0x7E, cap)
    kr, Ar, mr, cr = R.run(model, xy1[:count], xy2[:count], 600, thr, 0x7E)
    assert key == kr and _bits_equal(A, Ar) and c == cr and (mask[:count] == mr).all() and not mask[count:].any()
    assert (guard == 7).all()
    check_mask_vs_float64(A, xy1[:count], xy2[:count], thr, mask[:count])


@pytest.mark.parametrize("model", MODELS)
def test_64_part_view_uneven_counts(ctx, model):
    torch, dev = _dev()
    cap, parts = 130, 64
    counts = [0 if p % 7 == 3 else (53 * p + 11) % 131 for p in range(parts)]
    n = sum(counts)
    xy1, xy2, Ag, _ = wide_view(n, 640, WIDE_CASES[4], model)
    thr = thresh_for(WIDE_CASES[4], Ag)
    d1, d2, dc, pitch = _parts_view(torch, dev, xy1, xy2, counts, cap)
    view = api.PointsView(d1.data_ptr(), d2.data_ptr(), dc.data_ptr(), parts, cap, pitch, 1, 0)
    key, A, mask, c, guard = _run_dev(ctx, model, view, 0, 1500, thr, 0x40, parts * cap)
    kr, Ar, mr, cr = R.run(model, xy1, xy2, 1500, thr, 0x40)
    assert key == kr and _bits_equal(A, Ar) and c == cr and (mask[:n] == mr).all() and not mask[n:].any()
    assert (guard == 7).all()
    Ad, di = _refit_dev(ctx, model, view, np.concatenate([mr, np.zeros(parts * cap - n, np.uint8)]), Ar)
    st, Arr, info = _refit_both(ctx, model, xy1, xy2, mr, Ar, "64 parts")
    assert _bits_equal(Ad, Arr) and int(di["status"]) == st == 0


# ---- non-finite input and thresholds -------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("ci", [0, 6])
def test_nonfinite_rows(ctx, model, ci):
    """5 % of the rows, and rows the first 60 ids sample, carry NaN, +-Inf, +-1e30, 3e38, a subnormal or -0.0 in one
    coordinate of either image: key, A and mask bit for bit, NaN and Inf rows never inliers, samples that include one
    invalid; the refit on that mask stays finite."""
    case = WIDE_CASES[ci]
    xy1, xy2, Ag, inl = wide_view(3000, 900 + ci, case, model)
    thr, seed = thresh_for(case, Ag), 0xF0 + ci
    sampled = np.concatenate([R.sample(model, seed, h, 3000) for h in range(60)])
    a, b, bad, nonfin = poisoned_rows(xy1, xy2, 0.05, ci, ids=sampled)
    key, A, mask, c = _check_run(ctx, model, a, b, 1500, thr, seed, what=ci)
    assert key and not mask[nonfin].any()
    invalid = 0
    for h in range(60):
        idx = R.sample(model, seed, h, 3000)
        rc, Ah, mh, ch = ctx.ransac_affine_from_hyp(a, b, h, thr, seed, model=model)
        ok, Ar = R.model_of(model, a, b, seed, h)
        assert (rc == api.PM_OK) == ok and _bits_equal(Ah, Ar), h
        if nonfin[idx].any():
            assert rc == api.PM_E_NO_MODEL and not Ah.any() and not mh.any(), h
            invalid += 1
        elif ok:
            assert (mh == R.score(Ar, a, b, thr)[0]).all() and not mh[nonfin].any(), h
    assert invalid >= 10
    st, Ar, info = _refit_both(ctx, model, a, b, mask, A, ci)
    assert st == 0 and np.isfinite(Ar).all() and np.isfinite([info.cost_in, info.cost_out]).all()


@pytest.mark.parametrize("model", MODELS)
def test_threshold_edges(ctx, model):
    """thresh_px 0, NaN, +-inf, 2e19 (thr2 overflows to inf) admit nothing; a negative threshold acts as its magnitude,
    a subnormal thr2 admits only exact rows; everything bit for bit with the restatement."""
    xy1, xy2, Ag, inl = wide_view(1500, 12, WIDE_CASES[0], model)
    A32 = Ag.astype(np.float32)
    xy1[:4] = 0.0
    xy2[:4] = A32[:, 2]
    xy2[4:8] = A32[:, 2] + np.float32(3e-20)
    for t, admits in THRESH_EDGES:
        key, A, mask, c = _check_run(ctx, model, xy1, xy2, 400, t, 0x7, what=t)
        assert key and (api.ransac_key_inliers(key) > 0) == admits and (c > 0) == admits, t
        if not admits:
            assert not mask.any(), t
        rc, Ah, mh, ch = ctx.ransac_affine_from_hyp(xy1, xy2, 3, t, 0x7, model=model)
        ok, Ar = R.model_of(model, xy1, xy2, 0x7, 3)
        mr, cr = R.score(Ar, xy1, xy2, t)
        assert (rc == api.PM_OK) == ok and _bits_equal(Ah, Ar) and (mh == mr).all() and ch == cr, t
        if not admits:
            assert not mh.any(), t
    _, _, m_neg, _ = _check_run(ctx, model, xy1, xy2, 400, -2.5, 0x7, what="neg")
    _, _, m_pos, _ = _check_run(ctx, model, xy1, xy2, 400, 2.5, 0x7, what="pos")
    assert (m_neg == m_pos).all()
