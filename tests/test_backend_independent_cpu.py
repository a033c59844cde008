"""The 3-D back end's restatements (tests/triangulate_ref.c: SPEC S93-S96, tests/align3d_ref.c: S97-S101, tests/ba_ref.c:
S113-S117) against DIFFERENT algorithms at hard geometry (synth.multiview_scene_wide, synth.align3d_scene_wide: maps 1e4
units from the origin, any rotation, turns of 60 and 180 degrees, parallax of 1e-3, depths of 1:1000, 16000 px images,
scales of 1e-3 .. 1e3, exactly flat and collinear clouds, non-finite rows): numpy's SVD null vector and a damped
Gauss-Newton with full solves for triangulation, SVD Kabsch / Umeyama and float64 distances for the alignment, a dense
stacked-Jacobian least-squares solver for the bundle adjustment.  The GPU suites compare the HIP kernels with the
restatements bit for bit, so these tests anchor that chain; the case tables, helpers and tolerances live in
tests/backend_cases.py and are shared with tests/test_backend_independent_gpu.py, which runs the same checks on the
kernels' own output.  Every test prints the worst value of what it measures; the last one prints the table."""
import time

import numpy as np
import pytest

import align3d_ref as AR
import ba_ref as B
import backend_cases as BC
import triangulate_ref as T
from points_matching_amd import synth

T0 = time.time()
WORST = {}                    # quantity -> (worst value, the case it came from)


def note(measures, case):
    for k, v in measures.items():
        if isinstance(v, dict):
            continue
        if k not in WORST or v > WORST[k][0]:
            WORST[k] = (v, case)
    print(case, {k: (float("%.3g" % v) if not isinstance(v, dict) else v) for k, v in measures.items()})


TRI_RUNS = [(name, V) for name in BC.TRI_NAMES for V in BC.TRI_VIEWS]


def test_tables_and_parametrisations_have_the_same_names():
    import test_backend_independent_gpu as G
    assert [c[0] for c in BC.TRI_CASES] == ["far-1e3", "far-1e4", "parallax-1e-2", "parallax-1e-3", "depth-1000",
                                            "narrow-16000", "wide-fov", "rot-any", "forward", "noisy-far", "nonfinite"]
    assert [c[0] for c in BC.ALIGN_CASES] == ["far-1e4", "scale-1e-3", "scale-1e3", "rot-180", "rot-179.9", "rot-1e-6",
                                              "planar-1e-4", "planar-exact", "line-1e-3", "line-exact", "tiny-span",
                                              "half-outliers", "nonfinite"]
    assert [c[0] for c in BC.BA_CASES] == ["far-1e2", "far-1e3", "far-3e3", "far-1e4", "depth-1000", "narrow-16000", "rot-60",
                                           "parallax-0.05", "gated", "nonfinite"]
    assert TRI_RUNS == G.TRI_RUNS and {n for n, _ in TRI_RUNS} == set(BC.TRI_NAMES) and {v for _, v in TRI_RUNS} == {2, 5, 8}
    assert G.ALIGN_RUNS is BC.ALIGN_RUNS and {n for n, _ in BC.ALIGN_RUNS} == set(BC.ALIGN_NAMES)
    assert G.BA_RUNS is BC.BA_RUNS and {n for n, _, _ in BC.BA_RUNS} == set(BC.BA_NAMES)
    assert {v for _, v, _ in BC.BA_RUNS} == {3, 5} and {m for _, v, m in BC.BA_RUNS if v == 5} == {1, 3, 15}

    def params(fn):
        return [m.args[1] for m in fn.pytestmark if m.name == "parametrize"][0]

    for fn, table in ((G.test_triangulation_at_hard_geometry, TRI_RUNS), (G.test_alignment_at_hard_geometry, BC.ALIGN_RUNS),
                      (G.test_bundle_adjustment_at_hard_geometry, BC.BA_RUNS),
                      (test_restated_triangulation_matches_numpy, TRI_RUNS),
                      (test_restated_triangulation_from_a_perturbed_map_reaches_the_same_minimum, TRI_RUNS),
                      (test_restated_refit_matches_kabsch_umeyama, BC.ALIGN_RUNS),
                      (test_restated_run_finds_the_planted_transform, BC.ALIGN_RUNS),
                      (test_restated_bundle_adjustment_matches_the_dense_solver, BC.BA_RUNS)):
        assert params(fn) == table, fn.__name__


# ---- the scenes are what they claim -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.TRI_NAMES)
def test_multiview_scene_wide_geometry(name):
    kw = BC.tri_case(name)[1]
    V, n = 5, 400
    K, uv, Rt, X, sw = synth.multiview_scene_wide(n, V, seed=3, **{**kw, "noise_px": 0.0, "blank_frac": 0.0, "swap_every": 0})
    assert len(uv) == len(Rt) == V and all(u.shape == (n, 2) and u.dtype == np.float32 for u in uv) and X.shape == (n, 3)
    assert (Rt[0] is None) == bool(kw.get("first_identity")) and all(r is not None for r in Rt[1:])
    W = kw["width"]
    assert K[0] == kw["focal"] and abs(K[2] - W * (0.5 + kw.get("pp_offset", (0, 0))[0])) < 1e-9
    cen, zs = [], []
    for v in range(V):
        Rm, t = BC._pose(Rt[v])
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-14
        p, z = T.project(K, Rt[v], X)
        assert (z > 0).all()
        # noise-free pixels of the float64 points, f32 rounding of a pixel and fp64 cancellation at |X| = offset only
        assert np.abs(p - uv[v]).max() < 1e-3 * W / 1000 + 1e-9 * kw.get("offset", 0.0) * K[0], (name, v)
        cen.append(-Rm.T @ t)
        zs.append(z)
    cen = np.array(cen)
    if kw.get("offset"):
        assert abs(np.linalg.norm(X.mean(0)) / kw["offset"] - 1) < 0.05 and abs(np.linalg.norm(_t(Rt[1])) / kw["offset"] - 1) < 0.05
    lo, hi = kw.get("depth", (4.0, 12.0))
    assert zs[0].min() >= lo * (1 - 1e-9) and zs[0].max() <= hi * (1 + 1e-9) and zs[0].max() / zs[0].min() > 0.5 * hi / lo
    spread = np.linalg.norm(cen - cen[0], axis=1).max()
    assert 0.5 * kw.get("baseline", 0.25) * lo <= spread <= 1.2 * kw.get("baseline", 0.25) * lo
    Rl = BC._pose(Rt[-1])[0] @ BC._pose(Rt[0])[0].T
    assert abs(np.arccos(np.clip((np.trace(Rl) - 1) / 2, -1, 1)) - kw.get("angle", 0.1)) < 1e-6
    if kw.get("world_rot"):
        assert np.arccos(np.clip((np.trace(BC._pose(Rt[0])[0]) - 1) / 2, -1, 1)) > 0.05      # no pose near the identity
    if kw.get("forward"):
        d = BC._pose(Rt[0])[0] @ (cen[-1] - cen[0])
        assert d[2] > 0.99 * np.linalg.norm(d)
        e = T.project(K, Rt[0], cen[-1:])[0][0]
        assert 0 < e[0] < W and 0 < e[1] < kw["height"]                                       # the epipole lies in the image
    a, b = synth.multiview_scene_wide(40, 3, seed=5, **kw), synth.multiview_scene_wide(40, 3, seed=5, **kw)
    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a[1], b[1])) and np.array_equal(a[3], b[3])
    if kw.get("swap_every"):
        full = synth.multiview_scene_wide(n, V, seed=3, **kw)
        assert full[4].sum() == -(-n // kw["swap_every"]) and np.isnan(full[1][2]).any(1).mean() > 0.03


def _t(r):
    return np.asarray(r[9:])


@pytest.mark.parametrize("name,model", BC.ALIGN_RUNS)
def test_align3d_scene_wide_geometry(name, model):
    kw = BC.align_case(name)[1]
    n = 500
    x1, x2, s, Rg, tg, inl = synth.align3d_scene_wide(n, seed=2, model=model, **{**kw, "noise": 0.0})
    assert x1.shape == x2.shape == (n, 3) and x1.dtype == x2.dtype == np.float32
    assert np.abs(Rg @ Rg.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rg) - 1) < 1e-14
    assert s == (kw.get("scale", s) if model == AR.SIMILARITY else 1.0)
    fin = np.isfinite(x1).all(1) & np.isfinite(x2).all(1)
    assert inl.sum() == n - max(int(round(kw.get("outlier_frac", 0.3) * n)), int(round(kw.get("nan_frac", 0.0) * n)))
    assert (~fin).sum() == int(round(kw.get("nan_frac", 0.0) * n)) and not inl[~fin].any()
    a, b = x1[inl].astype(np.float64), x2[inl].astype(np.float64)
    mag = max(np.abs(a).max() * s, np.abs(b).max())
    assert np.abs(s * a @ Rg.T + tg - b).max() <= 4 * BC.U24 * mag * 3                        # f32 rounding of both frames only
    if kw.get("angle") is not None:
        assert abs(np.arccos(np.clip((np.trace(Rg) - 1) / 2, -1, 1)) - kw["angle"]) < 2e-8
    if kw.get("offset"):
        assert abs(np.linalg.norm(a.mean(0)) / kw["offset"] - 1) < 0.01
    span = kw.get("span", 8.0)
    Sv = np.linalg.svd(a - a.mean(0), compute_uv=False) / np.sqrt(len(a))
    assert 0.15 * span < Sv[0] < 0.6 * span
    if "flat" in kw:
        assert (Sv[2] == 0.0 or Sv[2] / Sv[0] < 1e-7) if kw["flat"] == 0 else 0.2 * kw["flat"] < Sv[2] / Sv[0] < 2 * kw["flat"]
        assert Sv[1] / Sv[0] > 0.3
    if "line" in kw:
        assert (Sv[1] / Sv[0] < 1e-7) if kw["line"] == 0 else 0.2 * kw["line"] < Sv[1] / Sv[0] < 2 * kw["line"]
    if kw.get("flat") == 0:
        # EXACTLY coplanar in float32: some plane through three of the rows holds every inlier with a zero triple product
        p0, p1 = a[0], a[np.argmax(np.linalg.norm(a - a[0], axis=1))]
        p2 = a[np.argmax(np.linalg.norm(np.cross(a - p0, p1 - p0), axis=1))]
        assert (np.cross(p1 - p0, p2 - p0) @ (a - p0).T == 0).all()
    if kw.get("line") == 0:
        p1 = a[np.argmax(np.linalg.norm(a - a[0], axis=1))]
        assert (np.cross(a - a[0], p1 - a[0]) == 0).all()                                     # EXACTLY collinear
    again = synth.align3d_scene_wide(n, seed=2, model=model, **{**kw, "noise": 0.0})
    assert np.array_equal(x1, again[0], equal_nan=True) and np.array_equal(x2, again[1], equal_nan=True)


# ---- triangulation ---------------------------------------------------------------------------------------------------------
def tri_run(name, V, initial=False):
    K, uv, Rt, _, _, _ = BC.tri_scene(name, V)
    g = BC.tri_gates(name)
    if initial:
        return T.run(K, uv, Rt, g[0], g[1], g[2], 100, flags=T.USE_INITIAL, xyz0=BC.tri_start(name, V))
    return T.run(K, uv, Rt, g[0], g[1], g[2], 100)


@pytest.mark.parametrize("name,V", TRI_RUNS)
def test_restated_triangulation_matches_numpy(name, V):
    note(BC.tri_checks(name, V, tri_run(name, V)), ("tri", name, V))


@pytest.mark.parametrize("name,V", TRI_RUNS)
def test_restated_triangulation_from_a_perturbed_map_reaches_the_same_minimum(name, V):
    r = tri_run(name, V, initial=True)
    assert not r.points4.any()
    note(BC.tri_checks(name, V, r, initial=True), ("tri initial", name, V))
    if name == "nonfinite":
        x0 = BC.tri_start(name, V)
        bad = ~np.isfinite(x0).all(1) & (r.status != T.FEW_VIEWS)
        assert bad.sum() >= 5 and (r.status[bad] == T.DEGENERATE).all()


# ---- 3-D alignment ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model", BC.ALIGN_RUNS)
def test_restated_refit_matches_kabsch_umeyama(name, model):
    x1, x2, s, Rg, tg, inl = BC.align_scene(name, model)
    start = BC.align_start(name, model)
    worst = {}
    for mask in (inl.astype(np.uint8), np.asarray(AR.score(AR.pack(s, Rg, tg), x1, x2, BC.align_case(name)[2])[0])):
        Tn, info = AR.refine(model, x1, x2, mask, start)
        m = BC.check_align_refit(name, model, mask, start, Tn, info)
        assert m.pop("checked") == (name in BC.ALIGN_DETERMINED), (name, model, m)
        for k, v in m.items():
            worst[k] = max(worst.get(k, 0.0), v) if k != "gap" else min(worst.get(k, 1.0), v)
    gap = worst.pop("gap")
    note({"ALIGN_COST_TOL": worst["cost"], "ALIGN_INFO_TOL": worst["info"], "ALIGN_ROT_TOL": worst["rot"],
          "ALIGN_FIT_TOL": worst["fit"]}, ("align", name, model, "gap %.3g" % gap))


@pytest.mark.parametrize("name,model", BC.ALIGN_RUNS)
def test_restated_run_finds_the_planted_transform(name, model):
    x1, x2, s, Rg, tg, inl = BC.align_scene(name, model)
    thresh = BC.align_case(name)[2]
    key, Tw, mask, c = AR.run(model, x1, x2, BC.ALIGN_ITERS, thresh, 0x3D + model)
    d, nband = BC.check_align_run(name, model, key, Tw, mask, c)
    # the float64 reference alone stays within the cap: the planted model's band
    dd, err = BC.align_band(AR.pack(s, Rg, tg), x1, x2, thresh)
    fin = np.isfinite(dd) & np.isfinite(err)
    share = (fin & ~(np.abs(dd - thresh) > err)).sum() / fin.sum()
    assert share <= BC.BAND_CAP, (name, model, share)
    note({"ALIGN_RUN_TOL": d, "align band share": max(share, nband / fin.sum())}, ("align run", name, model))
    if key:
        Tn, info = AR.refine(model, x1, x2, mask, Tw)
        BC.check_align_refit(name, model, mask, Tw, Tn, info)
        BC.check_align_mask(Tn, x1, x2, thresh, AR.score(Tn, x1, x2, thresh)[0], (name, model, "refit"))


@pytest.mark.parametrize("name,model", [r for r in BC.ALIGN_RUNS if r[0] in ("far-1e4", "scale-1e-3", "scale-1e3", "nonfinite")])
def test_restated_transform_equals_numpy_after_one_rounding(name, model):
    x1, x2, s, Rg, tg, inl = BC.align_scene(name, model)
    Tg = AR.pack(s, Rg, tg)
    assert BC.check_transform(Tg, x1, AR.transform(Tg, x1), (name, model)) >= 0.85 * len(x1)


# ---- bundle adjustment -----------------------------------------------------------------------------------------------------
def ba_runs(name, V, mask):
    K, uv, Rt0, xyz0, gate = BC.ba_scene(name, V, mask)
    return [B.run(K, uv, Rt0, xyz0, mask, it, gate) for it in BC.BA_BUDGETS]


@pytest.mark.parametrize("name,V,mask", BC.BA_RUNS)
def test_restated_bundle_adjustment_matches_the_dense_solver(name, V, mask):
    m = BC.ba_checks(name, V, mask, ba_runs(name, V, mask))
    note(m, ("ba", name, V, mask))
    for it, ex in m["excess"].items():
        k = "BA excess %s @ %d" % (name if name in BC.BA_FAR else "other", it)
        if k not in WORST or ex > WORST[k][0]:
            WORST[k] = (ex, ("ba", name, V, mask))
    if name == "gated":
        K, uv, Rt0, xyz0, gate = BC.ba_scene(name, V, mask)
        assert B.run(K, uv, Rt0, xyz0, mask, 0, 0.0).n_obs > B.run(K, uv, Rt0, xyz0, mask, 0, gate).n_obs
    if name == "nonfinite":
        K, uv, Rt0, xyz0, gate = BC.ba_scene(name, V, mask)
        assert (~np.isfinite(xyz0).all(1)).sum() >= 3 and (~np.isfinite(uv[0]).all(1)).sum() >= 1


# ---- every helper bites ------------------------------------------------------------------------------------------------------
def _raises(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)
    return True


def test_triangulation_helpers_bite():
    name, V = "far-1e3", 5
    r = tri_run(name, V)
    K, uv, Rt, _, _, _ = BC.tri_scene(name, V)
    obs, _, _, cmin = BC.tri_reference(name, V)
    BC.tri_checks(name, V, r)
    i = int(np.nonzero(r.status == T.OK)[0][0])
    ray = r.xyz64[i] + BC._pose(Rt[0])[0].T @ BC._pose(Rt[0])[1]
    ray /= np.linalg.norm(ray)
    # a point moved along its ray until its fp64 cost is ten tolerances up; until its f32 cost is ten allowances up
    for target, check, field in ((10 * BC.TRI_COST_TOL * (1 + cmin[i]), BC.check_tri_refined64, "xyz64"), (None, BC.check_tri_f32, "xyz")):
        X = np.array(getattr(r, field), np.float64)
        if target is None:
            target = 10 * (BC.f32_cost_allowance(K, Rt, X, obs, cmin)[i] + BC.TRI_COST_TOL * (1 + cmin[i]))
        step = 1e-9
        while BC.tri_costs(K, uv, Rt, X, obs)[i] - cmin[i] < target:
            X[i] = getattr(r, field)[i] + step * ray
            step *= 2
        assert step < 1.0 and _raises(check, name, V, X.astype(getattr(r, field).dtype), r.status)
    # points4: the null vector moved by ten tolerances of its unit across the ray
    p4 = r.points4.copy()
    Xs = (p4[i, :3] / p4[i, 3]).astype(np.float64)
    unit = BC.tri_lin_unit(K, uv, Rt, Xs[None], obs[:, i:i + 1])[0, 0]
    z0 = T.project(K, Rt[0], Xs[None])[1][0]
    side = BC._pose(Rt[0])[0].T @ np.array([1.0, 0.0, 0.0])
    Xs = Xs + side * 20 * BC.TRI_LIN_TOL * unit * z0 / K[0]
    p4[i] = np.r_[Xs, 1.0] / np.linalg.norm(np.r_[Xs, 1.0])
    assert _raises(BC.check_tri_points4, name, V, p4, r.status)
    # a status flipped on a row far from every gate; a count off by one; err2 off by ten tolerances
    st = r.status.copy()
    st[i] = T.REPROJ
    assert _raises(BC.check_tri_status, name, V, r.xyz64, st)
    assert _raises(BC.check_tri_counts, name, V, r.xyz64, r.status, r.err2, r.n_good + 1)
    e2 = r.err2.copy()
    e2[i] *= np.float32(1 + 10 * (BC.U24 + BC.TRI_ERR_TOL) + 2 * BC.U24)
    assert _raises(BC.check_tri_counts, name, V, r.xyz64, r.status, e2, r.n_good)


@pytest.mark.parametrize("model", (AR.RIGID, AR.SIMILARITY))
def test_alignment_helpers_bite(model):
    name = "half-outliers"
    x1, x2, s, Rg, tg, inl = BC.align_scene(name, model)
    thresh = BC.align_case(name)[2]
    mask, start = inl.astype(np.uint8), BC.align_start(name, model)
    Tn, info = AR.refine(model, x1, x2, mask, start)
    m = BC.check_align_refit(name, model, mask, start, Tn, info)
    sn, Rn, tn = AR.unpack(Tn)
    a = x1[inl].astype(np.float64)
    cen = a.mean(0)
    # a rotation turned further about the centroid: by ten fit tolerances, and until the cost is ten tolerances up
    for turn in (10 * BC.ALIGN_FIT_TOL / m["gap"], np.sqrt(10 * BC.ALIGN_COST_TOL * BC.align_cost(Tn, a, x2[inl]) / (sn * sn * ((a - cen) ** 2).sum())) * 3):
        Rt = T._rot(np.array([0.0, 0.0, turn])) @ Rn
        spoilt = AR.pack(sn, Rt, tn + sn * (Rn - Rt) @ cen)
        assert _raises(BC.check_align_refit, name, model, mask, start, spoilt, info)
    # a rotation that is none: scaled by ten tolerances
    assert _raises(BC.check_align_refit, name, model, mask, start, AR.pack(sn, Rn * (1 + 10 * BC.ALIGN_ROT_TOL), tn), info)
    # info's cost scaled up by ten tolerances
    up = AR.Info([info.cost_in, info.cost_out * (1 + 10 * BC.ALIGN_INFO_TOL)], [info.n_used, 0, 0])
    assert _raises(BC.check_align_refit, name, model, mask, start, Tn, up)
    # a mask with a row flipped outside the band; a non-finite row made an inlier
    key, Tw, mw, c = AR.run(model, x1, x2, BC.ALIGN_ITERS, thresh, 0x3D + model)
    BC.check_align_run(name, model, key, Tw, mw, c)
    d, err = BC.align_band(Tw, x1, x2, thresh)
    for i in (int(np.argmin(d)), int(np.argmax(d))):
        bad = mw.copy()
        bad[i] ^= 1
        assert _raises(BC.check_align_mask, Tw, x1, x2, thresh, bad) and _raises(BC.check_align_run, name, model, key, Tw, bad, int(bad.sum()))
    # a winner ten run tolerances away
    far = AR.pack(*AR.unpack(Tw)[:2], AR.unpack(Tw)[2] + 10 * BC.ALIGN_RUN_TOL * thresh)
    assert _raises(BC.check_align_run, name, model, key, far, AR.score(far, x1, x2, thresh)[0], AR.score(far, x1, x2, thresh)[1])
    # the point transform one ulp off on one row
    out = AR.transform(Tn, x1)
    BC.check_transform(Tn, x1, out)
    out[3, 1] = np.nextafter(out[3, 1], np.float32(np.inf))
    assert _raises(BC.check_transform, Tn, x1, out)


def test_bundle_adjustment_helpers_bite():
    name, V, mask = "far-1e2", 3, 1
    runs = ba_runs(name, V, mask)
    BC.ba_checks(name, V, mask, runs)
    r = runs[-1]
    dense = BC.ba_dense(name, V, mask)[0]
    # a cost scaled up by ten tolerances: cost_in, cost_out against its own output, cost_out against the dense minimum
    assert _raises(BC.check_ba_used, name, V, mask, r.used, r.cost_in * (1 + 10 * BC.BA_COSTIN_TOL), r.n_points, r.n_obs)
    assert _raises(BC.check_ba_cost, name, V, mask, r.used, r.Rt, r.xyz64, r.xyz, r.cost_out * (1 + 10 * BC.BA_COST_TOL))
    assert _raises(BC.check_ba_minimum, name, 100, dense * (1 + 10 * max(BC.BA_MIN_TOL, 10 * BC.BA_ITER_EXCESS.get((name, 100), 0.0))) * 1.01, dense)
    u = r.used.copy()
    u[np.nonzero(u)[0][0]] ^= 1
    assert _raises(BC.check_ba_used, name, V, mask, u, r.cost_in, r.n_points, r.n_obs)
    # a rotation turned further: a pose that is no rotation, and a pose whose cost no longer is cost_out
    Rt = r.Rt.copy()
    Rt[1, :9] *= 1 + 10 * BC.BA_ROT_TOL
    assert _raises(BC.check_ba_poses, Rt)
    Rt = r.Rt.copy()
    Rm, t = BC._pose(Rt[1])
    Rn = T._rot(np.array([0.0, 1e-4, 0.0])) @ Rm
    Rt[1] = np.r_[Rn.reshape(-1), Rn @ Rm.T @ t]
    BC.check_ba_poses(Rt)
    assert _raises(BC.check_ba_cost, name, V, mask, r.used, Rt, r.xyz64, r.xyz, r.cost_out)
    # a point moved along its ray until the f32 cost is ten allowances up
    K, uv, _, _, _ = BC.ba_scene(name, V, mask)
    i = int(np.nonzero(r.used)[0][0])
    ray = r.xyz64[i] + BC._pose(r.Rt[0])[0].T @ BC._pose(r.Rt[0])[1]
    x = r.xyz.copy()
    x[i] = (r.xyz64[i] + 0.05 * ray).astype(np.float32)
    assert _raises(BC.check_ba_cost, name, V, mask, r.used, r.Rt, r.xyz64, x, r.cost_out)
    # a cost that rises with the budget
    assert _raises(BC.check_ba_monotone, r.cost_in, [runs[0].cost_out, runs[1].cost_out * 1.001, runs[2].cost_out])
    assert _raises(BC.check_ba_monotone, r.cost_out * 0.5, [x.cost_out for x in runs])


def test_worst_value_table(capsys):
    """Prints what every tolerance of backend_cases.py was measured against (a whole-file run fills it)."""
    with capsys.disabled():
        print("\n-- worst values of tests/test_backend_independent_cpu.py (%.0f s) --" % (time.time() - T0))
        for k in sorted(WORST):
            print("%-34s %.3g  %s" % (k, WORST[k][0], WORST[k][1]))
    for k, (v, case) in WORST.items():
        if k.endswith("_TOL") and hasattr(BC, k):
            assert v <= getattr(BC, k), (k, v, case)
