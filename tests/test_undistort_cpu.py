"""CPU: SPEC S79-S83 (the 5-coefficient lens model; points through it both ways; undistorting an image at 1/32 pixel; the map and
the remap).  The plain-C restatement tests/undistort_ref.c against an independent numpy statement bit for bit, the exact cases,
an independent Newton inverse with a derived bound, round trips, the unusable positions, extreme map values, a derived accuracy
bound against fp64 bilinear resampling, and the ABI surface."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import undistort_ref as U
import warp_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"pm_undistort_points_dev": 11, "pm_undistort_points": 10, "pm_distort_points_dev": 9, "pm_distort_points": 8,
         "pm_undistort_dev": 16, "pm_undistort": 16, "pm_undistort_map_dev": 8, "pm_remap_dev": 13, "pm_remap": 13}
MODELS = [(lens, R, K_new) for lens in (U.LENS, None) for R in (None, U.ROT) for K_new in (None, U.CAM_NEW)]
ULP = 2.0 ** -17          # one fp32 ulp of a coordinate in [64, 128), the largest the frames here have


def both(src, lens, R=None, K_new=None, flags=0, border=0, dw=None, dh=None, K=U.CAM):
    """C (fused), C (map + remap) and numpy agree on every byte; returns C's (dst, valid, n_valid)."""
    c = U.undistort(src, K, lens, R, K_new, flags, border, dw, dh)
    n = U.np_undistort(src, K, lens, R, K_new, flags, border, dw, dh)
    dh, dw = c[1].shape
    m = U.make_map(K, lens, R, K_new, dw, dh)
    r = U.remap(src, m, flags, border)
    assert (m == U.np_map(K, lens, R, K_new, dw, dh)).all()
    for other in (n, r, U.np_remap(src, m, flags, border)):
        assert (c[0] == other[0]).all() and (c[1] == other[1]).all() and c[2] == other[2], (lens, R, K_new, flags)
    assert c[2] == int(c[1].sum())
    return c


# ---- 1. C equals numpy -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(MODELS)))
def test_c_equals_numpy_on_images_and_maps(k):
    lens, R, K_new = MODELS[k]
    src = U.random_source()
    for flags in (0, U.REPLICATE):
        for dw, dh in ((None, None), (90, 50)):
            dst, valid, n_valid = both(src, lens, R, K_new, flags, 77, dw, dh)
            assert 0 < n_valid <= valid.size
    if lens is not None or R is not None or K_new is not None:
        assert both(src, lens, R, K_new, 0, 77, 90, 50)[2] < 90 * 50          # the border is in play


@pytest.mark.parametrize("k", range(len(MODELS)))
def test_c_equals_numpy_on_points(k):
    lens, R, K_new = MODELS[k]
    pts = U.seeded_points(257)
    for iters, tol in ((U.ITERS, U.TOL_PX), (1, 1e-3), (50, 1e-9), (3, 0.5)):
        a = U.undistort_points(U.CAM, lens, R, K_new, pts, iters, tol)
        assert U.same_floats(a, U.np_undistort_points(U.CAM, lens, R, K_new, pts, iters, tol)), (iters, tol)
    d = U.distort_points(U.CAM, lens, R, K_new, pts)
    assert U.same_floats(d, U.np_distort_points(U.CAM, lens, R, K_new, pts))
    assert np.isnan(d[[7, 20, 33]]).all() and np.isfinite(d[0]).all()


def test_forward_model_is_the_formula_of_s79():
    k1, k2, p1, p2, k3 = lens = (-0.2, 0.05, 2e-3, -1e-3, 0.01)
    fx, fy, cx, cy = K = (500.0, 510.0, 320.5, 240.25)
    for x, y in ((0.0, 0.0), (0.3, -0.2), (-0.7, 0.45), (1e-9, 2.0)):
        r2 = x * x + y * y
        rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * rad + (2 * p1 * x * y + p2 * (r2 + 2 * (x * x)))
        yd = y * rad + (p1 * (r2 + 2 * (y * y)) + 2 * p2 * x * y)
        assert U.forward(K, lens, x, y) == (fx * xd + cx, fy * yd + cy, rad)
    assert U.forward(K, None, 0.25, -0.5) == (fx * 0.25 + cx, fy * -0.5 + cy, 1.0)


# ---- 2. the exact cases ----------------------------------------------------------------------------------------------------

def test_zero_lens_is_the_identity_on_the_image():
    src = U.random_source()
    for lens in (None, (0.0,) * 5, (-0.0, 0.0, 0.0, -0.0, 0.0)):
        for flags in (0, U.REPLICATE):
            dst, valid, n_valid = both(src, lens, None, None, flags, 9)
            assert (dst == src).all() and valid.all() and n_valid == src.size


def test_zero_lens_returns_the_input_bits_of_exact_points():
    """fx, fy, cx, cy powers of two and integer pixels: (u - cx) * ifx * fx + cx is exact."""
    K = (64.0, 32.0, 32.0, 16.0)
    ys, xs = np.mgrid[-4:40, -4:70]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    for lens in (None, (0.0,) * 5):
        assert U.same_floats(U.undistort_points(K, lens, None, None, pts), pts)
        assert U.same_floats(U.distort_points(K, lens, None, None, pts), pts)
        assert U.same_floats(U.undistort_points(K, lens, None, None, pts, 1, 1e-12), pts)


def forward_jacobian(lens, x, y):
    """The analytic Jacobian of S79 on normalised coordinates: arrays (..., 2, 2)."""
    k1, k2, p1, p2, k3 = lens
    r2 = x * x + y * y
    rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    drad = k1 + 2 * k2 * r2 + 3 * k3 * r2 * r2          # d rad / d r2
    J = np.empty(x.shape + (2, 2))
    J[..., 0, 0] = rad + 2 * x * x * drad + 2 * p1 * y + 6 * p2 * x
    J[..., 0, 1] = 2 * x * y * drad + 2 * p1 * x + 2 * p2 * y
    J[..., 1, 0] = 2 * x * y * drad + 2 * p1 * x + 2 * p2 * y
    J[..., 1, 1] = rad + 2 * y * y * drad + 6 * p1 * y + 2 * p2 * x
    return J


def newton_inverse(lens, x0, y0):
    """Solves S79(x, y) = (x0, y0) on normalised coordinates by Newton with the analytic Jacobian, to 1e-13."""
    x, y = x0.copy(), y0.copy()
    for _ in range(60):
        xd, yd, _ = U.np_forward_norm(lens, x, y)
        J = forward_jacobian(lens, x, y)
        step = np.linalg.solve(J, np.stack([xd - x0, yd - y0], -1)[..., None])[..., 0]
        x, y = x - step[..., 0], y - step[..., 1]
        if np.abs(step).max() < 1e-15:
            break
    xd, yd, _ = U.np_forward_norm(lens, x, y)
    assert max(np.abs(xd - x0).max(), np.abs(yd - y0).max()) < 1e-13
    return x, y


def test_undistort_points_against_an_independent_newton_inverse():
    """Every pixel of the 67 x 35 frame under the moderate lens.  S81 accepts (x, y) only when its re-distorted pixel g(x, y)
    lies within tol_px of the input p = g(x*, y*), x* being the true inverse.  g(x) - g(x*) = J (x - x*) with J the Jacobian of
    g (in pixels: diag(fx, fy) J_n diag(1 / fx, 1 / fy), J_n the analytic Jacobian of S79) somewhere on the segment, so
    |x - x*| <= tol_px / smin(J).  smin is taken over the grid of true inverses; the second derivatives of S79 are below 2 per
    normalised unit here and the segment is shorter than 1e-4 normalised units, so J on the segment differs from J on the grid
    by less than 2e-4, under 1 % of smin: the bound uses 0.99 smin.  Newton's own error is 1e-13 * fx < 1e-11 px.  The output
    is rounded to fp32 once: one ulp of a coordinate below 128 covers it.  The inputs are integers, exact in fp32.
        bound = tol_px / (0.99 smin) + 1e-11 + 2^-17   (pixels, per coordinate)"""
    fx, fy, cx, cy = U.CAM
    ys, xs = np.mgrid[0:U.SH, 0:U.SW].astype(np.float64)
    x0, y0 = (xs - cx) / fx, (ys - cy) / fy
    xt, yt = newton_inverse(U.MODERATE, x0, y0)
    S = np.array([[fx, 0.0], [0.0, fy]])
    J = S @ forward_jacobian(U.MODERATE, xt, yt) @ np.linalg.inv(S)
    smin = float(np.linalg.svd(J, compute_uv=False).min())
    assert 0.5 < smin <= 1.0
    bound = U.TOL_PX / (0.99 * smin) + 1e-11 + ULP
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    got = U.undistort_points(U.CAM, U.MODERATE, None, None, pts, U.ITERS, U.TOL_PX).astype(np.float64)
    assert np.isfinite(got).all()                                        # the restatement rejects no point of this grid
    want = np.stack([fx * xt.ravel() + cx, fy * yt.ravel() + cy], 1)
    worst = float(np.abs(got - want).max())
    print("smin %.4f, bound %.3e px, worst difference %.3e px, largest displacement %.2f px" %
          (smin, bound, worst, np.abs(want - pts).max()))
    assert worst <= bound
    assert np.abs(want - pts).max() > 2.0                                # the lens moves the corners by more than two pixels


def test_points_far_outside_and_non_finite_rows_are_nan():
    pts = U.seeded_points(257)
    for lens, R, K_new in MODELS:
        out = U.undistort_points(U.CAM, lens, R, K_new, pts)
        assert np.isnan(out[[7, 20, 33]]).all()
        if lens is not None:
            assert np.isnan(out[41]).all()                               # (5000, -4000): the fixed point iteration diverges
    # rad <= 0 on the way forward: k1 = -2 and r2 > 0.5
    strong = (-2.0, 0.0, 0.0, 0.0, 0.0)
    d = U.distort_points(U.CAM, strong, None, None, np.array([[33 + 60.0, 17.0], [33 + 30.0, 17.0]], np.float32))
    assert np.isnan(d[0]).all() and np.isfinite(d[1]).all()
    # iterations that have not converged are rejected by the gate, not returned
    one = U.undistort_points(U.CAM, U.MODERATE, None, None, np.array([[0.0, 0.0], [33.0, 17.0]], np.float32), 1, 1e-3)
    assert np.isnan(one[0]).all() and (one[1] == (33.0, 17.0)).all()
    # Z <= 0 after R on the way back
    quarter = U.rotation(0.0, 100.0, 0.0)
    back = U.undistort_points(U.CAM, None, quarter, None, np.array([[60.0, 17.0], [3.0, 17.0]], np.float32))
    assert np.isnan(back).all(axis=1).tolist() == [(quarter @ [0.45, 0, 1])[2] <= 0, (quarter @ [-0.5, 0, 1])[2] <= 0]
    assert np.isnan(back).all(axis=1).any()


def numeric_jacobian_smin_smax(K, lens, R, K_new, u, v, h=1e-4):
    """Singular values of the Jacobian of S80 (ideal pixel -> distorted pixel) by central differences in fp64: (min, max)."""
    _, ax, ay = U.np_source(K, lens, R, K_new, u + h, v)
    _, bx, by = U.np_source(K, lens, R, K_new, u - h, v)
    _, cx, cy = U.np_source(K, lens, R, K_new, u, v + h)
    _, dx, dy = U.np_source(K, lens, R, K_new, u, v - h)
    J = np.stack([np.stack([ax - bx, cx - dx], -1), np.stack([ay - by, cy - dy], -1)], -2) / (2 * h)
    s = np.linalg.svd(J, compute_uv=False)
    return float(s.min()), float(s.max())


@pytest.mark.parametrize("K_new", [None, U.CAM_NEW])
def test_round_trip_distort_of_undistort(K_new):
    """p -> q = undistort_points(p) -> distort_points(q).  The gate keeps q64 only when |g(q64) - p| <= tol_px.  q is q64
    rounded to fp32 (half an ulp per coordinate, sqrt(2) / 2 ulp in length), which g stretches by at most smax(J_g); the result
    is rounded to fp32 once more (half an ulp):  |distort(q) - p| <= tol_px + smax * sqrt(2) / 2 * ulp + ulp / 2 per coordinate,
    ulp = 2^-17 (all coordinates are below 128).  smax is computed over the points by central differences, taken 1 % up."""
    pts = U.seeded_points(257)
    q = U.undistort_points(U.CAM, U.MODERATE, None, K_new, pts)
    ok = np.isfinite(q).all(axis=1)
    assert ok.sum() == 257 - 4 and np.abs(q[ok]).max() < 128 and np.abs(pts[ok]).max() < 128
    _, smax = numeric_jacobian_smin_smax(U.CAM, U.MODERATE, None, K_new, q[ok, 0].astype(np.float64), q[ok, 1].astype(np.float64))
    bound = U.TOL_PX + 1.01 * smax * np.sqrt(0.5) * ULP + ULP / 2
    back = U.distort_points(U.CAM, U.MODERATE, None, K_new, q)
    assert np.isnan(back[~ok]).all()
    worst = float(np.abs(back[ok].astype(np.float64) - pts[ok]).max())
    print("smax %.4f, bound %.3e px, worst %.3e px" % (smax, bound, worst))
    assert worst <= bound


def test_the_two_directions_of_r_are_consistent():
    """For every output pixel P of the rectified frame, undistort_points of S82's unrounded source position s = G(P) returns P.
    As in the Newton test: the gate bounds the error of the normalised solution through the lens; here the whole map
    G (K_new^-1, R^T, lens, K) takes the place of g, its Jacobian comes from central differences (relative error ~1e-8) and the
    input s is rounded to fp32 first (sqrt(2) / 2 ulp in length), which adds to tol_px before the division:
        bound = (tol_px + sqrt(2) / 2 * 2^-17) / (0.99 smin(J_G)) + 2^-17   (pixels, per coordinate)
    R applied after the gate and R^T applied in G are inverses up to the orthonormality error of R, below 1e-15."""
    R = U.ROT
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15
    ys, xs = np.mgrid[0:U.SH, 0:U.SW].astype(np.float64)
    ok, sx, sy = U.np_source(U.CAM, U.MODERATE, R, None, xs, ys)
    cok, csx, csy = U.source_positions(U.CAM, U.MODERATE, R, None, U.SW, U.SH)
    assert ok.all() and cok.all() and (csx == sx).all() and (csy == sy).all()
    smin, _ = numeric_jacobian_smin_smax(U.CAM, U.MODERATE, R, None, xs, ys)
    bound = (U.TOL_PX + np.sqrt(0.5) * ULP) / (0.99 * smin) + ULP
    s32 = np.stack([sx.ravel(), sy.ravel()], 1).astype(np.float32)
    assert np.abs(s32).max() < 128
    back = U.undistort_points(U.CAM, U.MODERATE, R, None, s32).astype(np.float64)
    assert np.isfinite(back).all()
    worst = float(np.abs(back - np.stack([xs.ravel(), ys.ravel()], 1)).max())
    print("smin %.4f, bound %.3e px, worst %.3e px" % (smin, bound, worst))
    assert worst <= bound


# ---- 3. map and remap ------------------------------------------------------------------------------------------------------

def test_map_marks_exactly_the_unusable_positions():
    wide = (30.0, 30.0, 33.0, 17.0)
    cases = {"rad <= 0": ((-2.0, 0.0, 0.0, 0.0, 0.0), None, wide),
             "Z <= 0": (U.LENS, U.rotation(0.0, 80.0, 0.0), wide),
             "far away": (None, None, (1e-9, 1e-9, 33.0, 17.0))}
    for name, (lens, R, K_new) in cases.items():
        m = U.make_map(U.CAM, lens, R, K_new, U.SW, U.SH)
        assert (m == U.np_map(U.CAM, lens, R, K_new, U.SW, U.SH)).all(), name
        ys, xs = np.mgrid[0:U.SH, 0:U.SW].astype(np.float64)
        ok, sx, sy = U.np_source(U.CAM, lens, R, K_new, xs, ys)
        with np.errstate(all="ignore"):
            ok = ok & (np.abs(sx * 32.0) < 2.0 ** 30) & (np.abs(sy * 32.0) < 2.0 ** 30)
        marked = (m[..., 0] == U.INT32_MIN) & (m[..., 1] == U.INT32_MIN)
        assert (marked == ~ok).all() and 0 < marked.sum() < marked.size, (name, int(marked.sum()))
        assert not ((m == U.INT32_MIN).any(axis=2) & ~marked).any()
        src = U.random_source()
        dst, valid, n_valid = both(src, lens, R, K_new, 0, 123)
        assert (dst[marked] == 123).all() and not valid[marked].any()
        rep = both(src, lens, R, K_new, U.REPLICATE, 123)
        assert (rep[0][marked] == 123).all() and (rep[1] == valid).all()          # the border value, not a clamped pixel
    k1, R, K_new = cases["rad <= 0"]
    assert U.position(U.CAM, k1, None, wide, 33, 17) == (1, 33 * 32, 17 * 32) and U.position(U.CAM, k1, None, wide, 66, 17)[0] == 0


def test_remap_of_extreme_map_values():
    """qx in {INT32_MAX, INT32_MAX - 31, -1, -32, -33}: the border value or the replicated edge, never valid, no overflow."""
    src = U.random_source()
    m = U.extreme_map()
    for flags in (0, U.REPLICATE):
        dst, valid, n_valid = U.remap(src, m, flags, 200)
        n = U.np_remap(src, m, flags, 200)
        assert (dst == n[0]).all() and (valid == n[1]).all() and n_valid == n[2]
        assert not valid[:, :5].any() and not valid[1:].any()
        assert valid[0, 5] == 0 and dst[0, 5] == (src[0, 2] if flags else 200)          # (64, INT32_MIN): sampled, far above
        assert dst[1, 5] == (src[2, 0] if flags else 200)                                # (INT32_MIN, 64): sampled, far left
        assert dst[2, 5] == 200                                                          # the pair: the border value in both modes
        a = src[2].astype(np.int32)
        if flags:
            assert (dst[0, :5] == [a[-1], a[-1], a[0], a[0], a[0]]).all()
            assert (dst[1, :5] == [src[-1, -1], src[-1, -1], src[-1, 0], src[-1, 0], src[-1, 0]]).all()
        else:
            assert dst[0, 0] == 200 and dst[0, 1] == 200 and dst[0, 3] == 200 and dst[0, 4] == 200
            assert dst[0, 2] == (32 * (1 * 200 + 31 * a[0]) + 512) >> 10                  # qx = -1: 1/32 border, 31/32 column 0
            assert (dst[1, :5] == 200).all() and (dst[2, :5] == 200).all()


# ---- 4. accuracy against fp64 bilinear -------------------------------------------------------------------------------------

def test_accuracy_against_fp64_bilinear_within_the_derived_bound():
    """As tests/test_warp_cpu.py derives it: S77 is the exact bilinear interpolant at a position within 1/64 px per axis of the
    true one; the interpolant moves by at most Dx per pixel across and Dy down; both sides round once:
    |out - ref| <= (Dx + Dy) / 64 + 1 wherever both are valid."""
    src = W.smooth_source()
    I = src.astype(np.int32)
    Dx, Dy = int(np.abs(np.diff(I, axis=1)).max()), int(np.abs(np.diff(I, axis=0)).max())
    assert (Dx, Dy) == (15, 11)
    bound = int(np.ceil((Dx + Dy) / 64.0 + 1.0))
    assert bound == 2
    h, w = src.shape
    K = (140.0, 150.0, 79.5, 60.25)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    worst = 0
    for lens, R, K_new in ((U.MODERATE, None, None), (U.MODERATE, U.ROT, None), ((0.15, -0.02, -2e-3, 1e-3, 0.004), None, (120.0, 125.0, 85.0, 57.0))):
        dst, valid, _ = U.undistort(src, K, lens, R, K_new)
        ok, sx, sy = U.np_source(K, lens, R, K_new, xs, ys)
        ref, inside = W.bilinear_fp64(src, sx, sy)
        cmp = inside & ok & (valid == 1)
        assert cmp.sum() * 2 >= src.size, cmp.mean()
        d = int(np.abs(dst.astype(np.int32) - ref.astype(np.int32))[cmp].max())
        worst = max(worst, d)
        assert d <= bound, d
    print("worst difference %d grey levels (bound %d)" % (worst, bound))


# ---- 5. surface ------------------------------------------------------------------------------------------------------------

def _call_arity(text, start):
    """The number of top-level arguments of the call whose opening parenthesis is at text[start]."""
    depth, n, i = 0, 1, start
    while True:
        c = text[i]
        if c in "([":
            depth += 1
        elif c in ")]":
            depth -= 1
            if depth == 0:
                return n
        elif c == "," and depth == 1:
            n += 1
        i += 1


def test_abi_header_declares_and_library_exports_the_undistort_names():
    from points_matching_amd import api
    hdr = open(os.path.join(ROOT, "include", "pm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    py = open(os.path.join(ROOT, "points_matching_amd", "api.py")).read()
    for name, arity in ARITY.items():
        m = re.search(r"\bint\s+%s\s*\(" % name, code)
        assert m, name
        assert _call_arity(code, m.end() - 1) == arity, name
        assert name in api.EXPORTS, name
        calls = [c for c in re.finditer(r"lib\(\)\.%s\(" % name, py)]
        assert len(calls) == 1 and _call_arity(py, calls[0].end() - 1) == arity, name
    assert re.search(r"typedef struct pm_lens \{ double k1, k2, p1, p2, k3; \} pm_lens;", code)
    assert hdr.count("pm_undistort_points*") >= 2                      # the two "no distortion" comments point here
    r = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    syms = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    assert not [n for n in ARITY if n not in syms]
    assert tuple(f[0] for f in api.Lens._fields_) == ("k1", "k2", "p1", "p2", "k3") and ctypes.sizeof(api.Lens) == 40
    d = api.lens(-0.28, 0.07, 1e-3, -5e-4)
    assert (d.k1, d.k2, d.p1, d.p2, d.k3) == (-0.28, 0.07, 1e-3, -5e-4, 0.0)
    for method in ("undistort_points_dev", "undistort_points", "distort_points_dev", "distort_points", "undistort_dev", "undistort",
                   "undistort_map_dev", "remap_dev", "remap"):
        assert callable(getattr(api.Context, method)), method
    assert U.REPLICATE == api.PM_WARP_REPLICATE
