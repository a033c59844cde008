"""CPU: SPEC S75-S78 (image warp by H or A with integer bilinear sampling at 1/32 pixel; the point transform).  The plain-C
restatement tests/warp_ref.c against an independent numpy statement bit for bit, the exact cases the spec lists, a derived
accuracy bound against fp64 bilinear resampling, and the ABI surface."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import warp_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pm_warp_dev", "pm_warp", "pm_transform_points_dev", "pm_transform_points")


def both(src, M, flags=0, border=0, dw=None, dh=None):
    """C and numpy agree on every byte; returns C's (dst, valid, status, n_valid)."""
    c = W.warp(src, M, flags, border, dw, dh)
    n = W.np_warp(src, M, flags, border, dw, dh)
    assert (c[0] == n[0]).all() and (c[1] == n[1]).all() and c[2:] == n[2:], (M, flags)
    assert c[3] == int(c[1].sum())
    return c


# ---- 1. C equals numpy -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(67, 35), (35, 67)])
def test_c_equals_numpy_on_seeded_homographies(w, h):
    src = W.random_source(w, h)
    partial = 0
    for k in range(20):
        H = W.homography(k)
        for rep in (0, W.REPLICATE):
            flags = rep | (W.INVERT if k % 2 else 0)
            dst, valid, status, n_valid = both(src, H, flags, border=77)
            assert status == 0
            partial += 0 < n_valid < w * h
    assert partial >= 20          # the border is in play


# ---- 2. the exact cases ----------------------------------------------------------------------------------------------------

def test_identity_returns_the_source():
    src = W.random_source(67, 35)
    for flags in (0, W.REPLICATE, W.INVERT):
        dst, valid, status, n_valid = both(src, np.eye(3), flags, border=9)
        assert (dst == src).all() and valid.all() and status == 0 and n_valid == src.size


def test_integer_translation_is_a_shift_with_border_fill():
    src = W.random_source(67, 35)
    dst, valid, status, _ = both(src, W.translation(5, -3), 0, border=200)          # out(x, y) = src(x + 5, y - 3)
    want, ok = np.full_like(src, 200), np.zeros_like(src)
    want[3:, :-5] = src[:-3, 5:]
    ok[3:, :-5] = 1
    assert (dst == want).all() and (valid == ok).all() and status == 0
    inv = both(src, W.translation(-5, 3), W.INVERT, border=200)                  # the inverse of the negation
    assert (inv[0] == dst).all() and (inv[1] == valid).all()


def test_half_pixel_translation_is_the_rounded_mean():
    src = W.random_source(67, 35)
    dst, valid, _, _ = both(src, W.translation(0.5, 0), 0, border=0)
    a, b = src[:, :-1].astype(np.int32), src[:, 1:].astype(np.int32)
    assert (dst[:, :-1] == (a + b + 1) >> 1).all()
    assert valid[:, :-1].all() and not valid[:, -1].any()
    assert (dst[:, -1] == (src[:, -1].astype(np.int32) + 1) >> 1).all()          # half the last column, half the border 0


def test_quarter_turn_is_exact():
    src = W.random_source(67, 35)
    dst, valid, status, _ = both(src, W.quarter_turn(35), 0, border=3, dw=35, dh=67)
    assert status == 0 and valid.all()
    assert (dst == src[::-1, :].T).all()          # out(x, y) = src(y, h_src - 1 - x)


def test_unusable_positions_and_models_give_border():
    src = W.random_source(67, 35)
    M = np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -10.0]])          # W = x - 10: zero on column 10
    dst, valid, status, _ = both(src, M, 0, border=123)
    assert status == 0 and (dst[:, 10] == 123).all() and not valid[:, 10].any()
    for bad in (np.nan, np.inf, -np.inf):
        M = np.eye(3)
        M[1, 2] = bad
        for flags in (0, W.INVERT, W.REPLICATE):
            dst, valid, status, n_valid = both(src, M, flags, border=123)
            assert status == 1 and (dst == 123).all() and not valid.any() and n_valid == 0
    for flags in (0, W.INVERT, W.REPLICATE):
        dst, valid, status, n_valid = both(src, np.zeros((3, 3)), flags, border=5)
        assert status == 2 and (dst == 5).all() and n_valid == 0
    dst, valid, status, n_valid = both(src, np.zeros((2, 3)), W.AFFINE, border=5)
    assert status == 2 and (dst == 5).all() and n_valid == 0
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    dst, valid, status, n_valid = both(src, singular, W.INVERT, border=5)
    assert status == 1 and (dst == 5).all() and n_valid == 0
    far = W.translation(3e7, 0)                                          # 32 * 3e7 < 2^30 <= 32 * 4e7
    assert both(src, far, 0, border=8)[3] == 0
    dst, valid, status, n_valid = both(src, W.translation(4e7, 0), W.REPLICATE, border=8)
    assert status == 0 and (dst == 8).all() and n_valid == 0          # outside by S76: the border value, not the last column


def test_replicate_clamps_and_keeps_the_valid_rule():
    src = W.random_source(67, 35)
    dst, valid, _, _ = both(src, W.translation(-4, 2.5), W.REPLICATE, border=255)
    plain = both(src, W.translation(-4, 2.5), 0, border=255)
    assert (valid == plain[1]).all()
    assert (dst[:, :4] == dst[:, 4:5]).all()                             # columns left of the source repeat its first
    assert (dst[valid == 1] == plain[0][valid == 1]).all()
    assert (dst[-3:, 10] == src[-1, 6]).all()


def test_affine_equals_its_lift():
    src = W.random_source(67, 35)
    for k in range(6):
        H = W.homography(k)
        A = H[:2]
        L = np.vstack([A, [0.0, 0.0, 1.0]])
        for flags in (0, W.INVERT, W.REPLICATE | W.INVERT):
            a = both(src, A, flags | W.AFFINE, border=31)
            b = both(src, L, flags, border=31)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2:] == b[2:]


def test_unit_last_row_is_the_division_free_case():
    """S76: with the last row (0, 0, 1) r is exactly 32, so fx = X * 32 has the bits of X * (32 / W)."""
    status, m = W.model(np.vstack([W.homography(3)[:2], [0, 0, 1.0]]))
    assert status == 0
    for x, y in ((0, 0), (13, 7), (66, 34), (1000, -5)):
        ok, qx, qy = W.position(m, x, y)
        X = (m[0] * x + m[1] * y) + m[2]
        Y = (m[3] * x + m[4] * y) + m[5]
        assert ok and qx == int(np.rint(X * 32.0)) and qy == int(np.rint(Y * 32.0))


def test_ties_and_negative_positions():
    m = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])
    for t, q in ((0.5 / 32, 0), (1.5 / 32, 2), (2.5 / 32, 2), (-0.5 / 32, 0), (-1.5 / 32, -2), (-1.0, -32), (-1.0 - 1.0 / 32, -33)):
        m[2] = t
        assert W.position(m, 0, 0) == (1, q, 0), t
    src = W.random_source(67, 35)
    dst, valid, _, _ = both(src, W.translation(-1.0 - 1.0 / 32, 0), 0, border=0)      # q = -33: x0 = -2, ax = 31
    assert not valid[:, :2].any() and valid[:, 2:].all()
    a = src[:, 0].astype(np.int32)
    assert (dst[:, 1] == (31 * 32 * a + 512) >> 10).all() and (dst[:, 0] == 0).all()


# ---- 3. accuracy against fp64 bilinear -------------------------------------------------------------------------------------

def test_accuracy_against_fp64_bilinear_within_the_derived_bound():
    """S77 is the exact bilinear interpolant at a position within 1/64 px per axis of the true one; the interpolant moves by at
    most Dx per pixel across and Dy down; both sides round once: |out - ref| <= (Dx + Dy) / 64 + 1 wherever both are valid."""
    src = W.smooth_source()
    I = src.astype(np.int32)
    Dx, Dy = int(np.abs(np.diff(I, axis=1)).max()), int(np.abs(np.diff(I, axis=0)).max())
    assert (Dx, Dy) == (15, 11)
    bound = int(np.ceil((Dx + Dy) / 64.0 + 1.0))          # in whole grey levels
    assert bound == 2
    h, w = src.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    worst = 0
    for k in range(20):
        H = W.homography(k)
        dst, valid, status, _ = W.warp(src, H, 0, 0)
        den = H[2, 0] * xs + H[2, 1] * ys + H[2, 2]
        sx, sy = (H[0, 0] * xs + H[0, 1] * ys + H[0, 2]) / den, (H[1, 0] * xs + H[1, 1] * ys + H[1, 2]) / den
        ref, inside = W.bilinear_fp64(src, sx, sy)
        cmp = inside & (valid == 1)
        assert status == 0 and cmp.sum() * 2 >= src.size, (k, cmp.mean())
        d = int(np.abs(dst.astype(np.int32) - ref.astype(np.int32))[cmp].max())
        worst = max(worst, d)
        assert d <= bound, (k, d)
    print("worst difference %d grey levels (bound %d); last model compared %.0f %%" % (worst, bound, 100.0 * cmp.mean()))


# ---- 4. points -------------------------------------------------------------------------------------------------------------

def test_points_c_equals_numpy_and_nan_rules():
    rng = np.random.default_rng(78)
    pts = np.concatenate([rng.uniform(-50, 700, (300, 2)),
                          [[np.nan, 1.0], [1.0, np.inf], [-np.inf, np.nan], [10.0, 4.0], [3e38, 3e38]]]).astype(np.float32)
    for k in range(8):
        H = W.homography(k)
        for flags in (0, W.INVERT):
            assert W.same_floats(W.points(H, pts, flags), W.np_points(H, pts, flags))
        for flags in (W.AFFINE, W.AFFINE | W.INVERT):
            a = W.points(H[:2], pts, flags)
            assert W.same_floats(a, W.np_points(H[:2], pts, flags))
            assert W.same_floats(a, W.points(np.vstack([H[:2], [0, 0, 1.0]]), pts, flags & W.INVERT))
    out = W.points(W.homography(0), pts)
    assert np.isnan(out[300:303]).all() and np.isfinite(out[:300]).all() and np.isfinite(out[303]).all()
    M = np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -10.0]])          # W = x - 10
    out = W.points(M, pts)
    assert W.same_floats(out, W.np_points(M, pts))
    assert np.isnan(out[303]).all() and np.isfinite(out[0]).all()
    for M, flags in ((np.zeros((3, 3)), 0), (np.zeros((2, 3)), W.AFFINE), (np.full((3, 3), np.nan), 0),
                     (np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]]), W.INVERT), (np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]]), 0)):
        out = W.points(M, pts, flags)
        assert np.isnan(out).all() and W.same_floats(out, W.np_points(M, pts, flags))
    t = W.points(W.translation(2, -7), pts[:300])
    assert (t == pts[:300] + np.array([2, -7], np.float32)).all()
    back = W.points(W.translation(2, -7), t, W.INVERT)
    assert (back == (t.astype(np.float64) - np.array([2.0, -7.0])).astype(np.float32)).all()


def test_points_agree_with_the_pixel_positions():
    """The transformed corners of the frame lie within 1/64 px of the Q5 positions S76 gives those pixels: rint moves 32 X / W by at
    most 1/2, and the point's own rounding to fp32 adds at most half an ulp of a value below 256, 2^-17."""
    w, h = 160, 120
    bound = 1.0 / 64 + 2.0 ** -17
    for k in range(20):
        H = W.homography(k)
        for flags in (0, W.INVERT):
            status, m = W.model(H, flags)
            assert status == 0
            for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
                ok, qx, qy = W.position(m, x, y)
                p = W.points(H, np.array([[x, y]], np.float32), flags)[0].astype(np.float64)
                assert ok and abs(p).max() < 256 and abs(p[0] - qx / 32.0) <= bound and abs(p[1] - qy / 32.0) <= bound


# ---- 5. surface ------------------------------------------------------------------------------------------------------------

def test_abi_header_declares_and_library_exports_the_warp_names():
    from points_matching_amd import api
    hdr = open(os.path.join(ROOT, "include", "pm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in api.EXPORTS, name
    assert "pm_warp_params;" in code and "pm_warp_info;" in code
    for macro, value in (("PM_WARP_INVERT", 1), ("PM_WARP_REPLICATE", 2), ("PM_WARP_AFFINE", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code) and getattr(api, macro) == value
    r = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    syms = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    assert not [n for n in NAMES if n not in syms]
    assert tuple(f[0] for f in api.WarpParams._fields_) == ("flags", "border_value", "reserved") and ctypes.sizeof(api.WarpParams) == 16
    assert tuple(f[0] for f in api.WarpInfo._fields_) == ("status", "n_valid") and ctypes.sizeof(api.WarpInfo) == 8
    p = api.warp_params(api.PM_WARP_INVERT | api.PM_WARP_AFFINE, 17)
    assert (p.flags, p.border_value, tuple(p.reserved)) == (5, 17, (0, 0))
    for method in ("warp_dev", "warp", "transform_points_dev", "transform_points"):
        assert callable(getattr(api.Context, method))
    assert (W.INVERT, W.REPLICATE, W.AFFINE) == (api.PM_WARP_INVERT, api.PM_WARP_REPLICATE, api.PM_WARP_AFFINE)
