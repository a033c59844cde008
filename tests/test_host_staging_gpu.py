"""GPU: the host-pointer entry points called through api.lib() directly, on what the Python wrappers never pass: parts of
the staged device block that are shorter than their 256-byte padding, an empty train set, optional outputs left out and
a row stride wider than the frame.  Every result equals the _dev form's on torch buffers byte for byte, and an array that
is passed sits between sentinel bytes that must survive the call."""
import ctypes as C
import gc

import numpy as np
import pytest

from points_matching_amd import api

pytestmark = pytest.mark.gpu
NQ, NT, DIM, HAMMING_BYTES = 3, 5, 20, 36          # f32 rows of 80 bytes, u8 rows of 20, binary rows of 36
FORMS = {"l2_f32": (np.float32, DIM), "l2_u8": (np.uint8, DIM), "hamming_u8": (np.uint8, HAMMING_BYTES)}
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    import torch
    import points_matching_amd as pm
    c = pm.Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()
    gc.collect()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def dzeros(nbytes):
    import torch
    return torch.zeros(max(nbytes, 16), dtype=torch.uint8, device="cuda:0")


def dp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dbytes(t, nbytes):
    return t.cpu().numpy().tobytes()[:nbytes]


class Guarded:
    """A host array of `shape` / `dtype` between two runs of GUARD sentinel bytes."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.raw = np.full(n + 2 * GUARD, 0xA5, np.uint8)
        self.a = self.raw[GUARD:GUARD + n].view(dtype).reshape(shape)
        self.p = api._p(self.a)

    def intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all() and (self.raw[-GUARD:] == 0xA5).all())


def descriptor_rows(form, nt):
    """NQ query rows and nt train rows; with a train set, three train rows repeat the query rows (mutual neighbours)."""
    dtype, width = FORMS[form]
    r = np.random.default_rng(7)
    draw = (lambda n: r.standard_normal((n, width)).astype(np.float32)) if dtype == np.float32 else \
        (lambda n: r.integers(0, 256, (n, width), dtype=np.uint8))
    q, t = draw(NQ), draw(nt)
    if nt:
        t[[4, 0, 2]] = q
    return q, t, width


# ---- the three plain matchers ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [NT, 0])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_plain_matchers_equal_the_device_form(ctx, form, nt):
    import torch
    L, h = api.lib(), ctx._h
    q, t, width = descriptor_rows(form, nt)
    flags = (0,) if form == "l2_f32" else ()
    d_q, d_t = dev(q), dev(t) if nt else dzeros(0)
    for k in (1, 2):
        out = Guarded((NQ, k), api.MATCH_DTYPE)
        api._check(getattr(L, "pm_bf_knn_" + form)(h, api._p(q), NQ, api._p(t) if nt else None, nt, width, k, *flags, out.p))
        d_out = dzeros(out.a.nbytes)
        torch.cuda.synchronize()
        api._check(getattr(L, "pm_bf_knn_%s_dev" % form)(h, dp(d_q), NQ, dp(d_t), nt, width, k, *flags, dp(d_out)))
        ctx.synchronize()
        assert out.a.tobytes() == dbytes(d_out, out.a.nbytes) and out.intact()
        if nt:
            assert list(out.a["trainIdx"][:, 0]) == [4, 0, 2]
        else:
            assert (out.a["trainIdx"] == -1).all()


# ---- the three cross-check forms ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [NT, 0])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_cross_check_equals_the_device_form(ctx, form, nt):
    import torch
    L, h = api.lib(), ctx._h
    q, t, width = descriptor_rows(form, nt)
    knn_flags = (0,) if form == "l2_f32" else ()
    d_q, d_t = dev(q), dev(t) if nt else dzeros(0)
    for cross_flags in (0, api.PM_CROSS_RATIO_FWD | api.PM_CROSS_RATIO_REV):
        out, n = Guarded((NQ,), api.MATCH_DTYPE), Guarded((1,), np.int32)
        api._check(getattr(L, "pm_bf_match_cross_" + form)(h, api._p(q), NQ, api._p(t) if nt else None, nt, width, *knn_flags, cross_flags,
                                                           C.c_float(0.8), out.p, n.p))
        d_fwd, d_rev, d_good, d_n = dzeros(32 * NQ), dzeros(32 * nt), dzeros(16 * NQ), dzeros(4)
        torch.cuda.synchronize()
        api._check(getattr(L, "pm_bf_match_cross_%s_dev" % form)(h, dp(d_q), NQ, dp(d_t), nt, width, *knn_flags, cross_flags, C.c_float(0.8),
                                                                 None, None, dp(d_fwd), dp(d_rev), dp(d_good), None, None, dp(d_n)))
        ctx.synchronize()
        m = int(n.a[0])
        assert n.a.tobytes() == dbytes(d_n, 4) and m == (NQ if nt else 0)
        assert out.a[:m].tobytes() == dbytes(d_good, 16 * m)
        assert out.intact() and n.intact() and (out.raw[GUARD + 16 * m:] == 0xA5).all()     # nothing behind the survivors


# ---- guided k-NN, three forms -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [NT, 0])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_guided_knn_equals_the_device_form(ctx, form, nt):
    import torch
    L, h = api.lib(), ctx._h
    q, t, width = descriptor_rows(form, nt)
    r = np.random.default_rng(3)
    kp1, kp2 = r.uniform(0, 100, (NQ, 2)).astype(np.float32), r.uniform(0, 100, (nt, 2)).astype(np.float32)
    M = np.eye(3).reshape(9)                            # PM_GUIDE_H = 2 with the identity: admits train keypoints within tau of kp1
    d_q, d_t, d_kp1, d_kp2, d_M = dev(q), dev(t) if nt else dzeros(0), dev(kp1), dev(kp2) if nt else dzeros(0), dev(M)
    admitted = 0
    for k in (1, 3):
        d_out, d_adm = dzeros(16 * NQ * k), dzeros(4 * NQ)
        torch.cuda.synchronize()
        api._check(getattr(L, "pm_bf_knn_guided_%s_dev" % form)(h, dp(d_q), NQ, dp(d_t), nt, width, dp(d_kp1), dp(d_kp2), 2, dp(d_M),
                                                                C.c_float(60.0), k, dp(d_out), dp(d_adm)))
        ctx.synchronize()
        for with_adm in (True, False):
            out, adm = Guarded((NQ, k), api.MATCH_DTYPE), Guarded((NQ,), np.int32)
            api._check(getattr(L, "pm_bf_knn_guided_" + form)(h, api._p(q), NQ, api._p(t) if nt else None, nt, width, api._p(kp1),
                                                              api._p(kp2) if nt else None, 2, api._p(M), C.c_float(60.0), k, out.p,
                                                              adm.p if with_adm else None))
            assert out.a.tobytes() == dbytes(d_out, 16 * NQ * k) and out.intact()
            if with_adm:
                assert adm.a.tobytes() == dbytes(d_adm, 4 * NQ) and adm.intact()
                admitted += int(adm.a.sum())
            else:
                assert (adm.raw == 0xA5).all()
    assert (admitted > 0) == (nt > 0)


# ---- tracking -----------------------------------------------------------------------------------------------------------------

def smooth_frame(w, h, stride, seed, shift=0.0):
    """A band-limited pattern moved by `shift` pixels, in rows of `stride` bytes whose padding holds other values."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    im = np.zeros((h, w))
    for _ in range(12):
        fx, fy, ph = r.uniform(0.05, 0.45), r.uniform(0.05, 0.45), r.uniform(0, 6.28)
        im += np.sin(fx * (x - shift) + fy * (y - 0.5 * shift) + ph)
    buf = np.random.default_rng(seed + 100).integers(0, 256, (h, stride), dtype=np.uint8)
    buf[:, :w] = np.clip(np.rint(128 + 20 * im), 0, 255).astype(np.uint8)
    return buf


@pytest.mark.parametrize("use_init", [False, True])
def test_track_lk_strided_frames_and_optional_outputs(ctx, use_init):
    import torch
    L, h = api.lib(), ctx._h
    W, H, STRIDE, N = 64, 48, 67, 5
    img1, img2 = smooth_frame(W, H, STRIDE, 1), smooth_frame(W, H, STRIDE, 1, shift=1.25)
    pts = np.array([[32, 24], [20.5, 17.25], [45.75, 30.5], [3, 3], [60, 44]], np.float32)
    init = pts + np.float32(1.0) if use_init else None
    prm = api.lk_params(win_radius=5, max_level=1, fb_thresh=0.5, flags=api.PM_LK_USE_INITIAL if use_init else 0)
    d1, d2, d_pts, d_init = dev(img1), dev(img2), dev(pts), dev(init) if use_init else None
    d_out, d_st, d_err, d_fb = dzeros(8 * N), dzeros(N), dzeros(4 * N), dzeros(4 * N)
    torch.cuda.synchronize()
    pa, pb = ctx.pyramid(W, H, 1).build_dev(d1.data_ptr(), STRIDE), ctx.pyramid(W, H, 1).build_dev(d2.data_ptr(), STRIDE)
    try:
        api._check(L.pm_track_lk_dev(h, pa._h, pb._h, dp(d_pts), None, N, dp(d_init), C.byref(prm), dp(d_out), dp(d_st), dp(d_err), dp(d_fb)))
        ctx.synchronize()
    finally:
        pa.close()
        pb.close()
    want = [dbytes(d_out, 8 * N), dbytes(d_st, N), dbytes(d_err, 4 * N), dbytes(d_fb, 4 * N)]
    assert np.frombuffer(want[1], np.uint8).any()       # something is tracked
    for with_err in (True, False):
        for with_fb in (True, False):
            out, st, err, fb = Guarded((N, 2), np.float32), Guarded((N,), np.uint8), Guarded((N,), np.float32), Guarded((N,), np.float32)
            api._check(L.pm_track_lk(h, api._p(img1), api._p(img2), W, H, STRIDE, api._p(pts), N, api._p(init), C.byref(prm), out.p, st.p,
                                     err.p if with_err else None, fb.p if with_fb else None))
            assert [out.a.tobytes(), st.a.tobytes()] == want[:2] and out.intact() and st.intact()
            assert err.a.tobytes() == want[2] and err.intact() if with_err else (err.raw == 0xA5).all()
            assert fb.a.tobytes() == want[3] and fb.intact() if with_fb else (fb.raw == 0xA5).all()


# ---- feature front end --------------------------------------------------------------------------------------------------------

def blob_frame(w, h, stride):
    r = np.random.default_rng(11)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    im = np.full((h, w), 0.5)
    for _ in range(w * h // 60):
        cx, cy, s = r.uniform(0, w), r.uniform(0, h), r.uniform(1.2, 3.5)
        im += r.choice([-1, 1]) * r.uniform(0.2, 0.45) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    buf = r.integers(0, 256, (h, stride), dtype=np.uint8)
    buf[:, :w] = np.clip(np.rint(255 * im), 0, 255).astype(np.uint8)
    return buf


@pytest.mark.parametrize("bits", [False, True])
def test_detect_describe_strided_frame_and_optional_outputs(ctx, bits):
    import torch
    L, h = api.lib(), ctx._h
    W, H, STRIDE, MAX_KP = 96, 80, 100, 128
    img = blob_frame(W, H, STRIDE)
    row_u8 = 32 if bits else 128
    d_img, d_kp, d_u8, d_f32, d_meta, d_n = dev(img), dzeros(8 * MAX_KP), dzeros(row_u8 * MAX_KP), dzeros(512 * MAX_KP), dzeros(16 * MAX_KP), dzeros(4)
    torch.cuda.synchronize()
    if bits:
        ctx.detect_describe_bits_dev(d_img.data_ptr(), W, H, STRIDE, MAX_KP, d_kp.data_ptr(), d_u8.data_ptr(), d_meta.data_ptr(), d_n.data_ptr())
    else:
        ctx.detect_describe_dev(d_img.data_ptr(), W, H, STRIDE, MAX_KP, d_kp.data_ptr(), d_u8.data_ptr(), d_f32.data_ptr(), d_meta.data_ptr(),
                                d_n.data_ptr())
    ctx.synchronize()
    m = int(np.frombuffer(dbytes(d_n, 4), np.int32)[0])
    assert 0 < m <= MAX_KP
    absent = [()] + ([("meta",)] if bits else [("f32",), ("meta",), ("u8",)])
    for skip in absent:
        kp, u8, meta = Guarded((MAX_KP, 2), np.float32), Guarded((MAX_KP, row_u8), np.uint8), Guarded((MAX_KP, 4), np.float32)
        f32, n = Guarded((MAX_KP, 128), np.float32), Guarded((1,), np.int32)
        give = lambda name, g: None if name in skip else g.p
        args = (h, api._p(img), W, H, STRIDE, MAX_KP, C.c_float(0.03), C.c_float(10.0), kp.p, give("u8", u8))
        if bits:
            api._check(L.pm_detect_describe_bits(*args, give("meta", meta), n.p))
        else:
            api._check(L.pm_detect_describe(*args, give("f32", f32), give("meta", meta), n.p))
        assert int(n.a[0]) == m and n.intact() and kp.a[:m].tobytes() == dbytes(d_kp, 8 * m) and kp.intact()
        for name, g, d, row in (("u8", u8, d_u8, row_u8), ("f32", f32, d_f32, 512), ("meta", meta, d_meta, 16)):
            if name in skip or (bits and name == "f32"):
                assert (g.raw == 0xA5).all(), name
            else:
                assert g.a[:m].tobytes() == dbytes(d, row * m) and g.intact(), name
