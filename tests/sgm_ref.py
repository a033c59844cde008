"""ctypes loader of tests/sgm_ref.c, the plain-C restatement of SPEC S89-S92 (semi-global matching: census cost, 4 or 8 paths,
S85's winner on the summed path costs), the shim over csrc/stereo_sgm_plan.hpp, and an independent numpy statement that is
organised differently: the census as 62 boolean planes, the cost as a count of unequal booleans, one generic stepping loop for
every direction (a whole line of pixels per step), the winner rules vectorised as in stereo_ref.np_bm.  The scenes, the
left-right check and the depth at points are stereo_ref's.  Built once per process through tests/cref.py."""
import ctypes as C
import os

import numpy as np

import cref
import stereo_ref as S

INVALID = S.INVALID
FROM_RIGHT = S.FROM_RIGHT
ROOT = S.ROOT
DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))          # S91's order
PENALTIES = ((0, 0), (7, 7), (4, 24), (0, 1023), (1023, 1023))

_L = None
_P = None
_V, _I = C.c_void_p, C.c_int


def lib():
    global _L
    if _L is None:
        _L = cref.load("sgm_ref", {"sg_invalid": [], "sg_sgm": [_V, _V] + [_I] * 11 + [_V, _I]})
    return _L


def plan_shim():
    global _P
    if _P is None:
        _P = cref.load("stereo_sgm_plan_shim", {"sgm_plan_shim": [_I, _I, _I, _I, _I, _V, _V], "sgm_plan_sizeof_params": []},
                       include=(os.path.join(ROOT, "points_matching_amd", "csrc"), os.path.join(ROOT, "include")))
    return _P


# ---- the C restatement ---------------------------------------------------------------------------------------------------------

def sgm(left, right, min_disp, num_disp, p1, p2, paths=8, uniqueness=0, flags=0, w=None, disp=None, dstride=None):
    """S89-S92: (disp (h, dstride) int16 with w columns written, n_valid).  left, right: (h, stride >= w) u8; with disp given
    it is written in place (the elements beyond w stay)."""
    left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
    h = left.shape[0]
    w = left.shape[1] if w is None else w
    dstride = w if dstride is None else dstride
    if disp is None:
        disp = np.zeros((h, dstride), np.int16)
    assert right.shape[0] == h and disp.shape == (h, dstride) and disp.dtype == np.int16 and disp.flags.c_contiguous
    n = lib().sg_sgm(cref.ptr(left), cref.ptr(right), w, h, left.shape[1], right.shape[1], min_disp, num_disp, p1, p2, paths, uniqueness, flags,
                     cref.ptr(disp), dstride)
    assert n >= 0, "the restatement ran out of memory"
    return disp, n


def plan(w, h, prm, lstride=None, rstride=None, dstride=None):
    """The plan header through its shim: (status, dict of fields or None).  prm: the eight ints of pm_sgm_params."""
    out = np.zeros(12 + 32, np.float64)
    p = np.asarray(prm, np.int32)
    assert p.shape == (8,)
    rc = plan_shim().sgm_plan_shim(w, h, lstride or w, rstride or w, dstride or w, cref.ptr(p), cref.ptr(out))
    if rc != S.PM_OK:
        return rc, None
    names = ("cx0", "cx1", "cy0", "cy1", "wc", "hc", "nc", "census_bytes", "s_bytes", "need", "census_grid_x", "npass")
    f = {k: int(v) for k, v in zip(names, out[:12])}
    f["passes"] = [tuple(int(v) for v in out[12 + 4 * i:16 + 4 * i]) for i in range(f["npass"])]
    return rc, f


# ---- the numpy statement -------------------------------------------------------------------------------------------------------

def computed_rect(w, h, min_disp, num_disp, flags=0):
    """S90: (x0, x1, y0, y1), inclusive; empty when x1 < x0 or y1 < y0."""
    x0, x1 = S.computed_columns(w, min_disp, num_disp, 4, flags)
    return x0, x1, 3, h - 4


def np_census(img):
    """(62, h, w) bool: plane n is I(x + i, y + j) < I(x, y) for the n-th offset; False where the window leaves the image."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    planes = np.zeros((62, h, w), bool)
    if h < 7 or w < 9:
        return planes
    n = 0
    for j in range(-3, 4):
        for i in range(-4, 5):
            if i == 0 and j == 0:
                continue
            planes[n, 3:h - 3, 4:w - 4] = img[3 + j:h - 3 + j, 4 + i:w - 4 + i] < img[3:h - 3, 4:w - 4]
            n += 1
    return planes


def np_cost_volume(left, right, min_disp, num_disp, flags=0):
    """(D, hc, wc) int64 over the computed rectangle, or None when it is empty."""
    h, w = left.shape
    x0, x1, y0, y1 = computed_rect(w, h, min_disp, num_disp, flags)
    if x1 < x0 or y1 < y0:
        return None
    base, other = (right, left) if flags & FROM_RIGHT else (left, right)
    cb, co = np_census(base)[:, y0:y1 + 1], np_census(other)[:, y0:y1 + 1]
    vol = np.zeros((num_disp, y1 - y0 + 1, x1 - x0 + 1), np.int64)
    for k in range(num_disp):
        s = (min_disp + k) if flags & FROM_RIGHT else -(min_disp + k)
        vol[k] = (cb[:, :, x0:x1 + 1] != co[:, :, x0 + s:x1 + 1 + s]).sum(0)
    return vol


def np_path(vol, dx, dy, p1, p2):
    """L_r over the whole rectangle for one direction: the volume is turned so that the path advances along axis 1 (rows for
    dy != 0, columns for dy == 0) and every step handles one whole line."""
    if dy != 0:
        V, fwd, shift = vol, dy, dx
    else:
        V, fwd, shift = vol.transpose(0, 2, 1), dx, 0
    D, n, m = V.shape
    L = np.zeros_like(V)
    lanes = np.arange(m)
    q = lanes - shift
    inside = (q >= 0) & (q < m)
    big = np.int64(1) << 40
    for t in (range(n) if fwd > 0 else range(n - 1, -1, -1)):
        c = V[:, t, :]
        tq = t - fwd
        if tq < 0 or tq >= n:
            L[:, t, :] = c
            continue
        prev = L[:, tq, np.clip(q, 0, m - 1)]                       # the predecessor's costs under each pixel of the line
        lo = prev.min(0)
        down = np.full_like(prev, big)
        up = np.full_like(prev, big)
        down[1:] = prev[:-1] + p1
        up[:-1] = prev[1:] + p1
        best = np.minimum(np.minimum(prev, lo + p2), np.minimum(down, up))
        L[:, t, :] = np.where(inside, c + best - lo, c)
    return L if dy != 0 else L.transpose(0, 2, 1)


def np_sgm(left, right, min_disp, num_disp, p1, p2, paths=8, uniqueness=0, flags=0):
    """S89-S92 in numpy: (disp (h, w) int16, n_valid)."""
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    h, w = left.shape
    out = np.full((h, w), INVALID, np.int64)
    vol = np_cost_volume(left, right, min_disp, num_disp, flags)
    if vol is None:
        return out.astype(np.int16), 0
    x0, x1, y0, y1 = computed_rect(w, h, min_disp, num_disp, flags)
    total = np.zeros_like(vol)
    for dx, dy in DIRS[:paths]:
        total += np_path(vol, dx, dy, p1, p2)
    k1 = total.argmin(0)                                           # the first minimum: the smallest d
    c1 = np.take_along_axis(total, k1[None], 0)[0]
    ks = np.arange(num_disp)[:, None, None]
    far = np.abs(ks - k1[None]) > 1
    c2 = np.where(far, total, np.int64(1) << 40).min(0)
    reject = far.any(0) & (c2 * (100 - uniqueness) < c1 * 100)
    inner = (k1 > 0) & (k1 < num_disp - 1)
    p = np.take_along_axis(total, np.clip(k1 - 1, 0, num_disp - 1)[None], 0)[0]
    n = np.take_along_axis(total, np.clip(k1 + 1, 0, num_disp - 1)[None], 0)[0]
    den = p + n - 2 * c1
    off = np.where(inner & (den != 0), (16 * (p - n) + den) // np.where(den == 0, 1, 2 * den), 0)          # floor division
    out[y0:y1 + 1, x0:x1 + 1] = np.where(reject, INVALID, 16 * (min_disp + k1) + off)
    return out.astype(np.int16), int((~reject).sum())


# ---- scenes ----------------------------------------------------------------------------------------------------------------

BAND_TRUE16 = 48                                                   # the band scene's disparity, 3 pixels


def band_scene(seed):
    """A textured pair shifted by three pixels with a constant band of 20 columns in the left image and no noise: (left, right,
    mask) with the mask on the 420 pixels whose census window lies wholly in the band."""
    left = S.texture(96, 48, seed).copy()
    left[:, 64:84] = 128
    right = np.random.default_rng(seed).integers(0, 256, (48, 96)).astype(np.uint8)
    right[:, :93] = left[:, 3:]
    mask = np.zeros((48, 96), bool)
    mask[3:45, 69:79] = True
    return left, right, mask


def off_by_more_than_half(disp, mask, true16):
    """The masked pixels that are invalid or further than 8 sixteenths from the truth."""
    v = np.asarray(disp, np.int64)[mask]
    return int(((v == INVALID) | (np.abs(v - true16) > 8)).sum())
