"""CPU: the plain-C restatement of SPEC S67-S70 (tests/corner_ref.c) is pinned here against an independent numpy statement
(integral images for the block sums, np.lexsort for the ranking, a Python loop for the greedy selection) and against the
tracker's restatement tests/lk_ref.c, so that the GPU tests compare the kernels with something that was itself checked; plus
the ABI of the corner entry points.  Every comparison is bit for bit: S67 makes the sums exact integers and fixes the order
of the few fp64 and fp32 operations."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import corner_ref as K
import lk_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["pm_corners_dev", "pm_corners_replenish_dev", "pm_corners"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def img():
    return R.fixture()[0]


# ---- the independent statement -----------------------------------------------------------------------------------------------

def response_np(img, r):
    """e of S67 on the whole image (fp64, -inf outside V), through integral images of the three products."""
    I = img.astype(np.int64)
    h, w = I.shape
    cx, cy = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    cx[:, 1:-1] = I[:, 2:] - I[:, :-2]
    cy[1:-1, :] = I[2:, :] - I[:-2, :]
    out = np.full((h, w), -np.inf)
    if w - 2 * r - 3 < 1 or h - 2 * r - 3 < 1:
        return out
    n = 2 * r + 1

    def block(p):
        ii = np.zeros((h + 1, w + 1), np.int64)
        ii[1:, 1:] = p.cumsum(0).cumsum(1)
        return ii[n:, n:] - ii[:-n, n:] - ii[n:, :-n] + ii[:-n, :-n]          # [y - r, x - r] = the block centred at (x, y)

    A, B, C = (block(cx * cx).astype(np.float64), block(cx * cy).astype(np.float64), block(cy * cy).astype(np.float64))
    e = ((A + C) - np.sqrt((A - C) * (A - C) + 4.0 * (B * B))) / (8.0 * (n * n))
    ys, xs = slice(r + 1, h - r - 2), slice(r + 1, w - r - 2)
    out[ys, xs] = e[1:h - 2 * r - 2, 1:w - 2 * r - 2]
    return out


def candidates_np(img, r, min_eig):
    e = response_np(img, r)
    h, w = e.shape
    p = np.full((h + 2, w + 2), -np.inf)
    p[1:-1, 1:-1] = e

    def nb(dx, dy):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    ok = (e >= np.float64(np.float32(min_eig))) & (e > 0)
    for dx, dy in ((-1, -1), (0, -1), (1, -1), (-1, 0)):
        ok &= e > nb(dx, dy)
    for dx, dy in ((1, 0), (-1, 1), (0, 1), (1, 1)):
        ok &= e >= nb(dx, dy)
    pos = np.flatnonzero(ok.ravel()).astype(np.int32)
    return pos, e.ravel()[pos]


def rank_np(pos, e, quality):
    s = e.astype(np.float32)
    order = np.lexsort((pos, -s.astype(np.float64)))
    rpos, rs = pos[order], s[order]
    kept = int((~(rs < np.float32(quality) * rs[0])).sum()) if rs.size else 0
    return rpos, rs, kept


def select_np(w, rpos, rs, n, min_dist, keep, max_corners):
    md2 = np.float32(min_dist) * np.float32(min_dist)
    keep = K.keep_array(keep)
    obst = [keep[:, 0].copy(), keep[:, 1].copy()]
    xy, sc = [], []
    for k in range(n):
        if len(xy) >= max_corners:
            break
        fx, fy = np.float32(rpos[k] % w), np.float32(rpos[k] // w)
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = fx - obst[0], fy - obst[1]
            if (dx * dx + dy * dy < md2).any():
                continue
        xy.append((fx, fy))
        sc.append(rs[k])
        obst = [np.append(obst[0], fx), np.append(obst[1], fy)]
    return np.array(xy, np.float32).reshape(-1, 2), np.array(sc, np.float32)


def detect_np(img, r, min_eig, quality, min_dist, keep, max_corners):
    pos, e = candidates_np(img, r, min_eig)
    rpos, rs, kept = rank_np(pos, e, quality)
    return select_np(img.shape[1], rpos, rs, kept, min_dist, keep, max_corners) + (pos.size,)


# ---- ABI -------------------------------------------------------------------------------------------------------------------

def test_abi_header_declares_and_library_exports_the_corner_names():
    from points_matching_amd import api
    hdr = open(os.path.join(ROOT, "include", "pm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in api.EXPORTS, name
    assert "pm_corner_params;" in code
    r = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    syms = {ln.split()[-1] for ln in r.stdout.splitlines() if ln.strip()}
    assert not [n for n in NAMES if n not in syms]
    assert tuple(f[0] for f in api.CornerParams._fields_) == ("block_radius", "min_eig", "quality", "min_dist", "capacity", "flags", "reserved")
    assert ctypes.sizeof(api.CornerParams) == 32
    p = api.corner_params(block_radius=7, min_eig=2.0, quality=0.5, min_dist=3.0, capacity=99)
    assert (p.block_radius, p.min_eig, p.quality, p.min_dist, p.capacity, p.flags, tuple(p.reserved)) == (7, 2.0, 0.5, 3.0, 99, 0, (0, 0))


def test_header_compiles_as_c99_with_an_initialiser(tmp_path):
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    src = tmp_path / "use_pm.c"
    src.write_text('#include "pm.h"\n'
                   "static const pm_corner_params prm = {10, 1e-4f, 0.01f, 8.0f, 0, 0, {0, 0}};\n"
                   "int use(pm_ctx* c, const pm_pyramid* p, float* xy, int32_t* n)\n"
                   "{ return sizeof(pm_corner_params) == 32 ? pm_corners_dev(c, p, &prm, 0, 0, 0, 100, xy, 0, n) : -1; }\n")
    r = subprocess.run([cc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "use_pm.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_restatement_is_not_part_of_the_library():
    pkg = os.path.join(ROOT, "points_matching_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".hip", ".cpp", ".hpp", ".h", ".py")):
                assert "corner_ref" not in open(os.path.join(d, f), errors="replace").read(), f


# ---- S67 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", [2, 10, 15])
def test_response_is_the_trackers_eigenvalue_bit_for_bit(img, r):
    """200 random pixels of V per radius: e of S67 == the e that lk_ref's template computes (S63), and the template is usable."""
    h, w = img.shape
    rng = np.random.default_rng(r)
    xs, ys = rng.integers(r + 1, w - r - 2, 200), rng.integers(r + 1, h - r - 2, 200)
    bad = 0
    for x, y in zip(xs.tolist(), ys.tolist()):
        code, _, _, _, G = R.template(img, float(x), float(y), r, 0.0)
        e = K.response(img, r, x, y)
        assert code in (0, 2)                                    # (2: flat by the determinant test, the eigenvalue is still formed)
        bad += int(bits64(G[4])[0] != bits64(e)[0])
    assert bad == 0


@pytest.mark.parametrize("r", [2, 10, 15])
def test_valid_region_is_where_the_template_stays_inside(img, r):
    h, w = img.shape
    for x, y in ((r + 1, r + 1), (w - r - 3, r + 1), (r + 1, h - r - 3), (w - r - 3, h - r - 3)):
        assert K.in_v(img.shape, r, x, y) and R.template(img, float(x), float(y), r, 0.0)[0] != 1, (x, y)
    for x, y in ((r, r + 1), (r + 1, r), (w - r - 2, r + 1), (r + 1, h - r - 2)):
        assert not K.in_v(img.shape, r, x, y) and R.template(img, float(x), float(y), r, 0.0)[0] == 1, (x, y)


@pytest.mark.parametrize("r", [1, 10, 15])
def test_response_equals_numpy_on_the_fixture(img, r):
    h, w = img.shape
    want = response_np(img, r)
    got = np.full((h, w), -np.inf)
    K.lib().corner_response_plane(K.cref.ptr(img), w, h, r, K.cref.ptr(got))
    assert (bits64(got) == bits64(want)).all()


# ---- S68 - S70 against numpy -------------------------------------------------------------------------------------------------

CASES = [("fixture", 1, 1.0), ("fixture", 10, 1.0), ("fixture", 15, 1.0), ("fixture", 1, 1e-4), ((67, 35), 2, 1e-4), ((130, 37), 3, 1e-4),
         ((64, 48), 1, 1e-4), ((16, 16), 6, 0.0), ((16, 16), 7, 0.0)]


def case_image(img, what):
    return img if what == "fixture" else K.random_image(*what)


@pytest.mark.parametrize("what,r,min_eig", CASES)
def test_candidates_and_ranking_equal_numpy(img, what, r, min_eig):
    im = case_image(img, what)
    pos, e = K.candidates(im, r, min_eig)
    pos_np, e_np = candidates_np(im, r, min_eig)
    print("%s r %d min_eig %g: %d candidates, %d distinct fp32 scores" % (what, r, min_eig, pos.size, np.unique(e.astype(np.float32)).size))
    assert pos.size == pos_np.size and (pos == pos_np).all() and (bits64(e) == bits64(e_np)).all()
    for q in (0.0, 0.05, 1.0):
        rpos, rs, kept = K.rank(pos, e, q)
        rpos_np, rs_np, kept_np = rank_np(pos_np, e_np, q)
        assert (rpos == rpos_np).all() and (bits(rs) == bits(rs_np)).all() and kept == kept_np
    if what == (16, 16):                                          # V is the single pixel (7, 7) at r = 6 and empty at r = 7
        assert (pos.tolist() == [7 * 16 + 7]) if r == 6 else (pos.size == 0)


def test_the_tie_rule_is_exercised_on_the_fixture(img):
    """r = 1, min_eig 1e-4: thousands of candidates share an fp32 score with another one, so the position half of the key decides."""
    pos, e = K.candidates(img, 1, 1e-4)
    s = e.astype(np.float32)
    print("fixture r 1: %d candidates, %d distinct fp32 scores" % (pos.size, np.unique(s).size))
    assert pos.size > 5000 and pos.size - np.unique(s).size > 1000
    rpos, rs, _ = K.rank(pos, e)
    same = rs[1:] == rs[:-1]
    assert (rs[1:] <= rs[:-1]).all() and (rpos[1:][same] > rpos[:-1][same]).all()


@pytest.mark.parametrize("min_dist,max_corners", [(0.0, 1 << 20), (5.0, 500), (10.0, 50), (8.0, 200)])
@pytest.mark.parametrize("quality", [0.0, 0.05, 1.0])
def test_selection_equals_numpy(img, min_dist, max_corners, quality):
    h, w = img.shape
    rng = np.random.default_rng(11)
    keep = np.stack([rng.uniform(0, w, 40), rng.uniform(0, h, 40)], 1).astype(np.float32)
    keep[3] = (np.nan, 100.0)
    keep[4] = (np.inf, 100.0)
    for r, kp in ((10, None), (10, keep), (3, keep)):
        xy, sc, nc = K.detect(img, r, 1.0, quality, min_dist, kp, max_corners)
        xy_np, sc_np, nc_np = detect_np(img, r, 1.0, quality, min_dist, kp, max_corners)
        assert nc == nc_np and xy.shape == xy_np.shape and (bits(xy) == bits(xy_np)).all() and (bits(sc) == bits(sc_np)).all()
        assert quality != 1.0 or xy.shape[0] >= 1


# ---- plateaus ----------------------------------------------------------------------------------------------------------------

def test_plateaus():
    # exact fp64 ties all over a periodic pattern
    im = K.block_pattern()
    for r in (1, 2, 3):
        pos, e = K.candidates(im, r, 0.0)
        pos_np, e_np = candidates_np(im, r, 0.0)
        assert (pos == pos_np).all() and (bits64(e) == bits64(e_np)).all() and pos.size > 0
        plane = response_np(im, r)
        assert np.unique(plane[np.isfinite(plane)]).size < 0.2 * np.isfinite(plane).sum()          # ties abound
        cand = set(pos.tolist())
        w = im.shape[1]
        # no two candidates are 8-neighbours with equal responses: one pixel per plateau pair
        for p in pos.tolist():
            for d in (1, w - 1, w, w + 1):
                assert not (p + d in cand and plane.ravel()[p + d] == plane.ravel()[p]), (r, p, d)
    # a two-pixel plateau: (19, y) and (20, y) carry the same response; exactly the first in scan order is a candidate
    im = K.two_pixel_plateau()
    w = im.shape[1]
    plane = response_np(im, 2)
    assert (bits64(plane[:, 4:20]) == bits64(plane[:, 35:19:-1])).all()                  # (V is columns 3 .. 35: not its own mirror image)
    pos, e = K.candidates(im, 2, 0.0)
    cand = set(pos.tolist())
    pairs = [p for p in pos.tolist() if p % w == 19 and plane.ravel()[p + 1] == plane.ravel()[p]]
    print("two-pixel plateau: %d candidates, %d on the axis" % (pos.size, len(pairs)))
    assert pairs and all(p + 1 not in cand for p in pairs)
    assert not [p for p in pos.tolist() if p % w == 20 and plane.ravel()[p - 1] == plane.ravel()[p]]
    # flat ground: e == 0 everywhere, no candidate, also with min_eig 0
    assert K.candidates(K.constant_image(), 3, 0.0)[0].size == 0
    assert K.detect(K.constant_image(), 3, 0.0)[0].shape[0] == 0


# ---- greedy properties -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_dist,max_corners", [(5.0, 500), (10.0, 50), (8.0, 100000)])
def test_greedy_properties(img, min_dist, max_corners):
    h, w = img.shape
    rng = np.random.default_rng(5)
    keep = np.stack([rng.uniform(0, w, 60), rng.uniform(0, h, 60)], 1).astype(np.float32)
    pos, e = K.candidates(img, 10, 1.0)
    rpos, rs, kept = K.rank(pos, e, 0.0)
    xy, sc, fate = K.select(w, rpos, rs, kept, min_dist, keep, max_corners)
    m = xy.shape[0]
    assert m == (fate == 1).sum() and m <= max_corners
    walked = np.flatnonzero(fate)
    assert walked.size == 0 or (walked == np.arange(walked.size)).all()                     # a prefix of the ranks
    assert m == max_corners or walked.size == kept
    P = xy.astype(np.float64)
    d = np.hypot(P[:, None, 0] - P[None, :, 0], P[:, None, 1] - P[None, :, 1])
    d[np.arange(m), np.arange(m)] = np.inf
    dk = np.hypot(P[:, None, 0] - keep[None, :, 0].astype(np.float64), P[:, None, 1] - keep[None, :, 1].astype(np.float64))
    print("min_dist %g: %d corners of %d walked; nearest pair %.3f, nearest keep %.3f" % (min_dist, m, walked.size, d.min(), dk.min()))
    assert d.min() >= min_dist and dk.min() >= min_dist
    obst = np.concatenate([P, keep.astype(np.float64)])
    rej = np.flatnonzero(fate == 2)
    rx, ry = (rpos[rej] % w).astype(np.float64), (rpos[rej] // w).astype(np.float64)
    near = np.hypot(rx[:, None] - obst[None, :, 0], ry[:, None] - obst[None, :, 1]).min(axis=1)
    assert rej.size > 0 and (near < min_dist).all()
    assert (bits(sc) == bits(rs[fate == 1])).all()
