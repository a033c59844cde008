"""CPU: the arithmetic of SPEC S71-S74 (oriented 256-bit descriptors of given points).  Three statements are compared: the
library's host-computed tables (pm_describe_points_tables, no GPU needed), the plain-C restatement tests/describe_ref.c and the
numpy statement in tests/describe_ref.py; then the properties the design rests on are checked on the C restatement, which the
GPU file holds the kernel to bit for bit: the bin rule against fp64 atan2, exact 90-degree rotation, and rotation invariance
under resampling."""
import hashlib

import numpy as np
import pytest

import describe_ref as D
import features_bits_ref as B
import lk_ref as R
from points_matching_amd import api


# ---- tables --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tabs():
    return {"lib": api.describe_points_tables(), "c": D.tables(), "np": D.np_tables()}


def test_tables_of_the_three_statements_are_equal_and_pinned(tabs):
    q, st = tabs["np"]
    assert hashlib.sha256(st.tobytes()).hexdigest() == D.TABLE_SHA256
    assert hashlib.sha256(q.astype("<i4").tobytes()).hexdigest() == D.Q20_SHA256
    assert q[:4].tolist() == [-1044586, -1012847, -950333, -858943]
    for name in ("lib", "c"):
        assert tabs[name][0].dtype == np.int32 and tabs[name][1].dtype == np.int8
        assert (tabs[name][0] == q).all() and (tabs[name][1] == st).all(), name
    assert (st[36] == B.base_pattern()).all() and B.pattern_sha256(st[36]) == B.PATTERN_SHA256
    assert (st[36] == api.detect_bits_table()[0]).all()


def test_either_table_pointer_may_be_null():
    import ctypes as C
    q = np.zeros(72, np.int32)
    st = np.zeros((37, 256, 4), np.int8)
    assert api.lib().pm_describe_points_tables(None, None) == 0
    assert api.lib().pm_describe_points_tables(q.ctypes.data_as(C.c_void_p), None) == 0
    assert api.lib().pm_describe_points_tables(None, st.ctypes.data_as(C.c_void_p)) == 0
    want = api.describe_points_tables()
    assert (q == want[0]).all() and (st == want[1]).all()


def test_rounding_ties_are_far(tabs):
    """Measured: the nearest rounding tie is 1.0e-4 away for the offsets and 1.5e-2 for the Q20 values.  A cosine that is one
    ulp off moves an offset by at most 2 * 15 * 1.2e-16 and a Q20 value by 2^20 * 1.2e-16 = 1.2e-10, so a margin of 1e-6, ten
    thousand times that, shows that libm's last bit cannot move an entry."""
    b = np.arange(36)
    theta = (b + 0.5) / 36 * 2 * np.pi - np.pi
    cs, sn = np.cos(theta), np.sin(theta)
    f = tabs["np"][1][36].astype(np.float64)
    vals = []
    for p in (0, 2):
        x, y = f[:, p], f[:, p + 1]
        vals += [cs[:, None] * x - sn[:, None] * y, sn[:, None] * x + cs[:, None] * y]
    v = np.stack(vals)
    margin = np.abs(np.abs(v - np.floor(v)) - 0.5).min()
    q = 1048576.0 * np.concatenate([cs, sn])
    qmargin = np.abs(np.abs(q - np.floor(q)) - 0.5).min()
    print("nearest tie: offsets %.3g, Q20 %.3g" % (margin, qmargin))
    assert margin >= 1e-6 and qmargin >= 1e-6


def test_offsets_stay_within_15_and_rows_turn_by_quarter_turns(tabs):
    st = tabs["np"][1].astype(np.int32)
    assert np.abs(st).max() == 15
    for b in range(36):
        a, c = st[b], st[(b + 9) % 36]
        assert (c[:, 0] == -a[:, 1]).all() and (c[:, 1] == a[:, 0]).all() and (c[:, 2] == -a[:, 3]).all() and (c[:, 3] == a[:, 2]).all(), b
    # tests that coincide after rounding exist and give bit 0 by the strict <
    same = (st[:36, :, 0] == st[:36, :, 2]) & (st[:36, :, 1] == st[:36, :, 3])
    print("coinciding steered tests per bin: max %d" % same.sum(axis=1).max())
    assert same.sum(axis=1).max() <= 4 and not same[:, :].all()


# ---- S72: the bin rule -----------------------------------------------------------------------------------------------------------

def atan2_bin(m10, m01):
    """The bin whose interval holds atan2(m01, m10), and the distance of the angle to the nearest bin boundary in degrees."""
    ang = np.degrees(np.arctan2(m01.astype(np.float64), m10.astype(np.float64)))            # -180 .. 180
    pos = (ang + 180.0) / 10.0
    b = np.floor(pos).astype(np.int64) % 36
    dist = np.minimum(pos - np.floor(pos), np.ceil(pos) - pos) * 10.0
    return b, dist


@pytest.mark.parametrize("limit,n", [(1150000, 400000), (40, 20000)])
def test_bin_rule_against_atan2(limit, n):
    rng = np.random.default_rng(limit)
    m10, m01 = rng.integers(-limit, limit + 1, n), rng.integers(-limit, limit + 1, n)
    nz = (m10 != 0) | (m01 != 0)
    m10, m01 = m10[nz], m01[nz]
    got = D.np_bin(m10, m01)
    want, dist = atan2_bin(m10, m01)
    clear = dist >= 0.01
    left_out = 1.0 - clear.mean()
    wrong = got != want
    print("limit %d: %d pairs, %.3f %% within 0.01 deg of a boundary, %d disagreements (largest distance %.3g deg)" %
          (limit, m10.size, 100 * left_out, wrong.sum(), dist[wrong].max() if wrong.any() else 0.0))
    assert (got[clear] == want[clear]).all()
    if limit > 1000:
        assert left_out <= 0.01
    else:               # on the small lattice only the axis directions are ON a boundary (exact ties, see test_bin_ties); the
        off_axis = (m10 != 0) & (m01 != 0)          # nearest other direction, 3 : 17, is 0.008 degrees away and must agree
        assert (got[off_axis] == want[off_axis]).all()
    # the C statement takes the same decisions
    idx = rng.integers(0, m10.size, 2000)
    assert [D.bin_of(m10[i], m01[i]) for i in idx] == got[idx].tolist()


def test_bin_ties():
    """(0, 0) gives bin 0.  An axis direction lies on the boundary of two bins, whose Q20 entries are mirror images: the two
    dots are equal and the lower bin wins."""
    assert D.bin_of(0, 0) == 0 and D.np_bin(0, 0)[0] == 0
    q = D.np_tables()[0].astype(np.int64)
    for m10, m01 in ((1000, 0), (-1000, 0), (0, 1000), (0, -1000), (1, 0), (0, -1)):
        dots = m10 * q[:36] + m01 * q[36:]
        top = np.flatnonzero(dots == dots.max())
        assert top.size == 2, (m10, m01)
        assert D.bin_of(m10, m01) == D.np_bin(m10, m01)[0] == top[0]
    assert D.bin_of(1000, 0) == 17 and D.bin_of(0, 1000) == 26 and D.bin_of(0, -1000) == 8
    assert D.bin_of(-1000, 0) == 0          # bins 0 and 35 tie


# ---- the C restatement against the numpy statement ---------------------------------------------------------------------------------

def assert_same(tag, got, want):
    for name, g, w in zip(("desc", "valid", "bin"), got, want):
        assert g.shape == w.shape and (g == w).all(), "%s: %s differs" % (tag, name)


@pytest.fixture(scope="module")
def fixture_rows():
    """The C restatement on the fixture at levels 0, 1, 2 of one pyramid."""
    img, pts = D.fixture_corners()
    pyr = R.Pyramid(img, 2)
    assert pyr.n == 3
    return img, pts, pyr, [D.describe(pyr.levels[l], l, pts) for l in range(3)]


def test_fixture_levels(fixture_rows):
    img, pts, pyr, rows = fixture_rows
    assert pts.shape == (344, 2) and int(rows[0][1].sum()) == 305
    for l in range(3):
        assert_same("fixture level %d" % l, rows[l], D.np_describe(pyr.levels[l], l, pts))
        d, v, b = rows[l]
        print("level %d: %d of %d valid, %d distinct bins" % (l, v.sum(), v.size, np.unique(b[v == 1]).size))
        assert v.sum() > 100 and (d[v == 0] == 0).all() and (b[v == 0] == 255).all() and (b[v == 1] < 36).all()
    assert_same("fixture upright", D.describe(img, 0, pts, D.UPRIGHT), D.np_describe(img, 0, pts, D.UPRIGHT))
    assert (D.describe(img, 0, pts, D.UPRIGHT)[2][rows[0][1] == 1] == 36).all()


@pytest.mark.parametrize("w,h", D.SMALL)
def test_small_images_and_the_lattice(w, h):
    img = D.small_image(w, h)
    for pts in (D.lattice(w, h), D.alternating(w, h)):
        got = D.describe(img, 0, pts)
        assert_same("%dx%d" % (w, h), got, D.np_describe(img, 0, pts))
        # S71 directly: ties to even, the border rule, the refused inputs
        x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(x) & np.isfinite(y) & (np.abs(x) <= 1e6) & (np.abs(y) <= 1e6)
            cx, cy = np.rint(np.where(fin, x, 0)), np.rint(np.where(fin, y, 0))
        want = fin & (cx >= 17) & (cx <= w - 18) & (cy >= 17) & (cy <= h - 18)
        assert (got[1] == want).all()
        assert got[1].sum() >= 1 and (got[1] == 0).sum() >= 1
    if (w, h) == (36, 40):
        one = lambda x, y: int(D.describe(img, 0, np.array([[x, y]], np.float32))[1][0])
        assert one(17.5, 20) == 1 and one(18.5, 20) == 1 and one(16.5, 20) == 0 and one(16.0, 20) == 0 and one(17.0, 20) == 1
        assert one(18.0, 20) == 1 and one(19.0, 20) == 0 and one(18.500002, 20) == 0
        # 17.5 -> 18 and 18.5 -> 18 share their row; 17.0 has another centre
        rows = D.describe(img, 0, np.array([[17.5, 20], [18.5, 20], [18.0, 20], [17.0, 20]], np.float32))[0]
        assert (rows[0] == rows[2]).all() and (rows[1] == rows[2]).all() and (rows[3] != rows[2]).any()


def test_constant_image():
    img = D.constant_image()
    h, w = img.shape
    pts = np.array([[17, 17], [w - 18, h - 18], [24.3, 20.7], [16, 17]], np.float32)
    for stmt in (D.describe, D.np_describe):
        d, v, b = stmt(img, 0, pts)
        assert v.tolist() == [1, 1, 1, 0] and b.tolist() == [0, 0, 0, 255] and (d == 0).all()


# ---- rotation ----------------------------------------------------------------------------------------------------------------------

def tied_rows(plane, pts, valid):
    """Rows whose arg-max of S72 is not unique."""
    q = D.np_tables()[0].astype(np.int64)
    h, w = plane.shape
    out = np.zeros(pts.shape[0], bool)
    for k in np.flatnonzero(valid):
        m = np.zeros(2, np.int32)
        cx, cy = int(np.rint(pts[k, 0])), int(np.rint(pts[k, 1]))
        D.lib().describe_moments(D.cref.ptr(plane), w, cx, cy, m[0:].ctypes.data, m[1:].ctypes.data)
        dots = int(m[0]) * q[:36] + int(m[1]) * q[36:]
        out[k] = (dots == dots.max()).sum() > 1
    return out


def test_exact_quarter_turn(fixture_rows):
    """np.rot90 moves pixel (x, y) to (y, w - 1 - x).  The moments turn with the image, the steered rows of bins b and b + 9 are
    quarter turns of each other and the box sums are those of the same pixels: equal bytes, bin' - bin = 27 mod 36."""
    img, pts, _, rows = fixture_rows
    h, w = img.shape
    rot = np.ascontiguousarray(np.rot90(img))
    rpts = np.stack([pts[:, 1], w - 1 - pts[:, 0]], 1).astype(np.float32)
    d0, v0, b0 = rows[0]
    d1, v1, b1 = D.describe(rot, 0, rpts)
    assert (v0 == v1).all()
    both = (v0 == 1) & (v1 == 1)
    tied = tied_rows(img, pts, both)
    use = both & ~tied
    equal = (d0[use] == d1[use]).all(axis=1)
    print("quarter turn: %d rows valid in both, %d tied, %d of %d equal" % (both.sum(), tied.sum(), equal.sum(), use.sum()))
    assert tied.sum() <= 0.01 * both.sum()
    assert equal.all()
    assert (((b1[use].astype(int) - b0[use].astype(int)) % 36) == 27).all()


def far_from_borders(p, shape, d=25.0):
    h, w = shape
    return (p[:, 0] > d) & (p[:, 0] < w - 1 - d) & (p[:, 1] > d) & (p[:, 1] < h - 1 - d)


def partner_share(img, pts, frame, mapped, flags):
    """Among the points valid in both frames and far from every border in both: the share whose Hamming nearest neighbour among
    the second frame's rows is their true partner (first minimum)."""
    mp = mapped.astype(np.float32)
    d1, v1, _ = D.describe(img, 0, pts, flags)
    d2, v2, _ = D.describe(frame, 0, mp, flags)
    sel = far_from_borders(pts, img.shape) & far_from_borders(mapped, img.shape) & (v1 == 1) & (v2 == 1)
    H = D.hamming(d1[sel], d2[sel])
    n = int(sel.sum())
    hit = H.argmin(axis=1) == np.arange(n)
    pair = np.diag(H)
    other = (H + np.eye(n, dtype=H.dtype) * 1000).min(axis=1)
    return int(hit.sum()), n, float(np.median(pair)), int(other.min())


@pytest.mark.parametrize("deg", [30.0, 45.0, 137.0])
def test_rotation_invariance_by_resampling(fixture_rows, deg):
    """Measured with this selection (more than 25 px from every border in both frames, valid in both): 217 of 218 at 30
    degrees, 210 of 211 at 45, 215 of 218 at 137; upright at 30 degrees 31 of 218."""
    img, pts = fixture_rows[0], fixture_rows[1]
    frame = D.rotate_frame(img, deg)
    mapped = D.rotate_map(pts, img.shape, deg)
    hit, n, med, other = partner_share(img, pts, frame, mapped, 0)
    print("%g deg steered: %d of %d, true-pair median %g bits, nearest non-pair %d" % (deg, hit, n, med, other))
    assert n >= 150 and hit >= 0.95 * n
    if deg == 30.0:
        hit_u, n_u, _, _ = partner_share(img, pts, frame, mapped, D.UPRIGHT)
        print("%g deg upright: %d of %d" % (deg, hit_u, n_u))
        assert n_u >= 150 and hit_u <= 0.20 * n_u


def test_one_degree_frame(fixture_rows):
    """Measured: 265 of 267; true-pair distance median 8 bits, nearest non-pair 19."""
    img, pts = fixture_rows[0], fixture_rows[1]
    hit, n, med, other = partner_share(img, pts, R.frame_r(img), R.frame_r_map(pts, img.shape), 0)
    print("frame R: %d of %d, true-pair median %g bits, nearest non-pair %d" % (hit, n, med, other))
    assert n >= 150 and hit >= 0.95 * n
