"""GPU: oriented 256-bit descriptors of given points (pm_describe_points*, SPEC S71-S74) against the plain-C restatement
tests/describe_ref.c, which tests/test_describe_points_cpu.py pins on the CPU.  Every comparison is bit for bit and there is no
tolerance anywhere: the moments, the box sums and the bin's dot products are exact integers."""
import gc

import numpy as np
import pytest

import corner_ref as K
import describe_ref as D
import lk_ref as R
from points_matching_amd import api

pytestmark = pytest.mark.gpu
PAT = 0xA5
PATTERN_F = -7.5


@pytest.fixture(scope="module")
def ctx():
    import torch
    import points_matching_amd as pm
    c = pm.Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()
    gc.collect()


class Frames:
    """Images by name, their device pyramids and the restatement's rows, each made once."""

    def __init__(self, ctx):
        self.ctx = ctx
        img, self.corners = D.fixture_corners()
        self.img = {"1": img, "S": R.frame_s(img), "rot30": D.rotate_frame(img, 30.0), "flat": D.constant_image()}
        for w, h in D.SMALL:
            self.img["%dx%d" % (w, h)] = D.small_image(w, h)
        self._dev, self._pyr, self._ref = {}, {}, {}

    def dev(self, name, max_level=0):
        import torch
        if (name, max_level) not in self._dev:
            d_img = torch.from_numpy(self.img[name]).to("cuda:0")
            torch.cuda.synchronize()
            h, w = self.img[name].shape
            p = self.ctx.pyramid(w, h, max_level).build_dev(d_img.data_ptr())
            self.ctx.synchronize()
            self._dev[(name, max_level)] = p
        return self._dev[(name, max_level)]

    def ref(self, name, level, pts, flags=0, max_level=0):
        key = (name, level, pts.tobytes(), flags, max_level)
        if key not in self._ref:
            if (name, max_level) not in self._pyr:
                self._pyr[(name, max_level)] = R.Pyramid(self.img[name], max_level)
            self._ref[key] = D.describe(self._pyr[(name, max_level)].levels[level], level, pts, flags)
        return self._ref[key]

    def close(self):
        for p in self._dev.values():
            p.close()


@pytest.fixture(scope="module")
def fr(ctx):
    f = Frames(ctx)
    yield f
    ctx.synchronize()
    f.close()


def dev_describe(ctx, pyr, pts, level=0, flags=0, count="none", cap=None, want_valid=True, want_bin=True):
    """pm_describe_points_dev on buffers pre-filled with a pattern -> (desc (cap, 32), valid (cap,), bin (cap,)).
    count: "none" = no count pointer, else the value of the device count."""
    import torch
    dev = torch.device("cuda", 0)
    pts = D.points_array(pts)
    cap = pts.shape[0] if cap is None else cap
    buf = np.full((cap, 2), PATTERN_F, np.float32)
    buf[:min(cap, pts.shape[0])] = pts[:cap]
    d_pts = torch.from_numpy(buf).to(dev)
    d_desc = torch.full((cap, 32), PAT, dtype=torch.uint8, device=dev)
    d_valid = torch.full((cap,), PAT, dtype=torch.uint8, device=dev)
    d_bin = torch.full((cap,), PAT, dtype=torch.uint8, device=dev)
    d_n = torch.tensor([count], dtype=torch.int32, device=dev) if count != "none" else None
    torch.cuda.synchronize()
    ctx.describe_points_dev(pyr, d_pts.data_ptr(), d_n.data_ptr() if d_n is not None else None, cap, api.describe_params(level, flags),
                            d_desc.data_ptr(), d_valid.data_ptr() if want_valid else None, d_bin.data_ptr() if want_bin else None)
    ctx.synchronize()
    return d_desc.cpu().numpy(), d_valid.cpu().numpy(), d_bin.cpu().numpy()


def assert_rows(tag, got, want, n=None):
    """Rows [0, n) equal the restatement's; everything at and beyond n still holds the pattern."""
    n = want[0].shape[0] if n is None else n
    for name, g, w in zip(("desc", "valid", "bin"), got, want):
        diff = np.flatnonzero((g[:n] != w[:n]).reshape(n, -1).any(axis=1)) if n else np.zeros(0, np.int64)
        print("%s: %s, %d rows, %d differ%s" % (tag, name, n, diff.size, (", first %d" % diff[0]) if diff.size else ""))
        assert diff.size == 0, "%s: %s" % (tag, name)
        assert (g[n:] == PAT).all(), "%s: %s written behind the count" % (tag, name)


# ---- the rows ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [0, 1, 2])
def test_fixture_corners_on_three_levels(ctx, fr, level):
    want = fr.ref("1", level, fr.corners, 0, 2)
    assert fr.corners.shape[0] == 344 and want[1].sum() > 100
    assert_rows("fixture level %d" % level, dev_describe(ctx, fr.dev("1", 2), fr.corners, level), want)


@pytest.mark.parametrize("w,h", D.SMALL)
def test_small_images_lattice_and_mixed_workgroups(ctx, fr, w, h):
    name = "%dx%d" % (w, h)
    for pts in (D.lattice(w, h), D.alternating(w, h)):
        want = fr.ref(name, 0, pts)
        assert 0 < want[1].sum() < pts.shape[0]
        assert_rows(name, dev_describe(ctx, fr.dev(name), pts), want)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 67])
def test_counts_that_are_no_multiple_of_four(ctx, fr, n):
    pts = D.alternating(67, 35, 67)[:n]
    assert_rows("%d points" % n, dev_describe(ctx, fr.dev("67x35"), pts), fr.ref("67x35", 0, pts))


@pytest.mark.parametrize("count,used", [("none", 40), (0, 0), (-1, 0), (55, 40), (40, 40), (17, 17), (1, 1)])
def test_device_count_protocol(ctx, fr, count, used):
    """cap = 40 rows of 67 points: no pointer = cap; 0; the -1 of an overflowed detector = 0; above cap = cap; inside."""
    pts = D.alternating(67, 35, 67)
    want = fr.ref("67x35", 0, pts[:40])
    assert_rows("count %s" % count, dev_describe(ctx, fr.dev("67x35"), pts, count=count, cap=40), want, used)


def test_null_valid_and_bin(ctx, fr):
    pts = D.lattice(36, 40)
    want = fr.ref("36x40", 0, pts)
    for wv, wb in ((False, True), (True, False), (False, False)):
        d, v, b = dev_describe(ctx, fr.dev("36x40"), pts, want_valid=wv, want_bin=wb)
        assert (d == want[0]).all()
        assert (v == want[1]).all() if wv else (v == PAT).all()
        assert (b == want[2]).all() if wb else (b == PAT).all()


def test_upright(ctx, fr):
    want = fr.ref("1", 0, fr.corners, D.UPRIGHT)
    assert (want[2][want[1] == 1] == 36).all() and (want[0] != fr.ref("1", 0, fr.corners)[0]).any()
    assert_rows("upright", dev_describe(ctx, fr.dev("1"), fr.corners, 0, api.PM_DESCRIBE_UPRIGHT), want)
    pts = D.lattice(67, 35)
    assert_rows("upright 67x35", dev_describe(ctx, fr.dev("67x35"), pts, 0, api.PM_DESCRIBE_UPRIGHT), fr.ref("67x35", 0, pts, D.UPRIGHT))


def test_constant_image(ctx, fr):
    h, w = fr.img["flat"].shape
    pts = np.array([[17, 17], [w - 18, h - 18], [24.3, 20.7], [16, 17], [20, 20]], np.float32)
    d, v, b = dev_describe(ctx, fr.dev("flat"), pts)
    assert v.tolist() == [1, 1, 1, 0, 1] and b.tolist() == [0, 0, 0, 255, 0] and (d == 0).all()
    assert_rows("flat", (d, v, b), fr.ref("flat", 0, pts))


def test_two_runs_give_identical_bytes(ctx, fr):
    a = dev_describe(ctx, fr.dev("1"), fr.corners)
    b = dev_describe(ctx, fr.dev("1"), fr.corners)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_host_form_equals_the_device_form(ctx, fr):
    img = fr.img["1"]
    for level, flags in ((0, 0), (2, 0), (1, api.PM_DESCRIBE_UPRIGHT)):
        want = fr.ref("1", level, fr.corners, flags, level)         # the host form builds the pyramid up to `level`
        got = ctx.describe_points(img, fr.corners, api.describe_params(level, flags))
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), (level, flags)
    dev = dev_describe(ctx, fr.dev("1", 2), fr.corners, 2)
    got = ctx.describe_points(img, fr.corners, api.describe_params(2))
    assert all(g.tobytes() == d.tobytes() for g, d in zip(got, dev))
    # a row stride
    h, w = fr.img["67x35"].shape
    buf = np.random.default_rng(5).integers(0, 256, (h, w + 5), dtype=np.uint8)
    buf[:, :w] = fr.img["67x35"]
    pts = D.lattice(w, h)
    got = ctx.describe_points(buf, pts, w=w)
    assert all(g.tobytes() == x.tobytes() for g, x in zip(got, fr.ref("67x35", 0, pts)))


# ---- the gather form -----------------------------------------------------------------------------------------------------------------

def dev_gather(ctx, pyr, d_pts_ptr, d_n_ptr, cap, level=0, flags=0, src=True):
    import torch
    dev = torch.device("cuda", 0)
    d_xy = torch.full((cap, 2), PATTERN_F, dtype=torch.float32, device=dev)
    d_desc = torch.full((cap, 32), PAT, dtype=torch.uint8, device=dev)
    d_src = torch.full((cap,), -9, dtype=torch.int32, device=dev)
    d_cnt = torch.full((1,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.describe_points_gather_dev(pyr, d_pts_ptr, d_n_ptr, cap, api.describe_params(level, flags), d_xy.data_ptr(), d_desc.data_ptr(),
                                   d_cnt.data_ptr(), d_src.data_ptr() if src else None)
    ctx.synchronize()
    return int(d_cnt.item()), d_xy.cpu().numpy(), d_desc.cpu().numpy(), d_src.cpu().numpy()


def assert_gathered(tag, got, pts, want, src_written=True):
    """got: dev_gather's tuple; pts: the input rows that were in range; want: the restatement's aligned rows of pts."""
    cnt, xy, desc, src = got
    keep = np.flatnonzero(want[1] == 1)
    print("%s: %d of %d rows gathered (restatement %d)" % (tag, cnt, pts.shape[0], keep.size))
    assert cnt == keep.size
    assert xy[:cnt].view(np.uint32).tobytes() == np.ascontiguousarray(pts[keep]).view(np.uint32).tobytes()
    assert (desc[:cnt] == want[0][keep]).all()
    assert (xy[cnt:] == PATTERN_F).all() and (desc[cnt:] == PAT).all()
    assert (src[:cnt] == keep).all() if src_written else (src[:cnt] == -9).all()
    assert (src[cnt:] == -9).all()


@pytest.mark.parametrize("count", ["none", 0, -1, 33, 90])
def test_gather_equals_the_aligned_form_compacted(ctx, fr, count):
    import torch
    pts = D.alternating(67, 35, 67)
    pts[7] = (np.nan, 20.0)                                          # a NaN row among the input: its bits are never copied
    d_pts = torch.from_numpy(pts).to("cuda:0")
    d_n = torch.tensor([count], dtype=torch.int32, device="cuda:0") if count != "none" else None
    used = 67 if count == "none" else min(max(count, 0), 67)
    got = dev_gather(ctx, fr.dev("67x35"), d_pts.data_ptr(), d_n.data_ptr() if d_n is not None else None, 67)
    assert_gathered("gather count %s" % count, got, pts[:used], fr.ref("67x35", 0, pts[:used]) if used else
                    (np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint8)))
    if count == "none":
        got = dev_gather(ctx, fr.dev("67x35"), d_pts.data_ptr(), None, 67, src=False)
        assert_gathered("gather without src_idx", got, pts, fr.ref("67x35", 0, pts), src_written=False)
        al = dev_describe(ctx, fr.dev("67x35"), pts)
        assert (got[2][:got[0]] == al[0][al[1] == 1]).all()


def test_gather_more_than_one_chunk(ctx, fr):
    """2500 points: three chunks of the compaction's 1024 rows, the running base carried across them."""
    import torch
    rng = np.random.default_rng(9)
    h, w = fr.img["1"].shape
    pts = np.stack([rng.uniform(-20, w + 20, 2500), rng.uniform(-20, h + 20, 2500)], 1).astype(np.float32)
    d_pts = torch.from_numpy(pts).to("cuda:0")
    want = fr.ref("1", 0, pts)
    assert 1024 < want[1].sum() < 2500
    assert_gathered("2500 points", dev_gather(ctx, fr.dev("1"), d_pts.data_ptr(), None, 2500), pts, want)


CHUNK_CAP = 2049                                                     # two chunks of the compaction's 1024 rows and one row
CHUNK_KEPT = {"all": lambda n: n, "none": lambda n: 0, "alternating": lambda n: (n + 1) // 2}


@pytest.fixture(scope="module")
def chunk_rows(ctx, fr):
    """pattern -> (points, the same on the device, their aligned rows from pm_describe_points_dev), each made once.  2049
    points of frame "1": every one at least 20 pixels inside the image, every one outside it, or the two in turn."""
    import torch
    h, w = fr.img["1"].shape
    rng = np.random.default_rng(21)
    inside = np.stack([rng.uniform(20, w - 21, CHUNK_CAP), rng.uniform(20, h - 21, CHUNK_CAP)], 1).astype(np.float32)
    outside = np.stack([rng.uniform(w + 5, w + 50, CHUNK_CAP), rng.uniform(-50, -5, CHUNK_CAP)], 1).astype(np.float32)
    mixed = np.where((np.arange(CHUNK_CAP) % 2 == 0)[:, None], inside, outside)
    out = {}
    for pattern, pts in (("all", inside), ("none", outside), ("alternating", mixed)):
        aligned = dev_describe(ctx, fr.dev("1"), pts)
        assert int(aligned[1].sum()) == CHUNK_KEPT[pattern](CHUNK_CAP)
        out[pattern] = (pts, torch.from_numpy(pts).to("cuda:0"), aligned)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("pattern", ["all", "none", "alternating"])
@pytest.mark.parametrize("count", [0, 1, 1023, 1024, 1025, 2049])
def test_gather_at_the_chunk_boundary(ctx, fr, chunk_rows, pattern, count):
    """The device count at 0, 1, one below, at and one above the compaction's chunk of 1024 rows, and at two chunks and a row,
    with every row kept, none, and every other one: rows, src_idx and count are the aligned form of the same points compacted on
    the host, and everything behind the count keeps its pattern."""
    import torch
    pts, d_pts, aligned = chunk_rows[pattern]
    d_n = torch.tensor([count], dtype=torch.int32, device="cuda:0")
    got = dev_gather(ctx, fr.dev("1"), d_pts.data_ptr(), d_n.data_ptr(), CHUNK_CAP)
    want = tuple(a[:count] for a in aligned)
    assert int(want[1].sum()) == CHUNK_KEPT[pattern](count)
    assert_gathered("%s, count %d" % (pattern, count), got, pts[:count], want)


def test_gather_chained_after_corners(ctx, fr):
    """pm_corners_dev -> pm_describe_points_gather_dev through the device count, no host round trip between them."""
    import torch
    dev = torch.device("cuda", 0)
    CAP = 500
    d_kp = torch.full((CAP, 2), PATTERN_F, dtype=torch.float32, device=dev)
    d_n = torch.full((1,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.corners_dev(fr.dev("1"), api.corner_params(10, 1e-4, 0.01, 8.0), CAP, d_kp.data_ptr(), d_n.data_ptr())
    got = dev_gather(ctx, fr.dev("1"), d_kp.data_ptr(), d_n.data_ptr(), CAP)
    assert int(d_n.item()) == 344 and d_kp.cpu().numpy()[:344].tobytes() == fr.corners.tobytes()
    assert_gathered("after corners", got, fr.corners, fr.ref("1", 0, fr.corners))
    assert got[0] == 305


def test_gather_chained_after_tracking(ctx, fr):
    """pm_track_lk_gather_dev into frame S -> its d_xy2 / d_count described on frame S's pyramid."""
    import torch
    dev = torch.device("cuda", 0)
    CAP = 400
    lk = api.lk_params(10, 2)
    buf = np.full((CAP, 2), PATTERN_F, np.float32)
    buf[:344] = fr.corners
    d_kp = torch.from_numpy(buf).to(dev)
    d_n = torch.tensor([344], dtype=torch.int32, device=dev)
    d_xy1 = torch.full((CAP, 2), PATTERN_F, dtype=torch.float32, device=dev)
    d_xy2 = torch.full((CAP, 2), PATTERN_F, dtype=torch.float32, device=dev)
    d_cnt = torch.full((1,), -9, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.track_lk_gather_dev(fr.dev("1", 2), fr.dev("S", 2), d_kp.data_ptr(), d_n.data_ptr(), CAP, lk, d_xy1.data_ptr(), d_xy2.data_ptr(),
                            d_cnt.data_ptr())
    got = dev_gather(ctx, fr.dev("S", 2), d_xy2.data_ptr(), d_cnt.data_ptr(), CAP)
    cnt = int(d_cnt.item())
    xy2 = d_xy2.cpu().numpy()[:cnt]
    out, status, _, _ = R.track(R.Pyramid(fr.img["1"], 2), R.Pyramid(fr.img["S"], 2), fr.corners, R.params(10, 2))
    assert cnt == (status == 1).sum() > 100 and xy2.tobytes() == out[status == 1].tobytes()
    assert_gathered("after tracking", got, xy2, fr.ref("S", 0, np.ascontiguousarray(xy2), 0, 2))


def test_chain_corners_describe_match(ctx, fr):
    """Corners + gather-describe on image 1 and on the 30-degree frame, then pm_bf_knn_hamming_u8_dev with k = 1: the neighbour
    indices are those computed on the host from the restatement's rows (first minimum, the matcher's tie rule)."""
    import torch
    dev = torch.device("cuda", 0)
    CAP = 500
    prm = api.corner_params(10, 1e-4, 0.01, 8.0)
    rows, counts, refs = [], [], []
    for name in ("1", "rot30"):
        d_kp = torch.zeros((CAP, 2), dtype=torch.float32, device=dev)
        d_n = torch.zeros(1, dtype=torch.int32, device=dev)
        d_xy = torch.zeros((CAP, 2), dtype=torch.float32, device=dev)
        d_desc = torch.zeros((CAP, 32), dtype=torch.uint8, device=dev)
        d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.corners_dev(fr.dev(name), prm, CAP, d_kp.data_ptr(), d_n.data_ptr())
        ctx.describe_points_gather_dev(fr.dev(name), d_kp.data_ptr(), d_n.data_ptr(), CAP, api.describe_params(), d_xy.data_ptr(),
                                       d_desc.data_ptr(), d_cnt.data_ptr())
        ctx.synchronize()
        kp = K.detect(fr.img[name], 10, 1e-4, 0.01, 8.0, None, CAP)[0]
        want = fr.ref(name, 0, kp)
        assert int(d_cnt.item()) == want[1].sum() > 100
        rows.append(d_desc)
        counts.append(int(d_cnt.item()))
        refs.append(want[0][want[1] == 1])
    d_knn = torch.zeros((counts[0], 4), dtype=torch.int32, device=dev)          # pm_match: 16 bytes
    torch.cuda.synchronize()
    ctx.bf_knn_hamming_dev(rows[0].data_ptr(), counts[0], rows[1].data_ptr(), counts[1], 32, 1, d_knn.data_ptr())
    ctx.synchronize()
    knn = d_knn.cpu().numpy().view(api.MATCH_DTYPE).reshape(-1)
    H = D.hamming(refs[0], refs[1])
    print("chain: %d and %d rows; median nearest distance %g bits" % (counts[0], counts[1], np.median(H.min(axis=1))))
    assert (knn["queryIdx"] == np.arange(counts[0])).all()
    assert (knn["distance"] == H.min(axis=1)).all()
    assert (knn["trainIdx"] == H.argmin(axis=1)).all()


# ---- arguments, capture ----------------------------------------------------------------------------------------------------------------

def test_argument_statuses(ctx, fr):
    import torch
    dev = torch.device("cuda", 0)
    pyr = fr.dev("1", 2)
    d_pts = torch.zeros((8, 2), dtype=torch.float32, device=dev)
    d_desc = torch.zeros((8, 32), dtype=torch.uint8, device=dev)
    d_xy = torch.zeros((8, 2), dtype=torch.float32, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def plain(pyr=pyr, pts=d_pts.data_ptr(), cap=8, prm=None, desc=d_desc.data_ptr()):
        ctx.describe_points_dev(pyr, pts, None, cap, prm or api.describe_params(), desc)

    def gather(pyr=pyr, pts=d_pts.data_ptr(), cap=8, prm=None, desc=d_desc.data_ptr(), xy=d_xy.data_ptr(), cnt=d_cnt.data_ptr()):
        ctx.describe_points_gather_dev(pyr, pts, None, cap, prm or api.describe_params(), xy, desc, cnt)

    class NoPyramid:
        _h = None

    flags, res0, res1 = api.describe_params(0, 2), api.describe_params(), api.describe_params()
    res0.reserved[0] = 1
    res1.reserved[1] = 1
    bad = [dict(prm=api.describe_params(3)), dict(prm=api.describe_params(-1)), dict(prm=api.describe_params(8)), dict(prm=flags),
           dict(prm=api.describe_params(0, 3)), dict(prm=res0), dict(prm=res1), dict(cap=-1), dict(pts=None), dict(desc=None),
           dict(pyr=NoPyramid())]
    for f in (plain, gather):
        for kw in bad:
            with pytest.raises(api.PmError) as e:
                f(**kw)
            assert e.value.status == api.PM_E_INVALID, (f.__name__, kw)
        with pytest.raises(api.PmError) as e:
            f(cap=0)
        assert e.value.status == api.PM_E_UNSUPPORTED
    for kw in (dict(xy=None), dict(cnt=None)):
        with pytest.raises(api.PmError) as e:
            gather(**kw)
        assert e.value.status == api.PM_E_INVALID, kw
    # the host form
    img = fr.img["1"]
    pts = fr.corners[:8]
    for prm in (api.describe_params(-1), api.describe_params(8), flags, res0, api.describe_params(6)):      # 496 x 330 has 5 levels
        with pytest.raises(api.PmError) as e:
            ctx.describe_points(img, pts, prm)
        assert e.value.status == api.PM_E_INVALID
    with pytest.raises(api.PmError) as e:
        ctx.describe_points(img, np.zeros((0, 2), np.float32))
    assert e.value.status == api.PM_E_UNSUPPORTED
    with pytest.raises(api.PmError) as e:
        ctx.describe_points(np.zeros((12, 40), np.uint8), pts)
    assert e.value.status == api.PM_E_UNSUPPORTED
    plain()
    gather()
    ctx.synchronize()


@pytest.mark.filterwarnings("ignore:The CUDA Graph is empty")
def test_capturing_stream_is_refused(fr):
    """Refused first thing with PM_E_UNSUPPORTED, on a context that has never described (so the table upload would be next):
    nothing is allocated, synchronised or launched, and the context keeps working afterwards."""
    import torch
    import points_matching_amd as pm
    dev = torch.device("cuda", 0)
    img = fr.img["1"]
    h, w = img.shape
    st = torch.cuda.Stream(device=dev)
    prev = torch.cuda.current_stream(dev)
    torch.cuda.set_stream(st)
    c = pm.Context(0)
    c.set_stream(st.cuda_stream)
    pyr = None
    bufs = None
    try:
        d_img = torch.from_numpy(img).to(dev)
        d_pts = torch.from_numpy(fr.corners).to(dev)
        d_desc = torch.full((344, 32), PAT, dtype=torch.uint8, device=dev)
        d_xy = torch.full((344, 2), PATTERN_F, dtype=torch.float32, device=dev)
        d_cnt = torch.full((1,), -5, dtype=torch.int32, device=dev)
        bufs = (d_img, d_pts, d_desc, d_xy, d_cnt)
        torch.cuda.synchronize()
        pyr = c.pyramid(w, h, 0).build_dev(d_img.data_ptr())
        torch.cuda.synchronize()
        prm = api.describe_params()
        calls = [lambda: c.describe_points_dev(pyr, d_pts.data_ptr(), None, 344, prm, d_desc.data_ptr()),
                 lambda: c.describe_points_gather_dev(pyr, d_pts.data_ptr(), None, 344, prm, d_xy.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr()),
                 lambda: c.describe_points(img, fr.corners, prm)]
        gc.collect()
        for call in calls:
            g = torch.cuda.CUDAGraph()
            with pytest.raises(pm.PmError) as err:
                with torch.cuda.graph(g, stream=st, capture_error_mode="relaxed"):
                    call()
            assert err.value.status == api.PM_E_UNSUPPORTED and "capturing" in str(err.value)
            del g, err
            torch.cuda.set_stream(st)
            torch.cuda.synchronize()
        assert (d_desc == PAT).all() and (d_xy == PATTERN_F).all() and int(d_cnt.item()) == -5
        calls[0]()
        torch.cuda.synchronize()
        assert (d_desc.cpu().numpy() == fr.ref("1", 0, fr.corners)[0]).all()
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(prev)
        if pyr is not None:
            pyr.close()
        c.close()
        del bufs
        gc.collect()
