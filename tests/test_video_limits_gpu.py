"""GPU: the video front end at its limits: lk_pyr_down, lk_track, lk_compact (csrc/track_lk.hip, SPEC S61-S66) and
corner_extrema, corner_rank, corner_select (csrc/corners.hip, S67-S70) at the structural edges of the kernels: level shapes at
the pyramid tile, eight levels, the last accepted and the first refused window origin on every side, weights of 0, -1 and
16384, every radius, level counts and max_level apart, eps 0 and eps 1e3, coordinates at the range test, compactions at the
chunk of 1024, valid regions at the corner tile, candidate counts at the rank block, the capacity and the selection chunk, and
selections whose conflicts chain through a whole chunk and across its end.

The inputs come from tests/video_limit_cases.py and the reference is the plain-C restatement (tests/lk_ref.c,
tests/corner_ref.c); tests/test_video_limits_cpu.py asserts on the CPU that each input reaches the edge it is named after.
Every comparison is bit for bit, outputs are pre-filled with a pattern, and everything behind the count must still hold it
(the helpers of tests/test_track_lk_gpu.py and tests/test_corners_gpu.py, imported unchanged)."""
import gc

import numpy as np
import pytest

import corner_ref as K
import video_limit_cases as V
from points_matching_amd import api
from test_corners_gpu import PATTERN_F, assert_rows, bits, dev_corners, dev_replenish
from test_track_lk_gpu import assert_equal, check_gather, dev_gather, dev_track

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    import points_matching_amd as pm
    c = pm.Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()
    gc.collect()


class Device:
    """The device pyramids of the frames and corner images of video_limit_cases, each built once."""

    def __init__(self, ctx):
        self.ctx, self._pyr = ctx, {}

    def _build(self, key, img, max_level):
        import torch
        if key not in self._pyr:
            d_img = torch.from_numpy(img).to("cuda:0")
            torch.cuda.synchronize()
            h, w = img.shape
            p = self.ctx.pyramid(w, h, max_level).build_dev(d_img.data_ptr())
            self.ctx.synchronize()
            self._pyr[key] = p
        return self._pyr[key]

    def frame(self, name, max_level):
        return self._build(("frame", name, max_level), V.frame(name), max_level)

    def corner(self, name):
        return self._build(("corner", name), V.corner_image(name), 0)

    def close(self):
        for p in self._pyr.values():
            p.close()


@pytest.fixture(scope="module")
def dev(ctx):
    d = Device(ctx)
    yield d
    ctx.synchronize()
    d.close()


def assert_levels(tag, p, want):
    assert p.levels == want.n, tag
    for l in range(want.n):
        got = p.level(l)
        assert got.shape == want.levels[l].shape and (got == want.levels[l]).all(), (tag, l)


def run_track(ctx, dev, case):
    pa, pb = dev.frame(case.a, case.built), dev.frame(case.b, case.built)
    assert pa.levels == case.pyramids()[0].n
    got = dev_track(ctx, pa, pb, case.pts, api.lk_params(*case.prm), init=case.init)
    assert_equal(case.tag, got, case.want())
    return got


# ---- S61 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", V.PYR_CASES)
def test_pyramid_at_the_tile_edges(ctx, name):
    """Level-1 widths of 32, 33, 64, 65 and heights of 16, 17, 24 (the 32 x 8 tile of lk_pyr_down), from odd and even inputs, with
    a row stride; an all-255 image and alternating columns of 0 and 255."""
    import torch
    img = V.frame(name)
    h, w = img.shape
    d_img = torch.from_numpy(V.padded(img)).to("cuda:0")
    torch.cuda.synchronize()
    p = ctx.pyramid(w, h, 7).build_dev(d_img.data_ptr(), w + V.PYR_PAD)
    try:
        assert_levels(name, p, V.pyramid(name, 7))
    finally:
        p.close()


def test_eight_levels_and_tracking_through_them(ctx, dev):
    """1921 x 1921: all 8 levels of PyrDesc and pm_pyramid, the last 16 x 16; a dozen points from level 7, or from the highest
    level their template fits, down to level 0."""
    for name in ("big", "bigroll"):
        assert_levels(name, dev.frame(name, 7), V.pyramid(name, 7))
    assert dev.frame("big", 7).levels == 8
    for case in V.big_cases():
        run_track(ctx, dev, case)


def test_seven_levels_of_1920(dev):
    assert_levels("big1920", dev.frame("big1920", 7), V.pyramid("big1920", 7))
    assert dev.frame("big1920", 7).levels == 7


# ---- S62 - S66: tracking -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", range(2, 16))
def test_every_radius(ctx, dev, r):
    """The divisions by 2r + 1 and 2r + 3 are multiplications by a rounded-up reciprocal: every radius runs once."""
    cases = [c for c in V.radius_cases() if c.prm[0] == r]
    assert len(cases) == 2
    for case in cases:
        run_track(ctx, dev, case)


@pytest.mark.parametrize("case", V.border_cases(), ids=repr)
def test_border_pairs(ctx, dev, case):
    """The last accepted and the first refused window origin on all four sides, template and search window, levels 0 and 1."""
    got = run_track(ctx, dev, case)
    assert got[1].tolist() == ([1, 2] * 4 if case.note["level"] == 0 else [1] * 8)


def test_weights(ctx, dev):
    for case in V.weight_cases():
        run_track(ctx, dev, case)


def test_max_level_and_level_count_apart(ctx, dev):
    for case in V.level_cases():
        run_track(ctx, dev, case)


def test_eps_and_identical_frames(ctx, dev):
    cases = V.eps_cases()
    for case in cases.values():
        got = run_track(ctx, dev, case)
    assert (bits(got[0]) == bits(cases["identical"].pts)).all()


def test_coordinates_at_the_range_test(ctx, dev):
    for case in V.coordinate_cases():
        got = run_track(ctx, dev, case)
        assert got[1][0] == 1 and (got[1][1:] == 2).all()


# ---- S66: compaction ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", V.COMPACT_CAPS)
def test_compaction_at_the_chunk(ctx, dev, cap):
    """Caps around one and two chunks of 1024; a first chunk that keeps nothing, everything, a mix; device counts that end on the
    chunk edge and one behind it; with the optional outputs and without (rows in the context's arena)."""
    pyr = dev.frame("n64", 0)
    for pattern in V.COMPACT_PATTERNS:
        case = V.compact_case(cap, pattern)
        for n, rows in V.compact_counts(cap):
            for full in (True, False):
                got = dev_gather(ctx, pyr, pyr, case.pts, api.lk_params(*case.prm), n, full)
                check_gather("%s, count %s, full %s" % (case.tag, n, full), got, case.pts, case.want(), rows, full)


def test_compaction_arena_grows_on_a_fresh_context(dev):
    """Without the optional outputs the rows live in the context's arena: a small cap first, then one that needs a larger arena."""
    import torch
    import points_matching_amd as pm
    c = pm.Context(0)
    pyr = None
    try:
        img = V.frame("n64")
        d_img = torch.from_numpy(img).to("cuda:0")
        torch.cuda.synchronize()
        pyr = c.pyramid(img.shape[1], img.shape[0], 0).build_dev(d_img.data_ptr())
        c.synchronize()
        for cap in (1023, 2049, 1025):
            case = V.compact_case(cap, "mix")
            got = dev_gather(c, pyr, pyr, case.pts, api.lk_params(*case.prm), None, False)
            check_gather("fresh context, " + case.tag, got, case.pts, case.want(), cap, False)
    finally:
        torch.cuda.synchronize()
        if pyr is not None:
            pyr.close()
        c.close()
        gc.collect()


# ---- S67, S68: the tile ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", V.TILE_RADII)
def test_corner_tiles(ctx, dev, r):
    """V one tile of 64 x 16 wide or high, one pixel more, two tiles, two and a pixel; at r = 15 the staged planes are at their
    full 98 x 50.  No floor, no minimum distance: the whole ranked list."""
    cases = [c for c in V.tile_cases() if c.r == r]
    assert len(cases) >= 12
    for case in cases:
        got = dev_corners(ctx, dev.corner(case.image), api.corner_params(r, case.min_eig, 0.0, 0.0), case.max_corners)
        assert_rows(case.tag, got, case.want())


# ---- S69: ranking -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", V.rank_cases(), ids=repr)
def test_ranking_at_the_block_and_the_capacity(ctx, dev, case):
    """Candidate counts around one, two and four blocks of 256 keys: every row comes back in scan order.  With the capacity equal
    to the count the list is complete; one below it the count is -1 and nothing is written."""
    n, pyr = case.candidates, dev.corner(case.image)
    want = case.want()
    assert want[2] == want[0].shape[0] == n
    assert_rows(case.tag, dev_corners(ctx, pyr, api.corner_params(1, case.min_eig, 0.0, 0.0), case.max_corners), want)
    got = dev_corners(ctx, pyr, api.corner_params(1, case.min_eig, 0.0, 0.0, capacity=n), case.max_corners)
    assert_rows(case.tag + ", capacity %d" % n, got, want)
    got = dev_corners(ctx, pyr, api.corner_params(1, case.min_eig, 0.0, 0.0, capacity=n - 1), case.max_corners)
    assert got[0] == -1 and (got[1] == PATTERN_F).all() and (got[2] == PATTERN_F).all()


def test_host_form_retries_past_the_capacity(ctx):
    case = V.rank_cases()[5]
    assert case.candidates == 513
    want = case.want()
    xy, sc = ctx.corners(V.corner_image(case.image), case.max_corners, api.corner_params(1, case.min_eig, 0.0, 0.0, capacity=512))
    assert xy.shape == want[0].shape and (bits(xy) == bits(want[0])).all() and (bits(sc) == bits(want[1])).all()


# ---- S70: selection ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", V.select_cases(), ids=repr)
def test_selection_chains(ctx, dev, case):
    """Equal dots 8 px apart with a minimum distance of 8.5: each rank's fate hangs on the rank before it, through every 64-lane
    word and across the chunk of 512; the limit at a chunk end, beside it and mid-chunk; two classes of dots; a grid."""
    prm = api.corner_params(case.r, case.min_eig, case.quality, case.min_dist)
    got = dev_corners(ctx, dev.corner(case.image), prm, case.max_corners, case.keep)
    assert_rows(case.tag, got, case.want())
    assert case.rows is None or got[0] == case.rows


def test_replenish_on_the_grid(ctx, dev):
    """pm_corners_replenish_dev with ten keep points on dots of the grid: the rows of pm_corners_dev with the same obstacles."""
    keep = V.grid_keep()
    case = [c for c in V.select_cases() if c.keep is not None][0]
    cap = 1100
    want = K.detect(V.corner_image(case.image), case.r, case.min_eig, case.quality, case.min_dist, keep, cap - 10)
    m = want[0].shape[0]
    assert 0 < m < cap - 10 and (bits(want[0]) == bits(case.want()[0])).all()
    prm = api.corner_params(case.r, case.min_eig, case.quality, case.min_dist)
    cnt, new, out, sc = dev_replenish(ctx, dev.corner(case.image), prm, keep, 10, cap, cap)
    assert new == m and cnt == 10 + m
    assert (bits(out[:10]) == bits(keep)).all() and (bits(out[10:10 + m]) == bits(want[0])).all() and (out[10 + m:] == PATTERN_F).all()
    assert (sc[:10] == PATTERN_F).all() and (bits(sc[10:10 + m]) == bits(want[1])).all() and (sc[10 + m:] == PATTERN_F).all()
    # a target that ends the walk inside the second chunk
    room = 300
    want = K.detect(V.corner_image(case.image), case.r, case.min_eig, case.quality, case.min_dist, keep, room)
    cnt, new, out, sc = dev_replenish(ctx, dev.corner(case.image), prm, keep, 10, cap, 10 + room)
    assert new == room == want[0].shape[0] and cnt == 10 + room
    assert (bits(out[10:10 + room]) == bits(want[0])).all() and (out[10 + room:] == PATTERN_F).all()
