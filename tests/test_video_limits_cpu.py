"""CPU: the inputs of tests/test_video_limits_gpu.py (tests/video_limit_cases.py), run through the restatements alone
(tests/lk_ref.c, tests/corner_ref.c, which tests/test_track_lk_cpu.py and tests/test_corners_cpu.py pin against numpy).
Each test asserts the condition that makes a GPU case worth running: that the level shapes are the ones at the tile edges,
that a border pair is accepted on one side of the edge and refused on the other, that a weight really comes out 0, -1 or 16384,
that a compaction pattern keeps the rows it is named after, that a dot image yields exactly the candidate count named.  The GPU
file runs the very same arrays, so it cannot pass on inputs that miss the path."""
import numpy as np
import pytest

import corner_ref as K
import lk_ref as R
import video_limit_cases as V


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- S61 -------------------------------------------------------------------------------------------------------------------

def test_pyramid_level_shapes_are_at_the_tile_edges():
    """The 32 x 8 output tile of lk_pyr_down: level-1 widths of 32, 33, 64 and 65 and heights of 16, 17 and 24, from odd and even
    inputs, and the same edges transposed."""
    for i, (shape, level1) in enumerate(zip(V.PYR_SHAPES, V.PYR_LEVEL1)):
        p = V.pyramid("pyr%d" % i, 7)
        assert p.n == 2 and p.levels[0].shape == shape and p.levels[1].shape == level1, shape
    assert {s[1] for s in V.PYR_LEVEL1[:6]} == {32, 33, 64, 65} and {s[0] for s in V.PYR_LEVEL1[:6]} == {16, 17, 24}
    assert {s[0] for s in V.PYR_LEVEL1[6:]} == {32, 33}
    for h, w in V.PYR_SHAPES[:4]:                                # an odd and an even input for each of the widths 32 and 33
        assert (w + 1) // 2 in (32, 33) and (h + 1) // 2 in (16, 17)
    assert sorted(w % 2 for h, w in V.PYR_SHAPES[:4]) == [0, 0, 1, 1]
    for name in ("all255", "columns"):
        p = V.pyramid(name, 7)
        assert p.n == 2 and p.levels[0].shape == (33, 65) and p.levels[1].shape == (17, 33)
    assert (V.pyramid("all255", 7).levels[1] == 255).all()       # (256 * 255 + 128) >> 8: no carry out of the byte
    # reflect-101 keeps the parity of a column, so every window weighs 8 columns of 0 and 8 of 255, at the edges too:
    # (16 * 8 * 255 + 128) >> 8 == 128; a reflection that repeats the edge column gives another value there
    assert (V.pyramid("columns", 7).levels[1] == 128).all()


def test_pyramid_of_1921_has_8_levels_and_of_1920_has_7():
    p = V.pyramid("big", 7)
    assert p.n == 8 and [l.shape for l in p.levels] == [(s, s) for s in (1921, 961, 481, 241, 121, 61, 31, 16)]
    q = V.pyramid("big1920", 7)
    assert q.n == 7 and [l.shape for l in q.levels] == [(s, s) for s in (1920, 960, 480, 240, 120, 60, 30)]
    assert all(l.min() < l.max() for l in p.levels)


def test_big_points_join_at_level_7_or_below_it():
    """At r = 6 the first six points have a template on level 7 and the last six do not, but have one from a lower level down;
    every point is tracked, to within a tenth of a pixel of the true shift."""
    pa = V.pyramid("big", 7)
    for case in V.big_cases():
        r = case.prm[0]
        top = []
        for x, y in case.pts:
            codes = [R.template(pa.levels[l], float(np.float32(x) * np.float32(1.0 / (1 << l))), float(np.float32(y) * np.float32(1.0 / (1 << l))), r,
                                case.prm[4])[0] for l in range(8)]
            top.append(max(l for l in range(8) if codes[l] == 0))
        if r == 6:
            assert top[:6] == [7] * 6 and all(t < 7 for t in top[6:]) and min(top) >= 3, top
        out, status, _, _ = case.want()
        assert (status == 1).all()
        assert np.abs(out - case.pts - np.array(V.BIG_SHIFT, np.float32)).max() <= 0.1


# ---- S62: borders -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in V.border_cases() if c.note["level"] == 0], ids=repr)
def test_border_pairs_at_level_0(case):
    """Left, top, right, bottom: the last accepted origin has status 1, the first refused status 2, for the template and for the
    search window; accepted and refused lie one float32 apart."""
    status = case.want()[1]
    assert status.tolist() == [1, 2] * 4
    moved = case.pts if case.note["kind"] == "template" else case.init
    for i in range(0, 8, 2):
        d = np.abs(bits(moved[i]).astype(np.int64) - bits(moved[i + 1]).astype(np.int64))
        assert sorted(d.tolist()) == [0, 1]


@pytest.mark.parametrize("case", [c for c in V.border_cases() if c.note["level"] == 1], ids=repr)
def test_border_pairs_at_level_1(case):
    """The same pairs on level 1: the window of the accepted point lies inside level 1 and that of the refused one does not.  The
    refusal does not show in the status (level 0 tracks both), but in the bits: for the template pairs the refused point comes
    out as in a run without level 1, the accepted point does not."""
    pa, pb = case.pyramids()
    r, lvl = case.prm[0], pa.levels[1]
    assert pa.n == 2 and lvl.shape == (49, 66)
    moved = case.pts if case.note["kind"] == "template" else case.init
    for i, (x, y) in enumerate(moved):
        x1, y1 = float(np.float32(x) * np.float32(0.5)), float(np.float32(y) * np.float32(0.5))
        if case.note["kind"] == "template":
            fits = R.template(lvl, x1, y1, r, case.prm[4])[0] == 0
        else:
            fits = R.sample_window(lvl, float(np.float32(x1) - np.float32(r)), float(np.float32(y1) - np.float32(r)), 2 * r + 1) is not None
            assert R.template(lvl, float(case.pts[i, 0]) * 0.5, float(case.pts[i, 1]) * 0.5, r, case.prm[4])[0] == 0
        assert fits == (i % 2 == 0), (case.tag, i)
    out, status, _, _ = case.want()
    assert (status == 1).all()
    if case.note["kind"] == "template":
        prm0 = list(case.prm)
        prm0[1] = 0
        out0, status0, _, _ = R.track(pa, pb, case.pts, R.params(*prm0))
        assert (status0 == 1).all()
        same = (bits(out) == bits(out0)).all(axis=1)
        assert same.tolist() == [False, True] * 4


# ---- S62: weights -------------------------------------------------------------------------------------------------------------

def test_weight_points_cover_every_class():
    found = V.weight_points()
    assert set(found) == set(V.WEIGHT_CLASSES)
    w = {name: [int(v) for v in V.weights_of(*found[name])] for name in found}
    assert w["w11 == 0"][3] == 0 and w["w11 == -1"][3] == -1 and w["w00 == 16384"][0] == 16384 and w["all 4096"] == [4096] * 4
    assert w["w11 == 0, w01 and w10 > 0"][3] == 0 and min(w["w11 == 0, w01 and w10 > 0"][1:3]) > 0
    x, y = found["w00 == 16384, a and b not 0"]
    assert w["w00 == 16384, a and b not 0"] == [16384, 0, 0, 0] and x != np.floor(x) and y != np.floor(y)
    for case in V.weight_cases():
        pts = case.pts[:len(found)]
        assert sorted(map(tuple, pts.tolist())) == sorted((float(x), float(y)) for x, y in found.values())
        assert (case.want()[1] == 1).all()
    # the band of neighbours: every w11 from -1 to 1 and further occurs among its templates
    w11 = {int(V.weights_of(x, y)[3]) for x, y in V.weight_cases()[0].pts}
    assert {-1, 0, 1} <= w11


# ---- S63 - S66 ----------------------------------------------------------------------------------------------------------------

def test_every_radius_tracks():
    cases = V.radius_cases()
    assert sorted({c.prm[0] for c in cases}) == list(range(2, 16)) and all(c.pts.shape == (16, 2) and c.prm[2] == 30 and c.prm[5] > 0 for c in cases)
    for case in cases:
        out, status, err, fb = case.want()
        assert (status == 1).sum() >= 12 and set(status.tolist()) <= {1, 4}, case.tag
        ok = status == 1
        assert np.abs(out[ok] - case.pts[ok] - np.array(V.SMALL_SHIFT, np.float32)).max() <= 0.5 and (fb[ok] >= 0).all()


def test_max_level_and_level_count_apart():
    cases = V.level_cases()
    assert [(c.pyramids()[0].n, c.prm[1]) for c in cases] == [(3, 0), (3, 1), (3, 2), (1, 7)]
    outs = [c.want() for c in cases]
    assert all((o[1] == 1).all() for o in outs)
    assert bits(outs[0][0]).tobytes() == bits(outs[3][0]).tobytes()             # top = 0 either way
    assert len({bits(o[0]).tobytes() for o in outs[:3]}) == 3                    # each further level leaves a trace


def test_eps_cases():
    c = V.eps_cases()
    zero, large, usual, one = c["zero"].want(), c["large"].want(), c["usual"].want(), c["one"].want()
    assert c["zero"].prm[2] == 100 and c["zero"].prm[3] == 0.0
    assert all((w[1] == 1).all() for w in (zero, large, usual, one))
    assert bits(large[0]).tobytes() == bits(one[0]).tobytes()                    # eps 1e3 stops after the first iteration
    assert (bits(large[0]) != bits(usual[0])).any(axis=1).all()                  # and short of where eps 0.01 ends
    assert np.abs(zero[0] - c["zero"].pts - np.array(V.SMALL_SHIFT, np.float32)).max() <= 0.1
    out, status, err, fb = c["identical"].want()
    assert (status == 1).all() and bits(out).tobytes() == bits(c["identical"].pts).tobytes()      # the first step is exactly zero
    assert (err == 0).all() and (fb == 0).all()


def test_coordinates_at_the_range_test():
    for case in V.coordinate_cases():
        out, status, err, fb = case.want()
        assert status[0] == 1 and (status[1:] == 2).all(), case.tag
    vals = V.edge_values(3)
    assert vals[0] == 1e6 and vals[1] == -1e6 and vals[2] > 1e6 and np.isinf(vals[12]) and np.isnan(vals[14])
    # the template origin of value 4 is exactly 1e6 (the range test passes it, the window test refuses it), of value 5 beyond it
    assert np.float32(vals[4]) - np.float32(4) == np.float32(1e6) and np.float32(vals[5]) - np.float32(4) > np.float32(1e6)
    assert np.float32(vals[8]) - np.float32(3) == np.float32(1e6) and np.float32(vals[10]) - np.float32(3) == np.float32(-1e6)
    pts = V.coordinate_cases()[0].pts
    assert pts.shape == (31, 2) and np.isfinite(pts[:, 0]).sum() == 28 and np.isfinite(pts[:, 1]).sum() == 28


# ---- S66: compaction ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", V.COMPACT_CAPS)
def test_compaction_patterns(cap):
    for pattern in V.COMPACT_PATTERNS:
        case = V.compact_case(cap, pattern)
        status = case.want()[1]
        assert case.pts.shape == (cap, 2) and set(status.tolist()) <= {1, 2}
        keep = status == 1
        assert (keep == case.keep).all()
        first, rest = int(keep[:1024].sum()), int(keep[1024:].sum())
        if pattern == "none first":
            assert first == 0 and (rest > 0) == (cap > 1024)
        elif pattern == "all first":
            assert first == min(cap, 1024) and (rest > 0) == (cap > 1024)
        else:
            assert 0 < first < min(cap, 1024) and keep[1023:1025].all()
        if cap > 1025:
            assert 0 < rest < cap - 1024
    assert [rows for _, rows in V.compact_counts(cap)] == [cap, min(cap, 1024), min(cap, 1025), cap - 1]


# ---- S67 - S70 ------------------------------------------------------------------------------------------------------------------

def test_tile_shapes():
    """V exactly one 64 x 16 tile wide or high, one pixel more, two tiles, two and a pixel, at r = 15 and r = 1."""
    r = 15
    shapes = V.tile_shapes(r)
    assert {w - 2 * r - 3 for w, h in shapes} == {1, 64, 65, 128, 129} and {h - 2 * r - 3 for w, h in shapes} == {1, 16, 17, 33}
    assert {(w - 5, h - 5) for w, h in V.tile_shapes(1)} >= {(64, 16), (65, 17), (128, 11), (129, 17), (64, 33)}
    for case in V.tile_cases():
        img = V.corner_image(case.image)
        assert min(img.shape) >= 16
        xy, score, n = case.want()
        assert n == xy.shape[0] >= 1, case.tag                    # the whole ranked list


def check_dots(img, r):
    """The dot rule: single pixels above a ground of 40, r + 4 from every border, 6 px at least from the next dot."""
    ys, xs = np.nonzero(img != V.GROUND)
    assert set(img[ys, xs].tolist()) <= {V.DOT, V.WEAK_DOT}
    assert xs.min() >= r + 4 and ys.min() >= r + 4 and xs.max() <= img.shape[1] - 1 - (r + 4) and ys.max() <= img.shape[0] - 1 - (r + 4)
    pos = np.stack([xs, ys], 1).astype(np.int64)
    order = np.lexsort((pos[:, 0], pos[:, 1]))
    pos = pos[order]
    near = np.abs(pos[1:] - pos[:-1]).max(axis=1)                 # scan-order neighbours; rows are PITCH apart as well
    assert near.min() >= 6 and min(img.shape) >= 16
    return pos


@pytest.mark.parametrize("case", V.rank_cases() + V.select_cases(), ids=repr)
def test_dot_images_yield_the_counts_named(case):
    img = V.corner_image(case.image)
    pos = check_dots(img, case.r)
    xy, score, n = case.want()
    assert n == case.candidates == pos.shape[0]
    if case.rows is not None:
        assert xy.shape[0] == case.rows
    one_amplitude = len(set(img[img != V.GROUND].tolist())) == 1
    if one_amplitude:
        assert len(set(bits(score).tolist())) == 1                # one score: rank order is scan order
    if case.min_dist == 0:
        assert (xy == pos[:xy.shape[0]]).all()                    # every candidate, in scan order, up to max_corners


def test_selection_results_are_the_ones_the_alternation_predicts():
    by_tag = {c.tag: c for c in V.select_cases()}
    m = 5                                                         # the first dot's column and, on the grid, row
    xy = by_tag["1025 dots, min_dist 8.5"].want()[0]
    assert xy.shape[0] == 513 and (xy[:, 0] == m + 16 * np.arange(513)).all()
    xy = by_tag["1024 dots from the second position, min_dist 8.5"].want()[0]
    assert xy.shape[0] == 512 and (xy[:, 0] == m + 8 + 16 * np.arange(512)).all()
    xy = by_tag["1025 dots, min_dist 16.5"].want()[0]
    assert xy.shape[0] == 342 and (xy[:, 0] == m + 24 * np.arange(342)).all()
    xy = by_tag["1025 dots, min_dist 8.5, max_corners 256"].want()[0]
    assert xy.shape[0] == 256 and xy[-1, 0] == m + 16 * 255       # rank 510: the limit falls on the last accepted rank of chunk 0
    xy, score, n = by_tag["600 strong + 600 weak dots, min_dist 8.5"].want()
    assert n == 1200 and xy.shape[0] == 600 and (xy[:, 0] == m + 16 * np.arange(600)).all() and len(set(bits(score).tolist())) == 1
    c = by_tag["600 strong + 600 weak dots, min_dist 8.5"]
    assert K.detect(V.corner_image(c.image), 1, c.min_eig, 0.0, 0.0)[0].shape[0] == 1200 and 512 < 600 < 1024   # the classes meet in chunk 2
    xy = by_tag["33 x 32 grid, min_dist 8.5"].want()[0]
    i, j = (xy[:, 0] - m) / 8, (xy[:, 1] - m) / 8
    assert xy.shape[0] == 528 and ((i + j) % 2 == 0).all()         # the checkerboard
    keep = V.grid_keep()
    img = V.corner_image("grid")
    assert keep.shape == (10, 2) and (img[keep[:, 1].astype(int), keep[:, 0].astype(int)] == V.DOT).all()
    xyk = by_tag["33 x 32 grid, min_dist 8.5, keep points"].want()[0]
    assert 0 < xyk.shape[0] < 528 and not any((xyk == k).all(axis=1).any() for k in keep)


def test_capacity_edge_image():
    """The 513-dot image of the capacity cases: n == capacity must pass, n == capacity + 1 must overflow."""
    assert V.rank_cases()[5].candidates == 513 and V.rank_cases()[5].want()[2] == 513
