"""GPU parity of the u8 route's prep kernel (knn_l2_prep8: packed converts, convert-back premise check, dot4 norms, DPP
row sums) at the shapes and values where it can go wrong: pad rows, partial last workgroups of the query and of the train
half of its grid, the block where the two halves meet, column guards (dim < 128), every rows-per-workgroup form, and the
edges of the premise "every element is an integer in [0, 255]".

Every comparison is exact: trainIdx and the distance bits against oracle.pm_oracle.bf_knn_l2 on the same arrays, through
pm_bf_knn_l2_f32_dev and pm_bf_knn_l2_ratio_dev with PM_KNN_HINT_U8.

Expected knn_stats of a wrong hint: knn_l2_refine8 (which this file's kernel only feeds) writes route 3, and for EVERY live
query of a call whose epoch flag is up it counts one re-scan and sets the flag word — so route 3, nonfinite 1,
rescans == nq, whatever the poison is and wherever it sits.  Clean data (-0.0 and 255 are clean) give route 3, nonfinite 0,
rescans 0 on rows without near ties (128 random bytes)."""
import numpy as np
import pytest

import points_matching_amd as pm
from points_matching_amd.api import (PM_KNN_HINT_U8, PM_OPT_FILTER_FUSION, PM_OPT_KNN_PREP_ROWS, PM_OPT_KNN_RING,
                                     PM_OPT_KNN_U8_GROUP)
from util import assert_matches_equal

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (15, 17), (16, 16), (63, 65), (257, 129), (300, 1000)]
DIMS = [4, 64, 100, 128]
PREP_ROWS = [1, 2, 3]                  # 64, 16 (the default's value) and 32 rows per workgroup
RATIO = 0.8
POISON = [0.5, 2.5, 254.5, -1.0, -0.0, 255.0, 256.0, 1e9, float("inf"), float("nan")]
CLEAN = (-0.0, 255.0)


def _bytes(rng, n, dim):
    return rng.integers(0, 256, (n, dim)).astype(np.float32)


def _knn_dev(ctx, q, t, k=2):
    import torch
    dev = torch.device("cuda", 0)
    d_q, d_t = torch.from_numpy(q).to(dev), torch.from_numpy(t).to(dev)
    d_out = torch.zeros((q.shape[0], k, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.knn_diag_enable(True)
    try:
        ctx.bf_knn_l2_dev(d_q.data_ptr(), q.shape[0], d_t.data_ptr(), t.shape[0], q.shape[1], k, d_out.data_ptr(), PM_KNN_HINT_U8)
        ctx.synchronize()
        st = ctx.knn_stats()
    finally:
        ctx.knn_diag_enable(False)
    return d_out.cpu().numpy().view(pm.MATCH_DTYPE).reshape(q.shape[0], k), st


def _ratio_dev(ctx, q, t, kp1, kp2):
    """-> (knn records, surviving matches, their points)"""
    import torch
    dev = torch.device("cuda", 0)
    nq, nt = q.shape[0], t.shape[0]
    d_q, d_t, d_kp1, d_kp2 = (torch.from_numpy(a).to(dev) for a in (q, t, kp1, kp2))
    d_knn = torch.zeros((nq, 2, 4), dtype=torch.int32, device=dev)
    d_good = torch.full((nq, 4), -7, dtype=torch.int32, device=dev)
    d_xy1 = torch.full((nq, 2), -1.0, dtype=torch.float32, device=dev)
    d_xy2 = torch.full((nq, 2), -1.0, dtype=torch.float32, device=dev)
    d_n = torch.full((1,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.bf_knn_l2_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, q.shape[1], PM_KNN_HINT_U8, RATIO, d_kp1.data_ptr(),
                            d_kp2.data_ptr(), d_knn.data_ptr(), d_good.data_ptr(), d_xy1.data_ptr(), d_xy2.data_ptr(), d_n.data_ptr())
    ctx.synchronize()
    n = int(d_n.item())
    return (d_knn.cpu().numpy().view(pm.MATCH_DTYPE).reshape(nq, 2), d_good.cpu().numpy().view(pm.MATCH_DTYPE).reshape(-1)[:n],
            d_xy1.cpu().numpy()[:n], d_xy2.cpu().numpy()[:n])


@pytest.fixture(scope="module")
def shape_cases(oracle):
    """One seeded pair of arrays per (shape, dim) with its oracle records, shared by every form of the kernel."""
    out = {}
    for nq, nt in SHAPES:
        for dim in DIMS:
            rng = np.random.default_rng(100000 * nq + 100 * nt + dim)
            q, t = _bytes(rng, nq, dim), _bytes(rng, nt, dim)
            m = min(nq, nt) // 3
            q[:m] = np.clip(t[nt - m:] + rng.integers(-2, 3, (m, dim)), 0, 255)       # matches that pass the ratio test
            kp1 = rng.uniform(0, 900, (nq, 2)).astype(np.float32)
            kp2 = rng.uniform(0, 900, (nt, 2)).astype(np.float32)
            want = oracle.bf_knn_l2(q, t, 2, nthreads=8)
            out[nq, nt, dim] = (q, t, kp1, kp2, want, oracle.filter_ratio(want, RATIO))
    return out


@pytest.mark.parametrize("rows", PREP_ROWS)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("nq,nt", SHAPES)
def test_shapes(ctx, shape_cases, nq, nt, dim, rows):
    q, t, kp1, kp2, want, good = shape_cases[nq, nt, dim]
    what = "%d x %d x %d, PREP_ROWS %d" % (nq, nt, dim, rows)
    try:
        ctx.set_option(PM_OPT_KNN_PREP_ROWS, rows)
        got, st = _knn_dev(ctx, q, t)
        assert_matches_equal(got, want, what + ", pm_bf_knn_l2_f32_dev")
        assert st["route"] == 3 and st["nonfinite"] == 0, (what, st)
        for fusion in (0, 1):                                       # the default form at this size, and two launches
            ctx.set_option(PM_OPT_FILTER_FUSION, fusion)
            knn, kept, xy1, xy2 = _ratio_dev(ctx, q, t, kp1, kp2)
            assert_matches_equal(knn, want, what + ", pm_bf_knn_l2_ratio_dev records")
            assert kept.size == good.size, (what, kept.size, good.size)
            assert_matches_equal(kept, good, what + ", pm_bf_knn_l2_ratio_dev survivors")
            assert (xy1 == kp1[good["queryIdx"]]).all() and (xy2 == kp2[good["trainIdx"]]).all(), what
    finally:
        ctx.set_option(PM_OPT_FILTER_FUSION, 0)
        ctx.set_option(PM_OPT_KNN_PREP_ROWS, 0)


def _placements(nq, nt, dim):
    for side, n in (("q", nq), ("t", nt)):
        for r in (0, n - 1):
            for c in (0, dim - 1):
                yield side, r, c


@pytest.fixture(scope="module")
def edge_base():
    """63 x 65 rows (pad rows, partial workgroups on both halves); dim 100 has a last live column inside a guarded dword
    row, dim 128 runs the unguarded form."""
    out = {}
    for dim in (100, 128):
        rng = np.random.default_rng(7000 + dim)
        out[dim] = (_bytes(rng, 63, dim), _bytes(rng, 65, dim))
    return out


@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("dim", [100, 128])
@pytest.mark.parametrize("poison", POISON, ids=[repr(p) for p in POISON])
def test_premise_edges(ctx, oracle, edge_base, poison, dim, rows):
    q0, t0 = edge_base[dim]
    nq, nt = q0.shape[0], t0.shape[0]
    try:
        ctx.set_option(PM_OPT_KNN_PREP_ROWS, rows)
        for side, r, c in _placements(nq, nt, dim):
            q, t = q0.copy(), t0.copy()
            (q if side == "q" else t)[r, c] = np.float32(poison)
            want = oracle.bf_knn_l2(q, t, 2, nthreads=8)
            got, st = _knn_dev(ctx, q, t)
            what = "poison %r at %s[%d, %d], dim %d, PREP_ROWS %d" % (poison, side, r, c, dim, rows)
            assert_matches_equal(got, want, what)
            if poison in CLEAN:
                assert st == {"route": 3, "nonfinite": 0, "rescans": 0}, (what, st)
            else:
                assert st == {"route": 3, "nonfinite": 1, "rescans": nq}, (what, st)
    finally:
        ctx.set_option(PM_OPT_KNN_PREP_ROWS, 0)


def test_a_clean_call_after_a_poisoned_one(ctx, oracle, edge_base):
    """The flag is epoch-tagged: a wrong hint leaves nothing behind for the next call."""
    q, t = edge_base[128]
    bad = t.copy()
    bad[64, 127] = 254.5
    got, st = _knn_dev(ctx, q, bad)
    assert_matches_equal(got, oracle.bf_knn_l2(q, bad, 2, nthreads=8), "poisoned call")
    assert st["nonfinite"] == 1, st
    got, st = _knn_dev(ctx, q, t)
    assert_matches_equal(got, oracle.bf_knn_l2(q, t, 2, nthreads=8), "clean call after it")
    assert st == {"route": 3, "nonfinite": 0, "rescans": 0}, st


def test_norms_and_seeds_through_the_matcher(ctx, oracle):
    """64 x 64 x 128.  The refinement's distances are ||q'||^2 + ||t'||^2 - 2 q'.t' with both norms read from what the
    prep kernel wrote, and the coarse pass ranks on its seeds (the seed array on the narrow forms, the pad slots of the
    144-byte train rows on the wide form): a wrong norm moves a distance, a wrong seed loses a neighbour.  Rows of
    extreme norm (all 0, all 255, all 128) sit next to the random ones."""
    rng = np.random.default_rng(64)
    q, t = _bytes(rng, 64, 128), _bytes(rng, 64, 128)
    q[0], q[1], q[2] = 0.0, 255.0, 128.0
    t[0], t[1], t[2], t[63] = 255.0, 0.0, 128.0, 127.0
    want = oracle.bf_knn_l2(q, t, 2, nthreads=8)
    results = []
    try:
        for ring in (1, 5):                                         # narrow train rows + seed array / wide rows with seed slots
            for group in (0, 1, 2, 3):
                for rows in (0, 1, 3):
                    ctx.set_option(PM_OPT_KNN_RING, ring)
                    ctx.set_option(PM_OPT_KNN_U8_GROUP, group)
                    ctx.set_option(PM_OPT_KNN_PREP_ROWS, rows)
                    got, st = _knn_dev(ctx, q, t)
                    assert_matches_equal(got, want, "RING %d U8_GROUP %d PREP_ROWS %d" % (ring, group, rows))
                    assert st["route"] == 3 and st["nonfinite"] == 0, st
                    results.append(got)
    finally:
        ctx.set_option(PM_OPT_KNN_RING, 0)
        ctx.set_option(PM_OPT_KNN_U8_GROUP, 0)
        ctx.set_option(PM_OPT_KNN_PREP_ROWS, 0)
    for got in results[1:]:
        assert_matches_equal(got, results[0], "forms agree")
