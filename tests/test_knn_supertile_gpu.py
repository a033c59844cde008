"""GPU parity of the u8 coarse kernel's super-tiles (PM_OPT_KNN_SUPERTILE: 1, 2 or 4 consecutive 128-row tiles per LDS
buffer and per workgroup barrier of the two-buffer form).  The candidate ids of a tile do not depend on the super-tile
size, so every size must return the oracle's records bit for bit — including splits whose tile count is not a multiple
of the size (partial last super-tiles), train sets that end inside a tile and query counts that end inside a workgroup."""
import numpy as np
import pytest

from points_matching_amd import synth
from points_matching_amd.api import PM_KNN_HINT_U8, PM_OPT_KNN_F16_WAVES, PM_OPT_KNN_RING, PM_OPT_KNN_SUPERTILE
from util import assert_matches_equal

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3)          # option values: 1, 2, 4 tiles per super-tile
TIMERS = {1: "knn_l2_mfma_u8", 2: "knn_l2_mfma_u8_s2", 3: "knn_l2_mfma_u8_s4"}     # the form that ran, by its timer


def _each_size(ctx, fn, waves=0):
    """fn(s) under every super-tile option; each must have launched the coarse form it names, and no other."""
    try:
        ctx.set_option(PM_OPT_KNN_RING, 1)
        ctx.set_option(PM_OPT_KNN_F16_WAVES, waves)
        for s in SIZES:
            ctx.set_option(PM_OPT_KNN_SUPERTILE, s)
            ctx.timing_enable(True)
            ctx.timing_reset()
            fn(s)
            launches = {o: ctx.timing_get(name)[1] for o, name in TIMERS.items()}
            ctx.timing_enable(False)
            assert launches[s] > 0 and all(n == 0 for o, n in launches.items() if o != s), (s, launches)
    finally:
        ctx.timing_enable(False)
        for o in (PM_OPT_KNN_SUPERTILE, PM_OPT_KNN_RING, PM_OPT_KNN_F16_WAVES):
            ctx.set_option(o, 0)


def test_c3_every_size(ctx, oracle):
    """Config C3 (8192 x 8192 SIFT-like, u8 hint): 8 tiles per split, whole super-tiles for every size."""
    q, t, _ = synth.sift_like(8192, 8192, 128, seed=0xC3)
    want = oracle.bf_knn_l2(q, t, 2, nthreads=8)

    def check(s):
        ctx.knn_diag_enable(True)
        try:
            got = ctx.bf_knn_l2(q, t, 2, PM_KNN_HINT_U8)
            st = ctx.knn_stats()
        finally:
            ctx.knn_diag_enable(False)
        assert_matches_equal(got, want, "C3, super-tile option %d" % s)
        assert st["route"] == 3, st
    _each_size(ctx, check)
    assert_matches_equal(ctx.bf_knn_l2(q, t, 2, PM_KNN_HINT_U8), want, "C3, automatic size")


# nq = 7999 (32 workgroups of 256 queries, the last one partial) -> 8 train splits; tiles per split 1, 2, 3, 5, 7 with
# nt ending inside a tile; 4700 and 6900 also leave a short last split (2 and 5 tiles)
@pytest.mark.parametrize("nt", [1000, 1901, 2950, 4700, 6900])
def test_partial_super_tiles(ctx, oracle, nt):
    q, t, _ = synth.sift_like(7999, nt, 128, seed=nt)
    want = oracle.bf_knn_l2(q, t, 2, nthreads=8)
    _each_size(ctx, lambda s: assert_matches_equal(ctx.bf_knn_l2(q, t, 2, PM_KNN_HINT_U8), want,
                                                   "nt %d, super-tile option %d" % (nt, s)))


# (at most 64 splits: 263 tiles -> 5 per split, 157 tiles -> 3 per split)
@pytest.mark.parametrize("nq,nt", [(300, 33645), (1000, 20000)])
def test_four_wave_form(ctx, oracle, nq, nt):
    """The 4-wave x 64-query form (long sweeps) with every super-tile size, small nq so that splits hold many tiles."""
    q, t, _ = synth.sift_like(nq, nt, 128, seed=nq + nt)
    want = oracle.bf_knn_l2(q, t, 2, nthreads=8)
    _each_size(ctx, lambda s: assert_matches_equal(ctx.bf_knn_l2(q, t, 2, PM_KNN_HINT_U8), want,
                                                   "4 waves, super-tile option %d" % s), waves=2)


def test_low_dimensional_near_ties_every_size(ctx, oracle):
    """20-dimensional u8 rows against 33 645 train rows (hundreds of near ties per query: a stale operand costs a true
    neighbour), 5 tiles per split: partial last super-tiles of 2 and 4."""
    q, t, _ = synth.sift_like(514, 33645, 20, seed=41)
    want = oracle.bf_knn_l2(q, t, 2, nthreads=8)
    q8, t8 = q.astype(np.uint8), t.astype(np.uint8)

    def check(s):
        for rep in range(3):
            assert_matches_equal(ctx.bf_knn_l2_u8(q8, t8, 2), want, "u8 rows, super-tile option %d, run %d" % (s, rep))
        assert_matches_equal(ctx.bf_knn_l2(q, t, 2, PM_KNN_HINT_U8), want, "u8 hint, super-tile option %d" % s)
    _each_size(ctx, check)


def test_wrong_hint_every_size(ctx, oracle):
    """Data that are not u8-valued (a 256, a negative value, a non-integer) under the u8 hint: still the oracle's bits."""
    q, t, _ = synth.sift_like(777, 20000, 128, seed=5)         # 3 tiles per split
    t[17, 3] = 256.0
    t[2000, 100] = -1.0
    q[5, 9] = 12.5
    want = oracle.bf_knn_l2(q, t, 2, nthreads=8)
    _each_size(ctx, lambda s: assert_matches_equal(ctx.bf_knn_l2(q, t, 2, PM_KNN_HINT_U8), want,
                                                   "wrong hint, super-tile option %d" % s))


@pytest.mark.parametrize("nq", [1, 45, 1001])
def test_query_fragment_copy_pad_rows(ctx, oracle, nq):
    """The coarse kernel reads the queries from a copy in B-fragment order; nq not a multiple of 32 leaves pad rows in
    the last 32-query block (u8 rows and the u8 hint, every super-tile size)."""
    q, t, _ = synth.sift_like(nq, 3000, 128, seed=nq)
    want = oracle.bf_knn_l2(q, t, 2, nthreads=8)
    q8, t8 = q.astype(np.uint8), t.astype(np.uint8)

    def check(s):
        assert_matches_equal(ctx.bf_knn_l2(q, t, 2, PM_KNN_HINT_U8), want, "nq %d, u8 hint, option %d" % (nq, s))
        assert_matches_equal(ctx.bf_knn_l2_u8(q8, t8, 2), want, "nq %d, u8 rows, option %d" % (nq, s))
    _each_size(ctx, check)
