"""GPU parity of the u8 route's refinement (knn_l2_refine8) at the shapes where reading a candidate row with eight lanes
can go wrong: train sets that end inside a half of a 16-lane row, fewer rows than k, more than one candidate slot per
lane, more than 16 candidate rows per query (several passes), both kinds of exact re-scan, the three group sizes, both
per-lane list lengths (k <= 2, k <= 4), 144-byte train rows, the u8-row and fused entry points, and a wrong hint.

Every comparison is exact: trainIdx and the distance bits of all k records against oracle.pm_oracle.bf_knn_l2 on the
same seeded arrays (squared distances of u8-valued rows are integers below 2^24, so no summation order can move them).
Which kernel forms a case runs is asserted through the route planner (csrc/knn_l2_plan.hpp, a pure function of the
request that the launcher follows) and ctx.knn_stats()."""
import ctypes as C
import os

import numpy as np
import pytest

import cref
import points_matching_amd as pm
from points_matching_amd import api
from points_matching_amd.api import PM_KNN_HINT_U8, PM_OPT_KNN_RING, PM_OPT_KNN_U8_GROUP
from util import assert_matches_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 2, 3, 4)                       # k <= 2: two keys per lane (KM = 2); k = 3, 4: four (KM = 4)
GROUPS = {1: 4, 2: 8, 3: 16}            # PM_OPT_KNN_U8_GROUP -> rows per candidate group
N_CU = 256


@pytest.fixture(scope="module")
def plan():
    L = cref.load("knn_l2_plan_shim", {"knn_plan_fields": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]},
                  {"knn_plan_field_names": C.c_char_p},
                  include=[os.path.join(ROOT, "include"), os.path.join(ROOT, "points_matching_amd", "csrc")])
    names = L.knn_plan_field_names().decode().split(",")
    nopt = L.knn_plan_opt_count()

    def one(nq, nt, dim, k, opts=None, u8_rows=False, fuse=False):
        req = np.array([[nq, nt, dim, k, 0 if u8_rows else PM_KNN_HINT_U8, N_CU, int(u8_rows), 1, int(fuse)]], np.int32)
        o = np.zeros((1, nopt), np.int32)
        for key, v in (opts or {}).items():
            o[0, key] = v
        out = np.zeros((1, len(names)), np.float64)
        assert L.knn_plan_fields(cref.ptr(req), cref.ptr(o), 1, cref.ptr(out)) == len(names)
        return {n: int(v) for n, v in zip(names, out[0])}
    return one


def _run(ctx, q, t, k, flags=PM_KNN_HINT_U8):
    ctx.knn_diag_enable(True)
    try:
        got = ctx.bf_knn_l2(q, t, k, flags)
        st = ctx.knn_stats()
    finally:
        ctx.knn_diag_enable(False)
    return got, st


def _bytes(rng, n, dim, hi=256):
    return rng.integers(0, hi, (n, dim)).astype(np.float32)


def _tie_set(dim=128, hi=256, seed=11):
    """About 300 train rows with runs of 3, 12 and 40 identical rows and a few queries equal to each run: 12 equal rows
    fill a candidate list (split re-scan), 40 of them span several groups and passes."""
    rng = np.random.default_rng(seed)
    t = _bytes(rng, 301, dim, hi)
    q = _bytes(rng, 45, dim, hi)
    t[10:13] = t[200]
    t[60:72] = t[201]
    t[130:170] = t[202]
    q[0] = q[17] = t[200]
    q[1] = q[18] = q[40] = t[201]
    q[2] = q[19] = q[44] = t[202]
    return q, t


@pytest.fixture(scope="module")
def tie_set(oracle):
    q, t = _tie_set()
    return q, t, oracle.bf_knn_l2(q, t, 4, nthreads=8)


@pytest.fixture(scope="module")
def near_ties(oracle):
    """20 dimensions with values 0..3: squared distances below 180, hundreds of near and exact ties per query."""
    rng = np.random.default_rng(23)
    q, t = _bytes(rng, 64, 20, 4), _bytes(rng, 300, 20, 4)
    return q, t, oracle.bf_knn_l2(q, t, 4, nthreads=8)


def _each_group(ctx, fn):
    try:
        for opt in GROUPS:
            ctx.set_option(PM_OPT_KNN_U8_GROUP, opt)
            fn(opt)
    finally:
        ctx.set_option(PM_OPT_KNN_U8_GROUP, 0)


@pytest.mark.parametrize("dim", [4, 20, 64, 128])
@pytest.mark.parametrize("nt", [1, 2, 7, 77, 129])
def test_row_and_column_padding(ctx, oracle, plan, nt, dim):
    """Fewer train rows than k, a lone partial group, a train set that ends inside a half of eight lanes (the row < nt
    guard), and rows shorter than the 128-byte copy."""
    rng = np.random.default_rng(1000 * nt + dim)
    q, t = _bytes(rng, 37, dim), _bytes(rng, nt, dim)
    want = oracle.bf_knn_l2(q, t, 4, nthreads=8)

    def check(opt):
        for k in KS:
            got, st = _run(ctx, q, t, k)
            assert_matches_equal(got, want[:, :k], "nt %d dim %d group %d k %d" % (nt, dim, GROUPS[opt], k))
            assert st["route"] == 3 and st["nonfinite"] == 0, st
            if nt < k:
                assert st["rescans"] > 0, (nt, k, st)               # fewer than k ranked groups: every row, exactly
                assert (got["trainIdx"][:, nt:] == -1).all()
    _each_group(ctx, check)
    assert plan(37, nt, dim, 2)["refine8"] == 1


def test_two_slots_per_lane(ctx, oracle, plan):
    """nq = 100 against 643 train rows: several train splits, so a 16-lane row holds more than 16 candidate slots."""
    rng = np.random.default_rng(5)
    q, t = _bytes(rng, 100, 128), _bytes(rng, 643, 128)
    t[300:303] = t[5]
    q[7] = t[5]
    want = oracle.bf_knn_l2(q, t, 4, nthreads=8)
    for k in KS:
        p = plan(100, 643, 128, k)
        assert p["refine8"] == 1 and p["refine_ns"] >= 2 and p["refine_km"] == (2 if k <= 2 else 4), p
        got, st = _run(ctx, q, t, k)
        assert_matches_equal(got, want[:, :k], "NS >= 2, k %d" % k)
        assert st["route"] == 3 and st["nonfinite"] == 0, st


def test_several_passes_and_split_rescans(ctx, tie_set):
    """Runs of 3, 12 and 40 identical train rows: more than 16 candidate rows per query, and lists that overflow."""
    q, t, want = tie_set
    seen = []

    def check(opt):
        for k in KS:
            got, st = _run(ctx, q, t, k)
            assert_matches_equal(got, want[:, :k], "runs of identical rows, group %d k %d" % (GROUPS[opt], k))
            assert st["route"] == 3 and st["nonfinite"] == 0, st
            seen.append(st["rescans"])
    _each_group(ctx, check)
    assert max(seen) > 0, seen                                      # the split re-scan occurred
    assert (want["trainIdx"][2] == [130, 131, 132, 133]).all()     # lowest index first among the 40 equal rows


def test_low_dimensional_near_ties(ctx, near_ties):
    q, t, want = near_ties

    def check(opt):
        for k in KS:
            got, st = _run(ctx, q, t, k)
            assert_matches_equal(got, want[:, :k], "near ties, group %d k %d" % (GROUPS[opt], k))
            assert st["route"] == 3 and st["nonfinite"] == 0, st
    _each_group(ctx, check)


def test_wide_train_rows(ctx, oracle, plan, tie_set, near_ties):
    """PM_OPT_KNN_RING = 5: the coarse form that takes 144-byte train rows; the refinement reads a row's first 128."""
    rng = np.random.default_rng(9)
    cases = [("ties",) + tie_set, ("near ties",) + near_ties]
    for nq, nt, dim in ((37, 129, 128), (100, 643, 128), (37, 7, 20)):
        q, t = _bytes(rng, nq, dim), _bytes(rng, nt, dim)
        cases.append(("%d x %d x %d" % (nq, nt, dim), q, t, oracle.bf_knn_l2(q, t, 4, nthreads=8)))
    try:
        ctx.set_option(PM_OPT_KNN_RING, 5)
        for name, q, t, want in cases:
            for k in KS:
                p = plan(q.shape[0], t.shape[0], q.shape[1], k, {PM_OPT_KNN_RING: 5})
                assert p["u8_form"] == 5 and p["t_wide"] == 1 and p["refine8"] == 1, p         # the planner keeps the form
                got, st = _run(ctx, q, t, k)
                assert_matches_equal(got, want[:, :k], "wide rows, %s, k %d" % (name, k))
                assert st["route"] == 3 and st["nonfinite"] == 0, st
    finally:
        ctx.set_option(PM_OPT_KNN_RING, 0)


def test_u8_row_entry_point(ctx, oracle, tie_set, near_ties):
    import torch
    rng = np.random.default_rng(31)
    qp, tp = _bytes(rng, 37, 64), _bytes(rng, 77, 64)
    cases = [tie_set, near_ties, (qp, tp, oracle.bf_knn_l2(qp, tp, 4, nthreads=8))]
    dev = torch.device("cuda", 0)
    for q, t, want in cases:
        nq, dim = q.shape
        d_q, d_t = torch.from_numpy(q.astype(np.uint8)).to(dev), torch.from_numpy(t.astype(np.uint8)).to(dev)
        for k in KS:
            d_out = torch.zeros((nq, k, 4), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctx.bf_knn_l2_u8_dev(d_q.data_ptr(), nq, d_t.data_ptr(), t.shape[0], dim, k, d_out.data_ptr())
            ctx.synchronize()
            got = d_out.cpu().numpy().view(pm.MATCH_DTYPE).reshape(nq, k)
            assert_matches_equal(got, want[:, :k], "pm_bf_knn_l2_u8_dev %s k %d" % ((nq, t.shape[0], dim), k))


@pytest.mark.parametrize("nq,nt", [(100, 643), (768, 301)])
def test_fused_form_equals_the_two_calls(ctx, oracle, plan, tie_set, nq, nt):
    """pm_bf_knn_l2_ratio_dev at nq <= 768 (the ratio test rides the refinement launch) against pm_bf_knn_l2_f32_dev +
    pm_filter_ratio_gather_dev, record for record."""
    import torch
    rng = np.random.default_rng(nq)
    q, t = _bytes(rng, nq, 128), _bytes(rng, nt, 128)
    if nt == 301:
        t = tie_set[1].copy()
        q[:45] = tie_set[0]
    q[50:80] = np.clip(t[250:280] + rng.integers(-2, 3, (30, 128)), 0, 255)     # matches that pass the ratio test
    kp1 = rng.uniform(0, 900, (nq, 2)).astype(np.float32)
    kp2 = rng.uniform(0, 900, (nt, 2)).astype(np.float32)
    assert plan(nq, nt, 128, 2, fuse=True)["refine_fuse"] == 1
    dev = torch.device("cuda", 0)
    d_q, d_t, d_kp1, d_kp2 = (torch.from_numpy(a).to(dev) for a in (q, t, kp1, kp2))

    def buffers():
        return {"knn": torch.zeros((nq, 2, 4), dtype=torch.int32, device=dev),
                "good": torch.full((nq, 4), -7, dtype=torch.int32, device=dev),
                "xy1": torch.full((nq, 2), -1.0, dtype=torch.float32, device=dev),
                "xy2": torch.full((nq, 2), -1.0, dtype=torch.float32, device=dev),
                "n": torch.full((1,), -1, dtype=torch.int32, device=dev)}
    a, b = buffers(), buffers()
    torch.cuda.synchronize()
    ctx.bf_knn_l2_ratio_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 128, PM_KNN_HINT_U8, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(),
                            a["knn"].data_ptr(), a["good"].data_ptr(), a["xy1"].data_ptr(), a["xy2"].data_ptr(), a["n"].data_ptr())
    ctx.bf_knn_l2_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 128, 2, b["knn"].data_ptr(), PM_KNN_HINT_U8)
    ctx.filter_ratio_gather_dev(b["knn"].data_ptr(), nq, 2, 0.8, d_kp1.data_ptr(), d_kp2.data_ptr(), b["good"].data_ptr(),
                                b["xy1"].data_ptr(), b["xy2"].data_ptr(), b["n"].data_ptr())
    ctx.synchronize()
    assert ctx.filter_fusion_gave_up() == 0
    rec = {key: v.cpu().numpy() for key, v in a.items()}, {key: v.cpu().numpy() for key, v in b.items()}
    knn = [r["knn"].view(pm.MATCH_DTYPE).reshape(nq, 2) for r in rec]
    assert_matches_equal(knn[0], oracle.bf_knn_l2(q, t, 2, nthreads=8), "fused form, records vs oracle")
    assert_matches_equal(knn[0], knn[1], "fused form vs two calls, records")
    n = int(rec[0]["n"][0])
    assert n == int(rec[1]["n"][0]) and n > 0
    for key in ("good", "xy1", "xy2"):
        assert np.array_equal(rec[0][key][:n].view(np.uint32), rec[1][key][:n].view(np.uint32)), key


def test_wrong_hint_still_the_oracle(ctx, oracle, tie_set):
    """One value 256 in the train set: the premise fails on the device and the f32 rows are scanned."""
    q, t, _ = tie_set
    t = t.copy()
    t[17, 5] = 256.0
    want = oracle.bf_knn_l2(q, t, 4, nthreads=8)
    for k in KS:
        got, st = _run(ctx, q, t, k)
        assert_matches_equal(got, want[:, :k], "wrong hint, k %d" % k)
        assert st["nonfinite"] == 1, st
